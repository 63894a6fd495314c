// run_warp.cpp -- the run_OF_WARP_{INT,RGB} command lines: frame b pulled back onto frame a along their flow.
//
//   run_OF_WARP_INT a.png b.png out.pgm [oppoint 1-4, default 2]
//   run_OF_WARP_RGB a.png b.png out.ppm [oppoint 1-4, default 2]
//
// The motion-compensated frame of ofdis_run_warp_u8_host at scale 1 (the flow a -> b, then b warped by it), written
// as a binary PGM / PPM.  SELECTCHANNEL (1 gray, 3 BGR) is compile-time, as in run_dense.cpp; both images must have
// one size.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/ofdis.h"

#ifndef SELECTCHANNEL
#define SELECTCHANNEL 1
#endif
#define NOCHANNELS (SELECTCHANNEL == 3 ? 3 : 1)

// cv::imread(path, GRAYSCALE / COLOR)
static bool load(const char *path, std::vector<uint8_t> &px, int &w, int &h) {
  int rc = ofdis_read_image(path, nullptr, &w, &h, NOCHANNELS, 0);
  if (rc == OFDIS_OK) {
    px.resize((size_t)w * h * NOCHANNELS);
    rc = ofdis_read_image(path, px.data(), &w, &h, NOCHANNELS, px.size());
  }
  if (rc != OFDIS_OK) std::fprintf(stderr, "cannot read %s (PNG, Netpbm or BMP expected): %s\n", path, ofdis_status_string(rc));
  return rc == OFDIS_OK;
}

int main(int argc, char **argv) {
  int op = 2;
  if (argc == 5) {
    char *end = nullptr;
    const long v = std::strtol(argv[4], &end, 10);
    op = (end == argv[4] || *end != '\0' || v < 1 || v > 4) ? -1 : (int)v;
  }
  if (argc < 4 || argc > 5 || op < 0) {
    std::fprintf(stderr, "usage: %s <image a> <image b> <out.%s> [oppoint 1-4]\n", argv[0], NOCHANNELS == 1 ? "pgm" : "ppm");
    return 1;
  }
  std::vector<uint8_t> a, b;
  int w = 0, h = 0, wb = 0, hb = 0;
  if (!load(argv[1], a, w, h) || !load(argv[2], b, wb, hb)) return 1;
  if (w != wb || h != hb) {
    std::fprintf(stderr, "image sizes differ: %dx%d and %dx%d\n", w, h, wb, hb);
    return 1;
  }
  ofdis_params p;
  int rc = ofdis_params_oppoint(&p, op, w, OFDIS_MODE_OF, NOCHANNELS);
  if (rc == OFDIS_OK) rc = ofdis_params_validate(&p, -1, -1, -1);
  if (rc != OFDIS_OK) {
    std::fprintf(stderr, "invalid parameters: %s\n", ofdis_status_string(rc));
    return 1;
  }
  ofdis_context *ctx = nullptr;
  rc = ofdis_context_create(0, &ctx);
  if (rc != OFDIS_OK) {
    std::fprintf(stderr, "no usable gfx950 device: %s\n", ofdis_status_string(rc));
    return 1;
  }
  std::vector<uint8_t> out(a.size());
  rc = ofdis_run_warp_u8_host(ctx, a.data(), b.data(), 1, w, h, &p, 1.0f, OFDIS_IMG_U8, out.data(), nullptr);
  ofdis_context_destroy(ctx);
  if (rc != OFDIS_OK) {
    std::fprintf(stderr, "warp failed: %s\n", ofdis_status_string(rc));
    return 1;
  }
  if (ofdis_write_pnm(argv[3], out.data(), w, h, NOCHANNELS) != OFDIS_OK) {
    std::fprintf(stderr, "cannot write %s\n", argv[3]);
    return 1;
  }
  return 0;
}

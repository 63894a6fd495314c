// run_interp.cpp -- the run_OF_INTERP_{INT,RGB} command lines: the K frames between frame a and frame b.
//
//   run_OF_INTERP_INT a.png b.png out_prefix K [oppoint 1-4, default 2 | the 20 parameters of run_OF_INT]
//   run_OF_INTERP_RGB a.png b.png out_prefix K [oppoint 1-4, default 2 | the 20 parameters of run_OF_RGB]
//
// The frames of ofdis_run_interp_u8_host at the times t = k / (K + 1), k = 1 .. K (float32: (float)k / (float)(K + 1)),
// written as out_prefix001.pgm, out_prefix002.pgm, ... (.ppm for RGB) through ofdis_write_pnm.  K is 1 ..
// OFDIS_INTERP_MAX_T.  SELECTCHANNEL (1 gray, 3 BGR) is compile-time, as in run_dense.cpp; both images must have one size.
#include <cstdio>
#include <cstdlib>
#include <string>
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

static long whole(const char *s, long lo, long hi) {  // -1: not a whole number in lo .. hi
  char *end = nullptr;
  const long v = std::strtol(s, &end, 10);
  return (end == s || *end != '\0' || v < lo || v > hi) ? -1 : v;
}

int main(int argc, char **argv) {
  const long K = argc >= 5 ? whole(argv[4], 1, OFDIS_INTERP_MAX_T) : -1;
  const long op = argc == 6 ? whole(argv[5], 1, 4) : 2;
  if ((argc != 5 && argc != 6 && argc != 25) || K < 0 || op < 0) {
    std::fprintf(stderr, "usage: %s <image a> <image b> <out prefix> <K 1-%d> [oppoint 1-4 | 20 parameters]\n", argv[0],
                 OFDIS_INTERP_MAX_T);
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
  int rc = argc == 25 ? ofdis_params_from_strings(&p, 20, (const char *const *)(argv + 5), OFDIS_MODE_OF, NOCHANNELS)
                      : ofdis_params_oppoint(&p, (int)op, w, OFDIS_MODE_OF, NOCHANNELS);
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
  std::vector<float> t(K);
  for (long k = 1; k <= K; ++k) t[k - 1] = (float)k / (float)(K + 1);
  std::vector<uint8_t> out(a.size() * K);
  rc = ofdis_run_interp_u8_host(ctx, a.data(), b.data(), 1, w, h, &p, t.data(), (int)K, OFDIS_IMG_U8, out.data(), nullptr);
  ofdis_context_destroy(ctx);
  if (rc != OFDIS_OK) {
    std::fprintf(stderr, "interpolation failed: %s\n", ofdis_status_string(rc));
    return 1;
  }
  for (long k = 1; k <= K; ++k) {
    char num[16];
    std::snprintf(num, sizeof(num), "%03ld", k);
    const std::string path = std::string(argv[3]) + num + (NOCHANNELS == 1 ? ".pgm" : ".ppm");
    if (ofdis_write_pnm(path.c_str(), out.data() + (size_t)(k - 1) * a.size(), w, h, NOCHANNELS) != OFDIS_OK) {
      std::fprintf(stderr, "cannot write %s\n", path.c_str());
      return 1;
    }
  }
  return 0;
}

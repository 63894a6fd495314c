// run_stereo.cpp -- the run_DE_LR_{INT,RGB} command lines: both views' disparities of a rectified pair and their
// left-right masks.
//
//   run_DE_LR_INT left right out_l.pfm out_r.pfm occ_l.pgm occ_r.pgm            operating point 2
//   run_DE_LR_INT left right out_l.pfm out_r.pfm occ_l.pgm occ_r.pgm X          operating point X = 1..4
//   run_DE_LR_INT left right out_l.pfm out_r.pfm occ_l.pgm occ_r.pgm p1 .. p20  all 20 parameters (as run_DE_INT)
//
// ofdis_run_stereo_u8_host with the suggested thresholds (alpha 0.01, beta 0.5).  Both .pfm files go through
// ofdis_write_pfm, which NEGATES and stores rows bottom-up like the reference's SavePFMFile: out_l.pfm is the file
// run_DE_INT writes (positive values), out_r.pfm holds -disp_r (negative values).  The masks are binary PGMs holding
// the raw codes 0 / 1 / 2 (ofdis_lr_check), top-down.  SELECTCHANNEL (1 gray, 3 BGR) is compile-time, as in
// run_dense.cpp; both images must have one size.
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
  if (argc != 7 && argc != 8 && argc != 27) {
    std::fprintf(stderr, "usage: %s left right out_l.pfm out_r.pfm occ_l.pgm occ_r.pgm [oppoint 1-4 | 20 parameters]\n",
                 argv[0]);
    return 1;
  }
  std::vector<uint8_t> l, r;
  int w = 0, h = 0, wr = 0, hr = 0;
  if (!load(argv[1], l, w, h) || !load(argv[2], r, wr, hr)) return 1;
  if (w != wr || h != hr) {
    std::fprintf(stderr, "image sizes differ: %dx%d and %dx%d\n", w, h, wr, hr);
    return 1;
  }
  ofdis_params p;
  int rc;
  if (argc <= 8)
    rc = ofdis_params_oppoint(&p, argc == 8 ? std::atoi(argv[7]) : 2, w, OFDIS_MODE_DE, NOCHANNELS);
  else
    rc = ofdis_params_from_strings(&p, 20, (const char *const *)(argv + 7), OFDIS_MODE_DE, NOCHANNELS);
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
  const size_t px = (size_t)w * h;
  std::vector<float> dl(px), dr(px);
  std::vector<uint8_t> ol(px), orr(px);
  rc = ofdis_run_stereo_u8_host(ctx, l.data(), r.data(), 1, w, h, &p, 0.01f, 0.5f, dl.data(), dr.data(), ol.data(),
                                orr.data(), nullptr, nullptr);
  ofdis_context_destroy(ctx);
  if (rc != OFDIS_OK) {
    std::fprintf(stderr, "stereo computation failed: %s\n", ofdis_status_string(rc));
    return 1;
  }
  const char *paths[4] = {argv[3], argv[4], argv[5], argv[6]};
  const int wrc[4] = {ofdis_write_pfm(paths[0], dl.data(), w, h), ofdis_write_pfm(paths[1], dr.data(), w, h),
                      ofdis_write_pnm(paths[2], ol.data(), w, h, 1), ofdis_write_pnm(paths[3], orr.data(), w, h, 1)};
  for (int k = 0; k < 4; ++k)
    if (wrc[k] != OFDIS_OK) {
      std::fprintf(stderr, "cannot write %s\n", paths[k]);
      return 1;
    }
  return 0;
}

// run_motion.cpp -- the run_OF_MOTION_{INT,RGB} command lines: the pixels of a list of video frames that moved on their
// own, against the camera's motion.
//
//   run_OF_MOTION_INT <out-prefix> <thr> <radius> <oppoint 1-4> <use_fb 0|1> img0 img1 ... img(T-1)
//
// The codes of pair i (frame i -> frame i + 1; 0 static, 1 moving, 2 unknown, the raw values as run_DE_LR_INT's masks)
// go to <out-prefix>%06d.pgm through ofdis_write_pnm -- the prefix `out_` gives out_000000.pgm, out_000001.pgm, ... --
// and <out-prefix>stats.txt takes one line per pair: the twelve integers of its statistics, then the six values of its
// transform as %.17g.  thr: the residual in pixels above which a pixel moves, in [0, 65536]; radius: the binary
// median's window, 0 .. 4.  use_fb = 1: the forward-backward check at the default thresholds 0.01 / 0.5 picks the fit's
// samples and marks the occluded pixels unknown.  The rest is the library's default: similarity, step 16, tau 2, 4
// re-solves, rel 0.05.  The masks are those of ofdis_run_sequence_motion_mask_u8_host on the whole list: one context,
// every image decoded once, every frame's pyramid built once.  SELECTCHANNEL (1 gray, 3 BGR) is compile-time, as in
// run_dense.cpp; all images must have one size.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ofdis.h"

#ifndef SELECTCHANNEL
#define SELECTCHANNEL 1
#endif
#define NOCHANNELS (SELECTCHANNEL == 3 ? 3 : 1)

// a whole decimal number in [lo, hi], or -1
static int parse_int(const char *s, int lo, int hi) {
  char *end = nullptr;
  const long v = std::strtol(s, &end, 10);
  if (end == s || *end != '\0' || v < lo || v > hi) return -1;
  return (int)v;
}

// thr in [0, 65536], or -1
static float parse_thr(const char *s) {
  char *end = nullptr;
  const float v = std::strtof(s, &end);
  if (end == s || *end != '\0' || !(v >= 0.0f && v <= 65536.0f)) return -1.0f;
  return v;
}

static bool read_error(const char *path, int rc) {
  std::fprintf(stderr, "cannot read %s (PNG, Netpbm or BMP expected): %s\n", path, ofdis_status_string(rc));
  return false;
}

// Every image's size (a PNG's from its header alone), before anything is computed: all must equal the first's.
static bool check_sizes(int n, char **paths, int &w, int &h) {
  for (int i = 0; i < n; ++i) {
    int iw = 0, ih = 0;
    const int rc = ofdis_read_image(paths[i], nullptr, &iw, &ih, NOCHANNELS, 0);
    if (rc != OFDIS_OK) return read_error(paths[i], rc);
    if (i == 0) {
      w = iw;
      h = ih;
    } else if (iw != w || ih != h) {
      std::fprintf(stderr, "image sizes differ: %s is %dx%d, %s is %dx%d\n", paths[i], iw, ih, paths[0], w, h);
      return false;
    }
  }
  return true;
}

int main(int argc, char **argv) {
  const float thr = argc >= 3 ? parse_thr(argv[2]) : -1.0f;
  const int radius = argc >= 4 ? parse_int(argv[3], 0, 4) : -1;
  const int op = argc >= 5 ? parse_int(argv[4], 1, 4) : -1;
  const int use_fb = argc >= 6 ? parse_int(argv[5], 0, 1) : -1;
  const int nframes = argc - 6;
  if (argc < 8 || thr < 0.0f || radius < 0 || op < 0 || use_fb < 0) {
    std::fprintf(stderr,
                 "usage: %s <out-prefix> <thr 0-65536> <radius 0-4> <oppoint 1-4> <use_fb 0|1> img0 img1 ... (two images or "
                 "more)\n       the codes of pair i -> <out-prefix>%%06d.pgm, statistics and transforms -> "
                 "<out-prefix>stats.txt\n",
                 argv[0]);
    return 1;
  }
  int w = 0, h = 0;
  if (!check_sizes(nframes, argv + 6, w, h)) return 1;
  const size_t px = (size_t)w * h, in_frame = px * NOCHANNELS;
  std::vector<uint8_t> frames(in_frame * nframes);
  for (int i = 0; i < nframes; ++i) {  // the one decode of each image
    int iw = 0, ih = 0;
    const int rc = ofdis_read_image(argv[6 + i], frames.data() + i * in_frame, &iw, &ih, NOCHANNELS, in_frame);
    if (rc != OFDIS_OK) return read_error(argv[6 + i], rc), 1;
    if (iw != w || ih != h) {  // (the file changed since check_sizes)
      std::fprintf(stderr, "image sizes differ: %s is %dx%d, expected %dx%d\n", argv[6 + i], iw, ih, w, h);
      return 1;
    }
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
  const int m = nframes - 1;
  std::vector<uint8_t> code(px * m);
  std::vector<int64_t> stats((size_t)m * OFDIS_MM_NSTATS);
  std::vector<double> xform((size_t)m * 6);
  rc = ofdis_run_sequence_motion_mask_u8_host(ctx, frames.data(), nframes, w, h, &p, OFDIS_MOTION_SIMILARITY, 16, 2.0, 4,
                                              use_fb, 0.01f, 0.5f, thr, 0.05f, radius, code.data(), nullptr, stats.data(),
                                              xform.data(), nullptr, nullptr);
  ofdis_context_destroy(ctx);
  if (rc != OFDIS_OK) {
    std::fprintf(stderr, "the motion mask failed: %s\n", ofdis_status_string(rc));
    return 1;
  }
  for (int i = 0; i < m; ++i) {
    char num[32];
    std::snprintf(num, sizeof(num), "%06d.pgm", i);
    const std::string path = std::string(argv[1]) + num;
    if (ofdis_write_pnm(path.c_str(), code.data() + i * px, w, h, 1) != OFDIS_OK) {
      std::fprintf(stderr, "cannot write %s\n", path.c_str());
      return 1;
    }
  }
  const std::string path = std::string(argv[1]) + "stats.txt";
  std::FILE *f = std::fopen(path.c_str(), "w");
  if (!f) {
    std::fprintf(stderr, "cannot write %s\n", path.c_str());
    return 1;
  }
  for (int i = 0; i < m; ++i) {
    const int64_t *s = stats.data() + (size_t)i * OFDIS_MM_NSTATS;
    for (int k = 0; k < OFDIS_MM_NSTATS; ++k) std::fprintf(f, "%lld ", (long long)s[k]);
    const double *x = xform.data() + 6 * (size_t)i;
    std::fprintf(f, "%.17g %.17g %.17g %.17g %.17g %.17g\n", x[0], x[1], x[2], x[3], x[4], x[5]);
  }
  if (std::fclose(f) != 0) {
    std::fprintf(stderr, "cannot write %s\n", path.c_str());
    return 1;
  }
  return 0;
}

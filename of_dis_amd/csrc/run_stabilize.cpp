// run_stabilize.cpp -- the run_OF_STAB_{INT,RGB} command lines: a list of video frames stabilised along its camera
// path.
//
//   run_OF_STAB_INT <out-prefix> <radius> <zoom> <oppoint 1-4> <use_fb 0|1> img0 img1 ... img(T-1)
//
// Stabilised frame i goes to <out-prefix>%06d.pgm (.ppm for RGB) through ofdis_write_pnm -- the prefix `out_` gives
// out_000000.pgm, out_000001.pgm, ... -- and <out-prefix>path.txt takes one line per frame with the six values of its
// correction transform as %.17g.  radius: frames either side in the path's smoothing window, 0 .. 256; zoom: the
// magnification about the frame centre that hides the moving border, in [1, 16].  use_fb = 1: only samples that pass
// the forward-backward check at the default thresholds 0.01 / 0.5 enter the fit.  The fit is the library's default:
// similarity, step 16, tau 2, 4 re-solves.  The pictures are those of ofdis_run_sequence_stabilize_u8_host on the whole
// list: one context, every image decoded once, every frame's pyramid built once.  SELECTCHANNEL (1 gray, 3 BGR) is
// compile-time, as in run_dense.cpp; all images must have one size.
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

// zoom in [1, 16], or -1
static double parse_zoom(const char *s) {
  char *end = nullptr;
  const double v = std::strtod(s, &end);
  if (end == s || *end != '\0' || !(v >= 1.0 && v <= 16.0)) return -1.0;
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
  const int radius = argc >= 3 ? parse_int(argv[2], 0, 256) : -1;
  const double zoom = argc >= 4 ? parse_zoom(argv[3]) : -1.0;
  const int op = argc >= 5 ? parse_int(argv[4], 1, 4) : -1;
  const int use_fb = argc >= 6 ? parse_int(argv[5], 0, 1) : -1;
  const int nframes = argc - 6;
  if (argc < 8 || radius < 0 || zoom < 0.0 || op < 0 || use_fb < 0) {
    std::fprintf(stderr,
                 "usage: %s <out-prefix> <radius 0-256> <zoom 1-16> <oppoint 1-4> <use_fb 0|1> img0 img1 ... (two images or "
                 "more)\n       stabilised frame i -> <out-prefix>%%06d.%s, the corrections -> <out-prefix>path.txt\n",
                 argv[0], NOCHANNELS == 1 ? "pgm" : "ppm");
    return 1;
  }
  int w = 0, h = 0;
  if (!check_sizes(nframes, argv + 6, w, h)) return 1;
  const size_t in_frame = (size_t)w * h * NOCHANNELS;
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
  std::vector<uint8_t> out(in_frame * nframes);
  std::vector<double> corr((size_t)nframes * 6);
  rc = ofdis_run_sequence_stabilize_u8_host(ctx, frames.data(), nframes, w, h, &p, OFDIS_MOTION_SIMILARITY, 16, 2.0, 4,
                                            use_fb, 0.01f, 0.5f, radius, zoom, OFDIS_IMG_U8, out.data(), nullptr, nullptr,
                                            corr.data(), nullptr);
  ofdis_context_destroy(ctx);
  if (rc != OFDIS_OK) {
    std::fprintf(stderr, "stabilising failed: %s\n", ofdis_status_string(rc));
    return 1;
  }
  for (int i = 0; i < nframes; ++i) {
    char num[32];
    std::snprintf(num, sizeof(num), "%06d.%s", i, NOCHANNELS == 1 ? "pgm" : "ppm");
    const std::string path = std::string(argv[1]) + num;
    if (ofdis_write_pnm(path.c_str(), out.data() + i * in_frame, w, h, NOCHANNELS) != OFDIS_OK) {
      std::fprintf(stderr, "cannot write %s\n", path.c_str());
      return 1;
    }
  }
  const std::string path = std::string(argv[1]) + "path.txt";
  std::FILE *f = std::fopen(path.c_str(), "w");
  if (!f) {
    std::fprintf(stderr, "cannot write %s\n", path.c_str());
    return 1;
  }
  for (int i = 0; i < nframes; ++i) {
    const double *m = corr.data() + 6 * (size_t)i;
    std::fprintf(f, "%.17g %.17g %.17g %.17g %.17g %.17g\n", m[0], m[1], m[2], m[3], m[4], m[5]);
  }
  if (std::fclose(f) != 0) {
    std::fprintf(stderr, "cannot write %s\n", path.c_str());
    return 1;
  }
  return 0;
}

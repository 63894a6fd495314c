// run_tfilter.cpp -- the run_OF_TFILTER_{INT,RGB} and run_OF_TFILTER_R_{INT,RGB} command lines: motion-compensated
// temporal denoising of a list of video frames.
//
//   run_OF_TFILTER_INT   <out-prefix> <sigma> <oppoint 1-4> <occ 0|1> img0 img1 ... img(T-1)
//   run_OF_TFILTER_R_INT <out-prefix> <radius 1-4> <sigma> <oppoint 1-4> <fb 0|1> img0 img1 ... img(T-1)
//
// Frame i filtered with its two neighbours pulled onto it along the flows goes to <out-prefix>%06d.pgm (.ppm for RGB)
// through ofdis_write_pnm -- the prefix `out_` gives out_000000.pgm, out_000001.pgm, ...  sigma: the grey-level
// difference per channel at which a neighbour's weight reaches zero, in [1/1024, 65536].  occ = 1: with the occlusion
// masks of the forward-backward check at the default thresholds 0.01 / 0.5.  The pictures are those of
// ofdis_run_sequence_tfilter_u8_host on the whole list: one context, every image decoded once, every frame's pyramid
// built once.  The _R_ pair (compiled with -DTFILTER_RADIUS) filters over `radius` frames on each side along chained
// flows, fb = 1 with the forward-backward check inside every chain step at the same thresholds
// (ofdis_run_sequence_tfilter_radius_u8_host); it writes the same file names.
// SELECTCHANNEL (1 gray, 3 BGR) is compile-time, as in run_dense.cpp; all images must have one size.
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
#ifdef TFILTER_RADIUS
#define RADIUS_ARG 1  // the radius comes after the prefix and shifts the other arguments by one
#else
#define RADIUS_ARG 0
#endif

// a whole decimal number in [lo, hi], or -1
static int parse_int(const char *s, int lo, int hi) {
  char *end = nullptr;
  const long v = std::strtol(s, &end, 10);
  if (end == s || *end != '\0' || v < lo || v > hi) return -1;
  return (int)v;
}

// sigma in [1/1024, 65536], or -1
static float parse_sigma(const char *s) {
  char *end = nullptr;
  const float v = std::strtof(s, &end);
  if (end == s || *end != '\0' || !(v >= 1.0f / 1024.0f && v <= 65536.0f)) return -1.0f;
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
  constexpr int A = RADIUS_ARG, first = 5 + A;  // argv[first]: the first image
  const int radius = !A ? 1 : argc >= 3 ? parse_int(argv[2], 1, 4) : -1;
  const float sigma = argc >= 3 + A ? parse_sigma(argv[2 + A]) : -1.0f;
  const int op = argc >= 4 + A ? parse_int(argv[3 + A], 1, 4) : -1;
  const int occ = argc >= 5 + A ? parse_int(argv[4 + A], 0, 1) : -1;
  const int nframes = argc - first;
  if (argc < first + 2 || radius < 0 || sigma < 0.0f || op < 0 || occ < 0) {
    std::fprintf(stderr,
                 "usage: %s <out-prefix> %s<sigma 1/1024-65536> <oppoint 1-4> <%s 0|1> img0 img1 ... (two images or more)\n"
                 "       frame i filtered with its neighbours -> <out-prefix>%%06d.%s\n",
                 argv[0], A ? "<radius 1-4> " : "", A ? "fb" : "occ", NOCHANNELS == 1 ? "pgm" : "ppm");
    return 1;
  }
  int w = 0, h = 0;
  if (!check_sizes(nframes, argv + first, w, h)) return 1;
  const size_t in_frame = (size_t)w * h * NOCHANNELS;
  std::vector<uint8_t> frames(in_frame * nframes);
  for (int i = 0; i < nframes; ++i) {  // the one decode of each image
    int iw = 0, ih = 0;
    const int rc = ofdis_read_image(argv[first + i], frames.data() + i * in_frame, &iw, &ih, NOCHANNELS, in_frame);
    if (rc != OFDIS_OK) return read_error(argv[first + i], rc), 1;
    if (iw != w || ih != h) {  // (the file changed since check_sizes)
      std::fprintf(stderr, "image sizes differ: %s is %dx%d, expected %dx%d\n", argv[first + i], iw, ih, w, h);
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
  if (A)
    rc = ofdis_run_sequence_tfilter_radius_u8_host(ctx, frames.data(), nframes, w, h, &p, radius, sigma, occ, 0.01f, 0.5f,
                                                   OFDIS_IMG_U8, out.data(), nullptr);
  else
    rc = ofdis_run_sequence_tfilter_u8_host(ctx, frames.data(), nframes, w, h, &p, sigma, occ, 0.01f, 0.5f, OFDIS_IMG_U8,
                                            out.data(), nullptr);
  ofdis_context_destroy(ctx);
  if (rc != OFDIS_OK) {
    std::fprintf(stderr, "filtering failed: %s\n", ofdis_status_string(rc));
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
  return 0;
}

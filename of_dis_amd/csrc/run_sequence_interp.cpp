// run_sequence_interp.cpp -- the run_OF_SEQ_INTERP_{INT,RGB} command lines: the frames between the frames of a video.
//
//   run_OF_SEQ_INTERP_INT <out-prefix> <K 1-16> <oppoint 1-4> <occ 0|1> img0 img1 ... img(T-1)
//
// Pair i is (img i, img i + 1), T - 1 pairs in all; its K frames at the times t = k / (K + 1), k = 1 .. K (float32:
// (float)k / (float)(K + 1), as run_OF_INTERP_INT computes them) go to <out-prefix>%06d_%03d.pgm (.ppm for RGB) through
// ofdis_write_pnm.  occ = 1: with the pair's occlusion masks (ofdis_run_interp_occ_u8's pictures at the default
// thresholds 0.01 / 0.5), occ = 0: ofdis_run_interp_u8's.  One context for the whole list, every image decoded once, and
// every frame's pyramid built once per window (ofdis_run_sequence_interp_u8_host): lists longer than kWindow pairs go
// through in windows of at most kWindow pairs whose frames overlap by one.
// SELECTCHANNEL (1 gray, 3 BGR) is compile-time, as in run_dense.cpp; all images must have one size.
#include <algorithm>
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

static const int kWindow = 64;  // pairs per call
static const int kStride = 1;

// a whole decimal number in [lo, hi], or -1
static int parse_int(const char *s, int lo, int hi) {
  char *end = nullptr;
  const long v = std::strtol(s, &end, 10);
  if (end == s || *end != '\0' || v < lo || v > hi) return -1;
  return (int)v;
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

// cv::imread(path, GRAYSCALE / COLOR) of a w x h image appended to `frames`: the one decode of that image
static bool load(const char *path, int w, int h, std::vector<uint8_t> &frames) {
  const size_t px = (size_t)w * h * NOCHANNELS, at = frames.size();
  frames.resize(at + px);
  int iw = 0, ih = 0;
  const int rc = ofdis_read_image(path, frames.data() + at, &iw, &ih, NOCHANNELS, px);
  if (rc != OFDIS_OK) return read_error(path, rc);
  if (iw != w || ih != h) {  // (the file changed since check_sizes)
    std::fprintf(stderr, "image sizes differ: %s is %dx%d, expected %dx%d\n", path, iw, ih, w, h);
    return false;
  }
  return true;
}

int main(int argc, char **argv) {
  const int K = argc >= 3 ? parse_int(argv[2], 1, OFDIS_INTERP_MAX_T) : -1;
  const int op = argc >= 4 ? parse_int(argv[3], 1, 4) : -1;
  const int occ = argc >= 5 ? parse_int(argv[4], 0, 1) : -1;
  const int nframes = argc - 5;
  if (argc < 7 || K < 0 || op < 0 || occ < 0) {
    std::fprintf(stderr,
                 "usage: %s <out-prefix> <K 1-%d> <oppoint 1-4> <occ 0|1> img0 img1 ... (at least two images)\n"
                 "       pair i = (img i, img i + 1), time k / (K + 1) -> <out-prefix>%%06d_%%03d.%s\n",
                 argv[0], OFDIS_INTERP_MAX_T, NOCHANNELS == 1 ? "pgm" : "ppm");
    return 1;
  }
  const int npairs = nframes - kStride;
  // the frames of one window, decoded once each: window k holds frames [k kWindow, k kWindow + pairs + 1)
  int w = 0, h = 0;
  if (!check_sizes(nframes, argv + 5, w, h)) return 1;
  std::vector<uint8_t> frames;
  if (!load(argv[5], w, h, frames)) return 1;
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
  std::vector<float> t(K);
  for (int k = 1; k <= K; ++k) t[k - 1] = (float)k / (float)(K + 1);
  const size_t in_frame = (size_t)w * h * NOCHANNELS;
  std::vector<uint8_t> out;
  int loaded = 1;  // frames [first, loaded) are in `frames`
  int status = 0;
  for (int first = 0; first < npairs && status == 0; first += kWindow) {
    const int m = std::min(kWindow, npairs - first);
    // drop the frames before this window, keep the one it shares with the last (already decoded)
    const int have_from = loaded - (int)(frames.size() / in_frame);
    if (first > have_from) frames.erase(frames.begin(), frames.begin() + (size_t)(first - have_from) * in_frame);
    for (; loaded < first + m + kStride; ++loaded)
      if (!load(argv[5 + loaded], w, h, frames)) {
        status = 1;
        break;
      }
    if (status) break;
    out.resize((size_t)m * K * in_frame);
    rc = ofdis_run_sequence_interp_u8_host(ctx, frames.data(), m + kStride, kStride, w, h, &p, t.data(), K, occ, 0.01f,
                                           0.5f, OFDIS_IMG_U8, out.data(), nullptr, nullptr, nullptr);
    if (rc != OFDIS_OK) {
      std::fprintf(stderr, "interpolation failed: %s\n", ofdis_status_string(rc));
      status = 1;
      break;
    }
    for (int i = 0; i < m && status == 0; ++i)
      for (int k = 1; k <= K; ++k) {
        char num[48];
        std::snprintf(num, sizeof(num), "%06d_%03d.%s", first + i, k, NOCHANNELS == 1 ? "pgm" : "ppm");
        const std::string path = std::string(argv[1]) + num;
        if (ofdis_write_pnm(path.c_str(), out.data() + ((size_t)i * K + (k - 1)) * in_frame, w, h, NOCHANNELS) != OFDIS_OK) {
          std::fprintf(stderr, "cannot write %s\n", path.c_str());
          status = 1;
          break;
        }
      }
  }
  ofdis_context_destroy(ctx);
  return status;
}

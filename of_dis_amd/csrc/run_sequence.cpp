// run_sequence.cpp -- the run_OF_SEQ_{INT,RGB} command lines: optical flow along a list of video frames.
//
//   run_OF_SEQ_INT <out-prefix> <oppoint 1-4> <stride> img0 img1 ... img(T-1)
//
// Pair i is (img i, img i + stride), T - stride pairs in all; its flow goes to <out-prefix>%06d.flo and is byte for
// byte what `run_OF_INT img(i) img(i + stride) out.flo <oppoint>` writes.  One context for the whole list, every image
// decoded once, and every frame's pyramid built once per window (ofdis_run_sequence_u8_host): lists longer than
// kWindow pairs go through in windows of at most kWindow pairs whose frames overlap by `stride`.
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

static const int kWindow = 256;  // pairs per call

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
  const int op = argc >= 3 ? parse_int(argv[2], 1, 4) : -1;
  const int stride = argc >= 4 ? parse_int(argv[3], 1, 1 << 20) : -1;
  const int nframes = argc - 4;
  if (argc < 6 || op < 0 || stride < 0 || nframes <= stride) {
    std::fprintf(stderr,
                 "usage: %s <out-prefix> <oppoint 1-4> <stride >= 1> img0 img1 ... (more than <stride> images)\n"
                 "       pair i = (img i, img i + stride) -> <out-prefix>%%06d.flo\n",
                 argv[0]);
    return 1;
  }
  const int npairs = nframes - stride;
  // the frames of one window, decoded once each: window k holds frames [k kWindow, k kWindow + pairs + stride)
  int w = 0, h = 0;
  if (!check_sizes(nframes, argv + 4, w, h)) return 1;
  std::vector<uint8_t> frames;
  if (!load(argv[4], w, h, frames)) return 1;
  ofdis_params p;
  int rc = ofdis_params_oppoint(&p, op, w, 1, NOCHANNELS);
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
  const size_t in_frame = (size_t)w * h * NOCHANNELS, out_frame = (size_t)w * h * 2;
  std::vector<float> flow;
  int loaded = 1;  // frames [first, loaded) are in `frames`
  int status = 0;
  for (int first = 0; first < npairs && status == 0; first += kWindow) {
    const int m = std::min(kWindow, npairs - first);
    // drop the frames before this window, keep the ones it shares with the last (already decoded)
    const int have_from = loaded - (int)(frames.size() / in_frame);
    if (first > have_from) frames.erase(frames.begin(), frames.begin() + (size_t)(first - have_from) * in_frame);
    for (; loaded < first + m + stride; ++loaded)
      if (!load(argv[4 + loaded], w, h, frames)) {
        status = 1;
        break;
      }
    if (status) break;
    flow.resize((size_t)m * out_frame);
    rc = ofdis_run_sequence_u8_host(ctx, frames.data(), m + stride, stride, nullptr, w, h, &p, 0.0f, 0.0f, flow.data(),
                                    nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc != OFDIS_OK) {
      std::fprintf(stderr, "flow computation failed: %s\n", ofdis_status_string(rc));
      status = 1;
      break;
    }
    for (int i = 0; i < m; ++i) {
      char num[32];
      std::snprintf(num, sizeof(num), "%06d.flo", first + i);
      const std::string path = std::string(argv[1]) + num;
      if (ofdis_write_flo(path.c_str(), flow.data() + (size_t)i * out_frame, w, h, 2) != OFDIS_OK) {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        status = 1;
        break;
      }
    }
  }
  ofdis_context_destroy(ctx);
  return status;
}

// run_eval.cpp -- the evaluation command lines: a flow scored against a ground-truth .flo file on the device.
//
//   run_OF_EVAL_INT a.png b.png gt.flo [oppoint 1-4, default 2 | the 20 explicit parameters] [mask.pgm [mask_eq]]
//   run_OF_EVAL_RGB a.png b.png gt.flo [oppoint 1-4, default 2 | the 20 explicit parameters] [mask.pgm [mask_eq]]
//   eval_OF         est.flo gt.flo [mask.pgm [mask_eq]]                                       (-DEVAL_FILES)
//
// run_OF_EVAL_*: ofdis_run_error_u8_host, the flow a -> b and its error in one call (no full-resolution flow exists).
// eval_OF: ofdis_flow_error on two files.  Unknown truth is marked as .flo files mark it (|value| > 1e9).  mask.pgm
// keeps its nonzero pixels, or with mask_eq (0 .. 255) the pixels equal to it.  Both print one readable line -- EPE,
// R1 / R3 / R5, Fl, the speed-class means, the maximum, the 99th percentile from the histogram -- and then the 16 raw
// numbers with %.17g on a line starting STATS.  SELECTCHANNEL (1 gray, 3 BGR) is compile-time, as in run_dense.cpp.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ofdis.h"

#ifdef EVAL_FILES
#include <hip/hip_runtime_api.h>
#endif

#ifndef SELECTCHANNEL
#define SELECTCHANNEL 1
#endif
#define NOCHANNELS (SELECTCHANNEL == 3 ? 3 : 1)

// cv::imread(path, GRAYSCALE / COLOR)
static bool load(const char *path, int noc, std::vector<uint8_t> &px, int &w, int &h) {
  int rc = ofdis_read_image(path, nullptr, &w, &h, noc, 0);
  if (rc == OFDIS_OK) {
    px.resize((size_t)w * h * noc);
    rc = ofdis_read_image(path, px.data(), &w, &h, noc, px.size());
  }
  if (rc != OFDIS_OK) std::fprintf(stderr, "cannot read %s (PNG, Netpbm or BMP expected): %s\n", path, ofdis_status_string(rc));
  return rc == OFDIS_OK;
}

static bool load_flo(const char *path, std::vector<float> &f, int &w, int &h) {
  int rc = ofdis_read_flo(path, nullptr, &w, &h, 2);
  if (rc == OFDIS_OK) {
    f.resize((size_t)w * h * 2);
    rc = ofdis_read_flo(path, f.data(), &w, &h, 2);
  }
  if (rc != OFDIS_OK) std::fprintf(stderr, "cannot read %s (.flo expected): %s\n", path, ofdis_status_string(rc));
  return rc == OFDIS_OK;
}

// An integer argument in [lo, hi]; false for anything else.
static bool parse_int(const char *s, long lo, long hi, int &v) {
  char *end = nullptr;
  const long r = std::strtol(s, &end, 10);
  if (end == s || *end != '\0' || r < lo || r > hi) return false;
  v = (int)r;
  return true;
}

// [mask.pgm [mask_eq]] from argv[i ..]: false for a bad mask_eq, an unreadable mask or one of another size.
static bool load_mask(int argc, char **argv, int i, int w, int h, std::vector<uint8_t> &mask, int &mask_eq) {
  mask_eq = -1;
  if (i >= argc) return true;
  if (i + 1 < argc && !parse_int(argv[i + 1], 0, 255, mask_eq)) {
    std::fprintf(stderr, "mask_eq must be 0 .. 255\n");
    return false;
  }
  int mw = 0, mh = 0;
  if (!load(argv[i], 1, mask, mw, mh)) return false;
  if (mw != w || mh != h) {
    std::fprintf(stderr, "the mask is %dx%d, the flow %dx%d\n", mw, mh, w, h);
    return false;
  }
  return true;
}

// The upper edge of the bin holding the q-quantile of the scored errors (1/16 px; the last bin is open).
static double percentile(const std::vector<uint32_t> &hist, double q) {
  unsigned long long total = 0, run = 0;
  for (uint32_t c : hist) total += c;
  if (!total) return std::nan("");
  unsigned long long rank = (unsigned long long)std::ceil(q * (double)total);
  if (rank < 1) rank = 1;
  for (size_t b = 0; b < hist.size(); ++b) {
    run += hist[b];
    if (run >= rank) return b + 1 == hist.size() ? INFINITY : (double)(b + 1) / 16.0;
  }
  return INFINITY;
}

static void report(const double *s, const std::vector<uint32_t> &hist) {
  auto div = [](double a, double b) { return b > 0 ? a / b : std::nan(""); };
  std::printf("EPE %.4f  R1 %.4f R3 %.4f R5 %.4f  Fl %.4f  s0-10 %.4f s10-40 %.4f s40+ %.4f  max %.4f  p99 %.4f  (%.0f px, %.0f non-finite)\n",
              div(s[2], s[0] - s[1]), div(s[4], s[0]), div(s[5], s[0]), div(s[6], s[0]), div(s[7], s[0]), div(s[9], s[8]),
              div(s[11], s[10]), div(s[13], s[12]), s[3], percentile(hist, 0.99), s[0], s[1]);
  std::printf("STATS");
  for (int k = 0; k < OFDIS_FE_NSTATS; ++k) std::printf(" %.17g", s[k]);
  std::printf("\n");
}

#ifdef EVAL_FILES

int main(int argc, char **argv) {
  if (argc < 3 || argc > 5) {
    std::fprintf(stderr, "usage: %s <est.flo> <gt.flo> [mask.pgm [mask_eq 0-255]]\n", argv[0]);
    return 1;
  }
  std::vector<float> est, gt;
  int w = 0, h = 0, wg = 0, hg = 0, mask_eq = -1;
  if (!load_flo(argv[1], est, w, h) || !load_flo(argv[2], gt, wg, hg)) return 1;
  if (w != wg || h != hg) {
    std::fprintf(stderr, "flow sizes differ: %dx%d and %dx%d\n", w, h, wg, hg);
    return 1;
  }
  std::vector<uint8_t> mask;
  if (!load_mask(argc, argv, 3, w, h, mask, mask_eq)) return 1;
  ofdis_context *ctx = nullptr;
  int rc = ofdis_context_create(0, &ctx);
  if (rc != OFDIS_OK) {
    std::fprintf(stderr, "no usable gfx950 device: %s\n", ofdis_status_string(rc));
    return 1;
  }
  // one device block: the estimate, the truth, the mask, the numbers, the histogram (each at a multiple of 256 bytes)
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t px = (size_t)w * h, off_gt = up(px * 8), off_mask = 2 * up(px * 8), off_stats = off_mask + up(px);
  const size_t off_hist = off_stats + up(OFDIS_FE_NSTATS * 8);
  char *d = nullptr;
  double stats[OFDIS_FE_NSTATS];
  std::vector<uint32_t> hist(OFDIS_FE_BINS);
  bool ok = hipMalloc((void **)&d, off_hist + OFDIS_FE_BINS * 4) == hipSuccess;
  ok = ok && hipMemcpy(d, est.data(), px * 8, hipMemcpyHostToDevice) == hipSuccess &&
       hipMemcpy(d + off_gt, gt.data(), px * 8, hipMemcpyHostToDevice) == hipSuccess &&
       (mask.empty() || hipMemcpy(d + off_mask, mask.data(), px, hipMemcpyHostToDevice) == hipSuccess);
  if (ok) {
    const ofdis_flow_view v{OFDIS_OUT_F32, OFDIS_OUT_INTERLEAVED, OFDIS_OUT_FULL, w, h, 1, 0, 0};
    rc = ofdis_flow_error(ctx, d, &v, (const float *)(d + off_gt), mask.empty() ? nullptr : (const uint8_t *)(d + off_mask),
                          mask_eq, 1, w, h, (double *)(d + off_stats), nullptr, (uint32_t *)(d + off_hist), nullptr);
    ok = rc == OFDIS_OK && hipDeviceSynchronize() == hipSuccess &&
         hipMemcpy(stats, d + off_stats, sizeof(stats), hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(hist.data(), d + off_hist, OFDIS_FE_BINS * 4, hipMemcpyDeviceToHost) == hipSuccess;
  }
  if (d) (void)hipFree(d);
  ofdis_context_destroy(ctx);
  if (!ok) {
    std::fprintf(stderr, "evaluation failed: %s\n", ofdis_status_string(rc != OFDIS_OK ? rc : OFDIS_ERR_DEVICE));
    return 1;
  }
  report(stats, hist);
  return 0;
}

#else

int main(int argc, char **argv) {
  // argv[4 ..]: nothing, an op-point, or the 20 explicit parameters; then the optional mask and mask_eq
  int op = 2, rest = 4;
  const bool explicit20 = argc >= 24;
  if (explicit20) rest = 24;
  else if (argc >= 5 && parse_int(argv[4], 1, 4, op)) rest = 5;
  if (argc < 4 || argc > rest + 2) {
    std::fprintf(stderr, "usage: %s <image a> <image b> <gt.flo> [oppoint 1-4 | 20 parameters] [mask.pgm [mask_eq 0-255]]\n", argv[0]);
    return 1;
  }
  std::vector<uint8_t> a, b, mask;
  std::vector<float> gt;
  int w = 0, h = 0, wb = 0, hb = 0, wg = 0, hg = 0, mask_eq = -1;
  if (!load(argv[1], NOCHANNELS, a, w, h) || !load(argv[2], NOCHANNELS, b, wb, hb) || !load_flo(argv[3], gt, wg, hg)) return 1;
  if (w != wb || h != hb || w != wg || h != hg) {
    std::fprintf(stderr, "sizes differ: %dx%d, %dx%d and %dx%d\n", w, h, wb, hb, wg, hg);
    return 1;
  }
  if (!load_mask(argc, argv, rest, w, h, mask, mask_eq)) return 1;
  ofdis_params p;
  int rc = explicit20 ? ofdis_params_from_strings(&p, 20, argv + 4, OFDIS_MODE_OF, NOCHANNELS)
                      : ofdis_params_oppoint(&p, op, w, OFDIS_MODE_OF, NOCHANNELS);
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
  double stats[OFDIS_FE_NSTATS];
  std::vector<uint32_t> hist(OFDIS_FE_BINS);
  rc = ofdis_run_error_u8_host(ctx, a.data(), b.data(), gt.data(), mask.empty() ? nullptr : mask.data(), mask_eq, 1, w, h,
                               &p, stats, nullptr, hist.data());
  ofdis_context_destroy(ctx);
  if (rc != OFDIS_OK) {
    std::fprintf(stderr, "evaluation failed: %s\n", ofdis_status_string(rc));
    return 1;
  }
  report(stats, hist);
  return 0;
}

#endif

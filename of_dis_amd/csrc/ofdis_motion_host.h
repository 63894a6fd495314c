// ofdis_motion_host.h -- the host-side arithmetic of the motion calls (include/ofdis.h: ofdis_fit_motion,
// ofdis_smooth_path, ofdis_motion_mask): the sample lattice, the scalar refusals and the annealed thresholds.  No device
// code and no HIP header: tools/motion_host_check.cpp and tools/motion_mask_host_check.cpp build these functions alone,
// under the host sanitizers.
#ifndef OFDIS_MOTION_HOST_H
#define OFDIS_MOTION_HOST_H

#include <cmath>

namespace ofdis {

constexpr int kMotionMaxSamples = 65536;  // OFDIS_FIT_MAX_SAMPLES
constexpr int kMotionMaxIters = 16;

// The lattice of a W x H frame at `step`: columns half + i * step for i < sx, rows likewise, ns = sx * sy samples.
struct FitLattice {
  int half = 0, sx = 0, sy = 0, ns = 0;
};

// False for what ofdis_fit_motion refuses of a size and a step: a non-positive size, step < 1, a first sample outside
// the frame (step / 2 > min(W, H) - 1), more than OFDIS_FIT_MAX_SAMPLES samples.
inline bool fit_lattice(int W, int H, int step, FitLattice &L) {
  if (W < 1 || H < 1 || step < 1) return false;
  const int half = step / 2;
  if (half > (W < H ? W : H) - 1) return false;
  const long sx = (long)(W - 1 - half) / step + 1, sy = (long)(H - 1 - half) / step + 1;
  if (sx * sy > kMotionMaxSamples) return false;
  L.half = half;
  L.sx = (int)sx;
  L.sy = (int)sy;
  L.ns = (int)(sx * sy);
  return true;
}

// model 0 (translation) or 1 (similarity), tau finite in [1/1024, 65536], iters in 0 .. 16.
inline bool fit_scalars_ok(int model, double tau, int iters) {
  if (model != 0 && model != 1) return false;
  if (!(tau >= 1.0 / 1024.0 && tau <= 65536.0)) return false;  // (false for NaN)
  return iters >= 0 && iters <= kMotionMaxIters;
}

// inv[it] = 1 / t_it^2 with t_it = tau * 2^(iters - it) for it = 1 .. iters (inv[0] is not read: solve 0 has no
// threshold).  The power of two is exact, the product and the division are rounded once each.
inline void fit_inv_table(double tau, int iters, double *inv) {
  inv[0] = 0.0;
  for (int it = 1; it <= iters; ++it) {
    const double t = std::ldexp(tau, iters - it);
    inv[it] = 1.0 / (t * t);
  }
}

// What ofdis_smooth_path refuses of its scalars: m < 1, radius outside 0 .. 256, zoom not finite or outside [1, 16], a
// non-positive size.
inline bool path_scalars_ok(int m, int radius, double zoom, int W, int H) {
  if (m < 1 || radius < 0 || radius > 256 || W < 1 || H < 1) return false;
  return zoom >= 1.0 && zoom <= 16.0;  // (false for NaN)
}

// What ofdis_motion_mask refuses of its scalars: m < 1, thr not finite or outside [0, 65536], rel not finite or outside
// [0, 16], radius outside 0 .. 4, a non-positive size, W * H >= 2^31.
constexpr int kMotionMaskMaxRadius = 4;
inline bool mask_scalars_ok(int m, float thr, float rel, int radius, int W, int H) {
  if (m < 1 || W < 1 || H < 1 || (long long)W * H > 0x7fffffffLL) return false;
  if (!(thr >= 0.0f && thr <= 65536.0f) || !(rel >= 0.0f && rel <= 16.0f)) return false;  // (false for NaN)
  return radius >= 0 && radius <= kMotionMaskMaxRadius;
}

}  // namespace ofdis

#endif  // OFDIS_MOTION_HOST_H

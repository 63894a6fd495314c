// motion_host_check.cpp -- the host-side arithmetic of the motion calls (of_dis_amd/csrc/ofdis_motion_host.h) on its
// own: the sample lattice over a sweep of sizes and steps, the scalar refusals at and around their limits, the annealed
// threshold table.  No device and no HIP: built and run under the host sanitizers,
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/motion_host_check.cpp \
//       -o motion_host_check && ./motion_host_check
//
// it prints one line per probe for tests/test_stabilize.py to compare with the Python statement, walks every sample of
// every lattice it builds through a frame-sized array (an index outside the frame is the sanitizer's to report), and
// returns 1 when a property fails.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../of_dis_amd/csrc/ofdis_motion_host.h"

using namespace ofdis;

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::fprintf(stderr, "line %d: %s fails\n", __LINE__, #c); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

int main() {
  // lattices: every sample inside the frame, the next one outside, the counts the kernel is launched with
  const int sizes[][2] = {{160, 120}, {150, 110}, {161, 121}, {176, 96}, {1920, 1080}, {4096, 2160}, {1, 1}, {7, 5}, {2100, 70}, {256, 256}};
  const int steps[] = {1, 2, 3, 8, 15, 16, 17, 64, 139, 512};
  for (const auto &sz : sizes) {
    const int W = sz[0], H = sz[1];
    std::vector<unsigned char> frame((size_t)W * H, 0);
    for (int step : steps) {
      FitLattice L;
      const bool ok = fit_lattice(W, H, step, L);
      std::printf("lattice %d %d %d -> %d %d %d %d %d\n", W, H, step, (int)ok, L.half, L.sx, L.sy, L.ns);
      if (!ok) continue;
      CHECK(L.ns == L.sx * L.sy && L.ns >= 1 && L.ns <= kMotionMaxSamples);
      for (int s = 0; s < L.ns; ++s) {
        const int r = s / L.sx, i = s - r * L.sx;
        const int x = L.half + i * step, y = L.half + r * step;
        frame[(size_t)y * W + x] += 1;  // (out of the frame: the sanitizer's)
      }
      CHECK(L.half + L.sx * step > W - 1 && L.half + L.sy * step > H - 1);  // the lattice is not one short
    }
  }
  FitLattice L;
  CHECK(!fit_lattice(0, 5, 1, L) && !fit_lattice(5, 0, 1, L) && !fit_lattice(5, 5, 0, L) && !fit_lattice(5, 5, -3, L));
  CHECK(!fit_lattice(16, 8, 16, L) && fit_lattice(16, 9, 16, L));         // step / 2 = 8 against min(W, H) - 1
  CHECK(fit_lattice(256, 256, 1, L) && L.ns == 65536 && !fit_lattice(257, 256, 1, L));
  const int big = std::numeric_limits<int>::max();
  CHECK(!fit_lattice(big, big, 1, L) && fit_lattice(big, big, big, L) && L.ns == 1);  // no overflow on the way
  CHECK(fit_lattice(46340, 46340, 200, L) && L.ns == 232 * 232);

  // scalars at and around their limits
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  CHECK(fit_scalars_ok(0, 2.0, 4) && fit_scalars_ok(1, 1.0 / 1024.0, 0) && fit_scalars_ok(1, 65536.0, 16));
  CHECK(!fit_scalars_ok(2, 2.0, 4) && !fit_scalars_ok(-1, 2.0, 4) && !fit_scalars_ok(1, 2.0, -1) && !fit_scalars_ok(1, 2.0, 17));
  CHECK(!fit_scalars_ok(1, nan, 4) && !fit_scalars_ok(1, inf, 4) && !fit_scalars_ok(1, -2.0, 4) && !fit_scalars_ok(1, 0.0, 4));
  CHECK(!fit_scalars_ok(1, std::nextafter(1.0 / 1024.0, 0.0), 4) && !fit_scalars_ok(1, std::nextafter(65536.0, inf), 4));
  CHECK(path_scalars_ok(1, 0, 1.0, 1, 1) && path_scalars_ok(1 << 20, 256, 16.0, 4096, 4096));
  CHECK(!path_scalars_ok(0, 2, 1.0, 8, 8) && !path_scalars_ok(3, -1, 1.0, 8, 8) && !path_scalars_ok(3, 257, 1.0, 8, 8));
  CHECK(!path_scalars_ok(3, 2, nan, 8, 8) && !path_scalars_ok(3, 2, inf, 8, 8) && !path_scalars_ok(3, 2, 0.999, 8, 8));
  CHECK(!path_scalars_ok(3, 2, 16.5, 8, 8) && !path_scalars_ok(3, 2, 1.0, 0, 8) && !path_scalars_ok(3, 2, 1.0, 8, -1));

  // the threshold table: every entry of every allowed length, at the extreme taus (guard values around the array)
  const double taus[] = {1.0 / 1024.0, 0.3, 2.0, 65536.0};
  for (double tau : taus) {
    for (int iters = 0; iters <= kMotionMaxIters; ++iters) {
      std::vector<double> inv((size_t)iters + 1, -1.0);  // exactly iters + 1 entries: one more write is the sanitizer's
      fit_inv_table(tau, iters, inv.data());
      CHECK(inv[0] == 0.0);
      for (int it = 1; it <= iters; ++it) {
        const double t = tau * std::pow(2.0, iters - it);
        CHECK(inv[it] == 1.0 / (t * t) && std::isfinite(inv[it]) && inv[it] > 0.0);
        if (it > 1) CHECK(inv[it] == 4.0 * inv[it - 1]);  // halving the threshold is exact
      }
      if (iters == 4 || iters == kMotionMaxIters) {
        std::printf("inv %.17g %d ->", tau, iters);
        for (int it = 1; it <= iters; ++it) std::printf(" %.17g", inv[it]);
        std::printf("\n");
      }
    }
  }
  std::printf("failures %d\n", failures);
  return failures ? 1 : 0;
}

// motion_mask_host_check.cpp -- the scalar refusals of the motion-mask calls (of_dis_amd/csrc/ofdis_motion_host.h:
// mask_scalars_ok) on their own, at and around their limits.  No device and no HIP: built and run under the host
// sanitizers,
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/motion_mask_host_check.cpp \
//       -o motion_mask_host_check && ./motion_mask_host_check
//
// it prints one line per probe of a sweep for tests/test_motion_mask.py to compare with the Python statement, and
// returns 1 when a property fails.
#include <cmath>
#include <cstdio>
#include <limits>

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
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  // the allowed corners
  CHECK(mask_scalars_ok(1, 0.0f, 0.0f, 0, 1, 1) && mask_scalars_ok(1 << 20, 65536.0f, 16.0f, 4, 4096, 4096));
  CHECK(mask_scalars_ok(5, 1.0f, 0.05f, 1, 160, 120));
  // m and the size
  CHECK(!mask_scalars_ok(0, 1.0f, 0.05f, 1, 8, 8) && !mask_scalars_ok(-1, 1.0f, 0.05f, 1, 8, 8));
  CHECK(!mask_scalars_ok(1, 1.0f, 0.05f, 1, 0, 8) && !mask_scalars_ok(1, 1.0f, 0.05f, 1, 8, -1));
  const int big = std::numeric_limits<int>::max();
  CHECK(mask_scalars_ok(1, 1.0f, 0.05f, 1, big, 1) && !mask_scalars_ok(1, 1.0f, 0.05f, 1, big, 2));  // W * H < 2^31
  CHECK(mask_scalars_ok(1, 1.0f, 0.05f, 1, 46340, 46340) && !mask_scalars_ok(1, 1.0f, 0.05f, 1, 46341, 46341));
  CHECK(!mask_scalars_ok(1, 1.0f, 0.05f, 1, big, big));  // no overflow on the way
  // thr
  CHECK(!mask_scalars_ok(1, nan, 0.05f, 1, 8, 8) && !mask_scalars_ok(1, inf, 0.05f, 1, 8, 8));
  CHECK(!mask_scalars_ok(1, -0.5f, 0.05f, 1, 8, 8) && !mask_scalars_ok(1, std::nextafter(65536.0f, inf), 0.05f, 1, 8, 8));
  CHECK(!mask_scalars_ok(1, std::nextafter(0.0f, -1.0f), 0.05f, 1, 8, 8) && mask_scalars_ok(1, -0.0f, 0.05f, 1, 8, 8));
  // rel
  CHECK(!mask_scalars_ok(1, 1.0f, nan, 1, 8, 8) && !mask_scalars_ok(1, 1.0f, inf, 1, 8, 8));
  CHECK(!mask_scalars_ok(1, 1.0f, -0.01f, 1, 8, 8) && !mask_scalars_ok(1, 1.0f, std::nextafter(16.0f, inf), 1, 8, 8));
  // radius
  CHECK(!mask_scalars_ok(1, 1.0f, 0.05f, -1, 8, 8) && !mask_scalars_ok(1, 1.0f, 0.05f, 5, 8, 8));
  CHECK(kMotionMaskMaxRadius == 4);
  for (int r = 0; r <= kMotionMaskMaxRadius; ++r) CHECK(mask_scalars_ok(1, 1.0f, 0.05f, r, 8, 8));

  // a sweep for the Python statement
  const float thrs[] = {-1.0f, 0.0f, 1.0f, 65536.0f, 65537.0f, nan};
  const float rels[] = {-0.5f, 0.0f, 0.05f, 16.0f, 16.5f, inf};
  const int radii[] = {-1, 0, 4, 5};
  const int ms[] = {0, 1, 7};
  const int sizes[][2] = {{160, 120}, {1, 1}, {0, 4}, {65536, 32768}, {65536, 32767}};
  for (int m : ms)
    for (float thr : thrs)
      for (float rel : rels)
        for (int radius : radii)
          for (const auto &sz : sizes)
            std::printf("mask %d %.9g %.9g %d %d %d -> %d\n", m, (double)thr, (double)rel, radius, sz[0], sz[1],
                        (int)mask_scalars_ok(m, thr, rel, radius, sz[0], sz[1]));
  std::printf("failures %d\n", failures);
  return failures ? 1 : 0;
}

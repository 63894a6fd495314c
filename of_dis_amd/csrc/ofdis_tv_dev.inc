// ofdis_tv_dev.inc -- device helpers of the variational refinement (included INSIDE namespace ofdis
// { namespace { ... } } of the kernel translation units, ofdis_kernels.hip and ofdis_tvrb.hip: every definition is
// internal to its unit).  Same expressions as the reference (FDF1.0.1), cited per function.
#pragma once

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float stdmaxf(float a, float b) { return (a < b) ? b : a; }
__device__ __forceinline__ float stdminf(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float ssemin(float a, float b) { return (a < b) ? a : b; }
__device__ __forceinline__ float ssemax(float a, float b) { return (a > b) ? a : b; }

// Pixel (x, y) of a w x h level sits in row d = x + y (its anti-diagonal), column y.  With `wrap` (h <= w)
// the rows are folded modulo w: row d mod w then holds exactly one pixel of every column, the plane has no
// holes (w * h slots instead of (w + h - 1) * h) and the pixels of one wavefront step stay contiguous.
__device__ __forceinline__ int skrow(int d, int w, int wrap) { return wrap && d >= w ? d - w : d; }
__device__ __forceinline__ long skw(int x, int y, int h, int w, int wrap) {
  return (long)skrow(x + y, w, wrap) * h + y;
}

// image_warp's mask (opticalflow_aux.c:47): 1 where the warped position (x + wx, y + wy) lies inside the level.
__device__ __forceinline__ float warp_mask(int x, int y, float wx, float wy, int w, int h) {
  const float xx = (float)x + wx, yy = (float)y + wy;
  return (xx >= 0 && xx <= (float)(w - 1) && yy >= 0 && yy <= (float)(h - 1)) ? 1.0f : 0.0f;
}

__constant__ float kK5[5] = {1.0f / 12.0f, -8.0f / 12.0f, -0.0f, 8.0f / 12.0f, -1.0f / 12.0f};
__constant__ float kK3[3] = {-0.5f, -0.0f, 0.5f};

// Load base[idx] through a 32-bit byte offset on a wave-uniform base: global_load's SGPR-base form, no
// 64-bit address arithmetic per load.  The runtime keeps every TV plane group below 2^30 floats.
__device__ __forceinline__ float ldu(const float *base, unsigned idx) {
  return *reinterpret_cast<const float *>(reinterpret_cast<const char *>(base) + (size_t)(idx * 4u));
}

#define DNORM (0.1f * 0.1f)
#define EPSC (0.001f * 0.001f)

// compute_data (opticalflow_aux.c:408-594) of an intensity image, one pixel, in its two halves: the colour
// (brightness constancy) term, :457-509, and the gradient constancy term, :510-571 with the final x 3 (:572-577).
// A11 .. B2 enter the colour half as 0 (the reference's zero-initialised a11 .. b2).  data_of runs the halves back to
// back for every caller: through sys_compute the system kernels (ofdis_kernels.hip) and the latency mode's level
// launch k_tv_level_rb (ofdis_tvrb.hip).
__device__ __forceinline__ void data_of_gray_colour(float u, float v, float m, float Ix, float Iy, float Iz, float hdo3,
                                                    float &A11, float &A12, float &A22, float &B1, float &B2) {
  A11 = 0.0f; A12 = 0.0f; A22 = 0.0f; B1 = 0.0f; B2 = 0.0f;
  if (hdo3 != 0.0f) {
    float tmp, tmp2, tmp3, tmpx, tmpy, n1;
    tmpx = Ix; tmpy = Iy;
    tmp2 = (Iz + tmpx * u) + tmpy * v;
    n1 = (DNORM + tmpx * tmpx) + tmpy * tmpy;
    tmp = (tmp2 * tmp2) / n1;
    tmp = (m * hdo3) / sqrtf(EPSC + 3.0f * tmp);
    tmp3 = tmp / n1;
    tmp2 = tmp3 * tmpx;
    tmp3 = tmp3 * tmpy;
    A11 = A11 + tmp2 * tmpx; A12 = A12 + tmp2 * tmpy; A22 = A22 + tmp3 * tmpy;
    B1 = B1 - tmp2 * Iz; B2 = B2 - tmp3 * Iz;
  }
}
__device__ __forceinline__ void data_of_gray_gradient(float u, float v, float m, float Ixx, float Ixy, float Iyy,
                                                      float Ixz, float Iyz, float hgo3, float &A11, float &A12,
                                                      float &A22, float &B1, float &B2) {
  float tmp, tmp2, tmp3, tmpx, tmpy, tmpxy, n1, n2;
  tmpx = Ixx; tmpy = Iyy; tmpxy = Ixy;
  tmp2 = (Ixz + tmpx * u) + tmpxy * v;
  tmp3 = (Iyz + tmpxy * u) + tmpy * v;
  tmpxy = tmpxy * tmpxy;
  n1 = (tmpxy + DNORM) + tmpx * tmpx;
  n2 = (tmpxy + DNORM) + tmpy * tmpy;
  tmp = (tmp2 * tmp2) / n1 + (tmp3 * tmp3) / n2;
  tmp = (m * hgo3) / sqrtf(EPSC + 3.0f * tmp);
  tmp2 = tmp / n2; tmp3 = tmp / n1;
  tmpxy = Ixy;
  A12 = A12 + ((tmp3 * tmpx) + tmp2 * tmpy) * tmpxy;
  B1 = (B1 - (tmp3 * tmpx) * Ixz) - (tmp2 * tmpxy) * Iyz;
  B2 = (B2 - (tmp2 * tmpy) * Iyz) - (tmp3 * tmpxy) * Ixz;
  tmpxy = tmpxy * tmpxy;
  A11 = (A11 + tmp3 * (tmpx * tmpx)) + tmp2 * tmpxy;
  A22 = (A22 + tmp2 * (tmpy * tmpy)) + tmp3 * tmpxy;
  A11 = A11 * 3.0f; A12 = A12 * 3.0f; A22 = A22 * 3.0f; B1 = B1 * 3.0f; B2 = B2 * 3.0f;
}

// compute_data (opticalflow_aux.c:408-594), one pixel; p* point at the pixel in channel plane 0.
__device__ __forceinline__ void data_of(int noc, long plane, float u, float v, float m, const float *Ix,
                                        const float *Iy, const float *Iz, const float *Ixx, const float *Ixy,
                                        const float *Iyy, const float *Ixz, const float *Iyz, float hdo3, float hgo3,
                                        float &A11, float &A12, float &A22, float &B1, float &B2) {
  if (noc == 1) {
    data_of_gray_colour(u, v, m, Ix[0], Iy[0], Iz[0], hdo3, A11, A12, A22, B1, B2);
    data_of_gray_gradient(u, v, m, Ixx[0], Ixy[0], Iyy[0], Ixz[0], Iyz[0], hgo3, A11, A12, A22, B1, B2);
    return;
  }
  A11 = 0.0f; A12 = 0.0f; A22 = 0.0f; B1 = 0.0f; B2 = 0.0f;
  float tmp, tmp2, tmp3, tmpx, tmpy, tmpxy, n1, n2;
  const long o2 = plane, o3 = 2 * plane;
  float n3, n4, n5, n6;
  if (hdo3 != 0.0f) {
    tmpx = Ix[0]; tmpy = Iy[0];
    tmp2 = (Iz[0] + tmpx * u) + tmpy * v;
    n1 = (DNORM + tmpx * tmpx) + tmpy * tmpy;
    tmp = (tmp2 * tmp2) / n1;
    tmpx = Ix[o2]; tmpy = Iy[o2];
    tmp2 = (Iz[o2] + tmpx * u) + tmpy * v;
    n2 = (DNORM + tmpx * tmpx) + tmpy * tmpy;
    tmp = tmp + (tmp2 * tmp2) / n2;
    tmpx = Ix[o3]; tmpy = Iy[o3];
    tmp2 = (Iz[o3] + tmpx * u) + tmpy * v;
    n3 = (DNORM + tmpx * tmpx) + tmpy * tmpy;
    tmp = tmp + (tmp2 * tmp2) / n3;
    tmp = (m * hdo3) / sqrtf(EPSC + tmp);
    tmp3 = tmp / n3; tmp2 = tmp3 * tmpx; tmp3 = tmp3 * tmpy;
    A11 = A11 + tmp2 * tmpx; A12 = A12 + tmp2 * tmpy; A22 = A22 + tmp3 * tmpy;
    B1 = B1 - tmp2 * Iz[o3]; B2 = B2 - tmp3 * Iz[o3];
    tmpx = Ix[o2]; tmpy = Iy[o2];
    tmp3 = tmp / n2; tmp2 = tmp3 * tmpx; tmp3 = tmp3 * tmpy;
    A11 = A11 + tmp2 * tmpx; A12 = A12 + tmp2 * tmpy; A22 = A22 + tmp3 * tmpy;
    B1 = B1 - tmp2 * Iz[o2]; B2 = B2 - tmp3 * Iz[o2];
    tmpx = Ix[0]; tmpy = Iy[o2];  // upstream slip: channel 2's Iy (opticalflow_aux.c:495-496)
    tmp3 = tmp / n1; tmp2 = tmp3 * tmpx; tmp3 = tmp3 * tmpy;
    A11 = A11 + tmp2 * tmpx; A12 = A12 + tmp2 * tmpy; A22 = A22 + tmp3 * tmpy;
    B1 = B1 - tmp2 * Iz[0]; B2 = B2 - tmp3 * Iz[0];
  }
  tmpx = Ixx[0]; tmpy = Iyy[0]; tmpxy = Ixy[0];
  tmp2 = (Ixz[0] + tmpx * u) + tmpxy * v;
  tmp3 = (Iyz[0] + tmpxy * u) + tmpy * v;
  tmpxy = tmpxy * tmpxy;
  n1 = (tmpxy + DNORM) + tmpx * tmpx;
  n2 = (tmpxy + DNORM) + tmpy * tmpy;
  tmp = (tmp2 * tmp2) / n1 + (tmp3 * tmp3) / n2;
  tmpx = Ixx[o2]; tmpy = Iyy[o2]; tmpxy = Ixy[o2];
  tmp2 = (Ixz[o2] + tmpx * u) + tmpxy * v;
  tmp3 = (Iyz[o2] + tmpxy * u) + tmpy * v;
  tmpxy = tmpxy * tmpxy;
  n3 = (tmpxy + DNORM) + tmpx * tmpx;
  n4 = (tmpxy + DNORM) + tmpy * tmpy;
  tmp = (tmp2 * tmp2) / n3 + (tmp3 * tmp3) / n4;  // upstream overwrite (opticalflow_aux.c:519,529,538)
  tmpx = Ixx[o3]; tmpy = Iyy[o3]; tmpxy = Ixy[o3];
  tmp2 = (Ixz[o3] + tmpx * u) + tmpxy * v;
  tmp3 = (Iyz[o3] + tmpxy * u) + tmpy * v;
  tmpxy = tmpxy * tmpxy;
  n5 = (tmpxy + DNORM) + tmpx * tmpx;
  n6 = (tmpxy + DNORM) + tmpy * tmpy;
  tmp = (tmp2 * tmp2) / n5 + (tmp3 * tmp3) / n6;
  tmp = (m * hgo3) / sqrtf(EPSC + tmp);
  tmp2 = tmp / n6; tmp3 = tmp / n5;
  A11 = (A11 + tmp3 * (tmpx * tmpx)) + tmp2 * tmpxy;
  A22 = (A22 + tmp2 * (tmpy * tmpy)) + tmp3 * tmpxy;
  tmpxy = Ixy[o3];
  A12 = A12 + ((tmp3 * tmpx) + tmp2 * tmpy) * tmpxy;
  B1 = (B1 - (tmp3 * tmpx) * Ixz[o3]) - (tmp2 * tmpxy) * Iyz[o3];
  B2 = (B2 - (tmp2 * tmpy) * Iyz[o3]) - (tmp3 * tmpxy) * Ixz[o3];
  tmp2 = tmp / n4; tmp3 = tmp / n3;
  tmpx = Ixx[o2]; tmpy = Iyy[o2]; tmpxy = Ixy[o2];
  A12 = A12 + ((tmp3 * tmpx) + tmp2 * tmpy) * tmpxy;
  B1 = (B1 - (tmp3 * tmpx) * Ixz[o2]) - (tmp2 * tmpxy) * Iyz[o2];
  B2 = (B2 - (tmp2 * tmpy) * Iyz[o2]) - (tmp3 * tmpxy) * Ixz[o2];
  tmpxy = tmpxy * tmpxy;
  A11 = (A11 + tmp3 * (tmpx * tmpx)) + tmp2 * tmpxy;
  A22 = (A22 + tmp2 * (tmpy * tmpy)) + tmp3 * tmpxy;
  tmpx = Ixx[0]; tmpy = Iyy[0];
  tmp2 = tmp / n2; tmp3 = tmp / n1;
  tmpxy = Ixy[0];
  A12 = A12 + ((tmp3 * tmpx) + tmp2 * tmpy) * tmpxy;
  B1 = (B1 - (tmp3 * tmpx) * Ixz[0]) - (tmp2 * tmpxy) * Iyz[0];
  B2 = (B2 - (tmp2 * tmpy) * Iyz[0]) - (tmp3 * tmpxy) * Ixz[0];
  tmpxy = tmpxy * tmpxy;
  A11 = (A11 + tmp3 * (tmpx * tmpx)) + tmp2 * tmpxy;
  A22 = (A22 + tmp2 * (tmpy * tmpy)) + tmp3 * tmpxy;
}

// compute_data_DE (opticalflow_aux.c:601-747), one pixel.
__device__ __forceinline__ void data_de(int noc, long plane, float u, float m, const float *Ix, const float *Iy,
                                        const float *Iz, const float *Ixx, const float *Ixy, const float *Iyy,
                                        const float *Ixz, const float *Iyz, float hdo3, float hgo3, float &A11,
                                        float &B1) {
  A11 = 0.0f; B1 = 0.0f;
  float tmp, tmp2, tmp3, tmpx, tmpy, tmpxy, n1, n2;
  if (noc == 1) {
    if (hdo3 != 0.0f) {
      tmpx = Ix[0]; tmpy = Iy[0];
      tmp2 = Iz[0] + tmpx * u;
      n1 = (DNORM + tmpy * tmpy) + tmpx * tmpx;
      tmp = (tmp2 * tmp2) / n1;
      tmp = (m * hdo3) / sqrtf(EPSC + 3.0f * tmp);
      tmp2 = (tmp / n1) * tmpx;
      A11 = A11 + tmp2 * tmpx;
      B1 = B1 - tmp2 * Iz[0];
    }
    tmpx = Ixx[0]; tmpy = Iyy[0]; tmpxy = Ixy[0];
    tmp2 = Iyz[0] + tmpxy * u;
    tmpxy = DNORM + tmpxy * tmpxy;
    n1 = tmpxy + tmpx * tmpx;
    n2 = tmpxy + tmpy * tmpy;
    tmp = (tmp2 * tmp2) / n2;
    tmp2 = Ixz[0] + tmpx * u;
    tmp = tmp + (tmp2 * tmp2) / n1;
    tmp = (m * hgo3) / sqrtf(EPSC + 3.0f * tmp);
    tmpxy = Ixy[0];
    tmp2 = (tmp / n2) * tmpxy; tmp3 = (tmp / n1) * tmpx;
    A11 = (A11 + tmp3 * tmpx) + tmp2 * tmpxy;
    B1 = (B1 - tmp3 * Ixz[0]) - tmp2 * Iyz[0];
    A11 = A11 * 3.0f; B1 = B1 * 3.0f;
    return;
  }
  const long o2 = plane, o3 = 2 * plane;
  float n3, n4, n5, n6;
  if (hdo3 != 0.0f) {
    tmpx = Ix[0]; tmpy = Iy[0];
    tmp2 = Iz[0] + tmpx * u;
    n1 = (DNORM + tmpy * tmpy) + tmpx * tmpx;
    tmp = (tmp2 * tmp2) / n1;
    tmpx = Ix[o2]; tmpy = Iy[o2];
    tmp2 = Iz[o2] + tmpx * u;
    n2 = (DNORM + tmpy * tmpy) + tmpx * tmpx;
    tmp = tmp + (tmp2 * tmp2) / n2;
    tmpx = Ix[o3]; tmpy = Iy[o3];
    tmp2 = Iz[o3] + tmpx * u;
    n3 = (DNORM + tmpy * tmpy) + tmpx * tmpx;
    tmp = tmp + (tmp2 * tmp2) / n3;
    tmp = (m * hdo3) / sqrtf(EPSC + tmp);
    tmp2 = (tmp / n3) * tmpx;
    A11 = A11 + tmp2 * tmpx; B1 = B1 - tmp2 * Iz[o3];
    tmpx = Ix[o2];
    tmp2 = (tmp / n2) * tmpx;
    A11 = A11 + tmp2 * tmpx; B1 = B1 - tmp2 * Iz[o2];
    tmpx = Ix[0];
    tmp2 = (tmp / n1) * tmpx;
    A11 = A11 + tmp2 * tmpx; B1 = B1 - tmp2 * Iz[0];
  }
  tmpx = Ixx[0]; tmpy = Iyy[0]; tmpxy = Ixy[0];
  tmp2 = Iyz[0] + tmpxy * u;
  tmpxy = DNORM + tmpxy * tmpxy;
  n1 = tmpxy + tmpx * tmpx;
  n2 = tmpxy + tmpy * tmpy;
  tmp = (tmp2 * tmp2) / n2;
  tmp2 = Ixz[0] + tmpx * u;
  tmp = tmp + (tmp2 * tmp2) / n1;
  tmpx = Ixx[o2]; tmpy = Iyy[o2]; tmpxy = Ixy[o2];
  tmp2 = Iyz[o2] + tmpxy * u;
  tmpxy = DNORM + tmpxy * tmpxy;
  n3 = tmpxy + tmpx * tmpx;
  n4 = tmpxy + tmpy * tmpy;
  tmp = tmp + (tmp2 * tmp2) / n4;
  tmp2 = Ixz[o2] + tmpx * u;
  tmp = tmp + (tmp2 * tmp2) / n3;
  tmpx = Ixx[o3]; tmpy = Iyy[o3]; tmpxy = Ixy[o3];
  tmp2 = Iyz[o3] + tmpxy * u;
  tmpxy = DNORM + tmpxy * tmpxy;
  n5 = tmpxy + tmpx * tmpx;
  n6 = tmpxy + tmpy * tmpy;
  tmp = tmp + (tmp2 * tmp2) / n6;
  tmp2 = Ixz[o3] + tmpx * u;
  tmp = tmp + (tmp2 * tmp2) / n5;
  tmp = (m * hgo3) / sqrtf(EPSC + tmp);
  tmpxy = Ixy[o3];
  tmp2 = (tmp / n6) * tmpxy; tmp3 = (tmp / n5) * tmpx;
  A11 = (A11 + tmp3 * tmpx) + tmp2 * tmpxy;
  B1 = (B1 - tmp3 * Ixz[o3]) - tmp2 * Iyz[o3];
  tmpx = Ixx[o2]; tmpxy = Ixy[o2];
  tmp2 = (tmp / n4) * tmpxy; tmp3 = (tmp / n3) * tmpx;
  A11 = (A11 + tmp3 * tmpx) + tmp2 * tmpxy;
  B1 = (B1 - tmp3 * Ixz[o2]) - tmp2 * Iyz[o2];
  tmpx = Ixx[0]; tmpxy = Ixy[0];
  tmp2 = (tmp / n2) * tmpxy; tmp3 = (tmp / n1) * tmpx;
  A11 = (A11 + tmp3 * tmpx) + tmp2 * tmpxy;
  B1 = (B1 - tmp3 * Ixz[0]) - tmp2 * Iyz[0];
}

// uu / vv of the current inner iteration (refine_variational.cpp:189-190,209-222,305-320)

// s of one pixel from (wx, du, wy, dv) of the pixel and its clamped 4-neighbourhood (centre, left, right,
// up, down): the arithmetic of compute_smoothness (opticalflow_aux.c:138-160) on uu = wx + du.
// uu (and vv) of one pixel: wx on the first inner iteration, else wx + du (DE: clamped to the camera side)
template <int NOP>
__device__ __forceinline__ float smooth_uu(const TvArgs &a, bool first, float wx, float du) {
  if (NOP == 2) return first ? wx : wx + du;
  return first ? wx : (a.camlr == 0 ? ssemin(wx + du, 0.0f) : ssemax(wx + du, 0.0f));
}
template <int NOP>
__device__ __forceinline__ float smooth_from_uu(const TvArgs &a, const float (&uu5)[5], const float (&vv5)[5]);
template <int NOP>
__device__ __forceinline__ float smooth_compute(const TvArgs &a, bool first, const float (&wx5)[5],
                                             const float (&du5)[5], const float (&wy5)[5], const float (&dv5)[5]) {
  float uu5[5], vv5[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    uu5[i] = smooth_uu<NOP>(a, first, wx5[i], du5[i]);
    vv5[i] = NOP == 2 ? smooth_uu<2>(a, first, wy5[i], dv5[i]) : 0.0f;
  }
  return smooth_from_uu<NOP>(a, uu5, vv5);
}
// the rest of compute_smoothness from the clamped 5-neighbourhood of uu (centre, left, right, up, down)
template <int NOP>
__device__ __forceinline__ float smooth_from_uu(const TvArgs &a, const float (&uu5)[5], const float (&vv5)[5]) {
  const float uc = uu5[0];
  const float ux = kK3[0] * uu5[1] + (kK3[1] * uc + kK3[2] * uu5[2]);
  const float uy = kK3[0] * uu5[3] + (kK3[1] * uc + kK3[2] * uu5[4]);
  float vx, vy;
  if (NOP == 2) {
    const float vc = vv5[0];
    vx = kK3[0] * vv5[1] + (kK3[1] * vc + kK3[2] * vv5[2]);
    vy = kK3[0] * vv5[3] + (kK3[1] * vc + kK3[2] * vv5[4]);
  } else {  // wy_dummy = 0 (refine_variational.cpp:268,294)
    vx = kK3[0] * 0.0f + (kK3[1] * 0.0f + kK3[2] * 0.0f);
    vy = vx;
  }
  const float eps = 0.001f * 0.001f;
  return a.quarter_alpha / sqrtf(eps + ((ux * ux + uy * uy) + (vx * vx + vy * vy)));
}

// The system of one pixel from its gathered inputs (s, wx, wy of the pixel and its 4-neighbourhood in the
// order centre, left, right, up, down; mask; du, dv; the derivative images).  Neighbours that do not exist
// (hasl ... hasd false) may hold any value: every use of them is behind a select.  OF: c0 = (a11, a12,
// a12, a22) (the inverse sor_coupled's first sweep computes, see below), c1 = (b1, b2, sh, sv); DE: c0 =
// (a11, b1, sh, sv).
template <int NOP>
__device__ __forceinline__ void sys_finish(const TvArgs &a, int x, int y, const float (&S5)[5], const float (&X5)[5],
                                           const float (&Y5)[5], float A11, float A12, float A22, float B1, float B2,
                                           float4 &c0, float4 &c1);
template <int NOP, int NOC>
__device__ __forceinline__ void sys_compute(const TvArgs &a, int x, int y, const float (&S5)[5], const float (&X5)[5],
                                            const float (&Y5)[5], float m, float u, float v, const float (&lIx)[NOC],
                                            const float (&lIy)[NOC], const float (&lIz)[NOC], const float (&lIxx)[NOC],
                                            const float (&lIxy)[NOC], const float (&lIyy)[NOC],
                                            const float (&lIxz)[NOC], const float (&lIyz)[NOC], float4 &c0,
                                            float4 &c1) {
  float A11, A12 = 0.0f, A22 = 0.0f, B1, B2 = 0.0f;
  if (NOP == 2)
    data_of(NOC, 1, u, v, m, lIx, lIy, lIz, lIxx, lIxy, lIyy, lIxz, lIyz, a.hdo3, a.hgo3, A11, A12, A22, B1, B2);
  else
    data_de(NOC, 1, u, m, lIx, lIy, lIz, lIxx, lIxy, lIyy, lIxz, lIyz, a.hdo3, a.hgo3, A11, B1);
  sys_finish<NOP>(a, x, y, S5, X5, Y5, A11, A12, A22, B1, B2, c0, c1);
}

// The rest of the system of one pixel once the data term (A11 .. B2) is known: sub_laplacian on wx / wy, then
// (OF) the 2x2 inverse / (DE) the point-SOR diagonal.  sys_compute runs it right after the data term, in the system
// kernels and in k_tv_level_rb (ofdis_tvrb.hip) alike.
template <int NOP>
__device__ __forceinline__ void sys_finish(const TvArgs &a, int x, int y, const float (&S5)[5], const float (&X5)[5],
                                           const float (&Y5)[5], float A11, float A12, float A22, float B1, float B2,
                                           float4 &c0, float4 &c1) {
  const int w = a.w, h = a.h;
  const bool hasl = x >= 1, hasr = x <= w - 2, hasu = y >= 1, hasd = y <= h - 2;
  const float sc = S5[0], sl = S5[1], sr = S5[2], su = S5[3], sd = S5[4];
  const float xc = X5[0], xl = X5[1], xr = X5[2], xu = X5[3], xd = X5[4];
  const float yc = Y5[0], yl = Y5[1], yr = Y5[2], yu = Y5[3], yd = Y5[4];
  const float shv = x < w - 1 ? sc + sr : 0.0f;  // h[x] = s[x] + s[x+1]
  const float svv = y < h - 1 ? sc + sd : 0.0f;  // v[y] = s[y] + s[y+1]
  // b = ((((b - th[x-1]) + th[x]) - tv[y-1]) + tv[y]) with th[x] = h[x] (wx[x+1] - wx[x]) etc.
  B1 = hasl ? B1 - (sl + sc) * (xc - xl) : B1;
  B1 = hasr ? B1 + shv * (xr - xc) : B1;
  B1 = hasu ? B1 - (su + sc) * (xc - xu) : B1;
  B1 = hasd ? B1 + svv * (xd - xc) : B1;
  if (NOP == 2) {
    B2 = hasl ? B2 - (sl + sc) * (yc - yl) : B2;
    B2 = hasr ? B2 + shv * (yr - yc) : B2;
    B2 = hasu ? B2 - (su + sc) * (yc - yu) : B2;
    B2 = hasd ? B2 + svv * (yd - yc) : B2;
    // sor_coupled's first sweep replaces a11/a12/a22 by the inverse of [[a11+d, a12], [a12, a22+d]] with
    // d = the sum of the four diffusivities (solver.c:122-128, border forms :131-190).  It depends on the
    // system only, so it is computed here, fully parallel, with the same expressions; every SOR sweep then
    // reads the inverse.  (w < 2 or h < 2 run the point-SOR fallback on the raw matrix, solver.c:34-78.)
    if (w >= 2 && h >= 2 && !a.sor_point) {
      const float hl = x > 0 ? sl + sc : 0.0f;  // h[x-1]
      const float vt = su + sc;                  // v[y-1] (y > 0)
      const float dpsis = y == 0 ? hl + (shv + svv) : (y < h - 1 ? (hl + shv) + (vt + svv) : hl + (shv + vt));
      const float M11 = A22 + dpsis, M22 = A11 + dpsis;
      const float det = M11 * M22 - A12 * A12;
      A11 = M11 / det;
      A22 = M22 / det;
      A12 = A12 / (0.0f - det);
    }
    c0 = make_float4(A11, A12, A12, A22);  // (a11, a12) and (a12, a22) pair up for packed fp32
    c1 = make_float4(B1, B2, shv, svv);
  } else {
    // the DE point SOR's diagonal a11 + (the four diffusivities of the pixel's existing neighbours), summed in
    // its order (top, left, bottom, right; solver.c's DE branch) -- it depends on the system only, so it is
    // computed here once instead of in every sweep (the SOR kernels read A = c0.x); vt / hl are the upper /
    // left pixel's sv / sh with the same operands, and sv / sh of a missing bottom / right neighbour are 0
    float dsum = 0.0f;
    if (y > 0) dsum = dsum + (su + sc);
    if (x > 0) dsum = dsum + (sl + sc);
    if (y < h - 1) dsum = dsum + svv;
    if (x < w - 1) dsum = dsum + shv;
    c0 = make_float4(A11 + dsum, B1, shv, svv);
    c1 = c0;
  }
}

// Lane i <- lane i-1 (wave_shr:1) / lane i+1 (wave_shl:1).  bound_ctrl: the lane without a source reads 0
// (its value is never used: border selects / cross-wave LDS values replace it), so no "old" register.
__device__ __forceinline__ float dpp_from_prev_lane(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x138, 0xF, 0xF, true));
}
__device__ __forceinline__ float dpp_from_next_lane(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x130, 0xF, 0xF, true));
}

// The three border variants of solver.c's block-SOR right-hand side as ONE branch-free expression tree.
// The reference evaluates (first row / last row / interior, solver.c:131-190 and :241-300)
//   top:      s = (b + X) + Z
//   bottom:   s = (b + X) + Y
//   interior: s = (X + Y) + (b + Z)
// with X = hr*u_right, Y = vt*u_top, Z = vv*u_bottom.  Selecting operands (and -0.0f, the exact additive
// identity of IEEE round-to-nearest: -0 + x == x bit-for-bit, x = +-0 included) reproduces every variant
// exactly, so a wave never splits into per-lane branches.
__device__ __forceinline__ float sor_rhs(bool border, bool notop, float b, float X, float Y, float Z) {
  const float l = X + (border ? b : Y);
  const float r = (border ? -0.0f : b) + (border ? (notop ? Z : Y) : Z);
  return l + r;
}

typedef float f2v __attribute__((ext_vector_type(2)));

// ---- red-black SOR (opt-in, sor_mode = 1): per-pixel coefficients and update (k_tv_sor_rb, k_tv_level_rb)
struct RbPix {
  float i11, i12, i22, b1, b2, hr, hl, vb, vt;
};
// One pixel's update from its four neighbours' current values (l, r, t, b; OF: u and v).
template <int MODE>
__device__ __forceinline__ void rb_update(const RbPix &d, int x, int y, int w, int h, float omega, float ul,
                                          float ur, float ut, float ub, float vl, float vr, float vt, float vb,
                                          float &u, float &v) {
  const bool border = y == 0 || y >= h - 1, notop = y == 0;
  ur = x < w - 1 ? ur : 0.0f;
  vr = x < w - 1 ? vr : 0.0f;
  if (MODE == 0) {
    const float s1 = sor_rhs(border, notop, d.b1, d.hr * ur, d.vt * ut, d.vb * ub);
    const float s2 = sor_rhs(border, notop, d.b2, d.hr * vr, d.vt * vt, d.vb * vb);
    const float B1 = x > 0 ? d.hl * ul + s1 : s1;
    const float B2 = x > 0 ? d.hl * vl + s2 : s2;
    const float nu = u + omega * (d.i11 * B1 + d.i12 * B2 - u);
    v = v + omega * (d.i12 * B1 + d.i22 * B2 - v);
    u = nu;
  } else {
    float su = 0.0f;  // (i11 = a11 + the diffusivities: sys_compute)
    if (y > 0) { su = su - d.vt * ut; }
    if (x > 0) { su = su - d.hl * ul; }
    if (y < h - 1) { su = su - d.vb * ub; }
    if (x < w - 1) { su = su - d.hr * ur; }
    const float A = d.i11, Bv = d.b1 - su;
    u = (1.0f - omega) * u + omega * (Bv / A);
  }
}

// The colour-split entry layout of the fused red-black level launch (TvArgs::lat, ofdis_tvrb.hip): pixel p = y w + x
// of colour (x + y) & 1 is entry p >> 1 of its colour, stored at colour * E + (p >> 1) with E = ceil(w h / 2).
__host__ __device__ __forceinline__ int lat_entries(int w, int h) { return (w * h + 1) >> 1; }
__device__ __forceinline__ int lat_idx(int x, int y, int w, int E) {
  const int p = y * w + x;
  return ((x + y) & 1) * E + (p >> 1);
}

// image_warp (opticalflow_aux.c:31-75) + the t / It inputs of get_derivatives (:77-132) for pixel (x, y), channel ch.
// The same for channel ch alone: t, It of that channel, the flow (tv_prep_values' expressions: same bits).
__device__ __forceinline__ void tv_prep_values_ch(const TvArgs &a, int x, int y, int f, int ch, float &t, float &it,
                                                  float &wx, float &wy) {
  const long plane = (long)a.w * a.h;
  const long o = (long)y * a.w + x;
  wx = a.flow[(long)f * a.nop * plane + o];
  wy = a.nop == 2 ? a.flow[(long)f * a.nop * plane + plane + o] : 0.0f;
  const float xx = (float)x + wx, yy = (float)y + wy;
  const int xi = (int)floorf(xx), yi = (int)floorf(yy);
  const float dx = xx - (float)xi, dy = yy - (float)yi;
  const int x1 = clampi(xi, 0, a.w - 1), x2 = clampi(xi + 1, 0, a.w - 1);
  const int y1 = clampi(yi, 0, a.h - 1), y2 = clampi(yi + 1, 0, a.h - 1);
  const long fs = (long)a.W * (a.h + 2 * a.pad) * a.noc;
  const float *B = a.img_b + f * fs, *A = a.img_a + f * fs;
#define SB(xq, yq) B[((long)((yq) + a.pad) * a.W + (xq) + a.pad) * a.noc + ch]
  const float w2 = SB(x1, y1) * (1.0f - dx) * (1.0f - dy) + SB(x2, y1) * dx * (1.0f - dy) +
                   SB(x1, y2) * (1.0f - dx) * dy + SB(x2, y2) * dx * dy;
#undef SB
  const float i1 = A[((long)(y + a.pad) * a.W + x + a.pad) * a.noc + ch];
  t = 0.5f * (w2 + i1);
  it = w2 - i1;
}
// Every channel of pixel (x, y) at once: the flow, the warp position and the bilinear weights once (they do not
// depend on the channel), then each channel's taps -- adjacent in the interleaved image, so one set of cache lines.
// Per channel the expressions of tv_prep_values_ch: same bits.
template <int NOC>
__device__ __forceinline__ void tv_prep_values_all(const TvArgs &a, int x, int y, int f, float (&t)[NOC],
                                                   float (&it)[NOC], float &wx, float &wy) {
  const long plane = (long)a.w * a.h;
  const long o = (long)y * a.w + x;
  wx = a.flow[(long)f * a.nop * plane + o];
  wy = a.nop == 2 ? a.flow[(long)f * a.nop * plane + plane + o] : 0.0f;
  const float xx = (float)x + wx, yy = (float)y + wy;
  const int xi = (int)floorf(xx), yi = (int)floorf(yy);
  const float dx = xx - (float)xi, dy = yy - (float)yi;
  const int x1 = clampi(xi, 0, a.w - 1), x2 = clampi(xi + 1, 0, a.w - 1);
  const int y1 = clampi(yi, 0, a.h - 1), y2 = clampi(yi + 1, 0, a.h - 1);
  const long fs = (long)a.W * (a.h + 2 * a.pad) * NOC;
  const float *B = a.img_b + f * fs, *A = a.img_a + f * fs;
  const float *b11 = B + ((long)(y1 + a.pad) * a.W + x1 + a.pad) * NOC, *b21 = B + ((long)(y1 + a.pad) * a.W + x2 + a.pad) * NOC;
  const float *b12 = B + ((long)(y2 + a.pad) * a.W + x1 + a.pad) * NOC, *b22 = B + ((long)(y2 + a.pad) * a.W + x2 + a.pad) * NOC;
  const float *a1 = A + ((long)(y + a.pad) * a.W + x + a.pad) * NOC;
#pragma unroll
  for (int ch = 0; ch < NOC; ++ch) {
    const float w2 = b11[ch] * (1.0f - dx) * (1.0f - dy) + b21[ch] * dx * (1.0f - dy) + b12[ch] * (1.0f - dx) * dy +
                     b22[ch] * dx * dy;
    const float i1 = a1[ch];
    t[ch] = 0.5f * (w2 + i1);
    it[ch] = w2 - i1;
  }
}

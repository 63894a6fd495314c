// ofdis_internal.h -- kernel argument blocks and launchers shared by ofdis_kernels.hip and the runtime.
//
// Device data layout (per batch of n frame pairs, all float32 unless noted):
//   pyramid level s   : [2n][H_s][W_s][noc]  padded by `pad` (W_s = w_s + 2 pad); frames 0..n-1 are
//                       image a, n..2n-1 image b (same layout as OFClass's inputs, oflow.h:99-106).
//                       A sequence call holds [n + stride] frames instead: pair f is (frame f, frame f + stride)
//   patch state       : p_iter [n][npatch][nop], pweight [n][npatch][novals]
//   flow level s      : planar [n][nop][h_s][w_s]  (wx, wy)
//   TV scratch        : planar [n][plane][h][w] for du, dv, mask, a11, a12, a22, b1, b2, sh, sv,
//                       t/dt, and the 8 derivative images (noc planes each)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ofdis {

struct LevelGeom {
  int w, h;        // unpadded level size
  int pad;         // imgpadding
  int W, H;        // padded size
  int nopw, noph, npatch, offw, offh;
  float tmp_lb, tmp_ubw, tmp_ubh;
  int level;       // scale index s
};

// The pyramid kernels build nf frames: frames 0..n-1 come from img_a, n..nf-1 from img_b.  Pairs: nf = 2n.
// A sequence (ofdis_run_sequence_u8): one array of nf = pairs + stride frames, n = nf, img_b unread.
struct PyrBaseArgs {
  const uint8_t *img_a, *img_b;  // [n][H0][W0][noc], [nf - n][H0][W0][noc]
  int n, nf, W0, H0, noc;
  int padl, padt;                // divisibility padding offsets (floor halves)
  int log2s;                     // level of the output (sc_l)
  int w, h;                      // output level size
  float *out;                    // unpadded level [nf][h][w][noc]
  int rgb_sad;                  // colour, 2^l = 4..16: k_pyr_base_rgb (option pyr_rgb)
  int stereo;                    // ofdis_run_stereo_u8: n stereo pairs (img_a left, img_b right), nf = 4n frames --
                                 // left, mirrored right, right, mirrored left, n of each; the mirrored frames are read
                                 // from img_b / img_a through a mirrored column index
};

// SELECTCHANNEL 2 (run_dense.cpp:139-148): level 0 = Sobel gradient magnitude of the divisibility-padded
// intensity frame, sqrt(dx*dx + dy*dy) (exact up to the correctly rounded sqrt: dx, dy are multiples of
// 1/8 below 2^10, their squares and sum exact in fp32).
struct PyrGradmagArgs {
  const uint8_t *img_a, *img_b;  // [n][H0][W0], [nf - n][H0][W0] (as PyrBaseArgs)
  int n, nf, W0, H0, padl, padt, Wp, Hp;
  float *out;                    // [nf][Hp][Wp]
  int stereo;                    // as PyrBaseArgs::stereo
};

struct PyrDownArgs {
  const float *src;  // [2n][2h][2w][noc]
  float *dst;        // [2n][h][w][noc]
  int n2, w, h, noc;
};

struct PyrPadGradArgs {
  const float *lvl;        // unpadded [2n][h][w][noc]
  float *img, *dx, *dy;    // padded [2n][H][W][noc]
  int n2, w, h, noc, pad;
  int per_value;           // colour: one thread per value (k_pyr_pad_grad_v; option pad_grad_v)
};

struct PatchArgs {
  const float *img_a, *dx_a, *dy_a, *img_b;  // padded level, frame stride = W*H*noc
  const float *prev;                          // coarse flow or NULL
  long prev_frame_stride;                     // floats per frame
  int prev_comp_stride, prev_elem_stride, prev_w;
  float *p_iter;                              // [n][npatch][nop]
  float *pweight;                             // [n][npatch][novals]
  int n, nop, noc, p, novals, steps;
  int costfct, patnorm, max_iter, min_iter;
  float dp_thresh_sq, dr_thresh, res_thresh, outlierthresh;
  float outlier_sq;                           // largest s with sqrt_rn(s) <= outlierthresh: the outlier test
                                              // sqrt(ex^2 + ey^2) > thresh (patch.cpp:197) without the sqrt
  int camlr;
  int wave_per_patch;                         // 1: force the one-wave-per-patch kernel (A/B testing)
  int generic;                                // 1: force the any-shape kernel k_patchg (parity testing)
  int window;                                 // LDS-windowed bilinear taps (k_patchw) where the shape has one
  int quad;                                   // four lanes per patch (k_patchq) where the shape has that form
  int x16;                                    // sixteen lanes per patch (k_patchx) for RGB p = 12 (2: exact evaluations)
  int absw;                                   // 1: write the aggregation weight of every patch pixel into the slot
                                              // planes (agg_plane_off) instead of the loss weights, where the kernel
                                              // can (launch_patch returns whether it did)
  int aslots;                                 // A = (p - 1) / steps + 1: slot planes per axis
  int buf32;                                  // the image array of the launch spans < 2^32 bytes (32-bit buffer offsets)
  int fdiv;                                   // 1: the LLT solves divide by FMA-corrected pivot reciprocals (llt_rcp)
  int maxres;                                 // 1: res_thresh = 0 and min_iter >= max_iter: the four- and sixteen-lane
                                              // kernels test the largest |w| > 0 instead of mean |w| > res_thresh
  int stage;                                  // 0 the whole patch optimisation; timing diagnostics (verbosity 2):
                                              // 1 construction only (pconst), 2 + initialisation (pinit)
  LevelGeom g;
};

struct AggArgs {
  const float *p_iter, *pweight;
  const float *cg_p_iter, *cg_pweight;  // complementary (backward) grid for usefbcon, or NULL
  float *flow;  // planar [n][nop][h][w]
  int n, nop, noc, p, novals, steps;
  int absw;     // 1: pweight holds the patch kernel's aggregation weights as slot planes ([n][A * A][h][w]), 0: loss weights
  int aslots;   // A
  int stage;    // k_aggregate: the tile's patch displacements staged in LDS (option agg_stage)
  LevelGeom g;
};

// TV arrays use a SKEWED (anti-diagonal-major) layout: pixel (x, y) of a w x h level lives at
// (x + y) * h + y of a plane of sp = (w + h - 1) * h floats, so the pixels of one wavefront step
// t = x + y are contiguous (lane = row y).  Both the stencil kernels (neighbours at +-h, +-(h+1)) and the
// exact-order SOR wavefront read it fully coalesced.
struct TvArgs {
  // level images (padded interleaved) and flow
  const float *img_a, *img_b;
  float *flow;                 // planar row-major [n][nop][h][w]  (wx, wy)
  float *wxs, *wys;            // skewed copies of the flow at the start of the level [n][sp]
  float *du, *dv, *mask, *s;   // skewed [n][sp]
  float *coef;                 // AoS per pixel: OF (a11,a12,a22,b1)(b2,sh,sv,-) = 8 floats; DE (a11,b1,sh,sv)
  float *t, *dt;               // skewed [n][noc][sp]
  float *Ix, *Iy, *Iz, *Ixx, *Ixy, *Iyy, *Ixz, *Iyz;  // skewed [n][noc][sp]
  long sp;                     // skewed plane stride: skew_slots + 64 dump slots (SOR), multiple of 4
  int wrap;                    // rows folded modulo w (h <= w): skew_slots = w * h, else (w + h - 1) * h
  int skew_slots;
  int n, nop, noc, w, h, pad, W;
  float quarter_alpha, hdo3, hgo3, omega;
  int first_iter;              // uu = wx (memcpy) on the first inner iteration
  int solverit;
  int camlr;
  int sor_generic;             // force the generic global-memory SOR wavefront (A/B testing)
  int sor_variant;             // 0 auto (sweep-per-wave when it fits), 1 register pipeline (A/B testing)
  int sor_point;               // OpenMP build: point SOR on the raw system (solver.c:34-78) for every size
  int sor_cring;               // lean SOR: coefficients loaded once by sweep 0, passed on through LDS (S <= 3);
                               // 2: the ring sized to the level's row groups
  int sor_pack;                // lean SOR: rows of several frames end to end in one workgroup (sor_pack_frames);
                               // 1: in launches with more frames than CUs, 2: in every launch
  int sor_rows2;               // lean SOR with two rows per lane for levels of 321..640 rows (else the pipeline)
  int smsys;                   // smoothness + system in one launch (k_tv_smsys)
  int prepd;                   // prep + derivatives in one launch (k_tv_prepd, intensity images; 0: three launches)
  int smsys2d;                 // ... and on 2-D tiles for tall levels (k_tv_smsys2d; 0: two launches there, A/B)
  int smsys_prefetch;          // k_tv_smsys, intensity images: derivative images loaded before the staging
  int smsys_small;             // k_tv_smsys: ~1 pixel per thread when a launch cannot fill the chip
  int smsys_march;             // tall levels: the register march k_tv_smsys_m (takes precedence over smsys2d)
  int smsys_deriv;             // row-block k_tv_smsys, intensity images: Ixx .. Iyz computed from staged Ix, Iy, Iz
  int prepd_df;                // smsys_deriv levels: the prep launch warps on a 2-pixel halo, all channels at once (k_tv_prepd_df)
                               // (k_tv_prepd then writes only Ix, Iy, Iz of the derivative planes); set by the
                               // runtime only where tv_deriv_fused() holds
  int sor_redblack;            // opt-in red-black SOR order (a different iteration: EPE-gated, not bit-exact)
  int lat;                     // sor_mode = 1 latency form (tv_level_rb_ok): k_tv_prepd writes the flow copies and
                               // the eight derivative planes in the colour-split entry layout (lat_idx) that
                               // k_tv_level_rb reads
};

struct UpArgs {
  const float *flow;  // planar [n][nop][hl][wl]
  float *out;         // [n][H0][W0][nop]
  int n, nop, wl, hl, log2s, W0, H0, offx, offy;
  int nt_store;       // non-temporal output stores (A/B option "nt_store")
  int form;           // nop = 2: 0 k_upsample_rows, 1 k_upsample_h<4>, 2 k_upsample_h<8> (option "up_form")
  int f16, planar;    // output format (ofdis_out_format): `out` holds binary16 values / is [n][nop][H0][W0].  Either set:
                      // one store form per nop whatever `form` (k_upsample_h<4>, k_upsample_rows1, k_upsample)
  float *out_r;       // ofdis_run_stereo_u8 (nop = 1, the plain format), else NULL: frames 0 .. n_l - 1 go to `out`; frame
  int n_l;            // n_l + i is the mirrored view of pair i and goes to out_r[i], its column x stored at W0 - 1 - x
                      // with the sign bit flipped -- the right view's disparity in the right view's coordinates
};

// The finest level's flow x 2^sc_l in an output format, no upsample (ofdis_out_format, OFDIS_OUT_LEVEL).
struct LevelOutArgs {
  const float *flow;  // planar [n][nop][hl][wl]
  void *out;          // float or binary16, [n][hl][wl][nop] or [n][nop][hl][wl]
  int n, nop, wl, hl, log2s;
  int f16, planar;
};

// Initial flow (run_dense.cpp:356-379): full-resolution [n][H0][W0][nop] -> replicate-padded, x sc,
// INTER_AREA by k = 2^(sc_f+1) -> [n][ho][wo][nop] interleaved (OFClass's initflow layout).
struct InitArgs {
  const float *init;  // [n][H0][W0][nop]
  float *out;         // [n][ho][wo][nop]
  int n, nop, W0, H0, padl, padt, log2k, wo, ho;
  float sc, scale;    // 2^-(sc_f+1), 1 / k^2
};

// Forward-backward consistency of two full-resolution flow fields (include/ofdis.h: ofdis_fb_check).
struct FbArgs {
  const float *fw, *bw;      // [n][H][W][2]
  uint8_t *occ_fw, *occ_bw;  // [n][H][W] mask codes 0 / 1 / 2, or NULL
  float *err_fw, *err_bw;    // [n][H][W] squared round-trip error, or NULL
  int n, W, H;               // W * H < 2^31
  float alpha, beta;
};

// Forward-backward consistency of two float32 interleaved level grids of one geometry, as if on the fields they
// expand to (include/ofdis.h: ofdis_fb_check_level).
struct FbLevelArgs {
  const float *gfw, *gbw;    // [n][gh][gw][2]
  uint8_t *occ_fw, *occ_bw;  // [n][H][W] mask codes 0 / 1 / 2, or NULL
  float *err_fw, *err_bw;    // [n][H][W] squared round-trip error, or NULL
  int n, W, H;               // W * H < 2^31
  float alpha, beta;
  int gw, gh, log2c, offx, offy;  // as WarpArgs
};

// Left-right consistency of two full-resolution disparity fields (include/ofdis.h: ofdis_lr_check).
struct LrArgs {
  const float *dl, *dr;    // [n][H][W]
  uint8_t *occ_l, *occ_r;  // [n][H][W] mask codes 0 / 1 / 2, or NULL
  float *err_l, *err_r;    // [n][H][W] squared round-trip error, or NULL
  int n, W, H;             // W * H < 2^31
  float alpha, beta;
};

// Backward warp of u8 frames along a flow view (include/ofdis.h: ofdis_warp_u8).
struct WarpArgs {
  const uint8_t *img;  // [n][H][W][noc]
  const void *flow;    // full grid: [n][H][W][2] or [n][2][H][W]; level grid: [n][gh][gw][2] or [n][2][gh][gw]
  void *out;           // u8 or float [n][H][W][noc]
  uint8_t *valid;      // [n][H][W] 1 / 0, or NULL
  int n, W, H, noc;    // W * H < 2^31
  float scale;
  int out_f32;             // `out` holds float32 values
  int f16, planar, level;  // the flow view (ofdis_out_format's dtype, layout, grid)
  int gw, gh, log2c, offx, offy;  // level grid: its size, log2 of the cell, the frame's offset in it (ofdis_out_geometry)
};

// The frame between two frames at nt times (include/ofdis.h: ofdis_interp_u8).  One view describes both flows.
constexpr int kInterpMaxT = 16;  // OFDIS_INTERP_MAX_T
struct InterpArgs {
  const uint8_t *img_a, *img_b;      // [n][H][W][noc]
  const void *flow_fw, *flow_bw;     // a -> b on a's grid, b -> a on b's grid; the layouts of WarpArgs::flow
  const uint8_t *occ_a, *occ_b;      // [n][H][W] occlusion masks of the two frames, or NULL
  void *out;                         // u8 or float [n][nt][H][W][noc]
  uint8_t *valid;                    // [n][nt][H][W] bit 0: frame a used, bit 1: frame b used; or NULL
  int n, W, H, noc;                  // W * H < 2^31
  int out_f32;
  int f16, planar, level;
  int gw, gh, log2c, offx, offy;
  int srows, scols;                  // level form: rows and columns of a staged window (set by launch_interp)
  int nt;
  float t[kInterpMaxT];
};

// Points followed along a chain of m flow fields (include/ofdis.h: ofdis_track_points).  One view describes both chains.
struct TrackArgs {
  const void *fw, *bw;   // m fields back to back in the layouts of WarpArgs::flow; bw NULL: no consistency check
  const float *points;   // [npts][2]
  const int32_t *start;  // [npts] or NULL
  float *tracks;         // [m + 1][npts][2] ([npts][2] with last), or NULL
  uint8_t *status;       // [m + 1][npts] ([npts] with last), or NULL
  int m, npts, W, H;     // W * H < 2^31
  float alpha, beta;
  int last;              // OFDIS_TRACK_LAST: only entry m is written
  int f16, planar, level;
  int gw, gh, log2c, offx, offy;  // as WarpArgs
};

// Every frame of a video averaged with its two motion-compensated neighbours (include/ofdis.h: ofdis_tfilter_u8).
// One view describes both chains of m = T - 1 fields.
struct TfilterArgs {
  const uint8_t *frames;         // [T][H][W][noc]
  const void *fw, *bw;           // m fields back to back in the layouts of WarpArgs::flow
  const uint8_t *occ_fw, *occ_bw;  // [m][H][W] occlusion masks, or NULL
  void *out;                     // u8 or float [T][H][W][noc]
  uint8_t *used;                 // [T][H][W] bit 0: the previous frame used, bit 1: the next; or NULL
  int T, W, H, noc;              // W * H < 2^31
  int f0, n;                     // the launch's output frames f0 .. f0 + n - 1 (set by launch_tfilter)
  float inv;                     // 1 / (sigma noc)
  int out_f32;
  int f16, planar, level;
  int gw, gh, log2c, offx, offy;  // as WarpArgs
  int srows, scols;              // level form: rows and columns of a staged window (set by launch_tfilter)
};

// Every frame averaged with up to `radius` motion-compensated frames on each side, the positions chained through the
// fields and checked step by step (include/ofdis.h: ofdis_tfilter_radius_u8).
struct TfilterRadiusArgs {
  TfilterArgs f;      // the frames, chains, outputs and view; occ_fw / occ_bw stay NULL; `used` holds 2 * radius bits
  int radius;         // 1 .. 4
  int use_fb;         // every step runs the tracker's round-trip test at alpha, beta
  float alpha, beta;
};

// A robust similarity or translation fitted to each of m flow fields (include/ofdis.h: ofdis_fit_motion).  One view
// describes both chains.
constexpr int kFitLanes = 256;         // OFDIS_FIT_LANES: one workgroup per pair, the pinned summation order
constexpr int kFitMaxSamples = 65536;  // OFDIS_FIT_MAX_SAMPLES
constexpr int kFitMaxIters = 16;
struct FitArgs {
  const void *fw, *bw;   // m fields back to back in the layouts of WarpArgs::flow; bw NULL: no consistency check
  double *xform;         // [m][6]
  int32_t *support;      // [m] or NULL
  float *weights;        // [m][ns] or NULL
  int m, W, H;           // W * H < 2^31
  int similarity;        // OFDIS_MOTION_SIMILARITY (else a translation)
  int step, half, sx, sy, ns;  // the lattice: columns half + i * step, i < sx; rows likewise; ns = sx * sy
  int iters;
  double inv[kFitMaxIters + 1];  // inv[it] = 1 / t_it^2 of solve it = 1 .. iters (the host's divisions)
  float alpha, beta;
  int f16, planar, level;
  int gw, gh, log2c, offx, offy;  // as WarpArgs
};

// Pair transforms to per-frame corrections (include/ofdis.h: ofdis_smooth_path).
struct PathArgs {
  const double *xform;  // [m][6]
  double *corr;         // [m + 1][6]
  double *chain;        // [m + 1][6] scratch: the cumulative transforms C_i
  int m, radius, W, H;
  double z;             // 1 / zoom (the host's division)
};

// Each of n u8 frames pulled through its own 2 x 3 transform (include/ofdis.h: ofdis_warp_affine_u8).
struct WarpAffineArgs {
  const uint8_t *img;  // [n][H][W][noc]
  const double *xf;    // [n][6], device
  void *out;           // u8 or float [n][H][W][noc]
  uint8_t *valid;      // [n][H][W] 1 / 0, or NULL
  int n, W, H, noc;    // W * H < 2^31
  int out_f32;
};

// n flow fields scored against ground truth (include/ofdis.h: ofdis_flow_error).  The row kernel leaves one FeRow per
// frame row in `rows`; launch_flow_error_sum folds them into the 16 numbers per pair.
constexpr int kFeLanes = 64;   // OFDIS_FE_LANES: one wave per row, the pinned summation order
constexpr int kFeStats = 16;   // OFDIS_FE_NSTATS
constexpr int kFeBins = 1024;  // OFDIS_FE_BINS
struct FeRow {
  double sum[4];    // the row's tree sums: Se and the three speed classes' sums
  uint32_t cnt[9];  // cnt, nonfinite, e > 1, e > 3, e > 5, fl, and the three speed classes' counts
  float emax;
  uint32_t pad[2];
};
static_assert(sizeof(FeRow) == 80, "the byte model and the workspace size count 80 bytes per row");
struct FlowErrorArgs {
  const void *flow;     // n fields back to back in the layouts of WarpArgs::flow
  const float *gt;      // [n][H][W][2]
  const uint8_t *mask;  // [n][H][W] or NULL
  int mask_eq;          // < 0: nonzero bytes pass, else the bytes equal to it
  FeRow *rows;          // [n][H]
  double *stats;        // [n][16]
  float *err;           // [n][H][W] or NULL
  uint32_t *hist;       // [n][1024] or NULL, zeroed before the row kernel
  int n, W, H;          // W * H < 2^31
  int f16, planar, level;
  int gw, gh, log2c, offx, offy;  // as WarpArgs
};

// m flow fields classified against the camera's motion (include/ofdis.h: ofdis_motion_mask).  A workgroup owns a
// kMmTileW x kMmTileH tile of pixels and classifies it with a halo of `radius`.
constexpr int kMmStats = 12;     // OFDIS_MM_NSTATS
constexpr int kMmMaxRadius = 4;  // the halo the tile's LDS planes are sized for
constexpr int kMmTileW = 64, kMmTileH = 16;
struct MotionMaskArgs {
  const void *flow;     // m fields back to back in the layouts of WarpArgs::flow
  const double *xform;  // [m][6]
  const uint8_t *occ;   // [m][H][W] or NULL
  uint8_t *code;        // [m][H][W] or NULL
  float *res;           // [m][H][W] or NULL
  int64_t *stats;       // [m][12] or NULL, reset before the mask kernel
  int m, W, H;          // W * H < 2^31
  float thr, rel;
  int radius;           // 0 .. kMmMaxRadius
  int f16, planar, level;
  int gw, gh, log2c, offx, offy;  // as WarpArgs
};

void launch_warp(const WarpArgs &a, hipStream_t s);
void launch_motion_mask(const MotionMaskArgs &a, hipStream_t s);
void launch_flow_error(const FlowErrorArgs &a, hipStream_t s);
void launch_flow_error_sum(const FlowErrorArgs &a, hipStream_t s);
void launch_fit_motion(const FitArgs &a, hipStream_t s);
void launch_smooth_path(const PathArgs &a, hipStream_t s);
void launch_warp_affine(const WarpAffineArgs &a, hipStream_t s);
void launch_track(const TrackArgs &a, hipStream_t s);
void launch_tfilter(const TfilterArgs &a, hipStream_t s);
void launch_tfilter_radius(const TfilterRadiusArgs &a, hipStream_t s);
void launch_interp(const InterpArgs &a, hipStream_t s);
void launch_fb_check(const FbArgs &a, hipStream_t s);
void launch_fb_check_level(const FbLevelArgs &a, hipStream_t s);
void launch_lr_check(const LrArgs &a, hipStream_t s);
void launch_init_area(const InitArgs &a, hipStream_t s);
void warm_kernels_module(hipStream_t s);  // one empty launch per kernel translation unit: loads its code object
void warm_tvrb_module(hipStream_t s);
void launch_pyr_base(const PyrBaseArgs &a, hipStream_t s);
void launch_pyr_gradmag(const PyrGradmagArgs &a, hipStream_t s);
void launch_pyr_down(const PyrDownArgs &a, hipStream_t s);
void launch_pyr_pad_grad(const PyrPadGradArgs &a, hipStream_t s);
bool launch_patch(const PatchArgs &a, hipStream_t s);  // true: wrote aggregation weights (PatchArgs::absw)
void launch_aggregate(const AggArgs &a, hipStream_t s);
void launch_tv_prep(const TvArgs &a, hipStream_t s);
void launch_tv_deriv1(const TvArgs &a, hipStream_t s);
void launch_tv_deriv2(const TvArgs &a, hipStream_t s);
bool tv_prepd_ok(const TvArgs &a);
void launch_tv_prepd(const TvArgs &a, hipStream_t s);
void launch_tv_smooth(const TvArgs &a, hipStream_t s);
void launch_tv_system(const TvArgs &a, hipStream_t s);
bool tv_smsys_ok(const TvArgs &a);
bool tv_deriv_fused(const TvArgs &a);  // the level's derivative filters can move into k_tv_smsys (smsys_deriv)
void launch_tv_smsys(const TvArgs &a, hipStream_t s);
void launch_tv_sor(const TvArgs &a, hipStream_t s);
bool tv_level_rb_ok(const TvArgs &a);  // ofdis_tvrb.hip
void launch_tv_level_rb(const TvArgs &a, int n_inner, hipStream_t s);
void launch_tv_final(const TvArgs &a, hipStream_t s);
void launch_upsample(const UpArgs &a, hipStream_t s);
void launch_level_out(const LevelOutArgs &a, hipStream_t s);

}  // namespace ofdis

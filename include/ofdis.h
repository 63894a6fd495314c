/*
 * ofdis.h -- C-ABI of the MI355X-native DIS optical-flow / stereo-depth hot path.
 *
 * This is the drop-in boundary for lordnn/OF_DIS.  Every entry point below names the
 * reference interface it replaces (paths relative to the reference tree).  Plain C types
 * only: no torch, no HIP types in any signature (device pointers and streams are void*).
 *
 * Library: of_dis_amd/libofdis.so (built by of_dis_amd/csrc/Makefile, hipcc --offload-arch=gfx950).
 */
#ifndef OFDIS_H
#define OFDIS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFDIS_ABI_VERSION 2

/* Status codes.  The reference has no error channel (it exit(1)s on OOM, FDF1.0.1/image.cpp:26-27,
 * and never validates parameters); every entry point here returns one of these instead. */
typedef enum ofdis_status {
  OFDIS_OK = 0,
  OFDIS_ERR_INVALID_ARGUMENT = 1, /* bad pointer / size / parameter combination          */
  OFDIS_ERR_UNSUPPORTED = 2,      /* valid in the reference but not implemented here       */
  OFDIS_ERR_OUT_OF_MEMORY = 3,    /* device or host allocation failed                      */
  OFDIS_ERR_DEVICE = 4,           /* a HIP runtime call failed                             */
  OFDIS_ERR_NO_DEVICE = 5,        /* no gfx950 device visible                              */
  OFDIS_ERR_IO = 6                /* file could not be opened / read / written             */
} ofdis_status;

/* SELECTMODE of the reference build (CMakeLists.txt:36-61): 1 = optical flow, 2 = stereo depth. */
enum { OFDIS_MODE_OF = 1, OFDIS_MODE_DE = 2 };

/*
 * Parameters of one run.  Mirrors OFC::optparam's explicitly-set fields (oflow.h:45-66) plus
 * the two compile-time switches SELECTMODE / SELECTCHANNEL, which are runtime fields here.
 * Values are taken exactly as the reference constructor receives them (oflow.cpp:80-104):
 * dp_thresh is NOT squared by the caller, steps/outlier threshold/novals are derived.
 */
typedef struct ofdis_params {
  int mode;         /* OFDIS_MODE_OF (nop = 2) or OFDIS_MODE_DE (nop = 1)                 */
  int noc;          /* channels: 1 = intensity, 3 = BGR interleaved (SELECTCHANNEL 1 / 3)  */
  int sc_f;         /* coarsest scale                                                     */
  int sc_l;         /* finest scale                                                       */
  int max_iter;     /* patch iterations                                                   */
  int min_iter;
  float dp_thresh;  /* early-stop on |delta_p| ratio (squared internally, oflow.cpp:87)    */
  float dr_thresh;  /* early-stop on residual ratio                                        */
  float res_thresh; /* early-stop on mean absolute residual                                */
  int p_samp_s;     /* patch edge length (even)                                            */
  float patove;     /* patch overlap in [0,1)                                              */
  int usefbcon;     /* forward-backward merging (patchgrid.cpp:277-375)                    */
  int costfct;      /* 0 L2, 1 L1, 2 pseudo-Huber (10 = NCC is unimplemented upstream)     */
  int patnorm;      /* mean-normalise patches                                              */
  int usetvref;     /* variational refinement                                              */
  float tv_alpha, tv_gamma, tv_delta;
  int tv_innerit;   /* TV outer iterations per level = tv_innerit * (level + 1)            */
  int tv_solverit;  /* SOR sweeps per TV iteration                                         */
  float tv_sor;     /* SOR relaxation omega                                                */
  int verbosity;    /* 0 silent, 1 total time, 2 per-scale TIME lines (oflow.cpp:297,336)  */
  /* Reference build variants (compile-time there, runtime fields here; 0 = the default build): */
  int omp_build;    /* USE_OPENMP build (CMakeLists.txt:4,17-23): optical-flow refinement runs
                       sor_coupled_slow_but_readable, point SOR (refine_variational.cpp:202-203,
                       solver.c:34-78), in its single-thread order (the multi-threaded build races rows) */
  int gradmag;      /* SELECTCHANNEL 2 (run_dense.cpp:139-148, 194-197): the pyramid is built on each
                       frame's Sobel gradient magnitude instead of its intensity (noc must be 1)          */
} ofdis_params;

/* ------------------------------------------------------------------ parameters */

int ofdis_abi_version(void);
const char *ofdis_status_string(int status);

/* AutoFirstScaleSelect (run_dense.cpp:181-184). */
int ofdis_auto_first_scale(int imgwidth, int fratio, int patchsize);

/* Operating points 1-4 with automatic coarsest scale (run_dense.cpp:226-268). */
int ofdis_params_oppoint(ofdis_params *p, int oppoint, int width_org, int mode, int noc);

/* The 20 explicit positional parameters of run_dense.cpp:270-295, as strings (argv[4..23]). */
int ofdis_params_from_strings(ofdis_params *p, int count, const char *const *values, int mode, int noc);

/* Validation the reference never does: p even and >= 2, p*p*noc divisible by 4 (patch.cpp:230),
 * 0 <= sc_l <= sc_f, width/height divisible by 2^sc_f, costfct in {0,1,2}, noc in {1,3}, gradmag only
 * with noc = 1.
 * With usetvref set, OFDIS_ERR_INVALID_ARGUMENT for the TV values under which the refinement is undefined
 * (DESIGN.md section 5): tv_alpha that is not a finite number above 0, tv_gamma or tv_delta that is not a finite
 * number >= 0, a tv_sor that is not finite.  Without a positive smoothness weight and non-negative data weights the
 * 2x2 system of a pixel (solver.c:122-128) has no inverse wherever the warp mask or the image gradients are zero;
 * its 0 / 0 spreads through the level, and the reference then takes (int)ceil(NaN) as a patch position
 * (patch.cpp:345-350).  Zero tv_gamma or tv_delta, any finite tv_sor and zero tv_solverit / tv_innerit are defined.
 * Finite weights so extreme that a system overflows or underflows in float (tv_alpha 1e-25, tv_gamma 1e30) end
 * the same way; that depends on the images, and they are not refused. */
int ofdis_params_validate(const ofdis_params *p, int width, int height, int imgpadding);

/* ------------------------------------------------------------------ library boundary */

/*
 * OFC::OFClass::OFClass (oflow.h:99-126, oflow.cpp:31-338) with host pointers.
 * im_ao[s] .. im_bo_dy[s] for s in [sc_l, sc_f]: padded (w_s + 2*imgpadding) x (h_s + 2*imgpadding)
 * x noc float arrays (images replicate-padded, gradients zero-padded); entries below sc_l may be NULL.
 * outflow: (width >> sc_l) * (height >> sc_l) * nop floats, interleaved.  initflow: NULL or
 * (width >> (sc_f+1)) * (height >> (sc_f+1)) * nop floats.  Runs on the default device; blocking.
 */
int ofdis_oflow_compute(const float *const *im_ao, const float *const *im_ao_dx, const float *const *im_ao_dy,
                        const float *const *im_bo, const float *const *im_bo_dx, const float *const *im_bo_dy,
                        int imgpadding, float *outflow, const float *initflow, int width, int height,
                        const ofdis_params *p);

/* ------------------------------------------------------------------ batched device path */

typedef struct ofdis_context ofdis_context;

/* One context per GPU (and per host thread using it).  No hidden globals. */
int ofdis_context_create(int device, ofdis_context **out);
void ofdis_context_destroy(ofdis_context *ctx);

/*
 * Whole run_dense.cpp main() hot path for a batch of n independent frame pairs, all on device:
 * divisibility padding (run_dense.cpp:299-312) -> pyramid + Sobel gradients (:131-179) ->
 * OFClass (:392-401) -> x 2^sc_l + INTER_LINEAR upsample + crop (:407-415).
 * img_a/img_b: device u8 [n][height][width][noc] (BGR order when noc = 3).
 * flow_out: device float [n][height][width][nop] (nop = 2 OF, 1 DE).
 * stream: hipStream_t, or NULL for the legacy default stream (torch's default): the call is then ordered
 * after the work already queued there and that stream's later work after the call.  Asynchronous w.r.t. the
 * host.  All calls on one context share its workspaces: a call waits for the previous call of the context
 * whatever stream either was issued on.  A batch is split into launches of at most
 * ofdis_max_frames_per_launch() frames.  n < 1, a non-positive size or a NULL image / flow pointer returns
 * OFDIS_ERR_INVALID_ARGUMENT before anything is enqueued (the context stays usable).
 */
int ofdis_run_batch_u8(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, int n, int width,
                       int height, const ofdis_params *p, float *flow_out, void *stream);

/* Same with host buffers (CLI path; synchronous). */
int ofdis_run_batch_u8_host(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, int n, int width,
                            int height, const ofdis_params *p, float *flow_out);

/* The same with an initial flow per pair (OFClass's initflow, oflow.h:106 / oflow.cpp:215-217, fed the way
 * run_dense.cpp's commented-out code prepares it, :293-294, :302, :356-379): init_flow is device float
 * [n][height][width][nop] at full resolution, or NULL (= ofdis_run_batch_u8).  With an initial flow the
 * frames are padded to a multiple of 2^(sc_f+1) and the flow is replicate-padded, scaled by 2^-(sc_f+1)
 * and INTER_AREA-reduced to the grid below the coarsest scale -- e.g. the previous frame's output for
 * video (temporal propagation). */
int ofdis_run_batch_u8_init(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, const float *init_flow,
                            int n, int width, int height, const ofdis_params *p, float *flow_out, void *stream);
int ofdis_run_batch_u8_init_host(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b,
                                 const float *init_flow, int n, int width, int height, const ofdis_params *p,
                                 float *flow_out);

/* ------------------------------------------------------------------ both directions and occlusion masks
 *
 * Not in the reference, which gives one field per pair and nothing that says where it can be trusted.  The
 * forward-backward consistency check (Sundaram, Brox, Keutzer, ECCV 2010) follows each pixel along its flow,
 * reads the opposite field there and asks whether the two cancel.
 *
 * ofdis_fb_check: the check on two full-resolution optical-flow fields (device pointers).
 * flow_fw, flow_bw: float [n][height][width][2]; occ_*: u8 [n][height][width]; err_*: float [n][height][width].
 * Any of the four outputs may be NULL (all NULL: OFDIS_OK, nothing enqueued).  Mask codes: 0 consistent,
 * 1 inconsistent (occluded or wrong), 2 the flow leaves the frame (err = +inf there).
 *
 * Definition, direction fw (bw: F and B exchanged), pixel (x, y), F = flow_fw, B = flow_bw of the same frame; all
 * arithmetic float32 in this order, every operation rounded on its own (no fused multiply-add):
 *   u = F[y][x][0];  v = F[y][x][1];  px = (float)x + u;  py = (float)y + v
 *   inside = px >= 0 && px <= (float)(W-1) && py >= 0 && py <= (float)(H-1)           (false for NaN)
 *   if !inside: occ = 2, err = +inf
 *   x0 = (int)floorf(px); y0 = (int)floorf(py); x1 = min(x0+1, W-1); y1 = min(y0+1, H-1)
 *   ax = px - (float)x0;  ay = py - (float)y0
 *   for k in 0, 1:  top = B[y0][x0][k] + ax*(B[y0][x1][k] - B[y0][x0][k])
 *                   bot = B[y1][x0][k] + ax*(B[y1][x1][k] - B[y1][x0][k])
 *                   b_k = top + ay*(bot - top)
 *   du = u + b_0;  dv = v + b_1;  err = du*du + dv*dv
 *   mag = (u*u + v*v) + (b_0*b_0 + b_1*b_1);  thr = alpha*mag + beta
 *   occ = (err <= thr) ? 0 : 1                                                        (NaN err -> 1)
 *   a NaN err is stored as the canonical quiet NaN 0x7fc00000 (IEEE 754 leaves a generated NaN's sign and payload open)
 * Suggested thresholds: alpha = 0.01, beta = 0.5 (the paper's).  alpha or beta negative or not finite, NULL flows,
 * n < 1, non-positive sizes or width * height >= 2^31 return OFDIS_ERR_INVALID_ARGUMENT before anything is
 * enqueued.  Stream and ordering rules are those of ofdis_run_batch_u8.
 */
int ofdis_fb_check(ofdis_context *ctx, const float *flow_fw, const float *flow_bw, int n, int width, int height,
                   float alpha, float beta, uint8_t *occ_fw, uint8_t *occ_bw, float *err_fw, float *err_bw,
                   void *stream);

/* Both directions of n pairs from one pyramid, plus the check: flow_fw == ofdis_run_batch_u8(a, b) and
 * flow_bw == ofdis_run_batch_u8(b, a), bit for bit, at less than the cost of the two calls -- the pyramid is built
 * once, and with usefbcon = 1 the backward patch grid and refinement that a plain call already runs above the
 * finest scale (and drops there, oflow.cpp:266,286) are run at the finest scale too instead of a second time from
 * scratch.  flow_bw and the occ / err outputs may be NULL (masks without flow_bw: the backward field stays in the
 * workspace; all five NULL: the plain call).  Optical flow only: OFDIS_MODE_DE returns OFDIS_ERR_UNSUPPORTED (the
 * depth path's right-camera clamp has no pinned counterpart), and so does a call while a stage capture is set.
 * No initial flow.  verbosity is ignored (no TIME lines).  Argument errors as for ofdis_run_batch_u8 and
 * ofdis_fb_check; stream, ordering, chunking and workspace rules are those of ofdis_run_batch_u8. */
int ofdis_run_bidir_u8(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height,
                       const ofdis_params *p, float alpha, float beta, float *flow_fw, float *flow_bw,
                       uint8_t *occ_fw, uint8_t *occ_bw, float *err_fw, float *err_bw, void *stream);
/* Same with host buffers (synchronous). */
int ofdis_run_bidir_u8_host(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, int n, int width,
                            int height, const ofdis_params *p, float alpha, float beta, float *flow_fw,
                            float *flow_bw, uint8_t *occ_fw, uint8_t *occ_bw, float *err_fw, float *err_bw);

/* ------------------------------------------------------------------ stereo: both views and left-right masks
 *
 * Not in the reference, whose depth mode gives the left view's disparity and nothing that says where it can be
 * trusted.  The left-right consistency check is the forward-backward check of a rectified pair: follow each pixel
 * along its disparity into the other view, read that view's disparity there and ask whether the two cancel.
 *
 * ofdis_lr_check: the check on two full-resolution disparity fields (device pointers).
 * disp_l, disp_r: float [n][height][width]; occ_*: u8 [n][height][width]; err_*: float [n][height][width].
 * disp_l[y][x] = d: left pixel x matches right pixel x + d (d <= 0 from the plain depth call); disp_r[y][x] = d: right
 * pixel x matches left pixel x + d (d >= 0).  The check does not assume the signs.  Any of the four outputs may be
 * NULL (all NULL: OFDIS_OK, nothing enqueued).  Mask codes: 0 consistent, 1 inconsistent (occluded or wrong), 2 the
 * disparity leaves the frame (err = +inf there).
 *
 * Definition, view l (r: D and O exchanged), pixel (x, y), D = the view's own field, O = the other field of the same
 * frame; all arithmetic float32 in this order, every operation rounded on its own (no fused multiply-add):
 *   u = D[y][x];  px = (float)x + u
 *   inside = px >= 0 && px <= (float)(W-1)                                            (false for NaN)
 *   if !inside: occ = 2, err = +inf
 *   x0 = (int)floorf(px);  x1 = min(x0+1, W-1);  ax = px - (float)x0
 *   b = O[y][x0] + ax*(O[y][x1] - O[y][x0])
 *   d = u + b;  err = d*d;  mag = u*u + b*b;  thr = alpha*mag + beta
 *   occ = (err <= thr) ? 0 : 1                                                        (NaN err -> 1)
 *   a NaN err is stored as the canonical quiet NaN 0x7fc00000
 * This is ofdis_fb_check on the two-component fields (d, 0), bit for bit, whenever both fields are finite (the v terms
 * are exact zeros there and the vertical tap has weight 0).  Thresholds, NULL rules, refusals, stream and ordering
 * rules are those of ofdis_fb_check.
 */
int ofdis_lr_check(ofdis_context *ctx, const float *disp_l, const float *disp_r, int n, int width, int height,
                   float alpha, float beta, uint8_t *occ_l, uint8_t *occ_r, float *err_l, float *err_r, void *stream);

/* Both views' disparities of n rectified pairs and the check, from one call.  img_l / img_r: device u8
 * [n][height][width][noc].  Definition, with mir(I)[y][x] = I[y][width-1-x]:
 *   disp_l == ofdis_run_batch_u8(img_l, img_r) in OFDIS_MODE_DE, bit for bit;
 *   M = ofdis_run_batch_u8(mir(img_r), mir(img_l)): the mirrored right image is the left camera of a valid rectified
 *   pair, so the plain depth call applies to it unchanged (the mirrored pair is padded for divisibility after
 *   mirroring, exactly as that call pads it: with an odd padding the two views' padded frames differ);
 *   disp_r[y][x] = M[y][width-1-x] with its sign bit flipped (+0 becomes -0, a NaN keeps its payload);
 *   the masks and errors are ofdis_lr_check(disp_l, disp_r).
 * (The reference's own backward field -- usefbcon's right-camera grid, patch.cpp:186-190 with camlr == 1, clamped to
 * >= 0 and then to <= 0 by the refinement -- is not a right-view disparity; it stays an internal of the plain call.)
 * At less than the cost of the two calls: both views of a chunk run as one batch of 2n flow pairs through the same
 * launches, the mirrored frames' pyramid base is read from img_l / img_r through a mirrored column index (no mirrored
 * copy of the images), and the upsample stores the mirrored half at column width-1-x with the sign flipped (no pass
 * over the float fields).
 * disp_l is required; disp_r and the occ / err outputs may be NULL (masks without disp_r: the right field stays in the
 * workspace; all five NULL: the plain call).  Depth only: OFDIS_MODE_OF returns OFDIS_ERR_UNSUPPORTED, and so does a
 * call while a stage capture is set.  No initial flow.  verbosity is ignored (no TIME lines).  Float32 outputs only.
 * Argument errors as for ofdis_run_bidir_u8; stream, ordering, chunking, graph and workspace rules are those of
 * ofdis_run_batch_u8, with chunk sizes counting stereo pairs: a stereo pair is two flow pairs and four pyramid frames,
 * so a launch takes at most ofdis_max_frames_per_launch() / 2 of them. */
int ofdis_run_stereo_u8(ofdis_context *ctx, const uint8_t *img_l, const uint8_t *img_r, int n, int width, int height,
                        const ofdis_params *p, float alpha, float beta, float *disp_l, float *disp_r,
                        uint8_t *occ_l, uint8_t *occ_r, float *err_l, float *err_r, void *stream);
/* Same with host buffers (synchronous). */
int ofdis_run_stereo_u8_host(ofdis_context *ctx, const uint8_t *img_l, const uint8_t *img_r, int n, int width,
                             int height, const ofdis_params *p, float alpha, float beta, float *disp_l, float *disp_r,
                             uint8_t *occ_l, uint8_t *occ_r, float *err_l, float *err_r);

/* ------------------------------------------------------------------ video sequences
 *
 * Not in the reference, which reads two files per process.  frames: device u8 [nframes][height][width][noc], the
 * consecutive frames of one video.  n = nframes - stride pairs are computed, pair i being (frame i, frame i + stride):
 * flow_fw == ofdis_run_batch_u8(frames, frames + stride frames, n), bit for bit -- but every frame's pyramid (base
 * level, 2x2 levels, padded image and gradients) is built once, nframes of them, where the two-array call builds 2n.
 * All outputs are [n]...: flow_fw (required) float [n][height][width][2].  flow_bw, occ_*, err_* are optional and
 * have ofdis_run_bidir_u8's meaning and arithmetic for every pair (flow_bw == the plain call on the pair reversed);
 * with all five NULL, alpha and beta are ignored.  init_flow: optional device float [n][height][width][2], the
 * initial flow per pair with ofdis_run_batch_u8_init's meaning.
 * Refusals, before anything is enqueued (the context stays usable): stride < 1 or nframes <= stride, a NULL frames /
 * flow_fw pointer or a non-positive size -> OFDIS_ERR_INVALID_ARGUMENT; with a backward output, alpha / beta as in
 * ofdis_fb_check; init_flow together with any of the five backward outputs -> OFDIS_ERR_UNSUPPORTED (the
 * bidirectional path has no pinned initial backward flow); OFDIS_MODE_DE -> OFDIS_ERR_UNSUPPORTED (a stereo pair is
 * not a sequence).  A stage capture behaves as in ofdis_run_batch_u8 when no backward output is asked for (pair 0,
 * one launch) and is refused as in ofdis_run_bidir_u8 otherwise.  verbosity is ignored (no TIME lines).
 * Chunked calls ("streams" / "chunk", batches beyond ofdis_max_frames_per_launch()): a chunk of m pairs from pair f0
 * reads frames [f0, f0 + m + stride), so neighbouring chunks rebuild the `stride` frames they share.  Stream,
 * ordering and workspace rules are those of ofdis_run_batch_u8. */
int ofdis_run_sequence_u8(ofdis_context *ctx, const uint8_t *frames, int nframes, int stride, const float *init_flow,
                          int width, int height, const ofdis_params *p, float alpha, float beta, float *flow_fw,
                          float *flow_bw, uint8_t *occ_fw, uint8_t *occ_bw, float *err_fw, float *err_bw,
                          void *stream);
/* Same with host buffers (synchronous). */
int ofdis_run_sequence_u8_host(ofdis_context *ctx, const uint8_t *frames, int nframes, int stride,
                               const float *init_flow, int width, int height, const ofdis_params *p, float alpha,
                               float beta, float *flow_fw, float *flow_bw, uint8_t *occ_fw, uint8_t *occ_bw,
                               float *err_fw, float *err_bw);

/* ------------------------------------------------------------------ compact output formats
 *
 * Not in the reference, whose one output is float32, interleaved, at full resolution (run_dense.cpp:407-415) -- the
 * largest array a call moves.  A format names the element type, the layout and the grid of the forward flow:
 *   dtype   F32, or F16: every float32 value converted to IEEE binary16, round to nearest even, overflow to +-inf,
 *           subnormals kept;
 *   layout  INTERLEAVED [n][H][W][nop], or PLANAR [n][nop][H][W] (the same values transposed; one layout when nop = 1);
 *   grid    FULL: the plain call's width x height field.  LEVEL: the finest level's flow as the coarse-to-fine loop
 *           leaves it (tv_flow[sc_l] of the stage capture; dis_flow[sc_l] with usetvref = 0 -- the values OFClass hands
 *           to run_dense.cpp:387-401), multiplied by 2^sc_l, so every format is in full-resolution pixels.  No
 *           upsample runs.  The level grid belongs to the divisibility-padded frame and is not cropped: cell (X, Y)
 *           covers the original pixels [X * cell - off_x, (X + 1) * cell - off_x) x [Y * cell - off_y, ...).
 * {F32, INTERLEAVED, FULL}, or a NULL format, is the plain call: the same launches. */
enum { OFDIS_OUT_F32 = 0, OFDIS_OUT_F16 = 1 };             /* dtype  */
enum { OFDIS_OUT_INTERLEAVED = 0, OFDIS_OUT_PLANAR = 1 };  /* layout */
enum { OFDIS_OUT_FULL = 0, OFDIS_OUT_LEVEL = 1 };          /* grid   */
typedef struct ofdis_out_format { int dtype, layout, grid; } ofdis_out_format;

/* The output grid of one pair in format fmt (NULL = the plain format), host only.  FULL: out_w x out_h = width x
 * height, offsets 0, cell 1.  LEVEL: out_w = Wp >> sc_l, out_h = Hp >> sc_l, cell = 2^sc_l, off_x = floor(padw / 2),
 * off_y = floor(padh / 2), where Wp = width + padw and Hp = height + padh are the sizes padded to a multiple of 2^sc_f,
 * or of 2^(sc_f+1) when with_init (run_dense.cpp:299-312).  bytes_per_pair = out_w * out_h * nop * element size.  Any
 * output pointer may be NULL.  Invalid parameters, sizes or enum values return OFDIS_ERR_INVALID_ARGUMENT. */
int ofdis_out_geometry(const ofdis_params *p, int width, int height, int with_init, const ofdis_out_format *fmt,
                       int *out_w, int *out_h, int *off_x, int *off_y, int *cell, size_t *bytes_per_pair);

/* ofdis_run_batch_u8_init writing flow_out in format fmt: n * bytes_per_pair bytes, nothing beyond them.  Both modes.
 * init_flow (or NULL) stays float32 [n][height][width][nop]; with it the level grid is the with_init one.  Stage
 * capture, options, streams, chunks and graphs behave as in the plain call; the _host form ignores verbosity.
 * Refusals before anything is enqueued: those of the plain call, an unknown enum value, and a frame of 2^31 pixels
 * or more (OFDIS_ERR_INVALID_ARGUMENT). */
int ofdis_run_batch_u8_fmt(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, const float *init_flow,
                           int n, int width, int height, const ofdis_params *p, const ofdis_out_format *fmt,
                           void *flow_out, void *stream);
int ofdis_run_batch_u8_fmt_host(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, const float *init_flow,
                                int n, int width, int height, const ofdis_params *p, const ofdis_out_format *fmt,
                                void *flow_out);
/* ofdis_run_sequence_u8's forward flow in format fmt (the backward flow, masks and errors are defined on float32
 * fields and stay with ofdis_run_sequence_u8). */
int ofdis_run_sequence_u8_fmt(ofdis_context *ctx, const uint8_t *frames, int nframes, int stride,
                              const float *init_flow, int width, int height, const ofdis_params *p,
                              const ofdis_out_format *fmt, void *flow_fw, void *stream);
int ofdis_run_sequence_u8_fmt_host(ofdis_context *ctx, const uint8_t *frames, int nframes, int stride,
                                   const float *init_flow, int width, int height, const ofdis_params *p,
                                   const ofdis_out_format *fmt, void *flow_fw);

/* ------------------------------------------------------------------ flow-driven image warping
 *
 * Not in the reference, which stops at the flow file.  The first thing a consumer does with a flow is pull frame b
 * back onto frame a along it (motion compensation, temporal denoising, interpolation, photometric error maps).
 *
 * ofdis_warp_u8: backward warp of n u8 frames by n optical-flow fields (device pointers).
 * img: u8 [n][height][width][noc] (noc 1 or 3); out: u8 or float32 (out_dtype) of the same shape; valid: u8
 * [n][height][width] or NULL.  flow: the field in any form ofdis_run_batch_u8_fmt can write, described by view.
 *
 * Definition, frame size W x H, pixel (x, y), channel c, (u, v) the flow at that pixel as float32 (a binary16 value
 * converted exactly); all arithmetic float32 in this order, every operation rounded on its own (no fused multiply-add):
 *   su = scale*u;  sv = scale*v
 *   px = (float)x + su;  py = (float)y + sv
 *   inside = px >= 0 && px <= (float)(W-1) && py >= 0 && py <= (float)(H-1)           (false for NaN)
 *   pxc = fminf(fmaxf(px, 0), (float)(W-1));  pyc likewise                  (NaN -> 0: IEEE maxNum / minNum)
 *   x0 = (int)floorf(pxc); y0 = (int)floorf(pyc); x1 = min(x0+1, W-1); y1 = min(y0+1, H-1)
 *   ax = pxc - (float)x0;  ay = pyc - (float)y0
 *   t.. = (float)img[y.][x.][c]
 *   top = t00 + ax*(t01 - t00);  bot = t10 + ax*(t11 - t10);  val = top + ay*(bot - top)
 *   float32 output: val.   u8 output: (uint8_t)rintf(val)                             (round half to even)
 *   valid = inside ? 1 : 0
 * The u8 form needs no clamp: the taps are integers in 0..255 and every rounding is monotonic, so val stays in [0, 255].
 * A pixel whose position leaves the frame samples the replicated border and is flagged valid = 0.
 *
 * Flow views.  dtype / layout / grid are ofdis_out_format's enums.  FULL: flow is [n][H][W][2] (INTERLEAVED) or
 * [n][2][H][W] (PLANAR); the other fields are ignored.  LEVEL: flow is [n][gh][gw][2] or [n][2][gh][gw], the level
 * grid of ofdis_run_batch_u8_fmt, and gw, gh, cell, off_x, off_y are what ofdis_out_geometry reports for it (out_w,
 * out_h, cell, off_x, off_y).  (u, v) at pixel (x, y) is then the value the plain call's upsample computes from those
 * cells -- cv::resize INTER_LINEAR's taps of column x + off_x and row y + off_y, h = s0*(1-fx) + s1*fx per source
 * row, then h0*(1-fy) + h1*fy; the cell at (x + off_x, y + off_y) itself when cell = 1 -- so a float32 level view gives
 * the picture of the full-resolution float32 field bit for bit, and that field is never written or read.
 *
 * Refused before anything is enqueued (OFDIS_ERR_INVALID_ARGUMENT, the context stays usable): NULL img / flow / view /
 * out, n < 1, non-positive sizes, noc not 1 or 3, unknown enum values, a level view whose cell is not a power of two in
 * 1..512 or whose grid does not cover the frame (gw*cell < width + off_x, gh*cell < height + off_y, a negative
 * offset), scale not finite, width * height >= 2^31.  Stream, ordering and workspace rules are those of ofdis_fb_check. */
enum { OFDIS_IMG_U8 = 0, OFDIS_IMG_F32 = 1 }; /* out_dtype */
typedef struct ofdis_flow_view { int dtype, layout, grid, gw, gh, cell, off_x, off_y; } ofdis_flow_view;
int ofdis_warp_u8(ofdis_context *ctx, const uint8_t *img, const void *flow, const ofdis_flow_view *view, int n,
                  int width, int height, int noc, float scale, int out_dtype, void *out, uint8_t *valid, void *stream);

/* The flow a -> b of each pair, then img_b warped by it: at scale = 1, frame b pulled back onto frame a.  By definition
 * out / valid == ofdis_warp_u8(img_b, ofdis_run_batch_u8(img_a, img_b)), bit for bit -- but the flow leaves the
 * coarse-to-fine loop as the float32 level grid, n * bytes_per_pair bytes in a buffer the context owns, and the warp
 * expands it on the fly: no full-resolution flow is allocated or written and no upsample runs.  valid may be NULL.
 * Optical flow only: OFDIS_MODE_DE returns OFDIS_ERR_UNSUPPORTED.  No initial flow.  verbosity is ignored (no TIME
 * lines).  A stage capture behaves as in ofdis_run_batch_u8_fmt.  Argument errors as for ofdis_run_batch_u8 and
 * ofdis_warp_u8; stream, ordering, chunking, graph and workspace rules are those of ofdis_run_batch_u8. */
int ofdis_run_warp_u8(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height,
                      const ofdis_params *p, float scale, int out_dtype, void *out, uint8_t *valid, void *stream);
/* Same with host buffers (synchronous). */
int ofdis_run_warp_u8_host(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, int n, int width,
                           int height, const ofdis_params *p, float scale, int out_dtype, void *out, uint8_t *valid);

/* ------------------------------------------------------------------ frame interpolation
 *
 * Not in the reference.  The frame between two frames at time t in [0, 1] (frame-rate conversion, slow motion), from
 * the two flows of the pair: every pixel of the new frame reads both frames along flows scaled to its time and blends
 * the two samples.
 *
 * ofdis_interp_u8: n pairs of u8 frames img_a, img_b ([n][height][width][noc], noc 1 or 3), the forward flow F (a -> b,
 * on a's pixel grid) and the backward flow B (b -> a, on b's pixel grid), both described by the one `view`, and nt times
 * t[k] (a host array, copied at the call).  out: u8 or float32 (out_dtype) [n][nt][height][width][noc]; valid: u8
 * [n][nt][height][width] or NULL.  occ_a / occ_b: u8 [n][height][width] occlusion masks of frame a / frame b
 * (ofdis_fb_check's occ_fw / occ_bw), either may be NULL.  All pointers but t are device pointers.
 *
 * Definition, pixel (x, y), time t, (fu, fv) = F and (bu, bv) = B at that pixel as float32 (a binary16 value converted
 * exactly; a level view expanded exactly as ofdis_warp_u8 defines); all arithmetic float32 in this order, every
 * operation rounded on its own (no fused multiply-add):
 *   c  = 1 - t
 *   ua = t*(t*bu - c*fu);   va = t*(t*bv - c*fv)        (flow from time t back to frame a: -(1-t)t F + t^2 B)
 *   ub = c*(c*fu - t*bu);   vb = c*(c*fv - t*bv)        (flow from time t on to frame b: (1-t)^2 F - t(1-t) B)
 *   A[ch], in_a, (pxc_a, pyc_a) = ofdis_warp_u8's val / inside / clamped position for img_a at (x + ua, y + va), scale 1
 *   Bv[ch], in_b, (pxc_b, pyc_b) = the same for img_b at (x + ub, y + vb)
 *   use_a = in_a;  use_b = in_b
 *   with masks:
 *     xa = (int)rintf(pxc_a), ya = (int)rintf(pyc_a);  if occ_a[ya][xa] != 0: use_b = false
 *                                                   (a's content there has no consistent match in b)
 *     xb, yb likewise from b's position;               if occ_b[yb][xb] != 0: use_a = false
 *   val = (use_a == use_b) ? A + t*(Bv - A) : (use_a ? A : Bv)
 *   float32 output: val.   u8 output: (uint8_t)rintf(val), no clamp
 *   valid = (use_a ? 1 : 0) | (use_b ? 2 : 0)
 * valid: 3 both frames, 1 frame a only, 2 frame b only, 0 neither -- the plain blend of two border samples.
 * Consequences: without masks and for finite flows, t = 0 returns frame a and t = 1 returns frame b, exactly in the u8
 * form (the displacements towards the returned frame are exact zeros; float32: t = 0 gives a exactly, t = 1 gives
 * A + (Bv - A), Bv to within one rounding).  With masks this does not hold: occ_a set at the sampled position at t = 1
 * leaves A alone, the sample of frame a, and occ_b set at t = 0 leaves Bv alone.  The u8 form needs no clamp, by the
 * warp's argument: both
 * samples lie in [0, 255] and every rounding is monotonic.  A NaN flow clamps the position to column or row 0 and
 * clears that frame's bit.
 *
 * Flow view: any dtype, layout and grid ofdis_warp_u8 accepts; for a level view both grids share the geometry of
 * ofdis_out_geometry, and the pictures equal those of the full-resolution float32 fields bit for bit.
 *
 * Refused before anything is enqueued (OFDIS_ERR_INVALID_ARGUMENT, the context stays usable): everything ofdis_warp_u8
 * refuses; a NULL img_b, flow_bw or t; nt outside 1..OFDIS_INTERP_MAX_T; any t[k] not finite or outside [0, 1].
 * Stream, ordering and workspace rules are those of ofdis_fb_check. */
#define OFDIS_INTERP_MAX_T 16
int ofdis_interp_u8(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, const void *flow_fw,
                    const void *flow_bw, const ofdis_flow_view *view, int n, int width, int height, int noc,
                    const float *t, int nt, const uint8_t *occ_a, const uint8_t *occ_b, int out_dtype, void *out,
                    uint8_t *valid, void *stream);

/* Both flows of each pair from one pyramid, then the nt frames between them.  By definition out / valid ==
 * ofdis_interp_u8(img_a, img_b, F, B, no masks) bit for bit, with F, B the two flows of ofdis_run_bidir_u8 -- but both
 * flows leave the coarse-to-fine loop as float32 level grids, 2 * n * bytes_per_pair bytes in the buffer the context
 * owns, and the interpolation expands them on the fly: no full-resolution flow is allocated or written and no upsample
 * runs, and every further time of a pair reuses the expanded flows.  valid may be NULL.
 * This call takes no masks; ofdis_run_interp_occ_u8 (below) is the fused call with them.
 * Optical flow only: OFDIS_MODE_DE returns OFDIS_ERR_UNSUPPORTED.  No initial flow.  verbosity is ignored.  A stage
 * capture that is set is refused as in ofdis_run_bidir_u8 (OFDIS_ERR_UNSUPPORTED).  Argument errors as for
 * ofdis_run_batch_u8 and ofdis_interp_u8; stream, ordering, chunking, round-robin, graph and workspace rules are those
 * of ofdis_run_batch_u8 (the graph is recorded anew when out, valid, out_dtype, nt or a t[k] changes). */
int ofdis_run_interp_u8(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height,
                        const ofdis_params *p, const float *t, int nt, int out_dtype, void *out, uint8_t *valid,
                        void *stream);
/* Same with host buffers (synchronous). */
int ofdis_run_interp_u8_host(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, int n, int width,
                             int height, const ofdis_params *p, const float *t, int nt, int out_dtype, void *out,
                             uint8_t *valid);

/* ------------------------------------------------------------------ occlusion masks on level grids, video interpolation
 *
 * ofdis_fb_check_level: ofdis_fb_check evaluated directly on two level grids.  grid_fw, grid_bw: device float32
 * [n][gh][gw][2], the forward and backward level grids of ofdis_run_batch_u8_fmt ({F32, INTERLEAVED, LEVEL}); view: that
 * format with the geometry ofdis_out_geometry reports (gw, gh, cell, off_x, off_y).  With E(G) the full-resolution
 * field ofdis_warp_u8's level view defines for grid G -- xtap on column x + off_x, ytap on row y + off_y, up_px_s: the
 * value the plain call's upsample computes; the cell at (x + off_x, y + off_y) itself when cell = 1 -- the outputs are
 * ofdis_fb_check(E(grid_fw), E(grid_bw)) bit for bit: masks, errors, the codes 0 / 1 / 2, +inf outside the frame and the
 * canonical NaN.  Neither expanded field is written: a pixel's own flow is expanded from its grid as the warp does it,
 * the other field at the four taps of x + flow from the other grid's cells.
 * Any other dtype, layout or grid in `view` returns OFDIS_ERR_UNSUPPORTED (a valid enum value; an unknown one is
 * OFDIS_ERR_INVALID_ARGUMENT); a NULL view or a geometry ofdis_warp_u8 refuses returns OFDIS_ERR_INVALID_ARGUMENT.
 * Thresholds, NULL rules (all four outputs NULL: OFDIS_OK, nothing enqueued), stream and ordering rules are those of
 * ofdis_fb_check. */
int ofdis_fb_check_level(ofdis_context *ctx, const float *grid_fw, const float *grid_bw, const ofdis_flow_view *view,
                         int n, int width, int height, float alpha, float beta, uint8_t *occ_fw, uint8_t *occ_bw,
                         float *err_fw, float *err_bw, void *stream);

/* ofdis_run_interp_u8 with occlusion masks.  By definition out / valid == ofdis_interp_u8(img_a, img_b, F, B,
 * occ_a = occ_fw, occ_b = occ_bw) bit for bit, where F, B, occ_fw, occ_bw are the four outputs of
 * ofdis_run_bidir_u8(alpha, beta) -- but per chunk the two level grids are written, ofdis_fb_check_level computes the
 * masks from them and the interpolation reads grids and masks: no upsample runs and no full-resolution flow exists.
 * occ_fw / occ_bw: optional device u8 [n][height][width] outputs, equal to ofdis_run_bidir_u8's; a mask that is NULL
 * lives in the chunk's workspace (sized per chunk, not per call).
 * Refusals and modes are those of ofdis_run_interp_u8, plus ofdis_fb_check's threshold rules.  The graph is recorded
 * anew when, beyond ofdis_run_interp_u8's list, alpha, beta or a mask pointer changes, and a call with masks never
 * replays the graph of one without. */
int ofdis_run_interp_occ_u8(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height,
                            const ofdis_params *p, const float *t, int nt, float alpha, float beta, int out_dtype,
                            void *out, uint8_t *valid, uint8_t *occ_fw, uint8_t *occ_bw, void *stream);
/* Same with host buffers (synchronous). */
int ofdis_run_interp_occ_u8_host(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, int n, int width,
                                 int height, const ofdis_params *p, const float *t, int nt, float alpha, float beta,
                                 int out_dtype, void *out, uint8_t *valid, uint8_t *occ_fw, uint8_t *occ_bw);

/* The frames between the frames of one video.  frames: device u8 [nframes][height][width][noc]; n = nframes - stride
 * pairs, pair i being (frame i, frame i + stride); out [n][nt][height][width][noc], valid [n][nt][height][width] or
 * NULL.  use_occ = 0: out / valid == ofdis_run_interp_u8(frames, frames + stride frames, n) bit for bit (alpha, beta,
 * occ_fw, occ_bw are ignored); use_occ = 1: == ofdis_run_interp_occ_u8 on those arrays, occ_fw / occ_bw optional
 * [n][height][width] outputs.  Every frame's pyramid is built once, nframes of them where the pair call builds 2n
 * (ofdis_run_sequence_u8's plan); the interpolation reads frame b of pair i at frame i + stride of the same array.
 * Chunked calls overlap by `stride` frames as documented for ofdis_run_sequence_u8.  Refusals: those of
 * ofdis_run_sequence_u8's bidirectional form (stride < 1, nframes <= stride, OFDIS_MODE_DE, a set stage capture) and
 * those of ofdis_run_interp_u8 / ofdis_run_interp_occ_u8.  A graph recorded by the pair call is never replayed by the
 * sequence call on the same pointers, nor one of another stride. */
int ofdis_run_sequence_interp_u8(ofdis_context *ctx, const uint8_t *frames, int nframes, int stride, int width,
                                 int height, const ofdis_params *p, const float *t, int nt, int use_occ, float alpha,
                                 float beta, int out_dtype, void *out, uint8_t *valid, uint8_t *occ_fw,
                                 uint8_t *occ_bw, void *stream);
/* Same with host buffers (synchronous). */
int ofdis_run_sequence_interp_u8_host(ofdis_context *ctx, const uint8_t *frames, int nframes, int stride, int width,
                                      int height, const ofdis_params *p, const float *t, int nt, int use_occ,
                                      float alpha, float beta, int out_dtype, void *out, uint8_t *valid,
                                      uint8_t *occ_fw, uint8_t *occ_bw);

/* ------------------------------------------------------------------ point tracking along a video
 *
 * Not in the reference.  Points followed through the frames of a video along its flows (long-range correspondence,
 * dense trajectories, stabilisation), each with a flag that says where its track stopped being trustworthy.
 *
 * ofdis_track_points: npts points through a chain of m fields.  All pointers are device pointers.
 * flow_fw: m fields back to back, field j the flow from frame j to frame j + 1 on frame j's pixel grid --
 * ofdis_run_sequence_u8's flow_fw (stride 1), or its level-grid form.  flow_bw: NULL, or the m backward fields, field j
 * the flow from frame j + 1 to frame j on frame j + 1's grid (ofdis_run_sequence_u8's flow_bw).  Both are described by
 * the one `view`: a full view of any dtype and layout ofdis_warp_u8 takes, or a level view, float32 interleaved only, with
 * the geometry of ofdis_out_geometry (any other valid enum value in a level view returns OFDIS_ERR_UNSUPPORTED, as in
 * ofdis_fb_check_level).  points: float [npts][2], (x, y) in pixels.  start: NULL (= 0) or int32 [npts], the frame at
 * which point k enters, clamped on the device to [0, m].
 * Outputs, frame-major: tracks float [m + 1][npts][2], status u8 [m + 1][npts]; with flags & OFDIS_TRACK_LAST only entry
 * m is written, tracks [npts][2] and status [npts].  Either may be NULL (both NULL: OFDIS_OK, nothing enqueued).
 * Status codes: 0 tracked, every step so far consistent; 1 tracked, but some step so far failed the forward-backward
 * check (sticky; the position keeps advancing); 2 left the frame (the position is frozen); 3 not started yet.
 *
 * Definition; all arithmetic float32 in this order, every operation rounded on its own (no fused multiply-add).
 * S(G, px, py), field G at an in-frame position, is ofdis_fb_check's bilinear gather:
 *   x0 = (int)floorf(px);  x1 = min(x0+1, W-1);  ax = px - (float)x0;  y0, y1, ay likewise
 *   for each of the two components:  top = G[y0][x0] + ax*(G[y0][x1] - G[y0][x0])
 *                                    bot = G[y1][x0] + ax*(G[y1][x1] - G[y1][x0])
 *                                    S   = top + ay*(bot - top)
 * G at integer pixels holds the values the view defines: a binary16 value converted exactly; for a level view the value
 * the plain call's upsample computes, E(G) of ofdis_fb_check_level.
 *   in(px, py) = px >= 0 && px <= (float)(W-1) && py >= 0 && py <= (float)(H-1)       (false for NaN)
 * Point k, s0 = its clamped start:
 *   entries j < s0 hold the query point itself, status 3;
 *   entry s0 holds the point, status in(x, y) ? 0 : 2;
 *   a step from entry j at (px, py) with status s in {0, 1}:
 *     (fu, fv) = S(F_j, px, py);  qx = px + fu;  qy = py + fv;  entry j + 1 is (qx, qy)
 *     if !in(qx, qy): its status is 2, and every later entry repeats entry j + 1 with status 2
 *     else with flow_bw:  (bu, bv) = S(B_j, qx, qy);  du = fu + bu;  dv = fv + bv;  err = du*du + dv*dv
 *                         mag = (fu*fu + fv*fv) + (bu*bu + bv*bv);  thr = alpha*mag + beta
 *                         fail = !(err <= thr)   (a NaN fails);   the status of entry j + 1 is s | fail
 *     else (no flow_bw): the status stays s
 *   a point whose status at entry s0 is 2 is frozen there; a NaN coordinate is stored as the canonical quiet NaN 0x7fc00000.
 * Consequences: positions never depend on flow_bw, alpha or beta; a point on the last row or column is inside; zero
 * fields return the points unchanged.
 * Refused before anything is enqueued (OFDIS_ERR_INVALID_ARGUMENT, the context stays usable): whatever ofdis_warp_u8
 * refuses of a view and a size; NULL flow_fw or points; m < 1 or npts < 1; unknown flag bits; with flow_bw, the threshold
 * rules of ofdis_fb_check.  Stream and ordering rules are those of ofdis_fb_check.  Index arithmetic over npts * (m + 1)
 * is 64-bit. */
enum { OFDIS_TRACK_LAST = 1 }; /* flags */
int ofdis_track_points(ofdis_context *ctx, const void *flow_fw, const void *flow_bw, const ofdis_flow_view *view,
                       int m, int width, int height, const float *points, const int32_t *start, int npts,
                       float alpha, float beta, int flags, float *tracks, uint8_t *status, void *stream);

/* The flows of a video and the tracks through them from one call: frames u8 [nframes][height][width][noc], m = nframes - 1,
 * pair j = (frame j, frame j + 1).  By definition tracks / status == ofdis_track_points on the fields of
 * ofdis_run_sequence_u8(frames, stride 1), bit for bit -- the forward and backward fields when use_fb, the forward ones
 * alone otherwise (alpha, beta ignored) -- but every pair's flows leave the coarse-to-fine loop as float32 level grids,
 * m * (1 or 2) * bytes_per_pair bytes in the buffer the context owns, and one launch marches every point through all
 * of them after the last chunk: no upsample runs, no full-resolution field exists, and every frame's pyramid is built
 * once (chunked calls overlap by one frame as documented for ofdis_run_sequence_u8).
 * Optical flow only: OFDIS_MODE_DE returns OFDIS_ERR_UNSUPPORTED, and so does a call while a stage capture is set.  No
 * initial flow.  verbosity is ignored.  Argument errors are those of ofdis_run_sequence_u8 (nframes < 2, ...) and of
 * ofdis_track_points; stream, ordering, chunking, round-robin, graph and workspace rules are those of
 * ofdis_run_batch_u8 (the graph is recorded anew when a point, start or output pointer, npts, flags, use_fb, alpha or
 * beta changes; the point values are read at every replay). */
int ofdis_run_sequence_track_u8(ofdis_context *ctx, const uint8_t *frames, int nframes, int width, int height,
                                const ofdis_params *p, const float *points, const int32_t *start, int npts,
                                int use_fb, float alpha, float beta, int flags, float *tracks, uint8_t *status,
                                void *stream);
/* Same with host buffers (synchronous). */
int ofdis_run_sequence_track_u8_host(ofdis_context *ctx, const uint8_t *frames, int nframes, int width, int height,
                                     const ofdis_params *p, const float *points, const int32_t *start, int npts,
                                     int use_fb, float alpha, float beta, int flags, float *tracks, uint8_t *status);

/* ------------------------------------------------------------------ motion-compensated temporal denoising
 *
 * Not in the reference.  Every frame of a video averaged with its two neighbours pulled onto it along the flows, each
 * neighbour weighted per pixel by how well it agrees with the frame: noise averages out where the motion is known, and a
 * neighbour that disagrees (a wrong flow, an occlusion, a position outside its frame) drops out.
 *
 * ofdis_tfilter_u8: all pointers are device pointers.  frames: u8 [nframes][height][width][noc], T = nframes, m = T - 1.
 * flow_fw / flow_bw: the m forward / backward fields of ofdis_run_sequence_u8 at stride 1 -- flow_fw field j on frame
 * j's grid (frame j -> j + 1), flow_bw field j on frame j + 1's grid (frame j + 1 -> j).  Both are described by the one
 * `view`, with ofdis_track_points's rules: a full view of any dtype and layout, or a level view, float32 interleaved
 * only (any other valid enum value in a level view returns OFDIS_ERR_UNSUPPORTED).  occ_fw / occ_bw: NULL, or u8
 * [m][height][width], ofdis_run_sequence_u8's occ_fw / occ_bw (mask j of occ_fw on frame j's grid, of occ_bw on frame
 * j + 1's); either may be NULL alone.  out: u8 or float32 (out_dtype) [nframes][height][width][noc].  used: u8
 * [nframes][height][width] or NULL.
 *
 * Definition, frame i, pixel (x, y); all arithmetic float32 in this order, every operation rounded on its own (no fused
 * multiply-add), `/` the correctly rounded division:
 *   inv = 1.0f / (sigma * (float)noc)             computed once on the host
 *   C[ch] = (float)frames[i][y][x][ch]
 *   acc[ch] = C[ch];  wsum = 1;  bits = 0
 *   neighbours in this order:
 *     k = 0 (previous, only if i > 0):     G = flow_bw[i-1], O = occ_bw[i-1], N = frames[i-1]
 *     k = 1 (next,     only if i < T-1):   G = flow_fw[i],   O = occ_fw[i],   N = frames[i+1]
 *     (u, v) = G at (x, y) as the view defines it (binary16 converted exactly; a level view expanded as ofdis_warp_u8
 *              defines)
 *     S[ch], inside = ofdis_warp_u8's val / inside for image N at (x + u, y + v), scale 1
 *     ok = inside && (O == NULL || O[y][x] == 0)
 *     d = |S[0] - C[0]|  (+ |S[1] - C[1]| + |S[2] - C[2]| in this order for noc = 3)
 *     r = d * inv;   w = ok ? fmaxf(1 - r*r, 0) : 0
 *     acc[ch] = acc[ch] + w * S[ch];   wsum = wsum + w;   if w > 0: bits |= 1 << k
 *   val[ch] = acc[ch] / wsum
 *   float32 output: val.    u8 output: (uint8_t)rintf(fminf(val, 255))          (round half to even)
 *   used = bits            (0 the frame itself alone, 1 previous, 2 next, 3 both)
 * Consequences: a NaN or infinite flow clears `inside`, so val is always finite; identical frames with zero flows
 * return the frames exactly, in both output types; a neighbour that differs by sigma grey levels or more per channel
 * (d >= sigma * noc) contributes nothing; the first and the last frame have one neighbour; the positions and weights of
 * one neighbour never depend on the other.
 * Refused before anything is enqueued (OFDIS_ERR_INVALID_ARGUMENT, the context stays usable): whatever ofdis_warp_u8
 * refuses of a view, a size and noc; NULL frames, flow_fw, flow_bw, view or out; nframes < 2; sigma not finite or
 * outside [1/1024, 65536]; an unknown out_dtype; out overlapping frames (neighbours are read after a frame is written).
 * Stream and ordering rules are those of ofdis_fb_check. */
int ofdis_tfilter_u8(ofdis_context *ctx, const uint8_t *frames, int nframes, const void *flow_fw, const void *flow_bw,
                     const ofdis_flow_view *view, int width, int height, int noc, float sigma,
                     const uint8_t *occ_fw, const uint8_t *occ_bw, int out_dtype, void *out, uint8_t *used, void *stream);

/* The flows of a video and its filtered frames from one call.  By definition out / used == ofdis_tfilter_u8 on the
 * fields of ofdis_run_sequence_u8(frames, stride 1) in both directions, bit for bit; with use_occ the masks are that
 * call's occ_fw / occ_bw at alpha, beta (alpha and beta are ignored otherwise).  Every pair's two flows leave the
 * coarse-to-fine loop as float32 level grids, 2 * m * bytes_per_pair bytes in the buffer the context owns; with use_occ
 * every chunk runs the check on its own grids (ofdis_fb_check_level) into 2 * m * width * height bytes of masks behind
 * the grids in that buffer, sized per call; and one launch filters all frames from the grids after the last chunk: no upsample runs and no
 * full-resolution flow exists.
 * Optical flow only: OFDIS_MODE_DE returns OFDIS_ERR_UNSUPPORTED, and so does a call while a stage capture is set.  No
 * initial flow.  verbosity is ignored.  Argument errors are those of ofdis_run_sequence_track_u8 (nframes < 2, ...) and
 * of ofdis_tfilter_u8 (with use_occ, the threshold rules of ofdis_fb_check); stream, ordering, chunking, round-robin,
 * graph and workspace rules are those of ofdis_run_batch_u8 (the graph is recorded anew when an output pointer,
 * out_dtype, sigma, use_occ, alpha or beta changes; a graph of another call kind is never replayed). */
int ofdis_run_sequence_tfilter_u8(ofdis_context *ctx, const uint8_t *frames, int nframes, int width, int height,
                                  const ofdis_params *p, float sigma, int use_occ, float alpha, float beta,
                                  int out_dtype, void *out, uint8_t *used, void *stream);
/* Same with host buffers (synchronous). */
int ofdis_run_sequence_tfilter_u8_host(ofdis_context *ctx, const uint8_t *frames, int nframes, int width, int height,
                                       const ofdis_params *p, float sigma, int use_occ, float alpha, float beta,
                                       int out_dtype, void *out, uint8_t *used);

/* ------------------------------------------------------------------ temporal denoising over a radius of frames
 *
 * Not in the reference.  ofdis_tfilter_u8 with up to R frames on each side instead of one: the position of a pixel is
 * chained through the fields as ofdis_track_points chains a point, every frame it passes is sampled there and weighted
 * as ofdis_tfilter_u8 weights its neighbours, and the forward-backward check runs inside the chain, step by step, so
 * there are no mask inputs.
 *
 * ofdis_tfilter_radius_u8: frames, flow_fw, flow_bw, view, out and out_dtype are exactly ofdis_tfilter_u8's (a full view
 * of any dtype and layout, or a level view, float32 interleaved only).  radius R in [1, 4].  used: u8
 * [nframes][height][width] or NULL.  Occlusion handling is use_fb with alpha and beta.
 *
 * Definition, frame i, pixel (x, y); all arithmetic float32 in this order, every operation rounded on its own (no fused
 * multiply-add), `/` the correctly rounded division.  inv, C, acc, wsum and bits start as in ofdis_tfilter_u8; S(G, px, py)
 * and in(px, py) are ofdis_track_points's gather and predicate (in is false for NaN).  Two chains, the previous
 * direction (d = 0) first, then the next (d = 1); in a direction k = 1 .. R while frame j exists:
 *     previous: j = i - k >= 0;   step field F_k = flow_bw[j],    opposite field B_k = flow_fw[j]
 *     next:     j = i + k <= T-1; step field F_k = flow_fw[j-1],  opposite field B_k = flow_bw[j-1]
 *   start: P_0 = ((float)x, (float)y), alive, not failed
 *   (fu, fv) = for k = 1 the pixel's own value of F_1 as the view defines it (exactly as ofdis_tfilter_u8 reads it);
 *              for k >= 2 S(F_k, P_{k-1})
 *   P_k = P_{k-1} + (fu, fv)                       one float add per component
 *   if !in(P_k): the chain is dead -- this neighbour and every farther one of the direction contribute nothing, and
 *                nothing further is read
 *   with use_fb: (bu, bv) = S(B_k, P_k);  du = fu + bu;  dv = fv + bv;  err = du*du + dv*dv
 *                mag = (fu*fu + fv*fv) + (bu*bu + bv*bv);  thr = alpha*mag + beta
 *                failed = failed || !(err <= thr)      (a NaN fails; sticky along the chain; ofdis_track_points's step)
 *   S[ch] = ofdis_warp_u8's val for image frames[j], pixel (0, 0), flow P_k, scale 1 -- the bilinear taps at the position
 *           P_k itself (1 * p and 0 + p are p); for k = 1 this is ofdis_tfilter_u8's sample at (x + u, y + v)
 *   ok = alive && !failed
 *   d = |S[0] - C[0]|  (+ |S[1] - C[1]| + |S[2] - C[2]| in this order for noc = 3)
 *   r = d * inv;   w = ok ? fmaxf(1 - r*r, 0) : 0
 *   acc[ch] = acc[ch] + w * S[ch];   wsum = wsum + w;   if w > 0: bits |= 1 << (2 * (k - 1) + d)
 *   val[ch] = acc[ch] / wsum;  the output conversions are ofdis_tfilter_u8's;  used = bits
 * Without use_fb alpha and beta are ignored and flow_bw is read only as the previous direction's step fields.
 * Consequences: val is always finite; identical frames with zero flows return the frames; positions never depend on the
 * pictures, on sigma, on alpha and beta, or on the other direction; a failed step contributes a weight of 0 to every
 * later step of its direction, which adds exact zeros, so an implementation may stop a chain there; R = 1 without use_fb
 * is ofdis_tfilter_u8 without masks, bit for bit, `used` included; R = 1 with use_fb is ofdis_tfilter_u8 with the
 * occ_fw / occ_bw of ofdis_fb_check(alpha, beta) on the same float32 fields (of ofdis_fb_check_level on the same
 * grids), bit for bit; frames within R of an end have shorter chains.
 * Refused before anything is enqueued (OFDIS_ERR_INVALID_ARGUMENT, the context stays usable): whatever ofdis_tfilter_u8
 * refuses; radius outside [1, 4]; with use_fb, the threshold rules of ofdis_fb_check.  Stream and ordering rules are
 * those of ofdis_tfilter_u8. */
int ofdis_tfilter_radius_u8(ofdis_context *ctx, const uint8_t *frames, int nframes, const void *flow_fw,
                            const void *flow_bw, const ofdis_flow_view *view, int width, int height, int noc,
                            int radius, float sigma, int use_fb, float alpha, float beta, int out_dtype, void *out,
                            uint8_t *used, void *stream);

/* The flows of a video and its frames filtered over a radius from one call.  By definition out / used ==
 * ofdis_tfilter_radius_u8 on the fields of ofdis_run_sequence_u8(frames, stride 1) in both directions, bit for bit.
 * Every pair's two flows leave the coarse-to-fine loop as float32 level grids, 2 * m * bytes_per_pair bytes in the buffer
 * the context owns, and one launch filters all frames from the grids after the last chunk: no upsample and no
 * forward-backward check launch runs, no mask plane and no full-resolution flow exists.
 * Optical flow only: OFDIS_MODE_DE returns OFDIS_ERR_UNSUPPORTED, and so does a call while a stage capture is set.  No
 * initial flow.  verbosity is ignored.  Argument errors are those of ofdis_run_sequence_tfilter_u8 and of
 * ofdis_tfilter_radius_u8; stream, ordering, chunking, round-robin, graph and workspace rules are those of
 * ofdis_run_batch_u8 (the graph is recorded anew when an output pointer, out_dtype, radius, sigma, use_fb, alpha or beta
 * changes; a graph of another call kind is never replayed). */
int ofdis_run_sequence_tfilter_radius_u8(ofdis_context *ctx, const uint8_t *frames, int nframes, int width, int height,
                                         const ofdis_params *p, int radius, float sigma, int use_fb, float alpha,
                                         float beta, int out_dtype, void *out, uint8_t *used, void *stream);
/* Same with host buffers (synchronous). */
int ofdis_run_sequence_tfilter_radius_u8_host(ofdis_context *ctx, const uint8_t *frames, int nframes, int width,
                                              int height, const ofdis_params *p, int radius, float sigma, int use_fb,
                                              float alpha, float beta, int out_dtype, void *out, uint8_t *used);

/* ------------------------------------------------------------------ global motion and video stabilisation
 *
 * Not in the reference.  The camera's motion between the frames of a video as one 2 x 3 transform per frame pair, fitted
 * robustly to the flow at a sparse lattice of samples, and the stabilised video built from those transforms: the
 * cumulative camera path, smoothed, and every frame pulled through the difference.  Three device primitives and one
 * fused call.  All transform arithmetic is float64 (normal equations over coordinates up to 4096 px are ill-conditioned
 * in float32); every operation below is rounded on its own (no fused multiply-add), `/` is the correctly rounded
 * division, and there is no square root and no transcendental function, so numpy restates every bit
 * (tests/test_stabilize.py).  A transform is six doubles (m00, m01, m02, m10, m11, m12) in pixel coordinates.
 *
 * ofdis_fit_motion: a robust similarity (or translation) per field of a chain of m fields.  All pointers are device
 * pointers.  flow_fw / flow_bw / view: ofdis_track_points's rules -- a full view of any dtype and layout, or a level
 * view, float32 interleaved only (any other valid enum value in a level view returns OFDIS_ERR_UNSUPPORTED), which gives
 * the bits of the full float32 field.  flow_bw NULL: no consistency check (alpha, beta ignored).
 * xform: double [m][6]; support: int32 [m] or NULL; weights: float [m][ns] or NULL.
 *
 * Definition for pair j, h = step / 2 (integer division):
 *   lattice   columns x_i = h + i*step for i < sx = (W-1-h)/step + 1, rows y_r likewise with sy; ns = sx*sy, sample
 *             s = r*sx + i (row-major).  cx = (double)(W-1) / 2, cy = (double)(H-1) / 2 (exact);
 *             xc = (double)x - cx, yc = (double)y - cy.
 *   value     (u, v) = the field at the integer pixel as the view defines it (binary16 converted exactly; a level view
 *             expanded as ofdis_warp_u8 defines), converted to double.  ok = isfinite(u) && isfinite(v); with flow_bw
 *             also: ofdis_fb_check(alpha, beta)'s occ_fw code at that pixel is 0 (for a level view
 *             ofdis_fb_check_level's), evaluated at the samples alone -- no mask is written.  A sample that is not ok
 *             has u = v = 0 before any arithmetic (a select, so a NaN flow never reaches a sum).
 *   weights   solve 0: w = ok ? 1 : 0.  Solve it = 1 .. iters, with (p0 .. p3) of the solve before:
 *               t_it = tau * 2^(iters - it);  inv = 1.0 / (t_it * t_it)        (the power exact; inv computed on the host)
 *               ru = u - ((p0*xc - p1*yc) + p2);  rv = v - ((p1*xc + p0*yc) + p3);  r2 = ru*ru + rv*rv
 *               w  = ok ? fmax(1 - r2*inv, 0) : 0
 *   sums      Sw, Sx, Sy, Sr, Su, Sv, Sa, Sb of the per-sample terms w, w*xc, w*yc, w*((xc*xc)+(yc*yc)), w*u, w*v,
 *             w*((xc*u)+(yc*v)), w*((xc*v)-(yc*u)), and cnt = #{w > 0}.
 *   order     part[t] = ((0 + term[t]) + term[t + 256]) + ... for t in 0 .. OFDIS_FIT_LANES - 1 (no sample: +0.0);
 *             then for stride = 128, 64, ..., 1: part[i] = part[i] + part[i + stride] for i < stride; the sum is part[0].
 *   solve     D  = Sw*Sr - (Sx*Sx + Sy*Sy)
 *             p0 = (Sw*Sa - (Sx*Su + Sy*Sv)) / D;   p1 = (Sw*Sb - (Sx*Sv - Sy*Su)) / D
 *             p2 = (Su - (p0*Sx - p1*Sy)) / Sw;     p3 = (Sv - (p1*Sx + p0*Sy)) / Sw
 *             OFDIS_MOTION_TRANSLATION: p0 = p1 = 0.  The solve fails when cnt < 3 or !(D > 0) (translation: cnt < 1 or
 *             !(Sw > 0)).  Any failed solve ends the pair: the identity (1, 0, 0, 0, 1, 0), support 0, all weights 0.
 *   output    position in frame j + 1 = M * position in frame j:
 *             M = (1+p0, -p1, p2 - (p0*cx - p1*cy),   p1, 1+p0, p3 - (p1*cx + p0*cy)) of the last solve; support = its
 *             cnt; weights = its w as float32.
 * Consequences: zero fields give the identity; a NaN or infinite sample changes nothing but the support; the result never
 * depends on how the work is spread over the device.  Breakdown: the annealed fit is a redescending M-estimator started
 * from least squares, so it needs the dominant motion to hold a clear majority -- on an exact similarity field with 25 %
 * of the columns displaced by (10, -6), iters >= 2 at tau = 2 recovers every parameter to 5e-9 where iters = 0 misses
 * by 2; with 40 % displaced it locks on to nothing useful (error about 4).  Use the check (flow_bw) or a coarser model
 * when the foreground is that large.
 * Refused before anything is enqueued (OFDIS_ERR_INVALID_ARGUMENT, the context stays usable): whatever
 * ofdis_track_points refuses of a view and a size; NULL flow_fw, view or xform; m < 1; an unknown model; step < 1;
 * step / 2 > min(W, H) - 1; ns > OFDIS_FIT_MAX_SAMPLES; tau not finite or outside [1/1024, 65536]; iters outside 0 .. 16;
 * with flow_bw, the threshold rules of ofdis_fb_check.  Stream and ordering rules are those of ofdis_fb_check. */
enum { OFDIS_MOTION_TRANSLATION = 0, OFDIS_MOTION_SIMILARITY = 1 };
#define OFDIS_FIT_MAX_SAMPLES 65536
#define OFDIS_FIT_LANES 256 /* part of the definition: the summation order above */
int ofdis_fit_motion(ofdis_context *ctx, const void *flow_fw, const void *flow_bw, const ofdis_flow_view *view, int m,
                     int width, int height, int model, int step, double tau, int iters, float alpha, float beta,
                     double *xform, int32_t *support, float *weights, void *stream);

/* ofdis_smooth_path: the m pair transforms to m + 1 per-frame corrections, on the device.  xform: double [m][6];
 * corr: double [m + 1][6]; corr_i maps a pixel of stabilised frame i to the position in input frame i that it shows.
 *   compose(P, C):  r00 = P00*C00 + P01*C10;  r01 = P00*C01 + P01*C11;  r02 = (P00*C02 + P01*C12) + P02;  row 1 likewise
 *   path      C_0 = I;  C_{j+1} = compose(P_j, C_j)
 *   smoothing S_i, entry by entry: (sum over k = -R .. R, ascending, starting from 0.0, of g_k * C_clamp(i+k, 0, m)) / G
 *             with g_k = (double)(R+1-|k|), G = (double)((R+1)*(R+1)) -- a triangular window with integer weights
 *   inverse   det = S00*S11 - S01*S10; det zero or not finite: corr_i = I.  Else i00 = S11/det, i01 = -S01/det,
 *             i10 = -S10/det, i11 = S00/det, i02 = -(i00*S02 + i01*S12), i12 = -(i10*S02 + i11*S12)
 *   result    corr_i = compose(compose(C_i, Sinv_i), Z),  z = 1.0 / zoom,  Z = (z, 0, cx - z*cx, 0, z, cy - z*cy)
 * Refused (OFDIS_ERR_INVALID_ARGUMENT): NULL pointers, m < 1, radius outside 0 .. 256, zoom not finite or outside
 * [1, 16], a non-positive size.  The chain C lives in the context's workspace.  Stream and ordering rules are those of
 * ofdis_fb_check. */
int ofdis_smooth_path(ofdis_context *ctx, const double *xform, int m, int radius, double zoom, int width, int height,
                      double *corr, void *stream);

/* ofdis_warp_affine_u8: each of n u8 frames pulled through its own transform.  img: u8 [n][height][width][noc]; xf:
 * device double [n][6]; out: u8 or float32 (out_dtype) of img's shape; valid: u8 [n][height][width] or NULL.  Per pixel
 *   px = (float)((M00*(double)x + M01*(double)y) + M02);   py = (float)((M10*(double)x + M11*(double)y) + M12)
 * then ofdis_warp_u8's inside, clamp, taps, val, rounding and valid, verbatim, at (px, py): a replicated border, and
 * valid = 0 outside.  The identity returns the frame.
 * Refused (OFDIS_ERR_INVALID_ARGUMENT): what ofdis_warp_u8 refuses of a size, noc and out_dtype; NULL img, xf or out;
 * n < 1; out overlapping img.  Stream and ordering rules are those of ofdis_fb_check. */
int ofdis_warp_affine_u8(ofdis_context *ctx, const uint8_t *img, int n, int width, int height, int noc, const double *xf,
                         int out_dtype, void *out, uint8_t *valid, void *stream);

/* The flows of a video, its camera path and the stabilised frames from one call: frames u8 [nframes][height][width][noc],
 * m = nframes - 1.  By definition out / valid / xform / corr / support == ofdis_warp_affine_u8(frames,
 * ofdis_smooth_path(ofdis_fit_motion(F, use_fb ? B : NULL))) bit for bit, with F, B the fields of
 * ofdis_run_sequence_u8(frames, stride 1) -- but every pair's flows leave the coarse-to-fine loop as float32 level
 * grids in the buffer the context owns, and after the last chunk come three launches: the fit over all m pairs (which
 * evaluates the check at its own samples), the path, and the affine warp over all nframes frames.  No upsample runs, no
 * full-resolution field and no mask exists, and every frame's pyramid is built once.  xform [m][6], corr [nframes][6]
 * and support [m] are optional outputs; those not asked for live behind the grids in that buffer.
 * Optical flow only: OFDIS_MODE_DE returns OFDIS_ERR_UNSUPPORTED, and so does a call while a stage capture is set.  No
 * initial flow.  verbosity is ignored.  Argument errors are those of ofdis_run_sequence_track_u8 (nframes < 2, ...), of
 * the three primitives and, with use_fb, the threshold rules of ofdis_fb_check; stream, ordering, chunking, round-robin,
 * graph and workspace rules are those of ofdis_run_batch_u8 (the graph is recorded anew when an output pointer or any
 * scalar of the call changes; a graph of another call kind is never replayed). */
int ofdis_run_sequence_stabilize_u8(ofdis_context *ctx, const uint8_t *frames, int nframes, int width, int height,
                                    const ofdis_params *p, int model, int step, double tau, int iters, int use_fb,
                                    float alpha, float beta, int radius, double zoom, int out_dtype, void *out,
                                    uint8_t *valid, double *xform, double *corr, int32_t *support, void *stream);
/* Same with host buffers (synchronous). */
int ofdis_run_sequence_stabilize_u8_host(ofdis_context *ctx, const uint8_t *frames, int nframes, int width, int height,
                                         const ofdis_params *p, int model, int step, double tau, int iters, int use_fb,
                                         float alpha, float beta, int radius, double zoom, int out_dtype, void *out,
                                         uint8_t *valid, double *xform, double *corr, int32_t *support);

/* ------------------------------------------------------------------ moving-object masks
 *
 * ofdis_motion_mask answers which pixels moved on their own: per pixel the distance of the flow estimate from the
 * camera's flow there (the transform of ofdis_fit_motion), a threshold, and a binary median as clean-up.  All pointers
 * are device pointers.  flow / view: ofdis_track_points's rules -- a full view of either dtype and layout; a level view
 * must be float32 interleaved (any other valid enum value: OFDIS_ERR_UNSUPPORTED) and stands for the float32 field it
 * expands to, as ofdis_warp_u8 defines.  xform: double [m][6] = (M00, M01, M02, M10, M11, M12), a position in frame j to
 * frame j + 1.  occ: u8 [m][height][width] or NULL, ofdis_fb_check's occ_fw plane.  code: u8 [m][height][width]; res:
 * float32 [m][height][width]; stats: int64 [m][OFDIS_MM_NSTATS]; each may be NULL, not all three.
 *
 * Per pixel (x, y) with the estimate (u, v) as float32 (binary16 converted exactly), every operation rounded on its own
 * (no fused multiply-add), sqrtf correctly rounded:
 *   pu = (float)(((M00 * (double)x + M01 * (double)y) + M02) - (double)x)     the bracket in float64
 *   pv = (float)(((M10 * (double)x + M11 * (double)y) + M12) - (double)y)
 *   du = u - pu;  dv = v - pv;  e = sqrtf(du * du + dv * dv);  g = sqrtf(pu * pu + pv * pv)
 *   fin = isfinite(u) && isfinite(v);  e = fin ? e : +inf                    (a select after the test)
 *   unknown = !fin || (occ != NULL && occ byte != 0)
 *   b = !unknown && e > thr && e > rel * g                                   (false for a NaN e)
 * Clean-up: over the (2 radius + 1)^2 window clipped to the frame (in-frame pixels only, no border replication), mov =
 * the window pixels with b set, known = those that are not unknown, c = 2 * mov > known in integers; radius 0 gives
 * c = b.
 *   code = unknown ? 2 : (c ? 1 : 0)       the 0 / 1 / 2 conventions of the occlusion masks
 *   res  = e                               +inf at a non-finite estimate, the canonical quiet NaN (0x7fc00000) for a NaN;
 *                                          independent of occ and of the clean-up
 *   stats of a pair, exact integers (any accumulation order gives the same values):
 *     [0], [1], [2]   the counts of codes 0, 1, 2
 *     [3] .. [6]      xmin, ymin, xmax, ymax of code 1; width, height, -1, -1 when there is none
 *     [7]             the count of b, before the clean-up
 *     [8], [9]        the sums of x and of y over code 1
 *     [10], [11]      0
 * Consequences: an exact similarity field under its own transform gives res of a few ulp of the flow's magnitude and
 * all zeros in code; a NaN transform entry makes e NaN, hence b false and code 0 (2 where unknown), and res holds the
 * NaN; rel plays the role of the 0.05 relative term in KITTI's Fl rule (a pixel of a fast pan moves on its own only if
 * its residual also exceeds rel times the camera's flow there).
 * Refused before anything is enqueued with OFDIS_ERR_INVALID_ARGUMENT (the context stays usable): whatever
 * ofdis_track_points refuses of a view and a size; NULL ctx, flow, view or xform; all three outputs NULL; m < 1; thr not
 * finite or outside [0, 65536]; rel not finite or outside [0, 16]; radius outside 0 .. 4; width * height >= 2^31.
 * Stream and ordering rules are those of ofdis_fb_check; stats is reset on the stream before the kernel. */
#define OFDIS_MM_NSTATS 12
int ofdis_motion_mask(ofdis_context *ctx, const void *flow, const ofdis_flow_view *view, int m, int width, int height,
                      const double *xform, const uint8_t *occ, float thr, float rel, int radius, uint8_t *code,
                      float *res, int64_t *stats, void *stream);

/* The flows of a video, its camera motion and the moving-object masks from one call: frames u8
 * [nframes][height][width][noc], m = nframes - 1.  By definition code / res / stats / xform / support / occ ==
 * ofdis_motion_mask(F, ofdis_fit_motion(F, use_fb ? B : NULL), use_fb ? occ_fw of ofdis_fb_check(F, B) : NULL) bit for
 * bit, with F, B the fields of ofdis_run_sequence_u8(frames, stride 1) -- but every pair's flows leave the
 * coarse-to-fine loop as float32 level grids in the buffer the context owns (without use_fb the forward chain alone is
 * computed), and after the last chunk come the launches: the fit over all m pairs, with use_fb one ofdis_fb_check_level
 * launch that writes occ_fw, and the mask kernel on the grids over all m pairs.  No upsample runs and no
 * full-resolution flow exists.  xform [m][6], support [m] and occ [m][height][width] (written with use_fb alone) are
 * optional outputs; those not asked for live behind the grids in that buffer.
 * Optical flow only: OFDIS_MODE_DE returns OFDIS_ERR_UNSUPPORTED, and so does a call while a stage capture is set.  No
 * initial flow.  verbosity is ignored.  Argument errors are those of ofdis_run_sequence_stabilize_u8's fit part
 * (nframes < 2, the fit's scalars, with use_fb the threshold rules of ofdis_fb_check) and of ofdis_motion_mask; stream,
 * ordering, chunking, round-robin, graph and workspace rules are those of ofdis_run_batch_u8 (the graph is recorded anew
 * when an output pointer or any scalar of the call changes; a graph of another call kind is never replayed). */
int ofdis_run_sequence_motion_mask_u8(ofdis_context *ctx, const uint8_t *frames, int nframes, int width, int height,
                                      const ofdis_params *p, int model, int step, double tau, int iters, int use_fb,
                                      float alpha, float beta, float thr, float rel, int radius, uint8_t *code,
                                      float *res, int64_t *stats, double *xform, int32_t *support, uint8_t *occ,
                                      void *stream);
/* Same with host buffers (synchronous). */
int ofdis_run_sequence_motion_mask_u8_host(ofdis_context *ctx, const uint8_t *frames, int nframes, int width, int height,
                                           const ofdis_params *p, int model, int step, double tau, int iters,
                                           int use_fb, float alpha, float beta, float thr, float rel, int radius,
                                           uint8_t *code, float *res, int64_t *stats, double *xform, int32_t *support,
                                           uint8_t *occ);

/* ------------------------------------------------------------------ flow error against ground truth
 *
 * ofdis_flow_error scores n flow fields against n ground-truth fields on the device: the end-point error (EPE) sums,
 * outlier counts, KITTI's Fl count, Sintel's speed classes, optionally the per-pixel error map and a histogram.  The
 * definition fixes every operation and the order of every float64 sum, so the 16 numbers per pair are a pure function
 * of the inputs, whatever the device does with the work (tests/test_flow_error.py restates it in numpy).
 *
 * flow / view: ofdis_track_points's rules -- a full view of either dtype and layout, or a level view that is float32
 * interleaved (any other valid dtype / layout in a level view: OFDIS_ERR_UNSUPPORTED).  A level view stands for the
 * float32 field it expands to, bit for bit, as ofdis_warp_u8 defines.  gt: float32 [n][H][W][2] -- the truth, or any
 * other flow of a run when two estimates are compared.  mask: u8 [n][H][W] or NULL.  stats: double
 * [n][OFDIS_FE_NSTATS].  err: float32 [n][H][W] or NULL.  hist: uint32 [n][OFDIS_FE_BINS] or NULL.  All device
 * pointers.
 *
 * Per pixel, with (u, v) the estimate as float32 (binary16 converted exactly), (gu, gv) the truth and m the mask
 * byte; all arithmetic float32, every operation rounded on its own (no fused multiply-add), sqrtf correctly rounded:
 *   known   = fabsf(gu) <= 1e9f && fabsf(gv) <= 1e9f          (false for NaN; .flo files mark unknown flow with 1e10)
 *   pass    = mask == NULL || (mask_eq < 0 ? m != 0 : m == mask_eq)
 *             (mask_eq 0 with an occlusion mask of ofdis_run_bidir_u8: the consistent pixels, "EPE-noc"; -1 with a
 *             KITTI-style valid mask: its nonzero pixels)
 *   ok      = known && pass
 *   fin     = isfinite(u) && isfinite(v)
 *   du = u - gu;  dv = v - gv;  e = sqrtf(du * du + dv * dv);  g = sqrtf(gu * gu + gv * gv)
 *   e       = fin ? e : +inf       (a select after the test: a non-finite estimate never reaches a sum)
 *   counted = ok && fin
 * stats of a pair (all counts exact integers stored as doubles):
 *   [0] cnt = #ok                        [1] nonfinite = #(ok && !fin)
 *   [2] Se = sum over counted of (double)e                [3] emax = max over counted of e (0 if none)
 *   [4] #(ok && e > 1)   [5] #(ok && e > 3)   [6] #(ok && e > 5)      (a non-finite estimate counts in all three)
 *   [7] fl = #(ok && e > 3 && e > 0.05f * g)              (KITTI's outlier rule without the division)
 *   [8], [9]   count and sum of (double)e over counted pixels with g < 10
 *   [10], [11] the same with 10 <= g < 40       [12], [13] the same with g >= 40       (Sintel's speed classes)
 *   [14], [15] 0
 * err: e at counted pixels, +inf where ok && !fin, -1 where !ok.
 * hist: over ok pixels, bin e < 64 ? (int)(e * 16.0f) : OFDIS_FE_BINS - 1 -- bin 1023 also holds everything from
 * 63.9375 px up and every non-finite estimate.  Integer counts: any order.
 *
 * Order of the four float64 sums ([2], [9], [11], [13]), L = OFDIS_FE_LANES.  A row y: for t in 0 .. L - 1,
 * part[t] = ((0.0 + term(t)) + term(t + L)) + ... over the columns x = t + L k < W in ascending k; then for stride =
 * L / 2, L / 4, ..., 1: part[i] = part[i] + part[i + stride] for every i < stride; the row's sum is part[0].  The
 * frame: the same scheme over the row sums -- part[t] = ((0.0 + row[t]) + row[t + L]) + ..., the same tree, the sum is
 * part[0].  A pixel that is not counted contributes nothing (every term is >= 0, so adding +0.0 for it gives the same
 * bits).  No angular error: it needs acos, which numpy and the device do not share bit for bit.
 *
 * Refused before anything is enqueued (OFDIS_ERR_INVALID_ARGUMENT, the context stays usable): what
 * ofdis_track_points refuses of a view and a size, NULL ctx / flow / view / gt / stats, n < 1, mask_eq outside
 * -1 .. 255, width * height >= 2^31.  Stream and ordering rules are those of ofdis_fb_check; the per-row partial sums
 * live in the context's workspace.  Timers "flow_error" (full views) / "flow_error_level" (level views) and
 * "flow_error_sum" (the per-row partials to the 16 numbers). */
#define OFDIS_FE_LANES  64     /* part of the definition: the summation order */
#define OFDIS_FE_NSTATS 16
#define OFDIS_FE_BINS   1024
int ofdis_flow_error(ofdis_context *ctx, const void *flow, const ofdis_flow_view *view, const float *gt,
                     const uint8_t *mask, int mask_eq, int n, int width, int height,
                     double *stats, float *err, uint32_t *hist, void *stream);
/* Flow and its error in one call: by definition ofdis_flow_error(ofdis_run_batch_u8(img_a, img_b), gt, ...) bit for
 * bit.  The flow leaves the coarse-to-fine loop as the float32 level grid in the buffer the context owns, and the error
 * launches follow the last chunk; no upsample runs and no full-resolution flow exists.  Optical flow only:
 * OFDIS_MODE_DE returns OFDIS_ERR_UNSUPPORTED.  No initial flow.  A set stage capture is honoured as in
 * ofdis_run_warp_u8.  Argument errors are those of ofdis_run_batch_u8 and of ofdis_flow_error; stream, ordering,
 * chunking, round-robin, graph and workspace rules are those of ofdis_run_batch_u8 (the graph is recorded anew when an
 * output pointer, the mask or mask_eq changes; a graph of another call kind is never replayed). */
int ofdis_run_error_u8(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, const float *gt,
                       const uint8_t *mask, int mask_eq, int n, int width, int height, const ofdis_params *p,
                       double *stats, float *err, uint32_t *hist, void *stream);
/* Same with host buffers (synchronous). */
int ofdis_run_error_u8_host(ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, const float *gt,
                            const uint8_t *mask, int mask_eq, int n, int width, int height, const ofdis_params *p,
                            double *stats, float *err, uint32_t *hist);

/* Device pyramid only (run_dense.cpp:131-179 + :299-312): writes, for each level s in [sc_l, sc_f],
 * padded image/dx/dy of frame 0 to host arrays (same layout as ofdis_oflow_compute's inputs). */
int ofdis_pyramid_u8_host(ofdis_context *ctx, const uint8_t *img, int width, int height, const ofdis_params *p,
                          int imgpadding, float *const *img_pyr, float *const *dx_pyr, float *const *dy_pyr);

/* Per-stage capture for parity tests: when set, the next run copies frame 0's flow at scale s after
 * patch aggregation (dis_flow[s]) and after variational refinement (tv_flow[s]), each
 * w_s*h_s*nop interleaved floats, into these host arrays (entries may be NULL).  A capturing run issues
 * the whole batch as one launch on one stream whatever the "streams" / "chunk" options; a batch larger
 * than ofdis_max_frames_per_launch() returns OFDIS_ERR_UNSUPPORTED while a capture is set. */
int ofdis_context_set_stage_capture(ofdis_context *ctx, float *const *dis_flow, float *const *tv_flow, int nscales);

/* Tuning / A-B switches:
 *   "sor_generic" (0/1): force the generic global-memory SOR wavefront;
 *   "sor_pipe" (0/1):    force the one-wave-per-row-group register pipeline (the default for tall levels)
 *                        instead of the sweep-per-wave SOR;
 *   "sor_cring" (0..3, default 2): in the sweep-per-wave SOR, sweep 0 loads each pixel's coefficients once and
 *                        hands them to the later sweeps through LDS (solverit <= 3); 2: the LDS ring sized to
 *                        the level's rows (more frames per CU at 3 sweeps), and in launches with more frames than
 *                        CUs the lanes outside the frame load a slot of their wave's in-frame run (fewer fetched
 *                        lines, one v_med3 per load); 3: that load form in every launch; 1: sized to the
 *                        workgroup limit;
 *   "sor_pack" (0..2, default 1): the sweep-per-wave SOR lays the rows of several frames end to end in one
 *                        workgroup, so that levels of up to 128 rows fill their 64-lane waves (2 or 3 sweeps with
 *                        the coefficient ring, where that saves a quarter of the waves or more); 1: in launches
 *                        with more frames than CUs; 2: in every launch; 0: one frame per workgroup.  Same bits;
 *   "sor_rows2" (0/1, default 1): levels too tall for one row per lane in a 1024-thread workgroup run the
 *                        sweep-per-wave SOR with two rows per lane -- 321..640 rows at 3 sweeps, 513..1024 at
 *                        2 (else the register pipeline);
 *   "smsys" (0/1, default 1): smoothness and system of a TV iteration in one launch;
 *   "smsys2d" (0/1/2, default 2): the fused launch on 2-D tiles for levels taller than 256 rows (0: two
 *                        launches there; 2 = automatic: on for calls of fewer than 512 pairs);
 *   "smsys_prefetch" (0/1, default 1): the fused launch (levels up to 256 rows, intensity images) issues a
 *                        thread's derivative-image loads before the staging, not after two barriers;
 *   "smsys_small" (0/1, default 1): a fused launch that cannot fill the chip (fewer than 4096 row blocks:
 *                        a few pairs per call) takes ~1 pixel per thread (>= 4 rows per block) instead of 4;
 *   "smsys_deriv" (0/1, default 1): where "prepd" and the fused launch (levels up to 256 rows, intensity images)
 *                        or the register march (taller levels, intensity and colour images) run, the system kernel
 *                        filters Ixx, Ixy, Iyy, Ixz, Iyz from Ix, Iy, Iz and the prep launch does not write those
 *                        five planes (per channel);
 *   "pyr_rgb" (0/1, default 1): colour images, pyramid base levels 2..4: dword loads and per-channel masked byte
 *                        sums (v_sad_u8) instead of the byte loop;
 *   "pad_grad_v" (0/1, default 1): colour images: the pyramid's pad + Sobel launch runs one thread per value
 *                        (0: one per pixel, the channels inside the thread);
 *   "agg_stage" (0/1, default 1): the aggregation stages the displacements of the patches covering each 64 x 16
 *                        tile in LDS (0: every pixel gathers them from the patch array);
 *   "prepd_df" (0/1, default 1): on those levels the prep launch warps a 2-pixel halo with every channel in one pass
 *                        and writes Ix, Iy, It only (k_tv_prepd_df; 0: intensity images run k_tv_prepd on its 4-pixel
 *                        halo, colour images k_tv_prepd_c3, which writes all eight derivative planes);
 *   "smsys_march" (0/1, default 1): levels taller than 256 rows run smoothness + system as a register march
 *                        (one wave per 60 columns x 64 rows, no LDS; takes precedence over smsys2d);
 *   "prepd" (0..2, default 2): image warp, temporal images and the derivative filters of a level in one launch
 *                        (1: intensity images only, colour images in three launches; 0: three launches);
 *   "sor_mode" (0/1, default 0): 0 = sor_coupled's exact lexicographic order (the reference's bits);
 *                        1 = the latency mode, red-black order (every half-sweep fully parallel):
 *                        levels of at most 8192 pixels run their whole inner loop -- smoothness, system, 2 x solverit
 *                        half-sweeps per inner iteration -- and the flow update in one launch of one workgroup per
 *                        frame (k_tv_level_rb), larger levels the system launches and one launch per half-sweep.
 *                        A different iteration -- NOT the reference's bits: bit-exact against the oracle's
 *                        red-black restatement, end-point error gated against the exact path; the one option
 *                        that changes results.  For calls that cannot fill the chip (one pair, a few dozen);
 *   "wave_per_patch" (0/1): one wave64 per patch instead of eight lanes per patch (patches of at most
 *                        448 values; larger ones always run the any-shape kernel);
 *   "patch_window" (0/1, default 1): p = 8 / 12 patches read their bilinear taps from an LDS copy of the
 *                        sample window (0: eight-lane patches gathering the taps from the L1 cache);
 *   "patch_quad" (0/1, default 1): windowed gray patches (p = 8 / 12) on four lanes per patch, the Eigen
 *                        slot pairs packed (0: eight lanes per patch);
 *   "patch_x16" (0..2, default 1): windowed RGB p = 12 patches on sixteen lanes per patch, the Eigen slot chains
 *                        folded in block order on eight owner lanes (0: eight lanes per patch; 2: sixteen lanes,
 *                        every evaluation on the exact square-root form -- parity testing of the fallback);
 *   "patch_absw" (0/1, default 1): without usefbcon, the four- and sixteen-lane patch kernels store each patch
 *                        pixel's aggregation weight into slot planes ([n][A*A][h][w], A = (p-1)/steps + 1) instead
 *                        of their loss weights, so the aggregation reads coalesced plane rows (0: loss weights);
 *   "patch_buf" (0/1, default 1): gray p = 12 patch windows by buffer loads with 32-bit offsets where the level's
 *                        image array spans less than 4 GiB (0: 64-bit address arithmetic per load);
 *   "patch_fdiv" (0/1, default 1): the 2x2 / 1x1 LLT solves of every patch iteration divide by one correctly
 *                        rounded reciprocal of each pivot per patch plus two FMAs (exact by Markstein's theorem in
 *                        the range the kernels check; tools/divcheck_l.c), IEEE divisions outside it (0: IEEE always);
 *   "patch_maxres" (0/1, default 1): with res_thresh = 0 and min_iter >= max_iter (every op-point) the four- and
 *                        sixteen-lane patch kernels stop on the largest |w| of an evaluation being 0 instead of
 *                        summing |w| (the same decision; NaN and tiny terms redo the evaluation with the sum);
 *   "patch_generic" (0/1, default 0): every patch shape on the any-shape kernel (runtime value loops: the
 *                        default for p*p*noc > 448, e.g. RGB p >= 14, gray p >= 22);
 *   "nt_store" (0/1, default 0): write the full-resolution flow with non-temporal stores (the plain format);
 *   "up_form" (0..3, default 3): optical-flow upsample: 1 / 2 = each staged source row's horizontal taps once per
 *                        column for blocks of 4 / 8 output rows, 0 = once per output row that reads them (round 4),
 *                        3 = 1 on frames at least 1024 wide for calls on two or more streams or of fewer than
 *                        1024 pairs, else 0 (the faster of the two end to end in each measured regime); the other
 *                        output formats have one store form each and ignore it;
 *   "graph" (0/1/2, default 1): replay a batch as one captured HIP graph while its pointers, sizes and
 *                        parameters repeat (re-captured when they change); 1 captures single-stream
 *                        batches, 2 also the multi-stream ones (chunks forked over lanes and joined);
 *   "streams" (0-16, default 0 = automatic: 2 from 256 pairs, else 1): a batch is cut into chunks that run
 *                        round-robin on that many HIP streams with separate workspaces, overlapping one
 *                        chunk's latency-bound wavefront with another's streaming kernels (1 stream and
 *                        several chunks: the chunks run one after the other);
 *   "chunk" (frames per chunk, 0 to 2^30, default 0 = the batch split evenly over the streams);
 * Setting any option drops the captured graph.  Unknown keys and out-of-range values return
 * OFDIS_ERR_INVALID_ARGUMENT.  Apart from "sor_mode", results never depend on these settings. */
int ofdis_context_set_option(ofdis_context *ctx, const char *key, int value);

/* Largest number of frame pairs one launch takes at this size; larger batches are chunked.  Two rules, the smaller
 * one holds.  The refinement kernels address their plane groups with 32-bit offsets: frames * noc * plane < 2^30
 * floats (with usetvref 0 this rule sets no bound).  And no launch puts more than 65535 in grid y or z: a pair is two
 * frames of the pyramid kernels' grid z, and with the refinement on, noc rows of its derivative launches' grid y, so
 * at most 65535 / max(2, noc) pairs (32767 grey, 21845 colour).  A stereo call takes half of this value in stereo
 * pairs; a sequence chunk of m pairs builds m + stride frames, so its bound is min(plane rule, 65535 / noc
 * with the refinement on, 65535 - stride) pairs.  An explicit "chunk" option above the bound is clamped to it.
 * A size at which one frame alone exceeds that (e.g. ~20k x 20k RGB with sc_l 0) returns
 * OFDIS_ERR_INVALID_ARGUMENT here and from every run entry point. */
int ofdis_max_frames_per_launch(const ofdis_params *p, int width, int height, int *frames);

/* HIP-event timing of individual kernels on the launch stream (used by bench.py for the roofline). */
int ofdis_context_enable_kernel_timing(ofdis_context *ctx, int enable);
/* Accumulated device time (ms) and launch count for kernel `name` since timing was enabled. */
int ofdis_context_kernel_time(ofdis_context *ctx, const char *name, double *total_ms, long *launches);
/* Comma-separated list of kernel names known to the timer.  The forward-backward check is timed as "fb_check"
 * when it writes masks only and as "fb_check_err" when it also writes an error map; the upsample as "upsample" when
 * it writes the plain format alone, else as "upsample_f16", "upsample_planar" or "upsample_planar_f16", and the
 * level-grid output that replaces it as "level_out"; the warp as "warp" with a full-resolution flow view and as
 * "warp_level" with a level-grid view; the left-right check as "lr_check" / "lr_check_err" like the forward-backward
 * one; the interpolation as "interp" with full-resolution flow views and as "interp_level" with level-grid views; the
 * forward-backward check on level grids as "fb_check_level", whatever it writes; the point tracker as "track" with
 * full-resolution flow views and as "track_level" with level-grid views; the temporal filter as "tfilter" with
 * full-resolution flow views and as "tfilter_level" with level-grid views; the motion fit as "fit_motion" with
 * full-resolution flow views and as "fit_motion_level" with level-grid views, the path kernel as "smooth_path" and the
 * affine warp as "warp_affine"; the temporal filter over a radius as "tfilter_radius" with full-resolution flow views
 * and as "tfilter_radius_level" with level-grid views. */
const char *ofdis_kernel_names(void);
/* The names added after those of ofdis_kernel_names (whose list is closed: callers count it), comma-separated, in
 * timer-slot order; ofdis_context_kernel_time and ofdis_algorithmic_bytes know both lists.  The flow error as
 * "flow_error" with a full-resolution flow view and as "flow_error_level" with a level-grid view, and the reduction of
 * its per-row partial sums as "flow_error_sum". */
const char *ofdis_kernel_names_ext(void);
/* Every timer name, comma-separated, in slot order: the two lists above and whatever later features add.  This list
 * is open -- callers look names up in it and do not count it.  After the two lists: the motion mask as "motion_mask"
 * with a full-resolution flow view and as "motion_mask_level" with a level-grid view (the reset of `stats` included). */
const char *ofdis_kernel_names_all(void);

/* Per-frame algorithmic byte counts of the §8(d) byte model for this workload.  The output kernels: the
 * bytes written ("level_out": the float32 level plane read and a float32 write).  "warp" / "warp_level": p->noc bytes
 * of image read per pixel, the flow view (8 bytes per pixel; the level grid's gw * gh * 2 * 4 bytes per frame), noc
 * bytes of u8 output and the mask byte -- the float32 views and the u8 output with its mask, as ofdis_run_warp_u8
 * issues them.  "lr_check" / "lr_check_err": both views, the pixel's own disparity and the gathered one (8 bytes), the
 * mask byte, and the 4-byte error with "lr_check_err" -- 2 * W * H * (8 + 1 [+ 4]).  "interp" / "interp_level": per
 * intermediate frame (the function has no nt argument; a call with nt times reads its flows once and does the rest nt
 * times): the two float32 flow views (16 bytes per pixel; the two level grids' 2 * gw * gh * 8 bytes per pair), 2 noc
 * bytes of image read, noc bytes of u8 output and the mask byte per pixel -- W * H * (16 + 3 noc + 1) and
 * 2 * gw * gh * 8 + W * H * (3 noc + 1).  "fb_check_level": both grids once, the mask byte and the 4-byte error per
 * pixel and direction -- 2 * gw * gh * 8 + 2 * W * H * (1 + 4).  "tfilter" / "tfilter_level": per output frame with
 * both neighbours, in "interp"'s convention (masks not counted): the two float32 flow views (16 bytes per pixel; two
 * level grids, 2 * gw * gh * 8 bytes), 3 noc bytes of image read (the frame and its two neighbours), noc bytes of u8
 * output and the `used` byte per pixel -- W * H * (16 + 4 noc + 1) and 2 * gw * gh * 8 + W * H * (4 noc + 1).
 * "fit_motion" / "fit_motion_level": per pair at the default lattice (step 16, ns samples; the check's gather not
 * counted): the 8-byte value of a float32 view per sample, ns * 8; of a level grid the up to nine 8-byte cells a
 * sample's expansion reads, ns * 72.  "smooth_path": six doubles per pair in and per frame out, 96.  "warp_affine": per
 * frame, noc bytes of image read, noc bytes of u8 output and the mask byte per pixel and the six doubles --
 * W * H * (2 noc + 1) + 48.  "tfilter_radius" / "tfilter_radius_level": ofdis_tfilter_radius_bytes at radius 1 with a
 * u8 picture (the counts of "tfilter" / "tfilter_level").  "flow_error" / "flow_error_level": per pair, the float32
 * estimate and the truth, W * H * 16 (the function has no mask argument: the mask byte, the error map and the
 * histogram are not counted); with a level grid gw * gh * 8 + W * H * 8.  "flow_error_sum": the per-row partials read
 * and the 16 doubles written, H * 80 + 128.  "motion_mask" / "motion_mask_level": per pair, the float32 estimate and
 * the code byte, W * H * 9 (the function has no argument for them: the occlusion byte, one more per pixel, the residual
 * map, four more, and the statistics are not counted); with a level grid gw * gh * 8 + W * H. */
int ofdis_algorithmic_bytes(const ofdis_params *p, int width, int height, const char *kernel, double *bytes_per_frame);
/* The same model for the temporal filter over a radius R (ofdis_tfilter_radius_u8), which depends on R and on the
 * picture's dtype: per interior output frame, in "tfilter"'s convention, each of the 2 R steps reads one field once (8
 * bytes per pixel of a full-resolution float32 view, or one level grid; the check's gathers are not counted, as in
 * "track") and one neighbour's taps (noc), plus the frame itself (noc), the picture (noc as u8, 4 noc as float32) and
 * the `used` byte -- W * H * (16 R + (2 R + 2) noc + 1) with full-resolution views (level = 0) and
 * 2 R * gw * gh * 8 + W * H * ((2 R + 2) noc + 1) with level grids (level != 0); a float32 picture has 4 noc in place
 * of the output's noc.  radius outside [1, 4] or an unknown out_dtype: OFDIS_ERR_INVALID_ARGUMENT. */
int ofdis_tfilter_radius_bytes(const ofdis_params *p, int width, int height, int level, int radius, int out_dtype,
                               double *bytes_per_frame);

/* ------------------------------------------------------------------ files and inputs */

/* SaveFlowFile (run_dense.cpp:17-58): "PIEH", int32 w, int32 h, w*h*nc float32 row-major. */
int ofdis_write_flo(const char *path, const float *flow, int width, int height, int nc);
/* SavePFMFile (run_dense.cpp:61-82): "Pf\n%d %d\n%f\n" with -1.0, rows bottom-up, values negated. */
int ofdis_write_pfm(const char *path, const float *depth, int width, int height);
/* ReadFlowFile (run_dense.cpp:85-129). w/h out; flow may be NULL to query the size. */
int ofdis_read_flo(const char *path, float *flow, int *width, int *height, int nc);
/* Binary PGM (P5, noc = 1) / PPM (P6, noc = 3, returned in BGR order like cv::imread). */
int ofdis_read_pnm(const char *path, uint8_t *pixels, int *width, int *height, int *noc, size_t capacity);
/* Binary PGM (P5, noc = 1) / PPM (P6, noc = 3: pixels in BGR order, written as RGB) -- the inverse of ofdis_read_pnm. */
int ofdis_write_pnm(const char *path, const uint8_t *pixels, int width, int height, int noc);
/* cv::imread(path, want_noc == 1 ? CV_LOAD_IMAGE_GRAYSCALE : CV_LOAD_IMAGE_COLOR) (run_dense.cpp:202-206)
 * for PNG (zlib inflate; gray / RGB / palette / alpha, 1-16 bit, Adam7; libpng's transform chain as
 * OpenCV configures it, incl. png_set_rgb_to_gray(0.299, 0.587)) and Netpbm P1-P6 (colour -> gray with
 * OpenCV's fixed-point BGR2Gray) and BMP (BmpDecoder: 1/4/8-bit palette, 16-bit 555 / 565, 24-bit, 32-bit,
 * core / info / V4 / V5 headers, bottom-up or top-down; colour -> gray by the same BGR2Gray).  Output
 * [h][w][want_noc], BGR for 3.  pixels may be NULL to query the size (PNG: from the checked chunk structure and
 * header, nothing inflated; a corrupt stream then fails the pixel call).  OFDIS_ERR_UNSUPPORTED for other formats
 * (JPEG, TIFF, RLE-compressed BMP, ...), OFDIS_ERR_IO for corrupt files. */
int ofdis_read_image(const char *path, uint8_t *pixels, int *width, int *height, int want_noc, size_t capacity);

/* Deterministic synthetic frame pair: band-limited texture + noise, frame b is frame
 * a moved along a known smooth flow (OF) or a horizontal disparity (DE).  Host buffers [h][w][noc]. */
int ofdis_synth_pair_u8(uint8_t *img_a, uint8_t *img_b, int width, int height, int noc, int frame, int mode);
/* The same texture and noise, frame b a pure translation of frame a: b(x, y) = a(x - sx, y - sy), i.e. the
 * true flow is (sx, sy) at every pixel (the known-answer setups of SURVEY §4). */
int ofdis_synth_shift_pair_u8(uint8_t *img_a, uint8_t *img_b, int width, int height, int noc, int frame, float sx,
                              float sy);

#ifdef __cplusplus
}
#endif

#endif /* OFDIS_H */

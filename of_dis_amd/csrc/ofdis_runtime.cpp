// ofdis_runtime.cpp -- contexts, device workspace planning and the coarse-to-fine driver
// (the OFClass constructor, oflow.cpp:31-338, restated for batches of frame pairs on one MI355X).
//
// One context per GPU.  A batch of n frame pairs is processed level by level; every kernel carries
// the frame index in its grid, so even the 30x17 coarsest level of a 1080p frame fills the chip when
// n is large.  All launches go to one stream; nothing synchronises the host unless a capture, the
// verbosity timers or a host-buffer entry point asks for it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ofdis.h"
#include "ofdis_internal.h"
#include "ofdis_motion_host.h"

using namespace ofdis;

namespace {

const char *const kKernelNames[] = {"pyr_base", "pyr_down", "pyr_pad_grad", "patch",    "aggregate", "tv_prep",
                                    "tv_deriv", "tv_system", "tv_sor",       "tv_final", "upsample",  "tv_level",
                                    "fb_check", "fb_check_err",
                                    // the upsample writing an output format other than the plain one, and the
                                    // level-grid output that replaces it ("upsample": the plain format alone)
                                    "upsample_f16", "upsample_planar", "upsample_planar_f16", "level_out",
                                    // the warp with a full-resolution flow view / with a level-grid view
                                    "warp", "warp_level",
                                    // the left-right check writing masks only / also an error map
                                    "lr_check", "lr_check_err",
                                    // the interpolation with full-resolution flow views / with level-grid views
                                    "interp", "interp_level",
                                    // the forward-backward check on two level grids
                                    "fb_check_level",
                                    // the point tracker on full-resolution fields / on level grids
                                    "track", "track_level",
                                    // the temporal filter on full-resolution fields / on level grids
                                    "tfilter", "tfilter_level",
                                    // the motion fit on full-resolution fields / on level grids, the path kernel
                                    // and the affine warp
                                    "fit_motion", "fit_motion_level", "smooth_path", "warp_affine",
                                    // the temporal filter over a radius on full-resolution fields / on level grids
                                    "tfilter_radius", "tfilter_radius_level"};
// The names after those (ofdis_kernel_names_ext): timer slots continue where kKernelNames ends.  The flow error on
// full-resolution fields / on level grids, and the reduction of its per-row partials
const char *const kKernelNamesExt[] = {"flow_error", "flow_error_level", "flow_error_sum"};
constexpr int kNumKernelNames = (int)(sizeof(kKernelNames) / sizeof(kKernelNames[0]));
constexpr int kSlotFlowError = kNumKernelNames, kSlotFlowErrorLevel = kNumKernelNames + 1,
              kSlotFlowErrorSum = kNumKernelNames + 2;
// The names after both lists (ofdis_kernel_names_ext is closed at its three as well; ofdis_kernel_names_all lists every
// slot and stays open).  The motion mask on full-resolution fields / on level grids
const char *const kKernelNamesMore[] = {"motion_mask", "motion_mask_level"};
constexpr int kNumKernelNamesExt = (int)(sizeof(kKernelNamesExt) / sizeof(kKernelNamesExt[0]));
constexpr int kSlotMotionMask = kNumKernelNames + kNumKernelNamesExt, kSlotMotionMaskLevel = kSlotMotionMask + 1;

// Output format of a call's forward flow (ofdis_out_format, validated); all zero: the plain format.
struct OutFmt {
  int f16 = 0, planar = 0, level = 0;
  bool plain() const { return !f16 && !planar && !level; }
};

struct Plan {
  // n pairs over nfr pyramid frames, frame b of pair f lying bdist frames after its frame a: two arrays of n frames
  // (nfr = 2n, bdist = n), or one sequence of n + stride frames (bdist = stride; ofdis_run_sequence_u8)
  int nfr = 0, bdist = 0;
  bool seq = false;
  // ofdis_run_stereo_u8: n = 2m flow pairs of m stereo pairs -- pair i is (left i, right i), pair m + i is (mirrored
  // right i, mirrored left i) -- over nfr = 4m frames laid out left, mirrored right, right, mirrored left (bdist = 2m)
  bool stereo = false;
  int n = 0, W0 = 0, H0 = 0, Wp = 0, Hp = 0, padl = 0, padt = 0, padw = 0, padh = 0;
  int nop = 2, noc = 1, pad = 8, sc_f = 0, sc_l = 0;
  std::vector<LevelGeom> lv;                       // index s - sc_l
  std::vector<size_t> off_lvl, off_img, off_dx, off_dy, off_flow, off_flow_bw;
  size_t off_piter = 0, off_pw = 0, off_piter_bw = 0, off_pw_bw = 0, off_tv = 0, tv_plane = 0;
  size_t off_init = 0;  // initial flow at the coarsest scale - 1, [n][Hp >> (sc_f+1)][Wp >> (sc_f+1)][nop]
  bool init = false;    // an initial flow is given: divisibility 2^(sc_f+1) (run_dense.cpp:302)
  bool fb = false;      // usefbcon: backward grid, flow and refinement
  bool bidir = false;   // ofdis_run_bidir_u8: the backward grid, flow and refinement at every level, sc_l included
  size_t off_up_bw = 0; // bidir without a caller's flow_bw: the full-resolution backward flow [n][H0][W0][2];
                        // stereo without a caller's disp_r: the right view's disparity [n / 2][H0][W0];
                        // an interpolation with masks: the chunk's two masks, u8 [2][n][H0][W0]
  bool gradmag = false; // SELECTCHANNEL 2: float level 0 (gradient magnitude) halved down to sc_l
  size_t off_gm = 0;    // its scratch: [nfr][Hp][Wp] + [nfr][Hp/2][Wp/2] (ping-pong)
  size_t total = 0;
};

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// Skewed TV plane: w * h slots when the anti-diagonal rows fold modulo w (h <= w), else (w + h - 1) * h,
// plus 64 per-lane dump slots for the SOR kernels; a multiple of 4 floats (16-byte AoS coefficients).
inline long skew_plane(int w, int h) {
  const long slots = h <= w ? (long)w * h : (long)(w + h - 1) * h;
  return (slots + 64 + 3) / 4 * 4;
}

}  // namespace

struct ofdis_context {
  int device = 0;
  hipStream_t stream = nullptr;
  char *ws = nullptr;
  size_t ws_cap = 0;
  // ofdis_run_warp_u8: the call's flow as the float32 level grid, [n] x bytes_per_pair (ofdis_out_geometry);
  // ofdis_run_interp_u8: the forward grids of the n pairs, then their backward grids
  char *warp_buf = nullptr;
  size_t warp_cap = 0;
  // stage capture (frame 0), indexed by scale
  std::vector<float *> cap_dis, cap_tv;
  // kernel timing
  bool timing = false;
  struct Pending {
    int kernel;
    hipEvent_t a, b;
  };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> pool;
  std::map<int, std::pair<double, long>> acc;
  int opt_sor_generic = 0;
  int opt_sor_pipe = 0;  // 1: force the single-wave-per-row-group register pipeline (A/B)
  int opt_graph = 1;           // replay the whole batch as one HIP graph (captured once per shape / pointers)
  // What the one recorded graph bakes in.  The part every call has comes first (graph_key() fills all of it), then the
  // payload of the call's family alone; the whole key is zeroed before it is filled and compared bytewise, padding
  // included, and the family tag keeps the keys of two families apart whatever their payloads hold.
  struct GraphKey {
    enum Family : int { kNone = 0, kBatch, kInterp, kTrack, kTfilter, kStab, kTfilterRadius, kError, kMotionMask };
    // run_batch: ofdis_run_batch_u8*, bidir, stereo, sequence, the formatted calls and ofdis_run_warp_u8
    struct Batch {
      const void *flow_bw, *occ_fw, *occ_bw, *err_fw, *err_bw;  // the bidirectional / stereo call's extra outputs,
      float alpha, beta;                                        // its thresholds
      int bidir, stereo;                                        // and which of the two it is
      int out_f16, out_planar, out_level;  // output format: a formatted call on a plain call's buffers records anew
      int warp, warp_f32;                  // ofdis_run_warp_u8: the picture's dtype, the picture, its mask, the scale
      const void *warp_out, *warp_valid;   // (`out` and `buf` of the common part are then the level-grid buffer)
      float warp_scale;
    };
    // run_batch_interp: the pictures, their dtype and mask, the times; with masks the mask arrays and thresholds
    struct Interp {
      const void *pictures, *valid, *occ_fw, *occ_bw;
      int f32, use_occ;
      float alpha, beta;
      int nt;
      float t[kInterpMaxT];
    };
    // run_batch_track: the points, their first frames and the outputs; with use_fb the thresholds
    struct Track {
      const void *points, *start, *tracks, *status;
      int npts, flags, use_fb;
      float alpha, beta;
    };
    // run_batch_tfilter: the picture, its dtype and `used` bytes, sigma; with masks their place in the context's
    // buffer (else NULL) and the thresholds
    struct Tfilter {
      const void *picture, *used, *masks;
      int f32;
      float sigma, alpha, beta;
    };
    // run_batch_stabilize: the picture, its dtype and mask, where the transforms and supports go (the caller's arrays
    // or their place in the context's buffer), the fit's and the path's scalars; with use_fb the thresholds
    struct Stab {
      const void *picture, *valid, *xform, *corr, *support;
      int f32, model, step, iters, use_fb, radius;
      float alpha, beta;
      double tau, zoom;
    };
    // run_batch_tfilter_radius: the picture, its dtype and `used` bytes, sigma, the radius; with use_fb the thresholds
    struct TfilterRadius {
      const void *picture, *used;
      int f32, radius, use_fb;
      float sigma, alpha, beta;
    };
    // run_batch_error: the truth, the mask and its rule, the three outputs
    struct Error {
      const void *gt, *mask, *stats, *err, *hist;
      int mask_eq;
    };
    // run_batch_motion_mask: the outputs (the caller's arrays or their place in the context's buffer), the fit's and the
    // mask's scalars; with use_fb the thresholds
    struct MotionMask {
      const void *code, *res, *stats, *xform, *support, *occ;
      int model, step, iters, use_fb, radius;
      float alpha, beta, thr, rel;
      double tau;
    };
    int family;
    int n, w, h;
    int seq, stride;  // a sequence call: `a` is one array of n + stride frames
    const void *a, *b, *init, *out, *ws;
    const void *buf;  // the context's level-grid buffer, in the calls whose flow passes through it
    ofdis_params p;
    union {
      Batch batch;
      Interp interp;
      Track track;
      Tfilter tfilter;
      Stab stab;
      TfilterRadius tfilter_radius;
      Error error;
      MotionMask motion_mask;
    } u;
  } gkey{};
  hipGraphExec_t gexec = nullptr;
  int opt_nt_store = 0;        // upsample output with non-temporal stores (A/B)
  // flow upsample: 0 per-output-row horizontal taps (k_upsample_rows), 1 / 2 once per staged source row (k_upsample_h,
  // 4 / 8 rows), 3 auto: 1 when the frame spans a whole 1024-column block and the call runs on two or more lanes or
  // has fewer than 1024 pairs, else 0 -- measured end to end, alternating on one box each (profiles/r05/s16/NOTE.md):
  // B two lanes 331.4k (1) vs 322.3k (0), one lane of 2048-pair chunks 294.6k vs 306.8k; C 11,260 vs 11,185; D
  // (2 x 128) 226.9k vs 224.1k; the 32-pair shard 64.67k vs 64.37k; A (640 wide) 122.7k vs 124.5k
  int opt_up_form = 3;
  int opt_smsys = 1;           // smoothness + system in one launch (0: two launches, A/B)
  // the fused launch on 2-D tiles for tall levels: 1 on, 0 off (two launches there), 2 auto = on for calls of
  // fewer than 512 pairs (one stream).  Measured at config E: alone on the GPU it cuts the system time 10 %
  // (580 vs 603 ms per 512 pairs on one stream), but beside a second chain (two streams) the LDS-holding
  // fused kernel overlaps worse with the other lane's patch kernel than the two plain launches (561 vs
  // 544-551 ms per step) -- profiles/r02/ab/ab_smsys2d.
  int opt_smsys2d = 2;
  int opt_smsys_march = 1;     // tall levels: smoothness + system as a register march (k_tv_smsys_m)
  int opt_smsys_prefetch = 1;  // fused smoothness + system (gray): derivative images issued before the staging
  int opt_smsys_small = 1;     // fused smoothness + system: small row blocks for launches that cannot fill the chip
  int opt_agg_stage = 1;       // k_aggregate: patch displacements of the tile staged in LDS (0: gathered from p_iter)
  int opt_pad_grad_v = 1;      // colour pyramid pad + gradients: one thread per value (0: per pixel, channels inside)
  int opt_pyr_rgb = 1;         // colour pyramid base by dword loads and masked v_sad_u8 (0: the byte loop)
  int opt_prepd_df = 1;        // smsys_deriv levels: k_tv_prepd_df (Ix, Iy, Iz from a 2-pixel halo, channels in one pass);
                               // 0: k_tv_prepd (intensity), k_tv_prepd_c3 (colour: all eight derivative planes)
  int opt_smsys_deriv = 1;     // fused smoothness + system (gray; colour: the march): second derivatives filtered from Ix, Iy, Iz
  int call_frames = 1;         // pairs of the current call (auto options)
  int call_lanes = 1;          // streams the current call's chunks run on (auto options)
  int opt_sor_cring = 2;       // sweep-per-wave SOR: coefficient ring in LDS (0: every sweep loads its coefficients;
                               // 2: ring sized to the level's row groups, the clamped in-frame load form in launches
                               // that oversubscribe the chip; 3: that load form in every launch; 1: workgroup limit)
  int opt_sor_pack = 1;        // sweep-per-wave SOR: several frames' rows packed into one workgroup's waves (0: one
                               // frame per workgroup; 1: launches with more frames than CUs; 2: every launch)
  int opt_prepd = 2;           // prep + derivatives in one launch: 1 intensity images, 2 colour images too (0: three launches)
  int opt_sor_rows2 = 1;       // sweep-per-wave SOR with two rows per lane for 321..640-row levels (0: pipeline)
  int opt_wave_per_patch = 0;  // 1: one wave per patch instead of eight lanes (A/B)
  int opt_sor_mode = 0;        // 0 exact lexicographic order (the reference's bits); 1 red-black (opt-in)
  int opt_patch_window = 1;    // eight-lane patches read their bilinear taps from an LDS window (0: L1 gathers)
  int opt_patch_quad = 1;      // windowed gray patches on four lanes per patch (k_patchq; 0: eight, k_patchw)
  int opt_patch_x16 = 1;       // windowed RGB p = 12 patches on sixteen lanes per patch (k_patchx; 0: eight, k_patchw;
                               // 2: k_patchx with the exact square-root evaluation every iteration, parity testing)
  int opt_patch_absw = 1;      // patch kernels that can hand the aggregation its weights directly do (0: loss weights)
  int opt_patch_buf = 1;       // gray p = 12 windows by buffer loads (32-bit offsets) where the image array allows
  int opt_patch_generic = 0;   // 1: every shape on the any-shape patch kernel k_patchg (parity testing)
  int opt_patch_fdiv = 1;      // the LLT solves divide by FMA-corrected pivot reciprocals (0: IEEE divisions)
  int opt_patch_maxres = 1;    // op-point stopping (res_thresh 0, min_iter = max_iter): largest |w| > 0 for mean > 0
  // sub-batch pipelining: chunks of `opt_chunk` frames round-robin over `opt_streams` streams, each with
  // its own workspace, so one chunk's latency-bound wavefront overlaps another chunk's streaming kernels.
  // streams 0 = auto: 2 for batches of >= 512 pairs (measured +7-9 % at 1024 1080p pairs: two 512-pair
  // chains on two streams), else 1; chunk 0 = the batch split evenly over the streams.
  int opt_streams = 0, opt_chunk = 0;
  struct Lane {
    hipStream_t s = nullptr;
    char *ws = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
  };
  std::vector<Lane> lanes;
  hipEvent_t entry = nullptr;
  // call ordering: ev_null hands the legacy NULL stream's queued work to the context's stream; ev_ws marks
  // the end of the previous call's use of the workspaces (a call on another stream waits for it)
  hipEvent_t ev_null = nullptr, ev_ws = nullptr;
  bool ws_pending = false;
  std::mutex mu;
};

static_assert(std::is_trivially_copyable<ofdis_context::GraphKey>::value && std::is_standard_layout<ofdis_context::GraphKey>::value,
              "the graph key is zeroed, copied and compared as bytes");
static_assert(sizeof(ofdis_context::GraphKey) <= 512, "the graph key is built on the stack by every replayed call");

namespace {

// OFDIS_TRACE=1: host-side progress lines on stderr (debugging the multi-stream paths)
bool trace_on() {
  static const bool on = std::getenv("OFDIS_TRACE") && std::getenv("OFDIS_TRACE")[0] == '1';
  return on;
}
#define OFDIS_TRACE(...)                  \
  do {                                    \
    if (trace_on()) {                     \
      std::fprintf(stderr, "ofdis: " __VA_ARGS__); \
      std::fputc('\n', stderr);           \
      std::fflush(stderr);                \
    }                                     \
  } while (0)

#define HIP_OK(x)                                                                                \
  do {                                                                                           \
    hipError_t e_ = (x);                                                                         \
    if (e_ != hipSuccess) {                                                                      \
      std::fprintf(stderr, "ofdis: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, \
                   __LINE__);                                                                    \
      return e_ == hipErrorOutOfMemory ? OFDIS_ERR_OUT_OF_MEMORY : OFDIS_ERR_DEVICE;             \
    }                                                                                            \
  } while (0)

int kernel_index(const char *name) {
  for (int i = 0; i < (int)(sizeof(kKernelNames) / sizeof(kKernelNames[0])); ++i)
    if (std::strcmp(kKernelNames[i], name) == 0) return i;
  for (int i = 0; i < (int)(sizeof(kKernelNamesExt) / sizeof(kKernelNamesExt[0])); ++i)
    if (std::strcmp(kKernelNamesExt[i], name) == 0) return kNumKernelNames + i;
  for (int i = 0; i < (int)(sizeof(kKernelNamesMore) / sizeof(kKernelNamesMore[0])); ++i)
    if (std::strcmp(kKernelNamesMore[i], name) == 0) return kSlotMotionMask + i;
  return -1;
}

hipEvent_t get_event(ofdis_context *c) {
  if (!c->pool.empty()) {
    hipEvent_t e = c->pool.back();
    c->pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreate(&e) != hipSuccess) return nullptr;
  return e;
}

template <class F>
void timed(ofdis_context *c, int kernel, hipStream_t s, F &&f) {
  if (!c->timing) {
    f();
    return;
  }
  hipEvent_t a = get_event(c), b = get_event(c);
  hipEventRecord(a, s);
  f();
  hipEventRecord(b, s);
  c->pending.push_back({kernel, a, b});
}

void drain_timing(ofdis_context *c) {
  for (auto &p : c->pending) {
    hipEventSynchronize(p.b);
    float ms = 0.0f;
    hipEventElapsedTime(&ms, p.a, p.b);
    auto &e = c->acc[p.kernel];
    e.first += ms;
    e.second += 1;
    c->pool.push_back(p.a);
    c->pool.push_back(p.b);
  }
  c->pending.clear();
}

void fill_level(const ofdis_params *p, int Wp, int Hp, int pad, int s, LevelGeom &g) {
  const float sc_fct = (float)std::pow(2.0, -s);  // oflow.cpp:142-153
  g.w = (int)((float)Wp * sc_fct);
  g.h = (int)((float)Hp * sc_fct);
  g.pad = pad;
  g.W = g.w + 2 * pad;
  g.H = g.h + 2 * pad;
  g.level = s;
  g.tmp_lb = -(float)p->p_samp_s / 2;
  g.tmp_ubw = (float)(g.w + p->p_samp_s / 2 - 2);
  g.tmp_ubh = (float)(g.h + p->p_samp_s / 2 - 2);
  const int st0 = (int)std::floor((float)p->p_samp_s * (1 - p->patove));  // oflow.cpp:90
  const int steps = st0 > 1 ? st0 : 1;
  g.nopw = (int)std::ceil((float)g.w / (float)steps);  // patchgrid.cpp:43-46
  g.noph = (int)std::ceil((float)g.h / (float)steps);
  g.offw = (g.w - (g.nopw - 1) * steps) / 2;
  g.offh = (g.h - (g.noph - 1) * steps) / 2;
  g.npatch = g.nopw * g.noph;
}

int steps_of(const ofdis_params *p) {
  const int st0 = (int)std::floor((float)p->p_samp_s * (1 - p->patove));
  return st0 > 1 ? st0 : 1;
}

Plan make_plan(const ofdis_params *p, int n, int Wp, int Hp, int pad, bool init = false, bool bidir = false,
               int stride = 0) {
  Plan P;
  P.n = n;
  P.seq = stride > 0;
  P.nfr = P.seq ? n + stride : 2 * n;
  P.bdist = P.seq ? stride : n;
  const size_t nfr = (size_t)P.nfr;
  P.Wp = Wp;
  P.Hp = Hp;
  P.nop = p->mode == OFDIS_MODE_OF ? 2 : 1;
  P.noc = p->noc;
  P.pad = pad;
  P.sc_f = p->sc_f;
  P.sc_l = p->sc_l;
  const int nsc = p->sc_f - p->sc_l + 1;
  P.lv.resize(nsc);
  P.off_lvl.resize(nsc);
  P.off_img.resize(nsc);
  P.off_dx.resize(nsc);
  P.off_dy.resize(nsc);
  P.off_flow.resize(nsc);
  P.off_flow_bw.resize(nsc);
  P.fb = p->usefbcon != 0;
  P.bidir = bidir;
  const bool bw = P.fb || bidir;  // a backward grid and flow
  size_t off = 0;
  const int novals = p->noc * p->p_samp_s * p->p_samp_s;
  size_t max_np = 0, max_plane = 0;
  for (int s = p->sc_l; s <= p->sc_f; ++s) {
    const int i = s - p->sc_l;
    fill_level(p, Wp, Hp, pad, s, P.lv[i]);
    const LevelGeom &g = P.lv[i];
    P.off_lvl[i] = off;
    off = align_up(off + sizeof(float) * nfr * g.w * g.h * P.noc);
    P.off_img[i] = off;  // (+64 floats: the windowed patch kernel's 16-byte row loads may read past the last row
                         // of the last frame -- frame nfr - 1, the last pair's frame b in either layout)
    off = align_up(off + sizeof(float) * (nfr * g.W * g.H * P.noc + 64));
    P.off_dx[i] = off;
    off = align_up(off + sizeof(float) * nfr * g.W * g.H * P.noc);
    P.off_dy[i] = off;
    off = align_up(off + sizeof(float) * nfr * g.W * g.H * P.noc);
    P.off_flow[i] = off;
    off = align_up(off + sizeof(float) * (size_t)n * P.nop * g.w * g.h);
    P.off_flow_bw[i] = off;
    if (bw) off = align_up(off + sizeof(float) * (size_t)n * P.nop * g.w * g.h);
    if ((size_t)g.npatch > max_np) max_np = g.npatch;
    if ((size_t)g.w * g.h > max_plane) max_plane = (size_t)g.w * g.h;
  }
  P.off_piter = off;
  off = align_up(off + sizeof(float) * (size_t)n * max_np * P.nop);
  P.off_pw = off;  // loss weights [n][npatch][novals], or the aggregation-weight slot planes [n][A * A][h][w]
  const size_t aslots = (size_t)((p->p_samp_s - 1) / steps_of(p) + 1);
  off = align_up(off + sizeof(float) * (size_t)n * std::max(max_np * novals, aslots * aslots * max_plane));
  P.off_piter_bw = off;
  if (bw) off = align_up(off + sizeof(float) * (size_t)n * max_np * P.nop);
  P.off_pw_bw = off;  // usefbcon: loss weights; bidir without it: the backward patch launch may write slot planes too
  if (P.fb) off = align_up(off + sizeof(float) * (size_t)n * max_np * novals);
  else if (bidir) off = align_up(off + sizeof(float) * (size_t)n * std::max(max_np * novals, aslots * aslots * max_plane));
  P.off_tv = off;
  size_t max_sp = 0;  // skewed TV plane
  for (const LevelGeom &g : P.lv) max_sp = std::max(max_sp, (size_t)skew_plane(g.w, g.h));
  P.tv_plane = max_sp;
  if (p->usetvref) off = align_up(off + sizeof(float) * (size_t)n * max_sp * (14 + 9 * (size_t)P.noc));
  P.off_gm = off;
  if (p->gradmag) {
    P.gradmag = true;
    off = align_up(off + sizeof(float) * nfr * ((size_t)Wp * Hp + (size_t)(Wp / 2) * (Hp / 2)));
  }
  P.off_init = off;
  if (init) {
    P.init = true;
    off = align_up(off + sizeof(float) * (size_t)n * P.nop * (Wp >> (p->sc_f + 1)) * (Hp >> (p->sc_f + 1)));
  }
  P.total = off;
  return P;
}

// A captured graph bakes in the workspace and lane pointers: drop it before any of them is reallocated.
int drop_graph(ofdis_context *c) {
  if (!c->gexec) return OFDIS_OK;
  HIP_OK(hipDeviceSynchronize());  // it may still run on a caller stream
  HIP_OK(hipGraphExecDestroy(c->gexec));
  c->gexec = nullptr;
  return OFDIS_OK;
}

int ensure_ws(ofdis_context *c, size_t bytes) {
  if (bytes <= c->ws_cap) return OFDIS_OK;
  if (c->ws) {
    int rc = drop_graph(c);
    if (rc) return rc;
    HIP_OK(hipDeviceSynchronize());  // callers may have queued work on their own streams
    HIP_OK(hipFree(c->ws));
    c->ws = nullptr;
    c->ws_cap = 0;
  }
  HIP_OK(hipMalloc(&c->ws, bytes));
  c->ws_cap = bytes;
  return OFDIS_OK;
}

int ensure_warp_buf(ofdis_context *c, size_t bytes) {
  if (bytes <= c->warp_cap) return OFDIS_OK;
  if (c->warp_buf) {
    int rc = drop_graph(c);
    if (rc) return rc;
    HIP_OK(hipDeviceSynchronize());  // callers may have queued work on their own streams
    HIP_OK(hipFree(c->warp_buf));
    c->warp_buf = nullptr;
    c->warp_cap = 0;
  }
  HIP_OK(hipMalloc(&c->warp_buf, bytes));
  c->warp_cap = bytes;
  return OFDIS_OK;
}

int capture(ofdis_context *c, hipStream_t s, const std::vector<float *> &cap, int scale, const Plan &P,
            const float *flow_planar) {
  if ((int)cap.size() <= scale || !cap[scale]) return OFDIS_OK;
  const LevelGeom &g = P.lv[scale - P.sc_l];
  const size_t plane = (size_t)g.w * g.h;
  std::vector<float> tmp(plane * P.nop);
  HIP_OK(hipMemcpyAsync(tmp.data(), flow_planar, tmp.size() * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  for (size_t i = 0; i < plane; ++i)
    for (int k = 0; k < P.nop; ++k) cap[scale][i * P.nop + k] = tmp[k * plane + i];
  return OFDIS_OK;
}

struct StageTimes {
  double pconst = 0, pinit = 0, poptim = 0, cflow = 0, tvopt = 0;
};

// The coarse-to-fine loop (oflow.cpp:182-330) over device pyramids already in the workspace.
// init: optional coarse initial flow (device, interleaved, (w_f/2)*(h_f/2)*nop per frame).
// The largest float s with sqrtf(s) <= t.  A correctly rounded square root is monotone, so for every float s
// (NaN and inf included) sqrtf(s) > t <=> s > sqrt_le_bound(t): the patch kernels' outlier test compares the
// squared distance against it, bit-for-bit the reference's norm() > outlierthresh without a square root.
static float sqrt_le_bound(float t) {
  if (!(t >= 0.0f) || std::isinf(t)) return t * t;
  float s = t * t;
  while (std::sqrt(std::nextafter(s, INFINITY)) <= t) s = std::nextafter(s, INFINITY);
  while (s > 0.0f && std::sqrt(s) > t) s = std::nextafter(s, -INFINITY);
  return s;
}

int run_levels(ofdis_context *c, char *ws, const Plan &P, const ofdis_params *p, hipStream_t s, const float *init,
               std::vector<StageTimes> *times) {
  const int nop = P.nop, noc = P.noc, n = P.n;
  const size_t bd = (size_t)P.bdist;  // frame b of pair f: bd frames after frame a in every pyramid array
  const int novals = noc * p->p_samp_s * p->p_samp_s;
  const int steps = steps_of(p);
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  if (times)
    for (auto &e : ev) HIP_OK(hipEventCreate(&e));
  for (int sl = p->sc_f; sl >= p->sc_l; --sl) {
    const int i = sl - p->sc_l;
    const LevelGeom &g = P.lv[i];
    const size_t fsp = (size_t)g.W * g.H * noc;  // floats per padded frame
    const float *img = (const float *)(ws + P.off_img[i]);
    const float *dxp = (const float *)(ws + P.off_dx[i]);
    const float *dyp = (const float *)(ws + P.off_dy[i]);
    float *flow = (float *)(ws + P.off_flow[i]);
    if (times) HIP_OK(hipEventRecord(ev[0], s));

    PatchArgs pa{};
    pa.img_a = img;
    pa.dx_a = dxp;
    pa.dy_a = dyp;
    pa.img_b = img + bd * fsp;
    if (sl < p->sc_f) {
      const LevelGeom &gc = P.lv[i + 1];
      pa.prev = (const float *)(ws + P.off_flow[i + 1]);
      pa.prev_frame_stride = (long)nop * gc.w * gc.h;
      pa.prev_comp_stride = gc.w * gc.h;
      pa.prev_elem_stride = 1;
      pa.prev_w = g.w / 2;
    } else if (init) {
      pa.prev = init;
      pa.prev_frame_stride = (long)nop * (g.w / 2) * (g.h / 2);
      pa.prev_comp_stride = 1;
      pa.prev_elem_stride = nop;
      pa.prev_w = g.w / 2;
    }
    pa.p_iter = (float *)(ws + P.off_piter);
    pa.pweight = (float *)(ws + P.off_pw);
    pa.n = n;
    pa.nop = nop;
    pa.noc = noc;
    pa.p = p->p_samp_s;
    pa.novals = novals;
    pa.steps = steps;
    pa.costfct = p->costfct;
    pa.patnorm = p->patnorm;
    pa.max_iter = p->max_iter;
    pa.min_iter = p->min_iter;
    pa.dp_thresh_sq = p->dp_thresh * p->dp_thresh;
    pa.dr_thresh = p->dr_thresh;
    pa.res_thresh = p->res_thresh;
    pa.outlierthresh = (float)p->p_samp_s / 2;
    pa.outlier_sq = sqrt_le_bound(pa.outlierthresh);
    pa.camlr = 0;
    pa.wave_per_patch = c->opt_wave_per_patch;
    pa.window = c->opt_patch_window;
    pa.quad = c->opt_patch_quad;
    pa.x16 = c->opt_patch_x16;
    pa.absw = !P.fb && c->opt_patch_absw;  // usefbcon: the complementary grid's loss weights are read raw
    pa.aslots = (p->p_samp_s - 1) / steps + 1;
    pa.fdiv = c->opt_patch_fdiv;
    pa.maxres = c->opt_patch_maxres && pa.res_thresh == 0.0f && pa.min_iter >= pa.max_iter;
    // the buffer resource starts at the launch's img_b and its offsets cover that pointer's n frames, whichever
    // frame of the array it is (forward: frame bd, backward: frame 0) -- the extent does not depend on bd
    pa.buf32 = c->opt_patch_buf && (size_t)n * fsp * sizeof(float) + 4096 <= 0xffffffffu;
    pa.generic = c->opt_patch_generic;
    pa.g = g;
    if (times) {  // verbosity 2: pconst / pinit from construction-only launches (their output is overwritten)
      PatchArgs pd = pa;
      pd.stage = 1;
      launch_patch(pd, s);
      HIP_OK(hipEventRecord(ev[1], s));
      pd.stage = 2;
      launch_patch(pd, s);
      HIP_OK(hipEventRecord(ev[2], s));
    }
    bool absw = false;
    timed(c, 3, s, [&] { absw = launch_patch(pa, s); });
    // usefbcon: the backward grid -- template on image b, target image a, right camera (camlr = 1),
    // initialised from the coarser backward flow (oflow.cpp:158-169, 193-196, 209-211, 231-233)
    PatchArgs pb = pa;
    const bool bw = P.fb || P.bidir;
    bool absw_bw = false;
    if (bw) {
      pb.img_a = img + bd * fsp;
      pb.dx_a = dxp + bd * fsp;
      pb.dy_a = dyp + bd * fsp;
      pb.img_b = img;
      pb.prev = nullptr;
      if (sl < p->sc_f) pb.prev = (const float *)(ws + P.off_flow_bw[i + 1]);
      pb.p_iter = (float *)(ws + P.off_piter_bw);
      pb.pweight = (float *)(ws + P.off_pw_bw);
      pb.camlr = 1;
      timed(c, 3, s, [&] { absw_bw = launch_patch(pb, s); });
    }

    AggArgs ag{};
    ag.p_iter = pa.p_iter;
    ag.pweight = pa.pweight;
    ag.flow = flow;
    ag.n = n;
    ag.nop = nop;
    ag.noc = noc;
    ag.p = p->p_samp_s;
    ag.novals = novals;
    ag.absw = absw;
    ag.aslots = pa.aslots;
    ag.stage = c->opt_agg_stage;
    ag.steps = steps;
    ag.g = g;
    ag.cg_p_iter = P.fb ? pb.p_iter : nullptr;
    ag.cg_pweight = P.fb ? pb.pweight : nullptr;
    float *flow_bw = (float *)(ws + P.off_flow_bw[i]);
    const int n_inner = p->tv_innerit * (sl + 1);  // refine_variational.cpp:36
    // the refinement's arguments for direction dir (dir 1: VarRefClass on the backward flow with the images swapped,
    // oflow.cpp:312-316)
    auto make_tv = [&](int dir) {
      const long sp = skew_plane(g.w, g.h);
      const size_t pl = (size_t)n * sp;
      float *t0 = (float *)(ws + P.off_tv);
      TvArgs tv{};
      tv.img_a = dir == 0 ? img : img + bd * fsp;
      tv.img_b = dir == 0 ? img + bd * fsp : img;
      tv.flow = dir == 0 ? flow : flow_bw;
      tv.du = t0;
      tv.dv = t0 + pl;
      tv.mask = t0 + 2 * pl;
      tv.coef = t0 + 3 * pl;  // 8 planes' worth (float4 x 2 per pixel), 16-byte aligned: sp % 4 == 0 ensured
      tv.s = t0 + 11 * pl;
      tv.wxs = t0 + 12 * pl;
      tv.wys = t0 + 13 * pl;
      tv.sp = sp;
      tv.wrap = g.h <= g.w;
      tv.skew_slots = tv.wrap ? g.w * g.h : (g.w + g.h - 1) * g.h;
      float *cp = t0 + 14 * pl;
      const size_t cpl = pl * noc;
      tv.t = cp;
      tv.dt = cp + cpl;
      tv.Iz = tv.dt;
      tv.Ix = cp + 2 * cpl;
      tv.Iy = cp + 3 * cpl;
      tv.Ixx = cp + 4 * cpl;
      tv.Ixy = cp + 5 * cpl;
      tv.Iyy = cp + 6 * cpl;
      tv.Ixz = cp + 7 * cpl;
      tv.Iyz = cp + 8 * cpl;
      tv.n = n;
      tv.nop = nop;
      tv.noc = noc;
      tv.w = g.w;
      tv.h = g.h;
      tv.pad = g.pad;
      tv.W = g.W;
      tv.quarter_alpha = 0.25f * p->tv_alpha;  // refine_variational.cpp:40-43
      tv.hgo3 = p->tv_gamma * 0.5f / 3.0f;
      tv.hdo3 = p->tv_delta * 0.5f / 3.0f;
      tv.omega = p->tv_sor;
      tv.solverit = p->tv_solverit;
      tv.camlr = dir;
      tv.sor_generic = c->opt_sor_generic;
      tv.sor_variant = c->opt_sor_pipe;
      tv.sor_cring = c->opt_sor_cring;
      tv.sor_pack = c->opt_sor_pack;      tv.sor_rows2 = c->opt_sor_rows2;
      tv.smsys = c->opt_smsys;
      tv.smsys2d = c->opt_smsys2d == 2 ? c->call_frames < 512 : c->opt_smsys2d;
      tv.smsys_march = c->opt_smsys_march;
      tv.smsys_prefetch = c->opt_smsys_prefetch;
      tv.smsys_small = c->opt_smsys_small;
      tv.smsys_deriv = c->opt_smsys_deriv;
      tv.prepd_df = c->opt_prepd_df;
      tv.sor_redblack = c->opt_sor_mode == 1;
      tv.sor_point = p->omp_build && nop == 2;  // refine_variational.cpp:202-203
      tv.prepd = c->opt_prepd;
      return tv;
    };
    if (times) HIP_OK(hipEventRecord(ev[3], s));
    timed(c, 4, s, [&] { launch_aggregate(ag, s); });
    // the backward flow is not needed after the last scale -- unless the caller asked for it (bidir)
    const bool bw_level = bw && (sl > p->sc_l || P.bidir);
    if (bw_level) {                               // patchgrid.cpp:213-397 with the roles swapped
      AggArgs ab = ag;
      ab.p_iter = pb.p_iter;
      ab.pweight = pb.pweight;
      ab.cg_p_iter = P.fb ? pa.p_iter : nullptr;
      ab.cg_pweight = P.fb ? pa.pweight : nullptr;
      ab.absw = absw_bw;
      ab.flow = flow_bw;
      timed(c, 4, s, [&] { launch_aggregate(ab, s); });
    }
    if (times) HIP_OK(hipEventRecord(ev[4], s));
    int rc = capture(c, s, c->cap_dis, sl, P, flow);
    if (rc) return rc;

    for (int dir = 0; dir < (bw_level ? 2 : 1) && p->usetvref && n_inner > 0; ++dir) {
      TvArgs tv = make_tv(dir);
      // latency form of sor_mode = 1: the whole inner loop and the flow update in one launch per level, prep writing
      // the colour-split layout that launch reads (all eight derivative planes)
      tv.lat = tv_level_rb_ok(tv);
      tv.smsys_deriv = !tv.lat && tv_deriv_fused(tv);  // before the prep launch: it decides which planes prepd writes
      if (tv_prepd_ok(tv)) {
        timed(c, 5, s, [&] { launch_tv_prepd(tv, s); });
      } else {
        timed(c, 5, s, [&] { launch_tv_prep(tv, s); });
        timed(c, 6, s, [&] {
          launch_tv_deriv1(tv, s);
          launch_tv_deriv2(tv, s);
        });
      }
      if (tv.lat) {
        timed(c, 11, s, [&] { launch_tv_level_rb(tv, n_inner, s); });
        continue;
      }
      for (int it = 0; it < n_inner; ++it) {
        tv.first_iter = it == 0;
        timed(c, 7, s, [&] {
          if (tv_smsys_ok(tv)) {
            launch_tv_smsys(tv, s);
          } else {
            launch_tv_smooth(tv, s);
            launch_tv_system(tv, s);
          }
        });
        timed(c, 8, s, [&] { launch_tv_sor(tv, s); });
      }
      timed(c, 9, s, [&] { launch_tv_final(tv, s); });
    }
    if (times) {
      HIP_OK(hipEventRecord(ev[5], s));
      HIP_OK(hipEventSynchronize(ev[5]));
      StageTimes st;
      float t01, t12, t23, t34, t45;
      hipEventElapsedTime(&t01, ev[0], ev[1]);
      hipEventElapsedTime(&t12, ev[1], ev[2]);
      hipEventElapsedTime(&t23, ev[2], ev[3]);
      hipEventElapsedTime(&t34, ev[3], ev[4]);
      hipEventElapsedTime(&t45, ev[4], ev[5]);
      // the optimisation launch repeats construction and initialisation: poptim is the rest of it
      st.pconst = t01;
      st.pinit = std::max(0.0, (double)t12 - t01);
      st.poptim = std::max(0.0, (double)t23 - t12);
      st.cflow = t34;
      st.tvopt = t45;
      times->push_back(st);
    }
    rc = capture(c, s, c->cap_tv, sl, P, flow);
    if (rc) return rc;
  }
  if (times)
    for (auto &e : ev) hipEventDestroy(e);
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

void print_times(const Plan &P, const std::vector<StageTimes> &t, double total_ms, int verbosity) {
  if (verbosity > 1) {
    for (size_t k = 0; k < t.size(); ++k) {
      const int sl = P.sc_f - (int)k;
      const LevelGeom &g = P.lv[sl - P.sc_l];
      const double all = t[k].pconst + t[k].pinit + t[k].poptim + t[k].cflow + t[k].tvopt;
      std::printf("TIME (Sc: %i, #p:%6i, pconst, pinit, poptim, cflow, tvopt, total): %8.2f %8.2f %8.2f %8.2f %8.2f -> %8.2f ms.\n",
                  sl, g.npatch, t[k].pconst, t[k].pinit, t[k].poptim, t[k].cflow, t[k].tvopt, all);
    }
  }
  if (verbosity > 0) std::printf("TIME (O.Flow Run-Time   ) (ms): %3g\n", total_ms);
}

int check_device(int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return OFDIS_ERR_NO_DEVICE;
  if (device < 0 || device >= count) return OFDIS_ERR_INVALID_ARGUMENT;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return OFDIS_ERR_DEVICE;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    std::fprintf(stderr, "ofdis: device %d is %s, this build targets gfx950 only\n", device, prop.gcnArchName);
    return OFDIS_ERR_NO_DEVICE;
  }
  return OFDIS_OK;
}

// Pyramid of the batch (run_dense.cpp:299-312,327-328,131-179) into the workspace.
// Pairs: frames 0..n-1 from a, n..2n-1 from b.  A sequence plan: its n + stride frames from a alone (b unread).
int run_pyramid(ofdis_context *c, char *ws, const Plan &P, const uint8_t *a, const uint8_t *b, hipStream_t s) {
  const int n2 = P.nfr, na = P.seq ? P.nfr : P.stereo ? P.n / 2 : P.n;  // (stereo: the caller's pairs)
  if (P.gradmag) {  // SELECTCHANNEL 2 (run_dense.cpp:139-148): float level 0, then 2x2 means down to sc_l
    float *lvl0 = (float *)(ws + P.off_lvl[0]);
    float *bufA = (float *)(ws + P.off_gm), *bufB = bufA + (size_t)n2 * P.Wp * P.Hp;
    PyrGradmagArgs g{};
    g.img_a = a;
    g.img_b = b;
    g.n = na;
    g.nf = n2;
    g.W0 = P.W0;
    g.H0 = P.H0;
    g.padl = P.padl;
    g.padt = P.padt;
    g.Wp = P.Wp;
    g.Hp = P.Hp;
    g.stereo = P.stereo;
    g.out = P.sc_l == 0 ? lvl0 : bufA;
    timed(c, 0, s, [&] { launch_pyr_gradmag(g, s); });
    const float *src = bufA;
    int w = P.Wp, h = P.Hp;
    for (int l = 1; l <= P.sc_l; ++l) {
      PyrDownArgs pd{};
      pd.src = src;
      pd.dst = l == P.sc_l ? lvl0 : ((l & 1) ? bufB : bufA);
      pd.n2 = n2;
      pd.w = w /= 2;
      pd.h = h /= 2;
      pd.noc = 1;
      timed(c, 1, s, [&] { launch_pyr_down(pd, s); });
      src = pd.dst;
    }
  } else {
    PyrBaseArgs pb{};
    pb.img_a = a;
    pb.img_b = b;
    pb.n = na;
    pb.nf = n2;
    pb.W0 = P.W0;
    pb.H0 = P.H0;
    pb.noc = P.noc;
    pb.padl = P.padl;
    pb.padt = P.padt;
    pb.log2s = P.sc_l;
    pb.w = P.lv[0].w;
    pb.h = P.lv[0].h;
    pb.out = (float *)(ws + P.off_lvl[0]);
    pb.rgb_sad = c->opt_pyr_rgb;
    pb.stereo = P.stereo;
    timed(c, 0, s, [&] { launch_pyr_base(pb, s); });
  }
  for (size_t i = 1; i < P.lv.size(); ++i) {
    PyrDownArgs pd{};
    pd.src = (const float *)(ws + P.off_lvl[i - 1]);
    pd.dst = (float *)(ws + P.off_lvl[i]);
    pd.n2 = n2;
    pd.w = P.lv[i].w;
    pd.h = P.lv[i].h;
    pd.noc = P.noc;
    timed(c, 1, s, [&] { launch_pyr_down(pd, s); });
  }
  for (size_t i = 0; i < P.lv.size(); ++i) {
    PyrPadGradArgs pg{};
    pg.lvl = (const float *)(ws + P.off_lvl[i]);
    pg.img = (float *)(ws + P.off_img[i]);
    pg.dx = (float *)(ws + P.off_dx[i]);
    pg.dy = (float *)(ws + P.off_dy[i]);
    pg.n2 = n2;
    pg.w = P.lv[i].w;
    pg.h = P.lv[i].h;
    pg.noc = P.noc;
    pg.pad = P.pad;
    pg.per_value = c->opt_pad_grad_v;
    timed(c, 2, s, [&] { launch_pyr_pad_grad(pg, s); });
  }
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// bidir: 0 plain, 1 both directions, 2 both directions and the full-resolution backward flow kept in the workspace,
//        3 both directions and the two occlusion masks of the pairs kept in the workspace (ofdis_run_interp_occ_u8)
// stride: 0 two arrays of n frames, k > 0 one sequence of n + k frames
// stereo: 0 no, 1 n stereo pairs as 2n flow pairs, 2 the same and the right view's disparity kept in the workspace
Plan batch_plan(const ofdis_params *p, int n, int width, int height, bool init = false, int bidir = 0,
                int stride = 0, int stereo = 0) {
  const int d = 1 << (p->sc_f + (init ? 1 : 0));  // run_dense.cpp:301-302
  const int padw = (width % d) ? d - width % d : 0, padh = (height % d) ? d - height % d : 0;
  Plan P = make_plan(p, stereo ? 2 * n : n, width + padw, height + padh, p->p_samp_s, init, bidir != 0, stride);
  P.stereo = stereo != 0;
  P.off_up_bw = P.total;
  if (bidir == 2 || stereo == 2) P.total = align_up(P.total + sizeof(float) * (size_t)n * width * height * P.nop);
  if (bidir == 3) P.total = align_up(P.total + 2 * (size_t)n * width * height);
  P.W0 = width;
  P.H0 = height;
  P.padw = padw;
  P.padh = padh;
  P.padl = padw / 2;  // copyMakeBorder(floor(padw/2), ceil(padw/2)) (run_dense.cpp:309)
  P.padt = padh / 2;
  return P;
}

}  // namespace

extern "C" {

int ofdis_context_create(int device, ofdis_context **out) {
  if (!out) return OFDIS_ERR_INVALID_ARGUMENT;
  *out = nullptr;
  int rc = check_device(device);
  if (rc) return rc;
  HIP_OK(hipSetDevice(device));
  ofdis_context *c = new ofdis_context();
  c->device = device;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return OFDIS_ERR_DEVICE;
  }
  // load the kernels' code objects now, not inside the first call's timers (the drop-in CLI's one pair)
  warm_kernels_module(c->stream);
  warm_tvrb_module(c->stream);
  if (hipStreamSynchronize(c->stream) != hipSuccess) {
    hipStreamDestroy(c->stream);
    delete c;
    return OFDIS_ERR_DEVICE;
  }
  *out = c;
  return OFDIS_OK;
}

void ofdis_context_destroy(ofdis_context *c) {
  if (!c) return;
  hipSetDevice(c->device);
  if (c->gexec) {  // it may still run on a caller stream
    hipDeviceSynchronize();
    hipGraphExecDestroy(c->gexec);
    c->gexec = nullptr;
  }
  if (c->ws_pending) hipEventSynchronize(c->ev_ws);  // the last call's work, on whatever stream it ran
  if (c->stream) hipStreamSynchronize(c->stream);
  drain_timing(c);
  for (auto e : c->pool) hipEventDestroy(e);
  if (c->ws) hipFree(c->ws);
  if (c->warp_buf) hipFree(c->warp_buf);
  for (auto &L : c->lanes) {
    if (L.s) hipStreamSynchronize(L.s);
    if (L.ws) hipFree(L.ws);
    if (L.done) hipEventDestroy(L.done);
    if (L.s) hipStreamDestroy(L.s);
  }
  if (c->entry) hipEventDestroy(c->entry);
  if (c->ev_null) hipEventDestroy(c->ev_null);
  if (c->ev_ws) hipEventDestroy(c->ev_ws);
  if (c->stream) hipStreamDestroy(c->stream);
  delete c;
}

extern "C++" {  // (templates among them)
namespace {

// The level grid of a plan (ofdis_out_geometry's OFDIS_OUT_LEVEL): the finest level's plane x 2^sc_l.  One pair's
// float32 grid in bytes, and the view that the warp, interpolation, check, tracker and filter read it through.
size_t level_grid_bytes(const Plan &P) { return (size_t)P.lv[0].w * P.lv[0].h * P.nop * 4; }

ofdis_flow_view level_view(const Plan &P) {
  return ofdis_flow_view{OFDIS_OUT_F32, OFDIS_OUT_INTERLEAVED, OFDIS_OUT_LEVEL, P.lv[0].w, P.lv[0].h, 1 << P.sc_l, P.padl, P.padt};
}

// The forward flows of the chunk in workspace ws as level grids into grid_fw, and (grid_bw not NULL) the backward
// flows into grid_bw; fmt: their dtype and layout, float32 interleaved by default (timer "level_out").
int run_level_out(ofdis_context *c, char *ws, const Plan &P, void *grid_fw, void *grid_bw, hipStream_t s,
                  const OutFmt &fmt = OutFmt()) {
  for (int dir = 0; dir < (grid_bw ? 2 : 1); ++dir) {
    LevelOutArgs lo{};
    lo.flow = (const float *)(ws + (dir ? P.off_flow_bw[0] : P.off_flow[0]));
    lo.out = dir ? grid_bw : grid_fw;
    lo.n = P.n;
    lo.nop = P.nop;
    lo.wl = P.lv[0].w;
    lo.hl = P.lv[0].h;
    lo.log2s = P.sc_l;
    lo.f16 = fmt.f16;
    lo.planar = fmt.planar;
    timed(c, 17, s, [&] { launch_level_out(lo, s); });
    if (hipGetLastError() != hipSuccess) return OFDIS_ERR_DEVICE;
  }
  return OFDIS_OK;
}

// x 2^sc_l + INTER_LINEAR upsample + crop of the finest level's flow in workspace ws (run_dense.cpp:407-415).
// A format other than the plain one (never with `backward`): the formatted store forms, or for the level grid no
// upsample at all -- the level plane x 2^sc_l in the format.
// disp_r (a stereo plan): the mirrored pairs' half of the batch goes there, mirrored back and negated by the store.
int run_upsample(ofdis_context *c, char *ws, const Plan &P, const ofdis_params *p, void *flow_out, hipStream_t s,
                 bool backward = false, const OutFmt &fmt = OutFmt(), float *disp_r = nullptr) {
  if (fmt.level) return run_level_out(c, ws, P, flow_out, nullptr, s, fmt);
  UpArgs up{};
  up.flow = (const float *)(ws + (backward ? P.off_flow_bw[0] : P.off_flow[0]));
  up.out = (float *)flow_out;
  up.n = P.n;
  up.nop = P.nop;
  up.wl = P.lv[0].w;
  up.hl = P.lv[0].h;
  up.log2s = p->sc_l;
  up.W0 = P.W0;
  up.H0 = P.H0;
  up.offx = P.padl;
  up.offy = P.padt;
  up.nt_store = c->opt_nt_store;
  up.form = c->opt_up_form == 3 ? (P.W0 >= 1024 && (c->call_lanes >= 2 || c->call_frames < 1024) ? 1 : 0)
                                 : c->opt_up_form;
  up.f16 = fmt.f16;
  up.planar = fmt.planar;
  up.out_r = disp_r;
  up.n_l = disp_r ? P.n / 2 : P.n;
  timed(c, fmt.f16 ? (fmt.planar ? 16 : 14) : fmt.planar ? 15 : 10, s, [&] { launch_upsample(up, s); });
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// The initial flow of a chunk (device, full resolution [n][H0][W0][nop]) -> OFClass's initflow input in the
// workspace (run_dense.cpp:356-379, restated: ofo_init_flow_area).
int run_init(ofdis_context *c, char *ws, const Plan &P, const ofdis_params *p, const float *init, hipStream_t s) {
  InitArgs ia{};
  ia.init = init;
  ia.out = (float *)(ws + P.off_init);
  ia.n = P.n;
  ia.nop = P.nop;
  ia.W0 = P.W0;
  ia.H0 = P.H0;
  ia.padl = P.padl;
  ia.padt = P.padt;
  ia.log2k = p->sc_f + 1;
  ia.wo = P.Wp >> (p->sc_f + 1);
  ia.ho = P.Hp >> (p->sc_f + 1);
  ia.sc = (float)std::pow(2.0, -p->sc_f - 1);  // flowinit *= sc_fct (float)
  ia.scale = 1.f / (float)(1 << (2 * (p->sc_f + 1)));
  launch_init_area(ia, s);
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// The outputs of a bidirectional call beyond the forward flow (ofdis_run_bidir_u8); at() is a chunk's share.
struct BidirOut {
  float *flow_bw = nullptr;
  uint8_t *occ_fw = nullptr, *occ_bw = nullptr;
  float *err_fw = nullptr, *err_bw = nullptr;
  float alpha = 0.f, beta = 0.f;
  // ofdis_run_stereo_u8: the same five outputs for the right view (flow_bw = disp_r, one component; occ_fw / err_fw
  // the left view's), the check ofdis_lr_check
  bool stereo = false;
  bool checks() const { return occ_fw || occ_bw || err_fw || err_bw; }
  BidirOut at(size_t f0, size_t px) const {
    BidirOut o = *this;
    if (flow_bw) o.flow_bw += f0 * px * (stereo ? 1 : 2);
    if (occ_fw) o.occ_fw += f0 * px;
    if (occ_bw) o.occ_bw += f0 * px;
    if (err_fw) o.err_fw += f0 * px;
    if (err_bw) o.err_bw += f0 * px;
    return o;
  }
};

// The consistency check of n frames (timer "fb_check_err" when an error map is written, else "fb_check").
int run_fb_check(ofdis_context *c, const float *fw, const float *bw, int n, int width, int height, const BidirOut &o,
                 hipStream_t s) {
  FbArgs fa{};
  fa.fw = fw;
  fa.bw = bw;
  fa.occ_fw = o.occ_fw;
  fa.occ_bw = o.occ_bw;
  fa.err_fw = o.err_fw;
  fa.err_bw = o.err_bw;
  fa.n = n;
  fa.W = width;
  fa.H = height;
  fa.alpha = o.alpha;
  fa.beta = o.beta;
  timed(c, o.err_fw || o.err_bw ? 13 : 12, s, [&] { launch_fb_check(fa, s); });
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// The consistency check of n frames on their two float32 interleaved level grids of geometry v (timer
// "fb_check_level").
int run_fb_check_level(ofdis_context *c, const float *gfw, const float *gbw, const ofdis_flow_view &v, int n, int width,
                       int height, const BidirOut &o, hipStream_t s) {
  FbLevelArgs fa{};
  fa.gfw = gfw;
  fa.gbw = gbw;
  fa.occ_fw = o.occ_fw;
  fa.occ_bw = o.occ_bw;
  fa.err_fw = o.err_fw;
  fa.err_bw = o.err_bw;
  fa.n = n;
  fa.W = width;
  fa.H = height;
  fa.alpha = o.alpha;
  fa.beta = o.beta;
  fa.gw = v.gw;
  fa.gh = v.gh;
  fa.offx = v.off_x;
  fa.offy = v.off_y;
  while ((1 << fa.log2c) < v.cell) ++fa.log2c;
  timed(c, 24, s, [&] { launch_fb_check_level(fa, s); });
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// The left-right check of n frames (timer "lr_check_err" when an error map is written, else "lr_check").
int run_lr_check(ofdis_context *c, const float *dl, const float *dr, int n, int width, int height, const BidirOut &o,
                 hipStream_t s) {
  LrArgs la{};
  la.dl = dl;
  la.dr = dr;
  la.occ_l = o.occ_fw;
  la.occ_r = o.occ_bw;
  la.err_l = o.err_fw;
  la.err_r = o.err_bw;
  la.n = n;
  la.W = width;
  la.H = height;
  la.alpha = o.alpha;
  la.beta = o.beta;
  timed(c, o.err_fw || o.err_bw ? 21 : 20, s, [&] { launch_lr_check(la, s); });
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// The picture of a warp (ofdis_warp_u8, ofdis_run_warp_u8); at() is a chunk's share.
struct WarpOut {
  void *out = nullptr;
  uint8_t *valid = nullptr;
  float scale = 1.f;
  int f32 = 0;
  WarpOut at(size_t f0, size_t px, int noc) const {
    WarpOut o = *this;
    o.out = (char *)out + f0 * px * noc * (f32 ? 4 : 1);
    if (valid) o.valid += f0 * px;
    return o;
  }
};

// n frames warped along a flow view (timer "warp_level" for a level-grid view, else "warp").
int run_warp(ofdis_context *c, const uint8_t *img, const void *flow, const ofdis_flow_view &v, int n, int width,
             int height, int noc, const WarpOut &o, hipStream_t s) {
  WarpArgs wa{};
  wa.img = img;
  wa.flow = flow;
  wa.out = o.out;
  wa.valid = o.valid;
  wa.n = n;
  wa.W = width;
  wa.H = height;
  wa.noc = noc;
  wa.scale = o.scale;
  wa.out_f32 = o.f32;
  wa.f16 = v.dtype == OFDIS_OUT_F16;
  wa.planar = v.layout == OFDIS_OUT_PLANAR;
  wa.level = v.grid == OFDIS_OUT_LEVEL;
  if (wa.level) {
    wa.gw = v.gw;
    wa.gh = v.gh;
    wa.offx = v.off_x;
    wa.offy = v.off_y;
    while ((1 << wa.log2c) < v.cell) ++wa.log2c;
  }
  timed(c, wa.level ? 19 : 18, s, [&] { launch_warp(wa, s); });
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// The pictures of an interpolation (ofdis_interp_u8, ofdis_run_interp_u8); at() is a chunk's share.
struct InterpOut {
  void *out = nullptr;
  uint8_t *valid = nullptr;
  const uint8_t *occ_a = nullptr, *occ_b = nullptr;
  int f32 = 0, nt = 0;
  float t[kInterpMaxT] = {};
  // the fused calls with masks (ofdis_run_interp_occ_u8): the masks come from the chunk's level grids at these
  // thresholds and go to the caller's arrays, or where one is NULL to the chunk's workspace
  bool use_occ = false;
  uint8_t *occ_fw = nullptr, *occ_bw = nullptr;
  float alpha = 0.f, beta = 0.f;
  InterpOut at(size_t f0, size_t px, int noc) const {
    InterpOut o = *this;
    o.out = (char *)out + f0 * nt * px * noc * (f32 ? 4 : 1);
    if (valid) o.valid += f0 * nt * px;
    if (occ_fw) o.occ_fw += f0 * px;
    if (occ_bw) o.occ_bw += f0 * px;
    return o;
  }
};

// The frames between n pairs along two flow views of one description (timer "interp_level" for level-grid views,
// else "interp").
int run_interp(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, const void *flow_fw, const void *flow_bw,
               const ofdis_flow_view &v, int n, int width, int height, int noc, const InterpOut &o, hipStream_t s) {
  InterpArgs ia{};
  ia.img_a = img_a;
  ia.img_b = img_b;
  ia.flow_fw = flow_fw;
  ia.flow_bw = flow_bw;
  ia.occ_a = o.occ_a;
  ia.occ_b = o.occ_b;
  ia.out = o.out;
  ia.valid = o.valid;
  ia.n = n;
  ia.W = width;
  ia.H = height;
  ia.noc = noc;
  ia.out_f32 = o.f32;
  ia.f16 = v.dtype == OFDIS_OUT_F16;
  ia.planar = v.layout == OFDIS_OUT_PLANAR;
  ia.level = v.grid == OFDIS_OUT_LEVEL;
  if (ia.level) {
    ia.gw = v.gw;
    ia.gh = v.gh;
    ia.offx = v.off_x;
    ia.offy = v.off_y;
    while ((1 << ia.log2c) < v.cell) ++ia.log2c;
  }
  ia.nt = o.nt;
  std::memcpy(ia.t, o.t, sizeof(ia.t));
  timed(c, ia.level ? 23 : 22, s, [&] { launch_interp(ia, s); });
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// One chunk of frames through the whole pipeline on stream s with workspace ws.  bd (P.bidir): the backward flow
// of the same pyramid upsampled too -- into the workspace when the caller wants only the masks -- and the check.
int run_chunk(ofdis_context *c, char *ws, const Plan &P, const ofdis_params *p, const uint8_t *img_a,
              const uint8_t *img_b, const float *init, void *flow_out, const BidirOut *bd, hipStream_t s,
              const OutFmt &fmt, const WarpOut *wo = nullptr) {
  int rc = run_pyramid(c, ws, P, img_a, img_b, s);
  if (rc) return rc;
  if (init && (rc = run_init(c, ws, P, p, init, s))) return rc;
  rc = run_levels(c, ws, P, p, s, init ? (const float *)(ws + P.off_init) : nullptr, nullptr);
  if (rc) return rc;
  if (P.stereo) {  // both views' fields from the one batch (bd, the plain format), then the check
    float *disp_r = bd->flow_bw ? bd->flow_bw : (float *)(ws + P.off_up_bw);
    if ((rc = run_upsample(c, ws, P, p, flow_out, s, false, fmt, disp_r))) return rc;
    return bd->checks() ? run_lr_check(c, (const float *)flow_out, disp_r, P.n / 2, P.W0, P.H0, *bd, s) : OFDIS_OK;
  }
  rc = run_upsample(c, ws, P, p, flow_out, s, false, fmt);
  // ofdis_run_warp_u8: flow_out is the chunk's float32 level grid (fmt), img_b warped by it
  if (!rc && wo) return run_warp(c, img_b, flow_out, level_view(P), P.n, P.W0, P.H0, P.noc, *wo, s);
  if (rc || !bd) return rc;  // (bd: the plain format, float32 fields)
  float *flow_bw = bd->flow_bw ? bd->flow_bw : (float *)(ws + P.off_up_bw);
  if ((rc = run_upsample(c, ws, P, p, flow_bw, s, true))) return rc;
  return bd->checks() ? run_fb_check(c, (const float *)flow_out, flow_bw, P.n, P.W0, P.H0, *bd, s) : OFDIS_OK;
}

// One chunk of a fused call that reads level grids (the interpolation, the tracker, the temporal filter; P without an
// initial flow, bidirectional when grid_bw is given): the pipeline of run_chunk, then the finest level's flows x 2^sc_l
// as float32 interleaved level grids into grid_fw and grid_bw, the chunk's share of the context's buffer (grid_bw NULL:
// the forward grids alone).  No upsample runs.  A sequence plan reads its n + stride frames from img_a, and not img_b.
int run_chunk_grids(ofdis_context *c, char *ws, const Plan &P, const ofdis_params *p, const uint8_t *img_a,
                    const uint8_t *img_b, void *grid_fw, void *grid_bw, hipStream_t s) {
  int rc = run_pyramid(c, ws, P, img_a, P.seq ? nullptr : img_b, s);
  if (rc) return rc;
  if ((rc = run_levels(c, ws, P, p, s, nullptr, nullptr))) return rc;
  return run_level_out(c, ws, P, grid_fw, grid_bw, s);
}

// One chunk of ofdis_run_interp_u8: its two level grids and the pictures from them.  io.use_occ: the check on the two
// grids in between, its masks read by the interpolation.  A sequence plan: img_a is the chunk's first frame; img_b,
// frame b of the chunk's first pair, is read by the interpolation alone.
int run_chunk_interp(ofdis_context *c, char *ws, const Plan &P, const ofdis_params *p, const uint8_t *img_a,
                     const uint8_t *img_b, void *grid_fw, void *grid_bw, const InterpOut &io, hipStream_t s) {
  int rc = run_chunk_grids(c, ws, P, p, img_a, img_b, grid_fw, grid_bw, s);
  if (rc) return rc;
  const ofdis_flow_view v = level_view(P);
  if (!io.use_occ) return run_interp(c, img_a, img_b, grid_fw, grid_bw, v, P.n, P.W0, P.H0, P.noc, io, s);
  const size_t px = (size_t)P.n * P.W0 * P.H0;
  BidirOut bo;
  bo.occ_fw = io.occ_fw ? io.occ_fw : (uint8_t *)(ws + P.off_up_bw);
  bo.occ_bw = io.occ_bw ? io.occ_bw : (uint8_t *)(ws + P.off_up_bw) + px;
  bo.alpha = io.alpha;
  bo.beta = io.beta;
  if ((rc = run_fb_check_level(c, (const float *)grid_fw, (const float *)grid_bw, v, P.n, P.W0, P.H0, bo, s))) return rc;
  InterpOut masked = io;
  masked.occ_a = bo.occ_fw;
  masked.occ_b = bo.occ_bw;
  return run_interp(c, img_a, img_b, grid_fw, grid_bw, v, P.n, P.W0, P.H0, P.noc, masked, s);
}

// k lanes (stream, done event, workspace of `bytes`).
int ensure_lanes(ofdis_context *c, int k, size_t bytes) {
  if ((int)c->lanes.size() < k) c->lanes.resize(k);
  if (!c->entry) HIP_OK(hipEventCreateWithFlags(&c->entry, hipEventDisableTiming));
  for (int i = 0; i < k; ++i) {
    auto &L = c->lanes[i];
    if (!L.s) HIP_OK(hipStreamCreateWithFlags(&L.s, hipStreamNonBlocking));
    if (!L.done) HIP_OK(hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
    if (L.cap < bytes) {
      if (L.ws) {
        int rc = drop_graph(c);
        if (rc) return rc;
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipFree(L.ws));
        L.ws = nullptr;
        L.cap = 0;
      }
      HIP_OK(hipMalloc(&L.ws, bytes));
      L.cap = bytes;
    }
  }
  return OFDIS_OK;
}

// two lanes from 256 pairs (config D, 256 pairs: 223.4-223.7k on one stream, 225.3-226.8k on two; profiles/r05/s22)
int stream_count(const ofdis_context *c, int n) { return c->opt_streams > 0 ? c->opt_streams : (n >= 256 ? 2 : 1); }

// Frames per launch such that every TV plane group (n * noc * sp floats, addressed with 32-bit byte
// offsets by the system kernels' ldu) stays below 2^30 floats.
int tv_frame_cap(const ofdis_params *p, int width, int height) {
  if (!p->usetvref) return 1 << 30;
  const Plan P1 = batch_plan(p, 1, width, height);
  const long per = (long)P1.noc * (long)P1.tv_plane;
  return (int)std::min((long)(1 << 30), ((1L << 30) - 1) / per);  // 0: one frame alone is too large
}

// Pairs per launch such that no grid y or z exceeds 65535, the limit the sliced launchers (kSlice) assume.  What a
// chunk of m pairs puts there: the pyramid base's z holds every frame (2m of two arrays, m + stride of a sequence);
// the refinement's separate derivative launches (colour with "prepd" < 2) put m * noc in y; aggregation, prep, the
// two-launch system, the red-black SOR, final, upsample and level-out put m in y or z.  (Patch, SOR and the fused
// system kernels count frames in grid x.)  The derivative term is taken whatever "prepd" says, so that the bound
// depends on the parameters alone.  A stride of 65535 or more leaves nothing: < 1.
constexpr int kGridYZ = 65535;
int grid_frame_cap(const ofdis_params *p, int stride) {
  const int per_pair = std::max(stride > 0 ? 1 : 2, p->usetvref ? p->noc : 1);
  return std::min(kGridYZ / per_pair, stride > 0 ? kGridYZ - stride : kGridYZ);
}

// Both rules: the pairs one launch takes (stride > 0: of a sequence chunk).
int frame_cap(const ofdis_params *p, int width, int height, int stride = 0) {
  return std::min(tv_frame_cap(p, width, height), grid_frame_cap(p, stride));
}

// How one call is issued: the whole batch on one stream and workspace (single), or chunks round-robin over
// lanes (round robin).  Everything the issue needs -- workspaces, lane streams, events -- is allocated by
// prepare(), before any capture begins.  (Round 5's software pipeline over a streaming stream and chain lanes,
// with CU-masked streams and a staggered round robin, measured slower in every form and was removed in round 6.)
struct CallPlan {
  enum Kind { kSingle, kRoundRobin } kind = kSingle;
  int n = 0, width = 0, height = 0, chunk = 0, nchunks = 1, lanes = 0;
  bool init = false;
  size_t out_pair = 0;      // bytes of one pair's output in the call's format
  Plan whole;               // kSingle
  std::vector<Plan> parts;  // kRoundRobin: one plan per chunk
};

// The plan of the first chunk: the geometry (levels, padding, components) that every chunk of the call shares.
const Plan &first_plan(const CallPlan &cp) { return cp.kind == CallPlan::kSingle ? cp.whole : cp.parts[0]; }

int prepare(ofdis_context *c, const ofdis_params *p, int n, int width, int height, bool init, bool capturing,
            CallPlan &cp, int bidir = 0, int stride = 0, int stereo = 0) {
  cp.n = n;
  c->call_frames = stereo ? 2 * n : n;  // (a stereo pair is two flow pairs)
  c->call_lanes = 1;
  cp.width = width;
  cp.height = height;
  cp.init = init;
  // a stage capture (frame 0's per-scale flow) runs the batch as one launch on one stream, whatever the
  // stream / chunk options; it is refused only for batches beyond the launch-size cap
  const int nstreams = capturing ? 1 : stream_count(c, c->call_frames);
  int chunk = capturing ? n : c->opt_chunk > 0 ? std::min(c->opt_chunk, n) : (n + nstreams - 1) / nstreams;
  // chunks count stereo pairs: two flow pairs of the launch-size cap each, four frames of the pyramid kernels' grid z
  // (half the pair call's cap bounds both: 4 * (cap / 2) <= 2 * cap)
  chunk = std::min(chunk, stereo ? frame_cap(p, width, height) / 2 : frame_cap(p, width, height, stride));
  if (chunk < 1) return OFDIS_ERR_INVALID_ARGUMENT;
  cp.chunk = chunk;
  cp.nchunks = (n + chunk - 1) / chunk;
  if (cp.nchunks > 1 && capturing) return OFDIS_ERR_UNSUPPORTED;
  if (cp.nchunks == 1) {
    cp.kind = CallPlan::kSingle;
    cp.whole = batch_plan(p, n, width, height, init, bidir, stride, stereo);
    return ensure_ws(c, cp.whole.total);
  }
  cp.kind = CallPlan::kRoundRobin;
  for (int ch = 0; ch < cp.nchunks; ++ch)
    cp.parts.push_back(batch_plan(p, std::min(chunk, n - ch * chunk), width, height, init, bidir, stride, stereo));
  cp.lanes = std::min(nstreams, cp.nchunks);
  c->call_lanes = cp.lanes;
  return ensure_lanes(c, cp.lanes, cp.parts[0].total);
}

// The chunks of a call, each through fn(f0, ws, P, stream) -- the chunk's first pair, workspace, plan and stream.
// Single: the whole batch in the context's workspace on s.  Round robin: the chunks over the lanes, each chunk's whole
// pipeline on one lane (fork from s, join into s; inside a capture the events are recorded into the graph).
// A sequence call: the chunk of m pairs from pair f0 reads frames [f0, f0 + m + stride) of the caller's array, so
// neighbouring chunks rebuild the `stride` frames they share; the outputs are per pair as ever.
template <class Fn>
int for_each_chunk(ofdis_context *c, const CallPlan &cp, hipStream_t s, Fn &&fn) {
  if (cp.kind == CallPlan::kSingle) return fn((size_t)0, c->ws, cp.whole, s);
  const int k = cp.lanes;
  HIP_OK(hipEventRecord(c->entry, s));
  for (int i = 0; i < k; ++i) HIP_OK(hipStreamWaitEvent(c->lanes[i].s, c->entry, 0));
  for (int ch = 0; ch < cp.nchunks; ++ch) {
    auto &L = c->lanes[ch % k];
    const int rc = fn((size_t)ch * cp.chunk, L.ws, cp.parts[ch], L.s);
    if (rc) return rc;
  }
  for (int i = 0; i < k; ++i) {
    HIP_OK(hipEventRecord(c->lanes[i].done, c->lanes[i].s));
    HIP_OK(hipStreamWaitEvent(s, c->lanes[i].done, 0));
  }
  return OFDIS_OK;
}

// Start of a call on stream s: NULL is the legacy default stream (torch's default), which the context's
// non-blocking stream does not order against -- hand its queued work over with an event; and the
// workspaces are shared by every call on this context, whatever its stream -- wait for the previous call.
int call_begin(ofdis_context *c, void *stream, hipStream_t &s) {
  if (!c->ev_null) HIP_OK(hipEventCreateWithFlags(&c->ev_null, hipEventDisableTiming));
  if (!c->ev_ws) HIP_OK(hipEventCreateWithFlags(&c->ev_ws, hipEventDisableTiming));
  s = stream ? (hipStream_t)stream : c->stream;
  if (!stream) {
    HIP_OK(hipEventRecord(c->ev_null, nullptr));
    HIP_OK(hipStreamWaitEvent(s, c->ev_null, 0));
  }
  if (c->ws_pending) HIP_OK(hipStreamWaitEvent(s, c->ev_ws, 0));
  return OFDIS_OK;
}

// End of a call: mark the workspaces' release; a NULL-stream caller's later work waits for the result.
int call_end(ofdis_context *c, void *stream, hipStream_t s) {
  HIP_OK(hipEventRecord(c->ev_ws, s));
  c->ws_pending = true;
  if (!stream) HIP_OK(hipStreamWaitEvent(nullptr, c->ev_ws, 0));
  return OFDIS_OK;
}

int validate_call(const ofdis_params *p, int width, int height, bool init) {
  int rc = ofdis_params_validate(p, -1, -1, -1);
  if (rc) return rc;
  Plan P = batch_plan(p, 1, width, height, init);
  rc = ofdis_params_validate(p, P.Wp, P.Hp, P.pad);
  if (rc) return rc;
  // one frame's TV plane group must stay below 2^30 floats (32-bit byte offsets in the system kernels)
  return tv_frame_cap(p, width, height) >= 1 ? OFDIS_OK : OFDIS_ERR_INVALID_ARGUMENT;
}

// A device entry point's frame around body(s), after its arguments are checked: the context's lock, the refusal of a
// set stage capture for the calls that cannot honour one, the device, the call's ordering on `stream` and the merged
// status.  nothing_asked: the call has no output to write -- OFDIS_OK once it is known to be allowed.
template <class Body>
int device_call(ofdis_context *c, void *stream, bool refuse_capture, Body &&body, bool nothing_asked = false) {
  std::lock_guard<std::mutex> lock(c->mu);
  if (refuse_capture && (!c->cap_dis.empty() || !c->cap_tv.empty())) return OFDIS_ERR_UNSUPPORTED;
  if (nothing_asked) return OFDIS_OK;
  HIP_OK(hipSetDevice(c->device));
  hipStream_t s;
  int rc = call_begin(c, stream, s);
  if (rc) return rc;
  rc = body(s);
  const int rc2 = call_end(c, stream, s);
  return rc ? rc : rc2;
}

// A graph key with the common part filled: the family, the images (a sequence call: stride > 0, b NULL or the
// interpolation's frame `stride`), the initial flow, where the flow goes, the workspace, the sizes and parameters, and
// `buf`, the context's level-grid buffer when the call's flow passes through it.  The family's payload is all zero.
using GraphKey = ofdis_context::GraphKey;
GraphKey graph_key(GraphKey::Family family, const ofdis_context *c, const void *a, const void *b, const void *init,
                   const void *out, const void *buf, int n, int width, int height, int stride, const ofdis_params *p) {
  GraphKey key;
  std::memset(&key, 0, sizeof(key));  // padding included: the key is compared bytewise
  key.family = family;
  key.a = a; key.b = b; key.init = init; key.out = out; key.ws = c->ws; key.buf = buf;
  key.n = n; key.w = width; key.h = height; key.p = *p;
  key.seq = stride > 0; key.stride = stride;  // a sequence call on a plain call's buffers records anew
  return key;
}

// issue(stream) enqueues the whole call.  Eagerly on s: with graph 0, for the multi-lane issues with graph 1 (graph 2
// captures their fork and join too), under the kernel timers or a stage capture.  Else ~80 dependent launches per
// chunk are recorded once as a HIP graph (on the context's own stream -- the caller's may be the legacy NULL stream,
// which cannot capture) and replayed on the caller's stream while the key -- pointers, sizes, parameters, the family's
// own values -- stays the same; set_option and every reallocation drop the graph.  One graph per context: a call with
// another key records anew.
template <class Issue>
int replay_or_record(ofdis_context *c, hipStream_t s, const CallPlan &cp, const GraphKey &key, Issue &&issue) {
  const bool graph = c->opt_graph == 2 || (c->opt_graph == 1 && cp.kind == CallPlan::kSingle);
  if (!graph || !c->cap_dis.empty() || !c->cap_tv.empty() || c->timing) return issue(s);
  if (!c->gexec || std::memcmp(&key, &c->gkey, sizeof(key)) != 0) {
    int rc = drop_graph(c);
    if (rc) return rc;
    OFDIS_TRACE("graph: capture (kind %d, %d chunks of %d)", (int)cp.kind, cp.nchunks, cp.chunk);
    HIP_OK(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
    rc = issue(c->stream);
    OFDIS_TRACE("graph: issued rc %d", rc);
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(c->stream, &graph);
    OFDIS_TRACE("graph: captured rc %d end %d", rc, (int)ce);
    if (rc) {
      if (graph) hipGraphDestroy(graph);
      return rc;
    }
    if (ce != hipSuccess || !graph) return OFDIS_ERR_DEVICE;
    const hipError_t ie = hipGraphInstantiate(&c->gexec, graph, nullptr, nullptr, 0);
    OFDIS_TRACE("graph: instantiated %d", (int)ie);
    hipGraphDestroy(graph);
    if (ie != hipSuccess) {
      c->gexec = nullptr;
      return OFDIS_ERR_DEVICE;
    }
    std::memcpy(&c->gkey, &key, sizeof(key));
  }
  HIP_OK(hipGraphLaunch(c->gexec, s));
  OFDIS_TRACE("graph: launched");
  return OFDIS_OK;
}

// The whole-batch device path on stream s (call ordering done by the caller).  stride > 0: img_a is a sequence of
// n + stride frames and pair i is (frame i, frame i + stride); img_b is NULL.
int run_batch(ofdis_context *c, hipStream_t s, const uint8_t *img_a, const uint8_t *img_b, const float *init, int n,
              int width, int height, const ofdis_params *p, void *flow_out, const BidirOut *bd = nullptr,
              int stride = 0, const OutFmt &fmt = OutFmt(), const WarpOut *wo = nullptr) {
  const bool capturing = !c->cap_dis.empty() || !c->cap_tv.empty();
  CallPlan cp;
  const int keep = bd ? (bd->flow_bw ? 1 : 2) : 0;  // 2: the second field stays in the workspace
  const bool stereo = bd && bd->stereo;
  int rc = prepare(c, p, n, width, height, init != nullptr, capturing, cp, stereo ? 0 : keep, stride, stereo ? keep : 0);
  if (rc) return rc;
  const Plan &P1 = first_plan(cp);
  const size_t px = (size_t)width * height, in_frame = px * p->noc, out_frame = px * P1.nop;
  // a chunk of m pairs from pair f0 writes the bytes [f0, f0 + m) * out_pair of flow_out
  cp.out_pair = (fmt.level ? level_grid_bytes(P1) : out_frame * 4) / (fmt.f16 ? 2 : 1);
  if (wo) {  // ofdis_run_warp_u8 (flow_out NULL, fmt the float32 level grid): the flow goes through the context's buffer
    if ((rc = ensure_warp_buf(c, (size_t)n * cp.out_pair))) return rc;
    flow_out = c->warp_buf;
  }
  OFDIS_TRACE("run_batch: kind %d, %d chunks of %d, %d lanes", (int)cp.kind, cp.nchunks, cp.chunk, cp.lanes);
  GraphKey key = graph_key(GraphKey::kBatch, c, img_a, img_b, init, flow_out, wo ? c->warp_buf : nullptr, n, width,
                           height, stride, p);
  GraphKey::Batch &kb = key.u.batch;
  kb.out_f16 = fmt.f16; kb.out_planar = fmt.planar; kb.out_level = fmt.level;
  if (bd) {  // a plain call after a bidirectional one on the same buffers records anew, and the other way round
    kb.bidir = !bd->stereo; kb.stereo = bd->stereo; kb.flow_bw = bd->flow_bw; kb.occ_fw = bd->occ_fw; kb.occ_bw = bd->occ_bw;
    kb.err_fw = bd->err_fw; kb.err_bw = bd->err_bw; kb.alpha = bd->alpha; kb.beta = bd->beta;
  }
  if (wo) {
    kb.warp = 1; kb.warp_out = wo->out; kb.warp_valid = wo->valid; kb.warp_scale = wo->scale; kb.warp_f32 = wo->f32;
  }
  return replay_or_record(c, s, cp, key, [&](hipStream_t q) {
    return for_each_chunk(c, cp, q, [&](size_t f0, char *ws, const Plan &P, hipStream_t ls) {
      const BidirOut part = bd ? bd->at(f0, px) : BidirOut();
      const WarpOut wpart = wo ? wo->at(f0, px, p->noc) : WarpOut();
      return run_chunk(c, ws, P, p, img_a + f0 * in_frame, img_b ? img_b + f0 * in_frame : nullptr,
                       init ? init + f0 * out_frame : nullptr, (char *)flow_out + f0 * cp.out_pair, bd ? &part : nullptr,
                       ls, fmt, wo ? &wpart : nullptr);
    });
  });
}

// ofdis_run_interp_u8 on stream s (no stage capture is set): the bidirectional plan with nothing kept at full
// resolution and the 2 n level grids in the context's buffer, the n forward grids and then the n backward ones.
// stride > 0: img_a is a sequence of n + stride frames (the sequence plan) and img_b its frame `stride`.
int run_batch_interp(ofdis_context *c, hipStream_t s, const uint8_t *img_a, const uint8_t *img_b, int n, int width,
                     int height, const ofdis_params *p, const InterpOut &io, int stride = 0) {
  CallPlan cp;
  // (masks the caller does not take live in the chunk's workspace)
  int rc = prepare(c, p, n, width, height, false, false, cp, io.use_occ && !(io.occ_fw && io.occ_bw) ? 3 : 1, stride);
  if (rc) return rc;
  cp.out_pair = level_grid_bytes(first_plan(cp));
  if ((rc = ensure_warp_buf(c, 2 * (size_t)n * cp.out_pair))) return rc;  // (drops the graph before it grows)
  char *grids = c->warp_buf, *grids_bw = grids + (size_t)n * cp.out_pair;
  GraphKey key = graph_key(GraphKey::kInterp, c, img_a, img_b, nullptr, grids, grids, n, width, height, stride, p);
  GraphKey::Interp &ki = key.u.interp;
  ki.pictures = io.out; ki.valid = io.valid; ki.f32 = io.f32;
  if (io.use_occ) {  // a call with masks after one without, or with other thresholds or mask arrays, records anew
    ki.use_occ = 1; ki.occ_fw = io.occ_fw; ki.occ_bw = io.occ_bw; ki.alpha = io.alpha; ki.beta = io.beta;
  }
  ki.nt = io.nt;  // and so does the same call with other times
  std::memcpy(ki.t, io.t, sizeof(float) * io.nt);
  const size_t px = (size_t)width * height, in_frame = px * p->noc;
  return replay_or_record(c, s, cp, key, [&](hipStream_t q) {
    return for_each_chunk(c, cp, q, [&](size_t f0, char *ws, const Plan &P, hipStream_t ls) {
      return run_chunk_interp(c, ws, P, p, img_a + f0 * in_frame, img_b + f0 * in_frame, grids + f0 * cp.out_pair,
                              grids_bw + f0 * cp.out_pair, io.at(f0, px, p->noc), ls);
    });
  });
}

// verbosity 2, one pair (the CLI): the reference's stdout timers -- pyramid (run_dense.cpp:352), grid
// allocation (oflow.cpp:177), per-scale stages (oflow.cpp:297) and the OFClass total (oflow.cpp:336) --
// from HIP events around eager launches on the context's stream.
int run_verbose(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, const float *init, int width,
                int height, const ofdis_params *p, float *flow_out) {
  hipStream_t s = c->stream;
  c->call_frames = 1;
  auto t0 = std::chrono::steady_clock::now();
  Plan P = batch_plan(p, 1, width, height, init != nullptr);
  int rc = ensure_ws(c, P.total);
  if (rc) return rc;
  const double alloc_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0));
  HIP_OK(hipEventCreate(&e1));
  HIP_OK(hipEventRecord(e0, s));
  rc = run_pyramid(c, c->ws, P, img_a, img_b, s);
  if (!rc && init) rc = run_init(c, c->ws, P, p, init, s);
  HIP_OK(hipEventRecord(e1, s));
  HIP_OK(hipEventSynchronize(e1));
  float pyr_ms = 0.0f;
  hipEventElapsedTime(&pyr_ms, e0, e1);
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  if (rc) return rc;
  std::printf("TIME (Pyramide+Gradients) (ms): %3g\n", pyr_ms);
  std::printf("TIME (Grid Memo. Alloc. ) (ms): %3g\n", alloc_ms);
  auto t1 = std::chrono::steady_clock::now();
  std::vector<StageTimes> times;
  rc = run_levels(c, c->ws, P, p, s, init ? (const float *)(c->ws + P.off_init) : nullptr, &times);
  if (rc) return rc;
  HIP_OK(hipStreamSynchronize(s));
  const double ms = alloc_ms + std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
  print_times(P, times, ms, p->verbosity);
  return run_upsample(c, c->ws, P, p, flow_out, s);
}

}  // namespace
}  // extern "C++"

int ofdis_run_batch_u8(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height,
                       const ofdis_params *p, float *flow_out, void *stream) {
  return ofdis_run_batch_u8_init(c, img_a, img_b, nullptr, n, width, height, p, flow_out, stream);
}

int ofdis_run_batch_u8_init(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, const float *init, int n,
                            int width, int height, const ofdis_params *p, float *flow_out, void *stream) {
  if (!c || !img_a || !img_b || !flow_out || n <= 0 || width <= 0 || height <= 0) return OFDIS_ERR_INVALID_ARGUMENT;
  const int rc = validate_call(p, width, height, init != nullptr);
  if (rc) return rc;
  return device_call(c, stream, false, [&](hipStream_t s) {
    return run_batch(c, s, img_a, img_b, init, n, width, height, p, flow_out);
  });
}

int ofdis_run_batch_u8_host(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, int n, int width,
                            int height, const ofdis_params *p, float *flow_out) {
  return ofdis_run_batch_u8_init_host(c, img_a, img_b, nullptr, n, width, height, p, flow_out);
}

int ofdis_run_batch_u8_init_host(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, const float *init,
                                 int n, int width, int height, const ofdis_params *p, float *flow_out) {
  if (!c || !img_a || !img_b || !flow_out || n <= 0 || width <= 0 || height <= 0 || !p)
    return OFDIS_ERR_INVALID_ARGUMENT;
  HIP_OK(hipSetDevice(c->device));
  const size_t in = (size_t)n * width * height * p->noc;
  const size_t out = (size_t)n * width * height * (p->mode == OFDIS_MODE_OF ? 2 : 1);
  uint8_t *da = nullptr, *db = nullptr;
  float *dout = nullptr, *dinit = nullptr;
  int rc = OFDIS_OK;
  auto step = [&](hipError_t e) {
    if (e != hipSuccess && rc == OFDIS_OK) rc = e == hipErrorOutOfMemory ? OFDIS_ERR_OUT_OF_MEMORY : OFDIS_ERR_DEVICE;
    return rc == OFDIS_OK;
  };
  if (step(hipMalloc(&da, in)) && step(hipMalloc(&db, in)) && step(hipMalloc(&dout, out * sizeof(float))) &&
      (!init || step(hipMalloc(&dinit, out * sizeof(float)))) &&
      step(hipMemcpyAsync(da, img_a, in, hipMemcpyHostToDevice, c->stream)) &&
      step(hipMemcpyAsync(db, img_b, in, hipMemcpyHostToDevice, c->stream)) &&
      (!init || step(hipMemcpyAsync(dinit, init, out * sizeof(float), hipMemcpyHostToDevice, c->stream)))) {
    const bool verbose = p->verbosity > 1 && n == 1 && c->cap_dis.empty() && c->cap_tv.empty() && !c->timing;
    auto t0 = std::chrono::steady_clock::now();
    if (verbose) {
      rc = validate_call(p, width, height, dinit != nullptr);
      if (!rc) {
        std::lock_guard<std::mutex> lock(c->mu);
        hipStream_t s;
        rc = call_begin(c, c->stream, s);
        if (!rc) rc = run_verbose(c, da, db, dinit, width, height, p, dout);
        if (!rc) rc = call_end(c, c->stream, s);
      }
    } else {
      rc = ofdis_run_batch_u8_init(c, da, db, dinit, n, width, height, p, dout, c->stream);
    }
    if (rc == OFDIS_OK && step(hipStreamSynchronize(c->stream))) {
      const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      if (p->verbosity == 1) std::printf("TIME (O.Flow Run-Time   ) (ms): %3g\n", ms);
      step(hipMemcpy(flow_out, dout, out * sizeof(float), hipMemcpyDeviceToHost));
    }
  }
  hipFree(da);
  hipFree(db);
  hipFree(dout);
  hipFree(dinit);
  return rc;
}

namespace {
bool fb_thresholds_ok(float alpha, float beta) {
  return std::isfinite(alpha) && std::isfinite(beta) && alpha >= 0.0f && beta >= 0.0f;
}
}  // namespace

int ofdis_fb_check(ofdis_context *c, const float *flow_fw, const float *flow_bw, int n, int width, int height,
                   float alpha, float beta, uint8_t *occ_fw, uint8_t *occ_bw, float *err_fw, float *err_bw,
                   void *stream) {
  if (!c || !flow_fw || !flow_bw || n <= 0 || width <= 0 || height <= 0 || !fb_thresholds_ok(alpha, beta) ||
      (long)width * height > 0x7fffffffL)
    return OFDIS_ERR_INVALID_ARGUMENT;
  BidirOut o;
  o.occ_fw = occ_fw;
  o.occ_bw = occ_bw;
  o.err_fw = err_fw;
  o.err_bw = err_bw;
  o.alpha = alpha;
  o.beta = beta;
  if (!o.checks()) return OFDIS_OK;
  return device_call(c, stream, false,
                     [&](hipStream_t s) { return run_fb_check(c, flow_fw, flow_bw, n, width, height, o, s); });
}

int ofdis_run_bidir_u8(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height,
                       const ofdis_params *p, float alpha, float beta, float *flow_fw, float *flow_bw,
                       uint8_t *occ_fw, uint8_t *occ_bw, float *err_fw, float *err_bw, void *stream) {
  if (!c || !img_a || !img_b || !flow_fw || n <= 0 || width <= 0 || height <= 0 || !p ||
      !fb_thresholds_ok(alpha, beta) || (long)width * height > 0x7fffffffL)
    return OFDIS_ERR_INVALID_ARGUMENT;
  int rc = validate_call(p, width, height, false);
  if (rc) return rc;
  if (p->mode != OFDIS_MODE_OF) return OFDIS_ERR_UNSUPPORTED;  // the depth path's right-camera clamp has no pinned counterpart
  BidirOut o;
  o.flow_bw = flow_bw;
  o.occ_fw = occ_fw;
  o.occ_bw = occ_bw;
  o.err_fw = err_fw;
  o.err_bw = err_bw;
  o.alpha = alpha;
  o.beta = beta;
  return device_call(c, stream, true, [&](hipStream_t s) {
    // nothing but the forward flow asked for: the plain call
    return run_batch(c, s, img_a, img_b, nullptr, n, width, height, p, flow_fw, flow_bw || o.checks() ? &o : nullptr);
  });
}

extern "C++" {  // (a template)
namespace {
// Host form of a call on two images that returns two fields of `comp` components, two masks and two error maps, any
// but the first field optional (ofdis_run_bidir_u8: comp = 2, ofdis_run_stereo_u8: comp = 1).  One device block: the two
// images, then (each at a multiple of 256 bytes) the outputs the caller asked for; call(img_a, img_b, f, u) issues
// the device form on the context's stream with the device pointers (NULL where the host pointer is).  Synchronous.
template <class Call>
int two_field_host(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, size_t px, int noc, int comp,
                   float *const (&host_f)[4], uint8_t *const (&host_u)[2], Call &&call) {
  HIP_OK(hipSetDevice(c->device));
  const size_t in = px * noc;
  const size_t bytes_f[4] = {px * comp * sizeof(float), px * comp * sizeof(float), px * sizeof(float), px * sizeof(float)};
  size_t off_f[4], off_u[2], total = align_up(in) * 2;
  for (int k = 0; k < 4; ++k) {
    off_f[k] = total;
    if (host_f[k]) total += align_up(bytes_f[k]);
  }
  for (int k = 0; k < 2; ++k) {
    off_u[k] = total;
    if (host_u[k]) total += align_up(px);
  }
  char *d = nullptr;
  HIP_OK(hipMalloc(&d, total));
  int rc = OFDIS_OK;
  auto step = [&](hipError_t e) {
    if (e != hipSuccess && rc == OFDIS_OK) rc = e == hipErrorOutOfMemory ? OFDIS_ERR_OUT_OF_MEMORY : OFDIS_ERR_DEVICE;
    return rc == OFDIS_OK;
  };
  float *dev_f[4];
  uint8_t *dev_u[2];
  for (int k = 0; k < 4; ++k) dev_f[k] = host_f[k] ? (float *)(d + off_f[k]) : nullptr;
  for (int k = 0; k < 2; ++k) dev_u[k] = host_u[k] ? (uint8_t *)(d + off_u[k]) : nullptr;
  if (step(hipMemcpyAsync(d, img_a, in, hipMemcpyHostToDevice, c->stream)) &&
      step(hipMemcpyAsync(d + align_up(in), img_b, in, hipMemcpyHostToDevice, c->stream))) {
    rc = call((const uint8_t *)d, (const uint8_t *)(d + align_up(in)), dev_f, dev_u);
    if (rc == OFDIS_OK && step(hipStreamSynchronize(c->stream))) {
      for (int k = 0; k < 4; ++k)
        if (host_f[k]) step(hipMemcpy(host_f[k], d + off_f[k], bytes_f[k], hipMemcpyDeviceToHost));
      for (int k = 0; k < 2; ++k)
        if (host_u[k]) step(hipMemcpy(host_u[k], d + off_u[k], px, hipMemcpyDeviceToHost));
    }
  }
  hipFree(d);
  return rc;
}
}  // namespace
}  // extern "C++"

int ofdis_run_bidir_u8_host(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height,
                            const ofdis_params *p, float alpha, float beta, float *flow_fw, float *flow_bw,
                            uint8_t *occ_fw, uint8_t *occ_bw, float *err_fw, float *err_bw) {
  if (!c || !img_a || !img_b || !flow_fw || n <= 0 || width <= 0 || height <= 0 || !p)
    return OFDIS_ERR_INVALID_ARGUMENT;
  float *const host_f[4] = {flow_fw, flow_bw, err_fw, err_bw};
  uint8_t *const host_u[2] = {occ_fw, occ_bw};
  return two_field_host(c, img_a, img_b, (size_t)n * width * height, p->noc, 2, host_f, host_u,
                        [&](const uint8_t *a, const uint8_t *b, float *const *f, uint8_t *const *u) {
                          return ofdis_run_bidir_u8(c, a, b, n, width, height, p, alpha, beta, f[0], f[1], u[0], u[1],
                                                    f[2], f[3], c->stream);
                        });
}

int ofdis_lr_check(ofdis_context *c, const float *disp_l, const float *disp_r, int n, int width, int height,
                   float alpha, float beta, uint8_t *occ_l, uint8_t *occ_r, float *err_l, float *err_r, void *stream) {
  if (!c || !disp_l || !disp_r || n <= 0 || width <= 0 || height <= 0 || !fb_thresholds_ok(alpha, beta) ||
      (long)width * height > 0x7fffffffL)
    return OFDIS_ERR_INVALID_ARGUMENT;
  BidirOut o;
  o.stereo = true;
  o.occ_fw = occ_l;
  o.occ_bw = occ_r;
  o.err_fw = err_l;
  o.err_bw = err_r;
  o.alpha = alpha;
  o.beta = beta;
  if (!o.checks()) return OFDIS_OK;
  return device_call(c, stream, false,
                     [&](hipStream_t s) { return run_lr_check(c, disp_l, disp_r, n, width, height, o, s); });
}

int ofdis_run_stereo_u8(ofdis_context *c, const uint8_t *img_l, const uint8_t *img_r, int n, int width, int height,
                        const ofdis_params *p, float alpha, float beta, float *disp_l, float *disp_r, uint8_t *occ_l,
                        uint8_t *occ_r, float *err_l, float *err_r, void *stream) {
  if (!c || !img_l || !img_r || !disp_l || n <= 0 || width <= 0 || height <= 0 || !p ||
      !fb_thresholds_ok(alpha, beta) || (long)width * height > 0x7fffffffL)
    return OFDIS_ERR_INVALID_ARGUMENT;
  int rc = validate_call(p, width, height, false);
  if (rc) return rc;
  if (p->mode != OFDIS_MODE_DE) return OFDIS_ERR_UNSUPPORTED;  // two views of one scene: a stereo pair
  BidirOut o;
  o.stereo = true;
  o.flow_bw = disp_r;
  o.occ_fw = occ_l;
  o.occ_bw = occ_r;
  o.err_fw = err_l;
  o.err_bw = err_r;
  o.alpha = alpha;
  o.beta = beta;
  return device_call(c, stream, true, [&](hipStream_t s) {
    // nothing but the left view's disparity asked for: the plain call
    return run_batch(c, s, img_l, img_r, nullptr, n, width, height, p, disp_l, disp_r || o.checks() ? &o : nullptr);
  });
}

int ofdis_run_stereo_u8_host(ofdis_context *c, const uint8_t *img_l, const uint8_t *img_r, int n, int width, int height,
                             const ofdis_params *p, float alpha, float beta, float *disp_l, float *disp_r,
                             uint8_t *occ_l, uint8_t *occ_r, float *err_l, float *err_r) {
  if (!c || !img_l || !img_r || !disp_l || n <= 0 || width <= 0 || height <= 0 || !p)
    return OFDIS_ERR_INVALID_ARGUMENT;
  float *const host_f[4] = {disp_l, disp_r, err_l, err_r};
  uint8_t *const host_u[2] = {occ_l, occ_r};
  return two_field_host(c, img_l, img_r, (size_t)n * width * height, p->noc, 1, host_f, host_u,
                        [&](const uint8_t *l, const uint8_t *r, float *const *f, uint8_t *const *u) {
                          return ofdis_run_stereo_u8(c, l, r, n, width, height, p, alpha, beta, f[0], f[1], u[0], u[1],
                                                     f[2], f[3], c->stream);
                        });
}

int ofdis_run_sequence_u8(ofdis_context *c, const uint8_t *frames, int nframes, int stride, const float *init,
                          int width, int height, const ofdis_params *p, float alpha, float beta, float *flow_fw,
                          float *flow_bw, uint8_t *occ_fw, uint8_t *occ_bw, float *err_fw, float *err_bw,
                          void *stream) {
  if (!c || !frames || !flow_fw || width <= 0 || height <= 0 || !p || stride < 1 || nframes <= stride)
    return OFDIS_ERR_INVALID_ARGUMENT;
  BidirOut o;
  o.flow_bw = flow_bw;
  o.occ_fw = occ_fw;
  o.occ_bw = occ_bw;
  o.err_fw = err_fw;
  o.err_bw = err_bw;
  o.alpha = alpha;
  o.beta = beta;
  const bool bidir = flow_bw || o.checks();
  if (bidir && (!fb_thresholds_ok(alpha, beta) || (long)width * height > 0x7fffffffL)) return OFDIS_ERR_INVALID_ARGUMENT;
  int rc = validate_call(p, width, height, init != nullptr);
  if (rc) return rc;
  if (p->mode != OFDIS_MODE_OF) return OFDIS_ERR_UNSUPPORTED;  // a stereo pair is not a sequence
  if (init && bidir) return OFDIS_ERR_UNSUPPORTED;              // no pinned initial backward flow
  return device_call(c, stream, bidir, [&](hipStream_t s) {
    return run_batch(c, s, frames, nullptr, init, nframes - stride, width, height, p, flow_fw, bidir ? &o : nullptr, stride);
  });
}

int ofdis_run_sequence_u8_host(ofdis_context *c, const uint8_t *frames, int nframes, int stride, const float *init,
                               int width, int height, const ofdis_params *p, float alpha, float beta, float *flow_fw,
                               float *flow_bw, uint8_t *occ_fw, uint8_t *occ_bw, float *err_fw, float *err_bw) {
  if (!c || !frames || !flow_fw || width <= 0 || height <= 0 || !p || stride < 1 || nframes <= stride)
    return OFDIS_ERR_INVALID_ARGUMENT;
  if (p->mode != OFDIS_MODE_OF) return OFDIS_ERR_UNSUPPORTED;  // (the buffers below are sized for two components)
  HIP_OK(hipSetDevice(c->device));
  const size_t px = (size_t)(nframes - stride) * width * height, in = (size_t)nframes * width * height * p->noc;
  // one device block: the frames, then (each at a multiple of 256 bytes) the initial flow and the outputs asked for
  float *const host_f[4] = {flow_fw, flow_bw, err_fw, err_bw};
  uint8_t *const host_u[2] = {occ_fw, occ_bw};
  const size_t bytes_f[4] = {px * 2 * sizeof(float), px * 2 * sizeof(float), px * sizeof(float), px * sizeof(float)};
  size_t off_f[4], off_u[2], total = align_up(in);
  const size_t off_init = total;
  if (init) total += align_up(bytes_f[0]);
  for (int k = 0; k < 4; ++k) {
    off_f[k] = total;
    if (host_f[k]) total += align_up(bytes_f[k]);
  }
  for (int k = 0; k < 2; ++k) {
    off_u[k] = total;
    if (host_u[k]) total += align_up(px);
  }
  char *d = nullptr;
  HIP_OK(hipMalloc(&d, total));
  int rc = OFDIS_OK;
  auto step = [&](hipError_t e) {
    if (e != hipSuccess && rc == OFDIS_OK) rc = e == hipErrorOutOfMemory ? OFDIS_ERR_OUT_OF_MEMORY : OFDIS_ERR_DEVICE;
    return rc == OFDIS_OK;
  };
  auto dev_f = [&](int k) { return host_f[k] ? (float *)(d + off_f[k]) : nullptr; };
  auto dev_u = [&](int k) { return host_u[k] ? (uint8_t *)(d + off_u[k]) : nullptr; };
  if (step(hipMemcpyAsync(d, frames, in, hipMemcpyHostToDevice, c->stream)) &&
      (!init || step(hipMemcpyAsync(d + off_init, init, bytes_f[0], hipMemcpyHostToDevice, c->stream)))) {
    rc = ofdis_run_sequence_u8(c, (const uint8_t *)d, nframes, stride, init ? (const float *)(d + off_init) : nullptr,
                               width, height, p, alpha, beta, dev_f(0), dev_f(1), dev_u(0), dev_u(1), dev_f(2),
                               dev_f(3), c->stream);
    if (rc == OFDIS_OK && step(hipStreamSynchronize(c->stream))) {
      for (int k = 0; k < 4; ++k)
        if (host_f[k]) step(hipMemcpy(host_f[k], d + off_f[k], bytes_f[k], hipMemcpyDeviceToHost));
      for (int k = 0; k < 2; ++k)
        if (host_u[k]) step(hipMemcpy(host_u[k], d + off_u[k], px, hipMemcpyDeviceToHost));
    }
  }
  hipFree(d);
  return rc;
}

// ------------------------------------------------------------------ output formats (include/ofdis.h)

namespace {
// fmt (NULL: the plain format) checked and restated; bytes: one pair's output.  With one component the two layouts
// are one: planar is dropped, so {F32, PLANAR, FULL} of a depth call is the plain call.  The formatted kernels index
// with 64-bit offsets; frames of 2^31 pixels or more are refused all the same (as ofdis_fb_check does), so that a
// pixel index within a plane always fits an int.
int out_format(const ofdis_params *p, int width, int height, bool init, const ofdis_out_format *fmt, OutFmt &of,
               size_t &bytes) {
  const int rc = ofdis_out_geometry(p, width, height, init, fmt, nullptr, nullptr, nullptr, nullptr, nullptr, &bytes);
  if (rc) return rc;
  of = OutFmt();
  if (!fmt) return OFDIS_OK;
  of.f16 = fmt->dtype == OFDIS_OUT_F16;
  of.planar = fmt->layout == OFDIS_OUT_PLANAR && p->mode == OFDIS_MODE_OF;
  of.level = fmt->grid == OFDIS_OUT_LEVEL;
  if (!of.plain() && (long)width * height > 0x7fffffffL) return OFDIS_ERR_INVALID_ARGUMENT;
  return OFDIS_OK;
}
}  // namespace

int ofdis_run_batch_u8_fmt(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, const float *init, int n,
                           int width, int height, const ofdis_params *p, const ofdis_out_format *fmt, void *flow_out,
                           void *stream) {
  if (!c || !img_a || !img_b || !flow_out || n <= 0 || width <= 0 || height <= 0) return OFDIS_ERR_INVALID_ARGUMENT;
  OutFmt of;
  size_t bytes = 0;
  int rc = out_format(p, width, height, init != nullptr, fmt, of, bytes);
  if (rc) return rc;
  if (of.plain())  // the existing path and kernel instantiations
    return ofdis_run_batch_u8_init(c, img_a, img_b, init, n, width, height, p, (float *)flow_out, stream);
  if ((rc = validate_call(p, width, height, init != nullptr))) return rc;
  return device_call(c, stream, false, [&](hipStream_t s) {
    return run_batch(c, s, img_a, img_b, init, n, width, height, p, flow_out, nullptr, 0, of);
  });
}

int ofdis_run_sequence_u8_fmt(ofdis_context *c, const uint8_t *frames, int nframes, int stride, const float *init,
                              int width, int height, const ofdis_params *p, const ofdis_out_format *fmt, void *flow_fw,
                              void *stream) {
  if (!c || !frames || !flow_fw || width <= 0 || height <= 0 || !p || stride < 1 || nframes <= stride)
    return OFDIS_ERR_INVALID_ARGUMENT;
  OutFmt of;
  size_t bytes = 0;
  int rc = out_format(p, width, height, init != nullptr, fmt, of, bytes);
  if (rc) return rc;
  if (of.plain())
    return ofdis_run_sequence_u8(c, frames, nframes, stride, init, width, height, p, 0.f, 0.f, (float *)flow_fw,
                                 nullptr, nullptr, nullptr, nullptr, nullptr, stream);
  if ((rc = validate_call(p, width, height, init != nullptr))) return rc;
  if (p->mode != OFDIS_MODE_OF) return OFDIS_ERR_UNSUPPORTED;  // a stereo pair is not a sequence
  return device_call(c, stream, false, [&](hipStream_t s) {
    return run_batch(c, s, frames, nullptr, init, nframes - stride, width, height, p, flow_fw, nullptr, stride, of);
  });
}

namespace {
// The host forms: frames (two arrays of nfr frames, or one when img_b is NULL) and the initial flow of n pairs up,
// the device call, n * bytes down (synchronous).
using FmtCall = std::function<int(const uint8_t *, const uint8_t *, const float *, void *)>;
int run_fmt_host(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, size_t nfr, const float *init, size_t n,
                 int width, int height, const ofdis_params *p, const ofdis_out_format *fmt, void *flow_out,
                 const FmtCall &call) {
  OutFmt of;
  size_t bytes = 0;
  int rc = out_format(p, width, height, init != nullptr, fmt, of, bytes);
  if (rc) return rc;
  HIP_OK(hipSetDevice(c->device));
  const size_t in = align_up(nfr * width * height * p->noc);
  const size_t ini = init ? align_up(n * width * height * (p->mode == OFDIS_MODE_OF ? 2 : 1) * sizeof(float)) : 0;
  const size_t off_b = in, off_init = img_b ? 2 * in : in, off_out = off_init + ini;
  char *d = nullptr;
  HIP_OK(hipMalloc(&d, off_out + n * bytes));
  auto step = [&](hipError_t e) {
    if (e != hipSuccess && rc == OFDIS_OK) rc = e == hipErrorOutOfMemory ? OFDIS_ERR_OUT_OF_MEMORY : OFDIS_ERR_DEVICE;
    return rc == OFDIS_OK;
  };
  const size_t in_bytes = nfr * width * height * p->noc;
  if (step(hipMemcpyAsync(d, img_a, in_bytes, hipMemcpyHostToDevice, c->stream)) &&
      (!img_b || step(hipMemcpyAsync(d + off_b, img_b, in_bytes, hipMemcpyHostToDevice, c->stream))) &&
      (!init || step(hipMemcpyAsync(d + off_init, init, n * width * height * (p->mode == OFDIS_MODE_OF ? 2 : 1) *
                                                            sizeof(float), hipMemcpyHostToDevice, c->stream)))) {
    rc = call((const uint8_t *)d, img_b ? (const uint8_t *)(d + off_b) : nullptr,
              init ? (const float *)(d + off_init) : nullptr, (void *)(d + off_out));
    if (rc == OFDIS_OK && step(hipStreamSynchronize(c->stream)))
      step(hipMemcpy(flow_out, d + off_out, n * bytes, hipMemcpyDeviceToHost));
  }
  hipFree(d);
  return rc;
}
}  // namespace

int ofdis_run_batch_u8_fmt_host(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, const float *init, int n,
                                int width, int height, const ofdis_params *p, const ofdis_out_format *fmt,
                                void *flow_out) {
  if (!c || !img_a || !img_b || !flow_out || n <= 0 || width <= 0 || height <= 0 || !p)
    return OFDIS_ERR_INVALID_ARGUMENT;
  return run_fmt_host(c, img_a, img_b, (size_t)n, init, (size_t)n, width, height, p, fmt, flow_out,
                      [&](const uint8_t *da, const uint8_t *db, const float *di, void *dout) {
                        return ofdis_run_batch_u8_fmt(c, da, db, di, n, width, height, p, fmt, dout, c->stream);
                      });
}

int ofdis_run_sequence_u8_fmt_host(ofdis_context *c, const uint8_t *frames, int nframes, int stride, const float *init,
                                   int width, int height, const ofdis_params *p, const ofdis_out_format *fmt,
                                   void *flow_fw) {
  if (!c || !frames || !flow_fw || width <= 0 || height <= 0 || !p || stride < 1 || nframes <= stride)
    return OFDIS_ERR_INVALID_ARGUMENT;
  if (p->mode != OFDIS_MODE_OF) return OFDIS_ERR_UNSUPPORTED;
  return run_fmt_host(c, frames, nullptr, (size_t)nframes, init, (size_t)(nframes - stride), width, height, p, fmt,
                      flow_fw, [&](const uint8_t *df, const uint8_t *, const float *di, void *dout) {
                        return ofdis_run_sequence_u8_fmt(c, df, nframes, stride, di, width, height, p, fmt, dout,
                                                         c->stream);
                      });
}

// ------------------------------------------------------------------ warping (include/ofdis.h)

namespace {
bool img_dtype_ok(int d) { return d == OFDIS_IMG_U8 || d == OFDIS_IMG_F32; }
}  // namespace

int ofdis_warp_u8(ofdis_context *c, const uint8_t *img, const void *flow, const ofdis_flow_view *v, int n, int width,
                  int height, int noc, float scale, int out_dtype, void *out, uint8_t *valid, void *stream) {
  if (!c || !img || !flow || !v || !out || n <= 0 || width <= 0 || height <= 0 || (noc != 1 && noc != 3) ||
      !std::isfinite(scale) || !img_dtype_ok(out_dtype) || (long)width * height > 0x7fffffffL)
    return OFDIS_ERR_INVALID_ARGUMENT;
  if ((v->dtype != OFDIS_OUT_F32 && v->dtype != OFDIS_OUT_F16) ||
      (v->layout != OFDIS_OUT_INTERLEAVED && v->layout != OFDIS_OUT_PLANAR) ||
      (v->grid != OFDIS_OUT_FULL && v->grid != OFDIS_OUT_LEVEL))
    return OFDIS_ERR_INVALID_ARGUMENT;
  if (v->grid == OFDIS_OUT_LEVEL) {
    if (v->cell < 1 || v->cell > 512 || (v->cell & (v->cell - 1)) || v->gw <= 0 || v->gh <= 0 || v->off_x < 0 ||
        v->off_y < 0 || (long)v->gw * v->cell < (long)width + v->off_x || (long)v->gh * v->cell < (long)height + v->off_y)
      return OFDIS_ERR_INVALID_ARGUMENT;
  }
  WarpOut o;
  o.out = out;
  o.valid = valid;
  o.scale = scale;
  o.f32 = out_dtype == OFDIS_IMG_F32;
  return device_call(c, stream, false,
                     [&](hipStream_t s) { return run_warp(c, img, flow, *v, n, width, height, noc, o, s); });
}

int ofdis_run_warp_u8(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height,
                      const ofdis_params *p, float scale, int out_dtype, void *out, uint8_t *valid, void *stream) {
  if (!c || !img_a || !img_b || !out || n <= 0 || width <= 0 || height <= 0 || !p || !std::isfinite(scale) ||
      !img_dtype_ok(out_dtype) || (long)width * height > 0x7fffffffL)
    return OFDIS_ERR_INVALID_ARGUMENT;
  int rc = validate_call(p, width, height, false);
  if (rc) return rc;
  if (p->mode != OFDIS_MODE_OF) return OFDIS_ERR_UNSUPPORTED;  // a disparity is not a flow view
  WarpOut o;
  o.out = out;
  o.valid = valid;
  o.scale = scale;
  o.f32 = out_dtype == OFDIS_IMG_F32;
  OutFmt of;
  of.level = 1;  // float32, interleaved
  return device_call(c, stream, false, [&](hipStream_t s) {
    return run_batch(c, s, img_a, img_b, nullptr, n, width, height, p, nullptr, nullptr, 0, of, &o);
  });
}

int ofdis_run_warp_u8_host(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height,
                           const ofdis_params *p, float scale, int out_dtype, void *out, uint8_t *valid) {
  if (!c || !img_a || !img_b || !out || n <= 0 || width <= 0 || height <= 0 || !p || !img_dtype_ok(out_dtype) ||
      (p->noc != 1 && p->noc != 3))
    return OFDIS_ERR_INVALID_ARGUMENT;
  HIP_OK(hipSetDevice(c->device));
  const size_t px = (size_t)n * width * height, in = px * p->noc, outb = in * (out_dtype == OFDIS_IMG_F32 ? 4 : 1);
  // one device block: the two images, the picture, the mask (each at a multiple of 256 bytes)
  const size_t off_b = align_up(in), off_out = 2 * align_up(in), off_valid = off_out + align_up(outb);
  char *d = nullptr;
  HIP_OK(hipMalloc(&d, off_valid + (valid ? px : 0)));
  int rc = OFDIS_OK;
  auto step = [&](hipError_t e) {
    if (e != hipSuccess && rc == OFDIS_OK) rc = e == hipErrorOutOfMemory ? OFDIS_ERR_OUT_OF_MEMORY : OFDIS_ERR_DEVICE;
    return rc == OFDIS_OK;
  };
  if (step(hipMemcpyAsync(d, img_a, in, hipMemcpyHostToDevice, c->stream)) &&
      step(hipMemcpyAsync(d + off_b, img_b, in, hipMemcpyHostToDevice, c->stream))) {
    rc = ofdis_run_warp_u8(c, (const uint8_t *)d, (const uint8_t *)(d + off_b), n, width, height, p, scale, out_dtype,
                           d + off_out, valid ? (uint8_t *)(d + off_valid) : nullptr, c->stream);
    if (rc == OFDIS_OK && step(hipStreamSynchronize(c->stream))) {
      step(hipMemcpy(out, d + off_out, outb, hipMemcpyDeviceToHost));
      if (valid) step(hipMemcpy(valid, d + off_valid, px, hipMemcpyDeviceToHost));
    }
  }
  hipFree(d);
  return rc;
}

// ------------------------------------------------------------------ frame interpolation (include/ofdis.h)

static_assert(OFDIS_INTERP_MAX_T == kInterpMaxT, "the header's limit is the kernel argument's array");

namespace {
// A flow view an interpolation of width x height frames can read: what ofdis_warp_u8 accepts.
bool flow_view_ok(const ofdis_flow_view *v, int width, int height) {
  if ((v->dtype != OFDIS_OUT_F32 && v->dtype != OFDIS_OUT_F16) ||
      (v->layout != OFDIS_OUT_INTERLEAVED && v->layout != OFDIS_OUT_PLANAR) ||
      (v->grid != OFDIS_OUT_FULL && v->grid != OFDIS_OUT_LEVEL))
    return false;
  if (v->grid == OFDIS_OUT_LEVEL) {
    if (v->cell < 1 || v->cell > 512 || (v->cell & (v->cell - 1)) || v->gw <= 0 || v->gh <= 0 || v->off_x < 0 ||
        v->off_y < 0 || (long)v->gw * v->cell < (long)width + v->off_x || (long)v->gh * v->cell < (long)height + v->off_y)
      return false;
  }
  return true;
}

// The times of an interpolation: 1 .. OFDIS_INTERP_MAX_T finite values in [0, 1].
bool interp_times_ok(const float *t, int nt) {
  if (!t || nt < 1 || nt > OFDIS_INTERP_MAX_T) return false;
  for (int k = 0; k < nt; ++k)
    if (!(t[k] >= 0.0f && t[k] <= 1.0f)) return false;  // (false for NaN)
  return true;
}
}  // namespace

int ofdis_interp_u8(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, const void *flow_fw,
                    const void *flow_bw, const ofdis_flow_view *v, int n, int width, int height, int noc, const float *t,
                    int nt, const uint8_t *occ_a, const uint8_t *occ_b, int out_dtype, void *out, uint8_t *valid,
                    void *stream) {
  if (!c || !img_a || !img_b || !flow_fw || !flow_bw || !v || !out || n <= 0 || width <= 0 || height <= 0 ||
      (noc != 1 && noc != 3) || !img_dtype_ok(out_dtype) || (long)width * height > 0x7fffffffL ||
      !interp_times_ok(t, nt) || !flow_view_ok(v, width, height))
    return OFDIS_ERR_INVALID_ARGUMENT;
  InterpOut o;
  o.out = out;
  o.valid = valid;
  o.occ_a = occ_a;
  o.occ_b = occ_b;
  o.f32 = out_dtype == OFDIS_IMG_F32;
  o.nt = nt;
  std::memcpy(o.t, t, sizeof(float) * nt);
  return device_call(c, stream, false, [&](hipStream_t s) {
    return run_interp(c, img_a, img_b, flow_fw, flow_bw, *v, n, width, height, noc, o, s);
  });
}

int ofdis_run_interp_u8_host(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height,
                             const ofdis_params *p, const float *t, int nt, int out_dtype, void *out, uint8_t *valid) {
  if (!c || !img_a || !img_b || !out || n <= 0 || width <= 0 || height <= 0 || !p || !img_dtype_ok(out_dtype) ||
      (p->noc != 1 && p->noc != 3) || !interp_times_ok(t, nt))
    return OFDIS_ERR_INVALID_ARGUMENT;
  HIP_OK(hipSetDevice(c->device));
  const size_t px = (size_t)n * width * height, in = px * p->noc, outb = in * nt * (out_dtype == OFDIS_IMG_F32 ? 4 : 1);
  // one device block: the two images, the pictures, the masks (each at a multiple of 256 bytes)
  const size_t off_b = align_up(in), off_out = 2 * align_up(in), off_valid = off_out + align_up(outb);
  char *d = nullptr;
  HIP_OK(hipMalloc(&d, off_valid + (valid ? px * nt : 0)));
  int rc = OFDIS_OK;
  auto step = [&](hipError_t e) {
    if (e != hipSuccess && rc == OFDIS_OK) rc = e == hipErrorOutOfMemory ? OFDIS_ERR_OUT_OF_MEMORY : OFDIS_ERR_DEVICE;
    return rc == OFDIS_OK;
  };
  if (step(hipMemcpyAsync(d, img_a, in, hipMemcpyHostToDevice, c->stream)) &&
      step(hipMemcpyAsync(d + off_b, img_b, in, hipMemcpyHostToDevice, c->stream))) {
    rc = ofdis_run_interp_u8(c, (const uint8_t *)d, (const uint8_t *)(d + off_b), n, width, height, p, t, nt, out_dtype,
                             d + off_out, valid ? (uint8_t *)(d + off_valid) : nullptr, c->stream);
    if (rc == OFDIS_OK && step(hipStreamSynchronize(c->stream))) {
      step(hipMemcpy(out, d + off_out, outb, hipMemcpyDeviceToHost));
      if (valid) step(hipMemcpy(valid, d + off_valid, px * nt, hipMemcpyDeviceToHost));
    }
  }
  hipFree(d);
  return rc;
}

// ------------------------------------------------- occlusion masks on level grids, video interpolation (include/ofdis.h)

int ofdis_fb_check_level(ofdis_context *c, const float *grid_fw, const float *grid_bw, const ofdis_flow_view *v, int n,
                         int width, int height, float alpha, float beta, uint8_t *occ_fw, uint8_t *occ_bw,
                         float *err_fw, float *err_bw, void *stream) {
  if (!c || !grid_fw || !grid_bw || !v || n <= 0 || width <= 0 || height <= 0 || !fb_thresholds_ok(alpha, beta) ||
      (long)width * height > 0x7fffffffL)
    return OFDIS_ERR_INVALID_ARGUMENT;
  if ((v->dtype != OFDIS_OUT_F32 && v->dtype != OFDIS_OUT_F16) ||
      (v->layout != OFDIS_OUT_INTERLEAVED && v->layout != OFDIS_OUT_PLANAR) ||
      (v->grid != OFDIS_OUT_FULL && v->grid != OFDIS_OUT_LEVEL))
    return OFDIS_ERR_INVALID_ARGUMENT;
  if (v->dtype != OFDIS_OUT_F32 || v->layout != OFDIS_OUT_INTERLEAVED || v->grid != OFDIS_OUT_LEVEL)
    return OFDIS_ERR_UNSUPPORTED;  // the float32 interleaved level grid alone
  if (!flow_view_ok(v, width, height)) return OFDIS_ERR_INVALID_ARGUMENT;
  BidirOut o;
  o.occ_fw = occ_fw;
  o.occ_bw = occ_bw;
  o.err_fw = err_fw;
  o.err_bw = err_bw;
  o.alpha = alpha;
  o.beta = beta;
  if (!o.checks()) return OFDIS_OK;
  return device_call(c, stream, false, [&](hipStream_t s) {
    return run_fb_check_level(c, grid_fw, grid_bw, *v, n, width, height, o, s);
  });
}

namespace {
// The fused interpolation calls: ofdis_run_interp_u8, with masks (use_occ: their thresholds checked too) and on the
// sequence plan (stride > 0: img_a is the array of n + stride frames).
int run_interp_call(ofdis_context *c, const uint8_t *img_a, int n, int stride, const uint8_t *img_b, int width,
                    int height, const ofdis_params *p, const float *t, int nt, bool use_occ, float alpha, float beta,
                    int out_dtype, void *out, uint8_t *valid, uint8_t *occ_fw, uint8_t *occ_bw, void *stream) {
  if (!c || !img_a || !out || n <= 0 || width <= 0 || height <= 0 || !p || !img_dtype_ok(out_dtype) ||
      (long)width * height > 0x7fffffffL || !interp_times_ok(t, nt) || (use_occ && !fb_thresholds_ok(alpha, beta)))
    return OFDIS_ERR_INVALID_ARGUMENT;
  int rc = validate_call(p, width, height, false);
  if (rc) return rc;
  if (p->mode != OFDIS_MODE_OF) return OFDIS_ERR_UNSUPPORTED;  // (as ofdis_run_bidir_u8)
  InterpOut o;
  o.out = out;
  o.valid = valid;
  o.f32 = out_dtype == OFDIS_IMG_F32;
  o.nt = nt;
  std::memcpy(o.t, t, sizeof(float) * nt);
  if (use_occ) {
    o.use_occ = true;
    o.occ_fw = occ_fw;
    o.occ_bw = occ_bw;
    o.alpha = alpha;
    o.beta = beta;
  }
  if (stride > 0) img_b = img_a + (size_t)stride * width * height * p->noc;
  return device_call(c, stream, true, [&](hipStream_t s) {
    return run_batch_interp(c, s, img_a, img_b, n, width, height, p, o, stride);
  });
}

// Host form of run_interp_call (synchronous): one device block -- the in_a bytes of img_a, the in_b bytes of img_b (a
// sequence has none), the pictures, and the masks asked for, each at a multiple of 256 bytes.
int run_interp_call_host(ofdis_context *c, const uint8_t *img_a, size_t in_a, const uint8_t *img_b, size_t in_b, int n,
                         int stride, int width, int height, const ofdis_params *p, const float *t, int nt, bool use_occ,
                         float alpha, float beta, int out_dtype, void *out, uint8_t *valid, uint8_t *occ_fw,
                         uint8_t *occ_bw) {
  HIP_OK(hipSetDevice(c->device));
  const size_t px = (size_t)n * width * height, outb = px * p->noc * nt * (out_dtype == OFDIS_IMG_F32 ? 4 : 1);
  uint8_t *const host_u[3] = {valid, use_occ ? occ_fw : nullptr, use_occ ? occ_bw : nullptr};
  const size_t bytes_u[3] = {px * nt, px, px};
  const size_t off_b = align_up(in_a), off_out = off_b + align_up(in_b);
  size_t off_u[3], total = off_out + align_up(outb);
  for (int k = 0; k < 3; ++k) {
    off_u[k] = total;
    if (host_u[k]) total += align_up(bytes_u[k]);
  }
  char *d = nullptr;
  HIP_OK(hipMalloc(&d, total));
  int rc = OFDIS_OK;
  auto step = [&](hipError_t e) {
    if (e != hipSuccess && rc == OFDIS_OK) rc = e == hipErrorOutOfMemory ? OFDIS_ERR_OUT_OF_MEMORY : OFDIS_ERR_DEVICE;
    return rc == OFDIS_OK;
  };
  auto dev_u = [&](int k) { return host_u[k] ? (uint8_t *)(d + off_u[k]) : nullptr; };
  if (step(hipMemcpyAsync(d, img_a, in_a, hipMemcpyHostToDevice, c->stream)) &&
      (!in_b || step(hipMemcpyAsync(d + off_b, img_b, in_b, hipMemcpyHostToDevice, c->stream)))) {
    rc = run_interp_call(c, (const uint8_t *)d, n, stride, in_b ? (const uint8_t *)(d + off_b) : nullptr, width, height,
                         p, t, nt, use_occ, alpha, beta, out_dtype, d + off_out, dev_u(0), dev_u(1), dev_u(2), c->stream);
    if (rc == OFDIS_OK && step(hipStreamSynchronize(c->stream))) {
      step(hipMemcpy(out, d + off_out, outb, hipMemcpyDeviceToHost));
      for (int k = 0; k < 3; ++k)
        if (host_u[k]) step(hipMemcpy(host_u[k], d + off_u[k], bytes_u[k], hipMemcpyDeviceToHost));
    }
  }
  hipFree(d);
  return rc;
}
}  // namespace

int ofdis_run_interp_u8(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height,
                        const ofdis_params *p, const float *t, int nt, int out_dtype, void *out, uint8_t *valid,
                        void *stream) {
  if (!img_b) return OFDIS_ERR_INVALID_ARGUMENT;
  return run_interp_call(c, img_a, n, 0, img_b, width, height, p, t, nt, false, 0.f, 0.f, out_dtype, out, valid, nullptr,
                         nullptr, stream);
}

int ofdis_run_interp_occ_u8(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height,
                            const ofdis_params *p, const float *t, int nt, float alpha, float beta, int out_dtype,
                            void *out, uint8_t *valid, uint8_t *occ_fw, uint8_t *occ_bw, void *stream) {
  if (!img_b) return OFDIS_ERR_INVALID_ARGUMENT;
  return run_interp_call(c, img_a, n, 0, img_b, width, height, p, t, nt, true, alpha, beta, out_dtype, out, valid, occ_fw,
                         occ_bw, stream);
}

int ofdis_run_interp_occ_u8_host(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, int n, int width,
                                 int height, const ofdis_params *p, const float *t, int nt, float alpha, float beta,
                                 int out_dtype, void *out, uint8_t *valid, uint8_t *occ_fw, uint8_t *occ_bw) {
  if (!c || !img_a || !img_b || !out || n <= 0 || width <= 0 || height <= 0 || !p || !img_dtype_ok(out_dtype) ||
      (p->noc != 1 && p->noc != 3) || !interp_times_ok(t, nt))
    return OFDIS_ERR_INVALID_ARGUMENT;
  const size_t in = (size_t)n * width * height * p->noc;
  return run_interp_call_host(c, img_a, in, img_b, in, n, 0, width, height, p, t, nt, true, alpha, beta, out_dtype, out,
                              valid, occ_fw, occ_bw);
}

int ofdis_run_sequence_interp_u8(ofdis_context *c, const uint8_t *frames, int nframes, int stride, int width,
                                 int height, const ofdis_params *p, const float *t, int nt, int use_occ, float alpha,
                                 float beta, int out_dtype, void *out, uint8_t *valid, uint8_t *occ_fw,
                                 uint8_t *occ_bw, void *stream) {
  if (stride < 1 || nframes <= stride) return OFDIS_ERR_INVALID_ARGUMENT;
  return run_interp_call(c, frames, nframes - stride, stride, nullptr, width, height, p, t, nt, use_occ != 0, alpha,
                         beta, out_dtype, out, valid, occ_fw, occ_bw, stream);
}

int ofdis_run_sequence_interp_u8_host(ofdis_context *c, const uint8_t *frames, int nframes, int stride, int width,
                                      int height, const ofdis_params *p, const float *t, int nt, int use_occ,
                                      float alpha, float beta, int out_dtype, void *out, uint8_t *valid,
                                      uint8_t *occ_fw, uint8_t *occ_bw) {
  if (!c || !frames || !out || stride < 1 || nframes <= stride || width <= 0 || height <= 0 || !p ||
      !img_dtype_ok(out_dtype) || (p->noc != 1 && p->noc != 3) || !interp_times_ok(t, nt))
    return OFDIS_ERR_INVALID_ARGUMENT;
  return run_interp_call_host(c, frames, (size_t)nframes * width * height * p->noc, nullptr, 0, nframes - stride, stride,
                              width, height, p, t, nt, use_occ != 0, alpha, beta, out_dtype, out, valid, occ_fw, occ_bw);
}

// ------------------------------------------------------------------ point tracking (include/ofdis.h)

namespace {
// The points and outputs of a tracking call (ofdis_track_points, ofdis_run_sequence_track_u8).
struct TrackIo {
  const float *points = nullptr;
  const int32_t *start = nullptr;
  int npts = 0, flags = 0;
  bool use_fb = false;
  float alpha = 0.f, beta = 0.f;
  float *tracks = nullptr;
  uint8_t *status = nullptr;
};

// What every tracking call checks of its points, flags, thresholds and frame size.
bool track_io_ok(const TrackIo &io, int width, int height) {
  return io.points && io.npts >= 1 && !(io.flags & ~OFDIS_TRACK_LAST) && width > 0 && height > 0 &&
         (long)width * height <= 0x7fffffffL && (!io.use_fb || fb_thresholds_ok(io.alpha, io.beta));
}

// The points through m fields of view v (timer "track_level" for a level-grid view, else "track").
int run_track(ofdis_context *c, const void *fw, const void *bw, const ofdis_flow_view &v, int m, int width, int height,
              const TrackIo &io, hipStream_t s) {
  TrackArgs ta{};
  ta.fw = fw;
  ta.bw = bw;
  ta.points = io.points;
  ta.start = io.start;
  ta.tracks = io.tracks;
  ta.status = io.status;
  ta.m = m;
  ta.npts = io.npts;
  ta.W = width;
  ta.H = height;
  ta.alpha = io.alpha;
  ta.beta = io.beta;
  ta.last = (io.flags & OFDIS_TRACK_LAST) != 0;
  ta.f16 = v.dtype == OFDIS_OUT_F16;
  ta.planar = v.layout == OFDIS_OUT_PLANAR;
  ta.level = v.grid == OFDIS_OUT_LEVEL;
  if (ta.level) {
    ta.gw = v.gw;
    ta.gh = v.gh;
    ta.offx = v.off_x;
    ta.offy = v.off_y;
    while ((1 << ta.log2c) < v.cell) ++ta.log2c;
  }
  timed(c, ta.level ? 26 : 25, s, [&] { launch_track(ta, s); });
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// ofdis_run_sequence_track_u8 on stream s (no stage capture is set): the sequence plan of stride 1, bidirectional with
// use_fb; the m forward level grids in the context's buffer and then, with use_fb, the m backward ones, every chunk
// writing its share; after the chunks one track launch on s over all grids.
int run_batch_track(ofdis_context *c, hipStream_t s, const uint8_t *frames, int m, int width, int height,
                    const ofdis_params *p, const TrackIo &io) {
  CallPlan cp;
  int rc = prepare(c, p, m, width, height, false, false, cp, io.use_fb ? 1 : 0, 1);
  if (rc) return rc;
  const ofdis_flow_view v = level_view(first_plan(cp));
  cp.out_pair = level_grid_bytes(first_plan(cp));
  if ((rc = ensure_warp_buf(c, (io.use_fb ? 2 : 1) * (size_t)m * cp.out_pair))) return rc;  // (drops the graph before it grows)
  char *grids = c->warp_buf, *grids_bw = io.use_fb ? grids + (size_t)m * cp.out_pair : nullptr;
  GraphKey key = graph_key(GraphKey::kTrack, c, frames, nullptr, nullptr, grids, grids, m, width, height, 1, p);
  GraphKey::Track &kt = key.u.track;
  kt.points = io.points; kt.start = io.start; kt.tracks = io.tracks; kt.status = io.status;
  kt.npts = io.npts; kt.flags = io.flags;
  if (io.use_fb) {
    kt.use_fb = 1; kt.alpha = io.alpha; kt.beta = io.beta;
  }
  const size_t in_frame = (size_t)width * height * p->noc;
  return replay_or_record(c, s, cp, key, [&](hipStream_t q) {
    const int err = for_each_chunk(c, cp, q, [&](size_t f0, char *ws, const Plan &P, hipStream_t ls) {
      return run_chunk_grids(c, ws, P, p, frames + f0 * in_frame, nullptr, grids + f0 * cp.out_pair,
                             grids_bw ? grids_bw + f0 * cp.out_pair : nullptr, ls);
    });
    return err ? err : run_track(c, grids, grids_bw, v, m, width, height, io, q);
  });
}
}  // namespace

int ofdis_track_points(ofdis_context *c, const void *flow_fw, const void *flow_bw, const ofdis_flow_view *v, int m,
                       int width, int height, const float *points, const int32_t *start, int npts, float alpha,
                       float beta, int flags, float *tracks, uint8_t *status, void *stream) {
  TrackIo io;
  io.points = points;
  io.start = start;
  io.npts = npts;
  io.flags = flags;
  io.use_fb = flow_bw != nullptr;
  io.alpha = alpha;
  io.beta = beta;
  io.tracks = tracks;
  io.status = status;
  if (!c || !flow_fw || !v || m < 1 || !track_io_ok(io, width, height)) return OFDIS_ERR_INVALID_ARGUMENT;
  if ((v->dtype != OFDIS_OUT_F32 && v->dtype != OFDIS_OUT_F16) ||
      (v->layout != OFDIS_OUT_INTERLEAVED && v->layout != OFDIS_OUT_PLANAR) ||
      (v->grid != OFDIS_OUT_FULL && v->grid != OFDIS_OUT_LEVEL))
    return OFDIS_ERR_INVALID_ARGUMENT;
  if (v->grid == OFDIS_OUT_LEVEL && (v->dtype != OFDIS_OUT_F32 || v->layout != OFDIS_OUT_INTERLEAVED))
    return OFDIS_ERR_UNSUPPORTED;  // level grids: float32 interleaved alone (as ofdis_fb_check_level)
  if (!flow_view_ok(v, width, height)) return OFDIS_ERR_INVALID_ARGUMENT;
  if (!tracks && !status) return OFDIS_OK;
  return device_call(c, stream, false,
                     [&](hipStream_t s) { return run_track(c, flow_fw, flow_bw, *v, m, width, height, io, s); });
}

int ofdis_run_sequence_track_u8(ofdis_context *c, const uint8_t *frames, int nframes, int width, int height,
                                const ofdis_params *p, const float *points, const int32_t *start, int npts, int use_fb,
                                float alpha, float beta, int flags, float *tracks, uint8_t *status, void *stream) {
  TrackIo io;
  io.points = points;
  io.start = start;
  io.npts = npts;
  io.flags = flags;
  io.use_fb = use_fb != 0;
  io.alpha = alpha;
  io.beta = beta;
  io.tracks = tracks;
  io.status = status;
  if (!c || !frames || !p || nframes < 2 || !track_io_ok(io, width, height)) return OFDIS_ERR_INVALID_ARGUMENT;
  int rc = validate_call(p, width, height, false);
  if (rc) return rc;
  if (p->mode != OFDIS_MODE_OF) return OFDIS_ERR_UNSUPPORTED;  // a stereo pair is not a sequence
  return device_call(
      c, stream, true, [&](hipStream_t s) { return run_batch_track(c, s, frames, nframes - 1, width, height, p, io); },
      !tracks && !status);
}

int ofdis_run_sequence_track_u8_host(ofdis_context *c, const uint8_t *frames, int nframes, int width, int height,
                                     const ofdis_params *p, const float *points, const int32_t *start, int npts,
                                     int use_fb, float alpha, float beta, int flags, float *tracks, uint8_t *status) {
  if (!c || !frames || !p || nframes < 2 || width <= 0 || height <= 0 || !points || npts < 1 ||
      (flags & ~OFDIS_TRACK_LAST) || (p->noc != 1 && p->noc != 3))
    return OFDIS_ERR_INVALID_ARGUMENT;
  HIP_OK(hipSetDevice(c->device));
  const size_t in = (size_t)nframes * width * height * p->noc, np = (size_t)npts;
  const size_t entries = (flags & OFDIS_TRACK_LAST) ? np : np * (size_t)nframes;
  // one device block: the frames, the points, the starts, the tracks, the status (each at a multiple of 256 bytes)
  const size_t off_pts = align_up(in), off_start = off_pts + align_up(np * 8), off_tr = off_start + align_up(np * 4);
  const size_t off_st = off_tr + align_up(entries * 8);
  char *d = nullptr;
  HIP_OK(hipMalloc(&d, off_st + align_up(entries)));
  int rc = OFDIS_OK;
  auto step = [&](hipError_t e) {
    if (e != hipSuccess && rc == OFDIS_OK) rc = e == hipErrorOutOfMemory ? OFDIS_ERR_OUT_OF_MEMORY : OFDIS_ERR_DEVICE;
    return rc == OFDIS_OK;
  };
  if (step(hipMemcpyAsync(d, frames, in, hipMemcpyHostToDevice, c->stream)) &&
      step(hipMemcpyAsync(d + off_pts, points, np * 8, hipMemcpyHostToDevice, c->stream)) &&
      (!start || step(hipMemcpyAsync(d + off_start, start, np * 4, hipMemcpyHostToDevice, c->stream)))) {
    rc = ofdis_run_sequence_track_u8(c, (const uint8_t *)d, nframes, width, height, p, (const float *)(d + off_pts),
                                     start ? (const int32_t *)(d + off_start) : nullptr, npts, use_fb, alpha, beta, flags,
                                     tracks ? (float *)(d + off_tr) : nullptr, status ? (uint8_t *)(d + off_st) : nullptr,
                                     c->stream);
    if (rc == OFDIS_OK && step(hipStreamSynchronize(c->stream))) {
      if (tracks) step(hipMemcpy(tracks, d + off_tr, entries * 8, hipMemcpyDeviceToHost));
      if (status) step(hipMemcpy(status, d + off_st, entries, hipMemcpyDeviceToHost));
    }
  }
  hipFree(d);
  return rc;
}

// ------------------------------------------------------------------ temporal filter (include/ofdis.h)

namespace {
// The parameters and outputs of a filtering call (ofdis_tfilter_u8, ofdis_run_sequence_tfilter_u8).
struct TfilterIo {
  float sigma = 0.f;
  const uint8_t *occ_fw = nullptr, *occ_bw = nullptr;  // the primitive's masks
  bool use_occ = false;                                // the fused call: masks from the chunks' grids at alpha, beta
  float alpha = 0.f, beta = 0.f;
  int radius = 0;       // the radius calls (ofdis_tfilter_radius_u8, ...): 1 .. 4, and whether every chain step is
  bool use_fb = false;  // checked at alpha, beta
  int f32 = 0;
  void *out = nullptr;
  uint8_t *used = nullptr;
};

// What every filtering call checks of its frames, sigma and outputs.
bool tfilter_io_ok(const TfilterIo &io, const uint8_t *frames, int nframes, int width, int height, int noc, int out_dtype) {
  if (!frames || !io.out || nframes < 2 || width <= 0 || height <= 0 || (noc != 1 && noc != 3) ||
      (long)width * height > 0x7fffffffL || !img_dtype_ok(out_dtype))
    return false;
  if (!(io.sigma >= 1.0f / 1024.0f && io.sigma <= 65536.0f)) return false;  // (false for NaN)
  // neighbours are read after a frame is written: the picture must not overlap the frames
  const size_t in = (size_t)nframes * width * height * noc, outb = in * (out_dtype == OFDIS_IMG_F32 ? 4 : 1);
  const uintptr_t f = (uintptr_t)frames, o = (uintptr_t)io.out;
  return f + in <= o || o + outb <= f;
}

// The kernel arguments of a filtering call on the two chains of view v.
TfilterArgs tfilter_args(const uint8_t *frames, int nframes, const void *fw, const void *bw, const ofdis_flow_view &v,
                         int width, int height, int noc, const TfilterIo &io) {
  TfilterArgs ta{};
  ta.frames = frames;
  ta.fw = fw;
  ta.bw = bw;
  ta.occ_fw = io.occ_fw;
  ta.occ_bw = io.occ_bw;
  ta.out = io.out;
  ta.used = io.used;
  ta.T = nframes;
  ta.W = width;
  ta.H = height;
  ta.noc = noc;
  ta.inv = 1.0f / (io.sigma * (float)noc);
  ta.out_f32 = io.f32;
  ta.f16 = v.dtype == OFDIS_OUT_F16;
  ta.planar = v.layout == OFDIS_OUT_PLANAR;
  ta.level = v.grid == OFDIS_OUT_LEVEL;
  if (ta.level) {
    ta.gw = v.gw;
    ta.gh = v.gh;
    ta.offx = v.off_x;
    ta.offy = v.off_y;
    while ((1 << ta.log2c) < v.cell) ++ta.log2c;
  }
  return ta;
}

// The T frames filtered along the two chains of view v (timer "tfilter_level" for a level-grid view, else "tfilter").
int run_tfilter(ofdis_context *c, const uint8_t *frames, int nframes, const void *fw, const void *bw,
                const ofdis_flow_view &v, int width, int height, int noc, const TfilterIo &io, hipStream_t s) {
  const TfilterArgs ta = tfilter_args(frames, nframes, fw, bw, v, width, height, noc, io);
  timed(c, ta.level ? 28 : 27, s, [&] { launch_tfilter(ta, s); });
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// The same over io.radius frames on each side (timers "tfilter_radius_level" / "tfilter_radius").
int run_tfilter_radius(ofdis_context *c, const uint8_t *frames, int nframes, const void *fw, const void *bw,
                       const ofdis_flow_view &v, int width, int height, int noc, const TfilterIo &io, hipStream_t s) {
  TfilterRadiusArgs ra{};
  ra.f = tfilter_args(frames, nframes, fw, bw, v, width, height, noc, io);
  ra.radius = io.radius;
  ra.use_fb = io.use_fb;
  ra.alpha = io.alpha;
  ra.beta = io.beta;
  timed(c, ra.f.level ? 34 : 33, s, [&] { launch_tfilter_radius(ra, s); });
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// ofdis_run_sequence_tfilter_u8 on stream s (no stage capture is set): run_batch_track's plan, always bidirectional;
// the 2 m level grids in the context's buffer and, with masks, the 2 m masks (u8 [2][m][H][W], the forward ones first)
// behind them in the same buffer.  Every chunk writes its share of the grids and, with masks, runs the check on its own
// grids into its share of the masks; after the chunks one filter launch on s over all frames.
int run_batch_tfilter(ofdis_context *c, hipStream_t s, const uint8_t *frames, int m, int width, int height,
                      const ofdis_params *p, const TfilterIo &io) {
  CallPlan cp;
  int rc = prepare(c, p, m, width, height, false, false, cp, 1, 1);
  if (rc) return rc;
  const ofdis_flow_view v = level_view(first_plan(cp));
  cp.out_pair = level_grid_bytes(first_plan(cp));
  const size_t px = (size_t)width * height, in_frame = px * p->noc;
  const size_t grid_bytes = align_up(2 * (size_t)m * cp.out_pair);
  const size_t mask_bytes = io.use_occ ? 2 * (size_t)m * px : 0;  // sized per call
  if ((rc = ensure_warp_buf(c, grid_bytes + mask_bytes))) return rc;  // (drops the graph before it grows)
  char *grids = c->warp_buf, *grids_bw = grids + (size_t)m * cp.out_pair;
  uint8_t *masks = io.use_occ ? (uint8_t *)c->warp_buf + grid_bytes : nullptr, *masks_bw = masks ? masks + (size_t)m * px : nullptr;
  GraphKey key = graph_key(GraphKey::kTfilter, c, frames, nullptr, nullptr, grids, grids, m, width, height, 1, p);
  GraphKey::Tfilter &kf = key.u.tfilter;
  kf.picture = io.out; kf.used = io.used; kf.f32 = io.f32; kf.sigma = io.sigma; kf.masks = masks;
  if (io.use_occ) {
    kf.alpha = io.alpha; kf.beta = io.beta;
  }
  return replay_or_record(c, s, cp, key, [&](hipStream_t q) {
    const int err = for_each_chunk(c, cp, q, [&](size_t f0, char *ws, const Plan &P, hipStream_t ls) {
      char *gfw = grids + f0 * cp.out_pair, *gbw = grids_bw + f0 * cp.out_pair;
      const int err = run_chunk_grids(c, ws, P, p, frames + f0 * in_frame, nullptr, gfw, gbw, ls);
      if (err || !io.use_occ) return err;
      BidirOut bo;
      bo.occ_fw = masks + f0 * px;
      bo.occ_bw = masks_bw + f0 * px;
      bo.alpha = io.alpha;
      bo.beta = io.beta;
      return run_fb_check_level(c, (const float *)gfw, (const float *)gbw, level_view(P), P.n, P.W0, P.H0, bo, ls);
    });
    if (err) return err;
    TfilterIo fio = io;  // the filter reads the call's own masks
    fio.occ_fw = masks;
    fio.occ_bw = masks_bw;
    return run_tfilter(c, frames, m + 1, grids, grids_bw, v, width, height, p->noc, fio, q);
  });
}

// ofdis_run_sequence_tfilter_radius_u8 on stream s: run_batch_tfilter's plan without the mask planes and without the
// check's launches -- every chunk writes its share of the 2 m level grids, then one filter launch on s over all frames.
int run_batch_tfilter_radius(ofdis_context *c, hipStream_t s, const uint8_t *frames, int m, int width, int height,
                             const ofdis_params *p, const TfilterIo &io) {
  CallPlan cp;
  int rc = prepare(c, p, m, width, height, false, false, cp, 1, 1);
  if (rc) return rc;
  const ofdis_flow_view v = level_view(first_plan(cp));
  cp.out_pair = level_grid_bytes(first_plan(cp));
  const size_t in_frame = (size_t)width * height * p->noc;
  if ((rc = ensure_warp_buf(c, 2 * (size_t)m * cp.out_pair))) return rc;  // (drops the graph before it grows)
  char *grids = c->warp_buf, *grids_bw = grids + (size_t)m * cp.out_pair;
  GraphKey key = graph_key(GraphKey::kTfilterRadius, c, frames, nullptr, nullptr, grids, grids, m, width, height, 1, p);
  GraphKey::TfilterRadius &kf = key.u.tfilter_radius;
  kf.picture = io.out; kf.used = io.used; kf.f32 = io.f32; kf.radius = io.radius; kf.sigma = io.sigma;
  kf.use_fb = io.use_fb;
  if (io.use_fb) {
    kf.alpha = io.alpha; kf.beta = io.beta;
  }
  return replay_or_record(c, s, cp, key, [&](hipStream_t q) {
    const int err = for_each_chunk(c, cp, q, [&](size_t f0, char *ws, const Plan &P, hipStream_t ls) {
      return run_chunk_grids(c, ws, P, p, frames + f0 * in_frame, nullptr, grids + f0 * cp.out_pair,
                             grids_bw + f0 * cp.out_pair, ls);
    });
    if (err) return err;
    return run_tfilter_radius(c, frames, m + 1, grids, grids_bw, v, width, height, p->noc, io, q);
  });
}

// What the radius calls check beyond tfilter_io_ok.
bool tfilter_radius_ok(const TfilterIo &io) {
  return io.radius >= 1 && io.radius <= 4 && (!io.use_fb || fb_thresholds_ok(io.alpha, io.beta));
}
}  // namespace

int ofdis_tfilter_u8(ofdis_context *c, const uint8_t *frames, int nframes, const void *flow_fw, const void *flow_bw,
                     const ofdis_flow_view *v, int width, int height, int noc, float sigma, const uint8_t *occ_fw,
                     const uint8_t *occ_bw, int out_dtype, void *out, uint8_t *used, void *stream) {
  TfilterIo io;
  io.sigma = sigma;
  io.occ_fw = occ_fw;
  io.occ_bw = occ_bw;
  io.f32 = out_dtype == OFDIS_IMG_F32;
  io.out = out;
  io.used = used;
  if (!c || !flow_fw || !flow_bw || !v || !tfilter_io_ok(io, frames, nframes, width, height, noc, out_dtype))
    return OFDIS_ERR_INVALID_ARGUMENT;
  if ((v->dtype != OFDIS_OUT_F32 && v->dtype != OFDIS_OUT_F16) ||
      (v->layout != OFDIS_OUT_INTERLEAVED && v->layout != OFDIS_OUT_PLANAR) ||
      (v->grid != OFDIS_OUT_FULL && v->grid != OFDIS_OUT_LEVEL))
    return OFDIS_ERR_INVALID_ARGUMENT;
  if (v->grid == OFDIS_OUT_LEVEL && (v->dtype != OFDIS_OUT_F32 || v->layout != OFDIS_OUT_INTERLEAVED))
    return OFDIS_ERR_UNSUPPORTED;  // level grids: float32 interleaved alone (as ofdis_track_points)
  if (!flow_view_ok(v, width, height)) return OFDIS_ERR_INVALID_ARGUMENT;
  return device_call(c, stream, false, [&](hipStream_t s) {
    return run_tfilter(c, frames, nframes, flow_fw, flow_bw, *v, width, height, noc, io, s);
  });
}

int ofdis_run_sequence_tfilter_u8(ofdis_context *c, const uint8_t *frames, int nframes, int width, int height,
                                  const ofdis_params *p, float sigma, int use_occ, float alpha, float beta,
                                  int out_dtype, void *out, uint8_t *used, void *stream) {
  TfilterIo io;
  io.sigma = sigma;
  io.use_occ = use_occ != 0;
  io.alpha = alpha;
  io.beta = beta;
  io.f32 = out_dtype == OFDIS_IMG_F32;
  io.out = out;
  io.used = used;
  if (!c || !p || !tfilter_io_ok(io, frames, nframes, width, height, p->noc, out_dtype) ||
      (io.use_occ && !fb_thresholds_ok(alpha, beta)))
    return OFDIS_ERR_INVALID_ARGUMENT;
  int rc = validate_call(p, width, height, false);
  if (rc) return rc;
  if (p->mode != OFDIS_MODE_OF) return OFDIS_ERR_UNSUPPORTED;  // a stereo pair is not a sequence
  return device_call(c, stream, true, [&](hipStream_t s) {
    return run_batch_tfilter(c, s, frames, nframes - 1, width, height, p, io);
  });
}

extern "C++" {  // (a template)
namespace {
// The host forms of the fused filters: the frames up, call(frames, out, used) on the context's stream, the picture and
// the `used` bytes down (synchronous).
template <class Call>
int tfilter_host(ofdis_context *c, const uint8_t *frames, int nframes, int width, int height, const ofdis_params *p,
                 int out_dtype, void *out, uint8_t *used, Call &&call) {
  if (!c || !frames || !p || !out || nframes < 2 || width <= 0 || height <= 0 || !img_dtype_ok(out_dtype) ||
      (p->noc != 1 && p->noc != 3))
    return OFDIS_ERR_INVALID_ARGUMENT;
  HIP_OK(hipSetDevice(c->device));
  const size_t px = (size_t)nframes * width * height, in = px * p->noc, outb = in * (out_dtype == OFDIS_IMG_F32 ? 4 : 1);
  // one device block: the frames, the picture, the `used` bytes (each at a multiple of 256 bytes)
  const size_t off_out = align_up(in), off_used = off_out + align_up(outb);
  char *d = nullptr;
  HIP_OK(hipMalloc(&d, off_used + (used ? px : 0)));
  int rc = OFDIS_OK;
  auto step = [&](hipError_t e) {
    if (e != hipSuccess && rc == OFDIS_OK) rc = e == hipErrorOutOfMemory ? OFDIS_ERR_OUT_OF_MEMORY : OFDIS_ERR_DEVICE;
    return rc == OFDIS_OK;
  };
  if (step(hipMemcpyAsync(d, frames, in, hipMemcpyHostToDevice, c->stream))) {
    rc = call((const uint8_t *)d, (void *)(d + off_out), used ? (uint8_t *)(d + off_used) : nullptr);
    if (rc == OFDIS_OK && step(hipStreamSynchronize(c->stream))) {
      step(hipMemcpy(out, d + off_out, outb, hipMemcpyDeviceToHost));
      if (used) step(hipMemcpy(used, d + off_used, px, hipMemcpyDeviceToHost));
    }
  }
  hipFree(d);
  return rc;
}
}  // namespace
}  // extern "C++"

int ofdis_run_sequence_tfilter_u8_host(ofdis_context *c, const uint8_t *frames, int nframes, int width, int height,
                                       const ofdis_params *p, float sigma, int use_occ, float alpha, float beta,
                                       int out_dtype, void *out, uint8_t *used) {
  return tfilter_host(c, frames, nframes, width, height, p, out_dtype, out, used, [&](const uint8_t *d, void *dout, uint8_t *dused) {
    return ofdis_run_sequence_tfilter_u8(c, d, nframes, width, height, p, sigma, use_occ, alpha, beta, out_dtype, dout,
                                         dused, c->stream);
  });
}

int ofdis_tfilter_radius_u8(ofdis_context *c, const uint8_t *frames, int nframes, const void *flow_fw,
                            const void *flow_bw, const ofdis_flow_view *v, int width, int height, int noc, int radius,
                            float sigma, int use_fb, float alpha, float beta, int out_dtype, void *out, uint8_t *used,
                            void *stream) {
  TfilterIo io;
  io.sigma = sigma;
  io.radius = radius;
  io.use_fb = use_fb != 0;
  io.alpha = alpha;
  io.beta = beta;
  io.f32 = out_dtype == OFDIS_IMG_F32;
  io.out = out;
  io.used = used;
  if (!c || !flow_fw || !flow_bw || !v || !tfilter_io_ok(io, frames, nframes, width, height, noc, out_dtype) ||
      !tfilter_radius_ok(io))
    return OFDIS_ERR_INVALID_ARGUMENT;
  if ((v->dtype != OFDIS_OUT_F32 && v->dtype != OFDIS_OUT_F16) ||
      (v->layout != OFDIS_OUT_INTERLEAVED && v->layout != OFDIS_OUT_PLANAR) ||
      (v->grid != OFDIS_OUT_FULL && v->grid != OFDIS_OUT_LEVEL))
    return OFDIS_ERR_INVALID_ARGUMENT;
  if (v->grid == OFDIS_OUT_LEVEL && (v->dtype != OFDIS_OUT_F32 || v->layout != OFDIS_OUT_INTERLEAVED))
    return OFDIS_ERR_UNSUPPORTED;  // level grids: float32 interleaved alone (as ofdis_tfilter_u8)
  if (!flow_view_ok(v, width, height)) return OFDIS_ERR_INVALID_ARGUMENT;
  return device_call(c, stream, false, [&](hipStream_t s) {
    return run_tfilter_radius(c, frames, nframes, flow_fw, flow_bw, *v, width, height, noc, io, s);
  });
}

int ofdis_run_sequence_tfilter_radius_u8(ofdis_context *c, const uint8_t *frames, int nframes, int width, int height,
                                         const ofdis_params *p, int radius, float sigma, int use_fb, float alpha,
                                         float beta, int out_dtype, void *out, uint8_t *used, void *stream) {
  TfilterIo io;
  io.sigma = sigma;
  io.radius = radius;
  io.use_fb = use_fb != 0;
  io.alpha = alpha;
  io.beta = beta;
  io.f32 = out_dtype == OFDIS_IMG_F32;
  io.out = out;
  io.used = used;
  if (!c || !p || !tfilter_io_ok(io, frames, nframes, width, height, p->noc, out_dtype) || !tfilter_radius_ok(io))
    return OFDIS_ERR_INVALID_ARGUMENT;
  int rc = validate_call(p, width, height, false);
  if (rc) return rc;
  if (p->mode != OFDIS_MODE_OF) return OFDIS_ERR_UNSUPPORTED;  // a stereo pair is not a sequence
  return device_call(c, stream, true, [&](hipStream_t s) {
    return run_batch_tfilter_radius(c, s, frames, nframes - 1, width, height, p, io);
  });
}

int ofdis_run_sequence_tfilter_radius_u8_host(ofdis_context *c, const uint8_t *frames, int nframes, int width,
                                              int height, const ofdis_params *p, int radius, float sigma, int use_fb,
                                              float alpha, float beta, int out_dtype, void *out, uint8_t *used) {
  return tfilter_host(c, frames, nframes, width, height, p, out_dtype, out, used, [&](const uint8_t *d, void *dout, uint8_t *dused) {
    return ofdis_run_sequence_tfilter_radius_u8(c, d, nframes, width, height, p, radius, sigma, use_fb, alpha, beta,
                                                out_dtype, dout, dused, c->stream);
  });
}

// ------------------------------------------------------------------ global motion and stabilisation (include/ofdis.h)

static_assert(OFDIS_FIT_MAX_SAMPLES == kFitMaxSamples && OFDIS_FIT_MAX_SAMPLES == kMotionMaxSamples &&
                  OFDIS_FIT_LANES == kFitLanes && kFitMaxIters == kMotionMaxIters,
              "the header's limits are the kernel's and the host helpers'");
static_assert(OFDIS_MOTION_TRANSLATION == 0 && OFDIS_MOTION_SIMILARITY == 1, "fit_scalars_ok takes the enum's values");

namespace {
// The scalars and outputs of a fit (ofdis_fit_motion, ofdis_run_sequence_stabilize_u8).
struct FitIo {
  int model = 0, step = 0, iters = 0;
  double tau = 0.0;
  bool use_fb = false;
  float alpha = 0.f, beta = 0.f;
  double *xform = nullptr;
  int32_t *support = nullptr;
  float *weights = nullptr;
};

// What every fitting call checks of its size, scalars and thresholds; L: the lattice.
bool fit_io_ok(const FitIo &io, int width, int height, FitLattice &L) {
  return width > 0 && height > 0 && (long)width * height <= 0x7fffffffL && fit_scalars_ok(io.model, io.tau, io.iters) &&
         fit_lattice(width, height, io.step, L) && (!io.use_fb || fb_thresholds_ok(io.alpha, io.beta));
}

// The m fields of view v fitted (timer "fit_motion_level" for a level-grid view, else "fit_motion").
int run_fit(ofdis_context *c, const void *fw, const void *bw, const ofdis_flow_view &v, int m, int width, int height,
            const FitIo &io, const FitLattice &L, hipStream_t s) {
  FitArgs fa{};
  fa.fw = fw;
  fa.bw = bw;
  fa.xform = io.xform;
  fa.support = io.support;
  fa.weights = io.weights;
  fa.m = m;
  fa.W = width;
  fa.H = height;
  fa.similarity = io.model == OFDIS_MOTION_SIMILARITY;
  fa.step = io.step;
  fa.half = L.half;
  fa.sx = L.sx;
  fa.sy = L.sy;
  fa.ns = L.ns;
  fa.iters = io.iters;
  fit_inv_table(io.tau, io.iters, fa.inv);
  fa.alpha = io.alpha;
  fa.beta = io.beta;
  fa.f16 = v.dtype == OFDIS_OUT_F16;
  fa.planar = v.layout == OFDIS_OUT_PLANAR;
  fa.level = v.grid == OFDIS_OUT_LEVEL;
  if (fa.level) {
    fa.gw = v.gw;
    fa.gh = v.gh;
    fa.offx = v.off_x;
    fa.offy = v.off_y;
    while ((1 << fa.log2c) < v.cell) ++fa.log2c;
  }
  timed(c, fa.level ? 30 : 29, s, [&] { launch_fit_motion(fa, s); });
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// The m pair transforms to m + 1 corrections; chain: (m + 1) * 6 doubles of scratch.
int run_path(ofdis_context *c, const double *xform, int m, int radius, double zoom, int width, int height, double *corr,
             double *chain, hipStream_t s) {
  PathArgs pa{};
  pa.xform = xform;
  pa.corr = corr;
  pa.chain = chain;
  pa.m = m;
  pa.radius = radius;
  pa.W = width;
  pa.H = height;
  pa.z = 1.0 / zoom;
  timed(c, 31, s, [&] { launch_smooth_path(pa, s); });
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// What the affine warp checks of its frames and picture: ofdis_warp_u8's rules, and no overlap (a frame's taps are read
// while other pixels of it are written).
bool warp_affine_ok(const uint8_t *img, int n, int width, int height, int noc, int out_dtype, const void *out) {
  if (!img || !out || n < 1 || width <= 0 || height <= 0 || (noc != 1 && noc != 3) || !img_dtype_ok(out_dtype) ||
      (long)width * height > 0x7fffffffL)
    return false;
  const size_t in = (size_t)n * width * height * noc, outb = in * (out_dtype == OFDIS_IMG_F32 ? 4 : 1);
  const uintptr_t f = (uintptr_t)img, o = (uintptr_t)out;
  return f + in <= o || o + outb <= f;
}

int run_warp_affine(ofdis_context *c, const uint8_t *img, int n, int width, int height, int noc, const double *xf,
                    int f32, void *out, uint8_t *valid, hipStream_t s) {
  WarpAffineArgs wa{};
  wa.img = img;
  wa.xf = xf;
  wa.out = out;
  wa.valid = valid;
  wa.n = n;
  wa.W = width;
  wa.H = height;
  wa.noc = noc;
  wa.out_f32 = f32;
  timed(c, 32, s, [&] { launch_warp_affine(wa, s); });
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// The path's and the picture's side of a stabilising call.
struct StabIo {
  FitIo fit;
  int radius = 0;
  double zoom = 1.0;
  int f32 = 0;
  void *out = nullptr;
  uint8_t *valid = nullptr;
  double *corr = nullptr;
};

// ofdis_run_sequence_stabilize_u8 on stream s (no stage capture is set): run_batch_track's plan; the m forward level
// grids in the context's buffer, with use_fb the m backward ones, and behind them the transforms the caller did not ask
// for (pair transforms, corrections, supports) and the path's chain.  Every chunk writes its share of the grids; after
// the chunks three launches on s: the fit over all pairs, the path, the affine warp over all frames.
int run_batch_stabilize(ofdis_context *c, hipStream_t s, const uint8_t *frames, int m, int width, int height,
                        const ofdis_params *p, const StabIo &io, const FitLattice &L) {
  CallPlan cp;
  int rc = prepare(c, p, m, width, height, false, false, cp, io.fit.use_fb ? 1 : 0, 1);
  if (rc) return rc;
  const ofdis_flow_view v = level_view(first_plan(cp));
  cp.out_pair = level_grid_bytes(first_plan(cp));
  const size_t grid_bytes = align_up((io.fit.use_fb ? 2 : 1) * (size_t)m * cp.out_pair);
  const size_t xf_bytes = align_up((size_t)m * 48), corr_bytes = align_up((size_t)(m + 1) * 48);
  if ((rc = ensure_warp_buf(c, grid_bytes + xf_bytes + 2 * corr_bytes + align_up((size_t)m * 4)))) return rc;  // (drops the graph before it grows)
  char *grids = c->warp_buf, *grids_bw = io.fit.use_fb ? grids + (size_t)m * cp.out_pair : nullptr;
  char *tail = c->warp_buf + grid_bytes;
  StabIo q = io;  // the call's own arrays where the caller gives none
  if (!q.fit.xform) q.fit.xform = (double *)tail;
  if (!q.corr) q.corr = (double *)(tail + xf_bytes);
  double *chain = (double *)(tail + xf_bytes + corr_bytes);
  if (!q.fit.support) q.fit.support = (int32_t *)(tail + xf_bytes + 2 * corr_bytes);
  GraphKey key = graph_key(GraphKey::kStab, c, frames, nullptr, nullptr, grids, grids, m, width, height, 1, p);
  GraphKey::Stab &ks = key.u.stab;
  ks.picture = q.out; ks.valid = q.valid; ks.xform = q.fit.xform; ks.corr = q.corr; ks.support = q.fit.support;
  ks.f32 = q.f32; ks.model = q.fit.model; ks.step = q.fit.step; ks.iters = q.fit.iters; ks.radius = q.radius;
  ks.tau = q.fit.tau; ks.zoom = q.zoom;
  if (q.fit.use_fb) {
    ks.use_fb = 1; ks.alpha = q.fit.alpha; ks.beta = q.fit.beta;
  }
  const size_t in_frame = (size_t)width * height * p->noc;
  return replay_or_record(c, s, cp, key, [&](hipStream_t g) {
    int err = for_each_chunk(c, cp, g, [&](size_t f0, char *ws, const Plan &P, hipStream_t ls) {
      return run_chunk_grids(c, ws, P, p, frames + f0 * in_frame, nullptr, grids + f0 * cp.out_pair,
                             grids_bw ? grids_bw + f0 * cp.out_pair : nullptr, ls);
    });
    if (err) return err;
    if ((err = run_fit(c, grids, grids_bw, v, m, width, height, q.fit, L, g))) return err;
    if ((err = run_path(c, q.fit.xform, m, q.radius, q.zoom, width, height, q.corr, chain, g))) return err;
    return run_warp_affine(c, frames, m + 1, width, height, p->noc, q.corr, q.f32, q.out, q.valid, g);
  });
}
}  // namespace

int ofdis_fit_motion(ofdis_context *c, const void *flow_fw, const void *flow_bw, const ofdis_flow_view *v, int m,
                     int width, int height, int model, int step, double tau, int iters, float alpha, float beta,
                     double *xform, int32_t *support, float *weights, void *stream) {
  FitIo io;
  io.model = model;
  io.step = step;
  io.tau = tau;
  io.iters = iters;
  io.use_fb = flow_bw != nullptr;
  io.alpha = alpha;
  io.beta = beta;
  io.xform = xform;
  io.support = support;
  io.weights = weights;
  FitLattice L;
  if (!c || !flow_fw || !v || !xform || m < 1 || !fit_io_ok(io, width, height, L)) return OFDIS_ERR_INVALID_ARGUMENT;
  if ((v->dtype != OFDIS_OUT_F32 && v->dtype != OFDIS_OUT_F16) ||
      (v->layout != OFDIS_OUT_INTERLEAVED && v->layout != OFDIS_OUT_PLANAR) ||
      (v->grid != OFDIS_OUT_FULL && v->grid != OFDIS_OUT_LEVEL))
    return OFDIS_ERR_INVALID_ARGUMENT;
  if (v->grid == OFDIS_OUT_LEVEL && (v->dtype != OFDIS_OUT_F32 || v->layout != OFDIS_OUT_INTERLEAVED))
    return OFDIS_ERR_UNSUPPORTED;  // level grids: float32 interleaved alone (as ofdis_track_points)
  if (!flow_view_ok(v, width, height)) return OFDIS_ERR_INVALID_ARGUMENT;
  return device_call(c, stream, false,
                     [&](hipStream_t s) { return run_fit(c, flow_fw, flow_bw, *v, m, width, height, io, L, s); });
}

int ofdis_smooth_path(ofdis_context *c, const double *xform, int m, int radius, double zoom, int width, int height,
                      double *corr, void *stream) {
  if (!c || !xform || !corr || !path_scalars_ok(m, radius, zoom, width, height)) return OFDIS_ERR_INVALID_ARGUMENT;
  return device_call(c, stream, false, [&](hipStream_t s) {
    const int rc = ensure_ws(c, (size_t)(m + 1) * 48);  // the chain (the workspace is this call's until call_end)
    return rc ? rc : run_path(c, xform, m, radius, zoom, width, height, corr, (double *)c->ws, s);
  });
}

int ofdis_warp_affine_u8(ofdis_context *c, const uint8_t *img, int n, int width, int height, int noc, const double *xf,
                         int out_dtype, void *out, uint8_t *valid, void *stream) {
  if (!c || !xf || !warp_affine_ok(img, n, width, height, noc, out_dtype, out)) return OFDIS_ERR_INVALID_ARGUMENT;
  return device_call(c, stream, false, [&](hipStream_t s) {
    return run_warp_affine(c, img, n, width, height, noc, xf, out_dtype == OFDIS_IMG_F32, out, valid, s);
  });
}

int ofdis_run_sequence_stabilize_u8(ofdis_context *c, const uint8_t *frames, int nframes, int width, int height,
                                    const ofdis_params *p, int model, int step, double tau, int iters, int use_fb,
                                    float alpha, float beta, int radius, double zoom, int out_dtype, void *out,
                                    uint8_t *valid, double *xform, double *corr, int32_t *support, void *stream) {
  StabIo io;
  io.fit.model = model;
  io.fit.step = step;
  io.fit.tau = tau;
  io.fit.iters = iters;
  io.fit.use_fb = use_fb != 0;
  io.fit.alpha = alpha;
  io.fit.beta = beta;
  io.fit.xform = xform;
  io.fit.support = support;
  io.radius = radius;
  io.zoom = zoom;
  io.f32 = out_dtype == OFDIS_IMG_F32;
  io.out = out;
  io.valid = valid;
  io.corr = corr;
  FitLattice L;
  if (!c || !p || nframes < 2 || !warp_affine_ok(frames, nframes, width, height, p->noc, out_dtype, out) ||
      !fit_io_ok(io.fit, width, height, L) || !path_scalars_ok(nframes - 1, radius, zoom, width, height))
    return OFDIS_ERR_INVALID_ARGUMENT;
  int rc = validate_call(p, width, height, false);
  if (rc) return rc;
  if (p->mode != OFDIS_MODE_OF) return OFDIS_ERR_UNSUPPORTED;  // a stereo pair is not a sequence
  return device_call(c, stream, true, [&](hipStream_t s) {
    return run_batch_stabilize(c, s, frames, nframes - 1, width, height, p, io, L);
  });
}

int ofdis_run_sequence_stabilize_u8_host(ofdis_context *c, const uint8_t *frames, int nframes, int width, int height,
                                         const ofdis_params *p, int model, int step, double tau, int iters, int use_fb,
                                         float alpha, float beta, int radius, double zoom, int out_dtype, void *out,
                                         uint8_t *valid, double *xform, double *corr, int32_t *support) {
  if (!c || !frames || !p || !out || nframes < 2 || width <= 0 || height <= 0 || !img_dtype_ok(out_dtype) ||
      (p->noc != 1 && p->noc != 3))
    return OFDIS_ERR_INVALID_ARGUMENT;
  HIP_OK(hipSetDevice(c->device));
  const size_t px = (size_t)nframes * width * height, in = px * p->noc, outb = in * (out_dtype == OFDIS_IMG_F32 ? 4 : 1);
  const size_t m = (size_t)nframes - 1;
  // one device block: the frames, the picture, the mask, the transforms, the corrections, the supports (each at a
  // multiple of 256 bytes)
  const size_t off_out = align_up(in), off_valid = off_out + align_up(outb), off_xf = off_valid + align_up(px);
  const size_t off_corr = off_xf + align_up(m * 48), off_sup = off_corr + align_up((m + 1) * 48);
  char *d = nullptr;
  HIP_OK(hipMalloc(&d, off_sup + align_up(m * 4)));
  int rc = OFDIS_OK;
  auto step_ok = [&](hipError_t e) {
    if (e != hipSuccess && rc == OFDIS_OK) rc = e == hipErrorOutOfMemory ? OFDIS_ERR_OUT_OF_MEMORY : OFDIS_ERR_DEVICE;
    return rc == OFDIS_OK;
  };
  if (step_ok(hipMemcpyAsync(d, frames, in, hipMemcpyHostToDevice, c->stream))) {
    rc = ofdis_run_sequence_stabilize_u8(c, (const uint8_t *)d, nframes, width, height, p, model, step, tau, iters, use_fb,
                                         alpha, beta, radius, zoom, out_dtype, d + off_out,
                                         valid ? (uint8_t *)(d + off_valid) : nullptr,
                                         xform ? (double *)(d + off_xf) : nullptr, corr ? (double *)(d + off_corr) : nullptr,
                                         support ? (int32_t *)(d + off_sup) : nullptr, c->stream);
    if (rc == OFDIS_OK && step_ok(hipStreamSynchronize(c->stream))) {
      step_ok(hipMemcpy(out, d + off_out, outb, hipMemcpyDeviceToHost));
      if (valid) step_ok(hipMemcpy(valid, d + off_valid, px, hipMemcpyDeviceToHost));
      if (xform) step_ok(hipMemcpy(xform, d + off_xf, m * 48, hipMemcpyDeviceToHost));
      if (corr) step_ok(hipMemcpy(corr, d + off_corr, (m + 1) * 48, hipMemcpyDeviceToHost));
      if (support) step_ok(hipMemcpy(support, d + off_sup, m * 4, hipMemcpyDeviceToHost));
    }
  }
  hipFree(d);
  return rc;
}

// ------------------------------------------------------------------ flow error against ground truth (include/ofdis.h)

static_assert(OFDIS_FE_LANES == kFeLanes && OFDIS_FE_NSTATS == kFeStats && OFDIS_FE_BINS == kFeBins,
              "the header's constants are the kernel's");

namespace {
// The truth, the mask rule and the outputs of an error call (ofdis_flow_error, ofdis_run_error_u8).
struct ErrorIo {
  const float *gt = nullptr;
  const uint8_t *mask = nullptr;
  int mask_eq = -1;
  double *stats = nullptr;
  float *err = nullptr;
  uint32_t *hist = nullptr;
};

// What every error call checks of its size and scalars.
bool error_io_ok(const ErrorIo &io, int n, int width, int height) {
  return io.gt && io.stats && n >= 1 && width > 0 && height > 0 && (long)width * height <= 0x7fffffffL &&
         io.mask_eq >= -1 && io.mask_eq <= 255;
}

// Bytes of the per-row partials of n pairs.
size_t error_rows_bytes(int n, int height) { return (size_t)n * height * sizeof(FeRow); }

// The n fields of view v scored (timer "flow_error_level" for a level-grid view, else "flow_error"), then their rows
// folded ("flow_error_sum"); rows: error_rows_bytes of scratch.
int run_flow_error(ofdis_context *c, const void *flow, const ofdis_flow_view &v, int n, int width, int height,
                   const ErrorIo &io, void *rows, hipStream_t s) {
  FlowErrorArgs fa{};
  fa.flow = flow;
  fa.gt = io.gt;
  fa.mask = io.mask;
  fa.mask_eq = io.mask_eq;
  fa.rows = (FeRow *)rows;
  fa.stats = io.stats;
  fa.err = io.err;
  fa.hist = io.hist;
  fa.n = n;
  fa.W = width;
  fa.H = height;
  fa.f16 = v.dtype == OFDIS_OUT_F16;
  fa.planar = v.layout == OFDIS_OUT_PLANAR;
  fa.level = v.grid == OFDIS_OUT_LEVEL;
  if (fa.level) {
    fa.gw = v.gw;
    fa.gh = v.gh;
    fa.offx = v.off_x;
    fa.offy = v.off_y;
    while ((1 << fa.log2c) < v.cell) ++fa.log2c;
  }
  timed(c, fa.level ? kSlotFlowErrorLevel : kSlotFlowError, s, [&] { launch_flow_error(fa, s); });
  timed(c, kSlotFlowErrorSum, s, [&] { launch_flow_error_sum(fa, s); });
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// ofdis_run_error_u8 on stream s: run_batch's plan with the flow written as n float32 level grids into the context's
// buffer and the per-row partials behind them.  Every chunk writes its share of the grids; after the chunks the two
// error launches on s over all pairs.
int run_batch_error(ofdis_context *c, hipStream_t s, const uint8_t *img_a, const uint8_t *img_b, int n, int width,
                    int height, const ofdis_params *p, const ErrorIo &io) {
  const bool capturing = !c->cap_dis.empty() || !c->cap_tv.empty();
  CallPlan cp;
  int rc = prepare(c, p, n, width, height, false, capturing, cp);
  if (rc) return rc;
  const ofdis_flow_view v = level_view(first_plan(cp));
  cp.out_pair = level_grid_bytes(first_plan(cp));
  const size_t grid_bytes = align_up((size_t)n * cp.out_pair);
  if ((rc = ensure_warp_buf(c, grid_bytes + error_rows_bytes(n, height)))) return rc;  // (drops the graph before it grows)
  char *grids = c->warp_buf, *rows = c->warp_buf + grid_bytes;
  GraphKey key = graph_key(GraphKey::kError, c, img_a, img_b, nullptr, grids, grids, n, width, height, 0, p);
  GraphKey::Error &ke = key.u.error;
  ke.gt = io.gt; ke.mask = io.mask; ke.stats = io.stats; ke.err = io.err; ke.hist = io.hist;
  ke.mask_eq = io.mask ? io.mask_eq : -1;  // (without a mask the rule is not read)
  const size_t in_frame = (size_t)width * height * p->noc;
  return replay_or_record(c, s, cp, key, [&](hipStream_t g) {
    const int err = for_each_chunk(c, cp, g, [&](size_t f0, char *ws, const Plan &P, hipStream_t ls) {
      return run_chunk_grids(c, ws, P, p, img_a + f0 * in_frame, img_b + f0 * in_frame, grids + f0 * cp.out_pair,
                             nullptr, ls);
    });
    return err ? err : run_flow_error(c, grids, v, n, width, height, io, rows, g);
  });
}
}  // namespace

int ofdis_flow_error(ofdis_context *c, const void *flow, const ofdis_flow_view *v, const float *gt, const uint8_t *mask,
                     int mask_eq, int n, int width, int height, double *stats, float *err, uint32_t *hist,
                     void *stream) {
  ErrorIo io;
  io.gt = gt;
  io.mask = mask;
  io.mask_eq = mask_eq;
  io.stats = stats;
  io.err = err;
  io.hist = hist;
  if (!c || !flow || !v || !error_io_ok(io, n, width, height)) return OFDIS_ERR_INVALID_ARGUMENT;
  if ((v->dtype != OFDIS_OUT_F32 && v->dtype != OFDIS_OUT_F16) ||
      (v->layout != OFDIS_OUT_INTERLEAVED && v->layout != OFDIS_OUT_PLANAR) ||
      (v->grid != OFDIS_OUT_FULL && v->grid != OFDIS_OUT_LEVEL))
    return OFDIS_ERR_INVALID_ARGUMENT;
  if (v->grid == OFDIS_OUT_LEVEL && (v->dtype != OFDIS_OUT_F32 || v->layout != OFDIS_OUT_INTERLEAVED))
    return OFDIS_ERR_UNSUPPORTED;  // level grids: float32 interleaved alone (as ofdis_track_points)
  if (!flow_view_ok(v, width, height)) return OFDIS_ERR_INVALID_ARGUMENT;
  return device_call(c, stream, false, [&](hipStream_t s) {
    const int rc = ensure_ws(c, error_rows_bytes(n, height));  // (the workspace is this call's until call_end)
    return rc ? rc : run_flow_error(c, flow, *v, n, width, height, io, c->ws, s);
  });
}

int ofdis_run_error_u8(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, const float *gt,
                       const uint8_t *mask, int mask_eq, int n, int width, int height, const ofdis_params *p,
                       double *stats, float *err, uint32_t *hist, void *stream) {
  ErrorIo io;
  io.gt = gt;
  io.mask = mask;
  io.mask_eq = mask_eq;
  io.stats = stats;
  io.err = err;
  io.hist = hist;
  if (!c || !img_a || !img_b || !p || !error_io_ok(io, n, width, height)) return OFDIS_ERR_INVALID_ARGUMENT;
  const int rc = validate_call(p, width, height, false);
  if (rc) return rc;
  if (p->mode != OFDIS_MODE_OF) return OFDIS_ERR_UNSUPPORTED;  // a disparity is not a flow view
  return device_call(c, stream, false,
                     [&](hipStream_t s) { return run_batch_error(c, s, img_a, img_b, n, width, height, p, io); });
}

int ofdis_run_error_u8_host(ofdis_context *c, const uint8_t *img_a, const uint8_t *img_b, const float *gt,
                            const uint8_t *mask, int mask_eq, int n, int width, int height, const ofdis_params *p,
                            double *stats, float *err, uint32_t *hist) {
  if (!c || !img_a || !img_b || !gt || !stats || !p || n < 1 || width <= 0 || height <= 0 ||
      (long)width * height > 0x7fffffffL || (p->noc != 1 && p->noc != 3))
    return OFDIS_ERR_INVALID_ARGUMENT;
  HIP_OK(hipSetDevice(c->device));
  const size_t px = (size_t)n * width * height, in = px * p->noc;
  // one device block: the two images, the truth, the mask, the numbers, the error map, the histogram (each at a
  // multiple of 256 bytes)
  const size_t off_b = align_up(in), off_gt = 2 * align_up(in), off_mask = off_gt + align_up(px * 8);
  const size_t off_stats = off_mask + align_up(px), off_err = off_stats + align_up((size_t)n * kFeStats * 8);
  const size_t off_hist = off_err + align_up(px * 4), hist_bytes = (size_t)n * kFeBins * 4;
  char *d = nullptr;
  HIP_OK(hipMalloc(&d, off_hist + align_up(hist_bytes)));
  int rc = OFDIS_OK;
  auto step = [&](hipError_t e) {
    if (e != hipSuccess && rc == OFDIS_OK) rc = e == hipErrorOutOfMemory ? OFDIS_ERR_OUT_OF_MEMORY : OFDIS_ERR_DEVICE;
    return rc == OFDIS_OK;
  };
  if (step(hipMemcpyAsync(d, img_a, in, hipMemcpyHostToDevice, c->stream)) &&
      step(hipMemcpyAsync(d + off_b, img_b, in, hipMemcpyHostToDevice, c->stream)) &&
      step(hipMemcpyAsync(d + off_gt, gt, px * 8, hipMemcpyHostToDevice, c->stream)) &&
      (!mask || step(hipMemcpyAsync(d + off_mask, mask, px, hipMemcpyHostToDevice, c->stream)))) {
    rc = ofdis_run_error_u8(c, (const uint8_t *)d, (const uint8_t *)(d + off_b), (const float *)(d + off_gt),
                            mask ? (const uint8_t *)(d + off_mask) : nullptr, mask_eq, n, width, height, p,
                            (double *)(d + off_stats), err ? (float *)(d + off_err) : nullptr,
                            hist ? (uint32_t *)(d + off_hist) : nullptr, c->stream);
    if (rc == OFDIS_OK && step(hipStreamSynchronize(c->stream))) {
      step(hipMemcpy(stats, d + off_stats, (size_t)n * kFeStats * 8, hipMemcpyDeviceToHost));
      if (err) step(hipMemcpy(err, d + off_err, px * 4, hipMemcpyDeviceToHost));
      if (hist) step(hipMemcpy(hist, d + off_hist, hist_bytes, hipMemcpyDeviceToHost));
    }
  }
  hipFree(d);
  return rc;
}

// ------------------------------------------------------------------ moving-object masks (include/ofdis.h)

static_assert(OFDIS_MM_NSTATS == kMmStats && kMmMaxRadius == kMotionMaskMaxRadius,
              "the header's constant and the host helpers' limit are the kernel's");

namespace {
// The transforms, the occlusion plane, the scalars and the outputs of a mask (ofdis_motion_mask,
// ofdis_run_sequence_motion_mask_u8).
struct MaskIo {
  const double *xform = nullptr;
  const uint8_t *occ = nullptr;
  float thr = 0.f, rel = 0.f;
  int radius = 0;
  uint8_t *code = nullptr;
  float *res = nullptr;
  int64_t *stats = nullptr;
};

// The m fields of view v classified (timer "motion_mask_level" for a level-grid view, else "motion_mask").
int run_motion_mask(ofdis_context *c, const void *flow, const ofdis_flow_view &v, int m, int width, int height,
                    const MaskIo &io, hipStream_t s) {
  MotionMaskArgs ma{};
  ma.flow = flow;
  ma.xform = io.xform;
  ma.occ = io.occ;
  ma.code = io.code;
  ma.res = io.res;
  ma.stats = io.stats;
  ma.m = m;
  ma.W = width;
  ma.H = height;
  ma.thr = io.thr;
  ma.rel = io.rel;
  ma.radius = io.radius;
  ma.f16 = v.dtype == OFDIS_OUT_F16;
  ma.planar = v.layout == OFDIS_OUT_PLANAR;
  ma.level = v.grid == OFDIS_OUT_LEVEL;
  if (ma.level) {
    ma.gw = v.gw;
    ma.gh = v.gh;
    ma.offx = v.off_x;
    ma.offy = v.off_y;
    while ((1 << ma.log2c) < v.cell) ++ma.log2c;
  }
  timed(c, ma.level ? kSlotMotionMaskLevel : kSlotMotionMask, s, [&] { launch_motion_mask(ma, s); });
  return hipGetLastError() == hipSuccess ? OFDIS_OK : OFDIS_ERR_DEVICE;
}

// ofdis_run_sequence_motion_mask_u8 on stream s (no stage capture is set): run_batch_stabilize's plan; the m forward
// level grids in the context's buffer, with use_fb the m backward ones, and behind them the outputs the caller did not
// ask for (transforms, supports, with use_fb the forward occlusion planes).  Every chunk writes its share of the grids;
// after the chunks the launches on s over all pairs: the fit, with use_fb the check on the grids, the mask.
int run_batch_motion_mask(ofdis_context *c, hipStream_t s, const uint8_t *frames, int m, int width, int height,
                          const ofdis_params *p, const FitIo &fit, const FitLattice &L, const MaskIo &io,
                          uint8_t *occ_out) {
  CallPlan cp;
  int rc = prepare(c, p, m, width, height, false, false, cp, fit.use_fb ? 1 : 0, 1);
  if (rc) return rc;
  const ofdis_flow_view v = level_view(first_plan(cp));
  cp.out_pair = level_grid_bytes(first_plan(cp));
  const size_t px = (size_t)width * height;
  const size_t grid_bytes = align_up((fit.use_fb ? 2 : 1) * (size_t)m * cp.out_pair);
  const size_t xf_bytes = align_up((size_t)m * 48), sup_bytes = align_up((size_t)m * 4);
  const size_t occ_bytes = fit.use_fb && !occ_out ? (size_t)m * px : 0;
  if ((rc = ensure_warp_buf(c, grid_bytes + xf_bytes + sup_bytes + occ_bytes))) return rc;  // (drops the graph before it grows)
  char *grids = c->warp_buf, *grids_bw = fit.use_fb ? grids + (size_t)m * cp.out_pair : nullptr;
  char *tail = c->warp_buf + grid_bytes;
  FitIo q = fit;  // the call's own arrays where the caller gives none
  if (!q.xform) q.xform = (double *)tail;
  if (!q.support) q.support = (int32_t *)(tail + xf_bytes);
  uint8_t *occ = fit.use_fb ? (occ_out ? occ_out : (uint8_t *)(tail + xf_bytes + sup_bytes)) : nullptr;
  MaskIo mio = io;
  mio.xform = q.xform;
  mio.occ = occ;
  GraphKey key = graph_key(GraphKey::kMotionMask, c, frames, nullptr, nullptr, grids, grids, m, width, height, 1, p);
  GraphKey::MotionMask &km = key.u.motion_mask;
  km.code = io.code; km.res = io.res; km.stats = io.stats; km.xform = q.xform; km.support = q.support; km.occ = occ;
  km.model = q.model; km.step = q.step; km.iters = q.iters; km.tau = q.tau;
  km.radius = io.radius; km.thr = io.thr; km.rel = io.rel;
  if (q.use_fb) {
    km.use_fb = 1; km.alpha = q.alpha; km.beta = q.beta;
  }
  const size_t in_frame = px * p->noc;
  return replay_or_record(c, s, cp, key, [&](hipStream_t g) {
    int err = for_each_chunk(c, cp, g, [&](size_t f0, char *ws, const Plan &P, hipStream_t ls) {
      return run_chunk_grids(c, ws, P, p, frames + f0 * in_frame, nullptr, grids + f0 * cp.out_pair,
                             grids_bw ? grids_bw + f0 * cp.out_pair : nullptr, ls);
    });
    if (err) return err;
    if ((err = run_fit(c, grids, grids_bw, v, m, width, height, q, L, g))) return err;
    if (q.use_fb) {
      BidirOut bo;
      bo.occ_fw = occ;
      bo.alpha = q.alpha;
      bo.beta = q.beta;
      if ((err = run_fb_check_level(c, (const float *)grids, (const float *)grids_bw, v, m, width, height, bo, g)))
        return err;
    }
    return run_motion_mask(c, grids, v, m, width, height, mio, g);
  });
}
}  // namespace

int ofdis_motion_mask(ofdis_context *c, const void *flow, const ofdis_flow_view *v, int m, int width, int height,
                      const double *xform, const uint8_t *occ, float thr, float rel, int radius, uint8_t *code,
                      float *res, int64_t *stats, void *stream) {
  MaskIo io;
  io.xform = xform;
  io.occ = occ;
  io.thr = thr;
  io.rel = rel;
  io.radius = radius;
  io.code = code;
  io.res = res;
  io.stats = stats;
  if (!c || !flow || !v || !xform || (!code && !res && !stats) || !mask_scalars_ok(m, thr, rel, radius, width, height))
    return OFDIS_ERR_INVALID_ARGUMENT;
  if ((v->dtype != OFDIS_OUT_F32 && v->dtype != OFDIS_OUT_F16) ||
      (v->layout != OFDIS_OUT_INTERLEAVED && v->layout != OFDIS_OUT_PLANAR) ||
      (v->grid != OFDIS_OUT_FULL && v->grid != OFDIS_OUT_LEVEL))
    return OFDIS_ERR_INVALID_ARGUMENT;
  if (v->grid == OFDIS_OUT_LEVEL && (v->dtype != OFDIS_OUT_F32 || v->layout != OFDIS_OUT_INTERLEAVED))
    return OFDIS_ERR_UNSUPPORTED;  // level grids: float32 interleaved alone (as ofdis_track_points)
  if (!flow_view_ok(v, width, height)) return OFDIS_ERR_INVALID_ARGUMENT;
  return device_call(c, stream, false,
                     [&](hipStream_t s) { return run_motion_mask(c, flow, *v, m, width, height, io, s); });
}

int ofdis_run_sequence_motion_mask_u8(ofdis_context *c, const uint8_t *frames, int nframes, int width, int height,
                                      const ofdis_params *p, int model, int step, double tau, int iters, int use_fb,
                                      float alpha, float beta, float thr, float rel, int radius, uint8_t *code,
                                      float *res, int64_t *stats, double *xform, int32_t *support, uint8_t *occ,
                                      void *stream) {
  FitIo fit;
  fit.model = model;
  fit.step = step;
  fit.tau = tau;
  fit.iters = iters;
  fit.use_fb = use_fb != 0;
  fit.alpha = alpha;
  fit.beta = beta;
  fit.xform = xform;
  fit.support = support;
  MaskIo io;
  io.thr = thr;
  io.rel = rel;
  io.radius = radius;
  io.code = code;
  io.res = res;
  io.stats = stats;
  FitLattice L;
  if (!c || !frames || !p || nframes < 2 || (p->noc != 1 && p->noc != 3) || (!code && !res && !stats) ||
      !fit_io_ok(fit, width, height, L) || !mask_scalars_ok(nframes - 1, thr, rel, radius, width, height))
    return OFDIS_ERR_INVALID_ARGUMENT;
  const int rc = validate_call(p, width, height, false);
  if (rc) return rc;
  if (p->mode != OFDIS_MODE_OF) return OFDIS_ERR_UNSUPPORTED;  // a stereo pair is not a sequence
  return device_call(c, stream, true, [&](hipStream_t s) {
    return run_batch_motion_mask(c, s, frames, nframes - 1, width, height, p, fit, L, io, fit.use_fb ? occ : nullptr);
  });
}

int ofdis_run_sequence_motion_mask_u8_host(ofdis_context *c, const uint8_t *frames, int nframes, int width, int height,
                                           const ofdis_params *p, int model, int step, double tau, int iters,
                                           int use_fb, float alpha, float beta, float thr, float rel, int radius,
                                           uint8_t *code, float *res, int64_t *stats, double *xform, int32_t *support,
                                           uint8_t *occ) {
  if (!c || !frames || !p || nframes < 2 || width <= 0 || height <= 0 || (long)width * height > 0x7fffffffL ||
      (p->noc != 1 && p->noc != 3) || (!code && !res && !stats))
    return OFDIS_ERR_INVALID_ARGUMENT;
  HIP_OK(hipSetDevice(c->device));
  const size_t m = (size_t)nframes - 1, px = m * width * height, in = (size_t)nframes * width * height * p->noc;
  const bool want_occ = occ && use_fb;
  // one device block: the frames, the codes, the residuals, the statistics, the transforms, the supports, the occlusion
  // planes (each at a multiple of 256 bytes)
  const size_t off_code = align_up(in), off_res = off_code + align_up(px), off_stats = off_res + align_up(px * 4);
  const size_t off_xf = off_stats + align_up(m * kMmStats * 8), off_sup = off_xf + align_up(m * 48);
  const size_t off_occ = off_sup + align_up(m * 4);
  char *d = nullptr;
  HIP_OK(hipMalloc(&d, off_occ + align_up(px)));
  int rc = OFDIS_OK;
  auto step_ok = [&](hipError_t e) {
    if (e != hipSuccess && rc == OFDIS_OK) rc = e == hipErrorOutOfMemory ? OFDIS_ERR_OUT_OF_MEMORY : OFDIS_ERR_DEVICE;
    return rc == OFDIS_OK;
  };
  if (step_ok(hipMemcpyAsync(d, frames, in, hipMemcpyHostToDevice, c->stream))) {
    rc = ofdis_run_sequence_motion_mask_u8(c, (const uint8_t *)d, nframes, width, height, p, model, step, tau, iters,
                                           use_fb, alpha, beta, thr, rel, radius,
                                           code ? (uint8_t *)(d + off_code) : nullptr,
                                           res ? (float *)(d + off_res) : nullptr,
                                           stats ? (int64_t *)(d + off_stats) : nullptr,
                                           xform ? (double *)(d + off_xf) : nullptr,
                                           support ? (int32_t *)(d + off_sup) : nullptr,
                                           want_occ ? (uint8_t *)(d + off_occ) : nullptr, c->stream);
    if (rc == OFDIS_OK && step_ok(hipStreamSynchronize(c->stream))) {
      if (code) step_ok(hipMemcpy(code, d + off_code, px, hipMemcpyDeviceToHost));
      if (res) step_ok(hipMemcpy(res, d + off_res, px * 4, hipMemcpyDeviceToHost));
      if (stats) step_ok(hipMemcpy(stats, d + off_stats, m * kMmStats * 8, hipMemcpyDeviceToHost));
      if (xform) step_ok(hipMemcpy(xform, d + off_xf, m * 48, hipMemcpyDeviceToHost));
      if (support) step_ok(hipMemcpy(support, d + off_sup, m * 4, hipMemcpyDeviceToHost));
      if (want_occ) step_ok(hipMemcpy(occ, d + off_occ, px, hipMemcpyDeviceToHost));
    }
  }
  hipFree(d);
  return rc;
}

int ofdis_pyramid_u8_host(ofdis_context *c, const uint8_t *img, int width, int height, const ofdis_params *p,
                          int imgpadding, float *const *img_pyr, float *const *dx_pyr, float *const *dy_pyr) {
  if (!c || !img || !p || width <= 0 || height <= 0) return OFDIS_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_OK(hipSetDevice(c->device));
  ofdis_params q = *p;
  q.p_samp_s = imgpadding;  // pad by imgpadding
  Plan P = batch_plan(p, 1, width, height);
  P = make_plan(p, 1, P.Wp, P.Hp, imgpadding);
  {
    const int d = 1 << p->sc_f;
    P.W0 = width;
    P.H0 = height;
    P.padw = (width % d) ? d - width % d : 0;
    P.padh = (height % d) ? d - height % d : 0;
    P.padl = P.padw / 2;
    P.padt = P.padh / 2;
  }
  int rc = ensure_ws(c, P.total);
  if (rc) return rc;
  const size_t in = (size_t)width * height * p->noc;
  uint8_t *d = nullptr;
  HIP_OK(hipMalloc(&d, in));
  HIP_OK(hipMemcpy(d, img, in, hipMemcpyHostToDevice));
  hipStream_t st;
  rc = call_begin(c, c->stream, st);
  if (rc == OFDIS_OK) rc = run_pyramid(c, c->ws, P, d, d, st);
  if (rc == OFDIS_OK) rc = call_end(c, c->stream, st);
  if (rc == OFDIS_OK) {
    HIP_OK(hipStreamSynchronize(c->stream));
    for (int s = p->sc_l; s <= p->sc_f; ++s) {
      const LevelGeom &g = P.lv[s - p->sc_l];
      const size_t bytes = sizeof(float) * (size_t)g.W * g.H * p->noc;
      if (img_pyr && img_pyr[s]) HIP_OK(hipMemcpy(img_pyr[s], c->ws + P.off_img[s - p->sc_l], bytes, hipMemcpyDeviceToHost));
      if (dx_pyr && dx_pyr[s]) HIP_OK(hipMemcpy(dx_pyr[s], c->ws + P.off_dx[s - p->sc_l], bytes, hipMemcpyDeviceToHost));
      if (dy_pyr && dy_pyr[s]) HIP_OK(hipMemcpy(dy_pyr[s], c->ws + P.off_dy[s - p->sc_l], bytes, hipMemcpyDeviceToHost));
    }
  }
  hipFree(d);
  (void)q;
  return rc;
}

int ofdis_context_set_stage_capture(ofdis_context *c, float *const *dis_flow, float *const *tv_flow, int nscales) {
  if (!c || nscales < 0) return OFDIS_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(c->mu);
  c->cap_dis.assign(nscales, nullptr);
  c->cap_tv.assign(nscales, nullptr);
  bool any = false;
  for (int i = 0; i < nscales; ++i) {
    if (dis_flow) c->cap_dis[i] = dis_flow[i];
    if (tv_flow) c->cap_tv[i] = tv_flow[i];
    any = any || c->cap_dis[i] || c->cap_tv[i];
  }
  if (!any) {  // no capture: the batch runs as usual (chunked, graph-replayed)
    c->cap_dis.clear();
    c->cap_tv.clear();
  }
  return OFDIS_OK;
}

int ofdis_context_set_option(ofdis_context *c, const char *key, int value) {
  if (!c || !key) return OFDIS_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(c->mu);
  struct Opt {
    const char *name;
    int ofdis_context::*field;
    int lo, hi;
  };
  static const Opt opts[] = {
      {"sor_generic", &ofdis_context::opt_sor_generic, 0, 1},
      {"sor_pipe", &ofdis_context::opt_sor_pipe, 0, 1},     {"smsys", &ofdis_context::opt_smsys, 0, 1},
      {"sor_cring", &ofdis_context::opt_sor_cring, 0, 3},   {"smsys2d", &ofdis_context::opt_smsys2d, 0, 2},
      {"sor_pack", &ofdis_context::opt_sor_pack, 0, 2},      {"smsys_march", &ofdis_context::opt_smsys_march, 0, 1},
      {"smsys_prefetch", &ofdis_context::opt_smsys_prefetch, 0, 1},
      {"smsys_small", &ofdis_context::opt_smsys_small, 0, 1},
      {"smsys_deriv", &ofdis_context::opt_smsys_deriv, 0, 1},
      {"prepd_df", &ofdis_context::opt_prepd_df, 0, 1},
      {"pyr_rgb", &ofdis_context::opt_pyr_rgb, 0, 1},
      {"pad_grad_v", &ofdis_context::opt_pad_grad_v, 0, 1},
      {"agg_stage", &ofdis_context::opt_agg_stage, 0, 1},
      {"sor_rows2", &ofdis_context::opt_sor_rows2, 0, 1},   {"prepd", &ofdis_context::opt_prepd, 0, 2},
      {"wave_per_patch", &ofdis_context::opt_wave_per_patch, 0, 1},
      {"nt_store", &ofdis_context::opt_nt_store, 0, 1},     {"up_form", &ofdis_context::opt_up_form, 0, 3},
      {"graph", &ofdis_context::opt_graph, 0, 2},
      {"patch_window", &ofdis_context::opt_patch_window, 0, 1}, {"patch_quad", &ofdis_context::opt_patch_quad, 0, 1},
      {"patch_generic", &ofdis_context::opt_patch_generic, 0, 1}, {"sor_mode", &ofdis_context::opt_sor_mode, 0, 1},
      {"patch_x16", &ofdis_context::opt_patch_x16, 0, 2},  {"patch_absw", &ofdis_context::opt_patch_absw, 0, 1},
      {"patch_buf", &ofdis_context::opt_patch_buf, 0, 1},  {"patch_fdiv", &ofdis_context::opt_patch_fdiv, 0, 1},
      {"patch_maxres", &ofdis_context::opt_patch_maxres, 0, 1},
      {"streams", &ofdis_context::opt_streams, 0, 16},      {"chunk", &ofdis_context::opt_chunk, 0, 1 << 30},
  };
  for (const Opt &o : opts) {
    if (std::strcmp(key, o.name) != 0) continue;
    if (value < o.lo || value > o.hi) return OFDIS_ERR_INVALID_ARGUMENT;
    HIP_OK(hipSetDevice(c->device));
    const int rc = drop_graph(c);  // a captured graph bakes in the options it was recorded with
    if (rc) return rc;
    c->*o.field = (o.hi == 1) ? (value != 0) : value;
    return OFDIS_OK;
  }
  return OFDIS_ERR_INVALID_ARGUMENT;
}

int ofdis_context_enable_kernel_timing(ofdis_context *c, int enable) {
  if (!c) return OFDIS_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(c->mu);
  drain_timing(c);
  c->acc.clear();
  c->timing = enable != 0;
  return OFDIS_OK;
}

int ofdis_context_kernel_time(ofdis_context *c, const char *name, double *total_ms, long *launches) {
  if (!c || !name) return OFDIS_ERR_INVALID_ARGUMENT;
  const int k = kernel_index(name);
  if (k < 0) return OFDIS_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(c->mu);
  drain_timing(c);
  auto it = c->acc.find(k);
  if (total_ms) *total_ms = it == c->acc.end() ? 0.0 : it->second.first;
  if (launches) *launches = it == c->acc.end() ? 0 : it->second.second;
  return OFDIS_OK;
}

const char *ofdis_kernel_names(void) {
  static const std::string names = [] {
    std::string r;
    for (const char *k : kKernelNames) r += (r.empty() ? "" : ",") + std::string(k);
    return r;
  }();
  return names.c_str();
}

const char *ofdis_kernel_names_ext(void) {
  static const std::string names = [] {
    std::string r;
    for (const char *k : kKernelNamesExt) r += (r.empty() ? "" : ",") + std::string(k);
    return r;
  }();
  return names.c_str();
}

const char *ofdis_kernel_names_all(void) {
  static const std::string names = [] {
    std::string r;
    for (const char *k : kKernelNames) r += (r.empty() ? "" : ",") + std::string(k);
    for (const char *k : kKernelNamesExt) r += "," + std::string(k);
    for (const char *k : kKernelNamesMore) r += "," + std::string(k);
    return r;
  }();
  return names.c_str();
}

// The filter over a radius per interior output frame, in "tfilter"'s convention: per pixel the frame and the taps of
// its 2 R neighbours ((2 R + 1) noc), the picture (noc, or 4 noc as float32) and the `used` byte; each of the 2 R steps
// reads one field once -- 8 bytes per pixel of a full-resolution float32 view (16 R), or a level grid (the opposite
// fields of the check are gathers and are not counted, as in "track").
int ofdis_tfilter_radius_bytes(const ofdis_params *p, int width, int height, int level, int radius, int out_dtype,
                               double *bytes) {
  if (!p || !bytes || radius < 1 || radius > 4 || !img_dtype_ok(out_dtype)) return OFDIS_ERR_INVALID_ARGUMENT;
  const Plan P = batch_plan(p, 1, width, height);
  const double px = (double)width * height, R = radius;
  const double pic = (2.0 * R + 1.0) * P.noc + (out_dtype == OFDIS_IMG_F32 ? 4.0 : 1.0) * P.noc + 1.0;
  *bytes = level ? 2.0 * R * P.lv[0].w * P.lv[0].h * 8.0 + px * pic : px * (16.0 * R + pic);
  return OFDIS_OK;
}

// Byte model of SURVEY §8(d), per frame pair, for the roofline of each kernel family.
int ofdis_algorithmic_bytes(const ofdis_params *p, int width, int height, const char *kernel, double *bytes) {
  if (!p || !kernel || !bytes) return OFDIS_ERR_INVALID_ARGUMENT;
  Plan P = batch_plan(p, 1, width, height);
  const int nop = P.nop, noc = P.noc;
  const int novals = noc * p->p_samp_s * p->p_samp_s;
  double b = 0.0;
  const std::string k(kernel);
  if (kernel_index(kernel) < 0) return OFDIS_ERR_INVALID_ARGUMENT;
  for (const LevelGeom &g : P.lv) {
    const double px = (double)g.w * g.h;
    const int n_inner = p->usetvref ? p->tv_innerit * (g.level + 1) : 0;
    if (k == "tv_sor") b += n_inner * p->tv_solverit * px * (nop == 2 ? 44.0 : 24.0);
    // fused red-black level (latency form): wx, wy and the eight derivative planes in, the flow out -- once per level
    // (the later inner iterations re-read the derivative planes from the frame's L2-resident copy)
    if (k == "tv_level" && n_inner > 0) b += px * 4.0 * (2 * nop + 8 * noc);
    if (k == "tv_system") b += n_inner * px * (4.0 * (8 * noc + 1 + 2 * nop) + 4.0 * (nop == 2 ? 7 : 4));
    // patch: per patch the template + gradients, ONE (p+1)^2 target window, the outputs (the compulsory bytes;
    // re-reads of the window over the iterations are cache-resident, and the kernel is VALU-issue bound)
    if (k == "patch") b += (double)g.npatch * (12.0 * novals + 4.0 * (p->p_samp_s + 1) * (p->p_samp_s + 1) * noc +
                                               4.0 * (nop + novals));
    if (k == "aggregate") b += px * 4.0 * nop + (double)g.npatch * 4.0 * (nop + novals);
    if (k == "pyr_pad_grad") b += 2.0 * (px * 4.0 * noc + 3.0 * g.W * g.H * 4.0 * noc);
    if (k == "pyr_down" && g.level > p->sc_l) b += 2.0 * noc * 4.0 * (4.0 * px + px);
    if (p->usetvref) {
      if (k == "tv_prep") b += px * 4.0 * (4 * noc + 1 + 3 * nop);
      if (k == "tv_deriv") b += px * 4.0 * noc * (2 + 4 + 2 + 3);
      if (k == "tv_final") b += px * 4.0 * 3 * nop;
    }
  }
  if (k == "pyr_base") b = 2.0 * width * height * noc + 2.0 * 4.0 * P.lv[0].w * P.lv[0].h * noc;
  if (k == "upsample" || k == "upsample_planar") b = (double)width * height * nop * 4.0;  // bytes written
  if (k == "upsample_f16" || k == "upsample_planar_f16") b = (double)width * height * nop * 2.0;
  // the level grid: the float32 level plane read, and written (as float32; binary16 writes half of that)
  if (k == "level_out") b = 2.0 * P.lv[0].w * P.lv[0].h * nop * 4.0;
  // both directions: the pixel's own flow and the gathered one (16 B), the mask byte, the error with "fb_check_err"
  if (k == "fb_check") b = 2.0 * width * height * (16.0 + 1.0);
  if (k == "fb_check_err") b = 2.0 * width * height * (16.0 + 1.0 + 4.0);
  // both views: the pixel's own disparity and the gathered one (8 B), the mask byte, the error with "lr_check_err"
  if (k == "lr_check") b = 2.0 * width * height * (8.0 + 1.0);
  if (k == "lr_check_err") b = 2.0 * width * height * (8.0 + 1.0 + 4.0);
  // the warp as ofdis_run_warp_u8 issues it: image taps and u8 picture (noc each) and the mask byte per pixel, and the
  // float32 flow view -- 8 bytes per pixel, or the level grid once per frame
  if (k == "warp") b = (double)width * height * (2.0 * noc + 1.0 + 8.0);
  if (k == "warp_level") b = (double)width * height * (2.0 * noc + 1.0) + (double)P.lv[0].w * P.lv[0].h * 2 * 4.0;
  // the interpolation as ofdis_run_interp_u8 issues it, per intermediate frame (nt = 1): image taps of both frames
  // (2 noc), the u8 picture (noc) and the mask byte per pixel, and the two float32 flow views -- 16 bytes per pixel, or
  // the two level grids once per pair
  if (k == "interp") b = (double)width * height * (16.0 + 3.0 * noc + 1.0);
  if (k == "interp_level") b = 2.0 * P.lv[0].w * P.lv[0].h * 8.0 + (double)width * height * (3.0 * noc + 1.0);
  // the check on level grids: both grids once, the mask byte and the 4-byte error per pixel and direction
  if (k == "fb_check_level") b = 2.0 * P.lv[0].w * P.lv[0].h * 8.0 + 2.0 * width * height * (1.0 + 4.0);
  // the temporal filter per output frame with both neighbours, in the interpolation's convention (masks not counted):
  // the frame and the taps of its two neighbours (3 noc), the u8 picture (noc) and the `used` byte per pixel, and the
  // two float32 flow views -- 16 bytes per pixel, or the two level grids
  if (k == "tfilter") b = (double)width * height * (16.0 + 4.0 * noc + 1.0);
  if (k == "tfilter_level") b = 2.0 * P.lv[0].w * P.lv[0].h * 8.0 + (double)width * height * (4.0 * noc + 1.0);
  // the filter over a radius has the radius and the picture's dtype in its model (ofdis_tfilter_radius_bytes); here at
  // radius 1 with a u8 picture, which is "tfilter"'s count
  if (k == "tfilter_radius") return ofdis_tfilter_radius_bytes(p, width, height, 0, 1, OFDIS_IMG_U8, bytes);
  if (k == "tfilter_radius_level") return ofdis_tfilter_radius_bytes(p, width, height, 1, 1, OFDIS_IMG_U8, bytes);
  // the motion fit per pair at the default lattice (step 16), in "track"'s convention (the check's gather not
  // counted): 8 bytes per sample of a full-resolution float32 view; of a level grid the up to nine 8-byte cells a
  // sample's expansion reads.  The path kernel moves 6 doubles per pair in and per frame out (charged per pair)
  {
    FitLattice L;
    const double ns = fit_lattice(width, height, 16, L) ? (double)L.ns : 0.0;
    if (k == "fit_motion") b = ns * 8.0;
    if (k == "fit_motion_level") b = ns * 9.0 * 8.0;
  }
  if (k == "smooth_path") b = 2.0 * 48.0;
  // the affine warp per frame: image taps and u8 picture (noc each) and the mask byte per pixel, and its six doubles
  if (k == "warp_affine") b = (double)width * height * (2.0 * noc + 1.0) + 48.0;
  // the flow error per pair: the float32 estimate and the truth, 16 bytes per pixel (the function has no mask argument:
  // the mask byte, the error map and the histogram are not counted); of a level grid its cells and the truth.  The
  // reduction reads one FeRow per row and writes the 16 doubles
  if (k == "flow_error") b = (double)width * height * 16.0;
  if (k == "flow_error_level") b = (double)P.lv[0].w * P.lv[0].h * 8.0 + (double)width * height * 8.0;
  if (k == "flow_error_sum") b = (double)height * sizeof(FeRow) + 8.0 * kFeStats;
  // the motion mask per pair: the float32 estimate and the code byte, 9 bytes per pixel (the function has no argument
  // for them: the occlusion byte, the residual map and the statistics are not counted); of a level grid its cells and
  // the code byte
  if (k == "motion_mask") b = (double)width * height * 9.0;
  if (k == "motion_mask_level") b = (double)P.lv[0].w * P.lv[0].h * 8.0 + (double)width * height;
  *bytes = b;
  return OFDIS_OK;
}

// OFC::OFClass (oflow.h:99-126) with host pointers; one frame pair on device 0.
int ofdis_oflow_compute(const float *const *im_ao, const float *const *im_ao_dx, const float *const *im_ao_dy,
                        const float *const *im_bo, const float *const *im_bo_dx, const float *const *im_bo_dy,
                        int imgpadding, float *outflow, const float *initflow, int width, int height,
                        const ofdis_params *p) {
  if (!im_ao || !im_ao_dx || !im_ao_dy || !im_bo || !outflow) return OFDIS_ERR_INVALID_ARGUMENT;
  int rc = ofdis_params_validate(p, width, height, imgpadding);
  if (rc) return rc;
  for (int s = p->sc_l; s <= p->sc_f; ++s) {
    if (!im_ao[s] || !im_ao_dx[s] || !im_ao_dy[s] || !im_bo[s]) return OFDIS_ERR_INVALID_ARGUMENT;
    // image b's gradients are read only by the backward grid of usefbcon (oflow.cpp:193-196)
    if (p->usefbcon && (!im_bo_dx || !im_bo_dy || !im_bo_dx[s] || !im_bo_dy[s])) return OFDIS_ERR_INVALID_ARGUMENT;
  }
  static std::mutex gmu;
  static ofdis_context *gctx = nullptr;
  std::lock_guard<std::mutex> glock(gmu);
  if (!gctx) {
    rc = ofdis_context_create(0, &gctx);
    if (rc) return rc;
  }
  ofdis_context *c = gctx;
  std::lock_guard<std::mutex> lock(c->mu);
  HIP_OK(hipSetDevice(c->device));
  auto t0 = std::chrono::steady_clock::now();
  Plan P = make_plan(p, 1, width, height, imgpadding);
  rc = ensure_ws(c, P.total);
  if (rc) return rc;
  hipStream_t s;
  if ((rc = call_begin(c, c->stream, s))) return rc;
  for (int sl = p->sc_l; sl <= p->sc_f; ++sl) {
    const LevelGeom &g = P.lv[sl - p->sc_l];
    const size_t fb = sizeof(float) * (size_t)g.W * g.H * p->noc;
    char *img = c->ws + P.off_img[sl - p->sc_l];
    HIP_OK(hipMemcpyAsync(img, im_ao[sl], fb, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(img + fb, im_bo[sl], fb, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->ws + P.off_dx[sl - p->sc_l], im_ao_dx[sl], fb, hipMemcpyHostToDevice, s));
    HIP_OK(hipMemcpyAsync(c->ws + P.off_dy[sl - p->sc_l], im_ao_dy[sl], fb, hipMemcpyHostToDevice, s));
    if (p->usefbcon) {
      HIP_OK(hipMemcpyAsync(c->ws + P.off_dx[sl - p->sc_l] + fb, im_bo_dx[sl], fb, hipMemcpyHostToDevice, s));
      HIP_OK(hipMemcpyAsync(c->ws + P.off_dy[sl - p->sc_l] + fb, im_bo_dy[sl], fb, hipMemcpyHostToDevice, s));
    }
  }
  float *dinit = nullptr;
  if (initflow) {
    const size_t nb = sizeof(float) * (size_t)(width >> (p->sc_f + 1)) * (height >> (p->sc_f + 1)) * P.nop;
    HIP_OK(hipMalloc(&dinit, nb > 0 ? nb : 4));
    if (nb) HIP_OK(hipMemcpyAsync(dinit, initflow, nb, hipMemcpyHostToDevice, s));
  }
  std::vector<StageTimes> times;
  c->call_frames = 1;
  rc = run_levels(c, c->ws, P, p, s, dinit, p->verbosity > 1 ? &times : nullptr);
  if (rc == OFDIS_OK) {
    const LevelGeom &g = P.lv[0];
    const size_t plane = (size_t)g.w * g.h;
    std::vector<float> tmp(plane * P.nop);
    HIP_OK(hipMemcpyAsync(tmp.data(), c->ws + P.off_flow[0], tmp.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    for (size_t i = 0; i < plane; ++i)
      for (int k = 0; k < P.nop; ++k) outflow[i * P.nop + k] = tmp[k * plane + i];
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    print_times(P, times, ms, p->verbosity);
  }
  if (rc == OFDIS_OK) rc = call_end(c, c->stream, s);
  if (dinit) hipFree(dinit);
  return rc;
}

int ofdis_max_frames_per_launch(const ofdis_params *p, int width, int height, int *frames) {
  if (!p || !frames || width <= 0 || height <= 0) return OFDIS_ERR_INVALID_ARGUMENT;
  const int rc = ofdis_params_validate(p, -1, -1, -1);
  if (rc) return rc;
  *frames = frame_cap(p, width, height);
  return *frames >= 1 ? OFDIS_OK : OFDIS_ERR_INVALID_ARGUMENT;
}

}  // extern "C"

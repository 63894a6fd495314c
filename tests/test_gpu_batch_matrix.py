"""Batched parity: every kernel family, kernel variant and batch-size launch regime at a frame index > 0.

The single-pair suites (test_gpu_parity.CASES / VARIANTS, test_gpu_patch_shapes) prove each kernel at n = 1, where
the frame index is 0 everywhere: `gp / npatch`, `blockIdx.x` as the frame, the flat `task` index of the register
march and the chunk offsets of the round robin never see another value.  Here the same cases run as batches of
distinct scenes and every checked frame is compared, as uint32 bit patterns, with the CPU oracle's run of that frame
alone (never with another GPU run):

1. `test_batch3_bitexact`: every entry of CASES (plus three patch shapes off the op-points) as one [3, h, w, noc]
   call, with and without the stage capture of frame 0;
2. `test_variants_in_batch`: every non-default kernel option at n = 3 on a case list that reaches every kernel an
   option can touch;
3. `test_chunked_issue_colour_and_depth`: 5 frames in chunks of 2, 2, 1 over 1-3 streams, eager and graph-replayed,
   for noc = 3 and nop = 1 (the chunk offsets `f0 * width * height * noc / nop` of issue_round_robin);
4. `test_more_frames_than_cus*`: n = CUs + 1 frames in one launch, where launch_tv_sor takes the clamped in-frame
   load form (SL) of every k_tv_sor_lanes instance and the fused system kernel its throughput row blocks.

Frames of a batch are synth_pair scenes whose numbers differ mod 8 (the scenes repeat with period 8).  The oracle's
result per (case, frame, SOR order) is computed once and shared (`oracle_frame`).
"""
import math

import numpy as np
import pytest

from test_gpu_parity import CASES, VARIANTS, _params, assert_bitexact
from test_gpu_patch_shapes import shape_params

pytestmark = pytest.mark.gpu

# scene numbers of the frames of a batch, distinct mod 8; test_pipeline_bitexact captures scene 3 at frame 0, the
# single-pair variant test runs scene 4
FRAMES = (5, 2, 7, 0, 6)


@pytest.fixture(scope="module")
def od():
    import of_dis_amd
    return of_dis_amd


@pytest.fixture(scope="module")
def ctx(od):
    c = od.Context(0)
    yield c
    c.close()


def case_id(case):
    w, h, noc, mode, op, over = case
    return f"{w}x{h}-c{noc}-m{mode}-op{op}" + "".join(f"-{k}={v}" for k, v in over.items())


def case_params(od, O, case):
    """(GPU, oracle) parameters of a case; an override of p_samp_s re-derives the scales for that patch size like the
    CLI does (test_gpu_patch_shapes.shape_params)."""
    w, h, noc, mode, op, over = case
    if "p_samp_s" in over:
        return shape_params(od, O, w, noc, mode, op, over["p_samp_s"], {k: v for k, v in over.items() if k != "p_samp_s"})
    return _params(od, O, w, noc, mode, op, over)


_ORACLE = {}


def oracle_frame(O, od, case, frame, order=0, capture=False):
    """oracle.run_u8 of one scene of a case, memoised: (flow, per-scale flow after aggregation, ... after refinement);
    the two dicts are None unless a capture was asked for.  The arrays are shared between tests and read-only."""
    w, h, noc, mode, op, over = case
    key = (w, h, noc, mode, op, tuple(sorted(over.items())), frame, order)
    hit = _ORACLE.get(key)
    if hit is None or (capture and hit[1] is None):
        a, b = od.synth_pair(w, h, noc, frame, mode)
        q = case_params(od, O, case)[1]
        with O.sor_order(order):
            r = O.run_u8(a, b, q, capture=capture)
        hit = r if capture else (r, None, None)
        for x in (hit[0], *(hit[1] or {}).values(), *(hit[2] or {}).values()):
            x.flags.writeable = False
        _ORACLE[key] = hit
    return hit


def stack(od, case, frames):
    w, h, noc, mode = case[:4]
    pairs = [od.synth_pair(w, h, noc, f, mode) for f in frames]
    return np.stack([x[0] for x in pairs]), np.stack([x[1] for x in pairs])


# ---------------------------------------------------------------------------------------------------------------
# 1. every case as a batch of three

def patch_family(p, noc):
    """The patch kernel of a shape at the default options and its patches per workgroup (launch_patch,
    launch_patch_loss, patch_jm: ofdis_kernels.hip)."""
    novals = p * p * noc
    if p == 12 and noc == 3:
        return "k_patchx", 16
    if noc == 1 and p in (8, 12):
        return "k_patchq", 64
    if p in (8, 12):
        return "k_patchw", 32
    if novals in (64, 144, 192, 36, 100, 16, 4):
        return "k_patch8", 32
    if (novals + 63) // 64 > 7:
        return "k_patchg", 32
    return "k_patch", 4  # kPatchWaves


def levels(p, w, h):
    """[(scale, w_s, h_s, npatch)] of a call: the divisibility padding of batch_plan, the patch grid of fill_level."""
    d = 1 << p.sc_f
    wp, hp = w + (-w) % d, h + (-h) % d
    steps = max(1, int(math.floor(np.float32(p.p_samp_s) * (np.float32(1) - np.float32(p.patove)))))
    return [(s, wp >> s, hp >> s, -(-(wp >> s) // steps) * -(-(hp >> s) // steps)) for s in range(p.sc_l, p.sc_f + 1)]


# Frame f's patches start at global patch f * npatch: where npatch is no multiple of the patches per workgroup, a
# workgroup holds the last patches of one frame and the first of the next.  Of CASES (npatch finest level first):
#   k_patchq 64: 160x120 op2 -> 300, 80, 20; 173x97 gradmag -> 286, 77, 24; 192x128 gray op3 -> 2752, 704, 176 (% 64 = 48)
#   k_patchx 16: 192x128 RGB op3 -> 2752, 704, 176 (none straddles); 240x120 RGB depth op4 -> 3200, 800, 200, 50 (8, 2)
#   k_patchw 32 (RGB p = 8): 240x120 RGB depth op2 -> 450, 120, 32; 300x280 RGB -> 5250, 1330; 200x300 -> 3750, 950
#   k_patch8 / k_patch / k_patchg: no entry of CASES (shapes off the op-points)
BATCH_CASES = CASES + [
    (200, 136, 3, 1, 3, {"costfct": 1}),    # k_patchx in flow form: npatch 3082 (200x136), 782, 204: % 16 = 10, 14, 12
    (320, 240, 1, 1, 2, {"p_samp_s": 10}),  # k_patch8 (novals 100): npatch 540 (160x120), 140, 35: % 32 = 28, 12, 3
    (320, 240, 1, 1, 2, {"p_samp_s": 16}),  # k_patch<JM = 7> (novals 256): npatch 252, 63 (80x60), 20: 63 % 4 = 3
    (320, 240, 3, 1, 2, {"p_samp_s": 14, "costfct": 1}),  # k_patchg (novals 588): npatch 300, 80, 20: % 32 = 12, 16, 20
]


def test_case_list_straddles_every_patch_family(oracle, od):
    """Every patch kernel family has a case with a level whose npatch is no multiple of its patches per workgroup."""
    seen = {}
    for case in BATCH_CASES:
        p = case_params(od, oracle, case)[0]
        fam, per = patch_family(p.p_samp_s, p.noc)
        for s, ws, hs, npatch in levels(p, case[0], case[1]):
            if npatch % per:
                seen.setdefault(fam, []).append((case_id(case), s, npatch))
    assert set(seen) == {"k_patchq", "k_patchw", "k_patch8", "k_patchg", "k_patchx", "k_patch"}, seen


@pytest.mark.parametrize("capture", [False, True], ids=["plain", "capture"])
@pytest.mark.parametrize("case", BATCH_CASES, ids=case_id)
def test_batch3_bitexact(oracle, od, ctx, case, capture):
    """Three distinct scenes in one call: each frame is the oracle's flow for that scene; with the stage capture on,
    frame 0's per-scale flows are too."""
    frames = FRAMES[:3]
    a, b = stack(od, case, frames)
    p = case_params(od, oracle, case)[0]
    assert od.validate(p) == 0
    if capture:
        _, cap_d, cap_t = oracle_frame(oracle, od, case, frames[0], capture=True)
        dis = {s: np.zeros_like(v) for s, v in cap_d.items()}
        tv = {s: np.zeros_like(v) for s, v in cap_t.items()}
        ctx.set_capture(dis, tv)
    try:
        got = ctx.run_host(a, b, p)
    finally:
        if capture:
            ctx.set_capture(None, None)
    if capture:
        for s in sorted(cap_d, reverse=True):
            assert_bitexact(dis[s], cap_d[s], f"frame 0, scale {s} after aggregation")
            assert_bitexact(tv[s], cap_t[s], f"frame 0, scale {s} after TV refinement")
    for i, f in enumerate(frames):
        assert_bitexact(got[i], oracle_frame(oracle, od, case, f)[0], f"frame {i} (scene {f})")


# ---------------------------------------------------------------------------------------------------------------
# 2. kernel variants in a batch

BATCH_VARIANTS = VARIANTS + [v for v in (("nt_store", 1, 0), ("patch_window", 0, 1)) if v not in VARIANTS]

VARIANT_CASES = [
    (160, 120, 1, 1, 2, {}),                                  # gray op2: k_patchq p = 8, the row-block system kernel
    (192, 128, 1, 1, 3, {"usefbcon": 1, "costfct": 1}),       # gray op3, forward-backward: second grid, off_*_bw
    (192, 128, 3, 1, 3, {"usefbcon": 1, "costfct": 1}),       # RGB op3, L1, forward-backward: k_patchx
    (240, 120, 1, 2, 4, {"max_iter": 16, "min_iter": 16}),    # gray depth op4 (nop = 1)
    (240, 120, 3, 2, 2, {}),                                  # RGB depth (noc = 3, nop = 1): k_patchw p = 8
    (320, 600, 1, 1, 2, {"sc_l": 0, "sc_f": 1}),              # tall gray: the march, prepd_df<1, 32>, R = 2 / MAXT 1024
    (200, 300, 3, 2, 2, {"sc_l": 0, "sc_f": 1}),              # tall RGB depth: the march and prepd_df<3, 32> on colour
    (160, 120, 1, 1, 2, {"omp_build": 1}),                    # point SOR: the generic k_tv_sor
]


def variant_id(v):
    return f"{v[0]}={v[1]}" if isinstance(v[0], str) else "+".join(f"{k}={x}" for k, x in zip(v[0], v[1]))


@pytest.mark.parametrize("variant", BATCH_VARIANTS, ids=variant_id)
@pytest.mark.parametrize("case", VARIANT_CASES, ids=case_id)
def test_variants_in_batch(oracle, od, ctx, case, variant):
    """Every non-default kernel at frame indices 1 and 2: three distinct scenes in one call, each the oracle's."""
    key, val, default = variant
    keys, vals, defaults = ((key,), (val,), (default,)) if isinstance(key, str) else (key, val, default)
    frames = FRAMES[:3]
    a, b = stack(od, case, frames)
    p = case_params(od, oracle, case)[0]
    for k, v in zip(keys, vals):
        ctx.set_option(k, v)
    try:
        got = ctx.run_host(a, b, p)
    finally:
        for k, d in zip(keys, defaults):
            ctx.set_option(k, d)
    for i, f in enumerate(frames):
        assert_bitexact(got[i], oracle_frame(oracle, od, case, f)[0], f"{keys}={vals}: frame {i} (scene {f})")


# ---------------------------------------------------------------------------------------------------------------
# 3. chunked issue with noc != 1 and nop != 2

CHUNK_CASES = [
    (192, 128, 3, 1, 3, {}),                                  # RGB flow: input offset x 3
    (240, 120, 1, 2, 4, {"max_iter": 16, "min_iter": 16}),    # gray depth: output offset x 1
    (240, 120, 3, 2, 2, {}),                                  # RGB depth: both
    (192, 128, 3, 1, 3, {"usefbcon": 1, "costfct": 1}),       # forward-backward: the lanes' off_*_bw planes
]


@pytest.mark.parametrize("streams", [1, 2, 3])
@pytest.mark.parametrize("case", CHUNK_CASES, ids=case_id)
def test_chunked_issue_colour_and_depth(oracle, od, ctx, case, streams):
    """Five distinct scenes in chunks of 2, 2, 1 (issue_round_robin's `f0 * width * height * noc` input and
    `... * nop` output offsets), eager (graph 0 / 1: multi-lane issues are not captured at 1) and as a captured fork /
    join graph (2).  Each mode runs twice on the same input and output tensors with the options untouched in between,
    so that at graph 2 the second call finds the graph key unchanged (pointers, sizes, parameters) and replays the
    kept executable graph; the output is overwritten with NaN before every run, so a run that writes nothing fails.
    Every frame of every run is the oracle's."""
    import torch
    frames = FRAMES
    n = len(frames)
    an, bn = stack(od, case, frames)
    a, b = torch.from_numpy(an).cuda(), torch.from_numpy(bn).cuda()
    p = case_params(od, oracle, case)[0]
    outs = []
    try:
        for graph in (0, 1, 2):
            ctx.set_option("streams", streams)
            ctx.set_option("chunk", 2)
            ctx.set_option("graph", graph)
            out = torch.empty((n, case[1], case[0], p.nop), dtype=torch.float32, device="cuda")
            for rep in range(2):
                out.fill_(float("nan"))
                assert ctx.run(a, b, p, out=out) is out
                torch.cuda.synchronize()
                outs.append((graph, rep, out.cpu().numpy()))
    finally:
        ctx.set_option("graph", 1)
        ctx.set_option("streams", 0)
        ctx.set_option("chunk", 0)
    for i, f in enumerate(frames):
        ref = oracle_frame(oracle, od, case, f)[0]
        for graph, rep, o in outs:
            assert_bitexact(o[i], ref, f"streams {streams} graph {graph} run {rep}: frame {i} of {n} (scene {f})")


# ---------------------------------------------------------------------------------------------------------------
# 4. more frames than compute units

def sor_form(h, S, nop, cring, n, cus, rows2=1):
    """The exact-order SOR launch of an h-row level (launch_tv_sor, sor_lanes_s, sor_lanes: ofdis_kernels.hip) at the
    default options but sor_cring: ("lanes", S, MAXT, R, G, CR, SL, nop) or ("pipe", S)."""
    g1, g2 = -(-h // 64), -(-h // 128)
    lanes_fit = g1 * S <= 16 or (S <= 3 and g2 * S <= 16 and rows2)
    if not (2 <= S <= 4 and lanes_fit):
        return ("pipe", S)
    t = 64 * S * g1
    maxt, R = (512, 1) if t <= 512 else (1024, 1) if t <= 1024 else (1024, 2)
    G = -(-h // (64 * R))
    crn = 64 * R * (maxt // (64 * S)) + 2 if S <= 3 else 0  # sor_crn

    def lds(crn):  # sor_lanes_lds
        nr = G * 64 * R + 2
        uv = 4 * 2 * 3 * S * nr
        return uv + 4 * 3 * S * nr if crn == 0 else (uv + 15) // 16 * 16 + 6 * crn * (32 if nop == 2 else 16)
    CR = crn > 0 and cring != 0 and lds(crn) <= 160 * 1024
    SL = cring >= 3 or n > cus
    return ("lanes", S, maxt, R, G, CR, SL, nop)


def throughput_row_blocks(w, h, n):
    """Whether the row-block system kernel k_tv_smsys takes smsys_rb's rows per workgroup on a w x h level of an
    n-frame launch (smsys_rb_n: n x row blocks >= 4096); None where the level is not on that kernel (the march)."""
    rb = 1 if h >= 1024 else min(16, 1024 // h)
    if not (rb >= 4 and (rb + 4) * h * 16 + (rb + 2) * h * 4 <= 64 * 1024):
        return None
    rows = w if h <= w else w + h - 1
    return n * -(-rows // rb) >= 4096


def workspace_bound(p, n, w, h):
    """A coarse upper bound of an n-frame launch's workspace in bytes (make_plan: ofdis_runtime.cpp), for the memory
    guard only: the 14 + 9 noc refinement planes of at most (w + h) h slots (skew_plane), and 24 noc padded planes for
    the pyramid (8 per level, levels summing to under 4 / 3 of the finest), the flow and the patch state (under 5 noc)."""
    pad = p.p_samp_s
    return 4 * n * ((14 + 9 * p.noc) * (w + h) * h + 24 * p.noc * (w + 2 * pad) * (h + 2 * pad))


# (MAXT, R, G) of the k_tv_sor_lanes launch per (rows, sweeps), from sor_lanes_s: 64 S ceil(h / 64) <= 512 -> MAXT 512,
# <= 1024 -> MAXT 1024, else two rows per lane; None: S ceil(h / 64) > 16 waves (and no R = 2 at S = 4): the pipeline
LANES = {
    (600, 2): (1024, 2, 5), (300, 2): (1024, 1, 5), (150, 2): (512, 1, 3),
    (600, 3): (1024, 2, 5), (300, 3): (1024, 1, 5), (150, 3): (1024, 1, 3),
    (600, 4): None, (300, 4): None, (150, 4): (1024, 1, 3),
    (256, 2): (512, 1, 4), (128, 2): (512, 1, 2), (64, 2): (512, 1, 1),
    (256, 3): (1024, 1, 4), (128, 3): (512, 1, 2), (64, 3): (512, 1, 1),
    (256, 4): (1024, 1, 4), (128, 4): (512, 1, 2), (64, 4): (512, 1, 1),
}

# Narrow frames (96 columns: the coarsest level keeps a 6-patch-wide grid) whose three levels land on different forms.
# Throughput row blocks at n = 257 (rows = w + h - 1 of the unfolded layout, blocks = ceil(rows / rb)):
#   96x600: 24x150 -> rb 6, 29 blocks, x 257 = 7453 >= 4096 (600 and 300 rows: the march)
#   96x256: 96x256 -> rb 4, 88 blocks; 48x128 -> rb 8, 22 blocks, 5654; 24x64 -> rb 16, 6 blocks, 1542 (latency blocks)
# The regime needs a device of at least 142 CUs (the MI355X has 256): 29 row blocks x (CUs + 1) >= 4096, and the
# default two-stream split (from 256 pairs) of 2 CUs + 2 frames.
OVERSUB_SHAPES = [(96, 600), (96, 256)]
ND = 4  # distinct scenes of an oversubscribed batch


def oversubscribed(oracle, od, ctx, case, n, streams, cring):
    """n frames cycling through ND scenes in one call (streams 1: one launch; 0: the library's default split); every
    launch has more frames than CUs.  Frames 0 .. ND - 1 and n - 1 against the oracle, every other frame f against
    frame f % ND on the device."""
    import torch
    w, h, noc, mode, op, over = case
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p = case_params(od, oracle, case)[0]
    assert od.validate(p) == 0
    chunk = n if streams == 1 else (n + 1) // 2  # stream_count: two lanes from 256 pairs
    assert chunk > cus and (streams == 1 or n >= 256)
    assert od.max_frames_per_launch(p, w, h) >= chunk
    need = workspace_bound(p, chunk, w, h) * (1 if streams == 1 else 2) + n * w * h * (2 * noc + 8 * p.nop)
    free = torch.cuda.mem_get_info()[0]
    assert need <= free // 2, (need, free)
    S = p.tv_solverit
    forms, blocks = [], []
    for s, ws, hs, _ in levels(p, w, h):
        f = sor_form(hs, S, p.nop, cring, chunk, cus)
        want = LANES[(hs, S)]
        assert (f[2:5] if f[0] == "lanes" else None) == want, (hs, S, f, want)
        if f[0] == "lanes":
            assert f[6], f  # SL: the clamped in-frame load form
            # CR: the coefficient ring is off with sor_cring 0, has no S = 4 form (sor_crn), and at two rows per lane
            # its float4 x 2 flow entries pass the 160 KB of LDS (S = 3: 46224 + 123264 bytes, S = 2: 30816 + 196992)
            assert f[5] == (cring != 0 and S <= 3 and not (p.nop == 2 and f[3] == 2)), f
        forms.append(f)
        blocks.append(throughput_row_blocks(ws, hs, chunk))
    assert any(f[0] == "lanes" for f in forms) and any(blocks), (forms, blocks)
    print(f"{case_id(case)} n {n} streams {streams} sor_cring {cring}: (S, MAXT, R, CR, SL, nop) "
          f"{[(f[1], f[2], f[3], f[5], f[6], f[7]) if f[0] == 'lanes' else f for f in forms]}; "
          f"throughput row blocks per level {blocks}")
    an, bn = stack(od, case, FRAMES[:ND])
    idx = torch.arange(n, device="cuda") % ND
    a, b = torch.from_numpy(an).cuda()[idx], torch.from_numpy(bn).cuda()[idx]
    ctx.set_option("streams", streams)
    ctx.set_option("chunk", 0)
    ctx.set_option("sor_cring", cring)
    try:
        out = ctx.run(a, b, p)
        torch.cuda.synchronize()
    finally:
        ctx.set_option("sor_cring", 2)
        ctx.set_option("streams", 0)
    del a, b
    for i in list(range(ND)) + [n - 1]:
        ref = oracle_frame(oracle, od, case, FRAMES[i % ND])[0]
        assert_bitexact(out[i].cpu().numpy(), ref, f"frame {i} of {n}")
    ov = out.view(n, -1).view(torch.int32)
    same = (ov == ov[:ND][idx]).all(dim=1)
    assert bool(same.all()), [int(f) for f in torch.nonzero(~same).flatten()[:10]]
    del out, ov
    torch.cuda.empty_cache()


def _cus_plus(k, mul=1):
    import torch
    return mul * torch.cuda.get_device_properties(0).multi_processor_count + k


@pytest.mark.parametrize("cring", [0, 2])
@pytest.mark.parametrize("mode", [1, 2], ids=["flow", "depth"])
@pytest.mark.parametrize("S", [2, 3, 4])
@pytest.mark.parametrize("w,h", OVERSUB_SHAPES)
def test_more_frames_than_cus(oracle, od, ctx, w, h, S, mode, cring):
    """CUs + 1 frames on one stream: SL = true on every sweep-per-wave SOR form -- 2 to 4 sweeps, 512 / 1024 threads,
    two rows per lane, flow and depth, with the coefficient ring (sor_cring 2) and without (0: the CR = false,
    SL = true instances) -- and the throughput row blocks of k_tv_smsys<1, 1> / <2, 1>."""
    case = (w, h, 1, mode, 2, {"sc_l": 0, "sc_f": 2, "tv_solverit": S})
    oversubscribed(oracle, od, ctx, case, _cus_plus(1), 1, cring)


@pytest.mark.parametrize("w,h", OVERSUB_SHAPES)
def test_more_frames_than_cus_two_streams(oracle, od, ctx, w, h):
    """2 CUs + 2 frames at the default options: the library's two chunks of CUs + 1 frames on two streams."""
    case = (w, h, 1, 1, 2, {"sc_l": 0, "sc_f": 2, "tv_solverit": 3})
    oversubscribed(oracle, od, ctx, case, _cus_plus(2, 2), 0, 2)


@pytest.mark.parametrize("mode", [1, 2], ids=["flow", "depth"])
def test_more_frames_than_cus_rgb(oracle, od, ctx, mode):
    """Colour frames, the default ring: the same SOR forms after k_tv_smsys<2, 3> / <1, 3> on throughput row blocks."""
    case = (96, 256, 3, mode, 2, {"sc_l": 0, "sc_f": 2, "tv_solverit": 3})
    oversubscribed(oracle, od, ctx, case, _cus_plus(1), 1, 2)

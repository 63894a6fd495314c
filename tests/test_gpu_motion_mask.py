"""The moving-object mask on the device: ofdis_motion_mask against test_motion_mask.py's numpy restatement, bit for bit
(code as bytes, res as uint32, stats as int64), in every flow format and on the level-grid view; tile and halo edges on
hand-made fields; the statistics' reset; the fused call ofdis_run_sequence_motion_mask_u8 against its definition -- fit,
check and mask on the fields of run_sequence -- in every issue form; timers, host form, graph re-record, command lines,
refusals.

The scene is test_gpu_track.py's: a textured background that drifts by (1.5, -0.75) per frame and a 41 x 41 patch of
another texture that crosses it by (-6, 4) per frame, 6 frames.  The patch is what moves on its own.
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from test_gpu_sequence import _write_pngs
from test_gpu_track import CASES, T, scene
from test_gpu_warp import ISSUES, _dev, _np
from test_motion_mask import NSTATS, motion_mask_reference
from test_stabilize import bits, field_of, similarity_matrix

pytestmark = pytest.mark.gpu

f32 = np.float32
f64 = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TW, TH = 64, 16  # the kernel's tile (ofdis_internal.h: kMmTileW, kMmTileH)
MASK = dict(thr=1.0, rel=0.05)


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


_fields = {}


def fields(ctx, case):
    """The case's frames, run_sequence(bidir=True)'s two flows and forward occlusion plane and the fit with the check,
    computed once: torch tensors."""
    if case not in _fields:
        w, h, noc, mk = CASES[case]
        fr = _dev(scene(w, h, noc))
        fw, bw, occ = ctx.run_sequence(fr, mk(), bidir=True)[:3]
        _fields[case] = (fr, fw, bw, occ, ctx.fit_motion(fw, bw))
    return _fields[case]


def same_bits(got, want, what):
    """Tuples of numpy arrays or torch tensors, compared as raw bits."""
    assert len(got) == len(want), f"{what}: {len(got)} outputs, expected {len(want)}"
    for k, (g, w_) in enumerate(zip(got, want)):
        g = g if isinstance(g, np.ndarray) else _np(g)
        w_ = w_ if isinstance(w_, np.ndarray) else _np(w_)
        assert g.dtype == w_.dtype and g.shape == w_.shape, f"{what}: output {k} is {g.dtype} {g.shape}, expected {w_.dtype} {w_.shape}"
        a, b = (bits(g), bits(w_)) if g.dtype.itemsize in (4, 8) else (g, w_)
        bad = a != b
        assert not bad.any(), f"{what}: output {k}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}"


def all_outputs(ctx, flow, xform, occ=None, radius=1, **kw):
    return ctx.motion_mask(flow, xform, occ, radius=radius, want_res=True, want_stats=True, **MASK, **kw)


# --------------------------------------------------------------------------------------------- the kernel

@pytest.mark.parametrize("case", list(CASES))
def test_motion_mask_equals_the_restatement(ctx, case):
    import torch
    import of_dis_amd as od
    w, h, noc, mk = CASES[case]
    p = mk()
    fr, fw, bw, occ, xf = fields(ctx, case)
    nfw, nocc, nxf = _np(fw), _np(occ), _np(xf)
    gf = ctx.run_sequence(fr, p, grid="level")
    seen = set()
    for radius in (0, 1, 4):
        for o, no in ((None, None), (occ, nocc)):
            what = f"{case} radius {radius} occ {o is not None}"
            want = motion_mask_reference(nfw, nxf, no, radius=radius, **MASK)
            seen |= set(np.unique(want[0]).tolist())
            same_bits(all_outputs(ctx, fw, xf, o, radius), want, f"{what} float32 nhwc")
            same_bits(all_outputs(ctx, fw.permute(0, 3, 1, 2).contiguous(), xf, o, radius, layout="nchw"), want, f"{what} float32 nchw")
            # the level view gives the bits of the full float32 field
            same_bits(all_outputs(ctx, gf, xf, o, radius, grid="level", p=p, size=(w, h)), want, f"{what} level view")
            want16 = motion_mask_reference(nfw.astype(np.float16), nxf, no, radius=radius, **MASK)
            same_bits(all_outputs(ctx, fw.half(), xf, o, radius), want16, f"{what} float16 nhwc")
            same_bits(all_outputs(ctx, fw.half().permute(0, 3, 1, 2).contiguous(), xf, o, radius, layout="nchw"), want16, f"{what} float16 nchw")
    assert seen == {0, 1, 2}
    # each subset of the three outputs, on the full and on the level view
    want = motion_mask_reference(nfw, nxf, nocc, radius=1, **MASK)
    g = od.out_geometry(p, w, h, grid="level")
    views = ((fw, od.FlowView(0, 0, 0, w, h, 1, 0, 0)),
             (gf, od.FlowView(0, 0, 1, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])))
    for flow, view in views:
        for k in range(1, 8):
            code = torch.full((T - 1, h, w), 9, dtype=torch.uint8, device="cuda")
            res = torch.full((T - 1, h, w), -7.0, dtype=torch.float32, device="cuda")
            stats = torch.full((T - 1, NSTATS), -5, dtype=torch.int64, device="cuda")
            ctx.motion_mask_ptr(flow.data_ptr(), view, T - 1, w, h, xf.data_ptr(), occ.data_ptr(), 1.0, 0.05, 1,
                                code.data_ptr() if k & 1 else 0, res.data_ptr() if k & 2 else 0,
                                stats.data_ptr() if k & 4 else 0, torch.cuda.current_stream().cuda_stream)
            what = f"{case} outputs {k:03b} grid {view.grid}"
            same_bits((code,), (want[0] if k & 1 else np.full_like(want[0], 9),), what + " code")
            same_bits((res,), (want[1] if k & 2 else np.full_like(want[1], -7.0),), what + " res")
            same_bits((stats,), (want[2] if k & 4 else np.full_like(want[2], -5),), what + " stats")


# --------------------------------------------------------------------------------------------- tile and halo edges

EDGE_SIZES = ([(w, h) for w in (TW - 1, TW, TW + 1) for h in (TH - 1, TH, TH + 1)]
              + [(2 * TW + 3, 5),  # three tiles wide, shorter than a tile
                 (1, 1),           # the smallest frame the view rules accept
                 (3, 21)])         # narrower than the radius-4 halo, two tiles high


def edge_field(w, h, seed):
    """Two pairs of a similarity field with displaced boxes that touch every frame border and straddle the tile seams
    at x = TW and y = TH where the frame has them, an isolated moving pixel, a hole, NaN / inf specks, and a random
    occlusion plane."""
    rng = np.random.default_rng(seed)
    M = np.stack([similarity_matrix(1.01, 0.01, 3.0, -2.0, w, h), similarity_matrix(0.99, -0.015, -40.0, 1.0, w, h)])
    F = np.stack([field_of(M[0], w, h), field_of(M[1], w, h)])
    d = f32([10, -6])
    F[0, :max(h // 3, 1), :max(w // 4, 1)] += d            # the top-left corner
    F[0, h - max(h // 4, 1):, w - max(w // 3, 1):] += d    # the bottom-right corner
    F[1, :, :min(3, w)] += d                               # the whole left border
    F[1, h - 1, :] += d                                    # the whole bottom border
    F[1, 0, w // 2:] += d                                  # half the top border
    F[0, h // 2, w - 1] += d                               # one pixel on the right border
    if w > TW:
        F[:, max(h // 2 - 3, 0):h // 2 + 4, TW - 5:min(TW + 6, w)] += d   # across the seam x = TW
    if h > TH:
        F[:, TH - 2:min(TH + 3, h), w // 3:w // 3 + 7] += d   # across the seam y = TH
    if w > 12 and h > 8:
        F[0, 5, 9] += d                                    # a speck
        F[1, h - 1, 5] = field_of(M[1], w, h)[h - 1, 5]    # a hole in the bottom border's line
    k = max(w * h // 40, 1)
    F[rng.integers(0, 2, k), rng.integers(0, h, k), rng.integers(0, w, k), rng.integers(0, 2, k)] = rng.choice([np.nan, np.inf, -np.inf], k)
    occ = ((rng.random((2, h, w)) < 0.1) * rng.integers(1, 3, (2, h, w))).astype(np.uint8)
    return F.astype(f32), M, occ


@pytest.mark.parametrize("size", EDGE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_and_halo_edges(ctx, size):
    import torch
    import of_dis_amd as od
    w, h = size
    F, M, occ = edge_field(w, h, w * 1000 + h)
    dF, dM, docc = _dev(F), _dev(M), _dev(occ)
    for radius in range(5):
        for o, no in ((None, None), (docc, occ)):
            want = motion_mask_reference(F, M, no, radius=radius, **MASK)
            same_bits(all_outputs(ctx, dF, dM, o, radius), want, f"{w}x{h} radius {radius} occ {o is not None}")
        want16 = motion_mask_reference(F.astype(np.float16), M, occ, radius=radius, **MASK)
        same_bits(all_outputs(ctx, dF.half().permute(0, 3, 1, 2).contiguous(), dM, docc, radius, layout="nchw"), want16,
                  f"{w}x{h} radius {radius} float16 nchw")
    if w % 4 == 0:  # pointers off the vector stores' alignment: the pixel-by-pixel stores
        want = motion_mask_reference(F, M, occ, radius=2, **MASK)
        code = torch.zeros(2 * h * w + 1, dtype=torch.uint8, device="cuda")
        res = torch.zeros(2 * h * w + 1, dtype=torch.float32, device="cuda")
        ctx.motion_mask_ptr(dF.data_ptr(), od.FlowView(0, 0, 0, w, h, 1, 0, 0), 2, w, h, dM.data_ptr(), docc.data_ptr(), 1.0,
                            0.05, 2, code.data_ptr() + 1, res.data_ptr() + 4, 0, torch.cuda.current_stream().cuda_stream)
        same_bits((code[1:].view(2, h, w), res[1:].view(2, h, w)), want[:2], f"{w}x{h}: unaligned outputs")
        assert int(code[0]) == 0 and float(res[0]) == 0.0


# --------------------------------------------------------------------------------------------- the statistics

@pytest.mark.parametrize("m", [1, 5])
def test_stats_of_empty_and_full_pairs_and_the_reset(ctx, m):
    import torch
    import of_dis_amd as od
    w, h = 2 * TW + 3, TH + 5
    M = similarity_matrix(1.0, 0.0, 2.0, 1.0, w, h)
    still = np.repeat(field_of(M, w, h)[None], m, 0)
    moving = still + f32([10, -6])
    Ms = _dev(np.repeat(M[None], m, 0))
    none = [w * h, 0, 0, w, h, -1, -1, 0, 0, 0, 0, 0]
    every = [0, w * h, 0, 0, 0, w - 1, h - 1, w * h, h * w * (w - 1) // 2, w * h * (h - 1) // 2, 0, 0]
    for radius in (0, 2):
        _, _, s = all_outputs(ctx, _dev(still), Ms, None, radius)
        assert _np(s).tolist() == [none] * m
        _, _, s = all_outputs(ctx, _dev(moving), Ms, None, radius)
        assert _np(s).tolist() == [every] * m
    mixed = still.copy()
    mixed[m - 1] = moving[m - 1]
    same_bits(all_outputs(ctx, _dev(mixed), Ms, None, 1), motion_mask_reference(mixed, _np(Ms), None, radius=1, **MASK), f"m {m} mixed")
    # two calls in a row into one array: a value the first call left would show if the reset were missing
    stats = torch.full((m, NSTATS), 123456, dtype=torch.int64, device="cuda")
    view = od.FlowView(0, 0, 0, w, h, 1, 0, 0)
    for field, want in ((moving, every), (still, none), (moving, every)):
        ctx.motion_mask_ptr(_dev(field).data_ptr(), view, m, w, h, Ms.data_ptr(), 0, 1.0, 0.05, 1, 0, 0, stats.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
        assert _np(stats).tolist() == [want] * m


# --------------------------------------------------------------------------------------------- the fused call

FIT = dict(model=1, step=16, tau=2.0, iters=4)


def composition(c, fr, p, fb, radius=1, thr=1.0, rel=0.05, alpha=0.01, beta=0.5):
    """(code, res, stats, xform, support[, occ]) of the definition on the fields of run_sequence."""
    if fb:
        fw, bw, occ = c.run_sequence(fr, p, bidir=True, alpha=alpha, beta=beta)[:3]
    else:
        fw, bw, occ = c.run_sequence(fr, p), None, None
    xf, sup = c.fit_motion(fw, bw, alpha=alpha, beta=beta, want_support=True, **FIT)
    out = c.motion_mask(fw, xf, occ, thr, rel, radius, want_res=True, want_stats=True)
    return tuple(out) + (xf, sup) + ((occ,) if fb else ())


@pytest.mark.parametrize("issue", list(ISSUES))
@pytest.mark.parametrize("case", list(CASES))
def test_run_sequence_motion_mask_equals_its_definition(case, issue):
    import torch
    import of_dis_amd as od
    w, h, noc, mk = CASES[case]
    p = mk()
    fr = _dev(scene(w, h, noc))
    c = od.Context(0)
    try:
        for k, v in ISSUES[issue].items():
            c.set_option(k, v)
        for fb in (False, True):
            what = f"{case} {issue} fb {fb}"
            want = composition(c, fr, p, fb)
            got = c.run_sequence_motion_mask(fr, p, fb=fb, want_res=True, want_stats=True, want_xform=True, want_occ=fb, **FIT, **MASK)
            same_bits(got, want, f"{what}: every output")
            assert (_np(got[0]) == 1).any() and (_np(got[0]) == 0).any() and ((_np(got[0]) == 2).any() or not fb)
            # each optional output on its own, and none: the ones not asked for live in the context's buffer
            same_bits((c.run_sequence_motion_mask(fr, p, fb=fb, **FIT, **MASK),), want[:1], f"{what}: code alone")
            same_bits(c.run_sequence_motion_mask(fr, p, fb=fb, want_res=True, **FIT, **MASK), want[:2], f"{what}: + res")
            same_bits(c.run_sequence_motion_mask(fr, p, fb=fb, want_stats=True, **FIT, **MASK), (want[0], want[2]), f"{what}: + stats")
            same_bits(c.run_sequence_motion_mask(fr, p, fb=fb, want_xform=True, **FIT, **MASK), (want[0],) + want[3:5], f"{what}: + xform")
            if fb:
                same_bits(c.run_sequence_motion_mask(fr, p, fb=True, want_occ=True, **FIT, **MASK), (want[0], want[5]), f"{what}: + occ")
            # other scalars
            want2 = composition(c, fr, p, fb, radius=3, thr=2.5, rel=0.0, alpha=0.02, beta=0.25)
            got2 = c.run_sequence_motion_mask(fr, p, fb=fb, alpha=0.02, beta=0.25, thr=2.5, rel=0.0, radius=3, want_res=True,
                                              want_stats=True, want_xform=True, want_occ=fb, **FIT)
            same_bits(got2, want2, f"{what}: radius 3, thr 2.5, rel 0")
        # a graph of this call kind is not replayed by another: the plain sequence still gives its flow
        fw = c.run_sequence(fr, p)
        c.run_sequence_motion_mask(fr, p, **FIT, **MASK)
        assert torch.equal(c.run_sequence(fr, p).view(torch.int32), fw.view(torch.int32)), f"{case} {issue}: run_sequence after the fused call"
    finally:
        c.close()


def test_graph_is_recorded_anew(ctx):
    """The default context replays a recorded graph while nothing changes; thr, radius and an output pointer are part
    of what must not change."""
    import torch
    w, h, noc, mk = CASES["160x120"]
    p = mk()
    fr = _dev(scene(w, h, noc))
    base = composition(ctx, fr, p, True)
    for _ in range(2):  # the second call replays
        same_bits((ctx.run_sequence_motion_mask(fr, p, fb=True, **FIT, **MASK),), base[:1], "thr 1 radius 1")
    for kw in (dict(thr=3.0, radius=1), dict(thr=3.0, radius=0), dict(thr=1.0, radius=0), dict(thr=1.0, radius=1)):
        want = composition(ctx, fr, p, True, radius=kw["radius"], thr=kw["thr"])
        got = ctx.run_sequence_motion_mask(fr, p, fb=True, rel=0.05, **FIT, **kw)
        same_bits((got,), want[:1], f"{kw}")
    assert not np.array_equal(_np(composition(ctx, fr, p, True, thr=3.0)[0]), _np(base[0]))
    assert not np.array_equal(_np(composition(ctx, fr, p, True, radius=0)[0]), _np(base[0]))
    a = torch.full((T - 1, h, w), 7, dtype=torch.uint8, device="cuda")
    b = torch.full((T - 1, h, w), 7, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    args = (fr.data_ptr(), T, w, h, p, 1, 16, 2.0, 4, 1.0, 0.05, 1)
    ctx.run_sequence_motion_mask_ptr(*args, code_ptr=a.data_ptr(), fb=True, stream=s)
    ctx.run_sequence_motion_mask_ptr(*args, code_ptr=a.data_ptr(), fb=True, stream=s)
    same_bits((a,), base[:1], "first pointer")
    a.fill_(7)
    ctx.run_sequence_motion_mask_ptr(*args, code_ptr=b.data_ptr(), fb=True, stream=s)
    same_bits((b,), base[:1], "second pointer")
    assert torch.all(a == 7)  # the recorded graph that wrote to the first pointer was not replayed


def test_timers(ctx):
    import of_dis_amd as od
    w, h, noc, mk = CASES["160x120"]
    p = mk()
    fr, fw, bw, occ, xf = fields(ctx, "160x120")
    gf = ctx.run_sequence(fr, p, grid="level")
    names = od.kernel_names_all()
    assert "motion_mask" in names and "motion_mask_level" in names

    def launches(call):
        before = {k: ctx.kernel_time(k)[1] for k in names}
        call()
        after = {k: ctx.kernel_time(k)[1] for k in names}
        return {k: after[k] - before[k] for k in names if after[k] != before[k]}

    def fused_only(ran, fb):
        other = [k for k in ran if k.startswith("upsample") or k in ("fb_check", "fb_check_err", "fit_motion", "motion_mask")]
        return not other and ran["fit_motion_level"] == 1 and ran["motion_mask_level"] == 1 and ran.get("fb_check_level", 0) == int(fb)

    ctx.enable_kernel_timing(True)
    try:
        ran = launches(lambda: ctx.run_sequence_motion_mask(fr, p, **FIT, **MASK))
        assert ran["level_out"] == 1 and ran["pyr_base"] == 1 and fused_only(ran, False), ran
        ran = launches(lambda: ctx.run_sequence_motion_mask(fr, p, fb=True, want_stats=True, **FIT, **MASK))
        assert ran["level_out"] == 2 and fused_only(ran, True), ran
        ctx.set_option("streams", 2)
        ctx.set_option("chunk", 2)
        ran = launches(lambda: ctx.run_sequence_motion_mask(fr, p, fb=True, **FIT, **MASK))  # chunks of 2, 2 and 1 pairs
        assert ran["level_out"] == 6 and ran["pyr_base"] == 3 and fused_only(ran, True), ran  # one check after the chunks
        ctx.set_option("streams", 0)
        ctx.set_option("chunk", 0)
        assert launches(lambda: ctx.motion_mask(fw, xf, occ, want_stats=True)) == {"motion_mask": 1}
        assert launches(lambda: ctx.motion_mask(gf, xf, grid="level", p=p, size=(w, h))) == {"motion_mask_level": 1}
        for k in ("motion_mask", "motion_mask_level"):
            assert ctx.kernel_time(k)[0] > 0
    finally:
        ctx.set_option("streams", 0)
        ctx.set_option("chunk", 0)
        ctx.enable_kernel_timing(False)


@pytest.mark.parametrize("case", ["160x120", "150x110-rgb"])
def test_host_form(ctx, case):
    w, h, noc, mk = CASES[case]
    p = mk()
    fr = scene(w, h, noc)
    for fb in (False, True):
        kw = dict(fb=fb, want_res=True, want_stats=True, want_xform=True, want_occ=fb, **FIT, **MASK)
        want = ctx.run_sequence_motion_mask(_dev(fr), p, **kw)
        got = ctx.run_sequence_motion_mask_host(fr, p, **kw)
        assert got[0].shape == (T - 1, h, w) and got[2].shape == (T - 1, NSTATS) and got[3].shape == (T - 1, 6)
        same_bits(got, want, f"{case}: host form, fb {fb}")
        same_bits((ctx.run_sequence_motion_mask_host(fr, p, fb=fb, **FIT, **MASK),), want[:1], f"{case}: host form, code alone")
    two = ctx.run_sequence_motion_mask_host(fr[:2], p, want_stats=True)
    same_bits(two, ctx.run_sequence_motion_mask(_dev(fr[:2]), p, want_stats=True), f"{case}: host form, two frames")


# --------------------------------------------------------------------------------------------- command lines

@pytest.mark.parametrize("exe,case,fb", [("run_OF_MOTION_INT", "160x120", 1), ("run_OF_MOTION_INT", "150x110", 0),
                                         ("run_OF_MOTION_RGB", "150x110-rgb", 1)])
def test_cli_motion(ctx, tmp_path, exe, case, fb):
    import of_dis_amd as od
    w, h, noc, _ = CASES[case]
    fr = scene(w, h, noc)
    paths = _write_pngs(tmp_path, fr if noc == 3 else fr[..., None])
    prefix = str(tmp_path / "out_")
    r = subprocess.run([os.path.join(ROOT, "of_dis_amd", "bin", exe), prefix, "1.5", "2", "2", str(fb)] + paths,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    code, stats, xform, _ = ctx.run_sequence_motion_mask_host(fr, od.oppoint(2, w, od.MODE_OF, noc), fb=bool(fb), thr=1.5,
                                                               radius=2, want_stats=True, want_xform=True)
    assert len(list(tmp_path.glob("out_*.pgm"))) == T - 1
    for i in range(T - 1):
        got = od.read_image(f"{prefix}{i:06d}.pgm", 1)
        assert np.array_equal(got[..., 0], code[i]), f"{exe} fb {fb} pair {i}"  # the raw codes 0 / 1 / 2
    lines = [line.split() for line in open(prefix + "stats.txt")]
    assert len(lines) == T - 1 and all(len(t) == NSTATS + 6 for t in lines)
    assert np.array_equal(np.array([[int(v) for v in t[:NSTATS]] for t in lines], np.int64), stats)
    assert np.array_equal(bits(np.array([[float(v) for v in t[NSTATS:]] for t in lines])), bits(xform))  # %.17g round-trips
    assert (code == 1).any()
    for bad in (["-1", "1", "2", "0"], ["nan", "1", "2", "0"], ["65537", "1", "2", "0"], ["1.5", "5", "2", "0"],
                ["1.5", "-1", "2", "0"], ["1.5", "1", "5", "0"], ["1.5", "1", "2", "2"]):
        r = subprocess.run([os.path.join(ROOT, "of_dis_amd", "bin", exe), str(tmp_path / "bad_")] + bad + paths,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "usage" in r.stderr and not list(tmp_path.glob("bad_*")), bad


# --------------------------------------------------------------------------------------------- refusals

def test_refusals_leave_the_context_usable(ctx):
    import torch
    import of_dis_amd as od
    L = od.lib()
    INV, UNS, OK = od._lib.ERR_INVALID_ARGUMENT, od._lib.ERR_UNSUPPORTED, od._lib.OK
    w, h, noc, mk = CASES["160x120"]
    p = mk()
    host = scene(w, h, noc, 4)
    fr = _dev(host)
    fw, bw, occ = ctx.run_sequence(fr, p, bidir=True)[:3]
    xf = ctx.fit_motion(fw, bw)
    gf = ctx.run_sequence(fr, p, grid="level")
    g = od.out_geometry(p, w, h, grid="level")
    code = torch.full((3, h, w), 7, dtype=torch.uint8, device="cuda")
    stats = torch.full((3, NSTATS), 7, dtype=torch.int64, device="cuda")
    plain = ctx.run_sequence_host(host, p)
    full = od.FlowView(0, 0, 0, w, h, 1, 0, 0)
    lvl = od.FlowView(0, 0, 1, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])

    def still_works(what):
        torch.cuda.synchronize()
        assert torch.all(code == 7) and torch.all(stats == 7), what  # nothing was enqueued
        got = ctx.run_sequence_host(host, p)
        assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), f"after the refusal of {what}"

    def mask(a=fw.data_ptr(), view=full, m=3, width=w, height=h, x=xf.data_ptr(), o=occ.data_ptr(), thr=1.0, rel=0.05,
             radius=1, c_=code.data_ptr(), r_=None, s_=stats.data_ptr()):
        return L.ofdis_motion_mask(ctx._h, a, None if view is None else C.byref(view), m, width, height, x, o, thr, rel,
                                   radius, c_, r_, s_, None)

    def fused(frames=fr.data_ptr(), nframes=4, params=p, width=w, height=h, model=1, step=16, tau=2.0, iters=4, use_fb=1,
              alpha=0.01, beta=0.5, thr=1.0, rel=0.05, radius=1, c_=code.data_ptr(), s_=stats.data_ptr()):
        return L.ofdis_run_sequence_motion_mask_u8(ctx._h, frames, nframes, width, height, C.byref(params), model, step, tau,
                                                   iters, use_fb, alpha, beta, thr, rel, radius, c_, None, s_, None, None,
                                                   None, None)

    for call, name in ((mask, "motion_mask"), (fused, "run_sequence_motion_mask")):
        for t in (float("nan"), float("inf"), -0.5, 65537.0):
            assert call(thr=t) == INV, t
        for r in (float("nan"), float("inf"), -0.01, 16.5):
            assert call(rel=r) == INV, r
        assert call(radius=-1) == INV and call(radius=5) == INV
        assert call(width=0) == INV and call(height=-3) == INV
        assert call(c_=None, s_=None) == INV  # all outputs NULL
        still_works(f"{name}: scalars")
    assert mask(a=None) == INV and mask(view=None) == INV and mask(x=None) == INV and mask(m=0) == INV
    assert mask(view=od.FlowView(2, 0, 0, w, h, 1, 0, 0)) == INV and mask(view=od.FlowView(0, 0, 3, w, h, 1, 0, 0)) == INV
    assert mask(a=gf.data_ptr(), view=od.FlowView(0, 0, 1, g["out_w"], g["out_h"], 3, 0, 0)) == INV
    assert mask(a=gf.data_ptr(), view=od.FlowView(0, 0, 1, g["out_w"] - 1, g["out_h"], g["cell"], g["off_x"], g["off_y"])) == INV
    for dt, lay in ((1, 0), (0, 1), (1, 1)):  # level grids: float32 interleaved alone
        assert mask(a=gf.data_ptr(), view=od.FlowView(dt, lay, 1, lvl.gw, lvl.gh, lvl.cell, lvl.off_x, lvl.off_y)) == UNS
    still_works("motion_mask: pointers and views")
    for kw in (dict(model=2), dict(step=0), dict(step=2 * h), dict(tau=float("nan")), dict(iters=17), dict(alpha=-0.01),
               dict(beta=float("nan")), dict(nframes=1), dict(frames=None)):
        assert fused(**kw) == INV, kw
    assert fused(params=od.oppoint(2, w, od.MODE_DE, 1)) == UNS
    still_works("run_sequence_motion_mask: the fit's scalars, frames, depth mode")
    tv = {p.sc_l: np.zeros((h >> p.sc_l, w >> p.sc_l, 2), f32)}
    ctx.set_capture(None, tv)
    try:
        assert fused() == UNS and fused(use_fb=0) == UNS
    finally:
        ctx.set_capture(None, None)
    still_works("run_sequence_motion_mask: a stage capture")
    hp = L.ofdis_run_sequence_motion_mask_u8_host
    code_h = np.zeros((3, h, w), np.uint8)
    tail = (code_h.ctypes.data, None, None, None, None, None)
    assert hp(ctx._h, host.ctypes.data, 1, w, h, C.byref(p), 1, 16, 2.0, 4, 0, 0.01, 0.5, 1.0, 0.05, 1, *tail) == INV
    assert hp(ctx._h, host.ctypes.data, 4, w, h, C.byref(p), 1, 16, 2.0, 4, 0, 0.01, 0.5, float("nan"), 0.05, 1, *tail) == INV
    assert hp(ctx._h, host.ctypes.data, 4, w, h, C.byref(p), 1, 16, 2.0, 4, 0, 0.01, 0.5, 1.0, 0.05, 5, *tail) == INV
    assert hp(ctx._h, host.ctypes.data, 4, w, h, C.byref(p), 1, 16, 2.0, 4, 0, 0.01, 0.5, 1.0, 0.05, 1, None, None, None, None, None, None) == INV
    still_works("the host form")
    want = motion_mask_reference(_np(fw), _np(xf), _np(occ), radius=1, **MASK)
    assert mask() == OK
    same_bits((code, stats), (want[0], want[2]), "after the refusals: the mask")
    assert mask(a=gf.data_ptr(), view=lvl) == OK
    same_bits((code, stats), (want[0], want[2]), "after the refusals: the mask on the level view")
    code.fill_(7)
    assert fused(use_fb=0, alpha=-1.0, beta=float("nan")) == OK  # without the check the thresholds are ignored
    same_bits((code,), (ctx.run_sequence_motion_mask(fr, p, **FIT, **MASK),), "after the refusals: the fused call")
    assert fused() == OK
    same_bits((code, stats), (want[0], want[2]), "after the refusals: the fused call with the check")

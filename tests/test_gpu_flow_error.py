"""The flow-error kernels and the fused evaluation call (ofdis_flow_error, ofdis_run_error_u8, run_OF_EVAL_INT, eval_OF).

Every comparison is on raw bits (float64 as uint64, float32 as uint32).  The kernels must give the numpy restatement of
test_flow_error.py; the level view must give what the full field gives; run_error must give flow_error(run(a, b), gt)
in every issue form; the command lines must print the library's numbers.
"""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from test_flow_error import BINS, NSTATS, flow_error_reference, make_case
from test_gpu_stabilize import same_bits
from test_gpu_track import CASES as LEVEL_CASES
from test_gpu_warp import ISSUES, RUN_CASES, _dev, _np, op2, pairs

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (63, 65), (64, 64), (65, 63), (200, 130)]  # lanes with no term, a partial second term, three row terms
MASKS = [None, -1, 0, 2]                                    # no mask, then mask_eq
_cases, _refs = {}, {}


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


def case(w, h):
    if (w, h) not in _cases:
        _cases[(w, h)] = make_case(w, h)
    return _cases[(w, h)]


def reference(w, h, mask_eq, half=False):
    """The restatement of case (w, h), computed once per (size, mask rule, estimate dtype) and never modified."""
    key = (w, h, mask_eq, half)
    if key not in _refs:
        est, gt, mask = case(w, h)
        _refs[key] = flow_error_reference(est.astype(np.float16) if half else est, gt,
                                          None if mask_eq is None else mask, -1 if mask_eq is None else mask_eq)
    return _refs[key]


def hist_u32(t):
    return _np(t).view(np.uint32)


def truth_for(flow, seed=3):
    """A truth around a computed flow [n, h, w, 2] (numpy): the flow plus noise, with unknown pixels and a mask."""
    rng = np.random.default_rng(seed)
    gt = (flow + (2.0 * rng.standard_normal(flow.shape)).astype(f32)).astype(f32)
    gt[:, ::7, ::5] = 1e10
    mask = rng.integers(0, 3, flow.shape[:3]).astype(np.uint8)
    return gt, mask


# --------------------------------------------------------------------------------------------- kernel == restatement

def test_the_cases_populate_every_slot():
    hit = np.zeros(14, bool)
    for (w, h), m in itertools.product(SIZES, MASKS):
        hit |= (reference(w, h, m)[0][:, :14] != 0).any(axis=0)
    assert hit.all(), hit


@pytest.mark.parametrize("mask_eq", MASKS, ids=lambda m: f"mask_eq{m}")
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_equals_the_restatement(ctx, size, mask_eq):
    import torch
    w, h = size
    est, gt, mask = case(w, h)
    d_gt, d_mask = _dev(gt), (None if mask_eq is None else _dev(mask))
    eq = -1 if mask_eq is None else mask_eq
    for dtype, layout in itertools.product((torch.float32, torch.float16), ("nhwc", "nchw")):
        half = dtype == torch.float16
        want = reference(w, h, mask_eq, half)
        flow = _dev(est).to(dtype)
        if layout == "nchw":
            flow = flow.permute(0, 3, 1, 2).contiguous()
        for want_err, want_hist in itertools.product((False, True), repeat=2):  # every subset of the optional outputs
            got = ctx.flow_error(flow, d_gt, d_mask, eq, want_err=want_err, want_hist=want_hist, layout=layout)
            got = got if isinstance(got, tuple) else (got,)
            what = f"{w}x{h} mask_eq {mask_eq} {dtype} {layout} err {want_err} hist {want_hist}"
            same_bits(got[:1], want[:1], what + ": stats")
            if want_err:
                same_bits(got[1:2], want[1:2], what + ": err")
            if want_hist:
                assert np.array_equal(hist_u32(got[-1]), want[2]), what + ": hist"


# --------------------------------------------------------------------------------------------- level view == full field

@pytest.mark.parametrize("name", list(LEVEL_CASES))
def test_level_view_equals_the_full_field(ctx, name):
    w, h, noc, mk = LEVEL_CASES[name]
    p = mk()
    a, b = (_dev(x) for x in pairs(w, h, noc, 2))
    full = ctx.run(a, b, p)
    level = ctx.run(a, b, p, grid="level")
    gt, mask = truth_for(_np(full))
    d_gt, d_mask = _dev(gt), _dev(mask)
    for m, eq in ((None, -1), (d_mask, -1), (d_mask, 0)):
        want = ctx.flow_error(full, d_gt, m, eq, want_err=True, want_hist=True)
        got = ctx.flow_error(level, d_gt, m, eq, grid="level", p=p, size=(w, h), want_err=True, want_hist=True)
        same_bits(got, want, f"{name} mask_eq {eq} mask {m is not None}")
        same_bits((ctx.flow_error(level, d_gt, m, eq, grid="level", p=p, size=(w, h)),), want[:1], f"{name}: stats alone")
    ref = flow_error_reference(_np(full), gt, mask, 0)   # and the full field's numbers are the restatement's
    same_bits(want[:2], ref[:2], f"{name}: restatement")
    assert np.array_equal(hist_u32(want[2]), ref[2])
    assert _np(want[0])[:, 0].min() > 0


# --------------------------------------------------------------------------------------------- fused == composition

@pytest.mark.parametrize("issue", list(ISSUES))
@pytest.mark.parametrize("name", list(RUN_CASES))
def test_run_error_equals_flow_error_of_run(name, issue):
    import torch
    import of_dis_amd as od
    w, h, noc, op, n = RUN_CASES[name]
    p = od.oppoint(op, w, od.MODE_OF, noc)
    a, b = (_dev(x) for x in pairs(w, h, noc, n))
    c = od.Context(0)
    try:
        for k, v in ISSUES[issue].items():
            c.set_option(k, v)
        flow = c.run(a, b, p)
        gt, mask = truth_for(_np(flow))
        d_gt, d_mask = _dev(gt), _dev(mask)
        want = c.flow_error(flow, d_gt, d_mask, 0, want_err=True, want_hist=True)
        for rep in range(2):
            got = c.run_error(a, b, p, d_gt, d_mask, 0, want_err=True, want_hist=True)
            same_bits(got, want, f"{name} {issue}: call {rep}")
        # the same pointers twice: the second call replays the recorded graph
        stats = torch.empty_like(want[0])
        err = torch.empty_like(want[1])
        hist = torch.empty_like(want[2])
        for rep in range(2):
            stats.fill_(7), err.fill_(7), hist.fill_(7)
            c.run_error_ptr(a.data_ptr(), b.data_ptr(), d_gt.data_ptr(), n, w, h, p, stats.data_ptr(), d_mask.data_ptr(),
                            0, err.data_ptr(), hist.data_ptr(), torch.cuda.current_stream().cuda_stream)
            same_bits((stats, err, hist), want, f"{name} {issue}: call {rep} on fixed pointers")
        # another mask rule on the same pointers records anew; so does dropping the optional outputs
        stats.fill_(7)
        c.run_error_ptr(a.data_ptr(), b.data_ptr(), d_gt.data_ptr(), n, w, h, p, stats.data_ptr(), d_mask.data_ptr(),
                        -1, 0, 0, torch.cuda.current_stream().cuda_stream)
        same_bits((stats,), (c.flow_error(flow, d_gt, d_mask, -1),), f"{name} {issue}: mask_eq -1 on the same pointers")
        same_bits((c.run_error(a, b, p, d_gt),), (c.flow_error(flow, d_gt),), f"{name} {issue}: no mask, stats alone")
        # a different call kind, and this one again (a graph of another kind is never replayed)
        same_bits((c.run(a, b, p),), (flow,), f"{name} {issue}: plain run after run_error")
        pic = c.run_warp(a, b, p)
        same_bits((pic,), (c.warp(b, flow),), f"{name} {issue}: run_warp after run_error")
        for rep in range(2):
            stats.fill_(7), err.fill_(7), hist.fill_(7)
            c.run_error_ptr(a.data_ptr(), b.data_ptr(), d_gt.data_ptr(), n, w, h, p, stats.data_ptr(), d_mask.data_ptr(),
                            0, err.data_ptr(), hist.data_ptr(), torch.cuda.current_stream().cuda_stream)
            same_bits((stats, err, hist), want, f"{name} {issue}: call {rep} after the other kinds")
    finally:
        c.close()


# --------------------------------------------------------------------------------------------- host form, timers, capture

def test_host_form(ctx):
    import of_dis_amd as od
    w, h = 176, 96
    p = op2(w)
    a, b = pairs(w, h, 1, 2)
    flow = ctx.run(_dev(a), _dev(b), p)
    gt, mask = truth_for(_np(flow))
    want = ctx.flow_error(flow, _dev(gt), _dev(mask), 2, want_err=True, want_hist=True)
    stats, err, hist = ctx.run_error_host(a, b, p, gt, mask, 2, want_err=True, want_hist=True)
    same_bits((stats, err), want[:2], "run_error_host")
    assert np.array_equal(hist, hist_u32(want[2]))
    same_bits((ctx.run_error_host(a, b, p, gt),), (ctx.flow_error(flow, _dev(gt)),), "run_error_host, stats alone")
    a1, b1 = od.synth_pair(w, h, 1, 0, od.MODE_OF)  # a single pair [h, w, 1]
    same_bits((ctx.run_error_host(a1, b1, p, gt[0], mask[0], 2),), (_np(want[0])[:1],), "run_error_host, single pair")
    s = od.error_summary(stats)
    assert s["pooled"]["count"] == int(stats[:, 0].sum()) and 0 < s["pooled"]["epe"] < 10
    assert 0 < od.error_percentile(hist, 0.99) <= 64


def test_timers(ctx):
    w, h = 176, 96
    p = op2(w)
    a, b = (_dev(x) for x in pairs(w, h, 1, 2))
    flow = ctx.run(a, b, p)
    level = ctx.run(a, b, p, grid="level")
    gt = _dev(truth_for(_np(flow))[0])
    names = ("flow_error", "flow_error_level", "flow_error_sum", "upsample", "level_out")
    ctx.enable_kernel_timing(True)
    try:
        count = lambda: tuple(ctx.kernel_time(k)[1] for k in names)  # noqa: E731
        assert count() == (0, 0, 0, 0, 0)
        ctx.flow_error(flow, gt)
        assert count() == (1, 0, 1, 0, 0)
        ctx.flow_error(level, gt, grid="level", p=p, size=(w, h), want_hist=True)
        assert count() == (1, 1, 2, 0, 0)
        ctx.run_error(a, b, p, gt)
        assert count() == (1, 2, 3, 0, 1)  # no upsample in run_error
        ctx.run(a, b, p)
        assert count() == (1, 2, 3, 1, 1)
        assert all(ctx.kernel_time(k)[0] > 0 for k in names)
    finally:
        ctx.enable_kernel_timing(False)


def test_run_error_stage_capture(ctx):
    """A stage capture behaves as in run_warp: frame 0's finest level comes back, and the numbers are right."""
    w, h = 176, 96
    p = op2(w)
    a, b = (_dev(x) for x in pairs(w, h, 1, 2))
    flow = ctx.run(a, b, p)
    gt = _dev(truth_for(_np(flow))[0])
    want = ctx.flow_error(flow, gt, want_err=True)
    level = _np(ctx.run(a, b, p, grid="level"))
    tv = {p.sc_l: np.zeros((h >> p.sc_l, w >> p.sc_l, 2), f32)}
    ctx.set_capture(None, tv)
    try:
        same_bits(ctx.run_error(a, b, p, gt, want_err=True), want, "run_error with a stage capture")
    finally:
        ctx.set_capture(None, None)
    same_bits((tv[p.sc_l] * f32(1 << p.sc_l),), (level[0],), "captured finest level")


# --------------------------------------------------------------------------------------------- CLIs

def parse_stats(stdout):
    lines = stdout.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("EPE ") and lines[1].startswith("STATS "), stdout
    vals = np.array([float(x) for x in lines[1].split()[1:]], np.float64)
    assert vals.shape == (NSTATS,)
    return vals, lines[0]


def test_cli_eval(ctx, tmp_path):
    import of_dis_amd as od
    w, h = 176, 96
    p = op2(w)
    a, b = pairs(w, h, 1, 1)
    flow = ctx.run(_dev(a), _dev(b), p)
    gt, mask = truth_for(_np(flow))
    pa, pb, pg, pe, pm = (str(tmp_path / x) for x in ("a.pgm", "b.pgm", "gt.flo", "est.flo", "mask.pgm"))
    od.write_pnm(pa, a[0])
    od.write_pnm(pb, b[0])
    od.write_pnm(pm, mask[0])
    od.write_flo(pg, gt[0])
    od.write_flo(pe, _np(flow)[0])
    fused = os.path.join(ROOT, "of_dis_amd", "bin", "run_OF_EVAL_INT")
    files = os.path.join(ROOT, "of_dis_amd", "bin", "eval_OF")
    for tail, m, eq in (([], None, -1), ([pm], _dev(mask), -1), ([pm, "2"], _dev(mask), 2)):
        want, hist = ctx.flow_error(flow, _dev(gt), m, eq, want_hist=True)
        for cmd in ([fused, pa, pb, pg, "2"] + tail, [files, pe, pg] + tail):
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            vals, line = parse_stats(r.stdout)
            same_bits((vals[None],), (want,), " ".join(cmd[:1] + tail))
            s = od.error_summary(vals)["pooled"]
            assert f"EPE {s['epe']:.4f}" in line and f"p99 {od.error_percentile(hist, 0.99):.4f}" in line
    r = subprocess.run([fused, pa, pb, pg] + [pm], capture_output=True, text=True, timeout=120)  # op-point 2 by default
    assert r.returncode == 0, r.stderr
    same_bits((parse_stats(r.stdout)[0][None],), (ctx.flow_error(flow, _dev(gt), _dev(mask), -1),), "default op-point")
    for cmd in ([fused, pa, pb], [files, pe], [fused, pa, pb, pg, "2", pm, "256"], [files, pe, pg, pm, "-1"]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and r.stderr, cmd


def test_cli_eval_rgb(ctx, tmp_path):
    import of_dis_amd as od
    w, h = 176, 96
    p = op2(w, 3)
    a, b = pairs(w, h, 3, 1)
    flow = ctx.run(_dev(a), _dev(b), p)
    gt, _ = truth_for(_np(flow))
    pa, pb, pg = (str(tmp_path / x) for x in ("a.ppm", "b.ppm", "gt.flo"))
    od.write_pnm(pa, a[0])
    od.write_pnm(pb, b[0])
    od.write_flo(pg, gt[0])
    r = subprocess.run([os.path.join(ROOT, "of_dis_amd", "bin", "run_OF_EVAL_RGB"), pa, pb, pg], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    same_bits((parse_stats(r.stdout)[0][None],), (ctx.flow_error(flow, _dev(gt)),), "run_OF_EVAL_RGB")


# --------------------------------------------------------------------------------------------- refusals

def test_refusals_leave_the_context_usable(ctx):
    import torch
    import of_dis_amd as od
    L = od.lib()
    INV, UNS, OK = od._lib.ERR_INVALID_ARGUMENT, od._lib.ERR_UNSUPPORTED, od._lib.OK
    w, h = 16, 8
    flow = torch.zeros(w * h * 2, dtype=torch.float32, device="cuda")
    gt = torch.ones(64 * 64 * 2, dtype=torch.float32, device="cuda")
    img = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device="cuda")
    stats = torch.full((16,), 7.0, dtype=torch.float64, device="cuda")
    err = torch.full((64 * 64,), 7.0, dtype=torch.float32, device="cuda")
    hist = torch.full((1024,), 7, dtype=torch.int32, device="cuda")
    f, g, i, s, e, hs, hd = (flow.data_ptr(), gt.data_ptr(), img.data_ptr(), stats.data_ptr(), err.data_ptr(),
                             hist.data_ptr(), ctx._h)

    def view(dtype=0, layout=0, grid=0, gw=w, gh=h, cell=1, off_x=0, off_y=0):
        return C.byref(od.FlowView(dtype, layout, grid, gw, gh, cell, off_x, off_y))

    def fe(flow=f, v=None, gt=g, mask=None, mask_eq=-1, n=1, width=w, height=h, stats=s):
        return L.ofdis_flow_error(hd, flow, v if v is not None else view(), gt, mask, mask_eq, n, width, height, stats,
                                  e, hs, None)

    assert fe(flow=None) == INV and fe(gt=None) == INV and fe(stats=None) == INV
    assert L.ofdis_flow_error(hd, f, None, g, None, -1, 1, w, h, s, e, hs, None) == INV
    assert fe(n=0) == INV and fe(n=-1) == INV
    assert fe(width=0) == INV and fe(height=0) == INV and fe(width=-4) == INV
    assert fe(mask_eq=-2) == INV and fe(mask_eq=256) == INV
    assert fe(width=65536, height=32768) == INV                                # 2^31 pixels
    assert fe(v=view(dtype=2)) == INV and fe(v=view(layout=2)) == INV and fe(v=view(grid=2)) == INV
    assert fe(v=view(dtype=-1)) == INV
    for cell in (0, 3, 6, 1024, -2):
        assert fe(v=view(grid=1, cell=cell)) == INV, cell
    assert fe(v=view(grid=1, cell=2, gw=w // 2 - 1, gh=h // 2)) == INV        # the grid does not cover the columns
    assert fe(v=view(grid=1, cell=2, gw=w // 2, gh=h // 2 - 1)) == INV        # ... the rows
    assert fe(v=view(grid=1, cell=2, gw=w // 2, gh=h // 2, off_x=1)) == INV   # ... once the offset is counted
    assert fe(v=view(grid=1, cell=2, gw=w // 2, gh=h // 2, off_x=-1)) == INV
    assert fe(v=view(dtype=1, grid=1, cell=2, gw=w // 2, gh=h // 2)) == UNS   # a level view: float32 interleaved alone
    assert fe(v=view(layout=1, grid=1, cell=2, gw=w // 2, gh=h // 2)) == UNS
    # the fused call
    p = od.oppoint(2, 64, od.MODE_OF, 1)

    def run(a=i, b=i, gt=g, mask_eq=-1, n=1, width=64, height=64, p=p, stats=s):
        return L.ofdis_run_error_u8(hd, a, b, gt, None, mask_eq, n, width, height, C.byref(p) if p is not None else None,
                                    stats, e, hs, None)

    assert run(a=None) == INV and run(b=None) == INV and run(gt=None) == INV and run(stats=None) == INV
    assert run(n=0) == INV and run(width=0) == INV and run(height=-1) == INV and run(p=None) == INV
    assert run(mask_eq=-2) == INV and run(mask_eq=256) == INV
    assert run(p=p.copy(noc=2)) == INV
    assert run(p=od.oppoint(2, 64, od.MODE_DE, 1)) == UNS                      # depth mode
    with pytest.raises(od.OfdisError):
        ctx.flow_error(torch.zeros((1, h, w, 2), device="cuda"), torch.zeros((1, h, w, 2), device="cuda"), mask_eq=300)
    torch.cuda.synchronize()
    assert torch.all(stats == 7) and torch.all(err == 7) and torch.all(hist == 7)  # nothing was enqueued
    # the context still works: a level view that just covers the frame, and the fused call
    assert fe(v=view(grid=1, cell=2, gw=w // 2, gh=h // 2)) == OK
    torch.cuda.synchronize()
    want = np.zeros(16)
    want[[0, 4, 8]] = w * h          # zero flow against a truth of (1, 1): e = sqrt(2) everywhere
    want[[2, 9]] = flow_error_reference(np.zeros((1, h, w, 2), f32), np.ones((1, h, w, 2), f32))[0][0, 2]
    want[3] = float(np.sqrt(f32(2)))
    assert np.array_equal(_np(stats), want)
    assert torch.all(err[:w * h] == float(np.sqrt(f32(2)))) and torch.all(err[w * h:] == 7)
    assert int(hist[22]) == w * h and int(hist.sum()) == w * h
    assert run() == OK
    torch.cuda.synchronize()
    assert float(stats[0]) == 64 * 64
    a, b = (_dev(x) for x in pairs(176, 96, 1, 1))
    q = op2(176)
    flow = ctx.run(a, b, q)
    gt2 = _dev(truth_for(_np(flow))[0])
    same_bits((ctx.run_error(a, b, q, gt2),), (ctx.flow_error(flow, gt2),), "after the refusals")

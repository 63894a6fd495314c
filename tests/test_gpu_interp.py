"""The level-grid interpolation and the fused call (ofdis_interp_u8 with level views, ofdis_run_interp_u8,
run_OF_INTERP_INT / _RGB).

Every comparison is on raw bits.  The level form must give the pictures of the full-resolution form; run_interp must
give interp(a, b, the two flows of run_bidir); the full-resolution form itself is pinned to the numpy reference by
test_interp.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_warp import ISSUES, LEVEL_CASES, RUN_CASES, _dev, _np, assert_same_pictures, expand_level, op2, pairs
from test_interp import interp_reference
from test_warp import assert_picture

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


# --------------------------------------------------------------------------------------------- level form == full form

def _level_against_full(ctx, w, h, noc, p, what, n=2, half=True):
    import torch
    import of_dis_amd as od
    a, b = (_dev(x) for x in pairs(w, h, noc, n))
    g = od.out_geometry(p, w, h, grid="level")
    full = ctx.run(a, b, p), ctx.run(b, a, p)
    level = ctx.run(a, b, p, grid="level"), ctx.run(b, a, p, grid="level")
    t = (0.25, 0.5)
    for out_dtype in (torch.uint8, torch.float32):
        want = ctx.interp(a, b, *full, t, out_dtype=out_dtype, want_valid=True)
        got = ctx.interp(a, b, *level, t, out_dtype=out_dtype, grid="level", p=p, want_valid=True)
        assert_same_pictures(got, want, f"{what} {out_dtype}")
    assert len(np.unique(_np(want[0]))) > 2  # (a picture, not a constant)
    planar = ctx.run(a, b, p, layout="nchw", grid="level"), ctx.run(b, a, p, layout="nchw", grid="level")
    got = ctx.interp(a, b, *planar, t, layout="nchw", grid="level", p=p, want_valid=True)
    assert_same_pictures(got, ctx.interp(a, b, *full, t, want_valid=True), f"{what} planar level grids")
    if not half:
        return
    # float16 cells: the upsample's taps restated in numpy (expand_level, checked against the plain call by
    # test_gpu_warp.py) feed interp_reference
    for layout in ("nhwc", "nchw"):
        halves = [ctx.run(x, y, p, dtype=torch.float16, layout=layout, grid="level") for x, y in ((a, b), (b, a))]
        cells = [_np(x).astype(f32) for x in halves]
        if layout == "nchw":
            cells = [c.transpose(0, 2, 3, 1) for c in cells]
        want, want_valid = interp_reference(_np(a), _np(b), *(expand_level(c, g, w, h) for c in cells), t)
        got = ctx.interp(a, b, *halves, t, layout=layout, grid="level", p=p, want_valid=True)
        assert_picture(_np(got[0]), want, f"{what} float16 {layout} level grids")
        assert_picture(_np(got[1]), want_valid, f"{what} float16 {layout} level grids (valid)")


@pytest.mark.parametrize("case", list(LEVEL_CASES))
def test_level_form_equals_full_form(ctx, case):
    w, h, noc, mk = LEVEL_CASES[case]
    _level_against_full(ctx, w, h, noc, mk(), case)


def test_level_form_equals_full_form_1080p(ctx):
    """One 1920 x 1080 op-point-2 pair: 16-pixel cells, 8 padded rows (off_y 4), two 1024-column blocks."""
    import of_dis_amd as od
    w, h = 1920, 1080
    p = op2(w)
    assert od.out_geometry(p, w, h, grid="level")["cell"] == 16
    _level_against_full(ctx, w, h, 1, p, "1080p", n=1, half=False)
    a, b = (_dev(x) for x in pairs(w, h, 1, 1))
    fw, bw = ctx.run_bidir(a, b, p)[:2]
    assert_same_pictures(ctx.run_interp(a, b, p, (0.5,), want_valid=True), ctx.interp(a, b, fw, bw, (0.5,), want_valid=True),
                         "1080p run_interp")


# --------------------------------------------------------------------------------------------- run_interp

FB_CASE = "gray-fbcon-5"
CASES = dict(RUN_CASES)
CASES[FB_CASE] = (176, 96, 1, 2, 5)   # usefbcon = 1: the backward work is shared


MATRIX = [(case, issue) for case in RUN_CASES for issue in ISSUES] + [(FB_CASE, "default")]


@pytest.mark.parametrize("case,issue", MATRIX, ids=[f"{c}-{i}" for c, i in MATRIX])
def test_run_interp_equals_interp_of_run_bidir(case, issue):
    import torch
    import of_dis_amd as od
    w, h, noc, op, n = CASES[case]
    p = od.oppoint(op, w, od.MODE_OF, noc)
    if case == FB_CASE:
        p = p.copy(usefbcon=1)
    a, b = (_dev(x) for x in pairs(w, h, noc, n))
    c = od.Context(0)
    try:
        for k, v in ISSUES[issue].items():
            c.set_option(k, v)
        fw, bw = c.run_bidir(a, b, p)[:2]
        flow = c.run(a, b, p)
        level = c.run(a, b, p, grid="level")
        bidir = c.run_bidir(a, b, p)
        warped = c.run_warp(a, b, p, want_valid=True)
        for t, out_dtype in (((0.5,), torch.uint8), ((0.25, 0.5, 0.75), torch.float32)):
            want = c.interp(a, b, fw, bw, t, out_dtype=out_dtype, want_valid=True)
            first = c.run_interp(a, b, p, t, out_dtype, want_valid=True)
            second = c.run_interp(a, b, p, t, out_dtype, want_valid=True)
            assert_same_pictures(first, want, f"{case} {issue} t {t}: first call")
            assert_same_pictures(second, want, f"{case} {issue} t {t}: second call")
        # the same output pointers twice: the second call replays the captured graph
        out = torch.empty_like(want[0])
        valid = torch.empty_like(want[1])
        s = torch.cuda.current_stream().cuda_stream
        for rep in range(2):
            out.fill_(77)
            valid.fill_(77)
            c.run_interp_ptr(a.data_ptr(), b.data_ptr(), n, w, h, p, t, od.IMG_F32, out.data_ptr(), valid.data_ptr(), s)
            assert_same_pictures((out, valid), want, f"{case} {issue}: call {rep} on fixed pointers")
        # other times on the same pointers: another picture (the graph key carries the times)
        t2 = (0.25, 0.5, 0.625)
        c.run_interp_ptr(a.data_ptr(), b.data_ptr(), n, w, h, p, t2, od.IMG_F32, out.data_ptr(), valid.data_ptr(), s)
        assert_same_pictures((out, valid), c.interp(a, b, fw, bw, t2, out_dtype=torch.float32, want_valid=True),
                             f"{case} {issue}: other times on fixed pointers")
        assert not np.array_equal(_np(out), _np(want[0]))
        # without the mask
        assert_picture(_np(c.run_interp(a, b, p, (0.5,))), _np(c.interp(a, b, fw, bw, (0.5,))), f"{case} {issue}: no mask")
        # the other calls on the same images still return their own results (the graph key)
        assert_picture(_np(c.run(a, b, p)), _np(flow), f"{case} {issue}: plain run after run_interp")
        assert_picture(_np(c.run(a, b, p, grid="level")), _np(level), f"{case} {issue}: level run after run_interp")
        for got, ref in zip(c.run_bidir(a, b, p), bidir):
            assert_picture(_np(got), _np(ref), f"{case} {issue}: run_bidir after run_interp")
        assert_same_pictures(c.run_warp(a, b, p, want_valid=True), warped, f"{case} {issue}: run_warp after run_interp")
        assert_same_pictures(c.run_interp(a, b, p, (0.5,), want_valid=True), c.interp(a, b, fw, bw, (0.5,), want_valid=True),
                             f"{case} {issue}: run_interp after the other runs")
    finally:
        c.close()


def test_run_interp_host_and_timers(ctx):
    import of_dis_amd as od
    w, h = 176, 96
    p = op2(w)
    a, b = pairs(w, h, 1, 2)
    t = (0.25, 0.75)
    want = ctx.run_interp(_dev(a), _dev(b), p, t, want_valid=True)
    out, valid = ctx.run_interp_host(a, b, p, t, want_valid=True)
    assert out.shape == (2, 2, h, w)
    assert_picture(out, _np(want[0]), "run_interp_host")
    assert_picture(valid, _np(want[1]), "run_interp_host (valid)")
    a1, b1 = od.synth_pair(w, h, 1, 0, od.MODE_OF)  # a single pair [h, w, 1]
    one = ctx.run_interp_host(a1, b1, p, t)
    assert one.shape == (2, h, w, 1)
    assert_picture(one[..., 0], out[0], "run_interp_host, single pair")
    names = od.kernel_names()
    ctx.enable_kernel_timing(True)
    try:
        before = {k: ctx.kernel_time(k)[1] for k in names}
        ctx.run_interp(_dev(a), _dev(b), p, t)
        after = {k: ctx.kernel_time(k)[1] for k in names}
        ran = {k: after[k] - before[k] for k in names if after[k] != before[k]}
        assert ran["level_out"] == 2 and ran["interp_level"] == 1 and "interp" not in ran
        assert not [k for k in ran if k.startswith("upsample")]  # no upsample in run_interp
    finally:
        ctx.enable_kernel_timing(False)


# --------------------------------------------------------------------------------------------- refusals

def test_refusals_leave_the_context_usable(ctx):
    import torch
    import of_dis_amd as od
    L = od.lib()
    INV, UNS, OK = od._lib.ERR_INVALID_ARGUMENT, od._lib.ERR_UNSUPPORTED, od._lib.OK
    w, h = 16, 8
    img = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
    flow = torch.zeros(w * h * 2, dtype=torch.float32, device="cuda")
    out = torch.full((w * h * 3 * 4 * 17,), 7, dtype=torch.uint8, device="cuda")
    val = torch.full((w * h * 17,), 7, dtype=torch.uint8, device="cuda")
    i, f, o, m, hd = img.data_ptr(), flow.data_ptr(), out.data_ptr(), val.data_ptr(), ctx._h
    qa, qb = (_dev(x) for x in pairs(176, 96, 1, 1))
    q = op2(176)
    plain = _np(ctx.run(qa, qb, q))

    def still_works(what):
        torch.cuda.synchronize()
        assert torch.all(out == 7) and torch.all(val == 7), what  # nothing was enqueued by the refused call
        assert_picture(_np(ctx.run(qa, qb, q)), plain, f"plain run after the refusal of {what}")

    def times(*t):
        arr = np.array(t, f32)
        return arr, arr.ctypes.data

    def view(dtype=0, layout=0, grid=0, gw=w, gh=h, cell=1, off_x=0, off_y=0):
        return C.byref(od.FlowView(dtype, layout, grid, gw, gh, cell, off_x, off_y))

    half = times(0.5)

    def interp(a=i, b=i, fw=f, bw=f, v=None, n=1, width=w, height=h, noc=1, t=half, nt=None, out_dtype=0, out=o):
        return L.ofdis_interp_u8(hd, a, b, fw, bw, v if v is not None else view(), n, width, height, noc, t[1],
                                 len(t[0]) if nt is None else nt, None, None, out_dtype, out, m, None)

    p = od.oppoint(2, 64, od.MODE_OF, 1)

    def run_interp(a=i, b=i, n=1, width=64, height=64, p=p, t=half, nt=None, out_dtype=0, out=o):
        return L.ofdis_run_interp_u8(hd, a, b, n, width, height, C.byref(p) if p is not None else None, t[1],
                                     len(t[0]) if nt is None else nt, out_dtype, out, m, None)

    long_t = times(*([0.5] * 17))
    for call, name in ((interp, "interp"), (run_interp, "run_interp")):
        assert call(nt=0) == INV, name
        still_works(f"{name} nt 0")
        assert call(t=long_t) == INV, name
        still_works(f"{name} nt 17")
        for bad in (-0.1, 1.5, float("nan"), float("inf")):
            assert call(t=times(0.5, bad)) == INV, (name, bad)
            still_works(f"{name} t {bad}")
        assert call(a=None) == INV and call(b=None) == INV and call(out=None) == INV and call(t=(half[0], None)) == INV
        assert call(n=0) == INV and call(width=0) == INV and call(height=-1) == INV and call(out_dtype=2) == INV
        still_works(f"{name} NULL pointers and sizes")
    assert interp(fw=None) == INV and interp(bw=None) == INV and interp(noc=2) == INV
    assert L.ofdis_interp_u8(hd, i, i, f, f, None, 1, w, h, 1, half[1], 1, None, None, 0, o, m, None) == INV
    assert interp(v=view(dtype=2)) == INV and interp(v=view(layout=2)) == INV and interp(v=view(grid=2)) == INV
    assert interp(v=view(grid=1, cell=3)) == INV
    assert interp(v=view(grid=1, cell=2, gw=w // 2 - 1, gh=h // 2)) == INV        # the grid does not cover the columns
    assert interp(v=view(grid=1, cell=2, gw=w // 2, gh=h // 2 - 1)) == INV        # ... the rows
    assert interp(v=view(grid=1, cell=2, gw=w // 2, gh=h // 2, off_x=1)) == INV   # ... once the offset is counted
    still_works("interp views")
    assert run_interp(p=None) == INV and run_interp(p=p.copy(noc=2)) == INV
    assert run_interp(p=od.oppoint(2, 64, od.MODE_DE, 1)) == UNS                  # depth mode
    still_works("run_interp parameters and depth mode")
    tv = {q.sc_l: np.zeros((96 >> q.sc_l, 176 >> q.sc_l, 2), f32)}
    ctx.set_capture(None, tv)
    try:
        assert run_interp() == UNS                                                # a stage capture that is set
    finally:
        ctx.set_capture(None, None)
    still_works("run_interp with a stage capture")
    # the context still works: the largest nt, a level view that just covers the frame, and the fused call
    most = times(*([0.5] * 16))
    assert interp(t=most) == OK
    torch.cuda.synchronize()
    assert torch.all(out[:16 * w * h] == 0) and torch.all(out[16 * w * h:] == 7)
    assert torch.all(val[:16 * w * h] == 3) and torch.all(val[16 * w * h:] == 7)
    assert interp(v=view(grid=1, cell=2, gw=w // 2, gh=h // 2)) == OK
    fw, bw = ctx.run_bidir(qa, qb, q)[:2]
    assert_same_pictures(ctx.run_interp(qa, qb, q, want_valid=True), ctx.interp(qa, qb, fw, bw, want_valid=True),
                         "after the refusals")


# --------------------------------------------------------------------------------------------- CLI

# t = k / (K + 1) for K = 2 as the CLI computes it: (float)k / (float)(K + 1)
CLI_TIMES = (f32(1) / f32(3), f32(2) / f32(3))


@pytest.mark.parametrize("noc,exe,ext", [(1, "run_OF_INTERP_INT", "pgm"), (3, "run_OF_INTERP_RGB", "ppm")])
def test_cli_interp(ctx, tmp_path, noc, exe, ext):
    """run_OF_INTERP_* with K = 2 writes run_interp_host's pictures at t = 1/3 and 2/3."""
    import of_dis_amd as od
    assert CLI_TIMES[0].dtype == f32 and float(CLI_TIMES[0]) == 0.3333333432674408 and float(CLI_TIMES[1]) == 0.6666666865348816
    w, h = 176, 96
    a, b = pairs(w, h, noc, 1)
    pa, pb = (str(tmp_path / f"{x}.{ext}") for x in ("a", "b"))
    od.write_pnm(pa, a[0])
    od.write_pnm(pb, b[0])
    prefix = str(tmp_path / "mid_")
    path = os.path.join(ROOT, "of_dis_amd", "bin", exe)
    r = subprocess.run([path, pa, pb, prefix, "2", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = ctx.run_interp_host(a, b, op2(w, noc), CLI_TIMES)
    for k in (1, 2):
        got = od.read_image(f"{prefix}{k:03d}.{ext}", noc)
        assert_picture(got[..., 0] if noc == 1 else got, want[0, k - 1], f"{exe} frame {k}")
    assert not np.array_equal(want[0, 0], want[0, 1])  # (the pair moves)
    assert not os.path.exists(f"{prefix}003.{ext}")
    r = subprocess.run([path, pa, pb, prefix], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "usage" in r.stderr
    r = subprocess.run([path, pa, pb, prefix, "17"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "usage" in r.stderr

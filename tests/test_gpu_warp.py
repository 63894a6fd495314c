"""The level-grid warp and the fused motion-compensation call (ofdis_warp_u8 with a level view, ofdis_run_warp_u8,
run_OF_WARP_INT).

Every comparison is on raw bits.  The level form must give the picture of the full-resolution form; run_warp must give
warp(b, run(a, b)); the full-resolution form itself is pinned to the numpy reference by test_warp.py, and the plain
flow to the oracle by the parity tests.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_warp import assert_picture, warp_reference

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_pairs = {}


def pairs(w, h, noc, n):
    """n distinct synthetic pairs, u8 [n, h, w(, 3)] twice; every pair is generated once."""
    import of_dis_amd as od
    have = _pairs.setdefault((w, h, noc), [])
    while len(have) < n:
        a, b = od.synth_pair(w, h, noc, len(have), od.MODE_OF)
        have.append((a[..., 0], b[..., 0]) if noc == 1 else (a, b))
    return tuple(np.stack([x[k] for x in have[:n]]) for k in (0, 1))


def explicit(sc_f, sc_l, noc=1):
    """Op-point-2-like parameters with the scales spelled out (the 20 positional CLI parameters)."""
    import of_dis_amd as od
    return od.params_from_strings(f"{sc_f} {sc_l} 12 12 0.05 0.95 0 8 0.40 0 1 0 1 10 10 5 1 3 1.6 0".split(),
                                  od.MODE_OF, noc)


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def assert_same_pictures(got, want, what):
    """Tuples (picture, valid) of torch tensors."""
    assert_picture(_np(got[0]), _np(want[0]), what)
    assert_picture(_np(got[1]), _np(want[1]), what + " (valid)")


# --------------------------------------------------------------------------------------------- level form == full form

def op2(w, noc=1):
    import of_dis_amd as od
    return od.oppoint(2, w, od.MODE_OF, noc)


LEVEL_CASES = {
    "160x120": (160, 120, 1, lambda: op2(160)),             # cell 2, no divisibility padding, vector form
    "150x110": (150, 110, 1, lambda: op2(150)),             # cell 1, off 1 / 1, scalar form
    "161x121": (161, 121, 1, lambda: op2(161)),             # cell 2, off 3 / 3, scalar form
    "150x110-rgb": (150, 110, 3, lambda: op2(150, 3)),
    "176x96-l0": (176, 96, 1, lambda: explicit(3, 0)),      # sc_l 0 / 1 / 2: cell 1 / 2 / 4, vector form
    "176x96-l1": (176, 96, 1, lambda: explicit(3, 1)),
    "176x96-l2": (176, 96, 1, lambda: explicit(3, 2)),
    "150x110-l0": (150, 110, 1, lambda: explicit(3, 0)),    # the same with off 1 / 1, scalar form
    "150x110-l1": (150, 110, 1, lambda: explicit(3, 1)),
    "150x110-l2": (150, 110, 1, lambda: explicit(3, 2)),
    "2100x70-l1": (2100, 70, 1, lambda: explicit(2, 1)),    # three 1024-column blocks, the last one partial
}


def expand_level(cells, g, W, H):
    """The full-resolution field of a level grid [n, gh, gw, 2] (float32): cv::resize INTER_LINEAR's taps as k_upsample
    applies them (xtap, the row clamp, up_px on values that already hold S * 2^sc_l), restated in numpy float32."""
    cells = np.ascontiguousarray(cells, f32)
    c, ox, oy = g["cell"], g["off_x"], g["off_y"]
    gh, gw = cells.shape[1:3]
    if c == 1:
        return cells[:, oy:oy + H, ox:ox + W]
    scale = 1.0 / c
    fx = ((np.arange(W) + ox + 0.5) * scale - 0.5).astype(f32)
    sx = np.floor(fx).astype(np.int64)
    fx = fx - sx.astype(f32)
    fx[sx < 0], sx[sx < 0] = 0, 0
    lin = sx + 1 < gw
    fx[~lin], sx[~lin] = 0, gw - 1
    fy = ((np.arange(H) + oy + 0.5) * scale - 0.5).astype(f32)
    sy = np.floor(fy).astype(np.int64)
    fy = (fy - sy.astype(f32))[None, :, None, None]
    r0, r1 = np.clip(sy, 0, gh - 1), np.clip(sy + 1, 0, gh - 1)
    fxb, linb = fx[None, None, :, None], lin[None, None, :, None]
    s0, s1 = cells[:, :, sx], cells[:, :, np.minimum(sx + 1, gw - 1)]
    with np.errstate(all="ignore"):
        hrow = np.where(linb, s0 * (f32(1) - fxb) + s1 * fxb, s0)
        out = hrow[:, r0] * (f32(1) - fy) + hrow[:, r1] * fy
    assert out.dtype == f32
    return out


@pytest.mark.parametrize("case", list(LEVEL_CASES))
def test_level_form_equals_full_form(ctx, case):
    import torch
    import of_dis_amd as od
    w, h, noc, mk = LEVEL_CASES[case]
    p = mk()
    a, b = (_dev(x) for x in pairs(w, h, noc, 2))
    full = ctx.run(a, b, p)
    level = ctx.run(a, b, p, grid="level")
    g = od.out_geometry(p, w, h, grid="level")
    for scale in (1.0, 0.5):
        for out_dtype in (torch.uint8, torch.float32):
            want = ctx.warp(b, full, scale, out_dtype, want_valid=True)
            got = ctx.warp(b, level, scale, out_dtype, grid="level", p=p, want_valid=True)
            assert_same_pictures(got, want, f"{case} scale {scale} {out_dtype}")
    # the planar level grid is the same view transposed
    planar = ctx.run(a, b, p, layout="nchw", grid="level")
    got = ctx.warp(b, planar, 1.0, torch.uint8, layout="nchw", grid="level", p=p, want_valid=True)
    assert_same_pictures(got, ctx.warp(b, full, want_valid=True), f"{case} planar level grid")
    # float16 cells: no kernel expands a binary16 grid to a field, so the upsample's taps are restated in numpy
    # (expand_level) -- checked first on the float32 grid, where it must reproduce the plain call's field -- and
    # warp_reference is fed with the expansion of the float16 cells
    assert_picture(expand_level(_np(level), g, w, h), _np(full), f"{case}: expand_level against the plain call")
    for layout in ("nhwc", "nchw"):
        half = ctx.run(a, b, p, dtype=torch.float16, layout=layout, grid="level")
        cells = _np(half).astype(f32)
        if layout == "nchw":
            cells = cells.transpose(0, 2, 3, 1)
        want, want_valid = warp_reference(_np(b), expand_level(cells, g, w, h))
        got = ctx.warp(b, half, layout=layout, grid="level", p=p, want_valid=True)
        assert_picture(_np(got[0]), want, f"{case} float16 {layout} level grid")
        assert_picture(_np(got[1]), want_valid, f"{case} float16 {layout} level grid (valid)")


def test_level_form_equals_full_form_1080p(ctx):
    """One 1920 x 1080 op-point-2 pair: 16-pixel cells, 8 padded rows (off_y 4), two 1024-column blocks."""
    import torch
    import of_dis_amd as od
    w, h = 1920, 1080
    p = op2(w)
    g = od.out_geometry(p, w, h, grid="level")
    assert (g["cell"], g["off_x"], g["off_y"], g["out_w"], g["out_h"]) == (16, 0, 4, 120, 68)
    a, b = (_dev(x) for x in pairs(w, h, 1, 1))
    full = ctx.run(a, b, p)
    level = ctx.run(a, b, p, grid="level")
    for out_dtype in (torch.uint8, torch.float32):
        want = ctx.warp(b, full, 1.0, out_dtype, want_valid=True)
        got = ctx.warp(b, level, 1.0, out_dtype, grid="level", p=p, want_valid=True)
        assert_same_pictures(got, want, f"1080p {out_dtype}")
    assert_same_pictures(ctx.run_warp(a, b, p, want_valid=True), ctx.warp(b, full, want_valid=True), "1080p run_warp")


# --------------------------------------------------------------------------------------------- run_warp

RUN_CASES = {
    "gray-1": (176, 96, 1, 2, 1),
    "gray-5": (176, 96, 1, 2, 5),
    "gray-odd-5": (173, 97, 1, 2, 5),   # padding on both axes, scalar form
    "rgb-1": (176, 96, 3, 2, 1),
    "rgb-5": (176, 96, 3, 2, 5),
    "rgb-op3-5": (192, 128, 3, 3, 5),   # sc_l 0: cell 1
}
ISSUES = {"default": {}, "streams2-chunk2": {"streams": 2, "chunk": 2}, "graph0": {"graph": 0},
          "streams2-chunk2-graph2": {"streams": 2, "chunk": 2, "graph": 2}}


@pytest.mark.parametrize("issue", list(ISSUES))
@pytest.mark.parametrize("case", list(RUN_CASES))
def test_run_warp_equals_warp_of_run(case, issue):
    import torch
    import of_dis_amd as od
    w, h, noc, op, n = RUN_CASES[case]
    p = od.oppoint(op, w, od.MODE_OF, noc)
    a, b = (_dev(x) for x in pairs(w, h, noc, n))
    c = od.Context(0)
    try:
        for k, v in ISSUES[issue].items():
            c.set_option(k, v)
        flow = c.run(a, b, p)
        level = c.run(a, b, p, grid="level")
        for scale, out_dtype in ((1.0, torch.uint8), (0.5, torch.float32)):
            want = c.warp(b, flow, scale, out_dtype, want_valid=True)
            first = c.run_warp(a, b, p, scale, out_dtype, want_valid=True)
            second = c.run_warp(a, b, p, scale, out_dtype, want_valid=True)
            assert_same_pictures(first, want, f"{case} {issue} scale {scale}: first call")
            assert_same_pictures(second, want, f"{case} {issue} scale {scale}: second call")
        # the same output pointers twice: the second call replays the captured graph
        out = torch.empty_like(want[0])
        valid = torch.empty_like(want[1])
        for rep in range(2):
            out.fill_(77)
            valid.fill_(77)
            c.run_warp_ptr(a.data_ptr(), b.data_ptr(), n, w, h, p, 0.5, od.IMG_F32, out.data_ptr(), valid.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
            assert_same_pictures((out, valid), want, f"{case} {issue}: call {rep} on fixed pointers")
        # without the mask
        assert_picture(_np(c.run_warp(a, b, p)), _np(c.warp(b, flow)), f"{case} {issue}: no mask")
        # the plain and the level-grid calls on the same images still return their flows (the graph key)
        assert_picture(_np(c.run(a, b, p)), _np(flow), f"{case} {issue}: plain run after run_warp")
        assert_picture(_np(c.run(a, b, p, grid="level")), _np(level), f"{case} {issue}: level run after run_warp")
        assert_same_pictures(c.run_warp(a, b, p, want_valid=True), c.warp(b, flow, want_valid=True),
                             f"{case} {issue}: run_warp after the plain runs")
    finally:
        c.close()


def test_run_warp_host_and_timers(ctx):
    import of_dis_amd as od
    w, h = 176, 96
    p = op2(w)
    a, b = pairs(w, h, 1, 2)
    want = ctx.warp(_dev(b), ctx.run(_dev(a), _dev(b), p), want_valid=True)
    out, valid = ctx.run_warp_host(a, b, p, want_valid=True)
    assert_picture(out, _np(want[0]), "run_warp_host")
    assert_picture(valid, _np(want[1]), "run_warp_host (valid)")
    a1, b1 = od.synth_pair(w, h, 1, 0, od.MODE_OF)  # a single pair [h, w, 1]
    assert_picture(ctx.run_warp_host(a1, b1, p)[..., 0], out[0], "run_warp_host, single pair")
    ctx.enable_kernel_timing(True)
    try:
        ctx.run_warp(_dev(a), _dev(b), p)
        ctx.warp(_dev(b), ctx.run(_dev(a), _dev(b), p))
        assert ctx.kernel_time("warp_level")[1] == 1 and ctx.kernel_time("warp")[1] == 1
        assert ctx.kernel_time("level_out")[1] == 1 and ctx.kernel_time("upsample")[1] == 1  # no upsample in run_warp
    finally:
        ctx.enable_kernel_timing(False)


def test_run_warp_stage_capture(ctx):
    """A stage capture behaves as in the formatted call: frame 0's finest level comes back, and the picture is right."""
    w, h = 176, 96
    p = op2(w)
    a, b = (_dev(x) for x in pairs(w, h, 1, 2))
    want = ctx.warp(b, ctx.run(a, b, p), want_valid=True)
    level = _np(ctx.run(a, b, p, grid="level"))
    tv = {p.sc_l: np.zeros((h >> p.sc_l, w >> p.sc_l, 2), f32)}
    ctx.set_capture(None, tv)
    try:
        got = ctx.run_warp(a, b, p, want_valid=True)
        assert_same_pictures(got, want, "run_warp with a stage capture")
    finally:
        ctx.set_capture(None, None)
    assert_picture(tv[p.sc_l] * f32(1 << p.sc_l), level[0], "captured finest level")


# --------------------------------------------------------------------------------------------- refusals

def test_refusals_leave_the_context_usable(ctx):
    import torch
    import of_dis_amd as od
    L = od.lib()
    INV, UNS, OK = od._lib.ERR_INVALID_ARGUMENT, od._lib.ERR_UNSUPPORTED, od._lib.OK
    w, h = 16, 8
    img = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
    flow = torch.zeros(w * h * 2, dtype=torch.float32, device="cuda")
    out = torch.full((w * h * 3 * 4,), 7, dtype=torch.uint8, device="cuda")
    val = torch.full((w * h,), 7, dtype=torch.uint8, device="cuda")
    i, f, o, m, hd = img.data_ptr(), flow.data_ptr(), out.data_ptr(), val.data_ptr(), ctx._h

    def view(dtype=0, layout=0, grid=0, gw=w, gh=h, cell=1, off_x=0, off_y=0):
        return C.byref(od.FlowView(dtype, layout, grid, gw, gh, cell, off_x, off_y))

    def warp(img=i, flow=f, v=None, n=1, width=w, height=h, noc=1, scale=1.0, out_dtype=0, out=o):
        return L.ofdis_warp_u8(hd, img, flow, v if v is not None else view(), n, width, height, noc, scale, out_dtype,
                               out, m, None)

    assert warp(img=None) == INV and warp(flow=None) == INV and warp(out=None) == INV
    assert L.ofdis_warp_u8(hd, i, f, None, 1, w, h, 1, 1.0, 0, o, m, None) == INV
    assert warp(n=0) == INV and warp(n=-1) == INV
    assert warp(width=0) == INV and warp(height=0) == INV and warp(width=-4) == INV
    assert warp(noc=2) == INV and warp(noc=0) == INV and warp(noc=4) == INV
    assert warp(out_dtype=2) == INV and warp(out_dtype=-1) == INV
    assert warp(v=view(dtype=2)) == INV and warp(v=view(layout=2)) == INV and warp(v=view(grid=2)) == INV
    assert warp(v=view(dtype=-1)) == INV
    for cell in (0, 3, 6, 1024, -2):
        assert warp(v=view(grid=1, cell=cell, gw=w, gh=h)) == INV, cell
    assert warp(v=view(grid=1, cell=2, gw=w // 2 - 1, gh=h // 2)) == INV        # the grid does not cover the columns
    assert warp(v=view(grid=1, cell=2, gw=w // 2, gh=h // 2 - 1)) == INV        # ... the rows
    assert warp(v=view(grid=1, cell=2, gw=w // 2, gh=h // 2, off_x=1)) == INV   # ... once the offset is counted
    assert warp(v=view(grid=1, cell=2, gw=w // 2, gh=h // 2, off_y=1)) == INV
    assert warp(v=view(grid=1, cell=2, gw=w // 2, gh=h // 2, off_x=-1)) == INV
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert warp(scale=bad) == INV
    assert warp(width=65536, height=32768) == INV                                # 2^31 pixels
    # the fused call
    p = od.oppoint(2, 64, od.MODE_OF, 1)

    def run_warp(a=i, b=i, n=1, width=64, height=64, p=p, scale=1.0, out_dtype=0, out=o):
        return L.ofdis_run_warp_u8(hd, a, b, n, width, height, C.byref(p) if p is not None else None, scale,
                                   out_dtype, out, m, None)

    assert run_warp(a=None) == INV and run_warp(b=None) == INV and run_warp(out=None) == INV
    assert run_warp(n=0) == INV and run_warp(width=0) == INV and run_warp(height=-1) == INV and run_warp(p=None) == INV
    assert run_warp(scale=float("nan")) == INV and run_warp(scale=float("inf")) == INV
    assert run_warp(out_dtype=2) == INV
    assert run_warp(p=p.copy(noc=2)) == INV
    assert run_warp(p=od.oppoint(2, 64, od.MODE_DE, 1)) == UNS                   # depth mode
    torch.cuda.synchronize()
    assert torch.all(out == 7) and torch.all(val == 7)  # nothing was enqueued by the refused calls
    # the context still works: a level view that just covers the frame, and the fused call
    assert warp(v=view(grid=1, cell=2, gw=w // 2, gh=h // 2)) == OK
    torch.cuda.synchronize()
    assert torch.all(out[:w * h] == 0) and torch.all(out[w * h:] == 7) and torch.all(val == 1)
    a, b = (_dev(x) for x in pairs(176, 96, 1, 1))
    q = op2(176)
    assert_same_pictures(ctx.run_warp(a, b, q, want_valid=True), ctx.warp(b, ctx.run(a, b, q), want_valid=True),
                         "after the refusals")


# --------------------------------------------------------------------------------------------- CLI

def test_cli_warp_int(ctx, tmp_path):
    """run_OF_WARP_INT on two PGMs writes run_warp_host's picture."""
    import of_dis_amd as od
    w, h = 176, 96
    a, b = pairs(w, h, 1, 1)
    pa, pb, po = (str(tmp_path / x) for x in ("a.pgm", "b.pgm", "out.pgm"))
    od.write_pnm(pa, a[0])
    od.write_pnm(pb, b[0])
    exe = os.path.join(ROOT, "of_dis_amd", "bin", "run_OF_WARP_INT")
    r = subprocess.run([exe, pa, pb, po, "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = od.read_image(po, 1)[..., 0]
    assert_picture(got, ctx.run_warp_host(a, b, op2(w))[0], "run_OF_WARP_INT")
    assert not np.array_equal(got, b[0])  # (the pair moves)
    r = subprocess.run([exe, pa, pb], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "usage" in r.stderr


def test_cli_warp_rgb(ctx, tmp_path):
    import of_dis_amd as od
    w, h = 176, 96
    a, b = pairs(w, h, 3, 1)
    pa, pb, po = (str(tmp_path / x) for x in ("a.ppm", "b.ppm", "out.ppm"))
    od.write_pnm(pa, a[0])
    od.write_pnm(pb, b[0])
    exe = os.path.join(ROOT, "of_dis_amd", "bin", "run_OF_WARP_RGB")
    r = subprocess.run([exe, pa, pb, po], capture_output=True, text=True, timeout=120)  # op-point 2 by default
    assert r.returncode == 0, r.stderr
    assert_picture(od.read_image(po, 3), ctx.run_warp_host(a, b, op2(w, 3))[0], "run_OF_WARP_RGB")

"""The forward-backward check on level grids (ofdis_fb_check_level, k_fb_check_level).

Every comparison is on raw bits.  On the pipeline's own grids the level check must give what ofdis_fb_check gives on
the two full-resolution flows; on synthetic grids, independent of the flow pipeline, it must give the numpy reference
of test_fb_check.py applied to the grids expanded in numpy (expand_level of test_gpu_warp.py, itself checked against
the plain call there).
"""
import ctypes as C

import numpy as np
import pytest

from test_fb_check import assert_err_equal, fb_reference
from test_gpu_warp import LEVEL_CASES, _dev, _np, expand_level, pairs

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 64  # bytes of sentinel on both sides of every output


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


def assert_check_equal(got, want, what):
    """(occ_fw, occ_bw, err_fw, err_bw) as numpy arrays."""
    for k in (0, 1):
        bad = got[k] != want[k]
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} codes of mask {k} differ, first at {np.argwhere(bad)[0]}"
        assert_err_equal(got[2 + k], want[2 + k], want[k], f"{what}: err {k}")


# --------------------------------------------------------------------------------------------- the pipeline's grids

@pytest.mark.parametrize("case", list(LEVEL_CASES))
def test_level_check_equals_full_check(ctx, case):
    w, h, noc, mk = LEVEL_CASES[case]
    p = mk()
    a, b = (_dev(x) for x in pairs(w, h, noc, 2))
    want = [_np(x) for x in ctx.fb_check(ctx.run(a, b, p), ctx.run(b, a, p), want_err=True)]
    gf, gb = ctx.run(a, b, p, grid="level"), ctx.run(b, a, p, grid="level")
    got = [_np(x) for x in ctx.fb_check(gf, gb, grid="level", p=p, size=(w, h), want_err=True)]
    assert_check_equal(got, want, case)
    assert any((m == 0).any() and (m != 0).any() for m in want[:2]), f"{case}: the masks are constant"


# --------------------------------------------------------------------------------------------- synthetic grids

# name: (W, H, cell, off_x, off_y, gw, gh)
GEOMS = {
    "1x1-c2": (1, 1, 2, 0, 0, 1, 1),
    "5x3-c4": (5, 3, 4, 1, 1, 2, 1),          # scalar form, a partial cell on every edge
    "64x4-c1": (64, 4, 1, 0, 0, 64, 4),       # the log2c == 0 branch, vector form
    "67x5-c2": (67, 5, 2, 1, 1, 34, 3),
    "176x96-c16": (176, 96, 16, 0, 4, 11, 7),
    "2100x6-c2": (2100, 6, 2, 0, 0, 1050, 3),  # three column blocks, the last partial
}
KINDS = ["zero", "opposite", "smooth", "large", "nonfinite", "threshold"]


def geom_dict(name):
    W, H, cell, ox, oy, gw, gh = GEOMS[name]
    return W, H, {"cell": cell, "off_x": ox, "off_y": oy, "out_w": gw, "out_h": gh}


def make_grids(kind, gw, gh, n, seed):
    """-> (grid_fw, grid_bw, alpha, beta), float32 [n, gh, gw, 2]"""
    rng = np.random.default_rng(seed)
    gf = np.zeros((n, gh, gw, 2), f32)
    alpha, beta = 0.01, 0.5
    if kind == "zero":
        gb = gf.copy()
    elif kind == "opposite":
        gf[..., 0], gf[..., 1] = 2.5, -1.25
        gb = -gf
    elif kind in ("smooth", "nonfinite"):
        gf = (rng.standard_normal(gf.shape) * 3).astype(f32)
        gb = (-gf + rng.standard_normal(gf.shape).astype(f32) * f32(0.4)).astype(f32)  # some pass, some fail
        if kind == "nonfinite":
            for fld in (gf, gb):
                flat = fld.reshape(-1)
                k = max(3, flat.size // 50) if flat.size >= 6 else 1
                flat[rng.choice(flat.size, size=k, replace=False)] = np.resize(np.array([np.nan, np.inf, -np.inf], f32), k)
    elif kind == "large":  # flows that leave the frame: code 2 and +inf
        gf = (rng.standard_normal(gf.shape) * 40).astype(f32)
        gb = (rng.standard_normal(gf.shape) * 40).astype(f32)
    elif kind == "threshold":  # err = 2 = alpha * 2 + beta exactly where u = (1, 1); 1 + 2^-20 tips it over
        alpha, beta = 0.75, 0.5
        gf[...] = 1
        gf[..., 0][rng.random((n, gh, gw)) < 0.5] = f32(1 + 2.0 ** -20)
        gb = np.zeros_like(gf)
    return gf, gb, alpha, beta


def view_of(g, dtype=0, layout=0, grid=1):
    import of_dis_amd as od
    return od._lib.FlowView(dtype, layout, grid, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])


def gpu_level_check(ctx, gf, gb, g, W, H, alpha, beta, outs=(1, 1, 1, 1), occ_off=0, err_off=0):
    """ofdis_fb_check_level through raw pointers.  outs: which of (occ_fw, occ_bw, err_fw, err_bw) are passed; occ_off /
    err_off bytes shift the mask / error buffers off their natural alignment.  Every output sits between sentinels,
    which must survive.  -> the four outputs as numpy arrays (None where not passed)."""
    import torch
    n = gf.shape[0]
    px = n * H * W
    dev = [_dev(np.ascontiguousarray(x, f32)) for x in (gf, gb)]
    bufs, ptrs = [], []
    for k in range(4):
        if not outs[k]:
            bufs.append(None)
            ptrs.append(0)
            continue
        size, off = (px, occ_off) if k < 2 else (4 * px, err_off)
        t = torch.full((size + 2 * GUARD + off,), 0xAB, dtype=torch.uint8, device="cuda")
        bufs.append((t, off, size))
        ptrs.append(t.data_ptr() + GUARD + off)
    ctx.fb_check_level_ptr(dev[0].data_ptr(), dev[1].data_ptr(), view_of(g), n, W, H, alpha, beta, *ptrs,
                           torch.cuda.current_stream().cuda_stream)
    res = []
    for k, buf in enumerate(bufs):
        if buf is None:
            res.append(None)
            continue
        t, off, size = buf
        raw = _np(t)
        assert np.all(raw[:GUARD + off] == 0xAB) and np.all(raw[GUARD + off + size:] == 0xAB), f"output {k}: a sentinel was overwritten"
        body = raw[GUARD + off:GUARD + off + size].copy()
        res.append(body.reshape(n, H, W) if k < 2 else body.view(f32).reshape(n, H, W))
    return res


_refs = {}


def reference(geom, kind, n=3):
    """The grids of a case and the numpy reference of their check, computed once."""
    key = (geom, kind, n)
    if key not in _refs:
        W, H, g = geom_dict(geom)
        gf, gb, alpha, beta = make_grids(kind, g["out_w"], g["out_h"], n, sum(map(ord, geom + kind)) + n)
        want = fb_reference(expand_level(gf, g, W, H), expand_level(gb, g, W, H), alpha, beta)
        _refs[key] = (gf, gb, alpha, beta, want)
    return _refs[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_synthetic_grids(ctx, geom, kind):
    W, H, g = geom_dict(geom)
    gf, gb, alpha, beta, want = reference(geom, kind)
    got = gpu_level_check(ctx, gf, gb, g, W, H, alpha, beta)
    assert_check_equal(got, want, f"{geom} {kind}")
    if kind == "large" and W * H > 1:
        assert (want[0] == 2).any() and np.isposinf(want[2]).any()
    if kind == "smooth" and W * H > 100:
        assert (want[0] == 0).any() and (want[0] == 1).any()


# --------------------------------------------------------------------------------------------- outputs and pointers

@pytest.mark.parametrize("geom", ["64x4-c1", "176x96-c16", "67x5-c2"])
def test_each_output_alone(ctx, geom):
    W, H, g = geom_dict(geom)
    gf, gb, alpha, beta, want = reference(geom, "smooth")
    for k in range(4):
        outs = tuple(int(j == k) for j in range(4))
        got = gpu_level_check(ctx, gf, gb, g, W, H, alpha, beta, outs)
        assert [x is not None for x in got] == [bool(o) for o in outs]
        if k < 2:
            assert np.array_equal(got[k], want[k]), f"{geom}: mask {k} alone"
        else:
            assert_err_equal(got[k], want[k], want[k - 2], f"{geom}: err {k - 2} alone")


def test_no_output_is_ok_and_enqueues_nothing(ctx):
    import of_dis_amd as od
    W, H, g = geom_dict("64x4-c1")
    gf, gb, alpha, beta, _ = reference("64x4-c1", "smooth")
    assert gpu_level_check(ctx, gf, gb, g, W, H, alpha, beta, (0, 0, 0, 0)) == [None] * 4
    ctx.enable_kernel_timing(True)
    try:
        before = ctx.kernel_time("fb_check_level")[1]
        gpu_level_check(ctx, gf, gb, g, W, H, alpha, beta, (0, 0, 0, 0))
        assert ctx.kernel_time("fb_check_level")[1] == before
        gpu_level_check(ctx, gf, gb, g, W, H, alpha, beta, (1, 0, 0, 0))
        assert ctx.kernel_time("fb_check_level")[1] == before + 1
    finally:
        ctx.enable_kernel_timing(False)
    # a view is still checked
    assert od.lib().ofdis_fb_check_level(ctx._h, 16, 16, None, 1, W, H, 0.01, 0.5, None, None, None, None,
                                         None) == od._lib.ERR_INVALID_ARGUMENT


@pytest.mark.parametrize("geom", ["64x4-c1", "176x96-c16"])
@pytest.mark.parametrize("occ_off,err_off", [(1, 0), (2, 0), (3, 0), (0, 4), (1, 4)])
def test_unaligned_outputs_take_the_scalar_form(ctx, geom, occ_off, err_off):
    W, H, g = geom_dict(geom)
    gf, gb, alpha, beta, want = reference(geom, "smooth")
    got = gpu_level_check(ctx, gf, gb, g, W, H, alpha, beta, occ_off=occ_off, err_off=err_off)
    assert_check_equal(got, want, f"{geom} mask offset {occ_off} error offset {err_off}")


def test_one_frame_above_the_launch_slice(ctx):
    """32768 frames of 4 x 2 on a 2 x 1 grid of cell 2: the second launch holds the last frame alone.  65535 frames: three
    launches, the middle one full."""
    W, H, g = 4, 2, {"cell": 2, "off_x": 0, "off_y": 0, "out_w": 2, "out_h": 1}
    for n in (32768, 65535):
        gf, gb, alpha, beta = make_grids("smooth", 2, 1, n, 99)
        want = fb_reference(expand_level(gf, g, W, H), expand_level(gb, g, W, H), alpha, beta)
        got = gpu_level_check(ctx, gf, gb, g, W, H, alpha, beta)
        assert_check_equal(got, want, f"{n} frames")
        assert (want[0][-1] != want[0][0]).any() or (want[2][-1] != want[2][0]).any()  # (the last frame is its own)


# --------------------------------------------------------------------------------------------- refusals

def test_refusals_leave_the_context_usable(ctx):
    import torch
    import of_dis_amd as od
    L = od.lib()
    INV, UNS, OK = od._lib.ERR_INVALID_ARGUMENT, od._lib.ERR_UNSUPPORTED, od._lib.OK
    W, H, g = geom_dict("67x5-c2")
    gf, gb, alpha, beta, want = reference("67x5-c2", "smooth")
    n = gf.shape[0]
    dgf, dgb = _dev(gf), _dev(gb)
    occ = torch.full((n * H * W,), 7, dtype=torch.uint8, device="cuda")

    def call(fw=dgf.data_ptr(), bw=dgb.data_ptr(), v=None, n=n, width=W, height=H, alpha=alpha, beta=beta):
        return L.ofdis_fb_check_level(ctx._h, fw, bw, C.byref(v if v is not None else view_of(g)), n, width, height,
                                      alpha, beta, occ.data_ptr(), None, None, None, None)

    def untouched(what):
        torch.cuda.synchronize()
        assert torch.all(occ == 7), what

    assert call(v=view_of(g, dtype=1)) == UNS        # float16 cells
    assert call(v=view_of(g, layout=1)) == UNS       # planar
    assert call(v=view_of(g, grid=0)) == UNS         # a full-resolution field
    untouched("unsupported views")
    assert call(v=view_of(g, dtype=2)) == INV and call(v=view_of(g, layout=2)) == INV and call(v=view_of(g, grid=2)) == INV
    assert call(v=view_of(dict(g, out_w=g["out_w"] - 1))) == INV   # the grid does not cover the columns
    assert call(v=view_of(dict(g, out_h=g["out_h"] - 1))) == INV   # ... the rows
    assert call(v=view_of(dict(g, off_x=2))) == INV                # ... once the offset is counted
    assert call(v=view_of(dict(g, cell=3))) == INV and call(v=view_of(dict(g, off_y=-1))) == INV
    assert call(alpha=-0.01) == INV and call(beta=-1.0) == INV and call(alpha=float("nan")) == INV
    assert call(fw=None) == INV and call(bw=None) == INV
    assert call(n=0) == INV and call(width=0) == INV and call(height=-1) == INV
    untouched("invalid arguments")
    assert call() == OK
    assert np.array_equal(_np(occ).reshape(n, H, W), want[0])
    assert_check_equal(gpu_level_check(ctx, gf, gb, g, W, H, alpha, beta), want, "after the refusals")

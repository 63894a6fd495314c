"""Backward image warp along a flow (ofdis_warp_u8, include/ofdis.h).

`warp_reference` below restates the header's definition in vectorised numpy float32 -- every operation on float32
arrays, one rounding each, in the header's order -- and is the reference of every picture and mask comparison here and
in test_gpu_warp.py.

CPU part: the new symbols, their NULL-context refusal, the PNM writer, known answers of the reference itself, and the
photometric gain of warping along the oracle's flow.
GPU part (marked gpu): k_warp against the reference.  u8 pictures and masks must be equal, float32 pictures must have
equal uint32 views (the taps are finite and ax, ay lie in [0, 1), so no picture value is ever NaN).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_fb_check import _smooth

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------- reference

def warp_reference(img, flow, scale=1.0, out_dtype=np.uint8):
    """img u8 [n, h, w] or [n, h, w, c]; flow [n, h, w, 2] (converted to float32 exactly) -> (picture in img's shape,
    u8 or float32; valid u8 [n, h, w])."""
    img = np.asarray(img, np.uint8)
    im = img[..., None] if img.ndim == 3 else img
    F = np.ascontiguousarray(flow).astype(f32)
    n, h, w, _ = im.shape
    assert F.shape == (n, h, w, 2)
    xs = np.arange(w, dtype=f32)[None, None, :]
    ys = np.arange(h, dtype=f32)[None, :, None]
    s = f32(scale)
    with np.errstate(all="ignore"):
        su, sv = s * F[..., 0], s * F[..., 1]
        px, py = xs + su, ys + sv
        inside = (px >= 0) & (px <= f32(w - 1)) & (py >= 0) & (py <= f32(h - 1))  # False for NaN
        pxc = np.fmin(np.fmax(px, f32(0)), f32(w - 1))  # fmax / fmin: NaN -> 0
        pyc = np.fmin(np.fmax(py, f32(0)), f32(h - 1))
        x0, y0 = np.floor(pxc).astype(np.int64), np.floor(pyc).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        ax, ay = (pxc - x0.astype(f32))[..., None], (pyc - y0.astype(f32))[..., None]
        fi = np.arange(n)[:, None, None]
        t00, t01 = im[fi, y0, x0].astype(f32), im[fi, y0, x1].astype(f32)
        t10, t11 = im[fi, y1, x0].astype(f32), im[fi, y1, x1].astype(f32)
        top = t00 + ax * (t01 - t00)
        bot = t10 + ax * (t11 - t10)
        val = top + ay * (bot - top)
    assert val.dtype == f32 and ax.dtype == f32 and px.dtype == f32
    if np.dtype(out_dtype) == np.uint8:
        val = np.rint(val)  # round half to even
        assert val.min() >= 0 and val.max() <= 255  # no clamp needed
        val = val.astype(np.uint8)
    return val.reshape(img.shape), inside.astype(np.uint8)


# --------------------------------------------------------------------------------------------- CPU

SIGNATURES = {
    "ofdis_warp_u8": 13,
    "ofdis_run_warp_u8": 12,
    "ofdis_run_warp_u8_host": 11,
}


def test_symbols_exist_with_declared_signatures():
    import of_dis_amd as od
    L = od.lib()
    hdr = open(os.path.join(ROOT, "include", "ofdis.h")).read()
    for name, nargs in SIGNATURES.items():
        fn = getattr(L, name)
        assert len(fn.argtypes) == nargs and fn.restype is C.c_int
        m = re.search(rf"\bint {name}\(([^;]*)\);", hdr)
        assert m, f"{name} is not declared in ofdis.h"
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert len(args) == nargs, (name, args)
        assert args[0] == "ofdis_context *ctx"
    decl = re.search(r"\bint ofdis_warp_u8\(([^;]*)\);", hdr).group(1)
    assert re.sub(r"\s+", " ", decl) == (
        "ofdis_context *ctx, const uint8_t *img, const void *flow, const ofdis_flow_view *view, int n, int width, "
        "int height, int noc, float scale, int out_dtype, void *out, uint8_t *valid, void *stream")
    decl = re.search(r"\bint ofdis_run_warp_u8\(([^;]*)\);", hdr).group(1)
    assert re.sub(r"\s+", " ", decl) == (
        "ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height, "
        "const ofdis_params *p, float scale, int out_dtype, void *out, uint8_t *valid, void *stream")
    decl = re.search(r"\bint ofdis_write_pnm\(([^;]*)\);", hdr).group(1)
    assert re.sub(r"\s+", " ", decl) == "const char *path, const uint8_t *pixels, int width, int height, int noc"
    assert len(L.ofdis_write_pnm.argtypes) == 5
    m = re.search(r"typedef struct ofdis_flow_view \{([^}]*)\}", hdr)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "int dtype, layout, grid, gw, gh, cell, off_x, off_y;"
    assert [k for k, _ in od.FlowView._fields_] == ["dtype", "layout", "grid", "gw", "gh", "cell", "off_x", "off_y"]
    assert re.search(r"OFDIS_IMG_U8 = 0, OFDIS_IMG_F32 = 1", hdr) and (od.IMG_U8, od.IMG_F32) == (0, 1)
    assert L.ofdis_abi_version() == 2
    assert {"warp", "warp_level"} <= set(od.kernel_names())


def test_null_context_is_refused():
    import of_dis_amd as od
    L = od.lib()
    p = od.oppoint(2, 64, od.MODE_OF, 1)
    flow = np.zeros(64 * 64 * 2, f32)
    img = np.zeros(64 * 64, np.uint8)
    d, im = flow.ctypes.data, img.ctypes.data
    v = od.FlowView(0, 0, 0, 64, 64, 1, 0, 0)
    INV = od._lib.ERR_INVALID_ARGUMENT
    assert L.ofdis_warp_u8(None, im, d, C.byref(v), 1, 64, 64, 1, 1.0, 0, im, None, None) == INV
    assert L.ofdis_run_warp_u8(None, im, im, 1, 64, 64, C.byref(p), 1.0, 0, im, None, None) == INV
    assert L.ofdis_run_warp_u8_host(None, im, im, 1, 64, 64, C.byref(p), 1.0, 0, im, None) == INV


def test_byte_model():
    import of_dis_amd as od
    p = od.oppoint(2, 1920, od.MODE_OF, 1)
    px = 1920 * 1080
    g = od.out_geometry(p, 1920, 1080, grid="level")
    assert od.algorithmic_bytes(p, 1920, 1080, "warp") == px * (1 + 8 + 1 + 1)
    assert od.algorithmic_bytes(p, 1920, 1080, "warp_level") == px * (1 + 1 + 1) + g["bytes_per_pair"]
    p3 = od.oppoint(2, 1920, od.MODE_OF, 3)
    assert od.algorithmic_bytes(p3, 1920, 1080, "warp") == px * (3 + 8 + 3 + 1)


@pytest.mark.parametrize("noc", [1, 3])
def test_write_pnm_round_trip(tmp_path, noc):
    import of_dis_amd as od
    L = od.lib()
    rng = np.random.default_rng(noc)
    w, h = 13, 7
    px = rng.integers(0, 256, (h, w, noc), dtype=np.uint8)
    path = str(tmp_path / ("x.pgm" if noc == 1 else "x.ppm"))
    od.write_pnm(path, px)
    raw = open(path, "rb").read()
    head = b"P%d\n%d %d\n255\n" % (5 if noc == 1 else 6, w, h)
    assert raw.startswith(head) and len(raw) == len(head) + px.size
    body = np.frombuffer(raw[len(head):], np.uint8).reshape(h, w, noc)
    assert np.array_equal(body, px[..., ::-1])  # BGR in memory, RGB in the file
    back = np.zeros_like(px)
    rw, rh, rn = C.c_int(), C.c_int(), C.c_int()
    assert L.ofdis_read_pnm(path.encode(), back.ctypes.data, C.byref(rw), C.byref(rh), C.byref(rn), back.size) == 0
    assert (rw.value, rh.value, rn.value) == (w, h, noc) and np.array_equal(back, px)
    INV = od._lib.ERR_INVALID_ARGUMENT
    assert L.ofdis_write_pnm(path.encode(), px.ctypes.data, w, h, 2) == INV
    assert L.ofdis_write_pnm(path.encode(), None, w, h, noc) == INV
    assert L.ofdis_write_pnm(str(tmp_path / "no" / "dir.pgm").encode(), px.ctypes.data, w, h, noc) == od._lib.ERR_IO


def test_reference_zero_flow_is_identity():
    rng = np.random.default_rng(0)
    for shape in [(2, 5, 7), (2, 5, 7, 3)]:
        img = rng.integers(0, 256, shape, dtype=np.uint8)
        out, valid = warp_reference(img, np.zeros((2, 5, 7, 2), f32))
        assert out.dtype == np.uint8 and np.array_equal(out, img) and valid.all()
        outf, _ = warp_reference(img, np.zeros((2, 5, 7, 2), f32), out_dtype=f32)
        assert outf.dtype == f32 and np.array_equal(outf, img.astype(f32))


def test_reference_integer_shift():
    """u = 2, v = -1: out(x, y) = img(x + 2, y - 1); the last two columns and the first row leave the frame and read
    the replicated border."""
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (1, 6, 9), dtype=np.uint8)
    flow = np.zeros((1, 6, 9, 2), f32)
    flow[..., 0], flow[..., 1] = 2, -1
    out, valid = warp_reference(img, flow)
    assert np.array_equal(out[0, 1:, :7], img[0, :5, 2:])
    assert valid[0, 1:, :7].all() and not valid[0, 0].any() and not valid[0, :, 7:].any()
    assert np.array_equal(out[0, 1:, 7:], np.repeat(img[0, :5, 8:], 2, axis=1))  # border column replicated
    assert np.array_equal(out[0, 0, :7], img[0, 0, 2:])                           # border row replicated
    # scale -0.5 of (-4, 2) is the same displacement
    out2, valid2 = warp_reference(img, flow * f32(-2), scale=-0.5)
    assert np.array_equal(out2, out) and np.array_equal(valid2, valid)


def test_reference_half_pixel_rounds_half_to_even():
    """Columns alternate 0 / 1 (mean 0.5 -> 0), then 1 / 2 (1.5 -> 2), then 2 / 3 (2.5 -> 2): np.rint's half-even."""
    img = np.array([[[0, 1, 2, 3, 2]]], np.uint8)
    flow = np.zeros((1, 1, 5, 2), f32)
    flow[..., 0] = 0.5
    out, valid = warp_reference(img, flow)
    assert out[0, 0].tolist() == [0, 2, 2, 2, 2] and valid[0, 0].tolist() == [1, 1, 1, 1, 0]
    outf, _ = warp_reference(img, flow, out_dtype=f32)
    assert outf[0, 0].tolist() == [0.5, 1.5, 2.5, 2.5, 2.0]


def test_reference_positions_on_the_last_row_and_column_are_valid():
    img = np.arange(12, dtype=np.uint8).reshape(1, 3, 4)
    flow = np.zeros((1, 3, 4, 2), f32)
    flow[0, 0, 0] = (3, 2)        # exactly (W - 1, H - 1)
    flow[0, 1, 1] = (2.25, 0)     # a quarter past the last column
    flow[0, 2, 2, 0] = np.nan
    flow[0, 0, 3, 1] = np.inf
    out, valid = warp_reference(img, flow)
    assert out[0, 0, 0] == 11 and valid[0, 0, 0] == 1
    assert out[0, 1, 1] == 7 and valid[0, 1, 1] == 0
    assert out[0, 2, 2] == 8 and valid[0, 2, 2] == 0   # NaN -> column 0
    assert out[0, 0, 3] == 11 and valid[0, 0, 3] == 0  # +inf -> last row


# Measured with the oracle's flow (pyoracle, op-point 2) and warp_reference on synth_shift_pair(160, 120, (3.3, -1.7)),
# frame 0: mean |a - b| = 3.100 grey levels, mean |a - warp(b)| over the valid pixels = 2.030, ratio 0.655 (97.9 % of
# the pixels valid).  The two frames carry independent noise, which no warp removes: the true flow (3.3, -1.7) at every
# pixel gives 0.596, so the oracle's flow (mean end-point error 1.09 px on this small frame) costs 0.06 above that
# floor.  Other texture seeds (frames 1, 2) give 0.647 and 0.678: a spread of 0.03.  No compensation is 1.0 by
# definition and the flow with the wrong sign gives 1.42.  The bound 0.8 lies five seed spreads above the measured
# value and still well below 1.0.  It is a property of the reference, not of the code under test.
WARP_RATIO_BOUND = 0.8


def test_reference_warp_along_oracle_flow_compensates_motion(oracle):
    import of_dis_amd as od
    w, h = 160, 120
    a, b = od.synth_shift_pair(w, h, (3.3, -1.7))
    flow = oracle.run_u8(a, b, oracle.oppoint(2, w, 1, 1))
    out, valid = warp_reference(b[None, ..., 0], flow[None])
    av = a[..., 0].astype(np.float64)
    m = valid[0] == 1
    before = np.abs(av - b[..., 0]).mean()
    after = np.abs(av - out[0])[m].mean()
    print(f"mean|a-b| {before:.3f}  mean|a-warp(b)| over valid {after:.3f}  ratio {after / before:.4f}  "
          f"valid {m.mean():.4f}")
    assert m.mean() > 0.9
    assert after / before < WARP_RATIO_BOUND


# --------------------------------------------------------------------------------------------- GPU

SHAPES = [(64, 4), (67, 5), (1, 1), (160, 120)]  # vector form; scalar form (odd width); one pixel; several blocks
FIELDS = ["smooth", "random", "exact", "nonfinite"]
SCALES = [1.0, 0.5, -0.25]
N = 3


def make_image(w, h, n, noc):
    rng = np.random.default_rng(7 * w + h + noc)
    return rng.integers(0, 256, (n, h, w) if noc == 1 else (n, h, w, 3), dtype=np.uint8)


def make_flow(kind, w, h, n, scale=1.0):
    rng = np.random.default_rng(1000 * w + 10 * h + n)
    if kind in ("smooth", "nonfinite"):
        flow = _smooth(rng, n, h, w, 3.0)
        if kind == "nonfinite":
            flat = flow.reshape(-1)
            k = max(4, flat.size // 50) if flat.size >= 8 else 2
            pos = rng.choice(flat.size, size=k, replace=False)
            flat[pos] = np.resize(np.array([np.nan, np.inf, -np.inf, 1e30], f32), k)
        return flow
    if kind == "random":  # up to +-2W: most pixels leave the frame
        return rng.uniform(-2.0 * w, 2.0 * w, (n, h, w, 2)).astype(f32)
    assert kind == "exact"
    # positions on the half-pixel lattice from -1 to W (H), exactly W - 1 and H - 1 among them: the flow that lands
    # there under `scale` is a small dyadic number, exact in float32 (and in binary16 up to the sizes used here)
    tx = rng.integers(-2, 2 * w + 1, (n, h, w)) * 0.5
    ty = rng.integers(-2, 2 * h + 1, (n, h, w)) * 0.5
    tx[:, 0, 0], ty[:, 0, 0] = w - 1, h - 1
    tx[:, -1, -1], ty[:, -1, -1] = w - 1, h - 1
    tx[:, h // 2, w // 2], ty[:, h // 2, w // 2] = w - 1, 0
    flow = np.stack([(tx - np.arange(w)[None, None, :]) / scale, (ty - np.arange(h)[None, :, None]) / scale], -1)
    assert np.array_equal(flow.astype(f32).astype(np.float64), flow)
    return flow.astype(f32)


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


def assert_picture(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    view = np.uint32 if want.dtype == f32 else np.uint8
    bad = got.view(view) != want.view(view)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def flow_tensor(flow, dtype, layout):
    """The field as ctx.run would have written it in that format (and the float32 values the kernel then sees)."""
    import torch
    with np.errstate(over="ignore"):
        f = flow.astype(np.float16) if dtype == "float16" else flow
    seen = f.astype(f32)
    if layout == "nchw":
        f = np.ascontiguousarray(f.transpose(0, 3, 1, 2))
    return torch.from_numpy(f).cuda(), seen


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("w,h", SHAPES)
def test_gpu_warp(ctx, w, h, noc, kind):
    import torch
    img = make_image(w, h, N, noc)
    timg = torch.from_numpy(img).cuda()
    for scale in SCALES:
        flow = make_flow(kind, w, h, N, scale)
        for dtype in ("float32", "float16"):
            seen = flow_tensor(flow, dtype, "nhwc")[1]
            refs = {np_out: warp_reference(img, seen, scale, np_out) for np_out in (np.uint8, f32)}  # once per field
            for layout in ("nhwc", "nchw"):
                tf = flow_tensor(flow, dtype, layout)[0]
                for out_dtype, np_out in ((torch.uint8, np.uint8), (torch.float32, f32)):
                    want, want_valid = refs[np_out]
                    what = f"{kind} {w}x{h}x{N} noc {noc} scale {scale} {dtype} {layout} -> {np_out.__name__}"
                    got, valid = ctx.warp(timg, tf, scale, out_dtype, layout, want_valid=True)
                    alone = ctx.warp(timg, tf, scale, out_dtype, layout)
                    torch.cuda.synchronize()
                    assert_picture(got.cpu().numpy(), want, what)
                    assert_picture(valid.cpu().numpy(), want_valid, what + " (valid)")
                    assert_picture(alone.cpu().numpy(), want, what + " (no mask)")
    if kind == "random" and w > 1:
        assert want_valid.mean() < 0.5  # most pixels leave the frame


GUARD = 64


@pytest.mark.gpu
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("off", [(1, 0, 0), (0, 1, 0), (0, 0, 1)], ids=["flow", "out", "valid"])
@pytest.mark.parametrize("f32out", [0, 1])
def test_gpu_warp_unaligned(ctx, off, noc, f32out):
    """A width that is a multiple of 4 with one pointer an element off its alignment: the one-pixel-per-thread form.
    Every output sits between sentinels, which must survive."""
    import torch
    import of_dis_amd as od
    w, h = 64, 4
    img = make_image(w, h, N, noc)
    flow = make_flow("smooth", w, h, N)
    want, want_valid = warp_reference(img, flow, 1.0, f32 if f32out else np.uint8)
    flow_off, out_off, valid_off = off
    timg = torch.from_numpy(img).cuda()
    tf = torch.zeros(flow.size + flow_off, dtype=torch.float32, device="cuda")
    tf[flow_off:] = torch.from_numpy(flow.reshape(-1)).cuda()
    esz = 4 if f32out else 1
    tout = torch.full((want.size * esz + 2 * GUARD + 4,), 0xAB, dtype=torch.uint8, device="cuda")
    tval = torch.full((want_valid.size + 2 * GUARD + 4,), 0xAB, dtype=torch.uint8, device="cuda")
    # (torch allocations are 256-byte aligned; the offsets are whole elements of the output type)
    lo_out, lo_val = GUARD + out_off * esz, GUARD + valid_off
    view = od.FlowView(0, 0, 0, w, h, 1, 0, 0)
    ctx.warp_ptr(timg.data_ptr(), tf.data_ptr() + 4 * flow_off, view, N, w, h, noc, 1.0, f32out,
                 tout.data_ptr() + lo_out, tval.data_ptr() + lo_val, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o, v = tout.cpu().numpy(), tval.cpu().numpy()
    nb = want.size * esz
    assert np.all(o[:lo_out] == 0xAB) and np.all(o[lo_out + nb:] == 0xAB), "picture guard bytes overwritten"
    assert np.all(v[:lo_val] == 0xAB) and np.all(v[lo_val + want_valid.size:] == 0xAB), "mask guard bytes overwritten"
    assert_picture(o[lo_out:lo_out + nb].copy().view(want.dtype).reshape(want.shape), want, f"unaligned {off}")
    assert_picture(v[lo_val:lo_val + want_valid.size].reshape(want_valid.shape), want_valid, f"unaligned {off} (valid)")


@pytest.mark.gpu
def test_gpu_warp_one_frame_above_the_launch_slice(ctx):
    """launch_warp puts 65535 frames in one launch (grid z): 65536 frames of 8 x 4 take two, 131071 take three with a
    full middle one."""
    import torch
    w, h = 8, 4
    for n in (65536, 131071):
        rng = np.random.default_rng(5)
        img = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
        flow = rng.uniform(-3, 3, (n, h, w, 2)).astype(f32)
        want, want_valid = warp_reference(img, flow)
        got, valid = ctx.warp(torch.from_numpy(img).cuda(), torch.from_numpy(flow).cuda(), want_valid=True)
        torch.cuda.synchronize()
        assert_picture(got.cpu().numpy(), want, f"{n} frames")
        assert_picture(valid.cpu().numpy(), want_valid, f"{n} frames (valid)")
        assert not np.array_equal(want[-1], want[0]) and not np.array_equal(want[65535], want[0])

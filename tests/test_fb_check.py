"""Forward-backward consistency check (ofdis_fb_check, include/ofdis.h).

`fb_reference` below restates the header's definition in vectorised numpy float32 -- every operation on float32
arrays, one rounding each, in the header's order -- and is the reference of every mask and error comparison here and
in test_gpu_bidir.py.

CPU part: the three new symbols, their NULL-context refusal, and known answers of the reference itself.
GPU part (marked gpu): k_fb_check against the reference.  Masks must be equal; errors must have equal uint32 views,
and be +inf where the code is 2.  A NaN error (an in-frame pixel whose gathered taps hold NaN or infinities) is
stored as the canonical quiet NaN by definition: IEEE 754 fixes neither the sign nor the payload of a generated NaN,
and the raw results did differ (0xffc00000 from the kernel against numpy's 0x7fc00000 at 2 of 20 NaN errors of the
64 x 4 x 2 non-finite field).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------- reference

def fb_reference_dir(F, B, alpha=0.01, beta=0.5):
    """One direction: F walks, B is gathered.  F, B float32 [n, h, w, 2] -> (occ u8 [n, h, w], err f32 [n, h, w])."""
    F = np.ascontiguousarray(F, f32)
    B = np.ascontiguousarray(B, f32)
    n, h, w, _ = F.shape
    xs = np.arange(w, dtype=f32)[None, None, :]
    ys = np.arange(h, dtype=f32)[None, :, None]
    u, v = F[..., 0], F[..., 1]
    with np.errstate(all="ignore"):
        px, py = xs + u, ys + v
        inside = (px >= 0) & (px <= f32(w - 1)) & (py >= 0) & (py <= f32(h - 1))  # False for NaN
        pxs, pys = np.where(inside, px, f32(0)), np.where(inside, py, f32(0))
        x0, y0 = np.floor(pxs).astype(np.int64), np.floor(pys).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        ax, ay = pxs - x0.astype(f32), pys - y0.astype(f32)
        fi = np.arange(n)[:, None, None]
        b = []
        for k in (0, 1):
            b00, b01, b10, b11 = B[fi, y0, x0, k], B[fi, y0, x1, k], B[fi, y1, x0, k], B[fi, y1, x1, k]
            top = b00 + ax * (b01 - b00)
            bot = b10 + ax * (b11 - b10)
            b.append(top + ay * (bot - top))
        du, dv = u + b[0], v + b[1]
        err = du * du + dv * dv
        mag = (u * u + v * v) + (b[0] * b[0] + b[1] * b[1])
        thr = f32(alpha) * mag + f32(beta)
        occ = np.where(err <= thr, 0, 1)  # NaN err -> 1
        err = np.where(np.isnan(err), f32(np.nan), err)  # stored as the canonical quiet NaN 0x7fc00000
    assert err.dtype == f32 and thr.dtype == f32
    return np.where(inside, occ, 2).astype(np.uint8), np.where(inside, err, f32(np.inf)).astype(f32)


def fb_reference(fw, bw, alpha=0.01, beta=0.5):
    """(occ_fw, occ_bw, err_fw, err_bw) of two fields [n, h, w, 2]."""
    of, ef = fb_reference_dir(fw, bw, alpha, beta)
    ob, eb = fb_reference_dir(bw, fw, alpha, beta)
    return of, ob, ef, eb


def assert_err_equal(got, want, occ, what=""):
    """uint32 views equal, +inf where the code is 2."""
    bad = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} error values differ, first at {np.argwhere(bad)[0]}"
    assert np.all(np.isposinf(got[occ == 2])), f"{what}: err is not +inf where the code is 2"


# --------------------------------------------------------------------------------------------- CPU

SIGNATURES = {
    "ofdis_fb_check": 13,
    "ofdis_run_bidir_u8": 16,
    "ofdis_run_bidir_u8_host": 15,
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
    decl = re.search(r"\bint ofdis_fb_check\(([^;]*)\);", hdr).group(1)
    assert re.sub(r"\s+", " ", decl) == (
        "ofdis_context *ctx, const float *flow_fw, const float *flow_bw, int n, int width, int height, "
        "float alpha, float beta, uint8_t *occ_fw, uint8_t *occ_bw, float *err_fw, float *err_bw, void *stream")
    decl = re.search(r"\bint ofdis_run_bidir_u8\(([^;]*)\);", hdr).group(1)
    assert re.sub(r"\s+", " ", decl) == (
        "ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height, "
        "const ofdis_params *p, float alpha, float beta, float *flow_fw, float *flow_bw, "
        "uint8_t *occ_fw, uint8_t *occ_bw, float *err_fw, float *err_bw, void *stream")
    assert L.ofdis_abi_version() == 2
    assert {"fb_check", "fb_check_err"} <= set(od.kernel_names())


def test_null_context_is_refused():
    import of_dis_amd as od
    L = od.lib()
    p = od.oppoint(2, 64, od.MODE_OF, 1)
    buf = np.zeros(64 * 64 * 2, f32)
    img = np.zeros(64 * 64, np.uint8)
    d, im = buf.ctypes.data, img.ctypes.data
    assert L.ofdis_fb_check(None, d, d, 1, 64, 64, 0.01, 0.5, im, None, None, None, None) == od._lib.ERR_INVALID_ARGUMENT
    assert L.ofdis_run_bidir_u8(None, im, im, 1, 64, 64, C.byref(p), 0.01, 0.5, d, None, None, None, None, None,
                                None) == od._lib.ERR_INVALID_ARGUMENT
    assert L.ofdis_run_bidir_u8_host(None, im, im, 1, 64, 64, C.byref(p), 0.01, 0.5, d, None, None, None, None,
                                     None) == od._lib.ERR_INVALID_ARGUMENT


def test_byte_model():
    import of_dis_amd as od
    p = od.oppoint(2, 1920, od.MODE_OF, 1)
    assert od.algorithmic_bytes(p, 1920, 1080, "fb_check") == 2 * 1920 * 1080 * 17
    assert od.algorithmic_bytes(p, 1920, 1080, "fb_check_err") == 2 * 1920 * 1080 * 21


def test_reference_zero_flows():
    z = np.zeros((2, 5, 7, 2), f32)
    of, ob, ef, eb = fb_reference(z, z)
    assert not of.any() and not ob.any() and not ef.any() and not eb.any()


def test_reference_opposite_constant():
    """u = 2.5 against b = -2.5: consistent wherever x + 2.5 stays inside, code 2 in the last columns."""
    fw = np.zeros((1, 4, 10, 2), f32)
    fw[..., 0] = 2.5
    of, ob, ef, eb = fb_reference(fw, -fw)
    assert not of[..., :7].any() and not ef[..., :7].any()      # x + 2.5 <= 9  <=>  x <= 6
    assert np.all(of[..., 7:] == 2) and np.all(np.isposinf(ef[..., 7:]))
    assert not ob[..., 3:].any() and np.all(ob[..., :3] == 2)   # x - 2.5 >= 0  <=>  x >= 3


def test_reference_unit_error():
    """u = 1 against b = 0: err = 1 > 0.01 * 1 + 0.5, code 1 (2 in the last column)."""
    fw = np.zeros((1, 3, 6, 2), f32)
    fw[..., 0] = 1
    of, ob, ef, eb = fb_reference(fw, np.zeros_like(fw))
    assert np.all(of[..., :5] == 1) and np.all(ef[..., :5] == 1) and np.all(of[..., 5] == 2)
    assert np.all(ob == 1) and np.all(eb == 1)  # the backward field stays put and reads u = 1 there


def test_reference_nan():
    fw = np.zeros((1, 3, 4, 2), f32)
    fw[0, 1, 2, 0] = np.nan
    fw[0, 0, 0, 1] = np.inf
    fw[0, 2, 3, 1] = -np.inf
    of, ob, ef, eb = fb_reference(fw, np.zeros_like(fw))
    assert of[0, 1, 2] == 2 and of[0, 0, 0] == 2 and of[0, 2, 3] == 2
    assert np.isposinf(ef[0, 1, 2])
    assert (of == 2).sum() == 3
    assert ob[0, 1, 2] == 1 and np.isnan(eb[0, 1, 2])  # an in-frame pixel that gathers the NaN: inconsistent
    assert np.all(eb.view(np.uint32)[np.isnan(eb)] == 0x7FC00000)  # the canonical quiet NaN


def test_reference_threshold_is_inclusive():
    """u = (1, 1), b = 0, alpha = 0.75, beta = 0.5: err = 2 = 0.75 * 2 + 0.5 exactly -> consistent."""
    fw = np.ones((1, 4, 4, 2), f32)
    of, _, ef, _ = fb_reference(fw, np.zeros_like(fw), 0.75, 0.5)
    assert np.all(of[0, :3, :3] == 0) and np.all(ef[0, :3, :3] == 2)


# --------------------------------------------------------------------------------------------- GPU

SHAPES = [(1, 1, 1), (3, 2, 1), (4, 1, 2), (7, 5, 3), (64, 4, 2), (130, 3, 1), (256, 2, 2)]
FIELDS = ["zero", "opposite", "same", "smooth", "large", "nonfinite", "threshold"]


def _smooth(rng, n, h, w, sigma):
    """A band-limited field: normal values on an 8-pixel grid, bilinearly interpolated."""
    gh, gw = h // 8 + 2, w // 8 + 2
    g = rng.standard_normal((n, gh, gw, 2)) * sigma
    yy, xx = np.arange(h) / 8.0, np.arange(w) / 8.0
    y0, x0 = yy.astype(int), xx.astype(int)
    fy, fx = (yy - y0)[None, :, None, None], (xx - x0)[None, None, :, None]
    top = g[:, y0][:, :, x0] * (1 - fx) + g[:, y0][:, :, x0 + 1] * fx
    bot = g[:, y0 + 1][:, :, x0] * (1 - fx) + g[:, y0 + 1][:, :, x0 + 1] * fx
    return (top * (1 - fy) + bot * fy).astype(f32)


def make_field(kind, w, h, n):
    """-> (flow_fw, flow_bw, alpha, beta)"""
    rng = np.random.default_rng(1000 * w + 10 * h + n)
    fw = np.zeros((n, h, w, 2), f32)
    alpha, beta = 0.01, 0.5
    if kind == "zero":
        bw = fw.copy()
    elif kind == "opposite":
        fw[..., 0], fw[..., 1] = 2.5, -1.25
        bw = -fw
    elif kind == "same":
        fw[..., 0], fw[..., 1] = 1.5, 0.75
        bw = fw.copy()
    elif kind in ("smooth", "nonfinite"):
        fw = _smooth(rng, n, h, w, 3.0)
        bw = (-fw + rng.standard_normal(fw.shape).astype(f32) * f32(0.4)).astype(f32)  # some pass, some fail
        if kind == "nonfinite":
            for fld in (fw, bw):
                flat = fld.reshape(-1)
                k = max(3, flat.size // 100) if flat.size >= 6 else 1
                pos = rng.choice(flat.size, size=k, replace=False)
                flat[pos] = np.resize(np.array([np.nan, np.inf, -np.inf], f32), k)
    elif kind == "large":
        fw = (rng.standard_normal(fw.shape) * 40).astype(f32)
        bw = (rng.standard_normal(fw.shape) * 40).astype(f32)
    elif kind == "threshold":
        # err = 2 = alpha * 2 + beta exactly where u = (1, 1); u = 1 + 2^-20 tips it over (err = 2 + 2^-19 against
        # thr = 2 + 0.75 * 2^-19, all exact in float32)
        alpha, beta = 0.75, 0.5
        fw[...] = 1
        up = rng.random((n, h, w)) < 0.5
        fw[..., 0][up] = f32(1 + 2.0 ** -20)
        bw = np.zeros_like(fw)
    return fw, bw, alpha, beta


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


GUARD = 64  # bytes of sentinel on both sides of every output


def gpu_fb_check(ctx, fw, bw, alpha, beta, outs=(1, 1, 1, 1), flow_off=0, occ_off=0):
    """ofdis_fb_check through raw pointers.  outs: which of (occ_fw, occ_bw, err_fw, err_bw) are passed;
    flow_off floats / occ_off bytes shift the flow / mask buffers off their natural alignment.  Every output sits
    between sentinels, which must survive.  -> the four outputs as numpy arrays (None where not passed)."""
    import torch
    n, h, w, _ = fw.shape
    px = n * h * w
    dev = []
    for fld in (fw, bw):
        t = torch.zeros(fld.size + flow_off, dtype=torch.float32, device="cuda")
        t[flow_off:] = torch.from_numpy(fld.reshape(-1)).cuda()
        dev.append(t)
    bufs, ptrs = [], []
    for k in range(4):
        if not outs[k]:
            bufs.append(None)
            ptrs.append(0)
            continue
        if k < 2:
            t = torch.full((px + 2 * GUARD + occ_off,), 0xAB, dtype=torch.uint8, device="cuda")
            ptrs.append(t.data_ptr() + GUARD + occ_off)
        else:
            t = torch.full((px + 2 * GUARD // 4,), -123.0, dtype=torch.float32, device="cuda")
            ptrs.append(t.data_ptr() + GUARD)
        bufs.append(t)
    ctx.fb_check_ptr(dev[0].data_ptr() + 4 * flow_off, dev[1].data_ptr() + 4 * flow_off, n, w, h, alpha, beta,
                     ptrs[0], ptrs[1], ptrs[2], ptrs[3], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = []
    for k in range(4):
        if bufs[k] is None:
            res.append(None)
            continue
        a = bufs[k].cpu().numpy()
        if k < 2:
            lo = GUARD + occ_off
            assert np.all(a[:lo] == 0xAB) and np.all(a[lo + px:] == 0xAB), "mask guard bytes overwritten"
            res.append(a[lo:lo + px].reshape(n, h, w))
        else:
            lo = GUARD // 4
            assert np.all(a[:lo] == -123.0) and np.all(a[lo + px:] == -123.0), "error guard floats overwritten"
            res.append(a[lo:lo + px].reshape(n, h, w))
    return res


def compare(got, want, what):
    occ = {0: want[0], 1: want[1], 2: want[0], 3: want[1]}
    for k in range(4):
        if got[k] is None:
            continue
        if k < 2:
            bad = got[k] != want[k]
            assert not bad.any(), f"{what}: mask {k}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0]}"
        else:
            assert_err_equal(got[k], want[k], occ[k], f"{what}: err {k - 2}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("w,h,n", SHAPES)
def test_gpu_fb_check(ctx, w, h, n, kind):
    fw, bw, alpha, beta = make_field(kind, w, h, n)
    want = fb_reference(fw, bw, alpha, beta)
    compare(gpu_fb_check(ctx, fw, bw, alpha, beta), want, f"{kind} {w}x{h}x{n}")
    if kind == "threshold" and w > 2 and h > 1:  # the on-threshold pixels pass, those just above it do not
        inside = want[0][:, :h - 1, :w - 2]
        on = fw[:, :h - 1, :w - 2, 0] == 1
        assert np.all(inside[on] == 0) and np.all(inside[~on] == 1)


@pytest.mark.gpu
@pytest.mark.parametrize("flow_off,occ_off", [(1, 0), (0, 1)])
def test_gpu_fb_check_unaligned(ctx, flow_off, occ_off):
    """A width that is a multiple of 4 with a pointer off its alignment: the one-pixel-per-thread form."""
    fw, bw, alpha, beta = make_field("smooth", 64, 4, 2)
    want = fb_reference(fw, bw, alpha, beta)
    compare(gpu_fb_check(ctx, fw, bw, alpha, beta, flow_off=flow_off, occ_off=occ_off), want, "unaligned")


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("w,h,n", [(64, 4, 2), (7, 5, 3)])
def test_gpu_fb_check_single_output(ctx, w, h, n, which):
    fw, bw, alpha, beta = make_field("smooth", w, h, n)
    want = fb_reference(fw, bw, alpha, beta)
    outs = tuple(int(k == which) for k in range(4))
    got = gpu_fb_check(ctx, fw, bw, alpha, beta, outs=outs)
    assert got[which] is not None
    compare(got, want, f"output {which} alone")


@pytest.mark.gpu
def test_gpu_fb_check_tensor_api(ctx):
    import torch
    fw, bw, alpha, beta = make_field("nonfinite", 130, 3, 1)
    want = fb_reference(fw, bw, 0.02, 0.25)
    got = ctx.fb_check(torch.from_numpy(fw).cuda(), torch.from_numpy(bw).cuda(), 0.02, 0.25, want_err=True)
    torch.cuda.synchronize()
    compare([t.cpu().numpy() for t in got], want, "tensor api")
    occ = ctx.fb_check(torch.from_numpy(fw[0]).cuda(), torch.from_numpy(bw[0]).cuda(), 0.02, 0.25)
    assert len(occ) == 2 and occ[0].shape == (3, 130)
    assert np.array_equal(occ[0].cpu().numpy(), want[0][0]) and np.array_equal(occ[1].cpu().numpy(), want[1][0])


@pytest.mark.gpu
def test_gpu_fb_check_arguments(ctx):
    import torch
    import of_dis_amd as od
    L = od.lib()
    t = torch.zeros(2 * 8 * 8 * 2, dtype=torch.float32, device="cuda")
    o = torch.full((8 * 8,), 7, dtype=torch.uint8, device="cuda")
    d, m, h = t.data_ptr(), o.data_ptr(), ctx._h
    INV = od._lib.ERR_INVALID_ARGUMENT
    assert L.ofdis_fb_check(h, d, d, 1, 8, 8, 0.01, 0.5, None, None, None, None, None) == od._lib.OK  # nothing to do
    assert L.ofdis_fb_check(h, d, d, 1, 8, 8, -1.0, 0.5, m, None, None, None, None) == INV
    assert L.ofdis_fb_check(h, d, d, 1, 8, 8, 0.01, float("nan"), m, None, None, None, None) == INV
    assert L.ofdis_fb_check(h, d, d, 1, 8, 8, float("inf"), 0.5, m, None, None, None, None) == INV
    assert L.ofdis_fb_check(h, None, d, 1, 8, 8, 0.01, 0.5, m, None, None, None, None) == INV
    assert L.ofdis_fb_check(h, d, None, 1, 8, 8, 0.01, 0.5, m, None, None, None, None) == INV
    assert L.ofdis_fb_check(h, d, d, 0, 8, 8, 0.01, 0.5, m, None, None, None, None) == INV
    assert L.ofdis_fb_check(h, d, d, 1, 0, 8, 0.01, 0.5, m, None, None, None, None) == INV
    assert L.ofdis_fb_check(h, d, d, 1, 8, -1, 0.01, 0.5, m, None, None, None, None) == INV
    torch.cuda.synchronize()
    assert torch.all(o == 7)  # nothing was enqueued by the refused calls
    assert L.ofdis_fb_check(h, d, d, 1, 8, 8, 0.0, 0.0, m, None, None, None, None) == od._lib.OK  # zero is allowed
    torch.cuda.synchronize()
    assert torch.all(o == 0)

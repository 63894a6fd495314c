"""The moving-object mask (include/ofdis.h: ofdis_motion_mask) restated in numpy, its known answers, the header and
bindings, the host-side refusals on their own, and the definition's behaviour on the CPU oracle's flows.

motion_mask_reference is the statement the GPU tests compare the kernels with bit for bit (tests/test_gpu_motion_mask.py);
motion_mask_scalar walks the same definition pixel by pixel, and the two agree bit for bit.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_fb_check import fb_reference_dir
from test_interp import _texture
from test_stabilize import field_of, fit_motion_reference, similarity_matrix

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSTATS = 12
QNAN = np.array([0x7FC00000], np.uint32).view(f32)[0]  # the canonical quiet NaN `res` holds for a NaN


# --------------------------------------------------------------------------------------------- the restatement

def _window_sum(a, radius):
    """Per pixel the sum of integer plane a [h, w] over the (2 radius + 1)^2 window clipped to the frame."""
    h, w = a.shape
    p = np.zeros((h + 2 * radius, w + 2 * radius), np.int64)
    p[radius:radius + h, radius:radius + w] = a
    s = np.zeros((h, w), np.int64)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            s += p[dy:dy + h, dx:dx + w]
    return s


def stats_of(code, b):
    """The twelve integers of one pair from its codes and raw classes."""
    h, w = code.shape
    s = np.zeros(NSTATS, np.int64)
    s[0], s[1], s[2] = (code == 0).sum(), (code == 1).sum(), (code == 2).sum()
    ys, xs = np.nonzero(code == 1)
    s[3:7] = (xs.min(), ys.min(), xs.max(), ys.max()) if xs.size else (w, h, -1, -1)
    s[7] = b.sum()
    s[8], s[9] = xs.astype(np.int64).sum(), ys.astype(np.int64).sum()
    return s


def motion_mask_reference(flow, xform, occ=None, thr=1.0, rel=0.05, radius=1):
    """flow [m, h, w, 2] (converted to float32 exactly), xform float64 [m, 6], occ u8 [m, h, w] or None ->
    (code u8 [m, h, w], res float32 [m, h, w], stats int64 [m, 12])."""
    F = np.ascontiguousarray(flow).astype(f32)
    m, h, w, _ = F.shape
    M = np.asarray(xform, f64).reshape(m, 6)
    thr, rel = f32(thr), f32(rel)
    y, x = np.mgrid[0:h, 0:w].astype(f64)
    code, res, stats = np.empty((m, h, w), np.uint8), np.empty((m, h, w), f32), np.empty((m, NSTATS), np.int64)
    with np.errstate(all="ignore"):
        for j in range(m):
            u, v = F[j, ..., 0], F[j, ..., 1]
            pu = (((M[j, 0] * x + M[j, 1] * y) + M[j, 2]) - x).astype(f32)  # the bracket in float64
            pv = (((M[j, 3] * x + M[j, 4] * y) + M[j, 5]) - y).astype(f32)
            du, dv = u - pu, v - pv
            e, g = np.sqrt(du * du + dv * dv), np.sqrt(pu * pu + pv * pv)
            assert e.dtype == f32 and g.dtype == f32
            fin = np.isfinite(u) & np.isfinite(v)
            e = np.where(fin, e, f32(np.inf))  # a select after the test
            unknown = ~fin if occ is None else (~fin | (occ[j] != 0))
            b = ~unknown & (e > thr) & (e > rel * g)  # (false for a NaN e)
            mov, known = _window_sum(b, radius), _window_sum(~unknown, radius)
            c = 2 * mov > known
            code[j] = np.where(unknown, 2, np.where(c, 1, 0))
            res[j] = np.where(np.isnan(e), QNAN, e)
            stats[j] = stats_of(code[j], b)
    return code, res, stats


def motion_mask_scalar(flow, xform, occ=None, thr=1.0, rel=0.05, radius=1):
    """The same definition pixel by pixel, every float32 operation spelled out on numpy scalars."""
    F = np.ascontiguousarray(flow).astype(f32)
    m, h, w, _ = F.shape
    M = np.asarray(xform, f64).reshape(m, 6)
    thr, rel = f32(thr), f32(rel)
    code, res, stats = np.empty((m, h, w), np.uint8), np.empty((m, h, w), f32), np.empty((m, NSTATS), np.int64)
    with np.errstate(all="ignore"):
        for j in range(m):
            b, unknown = np.zeros((h, w), bool), np.zeros((h, w), bool)
            for y in range(h):
                for x in range(w):
                    u, v = F[j, y, x, 0], F[j, y, x, 1]
                    pu = f32(((M[j, 0] * f64(x) + M[j, 1] * f64(y)) + M[j, 2]) - f64(x))
                    pv = f32(((M[j, 3] * f64(x) + M[j, 4] * f64(y)) + M[j, 5]) - f64(y))
                    du, dv = f32(u - pu), f32(v - pv)
                    e = np.sqrt(f32(f32(du * du) + f32(dv * dv)))
                    g = np.sqrt(f32(f32(pu * pu) + f32(pv * pv)))
                    fin = bool(np.isfinite(u) and np.isfinite(v))
                    e = e if fin else f32(np.inf)
                    unknown[y, x] = (not fin) or (occ is not None and occ[j, y, x] != 0)
                    b[y, x] = (not unknown[y, x]) and bool(e > thr) and bool(e > f32(rel * g))
                    res[j, y, x] = QNAN if np.isnan(e) else e
            for y in range(h):
                for x in range(w):
                    mov = known = 0
                    for yy in range(max(y - radius, 0), min(y + radius, h - 1) + 1):
                        for xx in range(max(x - radius, 0), min(x + radius, w - 1) + 1):
                            mov += int(b[yy, xx])
                            known += int(not unknown[yy, xx])
                    code[j, y, x] = 2 if unknown[y, x] else (1 if 2 * mov > known else 0)
            stats[j] = stats_of(code[j], b)
    return code, res, stats


def same_mask(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: code"
    assert np.array_equal(np.ascontiguousarray(got[1]).view(np.uint32), np.ascontiguousarray(want[1]).view(np.uint32)), f"{what}: res"
    assert np.array_equal(got[2], want[2]), f"{what}: stats"


# --------------------------------------------------------------------------------------------- known answers

W, H = 64, 48
M0 = similarity_matrix(1.01, 0.01, 3.0, -2.0, W, H)


def boxed_field(x0, y0, x1, y1, w=W, h=H, M=M0):
    """The field of M with the box [x0, x1] x [y0, y1] displaced by (10, -6)."""
    F = field_of(M, w, h)
    F[y0:y1 + 1, x0:x1 + 1] += f32([10, -6])
    return F[None]


def test_similarity_field_under_its_own_transform_is_static():
    """pu is the float32 rounding of the float64 bracket; field_of rounds M00 x + M01 y + M02 summed in another order,
    then subtracts x -- so u and pu are two float32 roundings of float64 values that differ by a few float64 ulps of a
    position (at most 2^-44 here): each is within half a float32 ulp of the true flow, u - pu is exact (Sterbenz) or
    rounds once, and the squares, their sum and the root add at most 1.5 ulp of the result.  |du|, |dv| <= 1 ulp(f) with
    f the larger flow component, so e <= sqrt(2) (1 + 2^-22) ulp(f) < 2 ulp(f)."""
    F = field_of(M0, W, H)[None]
    code, res, stats = motion_mask_reference(F, M0[None], None, 1.0, 0.05, 1)
    assert not code.any()
    bound = 2 * np.spacing(np.abs(F).max(axis=-1))
    assert (res <= bound).all(), float((res / np.spacing(np.abs(F).max(axis=-1))).max())
    assert list(stats[0]) == [W * H, 0, 0, W, H, -1, -1, 0, 0, 0, 0, 0]


def test_displaced_box_is_the_mask_at_radius_zero():
    x0, y0, x1, y1 = 17, 9, 41, 30
    F = boxed_field(x0, y0, x1, y1)
    code, res, stats = motion_mask_reference(F, M0[None], None, 1.0, 0.05, 0)
    want = np.zeros((H, W), np.uint8)
    want[y0:y1 + 1, x0:x1 + 1] = 1
    assert np.array_equal(code[0], want)
    n = (x1 - x0 + 1) * (y1 - y0 + 1)
    assert list(stats[0]) == [W * H - n, n, 0, x0, y0, x1, y1, n, (x0 + x1) * n // 2, (y0 + y1) * n // 2, 0, 0]
    inside = res[0][want == 1]
    assert np.abs(inside - f32(np.sqrt(f32(136)))).max() < 1e-4  # |(10, -6)|


def test_median_removes_a_speck_and_fills_a_hole():
    F = boxed_field(20, 10, 40, 30)
    F[0, 5, 5] += f32([10, -6])           # an isolated moving pixel
    F[0, 20, 30] = field_of(M0, W, H)[20, 30]  # a single hole in the box
    raw = motion_mask_reference(F, M0[None], None, 1.0, 0.05, 0)[0][0]
    assert raw[5, 5] == 1 and raw[20, 30] == 0
    code, _, stats = motion_mask_reference(F, M0[None], None, 1.0, 0.05, 1)
    assert code[0, 5, 5] == 0 and code[0, 20, 30] == 1
    assert stats[0, 7] == raw.sum() == 21 * 21  # the raw count: the box less the hole plus the speck
    # the box's corners have 4 moving pixels of 9: the median rounds them off
    assert code[0, 10, 20] == 0 and code[0, 10, 21] == 1 and code[0].sum() == 21 * 21 - 4


def test_window_is_clipped_at_a_frame_corner():
    base = field_of(M0, W, H)
    for moving, want in ((((0, 0), (0, 1), (1, 0)), 1), (((0, 1), (1, 0)), 0)):
        F = base.copy()
        for (y, x) in moving:
            F[y, x] += f32([10, -6])
        code = motion_mask_reference(F[None], M0[None], None, 1.0, 0.05, 1)[0][0]
        assert code[0, 0] == want, (moving, code[:3, :3])  # 4 pixels in the window: 3 of 4 -> 1, 2 of 4 -> 0


def test_unknown_pixels_are_left_out_of_known():
    F = field_of(M0, W, H)[None].copy()
    occ = np.zeros((1, H, W), np.uint8)
    occ[0, 19:22, 29:32] = 1  # a 3 x 3 block of unknowns
    occ[0, 40, 10] = 2
    code = motion_mask_reference(F, M0[None], occ, 1.0, 0.05, 1)[0][0]
    assert (code[19:22, 29:32] == 2).all() and code[40, 10] == 2 and (code == 2).sum() == 10
    assert code[20, 30] == 2 and not (code[17:24, 27:34] == 1).any()  # a window of unknowns alone: 2 at the centre, c = 0 around
    # one moving pixel beside eight unknowns: mov 1 of known 1 -> moving
    F[0, 19, 29] += f32([10, -6])
    occ[0, 19, 29] = 0
    occ[0, 18:21, 28:31] = np.where(np.arange(9).reshape(3, 3) == 4, 0, 1)
    code = motion_mask_reference(F, M0[None], occ, 1.0, 0.05, 1)[0][0]
    assert code[19, 29] == 1
    # without the unknowns the same pixel is a speck the median removes
    assert motion_mask_reference(F, M0[None], None, 1.0, 0.05, 1)[0][0, 19, 29] == 0


def test_nonfinite_flow_is_unknown_and_nonfinite_transform_is_static():
    F = field_of(M0, W, H)[None].copy()
    F[0, 3, 4, 0] = np.nan
    F[0, 7, 8, 1] = np.inf
    F[0, 9, 9] = (-np.inf, np.nan)
    code, res, stats = motion_mask_reference(F, M0[None], None, 1.0, 0.05, 1)
    for (y, x) in ((3, 4), (7, 8), (9, 9)):
        assert code[0, y, x] == 2 and res[0, y, x] == np.inf
    assert stats[0, 2] == 3 and stats[0, 1] == 0
    Mn = M0.copy()
    Mn[2] = np.nan
    code, res, stats = motion_mask_reference(field_of(M0, W, H)[None], Mn[None], None, 1.0, 0.05, 1)
    assert not code.any() and (res.view(np.uint32) == 0x7FC00000).all() and stats[0, 7] == 0
    # a NaN transform leaves a non-finite estimate unknown, with res +inf
    code, res, _ = motion_mask_reference(F, Mn[None], None, 1.0, 0.05, 1)
    assert code[0, 3, 4] == 2 and res[0, 3, 4] == np.inf and code[0, 0, 0] == 0


def test_rel_keeps_a_small_residual_of_a_fast_pan_static():
    Mp = np.array([1.0, 0.0, 60.0, 0.0, 1.0, 0.0])  # a pan of 60 px: rel * g = 3
    F = field_of(Mp, W, H)[None].copy()
    F[0, 10:20, 10:20, 0] += f32(2.0)   # residual 2: above thr = 1, below 0.05 * 60
    F[0, 30:40, 30:40, 0] += f32(4.0)   # residual 4: above both
    code = motion_mask_reference(F, Mp[None], None, 1.0, 0.05, 0)[0][0]
    assert not code[10:20, 10:20].any() and code[30:40, 30:40].all() and code.sum() == 100
    assert motion_mask_reference(F, Mp[None], None, 1.0, 0.0, 0)[0][0].sum() == 200  # rel 0: the threshold alone


def _specked(w, h, seed):
    rng = np.random.default_rng(seed)
    M = similarity_matrix(0.99, -0.02, -1.5, 2.25, w, h)
    F = field_of(M, w, h)
    F[2:h // 2, 1:w // 2] += f32([3.0, 1.5])
    F += rng.normal(0, 0.6, F.shape).astype(f32)
    F[rng.integers(0, h, 6), rng.integers(0, w, 6), rng.integers(0, 2, 6)] = [np.nan, np.inf, -np.inf, np.nan, 1e30, -1e38]
    occ = (rng.random((h, w)) < 0.15).astype(np.uint8) * rng.integers(1, 3, (h, w)).astype(np.uint8)
    return F[None], M[None], occ[None]


@pytest.mark.parametrize("radius", [0, 1, 2, 4])
def test_scalar_twin_agrees_bit_for_bit(radius):
    F, M, occ = _specked(23, 17, radius)
    for o in (None, occ):
        a = motion_mask_reference(F, M, o, 0.75, 0.05, radius)
        b = motion_mask_scalar(F, M, o, 0.75, 0.05, radius)
        same_mask(a, b, f"radius {radius} occ {o is not None}")
        assert (a[0] == 1).any() and (a[0] == 0).any() and (a[0] == 2).any()
    with np.errstate(over="ignore"):
        F16 = F.astype(np.float16)  # (1e30 becomes +inf)
    same_mask(motion_mask_reference(F16, M, occ, 0.75, 0.05, radius),
              motion_mask_reference(F16.astype(f32), M, occ, 0.75, 0.05, radius), "binary16 is converted exactly")


# --------------------------------------------------------------------------------------------- header and bindings

SIGNATURES = {
    "ofdis_motion_mask": 15,
    "ofdis_run_sequence_motion_mask_u8": 23,
    "ofdis_run_sequence_motion_mask_u8_host": 22,
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
    decl = re.search(r"\bint ofdis_motion_mask\(([^;]*)\);", hdr).group(1)
    assert re.sub(r"\s+", " ", decl) == (
        "ofdis_context *ctx, const void *flow, const ofdis_flow_view *view, int m, int width, int height, "
        "const double *xform, const uint8_t *occ, float thr, float rel, int radius, uint8_t *code, float *res, "
        "int64_t *stats, void *stream")
    decl = re.search(r"\bint ofdis_run_sequence_motion_mask_u8\(([^;]*)\);", hdr).group(1)
    assert re.sub(r"\s+", " ", decl) == (
        "ofdis_context *ctx, const uint8_t *frames, int nframes, int width, int height, const ofdis_params *p, int model, "
        "int step, double tau, int iters, int use_fb, float alpha, float beta, float thr, float rel, int radius, "
        "uint8_t *code, float *res, int64_t *stats, double *xform, int32_t *support, uint8_t *occ, void *stream")
    assert re.search(r"#define OFDIS_MM_NSTATS 12\b", hdr) and od.MM_NSTATS == NSTATS
    # the section sits after the stabilisation calls and before the flow error
    assert hdr.index("global motion and video stabilisation") < hdr.index("moving-object masks") < hdr.index("flow error against ground truth")
    names = od.kernel_names_all()
    assert names[:35] == od.kernel_names() and names[35:38] == od.kernel_names_ext()
    assert names.index("motion_mask") == 38 and names.index("motion_mask_level") == 39
    for name in ("motion_mask", "motion_mask_ptr", "run_sequence_motion_mask", "run_sequence_motion_mask_ptr",
                 "run_sequence_motion_mask_host"):
        assert callable(getattr(od.Context, name))
    assert callable(od.motion_summary)


def test_null_context_is_refused():
    import of_dis_amd as od
    L = od.lib()
    p = od.oppoint(2, 64, od.MODE_OF, 1)
    buf = np.zeros(3 * 64 * 64 * 2, f32)
    d = buf.ctypes.data
    v = od.FlowView(0, 0, 0, 64, 64, 1, 0, 0)
    INV = od._lib.ERR_INVALID_ARGUMENT
    assert L.ofdis_motion_mask(None, d, C.byref(v), 1, 64, 64, d, None, 1.0, 0.05, 1, d, None, None, None) == INV
    assert L.ofdis_run_sequence_motion_mask_u8(None, d, 2, 64, 64, C.byref(p), 1, 16, 2.0, 4, 0, 0.01, 0.5, 1.0, 0.05, 1, d,
                                               None, None, None, None, None, None) == INV
    assert L.ofdis_run_sequence_motion_mask_u8_host(None, d, 2, 64, 64, C.byref(p), 1, 16, 2.0, 4, 0, 0.01, 0.5, 1.0, 0.05,
                                                    1, d, None, None, None, None, None) == INV
    assert L.ofdis_context_kernel_time(None, b"motion_mask", None, None) == INV


def test_byte_model():
    import of_dis_amd as od
    px = 1920 * 1080
    for noc in (1, 3):
        p = od.oppoint(2, 1920, od.MODE_OF, noc)
        g = od.out_geometry(p, 1920, 1080, grid="level")
        assert od.algorithmic_bytes(p, 1920, 1080, "motion_mask") == px * 9
        assert od.algorithmic_bytes(p, 1920, 1080, "motion_mask_level") == g["out_w"] * g["out_h"] * 8 + px
    with pytest.raises(od.OfdisError):
        od.algorithmic_bytes(p, 1920, 1080, "motion_mask_")


def test_python_refusals_come_before_any_library_call():
    import of_dis_amd as od
    from of_dis_amd import _lib

    class NoLibrary(od.Context):
        def __init__(self):
            self._h = None

    fr = np.zeros((3, 64, 64), np.uint8)
    p = od.oppoint(2, 64, od.MODE_OF, 1)
    for kw in (dict(model=2), dict(step=0), dict(tau=float("nan")), dict(iters=17), dict(thr=-0.5), dict(thr=float("nan")),
               dict(thr=float("inf")), dict(thr=65537.0), dict(rel=-0.1), dict(rel=16.5), dict(rel=float("nan")),
               dict(radius=-1), dict(radius=5), dict(radius=1.5), dict(want_occ=True)):
        with pytest.raises(od.OfdisError) as e:
            NoLibrary().run_sequence_motion_mask_host(fr, p, **kw)
        assert e.value.code == _lib.ERR_INVALID_ARGUMENT, kw
    with pytest.raises(od.OfdisError) as e:
        NoLibrary().run_sequence_motion_mask_host(fr[:1], p)
    assert e.value.code == _lib.ERR_INVALID_ARGUMENT


def test_motion_summary_by_hand():
    import of_dis_amd as od
    s = np.zeros((2, NSTATS), np.int64)
    s[0] = [90, 10, 20, 3, 4, 7, 9, 12, 50, 65, 0, 0]
    s[1] = [0, 0, 120, 12, 10, -1, -1, 0, 0, 0, 0, 0]
    a, b = od.motion_summary(s)
    assert (a["static"], a["moving"], a["unknown"], a["raw"]) == (90, 10, 20, 12)
    assert a["moving_share"] == 0.1 and a["bbox"] == (3, 4, 7, 9) and a["centroid"] == (5.0, 6.5)
    assert b["bbox"] is None and b["centroid"] is None and np.isnan(b["moving_share"])
    assert od.motion_summary(s[0]) == [a]


def mask_scalars_ok(m, thr, rel, radius, w, h):
    """The refusals of the header, stated in Python."""
    if m < 1 or w < 1 or h < 1 or w * h >= 2 ** 31:
        return False
    if not (np.isfinite(thr) and 0.0 <= thr <= 65536.0) or not (np.isfinite(rel) and 0.0 <= rel <= 16.0):
        return False
    return 0 <= radius <= 4


def test_host_refusals_stand_alone(tmp_path):
    """tools/motion_mask_host_check.cpp: the library's scalar refusals built on their own -- under the address and
    undefined-behaviour sanitizers where the toolchain links them -- as a program of its own, against this file's Python."""
    import shutil
    import subprocess
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe, src = str(tmp_path / "motion_mask_host_check"), os.path.join(ROOT, "tools", "motion_mask_host_check.cpp")
    base = [cxx, "-std=c++17", "-O1", "-g", src, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    empty = tmp_path / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    have = subprocess.run([cxx, str(empty), "-o", str(tmp_path / "empty")] + san, capture_output=True).returncode == 0
    r = subprocess.run(base + (san if have else []), capture_output=True, text=True)
    assert r.returncode == 0, f"the {'sanitized' if have else 'plain'} build fails:\n" + r.stderr[-4000:]
    print("motion_mask_host_check built " + ("with -fsanitize=address,undefined" if have else "WITHOUT sanitizers: no runtime to link"))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "failures 0"
    seen = 0
    for line in lines:
        if line.startswith("mask"):
            t = line.replace("->", " ").split()[1:]
            m, thr, rel, radius, w, h, ok = int(t[0]), float(t[1]), float(t[2]), int(t[3]), int(t[4]), int(t[5]), int(t[6])
            assert ok == int(mask_scalars_ok(m, thr, rel, radius, w, h)), line
            seen += 1
    assert seen == 3 * 6 * 6 * 4 * 5
    if not have:
        pytest.skip("no sanitizer runtime on this toolchain: the program's values were compared on a plain build only")


# --------------------------------------------------------------------------------------------- on the oracle's flows

SW, SH, ST = 160, 120, 6


def scene_frames():
    """tests/test_gpu_track.py's scene: a background `_texture(., ., 0)` that drifts by (1.5, -0.75) per frame and a
    41 x 41 patch of another texture that crosses it by (-6, 4) per frame; u8 [6, 120, 160]."""
    y, x = np.mgrid[0:SH, 0:SW].astype(f64)
    frames = []
    for j in range(ST):
        cx, cy = 100 - 6 * j, 30 + 4 * j
        box = (np.abs(x - cx) <= 20) & (np.abs(y - cy) <= 20)
        bg = _texture(x - 1.5 * j, y + 0.75 * j, 0)
        fg = _texture(1.7 * (x - cx) + 40, 1.3 * (y - cy) + 10, 2)
        frames.append(np.rint(np.where(box, fg, bg)).astype(np.uint8))
    return np.stack(frames)


def footprint(j):
    """The patch's pixels in frame j."""
    y, x = np.mgrid[0:SH, 0:SW]
    return (np.abs(x - (100 - 6 * j)) <= 20) & (np.abs(y - (30 + 4 * j)) <= 20)


# measured with the oracle's flows, fit_motion_reference with the check and motion_mask_reference (thr 1, rel 0.05,
# radius 1), pairs 0 .. 4 -- the docstring of test_mask_on_oracle_flows_finds_the_patch
IOU_MEASURED = (0.4040, 0.5588, 0.5820, 0.4511, 0.4893)
FALSE_MEASURED = (0.0039, 0.0113, 0.0077, 0.0110, 0.0058)
IOU_MARGIN = 0.18      # the pair-to-pair spread of the measured values, 0.582 - 0.404
FALSE_MARGIN = 0.0075  # likewise, 0.0113 - 0.0039


def test_mask_on_oracle_flows_finds_the_patch(oracle):
    """160 x 120, 6 frames, op-point 2, both chains from the oracle; the reference fit with the check (similarity, step
    16, tau 2, iters 4), the reference check's forward plane as occ, the reference mask at thr 1, rel 0.05.

    Conditions on the scene (checked on the CPU before the GPU tests were written; this scene gives all of them): each
    of the codes 0, 1, 2 occurs in every pair, and over the video the clean-up at radius 1 turns pixels from 1 to 0 (86)
    and from 0 to 1 (3).

    Measured per pair at radius 1, the moving pixels against the patch's true footprint in the pair's first frame:
      intersection over union  0.404  0.559  0.582  0.451  0.489
      background marked 1      0.0039 0.0113 0.0077 0.0110 0.0058  (of the pixels outside the footprint)
    The union is low because 37-58 % of the footprint fails the forward-backward check and is unknown (code 2); at most
    0.5 % of it is called static (measured with the same arrays).  Asserted: each pair no worse than its measured value less a margin of the size of the pair-to-pair spread,
    0.18 for the union and 0.0075 for the background share."""
    fr = scene_frames()
    p = oracle.oppoint(2, SW, 1, 1)
    fw = np.stack([oracle.run_u8(fr[j, ..., None], fr[j + 1, ..., None], p) for j in range(ST - 1)])
    bw = np.stack([oracle.run_u8(fr[j + 1, ..., None], fr[j, ..., None], p) for j in range(ST - 1)])
    xform = fit_motion_reference(fw, bw, 1, 16, 2.0, 4)[0]
    occ = fb_reference_dir(fw, bw)[0]
    raw = motion_mask_reference(fw, xform, occ, 1.0, 0.05, 0)[0]
    code, res, stats = motion_mask_reference(fw, xform, occ, 1.0, 0.05, 1)
    for j in range(ST - 1):
        assert stats[j, 0] > 0 and stats[j, 1] > 0 and stats[j, 2] > 0, f"pair {j}: {stats[j, :3]}"
    down, up = int(((raw == 1) & (code == 0)).sum()), int(((raw == 0) & (code == 1)).sum())
    print(f"clean-up at radius 1: {down} pixels 1 -> 0, {up} pixels 0 -> 1")
    assert down >= 1 and up >= 1
    assert np.array_equal((raw == 2), (code == 2))  # the clean-up never touches the unknowns
    for j in range(ST - 1):
        fp, m1 = footprint(j), code[j] == 1
        iou = (m1 & fp).sum() / (m1 | fp).sum()
        false = (m1 & ~fp).sum() / (~fp).sum()
        print(f"pair {j}: IoU {iou:.4f} (measured {IOU_MEASURED[j]}), background marked moving {false:.4f} "
              f"(measured {FALSE_MEASURED[j]})")
        assert iou >= IOU_MEASURED[j] - IOU_MARGIN
        assert false <= FALSE_MEASURED[j] + FALSE_MARGIN

"""Point tracking along a chain of flow fields (ofdis_track_points, include/ofdis.h).

`track_reference` below restates the header's definition in vectorised numpy float32 -- every operation on float32
arrays, one rounding each, in the header's order -- and is the reference of every comparison here and in
test_gpu_track.py.

CPU part: the new symbols, their NULL-context refusal, known answers of the reference itself, and what the tracks mean
on the oracle's flows of translated textures.
GPU part (marked gpu): k_track / k_track_level against the reference, positions by their uint32 views and status by
equality.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_fb_check import FIELDS, SHAPES, make_field
from test_interp import _texture

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------- reference

def _inside(px, py, w, h):
    return (px >= 0) & (px <= f32(w - 1)) & (py >= 0) & (py <= f32(h - 1))  # False for NaN


def _sample(G, px, py):
    """S(G, px, py): G float32 [h, w, 2], px / py float32 [N] in-frame positions -> (u, v) float32 [N]."""
    h, w, _ = G.shape
    x0, y0 = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    ax, ay = px - x0.astype(f32), py - y0.astype(f32)
    out = []
    for k in (0, 1):
        g00, g01, g10, g11 = G[y0, x0, k], G[y0, x1, k], G[y1, x0, k], G[y1, x1, k]
        top = g00 + ax * (g01 - g00)
        bot = g10 + ax * (g11 - g10)
        out.append(top + ay * (bot - top))
    assert out[0].dtype == f32
    return out


def _canon(x):
    return np.where(np.isnan(x), f32(np.nan), x).astype(f32)  # the canonical quiet NaN 0x7fc00000


def track_reference(fw, points, bw=None, start=None, alpha=0.01, beta=0.5):
    """fw (and bw) float32 [m, h, w, 2], points [N, 2], start None or int [N] ->
    (tracks float32 [m + 1, N, 2], status uint8 [m + 1, N])."""
    fw = np.ascontiguousarray(fw, f32)
    bw = None if bw is None else np.ascontiguousarray(bw, f32)
    pts = np.ascontiguousarray(points, f32)
    m, h, w, _ = fw.shape
    n = pts.shape[0]
    s0 = np.zeros(n, np.int64) if start is None else np.clip(np.asarray(start, np.int64), 0, m)
    px, py = pts[:, 0].copy(), pts[:, 1].copy()
    st = np.full(n, 3, np.uint8)
    tracks = np.empty((m + 1, n, 2), f32)
    status = np.empty((m + 1, n), np.uint8)
    with np.errstate(all="ignore"):
        for j in range(m + 1):
            st = np.where(s0 == j, np.where(_inside(px, py, w, h), 0, 2), st).astype(np.uint8)
            tracks[j, :, 0], tracks[j, :, 1] = _canon(px), _canon(py)
            status[j] = st
            if j == m:
                break
            act = st < 2  # tracked: the position is inside the frame
            fu, fv = _sample(fw[j], np.where(act, px, f32(0)), np.where(act, py, f32(0)))
            qx, qy = px + fu, py + fv
            inq = _inside(qx, qy, w, h)
            new = st.copy()
            if bw is not None:
                ok = act & inq
                bu, bv = _sample(bw[j], np.where(ok, qx, f32(0)), np.where(ok, qy, f32(0)))
                du, dv = fu + bu, fv + bv
                err = du * du + dv * dv
                mag = (fu * fu + fv * fv) + (bu * bu + bv * bv)
                thr = f32(alpha) * mag + f32(beta)
                assert err.dtype == f32 and thr.dtype == f32
                new = st | np.where(err <= thr, 0, 1).astype(np.uint8)  # a NaN fails
            st = np.where(act, np.where(inq, new, 2), st).astype(np.uint8)
            px, py = np.where(act, qx, px), np.where(act, qy, py)
    return tracks, status


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def assert_tracks_equal(got, want, what):
    """(tracks, status) pairs; None entries of `got` are skipped."""
    if got[0] is not None:
        bad = _bits(got[0]) != _bits(want[0])
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} coordinates differ, first at {np.argwhere(bad)[0]}"
    if got[1] is not None:
        bad = got[1] != want[1]
        assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} status codes differ, first at {np.argwhere(bad)[0]}"


# --------------------------------------------------------------------------------------------- CPU: the ABI

DECLARATIONS = {
    "ofdis_track_points": (
        "ofdis_context *ctx, const void *flow_fw, const void *flow_bw, const ofdis_flow_view *view, int m, int width, "
        "int height, const float *points, const int32_t *start, int npts, float alpha, float beta, int flags, "
        "float *tracks, uint8_t *status, void *stream"),
    "ofdis_run_sequence_track_u8": (
        "ofdis_context *ctx, const uint8_t *frames, int nframes, int width, int height, const ofdis_params *p, "
        "const float *points, const int32_t *start, int npts, int use_fb, float alpha, float beta, int flags, "
        "float *tracks, uint8_t *status, void *stream"),
    "ofdis_run_sequence_track_u8_host": (
        "ofdis_context *ctx, const uint8_t *frames, int nframes, int width, int height, const ofdis_params *p, "
        "const float *points, const int32_t *start, int npts, int use_fb, float alpha, float beta, int flags, "
        "float *tracks, uint8_t *status"),
}


def test_symbols_exist_with_declared_signatures():
    import of_dis_amd as od
    L = od.lib()
    hdr = open(os.path.join(ROOT, "include", "ofdis.h")).read()
    for name, decl in DECLARATIONS.items():
        fn = getattr(L, name)
        assert len(fn.argtypes) == decl.count(",") + 1 and fn.restype is C.c_int
        m = re.search(rf"\bint {name}\(([^;]*)\);", hdr)
        assert m, f"{name} is not declared in ofdis.h"
        assert re.sub(r"\s+", " ", m.group(1)) == decl
    assert re.search(r"#define OFDIS_ABI_VERSION 2\b", hdr) and L.ofdis_abi_version() == 2
    assert {"track", "track_level"} <= set(od.kernel_names())
    assert od.TRACK_LAST == 1 and re.search(r"OFDIS_TRACK_LAST = 1\b", hdr)


def test_null_context_is_refused():
    import of_dis_amd as od
    L = od.lib()
    INV = od._lib.ERR_INVALID_ARGUMENT
    p = od.oppoint(2, 64, od.MODE_OF, 1)
    flow = np.zeros((1, 64, 64, 2), f32)
    img = np.zeros((2, 64, 64), np.uint8)
    pts = np.zeros((4, 2), f32)
    tr, st = np.zeros((2, 4, 2), f32), np.zeros((2, 4), np.uint8)
    v = od.FlowView(0, 0, 0, 64, 64, 1, 0, 0)
    assert L.ofdis_track_points(None, flow.ctypes.data, None, C.byref(v), 1, 64, 64, pts.ctypes.data, None, 4, 0.01, 0.5,
                                0, tr.ctypes.data, st.ctypes.data, None) == INV
    assert L.ofdis_run_sequence_track_u8(None, img.ctypes.data, 2, 64, 64, C.byref(p), pts.ctypes.data, None, 4, 1, 0.01,
                                         0.5, 0, tr.ctypes.data, st.ctypes.data, None) == INV
    assert L.ofdis_run_sequence_track_u8_host(None, img.ctypes.data, 2, 64, 64, C.byref(p), pts.ctypes.data, None, 4, 1,
                                              0.01, 0.5, 0, tr.ctypes.data, st.ctypes.data) == INV


def test_pixel_grid():
    import of_dis_amd as od
    g = od.pixel_grid(7, 5)
    assert g.dtype == f32 and g.shape == (35, 2) and g.flags.c_contiguous
    assert np.array_equal(g[:8], [[0, 0], [1, 0], [2, 0], [3, 0], [4, 0], [5, 0], [6, 0], [0, 1]])  # row-major (x, y)
    g4 = od.pixel_grid(160, 120, 4)
    assert g4.shape == (40 * 30, 2) and np.array_equal(g4[41], [4, 4]) and g4[:, 0].max() == 156 and g4[:, 1].max() == 116
    assert od.pixel_grid(1920, 1080, 4).shape[0] == 129600
    with pytest.raises(ValueError):
        od.pixel_grid(4, 4, 0)


# --------------------------------------------------------------------------------------------- CPU: known answers

def _const(m, h, w, u, v):
    F = np.empty((m, h, w, 2), f32)
    F[..., 0], F[..., 1] = u, v
    return F


def test_reference_zero_fields_return_the_points():
    rng = np.random.default_rng(1)
    pts = (rng.random((50, 2)) * [8, 5]).astype(f32)
    z = np.zeros((4, 6, 9, 2), f32)
    tr, st = track_reference(z, pts, z)
    assert np.array_equal(_bits(tr), _bits(np.broadcast_to(pts, tr.shape))) and not st.any()


def test_reference_constant_chain_and_leaving():
    """F = (2, -1), B = (-2, 1): p + j (2, -1) exactly; status 2 from the step at which the point leaves, then frozen."""
    m, h, w = 6, 8, 12
    F, B = _const(m, h, w, 2, -1), _const(m, h, w, -2, 1)
    pts = np.array([[0, 7], [3, 2], [9.5, 7], [11, 0.5]], f32)
    tr, st = track_reference(F, pts, B)
    for k, (x, y) in enumerate(pts):
        leave = None
        for j in range(m + 1):
            qx, qy = x + 2 * j, y - j
            if leave is None and not (0 <= qx <= w - 1 and 0 <= qy <= h - 1):
                leave = j
            if leave is None:
                assert tuple(tr[j, k]) == (qx, qy) and st[j, k] == 0
            else:  # the entry of the leaving step holds the computed position; later entries repeat it
                assert tuple(tr[j, k]) == (x + 2 * leave, y - leave) and st[j, k] == 2
        assert leave == {0: 6, 1: 3, 2: 1, 3: 1}[k]


def test_reference_quarter_pixel_steps_are_exact():
    m, h, w = 5, 40, 40
    F, B = _const(m, h, w, 1.5, -0.75), _const(m, h, w, -1.5, 0.75)
    y, x = np.mgrid[0:8, 0:8]
    pts = np.stack([x.ravel() * 0.25 + 10, y.ravel() * 0.25 + 20], -1).astype(f32)
    tr, st = track_reference(F, pts, B)
    for j in range(m + 1):
        assert np.array_equal(tr[j], pts + f32(j) * np.array([1.5, -0.75], f32))
    assert not st.any()


def test_reference_threshold_is_inclusive_and_sticky():
    m, h, w = 4, 16, 16
    B = np.zeros((m, h, w, 2), f32)
    pts = np.array([[2, 2], [3.5, 4.25]], f32)
    tr, st = track_reference(_const(m, h, w, 1, 1), pts, B, alpha=0.75, beta=0.5)  # err = thr = 2
    assert not st.any() and np.array_equal(tr[m], pts + f32(m))
    F = _const(m, h, w, 1, 1)
    F[1, ..., 0] = f32(1 + 2.0 ** -20)  # the second step fails: err = 2 + 2^-19 > thr = 2 + 0.75 * 2^-19
    tr, st = track_reference(F, pts, B, alpha=0.75, beta=0.5)
    assert np.array_equal(st[:, 0], [0, 0, 1, 1, 1]) and np.array_equal(st[:, 1], [0, 0, 1, 1, 1])
    assert np.all(tr[m, :, 1] == pts[:, 1] + f32(m)) and np.all(tr[m, :, 0] > pts[:, 0] + f32(m) - f32(1e-3))  # still advances
    assert np.all(tr[3] != tr[2])


def test_reference_start_values():
    m, h, w = 3, 10, 10
    F = _const(m, h, w, 1, 0.5)
    pts = np.tile(np.array([[2, 3]], f32), (5, 1))
    tr, st = track_reference(F, pts, start=[-3, 0, 1, m, m + 5])
    assert np.array_equal(_bits(tr[:, 0]), _bits(tr[:, 1])) and np.array_equal(st[:, 0], st[:, 1])  # -3 behaves as 0
    assert np.array_equal(st[:, 1], [0, 0, 0, 0]) and tuple(tr[m, 1]) == (5, 4.5)
    assert np.array_equal(st[:, 2], [3, 0, 0, 0]) and tuple(tr[0, 2]) == (2, 3) and tuple(tr[m, 2]) == (4, 4)
    assert np.array_equal(st[:, 3], [3, 3, 3, 0]) and np.all(tr[:, 3] == pts[3])  # entries of status 3, then one status 0
    assert np.array_equal(_bits(tr[:, 3]), _bits(tr[:, 4])) and np.array_equal(st[:, 3], st[:, 4])  # m + 5 behaves as m


def test_reference_last_row_and_column_are_inside():
    m, h, w = 2, 6, 9
    z = np.zeros((m, h, w, 2), f32)
    pts = np.array([[w - 1, h - 1], [w - 1, 0], [0, h - 1], [w - 1 + 2.0 ** -10, 2], [3, -(2.0 ** -20)]], f32)
    tr, st = track_reference(z, pts, z)
    assert np.array_equal(st[m], [0, 0, 0, 2, 2]) and np.array_equal(tr[m], pts)


def test_reference_nan():
    m, h, w = 3, 6, 9
    F = _const(m, h, w, 1, 0)
    F[1, 2, 3, 0] = np.nan  # under the second point at its second step
    pts = np.array([[np.nan, 2], [2, 2], [2, 4]], f32)
    tr, st = track_reference(F, pts, np.zeros_like(F), alpha=0.0, beta=2.0)
    assert np.array_equal(st[:, 0], [2, 2, 2, 2]) and np.array_equal(st[:, 1], [0, 0, 2, 2]) and not st[:, 2].any()
    assert np.all(_bits(tr[:, 0, 0]) == 0x7FC00000) and np.all(tr[:, 0, 1] == 2)
    assert np.all(_bits(tr[2:, 1, 0]) == 0x7FC00000) and np.all(tr[2:, 1, 1] == 2) and tuple(tr[1, 1]) == (3, 2)
    neg = pts.copy()
    neg.view(np.uint32)[0, 0] = 0xFFC00001  # another NaN: stored as the canonical one
    assert np.all(_bits(track_reference(F, neg)[0][:, 0, 0]) == 0x7FC00000)


def test_reference_positions_do_not_depend_on_the_backward_chain():
    fw, bw, alpha, beta = make_field("smooth", 64, 4, 2)
    rng = np.random.default_rng(5)
    pts = (rng.random((200, 2)) * [63, 3]).astype(f32)
    with_bw, st_bw = track_reference(fw, pts, bw, alpha=alpha, beta=beta)
    without, st = track_reference(fw, pts)
    assert np.array_equal(_bits(with_bw), _bits(without))
    assert (st_bw == 1).any() and not (st == 1).any()
    assert np.array_equal(st_bw == 2, st == 2)


# --------------------------------------------------------------------------------------------- CPU: meaning

# Measured with the oracle's flows (op-point 2) on these noise-free 160 x 120 textures translated over 6 frames, the
# 4-pixel grid of points: of the points whose true final position stays in the frame 99.2 to 100 % end with status 0,
# and the mean final position error of the status-0 points is 0.052 to 0.092 px (the worst single point 1.8 px).  The
# share bound is below the worst measured share; the error bound is twice the worst measured mean, the rule
# INTERP_RATIO_BOUND of test_interp.py follows.  Both are properties of the reference, not of the code under test.
TRACK_STATUS0_SHARE = 0.98
TRACK_MEAN_ERROR = 0.2
TRACK_SHIFTS = [(3.3, -1.7), (5.0, 3.0), (-4.5, 2.5), (1.5, -0.75)]


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("shift", TRACK_SHIFTS, ids=lambda s: f"{s[0]}_{s[1]}")
def test_reference_tracks_along_oracle_flows_follow_the_translation(oracle, shift, k):
    import of_dis_amd as od
    w, h, nfr = 160, 120, 6
    sx, sy = shift
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = [np.rint(_texture(x - j * sx, y - j * sy, k)).astype(np.uint8)[..., None] for j in range(nfr)]
    p = oracle.oppoint(2, w, 1, 1)
    fw = np.stack([oracle.run_u8(frames[j], frames[j + 1], p) for j in range(nfr - 1)])
    bw = np.stack([oracle.run_u8(frames[j + 1], frames[j], p) for j in range(nfr - 1)])
    pts = od.pixel_grid(w, h, 4)
    tr, st = track_reference(fw, pts, bw)
    truth = pts.astype(np.float64) + (nfr - 1) * np.array([sx, sy])
    stays = (truth[:, 0] >= 0) & (truth[:, 0] <= w - 1) & (truth[:, 1] >= 0) & (truth[:, 1] <= h - 1)
    good = stays & (st[-1] == 0)
    share = good.sum() / stays.sum()
    err = np.hypot(*(tr[-1].astype(np.float64) - truth).T)
    print(f"shift {shift} k {k}: {int(stays.sum())} points stay, status-0 share {share:.4f}, "
          f"mean error {err[good].mean():.4f} px, worst {err[good].max():.3f} px")
    assert share >= TRACK_STATUS0_SHARE
    assert err[good].mean() < TRACK_MEAN_ERROR


# --------------------------------------------------------------------------------------------- GPU

GUARD = 64  # bytes of sentinel on both sides of every output


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


def case_points(w, h, seed):
    """Every pixel centre, 300 random sub-pixel positions, the four corners, positions exactly on the last row and
    column, three points outside the frame and one NaN."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    wm, hm = w - 1, h - 1
    parts = [np.stack([x.ravel(), y.ravel()], -1),
             rng.random((300, 2)) * [wm, hm],
             [[0, 0], [wm, 0], [0, hm], [wm, hm]],
             [[wm, hm * 0.5], [wm, hm * 0.25], [wm * 0.5, hm], [wm * 0.75, hm]],
             [[-0.5, 0], [wm + 0.25, hm], [wm * 0.5, hm + 3]],
             [[np.nan, 0]]]
    return np.ascontiguousarray(np.concatenate([np.asarray(q, np.float64) for q in parts]), f32)


def full_view(w, h, f16=False, planar=False):
    import of_dis_amd as od
    return od.FlowView(int(f16), int(planar), 0, w, h, 1, 0, 0)


def gpu_track(ctx, fw, bw, view, w, h, pts, start=None, alpha=0.01, beta=0.5, last=False, outs=(1, 1), npts=None):
    """ofdis_track_points through raw pointers.  fw / bw: numpy arrays in the view's dtype and layout (bw may be None).
    Both outputs sit between sentinels, which must survive.  -> (tracks, status), None where not passed."""
    import torch
    import of_dis_amd as od
    m = fw.shape[0]
    n = pts.shape[0] if npts is None else npts
    dev = [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (fw, bw, pts, start)]
    entries = n if last else (m + 1) * n
    sizes = (8 * entries, entries)
    bufs = [torch.full((s + 2 * GUARD,), 0xAB, dtype=torch.uint8, device="cuda") if o else None for s, o in zip(sizes, outs)]
    ctx.track_points_ptr(dev[0].data_ptr(), dev[1].data_ptr() if bw is not None else 0, view, m, w, h, dev[2].data_ptr(), n,
                         dev[3].data_ptr() if start is not None else 0, alpha, beta, od.TRACK_LAST if last else 0,
                         *[b.data_ptr() + GUARD if b is not None else 0 for b in bufs],
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    res = []
    for k, b in enumerate(bufs):
        if b is None:
            res.append(None)
            continue
        raw = b.cpu().numpy()
        assert np.all(raw[:GUARD] == 0xAB) and np.all(raw[GUARD + sizes[k]:] == 0xAB), f"output {k}: a sentinel was overwritten"
        body = raw[GUARD:GUARD + sizes[k]].copy()
        lead = () if last else (m + 1,)
        res.append(body.view(f32).reshape(lead + (n, 2)) if k == 0 else body.reshape(lead + (n,)))
    return res


_full_refs = {}


def full_reference(kind, w, h, m):
    """The fields of a case, its points and the references on the float32 and on the binary16-rounded values, once."""
    key = (kind, w, h, m)
    if key not in _full_refs:
        fw, bw, alpha, beta = make_field(kind, w, h, m)
        pts = case_points(w, h, 7 * w + h + m)
        with np.errstate(over="ignore"):
            fh, bh = fw.astype(np.float16), bw.astype(np.float16)
        _full_refs[key] = (fw, bw, fh, bh, alpha, beta, pts, track_reference(fw, pts, bw, None, alpha, beta),
                           track_reference(fh.astype(f32), pts, bh.astype(f32), None, alpha, beta))
    return _full_refs[key]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FIELDS)
@pytest.mark.parametrize("w,h,m", SHAPES)
def test_gpu_track_full_views(ctx, w, h, m, kind):
    fw, bw, fh, bh, alpha, beta, pts, want32, want16 = full_reference(kind, w, h, m)
    for f16 in (False, True):
        F, B, want = (fh, bh, want16) if f16 else (fw, bw, want32)
        for planar in (False, True):
            Fv, Bv = (np.ascontiguousarray(np.moveaxis(a, 3, 1)) for a in (F, B)) if planar else (F, B)
            got = gpu_track(ctx, Fv, Bv, full_view(w, h, f16, planar), w, h, pts, None, alpha, beta)
            assert_tracks_equal(got, want, f"{kind} {w}x{h}x{m} f16={f16} planar={planar}")
    centres = want32[1][:, :w * h]  # the pixel centres start inside the frame
    if kind == "large":
        assert (centres == 2).any(), "no point leaves the frame"
    if kind == "smooth" and w * h >= 35:  # (a handful of pixels need not hold both outcomes)
        assert (centres == 0).any() and (centres == 1).any(), "the check never passes or never fails"


_level_refs = {}


def level_reference(geom, kind, n=3):
    from test_gpu_fb_check_level import geom_dict, make_grids
    from test_gpu_warp import expand_level
    key = (geom, kind, n)
    if key not in _level_refs:
        W, H, g = geom_dict(geom)
        gf, gb, alpha, beta = make_grids(kind, g["out_w"], g["out_h"], n, sum(map(ord, geom + kind)) + n)
        pts = case_points(W, H, sum(map(ord, geom)))
        want = track_reference(expand_level(gf, g, W, H), pts, expand_level(gb, g, W, H), None, alpha, beta)
        _level_refs[key] = (gf, gb, alpha, beta, pts, want)
    return _level_refs[key]


def _level_cases():
    from test_gpu_fb_check_level import GEOMS, KINDS
    return [(g, k) for g in GEOMS for k in KINDS]


@pytest.mark.gpu
@pytest.mark.parametrize("geom,kind", _level_cases())
def test_gpu_track_level_views(ctx, geom, kind):
    from test_gpu_fb_check_level import geom_dict, view_of
    W, H, g = geom_dict(geom)
    gf, gb, alpha, beta, pts, want = level_reference(geom, kind)
    got = gpu_track(ctx, gf, gb, view_of(g), W, H, pts, None, alpha, beta)
    assert_tracks_equal(got, want, f"{geom} {kind}")
    if kind == "smooth":  # no backward chain: the same positions, no status 1
        fwd = gpu_track(ctx, gf, None, view_of(g), W, H, pts)
        assert np.array_equal(_bits(fwd[0]), _bits(want[0])) and np.array_equal(fwd[1] == 2, want[1] == 2)
        assert not (fwd[1] == 1).any()
    centres = want[1][:, :W * H]
    if kind == "large" and W * H > 1:
        assert (centres == 2).any()
    if kind == "smooth" and W * H >= 35:
        assert (centres == 0).any() and (centres == 1).any()


@pytest.mark.gpu
@pytest.mark.parametrize("npts", [1, 255, 256, 257])
def test_gpu_track_block_boundary(ctx, npts):
    fw, bw, _, _, alpha, beta, pts, _, _ = full_reference("smooth", 7, 5, 3)
    sel = pts[35:35 + npts]  # random sub-pixel positions first
    want = track_reference(fw, sel, bw, None, alpha, beta)
    assert_tracks_equal(gpu_track(ctx, fw, bw, full_view(7, 5), 7, 5, sel, None, alpha, beta), want, f"{npts} points")
    # a longer array behind the npts points is not read past them: the outputs end at their sentinels
    assert_tracks_equal(gpu_track(ctx, fw, bw, full_view(7, 5), 7, 5, pts[35:], None, alpha, beta, npts=npts), want,
                        f"{npts} of {len(pts) - 35} points")


@pytest.mark.gpu
@pytest.mark.parametrize("level", [False, True])
def test_gpu_track_start_last_and_single_outputs(ctx, level):
    from test_gpu_fb_check_level import geom_dict, view_of
    from test_gpu_warp import expand_level
    if level:
        W, H, g = geom_dict("67x5-c2")
        gf, gb, alpha, beta, pts, _ = level_reference("67x5-c2", "smooth")
        view, F, B, Fx, Bx = view_of(g), gf, gb, expand_level(gf, g, W, H), expand_level(gb, g, W, H)
    else:
        W, H = 7, 5
        Fx, Bx, _, _, alpha, beta, pts, _, _ = full_reference("smooth", 7, 5, 3)
        view, F, B = full_view(W, H), Fx, Bx
    m = F.shape[0]
    start = np.resize(np.array([-3, 0, 1, 2, m, m + 5, m - 1], np.int32), len(pts))  # every clamp case
    want = track_reference(Fx, pts, Bx, start, alpha, beta)
    assert (want[1] == 3).any() and (want[1][m] != 3).all()
    got = gpu_track(ctx, F, B, view, W, H, pts, start, alpha, beta)
    assert_tracks_equal(got, want, "start")
    last = gpu_track(ctx, F, B, view, W, H, pts, start, alpha, beta, last=True)
    assert_tracks_equal(last, (want[0][m], want[1][m]), "last_only")
    for outs in ((1, 0), (0, 1)):
        for is_last in (False, True):
            one = gpu_track(ctx, F, B, view, W, H, pts, start, alpha, beta, last=is_last, outs=outs)
            assert [x is not None for x in one] == [bool(o) for o in outs]
            assert_tracks_equal(one, (want[0][m], want[1][m]) if is_last else want, f"outputs {outs} last {is_last}")
    assert gpu_track(ctx, F, B, view, W, H, pts, start, alpha, beta, outs=(0, 0)) == [None, None]
    ctx.enable_kernel_timing(True)
    try:
        name = "track_level" if level else "track"
        other = "track" if level else "track_level"
        before, before_other = ctx.kernel_time(name)[1], ctx.kernel_time(other)[1]
        gpu_track(ctx, F, B, view, W, H, pts, start, alpha, beta, outs=(0, 0))  # both NULL: nothing is enqueued
        assert ctx.kernel_time(name)[1] == before
        gpu_track(ctx, F, B, view, W, H, pts, start, alpha, beta, outs=(0, 1))
        assert ctx.kernel_time(name)[1] == before + 1 and ctx.kernel_time(other)[1] == before_other
    finally:
        ctx.enable_kernel_timing(False)


@pytest.mark.gpu
def test_gpu_track_tensor_api(ctx):
    import torch
    fw, bw, fh, bh, alpha, beta, pts, want32, want16 = full_reference("smooth", 130, 3, 1)

    def d(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    tr, st = ctx.track_points(d(fw), d(pts), d(bw), alpha=alpha, beta=beta)
    assert tr.shape == (2, len(pts), 2) and st.shape == (2, len(pts)) and st.dtype == torch.uint8
    assert_tracks_equal((tr.cpu().numpy(), st.cpu().numpy()), want32, "tensor api")
    tr, st = ctx.track_points(d(np.moveaxis(fh, 3, 1)), d(pts), d(np.moveaxis(bh, 3, 1)), alpha=alpha, beta=beta,
                              layout="nchw", last_only=True)
    assert tr.shape == (len(pts), 2) and st.shape == (len(pts),)
    assert_tracks_equal((tr.cpu().numpy(), st.cpu().numpy()), (want16[0][-1], want16[1][-1]), "tensor api, f16 nchw last")
    tr, st = ctx.track_points(d(fw), d(pts))  # no backward chain
    assert_tracks_equal((tr.cpu().numpy(), st.cpu().numpy()), track_reference(fw, pts), "tensor api, forward only")
    with pytest.raises(ValueError):
        ctx.track_points(d(fw), d(pts), d(bw[:, :, :-1]))


@pytest.mark.gpu
def test_gpu_track_refusals_leave_the_context_usable(ctx):
    import torch
    import of_dis_amd as od
    from test_gpu_fb_check_level import geom_dict, view_of
    L = od.lib()
    INV, UNS, OK = od._lib.ERR_INVALID_ARGUMENT, od._lib.ERR_UNSUPPORTED, od._lib.OK
    W, H, g = geom_dict("67x5-c2")
    gf, gb, alpha, beta, pts, want = level_reference("67x5-c2", "smooth")
    m, n = gf.shape[0], len(pts)
    dgf, dgb, dp = (torch.from_numpy(a).cuda() for a in (gf, gb, pts))
    st = torch.full(((m + 1) * n,), 7, dtype=torch.uint8, device="cuda")

    def call(fw=dgf.data_ptr(), bw=dgb.data_ptr(), v=None, m=m, width=W, height=H, points=dp.data_ptr(), npts=n,
             alpha=alpha, beta=beta, flags=0, status=st.data_ptr()):
        return L.ofdis_track_points(ctx._h, fw, bw, None if v is False else C.byref(v if v is not None else view_of(g)), m,
                                    width, height, points, None, npts, alpha, beta, flags, None, status, None)

    def untouched(what):
        torch.cuda.synchronize()
        assert torch.all(st == 7), what

    assert call(v=view_of(g, dtype=1)) == UNS and call(v=view_of(g, layout=1)) == UNS  # level views: float32 interleaved
    assert call(v=view_of(g, dtype=2)) == INV and call(v=view_of(g, layout=2)) == INV and call(v=view_of(g, grid=2)) == INV
    assert call(v=False) == INV
    assert call(v=view_of(dict(g, out_w=g["out_w"] - 1))) == INV and call(v=view_of(dict(g, out_h=g["out_h"] - 1))) == INV
    assert call(v=view_of(dict(g, off_x=2))) == INV and call(v=view_of(dict(g, cell=3))) == INV
    assert call(v=view_of(dict(g, off_y=-1))) == INV
    assert call(fw=None) == INV and call(points=None) == INV
    assert call(m=0) == INV and call(npts=0) == INV and call(npts=-4) == INV
    assert call(width=0) == INV and call(height=-1) == INV and call(width=1 << 16, height=1 << 15) == INV
    assert call(flags=2) == INV and call(flags=-1) == INV and call(flags=3) == INV
    assert call(alpha=-0.01) == INV and call(beta=-1.0) == INV and call(alpha=float("nan")) == INV and call(beta=float("inf")) == INV
    untouched("refused calls")
    assert call(status=None) == OK  # both outputs NULL: nothing to do
    untouched("no outputs")
    assert call(bw=None, alpha=-1.0, beta=float("nan")) == OK  # without a backward chain the thresholds are not read
    torch.cuda.synchronize()
    from test_gpu_warp import expand_level
    assert np.array_equal(st.cpu().numpy().reshape(m + 1, n), track_reference(expand_level(gf, g, W, H), pts)[1])
    assert call() == OK
    torch.cuda.synchronize()
    assert np.array_equal(st.cpu().numpy().reshape(m + 1, n), want[1])
    assert_tracks_equal(gpu_track(ctx, gf, gb, view_of(g), W, H, pts, None, alpha, beta), want, "after the refusals")

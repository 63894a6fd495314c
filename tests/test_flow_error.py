"""The flow error against ground truth (include/ofdis.h: ofdis_flow_error) restated in numpy, and its host side.

``flow_error_reference`` is the definition written out: float32 per pixel, every operation rounded on its own, and the
four float64 sums in the header's order -- 64 lane chains per row, a halving tree over the lanes, the same scheme over
the row sums.  The GPU tests (test_gpu_flow_error.py) import it and hold the kernels to it bit for bit; here it is
checked against known answers, planted boundary pixels, math.fsum and the plain float64 mean of test_known_answer.
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import of_dis_amd as od
from test_known_answer import epe_stats

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES, NSTATS, BINS = 64, 16, 1024


# --------------------------------------------------------------------------------------------- the restatement

def lane_tree_sum(x):
    """The header's sum along the last axis of a float64 array of terms >= +0 (0.0 where a pixel is not counted --
    the same bits as leaving it out): part[t] = ((0.0 + x[t]) + x[t + 64]) + ..., then part[i] += part[i + stride] for
    stride = 32 .. 1."""
    x = np.asarray(x, f64)
    k = -(-x.shape[-1] // LANES)
    pad = np.zeros(x.shape[:-1] + (k * LANES,), f64)
    pad[..., :x.shape[-1]] = x
    pad = pad.reshape(x.shape[:-1] + (k, LANES))
    part = np.zeros(x.shape[:-1] + (LANES,), f64)
    with np.errstate(all="ignore"):
        for j in range(k):
            part = part + pad[..., j, :]
        stride = LANES // 2
        while stride >= 1:
            part = part[..., :stride] + part[..., stride:2 * stride]
            stride //= 2
    return part[..., 0]


def frame_sum(terms):
    """[n, H, W] float64 terms -> [n]: the rows by lane_tree_sum, then the row sums by the same scheme."""
    return lane_tree_sum(lane_tree_sum(terms))


def flow_error_reference(flow, gt, mask=None, mask_eq=-1):
    """flow [n, H, W, 2] float32 or float16, gt [n, H, W, 2] float32, mask u8 [n, H, W] or None ->
    (stats float64 [n, 16], err float32 [n, H, W], hist uint32 [n, 1024])."""
    flow = np.asarray(flow)
    assert flow.dtype in (np.dtype(f32), np.dtype(np.float16))
    flow = flow.astype(f32)  # binary16 converts exactly
    gt = np.asarray(gt)
    assert gt.dtype == f32 and flow.shape == gt.shape and gt.shape[-1] == 2
    n = gt.shape[0]
    u, v, gu, gv = flow[..., 0], flow[..., 1], gt[..., 0], gt[..., 1]
    with np.errstate(all="ignore"):
        known = (np.abs(gu) <= f32(1e9)) & (np.abs(gv) <= f32(1e9))  # false for NaN
        if mask is None:
            ok = known
        else:
            mask = np.asarray(mask)
            assert mask.dtype == np.uint8 and mask.shape == gu.shape
            ok = known & ((mask != 0) if mask_eq < 0 else (mask == mask_eq))
        fin = np.isfinite(u) & np.isfinite(v)
        du, dv = u - gu, v - gv
        e = np.sqrt(du * du + dv * dv)
        g = np.sqrt(gu * gu + gv * gv)
        assert e.dtype == f32 and g.dtype == f32
        e = np.where(fin, e, f32(np.inf))
        counted = ok & fin
        stats = np.zeros((n, NSTATS), f64)
        cnt = lambda m: m.reshape(n, -1).sum(axis=1).astype(f64)  # noqa: E731  (exact integers)
        stats[:, 0] = cnt(ok)
        stats[:, 1] = cnt(ok & ~fin)
        stats[:, 2] = frame_sum(np.where(counted, e.astype(f64), 0.0))
        stats[:, 3] = np.where(counted, e, f32(0)).reshape(n, -1).max(axis=1).astype(f64)
        stats[:, 4] = cnt(ok & (e > f32(1)))
        stats[:, 5] = cnt(ok & (e > f32(3)))
        stats[:, 6] = cnt(ok & (e > f32(5)))
        stats[:, 7] = cnt(ok & (e > f32(3)) & (e > f32(0.05) * g))
        classes = (g < f32(10), (g >= f32(10)) & (g < f32(40)), g >= f32(40))
        for k, cls in enumerate(classes):
            stats[:, 8 + 2 * k] = cnt(counted & cls)
            stats[:, 9 + 2 * k] = frame_sum(np.where(counted & cls, e.astype(f64), 0.0))
        err = np.where(ok, e, f32(-1)).astype(f32)
        scaled = np.where(e < f32(64), e * f32(16), f32(0))
        assert scaled.dtype == f32
        bins = np.where(e < f32(64), scaled.astype(np.int64), BINS - 1)
    hist = np.zeros((n, BINS), np.uint32)
    for i in range(n):
        hist[i] = np.bincount(bins[i][ok[i]], minlength=BINS).astype(np.uint32)
    return stats, err, hist


# --------------------------------------------------------------------------------------------- inputs the GPU tests share

# (estimate - truth, truth): e exactly 1, 3, 5 and 64; g exactly 10 and 40; the Fl rule on both sides of 0.05 g
# (g = 100: 0.05f * 100 rounds to 5, so e = 5 is not an outlier and e = 5.5 is; g = 10: e = 4 > 0.5 is)
PLANTS = [((1, 0), (0, 0)), ((3, 0), (0, 0)), ((3, 4), (0, 0)), ((64, 0), (0, 0)), ((0, 0), (6, 8)), ((0, 0), (24, 32)),
          ((3, 4), (60, 80)), ((5.5, 0), (60, 80)), ((4, 0), (6, 8)), ((0, 63.9375), (1, 1)), ((0.5, 0), (30, 0)),
          ((2, 0), (0, 50))]
# truth that is not known, and estimates that are not finite (over a known truth, and over an unknown one)
UNKNOWN = [(1e10, 0.0), (0.0, -1e10), (np.nan, 1.0), (np.inf, 0.0)]
NONFINITE = [(np.nan, 0.0), (0.0, np.inf), (-np.inf, np.nan)]


def make_case(w, h, n=3, seed=0):
    """gt = 25 N(0, 1), estimate = gt + 3 N(0, 1), a mask in {0, 1, 2}, and in the frames with room for them the
    planted pixels, at flat positions spread over the frame (mask 1 there, but for one NaN estimate under mask 0)."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    gt = (25.0 * rng.standard_normal((n, h, w, 2))).astype(f32)
    est = (gt + (3.0 * rng.standard_normal((n, h, w, 2))).astype(f32)).astype(f32)
    mask = rng.integers(0, 3, (n, h, w)).astype(np.uint8)
    total = len(PLANTS) + len(UNKNOWN) + 2 * len(NONFINITE) + 1
    if w * h >= 2 * total:
        step = (w * h) // total
        g2, e2, m2 = gt.reshape(n, -1, 2), est.reshape(n, -1, 2), mask.reshape(n, -1)
        for f in range(n):
            pos = 0
            for d, t in PLANTS:
                g2[f, pos], e2[f, pos], m2[f, pos] = t, (f32(t[0]) + f32(d[0]), f32(t[1]) + f32(d[1])), 1 + (pos // step) % 2
                pos += step
            for t in UNKNOWN:
                g2[f, pos], m2[f, pos] = t, 1
                pos += step
            for k, bad in enumerate(NONFINITE):
                e2[f, pos], m2[f, pos] = bad, 2          # over a known truth: counted as non-finite
                pos += step
                e2[f, pos], g2[f, pos], m2[f, pos] = bad, UNKNOWN[k], 2  # over an unknown truth: invisible
                pos += step
            e2[f, pos], m2[f, pos] = (np.nan, np.nan), 0  # under a mask that fails with mask_eq -1 and 2
    return est, gt, mask


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# --------------------------------------------------------------------------------------------- known answers

def test_estimate_equal_to_truth():
    _, gt, _ = make_case(70, 9, 2)
    gt = np.where(np.isfinite(gt) & (np.abs(gt) <= 1e9), gt, f32(1)).astype(f32)
    stats, err, hist = flow_error_reference(gt, gt)
    want = np.zeros((2, NSTATS))
    want[:, 0] = 70 * 9
    g = np.sqrt(gt[..., 0] * gt[..., 0] + gt[..., 1] * gt[..., 1])
    for k, cls in enumerate((g < 10, (g >= 10) & (g < 40), g >= 40)):
        want[:, 8 + 2 * k] = cls.reshape(2, -1).sum(1)  # (the class counts: the only other nonzero slots)
    assert np.array_equal(stats, want)
    assert not err.any() and np.array_equal(hist[:, 0], [630, 630]) and not hist[:, 1:].any()


def test_estimate_off_by_3_4():
    rng = np.random.default_rng(5)
    gt = rng.integers(-50, 50, (2, 65, 130, 2)).astype(f32)
    est = gt + np.array([3, 4], f32)
    stats, err, hist = flow_error_reference(est, gt)
    cnt = 65 * 130
    assert np.all(err == 5) and np.array_equal(stats[:, 0], [cnt] * 2) and np.all(stats[:, 1] == 0)
    assert np.array_equal(stats[:, 2], [5.0 * cnt] * 2) and np.all(stats[:, 3] == 5)
    assert np.all(stats[:, 4] == cnt) and np.all(stats[:, 5] == cnt) and np.all(stats[:, 6] == 0)  # 5 is not > 5
    assert np.array_equal(stats[:, 8] + stats[:, 10] + stats[:, 12], [cnt] * 2)
    assert np.array_equal(stats[:, 9] + stats[:, 11] + stats[:, 13], [5.0 * cnt] * 2)
    assert np.all(stats[:, 14:] == 0)
    assert np.all(hist[:, 80] == cnt) and hist.sum() == 2 * cnt


def one_pixel(d, t, mask=None, mask_eq=-1, est=None):
    gt = np.array(t, f32).reshape(1, 1, 1, 2)
    e = (gt + np.array(d, f32)).astype(f32) if est is None else np.array(est, f32).reshape(1, 1, 1, 2)
    m = None if mask is None else np.array(mask, np.uint8).reshape(1, 1, 1)
    stats, err, hist = flow_error_reference(e, gt, m, mask_eq)
    return stats[0], float(err[0, 0, 0]), hist[0]


def test_planted_thresholds():
    # e exactly 1, 3, 5: on the boundary, not above it
    for e, above in ((1, 0), (3, 1), (5, 2)):
        s, err, hist = one_pixel((e, 0), (0, 0))
        assert err == e and list(s[4:7]) == [1.0] * above + [0.0] * (3 - above) and hist[16 * e] == 1
    s, err, hist = one_pixel((np.nextafter(f32(1), f32(2)), 0), (0, 0))
    assert s[4] == 1 and hist[16] == 1
    # e exactly 64, and the largest error below it: both in the last bin; 63.93749 in the one before
    assert one_pixel((64, 0), (0, 0))[2][1023] == 1
    assert one_pixel((63.9375, 0), (0, 0))[2][1023] == 1
    assert one_pixel((np.nextafter(f32(63.9375), f32(0)), 0), (0, 0))[2][1022] == 1
    # g exactly 10 and 40 open their classes
    assert list(one_pixel((2, 0), (6, 8))[0][8:14]) == [0, 0, 1, 2, 0, 0]
    assert list(one_pixel((2, 0), (24, 32))[0][8:14]) == [0, 0, 0, 0, 1, 2]
    assert list(one_pixel((2, 0), (5, 8))[0][8:14]) == [1, 2, 0, 0, 0, 0]
    # Fl: e > 3 and e > 0.05f g.  g = 100: the float32 product 0.05f * 100 is 5
    assert f32(0.05) * f32(100) == f32(5)
    assert one_pixel((3, 4), (60, 80))[0][7] == 0 and one_pixel((5.5, 0), (60, 80))[0][7] == 1
    assert one_pixel((4, 0), (6, 8))[0][7] == 1 and one_pixel((3, 0), (6, 8))[0][7] == 0  # (3 is not > 3)
    assert one_pixel((4, 0), (60, 80))[0][7] == 0 and one_pixel((4, 0), (60, 80))[0][5] == 1  # above 3 px, below 5 %


def test_unknown_truth_and_nonfinite_estimates():
    for t in UNKNOWN:
        s, err, hist = one_pixel((1, 1), t)
        assert not s.any() and err == -1 and not hist.any()
    s, err, hist = one_pixel((1, 1), (1e9, 0))  # 1e9 itself is known
    assert s[0] == 1
    for bad in NONFINITE:
        s, err, hist = one_pixel(None, (1, 2), est=bad)
        assert list(s[:8]) == [1, 1, 0, 0, 1, 1, 1, 1] and not s[8:].any()  # in slot 1 and slots 4-7, in no sum or class
        assert err == np.inf and hist[1023] == 1 and hist.sum() == 1
        s, err, hist = one_pixel(None, (1, 2), mask=0, est=bad)  # a NaN under a failing mask is invisible
        assert not s.any() and err == -1 and not hist.any()
        s, err, hist = one_pixel(None, (1e10, 2), est=bad)
        assert not s.any() and err == -1
    # a finite estimate whose squares overflow is counted: its error is +inf by arithmetic, and so is the sum
    s, err, hist = one_pixel(None, (0, 0), est=(3e38, 3e38))
    assert s[0] == 1 and s[1] == 0 and s[2] == np.inf and s[3] == np.inf and hist[1023] == 1


def test_mask_rules():
    est, gt, mask = make_case(63, 65)
    known = (np.abs(gt) <= 1e9).all(-1)
    for mask_eq, keep in ((-1, mask != 0), (0, mask == 0), (2, mask == 2)):
        stats, err, hist = flow_error_reference(est, gt, mask, mask_eq)
        assert np.array_equal(stats[:, 0], (known & keep).reshape(3, -1).sum(1))
        assert np.array_equal(err == -1, ~(known & keep))
        assert np.array_equal(hist.sum(1), stats[:, 0])
    assert np.array_equal(flow_error_reference(est, gt)[0][:, 0], known.reshape(3, -1).sum(1))


def test_every_slot_is_populated_by_the_shared_case():
    est, gt, mask = make_case(200, 130)
    stats = flow_error_reference(est, gt, mask, -1)[0]
    assert np.all(stats[:, :14] != 0) and np.all(stats[:, 14:] == 0)
    assert np.array_equal(stats[:, 8] + stats[:, 10] + stats[:, 12], stats[:, 0] - stats[:, 1])


def test_float16_estimates_convert_exactly():
    est, gt, mask = make_case(65, 63)
    half = est.astype(np.float16)
    a = flow_error_reference(half, gt, mask, -1)
    b = flow_error_reference(half.astype(f32), gt, mask, -1)
    assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[:2], b[:2])) and np.array_equal(a[2], b[2])


# --------------------------------------------------------------------------------------------- against the plain mean

@pytest.mark.parametrize("w,h", [(1, 1), (63, 65), (64, 64), (200, 130), (1920, 40)])
def test_tree_sum_against_fsum(w, h):
    """<= ~24 float64 additions of positive terms lie on any path of the tree (ceil(W / 64) + 6 per stage at these
    sizes: at most 30 + 6 and 3 + 6), each with relative error <= 2^-53: (1 + 2^-53)^45 - 1 < 1e-14, far inside
    1e-12."""
    rng = np.random.default_rng(w * 7 + h)
    gt = (25 * rng.standard_normal((2, h, w, 2))).astype(f32)
    est = (gt + (3 * rng.standard_normal((2, h, w, 2))).astype(f32)).astype(f32)
    stats, err, _ = flow_error_reference(est, gt)
    for f in range(2):
        want = math.fsum(float(x) for x in err[f].ravel())
        assert abs(stats[f, 2] - want) <= 1e-12 * want
        assert stats[f, 9] + stats[f, 11] + stats[f, 13] == pytest.approx(want, rel=1e-12)


def test_mean_against_the_float64_epe_of_the_oracle_flow(oracle):
    """The 640 x 480 (3.3, -1.7) shift pair of test_known_answer: the restatement's mean is the float64 EPE up to the
    float32 rounding of each e (du, dv, their squares, the sum and the root: a handful of 2^-24 relative steps, and
    the truth itself rounded to float32) -- 1e-5 relative leaves two orders of margin -- and far below the zero flow's
    3.71 px."""
    W, H, shift = 640, 480, (3.3, -1.7)
    a, b = od.synth_shift_pair(W, H, shift, 1, 0)
    flow = oracle.run_u8(a, b, oracle.oppoint(2, W, 1, 1)).astype(f32)
    gt = np.broadcast_to(np.array(shift, f32), (1, H, W, 2)).copy()
    stats = flow_error_reference(flow[None], gt)[0]
    s = od.error_summary(stats)["pooled"]
    want = epe_stats(flow, shift)["whole"]
    print(f"restatement {s['epe']!r}, float64 mean {want!r}")
    assert s["count"] == W * H and abs(s["epe"] - want) <= 1e-5 * want
    zero = od.error_summary(flow_error_reference(np.zeros_like(gt), gt)[0])["pooled"]["epe"]
    assert abs(zero - 3.71) < 0.01 and s["epe"] < zero and s["epe"] <= 0.15  # (the existing whole-image gate)


# --------------------------------------------------------------------------------------------- helpers and plumbing

def test_error_summary_by_hand():
    s = np.zeros((2, 16))
    s[0, :14] = [10, 2, 4.0, 1.5, 5, 3, 2, 1, 4, 1.0, 3, 2.0, 1, 1.0]
    s[1, :14] = [30, 0, 6.0, 2.5, 3, 0, 0, 0, 30, 6.0, 0, 0.0, 0, 0.0]
    r = od.error_summary(s)
    p0, p1, pool = r["pairs"][0], r["pairs"][1], r["pooled"]
    assert p0["count"] == 10 and p0["nonfinite"] == 2 and p0["epe"] == 4.0 / 8 and p0["max"] == 1.5
    assert (p0["r1"], p0["r3"], p0["r5"], p0["fl"]) == (0.5, 0.3, 0.2, 0.1)
    assert (p0["epe_s0_10"], p0["epe_s10_40"], p0["epe_s40"]) == (0.25, 2.0 / 3, 1.0)
    assert p1["epe"] == 0.2 and math.isnan(p1["epe_s10_40"]) and math.isnan(p1["epe_s40"])
    assert pool["count"] == 40 and pool["epe"] == 10.0 / 38 and pool["max"] == 2.5 and pool["r1"] == 8 / 40
    assert pool["epe_s0_10"] == 7.0 / 34
    assert od.error_summary(s[0])["pooled"] == p0
    empty = od.error_summary(np.zeros(16))["pooled"]
    assert empty["count"] == 0 and math.isnan(empty["epe"]) and math.isnan(empty["r1"])


def test_error_percentile_by_hand():
    h = np.zeros(1024, np.uint32)
    h[0], h[16], h[80] = 90, 9, 1
    assert od.error_percentile(h, 0.5) == 1 / 16 and od.error_percentile(h, 0.9) == 1 / 16
    assert od.error_percentile(h, 0.91) == 17 / 16 and od.error_percentile(h, 0.99) == 17 / 16
    assert od.error_percentile(h, 1.0) == 81 / 16
    h[1023] = 100
    assert od.error_percentile(h, 0.99) == math.inf
    assert od.error_percentile(np.stack([h, h]), 0.25) == 1 / 16  # pooled over pairs
    assert math.isnan(od.error_percentile(np.zeros(1024, np.uint32), 0.5))
    assert od.error_percentile(h.view(np.int32), 0.45) == 1 / 16   # (the device returns the counts as int32 bits)
    for q in (0.0, -1.0, 1.5):
        with pytest.raises(ValueError):
            od.error_percentile(h, q)


def test_header_declares_and_library_exports():
    text = open(os.path.join(ROOT, "include", "ofdis.h")).read()
    for name in ("ofdis_flow_error", "ofdis_run_error_u8", "ofdis_run_error_u8_host", "ofdis_kernel_names_ext"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(od.lib(), name), name
    for macro, value in (("OFDIS_FE_LANES", 64), ("OFDIS_FE_NSTATS", 16), ("OFDIS_FE_BINS", 1024)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), text), macro
    assert "acos" in text  # why there is no angular error
    assert (od.FE_LANES, od.FE_NSTATS, od.FE_BINS) == (LANES, NSTATS, BINS)
    assert (od.FE_COUNT, od.FE_NONFINITE, od.FE_SUM, od.FE_MAX, od.FE_GT1, od.FE_GT3, od.FE_GT5, od.FE_FL) == tuple(range(8))
    assert (od.FE_S0_COUNT, od.FE_S0_SUM, od.FE_S1_COUNT, od.FE_S1_SUM, od.FE_S2_COUNT, od.FE_S2_SUM) == tuple(range(8, 14))
    assert od.lib().ofdis_abi_version() == 2


def test_kernel_names_and_byte_model():
    assert len(od.kernel_names()) == 35  # the closed list
    assert od.kernel_names_ext() == ["flow_error", "flow_error_level", "flow_error_sum"]
    assert not set(od.kernel_names()) & set(od.kernel_names_ext())
    p = od.oppoint(2, 1920)
    g = od.out_geometry(p, 1920, 1080, grid="level")
    assert od.algorithmic_bytes(p, 1920, 1080, "flow_error") == 1920 * 1080 * 16
    assert od.algorithmic_bytes(p, 1920, 1080, "flow_error_level") == g["out_w"] * g["out_h"] * 8 + 1920 * 1080 * 8
    assert od.algorithmic_bytes(p, 1920, 1080, "flow_error_sum") == 1080 * 80 + 128
    assert od.algorithmic_bytes(p, 1920, 1080, "upsample") == 1920 * 1080 * 8  # the old names still resolve
    with pytest.raises(od.OfdisError):
        od.algorithmic_bytes(p, 1920, 1080, "flow_error_")


def test_null_context_is_refused():
    L = od.lib()
    INV = od._lib.ERR_INVALID_ARGUMENT
    buf = (C.c_double * 64)()
    ptr = C.addressof(buf)
    v = od.FlowView(0, 0, 0, 4, 4, 1, 0, 0)
    p = od.oppoint(2, 64)
    assert L.ofdis_flow_error(None, ptr, C.byref(v), ptr, None, -1, 1, 4, 4, ptr, None, None, None) == INV
    assert L.ofdis_run_error_u8(None, ptr, ptr, ptr, None, -1, 1, 64, 64, C.byref(p), ptr, None, None, None) == INV
    assert L.ofdis_run_error_u8_host(None, ptr, ptr, ptr, None, -1, 1, 64, 64, C.byref(p), ptr, None, None) == INV
    assert L.ofdis_context_kernel_time(None, b"flow_error", None, None) == INV

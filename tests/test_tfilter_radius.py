"""Temporal denoising over a radius of frames along chained flows (ofdis_tfilter_radius_u8, include/ofdis.h), without a
device.

`tfilter_radius_reference` below restates the header's definition in vectorised numpy float32 -- every operation on
float32 arrays, one rounding each, in the header's order.  Step 1 samples through test_warp.py's `warp_reference` with
the pixel's own flow, exactly as test_tfilter.py's `tfilter_reference` does; steps k >= 2 take their flow from
test_track.py's restated gather `_sample` and their picture values from `sample_at`, warp_reference's taps at a position
(the two are compared below).  It is the reference of every comparison here and in test_gpu_tfilter_radius.py.
`tfilter_radius_scalar` spells the same definition pixel by pixel in numpy float32 scalars, written on its own, and the
two must agree bit for bit.

Also here: the equalities with the radius-1 filter and the check's masks, hand-built cases, the header's declarations
and the bindings, and the denoising gain of a wider radius on the oracle's flows.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_fb_check import fb_reference
from test_tfilter import noisy_video, tfilter_reference
from test_track import _inside, _sample
from test_warp import warp_reference

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------- reference

def sample_at(img, px, py):
    """ofdis_warp_u8's val at the positions themselves: img u8 [h, w, c], px / py float32 [...] (any values; NaN and
    positions outside the frame read the replicated border, as the warp's) -> float32 [..., c]."""
    h, w, _ = img.shape
    with np.errstate(all="ignore"):
        pxc = np.fmin(np.fmax(px, f32(0)), f32(w - 1))  # fmax / fmin: NaN -> 0
        pyc = np.fmin(np.fmax(py, f32(0)), f32(h - 1))
        x0, y0 = np.floor(pxc).astype(np.int64), np.floor(pyc).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
        ax, ay = (pxc - x0.astype(f32))[..., None], (pyc - y0.astype(f32))[..., None]
        t00, t01 = img[y0, x0].astype(f32), img[y0, x1].astype(f32)
        t10, t11 = img[y1, x0].astype(f32), img[y1, x1].astype(f32)
        top = t00 + ax * (t01 - t00)
        bot = t10 + ax * (t11 - t10)
        val = top + ay * (bot - top)
    assert val.dtype == f32
    return val


def _gather(G, qx, qy, at):
    """S(G, P) where `at`, zeros elsewhere (nothing is read there): float32 [h, w] each."""
    shape = qx.shape
    u, v = _sample(G, np.where(at, qx, f32(0)).ravel(), np.where(at, qy, f32(0)).ravel())
    return u.reshape(shape), v.reshape(shape)


def tfilter_radius_reference(frames, flow_fw, flow_bw, sigma, radius, fb=False, alpha=0.01, beta=0.5, out_dtype=np.uint8,
                             positions=None):
    """frames u8 [T, h, w] or [T, h, w, c]; flow_fw / flow_bw [T - 1, h, w, 2] (converted to float32 exactly) ->
    (filtered frames in the frames' shape, u8 or float32; used u8 [T, h, w]).  positions: a dict that receives
    (direction, frame, k) -> (P_k x, P_k y, alive, failed) of every step taken."""
    fr = np.asarray(frames, np.uint8)
    f4 = fr[..., None] if fr.ndim == 3 else fr
    T, h, w, noc = f4.shape
    m = T - 1
    assert m >= 1 and np.shape(flow_fw) == (m, h, w, 2) and np.shape(flow_bw) == (m, h, w, 2) and 1 <= radius <= 4
    fw, bw = np.ascontiguousarray(flow_fw).astype(f32), np.ascontiguousarray(flow_bw).astype(f32)
    inv = f32(1) / (f32(sigma) * f32(noc))
    Cf = f4.astype(f32)
    acc = Cf.copy()
    wsum = np.ones((T, h, w), f32)
    bits = np.zeros((T, h, w), np.uint8)
    ys, xs = (a.astype(f32) for a in np.mgrid[0:h, 0:w])
    with np.errstate(all="ignore"):
        for d in (0, 1):  # every pixel takes the previous direction before the next one
            for i in range(T):
                qx, qy = xs.copy(), ys.copy()
                alive, failed = np.ones((h, w), bool), np.zeros((h, w), bool)
                for k in range(1, radius + 1):
                    j = i + k if d else i - k
                    if not 0 <= j < T:
                        break
                    F, B = (fw[j - 1], bw[j - 1]) if d else (bw[j], fw[j])
                    fu, fv = (F[..., 0], F[..., 1]) if k == 1 else _gather(F, qx, qy, alive)
                    nx, ny = qx + fu, qy + fv
                    qx, qy = np.where(alive, nx, qx), np.where(alive, ny, qy)  # a dead chain reads and moves no more
                    alive = alive & _inside(qx, qy, w, h)
                    if fb:
                        bu, bv = _gather(B, qx, qy, alive)
                        du, dv = fu + bu, fv + bv
                        err = du * du + dv * dv
                        mag = (fu * fu + fv * fv) + (bu * bu + bv * bv)
                        thr = f32(alpha) * mag + f32(beta)
                        assert err.dtype == f32 and thr.dtype == f32
                        failed = failed | (alive & ~(err <= thr))  # a NaN fails; sticky
                    if k == 1:  # literally the radius-1 filter's sample
                        S, inside = warp_reference(f4[j][None], F[None], 1.0, f32)
                        S = S.reshape(h, w, noc)
                        assert np.array_equal(inside[0] != 0, alive)
                    else:
                        S = sample_at(f4[j], qx, qy)
                    ok = alive & ~failed
                    dist = np.abs(S[..., 0] - Cf[i, ..., 0])
                    for ch in range(1, noc):
                        dist = dist + np.abs(S[..., ch] - Cf[i, ..., ch])
                    r = dist * inv
                    wgt = np.where(ok, np.fmax(f32(1) - r * r, f32(0)), f32(0))
                    assert S.dtype == f32 and r.dtype == f32 and wgt.dtype == f32 and qx.dtype == f32
                    acc[i] = acc[i] + wgt[..., None] * S
                    wsum[i] = wsum[i] + wgt
                    bits[i] |= ((wgt > 0).astype(np.uint8) << (2 * (k - 1) + d)).astype(np.uint8)
                    if positions is not None:
                        positions[d, i, k] = (qx.copy(), qy.copy(), alive.copy(), failed.copy())
        val = acc / wsum[..., None]
    assert val.dtype == f32 and np.isfinite(val).all()
    if np.dtype(out_dtype) == np.uint8:
        val = np.rint(np.fmin(val, f32(255))).astype(np.uint8)  # round half to even
    return val.reshape(fr.shape), bits


def _field_scalar(G, px, py):
    """The tracker's gather for one in-frame position, in float32 scalars."""
    h, w, _ = G.shape
    x0, y0 = int(np.floor(px)), int(np.floor(py))
    x1, y1 = min(x0 + 1, w - 1), min(y0 + 1, h - 1)
    ax, ay = f32(px - f32(x0)), f32(py - f32(y0))
    out = []
    for c in (0, 1):
        g00, g01, g10, g11 = f32(G[y0, x0, c]), f32(G[y0, x1, c]), f32(G[y1, x0, c]), f32(G[y1, x1, c])
        top = f32(g00 + f32(ax * f32(g01 - g00)))
        bot = f32(g10 + f32(ax * f32(g11 - g10)))
        out.append(f32(top + f32(ay * f32(bot - top))))
    return out


def _picture_scalar(img, px, py):
    """The bilinear taps of img at an in-frame position, in float32 scalars."""
    h, w, noc = img.shape
    x0, y0 = int(np.floor(px)), int(np.floor(py))
    x1, y1 = min(x0 + 1, w - 1), min(y0 + 1, h - 1)
    ax, ay = f32(px - f32(x0)), f32(py - f32(y0))
    out = []
    for ch in range(noc):
        t00, t01, t10, t11 = f32(img[y0, x0, ch]), f32(img[y0, x1, ch]), f32(img[y1, x0, ch]), f32(img[y1, x1, ch])
        top = f32(t00 + f32(ax * f32(t01 - t00)))
        bot = f32(t10 + f32(ax * f32(t11 - t10)))
        out.append(f32(top + f32(ay * f32(bot - top))))
    return out


def tfilter_radius_scalar(frames, flow_fw, flow_bw, sigma, radius, fb=False, alpha=0.01, beta=0.5):
    """The definition one pixel and one chain at a time -> (float32 pictures [T, h, w, c], used [T, h, w]).  A chain
    ends where it leaves the frame or fails a check: every later weight of it would be an exact zero."""
    f4 = frames[..., None] if frames.ndim == 3 else frames
    T, h, w, noc = f4.shape
    inv = f32(f32(1) / f32(f32(sigma) * f32(noc)))
    wm, hm = f32(w - 1), f32(h - 1)
    out = np.zeros((T, h, w, noc), f32)
    used = np.zeros((T, h, w), np.uint8)
    with np.errstate(all="ignore"):
        for i in range(T):
            for y in range(h):
                for x in range(w):
                    Cc = [f32(f4[i, y, x, ch]) for ch in range(noc)]
                    acc, wsum, bits = list(Cc), f32(1), 0
                    for d, sign in ((0, -1), (1, 1)):
                        px, py = f32(x), f32(y)
                        for k in range(1, radius + 1):
                            j = i + sign * k
                            if j < 0 or j > T - 1:
                                break
                            step, back = (flow_fw[j - 1], flow_bw[j - 1]) if d else (flow_bw[j], flow_fw[j])
                            fu, fv = (f32(step[y, x, 0]), f32(step[y, x, 1])) if k == 1 else _field_scalar(step, px, py)
                            px, py = f32(px + fu), f32(py + fv)
                            if not (px >= 0 and px <= wm and py >= 0 and py <= hm):
                                break
                            if fb:
                                bu, bv = _field_scalar(back, px, py)
                                du, dv = f32(fu + bu), f32(fv + bv)
                                err = f32(f32(du * du) + f32(dv * dv))
                                mag = f32(f32(f32(fu * fu) + f32(fv * fv)) + f32(f32(bu * bu) + f32(bv * bv)))
                                if not err <= f32(f32(f32(alpha) * mag) + f32(beta)):
                                    break
                            S = _picture_scalar(f4[j], px, py)
                            dist = f32(abs(f32(S[0] - Cc[0])))
                            for ch in range(1, noc):
                                dist = f32(dist + f32(abs(f32(S[ch] - Cc[ch]))))
                            r = f32(dist * inv)
                            wgt = max(f32(f32(1) - f32(r * r)), f32(0))
                            acc = [f32(acc[ch] + f32(wgt * S[ch])) for ch in range(noc)]
                            wsum = f32(wsum + wgt)
                            if wgt > 0:
                                bits |= 1 << (2 * (k - 1) + d)
                    out[i, y, x] = [f32(acc[ch] / wsum) for ch in range(noc)]
                    used[i, y, x] = bits
    return out, used


def _zeros(T, h, w):
    return np.zeros((T - 1, h, w, 2), f32)


def _same(got, want, what=""):
    gp, gu = got
    wp, wu = want
    assert gp.dtype == wp.dtype and gp.shape == wp.shape, what
    if gp.dtype == f32:
        gp, wp = gp.view(np.uint32), wp.view(np.uint32)
    assert np.array_equal(gp, wp), f"{what}: {int((gp != wp).sum())} picture values differ"
    assert np.array_equal(gu, wu), f"{what}: {int((gu != wu).sum())} `used` bytes differ"


def random_video(seed, T, h, w, noc, amp, wild=False):
    """Random frames and flows of up to +-amp px; wild: a share of NaN, infinite and far components too."""
    rng = np.random.default_rng(seed)
    fr = rng.integers(0, 256, (T, h, w) if noc == 1 else (T, h, w, noc)).astype(np.uint8)
    fw = ((rng.random((T - 1, h, w, 2)) * 2 - 1) * amp).astype(f32)
    bw = ((rng.random((T - 1, h, w, 2)) * 2 - 1) * amp).astype(f32)
    if wild:
        for G in (fw, bw):
            for val in (np.nan, np.inf, -np.inf, 1000.0, -1000.0):
                G[rng.random(G.shape) < 0.02] = val
    return fr, fw, bw


# --------------------------------------------------------------------------------------------- the restatements

def test_sample_at_is_the_warp_at_the_position():
    rng = np.random.default_rng(4)
    for noc in (1, 3):
        img = rng.integers(0, 256, (9, 13, noc)).astype(np.uint8)
        flow = ((rng.random((1, 9, 13, 2)) * 2 - 1) * 8).astype(f32)
        flow[0, 0, 0], flow[0, 1, 1], flow[0, 2, 2] = (np.nan, 0), (np.inf, 1), (0, -np.inf)
        ys, xs = (a.astype(f32) for a in np.mgrid[0:9, 0:13])
        want, _ = warp_reference(img[None], flow, 1.0, f32)
        with np.errstate(all="ignore"):
            got = sample_at(img, xs + flow[0, ..., 0], ys + flow[0, ..., 1])
        assert np.array_equal(got.view(np.uint32), want.reshape(9, 13, noc).view(np.uint32))


@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("fb", [False, True], ids=["nofb", "fb"])
def test_vectorised_and_scalar_restatements_agree(noc, fb):
    fr, fw, bw = random_video(21 + noc, 6, 16, 24, noc, 6.0)
    if fb:  # one half moves rigidly, the backward fields its inverse: the check passes there and chains go on
        for j in range(5):
            fw[j, :, :12] = (f32(1.25) - f32(0.5) * j, f32(0.75))
            bw[j, :, :12] = -fw[j, :, :12]
    seen = np.zeros(8, bool), np.zeros(8, bool)
    for radius in (1, 2, 3, 4):
        got = tfilter_radius_reference(fr, fw, bw, 90.0 * noc, radius, fb, 0.05, 1.0, out_dtype=f32)
        want = tfilter_radius_scalar(fr, fw, bw, 90.0 * noc, radius, fb, 0.05, 1.0)
        _same((got[0].reshape(want[0].shape), got[1]), want, f"noc {noc} fb {fb} radius {radius}")
        assert got[1].max() < 1 << (2 * radius)
    for b in range(8):  # radius 4: every neighbour is taken somewhere and dropped somewhere
        assert ((got[1] >> b) & 1).any() and not ((got[1][2:4] >> b) & 1).all(), b


# --------------------------------------------------------------------------------------------- the radius-1 filter

@pytest.mark.parametrize("noc", [1, 3])
def test_radius_1_is_the_old_filter(noc):
    fr, fw, bw = random_video(31 + noc, 5, 14, 19, noc, 5.0, wild=True)
    for dt in (np.uint8, f32):
        got = tfilter_radius_reference(fr, fw, bw, 70.0, 1, out_dtype=dt)
        _same(got, tfilter_reference(fr, fw, bw, 70.0, out_dtype=dt), f"noc {noc} {np.dtype(dt).name}")
    assert len(set(got[1].ravel().tolist())) == 4


@pytest.mark.parametrize("noc", [1, 3])
def test_radius_1_with_the_check_is_the_old_filter_with_the_checks_masks(noc):
    fr, fw, bw = random_video(41 + noc, 5, 14, 19, noc, 3.0, wild=True)
    for j in range(4):  # one half moves rigidly and consistently: the check passes on a share of the pixels
        fw[j, :, :10] = (f32(0.75) * (j - 1), f32(-0.5))
        bw[j, :, :10] = -fw[j, :, :10]
    for alpha, beta in ((0.01, 0.5), (0.2, 4.0)):
        occ_fw, occ_bw = fb_reference(fw, bw, alpha, beta)[:2]
        assert {0, 1, 2} <= set(occ_fw.ravel().tolist()) and {0, 1, 2} <= set(occ_bw.ravel().tolist())
        for dt in (np.uint8, f32):
            got = tfilter_radius_reference(fr, fw, bw, 70.0, 1, True, alpha, beta, out_dtype=dt)
            _same(got, tfilter_reference(fr, fw, bw, 70.0, occ_fw, occ_bw, out_dtype=dt), f"noc {noc} alpha {alpha}")
        assert len(set(got[1].ravel().tolist())) == 4


# --------------------------------------------------------------------------------------------- hand-built cases

def test_identical_frames_with_zero_flows_return_the_frames():
    rng = np.random.default_rng(1)
    for noc in (1, 3):
        one = rng.integers(0, 256, (5, 7) if noc == 1 else (5, 7, 3)).astype(np.uint8)
        fr = np.stack([one] * 6)
        for radius in (1, 2, 3, 4):
            for fb in (False, True):
                for dt in (np.uint8, f32):
                    out, used = tfilter_radius_reference(fr, _zeros(6, 5, 7), _zeros(6, 5, 7), 12.0, radius, fb, out_dtype=dt)
                    assert out.dtype == dt and np.array_equal(out, fr.astype(dt))  # n C / n is exact for n <= 9
                    for i in range(6):  # frames within R of an end have shorter chains
                        want = sum(1 << (2 * (k - 1)) for k in range(1, radius + 1) if i - k >= 0)
                        want += sum(1 << (2 * (k - 1) + 1) for k in range(1, radius + 1) if i + k <= 5)
                        assert (used[i] == want).all(), (radius, i)


def test_end_frames_use_one_direction():
    fr, fw, bw = random_video(5, 5, 6, 8, 1, 1.0)
    out, used = tfilter_radius_reference(fr, fw, bw, 4000.0, 4, out_dtype=f32)
    assert ((used[0] & 0b01010101) == 0).all() and ((used[4] & 0b10101010) == 0).all()  # no previous / no next frame
    assert (used[0] != 0).any() and (used[4] != 0).any()
    # frame 0 never reads flow_bw without the check, frame T - 1 never reads flow_fw
    out2, used2 = tfilter_radius_reference(fr, fw, bw + f32(3), 4000.0, 4, out_dtype=f32)
    assert np.array_equal(out2[0], out[0]) and np.array_equal(used2[0], used[0])
    out3, used3 = tfilter_radius_reference(fr, fw - f32(2), bw, 4000.0, 4, out_dtype=f32)
    assert np.array_equal(out3[4], out[4]) and np.array_equal(used3[4], used[4])


def test_used_bits_sit_where_the_definition_puts_them():
    # constant frames of different greys, zero flows, sigma 10: the frame at distance >= 10 grey levels drops out
    T, h, w = 9, 3, 4
    grey = [100, 104, 120, 103, 100, 102, 130, 101, 105]
    fr = np.stack([np.full((h, w), g, np.uint8) for g in grey])
    out, used = tfilter_radius_reference(fr, _zeros(T, h, w), _zeros(T, h, w), 10.0, 4, out_dtype=f32)
    for i in range(T):
        want = 0
        for k in range(1, 5):
            for d, j in ((0, i - k), (1, i + k)):
                if 0 <= j < T and abs(grey[j] - grey[i]) < 10:
                    want |= 1 << (2 * (k - 1) + d)
        assert (used[i] == want).all(), (i, int(used[i, 0, 0]), want)
    # frame 4: previous 103 (k = 1), 104 (k = 3), 100 (k = 4); next 102 (k = 1), 101 (k = 3), 105 (k = 4)
    assert used[4, 0, 0] == 0b11110011
    a, ws = f32(100), f32(1)
    for g in (103, 104, 100, 102, 101, 105):  # the previous direction first, each by rising k
        r = f32(abs(g - 100)) * (f32(1) / f32(10))
        wt = f32(1) - r * r
        a, ws = a + wt * f32(g), ws + wt
    assert out[4, 0, 0] == a / ws


def test_a_chain_that_leaves_the_frame_at_step_2_drops_the_farther_neighbours_of_its_direction_only():
    T, h, w = 9, 4, 12
    fr = np.stack([np.full((h, w), 100 + j, np.uint8) for j in range(T)])
    fw, bw = _zeros(T, h, w), _zeros(T, h, w)
    bw[3, 1, 5] = (2, 0)     # frame 4 -> 3 (step 1 of frame 4's previous chain): pixel (5, 1) moves to (7, 1)
    bw[2, 1, 7] = (20, 0)    # frame 3 -> 2 at (7, 1): x = 27 leaves the frame at step 2
    pos = {}
    out, used = tfilter_radius_reference(fr, fw, bw, 1000.0, 4, out_dtype=f32, positions=pos)
    assert used[4, 1, 5] == 0b10101011  # previous: k = 1 alone; next: all four
    assert used[4, 1, 4] == 0xff and used[4, 2, 5] == 0xff and used[5, 1, 4] == 0b01111111
    assert used[5, 1, 5] == 0b00101111  # frame 5's chain joins the same way at its step 2 and leaves at step 3
    assert pos[0, 4, 1][0][1, 5] == 7 and pos[0, 4, 1][2][1, 5] and not pos[0, 4, 2][2][1, 5]
    # steps 3 and 4 of the dead chain read nothing: wild values along its way change nothing
    bw2 = bw.copy()
    bw2[1] = np.nan
    out2, used2 = tfilter_radius_reference(fr, fw, bw2, 1000.0, 4, out_dtype=f32)
    assert out2[4, 1, 5] == out[4, 1, 5] and used2[4, 1, 5] == used[4, 1, 5]
    # the value: the frame, its previous neighbour and the four next ones
    a, ws = f32(104), f32(1)
    for g in (103, 105, 106, 107, 108):
        r = f32(abs(g - 104)) * (f32(1) / f32(1000))
        wt = f32(1) - r * r
        a, ws = a + wt * f32(g), ws + wt
    assert out[4, 1, 5] == a / ws


def test_a_failed_check_at_step_1_drops_its_direction_and_leaves_positions_and_the_other_direction():
    T, h, w = 7, 5, 12
    rng = np.random.default_rng(8)
    fr = rng.integers(90, 110, (T, h, w)).astype(np.uint8)
    fw, bw = _zeros(T, h, w), _zeros(T, h, w)
    fw[:] = (1, 0)
    bw[:] = (-1, 0)          # consistent: a step right and back
    bw[3, 2, 6] = (-1, 3)    # frame 4 -> 3 at (6, 2) disagrees with frame 3's forward step from (5, 2)
    base, pbase = {}, {}
    free = tfilter_radius_reference(fr, fw, bw, 500.0, 3, False, out_dtype=f32, positions=base)
    chk = tfilter_radius_reference(fr, fw, bw, 500.0, 3, True, 0.0, 0.5, out_dtype=f32, positions=pbase)
    # frame 3, pixel (5, 2): the next chain's step 1 goes to (6, 2) of frame 4 and fails there (err 9 > 0.5)
    assert free[1][3, 2, 5] == 0b111111 and chk[1][3, 2, 5] == 0b010101
    for k in (1, 2, 3):
        for d in (0, 1):
            assert np.array_equal(pbase[d, 3, k][0], base[d, 3, k][0]) and np.array_equal(pbase[d, 3, k][1], base[d, 3, k][1])
        assert pbase[1, 3, k][3][2, 5] and pbase[1, 3, k][2][2, 5]  # failed, sticky, and still alive
    # the previous direction's weights are those of a call that has no next direction at all for this pixel
    a, ws = f32(fr[3, 2, 5]), f32(1)
    for k in (1, 2, 3):
        s = f32(fr[3 - k, 2, 5 - k])
        r = np.abs(s - f32(fr[3, 2, 5])) * (f32(1) / f32(500))
        wt = f32(1) - r * r
        a, ws = a + wt * s, ws + wt
    assert chk[0][3, 2, 5] == a / ws
    # frame 4's previous chain from (6, 2) lands on (5, 5): outside (h = 5) -- dead, bits of that direction clear
    assert (chk[1][4, 2, 6] & 0b010101) == 0 and (free[1][4, 2, 6] & 0b010101) == 0
    same = chk[1] == free[1]
    assert same.mean() > 0.9 and np.array_equal(chk[0][same].view(np.uint32), free[0][same].view(np.uint32))


def test_positions_do_not_depend_on_pictures_sigma_or_thresholds():
    fr, fw, bw = random_video(9, 5, 8, 10, 1, 2.0)
    a, b, c = {}, {}, {}
    tfilter_radius_reference(fr, fw, bw, 30.0, 3, False, positions=a)
    tfilter_radius_reference(255 - fr, fw, bw, 3000.0, 3, True, 0.3, 2.0, positions=b)
    tfilter_radius_reference(fr, fw, bw, 7.0, 3, True, 0.0, 0.0, positions=c)
    for key in a:
        for other in (b, c):
            assert np.array_equal(a[key][0].view(np.uint32), other[key][0].view(np.uint32))
            assert np.array_equal(a[key][1].view(np.uint32), other[key][1].view(np.uint32))
            assert np.array_equal(a[key][2], other[key][2])


# --------------------------------------------------------------------------------------------- header and bindings

SIGNATURES = {
    "ofdis_tfilter_radius_u8": 18,
    "ofdis_run_sequence_tfilter_radius_u8": 15,
    "ofdis_run_sequence_tfilter_radius_u8_host": 14,
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
    decl = re.search(r"\bint ofdis_tfilter_radius_u8\(([^;]*)\);", hdr).group(1)
    assert re.sub(r"\s+", " ", decl) == (
        "ofdis_context *ctx, const uint8_t *frames, int nframes, const void *flow_fw, const void *flow_bw, "
        "const ofdis_flow_view *view, int width, int height, int noc, int radius, float sigma, int use_fb, float alpha, "
        "float beta, int out_dtype, void *out, uint8_t *used, void *stream")
    decl = re.search(r"\bint ofdis_run_sequence_tfilter_radius_u8\(([^;]*)\);", hdr).group(1)
    assert re.sub(r"\s+", " ", decl) == (
        "ofdis_context *ctx, const uint8_t *frames, int nframes, int width, int height, const ofdis_params *p, "
        "int radius, float sigma, int use_fb, float alpha, float beta, int out_dtype, void *out, uint8_t *used, "
        "void *stream")
    for name in ("tfilter_radius", "tfilter_radius_ptr", "run_sequence_tfilter_radius", "run_sequence_tfilter_radius_ptr",
                 "run_sequence_tfilter_radius_host"):
        assert callable(getattr(od.Context, name))


def test_kernel_names_are_at_indices_33_and_34():
    import of_dis_amd as od
    names = od.kernel_names()
    assert names[33] == "tfilter_radius" and names[34] == "tfilter_radius_level" and len(names) == 35
    assert names[32] == "warp_affine" and names[27] == "tfilter" and names[28] == "tfilter_level"


def test_null_context_is_refused():
    import of_dis_amd as od
    L = od.lib()
    p = od.oppoint(2, 64, od.MODE_OF, 1)
    flow = np.zeros(64 * 64 * 2, f32)
    img, out = np.zeros(2 * 64 * 64, np.uint8), np.zeros(2 * 64 * 64, np.uint8)
    d, im, o = flow.ctypes.data, img.ctypes.data, out.ctypes.data
    v = od.FlowView(0, 0, 0, 64, 64, 1, 0, 0)
    INV = od._lib.ERR_INVALID_ARGUMENT
    assert L.ofdis_tfilter_radius_u8(None, im, 2, d, d, C.byref(v), 64, 64, 1, 2, 8.0, 0, 0.01, 0.5, 0, o, None, None) == INV
    assert L.ofdis_run_sequence_tfilter_radius_u8(None, im, 2, 64, 64, C.byref(p), 2, 8.0, 0, 0.01, 0.5, 0, o, None, None) == INV
    assert L.ofdis_run_sequence_tfilter_radius_u8_host(None, im, 2, 64, 64, C.byref(p), 2, 8.0, 0, 0.01, 0.5, 0, o, None) == INV


def test_byte_model():
    import of_dis_amd as od
    px = 1920 * 1080
    for noc in (1, 3):
        p = od.oppoint(2, 1920, od.MODE_OF, noc)
        g = od.out_geometry(p, 1920, 1080, grid="level")
        grid = g["out_w"] * g["out_h"] * 8
        for R in (1, 2, 3, 4):
            assert od.tfilter_radius_bytes(p, 1920, 1080, R) == px * (16 * R + (2 * R + 2) * noc + 1)
            assert od.tfilter_radius_bytes(p, 1920, 1080, R, level=True) == 2 * R * grid + px * ((2 * R + 2) * noc + 1)
            assert od.tfilter_radius_bytes(p, 1920, 1080, R, f32=True) == px * (16 * R + (2 * R + 1 + 4) * noc + 1)
            assert od.tfilter_radius_bytes(p, 1920, 1080, R, level=True, f32=True) == 2 * R * grid + px * ((2 * R + 5) * noc + 1)
        # by name: radius 1 with a u8 picture, the radius-1 filter's counts
        assert od.algorithmic_bytes(p, 1920, 1080, "tfilter_radius") == od.algorithmic_bytes(p, 1920, 1080, "tfilter")
        assert od.algorithmic_bytes(p, 1920, 1080, "tfilter_radius_level") == od.algorithmic_bytes(p, 1920, 1080, "tfilter_level")
        for R in (0, 5, -1):
            with pytest.raises(od.OfdisError):
                od.tfilter_radius_bytes(p, 1920, 1080, R)


def test_python_refusals_come_before_any_library_call():
    import of_dis_amd as od
    from of_dis_amd import _lib

    class NoLibrary(od.Context):
        def __init__(self):
            self._h = None

    fr = np.zeros((3, 64, 64), np.uint8)
    p = od.oppoint(2, 64, od.MODE_OF, 1)
    for kw in (dict(sigma=8.0, radius=0), dict(sigma=8.0, radius=5), dict(sigma=8.0, radius=-1), dict(sigma=8.0, radius=1.5),
               dict(sigma=float("nan"), radius=2), dict(sigma=0.0, radius=2), dict(sigma=65537.0, radius=2),
               dict(sigma=8.0, radius=2, out_dtype=np.float16), dict(sigma=8.0, radius=2, out_dtype=np.int32),
               dict(sigma=8.0, radius=2, fb=True, alpha=-1.0), dict(sigma=8.0, radius=2, fb=True, beta=float("nan"))):
        with pytest.raises(od.OfdisError) as e:
            NoLibrary().run_sequence_tfilter_radius_host(fr, p, **kw)
        assert e.value.code == _lib.ERR_INVALID_ARGUMENT, kw
    with pytest.raises(od.OfdisError) as e:
        NoLibrary().run_sequence_tfilter_radius_host(fr[:1], p, 8.0, 2)
    assert e.value.code == _lib.ERR_INVALID_ARGUMENT
    torch = pytest.importorskip("torch")
    for call in (lambda: NoLibrary().tfilter_radius(None, None, None, 8.0, 0),
                 lambda: NoLibrary().tfilter_radius(None, None, None, 8.0, 5),
                 lambda: NoLibrary().tfilter_radius(None, None, None, float("nan"), 2),
                 lambda: NoLibrary().tfilter_radius(None, None, None, 8.0, 2, out_dtype=torch.float16),
                 lambda: NoLibrary().run_sequence_tfilter_radius(None, p, 8.0, 0),
                 lambda: NoLibrary().run_sequence_tfilter_radius(None, p, 8.0, 5),
                 lambda: NoLibrary().run_sequence_tfilter_radius(None, p, 1e-5, 2),
                 lambda: NoLibrary().run_sequence_tfilter_radius(None, p, 8.0, 2, out_dtype=torch.int8)):
        with pytest.raises(od.OfdisError) as e:
            call()
        assert e.value.code == _lib.ERR_INVALID_ARGUMENT


# --------------------------------------------------------------------------------------------- quality

QUALITY_SHIFTS = [(2.5, -1.25), (-3.0, 2.0)]
R2_OVER_R1 = 0.85    # rms(R = 2) <= 0.85 rms(R = 1)
USED_SHARE = 0.95    # of the window's pixels, every neighbour


@pytest.mark.parametrize("shift", QUALITY_SHIFTS, ids=lambda s: f"{s[0]}_{s[1]}")
def test_a_wider_radius_denoises_more_along_oracle_flows(oracle, shift):
    """160 x 120, op-point 2, 9 frames, Gaussian noise sigma 4 (default_rng(7)), filter sigma 32, no check; the RMS
    against the clean frames over frames 3..5 with a 24-pixel margin.  Measured with the oracle's flows and
    tfilter_radius_reference:
      shift (2.5, -1.25): noisy 4.011, R = 1 1.767 (0.441), R = 2 1.342 (0.334), R = 3 1.094 (0.273); R2 / R1 0.759
      shift (-3, 2):      noisy 4.013, R = 1 2.271 (0.566), R = 2 1.755 (0.437), R = 3 1.476 (0.368); R2 / R1 0.773
    every neighbour contributes on 1.0000 of the window at every radius, the check at the default thresholds changes
    nothing inside the window (R = 3: 1.094 / 1.476 again), and the R = 1 picture is tfilter_reference's bit for bit.
    The bounds -- rms(R = 2) <= 0.85 rms(R = 1), rms(R = 3) < rms(R = 2), every neighbour used on >= 0.95 of the window
    -- are the issue's; they are properties of the definition on the oracle's flows, not of the code under test."""
    w, h, T = 160, 120, 9
    clean, noisy = noisy_video(w, h, T, shift)
    p = oracle.oppoint(2, w, 1, 1)
    fw = np.stack([oracle.run_u8(noisy[j, ..., None], noisy[j + 1, ..., None], p) for j in range(T - 1)])
    bw = np.stack([oracle.run_u8(noisy[j + 1, ..., None], noisy[j, ..., None], p) for j in range(T - 1)])
    win = (slice(3, 6), slice(24, h - 24), slice(24, w - 24))

    def rms(a):
        return float(np.sqrt(((a[win].astype(np.float64) - clean[win]) ** 2).mean()))

    r, share = {0: rms(noisy)}, {}
    for R in (1, 2, 3):
        out, used = tfilter_radius_reference(noisy, fw, bw, 32.0, R, out_dtype=f32)
        r[R] = rms(out)
        share[R] = min(float(((used[win] >> b) & 1).mean()) for b in range(2 * R))
    chk, cused = tfilter_radius_reference(noisy, fw, bw, 32.0, 3, True, out_dtype=f32)
    print(f"shift {shift}: noisy {r[0]:.3f} " + " ".join(f"R={R} {r[R]:.3f} ({r[R] / r[0]:.3f})" for R in (1, 2, 3))
          + f" R2/R1 {r[2] / r[1]:.3f} least-used neighbour " + " / ".join(f"{share[R]:.4f}" for R in (1, 2, 3))
          + f" with the check R=3 {rms(chk):.3f}")
    old, _ = tfilter_reference(noisy, fw, bw, 32.0, out_dtype=f32)
    one, _ = tfilter_radius_reference(noisy, fw, bw, 32.0, 1, out_dtype=f32)
    assert np.array_equal(one.view(np.uint32), old.view(np.uint32))
    assert r[2] <= R2_OVER_R1 * r[1]
    assert r[3] < r[2]
    for R in (1, 2, 3):
        assert share[R] >= USED_SHARE, (R, share[R])

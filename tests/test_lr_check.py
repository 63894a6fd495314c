"""Left-right consistency check (ofdis_lr_check, include/ofdis.h) and the stereo definition, the parts that need no GPU.

`lr_reference` restates the header's definition in vectorised numpy float32 -- every operation on float32 arrays, one
rounding each, in the header's order -- and is the reference of every mask and error comparison here and in
test_gpu_stereo.py.  It is pinned three ways: hand-computed pixels, equality with test_fb_check.fb_reference on the
fields (d, 0), and the CPU oracle run through the stereo definition (`stereo_definition`: the plain depth call, and
the plain depth call on the mirrored, swapped pair, mirrored back and negated).

The scenes (`stereo_scene`) and parameter cases (`STEREO_CASES`) are those of the GPU tests, so the code histograms
asserted here are the ones the GPU tests rely on: every code occurs at least 100 times in both views of every case.
"""
import numpy as np
import pytest

from test_fb_check import fb_reference

f32 = np.float32


# --------------------------------------------------------------------------------------------- reference

def lr_reference_view(D, O, alpha=0.01, beta=0.5):
    """One view: D walks, O is gathered.  D, O float32 [n, h, w] -> (occ u8 [n, h, w], err f32 [n, h, w])."""
    D = np.ascontiguousarray(D, f32)
    O = np.ascontiguousarray(O, f32)
    n, h, w = D.shape
    xs = np.arange(w, dtype=f32)[None, None, :]
    with np.errstate(all="ignore"):
        u = D
        px = xs + u
        inside = (px >= 0) & (px <= f32(w - 1))  # False for NaN
        pxs = np.where(inside, px, f32(0))
        x0 = np.floor(pxs).astype(np.int64)
        x1 = np.minimum(x0 + 1, w - 1)
        ax = pxs - x0.astype(f32)
        fi = np.arange(n)[:, None, None]
        yi = np.arange(h)[None, :, None]
        o0, o1 = O[fi, yi, x0], O[fi, yi, x1]
        b = o0 + ax * (o1 - o0)
        d = u + b
        err = d * d
        mag = u * u + b * b
        thr = f32(alpha) * mag + f32(beta)
        occ = np.where(err <= thr, 0, 1)  # NaN err -> 1
        err = np.where(np.isnan(err), f32(np.nan), err)  # stored as the canonical quiet NaN 0x7fc00000
    assert err.dtype == f32 and thr.dtype == f32 and b.dtype == f32
    return np.where(inside, occ, 2).astype(np.uint8), np.where(inside, err, f32(np.inf)).astype(f32)


def lr_reference(disp_l, disp_r, alpha=0.01, beta=0.5):
    """(occ_l, occ_r, err_l, err_r) of two fields [n, h, w]."""
    ol, el = lr_reference_view(disp_l, disp_r, alpha, beta)
    o_r, er = lr_reference_view(disp_r, disp_l, alpha, beta)
    return ol, o_r, el, er


def pack(d):
    """A disparity field [n, h, w] as the optical-flow field (d, 0) [n, h, w, 2]."""
    return np.stack([d, np.zeros_like(d)], -1)


# --------------------------------------------------------------------------------------------- the stereo definition

def stereo_definition(run, left, right):
    """(disp_l, disp_r) of include/ofdis.h, float32 [..., h, w], from `run(a, b)`: a plain depth call on u8 arrays
    [..., h, w, noc] that returns float32 disparities [..., h, w, 1]."""
    mir = lambda a: np.ascontiguousarray(np.flip(a, -2))  # noqa: E731  (the column axis of [..., h, w, noc])
    dl = np.ascontiguousarray(run(left, right), f32)[..., 0]
    m = np.ascontiguousarray(run(mir(right), mir(left)), f32)[..., 0]
    dr = np.ascontiguousarray(np.flip(m, -1)).view(np.uint32) ^ np.uint32(0x80000000)  # the sign bit flipped
    return dl, dr.view(f32)


# (w, h, noc, op-point, parameter overrides)
STEREO_CASES = [
    (160, 120, 1, 2, {}),
    (173, 97, 1, 2, {}),             # odd padding on both axes: the mirrored view pads on the other side
    (192, 128, 3, 3, {}),            # sc_l = 0 (cell = 1), colour
    (160, 120, 1, 2, {"usefbcon": 1}),
    (160, 120, 1, 2, {"usetvref": 0}),
    (160, 120, 1, 2, {"gradmag": 1}),
]
# sc_l = 2: the sizes at which the mirrored frames' base level takes the aligned load forms (4-byte rows of the
# intensity kernel, dword rows of the colour kernel) -- whole blocks at 320, blocks behind a 4-column padding at 328
STEREO_ALIGNED_CASES = [
    (320, 240, 1, 2, {}),
    (320, 240, 3, 2, {}),
    (328, 232, 1, 2, {}),
]
SCENES = ("synth", "planes")
# every case on both scenes; the aligned cases on the two-plane scene (the colour synthetic pair at 320 x 240 is matched
# so well that no pixel is inconsistent: code 1 would be missing)
CASE_SCENES = [c + (s,) for c in STEREO_CASES for s in SCENES] + [c + ("planes",) for c in STEREO_ALIGNED_CASES]
SCENE_FRAME = 3  # the generator's frame index of every scene here and in test_gpu_stereo.py


def stereo_scene(od, kind, w, h, noc=1, frame=0):
    """A rectified pair (left, right), u8 [h, w, noc].  "synth": the library's DE synthetic pair (true disparity -6.5).
    "planes": a background at disparity -3 and a central rectangle (the middle half of each axis) at -9, composited
    from two pure translations of the same frame -- the rectangle's right-view footprint is its left-view one moved
    by -9, and it hides the background there."""
    if kind == "synth":
        return od.synth_pair(w, h, noc, frame, od.MODE_DE)
    left, far = od.synth_shift_pair(w, h, (-3.0, 0.0), noc, frame)
    left2, near = od.synth_shift_pair(w, h, (-9.0, 0.0), noc, frame)
    assert np.array_equal(left, left2)
    right = far.copy()
    right[h // 4:h - h // 4, w // 4 - 9:w - w // 4 - 9] = near[h // 4:h - h // 4, w // 4 - 9:w - w // 4 - 9]
    return left, right


def _od():
    """The library's synthetic scenes (host code of libofdis.so); the oracle has no generator of its own."""
    try:
        import of_dis_amd as od
        od.lib()
        return od
    except (ImportError, OSError) as e:
        pytest.skip(f"libofdis.so is not available: {e}")


# --------------------------------------------------------------------------------------------- hand-computed pixels

def _one_row(dl, dr, alpha=0.01, beta=0.5):
    out = lr_reference(np.asarray(dl, f32)[None, None, :], np.asarray(dr, f32)[None, None, :], alpha, beta)
    return [x[0, 0] for x in out]


def test_reference_zero_and_opposite_fields():
    z = np.zeros((2, 3, 7), f32)
    assert not any(x.any() for x in lr_reference(z, z))
    dl = np.full((1, 2, 10), -2.5, f32)
    ol, o_r, el, er = lr_reference(dl, -dl)
    assert not ol[..., 3:].any() and not el[..., 3:].any() and np.all(ol[..., :3] == 2)  # x - 2.5 >= 0 <=> x >= 3
    assert np.all(np.isposinf(el[..., :3]))
    assert not o_r[..., :7].any() and np.all(o_r[..., 7:] == 2)                            # x + 2.5 <= 9 <=> x <= 6


def test_reference_position_on_the_last_column():
    """px = W - 1 exactly: inside, x0 = W - 1, x1 clamps to W - 1, ax = 0 -> b = O[W - 1]."""
    dl = np.array([3, 0, 0, 0], f32)       # pixel 0 lands on column 3 = W - 1
    dr = np.array([9, 9, 9, -3], f32)
    ol, o_r, el, er = _one_row(dl, dr)
    assert ol[0] == 0 and el[0] == 0       # 3 + (-3) = 0
    dr[3] = -1                             # d = 2, err = 4 > 0.01 * (9 + 1) + 0.5
    ol, o_r, el, er = _one_row(dl, dr)
    assert ol[0] == 1 and el[0] == 4
    ol, o_r, el, er = _one_row(np.array([np.nextafter(f32(3), f32(4)), 0, 0, 0], f32), dr)
    assert ol[0] == 2 and np.isposinf(el[0])  # one ulp beyond the last column leaves the frame


def test_reference_interpolates_between_two_taps():
    """px = 1.25: b = O[1] + 0.25 * (O[2] - O[1]) = -1 + 0.25 * (-3 + 1) = -1.5; d = 1.25 - 1.5 = -0.25."""
    ol, o_r, el, er = _one_row([1.25, 0, 0, 0], [0, -1, -3, 0])
    assert el[0] == f32(0.0625) and ol[0] == 0
    thr = f32(0.01) * (f32(1.25) * f32(1.25) + f32(1.5) * f32(1.5)) + f32(0)
    assert _one_row([1.25, 0, 0, 0], [0, -1, -3, 0], 0.01, 0.0)[0][0] == (0 if f32(0.0625) <= thr else 1) == 1


def test_reference_negative_zero_position():
    """u = -0.0 at x = 0: px = -0.0 passes px >= 0, floor gives column 0, ax = -0.0 and b = O[0]."""
    ol, o_r, el, er = _one_row([-0.0, 0], [5, 7])
    assert ol[0] == 1 and el[0] == 25      # 25 > 0.01 * 25 + 0.5
    ol, o_r, el, er = _one_row([-0.0, 0], [-0.0, 7])
    assert ol[0] == 0 and el[0] == 0 and not np.signbit(el[0])


def test_reference_nan_and_infinities():
    nan, inf = f32(np.nan), f32(np.inf)
    # a NaN or infinite own disparity leaves the frame (NaN fails both comparisons)
    for u in (nan, inf, -inf):
        ol, o_r, el, er = _one_row([u, 0, 0], [0, 0, 0])
        assert ol[0] == 2 and np.isposinf(el[0])
    # an in-frame pixel gathering a NaN tap: code 1, the canonical quiet NaN
    ol, o_r, el, er = _one_row([1, 0, 0], [0, nan, 0])
    assert ol[0] == 1 and el[:1].view(np.uint32)[0] == 0x7FC00000
    # gathering +inf at ax = 0: b = inf + 0 * (O[x1] - inf) = inf + NaN = NaN as well
    ol, o_r, el, er = _one_row([1, 0, 0], [0, inf, 0])
    assert ol[0] == 1 and el[:1].view(np.uint32)[0] == 0x7FC00000
    # gathering -inf at the clamped last column: O[x1] - O[x0] = -inf + inf = NaN
    ol, o_r, el, er = _one_row([2, 0, 0], [0, 0, -inf])
    assert ol[0] == 1 and np.isnan(el[0])
    # the other view: right pixel 1 stays put and reads the left view's 0 there; right pixel 2 leaves the frame
    assert o_r[1] == 0 and er[1] == 0 and o_r[2] == 2


def test_reference_one_pixel_frame():
    for u, code in ((0.0, 0), (-0.0, 0), (0.5, 2), (-0.5, 2), (np.nan, 2)):
        ol, o_r, el, er = lr_reference(np.full((1, 1, 1), u, f32), np.zeros((1, 1, 1), f32))
        # the right pixel stays put and reads u: 0.25 <= 0.01 * 0.25 + 0.5 is consistent, a NaN is not
        assert ol[0, 0, 0] == code and o_r[0, 0, 0] == (1 if np.isnan(u) else 0)
    ol, o_r, el, er = lr_reference(np.zeros((1, 1, 1), f32), np.full((1, 1, 1), 2, f32))
    assert ol[0, 0, 0] == 1 and el[0, 0, 0] == 4 and o_r[0, 0, 0] == 2


# --------------------------------------------------------------------------------------------- against fb_reference

def random_fields(w, h, n=2, seed=0):
    """Finite disparities of both signs, a few pixels wide, with exact zeros, -0.0 and on-border positions planted."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    dl = (rng.standard_normal((n, h, w)) * 4 - 3).astype(f32)
    dr = (rng.standard_normal((n, h, w)) * 4 + 3).astype(f32)
    for d in (dl, dr):
        k = max(1, d.size // 16)
        d.reshape(-1)[rng.choice(d.size, k, replace=False)] = 0
        d.reshape(-1)[rng.choice(d.size, k, replace=False)] = -0.0
    xs = np.arange(w, dtype=f32)
    dl[:, 0, :] = -xs                 # every pixel of row 0 lands on column 0 ...
    dr[:, 0, :] = f32(w - 1) - xs     # ... and on the last column
    return dl, dr


@pytest.mark.parametrize("w,h", [(5, 3), (64, 4), (173, 97)])
def test_reference_equals_fb_reference_on_packed_fields(w, h):
    dl, dr = random_fields(w, h)
    for alpha, beta in ((0.01, 0.5), (0.0, 0.0), (0.2, 0.1)):
        got = lr_reference(dl, dr, alpha, beta)
        want = fb_reference(pack(dl), pack(dr), alpha, beta)
        for k in range(4):
            assert np.array_equal(got[k].view(np.uint8 if k < 2 else np.uint32),
                                  want[k].view(np.uint8 if k < 2 else np.uint32)), (alpha, beta, k)
        assert set(np.unique(got[0])) == {0, 1, 2} or (w, h) == (5, 3)


# --------------------------------------------------------------------------------------------- the CPU oracle

@pytest.mark.parametrize("w,h,noc,op,over,scene", CASE_SCENES + [(176, 96, 1, 2, {}, s) for s in SCENES])
def test_oracle_stereo_definition(oracle, w, h, noc, op, over, scene):
    """The definition on the CPU oracle: the left map is <= 0, the right map >= 0, and every code occurs at least 100
    times in both views (no mask test can pass on a constant mask).  On the synthetic pair (true disparity -6.5) the
    medians of the refined fields lie within 0.5 of 6.5: -6.18 / +6.11 at 160 x 120, -6.30 / +6.31 at 173 x 97,
    -6.28 / +6.26 at 176 x 96, -6.55 / +6.56 at 192 x 128 colour, -6.19 / +6.20 with usefbcon = 1.  Two cases have no
    such median and it is printed, not asserted, there: without the variational refinement the oracle's 160 x 120 field
    underestimates (-5.61 / +5.61), and on gradient-magnitude input it scatters (-7.63 / +6.27, 65 % of the pixels
    inconsistent) -- properties of the plain depth call at this size, not of the stereo call."""
    od = _od()
    left, right = stereo_scene(od, scene, w, h, noc, SCENE_FRAME)
    p = oracle.oppoint(op, w, 2, noc)
    for k, v in over.items():
        setattr(p, k, v)
    dl, dr = stereo_definition(lambda a, b: oracle.run_u8(a, b, p), left, right)
    dl, dr = dl.reshape(h, w), dr.reshape(h, w)
    assert np.all(dl <= 0) and np.all(dr >= 0)
    occ_l, occ_r, err_l, err_r = lr_reference(dl[None], dr[None])
    counts = [np.bincount(o.reshape(-1), minlength=3) for o in (occ_l, occ_r)]
    ok = [float((o == 0).mean()) for o in (occ_l, occ_r)]
    print(f"{scene} {w}x{h} noc {noc} op {op} {over}: median l {np.median(dl):.2f} r {np.median(dr):.2f}, "
          f"codes l {counts[0].tolist()} r {counts[1].tolist()}, consistent {ok[0]:.2f} / {ok[1]:.2f}")
    for c in counts:
        assert c.min() >= 100, counts
    if scene == "synth" and over.get("usetvref", 1) and not over.get("gradmag", 0):
        assert abs(abs(np.median(dl)) - 6.5) <= 0.5 and abs(abs(np.median(dr)) - 6.5) <= 0.5

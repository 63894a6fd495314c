"""Global motion and stabilisation on the device: ofdis_fit_motion, ofdis_smooth_path and ofdis_warp_affine_u8 against
test_stabilize.py's numpy restatements, bit for bit (float64 compared as uint64), in every flow format; the level-grid
view against the full field; the fused call ofdis_run_sequence_stabilize_u8 against its definition -- the three
primitives on the fields of run_sequence -- in every issue form; timers, host form, command lines, refusals.

The scene is test_gpu_track.py's: a textured background that drifts by (1.5, -0.75) per frame and a 41 x 41 patch of
another texture that crosses it by (-6, 4) per frame, 6 frames.  The patch is the fit's outlier population: its samples
fail the forward-backward check at its border and carry a foreign motion inside.  test_every_sample_class_occurs has a
scene of its own and says why.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_fb_check import fb_reference_dir
from test_gpu_sequence import _write_pngs
from test_gpu_track import CASES, T, scene
from test_gpu_warp import ISSUES, _dev, _np
from test_interp import _texture
from test_stabilize import (IDENTITY, bits, fit_motion_reference, lattice, similarity_matrix, smooth_path_reference,
                            warp_affine_reference, zoom_transform)

pytestmark = pytest.mark.gpu

f32 = np.float32
f64 = np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (16, 8, 3)  # on 160 x 120: 70 samples (fewer than one lane row), 300 (a partial second row), 2120 (nine rows)
FIT = dict(tau=2.0, iters=4)


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


_fields = {}


def fields(ctx, case):
    """The case's frames and run_sequence(bidir=True)'s two flows, computed once: torch tensors."""
    if case not in _fields:
        w, h, noc, mk = CASES[case]
        fr = _dev(scene(w, h, noc))
        _fields[case] = (fr,) + tuple(ctx.run_sequence(fr, mk(), bidir=True)[:2])
    return _fields[case]


def same_bits(got, want, what):
    """Tuples of numpy arrays or torch tensors, compared as raw bits."""
    for k, (g, w_) in enumerate(zip(got, want)):
        g = g if isinstance(g, np.ndarray) else _np(g)
        w_ = w_ if isinstance(w_, np.ndarray) else _np(w_)
        assert g.dtype == w_.dtype and g.shape == w_.shape, f"{what}: output {k} is {g.dtype} {g.shape}, expected {w_.dtype} {w_.shape}"
        a, b = (bits(g), bits(w_)) if g.dtype.itemsize in (4, 8) else (g, w_)
        bad = a != b
        assert not bad.any(), f"{what}: output {k}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}"


# --------------------------------------------------------------------------------------------- the fit

@pytest.mark.parametrize("case", list(CASES))
def test_fit_motion_equals_the_restatement(ctx, case):
    w, h, noc, mk = CASES[case]
    p = mk()
    fr, fw, bw = fields(ctx, case)
    nfw, nbw = _np(fw), _np(bw)
    gf = ctx.run_sequence(fr, p, grid="level")
    gb = ctx.run(fr[1:], fr[:-1], p, grid="level")
    kw = dict(want_support=True, want_weights=True, **FIT)
    for step in STEPS:
        for model in (0, 1):
            for fb in (False, True):
                what = f"{case} step {step} model {model} fb {fb}"
                want = fit_motion_reference(nfw, nbw if fb else None, model, step, **FIT)
                assert want[1].min() >= 3 and want[2].shape == (T - 1, lattice(w, h, step)[0].size * lattice(w, h, step)[1].size)
                for layout in ("nhwc", "nchw"):
                    a, b = (fw, bw) if layout == "nhwc" else (fw.permute(0, 3, 1, 2).contiguous(), bw.permute(0, 3, 1, 2).contiguous())
                    got = ctx.fit_motion(a, b if fb else None, model, step, layout=layout, **kw)
                    same_bits(got, want, f"{what} float32 {layout}")
                # the level view gives the bits of the full float32 field
                got = ctx.fit_motion(gf, gb if fb else None, model, step, grid="level", p=p, size=(w, h), **kw)
                same_bits(got, want, f"{what} level view")
                alone = ctx.fit_motion(gf, gb if fb else None, model, step, grid="level", p=p, size=(w, h), **FIT)
                same_bits((alone,), want[:1], f"{what} level view, no support / weights")
                want16 = fit_motion_reference(nfw.astype(np.float16), nbw.astype(np.float16) if fb else None, model, step, **FIT)
                for layout in ("nhwc", "nchw"):
                    a, b = (fw.half(), bw.half())
                    if layout == "nchw":
                        a, b = a.permute(0, 3, 1, 2).contiguous(), b.permute(0, 3, 1, 2).contiguous()
                    got = ctx.fit_motion(a, b if fb else None, model, step, layout=layout, **kw)
                    same_bits(got, want16, f"{what} float16 {layout}")


def test_fit_motion_iterations_thresholds_and_one_pair(ctx):
    """Other taus and solve counts, one pair alone, and step 1: 19 200 samples, more than the kernel keeps between the
    solves, so every solve reads the fields again."""
    w, h, noc, mk = CASES["160x120"]
    p = mk()
    fr, fw, bw = fields(ctx, "160x120")
    nfw, nbw = _np(fw), _np(bw)
    gf = ctx.run_sequence(fr, p, grid="level")
    gb = ctx.run(fr[1:], fr[:-1], p, grid="level")
    kw = dict(want_support=True, want_weights=True)
    for tau, iters, step, alpha, beta in ((2.0, 0, 8, 0.01, 0.5), (0.5, 1, 8, 0.0, 0.05), (8.0, 16, 16, 0.05, 2.0), (2.0, 2, 1, 0.01, 0.5)):
        for model in (0, 1):
            want = fit_motion_reference(nfw, nbw, model, step, tau, iters, alpha, beta)
            what = f"tau {tau} iters {iters} step {step} model {model}"
            same_bits(ctx.fit_motion(fw, bw, model, step, tau, iters, alpha, beta, **kw), want, what)
            same_bits(ctx.fit_motion(gf, gb, model, step, tau, iters, alpha, beta, grid="level", p=p, size=(w, h), **kw), want,
                      what + " level view")
    one = fit_motion_reference(nfw[2:3], nbw[2:3], 1, 8, **FIT)
    same_bits(ctx.fit_motion(fw[2:3], bw[2:3], 1, 8, **FIT, **kw), one, "one pair")


def paused_scene(w=160, h=120, nfr=T):
    """A 41 x 41 square of another texture over a background that stands still: the square rests for the first pair
    (frames 0 and 1 are equal) and then crosses by (-6, 4) per frame.  u8 [nfr, h, w]."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = []
    for j in range(nfr):
        k = max(j - 1, 0)
        cx, cy = 100 - 6 * k, 30 + 4 * k
        box = (np.abs(x - cx) <= 20) & (np.abs(y - cy) <= 20)
        frames.append(np.rint(np.where(box, _texture(1.7 * (x - cx) + 40, 1.3 * (y - cy) + 10, 2), _texture(x, y, 0))).astype(np.uint8))
    return np.stack(frames)


def test_every_sample_class_occurs(ctx):
    """The four classes of a sample, each of them non-empty in one fit (160 x 120 grey, similarity, step 8, tau 2, iters 4,
    with the check).  test_gpu_track's `scene` gives three of them -- 149 dropped, 74 with weight 0 by residual, 1277
    strictly between 0 and 1 -- but no float32 weight of exactly 1: a weight rounds to 1 below a residual of
    tau * 2^-12.5 = 3.5e-4 px, and the oracle's flow of a background beside a moving square is not that close to any
    similarity (on a background that stands still its median magnitude is 0.01-0.03 px; over `scene` and two such
    scenes, steps 8 and 3, tau 2 and 4, at most 2 of up to 10 600 samples reach 1.0f, by chance).  `paused_scene` has
    the class by construction: equal frames have zero flow, residual 0 and weight 1.  Measured with the oracle's
    flows and the restatement, per pair: dropped 0 / 16 / 12 / 13 / 9, weight 0 by residual 0 / 30 / 28 / 28 / 28,
    between 0 and 1: 0 / 254 / 260 / 259 / 263, exactly 1: 300 / 0 / 0 / 0 / 0."""
    w, h, noc, mk = CASES["160x120"]
    fr = _dev(paused_scene(w, h))
    fw, bw = ctx.run_sequence(fr, mk(), bidir=True)[:2]
    nfw, nbw = _np(fw), _np(bw)
    xform, support, wgt = (_np(x) for x in ctx.fit_motion(fw, bw, 1, 8, want_support=True, want_weights=True, **FIT))
    same_bits((xform, support, wgt), fit_motion_reference(nfw, nbw, 1, 8, **FIT), "paused scene, step 8")
    xs, ys = lattice(w, h, 8)
    X, Y = (a.reshape(-1) for a in np.meshgrid(xs, ys))
    occ = fb_reference_dir(nfw, nbw)[0][:, Y, X]
    finite = np.isfinite(nfw[:, Y, X]).all(-1)
    dropped = (occ != 0) | ~finite
    classes = {"dropped by the check": int(dropped.sum()), "weight 0 by residual": int(((wgt == 0) & ~dropped).sum()),
               "weight strictly between 0 and 1": int(((wgt > 0) & (wgt < 1)).sum()), "weight 1": int((wgt == 1).sum())}
    print("paused scene, step 8, 5 x 300 samples:", classes)
    assert (wgt[dropped] == 0).all() and min(classes.values()) > 0, classes
    assert sum(classes.values()) == wgt.size and np.array_equal(support, (wgt > 0).sum(1))
    # the fit sees the background, which stands still, not the square's (-6, 4)
    assert np.array_equal(xform[0], IDENTITY) and np.abs(xform - IDENTITY).max() < 0.1
    # and on test_gpu_track's scene the background's drift (1.5, -0.75)
    fr, fw, bw = fields(ctx, "160x120")
    xform = _np(ctx.fit_motion(fw, bw, 1, 8, **FIT))
    cx, cy = (w - 1) / 2, (h - 1) / 2  # (measured with the oracle's flows: within 0.024 px at the frame centre)
    assert np.abs(xform[:, 0] * cx + xform[:, 1] * cy + xform[:, 2] - cx - 1.5).max() < 0.05
    assert np.abs(xform[:, 3] * cx + xform[:, 4] * cy + xform[:, 5] - cy + 0.75).max() < 0.05


def test_fit_motion_degenerate_fields(ctx):
    import torch
    w, h = 67, 45
    zero = torch.zeros((2, h, w, 2), device="cuda")
    for model in (0, 1):
        x, s, wg = ctx.fit_motion(zero, None, model, 8, want_support=True, want_weights=True, **FIT)
        assert (_np(x) == IDENTITY).all() and (_np(s) == 48).all() and (_np(wg) == 1).all()
    F = np.full((2, h, w, 2), np.nan, f32)
    F[1] = 0.25
    F[1, 4, 4] = (np.inf, 0)
    F[1, 4, 12] = (0, -np.inf)
    B = np.full((2, h, w, 2), -0.25, f32)
    for model in (0, 1):
        for bw_ in (None, B):
            want = fit_motion_reference(F, bw_, model, 8, **FIT)
            # 48 samples, two of them infinite; with the check the row y = 44 leaves the frame (44.25 > H - 1)
            assert np.array_equal(bits(want[0][0]), bits(IDENTITY)) and want[1].tolist() == [0, 46 if bw_ is None else 38]
            got = ctx.fit_motion(_dev(F), None if bw_ is None else _dev(bw_), model, 8, want_support=True, want_weights=True, **FIT)
            same_bits(got, want, f"all-NaN pair and non-finite samples, model {model}, fb {bw_ is not None}")


# --------------------------------------------------------------------------------------------- path and affine warp

def some_transforms(n, w, h, seed=5):
    rng = np.random.default_rng(seed)
    return np.array([similarity_matrix(1 + rng.uniform(-0.03, 0.03), rng.uniform(-0.05, 0.05), rng.uniform(-6, 6),
                                       rng.uniform(-6, 6), w, h) for _ in range(n)])


@pytest.mark.parametrize("case", ["160x120", "150x110-rgb"])
def test_smooth_path_and_warp_affine_equal_the_restatements(ctx, case):
    import torch
    w, h, noc, mk = CASES[case]
    fr, fw, bw = fields(ctx, case)
    frames = scene(w, h, noc)
    for xf in (_np(ctx.fit_motion(fw, bw, **FIT)), some_transforms(T - 1, w, h)):
        for radius in (0, 2, T + 3):  # the last: every window clamps at both ends
            for zoom in (1.0, 1.25):
                want = smooth_path_reference(xf, radius, zoom, w, h)
                got = ctx.smooth_path(_dev(xf), (w, h), radius, zoom)
                same_bits((got,), (want,), f"{case} smooth_path radius {radius} zoom {zoom}")
                for dt, tdt in ((np.uint8, torch.uint8), (f32, torch.float32)):
                    pic = ctx.warp_affine(fr, got, out_dtype=tdt, want_valid=True)
                    same_bits(pic, warp_affine_reference(frames, want, dt), f"{case} warp_affine radius {radius} zoom {zoom} {tdt}")
                    alone = ctx.warp_affine(fr, got, out_dtype=tdt)
                    same_bits((alone,), (pic[0],), f"{case} warp_affine without valid")
    # long paths: more frames than lanes, and a singular and a non-finite transform on the way
    xf = some_transforms(300, w, h, 6)
    xf[:, [2, 5]] *= 0.05
    for radius in (0, 5, 256):
        same_bits((ctx.smooth_path(_dev(xf), (w, h), radius, 1.5),), (smooth_path_reference(xf, radius, 1.5, w, h),), f"301 frames radius {radius}")
    xf = some_transforms(6, w, h, 7)
    xf[2] = 0
    xf[4, 0] = np.nan
    want = smooth_path_reference(xf, 1, 1.0, w, h)
    assert (want[4:] == IDENTITY).all() and not (want[:4] == IDENTITY).all(1).any()  # frame 3's window still holds C_2
    same_bits((ctx.smooth_path(_dev(xf), (w, h), 1, 1.0),), (want,), "singular and NaN transforms")
    bad = np.tile(IDENTITY, (T, 1))
    bad[1, 2], bad[2, 4], bad[3] = np.nan, np.inf, (0, 0, 500, 0, 0, -3)
    same_bits(ctx.warp_affine(fr, _dev(bad), want_valid=True), warp_affine_reference(frames, bad), "non-finite and constant transforms")


@pytest.mark.parametrize("noc", [1, 3])
def test_warp_affine_wide_frame_and_odd_widths(ctx, noc):
    """2100 x 70 (more than two 1024-column spans per row in the four-pixel form) and an odd width (the scalar form)."""
    import torch
    rng = np.random.default_rng(12)
    for w, h in ((2100, 70), (67, 45), (1, 1)):
        img = rng.integers(0, 256, (3, h, w) if noc == 1 else (3, h, w, 3)).astype(np.uint8)
        xf = some_transforms(3, w, h, 13)
        xf[0] = (1, 0, 0.5, 0, 1, 0.25)
        for dt, tdt in ((np.uint8, torch.uint8), (f32, torch.float32)):
            same_bits(ctx.warp_affine(_dev(img), _dev(xf), out_dtype=tdt, want_valid=True), warp_affine_reference(img, xf, dt),
                      f"{w} x {h} noc {noc} {tdt}")


@pytest.mark.parametrize("which", ["out", "valid"])
def test_warp_affine_misaligned_pointers_take_the_scalar_form(ctx, which):
    """160 is a multiple of 4: the four-pixel form runs unless an output is off its vector alignment."""
    import torch
    import of_dis_amd as od
    w, h, noc, mk = CASES["160x120"]
    fr, fw, bw = fields(ctx, "160x120")
    xf = ctx.smooth_path(ctx.fit_motion(fw, bw, **FIT), (w, h), 2, 1.25)
    for tdt in (torch.uint8, torch.float32):
        want = ctx.warp_affine(fr, xf, out_dtype=tdt, want_valid=True)
        out = torch.full((want[0].numel() + 4,), 77, dtype=tdt, device="cuda")
        valid = torch.full((want[1].numel() + 4,), 77, dtype=torch.uint8, device="cuda")
        o0, v0 = (1 if which == "out" else 0), (1 if which == "valid" else 0)
        ctx.warp_affine_ptr(fr.data_ptr(), T, w, h, noc, xf.data_ptr(), od.IMG_F32 if tdt == torch.float32 else od.IMG_U8,
                            out[o0:].data_ptr(), valid[v0:].data_ptr(), torch.cuda.current_stream().cuda_stream)
        got = (out[o0:o0 + want[0].numel()].view(want[0].shape), valid[v0:v0 + want[1].numel()].view(want[1].shape))
        same_bits(got, want, f"{which} misaligned, {tdt}")
        assert (out[:o0] == 77).all() and (out[o0 + want[0].numel():] == 77).all()  # nothing outside the picture
        assert (valid[:v0] == 77).all() and (valid[v0 + want[1].numel():] == 77).all()


# --------------------------------------------------------------------------------------------- the fused call

STAB = dict(model=1, step=8, tau=2.0, iters=4, radius=2, zoom=1.25)


def composition(c, fr, fw, bw, size, fb, tdt, model, step, tau, iters, radius, zoom, alpha=0.01, beta=0.5):
    """(picture, valid, xform, corr, support) of the three primitives on full fields."""
    xform, support = c.fit_motion(fw, bw if fb else None, model, step, tau, iters, alpha, beta, want_support=True)
    corr = c.smooth_path(xform, size, radius, zoom)
    return c.warp_affine(fr, corr, out_dtype=tdt, want_valid=True) + (xform, corr, support)


@pytest.mark.parametrize("issue", list(ISSUES))
@pytest.mark.parametrize("case", list(CASES))
def test_run_sequence_stabilize_equals_its_composition(case, issue):
    import torch
    import of_dis_amd as od
    w, h, noc, mk = CASES[case]
    p = mk()
    fr = _dev(scene(w, h, noc))
    c = od.Context(0)
    try:
        for k, v in ISSUES[issue].items():
            c.set_option(k, v)
        fw, bw = c.run_sequence(fr, p, bidir=True)[:2]
        for fb in (False, True):
            what = f"{case} {issue} fb {fb}"
            for tdt in (torch.uint8, torch.float32):
                want = composition(c, fr, fw, bw, (w, h), fb, tdt, **STAB)
                got = c.run_sequence_stabilize(fr, p, fb=fb, out_dtype=tdt, want_valid=True, want_path=True, **STAB)
                same_bits(got, want, f"{what} {tdt}: fused == the primitives on the full fields")
                alone = c.run_sequence_stabilize(fr, p, fb=fb, out_dtype=tdt, **STAB)  # every optional output NULL
                same_bits((alone,), want[:1], f"{what} {tdt}: the picture alone")
            assert not torch.equal(want[0], fr.float().view(want[0].shape))  # (the frames move)
            # two frames: one pair
            two = c.run_sequence_stabilize(fr[:2], p, fb=fb, want_valid=True, want_path=True, **STAB)
            same_bits(two, composition(c, fr[:2], fw[:1], bw[:1], (w, h), fb, torch.uint8, **STAB), f"{what}: two frames")
            # the same pointers twice (the second call replays the captured graph), then other scalars (re-record)
            want8 = composition(c, fr, fw, bw, (w, h), fb, torch.uint8, **STAB)
            outs = [torch.empty_like(x) for x in want8]
            s = torch.cuda.current_stream().cuda_stream

            def call(alpha=0.01, beta=0.5, **kw):
                a = dict(STAB, **kw)
                for o in outs:
                    o.fill_(77)
                c.run_sequence_stabilize_ptr(fr.data_ptr(), T, w, h, p, a["model"], a["step"], a["tau"], a["iters"], a["radius"],
                                             a["zoom"], od.IMG_U8, *(o.data_ptr() for o in outs), fb, alpha, beta, s)
                return outs

            for rep in range(2):
                same_bits(call(), want8, f"{what}: call {rep} on fixed pointers")
            for kw in (dict(model=0), dict(step=16), dict(tau=0.5), dict(iters=1), dict(radius=0), dict(zoom=1.0)):
                other = composition(c, fr, fw, bw, (w, h), fb, torch.uint8, **dict(STAB, **kw))
                assert not torch.equal(other[3], want8[3]), kw
                same_bits(call(**kw), other, f"{what}: {kw} on the same pointers")
            same_bits(call(), want8, f"{what}: the first scalars again")
            if fb:  # other thresholds: other samples
                strict = composition(c, fr, fw, bw, (w, h), True, torch.uint8, alpha=0.0, beta=0.05, **STAB)
                assert not torch.equal(strict[4], want8[4])
                same_bits(call(0.0, 0.05), strict, f"{what}: alpha 0 beta 0.05 on the same pointers")
        # the plain sequence call on the same frames still returns its flow (the graph key)
        assert torch.equal(c.run_sequence(fr, p).view(torch.int32), fw.view(torch.int32)), f"{case} {issue}: run_sequence after the fused call"
    finally:
        c.close()


def test_constant_frames_stabilise_to_themselves(ctx):
    import torch
    import of_dis_amd as od
    ns = lattice(128, 96, 16)[0].size * lattice(128, 96, 16)[1].size
    for noc in (1, 3):
        fr = torch.full((4, 96, 128) if noc == 1 else (4, 96, 128, 3), 93, dtype=torch.uint8, device="cuda")
        p = od.oppoint(2, 128, od.MODE_OF, noc)
        for fb in (False, True):
            out, valid, xform, corr, support = ctx.run_sequence_stabilize(fr, p, fb=fb, radius=2, want_valid=True, want_path=True)
            assert torch.equal(out, fr) and (_np(valid) == 1).all()
            assert (_np(xform) == IDENTITY).all() and (_np(corr) == IDENTITY).all()
            assert (_np(support) == ns).all()  # zero flow: every sample counts, the solve succeeds


@pytest.mark.parametrize("case", ["160x120", "150x110-rgb"])
def test_failed_solves_leave_the_frames_alone(ctx, case):
    """The failed-solve branch inside the fused call: at step 128 the lattice of these frames is one sample, too few for
    a similarity, so every pair's transform is the identity with support 0 and the moving frames come back unchanged; a
    translation needs one sample only and succeeds."""
    import torch
    w, h, noc, mk = CASES[case]
    p = mk()
    fr, fw, bw = fields(ctx, case)
    assert lattice(w, h, 128)[0].size * lattice(w, h, 128)[1].size == 1
    for fb in (False, True):
        kw = dict(step=128, tau=2.0, iters=4, radius=2, zoom=1.0)
        got = ctx.run_sequence_stabilize(fr, p, model=1, fb=fb, want_valid=True, want_path=True, **kw)
        same_bits(got, composition(ctx, fr, fw, bw, (w, h), fb, torch.uint8, model=1, **kw), f"{case} fb {fb}: one sample, similarity")
        out, valid, xform, corr, support = got
        assert torch.equal(out, fr) and (_np(valid) == 1).all() and (_np(support) == 0).all()
        assert np.array_equal(bits(_np(xform)), bits(np.tile(IDENTITY, (T - 1, 1)))) and (_np(corr) == IDENTITY).all()
        wg = ctx.fit_motion(fw, bw if fb else None, 1, 128, want_weights=True, **FIT)[1]
        assert (_np(wg) == 0).all()
        got = ctx.run_sequence_stabilize(fr, p, model=0, fb=fb, want_valid=True, want_path=True, **kw)
        same_bits(got, composition(ctx, fr, fw, bw, (w, h), fb, torch.uint8, model=0, **kw), f"{case} fb {fb}: one sample, translation")
        if not fb:  # (with the check the one sample may be dropped)
            assert (_np(got[4]) == 1).all() and not torch.equal(got[0], fr)


# --------------------------------------------------------------------------------------------- timers, host form

def test_timers(ctx):
    import of_dis_amd as od
    w, h, noc, mk = CASES["160x120"]
    p = mk()
    fr, fw, bw = fields(ctx, "160x120")
    gf = ctx.run_sequence(fr, p, grid="level")
    names = od.kernel_names()

    def launches(call):
        before = {k: ctx.kernel_time(k)[1] for k in names}
        call()
        after = {k: ctx.kernel_time(k)[1] for k in names}
        return {k: after[k] - before[k] for k in names if after[k] != before[k]}

    def fused_only(ran):
        other = [k for k in ran if k.startswith("upsample") or k.startswith("fb_check") or k in ("fit_motion", "warp", "warp_level")]
        return not other and ran["fit_motion_level"] == 1 and ran["smooth_path"] == 1 and ran["warp_affine"] == 1

    ctx.enable_kernel_timing(True)
    try:
        ran = launches(lambda: ctx.run_sequence_stabilize(fr, p, **STAB))
        assert ran["level_out"] == 1 and ran["pyr_base"] == 1 and fused_only(ran), ran
        ran = launches(lambda: ctx.run_sequence_stabilize(fr, p, fb=True, **STAB))  # the check runs inside the fit
        assert ran["level_out"] == 2 and fused_only(ran), ran
        ctx.set_option("streams", 2)
        ctx.set_option("chunk", 2)
        ran = launches(lambda: ctx.run_sequence_stabilize(fr, p, fb=True, **STAB))  # chunks of 2, 2 and 1 pairs
        assert ran["level_out"] == 6 and ran["pyr_base"] == 3 and fused_only(ran), ran
        ctx.set_option("streams", 0)
        ctx.set_option("chunk", 0)
        xf = None

        def fit(a, **kw):
            nonlocal xf
            xf = ctx.fit_motion(a, **kw)
        assert launches(lambda: fit(fw, flow_bw=bw)) == {"fit_motion": 1}
        assert launches(lambda: fit(gf, grid="level", p=p, size=(w, h))) == {"fit_motion_level": 1}
        assert launches(lambda: ctx.smooth_path(xf, (w, h))) == {"smooth_path": 1}
        corr = ctx.smooth_path(xf, (w, h))
        assert launches(lambda: ctx.warp_affine(fr, corr)) == {"warp_affine": 1}
        for k in ("fit_motion", "fit_motion_level", "smooth_path", "warp_affine"):
            assert ctx.kernel_time(k)[0] > 0
    finally:
        ctx.set_option("streams", 0)
        ctx.set_option("chunk", 0)
        ctx.enable_kernel_timing(False)


@pytest.mark.parametrize("case", ["160x120", "150x110-rgb"])
def test_host_form(ctx, case):
    import torch
    w, h, noc, mk = CASES[case]
    p = mk()
    fr = scene(w, h, noc)
    for fb in (False, True):
        want = ctx.run_sequence_stabilize(_dev(fr), p, fb=fb, want_valid=True, want_path=True, **STAB)
        got = ctx.run_sequence_stabilize_host(fr, p, fb=fb, want_valid=True, want_path=True, **STAB)
        assert got[0].shape == fr.shape and got[1].shape == (T, h, w) and got[2].shape == (T - 1, 6) and got[3].shape == (T, 6)
        same_bits(got, want, f"{case}: host form, fb {fb}")
    wantf = ctx.run_sequence_stabilize(_dev(fr), p, out_dtype=torch.float32, **STAB)
    gotf = ctx.run_sequence_stabilize_host(fr, p, out_dtype=np.float32, **STAB)
    same_bits((gotf,), (wantf,), f"{case}: host form, float32")
    two = ctx.run_sequence_stabilize_host(fr[:2], p, want_path=True, **STAB)
    same_bits(two, ctx.run_sequence_stabilize(_dev(fr[:2]), p, want_path=True, **STAB), f"{case}: host form, two frames")


# --------------------------------------------------------------------------------------------- command lines

@pytest.mark.parametrize("exe,case,fb", [("run_OF_STAB_INT", "160x120", 1), ("run_OF_STAB_INT", "150x110", 0),
                                         ("run_OF_STAB_RGB", "150x110-rgb", 1)])
def test_cli_stabilize(ctx, tmp_path, exe, case, fb):
    import of_dis_amd as od
    w, h, noc, _ = CASES[case]
    fr = scene(w, h, noc)
    paths = _write_pngs(tmp_path, fr if noc == 3 else fr[..., None])
    ext = "pgm" if noc == 1 else "ppm"
    prefix = str(tmp_path / "out_")
    r = subprocess.run([os.path.join(ROOT, "of_dis_amd", "bin", exe), prefix, "2", "1.25", "2", str(fb)] + paths,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want, _, corr, _ = ctx.run_sequence_stabilize_host(fr, od.oppoint(2, w, od.MODE_OF, noc), fb=bool(fb), radius=2, zoom=1.25,
                                                       want_path=True)
    assert len(list(tmp_path.glob(f"out_*.{ext}"))) == T
    for i in range(T):
        got = od.read_image(f"{prefix}{i:06d}.{ext}", noc)
        assert np.array_equal(got[..., 0] if noc == 1 else got, want[i]), f"{exe} fb {fb} frame {i}"
    text = np.array([[float(v) for v in line.split()] for line in open(prefix + "path.txt")])
    assert text.shape == (T, 6) and np.array_equal(bits(text), bits(corr))  # %.17g round-trips a double
    assert not np.array_equal(want, fr)
    for bad in (["-1", "1.25", "2", "0"], ["257", "1", "2", "0"], ["2", "0.5", "2", "0"], ["2", "nan", "2", "0"],
                ["2", "1.25", "5", "0"], ["2", "1.25", "2", "2"]):
        r = subprocess.run([os.path.join(ROOT, "of_dis_amd", "bin", exe), str(tmp_path / "bad_")] + bad + paths,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "usage" in r.stderr and not list(tmp_path.glob("bad_*")), bad


# --------------------------------------------------------------------------------------------- refusals

def test_refusals_leave_the_context_usable(ctx):
    import torch
    import of_dis_amd as od
    L = od.lib()
    INV, UNS, OK = od._lib.ERR_INVALID_ARGUMENT, od._lib.ERR_UNSUPPORTED, od._lib.OK
    w, h, noc, mk = CASES["160x120"]
    p = mk()
    host = scene(w, h, noc, 4)
    fr = _dev(host)
    fw, bw = ctx.run_sequence(fr, p, bidir=True)[:2]
    gf = ctx.run_sequence(fr, p, grid="level")
    gb = ctx.run(fr[1:], fr[:-1], p, grid="level")
    g = od.out_geometry(p, w, h, grid="level")
    out = torch.full((4, h, w), 7, dtype=torch.uint8, device="cuda")
    xf = torch.full((3, 6), 7, dtype=torch.float64, device="cuda")
    corr = torch.full((4, 6), 7, dtype=torch.float64, device="cuda")
    plain = ctx.run_sequence_host(host, p)
    full = od.FlowView(0, 0, 0, w, h, 1, 0, 0)
    lvl = od.FlowView(0, 0, 1, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])

    def still_works(what):
        torch.cuda.synchronize()
        assert torch.all(out == 7) and torch.all(xf == 7) and torch.all(corr == 7), what  # nothing was enqueued
        got = ctx.run_sequence_host(host, p)
        assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), f"after the refusal of {what}"

    def fit(a=fw.data_ptr(), b=bw.data_ptr(), view=full, m=3, width=w, height=h, model=1, step=16, tau=2.0, iters=4,
            alpha=0.01, beta=0.5, x=xf.data_ptr()):
        return L.ofdis_fit_motion(ctx._h, a, b, None if view is None else C.byref(view), m, width, height, model, step, tau,
                                  iters, alpha, beta, x, None, None, None)

    def path(x=xf.data_ptr(), m=3, radius=2, zoom=1.0, width=w, height=h, c_=corr.data_ptr()):
        return L.ofdis_smooth_path(ctx._h, x, m, radius, zoom, width, height, c_, None)

    def warp(img=fr.data_ptr(), n=4, width=w, height=h, nc=1, x=corr.data_ptr(), dtype=0, o=out.data_ptr()):
        return L.ofdis_warp_affine_u8(ctx._h, img, n, width, height, nc, x, dtype, o, None, None)

    def fused(frames=fr.data_ptr(), nframes=4, params=p, width=w, height=h, model=1, step=16, tau=2.0, iters=4, use_fb=1,
              alpha=0.01, beta=0.5, radius=2, zoom=1.0, dtype=0, o=out.data_ptr()):
        return L.ofdis_run_sequence_stabilize_u8(ctx._h, frames, nframes, width, height, C.byref(params), model, step, tau,
                                                 iters, use_fb, alpha, beta, radius, zoom, dtype, o, None, xf.data_ptr(),
                                                 corr.data_ptr(), None, None)

    for call, name in ((fit, "fit_motion"), (fused, "run_sequence_stabilize")):
        assert call(model=2) == INV and call(model=-1) == INV
        assert call(step=0) == INV and call(step=-16) == INV and call(step=2 * h) == INV  # step / 2 > min(W, H) - 1
        for t in (float("nan"), float("inf"), 0.0, 1.0 / 2048, 65537.0, -2.0):
            assert call(tau=t) == INV, t
        assert call(iters=-1) == INV and call(iters=17) == INV
        assert call(width=0) == INV and call(height=-3) == INV
        assert call(alpha=-0.01) == INV and call(beta=float("nan")) == INV  # with the check: its threshold rules
        still_works(f"{name}: scalars")
    assert fit(step=1, width=w * 4, height=h * 4, view=od.FlowView(0, 0, 0, 4 * w, 4 * h, 1, 0, 0)) == INV  # 307 200 samples
    assert fit(a=None) == INV and fit(view=None) == INV and fit(x=None) == INV and fit(m=0) == INV
    assert fit(view=od.FlowView(2, 0, 0, w, h, 1, 0, 0)) == INV and fit(view=od.FlowView(0, 0, 3, w, h, 1, 0, 0)) == INV
    assert fit(a=gf.data_ptr(), b=gb.data_ptr(), view=od.FlowView(0, 0, 1, g["out_w"], g["out_h"], 3, 0, 0)) == INV
    assert fit(a=gf.data_ptr(), b=gb.data_ptr(), view=od.FlowView(0, 0, 1, g["out_w"] - 1, g["out_h"], g["cell"], g["off_x"], g["off_y"])) == INV
    for dt, lay in ((1, 0), (0, 1), (1, 1)):  # level grids: float32 interleaved alone
        assert fit(a=gf.data_ptr(), b=gb.data_ptr(), view=od.FlowView(dt, lay, 1, lvl.gw, lvl.gh, lvl.cell, lvl.off_x, lvl.off_y)) == UNS
    still_works("fit_motion: pointers and views")
    assert path(x=None) == INV and path(c_=None) == INV and path(m=0) == INV and path(radius=-1) == INV and path(radius=257) == INV
    for z in (float("nan"), float("inf"), 0.99, 16.5, -1.0):
        assert path(zoom=z) == INV and fused(zoom=z) == INV, z
    assert path(width=0) == INV and path(height=0) == INV and fused(radius=-1) == INV and fused(radius=257) == INV
    still_works("smooth_path")
    assert warp(img=None) == INV and warp(x=None) == INV and warp(o=None) == INV and warp(n=0) == INV and warp(nc=2) == INV
    assert warp(dtype=2) == INV and warp(width=0) == INV and fused(dtype=-1) == INV
    for call in (warp, fused):  # the picture over the frames: in place, and shifted by one frame either way
        assert call(o=fr.data_ptr()) == INV and call(o=fr.data_ptr() + w * h) == INV
    assert warp(img=out.data_ptr() + w * h) == INV and fused(frames=out.data_ptr() + w * h) == INV
    still_works("warp_affine")
    assert fused(nframes=1) == INV and fused(frames=None) == INV and fused(o=None) == INV
    assert fused(params=od.oppoint(2, w, od.MODE_DE, 1)) == UNS
    still_works("run_sequence_stabilize: frames, depth mode")
    tv = {p.sc_l: np.zeros((h >> p.sc_l, w >> p.sc_l, 2), f32)}
    ctx.set_capture(None, tv)
    try:
        assert fused() == UNS and fused(use_fb=0) == UNS
    finally:
        ctx.set_capture(None, None)
    still_works("run_sequence_stabilize: a stage capture")
    hp = L.ofdis_run_sequence_stabilize_u8_host
    out_h = np.zeros((4, h, w), np.uint8)
    tail = (out_h.ctypes.data, None, None, None, None)
    assert hp(ctx._h, host.ctypes.data, 1, w, h, C.byref(p), 1, 16, 2.0, 4, 0, 0.01, 0.5, 2, 1.0, 0, *tail) == INV
    assert hp(ctx._h, host.ctypes.data, 4, w, h, C.byref(p), 1, 16, float("nan"), 4, 0, 0.01, 0.5, 2, 1.0, 0, *tail) == INV
    assert hp(ctx._h, host.ctypes.data, 4, w, h, C.byref(p), 1, 16, 2.0, 4, 0, 0.01, 0.5, 2, 1.0, 3, *tail) == INV
    assert hp(ctx._h, host.ctypes.data, 4, w, h, C.byref(p), 1, 16, 2.0, 4, 0, 0.01, 0.5, 2, 1.0, 0, None, None, None, None, None) == INV
    still_works("the host form")
    assert fit(b=None, alpha=-1.0, beta=float("nan")) == OK  # without the check the thresholds are ignored
    same_bits((xf,), (ctx.fit_motion(fw),), "after the refusals: the fit")
    assert path() == OK and warp() == OK
    want = ctx.warp_affine(fr, ctx.smooth_path(ctx.fit_motion(fw), (w, h), 2, 1.0))
    same_bits((out,), (want,), "after the refusals: path and warp")
    assert fused(use_fb=0, alpha=-1.0, beta=float("nan")) == OK
    same_bits((out,), (want,), "after the refusals: the fused call")
    assert fused() == OK and fit(a=gf.data_ptr(), b=gb.data_ptr(), view=lvl) == OK
    same_bits((xf,), (ctx.fit_motion(fw, bw),), "after the refusals: the level view with the check")

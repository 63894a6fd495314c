"""The temporal filter over a radius on the device: ofdis_tfilter_radius_u8 against test_tfilter_radius.py's numpy
restatement, bit for bit, in every flow format; the level-grid view against the full field; radius 1 against the
radius-1 filter with and without the check's masks; the fused call ofdis_run_sequence_tfilter_radius_u8 against its
definition -- tfilter_radius on the fields of run_sequence -- in every issue form; timers, host form, command lines,
refusals.

The scene, the noise and the sizes are test_gpu_tfilter.py's: 6 frames of a drifting background crossed by a patch of
another texture, Gaussian noise of sigma 4, filter sigma 12.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_sequence import _write_pngs
from test_gpu_tfilter import SIGMA, assert_pictures, fields, video
from test_gpu_track import CASES, T
from test_gpu_warp import ISSUES, _dev, _np
from test_tfilter_radius import tfilter_radius_reference

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ["160x120", "150x110", "150x110-rgb"]  # the four-pixel form, the scalar form (150 % 4 != 0), colour
USED_SHARE = 0.062  # see test_every_used_bit_is_set_and_clear


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


def level_grids(ctx, case):
    """The case's forward and backward level grids and their parameters."""
    w, h, noc, mk = CASES[case]
    p = mk()
    fr = fields(ctx, case)[0]
    return ctx.run_sequence(fr, p, grid="level"), ctx.run(fr[1:], fr[:-1], p, grid="level"), p


# --------------------------------------------------------------------------------------------- the primitive

@pytest.mark.parametrize("case", SIZES)
def test_tfilter_radius_equals_the_restatement(ctx, case):
    import torch
    w, h, noc, mk = CASES[case]
    fr, fw, bw = fields(ctx, case)[:3]
    frames = video(w, h, noc)
    nfw, nbw = _np(fw), _np(bw)
    for half in (False, True):
        ra, rb = (nfw.astype(np.float16), nbw.astype(np.float16)) if half else (nfw, nbw)
        for radius in (1, 2, 4):
            for fb in (False, True):
                want = {dt: tfilter_radius_reference(frames, ra, rb, SIGMA, radius, fb, out_dtype=dt) for dt in (np.uint8, f32)}
                codes = set(want[np.uint8][1].ravel().tolist())
                assert len(codes) >= (4 if radius == 1 else 12), sorted(codes)  # chains end in many ways
                for layout in ("nhwc", "nchw"):
                    a, b = (fw.half(), bw.half()) if half else (fw, bw)
                    if layout == "nchw":
                        a, b = a.permute(0, 3, 1, 2).contiguous(), b.permute(0, 3, 1, 2).contiguous()
                    for dt, tdt in ((np.uint8, torch.uint8), (f32, torch.float32)):
                        what = f"{case} {'f16' if half else 'f32'} {layout} R {radius} fb {fb} out {np.dtype(dt).name}"
                        got = ctx.tfilter_radius(fr, a, b, SIGMA, radius, fb, out_dtype=tdt, want_used=True, layout=layout)
                        assert_pictures(got, want[dt], what)
                        alone = ctx.tfilter_radius(fr, a, b, SIGMA, radius, fb, out_dtype=tdt, layout=layout)  # used NULL
                        assert_pictures((alone, got[1]), want[dt], what + ", no `used`")


def test_every_used_bit_is_set_and_clear(ctx):
    """160 x 120, R = 2, the check on, frames 2..3 (the frames with four neighbours).  Measured with the restatement on
    the CPU, on the oracle's flows of the same video (the device's flows are the oracle's bit for bit): the shares of
    the pixels on which bit 0 / 1 / 2 / 3 is set are 0.8755 / 0.8595 / 0.8057 / 0.7979, clear 0.1245 / 0.1405 / 0.1943 /
    0.2021 (without the check: set on 0.9115 / 0.8995 / 0.8643 / 0.8462); the smallest share is 0.1245 and the bound is
    half of it, 0.062."""
    fr, fw, bw = fields(ctx, "160x120")[:3]
    _, used = ctx.tfilter_radius(fr, fw, bw, SIGMA, 2, True, want_used=True)
    u = _np(used)[2:T - 2]
    sets = [float(((u >> b) & 1).mean()) for b in range(4)]
    print("160x120 R 2 fb: bits set on " + " / ".join(f"{s:.4f}" for s in sets))
    assert (u >> 4 == 0).all()
    for s in sets:
        assert s >= USED_SHARE and 1.0 - s >= USED_SHARE, sets


def test_level_view_equals_full_field(ctx):
    import torch
    for case in SIZES:
        w, h, noc, mk = CASES[case]
        fr, fw, bw = fields(ctx, case)[:3]
        gf, gb, p = level_grids(ctx, case)
        for radius in (1, 2, 4):
            for fb in (False, True):
                for tdt in (torch.uint8, torch.float32):
                    want = ctx.tfilter_radius(fr, fw, bw, SIGMA, radius, fb, out_dtype=tdt, want_used=True)
                    got = ctx.tfilter_radius(fr, gf, gb, SIGMA, radius, fb, out_dtype=tdt, want_used=True, grid="level", p=p,
                                             size=(w, h))
                    assert_pictures(got, want, f"{case}: level view, R {radius} fb {fb} {tdt}")
        for fb in (False, True):
            two = ctx.tfilter_radius(fr[:2], gf[:1], gb[:1], SIGMA, 3, fb, want_used=True, grid="level", p=p)
            assert_pictures(two, ctx.tfilter_radius(fr[:2], fw[:1], bw[:1], SIGMA, 3, fb, want_used=True),
                            f"{case}: level view, two frames, fb {fb}")


# (the level form reads cells one by one: no alignment rule for its grids)
@pytest.mark.parametrize("which,level", [("flow", False)] + [(x, lv) for x in ("out", "used", "frames") for lv in (False, True)])
def test_misaligned_pointers_take_the_scalar_form(ctx, which, level):
    """160 is a multiple of 4: the four-pixel form runs unless a pointer is off its vector alignment."""
    import torch
    import of_dis_amd as od
    case = "160x120"
    w, h, noc, mk = CASES[case]
    fr, fw, bw = fields(ctx, case)[:3]

    def shifted(t, elems):
        """A copy of t that starts `elems` elements into a fresh allocation."""
        flat = torch.empty(t.numel() + elems, dtype=t.dtype, device="cuda")
        sub = flat[elems:].view(t.shape)
        sub.copy_(t)
        return sub

    for tdt in (torch.uint8, torch.float32):
        want = ctx.tfilter_radius(fr, fw, bw, SIGMA, 3, True, out_dtype=tdt, want_used=True)
        frames, a, b = fr, fw, bw
        if level:
            a, b, p = level_grids(ctx, case)
            g = od.out_geometry(p, w, h, grid="level")
            view = od.FlowView(0, 0, 1, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])
        else:
            view = od.FlowView(0, 0, 0, w, h, 1, 0, 0)
        if which == "flow":
            a, b = shifted(a, 1), shifted(b, 2)  # 4 and 8 bytes off 16
        if which == "frames":
            frames = shifted(fr, 1)
        out = torch.full((want[0].numel() + 4,), 77, dtype=tdt, device="cuda")
        used = torch.full((want[1].numel() + 4,), 77, dtype=torch.uint8, device="cuda")
        o0 = 1 if which == "out" else 0
        u0 = 1 if which == "used" else 0
        ctx.tfilter_radius_ptr(frames.data_ptr(), T, a.data_ptr(), b.data_ptr(), view, w, h, noc, 3, SIGMA,
                               od.IMG_F32 if tdt == torch.float32 else od.IMG_U8, out[o0:].data_ptr(), used[u0:].data_ptr(),
                               True, 0.01, 0.5, torch.cuda.current_stream().cuda_stream)
        got = (out[o0:o0 + want[0].numel()].view(want[0].shape), used[u0:u0 + want[1].numel()].view(want[1].shape))
        assert_pictures(got, want, f"{which} misaligned, level {level}, {tdt}")
        torch.cuda.synchronize()
        assert (out[:o0] == 77).all() and (out[o0 + want[0].numel():] == 77).all()  # nothing outside the picture
        assert (used[:u0] == 77).all() and (used[u0 + want[1].numel():] == 77).all()


def test_radius_1_equals_the_old_calls(ctx):
    import torch
    for case in SIZES:
        w, h, noc, mk = CASES[case]
        fr, fw, bw, ofw, obw = fields(ctx, case)
        gf, gb, p = level_grids(ctx, case)
        strict = ctx.run_sequence(fr, p, bidir=True, alpha=0.0, beta=0.05)[2:4]
        for tdt in (torch.uint8, torch.float32):
            for lv in (False, True):
                a, b, kw = (gf, gb, dict(grid="level", p=p)) if lv else (fw, bw, {})
                what = f"{case} {tdt} level {lv}"
                want = ctx.tfilter(fr, a, b, SIGMA, out_dtype=tdt, want_used=True, **kw)
                assert_pictures(ctx.tfilter_radius(fr, a, b, SIGMA, 1, out_dtype=tdt, want_used=True, **kw), want,
                                what + ": without masks")
                want = ctx.tfilter(fr, a, b, SIGMA, ofw, obw, out_dtype=tdt, want_used=True, **kw)
                assert_pictures(ctx.tfilter_radius(fr, a, b, SIGMA, 1, True, out_dtype=tdt, want_used=True, **kw), want,
                                what + ": run_sequence's masks")
                want = ctx.tfilter(fr, a, b, SIGMA, *strict, out_dtype=tdt, want_used=True, **kw)
                assert_pictures(ctx.tfilter_radius(fr, a, b, SIGMA, 1, True, 0.0, 0.05, out_dtype=tdt, want_used=True, **kw),
                                want, what + ": masks at alpha 0, beta 0.05")


# --------------------------------------------------------------------------------------------- the fused call

@pytest.mark.parametrize("issue", list(ISSUES))
@pytest.mark.parametrize("case", SIZES)
def test_run_sequence_tfilter_radius_equals_its_composition(case, issue):
    import torch
    import of_dis_amd as od
    w, h, noc, mk = CASES[case]
    p = mk()
    fr = _dev(video(w, h, noc))
    what = f"{case} {issue}"
    c = od.Context(0)
    try:
        for k, v in ISSUES[issue].items():
            c.set_option(k, v)
        fw, bw = c.run_sequence(fr, p, bidir=True)[:2]
        for radius in (2, 4):
            for fb in (False, True):
                for tdt in (torch.uint8, torch.float32):
                    want = c.tfilter_radius(fr, fw, bw, SIGMA, radius, fb, out_dtype=tdt, want_used=True)
                    got = c.run_sequence_tfilter_radius(fr, p, SIGMA, radius, fb, out_dtype=tdt, want_used=True)
                    assert_pictures(got, want, f"{what} R {radius} fb {fb} {tdt}: fused == tfilter_radius on the full fields")
                    alone = c.run_sequence_tfilter_radius(fr, p, SIGMA, radius, fb, out_dtype=tdt)
                    assert_pictures((alone, got[1]), want, f"{what} R {radius} fb {fb} {tdt}: no `used`")
        for fb in (False, True):
            # two frames: one pair, one neighbour each
            two = c.run_sequence_tfilter_radius(fr[:2], p, SIGMA, 2, fb, want_used=True)
            assert_pictures(two, c.tfilter_radius(fr[:2], fw[:1], bw[:1], SIGMA, 2, fb, want_used=True), f"{what} fb {fb}: two frames")
            # the same pointers twice (the second call replays the captured graph), then another radius, another sigma
            # and, with the check, other thresholds (each records anew)
            out = torch.empty(fr.shape, dtype=torch.uint8, device="cuda")
            used = torch.empty((T, h, w), dtype=torch.uint8, device="cuda")
            s = torch.cuda.current_stream().cuda_stream

            def call(radius, sigma, alpha=0.01, beta=0.5):
                out.fill_(77)
                used.fill_(77)
                c.run_sequence_tfilter_radius_ptr(fr.data_ptr(), T, w, h, p, radius, sigma, od.IMG_U8, out.data_ptr(),
                                                  used.data_ptr(), fb, alpha, beta, s)
                return out, used

            want2 = c.tfilter_radius(fr, fw, bw, SIGMA, 2, fb, want_used=True)
            for rep in range(2):
                assert_pictures(call(2, SIGMA), want2, f"{what} fb {fb}: call {rep} on fixed pointers")
            want3 = c.tfilter_radius(fr, fw, bw, SIGMA, 3, fb, want_used=True)
            assert not torch.equal(want3[1], want2[1])
            assert_pictures(call(3, SIGMA), want3, f"{what} fb {fb}: radius 3 on the same pointers")
            wide = c.tfilter_radius(fr, fw, bw, 40.0, 3, fb, want_used=True)
            assert not torch.equal(wide[0], want3[0])
            assert_pictures(call(3, 40.0), wide, f"{what} fb {fb}: sigma 40 on the same pointers")
            assert_pictures(call(2, SIGMA), want2, f"{what} fb {fb}: the first radius and sigma again")
            if fb:
                strict = c.tfilter_radius(fr, fw, bw, SIGMA, 2, True, 0.0, 0.05, want_used=True)
                assert not torch.equal(strict[1], want2[1])
                assert_pictures(call(2, SIGMA, 0.0, 0.05), strict, f"{what}: alpha 0 beta 0.05 on the same pointers")
        # another call kind on the same frames never replays this call's graph, nor this call the other's
        old = c.run_sequence_tfilter(fr, p, SIGMA, want_used=True)
        assert_pictures(old, c.tfilter(fr, fw, bw, SIGMA, want_used=True), f"{what}: run_sequence_tfilter after the fused call")
        one = c.run_sequence_tfilter_radius(fr, p, SIGMA, 1, want_used=True)
        assert_pictures(one, old, f"{what}: radius 1 after run_sequence_tfilter")
        assert torch.equal(c.run_sequence(fr, p).view(torch.int32), fw.view(torch.int32)), f"{what}: run_sequence after the fused call"
    finally:
        c.close()


# --------------------------------------------------------------------------------------------- timers, host form

def test_timers(ctx):
    import of_dis_amd as od
    w, h, noc, mk = CASES["160x120"]
    fr, fw, bw = fields(ctx, "160x120")[:3]
    gf, gb, p = level_grids(ctx, "160x120")
    names = od.kernel_names()

    def launches(call):
        before = {k: ctx.kernel_time(k)[1] for k in names}
        call()
        after = {k: ctx.kernel_time(k)[1] for k in names}
        return {k: after[k] - before[k] for k in names if after[k] != before[k]}

    def fused_only(ran):
        other = [k for k in ran if k.startswith("upsample") or k.startswith("fb_check")
                 or (k.startswith("tfilter") and k != "tfilter_radius_level")]
        return not other and ran["tfilter_radius_level"] == 1

    ctx.enable_kernel_timing(True)
    try:
        for fb in (False, True):
            ran = launches(lambda: ctx.run_sequence_tfilter_radius(fr, p, SIGMA, 3, fb))
            assert ran["level_out"] == 2 and ran["pyr_base"] == 1 and fused_only(ran), ran
        ctx.set_option("streams", 2)
        ctx.set_option("chunk", 2)
        ran = launches(lambda: ctx.run_sequence_tfilter_radius(fr, p, SIGMA, 3, True))  # chunks of 2, 2 and 1 pairs
        assert ran["level_out"] == 6 and ran["pyr_base"] == 3 and fused_only(ran), ran
        ctx.set_option("streams", 0)
        ctx.set_option("chunk", 0)
        ran = launches(lambda: ctx.tfilter_radius(fr, fw, bw, SIGMA, 2, True))
        assert ran == {"tfilter_radius": 1}, ran
        ran = launches(lambda: ctx.tfilter_radius(fr, gf, gb, SIGMA, 2, True, grid="level", p=p))
        assert ran == {"tfilter_radius_level": 1}, ran
    finally:
        ctx.set_option("streams", 0)
        ctx.set_option("chunk", 0)
        ctx.enable_kernel_timing(False)


@pytest.mark.parametrize("case", ["160x120", "150x110-rgb"])
def test_host_form(ctx, case):
    import torch
    w, h, noc, mk = CASES[case]
    p = mk()
    fr = video(w, h, noc)
    for radius, fb in ((2, False), (4, True)):
        want = ctx.run_sequence_tfilter_radius(_dev(fr), p, SIGMA, radius, fb, want_used=True)
        got = ctx.run_sequence_tfilter_radius_host(fr, p, SIGMA, radius, fb, want_used=True)
        assert got[0].shape == fr.shape and got[1].shape == (T, h, w)
        assert_pictures(got, want, f"{case}: host form, R {radius} fb {fb}")
    wantf = ctx.run_sequence_tfilter_radius(_dev(fr), p, SIGMA, 2, out_dtype=torch.float32)
    gotf = ctx.run_sequence_tfilter_radius_host(fr, p, SIGMA, 2, out_dtype=np.float32)
    assert np.array_equal(gotf.view(np.uint32), _np(wantf).view(np.uint32))
    two = ctx.run_sequence_tfilter_radius_host(fr[:2], p, SIGMA, 2, want_used=True)
    assert_pictures(two, ctx.run_sequence_tfilter_radius(_dev(fr[:2]), p, SIGMA, 2, want_used=True), f"{case}: host form, two frames")


# --------------------------------------------------------------------------------------------- command lines

@pytest.mark.parametrize("exe,case,radius,fb", [("run_OF_TFILTER_R_INT", "160x120", 2, 1), ("run_OF_TFILTER_R_RGB", "150x110-rgb", 3, 0)])
def test_cli_tfilter_radius(ctx, tmp_path, exe, case, radius, fb):
    import of_dis_amd as od
    w, h, noc, _ = CASES[case]
    fr = video(w, h, noc)
    paths = _write_pngs(tmp_path, fr if noc == 3 else fr[..., None])
    ext = "pgm" if noc == 1 else "ppm"
    prefix = str(tmp_path / "out_")
    r = subprocess.run([os.path.join(ROOT, "of_dis_amd", "bin", exe), prefix, str(radius), "12", "2", str(fb)] + paths,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    p = od.oppoint(2, w, od.MODE_OF, noc)
    want = ctx.run_sequence_tfilter_radius_host(fr, p, SIGMA, radius, bool(fb))
    assert len(list(tmp_path.glob(f"out_*.{ext}"))) == T
    for i in range(T):
        got = od.read_image(f"{prefix}{i:06d}.{ext}", noc)
        assert np.array_equal(got[..., 0] if noc == 1 else got, want[i]), f"{exe} R {radius} fb {fb} frame {i}"
    assert not np.array_equal(want, ctx.run_sequence_tfilter_radius_host(fr, p, SIGMA, 1, bool(fb)))  # (the radius shows)
    for bad in (["0", "12", "2", "0"], ["5", "12", "2", "0"], ["2", "nan", "2", "0"], ["2", "12", "5", "0"], ["2", "12", "2", "2"]):
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
    host = video(w, h, noc, 4)
    fr = _dev(host)
    fw, bw = ctx.run_sequence(fr, p, bidir=True)[:2]
    gf = ctx.run_sequence(fr, p, grid="level")
    gb = ctx.run(fr[1:], fr[:-1], p, grid="level")
    g = od.out_geometry(p, w, h, grid="level")
    out = torch.full((4, h, w), 7, dtype=torch.uint8, device="cuda")
    used = torch.full((4, h, w), 7, dtype=torch.uint8, device="cuda")
    plain = ctx.run_sequence_host(host, p)
    full = od.FlowView(0, 0, 0, w, h, 1, 0, 0)
    lvl = od.FlowView(0, 0, 1, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])

    def still_works(what):
        torch.cuda.synchronize()
        assert torch.all(out == 7) and torch.all(used == 7), what  # nothing was enqueued by the refused call
        got = ctx.run_sequence_host(host, p)
        assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), f"after the refusal of {what}"

    def prim(frames=fr.data_ptr(), nframes=4, a=fw.data_ptr(), b=bw.data_ptr(), view=full, width=w, height=h, nc=1,
             radius=2, sigma=SIGMA, use_fb=1, alpha=0.01, beta=0.5, dtype=0, o=out.data_ptr()):
        return L.ofdis_tfilter_radius_u8(ctx._h, frames, nframes, a, b, None if view is None else C.byref(view), width,
                                         height, nc, radius, sigma, use_fb, alpha, beta, dtype, o, used.data_ptr(), None)

    def fused(frames=fr.data_ptr(), nframes=4, params=p, width=w, height=h, radius=2, sigma=SIGMA, use_fb=1, alpha=0.01,
              beta=0.5, dtype=0, o=out.data_ptr()):
        return L.ofdis_run_sequence_tfilter_radius_u8(ctx._h, frames, nframes, width, height, C.byref(params), radius,
                                                      sigma, use_fb, alpha, beta, dtype, o, used.data_ptr(), None)

    for call, name in ((prim, "tfilter_radius"), (fused, "run_sequence_tfilter_radius")):
        for r in (0, 5, -1, 1 << 20):
            assert call(radius=r) == INV and call(radius=r, use_fb=0) == INV, r
        still_works(f"{name}: radius out of range")
        assert call(alpha=-0.01) == INV and call(beta=-0.5) == INV and call(alpha=float("nan")) == INV and call(beta=float("inf")) == INV
        still_works(f"{name}: bad thresholds with use_fb")
        assert call(nframes=1) == INV and call(nframes=0) == INV and call(nframes=-2) == INV
        still_works(f"{name}: nframes < 2")
        assert call(frames=None) == INV and call(o=None) == INV
        still_works(f"{name}: NULL frames / out")
        for s in (float("nan"), float("inf"), 0.0, 1.0 / 2048, 65537.0, -12.0):
            assert call(sigma=s) == INV, s
        still_works(f"{name}: sigma")
        assert call(dtype=2) == INV and call(dtype=-1) == INV
        still_works(f"{name}: out_dtype")
        assert call(width=0) == INV and call(height=-3) == INV
        still_works(f"{name}: sizes")
        # the picture over the frames: in place, and shifted by one frame either way
        assert call(o=fr.data_ptr()) == INV and call(o=fr.data_ptr() + w * h) == INV
        assert call(frames=out.data_ptr() + w * h) == INV
        still_works(f"{name}: out overlapping frames")
    assert prim(a=None) == INV and prim(b=None) == INV and prim(view=None) == INV and prim(nc=2) == INV
    still_works("tfilter_radius: NULL flows / view, noc")
    assert prim(view=od.FlowView(2, 0, 0, w, h, 1, 0, 0)) == INV and prim(view=od.FlowView(0, 0, 3, w, h, 1, 0, 0)) == INV
    assert prim(a=gf.data_ptr(), b=gb.data_ptr(), view=od.FlowView(0, 0, 1, g["out_w"] - 1, g["out_h"], g["cell"], g["off_x"], g["off_y"])) == INV
    still_works("tfilter_radius: views")
    for dt, lay in ((1, 0), (0, 1), (1, 1)):  # level grids: float32 interleaved alone
        assert prim(a=gf.data_ptr(), b=gb.data_ptr(), view=od.FlowView(dt, lay, 1, lvl.gw, lvl.gh, lvl.cell, lvl.off_x, lvl.off_y)) == UNS
    still_works("tfilter_radius: a level view of another format")
    assert fused(params=od.oppoint(2, w, od.MODE_DE, 1)) == UNS
    still_works("run_sequence_tfilter_radius: depth mode")
    tv = {p.sc_l: np.zeros((h >> p.sc_l, w >> p.sc_l, 2), f32)}
    ctx.set_capture(None, tv)
    try:
        assert fused() == UNS and fused(use_fb=0) == UNS
    finally:
        ctx.set_capture(None, None)
    still_works("run_sequence_tfilter_radius: a stage capture")
    hp = L.ofdis_run_sequence_tfilter_radius_u8_host
    out_h = np.zeros((4, h, w), np.uint8)
    assert hp(ctx._h, host.ctypes.data, 1, w, h, C.byref(p), 2, SIGMA, 0, 0.01, 0.5, 0, out_h.ctypes.data, None) == INV
    assert hp(ctx._h, host.ctypes.data, 4, w, h, C.byref(p), 5, SIGMA, 0, 0.01, 0.5, 0, out_h.ctypes.data, None) == INV
    assert hp(ctx._h, host.ctypes.data, 4, w, h, C.byref(p), 2, float("nan"), 0, 0.01, 0.5, 0, out_h.ctypes.data, None) == INV
    assert hp(ctx._h, host.ctypes.data, 4, w, h, C.byref(p), 2, SIGMA, 0, 0.01, 0.5, 3, out_h.ctypes.data, None) == INV
    assert hp(ctx._h, host.ctypes.data, 4, w, h, C.byref(p), 2, SIGMA, 0, 0.01, 0.5, 0, None, None) == INV
    still_works("the host form")
    assert fused(use_fb=0, alpha=-1.0, beta=float("nan")) == OK  # without the check the thresholds are ignored
    assert_pictures((out, used), ctx.tfilter_radius(fr, fw, bw, SIGMA, 2, want_used=True), "after the refusals: without the check")
    assert fused() == OK
    want = ctx.tfilter_radius(fr, fw, bw, SIGMA, 2, True, want_used=True)
    assert_pictures((out, used), want, "after the refusals: with the check")
    out.fill_(7)
    assert prim(a=gf.data_ptr(), b=gb.data_ptr(), view=lvl) == OK
    assert_pictures((out, used), want, "after the refusals: the primitive on level grids")

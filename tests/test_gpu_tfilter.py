"""The temporal filter on the device: ofdis_tfilter_u8 against test_tfilter.py's numpy restatement, bit for bit, in
every flow format; the level-grid view against the full field; the fused call ofdis_run_sequence_tfilter_u8 against its
definition -- tfilter on the fields of run_sequence -- in every issue form; timers, host form, command lines, refusals.

The scene is test_gpu_track.py's -- a textured background that drifts by (1.5, -0.75) per frame and a 41 x 41 patch of
another texture that crosses it by (-6, 4) per frame, 6 frames -- with seeded Gaussian noise of sigma 4, clipped to u8.
With the filter's sigma = 12 the occluder's surroundings drop one neighbour or both, so every `used` code occurs.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_sequence import _write_pngs
from test_gpu_track import CASES, T, scene
from test_gpu_warp import ISSUES, _dev, _np
from test_tfilter import tfilter_reference

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA = 12.0
SHARE = 0.01  # of the pixels of frames 1..4 of the 160 x 120 grey case, each `used` code, with and without masks

_videos = {}


def video(w, h, noc, nfr=T):
    """The noisy scene: u8 [nfr, h, w] or [nfr, h, w, 3]."""
    key = (w, h, noc, nfr)
    if key not in _videos:
        clean = scene(w, h, noc, nfr).astype(np.float64)
        rng = np.random.default_rng(11)
        _videos[key] = np.clip(np.rint(clean + rng.normal(0.0, 4.0, clean.shape)), 0, 255).astype(np.uint8)
    return _videos[key]


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


_fields = {}


def fields(ctx, case):
    """The case's frames and run_sequence(bidir=True)'s four outputs, computed once: torch tensors."""
    if case not in _fields:
        w, h, noc, mk = CASES[case]
        fr = _dev(video(w, h, noc))
        _fields[case] = (fr,) + tuple(ctx.run_sequence(fr, mk(), bidir=True)[:4])
    return _fields[case]


def assert_pictures(got, want, what):
    """(picture, used) pairs of numpy arrays or torch tensors; float32 pictures compared as uint32."""
    gp, gu = (x if isinstance(x, np.ndarray) else _np(x) for x in got)
    wp, wu = (x if isinstance(x, np.ndarray) else _np(x) for x in want)
    assert gp.dtype == wp.dtype and gp.shape == wp.shape, what
    if gp.dtype == f32:
        gp, wp = gp.view(np.uint32), wp.view(np.uint32)
    bad = gp != wp
    assert not bad.any(), f"{what}: {int(bad.sum())} picture values differ, first at {tuple(np.argwhere(bad)[0])}"
    assert np.array_equal(gu, wu), f"{what}: {int((gu != wu).sum())} `used` bytes differ"


def shares(used):
    u = (used if isinstance(used, np.ndarray) else _np(used))[1:T - 1]
    return [float((u == k).mean()) for k in range(4)]


# --------------------------------------------------------------------------------------------- the primitive

def test_every_used_code_occurs(ctx):
    fr, fw, bw, ofw, obw = fields(ctx, "160x120")
    for masks in ((None, None), (ofw, obw)):
        _, used = ctx.tfilter(fr, fw, bw, SIGMA, *masks, want_used=True)
        sh = shares(used)
        print(f"160x120 {'with' if masks[0] is not None else 'without'} masks: used 0 / 1 / 2 / 3 on "
              + " / ".join(f"{s:.3f}" for s in sh))
        assert min(sh) >= SHARE, sh


@pytest.mark.parametrize("case", list(CASES))
def test_tfilter_equals_the_restatement(ctx, case):
    import torch
    w, h, noc, mk = CASES[case]
    fr, fw, bw, ofw, obw = fields(ctx, case)
    frames = video(w, h, noc)
    nfw, nbw, nofw, nobw = (_np(x) for x in (fw, bw, ofw, obw))
    want = {}
    for half in (False, True):
        a, b = (nfw.astype(np.float16), nbw.astype(np.float16)) if half else (nfw, nbw)
        for mk_ in ("none", "both", "fw", "bw"):
            occ = (nofw if mk_ in ("both", "fw") else None, nobw if mk_ in ("both", "bw") else None)
            for dt in (np.uint8, f32):
                want[half, mk_, dt] = tfilter_reference(frames, a, b, SIGMA, *occ, out_dtype=dt)
    if case == "160x120":
        for mk_ in ("none", "both"):
            assert min(shares(want[False, mk_, np.uint8][1])) >= SHARE
    else:
        assert len(set(want[False, "none", np.uint8][1].ravel().tolist())) == 4
    for half in (False, True):
        for layout in ("nhwc", "nchw"):
            a, b = (fw.half(), bw.half()) if half else (fw, bw)
            if layout == "nchw":
                a, b = a.permute(0, 3, 1, 2).contiguous(), b.permute(0, 3, 1, 2).contiguous()
            for mk_ in ("none", "both", "fw", "bw"):
                occ = (ofw if mk_ in ("both", "fw") else None, obw if mk_ in ("both", "bw") else None)
                for dt, tdt in ((np.uint8, torch.uint8), (f32, torch.float32)):
                    what = f"{case} {'f16' if half else 'f32'} {layout} masks {mk_} out {np.dtype(dt).name}"
                    got = ctx.tfilter(fr, a, b, SIGMA, *occ, out_dtype=tdt, want_used=True, layout=layout)
                    assert_pictures(got, want[half, mk_, dt], what)
                    alone = ctx.tfilter(fr, a, b, SIGMA, *occ, out_dtype=tdt, layout=layout)  # used NULL
                    assert_pictures((alone, got[1]), want[half, mk_, dt], what + ", no `used`")


def test_tfilter_level_view_equals_full_field(ctx):
    import torch
    for case in CASES:
        w, h, noc, mk = CASES[case]
        p = mk()
        fr, fw, bw, ofw, obw = fields(ctx, case)
        gf = ctx.run_sequence(fr, p, grid="level")
        gb = ctx.run(fr[1:], fr[:-1], p, grid="level")
        for occ in ((None, None), (ofw, obw), (None, obw)):
            for tdt in (torch.uint8, torch.float32):
                want = ctx.tfilter(fr, fw, bw, SIGMA, *occ, out_dtype=tdt, want_used=True)
                got = ctx.tfilter(fr, gf, gb, SIGMA, *occ, out_dtype=tdt, want_used=True, grid="level", p=p, size=(w, h))
                assert_pictures(got, want, f"{case}: level view, masks {[o is not None for o in occ]}, {tdt}")
        two = ctx.tfilter(fr[:2], gf[:1], gb[:1], SIGMA, want_used=True, grid="level", p=p)
        assert_pictures(two, ctx.tfilter(fr[:2], fw[:1], bw[:1], SIGMA, want_used=True), f"{case}: level view, two frames")


# (the level form reads cells one by one: no alignment rule for its grids)
@pytest.mark.parametrize("which,level", [("flow", False)] + [(x, lv) for x in ("out", "used", "frames", "occ") for lv in (False, True)])
def test_tfilter_misaligned_pointers_take_the_scalar_form(ctx, which, level):
    """160 is a multiple of 4: the four-pixel form runs unless a pointer is off its vector alignment."""
    import torch
    import of_dis_amd as od
    case = "160x120"
    w, h, noc, mk = CASES[case]
    p = mk()
    fr, fw, bw, ofw, obw = fields(ctx, case)

    def shifted(t, elems):
        """A copy of t that starts `elems` elements into a fresh allocation."""
        flat = torch.empty(t.numel() + elems, dtype=t.dtype, device="cuda")
        sub = flat[elems:].view(t.shape)
        sub.copy_(t)
        return sub

    for tdt in (torch.uint8, torch.float32):
        want = ctx.tfilter(fr, fw, bw, SIGMA, ofw, obw, out_dtype=tdt, want_used=True)
        frames, a, b, of_, ob_ = fr, fw, bw, ofw, obw
        if level:
            a, b = ctx.run_sequence(fr, p, grid="level"), ctx.run(fr[1:], fr[:-1], p, grid="level")
            g = od.out_geometry(p, w, h, grid="level")
            view = od.FlowView(0, 0, 1, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])
        else:
            view = od.FlowView(0, 0, 0, w, h, 1, 0, 0)
        if which == "flow":
            a, b = shifted(a, 1), shifted(b, 2)  # 4 and 8 bytes off 16
        if which == "frames":
            frames = shifted(fr, 1)
        if which == "occ":
            of_, ob_ = shifted(ofw, 3), shifted(obw, 2)
        out = torch.full((want[0].numel() + 4,), 77, dtype=tdt, device="cuda")
        used = torch.full((want[1].numel() + 4,), 77, dtype=torch.uint8, device="cuda")
        o0 = 1 if which == "out" else 0
        u0 = 1 if which == "used" else 0
        ctx.tfilter_ptr(frames.data_ptr(), T, a.data_ptr(), b.data_ptr(), view, w, h, noc, SIGMA,
                        od.IMG_F32 if tdt == torch.float32 else od.IMG_U8, out[o0:].data_ptr(), used[u0:].data_ptr(),
                        of_.data_ptr(), ob_.data_ptr(), torch.cuda.current_stream().cuda_stream)
        got = (out[o0:o0 + want[0].numel()].view(want[0].shape), used[u0:u0 + want[1].numel()].view(want[1].shape))
        assert_pictures(got, want, f"{which} misaligned, level {level}, {tdt}")
        torch.cuda.synchronize()
        assert (out[:o0] == 77).all() and (out[o0 + want[0].numel():] == 77).all()  # nothing outside the picture
        assert (used[:u0] == 77).all() and (used[u0 + want[1].numel():] == 77).all()


# --------------------------------------------------------------------------------------------- the fused call

@pytest.mark.parametrize("issue", list(ISSUES))
@pytest.mark.parametrize("case", list(CASES))
def test_run_sequence_tfilter_equals_tfilter_of_run_sequence(case, issue):
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
        fw, bw, ofw, obw = c.run_sequence(fr, p, bidir=True)[:4]
        for occ in (False, True):
            masks = (ofw, obw) if occ else (None, None)
            for tdt in (torch.uint8, torch.float32):
                want = c.tfilter(fr, fw, bw, SIGMA, *masks, out_dtype=tdt, want_used=True)
                got = c.run_sequence_tfilter(fr, p, SIGMA, occ=occ, out_dtype=tdt, want_used=True)
                assert_pictures(got, want, f"{what} occ {occ} {tdt}: fused == tfilter on the full fields")
                alone = c.run_sequence_tfilter(fr, p, SIGMA, occ=occ, out_dtype=tdt)
                assert_pictures((alone, got[1]), want, f"{what} occ {occ} {tdt}: no `used`")
            sh = shares(want[1])
            print(f"{what} occ {occ}: used 0 / 1 / 2 / 3 on " + " / ".join(f"{s:.3f}" for s in sh))
            if case == "160x120":
                assert min(sh) >= SHARE, sh
            else:
                assert min(sh) > 0.0, sh
            # two frames: one pair, one neighbour each
            two = c.run_sequence_tfilter(fr[:2], p, SIGMA, occ=occ, want_used=True)
            m2 = (ofw[:1], obw[:1]) if occ else (None, None)
            assert_pictures(two, c.tfilter(fr[:2], fw[:1], bw[:1], SIGMA, *m2, want_used=True), f"{what} occ {occ}: two frames")
            # the same pointers twice (the second call replays the captured graph), then another sigma (re-record)
            out = torch.empty_like(want[0], dtype=torch.uint8)
            used = torch.empty_like(want[1])
            s = torch.cuda.current_stream().cuda_stream

            def call(sigma, alpha=0.01, beta=0.5):
                out.fill_(77)
                used.fill_(77)
                c.run_sequence_tfilter_ptr(fr.data_ptr(), T, w, h, p, sigma, od.IMG_U8, out.data_ptr(), used.data_ptr(),
                                           occ, alpha, beta, s)
                return out, used

            want8 = c.tfilter(fr, fw, bw, SIGMA, *masks, want_used=True)
            for rep in range(2):
                assert_pictures(call(SIGMA), want8, f"{what} occ {occ}: call {rep} on fixed pointers")
            wide = c.tfilter(fr, fw, bw, 40.0, *masks, want_used=True)
            assert not torch.equal(wide[0], want8[0])
            assert_pictures(call(40.0), wide, f"{what} occ {occ}: sigma 40 on the same pointers")
            assert_pictures(call(SIGMA), want8, f"{what} occ {occ}: the first sigma again")
            if occ:  # other thresholds: other masks
                o2 = c.run_sequence(fr, p, bidir=True, alpha=0.0, beta=0.05)[2:4]
                strict = c.tfilter(fr, fw, bw, SIGMA, *o2, want_used=True)
                assert not torch.equal(strict[1], want8[1])
                assert_pictures(call(SIGMA, 0.0, 0.05), strict, f"{what}: alpha 0 beta 0.05 on the same pointers")
        # the plain sequence call on the same frames still returns its flow (the graph key)
        assert torch.equal(c.run_sequence(fr, p).view(torch.int32), fw.view(torch.int32)), f"{what}: run_sequence after the fused call"
    finally:
        c.close()


# --------------------------------------------------------------------------------------------- timers, host form

def test_timers(ctx):
    import of_dis_amd as od
    w, h, noc, mk = CASES["160x120"]
    p = mk()
    fr, fw, bw, ofw, obw = fields(ctx, "160x120")
    gf = ctx.run_sequence(fr, p, grid="level")
    gb = ctx.run(fr[1:], fr[:-1], p, grid="level")
    names = od.kernel_names()

    def launches(call):
        before = {k: ctx.kernel_time(k)[1] for k in names}
        call()
        after = {k: ctx.kernel_time(k)[1] for k in names}
        return {k: after[k] - before[k] for k in names if after[k] != before[k]}

    def fused_only(ran, checks):
        other = [k for k in ran if k.startswith("upsample") or (k.startswith("fb_check") and k != "fb_check_level")]
        return not other and "tfilter" not in ran and ran.get("fb_check_level", 0) == checks

    ctx.enable_kernel_timing(True)
    try:
        ran = launches(lambda: ctx.run_sequence_tfilter(fr, p, SIGMA))
        assert ran["tfilter_level"] == 1 and ran["level_out"] == 2 and ran["pyr_base"] == 1 and fused_only(ran, 0), ran
        ran = launches(lambda: ctx.run_sequence_tfilter(fr, p, SIGMA, occ=True))
        assert ran["tfilter_level"] == 1 and ran["level_out"] == 2 and fused_only(ran, 1), ran
        ctx.set_option("streams", 2)
        ctx.set_option("chunk", 2)
        ran = launches(lambda: ctx.run_sequence_tfilter(fr, p, SIGMA, occ=True))  # chunks of 2, 2 and 1 pairs
        assert ran["tfilter_level"] == 1 and ran["level_out"] == 6 and ran["pyr_base"] == 3 and fused_only(ran, 3), ran
        ctx.set_option("streams", 0)
        ctx.set_option("chunk", 0)
        ran = launches(lambda: ctx.tfilter(fr, fw, bw, SIGMA, ofw, obw))
        assert ran == {"tfilter": 1}, ran
        ran = launches(lambda: ctx.tfilter(fr, gf, gb, SIGMA, grid="level", p=p))
        assert ran == {"tfilter_level": 1}, ran
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
    for occ in (False, True):
        want = ctx.run_sequence_tfilter(_dev(fr), p, SIGMA, occ=occ, want_used=True)
        got = ctx.run_sequence_tfilter_host(fr, p, SIGMA, occ=occ, want_used=True)
        assert got[0].shape == fr.shape and got[1].shape == (T, h, w)
        assert_pictures(got, want, f"{case}: host form, occ {occ}")
    wantf = ctx.run_sequence_tfilter(_dev(fr), p, SIGMA, out_dtype=torch.float32)
    gotf = ctx.run_sequence_tfilter_host(fr, p, SIGMA, out_dtype=np.float32)
    assert np.array_equal(gotf.view(np.uint32), _np(wantf).view(np.uint32))
    two = ctx.run_sequence_tfilter_host(fr[:2], p, SIGMA, want_used=True)
    assert_pictures(two, ctx.run_sequence_tfilter(_dev(fr[:2]), p, SIGMA, want_used=True), f"{case}: host form, two frames")


# --------------------------------------------------------------------------------------------- command lines

@pytest.mark.parametrize("exe,case,occ", [("run_OF_TFILTER_INT", "160x120", 1), ("run_OF_TFILTER_INT", "150x110", 0),
                                          ("run_OF_TFILTER_RGB", "150x110-rgb", 1)])
def test_cli_tfilter(ctx, tmp_path, exe, case, occ):
    import of_dis_amd as od
    w, h, noc, _ = CASES[case]
    fr = video(w, h, noc)
    paths = _write_pngs(tmp_path, fr if noc == 3 else fr[..., None])
    ext = "pgm" if noc == 1 else "ppm"
    prefix = str(tmp_path / "out_")
    r = subprocess.run([os.path.join(ROOT, "of_dis_amd", "bin", exe), prefix, "12", "2", str(occ)] + paths,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = ctx.run_sequence_tfilter_host(fr, od.oppoint(2, w, od.MODE_OF, noc), SIGMA, occ=bool(occ))
    assert len(list(tmp_path.glob(f"out_*.{ext}"))) == T
    for i in range(T):
        got = od.read_image(f"{prefix}{i:06d}.{ext}", noc)
        assert np.array_equal(got[..., 0] if noc == 1 else got, want[i]), f"{exe} occ {occ} frame {i}"
    assert not np.array_equal(want, fr)  # (the filter changes the frames)
    for bad in (["nan", "2", "0"], ["0", "2", "0"], ["12", "5", "0"], ["12", "2", "2"]):
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
    fw, bw, ofw, obw = ctx.run_sequence(fr, p, bidir=True)[:4]
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
             sigma=SIGMA, dtype=0, o=out.data_ptr()):
        return L.ofdis_tfilter_u8(ctx._h, frames, nframes, a, b, None if view is None else C.byref(view), width, height,
                                  nc, sigma, ofw.data_ptr(), None, dtype, o, used.data_ptr(), None)

    def fused(frames=fr.data_ptr(), nframes=4, params=p, width=w, height=h, sigma=SIGMA, use_occ=1, alpha=0.01, beta=0.5,
              dtype=0, o=out.data_ptr()):
        return L.ofdis_run_sequence_tfilter_u8(ctx._h, frames, nframes, width, height, C.byref(params), sigma, use_occ,
                                               alpha, beta, dtype, o, used.data_ptr(), None)

    for call, name in ((prim, "tfilter"), (fused, "run_sequence_tfilter")):
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
    still_works("tfilter: NULL flows / view, noc")
    assert prim(view=od.FlowView(2, 0, 0, w, h, 1, 0, 0)) == INV and prim(view=od.FlowView(0, 0, 3, w, h, 1, 0, 0)) == INV
    assert prim(a=gf.data_ptr(), b=gb.data_ptr(), view=od.FlowView(0, 0, 1, g["out_w"], g["out_h"], 3, 0, 0)) == INV
    assert prim(a=gf.data_ptr(), b=gb.data_ptr(), view=od.FlowView(0, 0, 1, g["out_w"] - 1, g["out_h"], g["cell"], g["off_x"], g["off_y"])) == INV
    still_works("tfilter: views")
    for dt, lay in ((1, 0), (0, 1), (1, 1)):  # level grids: float32 interleaved alone
        assert prim(a=gf.data_ptr(), b=gb.data_ptr(), view=od.FlowView(dt, lay, 1, lvl.gw, lvl.gh, lvl.cell, lvl.off_x, lvl.off_y)) == UNS
    still_works("tfilter: a level view of another format")
    assert fused(params=od.oppoint(2, w, od.MODE_DE, 1)) == UNS
    still_works("run_sequence_tfilter: depth mode")
    tv = {p.sc_l: np.zeros((h >> p.sc_l, w >> p.sc_l, 2), f32)}
    ctx.set_capture(None, tv)
    try:
        assert fused() == UNS and fused(use_occ=0) == UNS
    finally:
        ctx.set_capture(None, None)
    still_works("run_sequence_tfilter: a stage capture")
    assert fused(alpha=-0.01) == INV and fused(beta=-0.5) == INV and fused(alpha=float("nan")) == INV and fused(beta=float("inf")) == INV
    still_works("run_sequence_tfilter: bad thresholds")
    hp = L.ofdis_run_sequence_tfilter_u8_host
    out_h = np.zeros((4, h, w), np.uint8)
    assert hp(ctx._h, host.ctypes.data, 1, w, h, C.byref(p), SIGMA, 0, 0.01, 0.5, 0, out_h.ctypes.data, None) == INV
    assert hp(ctx._h, host.ctypes.data, 4, w, h, C.byref(p), float("nan"), 0, 0.01, 0.5, 0, out_h.ctypes.data, None) == INV
    assert hp(ctx._h, host.ctypes.data, 4, w, h, C.byref(p), SIGMA, 0, 0.01, 0.5, 3, out_h.ctypes.data, None) == INV
    assert hp(ctx._h, host.ctypes.data, 4, w, h, C.byref(p), SIGMA, 0, 0.01, 0.5, 0, None, None) == INV
    still_works("the host form")
    assert fused(use_occ=0, alpha=-1.0, beta=float("nan")) == OK  # without masks the thresholds are ignored
    want = ctx.tfilter(fr, fw, bw, SIGMA, want_used=True)
    assert_pictures((out, used), want, "after the refusals: without masks")
    assert fused() == OK
    assert_pictures((out, used), ctx.tfilter(fr, fw, bw, SIGMA, ofw, obw, want_used=True), "after the refusals: with masks")
    assert prim(a=gf.data_ptr(), b=gb.data_ptr(), view=lvl) == OK
    assert_pictures((out, used), ctx.tfilter(fr, fw, bw, SIGMA, ofw, None, want_used=True), "after the refusals: the primitive")

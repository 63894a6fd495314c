"""The fused tracking call (ofdis_run_sequence_track_u8) against its definition: track_points on the fields of
run_sequence, bit for bit -- on full-resolution fields and on level grids, in every issue form -- plus its timers, host
form, command lines and refusals.

The scene has an occluder, so that all three outcomes occur: a textured background that drifts by (1.5, -0.75) per
frame and a 41 x 41 patch of another texture that crosses it by (-6, 4) per frame.  Measured with the oracle and
test_track.py's numpy restatement at 160 x 120, 6 frames, the 4-pixel grid of points: final status 0 / 1 / 2 for
0.668 / 0.250 / 0.082 of the points.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_sequence import _write_pngs
from test_gpu_warp import ISSUES, _dev, _np, explicit, op2
from test_interp import _texture
from test_track import assert_tracks_equal

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 6  # frames: 5 pairs, so chunks of 2 pairs are three chunks on two lanes

# name: (W, H, noc, parameters); the level grid's geometry in the comment
CASES = {
    "160x120": (160, 120, 1, lambda: op2(160)),          # cell 2, no padding
    "150x110": (150, 110, 1, lambda: op2(150)),          # cell 1, offsets 1 / 1
    "161x121": (161, 121, 1, lambda: op2(161)),          # cell 2, offsets 3 / 3
    "150x110-rgb": (150, 110, 3, lambda: op2(150, 3)),   # as 150x110
    "176x96-l2": (176, 96, 1, lambda: explicit(3, 2)),   # cell 4
}
SHARE = 0.02  # of the final entries, each of the three outcomes on the 160 x 120 grey case (measured: 0.668 / 0.250 / 0.082)

_scenes = {}


def scene(w, h, noc, nfr=T):
    """u8 [nfr, h, w] or [nfr, h, w, 3]"""
    key = (w, h, noc, nfr)
    if key not in _scenes:
        y, x = np.mgrid[0:h, 0:w].astype(np.float64)
        frames = []
        for j in range(nfr):
            cx, cy = 100 - 6 * j, 30 + 4 * j
            box = (np.abs(x - cx) <= 20) & (np.abs(y - cy) <= 20)
            chans = []
            for k in ((0,) if noc == 1 else (0, 1, 2)):
                bg = _texture(x - 1.5 * j, y + 0.75 * j, k)
                fg = _texture(1.7 * (x - cx) + 40, 1.3 * (y - cy) + 10, 2)
                chans.append(np.rint(np.where(box, fg, bg)).astype(np.uint8))
            frames.append(chans[0] if noc == 1 else np.stack(chans, -1))
        _scenes[key] = np.stack(frames)
    return _scenes[key]


def grid_points(w, h):
    import of_dis_amd as od
    return od.pixel_grid(w, h, 4)


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


def same(got, want, what):
    assert_tracks_equal((_np(got[0]), _np(got[1])), (_np(want[0]), _np(want[1])), what)


def shares(status):
    last = _np(status)[-1]
    return [float((last == k).mean()) for k in (0, 1, 2)]


# --------------------------------------------------------------------------------------------- the definition

@pytest.mark.parametrize("issue", list(ISSUES))
@pytest.mark.parametrize("case", list(CASES))
def test_run_sequence_track_equals_track_of_run_sequence(case, issue):
    import torch
    import of_dis_amd as od
    w, h, noc, mk = CASES[case]
    p = mk()
    fr = _dev(scene(w, h, noc))
    pts = _dev(grid_points(w, h))
    n = pts.shape[0]
    what = f"{case} {issue}"
    c = od.Context(0)
    try:
        for k, v in ISSUES[issue].items():
            c.set_option(k, v)
        fw, bw = c.run_sequence(fr, p, bidir=True)[:2]
        want = c.track_points(fw, pts, bw)
        got = c.run_sequence_track(fr, p, pts)
        same(got, want, f"{what}: fused == track_points on the full fields")
        gf = c.run_sequence(fr, p, grid="level")
        gb = c.run(fr[1:], fr[:-1], p, grid="level")
        same(c.track_points(gf, pts, gb, grid="level", p=p, size=(w, h)), want, f"{what}: track_points on the level grids")
        # forward only
        fwd = c.run_sequence_track(fr, p, pts, fb=False)
        same(fwd, c.track_points(c.run_sequence(fr, p), pts), f"{what}: fb=False")
        assert torch.equal(fwd[0].view(torch.int32), got[0].view(torch.int32)), f"{what}: positions depend on fb"
        assert not (_np(fwd[1]) == 1).any()
        # last_only
        last = c.run_sequence_track(fr, p, pts, last_only=True)
        same(last, (want[0][-1], want[1][-1]), f"{what}: last_only")
        # all outcomes occur
        sh = shares(want[1])
        print(f"{what}: final status shares 0 / 1 / 2 = {sh[0]:.3f} / {sh[1]:.3f} / {sh[2]:.3f}")
        if case == "160x120":
            assert min(sh) >= SHARE, sh
        else:
            assert max(sh) < 1.0, sh
        # the same pointers twice (the second call replays the captured graph), then new point values, thresholds
        pbuf = pts.clone()
        tr = torch.empty((T, n, 2), dtype=torch.float32, device="cuda")
        st = torch.empty((T, n), dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream().cuda_stream

        def call(alpha=0.01, beta=0.5):
            tr.fill_(77)
            st.fill_(77)
            c.run_sequence_track_ptr(fr.data_ptr(), T, w, h, p, pbuf.data_ptr(), n, 0, True, alpha, beta, 0,
                                     tr.data_ptr(), st.data_ptr(), s)
            return tr, st

        for rep in range(2):
            same(call(), want, f"{what}: call {rep} on fixed pointers")
        pbuf += torch.tensor([0.375, 1.25], device="cuda")
        moved = c.track_points(fw, pbuf, bw)
        same(call(), moved, f"{what}: new point values at the same pointer")
        assert not torch.equal(moved[0], want[0])
        for alpha, beta in ((1.0, 0.5), (0.01, 0.0)):  # far more lenient, far stricter
            other = c.track_points(fw, pbuf, bw, alpha=alpha, beta=beta)
            same(call(alpha, beta), other, f"{what}: alpha {alpha} beta {beta}")
            assert not torch.equal(other[1], moved[1]), f"{what}: alpha {alpha} beta {beta} changes no status"
        same(call(), moved, f"{what}: the first thresholds again")
        # the plain sequence call on the same frames still returns its flow (the graph key)
        assert torch.equal(c.run_sequence(fr, p).view(torch.int32), fw.view(torch.int32)), f"{what}: run_sequence after the fused call"
    finally:
        c.close()


def test_start_and_single_outputs(ctx):
    import torch
    import of_dis_amd as od
    w, h, noc, mk = CASES["161x121"]
    p = mk()
    fr = _dev(scene(w, h, noc))
    pts = _dev(grid_points(w, h))
    n = pts.shape[0]
    start = _dev(np.resize(np.array([-3, 0, 1, 3, T - 1, T + 4], np.int32), n))
    fw, bw = ctx.run_sequence(fr, p, bidir=True)[:2]
    want = ctx.track_points(fw, pts, bw, start=start)
    assert (_np(want[1]) == 3).any()
    same(ctx.run_sequence_track(fr, p, pts, start=start), want, "start")
    s = torch.cuda.current_stream().cuda_stream
    tr = torch.full((T, n, 2), 5.0, dtype=torch.float32, device="cuda")
    st = torch.full((T, n), 5, dtype=torch.uint8, device="cuda")
    ctx.run_sequence_track_ptr(fr.data_ptr(), T, w, h, p, pts.data_ptr(), n, start.data_ptr(), True, 0.01, 0.5, 0,
                               tr.data_ptr(), 0, s)
    ctx.run_sequence_track_ptr(fr.data_ptr(), T, w, h, p, pts.data_ptr(), n, start.data_ptr(), True, 0.01, 0.5, 0,
                               0, st.data_ptr(), s)
    same((tr, st), want, "each output alone")
    ctx.run_sequence_track_ptr(fr.data_ptr(), T, w, h, p, pts.data_ptr(), n, 0, True, 0.01, 0.5, 0, 0, 0, s)  # nothing to do


# --------------------------------------------------------------------------------------------- timers, host form

def test_timers(ctx):
    import of_dis_amd as od
    w, h, noc, mk = CASES["160x120"]
    p = mk()
    fr = _dev(scene(w, h, noc))
    pts = _dev(grid_points(w, h))
    names = od.kernel_names()

    def launches(call):
        before = {k: ctx.kernel_time(k)[1] for k in names}
        call()
        after = {k: ctx.kernel_time(k)[1] for k in names}
        return {k: after[k] - before[k] for k in names if after[k] != before[k]}

    def only_level(ran):
        return not [k for k in ran if k.startswith("upsample") or k.startswith("fb_check")] and "track" not in ran

    ctx.enable_kernel_timing(True)
    try:
        ran = launches(lambda: ctx.run_sequence_track(fr, p, pts))
        assert ran["track_level"] == 1 and ran["level_out"] == 2 and ran["pyr_base"] == 1 and only_level(ran), ran
        ran = launches(lambda: ctx.run_sequence_track(fr, p, pts, fb=False))
        assert ran["track_level"] == 1 and ran["level_out"] == 1 and only_level(ran), ran
        ctx.set_option("streams", 2)
        ctx.set_option("chunk", 2)
        ran = launches(lambda: ctx.run_sequence_track(fr, p, pts))  # chunks of 2, 2 and 1 pairs
        assert ran["track_level"] == 1 and ran["level_out"] == 6 and ran["pyr_base"] == 3 and only_level(ran), ran
        ran = launches(lambda: ctx.run_sequence_track(fr, p, pts, fb=False))
        assert ran["track_level"] == 1 and ran["level_out"] == 3 and only_level(ran), ran
        ctx.set_option("streams", 0)
        ctx.set_option("chunk", 0)
        fw, bw = ctx.run_sequence(fr, p, bidir=True)[:2]
        ran = launches(lambda: ctx.track_points(fw, pts, bw))
        assert ran == {"track": 1}, ran
    finally:
        ctx.set_option("streams", 0)
        ctx.set_option("chunk", 0)
        ctx.enable_kernel_timing(False)


@pytest.mark.parametrize("case", ["160x120", "150x110-rgb"])
def test_host_form(ctx, case):
    w, h, noc, mk = CASES[case]
    p = mk()
    fr = scene(w, h, noc)
    pts = grid_points(w, h)
    start = np.resize(np.array([0, 0, 2, 9], np.int32), len(pts))
    want = ctx.run_sequence_track(_dev(fr), p, _dev(pts), start=_dev(start))
    got = ctx.run_sequence_track_host(fr, p, pts, start=start)
    assert got[0].shape == (T, len(pts), 2) and got[1].shape == (T, len(pts))
    assert_tracks_equal(got, (_np(want[0]), _np(want[1])), f"{case}: host form")
    last = ctx.run_sequence_track_host(fr, p, pts, fb=False, last_only=True)
    fwd = ctx.run_sequence_track(_dev(fr), p, _dev(pts), fb=False)
    assert last[0].shape == (len(pts), 2)
    assert_tracks_equal(last, (_np(fwd[0])[-1], _np(fwd[1])[-1]), f"{case}: host form, forward only, last")
    two = ctx.run_sequence_track_host(fr[:2], p, pts)  # a 2-frame video: one pair
    one = ctx.run_sequence_track(_dev(fr[:2]), p, _dev(pts))
    assert two[0].shape == (2, len(pts), 2)
    assert_tracks_equal(two, (_np(one[0]), _np(one[1])), f"{case}: host form, two frames")
    fw, bw = ctx.run_bidir(_dev(fr[:1]), _dev(fr[1:2]), p)[:2]
    same(one, ctx.track_points(fw, _dev(pts), bw), f"{case}: two frames == the pair's two flows")


# --------------------------------------------------------------------------------------------- command lines

@pytest.mark.parametrize("exe,case,fb", [("run_OF_TRACK_INT", "160x120", 1), ("run_OF_TRACK_INT", "150x110", 0),
                                         ("run_OF_TRACK_RGB", "150x110-rgb", 1)])
def test_cli_track(ctx, tmp_path, exe, case, fb):
    import of_dis_amd as od
    w, h, noc, _ = CASES[case]
    fr = scene(w, h, noc)
    paths = _write_pngs(tmp_path, fr if noc == 3 else fr[..., None])
    pts = grid_points(w, h)[::7].copy()
    pts += np.array([0.3, 0.125], f32)
    start = np.resize(np.array([0, 1, 0, 7], np.int32), len(pts))
    lines = ["# x y [start]"] + [f"{x!r} {y!r}" + (f" {s}" if s else "") for (x, y), s in zip(pts.tolist(), start.tolist())]
    (tmp_path / "points.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([os.path.join(ROOT, "of_dis_amd", "bin", exe), str(tmp_path / "points.txt"),
                        str(tmp_path / "tracks.txt"), "2", str(fb)] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    rows = [ln.split() for ln in (tmp_path / "tracks.txt").read_text().splitlines()]
    n = len(pts)
    assert len(rows) == T * n and all(len(row) == 5 for row in rows)
    assert [(int(row[0]), int(row[1])) for row in rows] == [(k, j) for j in range(T) for k in range(n)]  # frame-major
    tr = np.array([[float(row[2]), float(row[3])] for row in rows], f32).reshape(T, n, 2)  # %.9g round-trips float32
    st = np.array([int(row[4]) for row in rows], np.uint8).reshape(T, n)
    want = ctx.run_sequence_track_host(fr, od.oppoint(2, w, od.MODE_OF, noc), pts, start=start, fb=bool(fb))
    assert_tracks_equal((tr, st), want, f"{exe} {case} fb {fb}")
    assert (st == 3).any() and len(set(st[-1].tolist())) > 1
    # an unreadable points file, a malformed line
    r = subprocess.run([os.path.join(ROOT, "of_dis_amd", "bin", exe), str(tmp_path / "none.txt"),
                        str(tmp_path / "t2.txt"), "2", str(fb)] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "cannot read points file" in r.stderr and not (tmp_path / "t2.txt").exists()
    (tmp_path / "bad.txt").write_text("1 2\n3 x\n")
    r = subprocess.run([os.path.join(ROOT, "of_dis_amd", "bin", exe), str(tmp_path / "bad.txt"),
                        str(tmp_path / "t2.txt"), "2", str(fb)] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "bad.txt:2" in r.stderr and not (tmp_path / "t2.txt").exists()


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
    pts = _dev(grid_points(w, h))
    n = pts.shape[0]
    st = torch.full((4 * n,), 7, dtype=torch.uint8, device="cuda")
    plain = ctx.run_sequence_host(host, p)

    def call(nframes=4, params=p, frames=fr.data_ptr(), points=pts.data_ptr(), npts=n, use_fb=1, alpha=0.01, beta=0.5,
             flags=0, width=w, height=h):
        return L.ofdis_run_sequence_track_u8(ctx._h, frames, nframes, width, height, C.byref(params), points, None, npts,
                                             use_fb, alpha, beta, flags, None, st.data_ptr(), None)

    def still_works(what):
        torch.cuda.synchronize()
        assert torch.all(st == 7), what  # nothing was enqueued by the refused call
        got = ctx.run_sequence_host(host, p)
        assert np.array_equal(got.view(np.uint32), plain.view(np.uint32)), f"after the refusal of {what}"

    assert call(params=od.oppoint(2, w, od.MODE_DE, 1)) == UNS
    still_works("depth mode")
    tv = {p.sc_l: np.zeros((h >> p.sc_l, w >> p.sc_l, 2), f32)}
    ctx.set_capture(None, tv)
    try:
        assert call() == UNS and call(use_fb=0) == UNS
    finally:
        ctx.set_capture(None, None)
    still_works("a stage capture")
    assert call(nframes=1) == INV and call(nframes=0) == INV and call(nframes=-2) == INV
    still_works("nframes < 2")
    assert call(points=None) == INV and call(frames=None) == INV and call(npts=0) == INV
    still_works("NULL points")
    assert call(alpha=-0.01) == INV and call(beta=-0.5) == INV and call(alpha=float("nan")) == INV and call(beta=float("inf")) == INV
    still_works("bad thresholds")
    assert call(flags=2) == INV and call(flags=-1) == INV
    still_works("an unknown flag")
    assert call(width=0) == INV and call(height=-3) == INV
    still_works("sizes")
    hp = od.lib().ofdis_run_sequence_track_u8_host
    tr_h, st_h = np.zeros((4, n, 2), f32), np.zeros((4, n), np.uint8)
    pts_h = grid_points(w, h)
    assert hp(ctx._h, host.ctypes.data, 1, w, h, C.byref(p), pts_h.ctypes.data, None, n, 1, 0.01, 0.5, 0, tr_h.ctypes.data,
              st_h.ctypes.data) == INV
    assert hp(ctx._h, host.ctypes.data, 4, w, h, C.byref(p), None, None, n, 1, 0.01, 0.5, 0, tr_h.ctypes.data,
              st_h.ctypes.data) == INV
    assert hp(ctx._h, host.ctypes.data, 4, w, h, C.byref(p), pts_h.ctypes.data, None, n, 1, 0.01, 0.5, 4, tr_h.ctypes.data,
              st_h.ctypes.data) == INV
    still_works("the host form")
    assert call(use_fb=0, alpha=-1.0, beta=float("nan")) == OK  # without the backward fields the thresholds are ignored
    torch.cuda.synchronize()
    want = ctx.run_sequence_track(fr, p, pts, fb=False)
    assert np.array_equal(_np(st).reshape(4, n), _np(want[1]))
    assert call() == OK
    torch.cuda.synchronize()
    assert np.array_equal(_np(st).reshape(4, n), _np(ctx.run_sequence_track(fr, p, pts)[1]))

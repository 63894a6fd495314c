"""The fused interpolation with occlusion masks and the sequence interpolation (ofdis_run_interp_occ_u8,
ofdis_run_sequence_interp_u8, run_OF_SEQ_INTERP_INT / _RGB).

Every comparison is on raw bits.  run_interp(occ=True) must give interp(a, b, the four outputs of run_bidir) and
run_bidir's masks; run_sequence_interp(frames) must give run_interp on the two slices of the frames.  ofdis_interp_u8
itself is pinned to the numpy reference by test_interp.py, the masks to theirs by test_fb_check.py.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_interp import CASES, FB_CASE, MATRIX
from test_gpu_sequence import _write_pngs, sequence
from test_gpu_warp import ISSUES, _dev, _np, assert_same_pictures, op2, pairs
from test_warp import assert_picture

pytestmark = pytest.mark.gpu

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


def assert_same_results(got, want, what):
    """Tuples of torch tensors of one length (pictures, valid[, occ_fw, occ_bw])."""
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert_picture(_np(g), _np(w), f"{what} (output {k})")


# --------------------------------------------------------------------------------------------- the pair call with masks

@pytest.mark.parametrize("case,issue", MATRIX, ids=[f"{c}-{i}" for c, i in MATRIX])
def test_run_interp_occ_equals_interp_of_run_bidir(case, issue):
    import torch
    import of_dis_amd as od
    w, h, noc, op, n = CASES[case]
    p = od.oppoint(op, w, od.MODE_OF, noc)
    if case == FB_CASE:
        p = p.copy(usefbcon=1)
    a, b = (_dev(x) for x in pairs(w, h, noc, n))
    c = od.Context(0)
    try:
        for k, v in ISSUES[issue].items():
            c.set_option(k, v)
        bidir = c.run_bidir(a, b, p)
        fw, bw, ofw, obw = bidir
        flow = c.run(a, b, p)
        level = c.run(a, b, p, grid="level")
        warped = c.run_warp(a, b, p, want_valid=True)
        for t, out_dtype in (((0.5,), torch.uint8), ((0.25, 0.5, 0.75), torch.float32)):
            want = c.interp(a, b, fw, bw, t, occ_fw=ofw, occ_bw=obw, out_dtype=out_dtype, want_valid=True) + (ofw, obw)
            first = c.run_interp(a, b, p, t, out_dtype, want_valid=True, occ=True, want_occ=True)
            second = c.run_interp(a, b, p, t, out_dtype, want_valid=True, occ=True, want_occ=True)
            assert_same_results(first, want, f"{case} {issue} t {t}: first call")
            assert_same_results(second, want, f"{case} {issue} t {t}: second call")
            # the masks matter: the masked picture is not the plain one
            plain = c.interp(a, b, fw, bw, t, out_dtype=out_dtype)
            assert not np.array_equal(_np(plain), _np(want[0])), f"{case} {issue} t {t}: the masks change no pixel"
            # without the mask outputs (they live in the workspace), and without valid
            assert_same_pictures(c.run_interp(a, b, p, t, out_dtype, want_valid=True, occ=True), want[:2],
                                 f"{case} {issue} t {t}: masks in the workspace")
            assert_picture(_np(c.run_interp(a, b, p, t, out_dtype, occ=True)), _np(want[0]), f"{case} {issue} t {t}: picture alone")
        # the same pointers twice: the second call replays the captured graph
        t = (0.25, 0.5, 0.75)
        out, valid = torch.empty_like(want[0]), torch.empty_like(want[1])
        mf, mb = torch.empty_like(ofw), torch.empty_like(obw)
        s = torch.cuda.current_stream().cuda_stream

        def masked(alpha, beta):
            for x in (out, valid, mf, mb):
                x.fill_(77)
            c.run_interp_occ_ptr(a.data_ptr(), b.data_ptr(), n, w, h, p, t, alpha, beta, od.IMG_F32, out.data_ptr(),
                                 valid.data_ptr(), mf.data_ptr(), mb.data_ptr(), s)
            return out, valid, mf, mb

        for rep in range(2):
            assert_same_results(masked(0.01, 0.5), want, f"{case} {issue}: call {rep} on fixed pointers")
        # another alpha, and another beta, on the same pointers: their own masks and pictures (the graph key carries
        # both thresholds)
        for alpha, beta in ((0.0, 0.5), (0.0, 0.01)):
            m2 = tuple(c.run_bidir(a, b, p, alpha, beta)[2:4])
            want2 = c.interp(a, b, fw, bw, t, occ_fw=m2[0], occ_bw=m2[1], out_dtype=torch.float32, want_valid=True) + m2
            assert_same_results(masked(alpha, beta), want2, f"{case} {issue}: thresholds {alpha} / {beta} on fixed pointers")
        assert not np.array_equal(_np(m2[0]), _np(ofw))  # (thresholds that far apart give other masks)
        # masks off on the same pointers: the plain fused call's pictures
        out.fill_(77)
        valid.fill_(77)
        c.run_interp_ptr(a.data_ptr(), b.data_ptr(), n, w, h, p, t, od.IMG_F32, out.data_ptr(), valid.data_ptr(), s)
        assert_same_pictures((out, valid), c.interp(a, b, fw, bw, t, out_dtype=torch.float32, want_valid=True),
                             f"{case} {issue}: masks off on fixed pointers")
        assert_same_results(masked(0.01, 0.5), want, f"{case} {issue}: masks on again")
        # the other calls on the same images still return their own results (the graph key)
        assert_picture(_np(c.run(a, b, p)), _np(flow), f"{case} {issue}: plain run after run_interp")
        assert_picture(_np(c.run(a, b, p, grid="level")), _np(level), f"{case} {issue}: level run after run_interp")
        for got, ref in zip(c.run_bidir(a, b, p), bidir):
            assert_picture(_np(got), _np(ref), f"{case} {issue}: run_bidir after run_interp")
        assert_same_pictures(c.run_warp(a, b, p, want_valid=True), warped, f"{case} {issue}: run_warp after run_interp")
        assert_same_pictures(c.run_interp(a, b, p, (0.5,), want_valid=True), c.interp(a, b, fw, bw, (0.5,), want_valid=True),
                             f"{case} {issue}: mask-free run_interp after the other runs")
    finally:
        c.close()


# --------------------------------------------------------------------------------------------- the sequence call

SEQ_SHAPES = [(176, 96, 1), (173, 97, 3)]
T = 6


def _frames(w, h, noc, t_frames=T):
    fr = sequence(w, h, noc, t_frames)
    return _dev(fr[..., 0] if noc == 1 else fr)


def _seq_against_pairs(c, fr, p, stride, occ, what):
    import torch
    for t, out_dtype in (((0.5,), torch.uint8), ((0.25, 0.5, 0.75), torch.float32)):
        want = c.run_interp(fr[:-stride], fr[stride:], p, t, out_dtype, want_valid=True, occ=occ, want_occ=occ)
        got = c.run_sequence_interp(fr, p, t, stride, out_dtype, want_valid=True, occ=occ, want_occ=occ)
        assert got[0].shape[0] == fr.shape[0] - stride
        assert_same_results(got, want, f"{what} t {t}")
        again = c.run_sequence_interp(fr, p, t, stride, out_dtype, want_valid=True, occ=occ, want_occ=occ)
        assert_same_results(again, want, f"{what} t {t}: second call")


@pytest.mark.parametrize("occ", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("w,h,noc", SEQ_SHAPES)
def test_sequence_interp_matches_pair_call(ctx, w, h, noc, stride, occ):
    import of_dis_amd as od
    fr = _frames(w, h, noc)
    p = od.oppoint(2, w, od.MODE_OF, noc)
    _seq_against_pairs(ctx, fr, p, stride, occ, f"{w}x{h} noc {noc} stride {stride} occ {occ}")
    pics = _np(ctx.run_sequence_interp(fr, p, 0.5, stride))
    assert not np.array_equal(pics[0], pics[1])  # (the frames move)


@pytest.mark.parametrize("stride", [1, 3])
def test_sequence_interp_one_pair(ctx, stride):
    """T = stride + 1: one pair, the frames in between built and unused."""
    w, h = 176, 96
    fr = _frames(w, h, 1, stride + 1)
    p = op2(w)
    got = ctx.run_sequence_interp(fr, p, (0.5,), stride, want_valid=True, occ=True, want_occ=True)
    assert got[0].shape == (1, 1, h, w)
    want = ctx.run_interp(fr[:1], fr[stride:], p, (0.5,), want_valid=True, occ=True, want_occ=True)
    assert_same_results(got, want, f"T {stride + 1} stride {stride}")


@pytest.mark.parametrize("issue", ["streams2-chunk2", "graph0", "streams2-chunk2-graph2"])
def test_sequence_interp_issue_forms(issue):
    """Chunks of two pairs overlap by `stride` frames; graph 0 / 2."""
    import of_dis_amd as od
    w, h = 176, 96
    fr = _frames(w, h, 1)
    p = op2(w)
    ref = od.Context(0)
    c = od.Context(0)
    try:
        for k, v in ISSUES[issue].items():
            c.set_option(k, v)
        for stride in (1, 2):
            for occ in (False, True):
                want = ref.run_interp(fr[:-stride], fr[stride:], p, (0.25, 0.75), want_valid=True, occ=occ, want_occ=occ)
                for rep in range(2):
                    got = c.run_sequence_interp(fr, p, (0.25, 0.75), stride, want_valid=True, occ=occ, want_occ=occ)
                    assert_same_results(got, want, f"{issue} stride {stride} occ {occ} call {rep}")
    finally:
        c.close()
        ref.close()


def test_sequence_interp_graph_keys():
    """Pair call, sequence stride 1, sequence stride 2, sequence with masks, pair call -- one context, the same
    pointers, each call twice (the second replays the graph): every call records its own graph."""
    import torch
    import of_dis_amd as od
    w, h = 176, 96
    fr = _frames(w, h, 1)
    p = op2(w)
    c = od.Context(0)
    try:
        t = (0.5,)
        n = T - 1
        want = {(k, occ): c.run_interp(fr[:-k], fr[k:], p, t, want_valid=True, occ=occ) for k in (1, 2) for occ in (False, True)}
        out = torch.empty((n, 1, h, w), dtype=torch.uint8, device="cuda")
        valid = torch.empty_like(out)
        s = torch.cuda.current_stream().cuda_stream
        a, b1 = fr.data_ptr(), fr.data_ptr() + w * h

        def pair():
            out.fill_(9)
            valid.fill_(9)
            c.run_interp_ptr(a, b1, n, w, h, p, t, od.IMG_U8, out.data_ptr(), valid.data_ptr(), s)
            assert_same_pictures((out, valid), want[1, False], "pair call")

        def seq(stride, occ):
            out.fill_(9)
            valid.fill_(9)
            c.run_sequence_interp_ptr(a, T, stride, w, h, p, t, od.IMG_U8, out.data_ptr(), valid.data_ptr(), occ, stream=s)
            assert_same_pictures((out[:T - stride], valid[:T - stride]), want[stride, occ], f"sequence stride {stride} occ {occ}")

        for call in (pair, lambda: seq(1, False), lambda: seq(2, False), lambda: seq(1, True), lambda: seq(1, False), pair):
            call()
            call()  # replayed
    finally:
        c.close()


def test_host_forms_and_timers(ctx):
    import of_dis_amd as od
    w, h = 176, 96
    p = op2(w)
    fr = sequence(w, h, 1, T)[..., 0]
    t = (0.25, 0.75)
    want = [_np(x) for x in ctx.run_sequence_interp(_dev(fr), p, t, 2, want_valid=True, occ=True, want_occ=True)]
    got = ctx.run_sequence_interp_host(fr, p, t, 2, want_valid=True, occ=True, want_occ=True)
    assert got[0].shape == (T - 2, 2, h, w) and got[2].shape == (T - 2, h, w)
    for k in range(4):
        assert_picture(got[k], want[k], f"run_sequence_interp_host (output {k})")
    plain = ctx.run_sequence_interp_host(fr, p, t, 2)
    assert_picture(plain, _np(ctx.run_sequence_interp(_dev(fr), p, t, 2)), "run_sequence_interp_host, no masks")
    a, b = fr[:-1], fr[1:]
    want = [_np(x) for x in ctx.run_interp(_dev(a), _dev(b), p, t, want_valid=True, occ=True, want_occ=True)]
    got = ctx.run_interp_host(a, b, p, t, want_valid=True, occ=True, want_occ=True)
    for k in range(4):
        assert_picture(got[k], want[k], f"run_interp_host with masks (output {k})")
    one = ctx.run_interp_host(fr[0], fr[1], p, t, occ=True, want_occ=True)  # a single pair [h, w]
    assert one[0].shape == (2, h, w) and one[1].shape == (h, w)
    assert_picture(one[0], want[0][0], "run_interp_host with masks, single pair")
    assert_picture(one[1], want[2][0], "run_interp_host with masks, single pair (occ_fw)")
    names = od.kernel_names()
    dfr = _dev(fr)

    def launches(call):
        before = {k: ctx.kernel_time(k)[1] for k in names}
        call()
        after = {k: ctx.kernel_time(k)[1] for k in names}
        return {k: after[k] - before[k] for k in names if after[k] != before[k]}

    ctx.enable_kernel_timing(True)
    try:
        ran = launches(lambda: ctx.run_sequence_interp(dfr, p, t, 1, occ=True))
        assert ran["level_out"] == 2 and ran["fb_check_level"] == 1 and ran["interp_level"] == 1
        assert not [k for k in ran if k.startswith("upsample")] and "interp" not in ran and "fb_check" not in ran
        # one pyramid over the T frames of the sequence where the pair call builds one over its 2 (T - 1): the same
        # launches (the frames are in the grid), so the count shows the sequence plan adds none
        pair = launches(lambda: ctx.run_interp(dfr[:-1], dfr[1:], p, t, occ=True))
        assert ran["pyr_base"] == pair["pyr_base"] == 1 and ran == pair
        ctx.set_option("streams", 2)
        ctx.set_option("chunk", 2)
        ran = launches(lambda: ctx.run_sequence_interp(dfr, p, t, 1, occ=True))  # chunks of 2, 2 and 1 pairs
        assert ran["level_out"] == 6 and ran["fb_check_level"] == 3 and ran["interp_level"] == 3 and ran["pyr_base"] == 3
        assert not [k for k in ran if k.startswith("upsample")]
    finally:
        ctx.set_option("streams", 0)
        ctx.set_option("chunk", 0)
        ctx.enable_kernel_timing(False)


# --------------------------------------------------------------------------------------------- refusals

def test_refusals_leave_the_context_usable(ctx):
    import torch
    import of_dis_amd as od
    L = od.lib()
    INV, UNS = od._lib.ERR_INVALID_ARGUMENT, od._lib.ERR_UNSUPPORTED
    w, h = 176, 96
    p = op2(w)
    fr = _frames(w, h, 1, 4)
    out = torch.full((3 * 17 * h * w,), 7, dtype=torch.uint8, device="cuda")
    plain = _np(ctx.run_sequence_interp(fr, p, 0.5))

    def times(*t):
        arr = np.array(t, f32)
        return arr, arr.ctypes.data

    half = times(0.5)

    def seq(nframes=4, stride=1, params=p, t=half, nt=None, use_occ=1, alpha=0.01, beta=0.5, frames=fr.data_ptr(), o=out.data_ptr()):
        return L.ofdis_run_sequence_interp_u8(ctx._h, frames, nframes, stride, w, h, C.byref(params), t[1],
                                              len(t[0]) if nt is None else nt, use_occ, alpha, beta, 0, o, None, None, None, None)

    def pair(t=half, nt=None, alpha=0.01, beta=0.5, params=p):
        return L.ofdis_run_interp_occ_u8(ctx._h, fr.data_ptr(), fr.data_ptr() + w * h, 3, w, h, C.byref(params), t[1],
                                         len(t[0]) if nt is None else nt, alpha, beta, 0, out.data_ptr(), None, None, None, None)

    def still_works(what):
        torch.cuda.synchronize()
        assert torch.all(out == 7), what  # nothing was enqueued by the refused call
        assert_picture(_np(ctx.run_sequence_interp(fr, p, 0.5)), plain, f"after the refusal of {what}")

    assert seq(stride=0) == INV and seq(stride=-1) == INV                  # stride < 1
    assert seq(nframes=4, stride=4) == INV and seq(nframes=2, stride=3) == INV   # nframes <= stride
    still_works("strides")
    assert seq(params=od.oppoint(2, w, od.MODE_DE, 1)) == UNS and pair(params=od.oppoint(2, w, od.MODE_DE, 1)) == UNS
    still_works("depth mode")
    tv = {p.sc_l: np.zeros((h >> p.sc_l, w >> p.sc_l, 2), f32)}
    ctx.set_capture(None, tv)
    try:
        assert seq() == UNS and seq(use_occ=0) == UNS and pair() == UNS    # a stage capture that is set
    finally:
        ctx.set_capture(None, None)
    still_works("a stage capture")
    long_t = times(*([0.5] * 17))
    for call, name in ((seq, "sequence"), (pair, "pair")):
        assert call(nt=0) == INV and call(t=long_t) == INV, name
        for bad in (-0.1, 1.5, float("nan")):
            assert call(t=times(0.5, bad)) == INV, (name, bad)
        assert call(alpha=-0.01) == INV and call(beta=-0.5) == INV and call(alpha=float("inf")) == INV, name
        still_works(f"{name} times and thresholds")
    assert seq(use_occ=0, alpha=-1.0) == od._lib.OK                        # without masks the thresholds are ignored
    torch.cuda.synchronize()
    assert_picture(_np(out[:3 * h * w]).reshape(3, 1, h, w), plain, "use_occ = 0 ignores alpha")
    out.fill_(7)
    assert seq(frames=None) == INV and seq(o=None) == INV
    with pytest.raises(od.OfdisError) as e:
        ctx.run_sequence_interp(fr, p, 0.5, stride=4)
    assert e.value.code == INV
    still_works("NULL pointers")


# --------------------------------------------------------------------------------------------- CLI

CLI_TIMES = (f32(1) / f32(3), f32(2) / f32(3))  # t = k / (K + 1) for K = 2, as the CLI computes it


@pytest.mark.parametrize("occ", [0, 1])
@pytest.mark.parametrize("noc,exe,ext", [(1, "run_OF_SEQ_INTERP_INT", "pgm"), (3, "run_OF_SEQ_INTERP_RGB", "ppm")])
def test_cli_sequence_interp(ctx, tmp_path, noc, exe, ext, occ):
    """The files from 4 PNG frames at K = 2 are run_sequence_interp's pictures at t = 1/3 and 2/3."""
    import of_dis_amd as od
    w, h = 176, 96
    fr = sequence(w, h, noc, 4)
    paths = _write_pngs(tmp_path, fr)
    prefix = str(tmp_path / "mid_")
    r = subprocess.run([os.path.join(ROOT, "of_dis_amd", "bin", exe), prefix, "2", "2", str(occ)] + paths,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    want = ctx.run_sequence_interp_host(fr[..., 0] if noc == 1 else fr, op2(w, noc), CLI_TIMES, occ=bool(occ))
    assert want.shape[:2] == (3, 2)
    for i in range(3):
        for k in (1, 2):
            got = od.read_image(f"{prefix}{i:06d}_{k:03d}.{ext}", noc)
            assert_picture(got[..., 0] if noc == 1 else got, want[i, k - 1], f"{exe} occ {occ} pair {i} frame {k}")
    assert len(list(tmp_path.glob(f"mid_*.{ext}"))) == 6

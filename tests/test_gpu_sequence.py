"""Video sequences: every frame's pyramid built once (ofdis_run_sequence_u8, run_OF_SEQ_INT / run_OF_SEQ_RGB).

Every comparison is a uint32 bit comparison against the plain path on the same context:
run_sequence(frames, stride=k) must be run(frames[:-k], frames[k:]), and with bidir its backward flow must be
run(frames[k:], frames[:-k]); masks and errors are compared against the numpy reference of test_fb_check.py applied
to those plain flows.  The plain path is pinned to the oracle by the parity tests.

The frames have real motion: frame t is the synth texture translated by t * (1.5, -0.75), so every pair (t, t + k)
is a translation by k * (1.5, -0.75).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_fb_check import assert_err_equal, fb_reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = (1.5, -0.75)
_cache = {}


def sequence(w, h, noc, t_frames):
    """u8 [t_frames, h, w, noc]; generated once per shape (seven frames) and sliced."""
    import of_dis_amd as od
    key = (w, h, noc)
    if key not in _cache:
        fr = [od.synth_shift_pair(w, h, (0, 0), noc, 0)[0]]
        fr += [od.synth_shift_pair(w, h, (STEP[0] * t, STEP[1] * t), noc, 0)[1] for t in range(1, 7)]
        _cache[key] = np.stack(fr)
        _cache[key].setflags(write=False)
    return _cache[key][:t_frames]


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = _bits(got) != _bits(want)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}"


def check_bidir(got, fw, bw, what, alpha=0.01, beta=0.5):
    """got = (flow_fw, flow_bw, occ_fw, occ_bw, err_fw, err_bw) as numpy; fw / bw the plain calls' flows."""
    assert_same(got[0], fw, f"{what}: forward flow")
    assert_same(got[1], bw, f"{what}: backward flow")
    want = fb_reference(fw, bw, alpha, beta)
    for k in (0, 1):
        assert np.array_equal(got[2 + k], want[k]), f"{what}: mask {k} differs"
        assert_err_equal(got[4 + k], want[2 + k], want[k], f"{what}: err {k}")


def _params(w, noc, op, over):
    import of_dis_amd as od
    p = od.oppoint(op, w, od.MODE_OF, noc)
    for k, v in over.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()  # (a copy: the cached frames are read-only)


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ shapes

SHAPES = [
    (176, 96, 1, 2, {}),
    (173, 97, 1, 2, {}),             # divisibility padding on both axes
    (192, 128, 3, 3, {}),            # sc_l = 0, colour: k_pyr_base_rgb and the generic forms
    (176, 96, 1, 2, {"usefbcon": 1}),
    (176, 96, 1, 2, {"usetvref": 0}),
    (176, 96, 1, 2, {"gradmag": 1}),
    (176, 96, 1, 2, {"omp_build": 1}),
]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("w,h,noc,op,over", SHAPES)
def test_sequence_matches_plain(ctx, w, h, noc, op, over, stride):
    fr = sequence(w, h, noc, 6)
    p = _params(w, noc, op, over)
    want = ctx.run_host(fr[:-stride], fr[stride:], p)
    got = ctx.run_sequence_host(fr, p, stride=stride)
    assert got.shape == (6 - stride, h, w, 2)
    assert_same(got, want, f"{w}x{h} noc {noc} {over} stride {stride}")
    assert np.abs(want).max() > 0.5  # the frames do move


@pytest.mark.parametrize("t_frames,stride", [(2, 1), (4, 3)])
def test_sequence_one_pair(ctx, t_frames, stride):
    """T = 2: the plain call of that pair.  T = 4, stride 3: one pair, frames 1 and 2 built and unused."""
    w, h = 176, 96
    fr = sequence(w, h, 1, t_frames)
    p = _params(w, 1, 2, {})
    got = ctx.run_sequence_host(fr, p, stride=stride)
    assert got.shape == (1, h, w, 2)
    assert_same(got[0], ctx.run_host(fr[0], fr[stride], p), f"T {t_frames} stride {stride}")


# ------------------------------------------------------------------------------------------------ issue forms

ISSUES = ((1, 0, 1), (1, 0, 1), (1, 0, 0), (2, 2, 1), (2, 2, 2), (1, 2, 1))


def test_sequence_chunk_overlap():
    """T = 7, stride 2: five pairs; in chunks of 2 / 2 / 1 pairs the chunks read frames [0, 4), [2, 6), [4, 7)."""
    import of_dis_amd as od
    w, h = 176, 96
    fr = _dev(sequence(w, h, 1, 7))
    p = _params(w, 1, 2, {})
    c = od.Context(0)
    want = _np(c.run(fr[:-2], fr[2:], p))
    for streams, chunk, graph in ISSUES:
        c.set_option("streams", streams)
        c.set_option("chunk", chunk)
        c.set_option("graph", graph)
        assert_same(_np(c.run_sequence(fr, p, stride=2)), want, str((streams, chunk, graph)))
    c.close()


@pytest.mark.parametrize("stride,over,issue", [(1, {}, None), (2, {}, None), (1, {"usefbcon": 1}, None),
                                               (2, {}, (2, 2, 1)), (1, {}, (2, 2, 2))])
def test_sequence_bidir(stride, over, issue):
    import of_dis_amd as od
    w, h = 176, 96
    fr = _dev(sequence(w, h, 1, 6))
    p = _params(w, 1, 2, over)
    c = od.Context(0)
    fw, bw = _np(c.run(fr[:-stride], fr[stride:], p)), _np(c.run(fr[stride:], fr[:-stride], p))
    if issue:
        for k, v in zip(("streams", "chunk", "graph"), issue):
            c.set_option(k, v)
    got = c.run_sequence(fr, p, stride=stride, bidir=True, want_err=True)
    assert len(got) == 6
    check_bidir([_np(t) for t in got], fw, bw, f"stride {stride} {over} {issue}")
    four = c.run_sequence(fr, p, stride=stride, bidir=True)
    assert len(four) == 4
    assert_same(_np(four[1]), bw, "backward flow without the errors")
    c.close()


def test_sequence_bidir_host(ctx):
    w, h = 176, 96
    fr = sequence(w, h, 1, 4)
    p = _params(w, 1, 2, {})
    fw, bw = ctx.run_host(fr[:-1], fr[1:], p), ctx.run_host(fr[1:], fr[:-1], p)
    check_bidir(ctx.run_sequence_host(fr, p, bidir=True, want_err=True), fw, bw, "host buffers")


# ------------------------------------------------------------------------------------------------ other modes

def test_sequence_init(ctx):
    """An initial flow per pair (the padding becomes a multiple of 2^(sc_f + 1)), device and host buffers."""
    w, h = 176, 96
    fr = sequence(w, h, 1, 5)
    p = _params(w, 1, 2, {})
    rng = np.random.default_rng(5)
    init = (rng.standard_normal((3, h, w, 2)) * 2 + np.array(STEP) * 2).astype(np.float32)
    want = ctx.run_host(fr[:-2], fr[2:], p, init=init)
    assert not np.array_equal(_bits(want), _bits(ctx.run_host(fr[:-2], fr[2:], p)))  # the initial flow matters
    assert_same(ctx.run_sequence_host(fr, p, stride=2, init=init), want, "init, host buffers")
    assert_same(_np(ctx.run_sequence(_dev(fr), p, stride=2, init=_dev(init))), want, "init, device buffers")


def test_sequence_latency_mode():
    """sor_mode = 1 (red-black refinement) against the sor_mode = 1 plain call."""
    import of_dis_amd as od
    w, h = 176, 96
    fr = sequence(w, h, 1, 4)
    p = _params(w, 1, 2, {})
    c = od.Context(0)
    exact = c.run_host(fr[:-1], fr[1:], p)
    c.set_option("sor_mode", 1)
    want = c.run_host(fr[:-1], fr[1:], p)
    assert not np.array_equal(_bits(want), _bits(exact))  # the option took effect
    assert_same(c.run_sequence_host(fr, p), want, "sor_mode 1")
    c.close()


def test_sequence_stage_capture(ctx):
    """A stage capture takes pair 0's flow per scale, as in the plain call."""
    w, h = 173, 97
    fr = sequence(w, h, 1, 5)
    p = _params(w, 1, 2, {})
    d = 1 << p.sc_f
    wp, hp = w + (d - w % d) % d, h + (d - h % d) % d
    scales = range(p.sc_l, p.sc_f + 1)

    def captured(run):
        dis = {s: np.zeros((hp >> s, wp >> s, 2), np.float32) for s in scales}
        tv = {s: np.zeros((hp >> s, wp >> s, 2), np.float32) for s in scales}
        ctx.set_capture(dis, tv)
        try:
            out = run()
        finally:
            ctx.set_capture(None, None)
        return out, dis, tv

    want, wd, wt = captured(lambda: ctx.run_host(fr[:-2], fr[2:], p))
    got, gd, gt = captured(lambda: ctx.run_sequence_host(fr, p, stride=2))
    assert_same(got, want, "full-resolution flow")
    for s in scales:
        assert np.abs(wt[s]).max() > 0
        assert_same(gd[s], wd[s], f"scale {s} after aggregation")
        assert_same(gt[s], wt[s], f"scale {s} after refinement")


def test_sequence_graph_keys():
    """Plain, sequence stride 1, sequence stride 2, bidirectional sequence, plain -- one context, the same buffers,
    each call twice (the second replays the graph): every call must record its own graph."""
    import torch
    import of_dis_amd as od
    w, h, T = 176, 96, 6
    fr = _dev(sequence(w, h, 1, T))
    p = _params(w, 1, 2, {})
    c = od.Context(0)
    a, b1 = fr.data_ptr(), fr.data_ptr() + w * h
    n = T - 1
    fw1 = _np(c.run(fr[:-1], fr[1:], p))
    bw1 = _np(c.run(fr[1:], fr[:-1], p))
    fw2 = _np(c.run(fr[:-2], fr[2:], p))
    out = torch.zeros((n, h, w, 2), dtype=torch.float32, device="cuda")
    obw = torch.zeros_like(out)
    occ = [torch.zeros((n, h, w), dtype=torch.uint8, device="cuda") for _ in range(2)]
    err = [torch.zeros((n, h, w), dtype=torch.float32, device="cuda") for _ in range(2)]
    s = torch.cuda.current_stream().cuda_stream

    def plain():
        out.fill_(3)
        c.run_ptr(a, b1, n, w, h, p, out.data_ptr(), s)
        assert_same(_np(out), fw1, "plain")

    def seq(stride):
        out.fill_(3)
        c.run_sequence_ptr(a, T, stride, w, h, p, out.data_ptr(), stream=s)
        assert_same(_np(out)[:T - stride], fw1 if stride == 1 else fw2, f"sequence stride {stride}")

    def bidir():
        for t in [out, obw] + occ + err:
            t.fill_(3)
        c.run_sequence_ptr(a, T, 1, w, h, p, out.data_ptr(), 0, 0.01, 0.5, obw.data_ptr(), occ[0].data_ptr(),
                           occ[1].data_ptr(), err[0].data_ptr(), err[1].data_ptr(), s)
        check_bidir([_np(t) for t in [out, obw] + occ + err], fw1, bw1, "bidirectional sequence")

    for call in (plain, lambda: seq(1), lambda: seq(2), bidir, plain):
        call()
        call()  # replayed
    c.close()


def test_sequence_refusals(ctx):
    import of_dis_amd as od
    w, h = 176, 96
    fr = sequence(w, h, 1, 4)
    p = _params(w, 1, 2, {})
    INV, UNS = od._lib.ERR_INVALID_ARGUMENT, od._lib.ERR_UNSUPPORTED
    d = _dev(fr)
    out = _dev(np.full((4, h, w, 2), 7, np.float32))
    L = od.lib()

    def call(nframes, stride, init=None, bw=None, params=p):
        return L.ofdis_run_sequence_u8(ctx._h, d.data_ptr(), nframes, stride, init, w, h, C.byref(params), 0.01, 0.5,
                                       out.data_ptr(), bw, None, None, None, None, None)

    assert call(4, 0) == INV                                       # stride < 1
    assert call(4, -1) == INV
    assert call(4, 4) == INV                                       # nframes <= stride
    assert call(2, 3) == INV
    assert call(4, 1, init=out.data_ptr(), bw=out.data_ptr()) == UNS   # init with a backward output
    assert call(4, 1, params=od.oppoint(2, w, od.MODE_DE, 1)) == UNS  # depth mode
    assert np.all(_np(out) == 7)  # nothing was enqueued
    flow = np.empty((3, h, w, 2), np.float32)
    assert L.ofdis_run_sequence_u8_host(ctx._h, fr.ctypes.data, 4, 4, None, w, h, C.byref(p), 0.01, 0.5, flow.ctypes.data,
                                        None, None, None, None, None) == INV
    with pytest.raises(od.OfdisError) as e:
        ctx.run_sequence_host(fr, od.oppoint(2, w, od.MODE_DE, 1))
    assert e.value.code == UNS
    assert_same(ctx.run_sequence_host(fr, p), ctx.run_host(fr[:-1], fr[1:], p), "after the refusals")


# ------------------------------------------------------------------------------------------------ meaning

# largest |mean interior flow - k * (1.5, -0.75)| over a pair's two components, measured with oracle/pyoracle.py on
# the CPU (the GPU flow is the oracle's bit for bit) and rounded up: {stride: (pair 0, the later pairs)}
MEANING_MARGIN = {1: (0.14, 1.31), 2: (0.08, 1.45)}


def test_sequence_meaning(ctx):
    """Mean flow over the interior (16-pixel margin) of every pair of the 192 x 128 colour sequence, op-point 3,
    against the translation k * (1.5, -0.75) the frames were generated with.

    The CPU oracle's figures (largest deviation of the two components, in pixels):
      stride 1: pair 0 0.1381; pairs 1..4 1.3034, 1.2993, 1.2982, 1.2973 (mean flow about (0.20, -0.11))
      stride 2: pair 0 0.0788; pairs 1..3 1.3662, 1.3673, 1.4411 (mean flow about (1.6, -0.87))
    Only pair 0 is a clean translation: the synthetic generator adds one fixed noise realisation (sigma 2 grey levels)
    to every translated frame, so two translated frames share a static pixel-level pattern that the finest scales
    lock onto, and the flow of the later pairs falls short of the translation by about 1.3 pixels at either stride.
    That is a property of the frames, the same on the CPU -- the margins below are those figures rounded up, so for
    the later pairs this check is weak; what pins the values is the bit comparison of the other tests."""
    w, h = 192, 128
    fr = sequence(w, h, 3, 6)
    p = _params(w, 3, 3, {})
    for stride in (1, 2):
        flow = ctx.run_sequence_host(fr, p, stride=stride)
        mean = flow[:, 16:h - 16, 16:w - 16].reshape(flow.shape[0], -1, 2).mean(1)
        dev = np.abs(mean - np.array(STEP) * stride).max(1)
        print(f"stride {stride}: mean interior flow per pair {mean.tolist()}, deviation per pair {dev.tolist()}")
        first, later = MEANING_MARGIN[stride]
        assert dev[0] <= first and dev[1:].max() <= later


# ------------------------------------------------------------------------------------------------ CLI

def _write_pngs(tmp_path, frames):
    from test_image_io import encode_png
    paths = []
    for t, im in enumerate(frames):
        path = tmp_path / f"f{t}.png"
        rgb = im[..., ::-1] if im.shape[-1] == 3 else np.repeat(im, 3, axis=-1)
        path.write_bytes(encode_png(rgb.astype(np.int64), 2, 8))
        paths.append(str(path))
    return paths


@pytest.mark.parametrize("stride", [1, 2])
def test_cli_sequence_int(tmp_path, stride):
    """Every file run_OF_SEQ_INT writes is, byte for byte, run_OF_INT's for that pair."""
    bindir = os.path.join(ROOT, "of_dis_amd", "bin")
    paths = _write_pngs(tmp_path, sequence(176, 96, 1, 4))
    r = subprocess.run([os.path.join(bindir, "run_OF_SEQ_INT"), str(tmp_path / "s_"), "2", str(stride)] + paths,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for i in range(4 - stride):
        one = tmp_path / f"one{i}.flo"
        r = subprocess.run([os.path.join(bindir, "run_OF_INT"), paths[i], paths[i + stride], str(one), "2"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / f"s_{i:06d}.flo").read_bytes() == one.read_bytes(), f"pair {i}"
    assert not (tmp_path / f"s_{4 - stride:06d}.flo").exists()


def test_cli_sequence_windows(tmp_path):
    """258 frames, 257 pairs: two windows (256 pairs and 1) that share one frame.  The pairs on both sides of the
    seam, and the first, against run_OF_INT."""
    bindir = os.path.join(ROOT, "of_dis_amd", "bin")
    w, h = 176, 96
    seven = sequence(w, h, 1, 7)
    distinct = []
    for t, im in enumerate(seven):
        path = tmp_path / f"d{t}.pgm"
        path.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + im.tobytes())
        distinct.append(str(path))
    paths = [distinct[t % 7] for t in range(258)]
    r = subprocess.run([os.path.join(bindir, "run_OF_SEQ_INT"), str(tmp_path / "w_"), "2", "1"] + paths,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert len(list(tmp_path.glob("w_*.flo"))) == 257
    for i in (0, 255, 256):
        one = tmp_path / f"one{i}.flo"
        r = subprocess.run([os.path.join(bindir, "run_OF_INT"), paths[i], paths[i + 1], str(one), "2"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / f"w_{i:06d}.flo").read_bytes() == one.read_bytes(), f"pair {i}"


def test_cli_sequence_rgb(tmp_path):
    bindir = os.path.join(ROOT, "of_dis_amd", "bin")
    paths = _write_pngs(tmp_path, sequence(192, 128, 3, 3))
    r = subprocess.run([os.path.join(bindir, "run_OF_SEQ_RGB"), str(tmp_path / "c_"), "3", "1"] + paths,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for i in range(2):
        one = tmp_path / f"one{i}.flo"
        r = subprocess.run([os.path.join(bindir, "run_OF_RGB"), paths[i], paths[i + 1], str(one), "3"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / f"c_{i:06d}.flo").read_bytes() == one.read_bytes(), f"pair {i}"

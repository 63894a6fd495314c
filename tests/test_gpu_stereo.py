"""Both views of a stereo pair from one batch, with the left-right check (ofdis_run_stereo_u8, ofdis_lr_check).

k_lr_check is compared bit for bit against the numpy reference of test_lr_check.py, and on finite fields against
k_fb_check on the fields (d, 0).  Every run_stereo case is compared with two calls of the plain depth path on the same
context: disp_l must be run(l, r) and disp_r must be -run(mir r, mir l) mirrored back, bit for bit; masks and errors
against the reference applied to those plain fields.  The plain path is pinned to the oracle by the parity tests, so
the code histograms of the scenes are known from the CPU (test_lr_check.py: at least 100 pixels of every code in both
views of every case).
"""
import os
import subprocess

import numpy as np
import pytest

from test_fb_check import assert_err_equal
from test_lr_check import (CASE_SCENES, SCENE_FRAME, lr_reference, pack, random_fields, stereo_definition,
                           stereo_scene)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


def _params(w, noc, op, over):
    import of_dis_amd as od
    p = od.oppoint(op, w, od.MODE_DE, noc)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def check_result(got, dl, dr, alpha=0.01, beta=0.5, what="", codes=False):
    """got = (disp_l, disp_r, occ_l, occ_r[, err_l, err_r]) as numpy; dl / dr the definition from the plain calls."""
    assert np.array_equal(_bits(got[0]), _bits(dl)), f"{what}: disp_l differs from run(l, r)"
    assert np.array_equal(_bits(got[1]), _bits(dr)), f"{what}: disp_r differs from -run(mir r, mir l) mirrored back"
    want = lr_reference(dl.reshape((-1,) + dl.shape[-2:]), dr.reshape((-1,) + dr.shape[-2:]), alpha, beta)
    want = [x.reshape(dl.shape) for x in want]
    for k in (0, 1):
        assert np.array_equal(got[2 + k], want[k]), f"{what}: mask {k} differs"
        if codes:
            assert set(np.unique(want[k])) == {0, 1, 2}, f"{what}: mask {k} lacks a code"
    if len(got) > 4:
        for k in (0, 1):
            assert_err_equal(got[4 + k], want[2 + k], want[k], f"{what}: err {k}")


# --------------------------------------------------------------------------------------------- k_lr_check

def _planted(w, h, n=2):
    """random_fields with non-finite values planted: NaN, +-inf in both fields (own values and gathered taps)."""
    dl, dr = random_fields(w, h, n, seed=7)
    rng = np.random.default_rng(w * 31 + h)
    for d in (dl, dr):
        for val in (np.nan, np.inf, -np.inf):
            k = max(1, d.size // 50) if d.size > 4 else 1
            d.reshape(-1)[rng.choice(d.size, k, replace=False)] = val
    return dl, dr


@pytest.mark.parametrize("w,h", [(160, 120), (173, 97), (4, 1), (1, 1)])
def test_lr_check_matches_numpy(ctx, w, h):
    """160 x 120: the four-pixel form; 173 x 97: the one-pixel form; 4 x 1 and 1 x 1: a single thread's worth."""
    import torch
    n = 2
    for planted in (False, True):
        dl, dr = _planted(w, h, n) if planted else random_fields(w, h, n, seed=3)
        tl, tr = torch.from_numpy(dl).cuda(), torch.from_numpy(dr).cuda()
        for alpha, beta in ((0.01, 0.5), (0.0, 0.0)):
            want = lr_reference(dl, dr, alpha, beta)
            both = [t.cpu().numpy() for t in ctx.lr_check(tl, tr, alpha, beta, want_err=True)]
            masks = [t.cpu().numpy() for t in ctx.lr_check(tl, tr, alpha, beta)]
            err = [torch.full((n, h, w), 7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
            ctx.lr_check_ptr(tl.data_ptr(), tr.data_ptr(), n, w, h, alpha, beta, 0, 0, err[0].data_ptr(),
                             err[1].data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            for k in (0, 1):
                what = f"{w}x{h} planted {planted} ({alpha}, {beta}) view {k}"
                assert np.array_equal(both[k], want[k]), what
                assert np.array_equal(masks[k], want[k]), what + " (masks only)"
                assert_err_equal(both[2 + k], want[2 + k], want[k], what)
                assert_err_equal(err[k].cpu().numpy(), want[2 + k], want[k], what + " (errors only)")
            if not planted:  # finite fields: ofdis_fb_check on (d, 0), the second pin
                fb = ctx.fb_check(torch.from_numpy(pack(dl)).cuda(), torch.from_numpy(pack(dr)).cuda(), alpha, beta,
                                  want_err=True)
                for k in range(4):
                    assert np.array_equal(_bits(both[k]) if k > 1 else both[k],
                                          _bits(fb[k].cpu().numpy()) if k > 1 else fb[k].cpu().numpy()), (w, h, k)
        if (w, h) in ((160, 120), (173, 97)):  # (the suggested thresholds: no comparison above is against a constant)
            assert all(set(np.unique(m)) == {0, 1, 2} for m in lr_reference(dl, dr)[:2])
    # one view's outputs alone, and an unaligned field (a view from the second float on): the one-pixel form
    occ_r = torch.full((n, h, w), 9, dtype=torch.uint8, device="cuda")
    ctx.lr_check_ptr(tl.data_ptr(), tr.data_ptr(), n, w, h, 0.01, 0.5, 0, occ_r.data_ptr(), 0, 0,
                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(occ_r.cpu().numpy(), lr_reference(dl, dr)[1])
    if w % 4 == 0:
        flat = torch.zeros(n * h * w + 1, dtype=torch.float32, device="cuda")
        flat[1:] = tl.reshape(-1)
        occ_l = torch.full((n, h, w), 9, dtype=torch.uint8, device="cuda")
        ctx.lr_check_ptr(flat.data_ptr() + 4, tr.data_ptr(), n, w, h, 0.01, 0.5, occ_l.data_ptr(), 0, 0, 0,
                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(occ_l.cpu().numpy(), lr_reference(dl, dr)[0])


def test_lr_check_refusals(ctx):
    import torch
    import of_dis_amd as od
    d = torch.zeros((1, 8, 8), dtype=torch.float32, device="cuda")
    o = torch.zeros((1, 8, 8), dtype=torch.uint8, device="cuda")
    for args in ((d.data_ptr(), d.data_ptr(), 1, 8, 8, -1.0, 0.5), (d.data_ptr(), d.data_ptr(), 1, 8, 8, 0.01, float("inf")),
                 (0, d.data_ptr(), 1, 8, 8, 0.01, 0.5), (d.data_ptr(), d.data_ptr(), 0, 8, 8, 0.01, 0.5),
                 (d.data_ptr(), d.data_ptr(), 1, 0, 8, 0.01, 0.5)):
        with pytest.raises(od.OfdisError) as e:
            ctx.lr_check_ptr(*args, o.data_ptr())
        assert e.value.code == od._lib.ERR_INVALID_ARGUMENT
    ctx.lr_check_ptr(d.data_ptr(), d.data_ptr(), 1, 8, 8, 0.01, 0.5)  # all four outputs NULL: nothing to do
    assert not ctx.lr_check(d, d)[0].any()


# --------------------------------------------------------------------------------------------- run_stereo

def _definition(c, left, right, p):
    return stereo_definition(lambda a, b: c.run_host(a, b, p), left, right)


@pytest.mark.parametrize("w,h,noc,op,over,scene", CASE_SCENES)
def test_stereo_matches_plain_calls(ctx, w, h, noc, op, over, scene):
    import of_dis_amd as od
    left, right = stereo_scene(od, scene, w, h, noc, SCENE_FRAME)
    p = _params(w, noc, op, over)
    dl, dr = _definition(ctx, left, right, p)
    got = ctx.run_stereo_host(left, right, p, want_err=True)
    assert got[0].shape == (h, w) and got[1].dtype == np.float32 and got[2].shape == (h, w) and got[2].dtype == np.uint8
    check_result(got, dl, dr, what=f"{scene} {over}", codes=True)
    assert np.all(got[0] <= 0) and np.all(got[1] >= 0)


@pytest.fixture(scope="module")
def batch():
    """Five pairs at 176 x 96 on the device, and the definition from plain calls."""
    import torch
    import of_dis_amd as od
    w, h, n = 176, 96, 5
    pairs = [od.synth_pair(w, h, 1, f, od.MODE_DE) for f in range(n)]
    left, right = np.stack([x[0] for x in pairs]), np.stack([x[1] for x in pairs])
    p = _params(w, 1, 2, {})
    c = od.Context(0)
    dl, dr = _definition(c, left, right, p)
    c.close()
    return w, h, n, torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda(), p, dl, dr


def test_stereo_batch_paths(batch):
    """One stream (graph, replayed), eager, round-robin chunks (eager and captured), chunks on one stream."""
    import torch
    import of_dis_amd as od
    w, h, n, left, right, p, dl, dr = batch
    c = od.Context(0)
    for streams, chunk, graph in ((1, 0, 1), (1, 0, 1), (1, 0, 0), (2, 2, 1), (2, 2, 2), (1, 2, 1)):
        c.set_option("streams", streams)
        c.set_option("chunk", chunk)
        c.set_option("graph", graph)
        for rep in range(2):  # the same arguments twice: the second call replays where a graph was recorded
            got = c.run_stereo(left, right, p, want_err=True)
            torch.cuda.synchronize()
            check_result([t.cpu().numpy() for t in got], dl, dr, what=str((streams, chunk, graph, rep)))
    c.close()


def test_stereo_graph_keys(batch):
    """Plain depth call, stereo, plain, stereo with another beta -- one context, the same buffers: each call must
    record its own graph."""
    import torch
    import of_dis_amd as od
    w, h, n, left, right, p, dl, dr = batch
    c = od.Context(0)
    dev = left.device
    out = torch.zeros((n, h, w), dtype=torch.float32, device=dev)
    o_r = torch.zeros_like(out)
    occ = [torch.zeros((n, h, w), dtype=torch.uint8, device=dev) for _ in range(2)]
    err = [torch.zeros((n, h, w), dtype=torch.float32, device=dev) for _ in range(2)]

    def plain():
        out.zero_()
        c.run_ptr(left.data_ptr(), right.data_ptr(), n, w, h, p, out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(dl))

    def stereo(beta):
        for t in [out, o_r] + occ + err:
            t.fill_(3)
        c.run_stereo_ptr(left.data_ptr(), right.data_ptr(), n, w, h, p, 0.01, beta, out.data_ptr(), o_r.data_ptr(),
                         occ[0].data_ptr(), occ[1].data_ptr(), err[0].data_ptr(), err[1].data_ptr(),
                         torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        check_result([t.cpu().numpy() for t in [out, o_r] + occ + err], dl, dr, 0.01, beta, f"beta {beta}")

    plain()
    plain()  # replayed
    stereo(0.5)
    plain()
    stereo(0.05)
    stereo(0.05)  # replayed
    want = lr_reference(dl, dr, 0.01, 0.5), lr_reference(dl, dr, 0.01, 0.05)
    assert not np.array_equal(want[0][0], want[1][0])  # the two betas do give different masks
    c.close()


def test_stereo_optional_outputs(ctx, batch):
    import torch
    w, h, n, left, right, p, dl, dr = batch
    want = lr_reference(dl, dr)
    out = torch.zeros((n, h, w), dtype=torch.float32, device=left.device)
    occ = [torch.full((n, h, w), 9, dtype=torch.uint8, device=left.device) for _ in range(2)]
    s = torch.cuda.current_stream().cuda_stream
    # masks without disp_r: the right view's field stays in the workspace
    ctx.run_stereo_ptr(left.data_ptr(), right.data_ptr(), n, w, h, p, 0.01, 0.5, out.data_ptr(), 0, occ[0].data_ptr(),
                       occ[1].data_ptr(), 0, 0, s)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(dl))
    assert np.array_equal(occ[0].cpu().numpy(), want[0]) and np.array_equal(occ[1].cpu().numpy(), want[1])
    # disp_r without masks
    o_r = torch.zeros_like(out)
    out.zero_()
    ctx.run_stereo_ptr(left.data_ptr(), right.data_ptr(), n, w, h, p, 0.01, 0.5, out.data_ptr(), o_r.data_ptr(), stream=s)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(dl)) and np.array_equal(_bits(o_r.cpu().numpy()), _bits(dr))
    # nothing but disp_l: the plain call
    out.zero_()
    ctx.run_stereo_ptr(left.data_ptr(), right.data_ptr(), n, w, h, p, 0.01, 0.5, out.data_ptr(), stream=s)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(dl))


def test_stereo_refusals(ctx):
    import torch
    import of_dis_amd as od
    w, h = 160, 120
    left, right = od.synth_pair(w, h, 1, 0, od.MODE_DE)
    with pytest.raises(od.OfdisError) as e:
        ctx.run_stereo_host(left, right, od.oppoint(2, w, od.MODE_OF, 1))
    assert e.value.code == od._lib.ERR_UNSUPPORTED
    p = od.oppoint(2, w, od.MODE_DE, 1)
    for alpha, beta in ((-1.0, 0.5), (0.01, float("nan"))):
        with pytest.raises(od.OfdisError) as e:
            ctx.run_stereo_host(left, right, p, alpha, beta)
        assert e.value.code == od._lib.ERR_INVALID_ARGUMENT
    tl, tr = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    with pytest.raises(od.OfdisError) as e:  # NULL disp_l
        ctx.run_stereo_ptr(tl.data_ptr(), tr.data_ptr(), 1, w, h, p, 0.01, 0.5, 0)
    assert e.value.code == od._lib.ERR_INVALID_ARGUMENT
    dis = {p.sc_l: np.zeros((h >> p.sc_l, w >> p.sc_l, 1), np.float32)}
    ctx.set_capture(dis, None)
    try:
        with pytest.raises(od.OfdisError) as e:
            ctx.run_stereo_host(left, right, p)
        assert e.value.code == od._lib.ERR_UNSUPPORTED
    finally:
        ctx.set_capture(None, None)
    got = ctx.run_stereo_host(left, right, p)  # the context still works
    check_result(got, *_definition(ctx, left, right, p), what="after the refusals")


def _read_pfm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"Pf"
        w, h = map(int, f.readline().split())
        assert float(f.readline()) < 0  # little endian
        return np.frombuffer(f.read(), "<f4").reshape(h, w)[::-1]


def _read_pgm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"P5"
        w, h = map(int, f.readline().split())
        assert int(f.readline()) == 255
        return np.frombuffer(f.read(), np.uint8).reshape(h, w)


def test_stereo_cli(ctx, tmp_path):
    """run_DE_LR_INT on a PGM pair: both .pfm files hold the negated fields (ofdis_write_pfm), the .pgm files the
    raw mask codes."""
    import of_dis_amd as od
    w, h = 160, 120
    left, right = stereo_scene(od, "synth", w, h, 1, SCENE_FRAME)
    od.write_pnm(str(tmp_path / "l.pgm"), left)
    od.write_pnm(str(tmp_path / "r.pgm"), right)
    outs = [str(tmp_path / n) for n in ("dl.pfm", "dr.pfm", "ol.pgm", "or.pgm")]
    exe = os.path.join(ROOT, "of_dis_amd", "bin", "run_DE_LR_INT")
    r = subprocess.run([exe, str(tmp_path / "l.pgm"), str(tmp_path / "r.pgm")] + outs, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    want = ctx.run_stereo_host(left, right, od.oppoint(2, w, od.MODE_DE, 1))
    assert np.array_equal(_bits(-_read_pfm(outs[0])), _bits(want[0]))
    assert np.array_equal(_bits(-_read_pfm(outs[1])), _bits(want[1]))
    assert np.array_equal(_read_pgm(outs[2]), want[2]) and np.array_equal(_read_pgm(outs[3]), want[3])
    assert set(np.unique(want[2])) == {0, 1, 2}
    assert subprocess.run([exe, "only", "two"], capture_output=True).returncode == 1  # usage

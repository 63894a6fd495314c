"""Both directions of a pair from one pyramid, with the forward-backward check (ofdis_run_bidir_u8).

Every case compares run_bidir with two calls of the plain path on the same context: flow_fw must be run(a, b) and
flow_bw must be run(b, a), bit for bit.  Masks and errors are compared against the numpy reference of
test_fb_check.py applied to those plain flows.  The plain path is pinned to the oracle by the parity tests, so the
code histograms of the synthetic pairs are known from the CPU: all three codes occur in every case below, in both
directions (the smallest count is 300, code 1 forward with usefbcon = 1).
"""
import numpy as np
import pytest

from test_fb_check import assert_err_equal, fb_reference

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def check_result(got, fw, bw, alpha=0.01, beta=0.5, what="", codes=False):
    """got = (flow_fw, flow_bw, occ_fw, occ_bw[, err_fw, err_bw]) as numpy; fw / bw the plain calls' flows."""
    assert np.array_equal(_bits(got[0]), _bits(fw)), f"{what}: forward flow differs from run(a, b)"
    assert np.array_equal(_bits(got[1]), _bits(bw)), f"{what}: backward flow differs from run(b, a)"
    want = fb_reference(fw.reshape((-1,) + fw.shape[-3:]), bw.reshape((-1,) + bw.shape[-3:]), alpha, beta)
    want = [x.reshape(fw.shape[:-1]) for x in want]
    for k in (0, 1):
        assert np.array_equal(got[2 + k], want[k]), f"{what}: mask {k} differs"
        if codes:
            assert set(np.unique(want[k])) == {0, 1, 2}, f"{what}: mask {k} lacks a code"
    if len(got) > 4:
        for k in (0, 1):
            assert_err_equal(got[4 + k], want[2 + k], want[k], f"{what}: err {k}")


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


def _params(w, noc, op, over):
    import of_dis_amd as od
    p = od.oppoint(op, w, od.MODE_OF, noc)
    for k, v in over.items():
        setattr(p, k, v)
    return p


CASES = [
    (160, 120, 1, 2, {}, 3),
    (173, 97, 1, 2, {}, 5),            # divisibility padding on both axes
    (192, 128, 3, 3, {}, 5),           # sc_l = 0, colour
    (160, 120, 1, 2, {"usefbcon": 1}, 5),
    (160, 120, 1, 2, {"usetvref": 0}, 5),
    (160, 120, 1, 2, {"gradmag": 1}, 5),
    (160, 120, 1, 2, {"omp_build": 1}, 5),
]


@pytest.mark.parametrize("w,h,noc,op,over,frame", CASES)
def test_bidir_matches_two_plain_calls(ctx, w, h, noc, op, over, frame):
    import of_dis_amd as od
    a, b = od.synth_pair(w, h, noc, frame, od.MODE_OF)
    p = _params(w, noc, op, over)
    fw, bw = ctx.run_host(a, b, p), ctx.run_host(b, a, p)
    got = ctx.run_bidir_host(a, b, p, want_err=True)
    assert got[0].shape == (h, w, 2) and got[2].shape == (h, w) and got[2].dtype == np.uint8
    check_result(got, fw, bw, what=str(over), codes=True)


@pytest.fixture(scope="module")
def batch():
    """Five pairs at 176 x 96 on the device."""
    import torch
    import of_dis_amd as od
    w, h, n = 176, 96, 5
    pairs = [od.synth_pair(w, h, 1, f, od.MODE_OF) for f in range(n)]
    a = torch.from_numpy(np.stack([x[0] for x in pairs])).cuda()
    b = torch.from_numpy(np.stack([x[1] for x in pairs])).cuda()
    return w, h, n, a, b


def _plain(c, a, b, p):
    import torch
    fw, bw = c.run(a, b, p), c.run(b, a, p)
    torch.cuda.synchronize()
    return fw.cpu().numpy(), bw.cpu().numpy()


@pytest.mark.parametrize("usefbcon", [0, 1])
def test_bidir_batch_paths(batch, usefbcon):
    """One stream (graph, replayed), eager, round-robin chunks (eager and captured), chunks on one stream."""
    import torch
    import of_dis_amd as od
    w, h, n, a, b = batch
    p = _params(w, 1, 2, {"usefbcon": usefbcon})
    c = od.Context(0)
    fw, bw = _plain(c, a, b, p)
    for streams, chunk, graph in ((1, 0, 1), (1, 0, 1), (1, 0, 0), (2, 2, 1), (2, 2, 2), (1, 2, 1)):
        c.set_option("streams", streams)
        c.set_option("chunk", chunk)
        c.set_option("graph", graph)
        got = c.run_bidir(a, b, p, want_err=True)
        torch.cuda.synchronize()
        check_result([t.cpu().numpy() for t in got], fw, bw, what=str((streams, chunk, graph)))
    c.close()


def test_bidir_graph_keys(batch):
    """Plain, bidirectional, plain, bidirectional with another alpha -- one context, the same buffers: each call
    must record its own graph."""
    import torch
    import of_dis_amd as od
    w, h, n, a, b = batch
    p = _params(w, 1, 2, {})
    c = od.Context(0)
    fw, bw = _plain(c, a, b, p)
    dev = a.device
    out = torch.zeros((n, h, w, 2), dtype=torch.float32, device=dev)
    obw = torch.zeros_like(out)
    occ = [torch.zeros((n, h, w), dtype=torch.uint8, device=dev) for _ in range(2)]
    err = [torch.zeros((n, h, w), dtype=torch.float32, device=dev) for _ in range(2)]

    def plain():
        out.zero_()
        c.run(a, b, p, out=out)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(fw))

    def bidir(alpha):
        for t in [out, obw] + occ + err:
            t.fill_(3)
        c.run_bidir_ptr(a.data_ptr(), b.data_ptr(), n, w, h, p, alpha, 0.5, out.data_ptr(), obw.data_ptr(),
                        occ[0].data_ptr(), occ[1].data_ptr(), err[0].data_ptr(), err[1].data_ptr(),
                        torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        check_result([t.cpu().numpy() for t in [out, obw] + occ + err], fw, bw, alpha, 0.5, f"alpha {alpha}")

    plain()
    plain()  # replayed
    bidir(0.01)
    plain()
    bidir(0.2)
    bidir(0.2)  # replayed
    want = fb_reference(fw, bw, 0.01, 0.5), fb_reference(fw, bw, 0.2, 0.5)
    assert not np.array_equal(want[0][0], want[1][0])  # the two alphas do give different masks
    c.close()


def test_bidir_latency_mode(batch):
    """sor_mode = 1 (red-black refinement): both directions against two sor_mode = 1 plain calls."""
    import torch
    import of_dis_amd as od
    w, h, n, a, b = batch
    p = _params(w, 1, 2, {})
    c = od.Context(0)
    exact = _plain(c, a[:2], b[:2], p)
    c.set_option("sor_mode", 1)
    fw, bw = _plain(c, a[:2], b[:2], p)
    assert not np.array_equal(_bits(fw), _bits(exact[0]))  # the option took effect
    got = c.run_bidir(a[:2], b[:2], p, want_err=True)
    torch.cuda.synchronize()
    check_result([t.cpu().numpy() for t in got], fw, bw, what="sor_mode 1")
    c.close()


def test_bidir_optional_outputs(ctx, batch):
    import torch
    w, h, n, a, b = batch
    p = _params(w, 1, 2, {})
    fw, bw = _plain(ctx, a, b, p)
    want = fb_reference(fw, bw)
    out = torch.zeros((n, h, w, 2), dtype=torch.float32, device=a.device)
    occ = [torch.full((n, h, w), 9, dtype=torch.uint8, device=a.device) for _ in range(2)]
    s = torch.cuda.current_stream().cuda_stream
    # masks without the backward flow: it stays in the workspace
    ctx.run_bidir_ptr(a.data_ptr(), b.data_ptr(), n, w, h, p, 0.01, 0.5, out.data_ptr(), 0, occ[0].data_ptr(),
                      occ[1].data_ptr(), 0, 0, s)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(fw))
    assert np.array_equal(occ[0].cpu().numpy(), want[0]) and np.array_equal(occ[1].cpu().numpy(), want[1])
    # the backward flow alone
    obw = torch.zeros_like(out)
    out.zero_()
    ctx.run_bidir_ptr(a.data_ptr(), b.data_ptr(), n, w, h, p, 0.01, 0.5, out.data_ptr(), obw.data_ptr(), stream=s)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(fw)) and np.array_equal(_bits(obw.cpu().numpy()), _bits(bw))
    # nothing but the forward flow: the plain call
    out.zero_()
    ctx.run_bidir_ptr(a.data_ptr(), b.data_ptr(), n, w, h, p, 0.01, 0.5, out.data_ptr(), stream=s)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(fw))


def test_bidir_refusals(ctx):
    import of_dis_amd as od
    w, h = 160, 120
    a, b = od.synth_pair(w, h, 1, 0, od.MODE_OF)
    with pytest.raises(od.OfdisError) as e:
        ctx.run_bidir_host(a, b, od.oppoint(2, w, od.MODE_DE, 1))
    assert e.value.code == od._lib.ERR_UNSUPPORTED
    p = od.oppoint(2, w, od.MODE_OF, 1)
    for alpha, beta in ((-1.0, 0.5), (0.01, float("nan"))):
        with pytest.raises(od.OfdisError) as e:
            ctx.run_bidir_host(a, b, p, alpha, beta)
        assert e.value.code == od._lib.ERR_INVALID_ARGUMENT
    dis = {p.sc_l: np.zeros((h >> p.sc_l, w >> p.sc_l, 2), np.float32)}
    ctx.set_capture(dis, None)
    try:
        with pytest.raises(od.OfdisError) as e:
            ctx.run_bidir_host(a, b, p)
        assert e.value.code == od._lib.ERR_UNSUPPORTED
    finally:
        ctx.set_capture(None, None)
    got = ctx.run_bidir_host(a, b, p)  # the context still works
    check_result(got, ctx.run_host(a, b, p), ctx.run_host(b, a, p), what="after the refusals")


def test_bidir_meaning(ctx):
    """A pure translation by (8, 0): the strip whose target leaves the frame is flagged, the interior is trusted.
    The GPU flows are the oracle's bit for bit, so the figures are the CPU's exactly (0.962 and 0.896); the margins
    only guard against a change in the synthetic generator."""
    import of_dis_amd as od
    w, h = 192, 128
    a, b = od.synth_shift_pair(w, h, (8, 0), 1, 0)
    p = od.oppoint(2, w, od.MODE_OF, 1)
    occ_fw = ctx.run_bidir_host(a, b, p)[2]
    leaving = float((occ_fw[:, w - 8:] != 0).mean())   # x + 8 > w - 1
    interior = float((occ_fw[16:h - 16, 16:w - 16] == 0).mean())
    print(f"flagged where the target leaves the frame: {leaving:.3f}; consistent in the interior: {interior:.3f}")
    assert leaving >= 0.90
    assert interior >= 0.80

"""GPU parity of the packed-frames sweep-per-wave SOR (option sor_pack): several frames' rows in one workgroup.

With sor_pack a workgroup of k_tv_sor_lanes_pack runs F consecutive frames of the launch, their rows end to end as
V = F h virtual rows (v = f h + y) over ceil(V / 64) row groups.  What can go wrong is a frame offset, a border taken
from the virtual row instead of the lane's own row, a neighbour that crosses a frame boundary, a ring sized by h, the
partial last workgroup, and the launch rule.  So every call here is single-scale (sc_l = sc_f = 0: the one refinement
level is the frame; op-point 2's parameters, tv_solverit overridden), goes through the batched tensor entry point with
sor_pack = 2 (small batches pack too), every frame of a batch is a different image pair, and every frame is compared
bit for bit with the CPU oracle's run of that pair alone.

F is re-derived from the launch rule (sor_pack_frames: ofdis_kernels.hip) in `pack_frames`; per size the frame counts
are n = 1, F - 1, F, F + 1 and 2 F + 1 (F + 1 and 2 F + 1 leave a partial last workgroup).
"""
import numpy as np
import pytest

from test_gpu_parity import assert_bitexact

pytestmark = pytest.mark.gpu

PACK_GROUPS = 4  # kSorPackGroups


def pack_frames(h, S, sp=0):
    """sor_pack_frames at sor_pack = 2 with the coefficient ring on: frames per workgroup, 0 = one frame per workgroup."""
    if S > 3 or h < 2 or h > 128:
        return 0
    F = 64 * PACK_GROUPS // h
    G, G1 = -(-F * h // 64), -(-h // 64)
    if F < 2 or G * S > 16 or 4 * G > 3 * G1 * F or F * sp * 32 >= 1 << 31:
        return 0
    return F


SIZES = [
    (120, 68), (60, 34), (30, 17),     # config B's levels (1080p, scales 4 .. 6)
    (40, 30), (20, 15),                # config A's levels that pack
    (24, 16), (24, 32),                # a frame boundary on every wave boundary
    (24, 17), (24, 21), (24, 65),      # frames straddling wave boundaries
    (24, 128), (24, 129),              # the rule's edge: 128 rows have no lanes to fill, 129 is past h <= 128
    (17, 30), (12, 68),                # the unfolded layout (h > w)
    (3, 17), (2, 34),                  # narrower than the 6-step block
    (24, 2),                           # h = 2: every row a border row
]


def test_rule_restated():
    """The sizes meet the rule where the comments above say so (a CPU check of this file's own restatement)."""
    got = {(w, h): pack_frames(h, 3) for w, h in SIZES}
    assert got[(120, 68)] == 3 and got[(60, 34)] == 7 and got[(30, 17)] == 15
    assert got[(24, 128)] == 0 and got[(24, 129)] == 0 and got[(24, 65)] == 3 and got[(24, 2)] == 128
    assert all(pack_frames(h, 2) == f for (w, h), f in got.items())
    assert pack_frames(68, 4) == 0


def counts(h, S):
    F = pack_frames(h, S)
    return sorted({1, 2, 3}) if not F else sorted({1, F - 1, F, F + 1, 2 * F + 1} - {0})


@pytest.fixture(scope="module")
def od():
    import of_dis_amd
    return of_dis_amd


@pytest.fixture(scope="module")
def ctx(od):
    c = od.Context(0)
    yield c
    c.close()


def params(od, O, w, mode, S, sc=(0, 0)):
    p, q = od.oppoint(2, w, mode, 1), O.oppoint(2, w, mode, 1)
    for r in (p, q):
        r.sc_f, r.sc_l = sc
        r.tv_solverit = S
    return p, q


_PAIR, _REF = {}, {}


def pair(od, w, h, mode, i):
    """Frame i's image pair: synth scene i mod 8 (the scenes repeat with period 8), from the ninth frame on with the
    two low bits of every pixel replaced by noise seeded by i, so that no two frames of a batch are the same."""
    key = (w, h, mode, i)
    if key not in _PAIR:
        a, b = od.synth_pair(w, h, 1, i % 8, mode)
        if i >= 8:
            rng = np.random.default_rng(1000 + i)
            a = a ^ rng.integers(0, 4, a.shape, dtype=np.uint8)
            b = b ^ rng.integers(0, 4, b.shape, dtype=np.uint8)
        for x in (a, b):
            x.setflags(write=False)
        _PAIR[key] = (a, b)
    return _PAIR[key]


def reference(od, O, w, h, mode, S, i, sc=(0, 0)):
    """The oracle's flow of frame i alone, computed once and shared."""
    key = (w, h, mode, S, i, sc)
    if key not in _REF:
        a, b = pair(od, w, h, mode, i)
        ref = O.run_u8(a, b, params(od, O, w, mode, S, sc)[1])
        assert np.isfinite(ref).all(), key
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def batch(od, O, ctx, w, h, mode, S, n, options, sc=(0, 0)):
    """Frames 0 .. n - 1 in one call of the tensor entry point under `options` [(key, value, default)]."""
    import torch
    ps = [pair(od, w, h, mode, i) for i in range(n)]
    a = torch.from_numpy(np.stack([x[0] for x in ps])).cuda()
    b = torch.from_numpy(np.stack([x[1] for x in ps])).cuda()
    p = params(od, O, w, mode, S, sc)[0]
    assert od.validate(p) == 0
    for k, v, _ in options:
        ctx.set_option(k, v)
    try:
        out = ctx.run(a, b, p)
        torch.cuda.synchronize()
    finally:
        for k, _, d in options:
            ctx.set_option(k, d)
    return out.cpu().numpy()


def sweep(od, O, ctx, sizes, mode, S, options):
    """Every size at every frame count of `counts`; one assertion that lists every (size, n, frame) that differs."""
    bad = []
    for w, h in sizes:
        for n in counts(h, S):
            got = batch(od, O, ctx, w, h, mode, S, n, options)
            for i in range(n):
                ref = reference(od, O, w, h, mode, S, i)
                assert got[i].shape == ref.shape, (w, h, n, i, got[i].shape, ref.shape)
                k = int((got[i].view(np.uint32) != ref.view(np.uint32)).sum())
                if k:
                    bad.append(f"{w}x{h} n {n} frame {i}: {k} / {ref.size} values differ")
    assert not bad, f"mode {mode} S {S} {[o[:2] for o in options]}: {len(bad)} frames differ:\n" + "\n".join(bad[:40])


MODES = [pytest.param(1, id="flow"), pytest.param(2, id="depth")]


@pytest.mark.parametrize("cring", [2, 3])
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("mode", MODES)
def test_packed_levels(oracle, od, ctx, mode, S, cring):
    """Every size and frame count on the packed form, lane-constant load slots (sor_cring 2: these launches have fewer
    frames than CUs) and the clamped in-frame loads (3)."""
    sweep(od, oracle, ctx, SIZES, mode, S, [("sor_pack", 2, 1), ("sor_cring", cring, 2)])


FALLBACK = [(120, 68), (30, 17), (24, 21), (17, 30)]


@pytest.mark.parametrize("S,cring", [(4, 2), (3, 0), (2, 0)], ids=["S4", "S3-noring", "S2-noring"])
@pytest.mark.parametrize("mode", MODES)
def test_unpacked_forms_under_sor_pack_2(oracle, od, ctx, mode, S, cring):
    """Four sweeps and sor_cring = 0 have no packed form: sor_pack = 2 leaves them on the one-frame kernels.  The
    frame counts are those of the three-sweep rule."""
    bad = []
    opts = [("sor_pack", 2, 1), ("sor_cring", cring, 2)]
    for w, h in FALLBACK:
        for n in counts(h, 3):
            got = batch(od, oracle, ctx, w, h, mode, S, n, opts)
            for i in range(n):
                ref = reference(od, oracle, w, h, mode, S, i)
                if not np.array_equal(got[i].view(np.uint32), ref.view(np.uint32)):
                    bad.append((w, h, n, i))
    assert not bad, bad


def test_sor_pack_values_agree(oracle, od, ctx):
    """sor_pack 0, 1 and 2 on a 5-frame 120x68 batch: identical bits, and the oracle's."""
    outs = [batch(od, oracle, ctx, 120, 68, 1, 3, 5, [("sor_pack", v, 1)]) for v in (0, 1, 2)]
    for v in (1, 2):
        assert np.array_equal(outs[0].view(np.uint32), outs[v].view(np.uint32)), f"sor_pack {v} against 0"
    for i in range(5):
        assert_bitexact(outs[2][i], reference(od, oracle, 120, 68, 1, 3, i), f"frame {i}")


def test_single_frame_default_rule(oracle, od, ctx):
    """One frame at the default rule (fewer frames than CUs: the one-frame kernels): sor_pack 1 against 0, and the
    oracle."""
    one, zero = (batch(od, oracle, ctx, 120, 68, 1, 3, 1, [("sor_pack", v, 1)]) for v in (1, 0))
    assert np.array_equal(one.view(np.uint32), zero.view(np.uint32))
    assert_bitexact(one[0], reference(od, oracle, 120, 68, 1, 3, 0), "frame 0")


ND = 4  # distinct scenes of the oversubscribed batch


@pytest.mark.parametrize("mode", MODES)
def test_rule_in_earnest(oracle, od, ctx, mode):
    """CUs + 1 frames of 120x68 with a three-level pyramid (120x68, 60x34, 30x17) at the default options: every SOR
    launch has more frames than CUs, so the default rule packs all three levels (F = 3, 7, 15; the last workgroup of
    each launch is partial for 257 frames).  Frames 0 .. ND - 1 and the last against the oracle, every other frame f
    against frame f % ND on the device."""
    import torch
    w, h, S, sc = 120, 68, 3, (2, 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus + 1
    p = params(od, oracle, w, mode, S, sc)[0]
    assert od.validate(p) == 0 and od.max_frames_per_launch(p, w, h) >= n
    assert all(pack_frames(h >> s, S) for s in range(3))
    ps = [pair(od, w, h, mode, i) for i in range(ND)]
    idx = torch.arange(n, device="cuda") % ND
    a = torch.from_numpy(np.stack([x[0] for x in ps])).cuda()[idx]
    b = torch.from_numpy(np.stack([x[1] for x in ps])).cuda()[idx]
    ctx.set_option("streams", 1)
    ctx.set_option("chunk", 0)
    try:
        out = ctx.run(a, b, p)
        torch.cuda.synchronize()
    finally:
        ctx.set_option("streams", 0)
    for i in list(range(ND)) + [n - 1]:
        assert_bitexact(out[i].cpu().numpy(), reference(od, oracle, w, h, mode, S, i % ND, sc), f"frame {i} of {n}")
    ov = out.view(n, -1).view(torch.int32)
    same = (ov == ov[:ND][idx]).all(dim=1)
    assert bool(same.all()), [int(f) for f in torch.nonzero(~same).flatten()[:10]]

"""Parity on degenerate image content: the inputs that drive the patch solves' fallback branches.

Every other parity test runs `synth_pair` scenes (smooth texture, a little noise, a few pixels of motion), on
which no 2x2 factorisation ever fails and no Hessian is singular (test_synth_scenes_never_fail_a_factorisation
keeps that on record).  The patterns below are ordinary inputs -- hatching, stripes, screen content, noise,
saturated and occluded frames -- on which they do, thousands of times per frame.  The oracle counts its branches
(pyoracle.patch_stats), so the CPU half of this file proves that each pattern reaches the branch it is here for,
and the GPU half compares the library with the oracle bit for bit on exactly those inputs: per stage, in mixed
batches, under every patch option, in latency mode and through run_bidir.

The oracle's output is finite on every (pattern, case) of the matrix; that is a condition of the matrix (a
pattern that broke it would be replaced), so the GPU comparison is a plain bit comparison with nothing masked.
"""
import numpy as np
import pytest

from test_gpu_parity import CASES as SYNTH_CASES
from test_gpu_parity import assert_bitexact
from test_gpu_patch_shapes import shape_params

# ------------------------------------------------------------------------------------------------ generators


def _hash_u8(h, w, noc, seed):
    """Uniform u8 [h][w][noc] from an integer hash of (x, y, c, seed): the bytes depend on no library RNG."""
    M = np.uint64(0xFFFFFFFF)
    y, x, c = np.ogrid[0:h, 0:w, 0:noc]
    v = (x.astype(np.uint64) * np.uint64(0x9E3779B1) + y.astype(np.uint64) * np.uint64(0x85EBCA77) +
         c.astype(np.uint64) * np.uint64(0xC2B2AE3D) + np.uint64(seed) * np.uint64(0x27D4EB2F) + np.uint64(0x165667B1)) & M
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(0x2C1B3C6D)) & M
    v ^= v >> np.uint64(12)
    v = (v * np.uint64(0x297A2D39)) & M
    v ^= v >> np.uint64(15)
    return (v >> np.uint64(24)).astype(np.uint8)


def _gray(img2d, noc):
    """A structured pattern: the same values in every channel."""
    return np.ascontiguousarray(np.repeat(np.asarray(img2d).astype(np.uint8)[:, :, None], noc, axis=2))


def _blocks(h, w, noc, seed):
    """4x4 blocks of uniform u8."""
    return np.ascontiguousarray(_hash_u8((h + 3) // 4, (w + 3) // 4, noc, seed).repeat(4, 0).repeat(4, 1)[:h, :w])


# The seed of the block frames (bigshift, occl): the first of 3, 4, .. with which both depth cases start patches
# out of bounds (seeds 3 .. 6 give oob_start = 0 on one of them; chosen on the oracle's counters alone).
BLOCK_SEED = 7


def _synth(od, w, h, noc, mode, frame=3):
    return od.synth_pair(w, h, noc, frame, mode)


def make_pair(od, name, w, h, noc, mode):
    y, x = np.mgrid[0:h, 0:w]
    if name == "diag":
        a = _gray(255 * (((x + y) // 3) % 2), noc)
        return a, np.roll(a, 2, axis=1)
    if name == "antidiag":
        a = _gray(255 * (((x - y) // 3) % 2), noc)
        return a, np.roll(a, 1, axis=0)
    if name == "diagramp":
        a = _gray((x + y) % 256, noc)
        return a, np.roll(a, 3, axis=1)
    if name == "vstripe":
        a = _gray(255 * ((x // 3) % 2), noc)
        return a, np.roll(a, 1, axis=1)
    if name == "hstripe":
        a = _gray(255 * ((y // 3) % 2), noc)
        return a, np.roll(a, 1, axis=0)
    if name == "checker1":
        a = _gray(255 * ((x + y) % 2), noc)
        return a, 255 - a
    if name == "noise":
        return _hash_u8(h, w, noc, 1), _hash_u8(h, w, noc, 2)
    if name == "bigshift":
        a = _blocks(h, w, noc, BLOCK_SEED)
        return a, np.roll(a, (23, 37), axis=(0, 1))
    if name == "const_vs_noise":
        return np.full((h, w, noc), 128, np.uint8), _hash_u8(h, w, noc, 4)
    if name == "sat":
        return np.full((h, w, noc), 255, np.uint8), np.zeros((h, w, noc), np.uint8)
    if name == "occl":
        a = _blocks(h, w, noc, BLOCK_SEED)
        b = a.copy()
        b[:, w // 2:] = 0
        return a, b
    if name == "mixed":  # one wave holds failing and ordinary patches side by side
        da, db = make_pair(od, "diag", w, h, noc, mode)
        sa, sb = _synth(od, w, h, noc, mode)
        a, b = sa.copy(), sb.copy()
        a[:, : w // 2] = da[:, : w // 2]
        b[:, : w // 2] = db[:, : w // 2]
        return a, b
    if name == "synth":
        return _synth(od, w, h, noc, mode)
    raise KeyError(name)


PATTERNS = ["diag", "antidiag", "diagramp", "vstripe", "hstripe", "checker1", "noise", "bigshift", "const_vs_noise",
            "sat", "occl", "mixed"]

CASES = [
    # (w, h, noc, mode, oppoint, overrides, patch size or None for the op-point's)
    (160, 120, 1, 1, 2, {}, None),                        # 0: gray p = 8 (k_patchq)
    (192, 128, 1, 1, 3, {"costfct": 1}, None),            # 1: gray p = 12, L1 (k_patchq)
    (192, 128, 3, 1, 3, {"costfct": 1}, None),            # 2: RGB p = 12, L1 (k_patchx)
    (240, 120, 1, 2, 4, {}, None),                        # 3: depth p = 12, 128 iterations
    (240, 120, 3, 2, 2, {}, None),                        # 4: RGB depth p = 8 (k_patchw)
    (160, 120, 1, 1, 2, {"usefbcon": 1}, None),           # 5: forward-backward merging
    (160, 120, 1, 1, 2, {"patnorm": 0, "costfct": 2}, None),  # 6: no mean normalisation, pseudo-Huber
    (160, 120, 1, 1, 2, {"min_iter": 2, "dp_thresh": 0.3, "dr_thresh": 0.9}, None),  # 7: early stopping
    (160, 120, 1, 1, 2, {}, 10),                          # 8: k_patch8
    (160, 120, 1, 1, 2, {}, 16),                          # 9: k_patch (one wave per patch)
    (192, 128, 3, 1, 3, {"costfct": 1}, 14),              # 10: k_patchg (p * p * noc = 588 > 448)
]
EARLY = 7
CASE_IDS = [f"c{i}" for i in range(len(CASES))]


def case_params(od, O, ci):
    w, h, noc, mode, op, over, p = CASES[ci]
    if p is not None:
        return shape_params(od, O, w, noc, mode, op, p, over)
    pg, pq = od.oppoint(op, w, mode, noc), O.oppoint(op, w, mode, noc)
    for k, v in over.items():
        setattr(pg, k, v)
        setattr(pq, k, v)
    return pg, pq


_PAIRS = {}
_ORACLE = {}


def pair_of(od, name, ci):
    key = (name, ci)
    if key not in _PAIRS:
        w, h, noc, mode = CASES[ci][:4]
        a, b = make_pair(od, name, w, h, noc, mode)
        assert a.shape == (h, w, noc) and a.dtype == np.uint8 and b.shape == a.shape and b.dtype == np.uint8
        a.setflags(write=False)
        b.setflags(write=False)
        _PAIRS[key] = (a, b)
    return _PAIRS[key]


def oracle_of(od, O, name, ci):
    """(flow, flow per scale after aggregation, after TV, branch counts) of one (pattern, case): computed once,
    shared by every test of the module and never written to."""
    key = (name, ci)
    if key not in _ORACLE:
        a, b = pair_of(od, name, ci)
        O.patch_stats_reset()
        ref, cap_d, cap_t = O.run_u8(a, b, case_params(od, O, ci)[1], capture=True)
        stats = O.patch_stats()
        for v in [ref] + list(cap_d.values()) + list(cap_t.values()):
            v.setflags(write=False)
        _ORACLE[key] = (ref, cap_d, cap_t, stats)
    return _ORACLE[key]


@pytest.fixture(scope="module")
def od():
    import of_dis_amd
    return of_dis_amd


# ------------------------------------------------------------------------------------------------ CPU tests


def test_generators_are_what_the_table_says(od):
    a, b = make_pair(od, "diag", 16, 12, 3, 1)
    assert a[0, :7, 0].tolist() == [0, 0, 0, 255, 255, 255, 0] and a[1, 2, 1] == 255 and (a[..., 0] == a[..., 2]).all()
    assert np.array_equal(b[:, 2:], a[:, :-2]) and np.array_equal(b[:, :2], a[:, -2:])
    a, b = make_pair(od, "bigshift", 64, 48, 1, 1)
    assert (a[:4, :4] == a[0, 0]).all() and np.array_equal(b[23:, 37:], a[:-23, :-37])
    n = _hash_u8(120, 160, 3, 1)
    assert n[0, 0].tolist() != n[0, 1].tolist() and abs(float(n.mean()) - 127.5) < 1.0 and len(np.unique(n)) == 256
    assert not np.array_equal(n[..., 0], n[..., 1])
    # the bytes themselves, in plain Python integers: they may never move with a numpy version
    M = 0xFFFFFFFF
    for (x, y, c, seed) in ((0, 0, 0, 7), (2, 1, 0, 7), (159, 119, 2, 1)):
        v = (x * 0x9E3779B1 + y * 0x85EBCA77 + c * 0xC2B2AE3D + seed * 0x27D4EB2F + 0x165667B1) & M
        v ^= v >> 15
        v = (v * 0x2C1B3C6D) & M
        v ^= v >> 12
        v = (v * 0x297A2D39) & M
        v ^= v >> 15
        assert int(_hash_u8(y + 1, x + 1, c + 1, seed)[y, x, c]) == v >> 24


@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
@pytest.mark.parametrize("name", PATTERNS)
def test_oracle_output_is_finite(oracle, od, name, ci):
    ref, cap_d, cap_t, stats = oracle_of(od, oracle, name, ci)
    for what, v in [("flow", ref)] + [(f"dis {s}", x) for s, x in cap_d.items()] + \
            [(f"tv {s}", x) for s, x in cap_t.items()]:
        assert np.isfinite(v).all(), (name, CASES[ci], what, int((~np.isfinite(v)).sum()))
    assert stats["nonfinite_delta"] == 0, stats


def _is_flow(ci):
    return CASES[ci][3] == 1


def _is_gray(ci):
    return CASES[ci][2] == 1


# (pattern, case) -> counters that must be at least 1 there
def _targets():
    t = {}

    def want(name, ci, *keys):
        t.setdefault((name, ci), set()).update(keys)

    for ci in range(len(CASES)):
        if _is_flow(ci):
            # a failed 2x2 factorisation: gradients along one diagonal only, H is singular up to rounding
            if _is_gray(ci):
                for name in ("diag", "antidiag", "diagramp"):
                    want(name, ci, "llt_failed")
            else:
                want("diagramp", ci, "llt_failed")
            # det == 0 exactly: one gradient (stripes) or both (checker at one pixel: Sobel of a period-2 signal;
            # constant frames) are zero
            for name in ("vstripe", "hstripe", "checker1", "sat", "const_vs_noise"):
                want(name, ci, "hess_regularised")
        else:
            # depth regularises on H00 == 0: every pattern above but vstripe has no horizontal gradient
            for name in ("hstripe", "checker1", "sat", "const_vs_noise"):
                want(name, ci, "hess_regularised")
            # patches that start, step or are thrown out of bounds.  The op-point-4 depth case (128 iterations on
            # five scales) reaches all three on each pattern; the RGB op-point-2 one (p = 8, 12 iterations, three
            # scales) only on the block shift: its diag / noise counts are in DESIGN.md section 5
            for name in ("bigshift", "noise", "diag") if CASES[ci][4] == 4 else ("bigshift",):
                want(name, ci, "oob_start", "outlier_reset", "oob_iter")
    for name in PATTERNS:
        want(name, EARLY, "early_stop")
    return t


TARGETS = _targets()


@pytest.mark.parametrize("name,ci", sorted(TARGETS), ids=lambda v: v if isinstance(v, str) else f"c{v}")
def test_pattern_reaches_its_branch(oracle, od, name, ci):
    stats = oracle_of(od, oracle, name, ci)[3]
    print(name, CASES[ci], stats)
    for key in sorted(TARGETS[(name, ci)]):
        assert stats[key] >= 1, (name, CASES[ci], key, stats)


def test_synth_scenes_never_fail_a_factorisation(oracle, od):
    """Why this file exists: on the scenes of every other parity test no factorisation fails and no Hessian is
    regularised, so the solves' fallbacks only ever saw zeros."""
    total = dict.fromkeys(oracle.PATCH_STATS, 0)
    for w, h, noc, mode, op, over in SYNTH_CASES:
        a, b = od.synth_pair(w, h, noc, 3, mode)
        q = oracle.oppoint(op, w, mode, noc)
        for k, v in over.items():
            setattr(q, k, v)
        oracle.patch_stats_reset()
        oracle.run_u8(a, b, q)
        st = oracle.patch_stats()
        assert st["llt_failed"] == 0 and st["hess_regularised"] == 0, ((w, h, noc, mode, op, over), st)
        for k in total:
            total[k] += st[k]
    print("synth scenes, frame 3, all of test_gpu_parity.CASES:", total)
    assert total["oob_start"] >= 1 and total["outlier_reset"] >= 1  # the counters do count


# ------------------------------------------------------------------------------------------------ GPU tests


@pytest.fixture(scope="module")
def ctx(od):
    c = od.Context(0)
    yield c
    c.close()


def _run_captured(ctx, a, b, pg, cap_d, cap_t):
    dis = {s: np.zeros_like(v) for s, v in cap_d.items()}
    tv = {s: np.zeros_like(v) for s, v in cap_t.items()}
    ctx.set_capture(dis, tv)
    try:
        got = ctx.run_host(a, b, pg)
    finally:
        ctx.set_capture(None, None)
    return got, dis, tv


def _check_stages(tag, got, dis, tv, ref, cap_d, cap_t):
    for s in sorted(cap_d, reverse=True):
        assert_bitexact(dis[s], cap_d[s], f"{tag}: scale {s} after aggregation")
        assert_bitexact(tv[s], cap_t[s], f"{tag}: scale {s} after TV refinement")
    assert_bitexact(got, ref, f"{tag}: full-resolution flow")


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
@pytest.mark.parametrize("name", PATTERNS)
def test_single_pair_bitexact(oracle, od, ctx, name, ci):
    """Every (pattern, case) alone, stage by stage: a difference names the scale and the stage."""
    a, b = pair_of(od, name, ci)
    ref, cap_d, cap_t, _ = oracle_of(od, oracle, name, ci)
    got, dis, tv = _run_captured(ctx, a, b, case_params(od, oracle, ci)[0], cap_d, cap_t)
    _check_stages(f"{name} {CASES[ci]}", got, dis, tv, ref, cap_d, cap_t)


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=CASE_IDS)
@pytest.mark.parametrize("names", [("synth", "diag", "mixed"), ("bigshift", "synth", "diagramp")], ids="+".join)
def test_mixed_batches_bitexact(oracle, od, ctx, names, ci):
    """Batches of three with degenerate frames at index > 0 beside an ordinary one: the calls where a workgroup
    straddles a degenerate and an ordinary frame.  Each frame equals the oracle's run of that frame alone."""
    import torch
    pairs = [pair_of(od, n, ci) for n in names]
    a = torch.from_numpy(np.stack([x[0] for x in pairs])).cuda()
    b = torch.from_numpy(np.stack([x[1] for x in pairs])).cuda()
    out = ctx.run(a, b, case_params(od, oracle, ci)[0])
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    for f, n in enumerate(names):
        assert_bitexact(out[f], oracle_of(od, oracle, n, ci)[0], f"{names} {CASES[ci]}: frame {f} ({n})")


def _touches(option, ci):
    """Whether a patch option changes the kernels that case ci runs (launch_patch's rules)."""
    w, h, noc, mode, op, over, p = CASES[ci]
    ps = p if p is not None else (12 if op >= 3 else 8)
    key = option[0]
    if key == "patch_quad":      # k_patchq: gray p = 8 / 12
        return noc == 1 and ps in (8, 12)
    if key == "patch_x16":       # k_patchx: RGB p = 12
        return noc == 3 and ps == 12
    if key == "patch_window":    # the LDS-windowed forms: p = 8 / 12
        return ps in (8, 12)
    if key == "patch_absw":      # aggregation weights written by k_patchq / k_patchx
        return (noc == 1 and ps in (8, 12)) or (noc == 3 and ps == 12)
    if key == "wave_per_patch":  # k_patch holds p * p * noc <= 448 values
        return ps * ps * noc <= 448
    return True                  # patch_fdiv, patch_maxres, patch_generic, agg_stage: every family


OPTIONS = [  # (option, value, default)
    ("patch_fdiv", 0, 1), ("patch_maxres", 0, 1), ("patch_quad", 0, 1), ("patch_x16", 0, 1), ("patch_x16", 2, 1),
    ("patch_generic", 1, 0), ("wave_per_patch", 1, 0), ("patch_window", 0, 1), ("patch_absw", 0, 1),
    ("agg_stage", 0, 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("option,ci", [(o, ci) for o in OPTIONS for ci in range(len(CASES)) if _touches(o, ci)],
                         ids=lambda v: f"c{v}" if isinstance(v, int) else f"{v[0]}={v[1]}")
def test_patch_options_bitexact(oracle, od, ctx, option, ci):
    """The non-default patch kernels and solve forms on the failing-factorisation patterns, per stage, for the
    cases whose kernels the option changes (_touches)."""
    key, val, default = option
    pg = case_params(od, oracle, ci)[0]
    ctx.set_option(key, val)
    try:
        for name in ("diag", "diagramp", "mixed", "bigshift"):
            a, b = pair_of(od, name, ci)
            ref, cap_d, cap_t, _ = oracle_of(od, oracle, name, ci)
            got, dis, tv = _run_captured(ctx, a, b, pg, cap_d, cap_t)
            _check_stages(f"{key}={val} {name} {CASES[ci]}", got, dis, tv, ref, cap_d, cap_t)
    finally:
        ctx.set_option(key, default)


@pytest.mark.gpu
@pytest.mark.parametrize("ci", [0, 5, 6, 7], ids=lambda i: f"c{i}")
@pytest.mark.parametrize("name", ["checker1", "sat", "diag", "noise"])
def test_latency_mode_bitexact(oracle, od, ctx, name, ci):
    """sor_mode = 1 against the oracle under its red-black order, on the largest (checker, noise) and the zero
    (sat) image gradients the TV kernels can see."""
    a, b = pair_of(od, name, ci)
    pg, pq = case_params(od, oracle, ci)
    with oracle.sor_order(1):
        ref, cap_d, cap_t = oracle.run_u8(a, b, pq, capture=True)
    ctx.set_option("sor_mode", 1)
    try:
        got, dis, tv = _run_captured(ctx, a, b, pg, cap_d, cap_t)
    finally:
        ctx.set_option("sor_mode", 0)
    _check_stages(f"sor_mode=1 {name} {CASES[ci]}", got, dis, tv, ref, cap_d, cap_t)


@pytest.mark.gpu
@pytest.mark.parametrize("ci", [i for i in range(len(CASES)) if _is_flow(i)], ids=lambda i: f"c{i}")
@pytest.mark.parametrize("name", ["diag", "occl"])
def test_bidir_equals_two_plain_calls(oracle, od, ctx, name, ci):
    """Context.run_bidir on a failing-factorisation and an occluded pair: the two plain calls, bit for bit."""
    from test_gpu_bidir import check_result
    a, b = pair_of(od, name, ci)
    pg = case_params(od, oracle, ci)[0]
    fw, bw = ctx.run_host(a, b, pg), ctx.run_host(b, a, pg)
    got = ctx.run_bidir_host(a, b, pg, want_err=True)
    check_result(got, fw, bw, what=f"{name} {CASES[ci]}")

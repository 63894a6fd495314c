"""Parity off the op-points: the stopping test, the TV weights and the sweep counts of the 20-value parameter list.

Every other parity test runs parameter sets shaped like the four op-points (min_iter == max_iter, res_thresh == 0,
tv_alpha / tv_gamma / tv_delta = 10 / 10 / 5, tv_solverit in 2 .. 4).  The cases below leave them one way at a time:

* stopping cases -- res_thresh > 0 alone (`res`: the bits of the mean absolute residual decide which patch stops) and
  with the two rate tests (`res3`), the rate tests alone on the RGB and depth kernels (`rate_*`), and the stops that
  the first evaluation at cnt == 0 decides: max_iter = 0 (`max0`), min_iter = 0 (`min0`: delta_p is still zero, and
  0 / 1e-10 < dp_thresh^2), res_thresh = 1e4 (`r1e4`), beside max_iter = 1 (`max1`) and min_iter = 9 > max_iter = 4
  (`min9`), on every patch kernel family (FAMILIES);
* TV cases -- tv_gamma = 0, tv_delta = 0, both, other weights, tv_alpha 0.01 and 25, tv_solverit 0 / 1 / 5 / 7 and
  tv_innerit = 0, on gray flow, RGB flow and gray depth.

This file is the CPU half: the oracle's stop-reason counters (pyoracle.stop_stats) prove on the oracle alone that
each case reaches the branch it is named for, with stopped and running patches side by side, and that every output
is finite, so that the GPU half (test_gpu_offpoint.py) is a plain bit comparison on exactly these inputs.

The res_thresh of a family (RES) is chosen from the oracle's own residuals on the synth scene: the smallest multiple of
RES_STEP under which the oracle meets the conditions (`unmet`) of the three cases that carry it
(test_res_thresholds_follow_the_rule restates the rule and the search).

Measured on the oracle (synth scene unless marked; the rate cases meet their conditions on the mixed one, see
`unmet`).  Columns: started patches | stops at cnt == 0, at max_iter | stops with the residual, the dp and the dr term
false (share of the started patches) | dp or dr stops at cnt == min_iter, patches that iterate on after it.  The
max0 / min0 / r1e4 cases stop every started patch at cnt == 0 (min0 under dp, r1e4 under the residual), max1 stops
every one at max_iter.
  res-f0                400 |   121   189 |   205 (51 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  res3-f0               400 |   118     0 |   166 (42 %)    39 (10 %)   231 (58 %) |   224    22
  min9-f0               400 |   115   231 |   169 (42 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  res-f1               3632 |    41  3375 |   229 ( 6 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  res3-f1              3632 |    51     0 |   138 ( 4 %)   219 ( 6 %)  3481 (96 %) |  3425    88
  min9-f1              3632 |    41  3494 |   138 ( 4 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  res-f2               3616 |   484  2839 |   750 (21 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  res3-f2              3613 |   434     0 |   663 (18 %)    20 ( 1 %)  2961 (82 %) |  2920   113
  min9-f2              3599 |   461  2927 |   662 (18 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  res-f3                602 |    95   470 |   128 (21 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  res3-f3               602 |    95     0 |   126 (21 %)   164 (27 %)   474 (79 %) |   471    10
  min9-f3               602 |    96   478 |   124 (21 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  res-f4               4250 |   154  4060 |   186 ( 4 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  res3-f4              4250 |   152     0 |   178 ( 4 %)    70 ( 2 %)  4060 (96 %) |  3987    94
  min9-f4              4250 |   149  4073 |   176 ( 4 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  res-f5                715 |    74   592 |   120 (17 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  res3-f5               715 |    69     0 |   102 (14 %)    25 ( 3 %)   612 (86 %) |   594    21
  min9-f5               715 |    70   608 |   107 (15 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  res-f6                335 |    80   198 |   137 (41 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  res3-f6               335 |    77     0 |   100 (30 %)     9 ( 3 %)   240 (72 %) |   236     6
  min9-f6               335 |    81   226 |   109 (33 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  res-f7               3632 |   541  2865 |   731 (20 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  res3-f7              3632 |   494     0 |   680 (19 %)    31 ( 1 %)  2974 (82 %) |  2924   122
  min9-f7              3632 |   508  2959 |   673 (19 %)     0 ( 0 %)     0 ( 0 %) |     0     0
  rate_l1-f2           3603 |     0     0 |     0 ( 0 %)   160 ( 4 %)  3562 (99 %) |  3431   159
  rate_l1-f2 mixed     3603 |     0     0 |     0 ( 0 %)   204 ( 6 %)  3519 (98 %) |  3375   215
  rate_huber-f2        3599 |     0     0 |     0 ( 0 %)   357 (10 %)  3445 (96 %) |  3551    38
  rate_huber-f2 mixed  3599 |     0     0 |     0 ( 0 %)   590 (16 %)  3451 (96 %) |  3298   291
  rate_fb-f2           7240 |     0     0 |     0 ( 0 %)   341 ( 5 %)  7158 (99 %) |  6900   304
  rate_fb-f2 mixed     7240 |     0     0 |     0 ( 0 %)   309 ( 4 %)  7138 (99 %) |  6810   412
  rate_l1-f3            602 |     0     0 |     0 ( 0 %)   135 (22 %)   595 (99 %) |   578    24
  rate_l1-f3 mixed      602 |     0     0 |     0 ( 0 %)   171 (28 %)   577 (96 %) |   487   115
  rate_huber-f3         602 |     0     0 |     0 ( 0 %)   234 (39 %)   577 (96 %) |   591    11
  rate_huber-f3 mixed   602 |     0     0 |     0 ( 0 %)   204 (34 %)   556 (92 %) |   459   143
  rate_fb-f3           1204 |     0     0 |     0 ( 0 %)   484 (40 %)  1171 (97 %) |  1179    25
  rate_fb-f3 mixed     1204 |     0     0 |    16 ( 1 %)   349 (29 %)  1096 (91 %) |  1033    97
  rate_l1-f4           4250 |     0     0 |     0 ( 0 %)    67 ( 2 %)  4235 (100 %) |  4207    43
  rate_l1-f4 mixed     4250 |     2     0 |     2 ( 0 %)   842 (20 %)  4122 (97 %) |  3381   867
  rate_huber-f4        4250 |     0     0 |     0 ( 0 %)   117 ( 3 %)  4216 (99 %) |  4145   105
  rate_huber-f4 mixed  4250 |     0     0 |     7 ( 0 %)  1808 (43 %)  2773 (65 %) |  3331   916
  rate_fb-f4           8487 |     0     0 |     0 ( 0 %)   239 ( 3 %)  8426 (99 %) |  8266   221
  rate_fb-f4 mixed     8473 |     0     0 |    74 ( 1 %)  3379 (40 %)  5584 (66 %) |  5872  2511
"""
import numpy as np
import pytest

from test_degenerate_content import make_pair
from test_gpu_patch_shapes import shape_params

# (w, h, noc, mode, oppoint, overrides, patch size or None for the op-point's): one per patch kernel family
FAMILIES = [
    (160, 120, 1, 1, 2, {}, None),                                  # 0: k_patchq, p = 8
    (192, 128, 1, 1, 3, {}, None),                                  # 1: k_patchq, p = 12
    (192, 128, 3, 1, 3, {"costfct": 1}, None),                      # 2: k_patchx (RGB p = 12, L1)
    (240, 120, 3, 2, 2, {}, None),                                  # 3: RGB k_patchw, depth
    (240, 120, 1, 2, 4, {"max_iter": 16, "min_iter": 16}, None),    # 4: gray depth, p = 12
    (160, 120, 1, 1, 2, {}, 10),                                    # 5: k_patch8
    (160, 120, 1, 1, 2, {}, 16),                                    # 6: k_patch, one wave per patch
    (192, 128, 3, 1, 3, {"costfct": 1}, 14),                        # 7: k_patchg (p * p * noc = 588 > 448)
]
GRAY_FLOW, RGB_FLOW, GRAY_DEPTH = 0, 2, 4

# res_thresh per family (module docstring; the candidates are multiples of RES_STEP)
RES = {0: 0.875, 1: 0.875, 2: 1.0, 3: 0.625, 4: 0.625, 5: 1.0, 6: 1.75, 7: 1.0}
RES_STEP = 0.125

RATES = {"min_iter": 2, "dp_thresh": 0.3, "dr_thresh": 0.9}


# the cases that carry a family's res_thresh: (kind, overrides as a function of it)
RES_KINDS = [
    ("res", lambda r: {"res_thresh": r}),
    ("res3", lambda r: dict(RATES, res_thresh=r)),
    ("min9", lambda r: {"min_iter": 9, "max_iter": 4, "dp_thresh": 0.3, "dr_thresh": 0.9, "res_thresh": r}),
]


def _stopping_cases():
    cases = []
    for f in range(len(FAMILIES)):
        cases += [(f"{kind}-f{f}", f, kind, over(RES[f])) for kind, over in RES_KINDS]
        cases += [
            (f"max0-f{f}", f, "cnt0", {"max_iter": 0}),
            (f"max1-f{f}", f, "max1", {"max_iter": 1}),
            (f"min0-f{f}", f, "cnt0", {"min_iter": 0}),
            (f"r1e4-f{f}", f, "cnt0", {"res_thresh": 1e4}),
        ]
    for f in (RGB_FLOW, 3, GRAY_DEPTH):  # the rate tests alone on the RGB and depth families
        cases += [
            (f"rate_l1-f{f}", f, "rate", dict(RATES, costfct=1)),
            (f"rate_huber-f{f}", f, "rate", dict(RATES, costfct=2)),
            (f"rate_fb-f{f}", f, "rate", dict(RATES, usefbcon=1)),
        ]
    return cases


TV_KINDS = [
    ("gamma0", {"tv_gamma": 0.0}),
    ("delta0", {"tv_delta": 0.0}),
    ("gamma0delta0", {"tv_gamma": 0.0, "tv_delta": 0.0}),
    ("weights", {"tv_alpha": 3.7, "tv_gamma": 0.3, "tv_delta": 21.0}),
    ("alpha001", {"tv_alpha": 0.01}),
    ("alpha25", {"tv_alpha": 25.0}),
    ("sweeps0", {"tv_solverit": 0}),
    ("sweeps1", {"tv_solverit": 1}),
    ("sweeps5", {"tv_solverit": 5}),
    ("sweeps7", {"tv_solverit": 7}),
    ("inner0", {"tv_innerit": 0}),
]
TV_FAMILIES = (GRAY_FLOW, RGB_FLOW, GRAY_DEPTH)

STOP_CASES = _stopping_cases()
TV_CASES = [(f"{k}-f{f}", f, "tv", over) for f in TV_FAMILIES for k, over in TV_KINDS]
DEFAULT_CASES = [(f"default-f{f}", f, "default", {}) for f in range(len(FAMILIES))]
CASES = {c[0]: c for c in STOP_CASES + TV_CASES + DEFAULT_CASES}
STOP_IDS = [c[0] for c in STOP_CASES]
TV_IDS = [c[0] for c in TV_CASES]
SCENES = ("synth", "mixed", "const")
RATE_SCENE = "mixed"  # where the rate cases meet their conditions (unmet)


def family_params(od, O, f, over):
    """(library, oracle) parameters: the family's, then the overrides."""
    w, h, noc, mode, op, base, p = FAMILIES[f]
    over = dict(base, **over)
    if p is not None:
        return shape_params(od, O, w, noc, mode, op, p, over)
    pg, pq = od.oppoint(op, w, mode, noc), O.oppoint(op, w, mode, noc)
    for k, v in over.items():
        setattr(pg, k, v)
        setattr(pq, k, v)
    return pg, pq


def case_params(od, O, cid):
    return family_params(od, O, CASES[cid][1], CASES[cid][3])


_PAIRS = {}
_ORACLE = {}


def pair_of(od, scene, f):
    """The image pair of a scene at a family's shape, shared and read-only.  `const` is a constant frame twice."""
    key = (scene, f)
    if key not in _PAIRS:
        w, h, noc, mode = FAMILIES[f][:4]
        if scene == "const":
            a = np.full((h, w, noc), 128, np.uint8)
            b = a.copy()
        else:
            a, b = make_pair(od, scene, w, h, noc, mode)
        for x in (a, b):
            x.setflags(write=False)
        _PAIRS[key] = (a, b)
    return _PAIRS[key]


def oracle_of(od, O, cid, scene="synth", order=0):
    """(flow, flow per scale after aggregation, after TV, stop counters, branch counters) of a (case, scene) under
    a SOR order: computed once, shared by both halves and never written to."""
    key = (cid, scene, order)
    if key not in _ORACLE:
        a, b = pair_of(od, scene, CASES[cid][1])
        O.stop_stats_reset()
        O.patch_stats_reset()
        with O.sor_order(order):
            ref, cap_d, cap_t = O.run_u8(a, b, case_params(od, O, cid)[1], capture=True)
        stop, stats = O.stop_stats(), O.patch_stats()
        for v in [ref] + list(cap_d.values()) + list(cap_t.values()):
            v.setflags(write=False)
        _ORACLE[key] = (ref, cap_d, cap_t, stop, stats)
    return _ORACLE[key]


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def od():
    import of_dis_amd
    return of_dis_amd


# ------------------------------------------------------------------------------------------------ the counters


def test_stop_counters_on_an_op_point(oracle, od):
    """At an op-point (min_iter == max_iter, res_thresh == 0) every started patch runs to max_iter unless an outlier
    reset ends it first or its residual is exactly zero, and the counters agree with the older early_stop."""
    st, ps = oracle_of(od, oracle, "default-f0")[3:]
    print(st, ps)
    assert st["started"] > 0 and st["dp"] == 0 and st["dr"] == 0
    assert st["stop_cnt0"] == st["res_cnt0"] <= st["res"]
    assert st["stop_max_iter"] + ps["outlier_reset"] + ps["oob_iter"] >= st["started"] - st["res"]
    assert ps["early_stop"] >= st["res"]
    oracle.stop_stats_reset()
    assert set(oracle.stop_stats().values()) == {0} and tuple(oracle.stop_stats()) == oracle.STOP_STATS


# ------------------------------------------------------------------------------------------------ stopping cases


def unmet(kind, st):
    """The conditions of a stopping case that the counters `st` of an oracle run do not meet ([] = all met).

    The term a case is named for is the false one in at least 100 stops and in at most 90 % of the patches started,
    so that stopped and running patches share waves; a residual case also stops at least 20 patches at cnt == 0.
    The residual threshold is the one free parameter (RES), so the 90 % rule binds the residual term.  The rate
    cases have none, and on the synth scene their thresholds 0.3 / 0.9 end 94 .. 98 % of the patches on the residual
    rate at cnt == min_iter, the first iteration that evaluates the rates (the table in the module docstring).  So
    their rule is put where the kernels can feel it, and on the scene that meets it (RATE_SCENE, the `mixed` one):
    100 stops under each rate term, and at least 64 patches that iterate on after that first evaluation -- 64 is the
    most patches a patch kernel holds in one workgroup (k_patchq), so they cannot all sit in one -- so that the
    wave-wide shortcut ballot(cnt >= min_iter) sees stopped and running patches side by side.  On the synth
    scene the rate cases are only required to reach both terms and to leave some patch running.

    `st` is the stop counters and the branch counters of one run, merged."""
    n = st["started"]
    want = []
    if kind in ("res", "res3", "min9"):
        want += [("res >= 100", st["res"] >= 100), ("res <= 90 %", st["res"] <= 0.9 * n)]
    if kind in ("res", "res3"):
        want += [("res_cnt0 >= 20", st["res_cnt0"] >= 20)]
    if kind in ("res", "min9", "max1"):  # cnt never reaches min_iter: the rate terms stay silent
        want += [("dp == 0", st["dp"] == 0), ("dr == 0", st["dr"] == 0)]
    if kind == "res3":                   # all three terms live
        want += [("dp >= 1", st["dp"] >= 1), ("dr >= 1", st["dr"] >= 1)]
    if kind == "rate":
        want += [("dp >= 100", st["dp"] >= 100), ("dr >= 100", st["dr"] >= 100),
                 ("64 go on past the first rate test", st["past_first"] >= 64)]
    if kind == "rate_synth":
        want += [("dp >= 1", st["dp"] >= 1), ("dr >= 100", st["dr"] >= 100), ("some go on", st["past_first"] >= 1)]
    if kind in ("min9", "max1"):
        want += [("stop_max_iter >= 100", st["stop_max_iter"] >= 100)]
    if kind == "max1":                   # nothing iterates twice
        want += [("all stop by cnt 1", st["stop_max_iter"] + st["stop_cnt0"] >= n)]
    if kind == "cnt0":
        want += [("all stop at cnt 0", st["stop_cnt0"] == n)]
    return [what for what, ok in want if not ok]


@pytest.mark.parametrize("cid", STOP_IDS)
def test_stopping_case_reaches_its_branch(oracle, od, cid):
    """The oracle alone meets the conditions of `unmet` for the case's kind: on the synth scene, and the rate cases
    on RATE_SCENE."""
    kind = CASES[cid][2]
    for scene, k in ((RATE_SCENE, kind), ("synth", "rate_synth")) if kind == "rate" else (("synth", kind),):
        _, _, _, stop, stats = oracle_of(od, oracle, cid, scene)
        st = dict(stop, **stats)
        print(cid, scene, st)
        assert st["started"] >= 300, st
        assert unmet(k, st) == [], (cid, scene, st)


@pytest.mark.parametrize("f", range(len(FAMILIES)), ids=lambda f: f"f{f}")
@pytest.mark.parametrize("scene", SCENES)
def test_zero_iteration_cases_give_the_same_bits(oracle, od, scene, f):
    """max_iter = 0, min_iter = 0 and res_thresh = 1e4 all stop at the evaluation of OptimizeStart: one output,
    which is not the op-point's (the iterations these cases skip do move the flow)."""
    outs = [oracle_of(od, oracle, f"{k}-f{f}", scene) for k in ("max0", "min0", "r1e4")]
    for o in outs[1:]:
        assert np.array_equal(_bits(o[0]), _bits(outs[0][0]))
        for s in outs[0][1]:
            assert np.array_equal(_bits(o[1][s]), _bits(outs[0][1][s]))
            assert np.array_equal(_bits(o[2][s]), _bits(outs[0][2][s]))
    if scene != "const":
        assert not np.array_equal(_bits(outs[0][0]), _bits(oracle_of(od, oracle, f"default-f{f}", scene)[0]))


def stop_stats_of(od, O, f, over):
    """The stop and branch counters of an oracle run of the synth scene under family f's parameters and `over`."""
    a, b = pair_of(od, "synth", f)
    O.stop_stats_reset()
    O.patch_stats_reset()
    O.run_u8(a, b, family_params(od, O, f, over)[1])
    return dict(O.stop_stats(), **O.patch_stats())


def res_qualifies(od, O, f, r):
    return all(unmet(kind, stop_stats_of(od, O, f, over(r))) == [] for kind, over in RES_KINDS)


@pytest.mark.parametrize("f", range(len(FAMILIES)), ids=lambda f: f"f{f}")
def test_res_thresholds_follow_the_rule(oracle, od, f):
    """RES[f] is the smallest multiple of RES_STEP under which the oracle meets the conditions of the three cases
    that use it: it comes from the oracle's residuals and from nothing else."""
    r = RES_STEP
    while not res_qualifies(od, oracle, f, r):
        r += RES_STEP
        assert r <= 16, f
    assert r == RES[f], (f, r, RES[f])


@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("cid", STOP_IDS + TV_IDS)
def test_oracle_output_is_finite(oracle, od, cid, scene):
    ref, cap_d, cap_t, _, stats = oracle_of(od, oracle, cid, scene)
    for what, v in [("flow", ref)] + [(f"dis {s}", x) for s, x in cap_d.items()] + \
            [(f"tv {s}", x) for s, x in cap_t.items()]:
        assert np.isfinite(v).all(), (cid, scene, what, int((~np.isfinite(v)).sum()))
    assert stats["nonfinite_delta"] == 0, stats


def test_mixed_scene_stops_beside_hatching(oracle, od):
    """The second batch scene does what it is there for: under the residual cases patches stop for the residual
    while others fail their factorisation (the hatched half) in the same run."""
    for f in (0, 1, 5):
        _, _, _, st, ps = oracle_of(od, oracle, f"res3-f{f}", "mixed")
        print(f, st, ps)
        assert st["res"] >= 20 and ps["llt_failed"] >= 1, (f, st, ps)


# ------------------------------------------------------------------------------------------------ TV cases


@pytest.mark.parametrize("cid", TV_IDS)
def test_tv_case_differs_from_the_default_weights(oracle, od, cid):
    """Each TV case changes bits against the default parameters on the same pair: otherwise it proves nothing."""
    f = CASES[cid][1]
    ref, _, cap_t, _, _ = oracle_of(od, oracle, cid)
    dref, _, dcap_t, _, _ = oracle_of(od, oracle, f"default-f{f}")
    assert not np.array_equal(_bits(ref), _bits(dref)), cid
    coarsest = max(cap_t)
    assert not np.array_equal(_bits(cap_t[coarsest]), _bits(dcap_t[coarsest])), (cid, "coarsest level")


@pytest.mark.parametrize("f", TV_FAMILIES, ids=lambda f: f"f{f}")
def test_no_sweeps_equals_no_inner_iterations(oracle, od, f):
    """tv_solverit = 0 leaves du = 0 after every system, tv_innerit = 0 runs none: the same bits, which are the
    warped and re-added flow and not the refined one."""
    a, b = oracle_of(od, oracle, f"sweeps0-f{f}"), oracle_of(od, oracle, f"inner0-f{f}")
    assert np.array_equal(_bits(a[0]), _bits(b[0]))
    for s in a[2]:
        assert np.array_equal(_bits(a[2][s]), _bits(b[2][s]))


def _table(oracle, od):
    rows = []
    for cid in STOP_IDS:
        st = oracle_of(od, oracle, cid)[3]
        over = {k: v for k, v in CASES[cid][3].items()}
        rows.append(f"  {cid:14s} {st['started']:5d} | {st['stop_cnt0']:5d} | {st['stop_max_iter']:5d} | "
                    f"{st['res']:5d} {st['dp']:5d} {st['dr']:5d}   {over}")
    return "\n".join(rows)


if __name__ == "__main__":  # prints the table of the module docstring
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import of_dis_amd
    from oracle import pyoracle
    print(_table(pyoracle, of_dis_amd))

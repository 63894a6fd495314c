"""GPU half of the off-point matrix (test_offpoint.py): the library against the CPU oracle, bit for bit, on the
stopping, TV-weight and sweep-count cases whose purpose the CPU half proves on the oracle's counters.

Everything is a comparison of uint32 bit patterns (test_gpu_parity.assert_bitexact), per stage wherever a single
frame runs: the flow after aggregation and after TV refinement per scale, then the full-resolution output.

* every case alone at the default options;
* the stopping cases under every patch option that changes their kernel, and as batches of three frames (synth,
  mixed, a constant frame) through the tensor entry point, eager and graph-replayed;
* the TV cases under the system-kernel options, on a tall level under the march / 2-D / two-launch forms, and in
  latency mode against the oracle's red-black order;
* tv_solverit 0 / 1 / 5 / 7 on 300- and 700-row levels, for flow and depth, and with sor_pack = 2 in batches;
* the CLIs with the explicit 20-value parameter list;
* the refusal of tv_alpha = 0 (ofdis_params_validate): nothing enqueued, the context still usable.  The refused
  values themselves never run on a device.
"""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_parity import VARIANTS, assert_bitexact
from test_offpoint import (CASES, FAMILIES, GRAY_FLOW, RATE_SCENE, SCENES, STOP_IDS, TV_FAMILIES,
                           TV_IDS, TV_KINDS, case_params, oracle_of, pair_of)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def od():
    import of_dis_amd
    return of_dis_amd


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


def _check_case(oracle, od, ctx, cid, scene, tag, order=0):
    a, b = pair_of(od, scene, CASES[cid][1])
    ref, cap_d, cap_t = oracle_of(od, oracle, cid, scene, order)[:3]
    got, dis, tv = _run_captured(ctx, a, b, case_params(od, oracle, cid)[0], cap_d, cap_t)
    _check_stages(f"{tag} {cid} {scene}", got, dis, tv, ref, cap_d, cap_t)


class options:
    """Context manager: set [(key, value, default)] on a context, restore the defaults on the way out."""

    def __init__(self, ctx, opts):
        self.ctx, self.opts = ctx, opts

    def __enter__(self):
        for k, v, _ in self.opts:
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k, _, d in self.opts:
            self.ctx.set_option(k, d)
        return False


def _split(variant):
    key, val, default = variant
    return [(key, val, default)] if isinstance(key, str) else list(zip(key, val, default))


def _vid(v):
    return f"{v[0]}={v[1]}" if isinstance(v[0], str) else "+".join(f"{k}={x}" for k, x in zip(v[0], v[1]))


def _proof_scene(cid):
    """The scene on which the CPU half proves the case's conditions."""
    return RATE_SCENE if CASES[cid][2] == "rate" else "synth"


# ------------------------------------------------------------------------------------------------ every case alone


@pytest.mark.parametrize("cid,scene", [(c, "synth") for c in STOP_IDS + TV_IDS] +
                         [(c, RATE_SCENE) for c in STOP_IDS if CASES[c][2] == "rate"])
def test_single_frame_bitexact(oracle, od, ctx, cid, scene):
    """Every case of the matrix at the default options, stage by stage."""
    _check_case(oracle, od, ctx, cid, scene, "default")


# ------------------------------------------------------------------------------------------------ patch options


def _patch_size(f):
    w, h, noc, mode, op, over, p = FAMILIES[f]
    return p if p is not None else (12 if op >= 3 else 8)


def _touches(key, f):
    """Whether a patch option changes the kernels family f runs (launch_patch's rules)."""
    noc, ps = FAMILIES[f][2], _patch_size(f)
    if key == "patch_quad":      # k_patchq: gray p = 8 / 12
        return noc == 1 and ps in (8, 12)
    if key == "patch_x16":       # k_patchx: RGB p = 12
        return noc == 3 and ps == 12
    if key == "patch_window":    # the LDS-windowed forms: p = 8 / 12
        return ps in (8, 12)
    if key == "patch_absw":      # aggregation weights written by k_patchq / k_patchx
        return (noc == 1 and ps in (8, 12)) or (noc == 3 and ps == 12)
    if key == "patch_buf":       # gray p = 12 windows by buffer loads
        return noc == 1 and ps == 12
    if key == "wave_per_patch":  # k_patch holds p * p * noc <= 448 values; gray p = 16 runs on it already
        return ps * ps * noc <= 448 and not (noc == 1 and ps == 16)
    return True                  # patch_fdiv, patch_maxres, patch_generic: every family


def _option_cases(key, f):
    """The stopping cases of family f that a patch option is run on.  patch_maxres only acts where the library would
    take the largest-term test: res_thresh == 0 and min_iter >= max_iter (max0, max1)."""
    ids = [c for c in STOP_IDS if CASES[c][1] == f]
    if key == "patch_maxres":
        ids = [c for c in ids if c.startswith(("max0", "max1"))]
    return ids


PATCH_OPTIONS = [  # (option, value, default)
    ("patch_quad", 0, 1), ("patch_x16", 0, 1), ("patch_x16", 2, 1), ("patch_generic", 1, 0), ("wave_per_patch", 1, 0),
    ("patch_window", 0, 1), ("patch_maxres", 0, 1), ("patch_fdiv", 0, 1), ("patch_absw", 0, 1), ("patch_buf", 0, 1),
]


@pytest.mark.parametrize("option,f", [(o, f) for o in PATCH_OPTIONS for f in range(len(FAMILIES)) if _touches(o[0], f)],
                         ids=lambda v: f"f{v}" if isinstance(v, int) else f"{v[0]}={v[1]}")
def test_stopping_cases_under_patch_options(oracle, od, ctx, option, f):
    """The stopping cases of a family under each patch option that changes its kernel, per stage."""
    with options(ctx, [option]):
        for cid in _option_cases(option[0], f):
            _check_case(oracle, od, ctx, cid, _proof_scene(cid), f"{option[0]}={option[1]}")


# ------------------------------------------------------------------------------------------------ batches of three


@pytest.mark.parametrize("cid", STOP_IDS)
def test_stopping_batch3_bitexact(oracle, od, ctx, cid):
    """(synth, mixed, constant frame) in one call of the tensor entry point: eager (graph 0), then captured and
    replayed (graph 1, twice on the same tensors).  Every frame of every run is the oracle's run of that frame
    alone; the output is overwritten with NaN before each run, so a run that writes nothing fails."""
    import torch
    f = CASES[cid][1]
    pairs = [pair_of(od, s, f) for s in SCENES]
    a = torch.from_numpy(np.stack([x[0] for x in pairs])).cuda()
    b = torch.from_numpy(np.stack([x[1] for x in pairs])).cuda()
    p = case_params(od, oracle, cid)[0]
    h, w = pairs[0][0].shape[:2]
    out = torch.empty((len(SCENES), h, w, p.nop), dtype=torch.float32, device="cuda")
    outs = []
    try:
        for graph, reps in ((0, 1), (1, 2)):
            ctx.set_option("graph", graph)
            for rep in range(reps):
                out.fill_(float("nan"))
                assert ctx.run(a, b, p, out=out) is out
                torch.cuda.synchronize()
                outs.append((graph, rep, out.cpu().numpy()))
    finally:
        ctx.set_option("graph", 1)
    for i, scene in enumerate(SCENES):
        ref = oracle_of(od, oracle, cid, scene)[0]
        for graph, rep, o in outs:
            assert_bitexact(o[i], ref, f"{cid} graph {graph} run {rep}: frame {i} ({scene})")


# ------------------------------------------------------------------------------------------------ TV cases


SYSTEM_KEYS = ("smsys", "smsys_small", "smsys_prefetch", "smsys_deriv", "prepd_df", "prepd")
SYSTEM_VARIANTS = [v for v in VARIANTS if v[0] in SYSTEM_KEYS]


def test_system_variants_are_the_parity_suites():
    assert sorted(_vid(v) for v in SYSTEM_VARIANTS) == ["prepd=0", "prepd=1", "prepd_df=0", "smsys=0", "smsys_deriv=0",
                                                        "smsys_prefetch=0", "smsys_small=0"]


@pytest.mark.parametrize("f", TV_FAMILIES, ids=lambda f: f"f{f}")
@pytest.mark.parametrize("variant", SYSTEM_VARIANTS, ids=_vid)
def test_tv_cases_under_system_kernel_options(oracle, od, ctx, variant, f):
    """Every TV case of a family (gray flow, RGB flow, gray depth) under each system-kernel option, per stage."""
    with options(ctx, _split(variant)):
        for kind, _ in TV_KINDS:
            _check_case(oracle, od, ctx, f"{kind}-f{f}", "synth", _vid(variant))


@pytest.mark.parametrize("cid", TV_IDS)
def test_tv_cases_in_latency_mode(oracle, od, ctx, cid):
    """sor_mode = 1 against the oracle under its red-black order."""
    with options(ctx, [("sor_mode", 1, 0)]):
        _check_case(oracle, od, ctx, cid, "synth", "sor_mode=1", order=1)


# Levels off the short ones: (w, h, mode, overrides).  One synth scene each; the oracle's run is shared.
_LEVEL = {}


def _level_params(od, O, w, mode, over):
    pg, pq = od.oppoint(2, w, mode, 1), O.oppoint(2, w, mode, 1)
    for k, v in over.items():
        setattr(pg, k, v)
        setattr(pq, k, v)
    return pg, pq


def _level_oracle(od, O, w, h, mode, over):
    key = (w, h, mode, tuple(sorted(over.items())))
    if key not in _LEVEL:
        a, b = od.synth_pair(w, h, 1, 3, mode)
        ref, cap_d, cap_t = O.run_u8(a, b, _level_params(od, O, w, mode, over)[1], capture=True)
        assert np.isfinite(ref).all(), key
        for v in [ref] + list(cap_d.values()) + list(cap_t.values()):
            v.setflags(write=False)
        _LEVEL[key] = (a, b, ref, cap_d, cap_t)
    return _LEVEL[key]


def _check_level(oracle, od, ctx, w, h, mode, over, tag):
    a, b, ref, cap_d, cap_t = _level_oracle(od, oracle, w, h, mode, over)
    got, dis, tv = _run_captured(ctx, a, b, _level_params(od, oracle, w, mode, over)[0], cap_d, cap_t)
    _check_stages(f"{tag} {w}x{h} mode {mode} {over}", got, dis, tv, ref, cap_d, cap_t)


TALL = (256, 704, {"sc_l": 0, "sc_f": 1})
TALL_VARIANTS = [v for v in VARIANTS if "smsys_march" in (v[0] if not isinstance(v[0], str) else (v[0],))]


@pytest.mark.parametrize("kind,over", TV_KINDS, ids=[k for k, _ in TV_KINDS])
def test_tv_cases_on_a_tall_level(oracle, od, ctx, kind, over):
    """One 256 x 704 level pair (sc_l 0, sc_f 1): the march (default), the 2-D tiled launch (smsys_march = 0) and
    the two launches (smsys_march = 0, smsys2d = 0) under every TV case."""
    assert len(TALL_VARIANTS) == 2
    w, h, sc = TALL
    o = dict(sc, **over)
    _check_level(oracle, od, ctx, w, h, 1, o, f"{kind} default")
    for variant in TALL_VARIANTS:
        with options(ctx, _split(variant)):
            _check_level(oracle, od, ctx, w, h, 1, o, f"{kind} {_vid(variant)}")


# ------------------------------------------------------------------------------------------------ sweep counts


@pytest.mark.parametrize("mode", [1, 2], ids=["flow", "depth"])
@pytest.mark.parametrize("w,h,sc", [(400, 300, {"sc_l": 0, "sc_f": 2}), (256, 704, {"sc_l": 0, "sc_f": 1})],
                         ids=["300rows", "704rows"])
@pytest.mark.parametrize("S", [0, 1, 5, 7])
def test_sweep_counts_on_taller_levels(oracle, od, ctx, S, w, h, sc, mode):
    """tv_solverit off {2, 3, 4} where launch_tv_sor's rules differ from the short levels': 300 rows (the sweep-per-
    wave forms would fit S <= 3) and 704 rows (a.h <= 1024: the register pipeline for S = 1, the generic kernel for
    S = 5 / 7); S = 0 launches no sweep at all."""
    _check_level(oracle, od, ctx, w, h, mode, dict(sc, tv_solverit=S), f"S={S}")


@pytest.mark.parametrize("mode", [1, 2], ids=["flow", "depth"])
@pytest.mark.parametrize("S", [0, 1, 5, 7])
def test_sweep_counts_with_sor_pack(oracle, od, ctx, S, mode):
    """sor_pack = 2 packs S = 2 / 3 only: with the other sweep counts a batch of three must still give every frame
    the oracle's bits, on a level that packs (60 x 34) and one that is a row group of its own (120 x 68)."""
    import test_gpu_sor_pack as sp
    for w, h in ((60, 34), (120, 68)):
        out = sp.batch(od, oracle, ctx, w, h, mode, S, 3, [("sor_pack", 2, 1)])
        for i in range(3):
            assert_bitexact(out[i], sp.reference(od, oracle, w, h, mode, S, i), f"S={S} {w}x{h} mode {mode}: frame {i}")


# ------------------------------------------------------------------------------------------------ CLI


@pytest.mark.parametrize("exe_name,noc,mode", [("run_OF_INT", 1, 1), ("run_DE_RGB", 3, 2)])
def test_cli_explicit_parameter_list(oracle, od, tmp_path, exe_name, noc, mode):
    """The argc = 24 form: 20 explicit values with res_thresh > 0, min_iter < max_iter and TV weights off the
    defaults, on the PNG pair of test_cli_png_inputs, against the oracle with the same values."""
    from test_image_io import encode_png
    w, h = 176, 112
    a3, b3 = od.synth_pair(w, h, 3, 4, mode)  # BGR
    for name, im in (("a.png", a3), ("b.png", b3)):
        (tmp_path / name).write_bytes(encode_png(im[..., ::-1].astype(np.int64), 2, 8, interlace=name == "b.png"))
    a = od.read_image(str(tmp_path / "a.png"), noc)
    b = od.read_image(str(tmp_path / "b.png"), noc)
    # sc_f sc_l max_iter min_iter dp_thresh dr_thresh res_thresh p_samp_s patove usefbcon patnorm costfct usetvref
    # tv_alpha tv_gamma tv_delta tv_innerit tv_solverit tv_sor verbosity
    vals = "3 1 12 2 0.3 0.9 0.75 8 0.4 0 1 0 1 3.7 0.3 21 2 5 1.3 0".split()
    q = oracle.oppoint(2, w, mode, noc)
    for k, v in zip(("sc_f", "sc_l", "max_iter", "min_iter"), vals[:4]):
        setattr(q, k, int(v))
    for k, v in zip(("dp_thresh", "dr_thresh", "res_thresh"), vals[4:7]):
        setattr(q, k, float(v))
    q.p_samp_s, q.patove, q.usefbcon, q.patnorm, q.costfct, q.usetvref = 8, 0.4, 0, 1, 0, 1
    q.tv_alpha, q.tv_gamma, q.tv_delta, q.tv_innerit, q.tv_solverit, q.tv_sor = 3.7, 0.3, 21.0, 2, 5, 1.3
    assert bytes(od.params_from_strings(vals, mode, noc))[:-12] == bytes(q)[:-12]  # all but verbosity and the two
    oracle.stop_stats_reset()                                                       # build switches after it
    want = oracle.run_u8(a, b, q)
    st = oracle.stop_stats()
    assert st["res"] >= 1 and st["dp"] + st["dr"] >= 1 and np.isfinite(want).all(), st
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "of_dis_amd", "bin", exe_name)
    out = tmp_path / ("o.flo" if mode == 1 else "o.pfm")
    r = subprocess.run([exe, str(tmp_path / "a.png"), str(tmp_path / "b.png"), str(out)] + vals, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    if mode == 1:
        got = od.read_flo(str(out))
    else:
        raw = out.read_bytes()
        head = f"Pf\n{w} {h}\n-1.000000\n".encode()
        assert raw.startswith(head)
        got = -np.frombuffer(raw[len(head):], np.float32).reshape(h, w)[::-1][..., None]
    assert_bitexact(got, want, f"{exe_name} with 20 explicit values")


# ------------------------------------------------------------------------------------------------ the refusal


def test_refused_tv_alpha_enqueues_nothing(oracle, od, ctx):
    """tv_alpha = 0 (no inverse of the refinement's systems: ofdis.h) is refused with
    OFDIS_ERR_INVALID_ARGUMENT before anything is enqueued: the output is untouched and the context runs the next
    call bit-exact.  The host-side validation is asserted first, so a library without the refusal never gets as far
    as the device call."""
    import torch
    from of_dis_amd import _lib
    w, h = 160, 120
    pa, pb = pair_of(od, "synth", GRAY_FLOW)
    p = od.oppoint(2, w, 1, 1)
    bad = p.copy(tv_alpha=0.0)
    assert od.validate(bad) == _lib.ERR_INVALID_ARGUMENT and od.validate(p) == 0
    a = torch.from_numpy(pa[None].copy()).cuda()
    b = torch.from_numpy(pb[None].copy()).cuda()
    out = torch.full((1, h, w, 2), 7.0, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(_lib.OfdisError) as e:
        ctx.run_ptr(a.data_ptr(), b.data_ptr(), 1, w, h, bad, out.data_ptr())
    assert e.value.code == _lib.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote the output"
    ctx.run_ptr(a.data_ptr(), b.data_ptr(), 1, w, h, p, out.data_ptr())
    torch.cuda.synchronize()
    assert_bitexact(out[0].cpu().numpy(), oracle_of(od, oracle, f"default-f{GRAY_FLOW}")[0], "after the refusal")

"""Frame counts at the edges of every launch that counts frames in grid y or z (limit 65535).

Two families.

* The sliced launchers (kSlice in ofdis_kernels.hip) cut a call into launches of 65535 frames, or of 32767 where grid z
  holds 2 x frame + direction, and re-base their pointers per slice.  Every one of them runs here one frame above the
  slice (two launches, the second holding one frame) and at twice the slice plus one (three launches, a full middle
  one), against the numpy restatement of the operator.
* The core path is not sliced: prepare() bounds a chunk so that no launch passes the limit (ofdis_max_frames_per_launch:
  min(plane rule, grid rule)).  Calls at the bound, one above it and at twice the bound plus one run here against the
  oracle's flow, in every call kind, with the fused calls against their compositions.

Every large input is P = 11 distinct items tiled by index % 11 on the device.  11 is coprime to 65535 = 3 5 17 257 and
to 32767 = 7 31 151, so a slice or chunk whose pointers are off by any whole number of items -- by another slice, or
applied twice -- lands on other content.  The expected output is the restatement of the 11 items, tiled; for the
temporal filters, whose output frame i reads frames i - R .. i + R, it is the restatement of a short video of length
L = T (mod 11), L >= 11 + 2 R, mapped by temporal_index().  Every comparison is on raw bits over the whole output (on
the device; a difference is reported through same_bits).  Frames are 8 x 4 (W % 4 == 0: the vector forms), 7 x 3 (the
pixel forms) and 4 x 2 on a 2 x 1 grid of cell 2 (the level view) for the operators, 8 x 8 for the core path.
"""
import numpy as np
import pytest

from test_fb_check import fb_reference
from test_flow_error import flow_error_reference
from test_gpu_motion_mask import same_bits
from test_gpu_warp import _dev, _np, expand_level
from test_interp import interp_reference
from test_lr_check import lr_reference, stereo_definition
from test_motion_mask import motion_mask_reference
from test_stabilize import field_of, similarity_matrix, warp_affine_reference
from test_tfilter import tfilter_reference
from test_tfilter_radius import tfilter_radius_reference
from test_warp import warp_reference

pytestmark = pytest.mark.gpu

f32 = np.float32
P = 11            # distinct items under every large input
GRID_YZ = 65535   # the limit of grid y and z
S1, S2 = 65535, 32767                      # the launchers' slices: frames in z, 2 x frame + direction in z
COUNTS1 = [S1 + 1, 2 * S1 + 1]             # one frame above the slice; a full middle slice
COUNTS2 = [S2 + 1, 2 * S2 + 1]
SIGMA = 40.0
LEVEL = {"cell": 2, "off_x": 0, "off_y": 0, "out_w": 2, "out_h": 1}  # 4 x 2 frames on a 2 x 1 grid


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


# --------------------------------------------------------------------------------------------- tiling and comparison

def tile_index(n, phase=0):
    return (np.arange(n) + phase) % P


def tiled(x, n):
    """The first n items of the P items x repeated for ever, on the device."""
    import torch
    t = x if isinstance(x, torch.Tensor) else _dev(np.ascontiguousarray(x))
    return t[torch.arange(n, device="cuda") % P].contiguous()


def short_length(T, R):
    """The shortest video that stands for a tiled one of T frames under a filter of radius R."""
    L = P + 2 * R
    while L % P != T % P:
        L += 1
    return L


def temporal_index(T, L, R):
    """Output frame i of the tiled video of T frames -> the frame of the tiled video of L frames that reads the same
    content: the first R frames onto the first R, the last R onto the last R (L = T mod 11 lines the ends up), every
    other frame onto the frame of its residue among R .. R + 10, whose whole window lies inside both videos."""
    assert L % P == T % P and L >= P + 2 * R and T >= L
    i = np.arange(T)
    j = np.where(i < R, i, R + (i - R) % P)
    tail = i > T - 1 - R
    j[tail] = L - 1 - (T - 1 - i[tail])
    return j


def _raw_t(t):
    import torch
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _raw_n(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same_tiled(got, want, index, what):
    """got: torch tensors [n, ...]; want: numpy arrays [k, ...].  got[i] must hold the bits of want[index[i]], over the
    whole output.  Compared on the device; a difference goes through same_bits for its message.  The outputs are
    overwritten afterwards."""
    import torch
    got = got if isinstance(got, (tuple, list)) else (got,)
    want = want if isinstance(want, (tuple, list)) else (want,)
    assert len(got) == len(want), f"{what}: {len(got)} outputs, expected {len(want)}"
    idx = torch.from_numpy(np.asarray(index, np.int64)).cuda()
    torch.cuda.synchronize()
    for k, (g, w_) in enumerate(zip(got, want)):
        w_ = np.ascontiguousarray(w_)
        assert tuple(g.shape) == (len(index),) + w_.shape[1:] and g.element_size() == w_.dtype.itemsize, \
            f"{what}: output {k} is {g.dtype} {tuple(g.shape)}, expected {w_.dtype} {(len(index),) + w_.shape[1:]}"
        if not torch.equal(_raw_t(g), torch.from_numpy(_raw_n(w_).copy()).cuda()[idx]):
            same_bits((_np(g).view(w_.dtype),), (w_[np.asarray(index)],), f"{what}: output {k}")
            raise AssertionError(f"{what}: output {k} differs")
    for g in got:  # the wrappers allocate outputs uninitialised, and the allocator hands a freed block to the next call of
        assert g.is_contiguous()  # the same size: leave nothing correct behind for a later call to leave unwritten
        g.view(torch.uint8).fill_(0x5A)


def specks(rng, field, k):
    """k values of the field become NaN / +inf / -inf."""
    flat = field.reshape(-1)
    flat[rng.choice(flat.size, size=k, replace=False)] = np.resize(np.array([np.nan, np.inf, -np.inf], f32), k)
    return field


_bases = {}


def bases(w, h):
    """The P distinct items of every kind at w x h, made once and never modified: frames (colour; channel 0 is the grey
    video), a forward and a backward field that mostly agree, two disparity fields, occlusion planes, transforms, a
    field around each transform's with displaced pixels, a truth with unknown pixels, a mask."""
    if (w, h) not in _bases:
        rng = np.random.default_rng(1000 * w + h)
        y, x = np.mgrid[0:h, 0:w]
        ramp = 90 + 9 * x[None, ..., None] + 13 * y[None, ..., None] + 7 * np.arange(P)[:, None, None, None]
        b = {"frames": np.clip(ramp + rng.integers(-20, 21, (P, h, w, 3)), 0, 255).astype(np.uint8)}
        fw = rng.uniform(-2.5, 2.5, (P, h, w, 2)).astype(f32)
        bw = (-fw + rng.standard_normal(fw.shape).astype(f32) * f32(0.4)).astype(f32)
        b["fw"], b["bw"] = specks(rng, fw, P), specks(rng, bw, P)
        dl = rng.uniform(-3, 3, (P, h, w)).astype(f32)
        dr = (-dl + rng.standard_normal(dl.shape).astype(f32) * f32(0.4)).astype(f32)
        b["dl"], b["dr"] = specks(rng, dl, P), specks(rng, dr, P)
        b["occ"] = ((rng.random((2, P, h, w)) < 0.1) * rng.integers(1, 3, (2, P, h, w))).astype(np.uint8)
        M = np.stack([similarity_matrix(1 + 0.01 * i, 0.02 * i - 0.1, 0.5 * i - 2.0, 1.0 - 0.3 * i, w, h) for i in range(P)])
        b["xf"] = M
        F = np.stack([field_of(M[i], w, h) for i in range(P)])
        F[rng.random((P, h, w)) < np.where(np.arange(P) % 2, 0.7, 0.2)[:, None, None]] += f32([10, -6])  # few / most move
        b["mm"] = specks(rng, F.astype(f32), P)
        gt = (fw + (1.5 * rng.standard_normal(fw.shape)).astype(f32)).astype(f32)
        gt[:, ::3, ::5] = 1e10
        b["gt"] = specks(rng, np.nan_to_num(gt, nan=0.0, posinf=2.0, neginf=-2.0).astype(f32), 3)
        b["mask"] = rng.integers(0, 3, (P, h, w)).astype(np.uint8)
        b["cells"] = specks(rng, rng.uniform(-1.5, 1.5, (3, P, LEVEL["out_h"], LEVEL["out_w"], 2)).astype(f32), 12)
        for v in b.values():
            v.setflags(write=False)
        _bases[(w, h)] = b
    return _bases[(w, h)]


def level_view():
    import of_dis_amd as od
    return od.FlowView(0, 0, 1, LEVEL["out_w"], LEVEL["out_h"], LEVEL["cell"], LEVEL["off_x"], LEVEL["off_y"])


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def flow_form(field, form):
    """A float32 [k, h, w, 2] field in the form's dtype and layout: (what the kernel is given, what it then sees)."""
    if form == "f16-planar":
        with np.errstate(over="ignore"):
            half = field.astype(np.float16)
        return np.ascontiguousarray(half.transpose(0, 3, 1, 2)), half
    return field, field


def geometry(form):
    """(w, h) of an operator form."""
    if form.startswith("level"):
        return 4, 2
    return (7, 3) if form.startswith("7x3") else (8, 4)


# --------------------------------------------------------------------------------------------- fb_check, lr_check

@pytest.mark.parametrize("n", COUNTS2)
@pytest.mark.parametrize("form", ["aligned", "unaligned"])
def test_fb_check(ctx, form, n):
    """Slices of 32767.  unaligned: every field and error map 4 bytes off its 16-byte alignment (the pixel form)."""
    import torch
    w, h = 8, 4
    b = bases(w, h)
    want = fb_reference(b["fw"], b["bw"])
    assert all(len({x[i].tobytes() for i in range(P)}) == P for x in want[2:])
    off = 1 if form == "unaligned" else 0
    flows = []
    for name in ("fw", "bw"):
        t = torch.zeros(n * h * w * 2 + off, dtype=torch.float32, device="cuda")
        t[off:] = tiled(b[name], n).reshape(-1)
        flows.append(t)
    occ = [torch.full((n, h, w), 9, dtype=torch.uint8, device="cuda") for _ in range(2)]
    err = [torch.full((n * h * w + off,), -7.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    ctx.fb_check_ptr(flows[0].data_ptr() + 4 * off, flows[1].data_ptr() + 4 * off, n, w, h, 0.01, 0.5, occ[0].data_ptr(),
                     occ[1].data_ptr(), err[0].data_ptr() + 4 * off, err[1].data_ptr() + 4 * off, stream())
    same_tiled(occ + [e[off:].view(n, h, w) for e in err], want, tile_index(n), f"fb_check {form} {n}")
    assert all(float(e[0]) == -7.0 for e in err) or not off


@pytest.mark.parametrize("n", COUNTS2)
def test_lr_check(ctx, n):
    b = bases(8, 4)
    want = lr_reference(b["dl"], b["dr"])
    assert all(len({x[i].tobytes() for i in range(P)}) == P for x in want[2:])
    got = ctx.lr_check(tiled(b["dl"], n), tiled(b["dr"], n), want_err=True)
    same_tiled(got, want, tile_index(n), f"lr_check {n}")


# --------------------------------------------------------------------------------------------- tfilter, tfilter_radius

def filter_inputs(form, T):
    """-> (w, h, noc, frames [P, ...], the two fields as the kernel is given them, as it sees them, layout, level)."""
    w, h = geometry(form)
    b = bases(w, h)
    noc = 3 if "noc3" in form else 1
    frames = b["frames"] if noc == 3 else np.ascontiguousarray(b["frames"][..., 0])
    if form.startswith("level"):
        given = (b["cells"][0], b["cells"][1])
        seen = tuple(expand_level(c, LEVEL, w, h) for c in given)
        return w, h, noc, frames, given, seen, "nhwc", True
    pairs = [flow_form(b[k], form) for k in ("fw", "bw")]
    return w, h, noc, frames, (pairs[0][0], pairs[1][0]), (pairs[0][1], pairs[1][1]), "nchw" if form == "f16-planar" else "nhwc", False


def short(x, k):
    return x[np.arange(k) % P]


TFILTER_FORMS = ["f32", "f32-masks", "f32-noc3", "f32-noc3-masks", "f16-planar", "level", "level-masks", "7x3-masks", "7x3"]


@pytest.mark.parametrize("T", COUNTS1)
@pytest.mark.parametrize("form", TFILTER_FORMS)
def test_tfilter(ctx, form, T):
    """launch_tfilter keeps the call's pointers and passes the slice's first frame: frame f0 + z reads its neighbours
    across the seam."""
    import torch
    w, h, noc, frames, given, seen, layout, level = filter_inputs(form, T)
    masks = bases(w, h)["occ"] if form.endswith("masks") else (None, None)
    L = short_length(T, 1)
    want = tfilter_reference(short(frames, L), short(seen[0], L - 1), short(seen[1], L - 1), SIGMA,
                             *(None if m is None else short(m, L - 1) for m in masks))
    assert len(np.unique(want[1])) > 1, "the `used` output is constant"
    fr, dfw, dbw = tiled(frames, T), tiled(given[0], T - 1), tiled(given[1], T - 1)
    dm = [None if m is None else tiled(m, T - 1) for m in masks]
    if level:
        out, used = torch.empty_like(fr), torch.empty((T, h, w), dtype=torch.uint8, device="cuda")
        ctx.tfilter_ptr(fr.data_ptr(), T, dfw.data_ptr(), dbw.data_ptr(), level_view(), w, h, noc, SIGMA, 0, out.data_ptr(),
                        used.data_ptr(), 0 if dm[0] is None else dm[0].data_ptr(), 0 if dm[1] is None else dm[1].data_ptr(),
                        stream())
        got = (out, used)
    else:
        got = ctx.tfilter(fr, dfw, dbw, SIGMA, dm[0], dm[1], want_used=True, layout=layout)
    same_tiled(got, want, temporal_index(T, L, 1), f"tfilter {form} {T}")


RADIUS_FORMS = ["f32", "f32-noc3", "f16-planar", "level", "7x3"]


@pytest.mark.parametrize("T", COUNTS1)
@pytest.mark.parametrize("fb", [False, True], ids=["nofb", "fb"])
@pytest.mark.parametrize("radius", [1, 4])
@pytest.mark.parametrize("form", RADIUS_FORMS)
def test_tfilter_radius(ctx, form, radius, fb, T):
    import torch
    w, h, noc, frames, given, seen, layout, level = filter_inputs(form, T)
    L = short_length(T, radius)
    want = tfilter_radius_reference(short(frames, L), short(seen[0], L - 1), short(seen[1], L - 1), SIGMA, radius, fb)
    assert len(np.unique(want[1])) > 1, "the `used` output is constant"
    fr, dfw, dbw = tiled(frames, T), tiled(given[0], T - 1), tiled(given[1], T - 1)
    if level:
        out, used = torch.empty_like(fr), torch.empty((T, h, w), dtype=torch.uint8, device="cuda")
        ctx.tfilter_radius_ptr(fr.data_ptr(), T, dfw.data_ptr(), dbw.data_ptr(), level_view(), w, h, noc, radius, SIGMA, 0,
                               out.data_ptr(), used.data_ptr(), fb, 0.01, 0.5, stream())
        got = (out, used)
    else:
        got = ctx.tfilter_radius(fr, dfw, dbw, SIGMA, radius, fb, want_used=True, layout=layout)
    same_tiled(got, want, temporal_index(T, L, radius), f"tfilter_radius {form} R {radius} fb {fb} {T}")


def test_temporal_index_is_the_restatement_of_the_long_video():
    """The mapping itself, on a video short enough for the restatement: 42 = 9 (mod 11) frames against 20."""
    w, h, noc, frames, given, seen, layout, level = filter_inputs("f32", 42)
    for R, T in ((1, 42), (4, 42), (4, 50)):
        L = short_length(T, R)
        long_ = tfilter_radius_reference(short(frames, T), short(seen[0], T - 1), short(seen[1], T - 1), SIGMA, R, True)
        small = tfilter_radius_reference(short(frames, L), short(seen[0], L - 1), short(seen[1], L - 1), SIGMA, R, True)
        j = temporal_index(T, L, R)
        same_bits(long_, tuple(x[j] for x in small), f"T {T} L {L} R {R}")


# --------------------------------------------------------------------------------------------- warp_affine

@pytest.mark.parametrize("n", COUNTS1)
@pytest.mark.parametrize("noc", [1, 3])
@pytest.mark.parametrize("out", ["u8", "f32"])
def test_warp_affine(ctx, out, noc, n):
    """launch_warp_affine advances the transforms by 6 doubles per frame of the slice."""
    import torch
    b = bases(8, 4)
    img = b["frames"] if noc == 3 else np.ascontiguousarray(b["frames"][..., 0])
    want = warp_affine_reference(img, b["xf"], f32 if out == "f32" else np.uint8)
    assert 0 < want[1].mean() < 1
    got = ctx.warp_affine(tiled(img, n), tiled(b["xf"], n), torch.float32 if out == "f32" else None, want_valid=True)
    same_tiled(got, want, tile_index(n), f"warp_affine {out} noc {noc} {n}")


# --------------------------------------------------------------------------------------------- flow_error

@pytest.mark.parametrize("n", COUNTS1)
@pytest.mark.parametrize("form", ["f32", "f32-mask", "f16-planar", "f16-planar-mask", "level", "level-mask", "7x3-mask"])
def test_flow_error(ctx, form, n):
    """launch_flow_error advances six pointers; the row sums and the histogram have strides of their own, the flow's
    depends on its dtype and on the level view.  stats is not optional; the other two outputs come in every subset on
    the float32 form and together elsewhere."""
    import torch
    w, h = geometry(form)
    b = bases(w, h)
    masked = form.endswith("mask")
    level = form.startswith("level")
    if level:
        given = b["cells"][2]
        seen = expand_level(given, LEVEL, w, h)
    else:
        given, seen = flow_form(b["fw"], "f16-planar" if form.startswith("f16-planar") else "f32")
    want = flow_error_reference(seen, b["gt"], b["mask"] if masked else None, 1 if masked else -1)
    assert (want[0][:, 0] > 0).all() and (want[0][:, 1] > 0).any(), "a pair with nothing scored, or no non-finite estimate"
    flow, gt = tiled(given, n), tiled(b["gt"], n)
    mask = tiled(b["mask"], n) if masked else None
    view = level_view() if level else None
    for want_err, want_hist in ((True, True), (False, False), (True, False), (False, True)):
        stats = torch.full((n, want[0].shape[1]), -5.0, dtype=torch.float64, device="cuda")
        err = torch.full((n, h, w), -7.0, dtype=torch.float32, device="cuda")
        hist = torch.full((n, want[2].shape[1]), 9, dtype=torch.int32, device="cuda")
        if level:
            ctx.flow_error_ptr(flow.data_ptr(), view, gt.data_ptr(), n, w, h, stats.data_ptr(), 0 if mask is None else mask.data_ptr(),
                               1 if masked else -1, err.data_ptr() if want_err else 0, hist.data_ptr() if want_hist else 0, stream())
        else:
            import of_dis_amd as od
            f16 = form.startswith("f16-planar")
            ctx.flow_error_ptr(flow.data_ptr(), od.FlowView(int(f16), int(f16), 0, w, h, 1, 0, 0), gt.data_ptr(), n, w, h,
                               stats.data_ptr(), 0 if mask is None else mask.data_ptr(), 1 if masked else -1,
                               err.data_ptr() if want_err else 0, hist.data_ptr() if want_hist else 0, stream())
        what = f"flow_error {form} {n} err {want_err} hist {want_hist}"
        same_tiled((stats, err, hist), (want[0], want[1] if want_err else np.full_like(want[1], -7.0),
                                        want[2] if want_hist else np.full_like(want[2], 9)), tile_index(n), what)
        if form != "f32":
            break


# --------------------------------------------------------------------------------------------- motion_mask

@pytest.mark.parametrize("n", COUNTS1)
@pytest.mark.parametrize("radius", [0, 4])
@pytest.mark.parametrize("form", ["f32", "f32-occ", "f16-planar", "level-occ", "7x3-occ"])
def test_motion_mask(ctx, form, radius, n):
    """launch_motion_mask advances the transforms by 6 doubles and the statistics by 12 numbers per pair."""
    import torch
    import of_dis_amd as od
    w, h = geometry(form)
    b = bases(w, h)
    level = form.startswith("level")
    if level:
        M = b["xf"]
        cells = np.stack([field_of(M[i], w, h)[::2, ::2][:LEVEL["out_h"], :LEVEL["out_w"]] for i in range(P)]) + b["cells"][2] * f32(4)
        given = cells.astype(f32)
        seen = expand_level(given, LEVEL, w, h)
    else:
        given, seen = flow_form(b["mm"], "f16-planar" if form == "f16-planar" else "f32")
    occ = b["occ"][0] if form.endswith("occ") else None
    want = motion_mask_reference(seen, b["xf"], occ, radius=radius)
    assert len(np.unique(want[0])) >= 2 and len({want[1][i].tobytes() for i in range(P)}) == P
    flow, xf = tiled(given, n), tiled(b["xf"], n)
    docc = None if occ is None else tiled(occ, n)
    f16 = form == "f16-planar"
    view = level_view() if level else od.FlowView(int(f16), int(f16), 0, w, h, 1, 0, 0)
    code = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    res = torch.empty((n, h, w), dtype=torch.float32, device="cuda")
    stats = torch.empty((n, want[2].shape[1]), dtype=torch.int64, device="cuda")
    ctx.motion_mask_ptr(flow.data_ptr(), view, n, w, h, xf.data_ptr(), 0 if docc is None else docc.data_ptr(), 1.0, 0.05, radius,
                        code.data_ptr(), res.data_ptr(), stats.data_ptr(), stream())
    same_tiled((code, res, stats), want, tile_index(n), f"motion_mask {form} radius {radius} {n}")


def test_the_operators_context_still_runs_one_pair(ctx, oracle):
    """The context every operator test above shared: one pair of the core configuration against the oracle."""
    a, b, p, fw, _ = core(oracle, "grey")
    same_bits((ctx.run_host(a[0], b[0], p),), (fw[0],), "one pair after the operator calls")


# ============================================================================================= the core path

W = H = 8
CORE = {"grey": (1, {}), "colour": (3, {}), "notv": (1, {"usetvref": 0})}
_core = {}


def core_params(name, mode=1, sc=(0, 0)):
    import of_dis_amd as od
    noc, over = CORE[name]
    p = od.oppoint(2, W, mode, noc)
    p.sc_f, p.sc_l = sc
    for k, v in over.items():
        setattr(p, k, v)
    assert od.validate(p) == 0
    return p


def core(oracle, name):
    """-> (a, b u8 [P, 8, 8, noc], the parameters, the oracle's forward and backward flow [P, 8, 8, 2]) of the P pairs
    of a configuration: single-scale flow at 8 x 8 (test_gpu_level_boundaries.SMALL[(0, 0)])."""
    if name not in _core:
        import of_dis_amd as od
        noc, over = CORE[name]
        q = oracle.oppoint(2, W, 1, noc)
        q.sc_f, q.sc_l = 0, 0
        for k, v in over.items():
            setattr(q, k, v)
        prs = [od.synth_pair(W, H, noc, i, od.MODE_OF) for i in range(P)]
        a, b = np.stack([x[0] for x in prs]), np.stack([x[1] for x in prs])
        fw = np.stack([oracle.run_u8(a[i], b[i], q) for i in range(P)])
        bw = np.stack([oracle.run_u8(b[i], a[i], q) for i in range(P)])
        for x in (fw, bw):
            assert np.isfinite(x).all() and len({x[i].tobytes() for i in range(P)}) == P
            x.setflags(write=False)
        _core[name] = (a, b, core_params(name), fw, bw)
    return _core[name]


def pair_cap(p):
    """The pairs one launch takes at 8 x 8: the grid rule (the plane rule allows millions)."""
    import of_dis_amd as od
    cap = od.max_frames_per_launch(p, W, H)
    assert cap == GRID_YZ // max(2, p.noc if p.usetvref else 1)
    return cap


class Issue:
    """A context of its own under the options `opts`; on the way out it must still run one pair correctly."""

    def __init__(self, check, **opts):
        self.check, self.opts = check, opts

    def __enter__(self):
        import of_dis_amd as od
        self.c = od.Context(0)
        for k, v in self.opts.items():
            self.c.set_option(k, v)
        return self.c

    def __exit__(self, kind, value, tb):
        try:
            if kind is None:
                a, b, p, want = self.check
                got = self.c.run_host(a, b, p)
                same_bits((got,), (want,), f"one pair after the call ({self.opts})")
        finally:
            self.c.close()
        return False


def one_pair(cfg):
    a, b, p, fw, _ = cfg
    return a[0], b[0], p, fw[0]


def launches(c, kernel, call):
    """How many launches of `kernel` the call made (kernel timing counts them)."""
    c.enable_kernel_timing(True)
    try:
        before = c.kernel_time(kernel)[1]
        out = call()
        return out, c.kernel_time(kernel)[1] - before
    finally:
        c.enable_kernel_timing(False)


@pytest.mark.parametrize("count", ["cap", "cap+1", "2cap+1"])
@pytest.mark.parametrize("name", list(CORE))
def test_plain_run_on_one_stream(oracle, name, count):
    """streams = 1, chunk = 0: chunks of exactly the bound.  The pyramid's grid z holds 2 x cap frames; colour with
    prepd = 0 puts cap x 3 in the derivative launches' grid y."""
    cfg = core(oracle, name)
    a, b, p, fw, _ = cfg
    cap = pair_cap(p)
    n = {"cap": cap, "cap+1": cap + 1, "2cap+1": 2 * cap + 1}[count]
    for prepd in ((2, 0) if name == "colour" and count == "cap+1" else (2,)):
        with Issue(one_pair(cfg), streams=1, chunk=0, prepd=prepd) as c:
            out, k = launches(c, "pyr_base", lambda: c.run(tiled(a, n), tiled(b, n), p))
            same_tiled(out, fw, tile_index(n), f"{name} {n} pairs prepd {prepd}")
            assert k == -(-n // cap), f"{k} pyramid launches for {n} pairs at {cap} per launch"


@pytest.mark.parametrize("name", ["grey", "notv"])
def test_plain_run_default_issue(oracle, name):
    """Two lanes by default: 2 cap + 1 pairs are halves above the bound, cut to three chunks."""
    cfg = core(oracle, name)
    a, b, p, fw, _ = cfg
    n = 2 * pair_cap(p) + 1
    with Issue(one_pair(cfg)) as c:
        for rep in range(2):  # the second call replays the recorded graph
            same_tiled(c.run(tiled(a, n), tiled(b, n), p), fw, tile_index(n), f"{name} default issue, call {rep}")


def test_explicit_chunk_is_clamped(oracle):
    """chunk = cap + 5000 on 2 cap + 1 pairs: unclamped it would be two launches, clamped it is three."""
    cfg = core(oracle, "grey")
    a, b, p, fw, _ = cfg
    cap = pair_cap(p)
    n = 2 * cap + 1
    for streams in (1, 2):
        with Issue(one_pair(cfg), streams=streams, chunk=cap + 5000) as c:
            out, k = launches(c, "pyr_base", lambda: c.run(tiled(a, n), tiled(b, n), p))
            same_tiled(out, fw, tile_index(n), f"chunk {cap + 5000}, streams {streams}")
            assert k == 3, k


@pytest.mark.parametrize("graph", [0, 1, 2])
def test_graph_modes(oracle, graph):
    cfg = core(oracle, "grey")
    a, b, p, fw, _ = cfg
    n = pair_cap(p) + 1
    for streams in (1, 2):
        with Issue(one_pair(cfg), streams=streams, chunk=pair_cap(p) if streams == 2 else 0, graph=graph) as c:
            ta, tb = tiled(a, n), tiled(b, n)
            for rep in range(2):
                same_tiled(c.run(ta, tb, p), fw, tile_index(n), f"graph {graph} streams {streams} call {rep}")


def test_formats(oracle):
    """The level grid (at sc_l = 0 without padding: the flow itself, cell 1) and float16 planar, cap + 1 pairs."""
    import torch
    import of_dis_amd as od
    cfg = core(oracle, "grey")
    a, b, p, fw, _ = cfg
    n = pair_cap(p) + 1
    g = od.out_geometry(p, W, H, grid="level")
    assert (g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"]) == (W, H, 1, 0, 0)
    with Issue(one_pair(cfg), streams=1) as c:
        ta, tb = tiled(a, n), tiled(b, n)
        same_tiled(c.run(ta, tb, p, grid="level"), fw, tile_index(n), "level grid")
        half = np.ascontiguousarray(fw.astype(np.float16).transpose(0, 3, 1, 2))
        same_tiled(c.run(ta, tb, p, dtype=torch.float16, layout="nchw"), half, tile_index(n), "float16 nchw")
        same_tiled(c.run(ta, tb, p, dtype=torch.float16, layout="nchw", grid="level"), half, tile_index(n), "float16 nchw level")


@pytest.mark.parametrize("streams", [1, 0])
def test_run_bidir(oracle, streams):
    """cap + 1 pairs with masks and errors: the check after the chunks counts 2 n in grid z (slices of 32767)."""
    cfg = core(oracle, "grey")
    a, b, p, fw, bw = cfg
    n = pair_cap(p) + 1
    want = (fw, bw) + fb_reference(fw, bw)
    with Issue(one_pair(cfg), streams=streams) as c:
        same_tiled(c.run_bidir(tiled(a, n), tiled(b, n), p, want_err=True), want, tile_index(n), f"run_bidir streams {streams}")


_seq = {}


def sequence(oracle, stride):
    """The P frames of the grey clip (frame a of every pair) and the oracle's flows of its pairs (i, i + stride mod P)."""
    if stride not in _seq:
        a, _, p, _, _ = core(oracle, "grey")
        q = oracle.oppoint(2, W, 1, 1)
        q.sc_f, q.sc_l = 0, 0
        fw = np.stack([oracle.run_u8(a[i], a[(i + stride) % P], q) for i in range(P)])
        bw = np.stack([oracle.run_u8(a[(i + stride) % P], a[i], q) for i in range(P)])
        for x in (fw, bw):
            assert np.isfinite(x).all() and len({x[i].tobytes() for i in range(P)}) == P
        _seq[stride] = (a, p, fw, bw)
    return _seq[stride]


def seq_cap(p, stride):
    """A sequence chunk of m pairs builds m + stride frames: m <= 65535 - stride at 8 x 8 grey."""
    assert p.noc == 1
    return GRID_YZ - stride


@pytest.mark.parametrize("streams", [1, 0])
@pytest.mark.parametrize("stride", [1, 3])
def test_run_sequence(oracle, stride, streams):
    """One pair more than a sequence chunk takes: cap_seq + 1 + stride frames (cap_seq + 2 at stride 1).  On one stream
    the first chunk's pyramid holds exactly 65535 frames."""
    cfg = core(oracle, "grey")
    a, p, fw, _ = sequence(oracle, stride)
    cap = seq_cap(p, stride)
    T = cap + 1 + stride
    with Issue(one_pair(cfg), streams=streams) as c:
        out, k = launches(c, "pyr_base", lambda: c.run_sequence(tiled(a, T), p, stride=stride))
        same_tiled(out, fw, tile_index(T - stride), f"run_sequence stride {stride} streams {streams}")
        assert k == 2, k


def test_run_sequence_bidir(oracle):
    cfg = core(oracle, "grey")
    a, p, fw, bw = sequence(oracle, 1)
    T = seq_cap(p, 1) + 2
    want = (fw, bw) + fb_reference(fw, bw)
    with Issue(one_pair(cfg), streams=1) as c:
        got = c.run_sequence(tiled(a, T), p, bidir=True, want_err=True)
        same_tiled(got, want, tile_index(T - 1), "run_sequence bidir")


_stereo = {}


def stereo(name="grey"):
    """P stereo pairs at 8 x 8, depth at sc 0 .. 3 (defined: test_gpu_level_boundaries.SMALL[(0, 3)]), and the definition
    of both disparities from plain depth calls, with the check's masks and errors."""
    if name not in _stereo:
        import of_dis_amd as od
        p = core_params(name, od.MODE_DE, (3, 0))
        prs = [od.synth_pair(W, H, p.noc, i, od.MODE_DE) for i in range(P)]
        left, right = np.stack([x[0] for x in prs]), np.stack([x[1] for x in prs])
        c = od.Context(0)
        try:
            dl, dr = stereo_definition(lambda x, y: c.run_host(x, y, p), left, right)
        finally:
            c.close()
        assert len({dl[i].tobytes() for i in range(P)}) == P
        _stereo[name] = (left, right, p, (dl, dr) + lr_reference(dl, dr))
    return _stereo[name]


@pytest.mark.parametrize("count", ["cap", "cap+1", "2cap+1"])
def test_run_stereo(oracle, count):
    """A stereo pair is two flow pairs and four pyramid frames: half the pair call's bound, 16383."""
    import of_dis_amd as od
    left, right, p, want = stereo()
    cap = od.max_frames_per_launch(p, W, H) // 2
    assert cap == 16383
    n = {"cap": cap, "cap+1": cap + 1, "2cap+1": 2 * cap + 1}[count]
    with Issue(one_pair(core(oracle, "grey")), streams=1) as c:
        out, k = launches(c, "pyr_base", lambda: c.run_stereo(tiled(left, n), tiled(right, n), p, want_err=True))
        same_tiled(out, want, tile_index(n), f"run_stereo {n}")
        assert k == -(-n // cap), k


# --------------------------------------------------------------------------------------------- the fused calls

def fused_issues(cap):
    """The default issue, and two lanes with chunks scaled to the bound (four chunks for cap + 1 pairs)."""
    return {"default": {}, "streams2-chunks": {"streams": 2, "chunk": cap // 3}}


@pytest.mark.parametrize("issue", ["default", "streams2-chunks"])
def test_run_warp(oracle, issue):
    import torch
    cfg = core(oracle, "grey")
    a, b, p, fw, _ = cfg
    n = pair_cap(p) + 1
    want = warp_reference(b[..., 0], fw, 1.0, f32)
    with Issue(one_pair(cfg), **fused_issues(pair_cap(p))[issue]) as c:
        small = c.warp(_dev(b[..., 0]), c.run(_dev(a), _dev(b), p), 1.0, torch.float32, want_valid=True)
        same_bits(small, want, "the composition on the P pairs")
        got = c.run_warp(tiled(a, n), tiled(b, n), p, 1.0, torch.float32, want_valid=True)
        same_tiled([got[0].reshape(n, H, W), got[1]], want, tile_index(n), f"run_warp {issue}")


@pytest.mark.parametrize("issue", ["default", "streams2-chunks"])
def test_run_interp(oracle, issue):
    import torch
    cfg = core(oracle, "grey")
    a, b, p, fw, bw = cfg
    n = pair_cap(p) + 1
    t = (0.25, 0.5)
    occ = fb_reference(fw, bw)[:2]
    want = interp_reference(a[..., 0], b[..., 0], fw, bw, t, *occ, out_dtype=f32)
    with Issue(one_pair(cfg), **fused_issues(pair_cap(p))[issue]) as c:
        got = c.run_interp(tiled(a[..., 0], n), tiled(b[..., 0], n), p, t, torch.float32, want_valid=True, occ=True, want_occ=True)
        same_tiled(got, tuple(want) + tuple(occ), tile_index(n), f"run_interp {issue}")


@pytest.mark.parametrize("issue", ["default", "streams2-chunks"])
def test_run_error(oracle, issue):
    cfg = core(oracle, "grey")
    a, b, p, fw, _ = cfg
    n = pair_cap(p) + 1
    bs = bases(W, H)
    gt = (fw + np.random.default_rng(3).standard_normal(fw.shape).astype(f32)).astype(f32)
    gt[:, ::3, ::5] = 1e10  # unknown
    want = flow_error_reference(fw, gt, bs["mask"], 1)
    assert (want[0][:, 0] > 0).all()
    with Issue(one_pair(cfg), **fused_issues(pair_cap(p))[issue]) as c:
        got = c.run_error(tiled(a, n), tiled(b, n), p, tiled(gt, n), tiled(bs["mask"], n), 1, want_err=True, want_hist=True)
        same_tiled(got, want, tile_index(n), f"run_error {issue}")


def fused_sequence_issues(cap):
    return {"default": {}, "streams2-chunks": {"streams": 2, "chunk": cap // 3}}


@pytest.mark.parametrize("issue", ["default", "streams2-chunks"])
def test_run_sequence_tfilter(oracle, issue):
    """A clip one frame longer than one sequence chunk takes; the filter after the chunks counts its frames in grid z."""
    cfg = core(oracle, "grey")
    a, p, fw, bw = sequence(oracle, 1)
    cap = seq_cap(p, 1)
    T = cap + 2
    L = short_length(T, 1)
    clip = short(a[..., 0], L)
    sfw, sbw = short(fw, L - 1), short(bw, L - 1)
    occ = fb_reference(sfw, sbw)[:2]
    want = tfilter_reference(clip, sfw, sbw, SIGMA, *occ)
    with Issue(one_pair(cfg), **fused_sequence_issues(cap)[issue]) as c:
        got = c.run_sequence_tfilter(tiled(a, T), p, SIGMA, occ=True, want_used=True)
        same_tiled([got[0].reshape(T, H, W), got[1]], want, temporal_index(T, L, 1), f"run_sequence_tfilter {issue}")


@pytest.mark.parametrize("issue", ["default", "streams2-chunks"])
def test_run_sequence_motion_mask(oracle, issue):
    """fb = True.  The fit is per pair, so the composition on the P pairs of a 12-frame clip is the whole expectation."""
    cfg = core(oracle, "grey")
    a, p, fw, bw = sequence(oracle, 1)
    cap = seq_cap(p, 1)
    T = cap + 2
    fit = dict(model=1, step=2, tau=2.0, iters=4)
    with Issue(one_pair(cfg), **fused_sequence_issues(cap)[issue]) as c:
        clip = _dev(short(a, P + 1))
        sfw, sbw, occ = c.run_sequence(clip, p, bidir=True)[:3]
        same_bits((sfw, sbw), (fw, bw), "the short clip's flows")
        xf, sup = c.fit_motion(sfw, sbw, want_support=True, **fit)
        want = tuple(c.motion_mask(sfw, xf, occ, radius=1, want_res=True, want_stats=True)) + (xf, sup, occ)
        want = tuple(_np(x) for x in want)
        ref = motion_mask_reference(fw, want[3], want[5], radius=1)
        same_bits(want[:3], ref, "the mask of the composition is the restatement's")
        got = c.run_sequence_motion_mask(tiled(a, T), p, fb=True, want_res=True, want_stats=True, want_xform=True,
                                         want_occ=True, **fit)
        same_tiled(got, want, tile_index(T - 1), f"run_sequence_motion_mask {issue}")

"""Output formats (ofdis_run_batch_u8_fmt, ofdis_run_sequence_u8_fmt): float16, planar and level-grid outputs.

Every comparison is on raw bits: float32 as uint32; float16 as uint16 wherever the expected value is not NaN, plus
equal NaN positions.  The expected float16 is ``want.astype(np.float16)`` of the plain call on the same context (numpy
rounds to nearest even, overflows to inf and keeps subnormals); the expected planar output is the plain one transposed;
the expected level grid is the stage capture of the finest level (tv_flow[sc_l], dis_flow[sc_l] without the
refinement) times 2^sc_l, which is exact.  The plain path is pinned to the oracle by the parity tests.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_sequence import ISSUES, sequence

pytestmark = pytest.mark.gpu

FORMATS = [("float32", "nchw"), ("float16", "nhwc"), ("float16", "nchw")]  # the full-grid formats beside the plain one
ALL_FORMATS = [("float32", "nhwc")] + FORMATS
OF, DE = 1, 2

# (w, h, noc, mode, op-point, overrides): the smallest shapes that reach each store path
S_176 = (176, 96, 1, OF, 2, {})                          # 2^l = 2, no padding, W % 4 == 0: the vector forms
S_173 = (173, 97, 1, OF, 2, {})                          # padding and crop on both axes; odd width: element stores,
                                                         # planar float16 rows 2-byte aligned on every other row
S_2100 = (2100, 70, 1, OF, 2, {"sc_l": 1, "sc_f": 2})    # three 1024-column blocks, the last one partial
S_640 = (640, 480, 1, OF, 2, {"sc_l": 2})                # 2^l = 4
S_1080 = (1920, 1080, 1, OF, 2, {})                      # 2^l = 16
S_RGB = (192, 128, 3, OF, 3, {})                         # sc_l = 0: the copy form
S_DE0 = (120, 64, 1, DE, 4, {})                          # nop = 1, sc_l = 0: k_upsample
S_DE1 = (120, 64, 1, DE, 4, {"sc_l": 1})                 # nop = 1, 2^l = 2: k_upsample_rows1
SHAPES = [S_176, S_173, S_2100, S_640, S_1080, S_RGB, S_DE0, S_DE1]

_pairs = {}


def params(shape):
    import of_dis_amd as od
    w, h, noc, mode, op, over = shape
    p = od.oppoint(op, w, mode, noc)
    for k, v in over.items():
        setattr(p, k, v)
    return p


def pairs(shape, n):
    """n distinct synthetic pairs of the shape, u8 [n, h, w, noc] twice; generated once (three) and sliced."""
    import of_dis_amd as od
    w, h, noc, mode = shape[:4]
    key = (w, h, noc, mode)
    if key not in _pairs:
        ab = [od.synth_pair(w, h, noc, f, mode) for f in range(3)]
        _pairs[key] = tuple(np.stack([x[k] for x in ab]) for k in (0, 1))
        for x in _pairs[key]:
            x.setflags(write=False)
    return _pairs[key][0][:n], _pairs[key][1][:n]


@pytest.fixture(scope="module")
def ctx():
    import of_dis_amd as od
    c = od.Context(0)
    yield c
    c.close()


def _dev(x):
    import torch
    return torch.from_numpy(np.array(x)).cuda()


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _tdtype(name):
    import torch
    return {"float32": torch.float32, "float16": torch.float16}[name]


def transform(want, dtype, layout):
    """The plain float32 [n, H, W, nop] output in another element type and layout."""
    x = want if layout == "nhwc" else np.ascontiguousarray(want.transpose(0, 3, 1, 2))
    if dtype == "float16":
        with np.errstate(over="ignore"):
            x = x.astype(np.float16)
    return x


def assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    if want.dtype == np.float16:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), f"{what}: NaN positions differ"
        bad = (np.ascontiguousarray(got).view(np.uint16) != np.ascontiguousarray(want).view(np.uint16)) & ~nan
    else:
        bad = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {tuple(np.argwhere(bad)[0])}"


def level_reference(c, shape, p, a, b, init=None):
    """capture x 2^sc_l of single-pair captured plain calls: float32 [n, hl, wl, nop]."""
    import of_dis_amd as od
    w, h = shape[:2]
    g = od.out_geometry(p, w, h, init is not None, grid="level")
    out = []
    for f in range(len(a)):
        cap = np.full((g["out_h"], g["out_w"], p.nop), np.nan, np.float32)
        if p.usetvref:
            c.set_capture(None, {p.sc_l: cap})
        else:
            c.set_capture({p.sc_l: cap}, None)
        c.run_host(a[f], b[f], p, init=None if init is None else init[f])
        c.set_capture(None, None)
        out.append(cap * np.float32(1 << p.sc_l))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------ 1. full grid

@pytest.mark.parametrize("shape", SHAPES, ids=["176x96", "173x97", "2100x70", "640x480", "1920x1080", "rgb", "depth0",
                                                "depth1"])
def test_full_grid(ctx, shape):
    n = 1 if shape is S_1080 else 2
    p = params(shape)
    a, b = (_dev(x) for x in pairs(shape, n))
    want = _np(ctx.run(a, b, p))
    assert np.abs(want).max() > 0.25  # there is a flow to convert
    for dtype, layout in FORMATS:
        got = ctx.run(a, b, p, dtype=_tdtype(dtype), layout=layout)
        assert got.dtype == _tdtype(dtype) and got.is_contiguous()
        assert_bits(_np(got), transform(want, dtype, layout), f"{shape} {dtype} {layout}")
    # the plain format through the new entry point: the plain call
    import of_dis_amd as od
    out = np.empty_like(want)
    od._lib.check(od.lib().ofdis_run_batch_u8_fmt_host(ctx._h, pairs(shape, n)[0].ctypes.data,
                                                       pairs(shape, n)[1].ctypes.data, None, n, shape[0], shape[1],
                                                       C.byref(p), C.byref(od.out_format()), out.ctypes.data))
    assert_bits(out, want, f"{shape} plain format")
    assert_bits(ctx.run_host(*pairs(shape, n), p, dtype=np.float16, layout="nchw"), transform(want, "float16", "nchw"),
                f"{shape} host form")


@pytest.mark.parametrize("shape", [S_173, S_2100], ids=["173x97", "2100x70"])
def test_full_grid_every_up_form(shape):
    """A format served by a single store form gives the same bits under every up_form setting."""
    import of_dis_amd as od
    c = od.Context(0)
    p = params(shape)
    a, b = (_dev(x) for x in pairs(shape, 2))
    want = _np(c.run(a, b, p))
    for form in (0, 1, 2):
        c.set_option("up_form", form)
        assert_bits(_np(c.run(a, b, p)), want, f"up_form {form} plain")
        for dtype, layout in FORMATS:
            assert_bits(_np(c.run(a, b, p, dtype=_tdtype(dtype), layout=layout)), transform(want, dtype, layout),
                        f"up_form {form} {dtype} {layout}")
    c.close()


# ------------------------------------------------------------------------------------------------ 2. level grid

@pytest.mark.parametrize("shape", [S_176, S_173, S_RGB, S_DE0, S_DE1, S_176[:5] + ({"usetvref": 0},)],
                         ids=["176x96", "173x97", "rgb", "depth0", "depth1", "notv"])
def test_level_grid(ctx, shape):
    import of_dis_amd as od
    p = params(shape)
    w, h = shape[:2]
    a, b = pairs(shape, 3)
    want = level_reference(ctx, shape, p, a, b)
    g = od.out_geometry(p, w, h, grid="level")
    assert want.shape == (3, g["out_h"], g["out_w"], p.nop) and not np.isnan(want).any()
    assert np.abs(want).max() > 0.25
    da, db = _dev(a), _dev(b)
    for dtype, layout in ALL_FORMATS:
        got = ctx.run(da, db, p, dtype=_tdtype(dtype), layout=layout, grid="level")
        shape_want = (3, p.nop, g["out_h"], g["out_w"]) if layout == "nchw" else (3, g["out_h"], g["out_w"], p.nop)
        assert tuple(got.shape) == shape_want
        assert got.numel() * got.element_size() == 3 * od.out_geometry(p, w, h, False, dtype, layout, "level")["bytes_per_pair"]
        assert_bits(_np(got), transform(want, dtype, layout), f"{shape} level {dtype} {layout}")


# ------------------------------------------------------------------------------------------------ 3. issue forms

def test_issue_forms():
    """Five pairs in chunks over streams, with and without graphs: every chunk writes at its own byte offset."""
    import torch
    import of_dis_amd as od
    w, h = 176, 96
    fr = _dev(sequence(w, h, 1, 7))
    a, b = fr[:-2], fr[2:]
    p = params(S_176)
    c = od.Context(0)
    want = _np(c.run(a, b, p))
    want_level = level_reference(c, S_176, p, _np(a), _np(b))
    for streams, chunk, graph in ISSUES:
        c.set_option("streams", streams)
        c.set_option("chunk", chunk)
        c.set_option("graph", graph)
        what = str((streams, chunk, graph))
        assert_bits(_np(c.run(a, b, p, dtype=torch.float16, layout="nchw")), transform(want, "float16", "nchw"), what)
        assert_bits(_np(c.run(a, b, p, dtype=torch.float16, grid="level")), transform(want_level, "float16", "nhwc"),
                    what + " level")
        assert_bits(_np(c.run(a, b, p)), want, what + " plain")
    c.close()


# ------------------------------------------------------------------------------------------------ 4. graph keys, extent

def test_graph_keys_and_extent():
    """Plain, float16, level and plain again on ONE output buffer, each twice (record, then replay): every call gives
    its own result, and a compact format leaves the bytes beyond n * bytes_per_pair alone."""
    import torch
    import of_dis_amd as od
    w, h, n = 176, 96, 2
    p = params(S_176)
    a, b = (_dev(x) for x in pairs(S_176, n))
    c = od.Context(0)
    want = _np(c.run(a, b, p))
    want_level = level_reference(c, S_176, p, *pairs(S_176, n))
    cases = [(od.out_format(), want),
             (od.out_format("float16"), transform(want, "float16", "nhwc")),
             (od.out_format("float32", "nhwc", "level"), want_level),
             (od.out_format(), want)]
    buf = torch.empty(want.nbytes, dtype=torch.uint8, device="cuda")
    for fmt, exp in cases:
        for rep in range(2):
            buf.fill_(0xA5)
            c.run_ptr_fmt(a.data_ptr(), b.data_ptr(), n, w, h, p, fmt, buf.data_ptr())
            raw = _np(buf)
            what = f"format ({fmt.dtype}, {fmt.layout}, {fmt.grid}) call {rep}"
            assert_bits(raw[:exp.nbytes].view(exp.dtype).reshape(exp.shape), exp, what)
            assert (raw[exp.nbytes:] == 0xA5).all(), what + ": wrote beyond n * bytes_per_pair"
    c.close()


# ------------------------------------------------------------------------------------------------ 5. sequences, init

@pytest.mark.parametrize("stride", [1, 2])
def test_sequence_formats(ctx, stride):
    import torch
    w, h = 176, 96
    fr = _dev(sequence(w, h, 1, 5))
    p = params(S_176)
    a, b = fr[:-stride], fr[stride:]
    for kw in (dict(dtype=torch.float16, layout="nchw"), dict(grid="level"), dict(dtype=torch.float16, grid="level")):
        want = _np(ctx.run(a, b, p, **kw))
        got = ctx.run_sequence(fr, p, stride=stride, **kw)
        assert_bits(_np(got), want, f"stride {stride} {kw}")
    assert_bits(ctx.run_sequence_host(_np(fr), p, stride=stride, dtype=np.float16, layout="nchw"),
                _np(ctx.run(a, b, p, dtype=torch.float16, layout="nchw")), "host form")


def test_init_formats(ctx):
    """With an initial flow the frame is padded to 2^(sc_f+1): 173 x 97 has another level grid then."""
    import torch
    import of_dis_amd as od
    w, h = 173, 97
    fr = sequence(w, h, 1, 4)
    p = params(S_173)
    a, b = _dev(fr[:-1]), _dev(fr[1:])
    init = ctx.run(a, b, p)
    want = _np(ctx.run(a, b, p, init=init))
    assert_bits(_np(ctx.run(a, b, p, init=init, dtype=torch.float16, layout="nchw")), transform(want, "float16", "nchw"),
                "init float16 planar")
    g0, g1 = od.out_geometry(p, w, h, False, grid="level"), od.out_geometry(p, w, h, True, grid="level")
    assert (g0["out_w"], g0["out_h"]) != (g1["out_w"], g1["out_h"])
    want_level = level_reference(ctx, S_173, p, fr[:-1], fr[1:], init=_np(init))
    lev = ctx.run(a, b, p, init=init, grid="level")
    assert tuple(lev.shape) == (3, g1["out_h"], g1["out_w"], 2)
    assert_bits(_np(lev), want_level, "init level")
    seq = ctx.run_sequence(_dev(fr), p, init=init, grid="level")
    assert_bits(_np(seq), want_level, "sequence init level")
    assert_bits(_np(ctx.run_sequence(_dev(fr), p, init=init, dtype=torch.float16)), transform(want, "float16", "nhwc"),
                "sequence init float16")


# ------------------------------------------------------------------------------------------------ 6. latency mode

def test_latency_mode():
    import of_dis_amd as od
    c = od.Context(0)
    c.set_option("sor_mode", 1)
    p = params(S_176)
    a, b = (_dev(x) for x in pairs(S_176, 2))
    want = _np(c.run(a, b, p))
    for dtype, layout in FORMATS:
        assert_bits(_np(c.run(a, b, p, dtype=_tdtype(dtype), layout=layout)), transform(want, dtype, layout),
                    f"sor_mode 1 {dtype} {layout}")
    want_level = level_reference(c, S_176, p, *pairs(S_176, 2))
    assert_bits(_np(c.run(a, b, p, dtype=_tdtype("float16"), layout="nchw", grid="level")),
                transform(want_level, "float16", "nchw"), "sor_mode 1 level")
    c.close()


# ------------------------------------------------------------------------------------------------ 7. refusals

def test_refusals(ctx):
    import torch
    import of_dis_amd as od
    L = od.lib()
    w, h, n = 176, 96, 2
    p = params(S_176)
    a, b = (_dev(x) for x in pairs(S_176, n))
    want = _np(ctx.run(a, b, p))
    buf = torch.full((want.nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    INV = od._lib.ERR_INVALID_ARGUMENT
    fr = _dev(sequence(w, h, 1, 3))
    for bad in ((2, 0, 0), (0, 2, 0), (0, 0, 2), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (7, 7, 7)):
        fmt = od.OutFormat(*bad)
        assert L.ofdis_run_batch_u8_fmt(ctx._h, a.data_ptr(), b.data_ptr(), None, n, w, h, C.byref(p), C.byref(fmt),
                                        buf.data_ptr(), None) == INV, bad
        assert L.ofdis_run_sequence_u8_fmt(ctx._h, fr.data_ptr(), 3, 1, None, w, h, C.byref(p), C.byref(fmt),
                                           buf.data_ptr(), None) == INV, bad
    good = od.out_format("float16", "nchw")
    assert L.ofdis_run_batch_u8_fmt(ctx._h, a.data_ptr(), b.data_ptr(), None, n, w, h, C.byref(p), C.byref(good),
                                    None, None) == INV                                    # NULL flow_out
    assert L.ofdis_run_batch_u8_fmt(ctx._h, a.data_ptr(), b.data_ptr(), None, 0, w, h, C.byref(p), C.byref(good),
                                    buf.data_ptr(), None) == INV                          # the plain call's errors
    assert L.ofdis_run_batch_u8_fmt(ctx._h, a.data_ptr(), b.data_ptr(), None, n, w, h, C.byref(p.copy(p_samp_s=7)),
                                    C.byref(good), buf.data_ptr(), None) == INV
    assert L.ofdis_run_sequence_u8_fmt(ctx._h, fr.data_ptr(), 3, 3, None, w, h, C.byref(p), C.byref(good),
                                       buf.data_ptr(), None) == INV
    assert (_np(buf) == 0xA5).all()  # nothing was enqueued
    with pytest.raises(od.OfdisError) as e:
        ctx.run_sequence(fr, p, bidir=True, dtype=torch.float16)
    assert e.value.code == od._lib.ERR_UNSUPPORTED
    with pytest.raises(od.OfdisError):
        ctx.run(a, b, p, layout="chwn")
    # the context stays usable
    assert_bits(_np(ctx.run(a, b, p)), want, "plain call after the refusals")
    assert_bits(_np(ctx.run(a, b, p, dtype=torch.float16)), transform(want, "float16", "nhwc"), "float16 afterwards")

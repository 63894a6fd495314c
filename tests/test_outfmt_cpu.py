"""Output formats, the parts that need no GPU: ofdis_out_geometry against its formula restated in numpy, the
refusals of bad enums, sizes and parameters, and the new symbols' argument lists as include/ofdis.h declares them."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import of_dis_amd as od
from of_dis_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = _lib.ERR_INVALID_ARGUMENT
SIZES = [(176, 96), (173, 97), (1920, 1080), (2100, 70)]
FORMATS = list(itertools.product(("float32", "float16"), ("nhwc", "nchw"), ("full", "level")))


def expected(p, w, h, with_init, dtype, grid):
    """include/ofdis.h, restated: the frame padded to a multiple of 2^sc_f (2^(sc_f+1) with an initial flow), the
    padding split floor / ceil, the level grid that of the padded frame."""
    d = np.int64(1) << (p.sc_f + (1 if with_init else 0))
    padw, padh = (-w) % d, (-h) % d
    if grid == "level":
        ow, oh, ox, oy, cell = (w + padw) >> p.sc_l, (h + padh) >> p.sc_l, padw // 2, padh // 2, 1 << p.sc_l
    else:
        ow, oh, ox, oy, cell = w, h, 0, 0, 1
    return dict(out_w=int(ow), out_h=int(oh), off_x=int(ox), off_y=int(oy), cell=int(cell),
                bytes_per_pair=int(ow) * int(oh) * p.nop * np.dtype(dtype).itemsize)


@pytest.mark.parametrize("mode", [od.MODE_OF, od.MODE_DE])
@pytest.mark.parametrize("op", [1, 2, 3])
@pytest.mark.parametrize("w,h", SIZES)
def test_out_geometry(w, h, op, mode):
    p = od.oppoint(op, w, mode, 1)
    for with_init in (False, True):
        for dtype, layout, grid in FORMATS:
            got = od.out_geometry(p, w, h, with_init, dtype, layout, grid)
            assert got == expected(p, w, h, with_init, dtype, grid), (with_init, dtype, layout, grid)
            if grid == "level":  # the cells cover the frame: the first reaches pixel 0, the last the last pixel
                assert got["out_w"] * got["cell"] - got["off_x"] >= w and got["out_h"] * got["cell"] - got["off_y"] >= h


def test_out_geometry_null_format_and_outputs():
    """A NULL format is the plain one; every output pointer may be NULL."""
    L = od.lib()
    p = od.oppoint(2, 173, od.MODE_OF, 1)
    ow, nb = C.c_int(), C.c_size_t()
    assert L.ofdis_out_geometry(C.byref(p), 173, 97, 0, None, C.byref(ow), None, None, None, None, C.byref(nb)) == 0
    assert (ow.value, nb.value) == (173, 173 * 97 * 2 * 4)
    assert L.ofdis_out_geometry(C.byref(p), 173, 97, 0, None, None, None, None, None, None, None) == 0


def test_out_geometry_refusals():
    L = od.lib()
    p = od.oppoint(2, 176, od.MODE_OF, 1)

    def call(q, w, h, fmt):
        nb = C.c_size_t(12345)
        rc = L.ofdis_out_geometry(C.byref(q) if q is not None else None, w, h, 0,
                                  C.byref(_lib.OutFormat(*fmt)), None, None, None, None, None, C.byref(nb))
        assert rc == 0 or nb.value == 12345  # a refusal writes nothing
        return rc

    assert call(p, 176, 96, (0, 0, 0)) == 0 and call(p, 176, 96, (1, 1, 1)) == 0
    for fmt in ((2, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -1, 0), (0, 0, 2), (0, 0, -1)):
        assert call(p, 176, 96, fmt) == INV, fmt
    for w, h in ((0, 96), (176, 0), (-176, 96), (176, -1)):
        assert call(p, w, h, (1, 1, 1)) == INV, (w, h)
    assert call(None, 176, 96, (0, 0, 0)) == INV
    for bad in (dict(mode=3), dict(noc=2), dict(sc_l=-1), dict(sc_l=p.sc_f + 1), dict(p_samp_s=7)):
        assert call(p.copy(**bad), 176, 96, (1, 0, 1)) == INV, bad
    # the Python spellings: an unknown dtype, layout or grid raises before the library is called
    for kw in (dict(dtype="bfloat16"), dict(dtype=np.float64), dict(layout="chwn"), dict(grid="coarse")):
        with pytest.raises(od.OfdisError) as e:
            od.out_geometry(p, 176, 96, **kw)
        assert e.value.code == INV


def test_run_fmt_null_refusals():
    """NULL context, images or output: refused before anything touches a device."""
    L = od.lib()
    p = od.oppoint(2, 64, od.MODE_OF, 1)
    img = np.zeros((3, 64, 64), np.uint8)
    out = np.zeros((2, 64, 64, 2), np.float32)
    fmt = _lib.OutFormat(1, 1, 0)
    a, o = img.ctypes.data, out.ctypes.data
    assert L.ofdis_run_batch_u8_fmt(None, a, a, None, 2, 64, 64, C.byref(p), C.byref(fmt), o, None) == INV
    assert L.ofdis_run_batch_u8_fmt_host(None, a, a, None, 2, 64, 64, C.byref(p), C.byref(fmt), o) == INV
    assert L.ofdis_run_sequence_u8_fmt(None, a, 3, 1, None, 64, 64, C.byref(p), C.byref(fmt), o, None) == INV
    assert L.ofdis_run_sequence_u8_fmt_host(None, a, 3, 1, None, 64, 64, C.byref(p), C.byref(fmt), o) == INV


def _header_args(name):
    """The parameter list of `name` in include/ofdis.h, one normalised type per parameter."""
    text = open(os.path.join(ROOT, "include", "ofdis.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    out = []
    for arg in m.group(1).split(","):
        arg = re.sub(r"/\*.*?\*/", "", arg).strip()
        out.append("ptr" if "*" in arg else arg.split()[-2] if len(arg.split()) > 1 else arg)
    return out


@pytest.mark.parametrize("name", ["ofdis_out_geometry", "ofdis_run_batch_u8_fmt", "ofdis_run_batch_u8_fmt_host",
                                  "ofdis_run_sequence_u8_fmt", "ofdis_run_sequence_u8_fmt_host"])
def test_symbols_declared_as_in_the_header(name):
    fn = getattr(od.lib(), name)
    want = _header_args(name)
    assert len(fn.argtypes) == len(want), (name, len(fn.argtypes), want)
    for t, w in zip(fn.argtypes, want):
        is_ptr = t in (C.c_void_p, C.c_char_p) or hasattr(t, "contents")
        assert is_ptr == (w == "ptr"), (name, t, w)
        if not is_ptr:
            assert {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t}[w] is t, (name, t, w)
    assert fn.restype is C.c_int


def test_abi_version_and_enums():
    assert od.lib().ofdis_abi_version() == 2  # functions are only added
    text = open(os.path.join(ROOT, "include", "ofdis.h")).read()
    for name, value in (("OUT_F32", 0), ("OUT_F16", 1), ("OUT_INTERLEAVED", 0), ("OUT_PLANAR", 1), ("OUT_FULL", 0),
                        ("OUT_LEVEL", 1)):
        assert re.search(r"\bOFDIS_%s\s*=\s*%d\b" % (name, value), text), name
        assert getattr(_lib, name) == value
    assert [f[0] for f in _lib.OutFormat._fields_] == ["dtype", "layout", "grid"]


def test_kernel_names_and_byte_models():
    """The formatted stores are timed under their own names ("upsample" stays the plain format alone), each with a
    byte model: the bytes written, plus the level plane read for level_out."""
    names = set(od.kernel_names())
    assert {"upsample", "upsample_f16", "upsample_planar", "upsample_planar_f16", "level_out"} <= names
    p = od.oppoint(2, 1920, od.MODE_OF, 1)
    px = 1920 * 1080 * 2
    assert od.algorithmic_bytes(p, 1920, 1080, "upsample") == px * 4
    assert od.algorithmic_bytes(p, 1920, 1080, "upsample_planar") == px * 4
    assert od.algorithmic_bytes(p, 1920, 1080, "upsample_f16") == px * 2
    assert od.algorithmic_bytes(p, 1920, 1080, "upsample_planar_f16") == px * 2
    g = od.out_geometry(p, 1920, 1080, grid="level")
    assert od.algorithmic_bytes(p, 1920, 1080, "level_out") == 2 * g["bytes_per_pair"]


def test_bidir_with_a_format_is_refused_without_the_library():
    """run_sequence_host(bidir=True) with a non-default format raises UNSUPPORTED before any call (no device here)."""
    class NoLibrary(od.Context):
        def __init__(self):
            self._h = None

    fr = np.zeros((3, 64, 64), np.uint8)
    p = od.oppoint(2, 64, od.MODE_OF, 1)
    with pytest.raises(od.OfdisError) as e:
        NoLibrary().run_sequence_host(fr, p, bidir=True, dtype=np.float16)
    assert e.value.code == _lib.ERR_UNSUPPORTED

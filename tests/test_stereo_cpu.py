"""The stereo entry points, the parts that need no GPU: the three new symbols' argument lists as include/ofdis.h
declares them, their ctypes bindings, the NULL-context refusal, the timers' names and the byte model."""
import ctypes as C
import os
import re

import numpy as np

import of_dis_amd as od
from of_dis_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = _lib.ERR_INVALID_ARGUMENT

DECLARED = {
    "ofdis_lr_check": (
        "ofdis_context *ctx, const float *disp_l, const float *disp_r, int n, int width, int height, "
        "float alpha, float beta, uint8_t *occ_l, uint8_t *occ_r, float *err_l, float *err_r, void *stream"),
    "ofdis_run_stereo_u8": (
        "ofdis_context *ctx, const uint8_t *img_l, const uint8_t *img_r, int n, int width, int height, "
        "const ofdis_params *p, float alpha, float beta, float *disp_l, float *disp_r, "
        "uint8_t *occ_l, uint8_t *occ_r, float *err_l, float *err_r, void *stream"),
    "ofdis_run_stereo_u8_host": (
        "ofdis_context *ctx, const uint8_t *img_l, const uint8_t *img_r, int n, int width, int height, "
        "const ofdis_params *p, float alpha, float beta, float *disp_l, float *disp_r, "
        "uint8_t *occ_l, uint8_t *occ_r, float *err_l, float *err_r"),
}


def _ctype(decl):
    """The ctypes type _lib.py binds for one declared parameter."""
    if "*" in decl:
        return C.POINTER(_lib.Params) if "ofdis_params" in decl else C.c_void_p
    return {"int": C.c_int, "float": C.c_float}[decl.split()[0]]


def test_header_declares_the_stereo_calls_and_lib_binds_them():
    L = od.lib()
    hdr = open(os.path.join(ROOT, "include", "ofdis.h")).read()
    for name, want in DECLARED.items():
        m = re.search(rf"\bint {name}\(([^;]*)\);", hdr)
        assert m, f"{name} is not declared in ofdis.h"
        decl = re.sub(r"\s+", " ", m.group(1)).strip()
        assert decl == want, name
        args = [a.strip() for a in decl.split(",")]
        fn = getattr(L, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(args), name
        for k, (a, t) in enumerate(zip(args, fn.argtypes)):
            assert t is _ctype(a), (name, k, a, t)
    assert hdr.index("stereo: both views and left-right masks") > hdr.index("both directions and occlusion masks")
    assert hdr.index("stereo: both views and left-right masks") < hdr.index("video sequences")
    assert L.ofdis_abi_version() == 2  # functions were added, nothing changed


def test_python_layer_exposes_the_stereo_calls():
    for name in ("lr_check_ptr", "lr_check", "run_stereo_ptr", "run_stereo", "run_stereo_host"):
        assert callable(getattr(od.Context, name)), name


def test_null_context_and_bad_arguments_are_refused():
    L = od.lib()
    p = od.oppoint(2, 64, od.MODE_DE, 1)
    buf = np.zeros(64 * 64, np.float32)
    img = np.zeros(64 * 64, np.uint8)
    d, im = buf.ctypes.data, img.ctypes.data
    assert L.ofdis_lr_check(None, d, d, 1, 64, 64, 0.01, 0.5, im, None, None, None, None) == INV
    assert L.ofdis_run_stereo_u8(None, im, im, 1, 64, 64, C.byref(p), 0.01, 0.5, d, None, None, None, None, None,
                                 None) == INV
    assert L.ofdis_run_stereo_u8_host(None, im, im, 1, 64, 64, C.byref(p), 0.01, 0.5, d, None, None, None, None,
                                      None) == INV


def test_timer_names_and_byte_model():
    assert {"lr_check", "lr_check_err"} <= set(od.kernel_names())
    hdr = open(os.path.join(ROOT, "include", "ofdis.h")).read()
    assert '"lr_check"' in hdr and '"lr_check_err"' in hdr
    p = od.oppoint(2, 1920, od.MODE_DE, 1)
    assert od.algorithmic_bytes(p, 1920, 1080, "lr_check") == 2 * 1920 * 1080 * 9
    assert od.algorithmic_bytes(p, 1920, 1080, "lr_check_err") == 2 * 1920 * 1080 * 13
    # fb_check's model is untouched
    assert od.algorithmic_bytes(p, 1920, 1080, "fb_check") == 2 * 1920 * 1080 * 17

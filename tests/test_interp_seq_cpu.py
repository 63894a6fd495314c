"""The level-grid consistency check, the fused interpolation with masks and the sequence interpolation: the parts that
need no GPU -- the new entry points' signatures and NULL-context refusals, the kernel-name table and byte model, and
the run_OF_SEQ_INTERP_INT / run_OF_SEQ_INTERP_RGB command lines' usage, size and no-device exits."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import of_dis_amd as od

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "of_dis_amd", "bin")
CLIS = ["run_OF_SEQ_INTERP_INT", "run_OF_SEQ_INTERP_RGB"]
INV = od._lib.ERR_INVALID_ARGUMENT

# the new entry points (the five C functions; the sixth symbol a caller sees is the timer name, checked below)
DECLS = {
    "ofdis_fb_check_level": (
        "ofdis_context *ctx, const float *grid_fw, const float *grid_bw, const ofdis_flow_view *view, int n, "
        "int width, int height, float alpha, float beta, uint8_t *occ_fw, uint8_t *occ_bw, float *err_fw, "
        "float *err_bw, void *stream"),
    "ofdis_run_interp_occ_u8": (
        "ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height, "
        "const ofdis_params *p, const float *t, int nt, float alpha, float beta, int out_dtype, void *out, "
        "uint8_t *valid, uint8_t *occ_fw, uint8_t *occ_bw, void *stream"),
    "ofdis_run_interp_occ_u8_host": (
        "ofdis_context *ctx, const uint8_t *img_a, const uint8_t *img_b, int n, int width, int height, "
        "const ofdis_params *p, const float *t, int nt, float alpha, float beta, int out_dtype, void *out, "
        "uint8_t *valid, uint8_t *occ_fw, uint8_t *occ_bw"),
    "ofdis_run_sequence_interp_u8": (
        "ofdis_context *ctx, const uint8_t *frames, int nframes, int stride, int width, int height, "
        "const ofdis_params *p, const float *t, int nt, int use_occ, float alpha, float beta, int out_dtype, "
        "void *out, uint8_t *valid, uint8_t *occ_fw, uint8_t *occ_bw, void *stream"),
    "ofdis_run_sequence_interp_u8_host": (
        "ofdis_context *ctx, const uint8_t *frames, int nframes, int stride, int width, int height, "
        "const ofdis_params *p, const float *t, int nt, int use_occ, float alpha, float beta, int out_dtype, "
        "void *out, uint8_t *valid, uint8_t *occ_fw, uint8_t *occ_bw"),
}


def _ctype(decl):
    """The ctypes type of one declared C parameter."""
    if "*" in decl:
        if "ofdis_params" in decl:
            return C.POINTER(od.Params)
        if "ofdis_flow_view" in decl:
            return C.POINTER(od._lib.FlowView)
        return C.c_void_p
    return {"int": C.c_int, "float": C.c_float}[decl.split()[0]]


def test_symbols_exist_with_declared_signatures():
    L = od.lib()
    hdr = open(os.path.join(ROOT, "include", "ofdis.h")).read()
    for name, want in DECLS.items():
        fn = getattr(L, name)
        m = re.search(rf"\bint {name}\(([^;]*)\);", hdr)
        assert m, f"{name} is not declared in ofdis.h"
        assert re.sub(r"\s+", " ", m.group(1)) == want, name
        args = [a.strip() for a in want.split(",")]
        assert fn.restype is C.c_int and list(fn.argtypes) == [_ctype(a) for a in args], name
    assert L.ofdis_abi_version() == 2  # functions were added, nothing changed
    for method in ("fb_check_level_ptr", "run_interp_occ_ptr", "run_sequence_interp", "run_sequence_interp_ptr",
                   "run_sequence_interp_host"):
        assert callable(getattr(od.Context, method))


def test_null_context_is_refused():
    L = od.lib()
    p = od.oppoint(2, 64, od.MODE_OF, 1)
    grid = np.zeros(32 * 32 * 2, np.float32)
    img = np.zeros((3, 64, 64), np.uint8)
    out = np.zeros((2, 64, 64), np.uint8)
    t = np.array([0.5], np.float32)
    view = od._lib.FlowView(od._lib.OUT_F32, od._lib.OUT_INTERLEAVED, od._lib.OUT_LEVEL, 32, 32, 2, 0, 0)
    g, im, o, tp = grid.ctypes.data, img.ctypes.data, out.ctypes.data, t.ctypes.data
    assert L.ofdis_fb_check_level(None, g, g, C.byref(view), 1, 64, 64, 0.01, 0.5, o, None, None, None, None) == INV
    assert L.ofdis_run_interp_occ_u8(None, im, im, 1, 64, 64, C.byref(p), tp, 1, 0.01, 0.5, 0, o, None, None, None,
                                     None) == INV
    assert L.ofdis_run_interp_occ_u8_host(None, im, im, 1, 64, 64, C.byref(p), tp, 1, 0.01, 0.5, 0, o, None, None,
                                          None) == INV
    for use_occ in (0, 1):
        assert L.ofdis_run_sequence_interp_u8(None, im, 3, 1, 64, 64, C.byref(p), tp, 1, use_occ, 0.01, 0.5, 0, o, None,
                                              None, None, None) == INV
        assert L.ofdis_run_sequence_interp_u8_host(None, im, 3, 1, 64, 64, C.byref(p), tp, 1, use_occ, 0.01, 0.5, 0, o,
                                                   None, None, None) == INV


def test_kernel_name_and_byte_model():
    assert "fb_check_level" in od.kernel_names()
    # both grids once (8 bytes per cell), the mask byte and the 4-byte error per pixel and direction
    p = od.oppoint(2, 1920, od.MODE_OF, 1)
    g = od.out_geometry(p, 1920, 1080, grid="level")
    assert (g["out_w"], g["out_h"]) == (120, 68)
    assert od.algorithmic_bytes(p, 1920, 1080, "fb_check_level") == 2 * 120 * 68 * 8 + 2 * 1920 * 1080 * (1 + 4)
    p = od.oppoint(3, 173, od.MODE_OF, 3)
    g = od.out_geometry(p, 173, 97, grid="level")
    assert od.algorithmic_bytes(p, 173, 97, "fb_check_level") == 2 * g["out_w"] * g["out_h"] * 8 + 2 * 173 * 97 * 5


@pytest.mark.parametrize("exe", CLIS)
@pytest.mark.parametrize("args", [[], ["out_"], ["out_", "2", "2", "0", "a.png"],   # one image
                                  ["out_", "0", "2", "0", "a.png", "b.png"],        # K out of range
                                  ["out_", "17", "2", "0", "a.png", "b.png"],
                                  ["out_", "2", "5", "0", "a.png", "b.png"],        # operating point out of range
                                  ["out_", "2", "2", "2", "a.png", "b.png"],        # occ not 0 / 1
                                  ["out_", "2", "2", "x", "a.png", "b.png"]])
def test_cli_usage(exe, args):
    path = os.path.join(BIN, exe)
    assert os.access(path, os.X_OK)
    r = subprocess.run([path] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stderr


def _pnm(tmp_path, name, im):
    h, w, noc = im.shape
    head = b"P5" if noc == 1 else b"P6"
    data = im if noc == 1 else im[..., ::-1]
    (tmp_path / name).write_bytes(head + b"\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(data).tobytes())
    return str(tmp_path / name)


@pytest.mark.parametrize("exe,noc", [("run_OF_SEQ_INTERP_INT", 1), ("run_OF_SEQ_INTERP_RGB", 3)])
def test_cli_sizes_and_no_device(tmp_path, exe, noc):
    """Images of two sizes: exit 1 with a message, before a device is looked for.  No visible device: a non-zero exit
    with the no-device message and no output file (the devices are hidden from the child process, so this runs the
    same on a GPU machine)."""
    path = os.path.join(BIN, exe)
    a, b = od.synth_pair(64, 64, noc, 0)
    small = od.synth_pair(48, 64, noc, 0)[0]
    files = [_pnm(tmp_path, "a.pnm", a), _pnm(tmp_path, "b.pnm", b), _pnm(tmp_path, "c.pnm", small)]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([path, str(tmp_path / "o_"), "2", "2", "1", files[0], files[1]], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode != 0 and "no usable gfx950 device" in r.stderr
    assert not list(tmp_path.glob("o_*"))
    r = subprocess.run([path, str(tmp_path / "o_"), "2", "2", "0", files[0], files[1], "missing.png"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and not list(tmp_path.glob("o_*"))
    # every image's size is checked before a device is looked for
    r = subprocess.run([path, str(tmp_path / "o_"), "2", "2", "1", files[0], files[1], files[2]], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 1 and "image sizes differ" in r.stderr

"""ctypes bindings to of_dis_amd/libofdis.so (the C-ABI declared in include/ofdis.h).

The shared library is the product: HIP kernels for gfx950 plus the host runtime.  There is no CPU
fallback -- if the library is missing or no gfx950 device is visible, calls fail loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# OFDIS_LIB: another build of the same library (A/B timing of kernel variants, tools/ab_session.sh)
LIB_PATH = os.environ.get("OFDIS_LIB") or os.path.join(PKG_DIR, "libofdis.so")
CSRC = os.path.join(PKG_DIR, "csrc")

OK = 0
ERR_INVALID_ARGUMENT = 1
ERR_UNSUPPORTED = 2
ERR_OUT_OF_MEMORY = 3
ERR_DEVICE = 4
ERR_NO_DEVICE = 5
ERR_IO = 6

MODE_OF = 1
MODE_DE = 2

# ofdis_out_format (include/ofdis.h): element type, layout and grid of the forward flow
OUT_F32, OUT_F16 = 0, 1
OUT_INTERLEAVED, OUT_PLANAR = 0, 1
OUT_FULL, OUT_LEVEL = 0, 1
# out_dtype of the warp entry points
IMG_U8, IMG_F32 = 0, 1
# OFDIS_INTERP_MAX_T: the most times one interpolation call takes
INTERP_MAX_T = 16
# OFDIS_TRACK_LAST: a tracking call writes only the last frame's entry
TRACK_LAST = 1
# the models of ofdis_fit_motion, and its limits (OFDIS_FIT_MAX_SAMPLES, OFDIS_FIT_LANES)
MOTION_TRANSLATION, MOTION_SIMILARITY = 0, 1
FIT_MAX_SAMPLES = 65536
FIT_LANES = 256
# ofdis_flow_error: OFDIS_FE_LANES (the summation order), OFDIS_FE_NSTATS, OFDIS_FE_BINS, and the slots of a pair's stats
FE_LANES, FE_NSTATS, FE_BINS = 64, 16, 1024
(FE_COUNT, FE_NONFINITE, FE_SUM, FE_MAX, FE_GT1, FE_GT3, FE_GT5, FE_FL,
 FE_S0_COUNT, FE_S0_SUM, FE_S1_COUNT, FE_S1_SUM, FE_S2_COUNT, FE_S2_SUM) = range(14)
# ofdis_motion_mask: OFDIS_MM_NSTATS, the int64 numbers of a pair
MM_NSTATS = 12


class OfdisError(RuntimeError):
    def __init__(self, code: int, what: str = ""):
        self.code = code
        msg = lib().ofdis_status_string(code).decode() if _lib is not None else str(code)
        super().__init__(f"{what}: {msg} (status {code})" if what else f"{msg} (status {code})")


class Params(C.Structure):
    """ofdis_params (include/ofdis.h), mirroring OFC::optparam's explicit fields (oflow.h:45-66)."""

    _fields_ = [
        ("mode", C.c_int), ("noc", C.c_int), ("sc_f", C.c_int), ("sc_l", C.c_int),
        ("max_iter", C.c_int), ("min_iter", C.c_int),
        ("dp_thresh", C.c_float), ("dr_thresh", C.c_float), ("res_thresh", C.c_float),
        ("p_samp_s", C.c_int), ("patove", C.c_float), ("usefbcon", C.c_int), ("costfct", C.c_int),
        ("patnorm", C.c_int), ("usetvref", C.c_int),
        ("tv_alpha", C.c_float), ("tv_gamma", C.c_float), ("tv_delta", C.c_float),
        ("tv_innerit", C.c_int), ("tv_solverit", C.c_int), ("tv_sor", C.c_float), ("verbosity", C.c_int),
        ("omp_build", C.c_int), ("gradmag", C.c_int),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    def copy(self, **kw):
        q = Params()
        C.memmove(C.byref(q), C.byref(self), C.sizeof(Params))
        for k, v in kw.items():
            setattr(q, k, v)
        return q

    @property
    def nop(self) -> int:
        return 2 if self.mode == MODE_OF else 1

    def __repr__(self):
        return "Params(" + ", ".join(f"{k}={v!r}" for k, v in self.as_dict().items()) + ")"


class OutFormat(C.Structure):
    """ofdis_out_format (include/ofdis.h)."""

    _fields_ = [("dtype", C.c_int), ("layout", C.c_int), ("grid", C.c_int)]


class FlowView(C.Structure):
    """ofdis_flow_view (include/ofdis.h): how a warp reads its flow -- an OutFormat plus, for the level grid, the
    geometry ofdis_out_geometry reports."""

    _fields_ = [("dtype", C.c_int), ("layout", C.c_int), ("grid", C.c_int), ("gw", C.c_int), ("gh", C.c_int),
                ("cell", C.c_int), ("off_x", C.c_int), ("off_y", C.c_int)]


def out_format(dtype="float32", layout="nhwc", grid="full") -> OutFormat:
    """OutFormat from the Python spellings: dtype float32 / float16 (a numpy or torch dtype, or its name), layout
    "nhwc" (interleaved) / "nchw" (planar), grid "full" / "level".  Anything else raises OfdisError(INVALID_ARGUMENT)."""
    name = str(getattr(dtype, "__name__", dtype)).replace("torch.", "")
    try:
        return OutFormat({"float32": OUT_F32, "float16": OUT_F16, "half": OUT_F16, "float": OUT_F32}[name],
                         {"nhwc": OUT_INTERLEAVED, "nchw": OUT_PLANAR}[layout], {"full": OUT_FULL, "level": OUT_LEVEL}[grid])
    except (KeyError, TypeError):
        raise OfdisError(ERR_INVALID_ARGUMENT, f"output format ({dtype!r}, {layout!r}, {grid!r})") from None


def build(verbose: bool = False) -> None:
    """Compile libofdis.so (+ CLI binaries) for gfx950 with hipcc, in-tree."""
    jobs = os.environ.get("MAX_JOBS", "4")
    subprocess.run(["make", "-s", "-j", str(jobs), "-C", CSRC], check=True,
                   stdout=None if verbose else subprocess.DEVNULL)


_lib = None


def lib():
    """Load libofdis.so; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    try:  # load torch's HIP runtime first: libofdis then binds to it (same SONAME) -> one runtime per process
        import torch  # noqa: F401
    except Exception:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C of_dis_amd/csrc` (hipcc, gfx950)")
    L = C.CDLL(LIB_PATH)
    vp, i, f, d = C.c_void_p, C.c_int, C.c_float, C.c_double
    P = C.POINTER(Params)
    F = C.POINTER(OutFormat)
    V = C.POINTER(FlowView)
    sig = {
        "ofdis_abi_version": ([], i),
        "ofdis_status_string": ([i], C.c_char_p),
        "ofdis_auto_first_scale": ([i, i, i], i),
        "ofdis_params_oppoint": ([P, i, i, i, i], i),
        "ofdis_params_from_strings": ([P, i, C.POINTER(C.c_char_p), i, i], i),
        "ofdis_params_validate": ([P, i, i, i], i),
        "ofdis_oflow_compute": ([vp] * 6 + [i, vp, vp, i, i, P], i),
        "ofdis_context_create": ([i, C.POINTER(vp)], i),
        "ofdis_context_destroy": ([vp], None),
        "ofdis_run_batch_u8": ([vp, vp, vp, i, i, i, P, vp, vp], i),
        "ofdis_run_batch_u8_host": ([vp, vp, vp, i, i, i, P, vp], i),
        "ofdis_run_batch_u8_init": ([vp, vp, vp, vp, i, i, i, P, vp, vp], i),
        "ofdis_run_batch_u8_init_host": ([vp, vp, vp, vp, i, i, i, P, vp], i),
        "ofdis_fb_check": ([vp, vp, vp, i, i, i, f, f, vp, vp, vp, vp, vp], i),
        "ofdis_run_bidir_u8": ([vp, vp, vp, i, i, i, P, f, f, vp, vp, vp, vp, vp, vp, vp], i),
        "ofdis_run_bidir_u8_host": ([vp, vp, vp, i, i, i, P, f, f, vp, vp, vp, vp, vp, vp], i),
        "ofdis_lr_check": ([vp, vp, vp, i, i, i, f, f, vp, vp, vp, vp, vp], i),
        "ofdis_run_stereo_u8": ([vp, vp, vp, i, i, i, P, f, f, vp, vp, vp, vp, vp, vp, vp], i),
        "ofdis_run_stereo_u8_host": ([vp, vp, vp, i, i, i, P, f, f, vp, vp, vp, vp, vp, vp], i),
        "ofdis_run_sequence_u8": ([vp, vp, i, i, vp, i, i, P, f, f, vp, vp, vp, vp, vp, vp, vp], i),
        "ofdis_run_sequence_u8_host": ([vp, vp, i, i, vp, i, i, P, f, f, vp, vp, vp, vp, vp, vp], i),
        "ofdis_out_geometry": ([P, i, i, i, F] + [C.POINTER(i)] * 5 + [C.POINTER(C.c_size_t)], i),
        "ofdis_run_batch_u8_fmt": ([vp, vp, vp, vp, i, i, i, P, F, vp, vp], i),
        "ofdis_run_batch_u8_fmt_host": ([vp, vp, vp, vp, i, i, i, P, F, vp], i),
        "ofdis_run_sequence_u8_fmt": ([vp, vp, i, i, vp, i, i, P, F, vp, vp], i),
        "ofdis_run_sequence_u8_fmt_host": ([vp, vp, i, i, vp, i, i, P, F, vp], i),
        "ofdis_warp_u8": ([vp, vp, vp, V, i, i, i, i, f, i, vp, vp, vp], i),
        "ofdis_run_warp_u8": ([vp, vp, vp, i, i, i, P, f, i, vp, vp, vp], i),
        "ofdis_run_warp_u8_host": ([vp, vp, vp, i, i, i, P, f, i, vp, vp], i),
        "ofdis_interp_u8": ([vp, vp, vp, vp, vp, V, i, i, i, i, vp, i, vp, vp, i, vp, vp, vp], i),
        "ofdis_run_interp_u8": ([vp, vp, vp, i, i, i, P, vp, i, i, vp, vp, vp], i),
        "ofdis_run_interp_u8_host": ([vp, vp, vp, i, i, i, P, vp, i, i, vp, vp], i),
        "ofdis_fb_check_level": ([vp, vp, vp, V, i, i, i, f, f, vp, vp, vp, vp, vp], i),
        "ofdis_run_interp_occ_u8": ([vp, vp, vp, i, i, i, P, vp, i, f, f, i, vp, vp, vp, vp, vp], i),
        "ofdis_run_interp_occ_u8_host": ([vp, vp, vp, i, i, i, P, vp, i, f, f, i, vp, vp, vp, vp], i),
        "ofdis_run_sequence_interp_u8": ([vp, vp, i, i, i, i, P, vp, i, i, f, f, i, vp, vp, vp, vp, vp], i),
        "ofdis_run_sequence_interp_u8_host": ([vp, vp, i, i, i, i, P, vp, i, i, f, f, i, vp, vp, vp, vp], i),
        "ofdis_track_points": ([vp, vp, vp, V, i, i, i, vp, vp, i, f, f, i, vp, vp, vp], i),
        "ofdis_run_sequence_track_u8": ([vp, vp, i, i, i, P, vp, vp, i, i, f, f, i, vp, vp, vp], i),
        "ofdis_run_sequence_track_u8_host": ([vp, vp, i, i, i, P, vp, vp, i, i, f, f, i, vp, vp], i),
        "ofdis_tfilter_u8": ([vp, vp, i, vp, vp, V, i, i, i, f, vp, vp, i, vp, vp, vp], i),
        "ofdis_run_sequence_tfilter_u8": ([vp, vp, i, i, i, P, f, i, f, f, i, vp, vp, vp], i),
        "ofdis_run_sequence_tfilter_u8_host": ([vp, vp, i, i, i, P, f, i, f, f, i, vp, vp], i),
        "ofdis_tfilter_radius_u8": ([vp, vp, i, vp, vp, V, i, i, i, i, f, i, f, f, i, vp, vp, vp], i),
        "ofdis_run_sequence_tfilter_radius_u8": ([vp, vp, i, i, i, P, i, f, i, f, f, i, vp, vp, vp], i),
        "ofdis_run_sequence_tfilter_radius_u8_host": ([vp, vp, i, i, i, P, i, f, i, f, f, i, vp, vp], i),
        "ofdis_fit_motion": ([vp, vp, vp, V, i, i, i, i, i, d, i, f, f, vp, vp, vp, vp], i),
        "ofdis_smooth_path": ([vp, vp, i, i, d, i, i, vp, vp], i),
        "ofdis_warp_affine_u8": ([vp, vp, i, i, i, i, vp, i, vp, vp, vp], i),
        "ofdis_run_sequence_stabilize_u8": ([vp, vp, i, i, i, P, i, i, d, i, i, f, f, i, d, i, vp, vp, vp, vp, vp, vp], i),
        "ofdis_run_sequence_stabilize_u8_host": ([vp, vp, i, i, i, P, i, i, d, i, i, f, f, i, d, i, vp, vp, vp, vp, vp], i),
        "ofdis_flow_error": ([vp, vp, V, vp, vp, i, i, i, i, vp, vp, vp, vp], i),
        "ofdis_run_error_u8": ([vp, vp, vp, vp, vp, i, i, i, i, P, vp, vp, vp, vp], i),
        "ofdis_run_error_u8_host": ([vp, vp, vp, vp, vp, i, i, i, i, P, vp, vp, vp], i),
        "ofdis_kernel_names_ext": ([], C.c_char_p),
        "ofdis_kernel_names_all": ([], C.c_char_p),
        "ofdis_motion_mask": ([vp, vp, V, i, i, i, vp, vp, f, f, i, vp, vp, vp, vp], i),
        "ofdis_run_sequence_motion_mask_u8": ([vp, vp, i, i, i, P, i, i, d, i, i, f, f, f, f, i, vp, vp, vp, vp, vp, vp, vp], i),
        "ofdis_run_sequence_motion_mask_u8_host": ([vp, vp, i, i, i, P, i, i, d, i, i, f, f, f, f, i, vp, vp, vp, vp, vp, vp], i),
        "ofdis_write_pnm": ([C.c_char_p, vp, i, i, i], i),
        "ofdis_pyramid_u8_host":([vp, vp, i, i, P, i, vp, vp, vp], i),
        "ofdis_context_set_stage_capture": ([vp, vp, vp, i], i),
        "ofdis_context_set_option": ([vp, C.c_char_p, i], i),
        "ofdis_context_enable_kernel_timing": ([vp, i], i),
        "ofdis_context_kernel_time": ([vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_long)], i),
        "ofdis_kernel_names": ([], C.c_char_p),
        "ofdis_algorithmic_bytes": ([P, i, i, C.c_char_p, C.POINTER(C.c_double)], i),
        "ofdis_tfilter_radius_bytes": ([P, i, i, i, i, i, C.POINTER(C.c_double)], i),
        "ofdis_max_frames_per_launch": ([P, i, i, C.POINTER(i)], i),
        "ofdis_write_flo": ([C.c_char_p, vp, i, i, i], i),
        "ofdis_write_pfm": ([C.c_char_p, vp, i, i], i),
        "ofdis_read_flo": ([C.c_char_p, vp, C.POINTER(i), C.POINTER(i), i], i),
        "ofdis_read_pnm": ([C.c_char_p, vp, C.POINTER(i), C.POINTER(i), C.POINTER(i), C.c_size_t], i),
        "ofdis_read_image": ([C.c_char_p, vp, C.POINTER(i), C.POINTER(i), i, C.c_size_t], i),
        "ofdis_synth_pair_u8": ([vp, vp, i, i, i, i, i], i),
        "ofdis_synth_shift_pair_u8": ([vp, vp, i, i, i, i, C.c_float, C.c_float], i),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    _lib = L
    return L


def check(rc: int, what: str = "") -> None:
    if rc != OK:
        raise OfdisError(rc, what)

"""Host-side mirror of the reference's operator interface for the hot path.

* ``OFClass`` -- same name, argument order and meaning as ``OFC::OFClass::OFClass`` (oflow.h:99-126):
  per-scale padded image/gradient pyramids in, flow at the finest computed scale out.  Computed on
  the GPU by libofdis.so (``ofdis_oflow_compute``).
* ``Context`` -- the batched device path (``ofdis_run_batch_u8``): u8 frame pairs already in HBM ->
  full-resolution flow, i.e. run_dense.cpp's main() minus image decode and file write.
* run_dense helpers: operating points, explicit parameters, .flo/.pfm I/O, synthetic pairs.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from ._lib import (ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED, FE_BINS, FE_COUNT, FE_FL, FE_GT1, FE_GT3, FE_GT5, FE_MAX,
                   FE_NONFINITE, FE_NSTATS, FE_S0_COUNT, FE_S0_SUM, FE_S1_COUNT, FE_S1_SUM, FE_S2_COUNT, FE_S2_SUM, FE_SUM,
                   FIT_MAX_SAMPLES, IMG_F32, IMG_U8, MM_NSTATS, MODE_DE, MODE_OF, MOTION_SIMILARITY, MOTION_TRANSLATION, TRACK_LAST,
                   FlowView, OfdisError, OutFormat, Params, check, lib, out_format)

_f32 = np.float32


def auto_first_scale(width: int, fratio: int = 5, patchsize: int = 8) -> int:
    """AutoFirstScaleSelect (run_dense.cpp:181-184)."""
    return lib().ofdis_auto_first_scale(width, fratio, patchsize)


def oppoint(op: int, width: int, mode: int = MODE_OF, noc: int = 1) -> Params:
    """Operating point 1-4 (run_dense.cpp:226-268) for an image of the given (unpadded) width."""
    p = Params()
    check(lib().ofdis_params_oppoint(C.byref(p), op, width, mode, noc), "ofdis_params_oppoint")
    return p


def params_from_strings(values: Sequence[str], mode: int = MODE_OF, noc: int = 1) -> Params:
    """The 20 explicit positional CLI parameters (run_dense.cpp:270-295)."""
    arr = (C.c_char_p * len(values))(*[str(v).encode() for v in values])
    p = Params()
    check(lib().ofdis_params_from_strings(C.byref(p), len(values), arr, mode, noc), "ofdis_params_from_strings")
    return p


def validate(p: Params, width: int = -1, height: int = -1, imgpadding: int = -1) -> int:
    return lib().ofdis_params_validate(C.byref(p), width, height, imgpadding)


def synth_pair(width: int, height: int, noc: int = 1, frame: int = 0, mode: int = MODE_OF):
    """Deterministic synthetic u8 pair [h][w][noc]; frame b moves by a known flow."""
    a = np.empty((height, width, noc), np.uint8)
    b = np.empty_like(a)
    check(lib().ofdis_synth_pair_u8(a.ctypes.data, b.ctypes.data, width, height, noc, frame, mode), "synth")
    return a, b


def synth_shift_pair(width: int, height: int, shift, noc: int = 1, frame: int = 0):
    """The synth_pair texture with frame b a pure translation of frame a by shift = (sx, sy) (true flow)."""
    a = np.empty((height, width, noc), np.uint8)
    b = np.empty((height, width, noc), np.uint8)
    check(lib().ofdis_synth_shift_pair_u8(a.ctypes.data, b.ctypes.data, width, height, noc, frame,
                                          float(shift[0]), float(shift[1])), "synth")
    return a, b


def write_flo(path: str, flow: np.ndarray) -> None:
    """SaveFlowFile (run_dense.cpp:17-58)."""
    flow = np.ascontiguousarray(flow, _f32)
    h, w = flow.shape[:2]
    nc = 1 if flow.ndim == 2 else flow.shape[2]
    check(lib().ofdis_write_flo(path.encode(), flow.ctypes.data, w, h, nc), "write_flo")


def write_pfm(path: str, depth: np.ndarray) -> None:
    """SavePFMFile (run_dense.cpp:61-82)."""
    depth = np.ascontiguousarray(depth.reshape(depth.shape[0], depth.shape[1]), _f32)
    check(lib().ofdis_write_pfm(path.encode(), depth.ctypes.data, depth.shape[1], depth.shape[0]), "write_pfm")


def read_flo(path: str, nc: int = 2) -> np.ndarray:
    """ReadFlowFile (run_dense.cpp:85-129)."""
    w, h = C.c_int(), C.c_int()
    check(lib().ofdis_read_flo(path.encode(), None, C.byref(w), C.byref(h), nc), "read_flo")
    out = np.empty((h.value, w.value, nc), _f32)
    check(lib().ofdis_read_flo(path.encode(), out.ctypes.data, C.byref(w), C.byref(h), nc), "read_flo")
    return out


def read_image(path: str, noc: int = 1) -> np.ndarray:
    """cv::imread(path, GRAYSCALE if noc == 1 else COLOR) for PNG / Netpbm: u8 [h, w, noc], BGR for 3."""
    w, h = C.c_int(), C.c_int()
    check(lib().ofdis_read_image(path.encode(), None, C.byref(w), C.byref(h), noc, 0), "read_image")
    out = np.empty((h.value, w.value, noc), np.uint8)
    check(lib().ofdis_read_image(path.encode(), out.ctypes.data, C.byref(w), C.byref(h), noc, out.size),
          "read_image")
    return out


def _ptr_list(arrs, n=32):
    out = (C.c_void_p * n)()
    keep = []
    for s, a in enumerate(arrs):
        if a is None:
            continue
        a = np.ascontiguousarray(a, _f32)
        keep.append(a)
        out[s] = a.ctypes.data
    return out, keep


class OFClass:
    """``OFC::OFClass`` (oflow.h:99-126): constructing it computes the flow into ``outflow``.

    Image/gradient arguments are sequences indexed by scale (entries below sc_l may be None); each
    entry is the padded (h_s + 2*imgpadding, w_s + 2*imgpadding[, noc]) float32 array.  ``outflow``
    (float32, (height>>sc_l)*(width>>sc_l)*nop elements, interleaved) is written in place.  Extra
    keyword-only ``mode`` selects SELECTMODE (1 flow, 2 depth); ``noc`` is SELECTCHANNEL.
    """

    def __init__(self, im_ao_in, im_ao_dx_in, im_ao_dy_in, im_bo_in, im_bo_dx_in, im_bo_dy_in,
                 imgpadding_in: int, outflow: np.ndarray, initflow: Optional[np.ndarray],
                 width_in: int, height_in: int, sc_f_in: int, sc_l_in: int, max_iter_in: int, min_iter_in: int,
                 dp_thresh_in: float, dr_thresh_in: float, res_thresh_in: float, p_samp_s_in: int, patove_in: float,
                 usefbcon_in: bool, costfct_in: int, noc_in: int, patnorm_in: int, usetvref_in: bool,
                 tv_alpha_in: float, tv_gamma_in: float, tv_delta_in: float, tv_innerit_in: int,
                 tv_solverit_in: int, tv_sor_in: float, verbosity_in: int, *, mode: int = MODE_OF):
        p = Params(mode=mode, noc=noc_in, sc_f=sc_f_in, sc_l=sc_l_in, max_iter=max_iter_in, min_iter=min_iter_in,
                   dp_thresh=dp_thresh_in, dr_thresh=dr_thresh_in, res_thresh=res_thresh_in, p_samp_s=p_samp_s_in,
                   patove=patove_in, usefbcon=int(bool(usefbcon_in)), costfct=costfct_in, patnorm=patnorm_in,
                   usetvref=int(bool(usetvref_in)), tv_alpha=tv_alpha_in, tv_gamma=tv_gamma_in,
                   tv_delta=tv_delta_in, tv_innerit=tv_innerit_in, tv_solverit=tv_solverit_in, tv_sor=tv_sor_in,
                   verbosity=verbosity_in)
        self.params = p
        if not (isinstance(outflow, np.ndarray) and outflow.dtype == _f32 and outflow.flags.c_contiguous):
            raise TypeError("outflow must be a C-contiguous float32 numpy array (written in place)")
        need = (width_in >> sc_l_in) * (height_in >> sc_l_in) * p.nop
        if outflow.size != need:
            raise ValueError(f"outflow has {outflow.size} elements, expected {need}")
        arrays = [_ptr_list(x) for x in (im_ao_in, im_ao_dx_in, im_ao_dy_in, im_bo_in, im_bo_dx_in, im_bo_dy_in)]
        init = None if initflow is None else np.ascontiguousarray(initflow, _f32)
        rc = lib().ofdis_oflow_compute(*[a[0] for a in arrays], imgpadding_in, outflow.ctypes.data,
                                       None if init is None else init.ctypes.data, width_in, height_in, C.byref(p))
        check(rc, "OFClass")


class Context:
    """One MI355X: batched u8 frame pairs -> full-resolution flow (``ofdis_run_batch_u8``)."""

    def __init__(self, device: int = 0):
        h = C.c_void_p()
        check(lib().ofdis_context_create(device, C.byref(h)), f"ofdis_context_create(device={device})")
        self._h = h
        self.device = device
        self._keep = []

    def close(self):
        if getattr(self, "_h", None):
            lib().ofdis_context_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run_ptr(self, a_ptr: int, b_ptr: int, n: int, width: int, height: int, p: Params, out_ptr: int,
                stream: int = 0, init_ptr: int = 0) -> None:
        """Device pointers in, device pointer out; asynchronous on `stream` (hipStream_t handle).
        init_ptr: optional device float [n, h, w, nop] initial flow (ofdis_run_batch_u8_init)."""
        check(lib().ofdis_run_batch_u8_init(self._h, a_ptr, b_ptr, init_ptr or None, n, width, height, C.byref(p),
                                            out_ptr, stream or None), "ofdis_run_batch_u8_init")

    def run_ptr_fmt(self, a_ptr: int, b_ptr: int, n: int, width: int, height: int, p: Params, fmt: OutFormat,
                    out_ptr: int, stream: int = 0, init_ptr: int = 0) -> None:
        """``ofdis_run_batch_u8_fmt`` on raw device pointers: run_ptr writing n * bytes_per_pair bytes (out_geometry)
        in the output format `fmt` (None: the plain format)."""
        check(lib().ofdis_run_batch_u8_fmt(self._h, a_ptr, b_ptr, init_ptr or None, n, width, height, C.byref(p),
                                           None if fmt is None else C.byref(fmt), out_ptr or None, stream or None),
              "ofdis_run_batch_u8_fmt")

    def run(self, a, b, p: Params, out=None, init=None, dtype=None, layout: str = "nhwc", grid: str = "full"):
        """torch.uint8 CUDA tensors [n, h, w] or [n, h, w, noc] -> torch.float32 [n, h, w, nop].
        init: optional float32 CUDA tensor [n, h, w, nop], the initial flow at full resolution.
        dtype (torch.float32, the default, or torch.float16), layout ("nhwc" or "nchw") and grid ("full", or "level":
        the finest level's 2^sc_l-pixel grid, see out_geometry) choose a compact output written by the kernels
        themselves: [n, H, W, nop] or [n, nop, H, W] of that dtype.  Values are in full-resolution pixels always."""
        import torch
        if dtype not in (None, torch.float32) or layout != "nhwc" or grid != "full":
            return self._run_fmt(a, b, p, out, init, out_format(dtype or torch.float32, layout, grid))
        if a.dim() == 3:
            a, b = a.unsqueeze(-1), b.unsqueeze(-1)
        n, h, w, noc = a.shape
        if noc != p.noc or a.dtype != torch.uint8 or not (a.is_cuda and b.is_cuda):
            raise ValueError("expected uint8 CUDA tensors with noc channels")
        a, b = a.contiguous(), b.contiguous()
        if out is None:
            out = torch.empty((n, h, w, p.nop), dtype=torch.float32, device=a.device)
        stream = torch.cuda.current_stream(a.device).cuda_stream
        if init is not None:
            if tuple(init.shape) != (n, h, w, p.nop) or init.dtype != torch.float32 or not init.is_cuda:
                raise ValueError("init must be a float32 CUDA tensor [n, h, w, nop]")
            init = init.contiguous()
        # stream 0 is torch's default (the legacy NULL stream): the C-ABI orders the call after the work queued
        # there (e.g. the copy kernels of .contiguous() above) and that stream's later work after the call
        self.run_ptr(a.data_ptr(), b.data_ptr(), n, w, h, p, out.data_ptr(), stream,
                     init.data_ptr() if init is not None else 0)
        return out

    def _run_fmt(self, a, b, p: Params, out, init, fmt: OutFormat):
        import torch
        if a.dim() == 3:
            a, b = a.unsqueeze(-1), b.unsqueeze(-1)
        n, h, w, noc = a.shape
        if noc != p.noc or a.dtype != torch.uint8 or not (a.is_cuda and b.is_cuda):
            raise ValueError("expected uint8 CUDA tensors with noc channels")
        a, b = a.contiguous(), b.contiguous()
        shape, tdt = _out_shape(p, w, h, n, init is not None, fmt), (torch.float16 if fmt.dtype else torch.float32)
        if out is None:
            out = torch.empty(shape, dtype=tdt, device=a.device)
        elif tuple(out.shape) != shape or out.dtype != tdt or not out.is_cuda or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {tdt} CUDA tensor {shape}")
        stream = torch.cuda.current_stream(a.device).cuda_stream
        if init is not None:
            if tuple(init.shape) != (n, h, w, p.nop) or init.dtype != torch.float32 or not init.is_cuda:
                raise ValueError("init must be a float32 CUDA tensor [n, h, w, nop]")
            init = init.contiguous()
        self.run_ptr_fmt(a.data_ptr(), b.data_ptr(), n, w, h, p, fmt, out.data_ptr(), stream,
                         init.data_ptr() if init is not None else 0)
        return out

    def run_host(self, a: np.ndarray, b: np.ndarray, p: Params, init: Optional[np.ndarray] = None, dtype=np.float32,
                 layout: str = "nhwc", grid: str = "full") -> np.ndarray:
        """numpy u8 [n,h,w,noc] (or a single [h,w,noc] pair) -> numpy float32 flow; synchronous.
        init: optional initial flow at full resolution, [n,h,w,nop] (or [h,w,nop] for a single pair).
        dtype (np.float32 or np.float16), layout and grid: the output format, as in ``run``."""
        single = a.ndim == 3
        a4 = np.ascontiguousarray(a[None] if single else a, np.uint8)
        b4 = np.ascontiguousarray(b[None] if single else b, np.uint8)
        n, h, w = a4.shape[:3]
        if np.dtype(dtype) != _f32 or layout != "nhwc" or grid != "full":
            fmt = out_format(np.dtype(dtype), layout, grid)
            out = np.empty(_out_shape(p, w, h, n, init is not None, fmt), np.float16 if fmt.dtype else _f32)
            i4 = None if init is None else np.ascontiguousarray(init, _f32).reshape(n, h, w, p.nop)
            check(lib().ofdis_run_batch_u8_fmt_host(self._h, a4.ctypes.data, b4.ctypes.data,
                                                    None if i4 is None else i4.ctypes.data, n, w, h, C.byref(p),
                                                    C.byref(fmt), out.ctypes.data), "ofdis_run_batch_u8_fmt_host")
            return out[0] if single else out
        out = np.empty((n, h, w, p.nop), _f32)
        i4 = None
        if init is not None:
            i4 = np.ascontiguousarray(init, _f32).reshape(n, h, w, p.nop)
        check(lib().ofdis_run_batch_u8_init_host(self._h, a4.ctypes.data, b4.ctypes.data,
                                                 None if i4 is None else i4.ctypes.data, n, w, h, C.byref(p),
                                                 out.ctypes.data), "ofdis_run_batch_u8_init_host")
        return out[0] if single else out

    def fb_check_ptr(self, fw_ptr: int, bw_ptr: int, n: int, width: int, height: int, alpha: float, beta: float,
                     occ_fw_ptr: int = 0, occ_bw_ptr: int = 0, err_fw_ptr: int = 0, err_bw_ptr: int = 0,
                     stream: int = 0) -> None:
        """``ofdis_fb_check`` on raw device pointers (0 = that output is not wanted)."""
        check(lib().ofdis_fb_check(self._h, fw_ptr or None, bw_ptr or None, n, width, height, alpha, beta,
                                   occ_fw_ptr or None, occ_bw_ptr or None, err_fw_ptr or None, err_bw_ptr or None,
                                   stream or None), "ofdis_fb_check")

    def fb_check_level_ptr(self, gfw_ptr: int, gbw_ptr: int, view: FlowView, n: int, width: int, height: int,
                           alpha: float, beta: float, occ_fw_ptr: int = 0, occ_bw_ptr: int = 0, err_fw_ptr: int = 0,
                           err_bw_ptr: int = 0, stream: int = 0) -> None:
        """``ofdis_fb_check_level`` on raw device pointers (0 = that output is not wanted): the check of the fields
        that the two float32 level grids described by `view` expand to."""
        check(lib().ofdis_fb_check_level(self._h, gfw_ptr or None, gbw_ptr or None,
                                         None if view is None else C.byref(view), n, width, height, alpha, beta,
                                         occ_fw_ptr or None, occ_bw_ptr or None, err_fw_ptr or None, err_bw_ptr or None,
                                         stream or None), "ofdis_fb_check_level")

    def fb_check(self, flow_fw, flow_bw, alpha: float = 0.01, beta: float = 0.5, want_err: bool = False,
                 grid: str = "full", p: Optional[Params] = None, size=None):
        """Forward-backward consistency of two flow fields: float32 CUDA tensors [n, h, w, 2] (or [h, w, 2]) ->
        (occ_fw, occ_bw[, err_fw, err_bw]); occ uint8 [n, h, w] with 0 consistent, 1 inconsistent, 2 the flow
        leaves the frame; err float32 [n, h, w], the squared round-trip error (+inf where occ is 2).
        grid="level": the two flows are the level grids of ``run(..., grid="level")`` with the parameters `p` for
        frames of size = (width, height); the result is that of the full-resolution flows, bit for bit, and neither of
        them is ever written."""
        import torch
        single = flow_fw.dim() == 3
        fw, bw = (flow_fw[None], flow_bw[None]) if single else (flow_fw, flow_bw)
        if (fw.dim() != 4 or fw.shape[-1] != 2 or fw.shape != bw.shape or fw.dtype != torch.float32
                or bw.dtype != torch.float32 or not (fw.is_cuda and bw.is_cuda)):
            raise ValueError("expected two float32 CUDA tensors [n, h, w, 2] of one shape")
        fw, bw = fw.contiguous(), bw.contiguous()
        if grid != "full":
            fmt = out_format(fw.dtype, "nhwc", grid)
            if p is None or size is None:
                raise OfdisError(ERR_INVALID_ARGUMENT, 'fb_check: grid="level" needs the parameters the flows were '
                                 "computed with and the frame size")
            w, h = int(size[0]), int(size[1])
            g = out_geometry(p, w, h, False, fw.dtype, "nhwc", grid)
            view = FlowView(fmt.dtype, fmt.layout, fmt.grid, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])
            n = fw.shape[0]
            if tuple(fw.shape) != (n, view.gh, view.gw, 2):
                raise ValueError(f"flows have shape {tuple(fw.shape)}, expected {(n, view.gh, view.gw, 2)}")
            occ = [torch.empty((n, h, w), dtype=torch.uint8, device=fw.device) for _ in range(2)]
            err = [torch.empty((n, h, w), dtype=torch.float32, device=fw.device) for _ in range(2 if want_err else 0)]
            self.fb_check_level_ptr(fw.data_ptr(), bw.data_ptr(), view, n, w, h, alpha, beta, occ[0].data_ptr(),
                                    occ[1].data_ptr(), err[0].data_ptr() if want_err else 0,
                                    err[1].data_ptr() if want_err else 0,
                                    torch.cuda.current_stream(fw.device).cuda_stream)
            out = tuple(occ + err)
            return tuple(t[0] for t in out) if single else out
        n, h, w = fw.shape[:3]
        occ = [torch.empty((n, h, w), dtype=torch.uint8, device=fw.device) for _ in range(2)]
        err = [torch.empty((n, h, w), dtype=torch.float32, device=fw.device) for _ in range(2 if want_err else 0)]
        stream = torch.cuda.current_stream(fw.device).cuda_stream
        self.fb_check_ptr(fw.data_ptr(), bw.data_ptr(), n, w, h, alpha, beta, occ[0].data_ptr(), occ[1].data_ptr(),
                          err[0].data_ptr() if want_err else 0, err[1].data_ptr() if want_err else 0, stream)
        out = tuple(occ + err)
        return tuple(t[0] for t in out) if single else out

    def run_bidir_ptr(self, a_ptr: int, b_ptr: int, n: int, width: int, height: int, p: Params, alpha: float,
                      beta: float, fw_ptr: int, bw_ptr: int = 0, occ_fw_ptr: int = 0, occ_bw_ptr: int = 0,
                      err_fw_ptr: int = 0, err_bw_ptr: int = 0, stream: int = 0) -> None:
        """``ofdis_run_bidir_u8`` on raw device pointers, asynchronous on `stream`; every output but the forward
        flow is optional (0)."""
        check(lib().ofdis_run_bidir_u8(self._h, a_ptr, b_ptr, n, width, height, C.byref(p), alpha, beta,
                                       fw_ptr or None, bw_ptr or None, occ_fw_ptr or None, occ_bw_ptr or None,
                                       err_fw_ptr or None, err_bw_ptr or None, stream or None), "ofdis_run_bidir_u8")

    def run_bidir(self, a, b, p: Params, alpha: float = 0.01, beta: float = 0.5, want_err: bool = False):
        """Both directions of each pair from one pyramid, and their consistency check: torch.uint8 CUDA tensors
        [n, h, w] or [n, h, w, noc] -> (flow_fw, flow_bw, occ_fw, occ_bw[, err_fw, err_bw]).  flow_fw is
        run(a, b), flow_bw is run(b, a), bit for bit; masks and errors as in fb_check.  Optical flow only."""
        import torch
        if a.dim() == 3:
            a, b = a.unsqueeze(-1), b.unsqueeze(-1)
        n, h, w, noc = a.shape
        if noc != p.noc or a.dtype != torch.uint8 or a.shape != b.shape or not (a.is_cuda and b.is_cuda):
            raise ValueError("expected uint8 CUDA tensors with noc channels")
        a, b = a.contiguous(), b.contiguous()
        flow = [torch.empty((n, h, w, 2), dtype=torch.float32, device=a.device) for _ in range(2)]
        occ = [torch.empty((n, h, w), dtype=torch.uint8, device=a.device) for _ in range(2)]
        err = [torch.empty((n, h, w), dtype=torch.float32, device=a.device) for _ in range(2 if want_err else 0)]
        stream = torch.cuda.current_stream(a.device).cuda_stream
        self.run_bidir_ptr(a.data_ptr(), b.data_ptr(), n, w, h, p, alpha, beta, flow[0].data_ptr(),
                           flow[1].data_ptr(), occ[0].data_ptr(), occ[1].data_ptr(),
                           err[0].data_ptr() if want_err else 0, err[1].data_ptr() if want_err else 0, stream)
        return tuple(flow + occ + err)

    def run_bidir_host(self, a: np.ndarray, b: np.ndarray, p: Params, alpha: float = 0.01, beta: float = 0.5,
                       want_err: bool = False):
        """run_bidir on numpy u8 [n,h,w,noc] (or a single [h,w,noc] pair); synchronous."""
        single = a.ndim == 3
        a4 = np.ascontiguousarray(a[None] if single else a, np.uint8)
        b4 = np.ascontiguousarray(b[None] if single else b, np.uint8)
        n, h, w = a4.shape[:3]
        flow = [np.empty((n, h, w, 2), _f32) for _ in range(2)]
        occ = [np.empty((n, h, w), np.uint8) for _ in range(2)]
        err = [np.empty((n, h, w), _f32) for _ in range(2 if want_err else 0)]
        check(lib().ofdis_run_bidir_u8_host(self._h, a4.ctypes.data, b4.ctypes.data, n, w, h, C.byref(p), alpha, beta,
                                            flow[0].ctypes.data, flow[1].ctypes.data, occ[0].ctypes.data,
                                            occ[1].ctypes.data, err[0].ctypes.data if want_err else None,
                                            err[1].ctypes.data if want_err else None), "ofdis_run_bidir_u8_host")
        out = tuple(flow + occ + err)
        return tuple(t[0] for t in out) if single else out

    def lr_check_ptr(self, l_ptr: int, r_ptr: int, n: int, width: int, height: int, alpha: float, beta: float,
                     occ_l_ptr: int = 0, occ_r_ptr: int = 0, err_l_ptr: int = 0, err_r_ptr: int = 0,
                     stream: int = 0) -> None:
        """``ofdis_lr_check`` on raw device pointers (0 = that output is not wanted)."""
        check(lib().ofdis_lr_check(self._h, l_ptr or None, r_ptr or None, n, width, height, alpha, beta,
                                   occ_l_ptr or None, occ_r_ptr or None, err_l_ptr or None, err_r_ptr or None,
                                   stream or None), "ofdis_lr_check")

    def lr_check(self, disp_l, disp_r, alpha: float = 0.01, beta: float = 0.5, want_err: bool = False):
        """Left-right consistency of two disparity fields: float32 CUDA tensors [n, h, w] (or [h, w]) ->
        (occ_l, occ_r[, err_l, err_r]); occ uint8 [n, h, w] with 0 consistent, 1 inconsistent, 2 the disparity
        leaves the frame; err float32 [n, h, w], the squared round-trip error (+inf where occ is 2)."""
        import torch
        single = disp_l.dim() == 2
        dl, dr = (disp_l[None], disp_r[None]) if single else (disp_l, disp_r)
        if (dl.dim() != 3 or dl.shape != dr.shape or dl.dtype != torch.float32 or dr.dtype != torch.float32
                or not (dl.is_cuda and dr.is_cuda)):
            raise ValueError("expected two float32 CUDA tensors [n, h, w] of one shape")
        dl, dr = dl.contiguous(), dr.contiguous()
        n, h, w = dl.shape
        occ = [torch.empty((n, h, w), dtype=torch.uint8, device=dl.device) for _ in range(2)]
        err = [torch.empty((n, h, w), dtype=torch.float32, device=dl.device) for _ in range(2 if want_err else 0)]
        stream = torch.cuda.current_stream(dl.device).cuda_stream
        self.lr_check_ptr(dl.data_ptr(), dr.data_ptr(), n, w, h, alpha, beta, occ[0].data_ptr(), occ[1].data_ptr(),
                          err[0].data_ptr() if want_err else 0, err[1].data_ptr() if want_err else 0, stream)
        out = tuple(occ + err)
        return tuple(t[0] for t in out) if single else out

    def run_stereo_ptr(self, l_ptr: int, r_ptr: int, n: int, width: int, height: int, p: Params, alpha: float,
                       beta: float, disp_l_ptr: int, disp_r_ptr: int = 0, occ_l_ptr: int = 0, occ_r_ptr: int = 0,
                       err_l_ptr: int = 0, err_r_ptr: int = 0, stream: int = 0) -> None:
        """``ofdis_run_stereo_u8`` on raw device pointers, asynchronous on `stream`; every output but the left
        view's disparity is optional (0)."""
        check(lib().ofdis_run_stereo_u8(self._h, l_ptr, r_ptr, n, width, height, C.byref(p), alpha, beta,
                                        disp_l_ptr or None, disp_r_ptr or None, occ_l_ptr or None, occ_r_ptr or None,
                                        err_l_ptr or None, err_r_ptr or None, stream or None), "ofdis_run_stereo_u8")

    def run_stereo(self, left, right, p: Params, alpha: float = 0.01, beta: float = 0.5, want_err: bool = False):
        """Both views' disparities of each rectified pair from one batch, and their left-right check: torch.uint8
        CUDA tensors [n, h, w] or [n, h, w, noc] -> (disp_l, disp_r, occ_l, occ_r[, err_l, err_r]).  disp_l is
        run(left, right) (values <= 0); disp_r is the right view's disparity in its own coordinates (values >= 0):
        -run(flip(right), flip(left)) flipped back, bit for bit; masks and errors as in lr_check.  Depth only."""
        import torch
        if left.dim() == 3:
            left, right = left.unsqueeze(-1), right.unsqueeze(-1)
        n, h, w, noc = left.shape
        if (noc != p.noc or left.dtype != torch.uint8 or left.shape != right.shape
                or not (left.is_cuda and right.is_cuda)):
            raise ValueError("expected uint8 CUDA tensors with noc channels")
        left, right = left.contiguous(), right.contiguous()
        disp = [torch.empty((n, h, w), dtype=torch.float32, device=left.device) for _ in range(2)]
        occ = [torch.empty((n, h, w), dtype=torch.uint8, device=left.device) for _ in range(2)]
        err = [torch.empty((n, h, w), dtype=torch.float32, device=left.device) for _ in range(2 if want_err else 0)]
        stream = torch.cuda.current_stream(left.device).cuda_stream
        self.run_stereo_ptr(left.data_ptr(), right.data_ptr(), n, w, h, p, alpha, beta, disp[0].data_ptr(),
                            disp[1].data_ptr(), occ[0].data_ptr(), occ[1].data_ptr(),
                            err[0].data_ptr() if want_err else 0, err[1].data_ptr() if want_err else 0, stream)
        return tuple(disp + occ + err)

    def run_stereo_host(self, left: np.ndarray, right: np.ndarray, p: Params, alpha: float = 0.01, beta: float = 0.5,
                        want_err: bool = False):
        """run_stereo on numpy u8 [n,h,w,noc] (or a single [h,w,noc] pair); synchronous."""
        single = left.ndim == 3
        l4 = np.ascontiguousarray(left[None] if single else left, np.uint8)
        r4 = np.ascontiguousarray(right[None] if single else right, np.uint8)
        n, h, w = l4.shape[:3]
        disp = [np.empty((n, h, w), _f32) for _ in range(2)]
        occ = [np.empty((n, h, w), np.uint8) for _ in range(2)]
        err = [np.empty((n, h, w), _f32) for _ in range(2 if want_err else 0)]
        check(lib().ofdis_run_stereo_u8_host(self._h, l4.ctypes.data, r4.ctypes.data, n, w, h, C.byref(p), alpha, beta,
                                             disp[0].ctypes.data, disp[1].ctypes.data, occ[0].ctypes.data,
                                             occ[1].ctypes.data, err[0].ctypes.data if want_err else None,
                                             err[1].ctypes.data if want_err else None), "ofdis_run_stereo_u8_host")
        out = tuple(disp + occ + err)
        return tuple(t[0] for t in out) if single else out

    def run_sequence_ptr(self, frames_ptr: int, nframes: int, stride: int, width: int, height: int, p: Params,
                         fw_ptr: int, init_ptr: int = 0, alpha: float = 0.01, beta: float = 0.5, bw_ptr: int = 0,
                         occ_fw_ptr: int = 0, occ_bw_ptr: int = 0, err_fw_ptr: int = 0, err_bw_ptr: int = 0,
                         stream: int = 0) -> None:
        """``ofdis_run_sequence_u8`` on raw device pointers, asynchronous on `stream`: frames u8
        [nframes, h, w, noc], pair i = (frame i, frame i + stride), outputs for nframes - stride pairs; every output
        but the forward flow is optional (0), and so is the initial flow."""
        check(lib().ofdis_run_sequence_u8(self._h, frames_ptr, nframes, stride, init_ptr or None, width, height,
                                          C.byref(p), alpha, beta, fw_ptr or None, bw_ptr or None, occ_fw_ptr or None,
                                          occ_bw_ptr or None, err_fw_ptr or None, err_bw_ptr or None, stream or None),
              "ofdis_run_sequence_u8")

    def run_sequence(self, frames, p: Params, stride: int = 1, init=None, bidir: bool = False, alpha: float = 0.01,
                     beta: float = 0.5, want_err: bool = False, dtype=None, layout: str = "nhwc", grid: str = "full"):
        """Flow along a video: torch.uint8 CUDA tensor [T, h, w] or [T, h, w, noc] -> the flow of the T - stride pairs
        (frame i, frame i + stride), bit for bit ``run(frames[:-stride], frames[stride:])`` with every frame's
        pyramid built once.  Returns the flow [T - stride, h, w, 2]; with ``bidir`` the tuple of ``run_bidir``
        (flow_fw, flow_bw, occ_fw, occ_bw[, err_fw, err_bw]).  init: optional float32 CUDA tensor
        [T - stride, h, w, 2] as in ``run`` (not together with ``bidir``).  Optical flow only.
        dtype, layout, grid: the forward flow's output format, as in ``run`` (not together with ``bidir``: the
        backward flow, masks and errors are float32 fields)."""
        import torch
        fmt = None
        if dtype not in (None, torch.float32) or layout != "nhwc" or grid != "full":
            fmt = out_format(dtype or torch.float32, layout, grid)
            if bidir:
                raise OfdisError(ERR_UNSUPPORTED, "run_sequence: bidir with an output format")
        if frames.dim() == 3:
            frames = frames.unsqueeze(-1)
        t, h, w, noc = frames.shape
        if noc != p.noc or frames.dtype != torch.uint8 or not frames.is_cuda:
            raise ValueError("expected a uint8 CUDA tensor with noc channels")
        n = t - stride
        if stride < 1 or n < 1:
            raise ValueError("a sequence needs stride >= 1 and more than `stride` frames")
        frames = frames.contiguous()
        if init is not None:
            if tuple(init.shape) != (n, h, w, 2) or init.dtype != torch.float32 or not init.is_cuda:
                raise ValueError("init must be a float32 CUDA tensor [T - stride, h, w, 2]")
            init = init.contiguous()
        if fmt is not None:
            out = torch.empty(_out_shape(p, w, h, n, init is not None, fmt),
                              dtype=torch.float16 if fmt.dtype else torch.float32, device=frames.device)
            check(lib().ofdis_run_sequence_u8_fmt(self._h, frames.data_ptr(), t, stride,
                                                  init.data_ptr() if init is not None else None, w, h, C.byref(p),
                                                  C.byref(fmt), out.data_ptr(),
                                                  torch.cuda.current_stream(frames.device).cuda_stream or None),
                  "ofdis_run_sequence_u8_fmt")
            return out
        flow = [torch.empty((n, h, w, 2), dtype=torch.float32, device=frames.device) for _ in range(2 if bidir else 1)]
        occ = [torch.empty((n, h, w), dtype=torch.uint8, device=frames.device) for _ in range(2 if bidir else 0)]
        err = [torch.empty((n, h, w), dtype=torch.float32, device=frames.device)
               for _ in range(2 if bidir and want_err else 0)]
        stream = torch.cuda.current_stream(frames.device).cuda_stream
        self.run_sequence_ptr(frames.data_ptr(), t, stride, w, h, p, flow[0].data_ptr(),
                              init.data_ptr() if init is not None else 0, alpha, beta,
                              flow[1].data_ptr() if bidir else 0, occ[0].data_ptr() if bidir else 0,
                              occ[1].data_ptr() if bidir else 0, err[0].data_ptr() if err else 0,
                              err[1].data_ptr() if err else 0, stream)
        return tuple(flow + occ + err) if bidir else flow[0]

    def run_sequence_host(self, frames: np.ndarray, p: Params, stride: int = 1, init: Optional[np.ndarray] = None,
                          bidir: bool = False, alpha: float = 0.01, beta: float = 0.5, want_err: bool = False,
                          dtype=np.float32, layout: str = "nhwc", grid: str = "full"):
        """run_sequence on a numpy u8 array [T, h, w] or [T, h, w, noc]; synchronous."""
        fmt = None
        if np.dtype(dtype) != _f32 or layout != "nhwc" or grid != "full":
            fmt = out_format(np.dtype(dtype), layout, grid)
            if bidir:
                raise OfdisError(ERR_UNSUPPORTED, "run_sequence_host: bidir with an output format")
        f4 = np.ascontiguousarray(frames[..., None] if frames.ndim == 3 else frames, np.uint8)
        t, h, w = f4.shape[:3]
        n = t - stride
        if stride < 1 or n < 1:
            raise ValueError("a sequence needs stride >= 1 and more than `stride` frames")
        i4 = None if init is None else np.ascontiguousarray(init, _f32).reshape(n, h, w, 2)
        if fmt is not None:
            out = np.empty(_out_shape(p, w, h, n, init is not None, fmt), np.float16 if fmt.dtype else _f32)
            check(lib().ofdis_run_sequence_u8_fmt_host(self._h, f4.ctypes.data, t, stride,
                                                       None if i4 is None else i4.ctypes.data, w, h, C.byref(p),
                                                       C.byref(fmt), out.ctypes.data), "ofdis_run_sequence_u8_fmt_host")
            return out
        flow = [np.empty((n, h, w, 2), _f32) for _ in range(2 if bidir else 1)]
        occ = [np.empty((n, h, w), np.uint8) for _ in range(2 if bidir else 0)]
        err = [np.empty((n, h, w), _f32) for _ in range(2 if bidir and want_err else 0)]
        check(lib().ofdis_run_sequence_u8_host(self._h, f4.ctypes.data, t, stride,
                                               None if i4 is None else i4.ctypes.data, w, h, C.byref(p), alpha, beta,
                                               flow[0].ctypes.data, flow[1].ctypes.data if bidir else None,
                                               occ[0].ctypes.data if bidir else None,
                                               occ[1].ctypes.data if bidir else None,
                                               err[0].ctypes.data if err else None,
                                               err[1].ctypes.data if err else None), "ofdis_run_sequence_u8_host")
        return tuple(flow + occ + err) if bidir else flow[0]

    def warp_ptr(self, img_ptr: int, flow_ptr: int, view: FlowView, n: int, width: int, height: int, noc: int,
                 scale: float, out_dtype: int, out_ptr: int, valid_ptr: int = 0, stream: int = 0) -> None:
        """``ofdis_warp_u8`` on raw device pointers (valid_ptr 0: no mask); out_dtype IMG_U8 / IMG_F32."""
        check(lib().ofdis_warp_u8(self._h, img_ptr or None, flow_ptr or None, C.byref(view), n, width, height, noc,
                                  scale, out_dtype, out_ptr or None, valid_ptr or None, stream or None),
              "ofdis_warp_u8")

    def warp(self, img, flow, scale: float = 1.0, out_dtype=None, layout: str = "nhwc", grid: str = "full",
             p: Optional[Params] = None, want_valid: bool = False):
        """Backward warp of u8 frames along a flow: torch.uint8 CUDA tensor [n, h, w] or [n, h, w, 3] read at
        (x + scale u, y + scale v) with bilinear taps and a replicated border (the definition is in ofdis.h) ->
        the picture in the image's shape, torch.uint8 (the default) or torch.float32; with want_valid the tuple
        (picture, valid uint8 [n, h, w], 0 where the position left the frame).
        flow: any output of ``run`` -- float32 or float16 (read from the tensor), layout "nhwc" / "nchw", grid "full"
        ([n, h, w, 2] / [n, 2, h, w]) or "level" (the level grid of ``run(..., grid="level")``; needs the same `p`, and
        gives the picture of the full-resolution flow bit for bit without that flow ever existing)."""
        import torch
        gray = img.dim() == 3
        im = img.unsqueeze(-1) if gray else img
        if im.dim() != 4 or im.shape[-1] not in (1, 3) or im.dtype != torch.uint8 or not (im.is_cuda and flow.is_cuda):
            raise ValueError("expected a uint8 CUDA tensor [n, h, w] or [n, h, w, 3] and a CUDA flow tensor")
        n, h, w, noc = im.shape
        fmt = out_format(flow.dtype, layout, grid)
        view = FlowView(fmt.dtype, fmt.layout, fmt.grid, w, h, 1, 0, 0)
        if grid == "level":
            if p is None:
                raise OfdisError(ERR_INVALID_ARGUMENT, 'warp: grid="level" needs the parameters the flow was computed with')
            g = out_geometry(p, w, h, False, flow.dtype, layout, grid)
            view = FlowView(fmt.dtype, fmt.layout, fmt.grid, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])
        want = (n, 2, view.gh, view.gw) if fmt.layout else (n, view.gh, view.gw, 2)
        if tuple(flow.shape) != want:
            raise ValueError(f"flow has shape {tuple(flow.shape)}, expected {want}")
        if out_dtype not in (None, torch.uint8, torch.float32):
            raise OfdisError(ERR_INVALID_ARGUMENT, f"warp: out_dtype {out_dtype!r}")
        f32 = out_dtype == torch.float32
        im, flow = im.contiguous(), flow.contiguous()
        out = torch.empty(img.shape, dtype=torch.float32 if f32 else torch.uint8, device=im.device)
        valid = torch.empty((n, h, w), dtype=torch.uint8, device=im.device) if want_valid else None
        self.warp_ptr(im.data_ptr(), flow.data_ptr(), view, n, w, h, noc, float(scale), IMG_F32 if f32 else IMG_U8,
                      out.data_ptr(), valid.data_ptr() if want_valid else 0,
                      torch.cuda.current_stream(im.device).cuda_stream)
        return (out, valid) if want_valid else out

    def run_warp_ptr(self, a_ptr: int, b_ptr: int, n: int, width: int, height: int, p: Params, scale: float,
                     out_dtype: int, out_ptr: int, valid_ptr: int = 0, stream: int = 0) -> None:
        """``ofdis_run_warp_u8`` on raw device pointers, asynchronous on `stream` (valid_ptr 0: no mask)."""
        check(lib().ofdis_run_warp_u8(self._h, a_ptr or None, b_ptr or None, n, width, height, C.byref(p), scale,
                                      out_dtype, out_ptr or None, valid_ptr or None, stream or None),
              "ofdis_run_warp_u8")

    def run_warp(self, a, b, p: Params, scale: float = 1.0, out_dtype=None, want_valid: bool = False):
        """Motion compensation in one call: the flow a -> b of each pair, then b warped by it -- at scale 1, frame b
        pulled back onto frame a.  torch.uint8 CUDA tensors [n, h, w] or [n, h, w, 3] -> the picture in that shape
        (torch.uint8, or torch.float32), with want_valid the tuple (picture, valid).  Bit for bit
        ``warp(b, run(a, b, p), scale)``, but the flow stays on its level grid: no full-resolution flow is written."""
        import torch
        a4, b4 = (a.unsqueeze(-1), b.unsqueeze(-1)) if a.dim() == 3 else (a, b)
        if (a4.dim() != 4 or a4.shape[-1] != p.noc or a4.dtype != torch.uint8 or a.shape != b.shape
                or b.dtype != torch.uint8 or not (a.is_cuda and b.is_cuda)):
            raise ValueError("expected two uint8 CUDA tensors of one shape with noc channels")
        if out_dtype not in (None, torch.uint8, torch.float32):
            raise OfdisError(ERR_INVALID_ARGUMENT, f"run_warp: out_dtype {out_dtype!r}")
        f32 = out_dtype == torch.float32
        n, h, w, _ = a4.shape
        a4, b4 = a4.contiguous(), b4.contiguous()
        out = torch.empty(a.shape, dtype=torch.float32 if f32 else torch.uint8, device=a.device)
        valid = torch.empty((n, h, w), dtype=torch.uint8, device=a.device) if want_valid else None
        self.run_warp_ptr(a4.data_ptr(), b4.data_ptr(), n, w, h, p, float(scale), IMG_F32 if f32 else IMG_U8,
                          out.data_ptr(), valid.data_ptr() if want_valid else 0,
                          torch.cuda.current_stream(a.device).cuda_stream)
        return (out, valid) if want_valid else out

    def run_warp_host(self, a: np.ndarray, b: np.ndarray, p: Params, scale: float = 1.0, out_dtype=np.uint8,
                      want_valid: bool = False):
        """run_warp on numpy u8 arrays; synchronous.  Colour: [n, h, w, 3] or a single pair [h, w, 3]; gray:
        [n, h, w, 1], [n, h, w], or a single pair [h, w, 1] (as synth_pair returns it) or [h, w].  The picture has the
        input's shape; valid is [n, h, w] ([h, w] for a single pair)."""
        if np.dtype(out_dtype) not in (np.dtype(np.uint8), np.dtype(_f32)):
            raise OfdisError(ERR_INVALID_ARGUMENT, f"run_warp_host: out_dtype {out_dtype!r}")
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        if a.shape != b.shape or a.ndim < 2 or a.ndim > 4:
            raise ValueError("expected two uint8 arrays of one shape")
        channels = a.ndim == 4 or (a.ndim == 3 and a.shape[-1] == p.noc and (p.noc == 3 or a.shape[-1] == 1))
        if channels and a.shape[-1] != p.noc:
            raise ValueError("expected noc channels")
        h, w = a.shape[-3:-1] if channels else a.shape[-2:]
        single = a.ndim == (3 if channels else 2)
        n = 1 if single else a.shape[0]
        out = np.empty(a.shape, out_dtype)
        valid = np.empty((h, w) if single else (n, h, w), np.uint8) if want_valid else None
        check(lib().ofdis_run_warp_u8_host(self._h, a.ctypes.data, b.ctypes.data, n, w, h, C.byref(p), float(scale),
                                           IMG_F32 if np.dtype(out_dtype) == _f32 else IMG_U8, out.ctypes.data,
                                           valid.ctypes.data if want_valid else None), "ofdis_run_warp_u8_host")
        return (out, valid) if want_valid else out

    def interp_ptr(self, a_ptr: int, b_ptr: int, fw_ptr: int, bw_ptr: int, view: FlowView, n: int, width: int,
                   height: int, noc: int, t, out_dtype: int, out_ptr: int, valid_ptr: int = 0, occ_a_ptr: int = 0,
                   occ_b_ptr: int = 0, stream: int = 0) -> None:
        """``ofdis_interp_u8`` on raw device pointers (0: no mask output / no occlusion mask); t a scalar or a sequence
        of times; out_dtype IMG_U8 / IMG_F32."""
        tt = _times(t)
        check(lib().ofdis_interp_u8(self._h, a_ptr or None, b_ptr or None, fw_ptr or None, bw_ptr or None,
                                    C.byref(view), n, width, height, noc, tt.ctypes.data, tt.size, occ_a_ptr or None,
                                    occ_b_ptr or None, out_dtype, out_ptr or None, valid_ptr or None, stream or None),
              "ofdis_interp_u8")

    def interp(self, a, b, flow_fw, flow_bw, t=0.5, occ_fw=None, occ_bw=None, out_dtype=None, layout: str = "nhwc",
               grid: str = "full", p: Optional[Params] = None, want_valid: bool = False):
        """The frames between a and b at the times t (a scalar or a sequence of at most INTERP_MAX_T values in [0, 1])
        from the pair's two flows (the definition is in ofdis.h): torch.uint8 CUDA tensors [n, h, w] or [n, h, w, 3] ->
        [n, nt, h, w] or [n, nt, h, w, 3], torch.uint8 (the default) or torch.float32; with want_valid the tuple
        (pictures, valid uint8 [n, nt, h, w]: 3 both frames, 1 frame a only, 2 frame b only, 0 neither).
        flow_fw (a -> b) and flow_bw (b -> a): two outputs of ``run`` / ``run_bidir`` in one format, described as for
        ``warp`` (dtype from the tensors, layout, grid; grid "level" needs `p`).  occ_fw / occ_bw: the occlusion masks
        of ``run_bidir`` / ``fb_check`` ([n, h, w] uint8); a pixel that samples a marked position of one frame takes the
        other frame alone."""
        import torch
        gray = a.dim() == 3
        a4, b4 = (a.unsqueeze(-1), b.unsqueeze(-1)) if gray else (a, b)
        if (a4.dim() != 4 or a4.shape[-1] not in (1, 3) or a4.dtype != torch.uint8 or a.shape != b.shape
                or b.dtype != torch.uint8 or not (a.is_cuda and b.is_cuda and flow_fw.is_cuda and flow_bw.is_cuda)):
            raise ValueError("expected two uint8 CUDA tensors [n, h, w] or [n, h, w, 3] of one shape and two CUDA flow tensors")
        n, h, w, noc = a4.shape
        if flow_fw.dtype != flow_bw.dtype:
            raise ValueError("the two flows must have one dtype")
        fmt = out_format(flow_fw.dtype, layout, grid)
        view = FlowView(fmt.dtype, fmt.layout, fmt.grid, w, h, 1, 0, 0)
        if grid == "level":
            if p is None:
                raise OfdisError(ERR_INVALID_ARGUMENT, 'interp: grid="level" needs the parameters the flows were computed with')
            g = out_geometry(p, w, h, False, flow_fw.dtype, layout, grid)
            view = FlowView(fmt.dtype, fmt.layout, fmt.grid, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])
        want = (n, 2, view.gh, view.gw) if fmt.layout else (n, view.gh, view.gw, 2)
        if tuple(flow_fw.shape) != want or tuple(flow_bw.shape) != want:
            raise ValueError(f"flows have shapes {tuple(flow_fw.shape)} and {tuple(flow_bw.shape)}, expected {want}")
        for occ in (occ_fw, occ_bw):
            if occ is not None and (tuple(occ.shape) != (n, h, w) or occ.dtype != torch.uint8 or not occ.is_cuda):
                raise ValueError(f"expected uint8 CUDA occlusion masks of shape {(n, h, w)}")
        if out_dtype not in (None, torch.uint8, torch.float32):
            raise OfdisError(ERR_INVALID_ARGUMENT, f"interp: out_dtype {out_dtype!r}")
        f32 = out_dtype == torch.float32
        tt = _times(t)
        a4, b4, flow_fw, flow_bw = a4.contiguous(), b4.contiguous(), flow_fw.contiguous(), flow_bw.contiguous()
        occ_fw = occ_fw.contiguous() if occ_fw is not None else None
        occ_bw = occ_bw.contiguous() if occ_bw is not None else None
        shape = (n, tt.size, h, w) if gray else (n, tt.size, h, w, 3)
        out = torch.empty(shape, dtype=torch.float32 if f32 else torch.uint8, device=a.device)
        valid = torch.empty((n, tt.size, h, w), dtype=torch.uint8, device=a.device) if want_valid else None
        self.interp_ptr(a4.data_ptr(), b4.data_ptr(), flow_fw.data_ptr(), flow_bw.data_ptr(), view, n, w, h, noc, tt,
                        IMG_F32 if f32 else IMG_U8, out.data_ptr(), valid.data_ptr() if want_valid else 0,
                        occ_fw.data_ptr() if occ_fw is not None else 0, occ_bw.data_ptr() if occ_bw is not None else 0,
                        torch.cuda.current_stream(a.device).cuda_stream)
        return (out, valid) if want_valid else out

    def run_interp_ptr(self, a_ptr: int, b_ptr: int, n: int, width: int, height: int, p: Params, t, out_dtype: int,
                       out_ptr: int, valid_ptr: int = 0, stream: int = 0) -> None:
        """``ofdis_run_interp_u8`` on raw device pointers, asynchronous on `stream` (valid_ptr 0: no mask)."""
        tt = _times(t)
        check(lib().ofdis_run_interp_u8(self._h, a_ptr or None, b_ptr or None, n, width, height, C.byref(p),
                                        tt.ctypes.data, tt.size, out_dtype, out_ptr or None, valid_ptr or None,
                                        stream or None), "ofdis_run_interp_u8")

    def run_interp_occ_ptr(self, a_ptr: int, b_ptr: int, n: int, width: int, height: int, p: Params, t, alpha: float,
                           beta: float, out_dtype: int, out_ptr: int, valid_ptr: int = 0, occ_fw_ptr: int = 0,
                           occ_bw_ptr: int = 0, stream: int = 0) -> None:
        """``ofdis_run_interp_occ_u8`` on raw device pointers, asynchronous on `stream` (0: that output is not
        wanted)."""
        tt = _times(t)
        check(lib().ofdis_run_interp_occ_u8(self._h, a_ptr or None, b_ptr or None, n, width, height, C.byref(p),
                                            tt.ctypes.data, tt.size, alpha, beta, out_dtype, out_ptr or None,
                                            valid_ptr or None, occ_fw_ptr or None, occ_bw_ptr or None, stream or None),
              "ofdis_run_interp_occ_u8")

    def run_interp(self, a, b, p: Params, t=0.5, out_dtype=None, want_valid: bool = False, occ: bool = False,
                   alpha: float = 0.01, beta: float = 0.5, want_occ: bool = False):
        """Frame interpolation in one call: both flows of each pair from one pyramid, then the frames at the times t.
        torch.uint8 CUDA tensors [n, h, w] or [n, h, w, 3] -> [n, nt, h, w] or [n, nt, h, w, 3] (torch.uint8, or
        torch.float32), with want_valid the tuple (pictures, valid [n, nt, h, w]).  Bit for bit
        ``interp(a, b, *run_bidir(a, b, p)[:2], t)``, but both flows stay on their level grids: no full-resolution
        flow is written.
        occ: with the pair's occlusion masks at the thresholds alpha / beta, computed from the level grids -- bit for
        bit ``interp(a, b, fw, bw, t, occ_fw, occ_bw)`` on the four outputs of ``run_bidir(a, b, p, alpha, beta)``;
        want_occ appends (occ_fw, occ_bw), ``run_bidir``'s masks, to the result."""
        import torch
        if want_occ and not occ:
            raise ValueError("want_occ needs occ=True")
        gray = a.dim() == 3
        a4, b4 = (a.unsqueeze(-1), b.unsqueeze(-1)) if gray else (a, b)
        if (a4.dim() != 4 or a4.shape[-1] != p.noc or a4.dtype != torch.uint8 or a.shape != b.shape
                or b.dtype != torch.uint8 or not (a.is_cuda and b.is_cuda)):
            raise ValueError("expected two uint8 CUDA tensors of one shape with noc channels")
        if out_dtype not in (None, torch.uint8, torch.float32):
            raise OfdisError(ERR_INVALID_ARGUMENT, f"run_interp: out_dtype {out_dtype!r}")
        f32 = out_dtype == torch.float32
        tt = _times(t)
        n, h, w, _ = a4.shape
        a4, b4 = a4.contiguous(), b4.contiguous()
        shape = (n, tt.size, h, w) if gray else (n, tt.size, h, w, 3)
        out = torch.empty(shape, dtype=torch.float32 if f32 else torch.uint8, device=a.device)
        valid = torch.empty((n, tt.size, h, w), dtype=torch.uint8, device=a.device) if want_valid else None
        if occ:
            masks = [torch.empty((n, h, w), dtype=torch.uint8, device=a.device) for _ in range(2 if want_occ else 0)]
            self.run_interp_occ_ptr(a4.data_ptr(), b4.data_ptr(), n, w, h, p, tt, alpha, beta,
                                    IMG_F32 if f32 else IMG_U8, out.data_ptr(), valid.data_ptr() if want_valid else 0,
                                    masks[0].data_ptr() if want_occ else 0, masks[1].data_ptr() if want_occ else 0,
                                    torch.cuda.current_stream(a.device).cuda_stream)
            res = [out] + ([valid] if want_valid else []) + masks
            return tuple(res) if len(res) > 1 else out
        self.run_interp_ptr(a4.data_ptr(), b4.data_ptr(), n, w, h, p, tt, IMG_F32 if f32 else IMG_U8, out.data_ptr(),
                            valid.data_ptr() if want_valid else 0, torch.cuda.current_stream(a.device).cuda_stream)
        return (out, valid) if want_valid else out

    def run_interp_host(self, a: np.ndarray, b: np.ndarray, p: Params, t=0.5, out_dtype=np.uint8,
                        want_valid: bool = False, occ: bool = False, alpha: float = 0.01, beta: float = 0.5,
                        want_occ: bool = False):
        """run_interp on numpy u8 arrays; synchronous.  The inputs as for ``run_warp_host``; the pictures have the
        input's shape with an axis of nt times in front of the frame axes ([n, nt, h, w(, c)]; [nt, h, w(, c)] for a
        single pair), valid is [n, nt, h, w] ([nt, h, w]), the masks of want_occ [n, h, w] ([h, w])."""
        if want_occ and not occ:
            raise ValueError("want_occ needs occ=True")
        if np.dtype(out_dtype) not in (np.dtype(np.uint8), np.dtype(_f32)):
            raise OfdisError(ERR_INVALID_ARGUMENT, f"run_interp_host: out_dtype {out_dtype!r}")
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        if a.shape != b.shape or a.ndim < 2 or a.ndim > 4:
            raise ValueError("expected two uint8 arrays of one shape")
        channels = a.ndim == 4 or (a.ndim == 3 and a.shape[-1] == p.noc and (p.noc == 3 or a.shape[-1] == 1))
        if channels and a.shape[-1] != p.noc:
            raise ValueError("expected noc channels")
        h, w = a.shape[-3:-1] if channels else a.shape[-2:]
        single = a.ndim == (3 if channels else 2)
        n = 1 if single else a.shape[0]
        tt = _times(t)
        lead = () if single else (n,)
        out = np.empty(lead + (tt.size,) + a.shape[a.ndim - (3 if channels else 2):], out_dtype)
        valid = np.empty(lead + (tt.size, h, w), np.uint8) if want_valid else None
        if occ:
            masks = [np.empty(lead + (h, w), np.uint8) for _ in range(2 if want_occ else 0)]
            check(lib().ofdis_run_interp_occ_u8_host(self._h, a.ctypes.data, b.ctypes.data, n, w, h, C.byref(p),
                                                     tt.ctypes.data, tt.size, alpha, beta,
                                                     IMG_F32 if np.dtype(out_dtype) == _f32 else IMG_U8, out.ctypes.data,
                                                     valid.ctypes.data if want_valid else None,
                                                     masks[0].ctypes.data if want_occ else None,
                                                     masks[1].ctypes.data if want_occ else None),
                  "ofdis_run_interp_occ_u8_host")
            res = [out] + ([valid] if want_valid else []) + masks
            return tuple(res) if len(res) > 1 else out
        check(lib().ofdis_run_interp_u8_host(self._h, a.ctypes.data, b.ctypes.data, n, w, h, C.byref(p), tt.ctypes.data,
                                             tt.size, IMG_F32 if np.dtype(out_dtype) == _f32 else IMG_U8,
                                             out.ctypes.data, valid.ctypes.data if want_valid else None),
              "ofdis_run_interp_u8_host")
        return (out, valid) if want_valid else out

    def run_sequence_interp_ptr(self, frames_ptr: int, nframes: int, stride: int, width: int, height: int, p: Params,
                                t, out_dtype: int, out_ptr: int, valid_ptr: int = 0, occ: bool = False,
                                alpha: float = 0.01, beta: float = 0.5, occ_fw_ptr: int = 0, occ_bw_ptr: int = 0,
                                stream: int = 0) -> None:
        """``ofdis_run_sequence_interp_u8`` on raw device pointers, asynchronous on `stream`: frames u8
        [nframes, h, w, noc], pair i = (frame i, frame i + stride), pictures for nframes - stride pairs (0: that
        output is not wanted)."""
        tt = _times(t)
        check(lib().ofdis_run_sequence_interp_u8(self._h, frames_ptr or None, nframes, stride, width, height,
                                                 C.byref(p), tt.ctypes.data, tt.size, int(bool(occ)), alpha, beta,
                                                 out_dtype, out_ptr or None, valid_ptr or None, occ_fw_ptr or None,
                                                 occ_bw_ptr or None, stream or None), "ofdis_run_sequence_interp_u8")

    def run_sequence_interp(self, frames, p: Params, t=0.5, stride: int = 1, out_dtype=None, want_valid: bool = False,
                            occ: bool = False, alpha: float = 0.01, beta: float = 0.5, want_occ: bool = False):
        """The frames between the frames of a video: torch.uint8 CUDA tensor [T, h, w] or [T, h, w, 3] -> the pictures
        of the T - stride pairs (frame i, frame i + stride), [T - stride, nt, h, w(, 3)] -- bit for bit
        ``run_interp(frames[:-stride], frames[stride:], p, t, ...)`` with the same options, every frame's pyramid
        built once.  The result is ordered as ``run_interp``'s: pictures[, valid][, occ_fw, occ_bw]."""
        import torch
        if want_occ and not occ:
            raise ValueError("want_occ needs occ=True")
        gray = frames.dim() == 3
        f4 = frames.unsqueeze(-1) if gray else frames
        if f4.dim() != 4 or f4.shape[-1] != p.noc or f4.dtype != torch.uint8 or not f4.is_cuda:
            raise ValueError("expected a uint8 CUDA tensor with noc channels")
        if out_dtype not in (None, torch.uint8, torch.float32):
            raise OfdisError(ERR_INVALID_ARGUMENT, f"run_sequence_interp: out_dtype {out_dtype!r}")
        f32 = out_dtype == torch.float32
        tt = _times(t)
        nf, h, w, _ = f4.shape
        n = max(nf - stride, 0) if stride >= 1 else 0  # (the library refuses stride < 1 and nf <= stride)
        f4 = f4.contiguous()
        shape = (n, tt.size, h, w) if gray else (n, tt.size, h, w, 3)
        out = torch.empty(shape, dtype=torch.float32 if f32 else torch.uint8, device=f4.device)
        valid = torch.empty((n, tt.size, h, w), dtype=torch.uint8, device=f4.device) if want_valid else None
        masks = [torch.empty((n, h, w), dtype=torch.uint8, device=f4.device) for _ in range(2 if want_occ else 0)]
        self.run_sequence_interp_ptr(f4.data_ptr(), nf, stride, w, h, p, tt, IMG_F32 if f32 else IMG_U8,
                                     out.data_ptr(), valid.data_ptr() if want_valid else 0, occ, alpha, beta,
                                     masks[0].data_ptr() if want_occ else 0, masks[1].data_ptr() if want_occ else 0,
                                     torch.cuda.current_stream(f4.device).cuda_stream)
        res = [out] + ([valid] if want_valid else []) + masks
        return tuple(res) if len(res) > 1 else out

    def run_sequence_interp_host(self, frames: np.ndarray, p: Params, t=0.5, stride: int = 1, out_dtype=np.uint8,
                                 want_valid: bool = False, occ: bool = False, alpha: float = 0.01, beta: float = 0.5,
                                 want_occ: bool = False):
        """run_sequence_interp on a numpy u8 array [T, h, w] or [T, h, w, noc]; synchronous."""
        if want_occ and not occ:
            raise ValueError("want_occ needs occ=True")
        if np.dtype(out_dtype) not in (np.dtype(np.uint8), np.dtype(_f32)):
            raise OfdisError(ERR_INVALID_ARGUMENT, f"run_sequence_interp_host: out_dtype {out_dtype!r}")
        gray = frames.ndim == 3
        f4 = np.ascontiguousarray(frames[..., None] if gray else frames, np.uint8)
        if f4.ndim != 4 or f4.shape[-1] != p.noc:
            raise ValueError("expected a uint8 array with noc channels")
        nf, h, w = f4.shape[:3]
        n = max(nf - stride, 0) if stride >= 1 else 0
        tt = _times(t)
        out = np.empty((n, tt.size, h, w) if gray else (n, tt.size, h, w, p.noc), out_dtype)
        valid = np.empty((n, tt.size, h, w), np.uint8) if want_valid else None
        masks = [np.empty((n, h, w), np.uint8) for _ in range(2 if want_occ else 0)]
        check(lib().ofdis_run_sequence_interp_u8_host(self._h, f4.ctypes.data, nf, stride, w, h, C.byref(p),
                                                      tt.ctypes.data, tt.size, int(bool(occ)), alpha, beta,
                                                      IMG_F32 if np.dtype(out_dtype) == _f32 else IMG_U8,
                                                      out.ctypes.data, valid.ctypes.data if want_valid else None,
                                                      masks[0].ctypes.data if want_occ else None,
                                                      masks[1].ctypes.data if want_occ else None),
              "ofdis_run_sequence_interp_u8_host")
        res = [out] + ([valid] if want_valid else []) + masks
        return tuple(res) if len(res) > 1 else out

    def track_points_ptr(self, fw_ptr: int, bw_ptr: int, view: FlowView, m: int, width: int, height: int,
                         points_ptr: int, npts: int, start_ptr: int = 0, alpha: float = 0.01, beta: float = 0.5,
                         flags: int = 0, tracks_ptr: int = 0, status_ptr: int = 0, stream: int = 0) -> None:
        """``ofdis_track_points`` on raw device pointers (0: no backward chain / no start array / that output is not
        wanted); flags 0 or TRACK_LAST."""
        check(lib().ofdis_track_points(self._h, fw_ptr or None, bw_ptr or None, None if view is None else C.byref(view),
                                       m, width, height, points_ptr or None, start_ptr or None, npts, alpha, beta, flags,
                                       tracks_ptr or None, status_ptr or None, stream or None), "ofdis_track_points")

    def track_points(self, flow_fw, points, flow_bw=None, start=None, alpha: float = 0.01, beta: float = 0.5,
                     layout: str = "nhwc", grid: str = "full", p: Optional[Params] = None, size=None,
                     last_only: bool = False):
        """Points followed along a chain of flow fields (the definition is in ofdis.h).  flow_fw: the m forward fields
        of a video, field j from frame j to frame j + 1 -- ``run_sequence``'s flow in any format, described as for
        ``warp`` (dtype from the tensor, layout, grid; grid "level" takes float32 "nhwc" grids and needs the parameters
        `p` and size = (width, height)).  flow_bw: the m backward fields in the same format, or None (no consistency
        check).  points: float32 CUDA tensor [N, 2], (x, y) in pixels; start: None or int32 CUDA tensor [N], the frame
        at which each point enters.  Returns (tracks float32 [m + 1, N, 2], status uint8 [m + 1, N]) -- status 0 tracked,
        1 tracked past a failed forward-backward check, 2 left the frame (frozen), 3 not started -- or with last_only
        the last entry alone, [N, 2] and [N]."""
        import torch
        if not (flow_fw.is_cuda and points.is_cuda) or points.dim() != 2 or points.shape[1] != 2 or points.dtype != torch.float32:
            raise ValueError("expected a CUDA flow tensor and a float32 CUDA tensor of points [N, 2]")
        if flow_fw.dim() != 4:
            raise ValueError("expected the m fields of a chain as one tensor of four dimensions")
        fmt = out_format(flow_fw.dtype, layout, grid)
        m = flow_fw.shape[0]
        if grid == "level":
            if p is None or size is None:
                raise OfdisError(ERR_INVALID_ARGUMENT, 'track_points: grid="level" needs the parameters the flows were '
                                 "computed with and the frame size")
            w, h = int(size[0]), int(size[1])
            g = out_geometry(p, w, h, False, flow_fw.dtype, layout, grid)
            view = FlowView(fmt.dtype, fmt.layout, fmt.grid, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])
        else:
            h, w = (flow_fw.shape[2], flow_fw.shape[3]) if fmt.layout else (flow_fw.shape[1], flow_fw.shape[2])
            view = FlowView(fmt.dtype, fmt.layout, fmt.grid, w, h, 1, 0, 0)
        want = (m, 2, view.gh, view.gw) if fmt.layout else (m, view.gh, view.gw, 2)
        if tuple(flow_fw.shape) != want:
            raise ValueError(f"flow_fw has shape {tuple(flow_fw.shape)}, expected {want}")
        if flow_bw is not None and (tuple(flow_bw.shape) != want or flow_bw.dtype != flow_fw.dtype or not flow_bw.is_cuda):
            raise ValueError(f"flow_bw must be a CUDA tensor of flow_fw's dtype and shape {want}")
        n = points.shape[0]
        if start is not None and (tuple(start.shape) != (n,) or start.dtype != torch.int32 or not start.is_cuda):
            raise ValueError(f"start must be an int32 CUDA tensor [{n}]")
        flow_fw, points = flow_fw.contiguous(), points.contiguous()
        flow_bw = flow_bw.contiguous() if flow_bw is not None else None
        start = start.contiguous() if start is not None else None
        tracks = torch.empty((n, 2) if last_only else (m + 1, n, 2), dtype=torch.float32, device=points.device)
        status = torch.empty((n,) if last_only else (m + 1, n), dtype=torch.uint8, device=points.device)
        self.track_points_ptr(flow_fw.data_ptr(), flow_bw.data_ptr() if flow_bw is not None else 0, view, m, w, h,
                              points.data_ptr(), n, start.data_ptr() if start is not None else 0, alpha, beta,
                              TRACK_LAST if last_only else 0, tracks.data_ptr(), status.data_ptr(),
                              torch.cuda.current_stream(points.device).cuda_stream)
        return tracks, status

    def run_sequence_track_ptr(self, frames_ptr: int, nframes: int, width: int, height: int, p: Params, points_ptr: int,
                               npts: int, start_ptr: int = 0, fb: bool = True, alpha: float = 0.01, beta: float = 0.5,
                               flags: int = 0, tracks_ptr: int = 0, status_ptr: int = 0, stream: int = 0) -> None:
        """``ofdis_run_sequence_track_u8`` on raw device pointers, asynchronous on `stream`: frames u8
        [nframes, h, w, noc], the points through its nframes - 1 pairs (0: no start array / that output is not wanted)."""
        check(lib().ofdis_run_sequence_track_u8(self._h, frames_ptr or None, nframes, width, height, C.byref(p),
                                                points_ptr or None, start_ptr or None, npts, int(bool(fb)), alpha, beta,
                                                flags, tracks_ptr or None, status_ptr or None, stream or None),
              "ofdis_run_sequence_track_u8")

    def run_sequence_track(self, frames, p: Params, points, start=None, fb: bool = True, alpha: float = 0.01,
                           beta: float = 0.5, last_only: bool = False):
        """The flows of a video and the tracks through them in one call: torch.uint8 CUDA tensor [T, h, w] or
        [T, h, w, noc] and float32 points [N, 2] -> (tracks [T, N, 2], status [T, N]) ([N, 2] and [N] with last_only),
        bit for bit ``track_points`` on ``run_sequence(frames, p, bidir=True)``'s two flows (fb=False: on the forward
        flow alone) -- but the flows stay on their level grids: no full-resolution flow is written."""
        import torch
        f4 = frames.unsqueeze(-1) if frames.dim() == 3 else frames
        if f4.dim() != 4 or f4.shape[-1] != p.noc or f4.dtype != torch.uint8 or not f4.is_cuda:
            raise ValueError("expected a uint8 CUDA tensor with noc channels")
        if not points.is_cuda or points.dim() != 2 or points.shape[1] != 2 or points.dtype != torch.float32:
            raise ValueError("expected a float32 CUDA tensor of points [N, 2]")
        t, h, w, _ = f4.shape
        n = points.shape[0]
        if start is not None and (tuple(start.shape) != (n,) or start.dtype != torch.int32 or not start.is_cuda):
            raise ValueError(f"start must be an int32 CUDA tensor [{n}]")
        f4, points = f4.contiguous(), points.contiguous()
        start = start.contiguous() if start is not None else None
        tracks = torch.empty((n, 2) if last_only else (t, n, 2), dtype=torch.float32, device=f4.device)
        status = torch.empty((n,) if last_only else (t, n), dtype=torch.uint8, device=f4.device)
        self.run_sequence_track_ptr(f4.data_ptr(), t, w, h, p, points.data_ptr(), n,
                                    start.data_ptr() if start is not None else 0, fb, alpha, beta,
                                    TRACK_LAST if last_only else 0, tracks.data_ptr(), status.data_ptr(),
                                    torch.cuda.current_stream(f4.device).cuda_stream)
        return tracks, status

    def run_sequence_track_host(self, frames: np.ndarray, p: Params, points: np.ndarray, start=None, fb: bool = True,
                                alpha: float = 0.01, beta: float = 0.5, last_only: bool = False):
        """run_sequence_track on numpy arrays (frames u8 [T, h, w] or [T, h, w, noc], points [N, 2]); synchronous."""
        f4 = np.ascontiguousarray(frames[..., None] if frames.ndim == 3 else frames, np.uint8)
        if f4.ndim != 4 or f4.shape[-1] != p.noc:
            raise ValueError("expected a uint8 array with noc channels")
        pts = np.ascontiguousarray(points, _f32)
        if pts.ndim != 2 or pts.shape[1] != 2:
            raise ValueError("expected points [N, 2]")
        t, h, w = f4.shape[:3]
        n = pts.shape[0]
        st = None if start is None else np.ascontiguousarray(start, np.int32)
        if st is not None and st.shape != (n,):
            raise ValueError(f"start must have shape ({n},)")
        tracks = np.empty((n, 2) if last_only else (t, n, 2), _f32)
        status = np.empty((n,) if last_only else (t, n), np.uint8)
        check(lib().ofdis_run_sequence_track_u8_host(self._h, f4.ctypes.data, t, w, h, C.byref(p),
                                                     pts.ctypes.data if n else None,
                                                     None if st is None else st.ctypes.data, n, int(bool(fb)), alpha, beta,
                                                     TRACK_LAST if last_only else 0, tracks.ctypes.data,
                                                     status.ctypes.data), "ofdis_run_sequence_track_u8_host")
        return tracks, status

    def tfilter_ptr(self, frames_ptr: int, nframes: int, fw_ptr: int, bw_ptr: int, view: FlowView, width: int,
                    height: int, noc: int, sigma: float, out_dtype: int, out_ptr: int, used_ptr: int = 0,
                    occ_fw_ptr: int = 0, occ_bw_ptr: int = 0, stream: int = 0) -> None:
        """``ofdis_tfilter_u8`` on raw device pointers (0: no `used` output / no occlusion mask); out_dtype IMG_U8 /
        IMG_F32."""
        check(lib().ofdis_tfilter_u8(self._h, frames_ptr or None, nframes, fw_ptr or None, bw_ptr or None,
                                     None if view is None else C.byref(view), width, height, noc, sigma,
                                     occ_fw_ptr or None, occ_bw_ptr or None, out_dtype, out_ptr or None,
                                     used_ptr or None, stream or None), "ofdis_tfilter_u8")

    def tfilter(self, frames, flow_fw, flow_bw, sigma: float, occ_fw=None, occ_bw=None, out_dtype=None,
                want_used: bool = False, grid: str = "full", p: Optional[Params] = None, size=None,
                layout: str = "nhwc"):
        """Motion-compensated temporal denoising (the definition is in ofdis.h): every frame of a video averaged with
        its two neighbours pulled onto it along the flows, each neighbour weighted per pixel by 1 - (d / (sigma noc))^2
        of its distance d to the frame's own pixel.  frames: torch.uint8 CUDA tensor [T, h, w] or [T, h, w, 3];
        flow_fw / flow_bw: the T - 1 forward / backward fields of ``run_sequence(frames, p, bidir=True)`` in one
        format, described as for ``track_points`` (dtype from the tensors, layout, grid; grid "level" takes float32
        "nhwc" grids and needs `p`; size defaults to the frames' (width, height)).  occ_fw / occ_bw: that call's masks
        ([T - 1, h, w] uint8), either or both; a marked pixel does not take that neighbour.  Returns the filtered
        frames in the frames' shape, torch.uint8 (the default) or torch.float32; with want_used the tuple (frames, used
        uint8 [T, h, w]: bit 0 the previous frame contributed, bit 1 the next)."""
        import torch
        _tfilter_checks("tfilter", sigma, out_dtype, (None, torch.uint8, torch.float32))
        gray = frames.dim() == 3
        f4 = frames.unsqueeze(-1) if gray else frames
        if (f4.dim() != 4 or f4.shape[-1] not in (1, 3) or f4.dtype != torch.uint8
                or not (f4.is_cuda and flow_fw.is_cuda and flow_bw.is_cuda)):
            raise ValueError("expected a uint8 CUDA tensor [T, h, w] or [T, h, w, 3] and two CUDA flow tensors")
        t, h, w, noc = f4.shape
        if t < 2:
            raise OfdisError(ERR_INVALID_ARGUMENT, "tfilter: a video needs two frames or more")
        if size is not None and (int(size[0]), int(size[1])) != (w, h):
            raise ValueError(f"size {tuple(size)} is not the frames' {(w, h)}")
        if flow_fw.dtype != flow_bw.dtype:
            raise ValueError("the two flows must have one dtype")
        fmt = out_format(flow_fw.dtype, layout, grid)
        view = FlowView(fmt.dtype, fmt.layout, fmt.grid, w, h, 1, 0, 0)
        if grid == "level":
            if p is None:
                raise OfdisError(ERR_INVALID_ARGUMENT, 'tfilter: grid="level" needs the parameters the flows were computed with')
            g = out_geometry(p, w, h, False, flow_fw.dtype, layout, grid)
            view = FlowView(fmt.dtype, fmt.layout, fmt.grid, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])
        want = (t - 1, 2, view.gh, view.gw) if fmt.layout else (t - 1, view.gh, view.gw, 2)
        if tuple(flow_fw.shape) != want or tuple(flow_bw.shape) != want:
            raise ValueError(f"flows have shapes {tuple(flow_fw.shape)} and {tuple(flow_bw.shape)}, expected {want}")
        for occ in (occ_fw, occ_bw):
            if occ is not None and (tuple(occ.shape) != (t - 1, h, w) or occ.dtype != torch.uint8 or not occ.is_cuda):
                raise ValueError(f"expected uint8 CUDA occlusion masks of shape {(t - 1, h, w)}")
        f32 = out_dtype == torch.float32
        f4, flow_fw, flow_bw = f4.contiguous(), flow_fw.contiguous(), flow_bw.contiguous()
        occ_fw = occ_fw.contiguous() if occ_fw is not None else None
        occ_bw = occ_bw.contiguous() if occ_bw is not None else None
        out = torch.empty(frames.shape, dtype=torch.float32 if f32 else torch.uint8, device=f4.device)
        used = torch.empty((t, h, w), dtype=torch.uint8, device=f4.device) if want_used else None
        self.tfilter_ptr(f4.data_ptr(), t, flow_fw.data_ptr(), flow_bw.data_ptr(), view, w, h, noc, float(sigma),
                         IMG_F32 if f32 else IMG_U8, out.data_ptr(), used.data_ptr() if want_used else 0,
                         occ_fw.data_ptr() if occ_fw is not None else 0, occ_bw.data_ptr() if occ_bw is not None else 0,
                         torch.cuda.current_stream(f4.device).cuda_stream)
        return (out, used) if want_used else out

    def run_sequence_tfilter_ptr(self, frames_ptr: int, nframes: int, width: int, height: int, p: Params, sigma: float,
                                 out_dtype: int, out_ptr: int, used_ptr: int = 0, occ: bool = False,
                                 alpha: float = 0.01, beta: float = 0.5, stream: int = 0) -> None:
        """``ofdis_run_sequence_tfilter_u8`` on raw device pointers, asynchronous on `stream`: frames u8
        [nframes, h, w, noc] -> the filtered frames (used_ptr 0: no `used` output); out_dtype IMG_U8 / IMG_F32."""
        check(lib().ofdis_run_sequence_tfilter_u8(self._h, frames_ptr or None, nframes, width, height, C.byref(p), sigma,
                                                  int(bool(occ)), alpha, beta, out_dtype, out_ptr or None,
                                                  used_ptr or None, stream or None), "ofdis_run_sequence_tfilter_u8")

    def run_sequence_tfilter(self, frames, p: Params, sigma: float, occ: bool = False, alpha: float = 0.01,
                             beta: float = 0.5, out_dtype=None, want_used: bool = False):
        """The flows of a video and its filtered frames in one call: torch.uint8 CUDA tensor [T, h, w] or
        [T, h, w, noc] -> the filtered frames in that shape (torch.uint8, or torch.float32), with want_used the tuple
        (frames, used [T, h, w]).  Bit for bit ``tfilter(frames, *run_sequence(frames, p, bidir=True)[:2], sigma)`` --
        with occ, also given that call's two masks at alpha, beta -- but the flows stay on their level grids: no
        full-resolution flow is written."""
        import torch
        _tfilter_checks("run_sequence_tfilter", sigma, out_dtype, (None, torch.uint8, torch.float32))
        f4 = frames.unsqueeze(-1) if frames.dim() == 3 else frames
        if f4.dim() != 4 or f4.shape[-1] != p.noc or f4.dtype != torch.uint8 or not f4.is_cuda:
            raise ValueError("expected a uint8 CUDA tensor with noc channels")
        t, h, w, _ = f4.shape
        if t < 2:
            raise OfdisError(ERR_INVALID_ARGUMENT, "run_sequence_tfilter: a video needs two frames or more")
        f32 = out_dtype == torch.float32
        f4 = f4.contiguous()
        out = torch.empty(frames.shape, dtype=torch.float32 if f32 else torch.uint8, device=f4.device)
        used = torch.empty((t, h, w), dtype=torch.uint8, device=f4.device) if want_used else None
        self.run_sequence_tfilter_ptr(f4.data_ptr(), t, w, h, p, float(sigma), IMG_F32 if f32 else IMG_U8,
                                      out.data_ptr(), used.data_ptr() if want_used else 0, occ, alpha, beta,
                                      torch.cuda.current_stream(f4.device).cuda_stream)
        return (out, used) if want_used else out

    def run_sequence_tfilter_host(self, frames: np.ndarray, p: Params, sigma: float, occ: bool = False,
                                  alpha: float = 0.01, beta: float = 0.5, out_dtype=np.uint8, want_used: bool = False):
        """run_sequence_tfilter on a numpy u8 array [T, h, w] or [T, h, w, noc]; synchronous."""
        _tfilter_checks("run_sequence_tfilter_host", sigma, np.dtype(np.uint8 if out_dtype is None else out_dtype),
                        (np.dtype(np.uint8), np.dtype(_f32)))
        f4 = np.ascontiguousarray(frames[..., None] if frames.ndim == 3 else frames, np.uint8)
        if f4.ndim != 4 or f4.shape[-1] != p.noc:
            raise ValueError("expected a uint8 array with noc channels")
        t, h, w = f4.shape[:3]
        if t < 2:
            raise OfdisError(ERR_INVALID_ARGUMENT, "run_sequence_tfilter_host: a video needs two frames or more")
        f32 = out_dtype is not None and np.dtype(out_dtype) == _f32
        out = np.empty(frames.shape, _f32 if f32 else np.uint8)
        used = np.empty((t, h, w), np.uint8) if want_used else None
        check(lib().ofdis_run_sequence_tfilter_u8_host(self._h, f4.ctypes.data, t, w, h, C.byref(p), float(sigma),
                                                       int(bool(occ)), alpha, beta, IMG_F32 if f32 else IMG_U8,
                                                       out.ctypes.data, used.ctypes.data if want_used else None),
              "ofdis_run_sequence_tfilter_u8_host")
        return (out, used) if want_used else out

    def tfilter_radius_ptr(self, frames_ptr: int, nframes: int, fw_ptr: int, bw_ptr: int, view: FlowView, width: int,
                           height: int, noc: int, radius: int, sigma: float, out_dtype: int, out_ptr: int,
                           used_ptr: int = 0, fb: bool = False, alpha: float = 0.01, beta: float = 0.5,
                           stream: int = 0) -> None:
        """``ofdis_tfilter_radius_u8`` on raw device pointers (0: no `used` output); out_dtype IMG_U8 / IMG_F32."""
        check(lib().ofdis_tfilter_radius_u8(self._h, frames_ptr or None, nframes, fw_ptr or None, bw_ptr or None,
                                            None if view is None else C.byref(view), width, height, noc, radius, sigma,
                                            int(bool(fb)), alpha, beta, out_dtype, out_ptr or None, used_ptr or None,
                                            stream or None), "ofdis_tfilter_radius_u8")

    def tfilter_radius(self, frames, flow_fw, flow_bw, sigma: float, radius: int, fb: bool = False, alpha: float = 0.01,
                       beta: float = 0.5, out_dtype=None, want_used: bool = False, layout: str = "nhwc",
                       grid: str = "full", p: Optional[Params] = None, size=None):
        """``tfilter`` over `radius` (1 .. 4) frames on each side (the definition is in ofdis.h): a pixel's position is
        chained through the fields as ``track_points`` chains a point, and every frame it passes is sampled there and
        weighted as ``tfilter`` weights a neighbour.  With fb every chain step runs the forward-backward check at alpha,
        beta, and a failed or out-of-frame step drops that frame and every farther one of its direction -- there are no
        mask inputs.  frames, flow_fw, flow_bw, layout, grid, p, size and out_dtype are ``tfilter``'s.  Returns the
        filtered frames, with want_used the tuple (frames, used uint8 [T, h, w]: bit 2 (k - 1) the k-th previous frame
        contributed, bit 2 (k - 1) + 1 the k-th next)."""
        import torch
        _tfilter_checks("tfilter_radius", sigma, out_dtype, (None, torch.uint8, torch.float32))
        _tfilter_radius_checks("tfilter_radius", radius, fb, alpha, beta)
        gray = frames.dim() == 3
        f4 = frames.unsqueeze(-1) if gray else frames
        if (f4.dim() != 4 or f4.shape[-1] not in (1, 3) or f4.dtype != torch.uint8
                or not (f4.is_cuda and flow_fw.is_cuda and flow_bw.is_cuda)):
            raise ValueError("expected a uint8 CUDA tensor [T, h, w] or [T, h, w, 3] and two CUDA flow tensors")
        t, h, w, noc = f4.shape
        if t < 2:
            raise OfdisError(ERR_INVALID_ARGUMENT, "tfilter_radius: a video needs two frames or more")
        if size is not None and (int(size[0]), int(size[1])) != (w, h):
            raise ValueError(f"size {tuple(size)} is not the frames' {(w, h)}")
        if flow_fw.dtype != flow_bw.dtype:
            raise ValueError("the two flows must have one dtype")
        fmt = out_format(flow_fw.dtype, layout, grid)
        view = FlowView(fmt.dtype, fmt.layout, fmt.grid, w, h, 1, 0, 0)
        if grid == "level":
            if p is None:
                raise OfdisError(ERR_INVALID_ARGUMENT,
                                 'tfilter_radius: grid="level" needs the parameters the flows were computed with')
            g = out_geometry(p, w, h, False, flow_fw.dtype, layout, grid)
            view = FlowView(fmt.dtype, fmt.layout, fmt.grid, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])
        want = (t - 1, 2, view.gh, view.gw) if fmt.layout else (t - 1, view.gh, view.gw, 2)
        if tuple(flow_fw.shape) != want or tuple(flow_bw.shape) != want:
            raise ValueError(f"flows have shapes {tuple(flow_fw.shape)} and {tuple(flow_bw.shape)}, expected {want}")
        f32 = out_dtype == torch.float32
        f4, flow_fw, flow_bw = f4.contiguous(), flow_fw.contiguous(), flow_bw.contiguous()
        out = torch.empty(frames.shape, dtype=torch.float32 if f32 else torch.uint8, device=f4.device)
        used = torch.empty((t, h, w), dtype=torch.uint8, device=f4.device) if want_used else None
        self.tfilter_radius_ptr(f4.data_ptr(), t, flow_fw.data_ptr(), flow_bw.data_ptr(), view, w, h, noc, int(radius),
                                float(sigma), IMG_F32 if f32 else IMG_U8, out.data_ptr(),
                                used.data_ptr() if want_used else 0, fb, alpha, beta,
                                torch.cuda.current_stream(f4.device).cuda_stream)
        return (out, used) if want_used else out

    def run_sequence_tfilter_radius_ptr(self, frames_ptr: int, nframes: int, width: int, height: int, p: Params,
                                        radius: int, sigma: float, out_dtype: int, out_ptr: int, used_ptr: int = 0,
                                        fb: bool = False, alpha: float = 0.01, beta: float = 0.5, stream: int = 0) -> None:
        """``ofdis_run_sequence_tfilter_radius_u8`` on raw device pointers, asynchronous on `stream`: frames u8
        [nframes, h, w, noc] -> the filtered frames (used_ptr 0: no `used` output); out_dtype IMG_U8 / IMG_F32."""
        check(lib().ofdis_run_sequence_tfilter_radius_u8(self._h, frames_ptr or None, nframes, width, height, C.byref(p),
                                                         radius, sigma, int(bool(fb)), alpha, beta, out_dtype,
                                                         out_ptr or None, used_ptr or None, stream or None),
              "ofdis_run_sequence_tfilter_radius_u8")

    def run_sequence_tfilter_radius(self, frames, p: Params, sigma: float, radius: int, fb: bool = False,
                                    alpha: float = 0.01, beta: float = 0.5, out_dtype=None, want_used: bool = False):
        """The flows of a video and its frames filtered over `radius` frames on each side in one call: torch.uint8 CUDA
        tensor [T, h, w] or [T, h, w, noc] -> the filtered frames in that shape (torch.uint8, or torch.float32), with
        want_used the tuple (frames, used [T, h, w]).  Bit for bit
        ``tfilter_radius(frames, *run_sequence(frames, p, bidir=True)[:2], sigma, radius, fb, alpha, beta)``, but the flows
        stay on their level grids and the check runs inside the filter: no full-resolution flow and no mask is
        written."""
        import torch
        _tfilter_checks("run_sequence_tfilter_radius", sigma, out_dtype, (None, torch.uint8, torch.float32))
        _tfilter_radius_checks("run_sequence_tfilter_radius", radius, fb, alpha, beta)
        f4 = frames.unsqueeze(-1) if frames.dim() == 3 else frames
        if f4.dim() != 4 or f4.shape[-1] != p.noc or f4.dtype != torch.uint8 or not f4.is_cuda:
            raise ValueError("expected a uint8 CUDA tensor with noc channels")
        t, h, w, _ = f4.shape
        if t < 2:
            raise OfdisError(ERR_INVALID_ARGUMENT, "run_sequence_tfilter_radius: a video needs two frames or more")
        f32 = out_dtype == torch.float32
        f4 = f4.contiguous()
        out = torch.empty(frames.shape, dtype=torch.float32 if f32 else torch.uint8, device=f4.device)
        used = torch.empty((t, h, w), dtype=torch.uint8, device=f4.device) if want_used else None
        self.run_sequence_tfilter_radius_ptr(f4.data_ptr(), t, w, h, p, int(radius), float(sigma),
                                             IMG_F32 if f32 else IMG_U8, out.data_ptr(),
                                             used.data_ptr() if want_used else 0, fb, alpha, beta,
                                             torch.cuda.current_stream(f4.device).cuda_stream)
        return (out, used) if want_used else out

    def run_sequence_tfilter_radius_host(self, frames: np.ndarray, p: Params, sigma: float, radius: int,
                                         fb: bool = False, alpha: float = 0.01, beta: float = 0.5, out_dtype=np.uint8,
                                         want_used: bool = False):
        """run_sequence_tfilter_radius on a numpy u8 array [T, h, w] or [T, h, w, noc]; synchronous."""
        _tfilter_checks("run_sequence_tfilter_radius_host", sigma, np.dtype(np.uint8 if out_dtype is None else out_dtype),
                        (np.dtype(np.uint8), np.dtype(_f32)))
        _tfilter_radius_checks("run_sequence_tfilter_radius_host", radius, fb, alpha, beta)
        f4 = np.ascontiguousarray(frames[..., None] if frames.ndim == 3 else frames, np.uint8)
        if f4.ndim != 4 or f4.shape[-1] != p.noc:
            raise ValueError("expected a uint8 array with noc channels")
        t, h, w = f4.shape[:3]
        if t < 2:
            raise OfdisError(ERR_INVALID_ARGUMENT, "run_sequence_tfilter_radius_host: a video needs two frames or more")
        f32 = out_dtype is not None and np.dtype(out_dtype) == _f32
        out = np.empty(frames.shape, _f32 if f32 else np.uint8)
        used = np.empty((t, h, w), np.uint8) if want_used else None
        check(lib().ofdis_run_sequence_tfilter_radius_u8_host(self._h, f4.ctypes.data, t, w, h, C.byref(p), int(radius),
                                                              float(sigma), int(bool(fb)), alpha, beta,
                                                              IMG_F32 if f32 else IMG_U8, out.ctypes.data,
                                                              used.ctypes.data if want_used else None),
              "ofdis_run_sequence_tfilter_radius_u8_host")
        return (out, used) if want_used else out

    def fit_motion_ptr(self, fw_ptr: int, bw_ptr: int, view: FlowView, m: int, width: int, height: int, model: int,
                       step: int, tau: float, iters: int, xform_ptr: int, support_ptr: int = 0, weights_ptr: int = 0,
                       alpha: float = 0.01, beta: float = 0.5, stream: int = 0) -> None:
        """``ofdis_fit_motion`` on raw device pointers (0: no backward chain / that output is not wanted)."""
        check(lib().ofdis_fit_motion(self._h, fw_ptr or None, bw_ptr or None, None if view is None else C.byref(view),
                                     m, width, height, model, step, tau, iters, alpha, beta, xform_ptr or None,
                                     support_ptr or None, weights_ptr or None, stream or None), "ofdis_fit_motion")

    def fit_motion(self, flow_fw, flow_bw=None, model: int = MOTION_SIMILARITY, step: int = 16, tau: float = 2.0,
                   iters: int = 4, alpha: float = 0.01, beta: float = 0.5, layout: str = "nhwc", grid: str = "full",
                   p: Optional[Params] = None, size=None, want_support: bool = False, want_weights: bool = False):
        """The camera's motion per frame pair (the definition is in ofdis.h): a robust similarity (or translation)
        fitted to each of the m fields of flow_fw at the lattice ``fit_lattice(width, height, step)``, with Tukey-like
        weights 1 - r^2 / t^2 annealed over `iters` re-solves down to the threshold tau (pixels).  flow_fw / flow_bw:
        described as for ``track_points`` (grid "level" takes float32 "nhwc" grids and needs `p` and size = (width,
        height)); with flow_bw a sample also has to pass the forward-backward check at alpha, beta.  Returns the
        transforms, torch.float64 [m, 6] = (m00, m01, m02, m10, m11, m12) with position in frame j + 1 = M position in
        frame j; with want_support also int32 [m], the samples with a positive weight; with want_weights also float32
        [m, ns]."""
        import torch
        if not flow_fw.is_cuda or flow_fw.dim() != 4:
            raise ValueError("expected the m fields of a chain as one CUDA tensor of four dimensions")
        fmt = out_format(flow_fw.dtype, layout, grid)
        m = flow_fw.shape[0]
        if grid == "level":
            if p is None or size is None:
                raise OfdisError(ERR_INVALID_ARGUMENT, 'fit_motion: grid="level" needs the parameters the flows were '
                                 "computed with and the frame size")
            w, h = int(size[0]), int(size[1])
        else:
            h, w = (flow_fw.shape[2], flow_fw.shape[3]) if fmt.layout else (flow_fw.shape[1], flow_fw.shape[2])
        ns = _motion_checks("fit_motion", w, h, model, step, tau, iters)
        if grid == "level":
            g = out_geometry(p, w, h, False, flow_fw.dtype, layout, grid)
            view = FlowView(fmt.dtype, fmt.layout, fmt.grid, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])
        else:
            view = FlowView(fmt.dtype, fmt.layout, fmt.grid, w, h, 1, 0, 0)
        want = (m, 2, view.gh, view.gw) if fmt.layout else (m, view.gh, view.gw, 2)
        if tuple(flow_fw.shape) != want:
            raise ValueError(f"flow_fw has shape {tuple(flow_fw.shape)}, expected {want}")
        if flow_bw is not None and (tuple(flow_bw.shape) != want or flow_bw.dtype != flow_fw.dtype or not flow_bw.is_cuda):
            raise ValueError(f"flow_bw must be a CUDA tensor of flow_fw's dtype and shape {want}")
        flow_fw = flow_fw.contiguous()
        flow_bw = flow_bw.contiguous() if flow_bw is not None else None
        xform = torch.empty((m, 6), dtype=torch.float64, device=flow_fw.device)
        support = torch.empty((m,), dtype=torch.int32, device=flow_fw.device) if want_support else None
        weights = torch.empty((m, ns), dtype=torch.float32, device=flow_fw.device) if want_weights else None
        self.fit_motion_ptr(flow_fw.data_ptr(), flow_bw.data_ptr() if flow_bw is not None else 0, view, m, w, h,
                            int(model), int(step), float(tau), int(iters), xform.data_ptr(),
                            support.data_ptr() if want_support else 0, weights.data_ptr() if want_weights else 0,
                            alpha, beta, torch.cuda.current_stream(flow_fw.device).cuda_stream)
        res = [xform] + ([support] if want_support else []) + ([weights] if want_weights else [])
        return tuple(res) if len(res) > 1 else xform

    def smooth_path_ptr(self, xform_ptr: int, m: int, radius: int, zoom: float, width: int, height: int, corr_ptr: int,
                        stream: int = 0) -> None:
        """``ofdis_smooth_path`` on raw device pointers."""
        check(lib().ofdis_smooth_path(self._h, xform_ptr or None, m, radius, zoom, width, height, corr_ptr or None,
                                      stream or None), "ofdis_smooth_path")

    def smooth_path(self, xform, size, radius: int = 8, zoom: float = 1.0):
        """The m pair transforms of ``fit_motion`` (torch.float64 CUDA tensor [m, 6]) to the m + 1 per-frame correction
        transforms of a stabilised video of size = (width, height): the cumulative camera path, smoothed with a
        triangular window of `radius` frames either side, and per frame the transform from the smoothed to the real
        path, zoomed in by `zoom` about the frame centre.  Returns torch.float64 [m + 1, 6] for ``warp_affine``."""
        import torch
        if not xform.is_cuda or xform.dim() != 2 or xform.shape[1] != 6 or xform.dtype != torch.float64:
            raise ValueError("expected a float64 CUDA tensor of transforms [m, 6]")
        m, w, h = xform.shape[0], int(size[0]), int(size[1])
        _path_checks("smooth_path", m, radius, zoom, w, h)
        xform = xform.contiguous()
        corr = torch.empty((m + 1, 6), dtype=torch.float64, device=xform.device)
        self.smooth_path_ptr(xform.data_ptr(), m, int(radius), float(zoom), w, h, corr.data_ptr(),
                             torch.cuda.current_stream(xform.device).cuda_stream)
        return corr

    def warp_affine_ptr(self, img_ptr: int, n: int, width: int, height: int, noc: int, xf_ptr: int, out_dtype: int,
                        out_ptr: int, valid_ptr: int = 0, stream: int = 0) -> None:
        """``ofdis_warp_affine_u8`` on raw device pointers (valid_ptr 0: no mask); out_dtype IMG_U8 / IMG_F32."""
        check(lib().ofdis_warp_affine_u8(self._h, img_ptr or None, n, width, height, noc, xf_ptr or None, out_dtype,
                                         out_ptr or None, valid_ptr or None, stream or None), "ofdis_warp_affine_u8")

    def warp_affine(self, img, xf, out_dtype=None, want_valid: bool = False):
        """Each of n u8 frames (torch.uint8 CUDA tensor [n, h, w] or [n, h, w, 3]) pulled through its own transform xf
        (torch.float64 CUDA tensor [n, 6]: output pixel (x, y) shows the input at M (x, y, 1)), with ``warp``'s
        bilinear taps, replicated border and rounding.  Returns the frames in img's shape, torch.uint8 (the default) or
        torch.float32; with want_valid the tuple (frames, valid uint8 [n, h, w])."""
        import torch
        if out_dtype not in (None, torch.uint8, torch.float32):
            raise OfdisError(ERR_INVALID_ARGUMENT, f"warp_affine: out_dtype {out_dtype!r}")
        i4 = img.unsqueeze(-1) if img.dim() == 3 else img
        if i4.dim() != 4 or i4.shape[-1] not in (1, 3) or i4.dtype != torch.uint8 or not i4.is_cuda:
            raise ValueError("expected a uint8 CUDA tensor [n, h, w] or [n, h, w, 3]")
        n, h, w, noc = i4.shape
        if not xf.is_cuda or tuple(xf.shape) != (n, 6) or xf.dtype != torch.float64:
            raise ValueError(f"expected a float64 CUDA tensor of transforms [{n}, 6]")
        f32 = out_dtype == torch.float32
        i4, xf = i4.contiguous(), xf.contiguous()
        out = torch.empty(img.shape, dtype=torch.float32 if f32 else torch.uint8, device=i4.device)
        valid = torch.empty((n, h, w), dtype=torch.uint8, device=i4.device) if want_valid else None
        self.warp_affine_ptr(i4.data_ptr(), n, w, h, noc, xf.data_ptr(), IMG_F32 if f32 else IMG_U8, out.data_ptr(),
                             valid.data_ptr() if want_valid else 0, torch.cuda.current_stream(i4.device).cuda_stream)
        return (out, valid) if want_valid else out

    def run_sequence_stabilize_ptr(self, frames_ptr: int, nframes: int, width: int, height: int, p: Params, model: int,
                                   step: int, tau: float, iters: int, radius: int, zoom: float, out_dtype: int,
                                   out_ptr: int, valid_ptr: int = 0, xform_ptr: int = 0, corr_ptr: int = 0,
                                   support_ptr: int = 0, fb: bool = False, alpha: float = 0.01, beta: float = 0.5,
                                   stream: int = 0) -> None:
        """``ofdis_run_sequence_stabilize_u8`` on raw device pointers, asynchronous on `stream`: frames u8
        [nframes, h, w, noc] -> the stabilised frames (0: that optional output is not wanted)."""
        check(lib().ofdis_run_sequence_stabilize_u8(self._h, frames_ptr or None, nframes, width, height, C.byref(p), model,
                                                    step, tau, iters, int(bool(fb)), alpha, beta, radius, zoom, out_dtype,
                                                    out_ptr or None, valid_ptr or None, xform_ptr or None,
                                                    corr_ptr or None, support_ptr or None, stream or None),
              "ofdis_run_sequence_stabilize_u8")

    def run_sequence_stabilize(self, frames, p: Params, model: int = MOTION_SIMILARITY, step: int = 16, tau: float = 2.0,
                               iters: int = 4, fb: bool = False, alpha: float = 0.01, beta: float = 0.5,
                               radius: int = 8, zoom: float = 1.0, out_dtype=None, want_valid: bool = False,
                               want_path: bool = False):
        """The flows of a video, its camera path and the stabilised frames in one call: torch.uint8 CUDA tensor
        [T, h, w] or [T, h, w, noc] -> the stabilised frames in that shape (torch.uint8, or torch.float32).  Bit for bit
        ``warp_affine(frames, smooth_path(fit_motion(F, B if fb else None, ...), size, radius, zoom))`` on
        ``run_sequence(frames, p, bidir=True)``'s flows -- but the flows stay on their level grids, the check runs at
        the fit's samples alone and no full-resolution flow or mask is written.  want_valid adds valid uint8 [T, h, w];
        want_path adds (xform float64 [T - 1, 6], corr float64 [T, 6], support int32 [T - 1])."""
        import torch
        if out_dtype not in (None, torch.uint8, torch.float32):
            raise OfdisError(ERR_INVALID_ARGUMENT, f"run_sequence_stabilize: out_dtype {out_dtype!r}")
        f4 = frames.unsqueeze(-1) if frames.dim() == 3 else frames
        if f4.dim() != 4 or f4.shape[-1] != p.noc or f4.dtype != torch.uint8 or not f4.is_cuda:
            raise ValueError("expected a uint8 CUDA tensor with noc channels")
        t, h, w, _ = f4.shape
        if t < 2:
            raise OfdisError(ERR_INVALID_ARGUMENT, "run_sequence_stabilize: a video needs two frames or more")
        _motion_checks("run_sequence_stabilize", w, h, model, step, tau, iters)
        _path_checks("run_sequence_stabilize", t - 1, radius, zoom, w, h)
        f32 = out_dtype == torch.float32
        f4 = f4.contiguous()
        dev = f4.device
        out = torch.empty(frames.shape, dtype=torch.float32 if f32 else torch.uint8, device=dev)
        valid = torch.empty((t, h, w), dtype=torch.uint8, device=dev) if want_valid else None
        xform = torch.empty((t - 1, 6), dtype=torch.float64, device=dev) if want_path else None
        corr = torch.empty((t, 6), dtype=torch.float64, device=dev) if want_path else None
        support = torch.empty((t - 1,), dtype=torch.int32, device=dev) if want_path else None
        self.run_sequence_stabilize_ptr(f4.data_ptr(), t, w, h, p, int(model), int(step), float(tau), int(iters),
                                        int(radius), float(zoom), IMG_F32 if f32 else IMG_U8, out.data_ptr(),
                                        valid.data_ptr() if want_valid else 0, xform.data_ptr() if want_path else 0,
                                        corr.data_ptr() if want_path else 0, support.data_ptr() if want_path else 0,
                                        fb, alpha, beta, torch.cuda.current_stream(dev).cuda_stream)
        res = [out] + ([valid] if want_valid else []) + ([xform, corr, support] if want_path else [])
        return tuple(res) if len(res) > 1 else out

    def run_sequence_stabilize_host(self, frames: np.ndarray, p: Params, model: int = MOTION_SIMILARITY, step: int = 16,
                                    tau: float = 2.0, iters: int = 4, fb: bool = False, alpha: float = 0.01,
                                    beta: float = 0.5, radius: int = 8, zoom: float = 1.0, out_dtype=np.uint8,
                                    want_valid: bool = False, want_path: bool = False):
        """run_sequence_stabilize on a numpy u8 array [T, h, w] or [T, h, w, noc]; synchronous."""
        if out_dtype is not None and np.dtype(out_dtype) not in (np.dtype(np.uint8), np.dtype(_f32)):
            raise OfdisError(ERR_INVALID_ARGUMENT, f"run_sequence_stabilize_host: out_dtype {out_dtype!r}")
        f4 = np.ascontiguousarray(frames[..., None] if frames.ndim == 3 else frames, np.uint8)
        if f4.ndim != 4 or f4.shape[-1] != p.noc:
            raise ValueError("expected a uint8 array with noc channels")
        t, h, w = f4.shape[:3]
        if t < 2:
            raise OfdisError(ERR_INVALID_ARGUMENT, "run_sequence_stabilize_host: a video needs two frames or more")
        _motion_checks("run_sequence_stabilize_host", w, h, model, step, tau, iters)
        _path_checks("run_sequence_stabilize_host", t - 1, radius, zoom, w, h)
        f32 = out_dtype is not None and np.dtype(out_dtype) == _f32
        out = np.empty(frames.shape, _f32 if f32 else np.uint8)
        valid = np.empty((t, h, w), np.uint8) if want_valid else None
        xform = np.empty((t - 1, 6), np.float64) if want_path else None
        corr = np.empty((t, 6), np.float64) if want_path else None
        support = np.empty((t - 1,), np.int32) if want_path else None
        check(lib().ofdis_run_sequence_stabilize_u8_host(
            self._h, f4.ctypes.data, t, w, h, C.byref(p), int(model), int(step), float(tau), int(iters), int(bool(fb)),
            alpha, beta, int(radius), float(zoom), IMG_F32 if f32 else IMG_U8, out.ctypes.data,
            valid.ctypes.data if want_valid else None, xform.ctypes.data if want_path else None,
            corr.ctypes.data if want_path else None, support.ctypes.data if want_path else None),
            "ofdis_run_sequence_stabilize_u8_host")
        res = [out] + ([valid] if want_valid else []) + ([xform, corr, support] if want_path else [])
        return tuple(res) if len(res) > 1 else out

    def motion_mask_ptr(self, flow_ptr: int, view: FlowView, m: int, width: int, height: int, xform_ptr: int,
                        occ_ptr: int, thr: float, rel: float, radius: int, code_ptr: int = 0, res_ptr: int = 0,
                        stats_ptr: int = 0, stream: int = 0) -> None:
        """``ofdis_motion_mask`` on raw device pointers (0: no occlusion plane / that output is not wanted)."""
        check(lib().ofdis_motion_mask(self._h, flow_ptr or None, None if view is None else C.byref(view), m, width,
                                      height, xform_ptr or None, occ_ptr or None, thr, rel, radius, code_ptr or None,
                                      res_ptr or None, stats_ptr or None, stream or None), "ofdis_motion_mask")

    def motion_mask(self, flow, xform, occ=None, thr: float = 1.0, rel: float = 0.05, radius: int = 1,
                    want_res: bool = False, want_stats: bool = False, layout: str = "nhwc", grid: str = "full",
                    p: Optional[Params] = None, size=None):
        """The pixels that moved on their own (the definition is in ofdis.h): per pixel the distance e of the estimate
        from the camera's flow under xform (``fit_motion``'s float64 [m, 6]), raw class e > thr and e > rel * |camera
        flow|, and a binary median over the clipped (2 radius + 1)^2 window.  flow: described as for ``track_points``
        (grid "level" takes float32 "nhwc" grids and needs `p` and size = (width, height)).  occ: ``fb_check``'s forward
        plane, torch.uint8 [m, h, w], or None; its nonzero pixels and non-finite estimates are unknown.  Returns code,
        torch.uint8 [m, h, w] (0 static, 1 moving, 2 unknown); with want_res also e as float32 [m, h, w]; with
        want_stats also int64 [m, 12] (``motion_summary`` reads them)."""
        import torch
        if not flow.is_cuda or flow.dim() != 4:
            raise ValueError("expected the m fields as one CUDA tensor of four dimensions")
        fmt = out_format(flow.dtype, layout, grid)
        m = flow.shape[0]
        if grid == "level":
            if p is None or size is None:
                raise OfdisError(ERR_INVALID_ARGUMENT, 'motion_mask: grid="level" needs the parameters the flows were '
                                 "computed with and the frame size")
            w, h = int(size[0]), int(size[1])
        else:
            h, w = (flow.shape[2], flow.shape[3]) if fmt.layout else (flow.shape[1], flow.shape[2])
        _mask_checks("motion_mask", m, thr, rel, radius, w, h)
        if grid == "level":
            g = out_geometry(p, w, h, False, flow.dtype, layout, grid)
            view = FlowView(fmt.dtype, fmt.layout, fmt.grid, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])
        else:
            view = FlowView(fmt.dtype, fmt.layout, fmt.grid, w, h, 1, 0, 0)
        want = (m, 2, view.gh, view.gw) if fmt.layout else (m, view.gh, view.gw, 2)
        if tuple(flow.shape) != want:
            raise ValueError(f"flow has shape {tuple(flow.shape)}, expected {want}")
        if not xform.is_cuda or tuple(xform.shape) != (m, 6) or xform.dtype != torch.float64:
            raise ValueError(f"expected a float64 CUDA tensor of transforms [{m}, 6]")
        if occ is not None and (occ.dtype != torch.uint8 or tuple(occ.shape) != (m, h, w) or not occ.is_cuda):
            raise ValueError(f"expected a uint8 CUDA occlusion plane of shape {(m, h, w)}")
        flow, xform = flow.contiguous(), xform.contiguous()
        occ = occ.contiguous() if occ is not None else None
        dev = flow.device
        code = torch.empty((m, h, w), dtype=torch.uint8, device=dev)
        res = torch.empty((m, h, w), dtype=torch.float32, device=dev) if want_res else None
        stats = torch.empty((m, MM_NSTATS), dtype=torch.int64, device=dev) if want_stats else None
        self.motion_mask_ptr(flow.data_ptr(), view, m, w, h, xform.data_ptr(), occ.data_ptr() if occ is not None else 0,
                             float(thr), float(rel), int(radius), code.data_ptr(), res.data_ptr() if want_res else 0,
                             stats.data_ptr() if want_stats else 0, torch.cuda.current_stream(dev).cuda_stream)
        out = [code] + ([res] if want_res else []) + ([stats] if want_stats else [])
        return tuple(out) if len(out) > 1 else code

    def run_sequence_motion_mask_ptr(self, frames_ptr: int, nframes: int, width: int, height: int, p: Params, model: int,
                                     step: int, tau: float, iters: int, thr: float, rel: float, radius: int,
                                     code_ptr: int = 0, res_ptr: int = 0, stats_ptr: int = 0, xform_ptr: int = 0,
                                     support_ptr: int = 0, occ_ptr: int = 0, fb: bool = False, alpha: float = 0.01,
                                     beta: float = 0.5, stream: int = 0) -> None:
        """``ofdis_run_sequence_motion_mask_u8`` on raw device pointers, asynchronous on `stream`: frames u8
        [nframes, h, w, noc] -> the masks (0: that output is not wanted)."""
        check(lib().ofdis_run_sequence_motion_mask_u8(self._h, frames_ptr or None, nframes, width, height, C.byref(p),
                                                      model, step, tau, iters, int(bool(fb)), alpha, beta, thr, rel,
                                                      radius, code_ptr or None, res_ptr or None, stats_ptr or None,
                                                      xform_ptr or None, support_ptr or None, occ_ptr or None,
                                                      stream or None), "ofdis_run_sequence_motion_mask_u8")

    def run_sequence_motion_mask(self, frames, p: Params, model: int = MOTION_SIMILARITY, step: int = 16,
                                 tau: float = 2.0, iters: int = 4, fb: bool = False, alpha: float = 0.01,
                                 beta: float = 0.5, thr: float = 1.0, rel: float = 0.05, radius: int = 1,
                                 want_res: bool = False, want_stats: bool = False, want_xform: bool = False,
                                 want_occ: bool = False):
        """The flows of a video, its camera motion and the moving-object masks in one call: torch.uint8 CUDA tensor
        [T, h, w] or [T, h, w, noc] -> code uint8 [T - 1, h, w].  Bit for bit ``motion_mask(F, fit_motion(F, B if fb
        else None, ...), occ_fw if fb else None, ...)`` on ``run_sequence(frames, p, bidir=fb)``'s flows and masks --
        but the flows stay on their level grids and no full-resolution flow is written.  want_res adds float32
        [T - 1, h, w], want_stats int64 [T - 1, 12], want_xform (xform float64 [T - 1, 6], support int32 [T - 1]),
        want_occ (with fb) the forward occlusion planes uint8 [T - 1, h, w]."""
        import torch
        f4 = frames.unsqueeze(-1) if frames.dim() == 3 else frames
        if f4.dim() != 4 or f4.shape[-1] != p.noc or f4.dtype != torch.uint8 or not f4.is_cuda:
            raise ValueError("expected a uint8 CUDA tensor with noc channels")
        t, h, w, _ = f4.shape
        if t < 2:
            raise OfdisError(ERR_INVALID_ARGUMENT, "run_sequence_motion_mask: a video needs two frames or more")
        if want_occ and not fb:
            raise OfdisError(ERR_INVALID_ARGUMENT, "run_sequence_motion_mask: want_occ needs fb")
        _motion_checks("run_sequence_motion_mask", w, h, model, step, tau, iters)
        _mask_checks("run_sequence_motion_mask", t - 1, thr, rel, radius, w, h)
        f4 = f4.contiguous()
        dev = f4.device
        code = torch.empty((t - 1, h, w), dtype=torch.uint8, device=dev)
        res = torch.empty((t - 1, h, w), dtype=torch.float32, device=dev) if want_res else None
        stats = torch.empty((t - 1, MM_NSTATS), dtype=torch.int64, device=dev) if want_stats else None
        xform = torch.empty((t - 1, 6), dtype=torch.float64, device=dev) if want_xform else None
        support = torch.empty((t - 1,), dtype=torch.int32, device=dev) if want_xform else None
        occ = torch.empty((t - 1, h, w), dtype=torch.uint8, device=dev) if want_occ else None
        self.run_sequence_motion_mask_ptr(f4.data_ptr(), t, w, h, p, int(model), int(step), float(tau), int(iters),
                                          float(thr), float(rel), int(radius), code.data_ptr(),
                                          res.data_ptr() if want_res else 0, stats.data_ptr() if want_stats else 0,
                                          xform.data_ptr() if want_xform else 0, support.data_ptr() if want_xform else 0,
                                          occ.data_ptr() if want_occ else 0, fb, alpha, beta,
                                          torch.cuda.current_stream(dev).cuda_stream)
        out = ([code] + ([res] if want_res else []) + ([stats] if want_stats else [])
               + ([xform, support] if want_xform else []) + ([occ] if want_occ else []))
        return tuple(out) if len(out) > 1 else code

    def run_sequence_motion_mask_host(self, frames: np.ndarray, p: Params, model: int = MOTION_SIMILARITY,
                                      step: int = 16, tau: float = 2.0, iters: int = 4, fb: bool = False,
                                      alpha: float = 0.01, beta: float = 0.5, thr: float = 1.0, rel: float = 0.05,
                                      radius: int = 1, want_res: bool = False, want_stats: bool = False,
                                      want_xform: bool = False, want_occ: bool = False):
        """run_sequence_motion_mask on a numpy u8 array [T, h, w] or [T, h, w, noc]; synchronous."""
        f4 = np.ascontiguousarray(frames[..., None] if frames.ndim == 3 else frames, np.uint8)
        if f4.ndim != 4 or f4.shape[-1] != p.noc:
            raise ValueError("expected a uint8 array with noc channels")
        t, h, w = f4.shape[:3]
        if t < 2:
            raise OfdisError(ERR_INVALID_ARGUMENT, "run_sequence_motion_mask_host: a video needs two frames or more")
        if want_occ and not fb:
            raise OfdisError(ERR_INVALID_ARGUMENT, "run_sequence_motion_mask_host: want_occ needs fb")
        _motion_checks("run_sequence_motion_mask_host", w, h, model, step, tau, iters)
        _mask_checks("run_sequence_motion_mask_host", t - 1, thr, rel, radius, w, h)
        code = np.empty((t - 1, h, w), np.uint8)
        res = np.empty((t - 1, h, w), _f32) if want_res else None
        stats = np.empty((t - 1, MM_NSTATS), np.int64) if want_stats else None
        xform = np.empty((t - 1, 6), np.float64) if want_xform else None
        support = np.empty((t - 1,), np.int32) if want_xform else None
        occ = np.empty((t - 1, h, w), np.uint8) if want_occ else None
        check(lib().ofdis_run_sequence_motion_mask_u8_host(
            self._h, f4.ctypes.data, t, w, h, C.byref(p), int(model), int(step), float(tau), int(iters), int(bool(fb)),
            alpha, beta, float(thr), float(rel), int(radius), code.ctypes.data, res.ctypes.data if want_res else None,
            stats.ctypes.data if want_stats else None, xform.ctypes.data if want_xform else None,
            support.ctypes.data if want_xform else None, occ.ctypes.data if want_occ else None),
            "ofdis_run_sequence_motion_mask_u8_host")
        out = ([code] + ([res] if want_res else []) + ([stats] if want_stats else [])
               + ([xform, support] if want_xform else []) + ([occ] if want_occ else []))
        return tuple(out) if len(out) > 1 else code

    def flow_error_ptr(self, flow_ptr: int, view: FlowView, gt_ptr: int, n: int, width: int, height: int,
                       stats_ptr: int, mask_ptr: int = 0, mask_eq: int = -1, err_ptr: int = 0, hist_ptr: int = 0,
                       stream: int = 0) -> None:
        """``ofdis_flow_error`` on raw device pointers (0: no mask / that output is not wanted)."""
        check(lib().ofdis_flow_error(self._h, flow_ptr or None, None if view is None else C.byref(view), gt_ptr or None,
                                     mask_ptr or None, mask_eq, n, width, height, stats_ptr or None, err_ptr or None,
                                     hist_ptr or None, stream or None), "ofdis_flow_error")

    def flow_error(self, flow, gt, mask=None, mask_eq: int = -1, grid: str = "full", p: Optional[Params] = None,
                   size=None, want_err: bool = False, want_hist: bool = False, layout: str = "nhwc"):
        """n flow fields scored against ground truth on the device (the definition is in ofdis.h).  flow: any output of
        ``run`` -- float32 or float16, layout "nhwc" / "nchw", grid "full" or "level" (float32 "nhwc" grids; needs `p`
        and size = (width, height)).  gt: torch.float32 CUDA tensor [n, h, w, 2], unknown pixels marked by |value| >
        1e9 or NaN.  mask: torch.uint8 [n, h, w] or None; mask_eq -1 keeps its nonzero pixels, 0 .. 255 the pixels
        equal to it.  Returns stats, torch.float64 [n, 16] (indices ``FE_COUNT`` .. ``FE_S2_SUM``; ``error_summary``
        reads them); with want_err also the error map float32 [n, h, w] (+inf: a non-finite estimate, -1: not scored),
        with want_hist also uint32 counts [n, 1024] in bins of 1/16 px (as torch.int32 bits)."""
        import torch
        if not (flow.is_cuda and gt.is_cuda) or flow.dim() != 4 or gt.dim() != 4 or gt.dtype != torch.float32 or gt.shape[-1] != 2:
            raise ValueError("expected a CUDA flow tensor of four dimensions and a float32 CUDA truth [n, h, w, 2]")
        fmt = out_format(flow.dtype, layout, grid)
        n, h, w, _ = gt.shape
        if grid == "level":
            if p is None or size is None:
                raise OfdisError(ERR_INVALID_ARGUMENT, 'flow_error: grid="level" needs the parameters the flow was '
                                 "computed with and the frame size")
            if (int(size[0]), int(size[1])) != (w, h):
                raise ValueError(f"size {tuple(size)} is not the truth's {(w, h)}")
            g = out_geometry(p, w, h, False, flow.dtype, layout, grid)
            view = FlowView(fmt.dtype, fmt.layout, fmt.grid, g["out_w"], g["out_h"], g["cell"], g["off_x"], g["off_y"])
        else:
            view = FlowView(fmt.dtype, fmt.layout, fmt.grid, w, h, 1, 0, 0)
        want = (n, 2, view.gh, view.gw) if fmt.layout else (n, view.gh, view.gw, 2)
        if tuple(flow.shape) != want:
            raise ValueError(f"flow has shape {tuple(flow.shape)}, expected {want}")
        mask = _error_mask(mask, (n, h, w), mask_eq, gt.device)
        flow, gt = flow.contiguous(), gt.contiguous()
        stats, err, hist = _error_outputs(n, h, w, want_err, want_hist, gt.device)
        self.flow_error_ptr(flow.data_ptr(), view, gt.data_ptr(), n, w, h, stats.data_ptr(),
                            mask.data_ptr() if mask is not None else 0, int(mask_eq), err.data_ptr() if want_err else 0,
                            hist.data_ptr() if want_hist else 0, torch.cuda.current_stream(gt.device).cuda_stream)
        res = [stats] + ([err] if want_err else []) + ([hist] if want_hist else [])
        return tuple(res) if len(res) > 1 else stats

    def run_error_ptr(self, a_ptr: int, b_ptr: int, gt_ptr: int, n: int, width: int, height: int, p: Params,
                      stats_ptr: int, mask_ptr: int = 0, mask_eq: int = -1, err_ptr: int = 0, hist_ptr: int = 0,
                      stream: int = 0) -> None:
        """``ofdis_run_error_u8`` on raw device pointers, asynchronous on `stream` (0: no mask / output not wanted)."""
        check(lib().ofdis_run_error_u8(self._h, a_ptr or None, b_ptr or None, gt_ptr or None, mask_ptr or None, mask_eq,
                                       n, width, height, C.byref(p), stats_ptr or None, err_ptr or None,
                                       hist_ptr or None, stream or None), "ofdis_run_error_u8")

    def run_error(self, a, b, p: Params, gt, mask=None, mask_eq: int = -1, want_err: bool = False,
                  want_hist: bool = False):
        """Flow and its error in one call: torch.uint8 CUDA tensors [n, h, w] or [n, h, w, 3] and the truth as for
        ``flow_error`` -> what ``flow_error(run(a, b, p), gt, ...)`` returns, bit for bit, but the flow stays on its
        level grid: no full-resolution flow is written."""
        import torch
        a4, b4 = (a.unsqueeze(-1), b.unsqueeze(-1)) if a.dim() == 3 else (a, b)
        if (a4.dim() != 4 or a4.shape[-1] != p.noc or a4.dtype != torch.uint8 or a.shape != b.shape
                or b.dtype != torch.uint8 or not (a.is_cuda and b.is_cuda)):
            raise ValueError("expected two uint8 CUDA tensors of one shape with noc channels")
        n, h, w, _ = a4.shape
        if not gt.is_cuda or gt.dtype != torch.float32 or tuple(gt.shape) != (n, h, w, 2):
            raise ValueError(f"expected a float32 CUDA truth of shape {(n, h, w, 2)}")
        mask = _error_mask(mask, (n, h, w), mask_eq, a.device)
        a4, b4, gt = a4.contiguous(), b4.contiguous(), gt.contiguous()
        stats, err, hist = _error_outputs(n, h, w, want_err, want_hist, a.device)
        self.run_error_ptr(a4.data_ptr(), b4.data_ptr(), gt.data_ptr(), n, w, h, p, stats.data_ptr(),
                           mask.data_ptr() if mask is not None else 0, int(mask_eq), err.data_ptr() if want_err else 0,
                           hist.data_ptr() if want_hist else 0, torch.cuda.current_stream(a.device).cuda_stream)
        res = [stats] + ([err] if want_err else []) + ([hist] if want_hist else [])
        return tuple(res) if len(res) > 1 else stats

    def run_error_host(self, a: np.ndarray, b: np.ndarray, p: Params, gt: np.ndarray, mask=None, mask_eq: int = -1,
                       want_err: bool = False, want_hist: bool = False):
        """run_error on numpy arrays; synchronous.  Images as for ``run_warp_host``; gt float32 [n, h, w, 2] ([h, w, 2]
        for a single pair), mask u8 [n, h, w] or None.  stats is [n, 16], err [n, h, w], hist uint32 [n, 1024]."""
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        if a.shape != b.shape or a.ndim < 2 or a.ndim > 4:
            raise ValueError("expected two uint8 arrays of one shape")
        channels = a.ndim == 4 or (a.ndim == 3 and a.shape[-1] == p.noc and (p.noc == 3 or a.shape[-1] == 1))
        if channels and a.shape[-1] != p.noc:
            raise ValueError("expected noc channels")
        h, w = a.shape[-3:-1] if channels else a.shape[-2:]
        n = 1 if a.ndim == (3 if channels else 2) else a.shape[0]
        gt = np.ascontiguousarray(gt, _f32)
        if gt.size != n * h * w * 2:
            raise ValueError(f"expected a truth of shape {(n, h, w, 2)}")
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.uint8)
            if mask.size != n * h * w:
                raise ValueError(f"expected a mask of shape {(n, h, w)}")
        stats = np.empty((n, 16), np.float64)
        err = np.empty((n, h, w), _f32) if want_err else None
        hist = np.empty((n, 1024), np.uint32) if want_hist else None
        check(lib().ofdis_run_error_u8_host(self._h, a.ctypes.data, b.ctypes.data, gt.ctypes.data,
                                            mask.ctypes.data if mask is not None else None, int(mask_eq), n, w, h,
                                            C.byref(p), stats.ctypes.data, err.ctypes.data if want_err else None,
                                            hist.ctypes.data if want_hist else None), "ofdis_run_error_u8_host")
        res = [stats] + ([err] if want_err else []) + ([hist] if want_hist else [])
        return tuple(res) if len(res) > 1 else stats

    def pyramid_host(self, img: np.ndarray, p: Params, imgpadding: Optional[int] = None):
        """Device pyramid of one u8 image -> {scale: (img, dx, dy)} padded float arrays."""
        h, w = img.shape[:2]
        pad = p.p_samp_s if imgpadding is None else imgpadding
        d = 1 << p.sc_f
        wp, hp = w + ((d - w % d) % d), h + ((d - h % d) % d)
        lev = {s: tuple(np.zeros(((hp >> s) + 2 * pad, (wp >> s) + 2 * pad, p.noc), _f32) for _ in range(3))
               for s in range(p.sc_l, p.sc_f + 1)}
        ptrs = []
        for k in range(3):
            arr = (C.c_void_p * 32)()
            for s, v in lev.items():
                arr[s] = v[k].ctypes.data
            ptrs.append(arr)
        img = np.ascontiguousarray(img, np.uint8)
        check(lib().ofdis_pyramid_u8_host(self._h, img.ctypes.data, w, h, C.byref(p), pad, *ptrs), "pyramid")
        return lev

    def set_capture(self, dis: Optional[dict], tv: Optional[dict], nscales: int = 32):
        """Capture frame 0's flow after aggregation / after TV per scale into the given arrays."""
        d = (C.c_void_p * nscales)()
        t = (C.c_void_p * nscales)()
        self._keep = []
        for src, dst in ((dis or {}, d), (tv or {}, t)):
            for s, a in src.items():
                assert a.dtype == _f32 and a.flags.c_contiguous
                dst[s] = a.ctypes.data
                self._keep.append(a)
        check(lib().ofdis_context_set_stage_capture(self._h, d, t, nscales), "capture")

    def set_option(self, key: str, value: int):
        check(lib().ofdis_context_set_option(self._h, key.encode(), int(value)), f"option {key}")

    def enable_kernel_timing(self, on: bool = True):
        check(lib().ofdis_context_enable_kernel_timing(self._h, int(on)), "timing")

    def kernel_time(self, name: str):
        ms, cnt = C.c_double(), C.c_long()
        check(lib().ofdis_context_kernel_time(self._h, name.encode(), C.byref(ms), C.byref(cnt)), "kernel_time")
        return ms.value, cnt.value


def out_geometry(p: Params, width: int, height: int, with_init: bool = False, dtype="float32", layout: str = "nhwc",
                 grid: str = "full") -> dict:
    """``ofdis_out_geometry``: the output grid of one pair in a format -- out_w, out_h, off_x, off_y, cell and
    bytes_per_pair.  Level cell (X, Y) covers the original pixels [X * cell - off_x, (X + 1) * cell - off_x) x
    [Y * cell - off_y, (Y + 1) * cell - off_y); the level grid is not cropped."""
    fmt = out_format(dtype, layout, grid)
    v = [C.c_int() for _ in range(5)]
    nb = C.c_size_t()
    check(lib().ofdis_out_geometry(C.byref(p), width, height, int(bool(with_init)), C.byref(fmt),
                                   *[C.byref(x) for x in v], C.byref(nb)), "ofdis_out_geometry")
    return dict(zip(("out_w", "out_h", "off_x", "off_y", "cell"), (x.value for x in v)), bytes_per_pair=nb.value)


def _out_shape(p: Params, width: int, height: int, n: int, with_init: bool, fmt: OutFormat):
    ow, oh = C.c_int(), C.c_int()
    check(lib().ofdis_out_geometry(C.byref(p), width, height, int(with_init), C.byref(fmt), C.byref(ow), C.byref(oh),
                                   None, None, None, None), "ofdis_out_geometry")
    return (n, p.nop, oh.value, ow.value) if fmt.layout else (n, oh.value, ow.value, p.nop)


def _times(t) -> np.ndarray:
    """The times of an interpolation call, a scalar or a sequence, as the float32 array the library copies."""
    return np.ascontiguousarray(np.atleast_1d(np.asarray(t, _f32)).reshape(-1))


def _tfilter_checks(what: str, sigma, out_dtype, dtypes) -> None:
    """What the filtering calls refuse of sigma and out_dtype, before any library call (ofdis_tfilter_u8's rules)."""
    s = float(sigma)
    if not (np.isfinite(s) and 1.0 / 1024.0 <= s <= 65536.0):
        raise OfdisError(ERR_INVALID_ARGUMENT, f"{what}: sigma {sigma!r} is not in [1/1024, 65536]")
    if out_dtype not in dtypes:
        raise OfdisError(ERR_INVALID_ARGUMENT, f"{what}: out_dtype {out_dtype!r}")


def _tfilter_radius_checks(what: str, radius, fb, alpha, beta) -> None:
    """What the radius calls refuse beyond _tfilter_checks, before any library call (ofdis_tfilter_radius_u8's rules)."""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= 4:
        raise OfdisError(ERR_INVALID_ARGUMENT, f"{what}: radius {radius!r} is not an integer in [1, 4]")
    if fb and not (np.isfinite(float(alpha)) and np.isfinite(float(beta)) and float(alpha) >= 0 and float(beta) >= 0):
        raise OfdisError(ERR_INVALID_ARGUMENT, f"{what}: thresholds alpha {alpha!r}, beta {beta!r}")


def pixel_grid(width: int, height: int, step: int = 1) -> np.ndarray:
    """The pixel centres (x, y) of every `step`-th column and row of a width x height frame, row-major: float32 [N, 2],
    the points a dense tracking call starts from."""
    if width < 1 or height < 1 or step < 1:
        raise ValueError("pixel_grid needs a positive size and step")
    xs, ys = np.arange(0, width, step, dtype=_f32), np.arange(0, height, step, dtype=_f32)
    return np.ascontiguousarray(np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2))


def fit_lattice(width: int, height: int, step: int = 16) -> np.ndarray:
    """The pixels (x, y) at which ``fit_motion`` samples a width x height field, row-major: int32 [ns, 2] -- columns
    step // 2 + i * step below width, rows likewise.  Raises OfdisError(INVALID_ARGUMENT) for a size or step the
    library refuses (a first sample outside the frame, more than FIT_MAX_SAMPLES samples)."""
    width, height, step = int(width), int(height), int(step)
    if width < 1 or height < 1 or step < 1 or step // 2 > min(width, height) - 1:
        raise OfdisError(ERR_INVALID_ARGUMENT, f"fit_lattice: size {(width, height)} at step {step}")
    half = step // 2
    xs, ys = np.arange(half, width, step, dtype=np.int32), np.arange(half, height, step, dtype=np.int32)
    if xs.size * ys.size > FIT_MAX_SAMPLES:
        raise OfdisError(ERR_INVALID_ARGUMENT, f"fit_lattice: {xs.size * ys.size} samples, the most is {FIT_MAX_SAMPLES}")
    return np.ascontiguousarray(np.stack(np.meshgrid(xs, ys), axis=-1).reshape(-1, 2))


def _motion_checks(what: str, width: int, height: int, model, step, tau, iters) -> int:
    """What the fitting calls refuse of their scalars, before any library call (ofdis_fit_motion's rules); returns the
    number of samples."""
    if model not in (MOTION_TRANSLATION, MOTION_SIMILARITY):
        raise OfdisError(ERR_INVALID_ARGUMENT, f"{what}: model {model!r}")
    t = float(tau)
    if not (np.isfinite(t) and 1.0 / 1024.0 <= t <= 65536.0):
        raise OfdisError(ERR_INVALID_ARGUMENT, f"{what}: tau {tau!r} is not in [1/1024, 65536]")
    if int(iters) != iters or not 0 <= iters <= 16:
        raise OfdisError(ERR_INVALID_ARGUMENT, f"{what}: iters {iters!r} is not in 0..16")
    if int(step) != step:
        raise OfdisError(ERR_INVALID_ARGUMENT, f"{what}: step {step!r}")
    return fit_lattice(width, height, step).shape[0]


def _path_checks(what: str, m: int, radius, zoom, width: int, height: int) -> None:
    """What the path calls refuse of their scalars, before any library call (ofdis_smooth_path's rules)."""
    if m < 1 or width < 1 or height < 1:
        raise OfdisError(ERR_INVALID_ARGUMENT, f"{what}: {m} transforms of a {width} x {height} frame")
    if int(radius) != radius or not 0 <= radius <= 256:
        raise OfdisError(ERR_INVALID_ARGUMENT, f"{what}: radius {radius!r} is not in 0..256")
    z = float(zoom)
    if not (np.isfinite(z) and 1.0 <= z <= 16.0):
        raise OfdisError(ERR_INVALID_ARGUMENT, f"{what}: zoom {zoom!r} is not in [1, 16]")


def _mask_checks(what: str, m: int, thr, rel, radius, width: int, height: int) -> None:
    """What the mask calls refuse of their scalars, before any library call (ofdis_motion_mask's rules)."""
    if m < 1 or width < 1 or height < 1 or width * height >= 2 ** 31:
        raise OfdisError(ERR_INVALID_ARGUMENT, f"{what}: {m} fields of a {width} x {height} frame")
    t, r = float(thr), float(rel)
    if not (np.isfinite(t) and 0.0 <= t <= 65536.0):
        raise OfdisError(ERR_INVALID_ARGUMENT, f"{what}: thr {thr!r} is not in [0, 65536]")
    if not (np.isfinite(r) and 0.0 <= r <= 16.0):
        raise OfdisError(ERR_INVALID_ARGUMENT, f"{what}: rel {rel!r} is not in [0, 16]")
    if int(radius) != radius or not 0 <= radius <= 4:
        raise OfdisError(ERR_INVALID_ARGUMENT, f"{what}: radius {radius!r} is not in 0..4")


def motion_summary(stats) -> list:
    """The readable figures of ``motion_mask`` / ``run_sequence_motion_mask`` stats ([m, 12] or [12]; numpy, or a
    tensor copied to the host): one dict per pair with static / moving / unknown (the counts of codes 0, 1, 2),
    moving_share = moving / (static + moving) (NaN when every pixel is unknown), raw (the count before the clean-up),
    bbox = (xmin, ymin, xmax, ymax) of the moving pixels and centroid = (mean x, mean y), both None when none moves."""
    s = np.asarray(stats.detach().cpu().numpy() if hasattr(stats, "detach") else stats, np.int64).reshape(-1, MM_NSTATS)
    out = []
    for r in s:
        n0, n1, n2 = int(r[0]), int(r[1]), int(r[2])
        out.append({"static": n0, "moving": n1, "unknown": n2, "raw": int(r[7]),
                    "moving_share": n1 / (n0 + n1) if n0 + n1 > 0 else float("nan"),
                    "bbox": tuple(int(v) for v in r[3:7]) if n1 else None,
                    "centroid": (int(r[8]) / n1, int(r[9]) / n1) if n1 else None})
    return out


def write_pnm(path: str, pixels: np.ndarray) -> None:
    """Binary PGM (u8 [h, w] or [h, w, 1]) / PPM (u8 [h, w, 3] in BGR order, written as RGB)."""
    pixels = np.ascontiguousarray(pixels, np.uint8)
    noc = 1 if pixels.ndim == 2 else pixels.shape[2]
    check(lib().ofdis_write_pnm(path.encode(), pixels.ctypes.data, pixels.shape[1], pixels.shape[0], noc), "write_pnm")


def kernel_names():
    return lib().ofdis_kernel_names().decode().split(",")


def kernel_names_ext():
    """The timer names added after the closed list of ``kernel_names``, in slot order."""
    return lib().ofdis_kernel_names_ext().decode().split(",")


def kernel_names_all():
    """Every timer name in slot order: ``kernel_names``, ``kernel_names_ext`` and the names later features add (an
    open list: look names up in it, do not count it)."""
    return lib().ofdis_kernel_names_all().decode().split(",")


def _error_mask(mask, shape, mask_eq, device):
    """The mask of an error call checked: torch.uint8 of `shape` on `device`, contiguous; mask_eq in -1 .. 255."""
    import torch
    if not -1 <= int(mask_eq) <= 255:
        raise OfdisError(ERR_INVALID_ARGUMENT, f"mask_eq {mask_eq!r} is outside -1 .. 255")
    if mask is None:
        return None
    if mask.dtype != torch.uint8 or tuple(mask.shape) != tuple(shape) or mask.device != device:
        raise ValueError(f"expected a uint8 mask of shape {tuple(shape)} on the truth's device")
    return mask.contiguous()


def _error_outputs(n: int, h: int, w: int, want_err: bool, want_hist: bool, device):
    import torch
    stats = torch.empty((n, FE_NSTATS), dtype=torch.float64, device=device)
    err = torch.empty((n, h, w), dtype=torch.float32, device=device) if want_err else None
    hist = torch.empty((n, FE_BINS), dtype=torch.int32, device=device) if want_hist else None  # (uint32 bits)
    return stats, err, hist


def error_summary(stats) -> dict:
    """The readable figures of ``flow_error`` / ``run_error`` stats ([n, 16] or [16]; numpy, or a tensor copied to the
    host).  Returns {"pairs": [one dict per pair], "pooled": dict}; pooling adds the pairs' sums, then their counts, in
    ascending pair order.  Each dict: count, nonfinite, epe = Se / (count - nonfinite), r1 / r3 / r5 (the shares of
    scored pixels with an error above 1, 3, 5 px) and fl (KITTI's outlier share) as fractions of count, epe_s0_10 /
    epe_s10_40 / epe_s40 (Sintel's speed classes), max.  A figure whose denominator is 0 is NaN."""
    s = np.asarray(stats.detach().cpu().numpy() if hasattr(stats, "detach") else stats, np.float64).reshape(-1, FE_NSTATS)

    def one(r):
        def div(a, b):
            return float(a) / float(b) if b > 0 else float("nan")
        return {"count": int(r[FE_COUNT]), "nonfinite": int(r[FE_NONFINITE]),
                "epe": div(r[FE_SUM], r[FE_COUNT] - r[FE_NONFINITE]),
                "r1": div(r[FE_GT1], r[FE_COUNT]), "r3": div(r[FE_GT3], r[FE_COUNT]), "r5": div(r[FE_GT5], r[FE_COUNT]),
                "fl": div(r[FE_FL], r[FE_COUNT]),
                "epe_s0_10": div(r[FE_S0_SUM], r[FE_S0_COUNT]), "epe_s10_40": div(r[FE_S1_SUM], r[FE_S1_COUNT]),
                "epe_s40": div(r[FE_S2_SUM], r[FE_S2_COUNT]), "max": float(r[FE_MAX])}

    pooled = np.zeros(FE_NSTATS, np.float64)
    for r in s:  # ascending pair order: the pooled sums are a function of the stats alone
        pooled = pooled + r
    pooled[FE_MAX] = s[:, FE_MAX].max() if len(s) else 0.0
    return {"pairs": [one(r) for r in s], "pooled": one(pooled)}


def error_percentile(hist, q: float) -> float:
    """The upper edge, in pixels, of the histogram bin holding the q-quantile (0 < q <= 1) of the scored errors: 1/16 px
    resolution.  hist: [1024] or [n, 1024] counts (pooled over the pairs).  The last bin is open (63.9375 px and up, and
    every non-finite estimate): its edge is +inf.  NaN for an empty histogram."""
    if not 0.0 < q <= 1.0:
        raise ValueError(f"q = {q!r} is outside (0, 1]")
    h = np.asarray(hist.detach().cpu().numpy() if hasattr(hist, "detach") else hist)
    h = h.view(np.uint32) if h.dtype == np.int32 else h
    h = h.reshape(-1, FE_BINS).astype(np.uint64).sum(axis=0)
    total = int(h.sum())
    if total == 0:
        return float("nan")
    rank = max(int(np.ceil(q * total)), 1)  # the rank-th smallest error, 1-based
    b = int(np.searchsorted(np.cumsum(h), rank, side="left"))
    return float("inf") if b >= FE_BINS - 1 else (b + 1) / 16.0


def max_frames_per_launch(p: Params, width: int, height: int) -> int:
    """Frames one launch of the refinement kernels takes at this size (32-bit plane-group offsets)."""
    v = C.c_int()
    check(lib().ofdis_max_frames_per_launch(C.byref(p), width, height, C.byref(v)), "max_frames_per_launch")
    return v.value


def algorithmic_bytes(p: Params, width: int, height: int, kernel: str) -> float:
    v = C.c_double()
    check(lib().ofdis_algorithmic_bytes(C.byref(p), width, height, kernel.encode(), C.byref(v)), "bytes")
    return v.value


def tfilter_radius_bytes(p: Params, width: int, height: int, radius: int, level: bool = False, f32: bool = False) -> float:
    """``ofdis_tfilter_radius_bytes``: the byte model of the temporal filter over `radius` frames per interior output
    frame, on full-resolution float32 views or (level) on level grids, with a u8 or (f32) a float32 picture."""
    v = C.c_double()
    check(lib().ofdis_tfilter_radius_bytes(C.byref(p), width, height, int(bool(level)), int(radius),
                                           IMG_F32 if f32 else IMG_U8, C.byref(v)), "ofdis_tfilter_radius_bytes")
    return v.value


__all__ = ["OFClass", "Context", "Params", "oppoint", "params_from_strings", "validate", "synth_pair", "synth_shift_pair",
           "write_flo", "write_pfm", "write_pnm", "read_flo", "read_image", "auto_first_scale", "kernel_names", "algorithmic_bytes",
           "tfilter_radius_bytes", "kernel_names_ext", "kernel_names_all", "error_summary", "error_percentile",
           "motion_summary",
           "max_frames_per_launch", "out_geometry", "pixel_grid", "fit_lattice",
           "MODE_OF", "MODE_DE", "MOTION_TRANSLATION", "MOTION_SIMILARITY"]

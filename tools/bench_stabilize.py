#!/usr/bin/env python3
"""The fused stabilising call against its compositions.

End to end at 1920 x 1080, op-point 2, intensity frames, a video of 33 frames (32 pairs); similarity fit at step 16
(120 x 67 samples per pair), tau 2, 4 re-solves; path radius 8, zoom 1; u8 output with the valid bytes; with and without
the forward-backward check (use_fb):
  fused    = one Context.run_sequence_stabilize_ptr call (level grids in the context's buffer, then fit_motion_level,
             smooth_path and warp_affine: three launches, the check inside the fit at its samples alone);
  composed = run_sequence_ptr writing the full float32 forward field (with use_fb also the backward one, no masks) +
             fit_motion_ptr + smooth_path_ptr + warp_affine_ptr on them, on one context: the same bits;
  torch    = the same run_sequence_ptr (forward field) + a torch composition: torch.linalg.lstsq on the same lattice in
             float64 (plain least squares: no re-solves, no check), the path by 3 x 3 products, a triangular window and
             torch.linalg.inv, then affine_grid and grid_sample (bilinear, border padding, align_corners) -- for time
             only, its fit and its rounding differ.
All are timed in the same process in alternating blocks (host clock around calls that end in a device synchronise) after
warming all; fused and composed are compared bit for bit first.  `aa_spread` is the fused call timed against itself
(twice per block): what the box cannot tell apart.  `torch_stab_ms` is the torch composition alone on a flow already
there.

Kernel: the launch times of "fit_motion_level", "fit_motion", "smooth_path" and "warp_affine" from the library's kernel
timer (HIP events around the launch, eager issue) with ofdis_algorithmic_bytes per pair / frame, the warp's as a fraction
of the HBM peak.  No counter pass is taken here.

    python tools/bench_stabilize.py [--frames 33] [--blocks 10] [--calls 50] [--torch-calls 2] [--out FILE]

Needs an MI355X; prints one JSON line per result.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, OP = 1920, 1080, 2
STEP, TAU, ITERS, RADIUS, ZOOM = 16, 2.0, 4, 8, 1.0
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=33)
    ap.add_argument("--blocks", type=int, default=10, help="alternating timed blocks per way")
    ap.add_argument("--calls", type=int, default=50, help="calls per block")
    ap.add_argument("--torch-calls", type=int, default=2, help="calls per block of the two torch ways (about half a second each)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import of_dis_amd as od
    if not torch.cuda.is_available():
        raise SystemExit("bench_stabilize.py needs a GPU")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    T = args.frames
    m = T - 1
    # frames a0, b0, a1, b1, ... of eight distinct synthetic pairs, repeated (tools/bench_track.py's video)
    distinct = [im[..., 0] for f in range(8) for im in od.synth_pair(W, H, 1, f, od.MODE_OF)]
    fr = torch.from_numpy(np.stack([distinct[f % len(distinct)] for f in range(T)])).cuda()
    p = od.oppoint(OP, W, od.MODE_OF, 1)
    p.verbosity = 0
    s = torch.cuda.current_stream().cuda_stream
    view = od.FlowView(0, 0, 0, W, H, 1, 0, 0)
    geo = od.out_geometry(p, W, H, False, "float32", "nhwc", "level")
    lat = od.fit_lattice(W, H, STEP)
    ns = lat.shape[0]
    fw = torch.empty((m, H, W, 2), dtype=torch.float32, device="cuda")
    bw = torch.empty_like(fw)
    emit({"what": "memory", "frames": T, "pairs": m, "samples_per_pair": ns, "pixels_per_pair": W * H,
          "level_grid": [geo["out_w"], geo["out_h"], geo["cell"]],
          "fused_flow_bytes_per_pair": {"no_fb": geo["bytes_per_pair"], "fb": 2 * geo["bytes_per_pair"]},
          "composed_flow_bytes_per_pair": {"no_fb": W * H * 8, "fb": 2 * W * H * 8}, "mask_bytes": 0})
    pics = [torch.empty((T, H, W), dtype=torch.uint8, device="cuda") for _ in range(2)]
    valid = [torch.empty((T, H, W), dtype=torch.uint8, device="cuda") for _ in range(2)]
    xf = [torch.empty((m, 6), dtype=torch.float64, device="cuda") for _ in range(2)]
    corr = [torch.empty((T, 6), dtype=torch.float64, device="cuda") for _ in range(2)]
    sup = [torch.empty((m,), dtype=torch.int32, device="cuda") for _ in range(2)]
    # the torch composition's constants
    cx, cy = (W - 1) / 2, (H - 1) / 2
    lx = torch.from_numpy(lat[:, 0].astype(np.int64)).cuda()
    ly = torch.from_numpy(lat[:, 1].astype(np.int64)).cuda()
    xc, yc = lx.double() - cx, ly.double() - cy
    one, zero = torch.ones_like(xc), torch.zeros_like(xc)
    A = torch.cat([torch.stack([xc, -yc, one, zero], 1), torch.stack([yc, xc, zero, one], 1)])  # [2 ns, 4]
    tri = torch.tensor([RADIUS + 1 - abs(k) for k in range(-RADIUS, RADIUS + 1)], dtype=torch.float64, device="cuda")
    tri = tri / tri.sum()
    Nm = torch.tensor([[2 / (W - 1), 0, -1], [0, 2 / (H - 1), -1], [0, 0, 1]], dtype=torch.float64, device="cuda")
    Ni = torch.linalg.inv(Nm)
    frf = None

    def torch_stab():
        nonlocal frf
        if frf is None:
            frf = fr[:, None].float()
        smp = fw[:, ly, lx].double()                                  # [m, ns, 2]
        b = torch.cat([smp[..., 0], smp[..., 1]], 1)                   # [m, 2 ns]
        q = torch.linalg.lstsq(A.expand(m, -1, -1), b[..., None]).solution[..., 0]  # [m, 4]: p0 .. p3
        P = torch.zeros((m, 3, 3), dtype=torch.float64, device="cuda")
        P[:, 0, 0] = P[:, 1, 1] = 1 + q[:, 0]
        P[:, 0, 1], P[:, 1, 0] = -q[:, 1], q[:, 1]
        P[:, 0, 2] = q[:, 2] - (q[:, 0] * cx - q[:, 1] * cy)
        P[:, 1, 2] = q[:, 3] - (q[:, 1] * cx + q[:, 0] * cy)
        P[:, 2, 2] = 1
        chain = [torch.eye(3, dtype=torch.float64, device="cuda")]
        for j in range(m):
            chain.append(P[j] @ chain[-1])
        Cm = torch.stack(chain)                                        # [T, 3, 3]
        pad = torch.cat([Cm[:1].expand(RADIUS, -1, -1), Cm, Cm[-1:].expand(RADIUS, -1, -1)])
        S = (pad.unfold(0, 2 * RADIUS + 1, 1) * tri).sum(-1)           # [T, 3, 3]
        corr_t = Cm @ torch.linalg.inv(S)
        theta = (Nm @ corr_t @ Ni)[:, :2].float()
        grid = F.affine_grid(theta, (T, 1, H, W), align_corners=True)
        pic = F.grid_sample(frf, grid, mode="bilinear", padding_mode="border", align_corners=True)[:, 0]
        ok = (grid.abs() <= 1).all(-1)
        return pic.round().to(torch.uint8), ok.to(torch.uint8)

    for fb in (False, True):
        ctx = {k: od.Context(0) for k in ("fused", "composed")}

        def fused():
            ctx["fused"].run_sequence_stabilize_ptr(fr.data_ptr(), T, W, H, p, od.MOTION_SIMILARITY, STEP, TAU, ITERS, RADIUS,
                                                    ZOOM, od.IMG_U8, pics[0].data_ptr(), valid[0].data_ptr(), xf[0].data_ptr(),
                                                    corr[0].data_ptr(), sup[0].data_ptr(), fb, 0.01, 0.5, s)

        def flows(both):
            ctx["composed"].run_sequence_ptr(fr.data_ptr(), T, 1, W, H, p, fw.data_ptr(), 0, 0.01, 0.5,
                                             bw.data_ptr() if both else 0, 0, 0, stream=s)

        def composed():
            c = ctx["composed"]
            flows(fb)
            c.fit_motion_ptr(fw.data_ptr(), bw.data_ptr() if fb else 0, view, m, W, H, od.MOTION_SIMILARITY, STEP, TAU, ITERS,
                             xf[1].data_ptr(), sup[1].data_ptr(), 0, 0.01, 0.5, s)
            c.smooth_path_ptr(xf[1].data_ptr(), m, RADIUS, ZOOM, W, H, corr[1].data_ptr(), s)
            c.warp_affine_ptr(fr.data_ptr(), T, W, H, 1, corr[1].data_ptr(), od.IMG_U8, pics[1].data_ptr(),
                              valid[1].data_ptr(), s)

        def torch_way():
            flows(False)
            torch_stab()

        fused()
        composed()
        torch.cuda.synchronize()
        same = all(torch.equal(a[0], a[1]) for a in (pics, valid, sup)) and \
            all(torch.equal(a[0].view(torch.int64), a[1].view(torch.int64)) for a in (xf, corr))
        if not same:
            raise SystemExit(f"fb {fb}: fused and composed differ")
        tp, _ = torch_stab()
        close = float(((tp.int() - pics[0].int()).abs() <= 1).float().mean())
        ways = {"fused": fused, "fused_again": fused, "composed": composed, "torch": torch_way, "torch_stab": torch_stab}
        for fn in ways.values():
            fn()
        torch.cuda.synchronize()
        tm = {k: [] for k in ways}
        for _ in range(args.blocks):
            for k, fn in ways.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                calls = args.torch_calls if k.startswith("torch") else args.calls
                for _ in range(calls):
                    fn()
                torch.cuda.synchronize()
                tm[k].append((time.perf_counter() - t0) / calls * 1e3)
        med = {k: statistics.median(v) for k, v in tm.items()}
        rec = {"what": "end_to_end", "use_fb": fb, "frames": T, "step": STEP, "tau": TAU, "iters": ITERS, "radius": RADIUS,
               "zoom": ZOOM, "outputs_identical": same, "support_share": round(float(sup[0].float().mean()) / ns, 4),
               "valid_share": round(float(valid[0].float().mean()), 4), "torch_within_one_level": round(close, 4),
               "blocks": args.blocks, "calls_per_block": args.calls, "torch_calls_per_block": args.torch_calls, "aa_spread": round(med["fused_again"] / med["fused"], 4)}
        for k in ways:
            rec[k + "_ms"] = round(med[k], 4)
            rec[k + "_ms_min_max"] = [round(min(tm[k]), 4), round(max(tm[k]), 4)]
        rec["fused_over_composed"] = round(med["fused"] / med["composed"], 4)
        rec["fused_over_torch"] = round(med["fused"] / med["torch"], 4)
        emit(rec)

        # kernel timer (eager issue: a launch has the chip alone)
        reps = 5
        rec = {"what": "kernel", "use_fb": fb, "frames": T, "counter_pass": False}
        for key, fn, kernels in (("fused", fused, ("fit_motion_level", "smooth_path", "warp_affine")),
                                 ("composed", composed, ("fit_motion",))):
            c = ctx[key]
            c.enable_kernel_timing(True)
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            for kernel in kernels:
                ms, cnt = c.kernel_time(kernel)
                us = ms / cnt * 1e3
                per = od.algorithmic_bytes(p, W, H, kernel)
                model = per * (T if kernel == "warp_affine" else m)
                gbs = model / (us * 1e-6) / 1e9
                rec[kernel] = {"avg_launch_us": round(us, 2), "launches": cnt, "model_bytes": model, "gb_s": round(gbs, 1)}
                if kernel == "warp_affine":
                    rec[kernel].update(us_per_frame=round(us / T, 2), frac_hbm_peak=round(gbs / HBM_PEAK_GBS, 4))
                if kernel.startswith("fit_motion"):
                    rec[kernel].update(us_per_pair=round(us / m, 2), samples=ns * m)
            c.enable_kernel_timing(False)
        rec["fit_motion_level_over_fit_motion"] = round(rec["fit_motion_level"]["avg_launch_us"] / rec["fit_motion"]["avg_launch_us"], 3)
        emit(rec)
        for c in ctx.values():
            c.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The fused motion-mask call against its compositions.

End to end at 1920 x 1080, op-point 2, intensity frames, a video of 33 frames (32 pairs); similarity fit at step 16, tau
2, 4 re-solves; mask at thr 1, rel 0.05, radius 1, the codes alone as output; with and without the forward-backward
check (use_fb):
  fused    = one Context.run_sequence_motion_mask_ptr call (level grids in the context's buffer, then fit_motion_level,
             with use_fb one fb_check_level launch for the forward plane, and motion_mask_level);
  composed = run_sequence_ptr writing the full float32 forward field (with use_fb also the backward one and the forward
             occlusion plane, which is its fb_check launch) + fit_motion_ptr + motion_mask_ptr on them, on one context:
             the same bits;
  torch    = the same run_sequence_ptr and fit_motion_ptr + a torch composition producing the same mask: the camera's
             field by broadcasting in float64, a subtraction, a norm and a threshold, and the binary median as two
             conv2d passes with a box of ones -- for time only, its rounding differs.
All are timed in the same process in alternating blocks (host clock around calls that end in a device synchronise) after
warming all; fused and composed are compared bit for bit first.  `aa_spread` is the fused call timed against itself
(twice per block): what the box cannot tell apart.  `torch_mask_ms` is the torch composition alone on a flow and
transforms already there.

Kernel: the launch times of "motion_mask" and "motion_mask_level" from the library's kernel timer (HIP events around the
launch, eager issue) against their byte models (the flow or its level grid, the code byte, plus the occlusion byte and
the four residual bytes where the call has them), as fractions of the HBM peak; beside them, in the same process,
"flow_error_level" and a float4 copy (torch's copy_ of 256 MiB, HIP events).  No counter pass is taken here.

    python tools/bench_motion_mask.py [--frames 33] [--blocks 10] [--calls 20] [--torch-calls 2] [--out FILE]

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
STEP, TAU, ITERS = 16, 2.0, 4
THR, REL, RADIUS = 1.0, 0.05, 1
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=33)
    ap.add_argument("--blocks", type=int, default=10, help="alternating timed blocks per way")
    ap.add_argument("--calls", type=int, default=20, help="calls per block")
    ap.add_argument("--torch-calls", type=int, default=2, help="calls per block of the two torch ways")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import of_dis_amd as od
    if not torch.cuda.is_available():
        raise SystemExit("bench_motion_mask.py needs a GPU")
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
    lview = od.FlowView(0, 0, 1, geo["out_w"], geo["out_h"], geo["cell"], geo["off_x"], geo["off_y"])
    fw = torch.empty((m, H, W, 2), dtype=torch.float32, device="cuda")
    bw = torch.empty_like(fw)
    occ = torch.empty((m, H, W), dtype=torch.uint8, device="cuda")
    emit({"what": "memory", "frames": T, "pairs": m, "pixels_per_pair": W * H,
          "level_grid": [geo["out_w"], geo["out_h"], geo["cell"]],
          "fused_flow_bytes_per_pair": {"no_fb": geo["bytes_per_pair"], "fb": 2 * geo["bytes_per_pair"]},
          "composed_flow_bytes_per_pair": {"no_fb": W * H * 8, "fb": 2 * W * H * 8}, "occ_bytes_per_pair_fb": W * H})
    code = [torch.empty((m, H, W), dtype=torch.uint8, device="cuda") for _ in range(2)]
    xf = [torch.empty((m, 6), dtype=torch.float64, device="cuda") for _ in range(2)]
    sup = [torch.empty((m,), dtype=torch.int32, device="cuda") for _ in range(2)]
    ys = torch.arange(H, dtype=torch.float64, device="cuda")[None, :, None]
    xs = torch.arange(W, dtype=torch.float64, device="cuda")[None, None, :]
    box = torch.ones((1, 1, 2 * RADIUS + 1, 2 * RADIUS + 1), dtype=torch.float32, device="cuda")

    def torch_mask(use_occ):
        M = xf[1]
        pu = ((M[:, 0, None, None] * xs + M[:, 1, None, None] * ys + M[:, 2, None, None]) - xs).float()
        pv = ((M[:, 3, None, None] * xs + M[:, 4, None, None] * ys + M[:, 5, None, None]) - ys).float()
        e = torch.sqrt((fw[..., 0] - pu) ** 2 + (fw[..., 1] - pv) ** 2)
        g = torch.sqrt(pu * pu + pv * pv)
        unknown = ~torch.isfinite(e)
        if use_occ:
            unknown = unknown | (occ != 0)
        b = ~unknown & (e > THR) & (e > REL * g)
        mov = F.conv2d(b[:, None].float(), box, padding=RADIUS)[:, 0]
        known = F.conv2d((~unknown)[:, None].float(), box, padding=RADIUS)[:, 0]
        return torch.where(unknown, 2, (2 * mov > known).to(torch.uint8)).to(torch.uint8)

    for fb in (False, True):
        ctx = {k: od.Context(0) for k in ("fused", "composed")}

        def fused():
            ctx["fused"].run_sequence_motion_mask_ptr(fr.data_ptr(), T, W, H, p, od.MOTION_SIMILARITY, STEP, TAU, ITERS, THR,
                                                      REL, RADIUS, code[0].data_ptr(), 0, 0, xf[0].data_ptr(),
                                                      sup[0].data_ptr(), 0, fb, 0.01, 0.5, s)

        def flows_and_fit():
            c = ctx["composed"]
            c.run_sequence_ptr(fr.data_ptr(), T, 1, W, H, p, fw.data_ptr(), 0, 0.01, 0.5, bw.data_ptr() if fb else 0,
                               occ.data_ptr() if fb else 0, 0, stream=s)
            c.fit_motion_ptr(fw.data_ptr(), bw.data_ptr() if fb else 0, view, m, W, H, od.MOTION_SIMILARITY, STEP, TAU, ITERS,
                             xf[1].data_ptr(), sup[1].data_ptr(), 0, 0.01, 0.5, s)

        def composed():
            flows_and_fit()
            ctx["composed"].motion_mask_ptr(fw.data_ptr(), view, m, W, H, xf[1].data_ptr(), occ.data_ptr() if fb else 0,
                                            THR, REL, RADIUS, code[1].data_ptr(), 0, 0, s)

        def torch_way():
            flows_and_fit()
            torch_mask(fb)

        def torch_only():
            torch_mask(fb)

        fused()
        composed()
        torch.cuda.synchronize()
        same = torch.equal(code[0], code[1]) and torch.equal(sup[0], sup[1]) and \
            torch.equal(xf[0].view(torch.int64), xf[1].view(torch.int64))
        if not same:
            raise SystemExit(f"fb {fb}: fused and composed differ")
        agree = float((torch_mask(fb) == code[0]).float().mean())
        ways = {"fused": fused, "fused_again": fused, "composed": composed, "torch": torch_way, "torch_mask": torch_only}
        for fn in ways.values():
            fn()
        torch.cuda.synchronize()
        tm = {k: [] for k in ways}
        for _ in range(args.blocks):
            for k, fn in ways.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                calls = args.torch_calls if k == "torch" else args.calls
                for _ in range(calls):
                    fn()
                torch.cuda.synchronize()
                tm[k].append((time.perf_counter() - t0) / calls * 1e3)
        med = {k: statistics.median(v) for k, v in tm.items()}
        shares = [round(float((code[0] == k).float().mean()), 4) for k in (0, 1, 2)]
        rec = {"what": "end_to_end", "use_fb": fb, "frames": T, "step": STEP, "tau": TAU, "iters": ITERS, "thr": THR,
               "rel": REL, "radius": RADIUS, "outputs_identical": same, "code_shares": shares,
               "torch_mask_agrees": round(agree, 6), "blocks": args.blocks, "calls_per_block": args.calls,
               "torch_calls_per_block": args.torch_calls, "aa_spread": round(med["fused_again"] / med["fused"], 4)}
        for k in ways:
            rec[k + "_ms"] = round(med[k], 4)
            rec[k + "_ms_min_max"] = [round(min(tm[k]), 4), round(max(tm[k]), 4)]
        rec["fused_over_composed"] = round(med["fused"] / med["composed"], 4)
        rec["fused_over_torch"] = round(med["fused"] / med["torch"], 4)
        emit(rec)

        # kernel timer (eager issue: a launch has the chip alone)
        reps = 5
        rec = {"what": "kernel", "use_fb": fb, "frames": T, "counter_pass": False}
        extra = W * H if fb else 0  # the occlusion byte
        for key, fn, kernels in (("fused", fused, ("motion_mask_level", "fit_motion_level") + (("fb_check_level",) if fb else ())),
                                 ("composed", composed, ("motion_mask",))):
            c = ctx[key]
            c.enable_kernel_timing(True)
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            for kernel in kernels:
                ms, cnt = c.kernel_time(kernel)
                us = ms / cnt * 1e3
                model = od.algorithmic_bytes(p, W, H, kernel) * m
                if kernel.startswith("motion_mask"):
                    model += extra * m
                if kernel == "fb_check_level":  # (the call writes the forward plane alone: one direction's mask byte)
                    model = (2 * geo["bytes_per_pair"] + W * H) * m
                gbs = model / (us * 1e-6) / 1e9
                rec[kernel] = {"avg_launch_us": round(us, 2), "launches": cnt, "us_per_pair": round(us / m, 2),
                               "model_bytes": model, "gb_s": round(gbs, 1), "frac_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
            c.enable_kernel_timing(False)
        rec["motion_mask_level_over_motion_mask"] = round(rec["motion_mask_level"]["avg_launch_us"] / rec["motion_mask"]["avg_launch_us"], 3)
        emit(rec)
        if fb:
            # every output of the primitive, and the yardsticks of DESIGN.md §7 in this process
            c = ctx["composed"]
            gf = c.run_sequence(fr, p, grid="level")
            res = torch.empty((m, H, W), dtype=torch.float32, device="cuda")
            st = torch.empty((m, od.MM_NSTATS), dtype=torch.int64, device="cuda")
            gt = fw.clone()
            rec = {"what": "kernel_all_outputs", "frames": T, "counter_pass": False}
            c.enable_kernel_timing(True)
            before = {k: c.kernel_time(k) for k in ("motion_mask", "motion_mask_level", "flow_error_level")}
            for _ in range(reps):
                c.motion_mask_ptr(fw.data_ptr(), view, m, W, H, xf[1].data_ptr(), occ.data_ptr(), THR, REL, RADIUS,
                                  code[1].data_ptr(), res.data_ptr(), st.data_ptr(), s)
                c.motion_mask_ptr(gf.data_ptr(), lview, m, W, H, xf[1].data_ptr(), occ.data_ptr(), THR, REL, RADIUS,
                                  code[1].data_ptr(), res.data_ptr(), st.data_ptr(), s)
                c.flow_error(gf, gt, grid="level", p=p, size=(W, H))
            torch.cuda.synchronize()
            for kernel in before:
                ms, cnt = c.kernel_time(kernel)
                us = (ms - before[kernel][0]) / (cnt - before[kernel][1]) * 1e3
                model = od.algorithmic_bytes(p, W, H, kernel) * m
                if kernel.startswith("motion_mask"):
                    model += W * H * (1 + 4) * m  # the occlusion byte and the residual
                gbs = model / (us * 1e-6) / 1e9
                rec[kernel] = {"avg_launch_us": round(us, 2), "model_bytes": model, "gb_s": round(gbs, 1),
                               "frac_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
            c.enable_kernel_timing(False)
            a = torch.empty(256 << 18, dtype=torch.float32, device="cuda")  # 256 MiB
            b = torch.empty_like(a)
            b.copy_(a)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                b.copy_(a)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / 20 * 1e3
            gbs = 2 * a.numel() * 4 / (us * 1e-6) / 1e9
            rec["float4_copy"] = {"avg_launch_us": round(us, 2), "model_bytes": 2 * a.numel() * 4, "gb_s": round(gbs, 1),
                                  "frac_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
            emit(rec)
        for c in ctx.values():
            c.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The fused temporal-filter call against its compositions.

End to end at 1920 x 1080, op-point 2, intensity frames, a video of 33 frames (32 pairs), filter sigma 12, u8 output
with the `used` bytes, with and without occlusion masks:
  fused    = one Context.run_sequence_tfilter_ptr call (level grids -- and masks -- in the context's buffers, one
             tfilter_level launch);
  composed = run_sequence_ptr writing both full float32 fields (and both masks) + tfilter_ptr on them, on one context:
             the same bits;
  torch    = the same run_sequence_ptr + two torch grid_sample calls over the full fields (bilinear, border padding,
             align_corners) and the weights, sum and division in torch -- for time only, its rounding differs.
All are timed in the same process in alternating blocks (host clock around calls that end in a device synchronise) after
warming all; fused and composed are compared bit for bit first.  `aa_spread` is the fused call timed against itself
(twice per block): what the box cannot tell apart.  `torch_filter_ms` is the torch weighting alone on flows already there.

Kernel: the launch times of "tfilter_level" and "tfilter" from the library's kernel timer (HIP events around the launch,
eager issue) against ofdis_algorithmic_bytes per output frame, as fractions of the HBM peak.  No counter pass is taken
here.  Memory: the flow bytes each route holds at its peak, from the geometry.

    python tools/bench_tfilter.py [--frames 33] [--blocks 10] [--calls 10] [--out FILE]

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
SIGMA = 12.0
HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=33)
    ap.add_argument("--blocks", type=int, default=10, help="alternating timed blocks per way")
    ap.add_argument("--calls", type=int, default=10, help="calls per block")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import of_dis_amd as od
    if not torch.cuda.is_available():
        raise SystemExit("bench_tfilter.py needs a GPU")
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
    fw = torch.empty((m, H, W, 2), dtype=torch.float32, device="cuda")
    bw = torch.empty_like(fw)
    ofw = torch.empty((m, H, W), dtype=torch.uint8, device="cuda")
    obw = torch.empty_like(ofw)
    emit({"what": "memory", "frames": T, "pairs": m, "level_grid": [geo["out_w"], geo["out_h"], geo["cell"]],
          "fused_flow_bytes_per_pair": 2 * geo["bytes_per_pair"], "composed_flow_bytes_per_pair": 2 * W * H * 8,
          "fused_flow_bytes": 2 * m * geo["bytes_per_pair"], "composed_flow_bytes": 2 * m * W * H * 8,
          "mask_bytes": 2 * m * W * H,
          "ratio": round(W * H * 8 / geo["bytes_per_pair"], 1)})
    pics = [torch.empty((T, H, W), dtype=torch.uint8, device="cuda") for _ in range(2)]
    used = [torch.empty((T, H, W), dtype=torch.uint8, device="cuda") for _ in range(2)]
    base = torch.stack(torch.meshgrid(torch.arange(W, device="cuda", dtype=torch.float32),
                                      torch.arange(H, device="cuda", dtype=torch.float32), indexing="xy"), -1)  # [H, W, 2]
    scale = torch.tensor([2.0 / (W - 1), 2.0 / (H - 1)], device="cuda")
    inv = 1.0 / SIGMA
    for occ in (False, True):
        ctx = {k: od.Context(0) for k in ("fused", "composed")}

        def fused():
            ctx["fused"].run_sequence_tfilter_ptr(fr.data_ptr(), T, W, H, p, SIGMA, od.IMG_U8, pics[0].data_ptr(),
                                                  used[0].data_ptr(), occ, 0.01, 0.5, s)

        def flows():
            ctx["composed"].run_sequence_ptr(fr.data_ptr(), T, 1, W, H, p, fw.data_ptr(), 0, 0.01, 0.5, bw.data_ptr(),
                                             ofw.data_ptr() if occ else 0, obw.data_ptr() if occ else 0, stream=s)

        def composed():
            flows()
            ctx["composed"].tfilter_ptr(fr.data_ptr(), T, fw.data_ptr(), bw.data_ptr(), view, W, H, 1, SIGMA, od.IMG_U8,
                                        pics[1].data_ptr(), used[1].data_ptr(), ofw.data_ptr() if occ else 0,
                                        obw.data_ptr() if occ else 0, s)

        def torch_filter():
            C = fr.float()
            acc, wsum = C.clone(), torch.ones_like(C)
            bits = torch.zeros((T, H, W), dtype=torch.uint8, device="cuda")
            for k, (own, N, G, O) in enumerate(((slice(1, T), C[:m], bw, obw), (slice(0, m), C[1:], fw, ofw))):
                pos = base + G
                S = F.grid_sample(N[:, None], pos * scale - 1.0, mode="bilinear", padding_mode="border",
                                  align_corners=True)[:, 0]
                ok = (pos[..., 0] >= 0) & (pos[..., 0] <= W - 1) & (pos[..., 1] >= 0) & (pos[..., 1] <= H - 1)
                if occ:
                    ok &= O == 0
                r = (S - C[own]).abs() * inv
                wgt = torch.where(ok, (1.0 - r * r).clamp(min=0.0), torch.zeros_like(r))
                acc[own] += wgt * S
                wsum[own] += wgt
                bits[own] |= (wgt > 0).to(torch.uint8) << k
            return (acc / wsum).clamp(max=255.0).round().to(torch.uint8), bits

        def torch_way():
            flows()
            torch_filter()

        fused()
        composed()
        torch.cuda.synchronize()
        same = torch.equal(pics[0], pics[1]) and torch.equal(used[0], used[1])
        if not same:
            raise SystemExit(f"occ {occ}: fused and composed differ")
        share = [round(float((used[0][1:m] == k).float().mean()), 4) for k in range(4)]
        tp, tu = torch_filter()
        close = float(((tp.int() - pics[0].int()).abs() <= 1).float().mean())
        ways = {"fused": fused, "fused_again": fused, "composed": composed, "torch": torch_way, "torch_filter": torch_filter}
        for fn in ways.values():
            fn()
        torch.cuda.synchronize()
        tm = {k: [] for k in ways}
        for _ in range(args.blocks):
            for k, fn in ways.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                torch.cuda.synchronize()
                tm[k].append((time.perf_counter() - t0) / args.calls * 1e3)
        med = {k: statistics.median(v) for k, v in tm.items()}
        rec = {"what": "end_to_end", "occ": occ, "frames": T, "sigma": SIGMA, "outputs_identical": same,
               "used_shares_inner_frames": share, "torch_within_one_level": round(close, 4), "blocks": args.blocks,
               "calls_per_block": args.calls, "aa_spread": round(med["fused_again"] / med["fused"], 4)}
        for k in ways:
            rec[k + "_ms"] = round(med[k], 4)
            rec[k + "_ms_min_max"] = [round(min(tm[k]), 4), round(max(tm[k]), 4)]
        rec["fused_over_composed"] = round(med["fused"] / med["composed"], 4)
        rec["fused_over_torch"] = round(med["fused"] / med["torch"], 4)
        emit(rec)

        # kernel timer (eager issue: a launch has the chip alone)
        reps = 5
        rec = {"what": "kernel", "occ": occ, "frames": T, "counter_pass": False}
        for key, fn, kernel in (("fused", fused, "tfilter_level"), ("composed", composed, "tfilter")):
            c = ctx[key]
            c.enable_kernel_timing(True)
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            ms, cnt = c.kernel_time(kernel)
            us = ms / cnt * 1e3
            model = od.algorithmic_bytes(p, W, H, kernel) * T  # (the two end frames read one neighbour: a little less)
            gbs = model / (us * 1e-6) / 1e9
            rec[kernel] = {"avg_launch_us": round(us, 2), "launches": cnt, "us_per_frame": round(us / T, 2),
                           "model_bytes": model, "gb_s": round(gbs, 1), "frac_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
            if occ and key == "fused":
                ms2, cnt2 = c.kernel_time("fb_check_level")
                rec["fb_check_level"] = {"avg_launch_us": round(ms2 / cnt2 * 1e3, 2), "launches": cnt2}
            c.enable_kernel_timing(False)
        rec["tfilter_level_over_tfilter"] = round(rec["tfilter_level"]["avg_launch_us"] / rec["tfilter"]["avg_launch_us"], 3)
        emit(rec)
        for c in ctx.values():
            c.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()

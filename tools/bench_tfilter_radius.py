#!/usr/bin/env python3
"""The fused temporal filter over a radius against its composition and against the radius-1 fused call with masks
(DESIGN.md §3.17).

End to end at 1920 x 1080, op-point 2, intensity frames, a video of 33 frames (32 pairs), filter sigma 12, u8 output
with the `used` bytes, at radius 1, 2 and 4, with and without the check:
  fused    = one Context.run_sequence_tfilter_radius_ptr call (level grids in the context's buffer, one
             tfilter_radius_level launch, the check inside the chain);
  composed = run_sequence_ptr writing both full float32 fields + tfilter_radius_ptr on them, on one context: the same
             bits;
  masks    = at radius 1 with the check only: Context.run_sequence_tfilter_ptr(occ=True) on the same frames -- the
             fb_check_level launches and the mask planes the in-kernel check replaces: the same bits.
All are timed in the same process in alternating blocks (host clock around calls that end in a device synchronise) after
warming all; the ways are compared bit for bit first.  `aa_spread` is the fused call timed against itself (twice per
block): what the box cannot tell apart.

Kernel: the launch times of "tfilter_radius_level" and "tfilter_radius" from the library's kernel timer (HIP events
around the launch, eager issue) against ofdis_tfilter_radius_bytes per output frame, as fractions of the HBM peak, and at
radius 1 with the check "tfilter_level" + "fb_check_level" of the masks way beside them.  No counter pass is taken here.

    python tools/bench_tfilter_radius.py [--frames 33] [--blocks 6] [--calls 5] [--out FILE]

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
    ap.add_argument("--blocks", type=int, default=6, help="alternating timed blocks per way")
    ap.add_argument("--calls", type=int, default=5, help="calls per block")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import of_dis_amd as od
    if not torch.cuda.is_available():
        raise SystemExit("bench_tfilter_radius.py needs a GPU")
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
    # frames a0, b0, a1, b1, ... of eight distinct synthetic pairs, repeated (tools/bench_tfilter.py's video)
    distinct = [im[..., 0] for f in range(8) for im in od.synth_pair(W, H, 1, f, od.MODE_OF)]
    fr = torch.from_numpy(np.stack([distinct[f % len(distinct)] for f in range(T)])).cuda()
    p = od.oppoint(OP, W, od.MODE_OF, 1)
    p.verbosity = 0
    s = torch.cuda.current_stream().cuda_stream
    view = od.FlowView(0, 0, 0, W, H, 1, 0, 0)
    fw = torch.empty((m, H, W, 2), dtype=torch.float32, device="cuda")
    bw = torch.empty_like(fw)
    pics = [torch.empty((T, H, W), dtype=torch.uint8, device="cuda") for _ in range(3)]
    used = [torch.empty((T, H, W), dtype=torch.uint8, device="cuda") for _ in range(3)]
    for radius in (1, 2, 4):
        for fb in (False, True):
            with_masks = radius == 1 and fb
            ctx = {k: od.Context(0) for k in ("fused", "composed", "masks")}

            def fused():
                ctx["fused"].run_sequence_tfilter_radius_ptr(fr.data_ptr(), T, W, H, p, radius, SIGMA, od.IMG_U8,
                                                             pics[0].data_ptr(), used[0].data_ptr(), fb, 0.01, 0.5, s)

            def composed():
                ctx["composed"].run_sequence_ptr(fr.data_ptr(), T, 1, W, H, p, fw.data_ptr(), 0, 0.01, 0.5, bw.data_ptr(),
                                                 0, 0, stream=s)
                ctx["composed"].tfilter_radius_ptr(fr.data_ptr(), T, fw.data_ptr(), bw.data_ptr(), view, W, H, 1, radius,
                                                   SIGMA, od.IMG_U8, pics[1].data_ptr(), used[1].data_ptr(), fb, 0.01, 0.5, s)

            def masks():
                ctx["masks"].run_sequence_tfilter_ptr(fr.data_ptr(), T, W, H, p, SIGMA, od.IMG_U8, pics[2].data_ptr(),
                                                      used[2].data_ptr(), True, 0.01, 0.5, s)

            ways = {"fused": fused, "fused_again": fused, "composed": composed}
            if with_masks:
                ways["masks"] = masks
            for fn in ways.values():
                fn()
            torch.cuda.synchronize()
            same = torch.equal(pics[0], pics[1]) and torch.equal(used[0], used[1])
            if with_masks:
                same = same and torch.equal(pics[0], pics[2]) and torch.equal(used[0], used[2])
            if not same:
                raise SystemExit(f"radius {radius} fb {fb}: the ways differ")
            inner = used[0][radius:T - radius]
            share = [round(float(((inner >> b) & 1).float().mean()), 4) for b in range(2 * radius)]
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
            rec = {"what": "end_to_end", "radius": radius, "fb": fb, "frames": T, "sigma": SIGMA, "outputs_identical": same,
                   "used_bit_shares_inner_frames": share, "blocks": args.blocks, "calls_per_block": args.calls,
                   "aa_spread": round(med["fused_again"] / med["fused"], 4)}
            for k in ways:
                rec[k + "_ms"] = round(med[k], 4)
                rec[k + "_ms_min_max"] = [round(min(tm[k]), 4), round(max(tm[k]), 4)]
            rec["fused_over_composed"] = round(med["fused"] / med["composed"], 4)
            if with_masks:
                rec["fused_over_masks"] = round(med["fused"] / med["masks"], 4)
            emit(rec)

            # kernel timer (eager issue: a launch has the chip alone)
            reps = 3
            rec = {"what": "kernel", "radius": radius, "fb": fb, "frames": T, "counter_pass": False}
            todo = [("fused", fused, "tfilter_radius_level", True), ("composed", composed, "tfilter_radius", False)]
            for key, fn, kernel, level in todo:
                c = ctx[key]
                c.enable_kernel_timing(True)
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                ms, cnt = c.kernel_time(kernel)
                us = ms / cnt * 1e3
                # (frames within `radius` of an end have shorter chains: a little less)
                model = od.tfilter_radius_bytes(p, W, H, radius, level=level) * T
                gbs = model / (us * 1e-6) / 1e9
                rec[kernel] = {"avg_launch_us": round(us, 2), "launches": cnt, "us_per_frame": round(us / T, 2),
                               "model_bytes": model, "gb_s": round(gbs, 1), "frac_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
                c.enable_kernel_timing(False)
            if with_masks:
                c = ctx["masks"]
                c.enable_kernel_timing(True)
                for _ in range(reps):
                    masks()
                torch.cuda.synchronize()
                for kernel in ("tfilter_level", "fb_check_level"):
                    ms, cnt = c.kernel_time(kernel)
                    rec[kernel] = {"avg_launch_us": round(ms / cnt * 1e3, 2), "launches": cnt,
                                   "us_per_call": round(ms / reps * 1e3, 2)}
                c.enable_kernel_timing(False)
                rec["radius_level_over_tfilter_level_plus_check"] = round(
                    rec["tfilter_radius_level"]["avg_launch_us"]
                    / (rec["tfilter_level"]["us_per_call"] + rec["fb_check_level"]["us_per_call"]), 3)
            emit(rec)
            for c in ctx.values():
                c.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""run_warp against the two routes to a motion-compensated frame without it.

End to end, per pairs-per-call at 1920 x 1080, op-point 2, intensity images, u8 picture plus valid mask:
  fused   = one Context.run_warp_ptr call (level-grid flow in the context's buffer, warp_level);
  route a = run_ptr (full float32 field) + warp_ptr on it, on one context, both replaying as a caller would issue them;
  route b = run_ptr + a torch pipeline: sampling grid from the field, torch.nn.functional.grid_sample (bilinear,
            border padding, align_corners) on a float copy of the image, round, to uint8.  Its rounding is torch's;
            its largest difference from ours is reported, not gated.
The three are timed in the same process in alternating blocks (host clock around calls that end in a device
synchronise) after warming all; fused and route a are compared bit for bit first.  `aa_spread` is the same way timed
against itself (fused twice per block): what the box cannot tell apart.

Kernel: the "warp" / "warp_level" launch times from the library's kernel timer (HIP events around the launch, eager
issue, one lane) against ofdis_algorithmic_bytes, beside the upsample's from the same calls, as fractions of the HBM
peak.  No counter pass is taken here.

    python tools/bench_warp.py [--pairs 1,256,2048] [--blocks 10] [--calls 0] [--out FILE]

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

HBM_PEAK_GBS = 8000.0
W, H, OP = 1920, 1080, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,256,2048")
    ap.add_argument("--blocks", type=int, default=10, help="alternating timed blocks per way")
    ap.add_argument("--calls", type=int, default=0, help="calls per block (0: 16 for one pair, 2 from 256, 1 from 2048)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import of_dis_amd as od
    if not torch.cuda.is_available():
        raise SystemExit("bench_warp.py needs a GPU")
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    distinct = [od.synth_pair(W, H, 1, f, od.MODE_OF) for f in range(8)]
    p = od.oppoint(OP, W, od.MODE_OF, 1)
    p.verbosity = 0
    s = torch.cuda.current_stream().cuda_stream
    view = od.FlowView(0, 0, 0, W, H, 1, 0, 0)
    xs = torch.arange(W, dtype=torch.float32, device="cuda")[None, None, :]
    ys = torch.arange(H, dtype=torch.float32, device="cuda")[None, :, None]
    for n in [int(x) for x in args.pairs.split(",")]:
        calls = args.calls or (16 if n < 16 else 2 if n < 1024 else 1)
        idx = [f % len(distinct) for f in range(n)]
        a = torch.from_numpy(np.stack([distinct[i][0][..., 0] for i in idx])).cuda()
        b = torch.from_numpy(np.stack([distinct[i][1][..., 0] for i in idx])).cuda()
        new = lambda *shape, dt=torch.uint8: torch.empty(shape, dtype=dt, device="cuda")  # noqa: E731
        flow = new(n, H, W, 2, dt=torch.float32)
        pic = {k: new(n, H, W) for k in ("fused", "a")}
        val = {k: new(n, H, W) for k in ("fused", "a")}
        c_f, c_a = od.Context(0), od.Context(0)

        def fused():
            c_f.run_warp_ptr(a.data_ptr(), b.data_ptr(), n, W, H, p, 1.0, od.IMG_U8, pic["fused"].data_ptr(),
                             val["fused"].data_ptr(), s)

        def route_a():
            c_a.run_ptr(a.data_ptr(), b.data_ptr(), n, W, H, p, flow.data_ptr(), s)
            c_a.warp_ptr(b.data_ptr(), flow.data_ptr(), view, n, W, H, 1, 1.0, od.IMG_U8, pic["a"].data_ptr(),
                         val["a"].data_ptr(), s)

        def route_b():
            c_a.run_ptr(a.data_ptr(), b.data_ptr(), n, W, H, p, flow.data_ptr(), s)
            gx = (xs + flow[..., 0]) * (2.0 / (W - 1)) - 1.0
            gy = (ys + flow[..., 1]) * (2.0 / (H - 1)) - 1.0
            img = b[:, None].float()
            res = F.grid_sample(img, torch.stack((gx, gy), -1), mode="bilinear", padding_mode="border",
                                align_corners=True)
            return res[:, 0].round().to(torch.uint8)

        ways = {"fused": fused, "fused_again": fused, "route_a": route_a}
        rec_b = None
        try:
            pic_b = route_b()
            torch.cuda.synchronize()
            ways["route_b"] = route_b
        except RuntimeError as e:  # out of memory at the largest batch: unmeasured, not estimated
            rec_b = f"unmeasured: {str(e).splitlines()[0][:120]}"
            torch.cuda.empty_cache()
        for _ in range(2):
            for fn in ways.values():
                fn()
        torch.cuda.synchronize()
        same = torch.equal(pic["fused"], pic["a"]) and torch.equal(val["fused"], val["a"])
        if not same:
            raise SystemExit(f"pairs {n}: run_warp differs from run + warp")
        diff_b = None
        if "route_b" in ways:
            diff_b = int((pic_b.int() - pic["fused"].int()).abs().max())
            del pic_b
        t = {k: [] for k in ways}
        for _ in range(args.blocks):
            for name, fn in ways.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn()
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / calls * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        rec = {"what": "end_to_end", "pairs": n, "outputs_identical": same, "blocks": args.blocks,
               "calls_per_block": calls, "aa_spread": round(med["fused_again"] / med["fused"], 4),
               "route_b_max_abs_diff_u8": diff_b}
        for k in ways:
            rec[k + "_ms"] = round(med[k], 4)
            rec[k + "_ms_min_max"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
        rec["fused_over_route_a"] = round(med["fused"] / med["route_a"], 4)
        rec["fused_over_route_b"] = round(med["fused"] / med["route_b"], 4) if "route_b" in ways else rec_b
        emit(rec)

        # kernel timer (eager issue, one lane: a launch has the chip alone)
        for c in (c_f, c_a):
            c.set_option("streams", 1)
        fused()
        route_a()
        torch.cuda.synchronize()
        reps = 5
        rec = {"what": "kernel", "pairs": n, "lanes": 1, "counter_pass": False}
        for c, fn, names in ((c_f, fused, ("warp_level", "level_out")), (c_a, route_a, ("warp", "upsample"))):
            c.enable_kernel_timing(True)
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            for k in names:
                ms, cnt = c.kernel_time(k)
                bytes_launch = od.algorithmic_bytes(p, W, H, k) * n / (cnt / reps)
                us = ms / cnt * 1e3
                gbs = bytes_launch / (us * 1e-6) / 1e9
                rec[k] = {"avg_launch_us": round(us, 2), "launches": cnt, "bytes_per_launch": bytes_launch,
                          "gb_s": round(gbs, 1), "frac_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
            c.enable_kernel_timing(False)
        emit(rec)
        c_f.close()
        c_a.close()
        del a, b, flow, pic, val
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()

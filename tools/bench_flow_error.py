#!/usr/bin/env python3
"""run_error against the three routes to "the EPE of these pairs" without it.

End to end, per pairs-per-call at 1920 x 1080, op-point 2, intensity images, no mask, stats alone:
  fused   = one Context.run_error_ptr call (level-grid flow in the context's buffer, flow_error_level);
  route a = run_ptr (full float32 field) + flow_error_ptr on it, on one context;
  route b = run_ptr + a torch composition: (f - gt).square().sum(-1).sqrt(), its mean over the known pixels and the
            three threshold counts, in slices of 64 pairs (float32 sums in torch's order: its numbers differ from ours in
            the last digits; the largest relative difference of the mean is reported, not gated);
  route c = run_ptr + a copy of the field to the host + numpy in float64, in slices of 32 pairs: what bench.py and the
            tests do today.  Timed in fewer blocks from 256 pairs (it takes seconds per call) and not at all beyond
            --host-max-pairs (default 256: at 2,048 pairs the truth alone is 34 GB of host memory); such a size is
            reported as unmeasured, not estimated.
The ways are timed in the same process in alternating blocks (host clock around calls that end in a device synchronise)
after warming all; fused and route a are compared bit for bit first.  `aa_spread` is the same way timed against itself
(fused twice per block): what the box cannot tell apart.

Kernel: the "flow_error" / "flow_error_level" / "flow_error_sum" launch times from the library's kernel timer (HIP events
around the launch, eager issue, one lane) against ofdis_algorithmic_bytes, as fractions of the HBM peak, beside the
upsample's and level_out's from the same calls.  No counter pass is taken here.

    python tools/bench_flow_error.py [--pairs 1,256,2048] [--blocks 10] [--calls 0] [--out FILE]

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
    ap.add_argument("--host-blocks", type=int, default=2, help="blocks of route c from 256 pairs")
    ap.add_argument("--host-max-pairs", type=int, default=256, help="route c is not run on larger calls")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import of_dis_amd as od
    if not torch.cuda.is_available():
        raise SystemExit("bench_flow_error.py needs a GPU")
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
    for n in [int(x) for x in args.pairs.split(",")]:
        calls = args.calls or (16 if n < 16 else 2 if n < 1024 else 1)
        idx = [f % len(distinct) for f in range(n)]
        a = torch.from_numpy(np.stack([distinct[i][0][..., 0] for i in idx])).cuda()
        b = torch.from_numpy(np.stack([distinct[i][1][..., 0] for i in idx])).cuda()
        flow = torch.empty((n, H, W, 2), dtype=torch.float32, device="cuda")
        stats = {k: torch.empty((n, 16), dtype=torch.float64, device="cuda") for k in ("fused", "a")}
        c_f, c_a = od.Context(0), od.Context(0)
        # the truth: the call's own flow plus half a pixel of noise, with a strip of unknown pixels
        c_a.run_ptr(a.data_ptr(), b.data_ptr(), n, W, H, p, flow.data_ptr(), s)
        gt = torch.empty_like(flow)
        gen = torch.Generator(device="cuda").manual_seed(1)
        for f0 in range(0, n, 64):
            part = flow[f0:f0 + 64]
            gt[f0:f0 + 64] = part + 0.5 * torch.randn(part.shape, generator=gen, device="cuda")
        gt[:, :8] = 1e10
        torch.cuda.synchronize()

        def fused():
            c_f.run_error_ptr(a.data_ptr(), b.data_ptr(), gt.data_ptr(), n, W, H, p, stats["fused"].data_ptr(), stream=s)

        def route_a():
            c_a.run_ptr(a.data_ptr(), b.data_ptr(), n, W, H, p, flow.data_ptr(), s)
            c_a.flow_error_ptr(flow.data_ptr(), view, gt.data_ptr(), n, W, H, stats["a"].data_ptr(), stream=s)

        def route_b():
            c_a.run_ptr(a.data_ptr(), b.data_ptr(), n, W, H, p, flow.data_ptr(), s)
            res = []
            for f0 in range(0, n, 64):
                f, g = flow[f0:f0 + 64], gt[f0:f0 + 64]
                known = (g.abs() <= 1e9).all(-1)
                e = (f - g).square().sum(-1).sqrt()
                e = torch.where(known, e, torch.zeros_like(e))
                cnt = known.sum((1, 2))
                res.append(torch.stack([cnt, e.sum((1, 2)), (e > 1).sum((1, 2)), (e > 3).sum((1, 2)),
                                        (e > 5).sum((1, 2))], 1))
            return torch.cat(res)

        def route_c():
            c_a.run_ptr(a.data_ptr(), b.data_ptr(), n, W, H, p, flow.data_ptr(), s)
            res = []
            for f0 in range(0, n, 32):
                f, g = flow[f0:f0 + 32].cpu().numpy(), gt_host[f0:f0 + 32]
                known = (np.abs(g) <= 1e9).all(-1)
                e = np.sqrt(((f.astype(np.float64) - g) ** 2).sum(-1))
                res.append([(e[k][known[k]].mean(), (e[k][known[k]] > 3).sum()) for k in range(len(e))])
            return res

        ways = {"fused": fused, "fused_again": fused, "route_a": route_a, "route_b": route_b}
        gt_host = None
        if n <= args.host_max_pairs:
            gt_host = gt.cpu().numpy()  # (the truth is on the host already in that route)
            ways["route_c"] = route_c
        for _ in range(2):
            for name, fn in ways.items():
                if name != "route_c":
                    fn()
        torch.cuda.synchronize()
        same = torch.equal(stats["fused"].view(torch.int64), stats["a"].view(torch.int64))
        if not same:
            raise SystemExit(f"pairs {n}: run_error differs from run + flow_error")
        tb = route_b().double()
        ours = stats["fused"]
        mean_rel = float((((tb[:, 1] / tb[:, 0]) - ours[:, 2] / ours[:, 0]).abs() / (ours[:, 2] / ours[:, 0])).max())
        counts_same = bool(torch.equal(tb[:, 0], ours[:, 0]))
        t = {k: [] for k in ways}
        for blk in range(args.blocks):
            for name, fn in ways.items():
                host = name == "route_c"
                if host and n >= 256 and blk >= args.host_blocks:
                    continue
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                reps = 1 if host and n >= 256 else calls
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / reps * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        summ = od.error_summary(stats["fused"])["pooled"]
        rec = {"what": "end_to_end", "pairs": n, "outputs_identical": same, "blocks": args.blocks,
               "calls_per_block": calls, "route_c_blocks": len(t.get("route_c", [])),
               "aa_spread": round(med["fused_again"] / med["fused"], 4),
               "route_b_mean_max_rel_diff": mean_rel, "route_b_counts_identical": counts_same,
               "pooled_epe": summ["epe"], "pooled_r3": summ["r3"]}
        for k in ways:
            rec[k + "_ms"] = round(med[k], 4)
            rec[k + "_ms_min_max"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
        for k in ("route_a", "route_b", "route_c"):
            rec["fused_over_" + k] = round(med["fused"] / med[k], 4) if k in med else "unmeasured"
        emit(rec)

        # kernel timer (eager issue, one lane: a launch has the chip alone)
        for c in (c_f, c_a):
            c.set_option("streams", 1)
        fused()
        route_a()
        torch.cuda.synchronize()
        reps = 5
        rec = {"what": "kernel", "pairs": n, "lanes": 1, "counter_pass": False}
        for c, fn, names, tag in ((c_f, fused, ("flow_error_level", "flow_error_sum", "level_out"), "fused"),
                                  (c_a, route_a, ("flow_error", "flow_error_sum", "upsample"), "route_a")):
            c.enable_kernel_timing(True)
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            for k in names:
                ms, cnt = c.kernel_time(k)
                bytes_launch = od.algorithmic_bytes(p, W, H, k) * n / (cnt / reps)
                us = ms / cnt * 1e3
                gbs = bytes_launch / (us * 1e-6) / 1e9
                rec[f"{tag}:{k}"] = {"avg_launch_us": round(us, 2), "launches": cnt, "bytes_per_launch": bytes_launch,
                                     "ms_per_2048_pairs": round(ms / reps / n * 2048, 3),
                                     "gb_s": round(gbs, 1), "frac_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
            c.enable_kernel_timing(False)
        emit(rec)
        c_f.close()
        c_a.close()
        del a, b, flow, gt, gt_host, stats
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()

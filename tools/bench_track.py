#!/usr/bin/env python3
"""The fused tracking call against its compositions.

End to end at 1920 x 1080, op-point 2, intensity frames, a video of 33 frames (32 pairs), with the forward-backward
check, for three sets of points -- 1024 random points, the 4-pixel grid (129,600) and every pixel (2,073,600, last
entry only):
  fused    = one Context.run_sequence_track_ptr call (level grids in the context's buffer, one track_level launch);
  composed = run_sequence_ptr writing both full float32 fields + track_points_ptr on them, on one context: the same bits;
  torch    = the same run_sequence_ptr + a loop of torch grid_sample calls over the full fields (bilinear, border
             padding, align_corners), positions and the forward-backward test -- for time only, its rounding differs.
All are timed in the same process in alternating blocks (host clock around calls that end in a device synchronise) after
warming all; fused and composed are compared bit for bit first.  `aa_spread` is the fused call timed against itself
(twice per block): what the box cannot tell apart.  `torch_loop_ms` is the grid_sample loop alone on flows already
there.

Kernel: the launch times of "track_level" and "track" from the library's kernel timer (HIP events around the launch,
eager issue), per point and step.  Memory: the flow bytes each route holds at its peak, from the geometry.

    python tools/bench_track.py [--frames 33] [--blocks 10] [--calls 50] [--out FILE]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=33)
    ap.add_argument("--blocks", type=int, default=10, help="alternating timed blocks per way")
    ap.add_argument("--calls", type=int, default=50, help="calls per block")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import of_dis_amd as od
    if not torch.cuda.is_available():
        raise SystemExit("bench_track.py needs a GPU")
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    T = args.frames
    m = T - 1
    # frames a0, b0, a1, b1, ... of eight distinct synthetic pairs, repeated (tools/bench_interp_seq.py's video)
    distinct = [im[..., 0] for f in range(8) for im in od.synth_pair(W, H, 1, f, od.MODE_OF)]
    fr = torch.from_numpy(np.stack([distinct[f % len(distinct)] for f in range(T)])).cuda()
    p = od.oppoint(OP, W, od.MODE_OF, 1)
    p.verbosity = 0
    s = torch.cuda.current_stream().cuda_stream
    view = od.FlowView(0, 0, 0, W, H, 1, 0, 0)
    geo = od.out_geometry(p, W, H, False, "float32", "nhwc", "level")
    fw = torch.empty((m, H, W, 2), dtype=torch.float32, device="cuda")
    bw = torch.empty_like(fw)
    emit({"what": "memory", "frames": T, "pairs": m, "level_grid": [geo["out_w"], geo["out_h"], geo["cell"]],
          "fused_flow_bytes": 2 * m * geo["bytes_per_pair"], "composed_flow_bytes": 2 * m * W * H * 8,
          "torch_flow_bytes": 2 * m * W * H * 8,
          "ratio": round(2 * m * W * H * 8 / (2 * m * geo["bytes_per_pair"]), 1)})
    rng = np.random.default_rng(0)
    sets = {"1024": ((rng.random((1024, 2)) * [W - 1, H - 1]).astype(np.float32), False),
            "grid4": (od.pixel_grid(W, H, 4), False),
            "every_pixel_last": (od.pixel_grid(W, H, 1), True)}
    scale = torch.tensor([2.0 / (W - 1), 2.0 / (H - 1)], device="cuda")
    for name, (host_pts, last) in sets.items():
        pts = torch.from_numpy(host_pts).cuda()
        n = pts.shape[0]
        flags = od.TRACK_LAST if last else 0
        shape = (n,) if last else (T, n)
        tr = [torch.empty(shape + (2,), dtype=torch.float32, device="cuda") for _ in range(2)]
        st = [torch.empty(shape, dtype=torch.uint8, device="cuda") for _ in range(2)]
        ctx = {k: od.Context(0) for k in ("fused", "composed")}

        def fused():
            ctx["fused"].run_sequence_track_ptr(fr.data_ptr(), T, W, H, p, pts.data_ptr(), n, 0, True, 0.01, 0.5, flags,
                                                tr[0].data_ptr(), st[0].data_ptr(), s)

        def flows():
            ctx["composed"].run_sequence_ptr(fr.data_ptr(), T, 1, W, H, p, fw.data_ptr(), 0, 0.01, 0.5, bw.data_ptr(),
                                             stream=s)

        def composed():
            flows()
            ctx["composed"].track_points_ptr(fw.data_ptr(), bw.data_ptr(), view, m, W, H, pts.data_ptr(), n, 0, 0.01, 0.5,
                                             flags, tr[1].data_ptr(), st[1].data_ptr(), s)

        def torch_loop():
            pos = pts.clone()
            bad = torch.zeros(n, dtype=torch.bool, device="cuda")
            keep = [] if last else [pos]
            for j in range(m):
                g = (pos * scale - 1.0).view(1, 1, n, 2)
                f = F.grid_sample(fw[j].permute(2, 0, 1)[None], g, mode="bilinear", padding_mode="border",
                                  align_corners=True)[0, :, 0].t()
                q = pos + f
                g = (q * scale - 1.0).view(1, 1, n, 2)
                b = F.grid_sample(bw[j].permute(2, 0, 1)[None], g, mode="bilinear", padding_mode="border",
                                  align_corners=True)[0, :, 0].t()
                d = f + b
                bad |= (d * d).sum(1) > 0.01 * ((f * f).sum(1) + (b * b).sum(1)) + 0.5
                pos = q
                if not last:
                    keep.append(pos)
            return (pos if last else torch.stack(keep)), bad

        def torch_way():
            flows()
            torch_loop()

        fused()
        composed()
        torch.cuda.synchronize()
        same = torch.equal(tr[0].view(torch.int32), tr[1].view(torch.int32)) and torch.equal(st[0], st[1])
        if not same:
            raise SystemExit(f"points {name}: fused and composed differ")
        final = st[0] if last else st[0][-1]
        share = [round(float((final == k).float().mean()), 4) for k in range(3)]
        ways = {"fused": fused, "fused_again": fused, "composed": composed, "torch": torch_way, "torch_loop": torch_loop}
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
        rec = {"what": "end_to_end", "points": name, "npts": n, "frames": T, "last_only": last, "outputs_identical": same,
               "final_status_shares": share, "blocks": args.blocks, "calls_per_block": args.calls,
               "aa_spread": round(med["fused_again"] / med["fused"], 4)}
        for k in ways:
            rec[k + "_ms"] = round(med[k], 4)
            rec[k + "_ms_min_max"] = [round(min(tm[k]), 4), round(max(tm[k]), 4)]
        rec["fused_over_composed"] = round(med["fused"] / med["composed"], 4)
        rec["fused_over_torch"] = round(med["fused"] / med["torch"], 4)
        emit(rec)

        # kernel timer (eager issue: a launch has the chip alone)
        reps = 5
        rec = {"what": "kernel", "points": name, "npts": n, "steps": m, "counter_pass": False}
        for key, fn, kernel in (("fused", fused, "track_level"), ("composed", composed, "track")):
            c = ctx[key]
            c.enable_kernel_timing(True)
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            ms, cnt = c.kernel_time(kernel)
            us = ms / cnt * 1e3
            rec[kernel] = {"avg_launch_us": round(us, 2), "launches": cnt, "ns_per_point_step": round(us * 1e3 / (n * m), 4)}
            c.enable_kernel_timing(False)
        rec["track_level_over_track"] = round(rec["track_level"]["avg_launch_us"] / rec["track"]["avg_launch_us"], 3)
        emit(rec)
        for c in ctx.values():
            c.close()
        del tr, st, pts
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""run_stereo against the composition a user writes without it.

End to end, per pairs-per-call at 1920 x 1080, DE op-point 2, intensity images, both disparities and both masks:
  stereo      = one Context.run_stereo_ptr call (one batch of 2n flow pairs, mirrored base level, mirrored store,
                k_lr_check);
  composition = run(l, r); the two images mirrored by torch; run(mir r, mir l); the field mirrored back and negated
                by torch; both fields packed into (d, 0) flow fields; fb_check.  Each plain call has its own context
                and fixed buffers (the mirrored images and fields are written into preallocated tensors), so both
                replay their graphs as the stereo call does.
Both are timed in the same process in alternating blocks (host clock around calls that end in a device synchronise)
after warming both; the disparities and masks are compared bit for bit first.  `aa_spread` is the stereo call timed
against itself (twice per block): what the box cannot tell apart.

Kernel: the "lr_check" / "lr_check_err" launch times from the library's kernel timer (HIP events around the launch,
eager issue, one lane) against ofdis_algorithmic_bytes, beside fb_check's on the packed fields, as fractions of the
HBM peak.  No counter pass is taken here.

    python tools/bench_stereo.py [--pairs 1,32,256] [--blocks 10] [--calls 0] [--out FILE]

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
    ap.add_argument("--pairs", default="1,32,256")
    ap.add_argument("--blocks", type=int, default=10, help="alternating timed blocks per way")
    ap.add_argument("--calls", type=int, default=0, help="calls per block (0: 16 for one pair, 4 at 32, 1 from 256)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import of_dis_amd as od
    if not torch.cuda.is_available():
        raise SystemExit("bench_stereo.py needs a GPU")
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    distinct = [od.synth_pair(W, H, 1, f, od.MODE_DE) for f in range(8)]
    p = od.oppoint(OP, W, od.MODE_DE, 1)
    p.verbosity = 0
    s = torch.cuda.current_stream().cuda_stream
    rev = torch.arange(W - 1, -1, -1, device="cuda")
    for n in [int(x) for x in args.pairs.split(",")]:
        calls = args.calls or (16 if n < 16 else 4 if n < 128 else 1)
        idx = [f % len(distinct) for f in range(n)]
        left = torch.from_numpy(np.stack([distinct[i][0][..., 0] for i in idx])).cuda()
        right = torch.from_numpy(np.stack([distinct[i][1][..., 0] for i in idx])).cuda()
        new = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device="cuda")  # noqa: E731
        # the stereo call's outputs
        sd = [new(n, H, W) for _ in range(2)]
        so = [new(n, H, W, dt=torch.uint8) for _ in range(2)]
        # the composition's buffers
        ml, mr = new(n, H, W, dt=torch.uint8), new(n, H, W, dt=torch.uint8)
        cd, cm, cr = new(n, H, W), new(n, H, W), new(n, H, W)
        pk = [torch.zeros((n, H, W, 2), dtype=torch.float32, device="cuda") for _ in range(2)]
        co = [new(n, H, W, dt=torch.uint8) for _ in range(2)]
        c_s, c_l, c_r = od.Context(0), od.Context(0), od.Context(0)

        def stereo():
            c_s.run_stereo_ptr(left.data_ptr(), right.data_ptr(), n, W, H, p, 0.01, 0.5, sd[0].data_ptr(),
                               sd[1].data_ptr(), so[0].data_ptr(), so[1].data_ptr(), 0, 0, s)

        def composition():
            c_l.run_ptr(left.data_ptr(), right.data_ptr(), n, W, H, p, cd.data_ptr(), s)
            torch.index_select(right, 2, rev, out=ml)  # torch.flip into a fixed buffer
            torch.index_select(left, 2, rev, out=mr)
            c_r.run_ptr(ml.data_ptr(), mr.data_ptr(), n, W, H, p, cm.data_ptr(), s)
            torch.index_select(cm, 2, rev, out=cr)
            cr.neg_()
            pk[0][..., 0] = cd
            pk[1][..., 0] = cr
            c_l.fb_check_ptr(pk[0].data_ptr(), pk[1].data_ptr(), n, W, H, 0.01, 0.5, co[0].data_ptr(),
                             co[1].data_ptr(), 0, 0, s)

        ways = {"stereo": stereo, "stereo_again": stereo, "composition": composition}
        for _ in range(2):
            for fn in ways.values():
                fn()
        torch.cuda.synchronize()
        same = (torch.equal(sd[0].view(torch.int32), cd.view(torch.int32))
                and torch.equal(sd[1].view(torch.int32), cr.view(torch.int32))
                and torch.equal(so[0], co[0]) and torch.equal(so[1], co[1]))
        if not same:
            raise SystemExit(f"pairs {n}: run_stereo differs from the composition")
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
               "calls_per_block": calls, "aa_spread": round(med["stereo_again"] / med["stereo"], 4)}
        for k in ways:
            rec[k + "_ms"] = round(med[k], 4)
            rec[k + "_ms_min_max"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
        rec["stereo_over_composition"] = round(med["stereo"] / med["composition"], 4)
        rec["stereo_pairs_per_s"] = round(n / med["stereo"] * 1e3, 1)
        emit(rec)

        # kernel timer (eager issue, one lane: a launch has the chip alone)
        c_s.set_option("streams", 1)
        reps = 5
        serr = [new(n, H, W) for _ in range(2)]
        cerr = [new(n, H, W) for _ in range(2)]

        def checks(err):
            e = [x.data_ptr() if err else 0 for x in serr], [x.data_ptr() if err else 0 for x in cerr]
            c_s.lr_check_ptr(sd[0].data_ptr(), sd[1].data_ptr(), n, W, H, 0.01, 0.5, so[0].data_ptr(),
                             so[1].data_ptr(), e[0][0], e[0][1], s)
            c_s.fb_check_ptr(pk[0].data_ptr(), pk[1].data_ptr(), n, W, H, 0.01, 0.5, co[0].data_ptr(),
                             co[1].data_ptr(), e[1][0], e[1][1], s)

        checks(False)
        checks(True)
        torch.cuda.synchronize()
        rec = {"what": "kernel", "pairs": n, "lanes": 1, "counter_pass": False}
        c_s.enable_kernel_timing(True)
        for _ in range(reps):
            checks(False)
            checks(True)
        torch.cuda.synchronize()
        for k in ("lr_check", "lr_check_err", "fb_check", "fb_check_err"):
            ms, cnt = c_s.kernel_time(k)
            bytes_launch = od.algorithmic_bytes(p, W, H, k) * n / (cnt / reps)
            us = ms / cnt * 1e3
            gbs = bytes_launch / (us * 1e-6) / 1e9
            rec[k] = {"avg_launch_us": round(us, 2), "launches": cnt, "bytes_per_launch": bytes_launch,
                      "gb_s": round(gbs, 1), "frac_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
        c_s.enable_kernel_timing(False)
        emit(rec)
        for c in (c_s, c_l, c_r):
            c.close()
        del left, right, sd, so, ml, mr, cd, cm, cr, pk, co, serr, cerr
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()

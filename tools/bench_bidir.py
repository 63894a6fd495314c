#!/usr/bin/env python3
"""run_bidir against the way to the same outputs without it ("Both directions and occlusion masks").

End to end, per cell (pairs per call x usefbcon) at 1920 x 1080, op-point 2, intensity images:
  bidir    = one Context.run_bidir_ptr call: both flows and both masks;
  baseline = run_ptr(a, b) + run_ptr(b, a) + fb_check_ptr, each direction on a context of its own, so that both
             replay their captured graph as a caller who knew the library would arrange it.
The two are timed in the same process in alternating blocks (host clock around calls that end in a device
synchronise) after warming both; the outputs of the two ways are compared bit for bit first.

Kernel: the fb_check launch time from the library's kernel timer (HIP events around the launch, eager issue)
against ofdis_algorithmic_bytes, beside the upsample's from the same calls, as fractions of the HBM peak --
masks only ("fb_check") and masks plus error maps ("fb_check_err").

    python tools/bench_bidir.py [--pairs 256,1] [--blocks 12] [--calls 8] [--out FILE]

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
    ap.add_argument("--pairs", default="256,1")
    ap.add_argument("--blocks", type=int, default=12, help="alternating timed blocks per way")
    ap.add_argument("--calls", type=int, default=8, help="calls per block")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import of_dis_amd as od
    if not torch.cuda.is_available():
        raise SystemExit("bench_bidir.py needs a GPU")
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    distinct = [od.synth_pair(W, H, 1, f, od.MODE_OF) for f in range(8)]
    for n in [int(x) for x in args.pairs.split(",")]:
        idx = [f % len(distinct) for f in range(n)]
        a = torch.from_numpy(np.stack([distinct[i][0] for i in idx])).cuda()
        b = torch.from_numpy(np.stack([distinct[i][1] for i in idx])).cuda()
        new = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device="cuda")  # noqa: E731
        base = dict(fw=new(n, H, W, 2), bw=new(n, H, W, 2), of=new(n, H, W, dt=torch.uint8), ob=new(n, H, W, dt=torch.uint8))
        bid = dict(fw=new(n, H, W, 2), bw=new(n, H, W, 2), of=new(n, H, W, dt=torch.uint8), ob=new(n, H, W, dt=torch.uint8))
        err = [new(n, H, W), new(n, H, W)]
        s = torch.cuda.current_stream().cuda_stream
        for usefbcon in (0, 1):
            p = od.oppoint(OP, W, od.MODE_OF, 1)
            p.usefbcon = usefbcon
            p.verbosity = 0
            c_ab, c_ba, c_bi = od.Context(0), od.Context(0), od.Context(0)

            def baseline():
                c_ab.run_ptr(a.data_ptr(), b.data_ptr(), n, W, H, p, base["fw"].data_ptr(), s)
                c_ba.run_ptr(b.data_ptr(), a.data_ptr(), n, W, H, p, base["bw"].data_ptr(), s)
                c_ab.fb_check_ptr(base["fw"].data_ptr(), base["bw"].data_ptr(), n, W, H, 0.01, 0.5,
                                  base["of"].data_ptr(), base["ob"].data_ptr(), 0, 0, s)

            def bidir(want_err=False, c=c_bi):
                c.run_bidir_ptr(a.data_ptr(), b.data_ptr(), n, W, H, p, 0.01, 0.5, bid["fw"].data_ptr(),
                                bid["bw"].data_ptr(), bid["of"].data_ptr(), bid["ob"].data_ptr(),
                                err[0].data_ptr() if want_err else 0, err[1].data_ptr() if want_err else 0, s)

            for _ in range(3):
                baseline()
                bidir()
            torch.cuda.synchronize()
            same = all(torch.equal(base[k].view(torch.int32) if base[k].dtype == torch.float32 else base[k],
                                   bid[k].view(torch.int32) if bid[k].dtype == torch.float32 else bid[k])
                       for k in base)
            if not same:
                raise SystemExit(f"pairs {n} usefbcon {usefbcon}: run_bidir differs from the two plain calls")
            t = {"baseline": [], "bidir": []}
            for _ in range(args.blocks):
                for name, fn in (("baseline", baseline), ("bidir", bidir)):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        fn()
                    torch.cuda.synchronize()
                    t[name].append((time.perf_counter() - t0) / args.calls * 1e3)
            med = {k: statistics.median(v) for k, v in t.items()}
            emit({"what": "end_to_end", "pairs": n, "usefbcon": usefbcon, "outputs_identical": same,
                  "baseline_ms": round(med["baseline"], 4), "bidir_ms": round(med["bidir"], 4),
                  "baseline_ms_min_max": [round(min(t["baseline"]), 4), round(max(t["baseline"]), 4)],
                  "bidir_ms_min_max": [round(min(t["bidir"]), 4), round(max(t["bidir"]), 4)],
                  "bidir_over_baseline": round(med["bidir"] / med["baseline"], 4),
                  "blocks": args.blocks, "calls_per_block": args.calls})

            # kernel timer (eager issue): the check and the upsample of the same calls -- as the call is issued by
            # default (from 256 pairs two lanes, whose kernels share the chip) and on one lane (a launch has it alone)
            for streams, want_err, name in ((0, False, "fb_check"), (0, True, "fb_check_err"),
                                            (1, False, "fb_check"), (1, True, "fb_check_err")):
                if streams and n < 256:
                    continue  # one lane already
                c_bi.set_option("streams", streams)
                bidir(want_err)  # this issue form's workspaces and code paths, outside the timers
                torch.cuda.synchronize()
                c_bi.enable_kernel_timing(True)
                reps = 5
                for _ in range(reps):
                    bidir(want_err)
                torch.cuda.synchronize()
                rec = {"what": "kernel", "pairs": n, "usefbcon": usefbcon, "lanes": 1 if streams or n < 256 else 2}
                for k in (name, "upsample"):
                    ms, cnt = c_bi.kernel_time(k)
                    per_call = cnt / reps / (2 if k == "upsample" else 1)  # two upsamples per call and chunk
                    bytes_launch = od.algorithmic_bytes(p, W, H, k) * n / per_call
                    us = ms / cnt * 1e3
                    gbs = bytes_launch / (us * 1e-6) / 1e9
                    rec[k] = {"avg_launch_us": round(us, 2), "launches": cnt, "bytes_per_launch": bytes_launch,
                              "gb_s": round(gbs, 1), "frac_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
                c_bi.enable_kernel_timing(False)
                emit(rec)
            for c in (c_ab, c_ba, c_bi):
                c.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()

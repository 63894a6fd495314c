#!/usr/bin/env python3
"""The fused interpolation with masks and the sequence interpolation against their compositions.

End to end, per pairs-per-call and per number of intermediate frames nt (t = k / (nt + 1)) at 1920 x 1080, op-point 2,
intensity images, u8 pictures plus valid mask.  The frames are one array of pairs + 1 frames; pair i is (frame i,
frame i + 1), so every way below computes the same pairs:
  fused_occ = one Context.run_interp_occ_ptr call (level grids, fb_check_level, interp_level with the masks, which
              stay in the chunk's workspace);
  composed  = run_bidir_ptr (both full float32 fields and both masks) + interp_ptr with the masks, on one context:
              the same bits;
  seq / seq_occ   = one Context.run_sequence_interp_ptr call on the frames, without / with masks;
  pair / fused_occ = run_interp_ptr / run_interp_occ_ptr on the two slices frames[:-1], frames[1:]: the same bits.
All are timed in the same process in alternating blocks (host clock around calls that end in a device synchronise)
after warming all, and compared bit for bit first.  `aa_spread` is one way timed against itself (fused_occ twice per
block): what the box cannot tell apart.

Kernel: the launch times of "fb_check_level", "fb_check" and "interp_level" with and without masks from the library's
kernel timer (HIP events around the launch, eager issue, one lane), from calls in the same process, against
ofdis_algorithmic_bytes as fractions of the HBM peak.  No counter pass is taken here.

    python tools/bench_interp_seq.py [--pairs 1,256,2048] [--nt 1,3] [--blocks 10] [--calls 0] [--out FILE]

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
    ap.add_argument("--nt", default="1,3")
    ap.add_argument("--blocks", type=int, default=10, help="alternating timed blocks per way")
    ap.add_argument("--calls", type=int, default=0, help="calls per block (0: 16 for one pair, 2 from 256, 1 from 2048)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import of_dis_amd as od
    if not torch.cuda.is_available():
        raise SystemExit("bench_interp_seq.py needs a GPU")
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    # frames a0, b0, a1, b1, ... of eight distinct synthetic pairs, repeated
    distinct = [im[..., 0] for f in range(8) for im in od.synth_pair(W, H, 1, f, od.MODE_OF)]
    p = od.oppoint(OP, W, od.MODE_OF, 1)
    p.verbosity = 0
    s = torch.cuda.current_stream().cuda_stream
    view = od.FlowView(0, 0, 0, W, H, 1, 0, 0)
    for n in [int(x) for x in args.pairs.split(",")]:
        calls = args.calls or (16 if n < 16 else 2 if n < 1024 else 1)
        fr = torch.from_numpy(np.stack([distinct[f % len(distinct)] for f in range(n + 1)])).cuda()
        a, b = fr.data_ptr(), fr.data_ptr() + W * H
        new = lambda *shape, dt=torch.uint8: torch.empty(shape, dtype=dt, device="cuda")  # noqa: E731
        fw, bw = new(n, H, W, 2, dt=torch.float32), new(n, H, W, 2, dt=torch.float32)
        occ = [new(n, H, W), new(n, H, W)]
        for nt in [int(x) for x in args.nt.split(",")]:
            times = np.array([k / (nt + 1) for k in range(1, nt + 1)], np.float32)
            names = ("fused_occ", "composed", "seq_occ", "pair", "seq")
            # two sets of pictures serve the five ways (a way keeps its set, so its graph replays): each is compared
            # with its counterpart right after the two have run
            where = {"fused_occ": 0, "composed": 1, "seq_occ": 1, "pair": 0, "seq": 1}
            pic = [new(n, nt, H, W) for _ in range(2)]
            val = [new(n, nt, H, W) for _ in range(2)]
            ctx = {k: od.Context(0) for k in names}
            o = lambda k: (pic[where[k]].data_ptr(), val[where[k]].data_ptr())  # noqa: E731

            def fused_occ():
                ctx["fused_occ"].run_interp_occ_ptr(a, b, n, W, H, p, times, 0.01, 0.5, od.IMG_U8, *o("fused_occ"), stream=s)

            def composed():
                c = ctx["composed"]
                c.run_bidir_ptr(a, b, n, W, H, p, 0.01, 0.5, fw.data_ptr(), bw.data_ptr(), occ[0].data_ptr(),
                                occ[1].data_ptr(), stream=s)
                c.interp_ptr(a, b, fw.data_ptr(), bw.data_ptr(), view, n, W, H, 1, times, od.IMG_U8, *o("composed"),
                             occ[0].data_ptr(), occ[1].data_ptr(), s)

            def seq_occ():
                ctx["seq_occ"].run_sequence_interp_ptr(a, n + 1, 1, W, H, p, times, od.IMG_U8, *o("seq_occ"), True, stream=s)

            def pair():
                ctx["pair"].run_interp_ptr(a, b, n, W, H, p, times, od.IMG_U8, *o("pair"), s)

            def seq():
                ctx["seq"].run_sequence_interp_ptr(a, n + 1, 1, W, H, p, times, od.IMG_U8, *o("seq"), False, stream=s)

            ways = {"fused_occ": fused_occ, "fused_occ_again": fused_occ, "composed": composed, "seq_occ": seq_occ,
                    "pair": pair, "seq": seq}

            def identical(x, y):  # way x (set 0) against way y (set 1)
                ways[x]()
                ways[y]()
                torch.cuda.synchronize()
                return torch.equal(pic[0], pic[1]) and torch.equal(val[0], val[1])

            same = all([identical("fused_occ", "composed"), identical("fused_occ", "seq_occ"), identical("pair", "seq")])
            if not same:
                raise SystemExit(f"pairs {n} nt {nt}: the ways differ")
            masks_matter = not identical("pair", "seq_occ")
            for fn in ways.values():
                fn()
            torch.cuda.synchronize()
            tm = {k: [] for k in ways}
            for _ in range(args.blocks):
                for name, fn in ways.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(calls):
                        fn()
                    torch.cuda.synchronize()
                    tm[name].append((time.perf_counter() - t0) / calls * 1e3)
            med = {k: statistics.median(v) for k, v in tm.items()}
            rec = {"what": "end_to_end", "pairs": n, "nt": nt, "outputs_identical": same, "masks_change_pixels": masks_matter,
                   "blocks": args.blocks, "calls_per_block": calls,
                   "aa_spread": round(med["fused_occ_again"] / med["fused_occ"], 4)}
            for k in ways:
                rec[k + "_ms"] = round(med[k], 4)
                rec[k + "_ms_min_max"] = [round(min(tm[k]), 4), round(max(tm[k]), 4)]
            rec["fused_occ_over_composed"] = round(med["fused_occ"] / med["composed"], 4)
            rec["seq_over_pair"] = round(med["seq"] / med["pair"], 4)
            rec["seq_occ_over_fused_occ"] = round(med["seq_occ"] / med["fused_occ"], 4)
            rec["fused_occ_over_pair"] = round(med["fused_occ"] / med["pair"], 4)
            emit(rec)

            # kernel timer (eager issue, one lane: a launch has the chip alone)
            reps = 5
            rec = {"what": "kernel", "pairs": n, "nt": nt, "lanes": 1, "counter_pass": False}
            for key, fn, kernels in (("fused_occ", fused_occ, ("fb_check_level", "interp_level")),
                                     ("composed", composed, ("fb_check",)), ("pair", pair, ("interp_level",))):
                c = ctx[key]
                c.set_option("streams", 1)
                fn()
                torch.cuda.synchronize()
                c.enable_kernel_timing(True)
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                for k in kernels:
                    ms, cnt = c.kernel_time(k)
                    us = ms / cnt * 1e3
                    r = {"avg_launch_us": round(us, 2), "launches": cnt}
                    if k != "interp_level":  # (its byte model is per intermediate frame: bench_interp.py)
                        bytes_launch = od.algorithmic_bytes(p, W, H, k) * n / (cnt / reps)
                        if k == "fb_check_level":  # the fused call writes masks only: no error maps
                            bytes_launch -= 2.0 * 4.0 * W * H * n / (cnt / reps)
                        gbs = bytes_launch / (us * 1e-6) / 1e9
                        r.update(bytes_per_launch=bytes_launch, gb_s=round(gbs, 1), frac_hbm_peak=round(gbs / HBM_PEAK_GBS, 4))
                    rec[k + ("_masked" if key == "fused_occ" and k == "interp_level" else "")] = r
                c.enable_kernel_timing(False)
            rec["fb_check_level_over_fb_check"] = round(rec["fb_check_level"]["avg_launch_us"] / rec["fb_check"]["avg_launch_us"], 3)
            rec["interp_level_masked_over_plain"] = round(
                rec["interp_level_masked"]["avg_launch_us"] / rec["interp_level"]["avg_launch_us"], 3)
            emit(rec)
            for c in ctx.values():
                c.close()
            del pic, val
            torch.cuda.empty_cache()
        del fr, fw, bw, occ
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()

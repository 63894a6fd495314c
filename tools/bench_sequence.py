#!/usr/bin/env python3
"""run_sequence against the way to the same output without it ("Video sequences").

End to end, per cell (pairs per call, stride 1) at 1920 x 1080, op-point 2, intensity images:
  sequence = one Context.run_sequence_ptr call on the n + 1 frames;
  baseline = one Context.run_ptr(frames, frames + one frame, n) call on a context of its own, so that both replay
             their captured graph -- the way a caller without run_sequence gets the same flows.
With --bidir-pairs the same for both directions and masks: run_sequence_ptr with the backward outputs against
run_bidir_ptr on the offset pointers.
The two ways are timed in one process in alternating blocks (host clock around calls that end in a device
synchronise) after warming both; their outputs are compared bit for bit first.

Kernel: the summed pyr_base + pyr_down + pyr_pad_grad time of one call from the library's kernel timer (HIP events
around eager launches), sequence over plain, beside the launched-work ratio (n + 1) / 2n.

    python tools/bench_sequence.py [--pairs 1,32,256,2048] [--bidir-pairs 256] [--kernel-pairs 256]
                                   [--blocks 12] [--calls 8] [--out FILE]

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
PYR = ("pyr_base", "pyr_down", "pyr_pad_grad")


def ints(text):
    return [int(x) for x in text.split(",") if x]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,32,256,2048")
    ap.add_argument("--bidir-pairs", default="256")
    ap.add_argument("--kernel-pairs", default="256")
    ap.add_argument("--blocks", type=int, default=12, help="alternating timed blocks per way")
    ap.add_argument("--calls", type=int, default=8, help="calls per block")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import of_dis_amd as od
    if not torch.cuda.is_available():
        raise SystemExit("bench_sequence.py needs a GPU")
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    # nine frames of one texture translating by (1.5, -0.75) per frame, repeated along the sequence
    distinct = [od.synth_shift_pair(W, H, (0, 0), 1, 0)[0]]
    distinct += [od.synth_shift_pair(W, H, (1.5 * t, -0.75 * t), 1, 0)[1] for t in range(1, 9)]
    distinct = [torch.from_numpy(x).cuda() for x in distinct]
    p = od.oppoint(OP, W, od.MODE_OF, 1)
    p.verbosity = 0
    s = torch.cuda.current_stream().cuda_stream
    frame_bytes = W * H
    new = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device="cuda")  # noqa: E731

    def bits(t):
        return t.view(torch.int32) if t.dtype == torch.float32 else t

    def compare_and_time(cell, ways, outs):
        for _ in range(3):
            for fn in ways.values():
                fn()
        torch.cuda.synchronize()
        names = list(ways)
        same = all(torch.equal(bits(x), bits(y)) for x, y in zip(outs[names[0]], outs[names[1]]))
        if not same:
            raise SystemExit(f"{cell}: the two ways' outputs differ")
        t = {k: [] for k in ways}
        for _ in range(args.blocks):
            for name, fn in ways.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                torch.cuda.synchronize()
                t[name].append((time.perf_counter() - t0) / args.calls * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        rec = dict(cell, outputs_identical=same, blocks=args.blocks, calls_per_block=args.calls)
        for k in names:
            rec[f"{k}_ms"] = round(med[k], 4)
            rec[f"{k}_ms_min_max"] = [round(min(t[k]), 4), round(max(t[k]), 4)]
        rec["sequence_over_baseline"] = round(med["sequence"] / med["baseline"], 4)
        b = t["baseline"]
        rec["baseline_block_spread"] = round((max(b) - min(b)) / med["baseline"], 4)
        emit(rec)

    for n in sorted(set(ints(args.pairs) + ints(args.bidir_pairs) + ints(args.kernel_pairs))):
        frames = torch.stack([distinct[t % len(distinct)] for t in range(n + 1)]).contiguous()
        fp = frames.data_ptr()
        if n in ints(args.pairs):
            c_seq, c_base = od.Context(0), od.Context(0)
            o = {"sequence": [new(n, H, W, 2)], "baseline": [new(n, H, W, 2)]}
            compare_and_time({"what": "end_to_end", "pairs": n, "stride": 1, "bidir": 0}, {
                "baseline": lambda: c_base.run_ptr(fp, fp + frame_bytes, n, W, H, p, o["baseline"][0].data_ptr(), s),
                "sequence": lambda: c_seq.run_sequence_ptr(fp, n + 1, 1, W, H, p, o["sequence"][0].data_ptr(), stream=s),
            }, o)
            c_seq.close()
            c_base.close()
            del o
        if n in ints(args.bidir_pairs):
            c_seq, c_base = od.Context(0), od.Context(0)
            o = {k: [new(n, H, W, 2), new(n, H, W, 2), new(n, H, W, dt=torch.uint8), new(n, H, W, dt=torch.uint8)]
                 for k in ("sequence", "baseline")}
            ptr = {k: [t.data_ptr() for t in v] for k, v in o.items()}
            compare_and_time({"what": "end_to_end", "pairs": n, "stride": 1, "bidir": 1}, {
                "baseline": lambda: c_base.run_bidir_ptr(fp, fp + frame_bytes, n, W, H, p, 0.01, 0.5,
                                                         *ptr["baseline"], 0, 0, s),
                "sequence": lambda: c_seq.run_sequence_ptr(fp, n + 1, 1, W, H, p, ptr["sequence"][0], 0, 0.01, 0.5,
                                                           *ptr["sequence"][1:], 0, 0, s),
            }, o)
            c_seq.close()
            c_base.close()
            del o
        if n in ints(args.kernel_pairs):
            # the kernel timer issues eagerly; one lane, so that a pyramid launch has the chip to itself
            c = od.Context(0)
            c.set_option("streams", 1)
            flow = new(n, H, W, 2)
            ways = {"plain": lambda: c.run_ptr(fp, fp + frame_bytes, n, W, H, p, flow.data_ptr(), s),
                    "sequence": lambda: c.run_sequence_ptr(fp, n + 1, 1, W, H, p, flow.data_ptr(), stream=s)}
            rec = {"what": "pyramid_kernels", "pairs": n, "stride": 1, "lanes": 1, "launched_work_ratio": (n + 1) / (2 * n)}
            reps = 5
            for name, fn in ways.items():
                fn()
                torch.cuda.synchronize()
                c.enable_kernel_timing(True)
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                per = {k: c.kernel_time(k)[0] / reps for k in PYR}
                c.enable_kernel_timing(False)
                rec[f"{name}_ms"] = {k: round(v, 4) for k, v in per.items()}
                rec[f"{name}_pyramid_ms"] = round(sum(per.values()), 4)
            rec["sequence_over_plain"] = round(rec["sequence_pyramid_ms"] / rec["plain_pyramid_ms"], 4)
            emit(rec)
            c.close()
        del frames
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The output formats against the plain call.

End to end, per batch size at 1920 x 1080, op-point 2, intensity images: one Context per way -- the plain call, the
plain call a second time (the A/A leg: its distance from the first is the run-to-run spread), float16, planar, planar
float16, the level grid in float32 and in planar float16 -- each replaying its own captured graph, all writing one
shared output buffer.  The ways are timed in the same process in alternating blocks (host clock around calls that end
in a device synchronise) after warming all of them; medians per way.  Before any timing every way's output is compared
bit for bit with the plain call's transformed (float16: torch's round-to-nearest-even conversion; level: pair 0 against
its stage capture x 2^sc_l, and every pair against the first pair made from the same images).

Kernel: the store kernel of each way from the library's kernel timer (HIP events around the launch, eager issue)
against ofdis_algorithmic_bytes as a fraction of the HBM peak, as the call is issued by default and on one lane.

    python tools/bench_outfmt.py [--pairs 256,2048] [--blocks 12] [--calls 8] [--out FILE]

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
DISTINCT = 8
# way -> (dtype, layout, grid, kernel timer name)
WAYS = {
    "plain": ("float32", "nhwc", "full", "upsample"),
    "plain_again": ("float32", "nhwc", "full", "upsample"),
    "f16": ("float16", "nhwc", "full", "upsample_f16"),
    "planar": ("float32", "nchw", "full", "upsample_planar"),
    "planar_f16": ("float16", "nchw", "full", "upsample_planar_f16"),
    "level": ("float32", "nhwc", "level", "level_out"),
    "level_planar_f16": ("float16", "nchw", "level", "level_out"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="256,2048")
    ap.add_argument("--blocks", type=int, default=12, help="alternating timed blocks per way")
    ap.add_argument("--calls", type=int, default=8, help="calls per block")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import of_dis_amd as od
    if not torch.cuda.is_available():
        raise SystemExit("bench_outfmt.py needs a GPU")
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    p = od.oppoint(OP, W, od.MODE_OF, 1)
    p.verbosity = 0
    distinct = [od.synth_pair(W, H, 1, f, od.MODE_OF) for f in range(DISTINCT)]
    da = torch.from_numpy(np.stack([d[0] for d in distinct])).cuda()
    db = torch.from_numpy(np.stack([d[1] for d in distinct])).cuda()
    geo = od.out_geometry(p, W, H, grid="level")
    hl, wl = geo["out_h"], geo["out_w"]
    s = torch.cuda.current_stream().cuda_stream
    tdt = {"float32": torch.float32, "float16": torch.float16}

    for n in [int(x) for x in args.pairs.split(",")]:
        idx = torch.arange(n, device="cuda") % DISTINCT
        a, b = da[idx].contiguous(), db[idx].contiguous()
        ref = torch.empty((n, H, W, 2), dtype=torch.float32, device="cuda")   # the plain call's output, kept
        buf = torch.empty(ref.numel() * 4, dtype=torch.uint8, device="cuda")  # every way's output
        ctxs = {k: od.Context(0) for k in WAYS}
        fmts = {k: od.out_format(*v[:3]) for k, v in WAYS.items()}

        def call(k, dst=None):
            ctxs[k].run_ptr_fmt(a.data_ptr(), b.data_ptr(), n, W, H, p, fmts[k], (dst if dst is not None else buf).data_ptr(), s)

        def view(k):
            dtype, layout, grid, _ = WAYS[k]
            hh, ww = (hl, wl) if grid == "level" else (H, W)
            shape = (n, 2, hh, ww) if layout == "nchw" else (n, hh, ww, 2)
            t = buf.view(tdt[dtype])
            return t[:n * 2 * hh * ww].view(shape)

        # ---- outputs first
        call("plain", ref)
        torch.cuda.synchronize()
        cap = np.empty((hl, wl, 2), np.float32)
        ctxs["plain"].set_capture(None, {p.sc_l: cap})
        ctxs["plain"].run_host(distinct[0][0], distinct[0][1], p)
        ctxs["plain"].set_capture(None, None)
        level0 = torch.from_numpy(cap * np.float32(1 << p.sc_l)).cuda()
        for k, (dtype, layout, grid, _) in WAYS.items():
            buf.fill_(0)
            call(k)
            torch.cuda.synchronize()
            got = view(k)
            ok = True
            for f0 in range(0, n, 64):  # in pieces: the transformed reference is a copy
                g = got[f0:f0 + 64]
                if grid == "level":
                    want = level0 if layout == "nhwc" else level0.permute(2, 0, 1)
                    want = want.to(tdt[dtype])
                    first = got[:DISTINCT][idx[f0:f0 + 64]]  # the first pair made from the same images
                    ok = ok and torch.equal(g.view(torch.int16 if dtype == "float16" else torch.int32),
                                            first.view(torch.int16 if dtype == "float16" else torch.int32))
                    if f0 == 0:
                        ok = ok and torch.equal(g[0].contiguous().view(torch.int16 if dtype == "float16" else torch.int32),
                                                want.contiguous().view(torch.int16 if dtype == "float16" else torch.int32))
                else:
                    want = ref[f0:f0 + 64]
                    want = (want if layout == "nhwc" else want.permute(0, 3, 1, 2)).to(tdt[dtype]).contiguous()
                    nan = torch.isnan(want)
                    ok = ok and torch.equal(torch.isnan(g), nan) and bool(
                        ((g.view(torch.int16 if dtype == "float16" else torch.int32) ==
                          want.view(torch.int16 if dtype == "float16" else torch.int32)) | nan).all())
            if not ok:
                raise SystemExit(f"pairs {n}: way {k} differs from the plain call transformed")
        del ref
        torch.cuda.empty_cache()

        # ---- end to end
        for _ in range(3):
            for k in WAYS:
                call(k)
        torch.cuda.synchronize()
        t = {k: [] for k in WAYS}
        for _ in range(args.blocks):
            for k in WAYS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    call(k)
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) / args.calls * 1e3)
        med = {k: statistics.median(v) for k, v in t.items()}
        spread = abs(med["plain_again"] / med["plain"] - 1.0)
        emit({"what": "end_to_end", "pairs": n, "outputs_identical": True, "blocks": args.blocks,
              "calls_per_block": args.calls, "aa_spread": round(spread, 4),
              "ms": {k: round(v, 4) for k, v in med.items()},
              "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in t.items()},
              "over_plain": {k: round(med[k] / med["plain"], 4) for k in WAYS},
              "pairs_per_s": {k: round(n / med[k] * 1e3, 1) for k in WAYS}})

        # ---- the store kernels (eager issue): as issued by default (from 256 pairs two lanes) and on one lane
        for streams in (0, 1):
            if streams and n < 256:
                continue
            rec = {"what": "kernel", "pairs": n, "lanes": 1 if streams or n < 256 else 2}
            for k, (dtype, layout, grid, name) in WAYS.items():
                if k == "plain_again":
                    continue
                c = ctxs[k]
                c.set_option("streams", streams)
                call(k)  # this issue form's workspaces, outside the timers
                torch.cuda.synchronize()
                c.enable_kernel_timing(True)
                reps = 5
                for _ in range(reps):
                    call(k)
                torch.cuda.synchronize()
                ms, cnt = c.kernel_time(name)
                c.enable_kernel_timing(False)
                c.set_option("streams", 0)
                nbytes = od.algorithmic_bytes(p, W, H, name) * n * reps
                if name == "level_out" and dtype == "float16":  # the model counts a float32 write
                    nbytes *= 0.75
                gbs = nbytes / (ms * 1e-3) / 1e9
                rec[k] = {"kernel": name, "avg_launch_us": round(ms / cnt * 1e3, 2), "launches": cnt,
                          "ms_per_call": round(ms / reps, 4), "gb_s": round(gbs, 1),
                          "frac_hbm_peak": round(gbs / HBM_PEAK_GBS, 4)}
            emit(rec)
        for c in ctxs.values():
            c.close()
        del a, b, buf
        torch.cuda.empty_cache()
    if out:
        out.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A/A companion of tools/bench_sequence.py at 256 pairs: two plain contexts and a sequence context
side by side in a fresh process, alternating blocks of 8 calls, medians of 8 blocks, for four (graph, streams)
settings.  The two plain columns show what one build's identical calls differ by; the sequence column against
them is the saving.  Needs an MI355X; prints one JSON line per setting (and writes them to the file given)."""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = sys.argv[1] if len(sys.argv) > 1 else None
import torch
import of_dis_amd as od
W, H, n = 1920, 1080, 256
distinct = [od.synth_shift_pair(W, H, (0, 0), 1, 0)[0]] + [od.synth_shift_pair(W, H, (1.5 * t, -0.75 * t), 1, 0)[1] for t in range(1, 9)]
distinct = [torch.from_numpy(x).cuda() for x in distinct]
frames = torch.stack([distinct[t % 9] for t in range(n + 1)]).contiguous()
fp = frames.data_ptr()
p = od.oppoint(2, W, od.MODE_OF, 1); p.verbosity = 0
s = torch.cuda.current_stream().cuda_stream
outs = [torch.empty((n, H, W, 2), dtype=torch.float32, device="cuda") for _ in range(3)]
res = []
for graph, streams in ((1, 0), (2, 0), (1, 1), (0, 1)):
    cA, cB, cS = od.Context(0), od.Context(0), od.Context(0)
    for c in (cA, cB, cS):
        c.set_option("graph", graph); c.set_option("streams", streams)
    ways = {"plainA": lambda: cA.run_ptr(fp, fp + W * H, n, W, H, p, outs[0].data_ptr(), s),
            "sequence": lambda: cS.run_sequence_ptr(fp, n + 1, 1, W, H, p, outs[1].data_ptr(), stream=s),
            "plainB": lambda: cB.run_ptr(fp, fp + W * H, n, W, H, p, outs[2].data_ptr(), s)}
    for _ in range(3):
        for fn in ways.values(): fn()
    torch.cuda.synchronize()
    t = {k: [] for k in ways}
    for _ in range(8):
        for k, fn in ways.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(8): fn()
            torch.cuda.synchronize(); t[k].append((time.perf_counter() - t0) / 8 * 1e3)
    rec = {"pairs": n, "graph": graph, "streams": streams, **{k: round(statistics.median(v), 4) for k, v in t.items()}}
    print(json.dumps(rec), flush=True); res.append(rec)
    for c in (cA, cB, cS): c.close()
if OUT:
    json.dump(res, open(OUT, "w"), indent=1)

"""When a call records its HIP graph: one graph per context, recorded anew exactly when the call's key
-- its family, pointers, sizes, parameters and the family's own scalars -- differs bytewise from the recorded one.

OFDIS_TRACE is read once per process, so the script below runs in a child process (this file run as a program) with the
variable set.  The child writes a `step K` line to stderr before each call, the library writes one `graph: capture`
line per recording, and the test counts the captures between the step lines.  The expected counts are written next to
each step; they follow from the rule above and are not measured.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, T, NPTS = 160, 120, 4, 16  # four gray frames: three pairs; a 4 x 4 grid of points
# the two passes: the defaults (one stream, the whole batch as one graph), then two lanes of chunks of two pairs with
# their fork and join captured
PASSES = ({}, {"streams": 2, "chunk": 2, "graph": 2})
CAPTURE_OF_PASS = ("graph: capture (kind 0, 1 chunks of 3)", "graph: capture (kind 1, 2 chunks of 2)")


def script(od, ctx):
    """The steps of one pass, (label, call, graphs recorded by it), on fixed device tensors.  Every leg starts after a
    call of another family or with other arguments, so its first call records; `run` is the plain call on the frames
    as pairs."""
    import torch
    frames = torch.from_numpy(np.stack([od.synth_pair(W, H, 1, k, od.MODE_OF)[0][..., 0] for k in range(T)])).cuda()
    n, px = T - 1, W * H
    a, b = frames.data_ptr(), frames.data_ptr() + px
    p = od.oppoint(2, W, od.MODE_OF, 1)
    flow, flow_bw = (torch.empty((n, H, W, 2), dtype=torch.float32, device="cuda") for _ in range(2))
    occ_fw, occ_bw = (torch.empty((n, H, W), dtype=torch.uint8, device="cuda") for _ in range(2))
    pic = torch.empty(T * px * 4, dtype=torch.uint8, device="cuda")  # any picture below, u8 or float32
    yy, xx = np.mgrid[0:4, 0:4]
    pts = torch.from_numpy(np.stack([20.0 + 40.0 * xx.ravel(), 15.0 + 30.0 * yy.ravel()], -1).astype(np.float32)).cuda()
    tracks = torch.empty((T, NPTS, 2), dtype=torch.float32, device="cuda")
    status = torch.empty((T, NPTS), dtype=torch.uint8, device="cuda")
    keep = (frames, flow, flow_bw, occ_fw, occ_bw, pic, pts, tracks, status)
    U8, F32 = od.IMG_U8, od.IMG_F32

    def run():
        ctx.run_ptr(a, b, n, W, H, p, flow.data_ptr())

    def run_f16():
        ctx.run_ptr_fmt(a, b, n, W, H, p, od.out_format("float16"), flow.data_ptr())

    def seq(alpha=0.01, beta=0.5):
        ctx.run_sequence_ptr(frames.data_ptr(), T, 1, W, H, p, flow.data_ptr(), 0, alpha, beta, flow_bw.data_ptr(),
                             occ_fw.data_ptr(), occ_bw.data_ptr())

    def warp(scale=1.0, dtype=U8):
        ctx.run_warp_ptr(a, b, n, W, H, p, scale, dtype, pic.data_ptr())

    def interp(t=0.5, dtype=U8):
        ctx.run_interp_ptr(a, b, n, W, H, p, t, dtype, pic.data_ptr())

    def interp_occ(alpha=0.01, beta=0.5):
        ctx.run_interp_occ_ptr(a, b, n, W, H, p, 0.5, alpha, beta, U8, pic.data_ptr())

    def track(alpha=0.01, beta=0.5, flags=0):
        ctx.run_sequence_track_ptr(frames.data_ptr(), T, W, H, p, pts.data_ptr(), NPTS, 0, True, alpha, beta, flags,
                                   tracks.data_ptr(), status.data_ptr())

    def tfilter(sigma=12.0, alpha=0.01, beta=0.5, dtype=U8):
        ctx.run_sequence_tfilter_ptr(frames.data_ptr(), T, W, H, p, sigma, dtype, pic.data_ptr(), 0, True, alpha, beta)

    def leg(name, call, variants):
        """The same call twice, each keyed scalar changed in turn, the first arguments again, a plain run, the call."""
        steps = [(name, call, 1), (name + " again", call, 0)]
        steps += [(f"{name} {what}", fn, 1) for what, fn in variants]
        return steps + [(name + " first arguments", call, 1), ("run after " + name, run, 1), (name + " after run", call, 1)]

    steps = [("run", run, 1), ("run again", run, 0), ("run out dtype", run_f16, 1), ("run first arguments", run, 1)]
    steps += leg("run_sequence", seq, [("alpha", lambda: seq(alpha=0.02)), ("beta", lambda: seq(beta=0.6))])
    steps += leg("run_warp", warp, [("scale", lambda: warp(scale=0.5)), ("out dtype", lambda: warp(dtype=F32))])
    steps += leg("run_interp", interp, [("t", lambda: interp(t=0.25)), ("out dtype", lambda: interp(dtype=F32)),
                                        ("masks", interp_occ), ("masks alpha", lambda: interp_occ(alpha=0.02)),
                                        ("masks beta", lambda: interp_occ(beta=0.6))])
    steps += leg("run_sequence_track", track, [("alpha", lambda: track(alpha=0.02)), ("beta", lambda: track(beta=0.6)),
                                               ("flags", lambda: track(flags=od.TRACK_LAST))])
    steps += leg("run_sequence_tfilter", tfilter, [("sigma", lambda: tfilter(sigma=6.0)), ("alpha", lambda: tfilter(alpha=0.02)),
                                                   ("beta", lambda: tfilter(beta=0.6)), ("out dtype", lambda: tfilter(dtype=F32))])
    return steps, keep


def child():
    """Both passes in this process: a `step K EXPECTED LABEL` line on stderr before each call, the number of steps on
    stdout at the end."""
    import torch
    sys.path.insert(0, ROOT)
    import of_dis_amd as od
    ctx = od.Context(0)
    steps, keep = script(od, ctx)
    k = 0
    for options in PASSES:
        for key, value in options.items():
            ctx.set_option(key, value)  # (drops the recorded graph)
        for label, call, expect in steps:
            sys.stderr.write(f"step {k} {expect} {label}\n")
            sys.stderr.flush()
            call()
            k += 1
    torch.cuda.synchronize()
    ctx.close()
    del keep
    print(f"steps {k}")


@pytest.mark.gpu
def test_graph_records():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, OFDIS_TRACE="1"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    parts = ("\n" + r.stderr).split("\nstep ")[1:]
    assert r.stdout.split() == ["steps", str(len(parts))], r.stdout + r.stderr[-2000:]
    per_pass = len(parts) // len(PASSES)
    assert per_pass > 0 and per_pass * len(PASSES) == len(parts)
    wrong = []
    for k, part in enumerate(parts):
        head, _, trace = part.partition("\n")
        index, expect, label = head.split(" ", 2)
        assert int(index) == k
        got = trace.count("graph: capture (")
        print(f"pass {k // per_pass} {label}: recorded {got}, expected {expect}")
        # a recording is of this pass's issue kind, and it succeeds
        if got != int(expect) or got != trace.count(CAPTURE_OF_PASS[k // per_pass]) or \
                got != trace.count("graph: captured rc 0 end 0") or got != trace.count("graph: instantiated 0"):
            wrong.append((k // per_pass, label, got, int(expect)))
    assert not wrong, f"(pass, step, recorded, expected): {wrong}"


if __name__ == "__main__":
    child()

"""Point tracking, the command lines' parts that need no GPU: the usage text of run_OF_TRACK_INT / run_OF_TRACK_RGB and
their size-mismatch, points-file and no-device exits."""
import os
import subprocess

import numpy as np
import pytest

import of_dis_amd as od

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "of_dis_amd", "bin")
CLIS = ["run_OF_TRACK_INT", "run_OF_TRACK_RGB"]


@pytest.mark.parametrize("exe", CLIS)
@pytest.mark.parametrize("args", [[], ["p.txt"], ["p.txt", "t.txt", "2", "1"],
                                  ["p.txt", "t.txt", "2", "1", "a.png"],          # fewer than two frames
                                  ["p.txt", "t.txt", "5", "1", "a.png", "b.png"],  # operating point out of range
                                  ["p.txt", "t.txt", "x", "1", "a.png", "b.png"],
                                  ["p.txt", "t.txt", "2", "2", "a.png", "b.png"],  # fb is 0 or 1
                                  ["p.txt", "t.txt", "2", "", "a.png", "b.png"]])
def test_cli_usage(exe, args):
    path = os.path.join(BIN, exe)
    assert os.access(path, os.X_OK)
    r = subprocess.run([path] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stderr and "points.txt" in r.stderr


def _pnm(tmp_path, name, im):
    h, w, noc = im.shape
    head = b"P5" if noc == 1 else b"P6"
    data = im if noc == 1 else im[..., ::-1]
    (tmp_path / name).write_bytes(head + b"\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(data).tobytes())
    return str(tmp_path / name)


@pytest.mark.parametrize("exe,noc", [("run_OF_TRACK_INT", 1), ("run_OF_TRACK_RGB", 3)])
def test_cli_sizes_points_and_no_device(tmp_path, exe, noc):
    """Frames of two sizes, an unreadable or malformed points file: exit 1 with a message, before a device is looked
    for.  No visible device: a non-zero exit with the no-device message and no output file (the devices are hidden from
    the child process, so this runs the same on a GPU machine)."""
    path = os.path.join(BIN, exe)
    a, b = od.synth_pair(64, 64, noc, 0)
    small = od.synth_pair(48, 64, noc, 0)[0]
    files = [_pnm(tmp_path, "a.pnm", a), _pnm(tmp_path, "b.pnm", b), _pnm(tmp_path, "c.pnm", small)]
    pts = tmp_path / "points.txt"
    pts.write_text("# x y [start]\n3 4\n10.5 20.25 1\n\n")
    out = tmp_path / "tracks.txt"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")

    def run(points, *frames):
        return subprocess.run([path, str(points), str(out), "2", "1", *frames], capture_output=True, text=True,
                              timeout=120, env=env)

    r = run(pts, files[0], files[1])
    assert r.returncode != 0 and "no usable gfx950 device" in r.stderr and not out.exists()
    r = run(pts, files[0], files[1], "missing.png")
    assert r.returncode != 0 and "cannot read missing.png" in r.stderr and not out.exists()
    # every image's size and the points file are checked before a device is looked for
    r = run(pts, files[0], files[1], files[2])
    assert r.returncode == 1 and "image sizes differ" in r.stderr
    r = run(tmp_path / "none.txt", files[0], files[1])
    assert r.returncode == 1 and "cannot read points file" in r.stderr
    for text, where in (("1 2\n3\n", ":2"), ("1 2 3 4\n", ":1"), ("1 2 0.5\n", ":1"), ("a b\n", ":1")):
        bad = tmp_path / "bad.txt"
        bad.write_text(text)
        r = run(bad, files[0], files[1])
        assert r.returncode == 1 and f"bad.txt{where}: expected" in r.stderr, (text, r.stderr)
    empty = tmp_path / "empty.txt"
    empty.write_text("# nothing\n\n")
    r = run(empty, files[0], files[1])
    assert r.returncode == 1 and "no points" in r.stderr
    assert not out.exists()

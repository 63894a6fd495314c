"""Video sequences, the parts that need no GPU: sharding a sequence over ranks, the new entry points' argument
refusals, and the run_OF_SEQ_INT / run_OF_SEQ_RGB command lines' usage and no-device exits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import of_dis_amd as od
from of_dis_amd.distributed import shard_range, shard_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "of_dis_amd", "bin")
CLIS = ["run_OF_SEQ_INT", "run_OF_SEQ_RGB"]


@pytest.mark.parametrize("n_frames,stride,world", [(2, 1, 1), (7, 2, 3), (10, 1, 4), (10, 3, 8), (5, 4, 3), (65, 1, 8),
                                                   (4097, 1, 8), (100, 7, 6)])
def test_shard_sequence(n_frames, stride, world):
    n = n_frames - stride
    pairs = []
    for rank in range(world):
        f0, f1, p0, p1 = shard_sequence(n_frames, stride, rank, world)
        assert (p0, p1) == shard_range(n, rank, world)
        assert (f0, f1) == (p0, p1 + stride)          # the frames of its pairs: pair i reads frames i and i + stride
        assert 0 <= f0 and f1 <= n_frames
        pairs += list(range(p0, p1))
    assert pairs == list(range(n))                    # the shards tile the pairs exactly, in rank order


def test_shard_sequence_refusals():
    for n_frames, stride in ((4, 0), (4, 4), (1, 1), (3, -1)):
        with pytest.raises(ValueError):
            shard_sequence(n_frames, stride, 0, 1)
    with pytest.raises(ValueError):
        shard_sequence(8, 1, 2, 2)


def test_sequence_symbols_and_null_refusals():
    L = od.lib()
    assert len(L.ofdis_run_sequence_u8.argtypes) == 17 and len(L.ofdis_run_sequence_u8_host.argtypes) == 16
    p = od.oppoint(2, 64, od.MODE_OF, 1)
    img = np.zeros((3, 64, 64), np.uint8)
    out = np.zeros((2, 64, 64, 2), np.float32)
    INV = od._lib.ERR_INVALID_ARGUMENT
    # a NULL context is refused before anything touches a device
    assert L.ofdis_run_sequence_u8(None, img.ctypes.data, 3, 1, None, 64, 64, C.byref(p), 0.01, 0.5, out.ctypes.data,
                                   None, None, None, None, None, None) == INV
    assert L.ofdis_run_sequence_u8_host(None, img.ctypes.data, 3, 1, None, 64, 64, C.byref(p), 0.01, 0.5,
                                        out.ctypes.data, None, None, None, None, None) == INV


@pytest.mark.parametrize("exe", CLIS)
@pytest.mark.parametrize("args", [[], ["out_"], ["out_", "2", "1", "a.png"],   # too few images
                                  ["out_", "5", "1", "a.png", "b.png"],        # operating point out of range
                                  ["out_", "2", "0", "a.png", "b.png"],        # stride < 1
                                  ["out_", "2", "x", "a.png", "b.png"],
                                  ["out_", "2", "2", "a.png", "b.png"]])       # no more images than the stride
def test_cli_usage(exe, args):
    path = os.path.join(BIN, exe)
    assert os.access(path, os.X_OK)
    r = subprocess.run([path] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stderr


def _pnm(tmp_path, name, im):
    h, w, noc = im.shape
    head = b"P5" if noc == 1 else b"P6"
    data = im if noc == 1 else im[..., ::-1]
    (tmp_path / name).write_bytes(head + b"\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(data).tobytes())
    return str(tmp_path / name)


@pytest.mark.parametrize("exe,noc", [("run_OF_SEQ_INT", 1), ("run_OF_SEQ_RGB", 3)])
def test_cli_sizes_and_no_device(tmp_path, exe, noc):
    """Images of two sizes: exit 1 with a message, before a device is looked for.  No visible device: a non-zero exit
    with the no-device message and no output file (the devices are hidden from the child process, so this runs the
    same on a GPU machine)."""
    path = os.path.join(BIN, exe)
    a, b = od.synth_pair(64, 64, noc, 0)
    small = od.synth_pair(48, 64, noc, 0)[0]
    files = [_pnm(tmp_path, "a.pnm", a), _pnm(tmp_path, "b.pnm", b), _pnm(tmp_path, "c.pnm", small)]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([path, str(tmp_path / "o_"), "2", "1", files[0], files[1]], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode != 0 and "no usable gfx950 device" in r.stderr
    assert not list(tmp_path.glob("o_*"))
    r = subprocess.run([path, str(tmp_path / "o_"), "2", "1", files[0], files[1], "missing.png"], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode != 0 and not list(tmp_path.glob("o_*"))
    # every image's size is checked before a device is looked for
    r = subprocess.run([path, str(tmp_path / "o_"), "2", "1", files[0], files[1], files[2]], capture_output=True,
                       text=True, timeout=120, env=env)
    assert r.returncode == 1 and "image sizes differ" in r.stderr

"""GPU parity at the launch rules' thresholds: level sizes on, one below and one above every switch.

The refinement launches switch kernels on the level's height (and on h <= w, and on the pixel count in latency
mode).  The other parity tests reach some two dozen level heights, none of them on a threshold.  Here every call is
single-scale (sc_l = sc_f = 0, op-point 2's parameters, synth scene 3), so the one refinement level has exactly
the frame's size -- for odd sizes the only way to get there without divisibility padding -- and the sizes are the
thresholds themselves, re-derived from the launch rules:

* launch_tv_sor / sor_lanes_s / sor_lanes: G = ceil(h / 64) row groups; with S = tv_solverit sweeps the 64 S G
  threads fit 512 up to G = 4 / 2 / 2 (S = 2 / 3 / 4), 1024 up to G = 8 / 5 / 4, two rows per lane (S <= 3) up to
  G2 = ceil(h / 128) = 8 / 5, i.e. h = 1024 / 640; then sor_pipe up to h = 1024 and k_tv_sor above.  The ring
  sized to the level (S = 3, CG) switches at every G = 1 .. 5.  All of these are multiples of 64: TALL.
* smsys_rb(h) = min(16, 1024 / h) steps after h = 64, 68, 73, 78, 85, 93, 102, 113, 128, 146, 170, 204, 256;
  smsys_rowblock_fits ends at 256 (rb < 4) and the march / 2-D tiles start at 257; smsys_rb_n's latency-regime
  rows ceil(256 / h) reach their floor of 4 at h = 64; smsys_rb_df's 40 KB cap, h (32 rb + 120) <= 40960, takes
  rb from 4 to 3 after h = 165 and to 2 (tv_deriv_fused false: eight planes again) after h = 189; with
  smsys_small = 0 the same cap trims smsys_rb's own rows (first at h = 73).  launch_tv_prepd takes 32-row tiles from h = 256: SYSTEM.
* the plane folds when h <= w (skw / skew_xy, smsys_rows = w instead of w + h - 1): FOLD.
* march_strips = ceil(h / 60), march_segments = ceil(rows / 64) for h >= 257: MARCH.
* tv_level_rb_ok (sor_mode = 1) ends at w h = 8192 pixels: LATENCY.
* launch_tv_sor's `tiny` (w < 2 or h < 2: point SOR, k_tv_sor<1>) and levels smaller than the patch: SMALL.
"""
import numpy as np
import pytest

from test_gpu_parity import _bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def od():
    import of_dis_amd
    return of_dis_amd


@pytest.fixture(scope="module")
def ctx(od):
    c = od.Context(0)
    yield c
    c.close()


_REF = {}


def _params(od, O, w, noc, mode, sc, over):
    p, q = od.oppoint(2, w, mode, noc), O.oppoint(2, w, mode, noc)
    for r in (p, q):
        r.sc_f, r.sc_l = sc
        for k, v in over.items():
            setattr(r, k, v)
    return p, q


def _reference(od, O, w, h, noc, mode, sc, over, order):
    """The oracle's flow of one size, computed once per module and shared by the option legs."""
    key = (w, h, noc, mode, sc, tuple(sorted(over.items())), order)
    if key not in _REF:
        a, b = od.synth_pair(w, h, noc, 3, mode)
        with O.sor_order(order):
            ref = O.run_u8(a, b, _params(od, O, w, noc, mode, sc, over)[1])
        ref.setflags(write=False)
        _REF[key] = (a, b, ref)
    return _REF[key]


def sweep(od, O, ctx, sizes, mode, noc=1, over=None, options=(), sc=(0, 0), order=0):
    """Every (w, h) of `sizes` under `options`; one assertion that lists every size that differs."""
    over = over or {}
    for k, v, _ in options:
        ctx.set_option(k, v)
    bad = []
    try:
        for w, h in sizes:
            a, b, ref = _reference(od, O, w, h, noc, mode, sc, over, order)
            p = _params(od, O, w, noc, mode, sc, over)[0]
            assert od.validate(p) == 0
            got = ctx.run_host(a, b, p)
            assert got.shape == ref.shape, (w, h, got.shape, ref.shape)
            assert np.isfinite(ref).all(), (w, h)
            n = int((_bits(got) != _bits(ref)).sum())
            if n:
                d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
                bad.append(f"{w}x{h}: {n} / {ref.size} values differ, max |d| = {np.nanmax(d):.3g}")
    finally:
        for k, _, d in options:
            ctx.set_option(k, d)
    assert not bad, f"mode {mode} noc {noc} {over} {[o[:2] for o in options]} sc {sc}:\n" + "\n".join(bad)


MODES = [pytest.param(1, id="flow"), pytest.param(2, id="depth")]

# h = 64 k - 1, 64 k, 64 k + 1: every row-group count G = 1 .. 16 and G + 1 at its first height.  Per S:
#   S = 2: 512 threads to h = 256, 1024 threads to h = 512, two rows per lane to h = 1024
#   S = 3: 512 threads to h = 128, 1024 threads to h = 320 (ring sized to G = 1 .. 5), two rows per lane to h = 640,
#          register pipeline (sor_pipe) to h = 1024
#   S = 4: 512 threads to h = 128, 1024 threads to h = 256 (lanes_fit: 4 G <= 16), register pipeline to h = 1024
#   every S: k_tv_sor (generic) at h = 1025; sor_pipe's 256 / 512 / 1024-thread forms switch at h = 256, 512
#   also smsys_rb 16 -> 15 (64 | 65), 8 -> 7 (128 | 129), row blocks -> march and prepd's 32-row tiles (255 | 256 | 257)
TALL = [(24, 64 * k + d) for k in range(1, 17) for d in (-1, 0, 1)]


@pytest.mark.parametrize("cring", [2, 3])
@pytest.mark.parametrize("solverit", [2, 3, 4])
@pytest.mark.parametrize("mode", MODES)
def test_tall_sweep(oracle, od, ctx, mode, solverit, cring):
    """sor_cring = 3 puts the clamped in-frame loads (lanes past the last row read row h - 1) on every launch."""
    sweep(od, oracle, ctx, TALL, mode, over={"tv_solverit": solverit}, options=[("sor_cring", cring, 2)])


SYSTEM = [(24, h) for h in (
    68, 69,      # smsys_rb 15 -> 14
    73, 74,      # 14 -> 13
    78, 79,      # 13 -> 12
    85, 86,      # 12 -> 11; smsys_rb_n: ceil(256 / h) 4 -> 3 (floored at 4)
    93, 94,      # 11 -> 10
    102, 103,    # 10 -> 9
    113, 114,    # 9 -> 8
    146, 147,    # 7 -> 6
    165, 166,    # smsys_rb_df: the 40 KB cap takes the latency regime's 4 rows to 3
    170, 171,    # 6 -> 5
    180, 181,    # inside the capped range (3 rows per block)
    189, 190,    # smsys_rb_df 3 -> 2: tv_deriv_fused false, prepd writes all eight planes
    204, 205,    # 5 -> 4
    255, 256, 257,  # smsys_rowblock_fits ends (rb 4 -> 3): march; launch_tv_prepd's TH = 32 from 256
)]


@pytest.mark.parametrize("deriv", [1, 0])
@pytest.mark.parametrize("small", [1, 0])
@pytest.mark.parametrize("mode", MODES)
def test_system_kernel_steps(oracle, od, ctx, mode, small, deriv):
    sweep(od, oracle, ctx, SYSTEM, mode, options=[("smsys_small", small, 1), ("smsys_deriv", deriv, 1)])


FOLD = [(63, 64), (64, 64), (65, 64), (64, 63), (64, 65),     # wrap = h <= w, at smsys_rb's first step
        (128, 128), (128, 129), (129, 128),                   # ... at 8 -> 7 rows, G 2 -> 3
        (256, 256), (256, 257), (257, 256),                   # ... at the row blocks' end
        (320, 63), (320, 64), (320, 65), (320, 128), (320, 129), (320, 256),  # folded, w a multiple of 64
        (320, 257), (321, 257)]                               # folded march: rows = w on / past a segment
FOLD_RGB = [(64, 64), (64, 65), (129, 128)]


@pytest.mark.parametrize("mode", MODES)
def test_fold_boundary(oracle, od, ctx, mode):
    sweep(od, oracle, ctx, FOLD, mode)


@pytest.mark.parametrize("mode", MODES)
def test_fold_boundary_rgb(oracle, od, ctx, mode):
    sweep(od, oracle, ctx, FOLD_RGB, mode, noc=3)


# unfolded (h > w): rows = w + h - 1; march_segments = ceil(rows / 64), march_strips = ceil(h / 60)
MARCH = [(64, 257), (65, 257),    # 5 strips; rows 320 (5 segments) | 321 (6)
         (21, 300), (22, 300),    # 5 strips exactly; rows 320 | 321
         (20, 301), (21, 301),    # 6 strips, one column in the last; rows 320 | 321
         (65, 320), (66, 320),    # rows 384 | 385; S = 3's last one-row-per-lane height
         (64, 321), (65, 321)]    # rows 384 | 385; two rows per lane


@pytest.mark.parametrize("deriv", [1, 0])
@pytest.mark.parametrize("mode", MODES)
def test_march_strips_and_segments(oracle, od, ctx, mode, deriv):
    sweep(od, oracle, ctx, MARCH, mode, options=[("smsys_deriv", deriv, 1)])


def test_march_strips_and_segments_rgb(oracle, od, ctx):
    sweep(od, oracle, ctx, MARCH[:6], 1, noc=3)


LATENCY = [(64, 128), (64, 129), (128, 64), (129, 64), (90, 91), (91, 91)]  # 8192 | 8256 | 8190 | 8281 pixels


@pytest.mark.parametrize("mode", MODES)
def test_latency_mode_pixel_cap(oracle, od, ctx, mode):
    """sor_mode = 1 at tv_level_rb_ok's 8192 pixels: the one-launch level on one side, the per-launch red-black
    kernels on the other, both the oracle's red-black order."""
    sweep(od, oracle, ctx, LATENCY, mode, options=[("sor_mode", 1, 0)], order=1)


# (sc_l, sc_f) -> frames.  Levels reached: 1 x 1, 1 x k, k x 1 (launch_tv_sor's `tiny` point SOR for flow; depth
# keeps its own point SOR on the sweep-per-wave kernel), 2 x 2 and 3 x 2 (the smallest block SOR), and levels
# narrower or shorter than the 8-pixel patch and the 4-pixel grid step (a single patch column / row).
SMALL = {
    (0, 0): [(8, 8), (9, 8), (8, 9), (7, 1), (1, 7), (2, 2), (1, 1), (3, 2)],
    (1, 3): [(16, 16), (8, 32)],                      # 8, 4, 2 squared; 4 x 16, 2 x 8, 1 x 4
    (0, 3): [(8, 8), (16, 8), (8, 16), (32, 8), (40, 24)],  # down to 1 x 1, 2 x 1, 1 x 2, 4 x 1, 5 x 3
    (0, 2): [(24, 16)],                               # 24 x 16, 12 x 8, 6 x 4
}


# Flow from an 8 x 8 frame at sc 0..3 has no defined result: the point SOR of its 1 x 1 level (raw 2 x 2 system, no
# neighbours, zero image derivatives) divides 0 by 0, and the next level's patches start at a NaN position, which
# passes the bounds test (every comparison false) into (int)ceil(NaN) -- undefined in the reference's text, a wild
# read in it and in the oracle.  Depth keeps the case (its 1 x 1 level stays finite); flow reaches 1 x 1 at sc 0..0.
NO_REFERENCE = {(1, (0, 3)): [(8, 8)]}


@pytest.mark.parametrize("sc", sorted(SMALL), ids=lambda s: f"sc{s[0]}..{s[1]}")
@pytest.mark.parametrize("mode", MODES)
def test_small_frames(oracle, od, ctx, mode, sc):
    """Levels smaller than a patch, one pixel wide or high, and 1 x 1.

    Why every access stays inside the padded pyramid and the planes (read from the kernels, all forms alike):
    * patches: a sample position is tested against [-p/2, w + p/2 - 2] x [-p/2, h + p/2 - 2] (LevelGeom::tmp_lb /
      tmp_ub*) before it is sampled, so the (p + 1)^2 taps lie in rows and columns pad - p .. pad + w - 1 + p - 1 of
      a level padded by pad >= p whatever w and h are; the template sits on a grid point inside the level.  The
      windowed forms' 16-byte row loads overrun a row by at most 3 floats (the 64 floats after each image array).
      The coarser flow is read at floor(pt / 2) <= w / 2 - 1 (every level but the coarsest is even).  Aggregation
      weights and the aggregation itself test 0 <= x < w, 0 <= y < h per pixel; the staged patch range is clamped
      to the grid.
    * prep and derivative tiles clamp every halo position into the level before the (clamped) bilinear read; the
      pyramid kernels clamp or reflect (reflect101 returns 0 for one pixel).
    * the fused system kernel stages plane rows r0 - 2 .. r0 + rb + 1: a negative folded row is skipped, one past
      the fold (at most 17 - w for w <= 16, h <= w) reads slot (18 - w) h - 1 <= w h + 63, inside the plane's 64
      dump slots, and is never used by a row that exists; stores test the row.  The SOR kernels clamp the row of
      every load into the plane (sor_row2, yc) -- the lower neighbour's + 1 is the first dump slot -- and store
      only where 0 <= x < w and y < h; k_tv_sor reads clamped coordinates.
    """
    sc_l, sc_f = sc
    sizes = [s for s in SMALL[sc] if s not in NO_REFERENCE.get((mode, sc), ())]
    sweep(od, oracle, ctx, sizes, mode, sc=(sc_f, sc_l))

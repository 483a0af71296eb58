"""The host restatement of the ball morphology (tests/morph_ref.py: scipy with an explicitly built ball) against a brute-force
float32 field -- cfun_morph.h's g1 -> g2 -> g3 with the virtual seeds, every operation rounded to float32 -- and against answers
written down by hand.  CPU only, no library: this is what pins the definition the device is then held to."""
import math

import numpy as np
import pytest

import morph_ref as mr

F = np.float32
LITS = (1.50625819, 0.79272507, 0.79272507)
# the seven spacing / radius pairs the definition was checked on
PAIRS = [((1.0, 1.0, 1.0), 0.5), ((1.0, 1.0, 1.0), 1.0), ((1.0, 1.0, 1.0), 2.0), ((1.5, 0.75, 0.75), 2.25), (LITS, 3.0),
         ((2.5, 0.7, 0.7), 1.0), ((5.0, 1.0, 1.0), 3.0)]


def _sweep(g, axis, a2, virt):
    """min over j of fl(g[j] + fl(float((i - j)^2) * a2)) along ``axis``; with ``virt`` also fl(float(k * k) * a2) for
    k = min(i + 1, L - i).  The first sweep is this with g = 0 on the seeds and +inf elsewhere: fl(0 + t) = t."""
    g = np.moveaxis(g, axis, -1)
    n = g.shape[-1]
    i = np.arange(n)
    t = mr.term(np.abs(i[:, None] - i[None, :]), a2)                   # [i, j]
    with np.errstate(invalid="ignore"):
        out = (g[..., None, :] + t).astype(F).min(axis=-1)
    if virt:
        out = np.minimum(out, mr.term(np.minimum(i + 1, n - i), a2))
    return np.moveaxis(out, -1, axis)


def field(seeds, spacing, virt):
    (sz2, sy2, sx2), _ = mr.squares(spacing, 0.0)
    g = np.where(seeds, F(0), F(np.inf)).astype(F)
    g = _sweep(g, 2, sx2, virt)
    g = _sweep(g, 1, sy2, virt)
    return _sweep(g, 0, sz2, virt)


def brute(obj, op, spacing, radius, outside):
    _, r2 = mr.squares(spacing, radius)

    def dil(o):
        return field(o, spacing, False) <= r2

    def ero(o):
        return o & ~(field(~o, spacing, not outside) <= r2)
    return {"erode": lambda: ero(obj), "dilate": lambda: dil(obj), "open": lambda: dil(ero(obj)),
            "close": lambda: ero(dil(obj))}[op]()


@pytest.mark.parametrize("spacing,radius", PAIRS, ids=lambda v: str(v).replace(" ", ""))
def test_restatement_equals_brute_force_field(spacing, radius):
    n = int(mr.ball(spacing, radius).sum())
    rng = np.random.default_rng(int(radius * 100) + n)
    p = 1.0 - 0.5 ** (1.0 / n)
    for density in (p, 1.0 - p):
        obj = rng.random((9, 12, 17)) < density
        for op in mr.OPS:
            for outside in (0, 1):
                want = brute(obj, op, spacing, radius, outside)
                got = mr.binary(obj, mr.ball(spacing, radius), op, outside)
                assert np.array_equal(got, want), (spacing, radius, op, outside, density)


def test_ball_sizes():
    assert [int(mr.ball((1, 1, 1), r).sum()) for r in (0.5, 1, 1.5, 1.8, 2, 3)] == [1, 7, 19, 27, 33, 123]
    assert int(mr.ball((1, 1, 1), math.sqrt(2)).sum()) == 19               # the double sqrt(2)^2 rounds to the float32 2: "<=" decides
    assert int(mr.ball(LITS, 3.0).sum()) == 119
    assert mr.ball((3, 1, 1), 2.0).shape == (1, 5, 5) and mr.ball((5, 1, 1), 0.5).shape == (1, 1, 1)


def one_voxel(n=11):
    v = np.zeros((n, n, n), np.uint8)
    v[n // 2, n // 2, n // 2] = 1
    return v


def cube(lo=3, hi=8, n=11, value=1):
    v = np.zeros((n, n, n), np.uint8)
    v[lo:hi, lo:hi, lo:hi] = value
    return v


def spur_cube():
    """The 5^3 cube with a three-voxel spur on a face centre: 128 voxels."""
    v = cube()
    v[5, 5, 8:11] = 1
    assert int(v.sum()) == 128
    return v


def two_blocks():
    """Two 5 x 5 x 3 blocks one voxel apart along x: 150 voxels."""
    v = np.zeros((9, 9, 11), np.uint8)
    v[2:7, 2:7, 2:5] = 1
    v[2:7, 2:7, 6:9] = 1
    assert int(v.sum()) == 150
    return v


def nested():
    """LiTS in small: a liver shell (1) from 2 to 10 with a hollow 4 .. 8 that holds a tumour block (2) at 5 .. 7."""
    v = np.zeros((13, 13, 13), np.uint8)
    v[2:11, 2:11, 2:11] = 1
    v[4:9, 4:9, 4:9] = 0
    v[5:8, 5:8, 5:8] = 2
    return v


def test_one_voxel_dilated():
    for r, n in ((1, 7), (1.5, 19), (1.8, 27), (2, 33)):
        out, stats = mr.morph(one_voxel(), 2, "dilate", r)
        assert int(out.sum()) == n and stats.tolist() == [[0, 0], [0, n - 1]]
    out, stats = mr.morph(one_voxel(), 2, "dilate", 2, spacing=(3, 1, 1))
    assert int(out.sum()) == 13 and int(out[5].sum()) == 13 and stats.tolist() == [[0, 0], [0, 12]]


def test_cube_eroded():
    out, stats = mr.morph(cube(), 2, "erode", 1)
    assert int(out.sum()) == 27 and bool(out[4:7, 4:7, 4:7].all()) and stats.tolist() == [[0, 0], [98, 0]]
    corner = cube(0, 5)
    out, _ = mr.morph(corner, 2, "erode", 1, outside=0)
    assert int(out.sum()) == 27 and bool(out[1:4, 1:4, 1:4].all())
    out, _ = mr.morph(corner, 2, "erode", 1, outside=1)
    assert int(out.sum()) == 64 and bool(out[0:4, 0:4, 0:4].all())
    assert np.array_equal(mr.morph(corner, 2, "erode", 1)[0], mr.morph(corner, 2, "erode", 1, outside=0)[0])     # the default


def test_spur_opened():
    out, stats = mr.morph(spur_cube(), 2, "open", 1)
    assert int(out.sum()) == 82 and stats.tolist() == [[0, 0], [46, 0]]
    assert out[5, 5, 8] == 1 and out[5, 5, 9] == 0 and out[5, 5, 10] == 0
    assert out[3, 3, 5] == 0 and out[3, 5, 5] == 1                     # an edge goes, a face stays
    assert not bool((out > spur_cube()).any())                         # a subset


def test_closed():
    holed = cube()
    holed[5, 5, 5] = 0
    out, stats = mr.morph(holed, 2, "close", 1)
    assert np.array_equal(out, cube()) and stats.tolist() == [[0, 0], [0, 1]]
    out, stats = mr.morph(two_blocks(), 2, "close", 1)
    assert int(out.sum()) == 159 and bool(out[3:6, 3:6, 5].all()) and int(out[:, :, 5].sum()) == 9
    assert stats.tolist() == [[0, 0], [0, 9]]
    # the corner cube with outside = 0: the binary closing loses the voxels near the faces, the map does not
    corner = cube(0, 5)
    b = mr.ball((1, 1, 1), 1)
    assert int(mr.binary(corner > 0, b, "close", 0).sum()) == 64
    out, stats = mr.morph(corner, 2, "close", 1, outside=0)
    assert np.array_equal(out, corner) and not stats.any()
    out, stats = mr.morph(corner, 2, "close", 1)                       # the default: outside = 1
    assert np.array_equal(out, corner) and not stats.any()


def mixed(seed=5, shape=(7, 8, 9)):
    """Background 20 %, liver 40 %, tumour 40 %, voxel by voxel: zero voxels that both classes' closings claim."""
    return np.random.default_rng(seed).choice(np.arange(3, dtype=np.uint8), size=shape, p=(0.2, 0.4, 0.4))


def test_highest_class_wins():
    for v, op in ((nested(), "dilate"), (mixed(), "dilate"), (mixed(), "close")):
        out, stats = mr.morph(v, 3, op, 1)
        assert np.array_equal(out[v != 0], v[v != 0])                  # no liver voxel, no tumour voxel rewritten
        alone2, s2 = mr.morph(v, 3, op, 1, classes=2)
        alone1, s1 = mr.morph(v, 3, op, 1, classes=(1,))
        claimed2, claimed1 = (alone2 == 2) & (v == 0), (alone1 == 1) & (v == 0)
        assert bool((claimed1 & claimed2).any()), "test setup: nothing is contested"
        assert bool((out[claimed2] == 2).all()) and bool((out[claimed1 & ~claimed2] == 1).all())
        assert stats[2, 1] == s2[2, 1] == int(claimed2.sum()) and stats[1, 1] == int((claimed1 & ~claimed2).sum()) < s1[1, 1]
        assert not stats[:, 0].any() and not stats[0].any()
    # by hand.  Dilate: the tumour block gains its 54 face neighbours; the liver gains 6 * 81 outside and, of the 98 voxels of
    # the gap between it and the tumour, the 44 on the gap's edges and corners -- the other 54 are the tumour's.
    v = nested()
    out, stats = mr.morph(v, 3, "dilate", 1)
    assert stats.tolist() == [[0, 0], [0, 6 * 81 + 44], [0, 54]]
    assert out[4, 6, 6] == 2 and out[4, 4, 4] == 1 and out[1, 6, 6] == 1 and out[0, 6, 6] == 0
    # Close: the tumour's closing is the tumour; the liver's closes those same 44 (a ball centred on a tumour voxel holds no liver)
    out, stats = mr.morph(v, 3, "close", 1)
    assert stats.tolist() == [[0, 0], [0, 44], [0, 0]] and out[4, 6, 6] == 0 and out[4, 4, 4] == 1


def test_foreground_and_fill_value():
    v = nested()
    for value in (1, 7, 255):
        out, stats = mr.morph(v, 3, "dilate", 1, by="foreground", fill_value=value)
        put = (out != v)
        assert bool((out[put] == value).all()) and bool((v[put] == 0).all()) and stats.tolist() == [[0, int(put.sum())], [0, 0], [0, 0]]
        want = mr.dilate(v != 0, mr.ball((1, 1, 1), 1))
        assert np.array_equal(out != 0, want)
    out, stats = mr.morph(v, 3, "erode", 1, by="foreground", fill_value=9)      # clears: the value is not used
    assert np.array_equal(out != 0, mr.erode(v != 0, mr.ball((1, 1, 1), 1), 0)) and stats[0, 0] == int(((out == 0) & (v != 0)).sum())
    assert np.array_equal(out[out != 0], v[out != 0])


def test_selected_classes_and_bytes_beyond_k():
    v = nested()
    out, stats = mr.morph(v, 3, "erode", 1, classes=(2,))
    assert np.array_equal(out == 1, v == 1) and int((out == 2).sum()) == 1 and stats.tolist() == [[0, 0], [0, 0], [26, 0]]
    w = v.copy()
    w[v == 2] = 9                                                      # a byte >= K: complement in class mode, copied through
    out, stats = mr.morph(w, 3, "open", 1)
    assert np.array_equal(out == 9, w == 9) and not stats[2].any() and not stats[0].any()
    out, stats = mr.morph(w, 3, "dilate", 1)
    assert np.array_equal(out == 9, w == 9) and not stats[2].any() and stats[1, 1] > 0
    out, stats = mr.morph(w, 3, "erode", 1, by="foreground")           # ... and object like any other in foreground mode
    assert out[6, 6, 6] == 9 and stats[0, 0] == int(((out == 0) & (w != 0)).sum())


def test_radius_below_every_spacing_is_the_identity():
    v = nested()
    for op in mr.OPS:
        for by in ("class", "foreground"):
            for spacing, r in (((1, 1, 1), 0.99), ((1.5, 0.8, 0.8), 0.79), ((1, 1, 1), 0.0)):
                out, stats = mr.morph(v, 3, op, r, spacing, by)
                assert np.array_equal(out, v) and not stats.any()

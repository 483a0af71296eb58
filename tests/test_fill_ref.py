"""tests/fill_ref.py against answers written by hand: the device tiers compare against that file, so it is checked on its own.
Most cases live in a 7^3 volume holding a 5^3 shell of class 1 at 1 .. 5 (walls one voxel thick, interior 3^3 at 2 .. 4)."""
import numpy as np
import pytest

import fill_ref as fr


def shell(n=7, lo=1, hi=5, value=1):
    v = np.zeros((n, n, n), np.uint8)
    v[lo:hi + 1, lo:hi + 1, lo:hi + 1] = value
    v[lo + 1:hi, lo + 1:hi, lo + 1:hi] = 0
    return v


def nested():
    """9^3: a class-1 shell at 1 .. 7 (interior 5^3), inside it a class-2 shell at 3 .. 5 around the one voxel (4,4,4); background
    in that cavity and in the gap between the two shells (5^3 - 3^3 = 98 voxels)."""
    v = shell(9, 1, 7, 1)
    v[3:6, 3:6, 3:6] = 2
    v[4, 4, 4] = 0
    return v


@pytest.mark.parametrize("conn", (6, 26))
@pytest.mark.parametrize("by", ("class", "foreground"))
def test_closed_shell(conn, by):
    v = shell()
    out, stats = fr.fill(v, 2, by, conn)
    want = v.copy()
    want[2:5, 2:5, 2:5] = 1
    assert out.dtype == np.uint8 and stats.dtype == np.int64 and stats.shape == (2, 2)
    assert np.array_equal(out, want) and int((out != v).sum()) == 27
    assert stats.tolist() == ([[0, 0], [1, 27]] if by == "class" else [[1, 27], [0, 0]])


def test_pinhole_in_a_plate():
    """The centre voxel (1,3,3) of the z = 1 plate removed: in 3-D the interior is open under either neighbourhood.  Slice by
    slice along axis 0 the rings at z = 2, 3, 4 are closed: 27 voxels in 3 components -- and the pinhole itself is a hole of
    the z = 1 plane (the plate surrounds it within that plane): one more voxel, one more component.  Along axis 1 the planes
    y = 2 and y = 4 hold closed rings; the plane y = 3 holds the ring with the gap."""
    v = shell()
    v[1, 3, 3] = 0
    for conn in (6, 26):
        out, stats = fr.fill(v, 2, "class", conn)
        assert np.array_equal(out, v) and stats.tolist() == [[0, 0], [0, 0]]
    for conn in (4, 8):
        out, stats = fr.fill(v, 2, "class", conn, axis=0)
        rings = v.copy()
        rings[2:5, 2:5, 2:5] = 1
        assert int((rings != v).sum()) == 27
        want = rings.copy()
        want[1, 3, 3] = 1
        assert np.array_equal(out, want) and stats.tolist() == [[0, 0], [3 + 1, 27 + 1]]
        _, count = fr.group_holes(v[2:5] == 1, conn, axis=0)          # the three ring planes alone
        assert count == 3
    out, stats = fr.fill(v, 2, "class", 4, axis=1)
    want = v.copy()
    want[2:5, 2, 2:5] = 1
    want[2:5, 4, 2:5] = 1
    assert np.array_equal(out, want) and stats.tolist() == [[0, 0], [2, 18]]


def test_gap_on_an_edge():
    """The edge voxel (1,1,3) removed: its face neighbours are shell or outside, so under 6 the interior stays closed; under 26 the
    interior voxel (2,2,3) touches the gap across an edge."""
    v = shell()
    v[1, 1, 3] = 0
    out, stats = fr.fill(v, 2, "class", 6)
    want = v.copy()
    want[2:5, 2:5, 2:5] = 1
    assert np.array_equal(out, want) and want[1, 1, 3] == 0 and stats.tolist() == [[0, 0], [1, 27]]
    out, stats = fr.fill(v, 2, "class", 26)
    assert np.array_equal(out, v) and stats.tolist() == [[0, 0], [0, 0]]


def test_nested_classes_highest_id_wins():
    v = nested()
    assert int((v == 0)[2:7, 2:7, 2:7].sum()) == 98 + 1
    for conn in (6, 26):
        out, stats = fr.fill(v, 3, "class", conn)
        want = v.copy()
        want[2:7, 2:7, 2:7][v[2:7, 2:7, 2:7] == 0] = 1                # the gap: liver
        want[4, 4, 4] = 2                                             # the cavity of the class-2 shell: class 2, not 1
        assert np.array_equal(out, want) and np.array_equal(out == 2, (v == 2) | (want == 2))
        assert np.array_equal(out[v != 0], v[v != 0])                 # no non-zero byte rewritten
        # class 2 encloses one component (the cavity, 1 voxel).  Class 1 encloses ONE component -- gap, class-2 shell and
        # cavity hang together in pred != 1 -- of which the 98 gap voxels change; the cavity went to class 2
        assert stats.tolist() == [[0, 0], [1, 98], [1, 1]]
        out, stats = fr.fill(v, 3, "foreground", conn, fill_value=7)
        want = v.copy()
        want[2:7, 2:7, 2:7][v[2:7, 2:7, 2:7] == 0] = 7
        assert np.array_equal(out, want) and stats.tolist() == [[2, 99], [0, 0], [0, 0]]
    # slice by slice: z = 2, 6: 25 voxels each; z = 3, 5: 25 - 9 (a solid class-2 plate); z = 4: 25 - 9 and the cavity
    out, stats = fr.fill(v, 3, "class", 4, axis=0)
    assert np.array_equal(out, fr.fill(v, 3, "class", 6)[0])
    assert stats.tolist() == [[0, 0], [5, 2 * 25 + 3 * 16], [1, 1]]


def test_blob_of_another_class_is_an_enclosed_component_that_changes_nothing():
    v = np.zeros((7, 7, 7), np.uint8)
    v[1:6, 1:6, 1:6] = 1
    v[2:5, 2:5, 2:5] = 2
    for conn in (6, 26):
        out, stats = fr.fill(v, 3, "class", conn)
        assert np.array_equal(out, v) and stats.tolist() == [[0, 0], [1, 0], [0, 0]]
        out, stats = fr.fill(v, 3, "foreground", conn)
        assert np.array_equal(out, v) and not stats.any()


def test_bytes_beyond_k():
    v = shell()
    v[3, 3, 3] = 9                                                    # K = 3: in class 1's complement, and foreground
    out, stats = fr.fill(v, 3, "class", 6)
    want = v.copy()
    want[2:5, 2:5, 2:5] = 1
    want[3, 3, 3] = 9
    assert np.array_equal(out, want) and stats.tolist() == [[0, 0], [1, 26], [0, 0]]
    out, stats = fr.fill(v, 3, "foreground", 6, fill_value=255)
    want[want == 1] = np.where(v[want == 1] == 0, 255, 1)
    assert np.array_equal(out, want) and stats.tolist() == [[1, 26], [0, 0], [0, 0]]
    w = shell(5, 1, 3, 9)                                             # a shell of the unknown byte around (2,2,2)
    out, stats = fr.fill(w, 3, "class", 6)
    assert np.array_equal(out, w) and not stats.any()                 # no group's object: nothing encloses
    out, stats = fr.fill(w, 3, "foreground", 6, fill_value=2)
    assert out[2, 2, 2] == 2 and int((out != w).sum()) == 1 and stats.tolist() == [[1, 1], [0, 0], [0, 0]]


def test_empty_full_and_single_voxel():
    for by in ("class", "foreground"):
        for conn, axis in ((6, None), (26, None), (4, 0), (8, 1), (4, 2)):
            for v in (np.zeros((3, 4, 5), np.uint8), np.ones((3, 4, 5), np.uint8), np.zeros((1, 1, 1), np.uint8),
                      np.ones((1, 1, 1), np.uint8)):
                out, stats = fr.fill(v, 2, by, conn, axis)
                assert np.array_equal(out, v) and stats.shape == (2, 2) and not stats.any()
    out, stats = fr.fill(np.zeros((0, 3, 4), np.uint8), 4)
    assert out.shape == (0, 3, 4) and stats.shape == (4, 2) and not stats.any()


def test_plane_of_extent_one_is_all_border():
    v = np.ones((3, 1, 7), np.uint8)
    v[:, 0, 3] = 0                                                    # walled in along x, but y has extent 1
    for axis, conns in ((None, (6, 26)), (0, (4, 8)), (2, (4, 8)), (1, (4, 8))):
        for conn in conns:
            out, stats = fr.fill(v, 2, "class", conn, axis)
            assert np.array_equal(out, v) and not stats.any(), (axis, conn)
    v[0, 0, 3] = v[2, 0, 3] = 1                                       # now (1,0,3) is walled in within the plane y = 0 ...
    out, stats = fr.fill(v, 2, "class", 4, axis=1)
    assert out[1, 0, 3] == 1 and stats.tolist() == [[0, 0], [1, 1]]   # ... whose edges are z = 0, 2 and x = 0, 6
    for axis, conn in ((None, 6), (0, 4), (2, 4)):                    # every other way y = 0 is an edge (or a face)
        out, stats = fr.fill(v, 2, "class", conn, axis)
        assert np.array_equal(out, v) and not stats.any()


def test_defaults_and_open_side():
    v = shell()
    assert np.array_equal(fr.fill(v, 2)[0], fr.fill(v, 2, "class", 6)[0])
    assert np.array_equal(fr.fill(v, 2, axis=0)[1], fr.fill(v, 2, "class", 4, axis=0)[1])
    assert fr.open_components(v, 2, "class", 6).tolist() == [0, 1]
    assert fr.open_components(v, 2, "class", 4, axis=0).tolist() == [0, 7]

"""TEST ONLY: numpy float64 restatement of the rule of include/cfun_sample_warp.h -- the control coordinate, the trilinear
displacement, the in-plane map, the flips, the nearest and the trilinear sample, and the box.  Written from the header, not from
the kernel; the box is sample_ref's.  tests/test_sample_warp_ref.py holds it to scipy.ndimage.map_coordinates and to hand
answers, tests/sample_warp_cases.py holds the kernels to it."""
import numpy as np

import sample_ref as sr


def lerp(a, b, t):
    return (1.0 - t) * a + t * b


def control(n, g):
    """Step 1 on one axis: (i int64 [n], t float64 [n])."""
    o = np.arange(n, dtype=np.float64)
    q = np.float64(0.0) if n == 1 else np.float64(g - 1) / np.float64(n - 1)
    u = o * q
    i = np.minimum(np.floor(u), np.float64(g - 2))
    return i.astype(np.int64), u - i


def displacement(grid, zs, dims):
    """Step 2: float64 [3, len(zs), H, W] from a float32 [3,gz,gy,gx] grid."""
    grid = np.asarray(grid, np.float32)
    (iz, tz), (iy, ty), (ix, tx) = [control(n, g) for n, g in zip(dims, grid.shape[1:])]
    iz, tz = iz[zs][:, None, None], tz[zs][:, None, None]
    iy, ty = iy[None, :, None], ty[None, :, None]
    ix, tx = ix[None, None, :], tx[None, None, :]
    out = []
    for c in range(3):
        v = grid[c].astype(np.float64)
        f = []
        for dz in (0, 1):
            e = [lerp(v[iz + dz, iy + dy, ix], v[iz + dz, iy + dy, ix + 1], tx) for dy in (0, 1)]
            f.append(lerp(e[0], e[1], ty))
        out.append(lerp(f[0], f[1], tz))
    return np.stack(out)


def coords(dims, grid=None, amap=None, flips=(False, False, False), planes=None):
    """Steps 1 to 5: the source coordinate stack float64 [3, len(planes), H, W] (z, y, x)."""
    d, h, w = [int(v) for v in dims]
    zs = np.arange(d) if planes is None else np.asarray(planes, np.int64)
    p = np.stack(np.broadcast_arrays(zs.astype(np.float64)[:, None, None], np.arange(h, dtype=np.float64)[None, :, None],
                                     np.arange(w, dtype=np.float64)[None, None, :])).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        if grid is not None:
            p = p + displacement(grid, zs, (d, h, w))                          # step 3
        s = p
        if amap is not None:                                                   # step 4
            m = [np.float64(v) for v in amap]
            col = m[0] * p[2] + m[1] * p[1] + m[2]
            row = m[3] * p[2] + m[4] * p[1] + m[5]
            s = np.stack([p[0], row, col])
        s = s.copy()
        for a in range(3):                                                     # step 5
            if flips[a]:
                s[a] = np.float64((d, h, w)[a] - 1) - s[a]
    return s


def round_half_away(v):
    with np.errstate(invalid="ignore"):
        return np.trunc(np.where(v > 0.0, v + 0.5, v - 0.5))


def nearest(src, s):
    """Step 6: the source element at round_half_away(s), 0 outside (a NaN fails every comparison)."""
    src = np.asarray(src)
    r = [round_half_away(s[a]) for a in range(3)]
    with np.errstate(invalid="ignore"):
        inside = np.ones(s.shape[1:], bool)
        for a in range(3):
            inside &= (r[a] >= 0.0) & (r[a] < np.float64(src.shape[a]))
    idx = [np.where(inside, r[a], 0.0).astype(np.int64) for a in range(3)]
    out = src[idx[0], idx[1], idx[2]]
    out[~inside] = 0
    return out


def trilinear(src, s):
    """Step 7 (and 8): float32."""
    src = np.asarray(src, np.float32)
    n = src.shape
    with np.errstate(invalid="ignore"):
        live = np.ones(s.shape[1:], bool)
        for a in range(3):
            live &= (s[a] > -1.0) & (s[a] < np.float64(n[a]))
    s = np.where(live[None], s, 0.0)
    i0 = np.floor(s)
    f = s - i0
    i0 = i0.astype(np.int64)

    def tap(dz, dy, dx):
        idx = [i0[0] + dz, i0[1] + dy, i0[2] + dx]
        ok = np.ones(live.shape, bool)
        for a in range(3):
            ok &= (idx[a] >= 0) & (idx[a] < n[a])
        v = src[tuple(np.where(ok, idx[a], 0) for a in range(3))].astype(np.float64)
        return np.where(ok, v, 0.0)

    with np.errstate(invalid="ignore", over="ignore"):
        fz = []
        for dz in (0, 1):
            e = [lerp(tap(dz, dy, 0), tap(dz, dy, 1), f[2]) for dy in (0, 1)]
            fz.append(lerp(e[0], e[1], f[1]))
        out = lerp(fz[0], fz[1], f[0]).astype(np.float32)
    out[~live] = 0.0
    return out


def warp(image, labels, grid=None, amap=None, flips=(False, False, False), image_order=1, planes=None):
    """The rule -> (image float32 [D,H,W], labels uint8 [D,H,W], raw_box, box, empty).  ``planes``: only these output z (the
    boxes are then those of the planes: not the kernel's)."""
    image, labels = np.asarray(image, np.float32), np.asarray(labels, np.uint8)
    s = coords(image.shape, grid, amap, flips, planes)
    img = trilinear(image, s) if image_order == 1 else nearest(image, s)
    lab = nearest(labels, s)
    raw, empty = sr.extract_box(lab)
    return np.ascontiguousarray(img), np.ascontiguousarray(lab), raw, sr.expand_box(raw, lab.shape), empty

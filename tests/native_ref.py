"""TEST ONLY: numpy float64 restatement of the rules of include/cfun_native.h -- cfun_mold_native (order-1 resample, clip, float32
cast, zero frame, nearest resize, clamp-normalisation as one gather) and cfun_map_resize (order-0 byte resize).  Written from the
header, not from the kernel; tests/test_native_ref.py holds it to scipy's zoom through oracle.cfun_oracle.skimage_resize bit for
bit and to the composition with sample_lits_ref, tests/native_cases.py holds the kernels to it."""
import numpy as np

import sample_lits_ref as lr

frame_index = lr.frame_index          # step 1 is cfun_sample_lits.h's step 1


def axis_taps(r, n, big_r):
    """Step 3 for resampled indices ``r`` (int array) of an axis of source extent n and resampled extent R ->
    (f int64, w0, w1 float64, in0, in1 bool): the two taps f and f + 1, their weights, and whether each lies inside the source."""
    c = (np.asarray(r, np.float64) + 0.5) * (float(n) / float(big_r)) - 0.5
    f = np.floor(c)
    w1 = c - f
    w0 = 1.0 - w1
    f = f.astype(np.int64)
    return f, w0, w1, (f >= 0) & (f < n), (f + 1 >= 0) & (f + 1 < n)


def blend(src, rh, rw, rd, resampled):
    """Steps 3-4: the order-1 value at the resampled indices rh x rw x rd (three int arrays, an outer product) -> float64
    [len(rh), len(rw), len(rd)].  The sum runs a (H), b (W), c (D) with D innermost; a tap outside the source is skipped."""
    src = np.asarray(src)
    taps = [axis_taps(r, n, big_r) for r, n, big_r in zip((rh, rw, rd), src.shape, resampled)]
    t = np.zeros((len(rh), len(rw), len(rd)), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in (0, 1):
            fa, wa, ina = taps[0][0] + a, taps[0][1 + a], taps[0][3 + a]
            for b in (0, 1):
                fb, wb, inb = taps[1][0] + b, taps[1][1 + b], taps[1][3 + b]
                for c in (0, 1):
                    fc, wc, inc = taps[2][0] + c, taps[2][1 + c], taps[2][3 + c]
                    v = src[np.clip(fa, 0, src.shape[0] - 1)[:, None, None], np.clip(fb, 0, src.shape[1] - 1)[None, :, None],
                            np.clip(fc, 0, src.shape[2] - 1)[None, None, :]].astype(np.float64)
                    term = ((v * wa[:, None, None]) * wb[None, :, None]) * wc[None, None, :]
                    inside = ina[:, None, None] & inb[None, :, None] & inc[None, None, :]
                    t = np.where(inside, t + term, t)
    return t


def clip_range(t, clip):
    """Step 5: t < lo ? lo : t, then t > hi ? hi : t -- a NaN stays, a NaN bound does not act."""
    if clip is None:
        return t
    lo, hi = np.float64(clip[0]), np.float64(clip[1])
    with np.errstate(invalid="ignore"):
        t = np.where(t < lo, lo, t)
        return np.where(t > hi, hi, t)


def resample(src, resampled, clip=None):
    """Steps 3-5 over the whole resampled grid: the float64 volume [Hr,Wr,Dr] preprocessing.py's resize produces."""
    return clip_range(blend(src, *[np.arange(n) for n in resampled], resampled), clip)


def offsets(frame, resampled):
    return lr.offsets(frame, resampled)


def mold_native(src, resampled, frame, out_shape, clip="range", norm=True, off=None, planes=None):
    """The whole rule -> float32 [D',H',W'] (or only the output planes ``planes``: a list of z).  ``clip``: (lo, hi), None, or
    "range": the source's own min / max, as the wrapper computes them."""
    src = np.asarray(src)
    if isinstance(clip, str):
        clip = (np.float64(src.min()), np.float64(src.max()))
    off = offsets(frame, resampled) if off is None else off
    zs = np.arange(out_shape[2]) if planes is None else np.asarray(planes)
    r = [frame_index(out_shape[0], frame[0]) - off[0], frame_index(out_shape[1], frame[1]) - off[1],
         frame_index(out_shape[2], frame[2])[zs] - off[2]]
    inside = [(ri >= 0) & (ri < big_r) for ri, big_r in zip(r, resampled)]
    t = clip_range(blend(src, *[np.where(ok, ri, 0) for ri, ok in zip(r, inside)], resampled), clip)
    with np.errstate(invalid="ignore", over="ignore"):
        s = t.astype(np.float32)                                              # step 6: round to nearest even
    if norm:
        s = lr.normalise(s)
    s = np.where(inside[0][:, None, None] & inside[1][None, :, None] & inside[2][None, None, :], s, np.float32(0))
    return np.ascontiguousarray(s.transpose(2, 0, 1)).astype(np.float32)


def map_resize(src, out_shape):
    """cfun_map_resize: src [H,W,D] uint8 -> [H',W',D'] uint8."""
    src = np.asarray(src)
    idx = [frame_index(m, n) for m, n in zip(out_shape, src.shape)]
    return src[idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]]

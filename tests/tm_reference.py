"""An independent statement of temporal accumulation, written from the prose of include/rt1w.h (the comment block "temporal
accumulation") and from nothing else: no library is loaded, nothing of csrc/rt_temporal.h is shared.  Everything is numpy longdouble
(64 bits of mantissa or more: asserted), whole images at a time, one gather per tap.  So the two sides differ in precision and in the
order of evaluation: what they share is the definition.

tests/test_temporal.py holds the CPU twin to this within 1e-12.

The definition is continuous in its inputs but at its tests: which floor a tap position falls to, and the depth and normal
thresholds.  accumulate() therefore returns, next to the images, a mask of the pixels that sit within 1e-9 of one of them, where two
evaluations that round differently may decide differently."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "numpy longdouble is no wider than double here: the reference would prove nothing"

EPS = LD(0.01)   # albedo floor
MAX_HISTORY, DEPTH_TOL, NORMAL_MIN = 32, 0.05, 0.9
NEAR = LD(1e-9)


def _v(cam, k):
    """quantity k of a camera given as 24 doubles: 0 origin, 1 lower_left_corner, 2 horizontal, 3 vertical, 4 u, 5 v, 6 w"""
    return np.asarray(cam, dtype=np.float64).reshape(24)[3 * k:3 * k + 3].astype(LD)


def _dot(a, b):
    return (a * b).sum(axis=-1)


def prepare(frame, aov, keep_albedo):
    """(A, c, unit normal) as the prepare pass of the denoiser forms them"""
    a = aov[..., 0:3].astype(LD)
    A = np.ones_like(a) if keep_albedo else np.where(np.isfinite(a) & (a > EPS), a, EPS)
    with np.errstate(all="ignore"):
        c = frame.astype(LD) / A
        n = aov[..., 3:6].astype(LD)
        m2 = (aov[..., 3:6] ** 2).sum(axis=-1)            # "is 0, underflows or is not finite" speaks of the 64-bit square
        unit = (m2 > 0) & np.isfinite(m2)
        u = np.where(unit[..., None], n / np.sqrt(np.where(unit, _dot(n, n), 1))[..., None], LD(0))
    return A, c, u


def accumulate(cur_frame, cur_aov, cur_cam, prev_hist, prev_len, prev_aov, prev_cam, keep_albedo=False, max_history=0, depth_tol=0.0,
               normal_min=0.0):
    """(hist, len, frame_out, record, near): the three outputs; record[..., 0:2] = fx, fy, [2:6] the taps' weights (0: not valid),
    [6] their sum, [7] 1 / 0 history; near: pixels within 1e-9 of a discontinuity of the definition"""
    cur_frame, cur_aov, prev_hist, prev_len, prev_aov = (np.asarray(x, dtype=np.float64) for x in (cur_frame, cur_aov, prev_hist, prev_len, prev_aov))
    h, w = cur_frame.shape[:2]
    max_history = max_history or MAX_HISTORY
    depth_tol = LD(depth_tol or DEPTH_TOL)
    normal_min = LD(normal_min or NORMAL_MIN)
    A, c, n_cur = prepare(cur_frame, cur_aov, keep_albedo)                                         # 1
    _, _, n_prev = prepare(prev_hist, prev_aov, True)
    z, cov = cur_aov[..., 6].astype(LD), cur_aov[..., 7]
    hit = (cov > 0) & np.isfinite(cur_aov[..., 6])                                                  # 2
    w1, h1 = LD(max(w - 1, 1)), LD(max(h - 1, 1))
    y, x = np.mgrid[0:h, 0:w]
    s = ((x.astype(LD) + LD(0.5)) / w1)[..., None]                                                  # 3
    t = ((y.astype(LD) + LD(0.5)) / h1)[..., None]
    with np.errstate(all="ignore"):
        d = _v(cur_cam, 1) + s * _v(cur_cam, 2) + t * _v(cur_cam, 3) - _v(cur_cam, 0)
        X = _v(cur_cam, 0) + d * (np.where(hit, z, LD(1)) / np.sqrt(_dot(d, d)))[..., None]
        P = X - _v(prev_cam, 0)                                                                     # 4
        pw = _dot(P, _v(prev_cam, 6))
        front = hit & (pw < 0)
        dist = np.sqrt(_dot(P, P))
        D = _v(prev_cam, 0) - _v(prev_cam, 1)
        q = D + P * (_dot(D, _v(prev_cam, 6)) / -np.where(front, pw, LD(-1)))[..., None]
        fx = _dot(q, _v(prev_cam, 2)) / _dot(_v(prev_cam, 2), _v(prev_cam, 2)) * w1 - LD(0.5)
        fy = _dot(q, _v(prev_cam, 3)) / _dot(_v(prev_cam, 3), _v(prev_cam, 3)) * h1 - LD(0.5)
        inside = front & (fx > -1) & (fx < w) & (fy > -1) & (fy < h)
        fx, fy = np.where(inside, fx, LD(0)), np.where(inside, fy, LD(0))
        ix, iy = np.floor(fx), np.floor(fy)                                                         # 5
        ax, ay = fx - ix, fy - iy
        near = inside & ((np.minimum(ax, 1 - ax) < NEAR) | (np.minimum(ay, 1 - ay) < NEAR) | (np.abs(pw) < NEAR * dist))
        num = np.zeros((h, w, 3), dtype=LD)
        numn = np.zeros((h, w), dtype=LD)
        den = np.zeros((h, w), dtype=LD)
        record = np.zeros((h, w, 8), dtype=LD)
        record[..., 0], record[..., 1] = fx, fy
        for k, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            qx, qy = ix.astype(np.int64) + dx, iy.astype(np.int64) + dy
            ok = inside & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            gx, gy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            n_q, z_q, cov_q = prev_len[gy, gx], prev_aov[gy, gx, 6], prev_aov[gy, gx, 7]
            h_q = prev_hist[gy, gx]
            cosv = _dot(n_prev[gy, gx], n_cur)
            dz = np.abs(z_q.astype(LD) - dist)
            valid = ok & (n_q > 0) & np.isfinite(n_q) & (cov_q > 0) & np.isfinite(z_q) & (dz <= depth_tol * dist) & (cosv >= normal_min) & \
                np.isfinite(h_q).all(axis=-1)
            near |= ok & ((np.abs(dz - depth_tol * dist) < NEAR * dist) | (np.abs(cosv - normal_min) < NEAR))
            wt = np.where(valid, (ax if dx else 1 - ax) * (ay if dy else 1 - ay), LD(0))
            record[..., 2 + k] = wt
            num += wt[..., None] * np.where(valid[..., None], h_q, 0.0).astype(LD)                  # 6
            numn += wt * np.where(valid, n_q, 0.0).astype(LD)
            den += wt
        history = den > 0
        safe = np.where(history, den, LD(1))
        N = np.minimum(numn / safe, LD(max_history - 1))                                            # 7
        hist = np.where(history[..., None], (N[..., None] * (num / safe[..., None]) + c) / (N[..., None] + 1), c)
        ln = np.where(history, N + 1, LD(1))
        record[..., 6], record[..., 7] = den, history
        return hist, ln, hist * A, record, near                                                     # 8

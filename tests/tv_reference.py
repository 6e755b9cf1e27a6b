"""An independent statement of the temporal second moments and of the variance made from them, written from the prose of
include/rt1w.h (the comment block "temporal second moments", and the weights of "rt1w_denoise" it points to) and from nothing else: no
library is loaded, nothing of csrc/ is shared.  Steps 1-8 of the moments entry are rt1w_temporal_accumulate's, so they are
tests/tm_reference.py's, whose record of every pixel (tap position, the four weights, their sum) is what the second moment is gathered
with.  Everything is numpy longdouble, whole images at a time.

tests/test_temporal_var.py holds the CPU twins to this within 1e-12.

Both return, next to their images, a mask of the pixels that sit within 1e-9 of one of the definition's decisions, where two evaluations
that round differently may decide differently: the floor of a tap position and the depth and normal thresholds (tm_reference's), the
length threshold, w > 0 at the falloff's cut-off, and the clamp at 0."""
import numpy as np

import tm_reference as TM

LD = TM.LD
NEAR = TM.NEAR
MIN_LEN, RADIUS = 4, 3
NORMAL_POWER, SIGMA_DEPTH, INV_SIGMA_COV2, CUTOFF = 32, LD(1) / LD(10), LD(16), LD(40)


def lum(c):
    c = np.asarray(c).astype(LD)
    return (LD(2126) / LD(10000)) * c[..., 0] + (LD(7152) / LD(10000)) * c[..., 1] + (LD(722) / LD(10000)) * c[..., 2]


def moments(cur_frame, cur_aov, cur_cam, prev_hist, prev_m2, prev_len, prev_aov, prev_cam, keep_albedo=False, max_history=0, **kw):
    """(hist, m2, len, frame_out, record, near)"""
    hist, ln, out, rec, near = TM.accumulate(cur_frame, cur_aov, cur_cam, prev_hist, prev_len, prev_aov, prev_cam, keep_albedo=keep_albedo,
                                             max_history=max_history, **kw)
    prev_m2 = np.asarray(prev_m2, dtype=np.float64)
    h, w = prev_m2.shape
    _, c, _ = TM.prepare(np.asarray(cur_frame, dtype=np.float64), np.asarray(cur_aov, dtype=np.float64), keep_albedo)
    with np.errstate(all="ignore"):
        l = lum(c)
        ix, iy = np.floor(rec[..., 0]).astype(np.int64), np.floor(rec[..., 1]).astype(np.int64)
        num = np.zeros((h, w), dtype=LD)
        for k, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
            wt = rec[..., 2 + k]
            valid = wt > 0                               # an invalid tap's prev_m2 is never read into a product
            q = prev_m2[np.clip(iy + dy, 0, h - 1), np.clip(ix + dx, 0, w - 1)]
            num += np.where(valid, wt * np.where(valid, q, 0.0).astype(LD), LD(0))
        history = rec[..., 7] > 0
        den = np.where(history, rec[..., 6], LD(1))
        N = ln - 1                                       # N' of step 7
        m2 = np.where(history, (N * (num / den) + l * l) / (N + 1), l * l)
    return hist, m2, ln, out, rec, near


def _guides(aov):
    n = aov[..., 3:6].astype(LD)
    with np.errstate(all="ignore"):
        sq = (aov[..., 3:6] ** 2).sum(axis=-1)           # "is 0, underflows or is not finite" speaks of the 64-bit square
        unit = (sq > 0) & np.isfinite(sq)
        u = np.where(unit[..., None], n / np.sqrt(np.where(unit, (n * n).sum(axis=-1), 1))[..., None], LD(0))
    return u, aov[..., 6].astype(LD), aov[..., 7].astype(LD)


def variance(hist, m2, length, aov):
    """(var, minuend over divisor, spatial, near, taps): var [h, w] as longdouble; the scale its tolerance is relative to (m2_p /
    (len_p - 1), resp. M2 / len_p; 0 where there is no estimate); which pixels took the spatial estimate; the pixels near a decision;
    of the spatial pixels' taps inside the image, how many were taken, had weight 0 (normals, the cut-off) or a value that is not finite"""
    hist, m2, length, aov = (np.asarray(x, dtype=np.float64) for x in (hist, m2, length, aov))
    h, w = m2.shape
    with np.errstate(all="ignore"):
        l1 = lum(hist)
        usable = np.isfinite(l1.astype(np.float64)) & np.isfinite(m2) & np.isfinite(length) & (length >= 1)
        n = np.where(usable, length, 1.0).astype(LD)
        # the length is an input, compared as it is: a length exactly ON a threshold is decided alike by every evaluation; one beside it is marked
        near = usable & (((np.abs(n - MIN_LEN) < NEAR) & (n != MIN_LEN)) | ((np.abs(n - 1) < NEAR) & (n != 1)))
        temporal = usable & (length >= MIN_LEN)
        spatial = usable & ~temporal
        m2l = m2.astype(LD)
        dt = m2l - l1 * l1
        vt = np.maximum(dt, 0) / np.where(temporal, n - 1, LD(1))
        scale_t = np.abs(m2l) / np.where(temporal, n - 1, LD(1))
        near |= temporal & (np.abs(dt) < NEAR * np.abs(m2l))
        u, z, cov = _guides(aov)
        zero = ~(u != 0).any(axis=-1)
        y, x = np.mgrid[0:h, 0:w]
        S0, S1, S2 = (np.zeros((h, w), dtype=LD) for _ in range(3))
        fin_q = np.isfinite(l1.astype(np.float64)) & np.isfinite(m2)
        taps = {"taken": 0, "weight 0": 0, "not finite": 0}
        for dy in range(-RADIUS, RADIUS + 1):
            for dx in range(-RADIUS, RADIUS + 1):
                qy, qx = y + dy, x + dx
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                gy, gx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                if dx == 0 and dy == 0:
                    wt = np.ones((h, w), dtype=LD)
                else:
                    uq, zq, cq = u[gy, gx], z[gy, gx], cov[gy, gx]
                    cosv = (u * uq).sum(axis=-1)
                    cosv = np.where(cosv > 0, np.minimum(cosv, 1), LD(0))            # NaN: 0
                    wn = np.where(zero & zero[gy, gx], LD(1), cosv ** NORMAL_POWER)
                    one_inf = (z == np.inf) | (zq == np.inf)
                    xd = np.where(z == zq, LD(0), np.where(one_inf, LD(np.inf), np.abs(z - zq) / (np.maximum(z, zq) * SIGMA_DEPTH)))
                    xs = xd + (cov - cq) * (cov - cq) * INV_SIGMA_COV2
                    k = np.where(xs < CUTOFF, np.where(xs > 0, np.exp(-np.where(xs < CUTOFF, xs, LD(0))), LD(1)), LD(0))   # +inf, NaN: 0
                    wt = wn * k
                    near |= spatial & inside & (wn > 0) & (np.abs(xs - CUTOFF) < NEAR)
                take = inside & (wt > 0) & fin_q[gy, gx]
                taps["taken"] += int((spatial & take).sum())
                taps["weight 0"] += int((spatial & inside & ~(wt > 0)).sum())
                taps["not finite"] += int((spatial & inside & (wt > 0) & ~fin_q[gy, gx]).sum())
                wt = np.where(take, wt, LD(0))
                S0 += wt
                S1 += wt * np.where(take, l1[gy, gx], LD(0))
                S2 += wt * np.where(take, m2l[gy, gx], LD(0))
        S0s = np.where(S0 > 0, S0, LD(1))
        M1, M2 = S1 / S0s, S2 / S0s
        ds = M2 - M1 * M1
        vs = np.maximum(ds, 0) / n
        scale_s = np.abs(M2) / n
        near |= spatial & (np.abs(ds) < NEAR * np.abs(M2))
        var = np.where(temporal, vt, np.where(spatial, vs, LD(0)))
        scale = np.where(temporal, scale_t, np.where(spatial, scale_s, LD(0)))
        bad = ~np.isfinite(var.astype(np.float64)) | (var < 0)
        var, scale = np.where(bad, LD(0), var), np.where(bad, LD(0), scale)
    return var, scale, spatial, near, taps

"""The translucent fluid's rule (include/tpgan_ops.h, "fluid thickness and absorption") stated in numpy: the thickness
pass and the absorption composite.  fp32 operations in the stated order (np.float32 arithmetic, np.sqrt on float32),
vectorised over a disc's box; the contributions are Python-exact int64 sums, so the points may be taken in any order.
The rule has no order dependence and no tolerance: whatever is compared with this statement must be EQUAL to it.
Projection and pixel radius are those of tests/render_rule.py and tests/surface_rule.py, imported, not restated.
"""
import numpy as np

import render_rule as R
import surface_rule as S

F32 = R.F32
ONE, HALF, ZERO = F32(1), F32(0.5), F32(0)
UNIT = F32(16777216.0)                                       # 2^24 units per world unit
MAX_RAD = 1024.0
FLT_MAX = float(np.finfo(F32).max)                           # the delta that makes S.smooth_rule a plain blur


def thickness_units(points, cams, W, H, rad, lengths=None, limit=None):
    """The integer sums (F,H,W) int64 in units of 2^-24, and how many spheres contributed per pixel (F,H,W) int32."""
    points = np.asarray(points, dtype=F32)
    F, N, _ = points.shape
    assert 0 < rad <= MAX_RAD
    rad = F32(rad)
    acc = np.zeros((F, H, W), np.int64)
    count = np.zeros((F, H, W), np.int32)
    for f in range(F):
        c = S._cam(cams, f)
        n = N if lengths is None else min(max(int(lengths[f]), 0), N)
        u, v, zv, t = R.project(points[f, :n], c)
        rp = S.pixel_radius(zv, c, rad)
        with np.errstate(invalid="ignore"):
            keep = ((t >= 0) & (zv <= c[16]) & (rp > 0) & (u >= -rp) & (u < F32(W) + rp) & (v >= -rp) & (v < F32(H) + rp))
        for i in np.nonzero(keep)[0]:
            x0, x1 = max(int(np.floor(u[i] - rp[i])), 0), min(int(np.floor(u[i] + rp[i])), W - 1)
            y0, y1 = max(int(np.floor(v[i] - rp[i])), 0), min(int(np.floor(v[i] + rp[i])), H - 1)
            if x1 < x0 or y1 < y0:
                continue
            dx = ((np.arange(x0, x1 + 1).astype(F32) + HALF) - u[i]) / rp[i]
            dy = ((np.arange(y0, y1 + 1).astype(F32) + HALF) - v[i]) / rp[i]
            s = (dx * dx)[None, :] + (dy * dy)[:, None]
            covered = s < ONE
            with np.errstate(invalid="ignore"):
                half = rad * np.sqrt(np.where(covered, ONE - s, ZERO))
                tp, tb = t[i] - half, t[i] + half
                a = np.where(tp > 0, tp, ZERO).astype(F32)   # the near-plane clamp of the fronts
                b = tb
                if limit is not None:
                    lim = np.asarray(limit, dtype=F32)[f, y0:y1 + 1, x0:x1 + 1]
                    b = np.where(lim < tb, lim, tb)          # false for a NaN: the whole chord
                term = b - a
                adds = covered & (term > 0)
                scaled = np.where(adds, term, ZERO) * UNIT
            assert s.dtype == F32 and half.dtype == F32 and term.dtype == F32 and scaled.dtype == F32
            acc[f, y0:y1 + 1, x0:x1 + 1] += scaled.astype(np.int64)             # truncated: the values are >= 0
            count[f, y0:y1 + 1, x0:x1 + 1] += adds
    return acc, count


def resolve(acc):
    """(float)acc * 2^-24f with the conversion rounded to nearest even: below 2^53 the float64 in between is exact."""
    assert acc.min() >= 0 and acc.max() < 2 ** 53
    return acc.astype(np.float64).astype(F32) * F32(2.0 ** -24)


def thickness_rule(points, cams, W, H, rad, lengths=None, limit=None):
    """(a) -> thickness (F,H,W) f32."""
    return resolve(thickness_units(points, cams, W, H, rad, lengths, limit)[0])


def blur_rule(thickness, k, iters=1):
    """(b): `iters` passes of the surface's smoothing with delta = FLT_MAX."""
    out = np.asarray(thickness, dtype=F32)
    for _ in range(iters):
        out = S.smooth_rule(out, k, FLT_MAX)
    return out


def level_rule(thickness, th_max):
    """tpg_render_points_f32's level rule with s = thickness, lo = 0, inv = 255/th_max."""
    inv = F32(255.0) / F32(th_max)
    with np.errstate(all="ignore"):
        cval = (np.asarray(thickness, dtype=F32) - ZERO) * inv
        level = np.where(cval >= 255, 255, np.where(cval > 0, cval + HALF, ZERO).astype(np.int32))
        return np.where(cval > 0, level, 0)


def absorb_rule(fluid, fdepth, thickness, behind, bdepth, table, th_max):
    """(c) -> (image (F,H,W,3) uint8, depth (F,H,W) f32)."""
    fluid, behind = np.asarray(fluid, np.uint8), np.asarray(behind, np.uint8)
    fdepth, bdepth = np.asarray(fdepth, F32), np.asarray(bdepth, F32)
    table = np.asarray(table, F32)
    assert table.shape == (256, 3)
    T = table[level_rule(thickness, th_max)]
    val = fluid.astype(F32) * (ONE - T) + behind.astype(F32) * T
    assert val.dtype == F32
    byte = np.where(val >= 255, 255, np.where(val > 0, val + HALF, ZERO).astype(np.int32))
    byte = np.where(val > 0, byte, 0).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        back = ~np.isfinite(fdepth) | (bdepth < fdepth)      # on equality the fluid is in front
    return np.where(back[..., None], behind, byte), np.where(back, bdepth, fdepth)

"""The surface renderer's rule (include/tpgan_ops.h, "fluid surface pictures") stated in numpy: sphere fronts, one smoothing
pass, normals and shading.  fp32 operations in the stated order (np.float32 arithmetic, np.sqrt on float32), vectorised
over pixels; the points are taken in index order with an explicit minimum of the 64-bit keys and the window offsets of
the smoothing are looped in the stated order.  The rule has no order dependence and no tolerance, so whatever is compared
with this statement must be EQUAL to it.  Cameras are built as in tests/render_rule.py.
"""
import numpy as np

import render_rule as R

F32 = R.F32
EMPTY = np.uint64(R.EMPTY)
MAX_RADIUS = 64
ONE, HALF, ZERO = F32(1), F32(0.5), F32(0)


def _cam(cams, f):
    cams = np.asarray(cams, dtype=F32).reshape(-1, 18)
    return cams[f if len(cams) > 1 else 0]


def pixel_radius(zv, c, rad):
    """rp of points at view depth zv (n,) under camera c."""
    with np.errstate(all="ignore"):
        rp = (F32(rad) / zv) * c[12] if c[17] != 0 else np.full_like(zv, F32(rad) * c[12])
        return np.fmin(rp, F32(MAX_RADIUS))                      # fminf: a NaN operand gives the other one


def spheres_rule(points, cams, W, H, rad, lengths=None):
    """(a) -> (depth (F,H,W) f32, +inf = background; winner (F,H,W) int32, -1 = background)."""
    points = np.asarray(points, dtype=F32)
    F, N, _ = points.shape
    rad = F32(rad)
    depth = np.empty((F, H, W), F32)
    winner = np.empty((F, H, W), np.int32)
    for f in range(F):
        c = _cam(cams, f)
        n = N if lengths is None else min(max(int(lengths[f]), 0), N)
        u, v, zv, t = R.project(points[f, :n], c)
        rp = pixel_radius(zv, c, rad)
        with np.errstate(invalid="ignore"):
            keep = ((t >= 0) & (zv <= c[16]) & (rp > 0) & (u >= -rp) & (u < F32(W) + rp) & (v >= -rp) & (v < F32(H) + rp))
        keys = np.full((H, W), EMPTY, np.uint64)
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
                tp = t[i] - rad * np.sqrt(ONE - s)
                tp = np.where(tp > 0, tp, ZERO).astype(F32)      # the front is clamped at the near plane
            assert s.dtype == F32 and tp.dtype == F32
            key = (tp.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(i)
            box = keys[y0:y1 + 1, x0:x1 + 1]
            np.minimum(box, np.where(covered, key, EMPTY), out=box)
        hit = keys != EMPTY
        winner[f] = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
        depth[f] = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(F32), F32(np.inf))
    return depth, winner


def binomial_row(k):
    row = [1]
    for _ in range(2 * k):
        row = [a + b for a, b in zip([0] + row, row + [0])]
    return row


def smooth_rule(depth, k, delta):
    """(b) one pass: depth (F,H,W) f32 -> (F,H,W) f32."""
    z = np.asarray(depth, dtype=F32)
    F, H, W = z.shape
    delta, bw = F32(delta), binomial_row(k)
    pad = np.full((F, H + 2 * k, W + 2 * k), F32(np.inf), F32)   # outside the image: never finite, never contributes
    pad[:, k:k + H, k:k + W] = z
    acc, ws = np.zeros_like(z), np.zeros_like(z)
    with np.errstate(all="ignore"):
        for oy in range(-k, k + 1):
            for ox in range(-k, k + 1):
                zj = pad[:, k + oy:k + oy + H, k + ox:k + ox + W]
                ok = np.isfinite(zj) & (np.abs(zj - z) <= delta)
                w = F32(bw[oy + k] * bw[ox + k])
                acc = np.where(ok, acc + w * zj, acc)
                ws = np.where(ok, ws + w, ws)
        out = np.where(np.isfinite(z), acc / ws, z)
    assert out.dtype == F32
    return out


def _points(xs, ys, z, c):
    """View-space points of the pixels (xs, ys) at depth z, as three arrays."""
    Zv = z + c[15]
    a = ((xs.astype(F32) + HALF) - c[13]) / c[12]
    b = ((ys.astype(F32) + HALF) - c[14]) / c[12]
    return (a * Zv, b * Zv, Zv) if c[17] != 0 else (a, b, Zv)


def _difference(P, surface, axis, c):
    """ddx (axis = 1) or ddy (axis = 0) per pixel: three (H,W) arrays."""
    def shifted(a, step, fill):                                  # a[y, x + step] (axis 1) or a[y + step, x] (axis 0)
        out = np.full_like(a, fill)
        src = [slice(None)] * 2
        dst = [slice(None)] * 2
        src[axis] = slice(step, None) if step > 0 else slice(None, step)
        dst[axis] = slice(None, -step) if step > 0 else slice(-step, None)
        out[tuple(dst)] = a[tuple(src)]
        return out
    has1, has0 = shifted(surface, 1, False), shifted(surface, -1, False)
    fw = [shifted(p, 1, F32(np.nan)) - p for p in P]
    bk = [p - shifted(p, -1, F32(np.nan)) for p in P]
    step = (P[2] / c[12]) if c[17] != 0 else np.full_like(P[2], ONE / c[12])
    none = [step if j == 1 - axis else np.zeros_like(step) for j in range(3)]
    back = has0 & (~has1 | (np.abs(bk[2]) < np.abs(fw[2])))      # forward on equality, or if it is the only one
    return [np.where(back, b, np.where(has1, f, d)) for f, b, d in zip(fw, bk, none)]


def normals_rule(depth, cams):
    """The unit normals (F,H,W,3) f32 of (c); rows of background pixels are NaN."""
    z = np.asarray(depth, dtype=F32)
    F, H, W = z.shape
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    out = np.full((F, H, W, 3), np.nan, F32)
    with np.errstate(all="ignore"):
        for f in range(F):
            c = _cam(cams, f)
            surface = np.isfinite(z[f])
            P = _points(xs, ys, z[f], c)
            ddx, ddy = _difference(P, surface, 1, c), _difference(P, surface, 0, c)
            nx = ddy[1] * ddx[2] - ddy[2] * ddx[1]
            ny = ddy[2] * ddx[0] - ddy[0] * ddx[2]
            nz = ddy[0] * ddx[1] - ddy[1] * ddx[0]
            length = np.sqrt((nx * nx + ny * ny) + nz * nz)
            ok = length > 0
            n = [np.where(ok, a / length, F32(d)) for a, d in zip((nx, ny, nz), (0, 0, -1))]
            assert all(a.dtype == F32 for a in n)
            out[f] = np.where(surface[..., None], np.stack(n, -1), F32(np.nan))
    return out


def shade_rule(depth, winner, cams, lut, background, shade, scalar=None, lo=0.0, hi=None):
    """(c) -> image (F,H,W,3) uint8."""
    z = np.asarray(depth, dtype=F32)
    F, H, W = z.shape
    cams = np.asarray(cams, dtype=F32).reshape(-1, 18)
    sh = np.asarray(shade, dtype=F32)
    hi = F32(cams[0, 16]) - F32(cams[0, 15]) if hi is None else hi
    lo32 = F32(lo)
    inv = F32(255.0) / (F32(hi) - lo32)
    normals = normals_rule(z, cams)
    image = np.empty((F, H, W, 3), np.uint8)
    lut = np.asarray(lut)
    with np.errstate(all="ignore"):
        for f in range(F):
            surface = np.isfinite(z[f])
            nx, ny, nz = (normals[f, ..., j] for j in range(3))
            dif = np.fmax((nx * sh[0] + ny * sh[1]) + nz * sh[2], ZERO)
            sp = np.fmax((nx * sh[3] + ny * sh[4]) + nz * sh[5], ZERO)
            for _ in range(int(sh[10])):
                sp = sp * sp
            m = ONE - np.fmax(-nz, ZERO)
            m2 = m * m
            fr = (m2 * m2) * m
            lit, gloss = sh[6] + sh[7] * dif, F32(255.0) * (sh[8] * sp + sh[9] * fr)
            if scalar is not None:
                s = np.asarray(scalar, dtype=F32)[f][np.clip(winner[f], 0, None)]
            else:
                s = z[f]
            cval = (s - lo32) * inv
            level = np.where(cval >= 255, 255, np.where(cval > 0, cval + HALF, ZERO).astype(np.int32))
            level = np.where(cval > 0, level, 0)
            base = lut[np.where(surface, level, 0)].astype(F32)
            val = base * lit[..., None] + gloss[..., None]
            assert val.dtype == F32
            byte = np.where(val >= 255, 255, np.where(val > 0, val + HALF, ZERO).astype(np.int32))
            byte = np.where(val > 0, byte, 0).astype(np.uint8)
            image[f] = np.where(surface[..., None], byte, np.asarray(background, np.uint8))
    return image


def surface_rule(points, cams, W, H, rad, lut, background, shade, lengths=None, scalar=None, lo=0.0, hi=None,
                 half_width=2, iters=3, delta=None):
    """The whole picture as `ops.render_surface` composes it -> (image, smoothed depth, winner)."""
    depth, winner = spheres_rule(points, cams, W, H, rad, lengths)
    delta = F32(2.0) * F32(rad) if delta is None else F32(delta)
    for _ in range(iters):
        depth = smooth_rule(depth, half_width, delta)
    return shade_rule(depth, winner, cams, lut, background, shade, scalar, lo, hi), depth, winner

"""The mesh renderer's rule (include/tpgan_ops.h, "mesh pictures") stated in numpy: projection and cull in fp32, snap to
1/256 pixel, coverage by exact integer edge functions with the left / top ownership of edges, depth in float64 with
every operation rounded on its own, an explicit minimum of the 64-bit keys with the faces taken in index order, and the
deferred shading.  The rule has no order dependence and no tolerance, so whatever is compared with this statement must
be EQUAL to it.  Cameras are built as in tests/render_rule.py.
"""
import numpy as np

import render_rule as R

F32, F64, I64 = R.F32, np.float64, np.int64
EMPTY = np.uint64(R.EMPTY)
GUARD = F32(32768.0)
ONE, HALF, ZERO = F32(1), F32(0.5), F32(0)


def _cam(cams, f):
    cams = np.asarray(cams, dtype=F32).reshape(-1, 18)
    return cams[f if len(cams) > 1 else 0]


def _length(lengths, m, n):
    return n if lengths is None else min(max(int(lengths[m]), 0), n)


def view_points(p, c):
    """p (n,3) fp32 -> xv, yv (n,) fp32: the first two view-space coordinates, as the projection computes them."""
    with np.errstate(all="ignore"):
        q = p - c[0:3]
        return ((q[:, 0] * c[3] + q[:, 1] * c[4]) + q[:, 2] * c[5], (q[:, 0] * c[6] + q[:, 1] * c[7]) + q[:, 2] * c[8])


def edge(ax, ay, bx, by, px, py):
    """E(a, b, p) in exact integers (int64 arrays or Python ints)."""
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def owns(dx, dy):
    return (dy < 0) | ((dy == 0) & (dx > 0))


class Setup:
    """The kept faces of one mesh under one camera: index (K,), X, Y (K,3) int64, d (K,3) fp32 (zv under a pinhole camera,
    else t), area (K,) = |A|, sign (K,), box (K,4) = x0, x1, y0, y1 clipped to the picture (possibly empty)."""

    def __init__(self, vertices, faces, c, W, H, vlen, tlen):
        v = np.asarray(vertices, dtype=F32)[:vlen]
        tri = np.asarray(faces)[:tlen].astype(I64)
        ok = ((tri >= 0) & (tri < vlen)).all(1) if len(tri) else np.zeros(0, bool)
        self.u, self.v, self.zv, self.t = R.project(v, c) if vlen else (np.zeros(0, F32),) * 4
        with np.errstate(invalid="ignore"):
            good = (self.t >= 0) & (self.zv <= c[16]) & (np.abs(self.u) < GUARD) & (np.abs(self.v) < GUARD)
        safe = np.where(ok[:, None], tri, 0)
        ok &= good[safe].all(1) if vlen else False
        with np.errstate(all="ignore"):                              # rows that failed the test are never converted
            X = np.where(good, np.floor(np.where(good, self.u, ZERO) * F32(256) + HALF), 0).astype(I64)
            Y = np.where(good, np.floor(np.where(good, self.v, ZERO) * F32(256) + HALF), 0).astype(I64)
        idx = np.nonzero(ok)[0]
        tri = tri[idx]
        X, Y = X[tri], Y[tri]
        A = edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
        keep = A != 0
        self.index, self.tri, self.X, self.Y, A = idx[keep], tri[keep], X[keep], Y[keep], A[keep]
        self.sign, self.area = np.sign(A), np.abs(A)
        self.d = (self.zv if c[17] != 0 else self.t)[self.tri].astype(F32)
        x0, x1 = np.maximum((self.X.min(1) + 127) >> 8, 0), np.minimum((self.X.max(1) - 128) >> 8, W - 1)
        y0, y1 = np.maximum((self.Y.min(1) + 127) >> 8, 0), np.minimum((self.Y.max(1) - 128) >> 8, H - 1)
        self.box = np.stack([x0, x1, y0, y1], 1).reshape(-1, 4)

    def weights(self, k, xs, ys):
        """w0, w1, w2 (int64 arrays shaped like xs) of kept face k at the centres of the pixels (xs, ys)."""
        px, py = 256 * np.asarray(xs, I64) + 128, 256 * np.asarray(ys, I64) + 128
        X, Y, s = self.X[k], self.Y[k], self.sign[k]
        return [s * edge(X[a], Y[a], X[b], Y[b], px, py) for a, b in ((1, 2), (2, 0), (0, 1))]

    def covered(self, k, w):
        X, Y, s = self.X[k], self.Y[k], self.sign[k]
        inside = np.ones(np.shape(w[0]), bool)
        for wi, (a, b) in zip(w, ((1, 2), (2, 0), (0, 1))):
            inside &= (wi > 0) | ((wi == 0) & bool(owns(s * (X[b] - X[a]), s * (Y[b] - Y[a]))))
        return inside

    def lambdas(self, k, w):
        area = F64(self.area[k])
        return [wi.astype(F64) / area for wi in w]

    def depth(self, k, lam, c):
        d = self.d[k].astype(F64)
        with np.errstate(all="ignore"):
            if c[17] != 0:
                Z = F64(1.0) / ((lam[0] / d[0] + lam[1] / d[1]) + lam[2] / d[2])
                t = (Z - F64(c[15])).astype(F32)
            else:
                t = ((lam[0] * d[0] + lam[1] * d[1]) + lam[2] * d[2]).astype(F32)
            return np.where(t > 0, t, ZERO).astype(F32)


def box_pixels(box):
    """The number of candidate pixels per row of a (K,4) box table (0 for an empty box)."""
    box = np.asarray(box).reshape(-1, 4)
    return np.maximum(box[:, 1] - box[:, 0] + 1, 0) * np.maximum(box[:, 3] - box[:, 2] + 1, 0)


def coverage_count(vertices, faces, cam, W, H):
    """(H,W) int: how many faces cover each pixel, whatever their depth."""
    s = Setup(vertices, faces, np.asarray(cam, F32), W, H, len(vertices), len(faces))
    count = np.zeros((H, W), np.int64)
    for k in range(len(s.index)):
        x0, x1, y0, y1 = s.box[k]
        if x1 < x0 or y1 < y0:
            continue
        ys, xs = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
        count[y0:y1 + 1, x0:x1 + 1] += s.covered(k, s.weights(k, xs, ys))
    return count


def raster_rule(vertices, faces, cams, W, H, F=None, vlengths=None, flengths=None):
    """(a) -> (depth (F,H,W) f32, +inf = background; winner (F,H,W) int32, -1 = background).  vertices (M,V,3), faces
    (M,T,3) with M = 1 or F; F defaults to max(M, the number of cameras)."""
    vertices, faces = np.asarray(vertices, dtype=F32), np.asarray(faces)
    M, V, _ = vertices.shape
    T = faces.shape[1]
    ncam = np.asarray(cams).reshape(-1, 18).shape[0]
    F = max(M, ncam) if F is None else F
    depth = np.empty((F, H, W), F32)
    winner = np.empty((F, H, W), np.int32)
    for f in range(F):
        m, c = (f if M > 1 else 0), _cam(cams, f)
        s = Setup(vertices[m], faces[m], c, W, H, _length(vlengths, m, V), _length(flengths, m, T))
        keys = np.full((H, W), EMPTY, np.uint64)
        for k in range(len(s.index)):
            x0, x1, y0, y1 = s.box[k]
            if x1 < x0 or y1 < y0:
                continue
            ys, xs = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
            w = s.weights(k, xs, ys)
            t = s.depth(k, s.lambdas(k, w), c)
            key = (t.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(s.index[k])
            box = keys[y0:y1 + 1, x0:x1 + 1]
            np.minimum(box, np.where(s.covered(k, w), key, EMPTY), out=box)
        hit = keys != EMPTY
        winner[f] = np.where(hit, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), -1).astype(np.int32)
        depth[f] = np.where(hit, (keys >> np.uint64(32)).astype(np.uint32).view(F32), F32(np.inf))
    return depth, winner


def _mix(lam, a, b, c):
    with np.errstate(all="ignore"):
        return ((lam[0] * a.astype(F64) + lam[1] * b.astype(F64)) + lam[2] * c.astype(F64)).astype(F32)


def shade_rule(depth, winner, vertices, faces, cams, lut, background, shade, vlengths=None, flengths=None, normals=None,
               scalar=None, lo=0.0, hi=None, base=None):
    """(b) -> image (F,H,W,3) uint8."""
    z = np.asarray(depth, dtype=F32)
    F, H, W = z.shape
    vertices, faces = np.asarray(vertices, dtype=F32), np.asarray(faces)
    M, V, _ = vertices.shape
    T = faces.shape[1]
    cams = np.asarray(cams, dtype=F32).reshape(-1, 18)
    sh = np.asarray(shade, dtype=F32)
    hi = F32(cams[0, 16]) - F32(cams[0, 15]) if hi is None else hi
    lo32 = F32(lo)
    inv = F32(255.0) / (F32(hi) - lo32)
    lut = np.asarray(lut)
    image = np.empty((F, H, W, 3), np.uint8)
    image[:] = np.asarray(background, np.uint8)
    for f in range(F):
        m, c = (f if M > 1 else 0), _cam(cams, f)
        vlen, tlen = _length(vlengths, m, V), _length(flengths, m, T)
        s = Setup(vertices[m], faces[m], c, W, H, vlen, tlen)
        slot = np.full(T + 1, -1, np.int64)
        slot[s.index] = np.arange(len(s.index))
        xv, yv = view_points(vertices[m][:vlen], c) if vlen else (np.zeros(0, F32),) * 2
        P = np.stack([xv, yv, s.zv], 1)
        for y in range(H):
            for x in range(W):
                j = int(winner[f, y, x])
                k = slot[j] if 0 <= j < tlen else -1
                if k < 0:
                    continue
                lam = s.lambdas(k, s.weights(k, x, y))
                tri = s.tri[k]
                with np.errstate(all="ignore"):
                    if normals is not None:
                        n0, n1, n2 = (np.asarray(normals, F32)[m][i] for i in tri)
                        nw = _mix(lam, n0, n1, n2)
                        n = [(nw[0] * c[3 + 3 * r] + nw[1] * c[4 + 3 * r]) + nw[2] * c[5 + 3 * r] for r in range(3)]
                    else:
                        a, b = P[tri[1]] - P[tri[0]], P[tri[2]] - P[tri[0]]
                        n = [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
                    length = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
                    n = [a / length for a in n] if length > 0 else [ZERO, ZERO, F32(-1)]
                    if n[2] > 0:
                        n = [-a for a in n]
                    assert all(isinstance(a, F32) for a in n)
                    dif = np.fmax((n[0] * sh[0] + n[1] * sh[1]) + n[2] * sh[2], ZERO)
                    sp = np.fmax((n[0] * sh[3] + n[1] * sh[4]) + n[2] * sh[5], ZERO)
                    for _ in range(int(sh[10])):
                        sp = sp * sp
                    mm = ONE - np.fmax(-n[2], ZERO)
                    m2 = mm * mm
                    fr = (m2 * m2) * mm
                    lit, gloss = sh[6] + sh[7] * dif, F32(255.0) * (sh[8] * sp + sh[9] * fr)
                    if base is not None:
                        col = np.asarray(base, np.uint8)
                    else:
                        if scalar is not None:
                            sc = np.asarray(scalar, F32)[m]
                            value = _mix(lam, sc[tri[0]], sc[tri[1]], sc[tri[2]])
                        else:
                            value = z[f, y, x]
                        cval = (value - lo32) * inv
                        level = 0
                        if cval > 0:
                            level = 255 if cval >= 255 else int(cval + HALF)
                        col = lut[level]
                    val = col.astype(F32) * lit + gloss
                    assert val.dtype == F32
                    image[f, y, x] = [0 if not v > 0 else (255 if v >= 255 else int(v + HALF)) for v in val]
    return image


def mesh_rule(vertices, faces, cams, W, H, lut, background, shade, F=None, vlengths=None, flengths=None, **colour):
    """The whole picture as `ops.render_mesh` composes it -> (image, depth, winner)."""
    depth, winner = raster_rule(vertices, faces, cams, W, H, F, vlengths, flengths)
    return shade_rule(depth, winner, vertices, faces, cams, lut, background, shade, vlengths, flengths, **colour), depth, winner


def compose_rule(layers):
    """[(image (..,H,W,3), depth (..,H,W)), ...] -> (image, depth): per pixel the layer of smallest depth, the earlier one
    on equality."""
    image, depth = (np.array(a) for a in layers[0])
    for img, dep in layers[1:]:
        take = np.asarray(dep) < depth
        image[take] = np.asarray(img)[take]
        depth[take] = np.asarray(dep)[take]
    return image, depth

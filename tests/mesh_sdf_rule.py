"""The signed distance to a triangle mesh (include/tpgan_ops.h, "signed distance to a triangle mesh") stated in numpy:
np.float32 arithmetic in the stated order for the magnitude, np.int64 for the sign, np.sqrt on float32, exact
comparisons.  One pass over the faces in ascending order, every query at once.  The rule has no tolerance, so whatever
is compared with this statement must be EQUAL to it.

The decisions of the rule are small module-level functions (`_owns`, `_ahead`, `_better`, `_skip`), so that a test can
plant a defect in one of them (tests/test_mesh_sdf_cpu.py).  `trace`, a dict, gains per-query arrays that the cases
(tests/mesh_sdf_cases.py) assert on to show that they reach their edge:
    region   (Q,F) int8: 0 vertex a, 1 vertex b, 2 edge ab, 3 vertex c, 4 edge ac, 5 edge bc, 6 face, -1 skipped
    dd       (Q,F) float32: the squared distance to every triangle (inf where skipped)
    on_edge  (Q,F) int8: how many edges of the projection the query lies exactly on (0 outside the closed projection)
    covers, ahead, det0 (Q,F) bool: the projection covers the query; det < 0; det == 0
    counted  (Q,F) bool
    inbox    (Q,) bool, qi (Q,3) int64, unit float"""
import numpy as np

F32 = np.float32
GRID = 65536


def _owns(dy, dz):
    """An edge of the positively oriented projection owns the points on it iff its direction lies in the half-open
    half-plane."""
    return (dy > 0) | ((dy == 0) & (dz > 0))


def _ahead(det):
    """The crossing lies STRICTLY ahead of the query."""
    return det < 0


def _better(dd, best):
    """Ascending faces with a strict comparison: ties go to the lowest face."""
    return dd < best


def _skip(normal_is_zero):
    """Triangles whose fp32 normal is exactly zero are skipped."""
    return normal_is_zero


def grid_of(vertices):
    """(box (6,) float32, inv_unit float): the smallest power of two >= largest extent / 2^16; 1 for no extent."""
    v = np.asarray(vertices, F32).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    ext = float((hi.astype(np.float64) - lo.astype(np.float64)).max())
    unit = 1.0
    if ext > 0.0:
        unit = 2.0 ** np.ceil(np.log2(ext / GRID))
        while unit / 2 >= ext / GRID:                       # log2's rounding must not decide
            unit /= 2
        while unit < ext / GRID:
            unit *= 2
    return np.concatenate([lo, hi]).astype(F32), float(1.0 / unit)


def snap(x, lo, inv_unit):
    """(..., 3) float32 -> int64."""
    with np.errstate(all="ignore"):
        t = np.floor((np.asarray(x, F32) - lo) * F32(inv_unit) + F32(0.5))
    assert t.dtype == F32
    t = np.where(t >= 0, t, F32(0))
    t = np.where(t <= F32(GRID), t, F32(GRID))
    return t.astype(np.int64)


def _dot(s, t):
    return (s[..., 0] * t[..., 0] + s[..., 1] * t[..., 1]) + s[..., 2] * t[..., 2]


def mesh_sdf_rule(query, vertices, faces, box=None, inv_unit=None, trace=None):
    """-> (dist (Q,) float32, face (Q,) int32)."""
    query = np.asarray(query, F32).reshape(-1, 3)
    vertices = np.asarray(vertices, F32).reshape(-1, 3)
    faces = np.clip(np.asarray(faces, np.int64).reshape(-1, 3), 0, len(vertices) - 1)
    if box is None:
        box, inv_unit = grid_of(vertices)
    lo, hi = np.asarray(box[:3], F32), np.asarray(box[3:], F32)
    Q, F = len(query), len(faces)
    with np.errstate(all="ignore"):
        inbox = ((query >= lo) & (query <= hi)).all(1)
    qi = np.where(inbox[:, None], snap(np.where(inbox[:, None], query, lo), lo, inv_unit), 0)
    best = np.full(Q, np.inf, F32)
    best_f = np.full(Q, -1, np.int64)
    count = np.zeros(Q, np.int64)
    if trace is not None:
        trace.update(region=np.full((Q, F), -1, np.int8), dd=np.full((Q, F), np.inf, F32),
                     on_edge=np.zeros((Q, F), np.int8), covers=np.zeros((Q, F), bool), ahead=np.zeros((Q, F), bool),
                     det0=np.zeros((Q, F), bool), counted=np.zeros((Q, F), bool), inbox=inbox, qi=qi,
                     unit=1.0 / inv_unit)
    for f in range(F):
        a, b, c = vertices[faces[f, 0]], vertices[faces[f, 1]], vertices[faces[f, 2]]
        with np.errstate(all="ignore"):
            u, v = b - a, c - a
            normal = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
        if _skip(normal[0] == 0 and normal[1] == 0 and normal[2] == 0):
            continue
        # ---- the sign
        A, B, C = snap(a, lo, inv_unit), snap(b, lo, inv_unit), snap(c, lo, inv_unit)
        area = (B[1] - A[1]) * (C[2] - A[2]) - (B[2] - A[2]) * (C[1] - A[1])
        if area < 0:
            B, C = C, B
        if area != 0:
            n = np.cross(B - A, C - A)
            assert n[0] == abs(area) and n.dtype == np.int64
            covers, closed = np.ones(Q, bool), np.ones(Q, bool)
            zeros = np.zeros(Q, np.int8)
            for U, W in ((B, C), (C, A), (A, B)):
                dy, dz = W[1] - U[1], W[2] - U[2]
                e = dy * (qi[:, 2] - U[2]) - dz * (qi[:, 1] - U[1])
                covers &= (e > 0) | ((e == 0) & _owns(dy, dz))
                zeros += (e == 0)
                closed &= e >= 0
            det = (n[0] * (qi[:, 0] - A[0]) + n[1] * (qi[:, 1] - A[1])) + n[2] * (qi[:, 2] - A[2])
            assert np.abs(det).max(initial=0) < 6 * 2 ** 48
            counted = covers & _ahead(det) & inbox
            count += counted
            if trace is not None:
                trace["on_edge"][:, f] = np.where(inbox & closed, zeros, 0)
                trace["covers"][:, f], trace["ahead"][:, f] = covers & inbox, (det < 0) & inbox
                trace["det0"][:, f], trace["counted"][:, f] = (det == 0) & inbox, counted
        # ---- the magnitude
        with np.errstate(all="ignore"):
            ab, ac = b - a, c - a
            ap, bp, cp = query - a, query - b, query - c
            d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
            vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
            e43, e56 = d4 - d3, d5 - d6
            s = (va + vb) + vc
            t = e43 / (e43 + e56)
            conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0),
                     (d6 >= 0) & (d5 <= d6), (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
            zero, one = np.zeros(Q, F32), np.ones(Q, F32)
            vs = [zero, one, d1 / (d1 - d3), zero, zero, one - t]
            ws = [zero, zero, zero, one, d2 / (d2 - d6), t]
            v_, w_ = np.select(conds, vs, vb / s).astype(F32), np.select(conds, ws, vc / s).astype(F32)
            r = ap - (v_[:, None] * ab + w_[:, None] * ac)
            dd = _dot(r, r)
        assert dd.dtype == F32 and r.dtype == F32
        better = _better(dd, best)                          # a NaN is never better
        best, best_f = np.where(better, dd, best), np.where(better, f, best_f)
        if trace is not None:
            trace["region"][:, f] = np.select(conds, range(6), 6)
            trace["dd"][:, f] = dd
    d = np.sqrt(best)
    assert d.dtype == F32
    return np.where(count % 2 == 1, -d, d).astype(F32), best_f.astype(np.int32)

"""The simulator's mesh obstacles (include/tpgan_ops.h, "mesh obstacles") stated in numpy for ONE scene, on top of the
unchanged functions of tests/pbf_rule.py and tests/pbf_obstacle_rule.py: np.float32 arithmetic in the stated order,
np.sqrt on float32, exact comparisons.  The rule has no tolerance, so whatever is compared with this statement must be
EQUAL to it.

A table row is 24 32-bit words (a float32 array whose words 17..21 hold integers): `make_row` / `decode` pack and unpack
them.  The decisions of the rule are small module-level functions (`_lt`, `_written`, `_final_clamp`, `_order`) so that a
test can plant a defect in one of them (tests/test_sdf_obstacles_cpu.py).  `trace`, a list, gains one dict of
intermediates per row that was not skipped; the cases (tests/pbf_sdf_cases.py) assert on them that they reach their
edge."""
import numpy as np

import pbf_obstacle_rule as O
import pbf_rule as P

F32 = np.float32
FLT_MAX = np.finfo(F32).max
WORDS = 24
KIND = 4
MAX_DIM = 4096


def _lt(phi, a):
    """Moved iff phi < a: strict."""
    return phi < a


def _order(M):
    return range(M)


def _written(moved):
    """Only a particle that moved is written back."""
    return moved


def _final_clamp(p, lo, hi, prm):
    return P.clamp_rule(p, lo, hi, prm)


def make_row(kind, centre, R, origin, step, dims, offset):
    row = np.zeros(WORDS, F32)
    row[0], row[1:4], row[4:13], row[13:16], row[16] = kind, centre, np.asarray(R, np.float64).reshape(-1), origin, step
    words = row.view(np.int32)
    words[17:20] = dims
    words[20:22] = np.array([offset], np.int64).view(np.int32)
    return row


def decode(row):
    """-> (floats (17,), dims (3 ints), offset int)."""
    row = np.ascontiguousarray(row, F32)
    words = row.view(np.int32)
    return row[:17], [int(w) for w in words[17:20]], (int(words[21]) << 32) | (int(words[20]) & 0xFFFFFFFF)


def skipped(row, fields_len):
    fl, dims, offset = decode(row)
    with np.errstate(all="ignore"):
        ok = fl[0] == F32(KIND) and bool((np.abs(fl[1:]) <= FLT_MAX).all()) and fl[16] > 0
    ok = ok and all(2 <= n <= MAX_DIM for n in dims)
    return not (ok and 0 <= offset <= fields_len and dims[0] * dims[1] * dims[2] <= fields_len - offset)


def collide_sdf_rule(p, lo, hi, table, fields, prm, hit=None, trace=None):
    """p (n,3) against the rows of table (M,24) in index order, then the box clamp -> the new p.  hit: an int32 (n,) array
    that gains bit o for the particles row o moved."""
    p = np.asarray(p, F32)
    table = np.asarray(table, F32).reshape(-1, WORDS)
    fields = np.asarray(fields, F32).reshape(-1)
    a = F32(prm.radius)
    px, py, pz = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    for o in _order(len(table)):
        if skipped(table[o], len(fields)):
            continue
        fl, (nx, ny, nz), off = decode(table[o])
        c, R, org, step = fl[1:4], fl[4:13].reshape(3, 3), fl[13:16], fl[16]
        n = (nx, ny, nz)
        with np.errstate(all="ignore"):
            dx, dy, dz = px - c[0], py - c[1], pz - c[2]
            q = [(dx * R[0, k] + dy * R[1, k]) + dz * R[2, k] for k in range(3)]
            g = [(q[k] - org[k]) / step for k in range(3)]
            inl = np.ones(len(px), bool)
            for k in range(3):
                inl &= (g[k] >= 0) & (g[k] <= F32(n[k] - 1))
            gs = [np.where(inl, g[k], F32(0)) for k in range(3)]                 # outside: a valid cell, result unused
            i = [np.minimum(np.floor(gs[k]).astype(np.int64), n[k] - 2) for k in range(3)]
            t = [gs[k] - i[k].astype(F32) for k in range(3)]
            base = off + (i[0] * ny + i[1]) * nz + i[2]
            assert base.min(initial=off) >= off and (base + (ny + 1) * nz + 1).max(initial=0) < off + nx * ny * nz
            f = lambda da, db, dc: fields[base + (da * ny + db) * nz + dc]        # noqa: E731
            x00, x10, x01, x11 = f(1, 0, 0) - f(0, 0, 0), f(1, 1, 0) - f(0, 1, 0), f(1, 0, 1) - f(0, 0, 1), f(1, 1, 1) - f(0, 1, 1)
            c00, c10 = f(0, 0, 0) + t[0] * x00, f(0, 1, 0) + t[0] * x10
            c01, c11 = f(0, 0, 1) + t[0] * x01, f(0, 1, 1) + t[0] * x11
            y0, y1 = c10 - c00, c11 - c01
            c0, c1 = c00 + t[1] * y0, c01 + t[1] * y1
            gz = c1 - c0
            phi = c0 + t[2] * gz
            gx0, gx1 = x00 + t[1] * (x10 - x00), x01 + t[1] * (x11 - x01)
            gx = gx0 + t[2] * (gx1 - gx0)
            gy = y0 + t[2] * (y1 - y0)
            n2 = (gx * gx + gy * gy) + gz * gz
            moved = inl & _lt(phi, a) & (n2 > 0) & (n2 <= FLT_MAX)
            length = np.sqrt(n2)
            s = a - phi
            new = [q[0] + s * (gx / length), q[1] + s * (gy / length), q[2] + s * (gz / length)]
            new = [np.where(moved, new[k], q[k]).astype(F32) for k in range(3)]  # a defect in _written: a round trip
            world = [c[k] + ((R[k, 0] * new[0] + R[k, 1] * new[1]) + R[k, 2] * new[2]) for k in range(3)]
        assert all(w.dtype == F32 for w in world) and phi.dtype == F32 and n2.dtype == F32
        w = _written(moved)
        px, py, pz = np.where(w, world[0], px), np.where(w, world[1], py), np.where(w, world[2], pz)
        if hit is not None:
            hit |= moved.astype(np.int32) << np.int32(o)
        if trace is not None:
            trace.append(dict(o=o, q=q, g=g, inl=inl, cell=i, t=t, phi=np.where(inl, phi, F32(np.nan)), n2=n2, moved=moved,
                              grad=(gx, gy, gz)))
    out = _final_clamp(np.stack([px, py, pz], 1).astype(F32), lo, hi, prm)
    assert out.dtype == F32
    return out


def substep_rule(x, v, lo, hi, dt, prm, table, fields, analytic=None):
    """One substep of one scene -> (x, v): the solids after predict and after every dp; analytic: a (M,16) table of
    tests/pbf_obstacle_rule.py applied first."""
    def solids(p):
        if analytic is not None:
            p = O.collide_rule(p, lo, hi, analytic, prm)
        return collide_sdf_rule(p, lo, hi, table, fields, prm)
    p, _ = P.predict_rule(x, v, lo, hi, dt, prm)
    p = solids(p)
    for _ in range(prm.iters):
        lam, _ = P.lambda_rule(p, prm)
        p, _ = P.dp_rule(p, lam, lo, hi, prm)
        p = solids(p)
    return p, P.finish_rule(p, x, dt, prm)


def frames_rule(x, v, lo, hi, frames, substeps, prm, table, fields):
    """`frames` exported frames after the initial state -> pos, vel (frames, n, 3)."""
    dt = F32(1.0 / (40.0 * substeps))
    pos, vel = [], []
    for _ in range(frames):
        for _ in range(substeps):
            x, v = substep_rule(x, v, lo, hi, dt, prm, table, fields)
        pos.append(x)
        vel.append(v)
    return np.stack(pos), np.stack(vel)

"""The simulator's solid obstacles (include/tpgan_ops.h, "solid obstacles") stated in numpy for ONE scene, on top of the
unchanged functions of tests/pbf_rule.py: np.float32 arithmetic in the stated order, np.sqrt on float32, exact
comparisons.  The rule has no tolerance, so whatever is compared with this statement must be EQUAL to it.

The decisions of the rule are small module-level functions (`_lt`, `_box_axis`, `_cap_first`, `_order`, `_written`,
`_final_clamp`), so that a test can plant a defect in one of them (tests/test_obstacles_cpu.py).  `trace`, a list, gains
one dict of intermediates per obstacle that was not skipped; the cases (tests/pbf_obstacle_cases.py) assert on them that
they reach their edge."""
import numpy as np

import pbf_rule as P

F32 = np.float32
FLT_MAX = np.finfo(F32).max


def _lt(a, b):
    """The inside tests: strict."""
    return a < b


def _box_axis(pen):
    """The axis of the smallest penetration, ties to the lowest."""
    k1 = pen[1] < pen[0]
    k2 = pen[2] < np.where(k1, pen[1], pen[0])
    return np.where(k2, 2, np.where(k1, 1, 0))


def _cap_first(pen_h, pen_r):
    """The cylinder's cap wins a tie against its side."""
    return pen_h <= pen_r


def _order(M):
    return range(M)


def _written(inside):
    """Only a particle that was inside is written back."""
    return inside


def _final_clamp(p, lo, hi, prm):
    return P.clamp_rule(p, lo, hi, prm)


def _side(q, E):
    return np.where(q < 0, -E, E).astype(F32)


def skipped(row):
    """A row whose kind is none of 1, 2, 3 or that holds a value that is not finite."""
    row = np.asarray(row, F32)
    with np.errstate(all="ignore"):
        return not (row[0] in (1.0, 2.0, 3.0) and bool((np.abs(row[1:]) <= FLT_MAX).all()))


def collide_rule(p, lo, hi, table, prm, hit=None, trace=None):
    """p (n,3) against the rows of table (M,16) in index order, then the box clamp -> the new p.  hit: an int32 (n,)
    array that gains bit o for the particles obstacle o moved."""
    p = np.asarray(p, F32)
    table = np.asarray(table, F32).reshape(-1, 16)
    a = F32(prm.radius)
    px, py, pz = p[:, 0].copy(), p[:, 1].copy(), p[:, 2].copy()
    for o in _order(len(table)):
        row = table[o]
        if skipped(row):
            continue
        kind, c, R, s = row[0], row[1:4], row[4:13].reshape(3, 3), row[13:16]
        t = {"o": o, "kind": int(kind)}
        with np.errstate(all="ignore"):
            dx, dy, dz = px - c[0], py - c[1], pz - c[2]
            q = [(dx * R[0, k] + dy * R[1, k]) + dz * R[2, k] for k in range(3)]
            if kind == 1.0:
                E = s[0] + a
                d2 = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]
                inside = _lt(d2, E * E)
                d = np.sqrt(d2)
                zero = d2 == 0
                new = [np.where(zero, E if k == 1 else F32(0), (q[k] / d) * E).astype(F32) for k in range(3)]
                t.update(E=E, d2=d2)
            elif kind == 2.0:
                E = [s[k] + a for k in range(3)]
                mag = [np.abs(q[k]) for k in range(3)]
                inside = _lt(mag[0], E[0]) & _lt(mag[1], E[1]) & _lt(mag[2], E[2])
                pen = [E[k] - mag[k] for k in range(3)]
                axis = _box_axis(pen)
                new = [np.where(axis == k, _side(q[k], E[k]), q[k]).astype(F32) for k in range(3)]
                t.update(E=E, pen=pen, axis=axis)
            else:
                Er, Eh = s[0] + a, s[1] + a
                r2 = q[0] * q[0] + q[2] * q[2]
                inside = _lt(r2, Er * Er) & _lt(np.abs(q[1]), Eh)
                r = np.sqrt(r2)
                pen_r, pen_h = Er - r, Eh - np.abs(q[1])
                cap = _cap_first(pen_h, pen_r)
                zero = r2 == 0
                new = [np.where(cap, q[0], np.where(zero, Er, (q[0] / r) * Er)).astype(F32),
                       np.where(cap, _side(q[1], Eh), q[1]).astype(F32),
                       np.where(cap, q[2], np.where(zero, F32(0), (q[2] / r) * Er)).astype(F32)]
                t.update(Er=Er, Eh=Eh, r2=r2, pen_r=pen_r, pen_h=pen_h, cap=cap)
            new = [np.where(inside, new[k], q[k]).astype(F32) for k in range(3)]      # a defect in _written: a round trip
            world = [c[k] + ((R[k, 0] * new[0] + R[k, 1] * new[1]) + R[k, 2] * new[2]) for k in range(3)]
        assert all(w.dtype == F32 for w in world) and all(x.dtype == F32 for x in q)
        w = _written(inside)
        px, py, pz = np.where(w, world[0], px), np.where(w, world[1], py), np.where(w, world[2], pz)
        if hit is not None:
            hit |= inside.astype(np.int32) << np.int32(o)
        if trace is not None:
            t.update(q=q, inside=inside)
            trace.append(t)
    out = _final_clamp(np.stack([px, py, pz], 1).astype(F32), lo, hi, prm)
    assert out.dtype == F32
    return out


def substep_rule(x, v, lo, hi, dt, prm, table):
    """One substep of one scene with obstacles -> (x, v): collide after predict and after every dp."""
    p, _ = P.predict_rule(x, v, lo, hi, dt, prm)
    p = collide_rule(p, lo, hi, table, prm)
    for _ in range(prm.iters):
        lam, _ = P.lambda_rule(p, prm)
        p, _ = P.dp_rule(p, lam, lo, hi, prm)
        p = collide_rule(p, lo, hi, table, prm)
    return p, P.finish_rule(p, x, dt, prm)


def frames_rule(x, v, lo, hi, frames, substeps, prm, table):
    """`frames` exported frames after the initial state -> pos, vel (frames, n, 3)."""
    dt = F32(1.0 / (40.0 * substeps))
    pos, vel = [], []
    for _ in range(frames):
        for _ in range(substeps):
            x, v = substep_rule(x, v, lo, hi, dt, prm, table)
        pos.append(x)
        vel.append(v)
    return np.stack(pos), np.stack(vel)

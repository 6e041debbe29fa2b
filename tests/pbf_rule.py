"""The fluid simulator's rule (include/tpgan_ops.h, "particle fluid simulator") stated in numpy for ONE scene: fp32
operations in the stated order (np.float32 arithmetic, np.sqrt on float32), brute-force O(N^2) neighbour sets from the
canonical distance, and every neighbourhood sum taken explicitly in 64-bit fixed point.  The rule has no order dependence
and no tolerance, so whatever is compared with this statement must be EQUAL to it.

`prm` is anything with the fp32-rounded constants radius, h, S0, wq, k, eps, dp_scale, cs, gravity, iters
(`ops.PbfParams`)."""
import numpy as np

F32 = np.float32
U32, U30 = F32(2.0 ** 32), F32(2.0 ** 30)
INV_U32, INV_U30 = F32(2.0 ** -32), F32(2.0 ** -30)
TERM_MAX = F32(1024.0)


def lattice_sum():
    """S0 in float64: sum of (1 - |z|^2/4)^3 over the lattice points z with |z| < 2, self included."""
    total = 0.0
    for x in range(-2, 3):
        for y in range(-2, 3):
            for z in range(-2, 3):
                total += max(1.0 - (x * x + y * y + z * z) / 4.0, 0.0) ** 3
    return total


class Pairs:
    """All ordered pairs (i, j) of p (n,3) fp32 as (n,n) arrays: membership d2 < h2, W, and G where d2 > 0."""

    def __init__(self, p, prm):
        p = np.asarray(p, dtype=F32)
        h = F32(prm.h)
        h2 = h * h
        self.d = [p[:, None, a] - p[None, :, a] for a in range(3)]
        d2 = (self.d[0] * self.d[0] + self.d[1] * self.d[1]) + self.d[2] * self.d[2]
        self.near = d2 < h2
        u = (h2 - d2) / h2
        self.W = (u * u) * u
        self.grad = self.near & (d2 != 0)
        with np.errstate(all="ignore"):
            dist = np.sqrt(d2)
            t = (h - dist) / h
            t2 = t * t
            self.G = [t2 * (dx / dist) for dx in self.d]
        assert self.W.dtype == F32 and all(g.dtype == F32 for g in self.G)


def _fix32(term, mask, signed):
    with np.errstate(all="ignore"):
        q = (np.where(mask, term, F32(0)) * U32).astype(np.int64 if signed else np.uint64)
    return q.sum(1, dtype=q.dtype).astype(F32) * INV_U32


def _fix30(term, mask, count=None):
    with np.errstate(all="ignore"):
        t = np.where(mask, term, F32(0))
        if count is not None:                   # what the clamp below met (a dict; the sums do not depend on it)
            count["over"] = count.get("over", 0) + int((np.abs(t) > TERM_MAX).sum())
            count["nan"] = count.get("nan", 0) + int(np.isnan(t).sum())
            count["max"] = max(count.get("max", 0.0), float(np.nanmax(np.abs(t), initial=0.0)))
        t = np.where(t < -TERM_MAX, -TERM_MAX, t)
        t = np.where(t > TERM_MAX, TERM_MAX, t)
        q = (t * U30).astype(np.int64)
    return q.sum(1, dtype=np.int64).astype(F32) * INV_U30


def clamp_rule(p, lo, hi, prm):
    lo_c, hi_c = np.asarray(lo, F32) + F32(prm.radius), np.asarray(hi, F32) - F32(prm.radius)
    p = np.where(p < lo_c, lo_c, p)
    return np.where(p > hi_c, hi_c, p).astype(F32)


def predict_rule(x, v, lo, hi, dt, prm):
    """-> (p, v')."""
    x, v, dt = np.asarray(x, F32), np.asarray(v, F32), F32(dt)
    vv = v + dt * np.asarray(prm.gravity, F32)
    return clamp_rule(x + dt * vv, lo, hi, prm), vv


def lambda_rule(p, prm):
    """-> (lambda (n,), C (n,))."""
    pr = Pairs(p, prm)
    n = _fix32(pr.W, pr.near, False)
    with np.errstate(all="ignore"):
        g2 = (pr.G[0] * pr.G[0] + pr.G[1] * pr.G[1]) + pr.G[2] * pr.G[2]
    sg2 = _fix32(g2, pr.grad, False)
    S = [_fix32(g, pr.grad, True) for g in pr.G]
    C = n / F32(prm.S0) - F32(1)
    C = np.where(C > 0, C, F32(0))
    lam = -(C / ((sg2 + ((S[0] * S[0] + S[1] * S[1]) + S[2] * S[2])) + F32(prm.eps)))
    assert lam.dtype == F32 and C.dtype == F32
    return lam, C


def dp_rule(p, lam, lo, hi, prm, count=None):
    """-> (clamped p + dp, dp).  count: a dict that gains, summed over the three axes, how many terms lay beyond the
    term clamp ("over"), how many were NaN ("nan") and the largest magnitude ("max")."""
    p = np.asarray(p, F32)
    pr = Pairs(p, prm)
    with np.errstate(all="ignore"):             # pairs far beyond the support overflow r2 * r2; the mask drops them
        r = pr.W / F32(prm.wq)
        r2 = r * r
        co = (lam[:, None] + lam[None, :]) + -(F32(prm.k) * (r2 * r2))
        dp = np.stack([F32(prm.dp_scale) * _fix30(co * g, pr.grad, count) for g in pr.G], 1)
    assert dp.dtype == F32
    return clamp_rule(p + dp, lo, hi, prm), dp


def finish_rule(p, x, dt, prm, count=None):
    """-> v after XSPH (x becomes p).  count: as in dp_rule."""
    p, x, dt = np.asarray(p, F32), np.asarray(x, F32), F32(dt)
    pr = Pairs(p, prm)
    v = (p - x) / dt
    out = np.stack([v[:, a] + F32(prm.cs) * _fix30((v[None, :, a] - v[:, None, a]) * pr.W, pr.near, count) for a in range(3)], 1)
    assert out.dtype == F32
    return out


def substep_rule(x, v, lo, hi, dt, prm):
    """One substep of one scene -> (x, v)."""
    p, _ = predict_rule(x, v, lo, hi, dt, prm)
    for _ in range(prm.iters):
        lam, _ = lambda_rule(p, prm)
        p, _ = dp_rule(p, lam, lo, hi, prm)
    return p, finish_rule(p, x, dt, prm)


def frames_rule(x, v, lo, hi, frames, substeps, prm):
    """`frames` exported frames after the initial state -> pos, vel (frames, n, 3)."""
    dt = F32(1.0 / (40.0 * substeps))
    pos, vel = [], []
    for _ in range(frames):
        for _ in range(substeps):
            x, v = substep_rule(x, v, lo, hi, dt, prm)
        pos.append(x)
        vel.append(v)
    return np.stack(pos), np.stack(vel)

"""The rule of vorticity confinement and per-particle viscosity (include/tpgan_ops.h, "vorticity confinement and
per-particle viscosity") stated in numpy for ONE scene, on top of tests/pbf_rule.py: the same brute-force pairs, fp32
operations in the stated order, 64-bit fixed-point sums.  No order dependence and no tolerance: whatever is compared with
this statement must be EQUAL to it.

The steps a planted defect alters are functions of this module (`terms30`, `gradient_pairs`, `curl_terms`, `pair_cs`,
`eta_coefficient`, `curl_velocity`), looked up at call time, so that a test can replace one by monkeypatching.

`prm`: an `ops.PbfParams` (the constants of pbf_rule and vs, delta, vorticity)."""
import numpy as np

import pbf_rule as P
from pbf_rule import F32, Pairs, _fix30  # noqa: F401  (Pairs and F32 are the rule's own; _fix30: see `fix30`)


def lattice_curl():
    """R0 in float64: (1/3) sum of ((2 - |z|)/2)^2 |z| over the lattice points z with 0 < |z| < 2."""
    total, count = 0.0, 0
    for x in range(-2, 3):
        for y in range(-2, 3):
            for z in range(-2, 3):
                r = float(np.sqrt(x * x + y * y + z * z))
                if 0.0 < r < 2.0:
                    total += ((2.0 - r) / 2.0) ** 2 * r
                    count += 1
    assert count == 26
    return total / 3.0


def terms30(term, mask):
    """fix30 of every pair: the clamp into +-1024, then (int64)(t * 2^30); 0 outside the mask -> int64 (n,n)."""
    with np.errstate(all="ignore"):
        t = np.where(mask, term, F32(0))
        t = np.where(t < -P.TERM_MAX, -P.TERM_MAX, t)
        t = np.where(t > P.TERM_MAX, P.TERM_MAX, t)
        return (t * P.U30).astype(np.int64)


def fix30(term, mask):
    """-> (the sums as fp32 (n,), the integer accumulators (n,)).  With the module's own `terms30` the first is
    pbf_rule._fix30(term, mask), which tests/test_vorticity_cpu.py asserts."""
    acc = terms30(term, mask).sum(1, dtype=np.int64)
    return acc.astype(F32) * P.INV_U30, acc


def gradient_pairs(pr):
    return pr.grad


def curl_terms(u, G):
    """u x G per pair: two products and one subtraction per component."""
    with np.errstate(all="ignore"):
        return [u[1] * G[2] - u[2] * G[1], u[2] * G[0] - u[0] * G[2], u[0] * G[1] - u[1] * G[0]]


def pair_cs(tab):
    return F32(0.5) * (tab[:, None] + tab[None, :])


def eta_coefficient(m):
    return m[:, None] - m[None, :]


def curl_velocity(before, after):
    """The velocities the curl is taken on: those BEFORE XSPH."""
    return before


def finish_ex_rule(p, x, dt, prm, cs_tab=None, curl=False, out=None):
    """-> v after XSPH, or (v, omega (n,4)) with curl.  out: a dict that gains the integer accumulators "xsph" (n,3) and,
    with curl, "curl" (n,3), and per kind of sum how many terms lay beyond the clamp ("xsph_over", "curl_over"), how many
    were NaN ("_nan") and the largest magnitude ("_max")."""
    p, x, dt = np.asarray(p, F32), np.asarray(x, F32), F32(dt)
    pr = Pairs(p, prm)
    out = {} if out is None else out
    v = (p - x) / dt
    u = [v[None, :, a] - v[:, None, a] for a in range(3)]
    with np.errstate(all="ignore"):
        if cs_tab is None:
            terms = [u[a] * pr.W for a in range(3)]
        else:
            cij = pair_cs(np.asarray(cs_tab, F32))
            terms = [cij * (u[a] * pr.W) for a in range(3)]
    sums = [fix30(t, pr.near) for t in terms]
    _count(out, "xsph", terms, pr.near)
    out["xsph"] = np.stack([s[1] for s in sums], 1)
    if cs_tab is None:
        after = np.stack([v[:, a] + F32(prm.cs) * sums[a][0] for a in range(3)], 1)
    else:
        after = np.stack([v[:, a] + sums[a][0] for a in range(3)], 1)
    assert after.dtype == F32
    if not curl:
        return after
    w = curl_velocity(v, after)
    uc = [w[None, :, a] - w[:, None, a] for a in range(3)]
    mask = gradient_pairs(pr)
    cterms = curl_terms(uc, pr.G)
    csums = [fix30(t, mask) for t in cterms]
    _count(out, "curl", cterms, mask)
    out["curl"] = np.stack([s[1] for s in csums], 1)
    om = [s[0] for s in csums]
    m = np.sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2])
    omega = np.stack(om + [m], 1)
    assert omega.dtype == F32
    return after, omega


def _count(out, kind, terms, mask):
    with np.errstate(all="ignore"):
        t = np.stack([np.where(mask, t, F32(0)) for t in terms])
        out[kind + "_over"] = int((np.abs(t) > P.TERM_MAX).sum())
        out[kind + "_nan"] = int(np.isnan(t).sum())
        out[kind + "_max"] = float(np.nanmax(np.abs(t), initial=0.0))


def vorticity_rule(p, omega, v, dt, prm, out=None):
    """-> v + (dt * vs) * (N x omega).  out gains "eta" (the integer accumulators (n,3)), "eta_f" (fp32) and "N"."""
    p, omega, v = np.asarray(p, F32), np.asarray(omega, F32), np.asarray(v, F32)
    pr = Pairs(p, prm)
    out = {} if out is None else out
    mask = gradient_pairs(pr)
    dm = eta_coefficient(omega[:, 3])
    with np.errstate(all="ignore"):
        terms = [dm * g for g in pr.G]
    sums = [fix30(t, mask) for t in terms]
    _count(out, "eta", terms, mask)
    eta = [s[0] for s in sums]
    length = np.sqrt((eta[0] * eta[0] + eta[1] * eta[1]) + eta[2] * eta[2])
    den = length + F32(prm.delta)
    n = [e / den for e in eta]
    f = [n[1] * omega[:, 2] - n[2] * omega[:, 1], n[2] * omega[:, 0] - n[0] * omega[:, 2],
         n[0] * omega[:, 1] - n[1] * omega[:, 0]]
    s = F32(dt) * F32(prm.vs)
    res = np.stack([v[:, a] + s * f[a] for a in range(3)], 1)
    out["eta"], out["eta_f"], out["N"] = np.stack([t[1] for t in sums], 1), np.stack(eta, 1), np.stack(n, 1)
    assert res.dtype == F32
    return res


def tail_rule(p, x, dt, prm, cs_tab=None, out=None):
    """The tail of a substep on the final p: finish_ex, then vorticity when prm.vorticity > 0 -> v."""
    if prm.vorticity > 0.0:
        v, omega = finish_ex_rule(p, x, dt, prm, cs_tab, True, out)
        return vorticity_rule(p, omega, v, dt, prm, out)
    return finish_ex_rule(p, x, dt, prm, cs_tab, False, out)


def substep_ex_rule(x, v, lo, hi, dt, prm, cs_tab=None, solids=lambda p: p):
    """One substep of one scene with the options -> (x, v).  solids(p): the obstacles' collide, applied after predict
    and after every dp (tests/pbf_obstacle_rule.py)."""
    p, _ = P.predict_rule(x, v, lo, hi, dt, prm)
    p = solids(p)
    for _ in range(prm.iters):
        lam, _ = P.lambda_rule(p, prm)
        p, _ = P.dp_rule(p, lam, lo, hi, prm)
        p = solids(p)
    return p, tail_rule(p, np.asarray(x, F32), dt, prm, cs_tab)

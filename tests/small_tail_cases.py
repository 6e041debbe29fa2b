"""Inputs of the 16 -> 16 -> 32 small tails (csrc/mlp_small.hip) shared by tests/test_small_tail_cpu.py and
tests/test_small_tail_gpu.py, with the oracle's forward (oracle.ref_ops.small_tail_fwd_ref) computed once per case.

Family A, dyadic: h = k/4 (|k| <= 8), W = k/4 (|k| <= 4), gout = k/4, slopes from {0, 1/4, 1/2, 1}.  Every product and
every partial sum of every quantity is then a small integer multiple of one power of two, i.e. exact in fp32 in ANY
summation order: the kernels must equal the oracle bit for bit.  `dyadic_case` asserts that condition (sum |terms| of
every quantity, counted in units of its own last bit, below 2^24) -- a case that violates it is an error.
Family B, random: h ~ N(0, 1), W ~ 0.3 N(0, 1): per element within the oracle's derived bounds.  `random_case` asserts,
from the oracle alone, that the pairs whose arg-max the bound cannot decide and the elements that carry the z1-sign
allowance are at most 0.1 % each.

At 65 589 points the backward runs 4100 tiles on its 4096 persistent waves: waves 0-3 take a second trip (tiles
4096-4099, points from 65 536 on) and the last tile has 5 live points.  There gout is dense on those waves' tiles
(`dense_points`) and non-zero on 2 % of the other entries: the dyadic weight gradients then stay exact, and one point
of a second-trip tile weighs ~1e-3 of a weight gradient's magnitude sum instead of 1e-5, far above h_w u."""
import functools

import torch

from oracle import ref_ops as R

SMALL_A_SHAPES = [(1, 1), (5, 1), (16, 3), (17, 3), (37, 3), (64, 2), (65, 2), (1000, 9), (5, 255), (65589, 2)]
SMALL_A_CASES = [(P, K, 0.25, 0.25) for P, K in SMALL_A_SHAPES] + \
                [(P, K, s1, s2) for P, K in ((37, 3), (1000, 9)) for s1, s2 in ((0.0, 0.0), (1.0, 1.0), (0.5, 0.0))]
SMALL_B_SHAPES = [(37, 3), (1000, 9), (4099, 20), (5, 255), (65589, 2)]
SMALL_B_SLOPES = [(0.2, 0.2), (0.01, 0.2)]
BIG = 65589
EXACT_UNITS = 2.0 ** 24


def second_trip_points(P):
    """Points of the tiles a wave of the backward reaches on a later trip of its grid-stride loop."""
    tiles, blocks = R.small_tail_geometry(P)
    first = 4 * blocks * 16
    return torch.arange(P) >= first


def dense_points(P):
    """Where gout stays dense: everywhere while every wave has one tile; else the tiles of the waves that take a second
    trip (both trips) and the ragged last tile."""
    tiles, blocks = R.small_tail_geometry(P)
    if tiles <= 4 * blocks:
        return torch.ones(P, dtype=torch.bool)
    n = torch.arange(P)
    waves2 = tiles - 4 * blocks                         # waves 0 .. waves2 - 1 take the second trip
    return (n < waves2 * 16) | (n >= 4 * blocks * 16) | (n // 16 == tiles - 1)


def _thin(gout, g):
    keep = dense_points(gout.shape[0])[:, None] | (torch.rand(gout.shape, generator=g) < 0.02)
    return gout * keep


def _slope_unit(s):
    """log2 of the unit of a slope from {0, 1/4, 1/2, 1}."""
    return {0.0: 0, 1.0: 0, 0.5: -1, 0.25: -2}[float(s)]


def dyadic_exactness(c, b):
    """sum |terms| of every quantity of the case c (backward b on the oracle's own arg / out) in units of the
    quantity's last bit: {name: peak}.  Raises unless every count is an integer below 2^24 (float64 holds integers
    below 2^53 exactly, so this is integer arithmetic)."""
    f, u1, u2 = c["fwd"], _slope_unit(c["s1"]), _slope_unit(c["s2"])
    W1, W2 = c["W1"].double().abs(), c["W2"].double().abs()
    sums = {                                                       # name: (sum |terms|, log2 unit)
        "z1": (f["M1"], -4), "a1": (f["a1"].abs(), -4 + u1), "z2": (f["M2"], -6 + u1), "out": (f["out"].abs(), -6 + u1 + u2),
        "gz2": (b["gz2"].abs(), -2 + u2), "ga1": (b["gz2"].abs() @ W2, -4 + u2), "gz1": (b["gz1"].abs(), -4 + u1 + u2),
        "gh": (b["gz1"].abs() @ W1, -6 + u1 + u2), "dW1": (b["S1"], -6 + u1 + u2), "dW2": (b["S2"], -6 + u1 + u2)}
    peaks = {}
    for name, (m, unit) in sums.items():
        q = m * 2.0 ** -unit
        if not bool((q == q.round()).all()) or not float(q.max() if q.numel() else 0.0) < EXACT_UNITS:
            raise AssertionError(f"dyadic case {c['P'], c['K'], c['s1'], c['s2']}: {name} is not exact in fp32 "
                                 f"({float(q.max()):.3g} units)")
        peaks[name] = float(q.max()) if q.numel() else 0.0
    return peaks


def dyadic_events(c):
    """(pairs tied between different edges, z1 == 0, best == 0) counted on the oracle's forward."""
    f, P, K = c["fwd"], c["P"], c["K"]
    z2v = f["z2"].view(P, K, 32)
    ties = int(((z2v == f["best"][:, None]).sum(1) > 1).sum())
    return ties, int((f["z1"] == 0).sum()), int((f["best"] == 0).sum())


@functools.lru_cache(maxsize=None)
def dyadic_case(P, K, s1, s2):
    """-> dict(h (P*K, 16), W1, W2, gout (P, 32) fp32 on the CPU; fwd, bwd: the oracle on them (bwd with its own arg
    and out); exact: dyadic_exactness; P, K, s1, s2).  The values are exact in bf16 too: both row types share it."""
    g = torch.Generator().manual_seed(1000 * P + K + int(8 * s1) + int(64 * s2))
    big = P == BIG

    def q(lim, *shape):
        return torch.randint(-lim, lim + 1, shape, generator=g).float() / 4
    h = q(8, P * K, 16)
    W1, W2 = q(4, 16, 16), q(4, 32, 16)
    gout = _thin(q(1, P, 32), g) if big else q(8, P, 32)
    if (P, K) == (1000, 9):
        # one all-zero edge row (z2 == 0 in every channel) in each of 64 points: where the point's other edges are all
        # negative in a channel, best == 0 exactly, out == 0, and the backward takes slope s2 on a real arg-max
        n = torch.arange(500, 564)
        h.view(P, K, 16)[n, n % K] = 0.0
    if K == 255:
        # small rows everywhere; two large rows A, B: A at edge 254 and B at edge 0 of every point (the maxima of the
        # channels go to one or the other), and A at edge 3 as well from point 2 on (exact ties between edges 3 and 254)
        h = q(1, P * K, 16).view(P, K, 16)
        A = torch.where(torch.arange(16) % 3 == 0, -2.0, 2.0)
        h[:, 254], h[:, 0] = A, -A
        h[2:, 3] = A
        h = h.reshape(P * K, 16).contiguous()
    c = dict(h=h, W1=W1, W2=W2, gout=gout, P=P, K=K, s1=s1, s2=s2)
    c["fwd"] = R.small_tail_fwd_ref(h, W1, W2, s1, s2, K)
    c["bwd"] = R.small_tail_bwd_ref(h, c["fwd"]["out"], gout, c["fwd"]["arg"], W1, W2, s1, s2, K)
    c["exact"] = dyadic_exactness(c, c["bwd"])
    if (P, K) == (1000, 9):
        ties, z0, b0 = dyadic_events(c)
        assert ties > 0 and z0 > 0 and b0 > 0, (ties, z0, b0)
    if K == 255:
        arg = c["fwd"]["arg"].long()
        z2v = c["fwd"]["z2"].view(P, K, 32)
        assert int((arg[:2] == 254).sum()) > 0 and int((arg[:2] == 0).sum()) > 0, "planted maxima at edges 254 and 0"
        tied = (arg[2:] == 3) & (z2v[2:, 3] == z2v[2:, 254])
        assert int(tied.sum()) > 0 and int((arg[2:] == 254).sum()) == 0, "planted ties between edges 3 and 254"
    return c


@functools.lru_cache(maxsize=None)
def random_case(P, K, s1, s2, bf16):
    """-> dict(h, W1, W2, gout: fp32 CPU tensors holding values of the row type; fwd: the oracle's forward; gap2: is the
    exact gap of a pair's maximum to its runner-up above 2 max_j E2 (the arg-max is then decided); undecided, allowance:
    the shares the conditions bound; P, K, s1, s2, bf16)."""
    g = torch.Generator().manual_seed(7 * P + K + int(1000 * s1) + (1 if bf16 else 0))

    def rows(t):
        return t.bfloat16().float() if bf16 else t
    h = rows(torch.randn(P * K, 16, generator=g))
    W1, W2 = 0.3 * torch.randn(16, 16, generator=g), 0.3 * torch.randn(32, 16, generator=g)
    gout = rows(_thin(torch.randn(P, 32, generator=g), g))
    f = R.small_tail_fwd_ref(h, W1, W2, s1, s2, K)
    top = f["z2"].view(P, K, 32).topk(2, 1)[0]
    gap2 = (top[:, 0] - top[:, 1]) > 2 * f["E2max"]
    undecided = 1.0 - float(gap2.double().mean())
    allowance = float((f["z1"].abs() <= f["E1"]).double().mean())
    assert undecided <= 1e-3 and allowance <= 1e-3, (P, K, undecided, allowance)
    return dict(h=h, W1=W1, W2=W2, gout=gout, fwd=f, gap2=gap2, undecided=undecided, allowance=allowance, P=P, K=K,
                s1=s1, s2=s2, bf16=bf16)


def stored(v, bf16):
    """A value as the kernels store a row element: fp32, then bf16 for bf16 rows (float64 carrier)."""
    return R.rbf16(R.r32(v)) if bf16 else R.r32(v)

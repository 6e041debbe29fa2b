"""The kNN rule in numpy (tests/knn_rule.py) against the C oracle, the oracle's order on NaN distances, and the stress
clouds of tests/knn_cases.py: the `shifted` levels must reach the regime where the filters' error bound E_q
(csrc/knn_gram.hpp) selects among near neighbours, or the GPU tests built on them check nothing new."""
import os
import sys

import numpy as np
import pytest

from oracle import ref_ops as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_rule  # noqa: E402
from knn_cases import KINDS, STRESS, feature_cloud, origin_tile, stress_cloud  # noqa: E402

FINITE = [(kind, level) for kind in STRESS if kind != "nonfinite" for level in STRESS[kind]]


def _equal(got, want):
    (gd, gi), (wd, wi) = got, want
    return np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


@pytest.mark.parametrize("D", [32, 64])
def test_rule_equals_oracle_on_finite_clouds(D):
    """Bit for bit, indices and distances (the distances' BITS: -0.0 or a flushed denormal would differ)."""
    rng = np.random.default_rng(D)
    pairs = [(feature_cloud(rng, 1, 64, D, kind), feature_cloud(rng, 1, 200, D, kind), kind) for kind in KINDS]
    pairs += [(stress_cloud(rng, 1, 64, D, kind, level), stress_cloud(rng, 1, 200, D, kind, level), f"{kind} {level}")
              for kind, level in FINITE]
    for p1, p2, name in pairs:
        for K in (2, 12, 24):
            assert _equal(knn_rule.knn(p1, p2, K), R.knn(p1, p2, K)), (name, K)


def test_rule_equals_oracle_on_ragged_clouds():
    rng = np.random.default_rng(3)
    p1, p2 = feature_cloud(rng, 4, 64, 32, "normal"), stress_cloud(rng, 4, 200, 32, "shifted", 20)
    l1, l2 = np.array([64, 10, 0, 33]), np.array([200, 5, 70, 0])           # fewer than K points; no query; an empty cloud
    got, want = knn_rule.knn(p1, p2, 12, l1, l2), R.knn(p1, p2, 12, l1, l2)
    assert _equal(got, want)
    assert not got[1][2].any() and not got[0][3].any() and not got[1][1, :, 5:].any()      # the (0, 0) padding


@pytest.mark.parametrize("name", STRESS["nonfinite"])
@pytest.mark.parametrize("D,K", [(32, 20), (64, 12), (32, 4)])
def test_rule_and_oracle_on_nonfinite_clouds(D, K, name):
    """The rule's order with NaN distances, and the oracle's: a NaN distance ranks after every other one."""
    rng = np.random.default_rng(D + K)
    p1, p2 = stress_cloud(rng, 2, 64, D, "nonfinite", name, K=K), stress_cloud(rng, 2, 200, D, "nonfinite", name, K=K)
    d, i = knn_rule.knn(p1, p2, K)
    keys = knn_rule.order_keys(d).astype(np.int64)
    assert (np.diff(keys, axis=-1) >= 0).all()                              # ascending, NaN last
    assert ((i >= 0) & (i < 200)).all() and (np.diff(np.sort(i, axis=-1), axis=-1) > 0).all()      # distinct valid rows
    bad_query = ~np.isfinite(p1).all(axis=-1)           # every distance of such a query is NaN (Inf: +Inf, one NaN)
    assert bad_query.any()
    assert (i[bad_query] == np.arange(K)).all()
    assert (np.isinf(d[bad_query]) if name == "inf_coord" else np.isnan(d[bad_query])).all()
    full = knn_rule.sqdist(p1[0], p2[0])
    assert np.array_equal(np.isnan(d[0]).sum(axis=-1), np.maximum(K - (~np.isnan(full)).sum(axis=-1), 0))
    rd, ri = R.knn(p1, p2, K)
    assert np.array_equal(ri, i) and np.array_equal(rd, d, equal_nan=True)


# ---- knn_small's selection on the CPU: exact distances, the kernel's threshold rule and the bound's constants ----------
KM_C1 = 2.0 ** -13                                      # csrc/knn_gram.hpp:104  KM_C1 = 2^-13
KM_CAP = 64                                             # csrc/knn_gram.hpp:25   candidate slots per query


def km_c2(D):
    return (8 * D + 64) * 2.0 ** -24                    # csrc/knn_gram.hpp:105  KM_C2<D> = (8 D + 64) 2^-24


def small_filter_list_lengths(p, K):
    """Entries of knn_small_kernel's candidate list per query of the self-search of one cloud p (P2, D), had its
    approximate distances no error: T = the K-th smallest of the 64 lane minima (lane = point index mod 64),
    the list = every point within T + 2 E_q x 1.001 (csrc/knn_small.hpp, "select")."""
    P2, D = p.shape
    y = p.astype(np.float64) - p[:origin_tile(D)].astype(np.float32).mean(axis=0, dtype=np.float64)
    norm = np.sqrt((y * y).sum(axis=1))
    d = ((y * y).sum(axis=1)[:, None] + (y * y).sum(axis=1)[None, :] - 2.0 * y @ y.T)
    lanes = np.full((P2, 64), np.inf)
    for lane in range(64):
        lanes[:, lane] = d[:, lane::64].min(axis=1)
    T = np.sort(lanes, axis=1)[:, K - 1]
    eq = KM_C1 * norm * norm.max() + km_c2(D) * (norm + norm.max()) ** 2
    return (d <= (T + 2.0 * eq * 1.001)[:, None]).sum(axis=1)


@pytest.mark.parametrize("D,K", [(32, 20), (64, 12)])
def test_shifted_levels_reach_the_regime_where_the_bound_selects(D, K):
    """Across the `shifted` sweep the candidate lists go from settled to overflowing: a level where no query overflows
    its 64 slots, one where 2 % .. 90 % do (T + 2 E_q selects among near neighbours), and nearly all at the top."""
    share = {}
    for level in STRESS["shifted"]:
        p = stress_cloud(np.random.default_rng(1000 * D + K), 1, 512, D, "shifted", level)[0]
        n = small_filter_list_lengths(p, K)
        share[level] = float((n > KM_CAP).mean())
        print(f"shifted level {level} D={D} K={K}: median list {int(np.median(n))}, {share[level] * 100:.1f} % of the queries overflow")
    assert min(share.values()) == 0.0
    assert any(0.02 < s < 0.90 for s in share.values())
    assert share[STRESS["shifted"][-1]] > 0.70

"""The feature-space clouds the matrix-core kNN filters are compared on (tests/test_ops_gpu.py,
tests/test_knn_small_gpu.py), and the stress clouds that load their error bound (tests/test_knn_bound_gpu.py)."""
import numpy as np

KINDS = ["normal", "manifold", "lattice", "offset", "dups", "same"]


def feature_cloud(rng, B, P, D, kind):
    """Feature-space clouds as the generator's bottleneck layers produce them: a few-dimensional manifold
    embedded in D dims plus noise ("manifold"), iid normal ("normal"), the same far from the origin
    ("offset": the Gram form cancels badly unless centred), a cloud of 1/4 exact duplicates ("dups"), and
    every point identical ("same": everything ties)."""
    assert kind in KINDS, kind
    if kind == "manifold":
        z = rng.standard_normal((B, P, 3)).astype(np.float32)
        x = np.tanh(z @ rng.standard_normal((3, D)).astype(np.float32)) + 0.05 * rng.standard_normal((B, P, D)).astype(np.float32)
    else:
        x = rng.standard_normal((B, P, D)).astype(np.float32)
    if kind == "lattice":
        # small integers: distances are small integers too -- exact ties everywhere, in particular AT the K-th
        # distance, where only the (dist, idx) order decides and the filter's margin test must give up
        x = rng.integers(0, 3, (B, P, D)).astype(np.float32) * 0.5
    if kind == "offset":
        x += 300.0
    if kind == "dups":
        x[:, P // 4 * 3:] = x[:, :P - P // 4 * 3]
    if kind == "same":
        x[:] = 0.37
    return np.ascontiguousarray(x.astype(np.float32))


# ---- clouds on which the filters' error bound E_q (csrc/knn_gram.hpp, km_bound) decides the answer or is void
# (tests/test_knn_rule_cpu.py, tests/test_knn_bound_gpu.py).  kind -> the levels the tests sweep.
STRESS = {
    "shifted": [0, 8, 16, 20, 24, 28, 100, 300],
    "first_far": [20, 300],
    "mixed": [0.5, 1, 1.5, 2],
    "jitter": [1e-4, 1e-3, 1e-2, 1e-1],
    "scaled": [-70, -64, -60, -40, 40, 60],
    "outlier": [1e12, 1e15, 3e18, 2e19],
    "nonfinite": ["nan_coord", "nan_first_tile", "inf_coord", "nan_row", "few_finite"],
}


def origin_tile(D):
    """km_tile_rows (csrc/knn_mfma.hpp): the kernels' origin is the mean of a cloud's first 128 (D = 32) / 64 (D = 64) points."""
    return 128 if D == 32 else 64


def stress_cloud(rng, B, P, D, kind, level, tile=None, K=None):
    """The kernels centre a cloud on the mean of its first `tile` points in index order; E_q and the real error of the
    approximate distance grow with |y|^2 = |x - origin|^2, the neighbour spacing does not.
      shifted    standard normal, rows tile.. moved by `level` in every dimension: they keep |y| ~ level sqrt(D);
      first_far  the mirror image: rows ..tile moved, the origin sits in them and every OTHER row is far;
      mixed      row norms spread over 2 `level` decades: for a query of small norm E_q is all max|y_p|^2;
      jitter     the "lattice" cloud plus `level` x standard normal: near-ties inside 2 E_q that are not ties;
      scaled     the "normal" cloud times 2^level (exact): products and distances under- / overflow;
      outlier    "normal", one row past the first tile times `level`: |y|^2 passes the padding norm 1e30, then fp32;
      nonfinite  "normal" with ONE kind of non-finite value, by name: NaN in one coordinate of a point past the first
                 tile ("nan_coord") or inside it ("nan_first_tile": the origin is NaN), +Inf in one coordinate
                 ("inf_coord"), a whole NaN row ("nan_row"), all but K - 3 rows NaN ("few_finite")."""
    assert kind in STRESS, kind
    tile = origin_tile(D) if tile is None else tile
    far = min(tile + 5, P - 1)                          # a row past the first tile (the last row of a shorter cloud)
    x = rng.standard_normal((B, P, D)).astype(np.float32)
    if kind == "shifted":
        x[:, tile:] += np.float32(level)
    elif kind == "first_far":
        x[:, :tile] += np.float32(level)
    elif kind == "mixed":
        x *= (10.0 ** rng.uniform(-level, level, (B, P, 1))).astype(np.float32)
    elif kind == "jitter":
        x = rng.integers(0, 3, (B, P, D)).astype(np.float32) * 0.5 + np.float32(level) * x
    elif kind == "scaled":
        x = np.ldexp(x, int(level))
    elif kind == "outlier":
        with np.errstate(over="ignore"):
            x[:, far] *= np.float32(level)
    else:
        assert level in STRESS["nonfinite"], level
        if level == "nan_coord":
            x[:, far, D // 3] = np.nan
        elif level == "nan_first_tile":
            x[:, min(3, P - 1), D - 1] = np.nan
        elif level == "inf_coord":
            x[:, far, D // 3] = np.inf
        elif level == "nan_row":
            x[:, far] = np.nan
        else:
            finite = np.linspace(0, P - 1, max(K - 3, 0)).astype(np.int64)        # spread over the cloud, first row included
            keep = x[:, finite].copy()
            x[:] = np.nan
            x[:, finite] = keep
    return np.ascontiguousarray(x.astype(np.float32))

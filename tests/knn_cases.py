"""The feature-space clouds the matrix-core kNN filters are compared on (tests/test_ops_gpu.py,
tests/test_knn_small_gpu.py)."""
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

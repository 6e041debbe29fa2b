"""Feature-space kNN on small clouds (csrc/knn_small.hpp: one sweep of the split-operand Gram filter, every approximate
distance in LDS, exact re-rank): `hip.knn` takes that path by itself for D = 32 / 64, 2 <= K <= 24 and
SMALL_MIN <= P2 <= 1024, and its output must equal the oracle's bit for bit, indices and distances, (0, 0) padding
included -- whichever queries the filter handed to the exhaustive kernel.  Every case also calls the path directly
(`hip.knn_small`, filter + redo): the kernel itself takes any P2 <= 1024, below the dispatch's bound too."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_ops as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from knn_cases import feature_cloud as _cloud  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL_MIN = 512       # TPG_KNN_SMALL_MIN_POINTS (csrc/knn.hip): the smallest P2 the dispatch gives to the new kernel


@pytest.fixture(scope="module")
def hip():
    import tpgan_amd.ops as ops
    assert torch.cuda.is_available()
    return ops.backend_for(torch.zeros(1, device="cuda"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_as_oracle(hip, p1, p2, K, l1=None, l2=None):
    d, i = hip.knn(dev(p1), dev(p2), None if l1 is None else dev(l1), None if l2 is None else dev(l2), K, None)
    rd, ri = R.knn(p1, p2, K, l1, l2)
    assert np.array_equal(i.cpu().numpy(), ri)
    assert np.array_equal(d.cpu().numpy(), rd)
    d, i = hip.knn_small(dev(p1), dev(p2), None if l1 is None else dev(l1), None if l2 is None else dev(l2), K)
    assert np.array_equal(i.cpu().numpy(), ri)
    assert np.array_equal(d.cpu().numpy(), rd)
    return rd, ri


@pytest.mark.parametrize("B,P1,P2,D,K", [
    (2, 512, 512, 64, 12), (2, 512, 512, 32, 20), (1, 512, 512, 64, 2), (1, 512, 512, 32, 24),
    (1, 70, 333, 64, 8), (1, 300, 130, 32, 20),                       # P1 != P2, ragged sub-tiles and query tiles
    (1, 100, SMALL_MIN, 64, 12), (1, 100, SMALL_MIN - 1, 64, 12),     # the dispatch's lower edge and one below
    (1, 40, 1024, 32, 16), (1, 40, 1024, 64, 12),                     # the largest distance matrix
    (1, 33, 64, 32, 24), (1, 33, 65, 64, 24)])                        # the kernel's own minimum of valid points
def test_knn_small_bit_exact(hip, B, P1, P2, D, K):
    rng = np.random.default_rng(B * 1000 + P1 + P2 + D + K)
    p2 = rng.standard_normal((B, P2, D)).astype(np.float32)
    p1 = p2.copy() if P1 == P2 else rng.standard_normal((B, P1, D)).astype(np.float32)
    p2[0, 5] = p2[0, 7]; p2[-1, 10:14] = p2[-1, 3]                    # exact duplicates
    _same_as_oracle(hip, p1, p2, K)


@pytest.mark.parametrize("D,K,kind", [
    (64, 12, "normal"), (32, 20, "manifold"), (64, 8, "manifold"), (32, 20, "offset"), (64, 12, "dups"),
    (32, 20, "lattice"), (64, 4, "lattice"), (32, 9, "same")])
def test_knn_small_cloud_kinds(hip, D, K, kind):
    """Bit-exact on every cloud kind; what the filter alone settled (redo=False) is already the answer, and on benign
    clouds it settles nearly everything (a wrong operand layout would send every query to the exhaustive kernel and still
    pass the first assertions); a cloud of identical points overflows every candidate list and is redone entirely."""
    rng = np.random.default_rng(D + K + len(kind))
    p = _cloud(rng, 2, 512, D, kind)
    rd, ri = _same_as_oracle(hip, p, p, K)
    rawd, raw = hip.knn_small(dev(p), dev(p), None, None, K, redo=False)
    raw, rawd = raw.cpu().numpy(), rawd.cpu().numpy()
    open_ = raw[:, :, 0] == -2
    print(f"small-cloud kNN {kind} D={D} K={K}: {open_.mean() * 100:.2f} % of the queries left to the exhaustive kernel")
    assert np.array_equal(raw[~open_], ri[~open_]) and np.array_equal(rawd[~open_], rd[~open_])
    if kind in ("manifold", "normal"):
        assert open_.mean() < 0.02
    if kind == "same":
        assert open_.all()


def test_knn_small_lengths(hip):
    """A full cloud, a cloud below the kernel's minimum of valid points, an empty one and a ragged one in one batch."""
    rng = np.random.default_rng(5)
    p1, p2 = _cloud(rng, 4, 200, 32, "normal"), _cloud(rng, 4, 512, 32, "normal")
    l1, l2 = np.array([200, 77, 200, 0]), np.array([512, 40, 0, 301])
    _same_as_oracle(hip, p1, p2, 16, l1, l2)
    _, raw = hip.knn_small(dev(p1), dev(p2), dev(l1), dev(l2), 16, redo=False)
    raw = raw.cpu().numpy()
    assert (raw[0, :, 0] != -2).mean() > 0.98                         # the full cloud is the filter's
    assert (raw[1, :, 0] == -2).all() and (raw[2, :, 0] == -2).all()  # 40 / 0 valid points: the exhaustive kernel's


def test_knn_small_repeatable(hip):
    rng = np.random.default_rng(6)
    p = dev(_cloud(rng, 3, 512, 64, "manifold"))
    d0, i0 = hip.knn(p, p, None, None, 12, None)
    d1, i1 = hip.knn(p, p, None, None, 12, None)
    assert torch.equal(d0, d1) and torch.equal(i0, i1)

"""The matrix-core kNN filters (csrc/knn_small.hpp, csrc/knn_mfma.hpp) where their error bound E_q (csrc/knn_gram.hpp,
km_bound) decides the answer or is void: clouds whose first tile -- the kernels' origin -- sits away from the rest, norms
over decades, near-ties, under- and overflowing products, non-finite rows (tests/knn_cases.py, stress_cloud).  The
claim under test: whatever the data, the output is the exhaustive kernels' output bit for bit, and a query the filter
does NOT hand to the exhaustive kernel (redo=False, first index slot != -2) already carries that answer.  With a bound
of zero the existing tests pass on their benign clouds; these do not (profiles/knn_bound.txt)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ref_ops as R

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_rule  # noqa: E402
from knn_cases import STRESS, origin_tile, stress_cloud  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL, MFMA = "knn_small", "knn_mfma"
DK = [(32, 20), (64, 12)]                               # knn_small<32> / <64>, knn_mfma<32, 14> / <64, 10>
P1 = 256


@pytest.fixture(scope="module")
def hip():
    import tpgan_amd.ops as ops
    assert torch.cuda.is_available()
    return ops.backend_for(torch.zeros(1, device="cuda"))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(d, i, rd, ri, nonfinite):
    """Indices equal; distances equal in their bits (a flushed denormal or a -0.0 differs), NaN == NaN on non-finite input
    (the host's and the device's NaN need not carry the same bits)."""
    d, i = np.asarray(d), np.asarray(i)
    if not np.array_equal(i, ri):
        return False
    return np.array_equal(d, rd, equal_nan=True) if nonfinite else np.array_equal(bits(d), bits(rd))


def check(hip, filt, p1, p2, K, l1=None, l2=None, nonfinite=False, tag=""):
    """hip.knn (the dispatch), the filter + redo and what the filter alone settled, against the reference (the oracle;
    the numpy rule on non-finite input).  Returns (per-query mask of the queries left to the exhaustive kernel, reference)."""
    rd, ri = knn_rule.knn(p1, p2, K, l1, l2) if nonfinite else R.knn(p1, p2, K, l1, l2)
    a1, a2, b1, b2 = dev(p1), dev(p2), dev(l1), dev(l2)
    d, i = hip.knn(a1, a2, b1, b2, K, None)
    assert _same(d.cpu().numpy(), i.cpu().numpy(), rd, ri, nonfinite), f"dispatch {tag}"
    call = hip.knn_small if filt == SMALL else hip.knn_mfma
    d, i = call(a1, a2, b1, b2, K, redo=True)
    assert _same(d.cpu().numpy(), i.cpu().numpy(), rd, ri, nonfinite), f"{filt} + redo {tag}"
    rawd, raw = call(a1, a2, b1, b2, K, redo=False)
    rawd, raw = rawd.cpu().numpy(), raw.cpu().numpy()
    open_ = raw[:, :, 0] == -2
    print(f"{filt} {tag} D={p2.shape[2]} K={K} P2={p2.shape[1]}: {open_.mean() * 100:.2f} % of the queries left to the exhaustive kernel")
    same_d = bits(rawd) == bits(rd)
    if nonfinite:
        same_d |= np.isnan(rawd) & np.isnan(rd)
    wrong = ~open_ & ~((raw == ri).all(axis=-1) & same_d.all(axis=-1))
    assert not wrong.any(), f"{filt} {tag}: {wrong.sum()} queries settled by the filter with a wrong list, the first {np.argwhere(wrong)[0]}"
    return open_, (rd, ri)


def clouds(seed, D, P2, kind, level, K, B=1):
    rng = np.random.default_rng(seed)
    return stress_cloud(rng, B, P1, D, kind, level, K=K), stress_cloud(rng, B, P2, D, kind, level, K=K)


def _shifted_shares(open_, D, level, filt):
    """What follows from the construction: at level 0 the cloud is `normal` (the existing tests' < 2 %); at level 300
    E_q exceeds the spacing of every neighbourhood, and every query whose neighbourhood holds more than the 64 list slots
    must be left to the exhaustive kernel."""
    if level == 0:
        assert open_.mean() < 0.02
    if level == 300:
        far = np.arange(open_.shape[1]) >= origin_tile(D)
        assert open_[:, far].all()
        if not (filt == SMALL and D == 64):
            # knn_small<64>: the 64 points of the first tile are the whole neighbourhood of a query of the first tile,
            # T + 2 E_q lists exactly those 64 = KM_CAP, no overflow: settled, and rightly (checked above)
            assert open_.all()


# ---- the first tile away from the rest ---------------------------------------------------------------------------------
@pytest.mark.parametrize("level", STRESS["shifted"])
@pytest.mark.parametrize("D,K", DK)
@pytest.mark.parametrize("filt,P2", [(SMALL, 512), (MFMA, 2048)])
def test_shifted_sweep(hip, filt, P2, D, K, level):
    p1, p2 = clouds(11 * D + K + P2, D, P2, "shifted", level, K)
    open_, _ = check(hip, filt, p1, p2, K, tag=f"shifted {level}")
    _shifted_shares(open_, D, level, filt)


@pytest.mark.parametrize("D,K", [(32, 20), (64, 12), (32, 24), (64, 2)])
@pytest.mark.parametrize("P2", [512, 1024])
def test_small_filter_shapes(hip, P2, D, K):
    p1, p2 = clouds(P2 + D + K, D, P2, "shifted", 20, K)
    check(hip, SMALL, p1, p2, K, tag="shifted 20")


def test_small_filter_ragged_last_subtile(hip):
    """130 points: below the dispatch's bound (hip.knn takes the exhaustive kernel), two rows in the last sub-tile."""
    p1, p2 = clouds(130, 32, 130, "shifted", 20, 20)
    check(hip, SMALL, p1, p2, 20, tag="shifted 20")


@pytest.mark.parametrize("D,K", [(32, 12), (32, 20), (32, 24), (64, 12), (64, 20), (64, 24)])       # M = 10, 14, 16
@pytest.mark.parametrize("P2", [1024, 2048, 4096])      # the filter's floor (direct call only), the dispatch's, 32-row entries
def test_matrix_core_filter_shapes(hip, P2, D, K):
    p1, p2 = clouds(P2 + D + K, D, P2, "shifted", 20, K)
    check(hip, MFMA, p1, p2, K, tag="shifted 20")


@pytest.mark.parametrize("D,K", DK)
@pytest.mark.parametrize("filt,P2", [(SMALL, 512), (MFMA, 2048)])
def test_short_first_tile(hip, filt, P2, D, K):
    """Clouds of tile - 1 and tile + 1 valid points beside a full one: the origin is the mean of a short first tile."""
    tile = origin_tile(D)
    p1, p2 = clouds(3 + D + P2, D, P2, "shifted", 20, K, B=3)
    check(hip, filt, p1, p2, K, l2=np.array([P2, tile - 1, tile + 1]), tag="shifted 20, lengths")


# ---- norms over decades, near-ties, the mirror image, one huge row ------------------------------------------------------
@pytest.mark.parametrize("kind,level", [(k, v) for k in ("first_far", "mixed", "jitter", "outlier") for v in STRESS[k]])
@pytest.mark.parametrize("D,K", DK)
@pytest.mark.parametrize("filt,P2", [(SMALL, 512), (MFMA, 2048)])
def test_stress_kinds(hip, filt, P2, D, K, kind, level):
    p1, p2 = clouds(7 * D + K + P2 + len(kind), D, P2, kind, level, K)
    open_, _ = check(hip, filt, p1, p2, K, tag=f"{kind} {level}")
    if (kind, level) == ("outlier", 2e19):              # |y|^2 of the row is +Inf in fp32: no threshold is finite
        assert open_.all()


# ---- under- and overflow ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", STRESS["scaled"])
@pytest.mark.parametrize("D,K", DK)
@pytest.mark.parametrize("filt,P2", [(SMALL, 512), (MFMA, 2048)])
def test_scaled(hip, filt, P2, D, K, level):
    """2^level times the `normal` cloud.  At +-40 nothing under- or overflows: the lists are the unscaled cloud's and the
    distances the unscaled ones times 2^(2 level) exactly, oracle or not.  At -60, -64 and -70 the split products, then
    the distances themselves, are fp32 denormals: the canonical sum keeps them (fp32, no fast-math), so must the output,
    and the bound, which is relative, does not hold: below max|y_p| = 2^-40 (KM_TINY) the filters settle nothing.
    (Before that rule knn_small returned wrong lists at 2^-70, D = 32 and 64: profiles/knn_bound.txt.)"""
    seed = 5 * D + K + P2
    p1, p2 = clouds(seed, D, P2, "scaled", level, K)
    open_, (rd, ri) = check(hip, filt, p1, p2, K, tag=f"scaled 2^{level}")
    if level <= -60:
        assert open_.all()
    if abs(level) == 40:
        u1, u2 = clouds(seed, D, P2, "scaled", 0, K)
        d, i = hip.knn(dev(u1), dev(u2), None, None, K, None)
        assert np.array_equal(i.cpu().numpy(), ri)
        assert np.array_equal(bits(np.ldexp(d.cpu().numpy(), 2 * level)), bits(rd))


# ---- non-finite rows -------------------------------------------------------------------------------------------------
def _guarded(hip, p1, p2, K):
    """tpg_knn_f32 on PRE-FILLED outputs (hip.knn allocates with torch.empty): every slot is written, with a row of p2."""
    guard_d, guard_i = 12345.0, -77
    B, n1, D = p1.shape
    a1, a2 = dev(p1), dev(p2)
    dist = torch.full((B, n1, K), guard_d, dtype=torch.float32, device="cuda")
    idx = torch.full((B, n1, K), guard_i, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc = hip.lib.tpg_knn_f32(a1.data_ptr(), a2.data_ptr(), None, None, B, n1, p2.shape[1], D, K, -1.0, dist.data_ptr(),
                             idx.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return dist.cpu().numpy(), idx.cpu().numpy(), guard_d


@pytest.mark.parametrize("name", STRESS["nonfinite"])
@pytest.mark.parametrize("D,K", DK)
@pytest.mark.parametrize("filt,P2", [(SMALL, 512), (MFMA, 2048)])
def test_nonfinite(hip, filt, P2, D, K, name):
    """NaN / Inf rows as a diverged training step sends them: the filters fall back, the exhaustive kernels order NaN
    distances last by index (the contract of csrc/knn_select.hpp's keys), no output slot is left unwritten and every
    index is a row of the cloud -- the next gather reads it."""
    p1, p2 = clouds(13 * D + K + P2, D, P2, "nonfinite", name, K)
    _, (rd, ri) = check(hip, filt, p1, p2, K, nonfinite=True, tag=name)
    d, i, guard = _guarded(hip, p1, p2, K)
    assert ((i >= 0) & (i < P2)).all() and not (d == guard).any()
    assert _same(d, i, rd, ri, True)


@pytest.mark.parametrize("name", STRESS["nonfinite"])
@pytest.mark.parametrize("D,K", DK)
def test_nonfinite_exhaustive_kernels(hip, D, K, name):
    """511 points: below the small filter's dispatch bound, hip.knn is the tiled exhaustive kernel."""
    p1, p2 = clouds(17 * D + K, D, 511, "nonfinite", name, K)
    rd, ri = knn_rule.knn(p1, p2, K)
    d, i, guard = _guarded(hip, p1, p2, K)
    assert ((i >= 0) & (i < 511)).all() and not (d == guard).any()
    assert _same(d, i, rd, ri, True)

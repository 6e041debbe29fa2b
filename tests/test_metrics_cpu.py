"""Earth mover's distance, Gaussian MMD and the evaluation metrics, the part that needs no GPU.

1. The numpy STATEMENTS of the two new ops, which the GPU tests (tests/test_metrics_gpu.py) compare the kernels with:
   `auction_statement` -- the forward auction of include/tpgan_ops.h, which csrc/emd.hip reproduces bit for bit -- and
   `gaussian_statement` -- the row sums of csrc/gauss_sum.hip in float64 with their error bound.
2. The auction statement against scipy's optimum: a permutation, within n * eps of the optimal sum, and
   epsilon-complementary slackness straight from the returned prices.
3. The interface: symbols, status codes of malformed calls without a device, CPU tensors refused, argument errors.
4. tests/golden/metrics.npz (the reference's own `position_loss` functions, captured with recording stand-ins for the
   `emd` and `geomloss` packages, tests/golden/capture_metrics_goldens.py) against `tpgan_amd.metrics` on a CPU test
   backend built from the statements: the clouds and scalars handed to the two ops, `cd`, `mmd`.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "metrics.npz")
F = np.float32
DEFAULTS = dict(eps=1e-4, iters=1_000_000, phases=3, scaling=4.0)
# Bound on expf's error in ulps.  ROCm's table of the device functions' maximum ulp errors (the HIP math documentation)
# is not installed with ROCm, so the fall-back value of 2 ulp is used.
EXPF_ULPS = 2.0


# ------------------------------------------------------------------------------------------ 1. the statements
def sq3(a, b):
    """(N,3), (M,3) fp32 -> (N,M) fp32: the canonical squared distance (t = a - b; d = t0*t0; d += t1*t1; d += t2*t2,
    every operation rounded to fp32)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    t = a[:, None, :] - b[None, :, :]
    d = t[..., 0] * t[..., 0]
    d = d + t[..., 1] * t[..., 1]
    d = d + t[..., 2] * t[..., 2]
    return d


def phase_eps(eps, scaling, k):
    e = F(eps)
    for _ in range(k):
        e = F(e * F(scaling))
    return e


def auction_statement(x1, x2, eps=DEFAULTS["eps"], iters=DEFAULTS["iters"], phases=DEFAULTS["phases"],
                      scaling=DEFAULTS["scaling"]):
    """One cloud: x1 (n,3) persons, x2 (n,3) objects -> dist (n,) f32, assignment (n,) i32, price (n,) f32, rounds.
    RuntimeError when `iters` rounds leave persons unassigned."""
    x1, x2 = np.asarray(x1, F), np.asarray(x2, F)
    n = x1.shape[0]
    c = sq3(x1, x2)
    p = np.zeros(n, F)
    assign = np.full(n, -1, np.int64)
    owner = np.full(n, -1, np.int64)
    rounds = 0
    if n == 1:
        assign[0] = 0
    else:
        for k in range(phases, -1, -1):
            e = phase_eps(eps, scaling, k)
            assign[:] = -1
            owner[:] = -1
            while True:
                U = np.flatnonzero(assign < 0)
                if U.size == 0:
                    break
                if rounds >= iters:
                    raise RuntimeError(f"auction: {U.size} unassigned persons after {rounds} rounds")
                v = (-c[U]) - p[None, :]                                   # fp32
                rows = np.arange(U.size)
                j1 = v.argmax(axis=1)                                      # first maximum: the lowest j
                v1 = v[rows, j1]
                v[rows, j1] = -np.inf
                v2 = v.max(axis=1)
                pj = p[j1]
                pn = pj + ((v1 - v2) + e)                                  # fp32, in this order
                stuck = ~(pn > pj)
                pn[stuck] = np.nextafter(pj[stuck], F(np.inf))
                key = (pn.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (0xFFFFFFFF - U).astype(np.uint64)
                best = np.zeros(n, np.uint64)
                np.maximum.at(best, j1, key)                               # highest bid, then lowest person
                js = np.flatnonzero(best)
                wi = (0xFFFFFFFF - (best[js] & np.uint64(0xFFFFFFFF)).astype(np.int64))
                prev = owner[js]
                assign[prev[prev >= 0]] = -1
                owner[js] = wi
                assign[wi] = js
                p[js] = (best[js] >> np.uint64(32)).astype(np.uint32).view(F)
                rounds += 1
    dist = c[np.arange(n), assign]
    return dist, assign.astype(np.int32), p, rounds


def gaussian_scale(sigma):
    s = float(F(sigma))
    return F(1.0 / (2.0 * s * s))


def gaussian_statement(a, b, sigma):
    """(N,3), (M,3) -> (sums (N,) float64, bound (N,) float64).  The canonical fp32 c, the fp32 product with
    fp32(1 / (2 sigma^2)), then a float64 exp.  The bound on the kernel's distance from it, per term: the product's
    rounding seen through the exponential (|arg| * 2^-24 * w), expf's error (EXPF_ULPS * 2^-24 * w) and the truncation
    to a multiple of 2^-32."""
    arg = (sq3(a, b) * gaussian_scale(sigma)).astype(np.float64)
    w = np.exp(-arg)
    bound = ((np.abs(arg) * 2.0 ** -24 + EXPF_ULPS * 2.0 ** -24) * w + 2.0 ** -32).sum(axis=1)
    return w.sum(axis=1), bound


def mmd_statement(x, y, blur):
    """-> (mmd, bound) of one pair of clouds from the row-sum statement."""
    (xx, bxx), (yy, byy), (xy, bxy) = gaussian_statement(x, x, blur), gaussian_statement(y, y, blur), \
        gaussian_statement(x, y, blur)
    N, M = x.shape[0], y.shape[0]
    mmd = 0.5 * xx.sum() / (N * N) + 0.5 * yy.sum() / (M * M) - xy.sum() / (N * M)
    return mmd, 0.5 * bxx.sum() / (N * N) + 0.5 * byy.sum() / (M * M) + bxy.sum() / (N * M)


# ------------------------------------------------------------------------------------------------ the cases
CASE_SIZES = (2, 64, 100, 257, 1024)
CASE_KINDS = ("uniform", "blobs", "duplicates", "permutation")


def auction_case(kind, n, seed=0):
    rng = np.random.RandomState(1000 * CASE_KINDS.index(kind) + n + seed)
    if kind == "uniform":
        return rng.rand(n, 3).astype(F), rng.rand(n, 3).astype(F)
    if kind == "blobs":
        centres = rng.rand(4, 3)
        def blob():
            return (centres[rng.randint(0, 4, n)] + 0.05 * rng.randn(n, 3)).astype(F)
        return blob(), blob()
    if kind == "duplicates":
        x1, x2 = rng.rand(n, 3).astype(F), rng.rand(n, 3).astype(F)
        x1[n // 2:n // 2 + n // 2] = x1[:n // 2]              # half of xyz1 repeated
        x2[::4] = x2[0]                                        # every fourth point of xyz2 equal
        return x1, x2
    x1 = rng.rand(n, 3).astype(F)
    return x1, x1[rng.permutation(n)].copy()


_STATEMENT_CACHE = {}


def auction_result(kind, n):
    """The statement's result on a case at the default schedule, computed once per process."""
    if (kind, n) not in _STATEMENT_CACHE:
        x1, x2 = auction_case(kind, n)
        _STATEMENT_CACHE[(kind, n)] = (x1, x2) + auction_statement(x1, x2)
    return _STATEMENT_CACHE[(kind, n)]


# ------------------------------------------------------------------------- 2. the statement against scipy
@pytest.mark.parametrize("n", CASE_SIZES)
@pytest.mark.parametrize("kind", CASE_KINDS)
def test_auction_statement_is_a_near_optimal_permutation(kind, n):
    from scipy.optimize import linear_sum_assignment
    x1, x2, dist, assign, price, rounds = auction_result(kind, n)
    eps = float(F(DEFAULTS["eps"]))
    assert sorted(assign.tolist()) == list(range(n))
    c = sq3(x1, x2).astype(np.float64)
    assert np.array_equal(dist, sq3(x1, x2)[np.arange(n), assign])
    r, col = linear_sum_assignment(c)
    optimum, total = c[r, col].sum(), c[np.arange(n), assign].sum()
    print(f"{kind} n={n}: rounds {rounds}, sum {total:.6f}, optimum {optimum:.6f}, gap {total - optimum:.3e}")
    assert total <= optimum + n * eps
    # epsilon-complementary slackness: nobody could gain more than eps (and the fp32 rounding of the two value
    # computations: four ulps of the larger c + p) by moving to another object at the final prices
    cp = c + price.astype(np.float64)[None, :]
    mine = cp[np.arange(n), assign]
    tol = 4.0 * np.spacing(mine.astype(F)).astype(np.float64)          # mine >= the row's minimum: the larger c + p
    assert np.all(mine <= cp.min(axis=1) + eps + tol)
    assert np.all(price >= 0)


def test_auction_statement_trivial_and_capped_cases():
    x = np.array([[0.5, 0.25, 0.125]], F)
    dist, assign, price, rounds = auction_statement(x, x + F(1))
    assert assign.tolist() == [0] and rounds == 0 and price.tolist() == [0.0] and dist[0] == F(3.0)
    x1, x2 = auction_case("uniform", 64)
    with pytest.raises(RuntimeError, match="unassigned"):
        auction_statement(x1, x2, iters=1)
    # the schedule changes the prices and the rounds, never the guarantee
    one = auction_statement(x1, x2, phases=0)
    assert sorted(one[1].tolist()) == list(range(64))


def test_gaussian_statement_bound_and_limits():
    a = np.zeros((1, 3), F)
    sums, bound = gaussian_statement(a, np.zeros((5, 3), F), 0.1)
    assert sums[0] == 5.0 and 0 < bound[0] < 1e-5
    far = np.full((1, 3), 999.0, F)
    assert gaussian_statement(a, far, 0.01)[0][0] == 0.0
    assert gaussian_scale(0.01) == F(5000.0)


# ------------------------------------------------------------------------------------------- 3. interface
NEW_SYMBOLS = ("tpg_emd_workspace_bytes", "tpg_emd_init_f32", "tpg_emd_rounds_f32", "tpg_emd_finish_f32",
               "tpg_gaussian_row_sums_f32")


def test_symbols_are_declared_exported_and_bound(hip_lib):
    from tpgan_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tpgan_ops.h")).read(), flags=re.S)
    bound = set(_lib.SIGNATURES) | set(_lib.SIZE_GETTERS)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(hip_lib, name) and name in bound, name


def test_entries_reject_malformed_calls_before_any_launch(hip_lib):
    raw = (C.c_char * 4096)()
    at = (C.addressof(raw) + 255) & ~255
    p, odd = C.c_void_p(at), C.c_void_p(at + 4)
    lib = hip_lib
    assert lib.tpg_emd_workspace_bytes(0, 8) == 0 and lib.tpg_emd_workspace_bytes(8, 0) == 0
    assert lib.tpg_emd_workspace_bytes(2, 100) >= 2 * 32 + 2 * 100 * (16 + 8 + 4 * 4)
    # init: negative sizes, n != m, phases, null pointers, workspace alignment, empty work
    assert lib.tpg_emd_init_f32(p, -1, 8, 8, 3, p, p, None) == -1
    assert lib.tpg_emd_init_f32(p, 1, -8, -8, 3, p, p, None) == -1
    assert lib.tpg_emd_init_f32(p, 1, 8, 9, 3, p, p, None) == -1
    assert lib.tpg_emd_init_f32(p, 1, 8, 8, -1, p, p, None) == -1
    assert lib.tpg_emd_init_f32(None, 1, 8, 8, 3, p, p, None) == -1
    assert lib.tpg_emd_init_f32(p, 1, 8, 8, 3, None, p, None) == -1
    assert lib.tpg_emd_init_f32(p, 1, 8, 8, 3, p, None, None) == -1
    assert lib.tpg_emd_init_f32(p, 1, 8, 8, 3, p, odd, None) == -1
    assert lib.tpg_emd_init_f32(p, 70000, 8, 8, 3, p, p, None) == -3
    assert lib.tpg_emd_init_f32(p, 0, 8, 8, 3, p, p, None) == 0 and lib.tpg_emd_init_f32(p, 1, 0, 0, 3, p, p, None) == 0

    def rounds(x=p, B=1, n=8, eps=1e-4, scaling=4.0, phases=3, iters=100, wide=4, narrow=16, at=4, a=p, ws=p):
        return lib.tpg_emd_rounds_f32(x, B, n, eps, scaling, phases, iters, wide, narrow, at, a, ws, None)
    assert rounds(eps=0.0) == -1 and rounds(eps=-1.0) == -1 and rounds(eps=float("nan")) == -1
    assert rounds(scaling=0.5) == -1 and rounds(phases=-1) == -1 and rounds(phases=65) == -1 and rounds(iters=0) == -1
    assert rounds(wide=-1) == -1 and rounds(narrow=-1) == -1 and rounds(at=-1) == -1 and rounds(wide=5000) == -1
    assert rounds(wide=0) == -1                  # some clouds could never advance
    assert rounds(narrow=0) == -1
    assert rounds(B=-1) == -1 and rounds(n=-1) == -1
    assert rounds(x=None) == -1 and rounds(a=None) == -1 and rounds(ws=None) == -1 and rounds(ws=odd) == -1
    assert rounds(B=0) == 0 and rounds(n=0, at=0) == 0
    assert lib.tpg_emd_finish_f32(p, 1, 8, p, p, None, p, p, None) == -1
    assert lib.tpg_emd_finish_f32(p, 1, 8, p, p, p, p, None, None) == -1
    assert lib.tpg_emd_finish_f32(p, 1, 8, p, None, p, p, p, None) == -1
    assert lib.tpg_emd_finish_f32(p, -1, 8, p, p, p, p, p, None) == -1
    assert lib.tpg_emd_finish_f32(p, 0, 8, p, p, p, p, p, None) == 0
    # Gaussian row sums
    assert lib.tpg_gaussian_row_sums_f32(p, p, None, None, 1, 8, 8, 0.0, p, None) == -1
    assert lib.tpg_gaussian_row_sums_f32(p, p, None, None, 1, 8, 8, -0.1, p, None) == -1
    assert lib.tpg_gaussian_row_sums_f32(p, p, None, None, -1, 8, 8, 0.1, p, None) == -1
    assert lib.tpg_gaussian_row_sums_f32(p, p, None, None, 1, -8, 8, 0.1, p, None) == -1
    assert lib.tpg_gaussian_row_sums_f32(p, p, None, None, 1, 8, -8, 0.1, p, None) == -1
    assert lib.tpg_gaussian_row_sums_f32(None, p, None, None, 1, 8, 8, 0.1, p, None) == -1
    assert lib.tpg_gaussian_row_sums_f32(p, None, None, None, 1, 8, 8, 0.1, p, None) == -1
    assert lib.tpg_gaussian_row_sums_f32(p, p, None, None, 1, 8, 8, 0.1, None, None) == -1
    assert lib.tpg_gaussian_row_sums_f32(p, p, None, None, 1, 8, 1 << 17, 0.1, p, None) == -3
    assert lib.tpg_gaussian_row_sums_f32(p, p, None, None, 70000, 8, 8, 0.1, p, None) == -3
    assert lib.tpg_gaussian_row_sums_f32(p, p, None, None, 0, 8, 8, 0.1, p, None) == 0
    assert lib.tpg_gaussian_row_sums_f32(p, p, None, None, 1, 0, 8, 0.1, p, None) == 0


def test_cpu_tensors_are_refused():
    import tpgan_amd  # noqa: F401
    from tpgan_amd import metrics, ops
    ops.unregister_backend("cpu")
    x = torch.rand(1, 16, 3)
    for call in (lambda: ops.emd_match(x, x), lambda: ops.gaussian_row_sums(x, x, 0.1),
                 lambda: metrics.emdModule()(x, x, 0.01, 100), lambda: metrics.earth_mover_distance(x, x),
                 lambda: metrics.gaussian_mmd(x, x), lambda: metrics.position_loss(x, x, x),
                 lambda: metrics.action_position_loss(x, x),
                 lambda: metrics.earth_mover_distance_loss(torch.rand(1024, 3), torch.rand(1030, 3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_argument_errors_of_the_ops_the_metrics_and_the_cli(capsys):
    import tpgan_amd  # noqa: F401
    from tpgan_amd import evaluate, metrics, ops
    x, y = torch.rand(1, 16, 3), torch.rand(1, 17, 3)
    with pytest.raises(RuntimeError, match="equal-size"):
        ops.emd_match(x, y)
    with pytest.raises(RuntimeError, match="batch mismatch"):
        ops.emd_match(x, torch.rand(2, 16, 3))
    with pytest.raises(RuntimeError, match=r"\(B,n,3\)"):
        ops.emd_match(x[0], x[0])
    for bad in (dict(eps=0.0), dict(iters=0), dict(phases=-1), dict(scaling=0.5), dict(_narrow_at=-1),
                dict(_check_every=0)):
        with pytest.raises(RuntimeError, match="must be"):
            ops.emd_match(x, x, **bad)
    with pytest.raises(RuntimeError, match="sigma must be positive"):
        ops.gaussian_row_sums(x, y, 0.0)
    with pytest.raises(RuntimeError, match=r"\(B,N,3\)"):
        ops.gaussian_row_sums(x, y[0], 0.1)
    with pytest.raises(RuntimeError, match="at least 1024 points"):
        metrics.earth_mover_distance_loss(torch.rand(100, 3), torch.rand(2000, 3))
    with pytest.raises(RuntimeError, match="clouds must be"):
        metrics.position_loss(x[0], x, x)
    with pytest.raises(RuntimeError, match="batch mismatch"):
        metrics.action_position_loss(x, torch.rand(2, 16, 3))
    ok = ["--pred", "p_{i}.npy", "--gt", "g_{i}.npz", "--count", "2"]
    a = evaluate.parse_args(ok)
    assert (a.start, a.emd_points, a.emd_iters, a.seed, a.out) == (0, None, None, 0, None)
    assert evaluate.parse_args(ok + ["--emd_iters", "7"]).emd_iters == 7
    assert [metrics.round_cap(n, 3000) for n in (1, 1024, 2048, 2049, 4096, 79872)] == [3000, 3000, 3000, 6000, 6000, 117000]
    assert evaluate.default_emd_points(5000, 4097) == 4096 and evaluate.default_emd_points(300, 5000) == 300
    for bad in (["--pred", "p.npy"] + ok[2:], ok[:3] + ["g.npz"] + ok[4:], ok[:5] + ["0"], ok + ["--start", "-1"],
                ok + ["--emd_points", "0"], ok + ["--emd_iters", "0"], ok[:4]):
        with pytest.raises(SystemExit):
            evaluate.parse_args(bad)
    capsys.readouterr()


# ------------------------------------------------------- 4. the golden against a backend of the statements
class StatementBackend:
    """A CPU test backend: the oracle's Chamfer search plus the two statements; records what the ops were handed."""

    name = "statement-cpu"

    def __init__(self):
        from oracle.torch_backend import OracleBackend
        self._oracle = OracleBackend()
        self.emd_calls, self.gauss_calls = [], []

    def chamfer_fwd(self, src, tgt):
        return self._oracle.chamfer_fwd(src, tgt)

    def emd_match(self, xyz1, xyz2, eps, iters, phases, scaling, narrow_at=None, check_every=None):
        self.emd_calls.append((xyz1.numpy().copy(), xyz2.numpy().copy(), eps, iters))
        out = [auction_statement(a, b, eps, iters, phases, scaling) for a, b in zip(xyz1.numpy(), xyz2.numpy())]
        return (torch.from_numpy(np.stack([o[0] for o in out])), torch.from_numpy(np.stack([o[1] for o in out])),
                torch.from_numpy(np.stack([o[2] for o in out])), torch.tensor([o[3] for o in out], dtype=torch.int32))

    def gaussian_row_sums(self, a, b, lena, lenb, sigma):
        assert lena is None and lenb is None
        self.gauss_calls.append((a.numpy().copy(), b.numpy().copy(), sigma))
        return torch.from_numpy(np.stack([gaussian_statement(x, y, sigma)[0] for x, y in zip(a.numpy(), b.numpy())]))


@pytest.fixture()
def statement_backend():
    import tpgan_amd  # noqa: F401
    from tpgan_amd import ops
    be = StatementBackend()
    ops.register_backend("cpu", be)
    yield be
    ops.unregister_backend("cpu")


def within_ulps(got, want, ulps):
    return np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulps * np.spacing(np.abs(want)))


def test_fluid_position_loss_hands_the_ops_what_the_reference_hands_its_packages(statement_backend):
    from tpgan_amd import metrics
    g = np.load(GOLDEN)
    masked, pred, gt = (torch.from_numpy(g[f"fluid/{k}"]) for k in ("masked_pos", "pos_pred", "pos_gt"))
    keep = [t.clone() for t in (masked, pred, gt)]
    cd, emd, mmd = metrics.position_loss(masked, pred, gt)
    for t, k in zip((masked, pred, gt), keep):
        assert torch.equal(t, k), "inputs must not be modified"
    (x1, x2, eps, iters), = statement_backend.emd_calls
    assert eps == float(g["fluid/emd_eps"]) == 0.03 and iters == int(g["fluid/emd_iters"]) == 3000
    assert within_ulps(x1, g["fluid/emd_xyz1"], 2) and within_ulps(x2, g["fluid/emd_xyz2"], 2)
    calls = statement_backend.gauss_calls
    assert len(calls) == 3 and all(c[2] == float(g["fluid/mmd_blur"]) == 0.01 for c in calls)
    assert within_ulps(calls[0][0], g["fluid/mmd_x"], 2) and within_ulps(calls[1][0], g["fluid/mmd_y"], 2)
    assert abs(float(cd) - float(g["fluid/cd"])) <= 1e-5 * abs(float(g["fluid/cd"]))
    want, bound = mmd_statement(g["fluid/mmd_x"][0], g["fluid/mmd_y"][0], 0.01)
    print(f"mmd {float(mmd):.9e} golden {float(g['fluid/mmd']):.9e} bound {bound:.3e}")
    assert abs(want - float(g["fluid/mmd"])) <= bound
    assert abs(float(mmd) - float(g["fluid/mmd"])) <= bound
    # emd: the mean distance of the statement's matching of the recorded clouds
    dist = auction_statement(g["fluid/emd_xyz1"][0], g["fluid/emd_xyz2"][0], 0.03, 3000, metrics.schedule_phases(0.03))[0]
    assert abs(float(emd) - float(np.sqrt(dist).mean())) <= 1e-6 * float(emd)
    # and the matching scipy filled the reference's stand-in with is within n * eps of it in the sum of squares
    assert dist.astype(np.float64).sum() <= float(g["fluid/emd_optimum"]) + dist.shape[0] * 0.03


def test_action_position_loss_hands_the_ops_what_the_reference_hands_its_package(statement_backend):
    from tpgan_amd import metrics
    g = np.load(GOLDEN)
    pred, gt = torch.from_numpy(g["action/pos_pred"]), torch.from_numpy(g["action/pos_gt"])
    keep = pred.clone(), gt.clone()
    cd, emd = metrics.action_position_loss(pred, gt)
    assert torch.equal(pred, keep[0]) and torch.equal(gt, keep[1])
    (x1, x2, eps, iters), = statement_backend.emd_calls
    assert eps == float(g["action/emd_eps"]) == 0.002 and iters == int(g["action/emd_iters"]) == 3000
    assert within_ulps(x1, g["action/emd_xyz1"], 2) and within_ulps(x2, g["action/emd_xyz2"], 2)
    assert abs(float(cd) - float(g["action/cd"])) <= 1e-5 * abs(float(g["action/cd"]))
    n = x1.shape[1]
    total = (float(emd) / 2.0)                                    # mean sqrt(dist) of the halved clouds
    assert total > 0
    dist = auction_statement(x1[0], x2[0], 0.002, 3000, metrics.schedule_phases(0.002))[0]
    assert dist.astype(np.float64).sum() <= float(g["action/emd_optimum"]) + n * 0.002


def test_emd_loss_is_differentiable_through_the_matched_distances(statement_backend):
    from tpgan_amd import metrics
    rng = np.random.RandomState(5)
    pred = torch.from_numpy(rng.rand(1024, 3).astype(F)).requires_grad_(True)
    target = torch.from_numpy(rng.rand(1100, 3).astype(F))
    gen = torch.Generator().manual_seed(3)
    loss = metrics.earth_mover_distance_loss(pred, target, gen)
    again = metrics.earth_mover_distance_loss(pred, target, torch.Generator().manual_seed(3))
    assert torch.equal(loss, again) and loss.requires_grad
    (x1, x2, eps, iters) = statement_backend.emd_calls[0]
    assert x1.shape == (1, 1024, 3) and (eps, iters) == (0.05, 2000)
    loss.backward()
    assert pred.grad is not None and torch.isfinite(pred.grad).all() and float(pred.grad.abs().sum()) > 0

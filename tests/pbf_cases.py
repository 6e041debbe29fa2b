"""The small batches the simulator's tests share (tests/test_simulate_cpu.py, tests/test_simulate_gpu.py): shapes at which
the kernels of csrc/pbf.hip can still go wrong, small enough for the O(N^2) numpy rule."""
import numpy as np

F32 = np.float32
A = F32(0.0125)                        # particle radius; spacing 0.025, support 0.05


def _lattice(origin, n, spacing=0.025):
    g = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), -1).reshape(-1, 3)
    return (np.asarray(origin) + g * spacing).astype(F32)


def small_case():
    """B = 2 ragged clouds of 700 and 451 particles in boxes only a few cells wide -> x, v (2,700,3) fp32 with NaN rows
    beyond the lengths, lengths, box_lo, box_hi (2,3).  Cloud 0: two lattice bodies on a collision course that also
    run into the walls, 20 exact duplicates, a tight cluster of 90 points (more than 64 candidates in one particle's cells:
    several trips of the candidate loop), a particle exactly on the clamp plane and one outside the box.  Cloud 1: a
    lattice at rest on the floor under random points, in another box."""
    rng = np.random.default_rng(11)
    lo = np.array([[0.0, 0.0, 0.0], [-0.1, 0.05, -0.2]], F32)
    hi = np.array([[0.22, 0.3, 0.17], [0.1, 0.3, 0.0]], F32)
    a = _lattice([0.02, 0.03, 0.02], (6, 6, 6))                                  # 216, thrown right and down
    b = _lattice([0.07, 0.14, 0.03], (6, 6, 5)) + F32(0.004)                     # 180, thrown left
    cluster = (np.array([0.11, 0.1, 0.09]) + rng.normal(0, 0.004, (90, 3))).astype(F32)
    plane = np.array([[lo[0, 0] + A, 0.2, 0.1], [0.3, 0.2, 0.05]], F32)          # on the clamp plane; outside the box
    fill = rng.uniform(lo[0] + 0.01, hi[0] - 0.01, (700 - 216 - 180 - 90 - 2 - 20, 3)).astype(F32)
    x0 = np.concatenate([a, b, cluster, plane, fill])
    twins = rng.choice(len(x0), 20, replace=False)
    x0 = np.concatenate([x0, x0[twins]])                                         # exact duplicates
    v0 = rng.normal(0, 0.3, x0.shape).astype(F32)
    v0[:216] += np.array([2.0, -1.0, 0.5], F32)
    v0[216:396] += np.array([-2.0, 0.0, -0.5], F32)
    v0[-20:-10] = v0[twins[:10]]                                                 # ten of them stay duplicates when they move
    x1 = np.concatenate([_lattice(lo[1] + A, (8, 4, 8)),                         # 256 on the floor, against two walls
                         rng.uniform(lo[1], hi[1], (451 - 256, 3)).astype(F32)])
    v1 = np.concatenate([np.zeros((256, 3), F32), rng.normal(0, 1.0, (451 - 256, 3)).astype(F32)])
    assert x0.shape == (700, 3) and x1.shape == (451, 3)
    x, v = np.full((2, 700, 3), np.nan, F32), np.full((2, 700, 3), np.nan, F32)
    x[0], v[0], x[1, :451], v[1, :451] = x0, v0, x1, v1
    return x, v, np.array([700, 451], np.int64), lo, hi


def tiny_case():
    """One 1-particle cloud and one empty cloud (N = 3: the rows beyond are NaN)."""
    x, v = np.full((2, 3, 3), np.nan, F32), np.full((2, 3, 3), np.nan, F32)
    x[0, 0], v[0, 0] = [0.05, 0.0126, 0.05], [0.3, -1.0, 0.0]
    lo, hi = np.zeros((2, 3), F32), np.full((2, 3), 0.2, F32)
    return x, v, np.array([1, 0], np.int64), lo, hi

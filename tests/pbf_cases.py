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


# ---- the grid the kernels walk, stated in numpy (csrc/frnn_grid_build.hpp, pbf_walk of csrc/pbf.hip) -------------------
class Grid:
    """The uniform grid of one scene p (n,3) for support h, in the header's fp32 operations: cell edge
    max(h, extent / 64) * 1.0001, `dim` cells per axis (<= 64), `cell` (n,3) the clamped cell of every particle."""

    def __init__(self, p, h):
        p = np.asarray(p, F32)
        self.lo, mx = p.min(0), p.max(0)
        self.extent = F32((mx - self.lo).max())
        self.edge = np.maximum(F32(h), self.extent / F32(64)) * F32(1.0001)
        self.inv = F32(1) / self.edge
        self.dim = np.clip(np.floor((mx - self.lo) * self.inv).astype(np.int64) + 1, 1, 64)
        self.cell = np.clip(np.floor((p - self.lo) * self.inv).astype(np.int64), 0, self.dim - 1)

    def walks(self, lower_strict=False):
        """Per particle the candidates of its walk in the walk's order (9 runs of up to 3 x-adjacent cells; inside a
        cell by index, where the device's order is not fixed).  lower_strict: the planted defect `yy > 0` for
        `yy >= 0` (and zz), which on an axis with dim == 1 cuts the only layer there is."""
        key = (self.cell[:, 2] * self.dim[1] + self.cell[:, 1]) * self.dim[0] + self.cell[:, 0]
        order = np.argsort(key, kind="stable")
        skey = key[order]
        first = 1 if lower_strict else 0
        out = []
        for cx, cy, cz in self.cell:
            x0, x1 = max(cx - 1, 0), min(cx + 1, self.dim[0] - 1)
            run = []
            for t in range(9):
                zz, yy = cz + t // 3 - 1, cy + t % 3 - 1
                if first <= zz < self.dim[2] and first <= yy < self.dim[1]:
                    row = (zz * self.dim[1] + yy) * self.dim[0]
                    run.append(order[np.searchsorted(skey, row + x0):np.searchsorted(skey, row + x1, side="right")])
            out.append(np.concatenate(run) if run else np.zeros(0, np.int64))
        return out


def params(name):
    """The `ops.PbfParams` a case runs with."""
    from tpgan_amd import ops
    return ops.PbfParams(**CASES[name][1])


def _pack(clouds, vels, N):
    B = len(clouds)
    x, v = np.full((B, N, 3), np.nan, F32), np.full((B, N, 3), np.nan, F32)
    for b, (c, w) in enumerate(zip(clouds, vels)):
        x[b, :len(c)], v[b, :len(c)] = c, w
    return x, v, np.array([len(c) for c in clouds], np.int64)


def _rule():
    import pbf_rule
    return pbf_rule


def chunk_case():
    """B = 130 scenes of up to N = 48 particles: three launches of the kernels that carry their boxes in the arguments
    (b0 = 0, 64, 128).  Ragged lengths with 0 and 48 among them; every scene in a box of its own, no lo or hi value
    shared by two scenes on any axis; a squeezed lattice thrown into one corner of its box (the lo corner in even
    scenes, the hi corner in odd ones).  Asserted: in every non-empty scene predict and the first dp each move at least one
    particle that lay strictly beyond a clamp plane onto it, so another scene's box row changes bits."""
    P, prm, dt = _rule(), params("chunk"), CASES["chunk"][2]
    rng = np.random.default_rng(130)
    B, N = 130, 48
    lengths = rng.integers(12, 48, B)
    lengths[[0, 5, 63, 64, 70, 128, 129]] = [48, 0, 31, 48, 0, 17, 48]
    lo = np.stack([-0.2 + 0.0013 * rng.permutation(B) for _ in range(3)], 1).astype(F32)
    hi = np.stack([0.2005 + 0.0013 * rng.permutation(B) for _ in range(3)], 1).astype(F32)
    for a in range(3):
        assert len(np.unique(np.concatenate([lo[:, a], hi[:, a]]))) == 2 * B
    clouds, vels = [], []
    for s in range(B):
        n = int(lengths[s])
        g = _lattice([0, 0, 0], (4, 3, 4), 0.018)[rng.permutation(48)[:n]]
        g = g + rng.uniform(0, 0.002, g.shape).astype(F32) * (g > 0)          # the layers on the planes stay on them
        w = (-1.5 + rng.normal(0, 0.2, g.shape)).astype(F32)
        if s % 2:
            c, w = (hi[s] - A) - g, -w
        else:
            c = (lo[s] + A) + g
        clouds.append(c.astype(F32))
        vels.append(w.astype(F32))
    x, v, lengths = _pack(clouds, vels, N)
    for s in range(B):
        n = int(lengths[s])
        if n == 0:
            continue
        lo_c, hi_c = lo[s] + A, hi[s] - A
        vv = v[s, :n] + F32(dt) * np.asarray(prm.gravity, F32)
        free = x[s, :n] + F32(dt) * vv
        assert ((free < lo_c) | (free > hi_c)).any(), s
        p, _ = P.predict_rule(x[s, :n], v[s, :n], lo[s], hi[s], dt, prm)
        lam, _ = P.lambda_rule(p, prm)
        _, dp = P.dp_rule(p, lam, lo[s], hi[s], prm)
        assert ((p + dp < lo_c) | (p + dp > hi_c)).any(), s
    return x, v, lengths, lo, hi


def wide_case():
    """Two scenes of three blobs in a box of 4.2 x 0.3 x 0.3 m, centres at x = 0.1, 2.0 and 4.1: the extent is above
    64 h, so the grid is coarse (cells wider than the support, 64 of them along x).  A cluster of 140 points within one
    support, a lattice of 48 and 52 random points; the second scene is the mirror image with 230 particles and other
    velocities.  Asserted at the predicted positions and after every dp of the substep: extent / 64 > h and dim = 64
    along x; and at the predicted positions some walk has more than 128 candidates."""
    P, prm, dt = _rule(), params("wide"), CASES["wide"][2]
    rng = np.random.default_rng(42)
    lo = np.zeros((2, 3), F32)
    hi = np.tile(np.array([4.2, 0.3, 0.3], F32), (2, 1))
    cluster = (np.array([0.1, 0.15, 0.14]) + rng.normal(0, 0.008, (140, 3))).astype(F32)
    body = _lattice([1.96, 0.1, 0.11], (4, 4, 3))
    cloud = (np.array([4.1, 0.12, 0.17]) + rng.normal(0, 0.03, (52, 3))).astype(F32)
    x0 = np.concatenate([cluster, body, cloud])
    v0 = rng.normal(0, 0.5, x0.shape).astype(F32)
    v0[140:188] += np.array([1.0, -0.5, 0.3], F32)
    x1 = (np.array([4.2, 0.3, 0.3], F32) - x0[rng.permutation(240)[:230]]).astype(F32)
    v1 = rng.normal(0, 1.0, x1.shape).astype(F32)
    x, v, lengths = _pack([x0, x1], [v0, v1], 240)
    for s in range(2):
        n = int(lengths[s])
        p, _ = P.predict_rule(x[s, :n], v[s, :n], lo[s], hi[s], dt, prm)
        g = Grid(p, prm.h)
        assert max(len(w) for w in g.walks()) > 128
        assert (np.bincount(np.nonzero(P.Pairs(p, prm).near)[0]) > 64).any()      # more than 64 WITHIN one support
        for it in range(prm.iters + 1):
            g = Grid(p, prm.h)
            assert g.extent / F32(64) > F32(prm.h) and g.dim[0] == 64 and g.edge > F32(prm.h) * F32(1.2), (s, it)
            if it < prm.iters:
                lam, _ = P.lambda_rule(p, prm)
                p, _ = P.dp_rule(p, lam, lo[s], hi[s], prm)
    return x, v, lengths, lo, hi


def flat_case():
    """Flat grids.  Scene 0: a sheet of 9 x 7 particles at y = lo + a (the floor's clamp plane), squeezed to a spacing
    of 0.02, with in-plane velocities: dim == 1 along y.  Scene 1: a row of 30 along x on the floor: dim == 1 along y
    and z.  Asserted: after the substep every particle has the y (y and z) it started with, exactly, and has moved."""
    P, prm, dt = _rule(), params("flat"), CASES["flat"][2]
    rng = np.random.default_rng(97)
    lo = np.array([[0.0, 0.0, 0.0], [-0.3, 0.1, 0.05]], F32)
    hi = np.array([[0.4, 0.2, 0.3], [0.5, 0.3, 0.2]], F32)
    sheet = _lattice([0.1, 0.0, 0.08], (9, 1, 7), 0.02)
    sheet[:, 1] = lo[0, 1] + A
    vs = rng.normal(0, 0.5, sheet.shape).astype(F32)
    vs[:, 1] = 0
    row = _lattice([-0.2, 0.0, 0.11], (30, 1, 1), 0.021)
    row[:, 1] = lo[1, 1] + A
    vr = np.zeros_like(row)
    vr[:, 0] = rng.normal(0, 0.5, 30).astype(F32)
    x, v, lengths = _pack([sheet, row], [vs, vr], 63)
    for s, flat in ((0, [1]), (1, [1, 2])):
        n = int(lengths[s])
        xs, _ = P.substep_rule(x[s, :n], v[s, :n], lo[s], hi[s], dt, prm)
        assert np.array_equal(xs[:, flat], x[s, :n][:, flat]) and (xs != x[s, :n]).any(1).all(), s
        p, _ = P.predict_rule(x[s, :n], v[s, :n], lo[s], hi[s], dt, prm)
        for g in (Grid(p, prm.h), Grid(xs, prm.h)):
            assert (g.dim[flat] == 1).all() and g.dim[0] > 3, s
    return x, v, lengths, lo, hi


def clamp_case():
    """The term clamp, with eps = 1e-30, no gravity and dt = 2^-20.  Scene 0: 12 exact duplicates, one partner 0.0499 away
    along x (a gradient of 4e-6 against a constraint of 1.3: lambda is -8e10 and the 24 dp terms of the pairs are near
    3e5), and a bystander at rest on the very spot of the wall where the clamp then puts the duplicates: the finish pass
    has pairs at distance 0 whose velocities differ by 9e4 m/s.  Scene 1: the same along z with 7 duplicates and the
    partner at the largest distance that is still inside the support: its gradient, 5e-14, vanishes from the fixed-point
    sums of the lambda pass, lambda is -C / eps = -4e29 and the dp terms are 2e16, beyond 2^33, where a clamp applied
    after the conversion to integer has already overflowed.  Asserted per scene: the dp and the XSPH terms of all pairs
    with a duplicate lie beyond the clamp (scene 1: beyond 2^33), no term is NaN, the results are finite."""
    P, prm, dt = _rule(), params("clamp"), CASES["clamp"][2]
    lo = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -0.1]], F32)
    hi = np.array([[0.3, 0.2, 0.2], [0.2, 0.2, 0.2]], F32)
    h = F32(prm.h)
    clouds = []
    for s, (axis, twins) in enumerate(((0, 12), (2, 7))):
        at = np.array([0.1, 0.1, 0.1], F32)
        partner, bystander = at.copy(), at.copy()
        partner[axis] += F32(0.0499)
        if s == 1:
            partner[axis] = at[axis] + h
            while not (partner[axis] - at[axis]) * (partner[axis] - at[axis]) < h * h:
                partner[axis] = np.nextafter(partner[axis], F32(0))
        bystander[axis] = lo[s, axis] + A
        clouds.append(np.stack([at] * twins + [partner, bystander]))
    x, v, lengths = _pack(clouds, [np.zeros_like(c) for c in clouds], 14)
    for s in range(2):
        n = int(lengths[s])
        p, _ = P.predict_rule(x[s, :n], v[s, :n], lo[s], hi[s], dt, prm)
        dp_count, xsph_count = {}, {}
        for _ in range(prm.iters):
            lam, _ = P.lambda_rule(p, prm)
            p, _ = P.dp_rule(p, lam, lo[s], hi[s], prm, dp_count)
        vf = P.finish_rule(p, x[s, :n], dt, prm, xsph_count)
        assert dp_count["over"] == 2 * (n - 2) and xsph_count["over"] == 2 * (n - 2), (dp_count, xsph_count)
        assert dp_count["nan"] == 0 and xsph_count["nan"] == 0
        assert s == 0 or dp_count["max"] > 2.0 ** 33
        assert np.isfinite(p).all() and np.isfinite(vf).all()
    return x, v, lengths, lo, hi


def full_small():
    """small_case with every row in use: the rows beyond the lengths hold particles at rest (duplicates of one point, outside
    scene 1's box), for calls without lengths and with lengths that stand for N."""
    x, v, _, lo, hi = small_case()
    return np.nan_to_num(x, nan=0.11), np.nan_to_num(v, nan=0.0), np.array([700, 700], np.int64), lo, hi


# PbfParams arguments other than the shipped ones: predict, grid and finish only; no tensile term; no XSPH; gravity off y
VARIANTS = {"iters0": dict(iters=0), "k0": dict(k=0.0), "c0": dict(c=0.0), "gravity": dict(gravity=(3.0, 0.0, -2.0))}


def odd_lengths(N):
    """Lengths of a 2-scene batch outside [0, N] and what they stand for (include/tpgan_ops.h: clamped into [0, N] as the
    64-bit values they are; 2^32 + 5 narrowed to int first would be 5)."""
    return [([N + 7, -3], [N, 0]), ([-3, 2 ** 32 + 5], [0, N]), ([2 ** 32 + 5, N + 7], [N, N]),
            ([2 ** 63 - 1, -2 ** 63], [N, 0])]


DT = float(F32(1.0 / 160.0))
# name -> (builder, PbfParams arguments, dt)
CASES = {
    "small": (small_case, {}, DT),
    "tiny": (tiny_case, {}, DT),
    "chunk": (chunk_case, {}, DT),
    "wide": (wide_case, {}, DT),
    "flat": (flat_case, {}, DT),
    "clamp": (clamp_case, dict(eps=1e-30, gravity=(0.0, 0.0, 0.0)), float(2.0 ** -20)),
}

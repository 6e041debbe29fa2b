"""The batches the obstacle tests share (tests/test_obstacles_cpu.py, tests/test_obstacles_gpu.py).  A case is a dict of
p (B,N,3) fp32 with NaN rows beyond the lengths, lengths (B,) int64, lo, hi (B,3) and table (B,M,16) fp32.  Every builder
asserts through the numpy rule (tests/pbf_obstacle_rule.py), by `hit` bits and by equality tests on the rule's
intermediates, that its particles sit on the edge they are for."""
import numpy as np

import pbf_obstacle_rule as O

F32 = np.float32
A = F32(0.0125)                        # particle radius
EYE = np.eye(3)
WIDE = ([-2.0, -2.0, -2.0], [2.0, 2.0, 2.0])          # a box no particle of the case comes near


def params(**kw):
    from tpgan_amd import ops
    return ops.PbfParams(**kw)


def row(kind, centre=(0, 0, 0), R=EYE, size=(0, 0, 0)):
    out = np.zeros(16, F32)
    size = np.atleast_1d(np.asarray(size, np.float64))
    out[0], out[1:4], out[4:13], out[13:13 + len(size)] = kind, centre, np.asarray(R, np.float64).reshape(-1), size
    return out


def as_dicts(rows):
    """Table rows as the obstacle dicts `ops.pbf_obstacles` takes (it gives these rows back, bit for bit)."""
    names = {1: ("ball", 1), 2: ("box", 3), 3: ("cylinder", 2)}
    return [{"shape": names[int(r[0])][0], "centre": [float(c) for c in r[1:4]], "rotation": [float(c) for c in r[4:13]],
             "size": [float(c) for c in r[13:13 + names[int(r[0])][1]]]} for r in rows if r[0] != 0]


def rotation(axis, degrees):
    """Rodrigues; exact entries for multiples of 90 degrees."""
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    if degrees % 90 == 0:
        c, s = float(round(c)), float(round(s))
    return np.eye(3) + s * K + (1 - c) * (K @ K)


def pack(clouds, boxes, tables, N=None):
    """clouds: (n,3) per scene; boxes: (lo, hi) per scene; tables: rows per scene (padded with kind-0 rows)."""
    B = len(clouds)
    N = N or max(len(c) for c in clouds)
    M = max(len(t) for t in tables)
    p = np.full((B, N, 3), np.nan, F32)
    table = np.zeros((B, M, 16), F32)
    for b in range(B):
        p[b, :len(clouds[b])] = clouds[b]
        for o, r in enumerate(tables[b]):
            table[b, o] = r
    return dict(p=p, lengths=np.array([len(c) for c in clouds], np.int64),
                lo=np.array([bx[0] for bx in boxes], F32).reshape(B, 3), hi=np.array([bx[1] for bx in boxes], F32).reshape(B, 3),
                table=table)


def run(case, b, prm=None, table=None):
    """The rule on scene b -> (p, hit, trace)."""
    prm = prm or params()
    n = int(case["lengths"][b])
    hit, trace = np.zeros(n, np.int32), []
    out = O.collide_rule(case["p"][b, :n], case["lo"][b], case["hi"][b], case["table"][b] if table is None else table, prm,
                         hit, trace)
    return out, hit, trace


def expected(case, prm=None):
    """Per scene (p, hit) by the rule."""
    return [run(case, b, prm)[:2] for b in range(len(case["lengths"]))]


def _same(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.int32), np.asarray(b, F32).view(np.int32))


# ---- the shapes' own edges ---------------------------------------------------------------------------------------------
def on_sphere(E, rng):
    """A point off the axes with d2 == E*E exactly whose projection (q / d) * E would change its bits: what a non-strict
    inside test would move."""
    for _ in range(100000):
        q = rng.normal(size=3)
        q = (q / np.linalg.norm(q) * float(E)).astype(F32)
        d2 = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]
        if d2 == E * E and not _same((q / np.sqrt(d2)) * E, q):
            return q
    raise AssertionError("no such point")


def ball_case():
    """One ball of radius 0.25 at the origin, unrotated (q == p exactly).  Particle 0 at its centre (d2 == 0: it leaves
    through +y); 1 exactly on d2 == E*E (not inside: its bits stay); 2 one ulp inside of that; then ordinary ones."""
    E = F32(0.25) + A
    rng = np.random.default_rng(1)
    pts = np.concatenate([np.array([[0, 0, 0], [E, 0, 0], [np.nextafter(E, F32(0)), 0, 0], [0, -0.1, 0.05], [0.3, 0.3, 0.3]], F32),
                          rng.uniform(-0.4, 0.4, (40, 3)).astype(F32), on_sphere(E, rng)[None]])
    case = pack([pts], [WIDE], [[row(1, size=0.25)]])
    out, hit, (t,) = run(case, 0)
    assert t["d2"][-1] == E * E and hit[-1] == 0                                 # the last: on the sphere, off the axes
    assert t["d2"][0] == 0 and hit[0] == 1 and _same(out[0], [0, E, 0])
    assert t["d2"][1] == E * E and hit[1] == 0 and _same(out[1], pts[1])
    assert t["d2"][2] < E * E and hit[2] == 1
    assert hit[4] == 0 and 5 < hit.sum() < len(pts) - 5 and all(_same(out[i], pts[i]) for i in np.nonzero(hit == 0)[0])
    return case


def box_case():
    """Scene 0, a cube of half extent 0.1: particle 0 on the body diagonal (a three-way tie of pen: axis 0), 1 with pen_1
    == pen_2 < pen_0 (axis 1), 2 with pen_0 == pen_2 < pen_1 (axis 0), 3 on the negative side, 4 exactly on a face of the
    expanded cube (not inside).  Scene 1, a slab thin along x: particle 0 has q_0 == 0 on the chosen axis and leaves through
    +x; 1 through -x."""
    E = F32(0.1) + A
    cube = np.array([[0.05, 0.05, 0.05], [0.02, 0.07, 0.07], [0.07, 0.02, 0.07], [-0.08, 0.01, 0.0], [E, 0.0, 0.0],
                     [0.0, 0.03, -0.09], [0.3, 0.0, 0.0]], F32)
    slab = np.array([[0.0, 0.05, -0.03], [-0.001, 0.0, 0.0], [0.0, 0.3, 0.0]], F32)
    Es = F32(0.02) + A
    case = pack([cube, slab], [WIDE, WIDE], [[row(2, size=(0.1, 0.1, 0.1))], [row(2, size=(0.02, 0.1, 0.1))]])
    out, hit, (t,) = run(case, 0)
    pen = np.stack(t["pen"], 1)
    assert pen[0, 0] == pen[0, 1] == pen[0, 2] and t["axis"][0] == 0 and _same(out[0], [E, 0.05, 0.05])
    assert pen[1, 1] == pen[1, 2] < pen[1, 0] and t["axis"][1] == 1 and _same(out[1], [0.02, E, 0.07])
    assert pen[2, 0] == pen[2, 2] < pen[2, 1] and t["axis"][2] == 0 and _same(out[2], [E, 0.02, 0.07])
    assert _same(out[3], [-E, 0.01, 0.0]) and hit[3] == 1
    assert pen[4, 0] == 0 and hit[4] == 0 and _same(out[4], cube[4])
    assert t["axis"][5] == 2 and _same(out[5], [0.0, 0.03, -E]) and hit[6] == 0
    out, hit, (t,) = run(case, 1)
    assert t["axis"][0] == 0 and t["q"][0][0] == 0 and hit[0] == 1 and _same(out[0], [Es, 0.05, -0.03])
    assert _same(out[1], [-Es, 0.0, 0.0]) and hit.tolist() == [1, 1, 0]
    return case


def cylinder_case():
    """A cylinder of radius 0.1 and half height 0.2 along y.  Particle 0 on the axis with pen_r < pen_h (r2 == 0: it leaves
    radially, through +x); 1 with pen_h == pen_r exactly (to the cap); 2 the same particle one ulp lower (radial);
    3 to the lower cap; 4 radial, ordinary; 5 exactly on the expanded radius (not inside); 6 exactly on the cap plane."""
    Er, Eh = F32(0.1) + A, F32(0.2) + A
    y = F32(0.15)
    x = Er - (Eh - y)                                                             # exact: pen_r == pen_h, asserted below
    assert Er - x == Eh - y and np.sqrt(x * x) == x
    pts = np.array([[0, 0.05, 0], [x, y, 0], [x, np.nextafter(y, F32(0)), 0], [0.01, -0.19, 0.02], [0.06, 0.0, -0.07],
                    [Er, 0.0, 0.0], [0.0, Eh, 0.0], [0.3, 0.0, 0.3]], F32)
    case = pack([pts], [WIDE], [[row(3, size=(0.1, 0.2))]])
    out, hit, (t,) = run(case, 0)
    assert t["r2"][0] == 0 and t["pen_r"][0] < t["pen_h"][0] and not t["cap"][0] and _same(out[0], [Er, 0.05, 0])
    assert t["pen_h"][1] == t["pen_r"][1] and t["cap"][1] and _same(out[1], [x, Eh, 0])
    assert t["pen_h"][2] > t["pen_r"][2] and not t["cap"][2] and out[2, 0] == Er and out[2, 1] == pts[2, 1]
    assert _same(out[3], [0.01, -Eh, 0.02]) and not t["cap"][4] and out[4, 1] == 0 and hit[:5].tolist() == [1] * 5
    assert t["r2"][5] == Er * Er and hit[5] == 0 and hit[6] == 0 and hit[7] == 0
    assert all(_same(out[i], pts[i]) for i in (5, 6, 7))
    return case


# ---- several obstacles ---------------------------------------------------------------------------------------------------
def order_case():
    """Scenes 0 and 1: the same particles against two overlapping balls given in both orders; the answers differ.
    Scene 2: a particle that ball 0 pushes into ball 1, which alone would not have touched it."""
    a, b = row(1, (0, 0, 0), size=0.1), row(1, (0.1, 0, 0), size=0.1)
    far = row(1, (0.2, 0, 0), size=0.1)
    pts = np.array([[0.05, 0.01, 0.0], [0.04, -0.03, 0.02], [0.06, 0.0, 0.05], [0.5, 0.5, 0.5]], F32)
    pushed = np.array([[0.08, 0.0, 0.001], [0.5, 0.5, 0.5]], F32)
    case = pack([pts, pts, pushed], [WIDE] * 3, [[a, b], [b, a], [a, far]])
    (o0, h0, _), (o1, h1, _) = run(case, 0), run(case, 1)
    assert all(not _same(o0[i], o1[i]) for i in range(3)) and _same(o0[3], o1[3]) and (h0[:3] > 0).all() and h0[3] == 0
    o2, h2, _ = run(case, 2)
    assert h2.tolist() == [3, 0]
    assert run(case, 2, table=np.stack([far]))[1].tolist() == [0, 0]              # ball 1 alone does not reach it
    return case


def wall_case():
    """A ball that leans on the wall x = 0 of the box [0, 1]^3: it pushes particle 0 through the wall, the final clamp
    puts it back, and its x is the clamp plane's bits.  Particle 1 leaves on the open side."""
    pts = np.array([[0.03, 0.5, 0.5], [0.1, 0.52, 0.5], [0.9, 0.9, 0.9]], F32)
    ball = row(1, (0.05, 0.5, 0.5), size=0.1)
    case = pack([pts], [([0, 0, 0], [1, 1, 1])], [[ball]])
    out, hit, _ = run(case, 0)
    open_case = dict(case, lo=np.array([[-2, -2, -2]], F32))
    free = run(open_case, 0)[0]
    assert hit.tolist() == [1, 1, 0] and free[0, 0] < F32(0) + A and _same(out[0, 0], F32(0) + A)
    assert _same(out[0, 1:], free[0, 1:]) and _same(out[1], free[1]) and _same(out[2], pts[2])
    return case


def rotation_case():
    """Scene 0 unrotated, scene 1 turned by 90 degrees about z (exact entries), scene 2 a generic rotation: each a box and
    a cylinder with centres that are no round numbers, under random particles.  Asserted per scene: both obstacles move
    some particles, and the many particles far from both keep their bits (no round trip through the local frame)."""
    rng = np.random.default_rng(7)
    clouds, tables = [], []
    for R in (EYE, rotation((0, 0, 1), 90), rotation((0.3, -1.0, 0.55), 37.0)):
        tables.append([row(2, (0.113, -0.071, 0.05), R, (0.12, 0.05, 0.08)), row(3, (-0.207, 0.093, -0.11), R, (0.07, 0.15))])
        clouds.append(np.concatenate([rng.uniform(-0.45, 0.45, (60, 3))] +
                                     [t[1:4] + rng.uniform(-0.16, 0.16, (30, 3)) for t in tables[-1]]).astype(F32))
    case = pack(clouds, [WIDE] * 3, tables)
    outs = []
    for b in range(3):
        out, hit, _ = run(case, b)
        n1, n2 = int((hit & 1).astype(bool).sum()), int((hit & 2).astype(bool).sum())
        assert n1 >= 3 and n2 >= 3 and (hit == 0).sum() > 50, (b, n1, n2)
        assert all(_same(out[i], clouds[b][i]) for i in np.nonzero(hit == 0)[0])
        assert all(not _same(out[i], clouds[b][i]) for i in np.nonzero(hit)[0])
        outs.append(out)
    # the rotation reaches the answer: scene 1's particles against scene 0's table give something else
    assert not _same(O.collide_rule(clouds[1], *WIDE, case["table"][0], params()), outs[1])
    return case


def skipped_case():
    """M = 8: kind 0, kind 7, a NaN size, an inf size, an inf centre, a NaN centre, a -inf size, and a valid ball at the
    end.  Every skipped row has a particle that the same row with a finite value in the bad slot would move."""
    rows = [row(0, (0, 0, 0), size=0.05), row(7, (0.2, 0, 0), size=0.05), row(1, (0.4, 0, 0), size=np.nan),
            row(2, (0.6, 0, 0), size=(0.05, np.inf, 0.05)), row(3, (np.inf, 0.3, 0), size=(0.05, 0.05)),
            row(1, (0, np.nan, 0.3), size=0.05), row(1, (0.4, 0.3, 0), size=-np.inf), row(1, (0.6, 0.3, 0), size=0.05)]
    mended = [r.copy() for r in rows]
    mended[0][0] = mended[1][0] = 1
    mended[2][13], mended[3][14], mended[4][1], mended[5][2], mended[6][13] = 0.05, 0.05, 0.2, 0.3, 0.05
    pts = np.array([r[1:4] for r in mended], F32) + np.array([0.01, 0.02, -0.01], F32)
    pts = np.concatenate([pts, np.array([[1.0, 1.0, 1.0]], F32)])
    case = pack([pts], [WIDE], [rows])
    out, hit, trace = run(case, 0)
    assert [O.skipped(r) for r in rows] == [True] * 7 + [False] and len(trace) == 1
    assert hit.tolist() == [0] * 7 + [128, 0] and all(_same(out[i], pts[i]) for i in range(7)) and not _same(out[7], pts[7])
    assert run(case, 0, table=np.stack(mended))[1].tolist() == [1 << o for o in range(8)] + [0]
    return case


def m0_case():
    """M == 0: the clamp alone (two particles beyond the walls)."""
    pts = np.array([[0.5, 0.5, 0.5], [-0.1, 0.5, 1.2], [0.0125, 0.3, 0.9875]], F32)
    case = pack([pts], [([0, 0, 0], [1, 1, 1])], [[]])
    assert case["table"].shape == (1, 0, 16)
    out, hit, trace = run(case, 0)
    assert not trace and not hit.any() and _same(out[1], [A, 0.5, F32(1) - A]) and _same(out[0], pts[0]) and _same(out[2], pts[2])
    return case


def m8_case():
    """M == 8 with all eight obstacles hitting some particle: bits 0 .. 7 all occur."""
    R = rotation((1, 1, 0), 50.0)
    rows = [row(1 + o % 3, (0.3 * (o % 4), 0.3 * (o // 4), 0.01 * o), R, (0.06, 0.07, 0.08)[:(1, 3, 2)[o % 3]]) for o in range(8)]
    rng = np.random.default_rng(8)
    pts = np.concatenate([np.array([r[1:4] for r in rows], F32) + rng.uniform(-0.03, 0.03, (8, 3)).astype(F32),
                          rng.uniform(-0.2, 1.1, (30, 3)).astype(F32)])
    case = pack([pts], [WIDE], [rows])
    _, hit, trace = run(case, 0)
    assert len(trace) == 8 and np.bitwise_or.reduce(hit) == 255 and hit[:8].tolist() == [1 << o for o in range(8)]
    return case


def batch_case():
    """130 scenes of up to N = 48 particles: three launches of the chunked kernel.  Every scene has a box of its own and a
    table of its own (a ball, a box and a cylinder, each rotated, M = 3); ragged lengths with 0 and 48 among them.
    Asserted per non-empty scene: an obstacle moves a particle, the clamp moves a particle, and another scene's box or
    table would give other bits."""
    rng = np.random.default_rng(131)
    B, N = 130, 48
    lengths = rng.integers(30, 48, B)
    lengths[[0, 5, 63, 64, 70, 128, 129]] = [48, 0, 31, 48, 0, 17, 48]
    clouds, boxes, tables = [], [], []
    for s in range(B):
        lo = rng.uniform(-0.3, -0.2, 3)
        hi = lo + rng.uniform(0.45, 0.55, 3)
        centres = lo + (hi - lo) * rng.uniform(0.25, 0.75, (3, 3))
        rows = [row(1 + o, centres[o], rotation(rng.normal(size=3), rng.uniform(0, 360)),
                    rng.uniform(0.05, 0.09, (1, 3, 2)[o])) for o in range(3)]
        pts = rng.uniform(lo - 0.02, hi + 0.02, (int(lengths[s]), 3))
        if len(pts):
            pts[:3] = centres + rng.uniform(-0.02, 0.02, (3, 3))
            pts[3] = hi + 0.01
        clouds.append(pts.astype(F32))
        boxes.append((lo, hi))
        tables.append(rows)
    case = pack(clouds, boxes, tables, N)
    want = expected(case)
    for s in range(B):
        n = int(lengths[s])
        if n == 0:
            continue
        out, hit = want[s]
        assert hit.any() and _same(out[3], case["hi"][s] - A), s
        t = (s + 64) % B if lengths[(s + 64) % B] else (s + 1) % B
        other = dict(case, lo=case["lo"][[t] * B], hi=case["hi"][[t] * B])
        assert not _same(run(other, s)[0], out), s                                # another chunk's box row
        assert not _same(run(case, s, table=case["table"][t])[0], out), s         # another chunk's table
    return case


# ---- whole substeps --------------------------------------------------------------------------------------------------------
def _lattice(origin, n, spacing=0.025):
    g = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), -1).reshape(-1, 3)
    return (np.asarray(origin) + g * spacing).astype(F32)


def drop_case():
    """A lattice of 500 particles whose lowest layers already reach into a ball and a rotated box near the floor of a
    box of 0.5 m, falling at 1.5 m/s: the first collide of the first substep moves particles, and within four frames the
    fluid flows round both.  Scene 1: 320 particles thrown sideways into a cylinder they already touch.
    -> (case, v): v (B,N,3) with NaN rows beyond the lengths."""
    ball = row(1, (0.16, 0.1, 0.2), size=0.08)
    box = row(2, (0.31, 0.11, 0.22), rotation((0.2, 1.0, 0.4), 33.0), (0.07, 0.05, 0.09))
    cyl = row(3, (0.3, 0.15, 0.25), rotation((1, 0, 0), 90), (0.05, 0.12))
    a = _lattice([0.1, 0.15, 0.14], (10, 5, 10)) + F32(0.002)
    b = _lattice([0.08, 0.05, 0.12], (8, 5, 8)) + F32(0.001)
    case = pack([a, b], [([0, 0, 0], [0.5, 0.5, 0.5]), ([0, 0, 0], [0.6, 0.4, 0.5])], [[ball, box], [cyl]])
    v = np.full(case["p"].shape, np.nan, F32)
    v[0, :500], v[1, :320] = [0.1, -1.5, 0.0], [2.5, 0.0, 0.4]
    assert case["lengths"].tolist() == [500, 320]
    for b, hits in ((0, (1, 2)), (1, (1,))):                                     # every obstacle holds particles at the start
        hit = run(case, b)[1]
        assert all(10 < int((hit & h).astype(bool).sum()) < 250 for h in hits), (b, np.bincount(hit))
    return case, v


CASES = {"ball": ball_case, "box": box_case, "cylinder": cylinder_case, "order": order_case, "wall": wall_case,
         "rotation": rotation_case, "skipped": skipped_case, "m0": m0_case, "m8": m8_case, "batch": batch_case}

"""A numpy statement of the isosurface rule of include/tpgan_ops.h ("isosurfaces"): marching tetrahedra on the Kuhn split
of every lattice cube, vectorised over nodes and cells.  The yardstick of csrc/isosurface.hip and of
`ops._iso_surface_torch`; written from the rule's text, with its own winding table from the integer recipe.

Everything that reaches a vertex or a normal is float32 with one rounding per operation (numpy never contracts)."""
import itertools

import numpy as np

F32 = np.float32
D = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)], dtype=np.int64)
PERMS = list(itertools.permutations(range(3)))        # xyz, xzy, yxz, yzx, zxy, zyx
MAX_NODES = 1 << 27


def tet_paths():
    """(6,4,3): the corner offsets v0..v3 of the six tetrahedra of a cube."""
    paths = np.zeros((6, 4, 3), dtype=np.int64)
    for p, perm in enumerate(PERMS):
        for s, axis in enumerate(perm):
            paths[p, s + 1] = paths[p, s]
            paths[p, s + 1, axis] += 1
    return paths


def _direction(offset):
    return int(np.nonzero((D == offset).all(1))[0][0])


def case_triangles(case):
    """The unwound triangles of one tetrahedron whose corner at path position a is inside iff bit a of `case` is set:
    a list of triangles, each three edges (lo, hi) of path positions."""
    ins = [a for a in range(4) if case >> a & 1]
    out = [a for a in range(4) if not case >> a & 1]
    edge = lambda a, b: (min(a, b), max(a, b))  # noqa: E731
    if len(ins) == 1 or len(out) == 1:
        s = (ins if len(ins) == 1 else out)[0]
        return [[edge(s, o) for o in range(4) if o != s]]
    if len(ins) == 2:
        (a, b), (c, d) = ins, out
        return [[edge(a, c), edge(a, d), edge(b, d)], [edge(a, c), edge(b, d), edge(b, c)]]
    return []


def winding_table():
    """table[p][case] = the list of WOUND triangles: exact integer arithmetic on edge midpoints in doubled lattice
    coordinates; a triangle (p, q, r) is kept when (q-p) x (r-p) . (sum of outside corners - sum of inside corners) > 0
    and has q and r exchanged otherwise.  -> (table, flip (6,16) bool)."""
    paths = tet_paths()
    table, flips = [], np.zeros((6, 16), dtype=bool)
    for p in range(6):
        row = []
        for case in range(16):
            tris = case_triangles(case)
            wound = []
            for tri in tris:
                mid = [paths[p, a] + paths[p, b] for a, b in tri]              # doubled coordinates: exact integers
                inside = sum(2 * paths[p, a] for a in range(4) if case >> a & 1)
                outside = sum(2 * paths[p, a] for a in range(4) if not case >> a & 1)
                s = int(np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), outside - inside))
                assert s != 0
                flips[p, case] = s < 0
                wound.append([tri[0], tri[2], tri[1]] if s < 0 else list(tri))
            row.append(wound)
        table.append(row)
    return table, flips


def gradient(f):
    """(nx,ny,nz,3): g_a = f[index_a + 1] - f[index_a - 1], indices clamped into the lattice."""
    g = np.zeros(f.shape + (3,), dtype=F32)
    for a in range(3):
        n = f.shape[a]
        hi = np.minimum(np.arange(n) + 1, n - 1)
        lo = np.maximum(np.arange(n) - 1, 0)
        with np.errstate(invalid="ignore"):
            g[..., a] = np.take(f, hi, axis=a) - np.take(f, lo, axis=a)
    return g


def iso_surface(field, origin, step, iso, normals=True):
    """-> (vertices (V,3) f32, faces (F,3) int32, normals (V,3) f32 or None) by the rule."""
    f = np.ascontiguousarray(field, dtype=F32)
    assert f.ndim == 3
    nx, ny, nz = f.shape
    origin = np.asarray(origin, dtype=F32).reshape(3)
    step, iso = F32(step), F32(iso)
    empty = (np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), np.zeros((0, 3), F32) if normals else None)
    if min(nx, ny, nz) < 2:
        return empty
    assert nx * ny * nz <= MAX_NODES
    with np.errstate(invalid="ignore"):
        inside = f >= iso                                                     # NaN: outside
    active = np.zeros((nx, ny, nz, 7), dtype=bool)
    for d, (dx, dy, dz) in enumerate(D):
        active[:nx - dx, :ny - dy, :nz - dz, d] = inside[:nx - dx, :ny - dy, :nz - dz] != inside[dx:, dy:, dz:]
    flat = active.reshape(-1)
    vid = np.cumsum(flat, dtype=np.int64) - flat                              # vertex number of edge 7 n + d
    keys = np.nonzero(flat)[0]
    node, d = keys // 7, keys % 7
    ia = np.stack(np.unravel_index(node, (nx, ny, nz)), 1)                    # (V,3)
    ib = ia + D[d]
    with np.errstate(all="ignore"):
        fa, fb = f[tuple(ia.T)], f[tuple(ib.T)]
        t = (iso - fa) / (fb - fa)
        pa = origin[None] + ia.astype(F32) * step
        pb = origin[None] + ib.astype(F32) * step
        vertices = pa + t[:, None] * (pb - pa)
        nrm = None
        if normals:
            g = gradient(f)
            ga, gb = g[tuple(ia.T)], g[tuple(ib.T)]
            gv = ga + t[:, None] * (gb - ga)
            length = np.sqrt((gv[:, 0] * gv[:, 0] + gv[:, 1] * gv[:, 1]) + gv[:, 2] * gv[:, 2])
            nrm = np.where((length == 0)[:, None], F32(0), -gv / length[:, None]).astype(F32)
    assert vertices.dtype == F32

    paths = tet_paths()
    table, _ = winding_table()
    vid3 = vid.reshape(nx, ny, nz, 7)
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    ci, cj, ck = np.meshgrid(np.arange(cx), np.arange(cy), np.arange(cz), indexing="ij")
    cell_id = (ci * ny + cj) * nz + ck
    faces, order = [], []
    for p in range(6):
        corner = [inside[paths[p, a, 0]:paths[p, a, 0] + cx, paths[p, a, 1]:paths[p, a, 1] + cy,
                         paths[p, a, 2]:paths[p, a, 2] + cz] for a in range(4)]
        case = sum(corner[a].astype(np.int64) << a for a in range(4))
        for c in range(1, 15):
            sel = case == c
            if not sel.any():
                continue
            si, sj, sk = ci[sel], cj[sel], ck[sel]
            for number, tri in enumerate(table[p][c]):
                cols = []
                for a, b in tri:
                    o = paths[p, a]
                    cols.append(vid3[si + o[0], sj + o[1], sk + o[2], _direction(paths[p, b] - paths[p, a])])
                faces.append(np.stack(cols, 1))
                order.append((cell_id[sel] * 6 + p) * 2 + number)
    if not faces:
        return vertices, np.zeros((0, 3), np.int32), nrm
    faces, order = np.concatenate(faces), np.concatenate(order)
    faces = faces[np.argsort(order, kind="stable")]
    assert faces.max() < vertices.shape[0] and faces.min() >= 0
    return vertices, faces.astype(np.int32), nrm


# ---- measurements of a mesh (float64) ----------------------------------------------------------------------------------
def volume(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float((np.cross(a, b) * c).sum() / 6.0)


def area(vertices, faces):
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.linalg.norm(np.cross(b - a, c - a), axis=1).sum() / 2.0)


def directed_edges(faces):
    f = np.asarray(faces, dtype=np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed_oriented(faces, n_vertices):
    """Every directed edge occurs once and its reverse occurs once."""
    e = directed_edges(faces)
    key = e[:, 0] * n_vertices + e[:, 1]
    rev = e[:, 1] * n_vertices + e[:, 0]
    uniq, counts = np.unique(key, return_counts=True)
    return bool((counts == 1).all()) and np.array_equal(uniq, np.unique(rev))


def euler_characteristic(faces, n_vertices):
    e = directed_edges(faces)
    und = np.unique(np.minimum(e[:, 0], e[:, 1]) * n_vertices + np.maximum(e[:, 0], e[:, 1]))
    used = np.unique(faces)
    return int(used.shape[0]) - int(und.shape[0]) + int(np.asarray(faces).shape[0])


def rotate_smallest_first(faces):
    """Each face rotated (cyclically: the orientation stays) so that its smallest index comes first."""
    f = np.asarray(faces)
    if f.shape[0] == 0:
        return f
    k = np.argmin(f, axis=1)
    idx = (k[:, None] + np.arange(3)[None]) % 3
    return np.take_along_axis(f, idx, axis=1)

"""The lattices and fields the isosurface kernels and the torch statement are compared on (tests/test_mesh_cpu.py,
tests/test_mesh_gpu.py).  The lattices are the smallest at which the kernels can go wrong: one cell; odd extents; a thin
slab that is long on the fastest axis; 80 850 nodes = 40 scan tiles of 2048, no multiple of any tile."""
import numpy as np

F32 = np.float32
SHAPES = [(2, 2, 2), (9, 7, 5), (3, 2, 64), (70, 33, 35)]
FIELDS = ["random", "planted", "outside", "shell", "single", "spheres"]
ISO = F32(0.25)
ORIGIN = np.array([-0.37, 0.11, 1.5], dtype=F32)
STEP = F32(0.0125)


def field(shape, kind, seed=0):
    """-> (nx,ny,nz) fp32.  All finite."""
    rng = np.random.default_rng(seed + 1000 * FIELDS.index(kind) + sum(shape))
    nx, ny, nz = shape
    if kind in ("random", "planted"):
        # uniform around iso: about half of the nodes inside, the densest output there is
        f = (ISO + rng.uniform(-1.0, 1.0, size=shape)).astype(F32)
        if kind == "planted":
            flat = f.reshape(-1)
            n = flat.shape[0]
            hit = rng.choice(n, size=max(1, n // 100), replace=False)
            flat[hit] = ISO                                                   # exactly iso: inside, t == 0 on their edges
            zero = rng.choice(n, size=max(2, n // 200), replace=False)
            flat[zero[::2]] = F32(0.0)
            flat[zero[1::2]] = F32(-0.0)
        return f
    if kind == "outside":
        return np.full(shape, ISO - F32(1.0), dtype=F32)
    if kind == "shell":                                                       # all inside except the boundary layer
        f = np.full(shape, ISO - F32(1.0), dtype=F32)
        f[1:-1, 1:-1, 1:-1] = ISO + F32(1.0)
        return f
    if kind == "single":
        f = np.zeros(shape, dtype=F32)
        f[nx // 2, ny // 2, nz // 2] = F32(1.0)
        return f
    if kind == "spheres":                                                     # two overlapping balls in unit coordinates
        u = [np.arange(n, dtype=np.float64) / (n - 1) for n in shape]
        X, Y, Z = np.meshgrid(*u, indexing="ij")
        a = 0.45 ** 2 - ((X - 0.25) ** 2 + (Y - 0.25) ** 2 + (Z - 0.25) ** 2)
        b = 0.45 ** 2 - ((X - 0.75) ** 2 + (Y - 0.75) ** 2 + (Z - 0.75) ** 2)
        return (np.maximum(a, b) + float(ISO)).astype(F32)
    raise ValueError(kind)


def is_empty(shape, kind):
    """Cases whose mesh is empty by construction; every other case must produce faces."""
    return kind == "outside" or (kind == "shell" and min(shape) < 3)


def lattice_ball(radius, spacing):
    """The points z * spacing of Z^3 with |z| <= radius (in spacings), shifted off the origin -> (N,3) fp32."""
    m = int(np.floor(radius))
    r = np.arange(-m, m + 1)
    Z = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    Z = Z[(Z * Z).sum(1) <= radius * radius]
    return (Z * float(spacing) + np.array([0.31, -0.12, 0.05])).astype(F32)

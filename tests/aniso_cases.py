"""The clouds the anisotropic kernels, their torch statements and the rule are compared on (tests/test_aniso_cpu.py,
tests/test_aniso_gpu.py).  The smallest at which the kernels can go wrong: the edges of the 64-candidate step, a full
neighbourhood (257), flat and thin clouds whose covariance is singular, coincident points, and two clusters far enough
apart for the grid's 64-cells-per-axis cap to set the cell size."""
import numpy as np

F32 = np.float32
SPACING = 0.025
SUPPORT = 2 * SPACING
RC = 2 * SUPPORT
S_MAX = 2.0
REACH = float(F32(S_MAX) * F32(SUPPORT))
CLOUDS = ["one", "pair", "random63", "random64", "random65", "random257", "sheet", "row", "coincident", "ball",
          "clusters"]


def lattice(shape, spacing=SPACING, origin=(0.0, 0.0, 0.0)):
    ax = [np.arange(n, dtype=np.float64) * spacing + o for n, o in zip(shape, origin)]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3).astype(F32)


def jittered(shape, amount, seed, spacing=SPACING):
    """A lattice with every coordinate moved uniformly by +- amount spacings."""
    rng = np.random.default_rng(seed)
    p = lattice(shape, spacing).astype(np.float64)
    return (p + rng.uniform(-amount, amount, size=p.shape) * spacing).astype(F32)


def ball(radius, spacing=SPACING, jitter=0.25, seed=21):
    """The lattice points within `radius` spacings, jittered: about 2 000 at 7.8."""
    m = int(np.floor(radius))
    r = np.arange(-m, m + 1)
    Z = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
    Z = Z[(Z * Z).sum(1) <= radius * radius].astype(np.float64)
    rng = np.random.default_rng(seed)
    return ((Z + rng.uniform(-jitter, jitter, size=Z.shape)) * spacing + np.array([0.31, -0.12, 0.05])).astype(F32)


def cloud(name):
    """-> (N,3) fp32, all finite."""
    rng = np.random.default_rng(100 + CLOUDS.index(name))
    if name == "one":
        return np.array([[0.3, -0.2, 0.1]], F32)
    if name == "pair":
        return np.array([[0.3, -0.2, 0.1], [0.32, -0.21, 0.13]], F32)
    if name.startswith("random"):
        n = int(name[6:])
        # dense enough that most neighbourhoods hold more than n_eps = 25 points: a box of about 1.5 rc
        return rng.uniform(0.0, 0.15, size=(n, 3)).astype(F32)
    if name == "sheet":
        return lattice((20, 20, 1))
    if name == "row":
        return lattice((40, 1, 1))
    if name == "coincident":
        return np.tile(np.array([[0.1, 0.2, -0.3]], F32), (30, 1))
    if name == "ball":
        return ball(7.8)
    if name == "clusters":
        # 100 reaches apart: the extent / 64 > reach > rc sets the cell edge, and each cluster falls into few cells
        a = rng.uniform(0.0, 0.12, size=(150, 3))
        return np.concatenate([a, a[::-1] * 0.9 + np.array([100 * REACH, 0.0, 0.0])]).astype(F32)
    raise ValueError(name)


def slab(layers, jitter, seed=7):
    """The 24 x 24 x layers slab of the ripple test."""
    return jittered((24, 24, layers), jitter, seed)

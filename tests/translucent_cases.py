"""The cases tests/test_translucent_cpu.py and tests/test_translucent_gpu.py share, with the rule's answer computed once
(tests/translucent_rule.py) and kept read-only."""
import functools

import numpy as np

import render_rule as R
import translucent_rule as T
from test_surface_gpu import MODES, SIZES, random_case as surface_case

F32 = np.float32
TH_MAX = 0.5                                                 # the absorb case's last level, world units
SIGMA = (6.0, 2.0, 0.5)                                      # and its absorption per world unit


def limit_image(args):
    """An opaque scene that cuts through the cloud: per frame a tilted plane's depth through the cloud's median depth,
    with a +inf block (nothing there) and one NaN pixel."""
    W, H, lengths = args["W"], args["H"], args["lengths"]
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    limit = np.empty((2, H, W), F32)
    for f in range(2):
        pts = args["points"][f, :lengths[f]]
        ok = np.isfinite(pts).all(-1) & (np.abs(pts) < 900).all(-1)
        t = R.project(pts[ok], args["cams"][f])[3]
        slope = 0.3 / max(W, H)
        limit[f] = (np.median(t) + slope * (xs - W / 2) * (1 - 2 * f) - 0.5 * slope * (ys - H / 2)).astype(F32)
    limit[0, : H // 3, : W // 4] = np.inf
    limit[1, H // 2:, 2 * W // 3:] = np.inf
    limit[0, H // 2, W // 2] = np.nan
    return limit


@functools.lru_cache(maxsize=None)
def random_case(mode, size):
    """test_surface_gpu.random_case's cloud (F = 2, 300 points, ragged, 30 duplicates, ten rows to drop, a camera per
    frame, discs of 3-6 pixels) with a limit image -> (arguments, limit, the rule's thickness with it, without it)."""
    args = surface_case(mode, size)[0]
    limit = limit_image(args)
    units, count = T.thickness_units(**args, limit=limit)
    free = T.thickness_units(**args)[0]
    assert (units > 0).mean() >= 0.10, "the case is vacuous"
    assert ((units < free) & (units > 0)).any() and ((units == 0) & (free > 0)).any(), "limit clips nothing"
    assert (units <= free).all() and count.max() >= 3, "no pixel sums three spheres"
    y, x = args["H"] // 2, args["W"] // 2
    assert units[0, y, x] == free[0, y, x] > 0, "the NaN pixel must leave the whole chord of some sphere"
    inf = np.isinf(limit)
    assert (units[inf] == free[inf]).all() and (free[inf] > 0).any()
    out = T.resolve(units), T.resolve(free)
    for a in (limit,) + out:
        a.setflags(write=False)
    return args, limit, out[0], out[1]


@functools.lru_cache(maxsize=None)
def absorb_case(W=37, H=23):
    """One picture holding every branch of the absorption rule -> a dict of the entry's arguments, the table included
    (computed as `ops.absorb_table` states it), with `branch`: masks by name.  Every branch occurs."""
    rng = np.random.default_rng(77)
    fluid = rng.integers(0, 256, (2, H, W, 3)).astype(np.uint8)
    behind = rng.integers(0, 256, (2, H, W, 3)).astype(np.uint8)
    fdepth = rng.uniform(0.5, 3.0, (2, H, W)).astype(F32)
    bdepth = (fdepth + rng.uniform(-0.4, 1.0, (2, H, W))).astype(F32)
    thickness = rng.uniform(0.0, 1.3 * TH_MAX, (2, H, W)).astype(F32)
    pick = rng.permutation(H * W)
    flat = lambda a: a.reshape(2, -1)                        # noqa: E731  (views)
    flat(fdepth)[:, pick[0:40]] = np.inf
    flat(fdepth)[0, pick[40:43]] = np.nan
    flat(fdepth)[1, pick[43:46]] = -np.inf
    flat(bdepth)[:, pick[46:86]] = flat(fdepth)[:, pick[46:86]]              # equality: the fluid wins
    flat(bdepth)[:, pick[86:200]] = np.inf
    flat(bdepth)[0, pick[200:203]] = np.nan                                  # no comparison holds: the fluid shows
    flat(bdepth)[:, pick[30:40]] = np.inf                                    # nothing at all: behind's colour, +inf
    flat(thickness)[:, pick[100:140]] = 0.0
    flat(thickness)[:, pick[140:160]] = TH_MAX
    flat(thickness)[0, pick[160:163]] = np.nan
    flat(thickness)[1, pick[163:166]] = -0.25
    flat(thickness)[1, pick[166:169]] = np.inf
    level = np.arange(256, dtype=np.float64).reshape(256, 1)
    table = np.exp(-np.asarray(SIGMA, np.float64).reshape(1, 3) * TH_MAX * level / 255.0).astype(F32)
    with np.errstate(invalid="ignore"):
        shows = np.isfinite(fdepth) & ~(bdepth < fdepth)
        branch = {"fdepth +inf": np.isposinf(fdepth), "bdepth < fdepth": np.isfinite(fdepth) & (bdepth < fdepth),
                  "bdepth == fdepth": shows & (bdepth == fdepth), "bdepth +inf": shows & np.isposinf(bdepth),
                  "thickness 0": shows & (thickness == 0), "thickness >= th_max": shows & (thickness >= TH_MAX),
                  "between": shows & (thickness > 0.1 * TH_MAX) & (thickness < 0.9 * TH_MAX)}
    for name, mask in branch.items():
        assert mask.sum() >= 3, name
    case = dict(fluid=fluid, fdepth=fdepth, thickness=thickness, behind=behind, bdepth=bdepth, table=table, th_max=TH_MAX)
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case, branch


__all__ = ["MODES", "SIZES", "random_case", "absorb_case", "limit_image", "TH_MAX", "SIGMA"]

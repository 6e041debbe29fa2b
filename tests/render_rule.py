"""The renderer's rule (include/tpgan_ops.h, "point-cloud pictures") stated in numpy, and the small hand-made cases both
test files share.  fp32 operations in the stated order, np.floor, a loop over the points in index order with an explicit
compare of the 64-bit keys: the rule has no order dependence and no tolerance, so whatever is compared with this
statement must be EQUAL to it, picture and winner map.
"""
import numpy as np

F32 = np.float32
EMPTY = 2 ** 64 - 1
ORTHO, PINHOLE = 0, 1


def cam_row(eye=(0, 0, 0), r=(1, 0, 0), d=(0, 1, 0), f=(0, 0, 1), scale=1.0, cx=0.0, cy=0.0, near=0.0, far=10.0,
            mode=ORTHO):
    return np.array([*eye, *r, *d, *f, scale, cx, cy, near, far, mode], dtype=F32)


def code_lut():
    """A table that spells the level out: lut[i] = (i, 255 - i, i ^ 0x55)."""
    i = np.arange(256)
    return np.stack([i, 255 - i, i ^ 0x55], 1).astype(np.uint8)


def project(p, c):
    """p (n,3) fp32, c (18,) fp32 -> u, v, zv, t, keep: every operation an fp32 operation, in the stated order."""
    with np.errstate(all="ignore"):
        q = p - c[0:3]

        def dot(b):
            return (q[:, 0] * b[0] + q[:, 1] * b[1]) + q[:, 2] * b[2]
        xv, yv, zv = dot(c[3:6]), dot(c[6:9]), dot(c[9:12])
        if c[17] != 0:
            u, v = (xv / zv) * c[12] + c[13], (yv / zv) * c[12] + c[14]
        else:
            u, v = xv * c[12] + c[13], yv * c[12] + c[14]
        t = zv - c[15]
    assert all(a.dtype == F32 for a in (u, v, zv, t))
    return u, v, zv, t


def render_rule(points, cams, W, H, size, lut, background, lengths=None, scalar=None, lo=0.0, hi=None):
    """-> (image (F,H,W,3) uint8, winner (F,H,W) int32)."""
    points = np.asarray(points, dtype=F32)
    F, N, _ = points.shape
    cams = np.asarray(cams, dtype=F32).reshape(-1, 18)
    S = int(size)
    hi = F32(cams[0, 16]) - F32(cams[0, 15]) if hi is None else hi
    lo32 = F32(lo)
    inv = F32(255.0) / (F32(hi) - lo32)
    image = np.empty((F, H, W, 3), np.uint8)
    winner = np.full((F, H, W), -1, np.int32)
    for f in range(F):
        c = cams[f if len(cams) > 1 else 0]
        n = N if lengths is None else min(max(int(lengths[f]), 0), N)
        u, v, zv, t = project(points[f, :n], c)
        with np.errstate(invalid="ignore"):
            keep = ((t >= 0) & (zv <= c[16]) & (u >= F32(-S)) & (u < F32(W + S)) & (v >= F32(-S)) & (v < F32(H + S)))
        bits = t.view(np.uint32)
        keys = [[EMPTY] * W for _ in range(H)]
        for i in range(n):
            if not keep[i]:
                continue
            px, py = int(np.floor(u[i])), int(np.floor(v[i]))
            key = (int(bits[i]) << 32) | i
            for y in range(max(py - S // 2, 0), min(py - S // 2 + S, H)):
                row = keys[y]
                for x in range(max(px - S // 2, 0), min(px - S // 2 + S, W)):
                    if key < row[x]:
                        row[x] = key
        for y in range(H):
            for x in range(W):
                key = keys[y][x]
                if key == EMPTY:
                    image[f, y, x] = background
                    continue
                i = key & 0xFFFFFFFF
                s = F32(scalar[f][i]) if scalar is not None else np.uint32(key >> 32).view(F32)
                with np.errstate(all="ignore"):
                    cval = (s - lo32) * inv
                    level = 0
                    if cval > 0:
                        level = 255 if cval >= 255 else int(cval + F32(0.5))
                image[f, y, x] = lut[level]
                winner[f, y, x] = i
    return image, winner


# ---------------------------------------------------------------------------------------------------------------------
# Hand-made cases on a 16 x 16 picture under the identity camera (u = x, v = y, t = z).  Each is a dict of the arguments
# of `render_rule` plus `expect`: a function of (image, winner) that asserts what the issue states in words.
W16 = H16 = 16
BG = (9, 8, 7)


def _case(points, size, expect, **kw):
    pts = np.asarray(points, dtype=F32)
    pts = pts[None] if pts.ndim == 2 else pts
    return dict(points=pts, cams=kw.pop("cams", cam_row()), W=W16, H=H16, size=size, lut=code_lut(), background=BG,
                expect=expect, **kw)


def _covered(winner, frame=0):
    ys, xs = np.nonzero(winner[frame] >= 0)
    return sorted(zip(xs.tolist(), ys.tolist()))


def _block(x0, x1, y0, y1):
    return sorted((x, y) for x in range(x0, x1 + 1) for y in range(y0, y1 + 1))


def small_cases():
    cases = {}
    # one point at u = 5.5, v = 7.5: px = 5, py = 7; size S covers px - S/2 .. px - S/2 + S - 1
    for S, (x0, x1, y0, y1) in {1: (5, 5, 7, 7), 3: (4, 6, 6, 8), 4: (3, 6, 5, 8)}.items():
        def expect(image, winner, box=(x0, x1, y0, y1)):
            assert _covered(winner) == _block(*box)
            assert (winner[0][winner[0] >= 0] == 0).all()
            assert (image[0][winner[0] < 0] == BG).all()
        cases[f"one_point_size{S}"] = _case([[5.5, 7.5, 1.0]], S, expect)

    # corners and just outside, S = 3, two frames: frame 0 holds the points, frame 1 stays empty
    def corner(image, winner):
        # u = v = -0.5: px = py = -1 -> columns -2..0: pixel (0,0) only.  u = W + S - 0.01 -> px = W + 2: nothing inside.
        assert _covered(winner, 0) == [(0, 0), (14, 14), (14, 15), (15, 14), (15, 15)]
        assert winner[0, 0, 0] == 0 and winner[0, 15, 15] == 3
        assert (winner[1] == -1).all() and (image[1] == BG).all()
    far_out = F32(W16 + 3) - F32(0.01)
    cases["corner_and_outside"] = _case(
        [[[-0.5, -0.5, 1.0], [far_out, 8.0, 1.0], [W16 + 3, 8.0, 1.0], [15.5, 15.5, 1.0], [8.0, H16 + 3, 1.0]],
         [[-9.0, -9.0, 1.0]] * 5], 3, corner)

    # occlusion: the nearer wins in both index orders; equal depth: the lower index
    def nearer(index):
        def expect(image, winner):
            assert winner[0, 4, 4] == index and _covered(winner) == [(4, 4)]
        return expect
    cases["occlusion_near_first"] = _case([[4.2, 4.2, 1.0], [4.7, 4.1, 2.0]], 1, nearer(0))
    cases["occlusion_near_last"] = _case([[4.2, 4.2, 2.0], [4.7, 4.1, 1.0]], 1, nearer(1))
    cases["occlusion_equal_depth"] = _case([[4.2, 4.2, 1.5], [4.7, 4.1, 1.5], [4.0, 4.9, 1.5]], 1, nearer(0))

    # culling: only the valid point (index 3) draws, and it keeps its pixel whatever shares it
    nan, inf = np.nan, np.inf
    just_below = np.nextafter(F32(0.5), F32(0))          # t = zv - near just below 0 with near = 0.5
    just_above = np.nextafter(F32(10), F32(20))          # zv just above far = 10

    def only_valid(image, winner):
        assert _covered(winner) == _block(5, 7, 5, 7) and (winner[0][winner[0] >= 0] == 3).all()
    culled = [[6.5, 6.5, just_below], [6.5, 6.5, just_above], [6.5, 6.5, nan], [6.5, 6.5, 5.0], [nan, 6.5, 1.0],
              [6.5, inf, 1.0], [-inf, 6.5, 1.0], [6.5, 6.5, inf], [6.5, 6.5, -inf], [999.0, 999.0, 999.0], [6.5, nan, 0.6],
              [6.5, 6.5, 0.7], [6.5, 6.5, 0.8]]
    # rows 11, 12 are nearer than the valid point but lie at or beyond lengths[0] = 11
    cases["culling"] = _case(culled, 3, only_valid, cams=cam_row(near=0.5), lengths=[11])
    beyond = [[6.5, 6.5, 5.0]] + [[nan, nan, nan]] * 3 + [[3e38, -3e38, 3e38]] * 3 + [[6.5, 6.5, 1.0]]

    def first_only(image, winner):
        assert _covered(winner) == [(6, 6)] and winner[0, 6, 6] == 0
    cases["beyond_length"] = _case(beyond, 1, first_only, lengths=[1])

    # colour: lo = 0, hi = 255 -> inv = 1 and c = s; one point per pixel of row 2
    values = [0.0, 0.49, 0.5, 254.5, 255.0, 300.0, nan, -3.0, 17.0]
    levels = [0, 0, 1, 255, 255, 255, 0, 0, 17]

    def colour(image, winner):
        lut = code_lut()
        for i, level in enumerate(levels):
            assert winner[0, 2, i] == i and (image[0, 2, i] == lut[level]).all(), (i, level, image[0, 2, i])
        assert (image[0][winner[0] < 0] == BG).all() and (winner[0] >= 0).sum() == len(levels)
    cases["colour"] = _case([[i + 0.5, 2.5, 1.0] for i in range(len(values))], 1, colour,
                            scalar=np.array([values], dtype=F32), lo=0.0, hi=255.0)
    return cases


def random_cloud(rng, F, N, spread=0.5):
    return (rng.normal(size=(F, N, 3)) * spread).astype(F32)


def tilted_cam(W, H, mode, eye=(1.1, -0.7, 2.9), target=(0.05, -0.02, 0.1), scale=None):
    """A camera that is not axis-aligned, rows orthonormal in float64 and rounded to fp32 once."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, [0.0, 1.0, 0.0])
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    dist = np.linalg.norm(target - eye)
    px = 0.3 * min(W, H) if scale is None else scale
    return cam_row(eye, r, d, f, px * dist if mode == PINHOLE else px, W / 2, H / 2, 0.25 * dist, 1.6 * dist, mode)

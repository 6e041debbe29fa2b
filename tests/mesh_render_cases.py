"""The mesh renderer's cases, shared by tests/test_mesh_render_cpu.py (the torch statement on CPU tensors) and
tests/test_mesh_render_gpu.py (the kernels): each is a dict of the arguments of `mesh_render_rule.raster_rule`, with the
rule's answer computed once per process and left read-only.  Hand-made cases live under the identity camera (u = x,
v = y, t = z), so a vertex at (a + 0.25, ..) snaps to 256 a + 64 and box edges can be placed exactly.
"""
import functools

import numpy as np

import mesh_render_rule as MR
import render_rule as R

F32 = np.float32
MODES = {"ortho": R.ORTHO, "pinhole": R.PINHOLE}
SIZES = {"37x23": (37, 23), "70x50": (70, 50)}      # smaller than and no multiple of a 32 x 8 tile; several tiles
SMALL = 16                                           # TPG_MESH_SMALL: the kernel's class edge
HUGE, LIST = 2048, 256                               # TPG_MESH_HUGE, TPG_MESH_LIST: the tile launch's class edge and list
WIDTHS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _torus(nu=20, nv=10, R_=0.75, r=0.35):
    from tpgan_amd import mesh
    return mesh.make_torus(R_, r, nu, nv)


def _icosphere(n=2):
    from tpgan_amd import mesh
    return mesh.make_icosphere(n)


@functools.lru_cache(maxsize=None)
def random_case(mode, size):
    """F = 2, M = F: an icosphere(2) and a torus, ragged, one camera per frame, 30 duplicated faces, faces with bad
    indices and faces on bad vertices -> (arguments, depth, winner, extras = normals, scalar, the duplicated faces)."""
    W, H = SIZES[size]
    rng = np.random.default_rng(100 * MODES[mode] + W)
    px = 0.42 * min(W, H)
    cams = np.stack([R.tilted_cam(W, H, MODES[mode], scale=px),
                     R.tilted_cam(W, H, MODES[mode], eye=(-2.0, 0.4, 1.5), scale=px)])
    target = np.array([0.05, -0.02, 0.1])
    meshes = [_icosphere(2), _torus()]
    V, T = 230, 480
    vertices = np.full((2, V, 3), np.nan, F32)
    faces = np.zeros((2, T, 3), np.int32)
    vlengths, flengths, dup = [], [], None
    for m, (v, f) in enumerate(meshes):
        c = cams[m].astype(np.float64)
        eye, r_, fw = c[0:3], c[3:6], c[9:12]
        bad = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], eye + fw * c[15] * 0.5, eye + fw * c[16] * 1.5,
                        eye + fw * 3.0 + r_ * 1e6, [np.nan] * 3])                    # 7 vertices that drop their faces
        nv, nf = len(v), len(f)
        vertices[m, :nv] = v + target
        vertices[m, nv:nv + 7] = bad
        vlen = nv + 7
        faces[m, :nf] = f
        extra = [[0, 1, nv + k] for k in range(7)] + [[-1, 0, 1], [0, vlen, 1], [0, 1, V - 1], [2 ** 31 - 1, 0, 1],
                                                      [-2 ** 31, 1, 2], [5, 5, 9], [7, 8, 7]]
        faces[m, nf:nf + len(extra)] = extra
        n = nf + len(extra)
        if m == 0:                                               # 30 faces that are seen, once more at the end
            _, win = MR.raster_rule(vertices[:1], faces[:1], cams[0], W, H, vlengths=[vlen], flengths=[n])
            dup = np.unique(win[win >= 0])[:30]
            assert len(dup) == 30
            faces[m, n:n + 30] = faces[m, dup]
            n += 30
        # what lies beyond the lengths would be seen if it were read: a triangle across the picture, in front
        vertices[m, vlen:vlen + 3] = [eye + fw * c[15] * 1.1 + r_ * a + c[6:9] * b for a, b in ((-9, -9), (9, -9), (0, 9))]
        faces[m, n:] = [vlen, vlen + 1, vlen + 2]
        vlengths.append(vlen)
        flengths.append(n)
    args = dict(vertices=vertices, faces=faces, cams=cams, W=W, H=H, vlengths=vlengths, flengths=flengths)
    depth, winner = MR.raster_rule(**args)
    surface = np.isfinite(depth).mean()
    assert surface >= 0.10 and np.isinf(depth).any(), "the case is vacuous"
    assert np.isin(dup, winner[0]).all() and winner[0].max() < flengths[0] - 30, "duplicates: the lower index shows"
    for m in range(2):                                           # only faces of the two solids are seen
        assert winner[m].max() < len(meshes[m][1])
    normals = np.nan_to_num(vertices - target.astype(F32), nan=0.0, posinf=0.0, neginf=0.0).astype(F32)
    normals /= np.maximum(np.linalg.norm(normals, axis=-1, keepdims=True), F32(1e-6))
    scalar = rng.normal(size=(2, V)).astype(F32)
    scalar[1, 3] = np.nan
    _frozen(vertices, faces, cams, depth, winner, normals, scalar)
    return args, depth, winner, dict(normals=normals, scalar=scalar, dup=dup)


def _identity(W, H, far=100.0):
    return R.cam_row(far=far)


def box_triangle(a, c, w, h, z=(5.0, 6.0, 7.0)):
    """A right triangle whose candidate box is columns a .. a+w-1, rows c .. c+h-1 (before clipping)."""
    b, d = a + w - 1, c + h - 1
    return [[a + 0.25, c + 0.25, z[0]], [b + 0.75, c + 0.25, z[1]], [a + 0.25, d + 0.75, z[2]]]


def _soup(triangles, W, H, **kw):
    """Triangles as (n,3,3) corner lists -> the arguments of one mesh under the identity camera."""
    tri = np.asarray(triangles, F32).reshape(-1, 3, 3)
    return dict(vertices=tri.reshape(1, -1, 3), faces=np.arange(3 * len(tri), dtype=np.int32).reshape(1, -1, 3),
                cams=_identity(W, H), W=W, H=H, **kw)


def _boxes(args):
    s = MR.Setup(args["vertices"][0], args["faces"][0], np.asarray(args["cams"], F32).reshape(-1, 18)[0], args["W"],
                 args["H"], args["vertices"].shape[1], args["faces"].shape[1])
    return s.box


def edge_cases():
    """name -> arguments; every box size the name promises is asserted from the rule's snapped boxes here."""
    cases = {}
    for w, h in ((4, 4), (16, 1), (1, 16), (17, 1), (1, 17), (2, 8), (3, 6)):
        args = _soup([box_triangle(3, 2, w, h), box_triangle(2, 1, 2, 2, (9.0, 9.0, 9.0))], 37, 23)
        assert MR.box_pixels(_boxes(args)).tolist() == [w * h, 4] and w * h in (SMALL, SMALL + 1, SMALL + 2)
        cases[f"box_{w}x{h}_{'small' if w * h <= SMALL else 'large'}"] = args
    for w in WIDTHS:                                             # the wave's lane layouts: 20 rows, so never small
        W, H = SIZES["37x23"] if w <= 33 else SIZES["70x50"]
        args = _soup([box_triangle(2, 1, w, 20), box_triangle(1, 3, min(w, 30), 18, (6.0, 5.0, 4.0))], W, H)
        box = _boxes(args)
        assert box[0].tolist() == [2, w + 1, 1, 20] and MR.box_pixels(box)[0] == 20 * w > SMALL
        cases[f"width_{w}"] = args
    args = _soup([box_triangle(30, 0, 5, 22)], 37, 23)
    assert _boxes(args)[0].tolist() == [30, 34, 0, 21]
    cases["taller_than_wide"] = args
    for (W, H) in SIZES.values():                                # a quad beyond the picture on all four sides
        q = [[-10.0, -12.0, 2.0], [W + 11.0, -12.0, 3.0], [W + 11.0, H + 9.0, 4.0], [-10.0, H + 9.0, 5.0]]
        args = _soup([[q[0], q[1], q[2]], [q[0], q[2], q[3]]], W, H)
        assert (_boxes(args) == [0, W - 1, 0, H - 1]).all()
        cases[f"quad_{W}x{H}"] = args
    # 40 x 30 cells of 0.37 pixels, two triangles each: most cover no pixel centre
    g = 0.37
    xs, ys = np.meshgrid(3.1 + g * np.arange(41), 2.2 + g * np.arange(31), indexing="ij")
    zs = 3.0 + 0.01 * xs + 0.02 * ys
    P = np.stack([xs, ys, zs], -1)
    tris = [[P[i, j], P[i + 1, j], P[i + 1, j + 1]] for i in range(40) for j in range(30)]
    tris += [[P[i, j], P[i + 1, j + 1], P[i, j + 1]] for i in range(40) for j in range(30)]
    cases["subpixel_grid"] = _soup(tris, 37, 23)
    # the tile launch: a box of exactly HUGE pixels is still a wave's, one of more goes on the frame's list
    for w, h in ((64, 32), (65, 32), (32, 48), (66, 46)):
        args = _soup([box_triangle(2, 1, w, h), box_triangle(1, 3, 40, 30, (6.0, 5.0, 4.0))], 70, 50)
        assert MR.box_pixels(_boxes(args)).tolist() == [w * h, 1200] and (w * h > HUGE) == ((w, h) in ((65, 32), (66, 46)))
        cases[f"box_{w}x{h}_{'huge' if w * h > HUGE else 'large'}"] = args
    assert 70 * 50 > HUGE                                        # quad_70x50 above is a pair of huge faces cut by every tile edge
    rng = np.random.default_rng(6)                               # more huge faces than a list holds: the rest go to the waves
    tris = [box_triangle(int(rng.integers(0, 3)), int(rng.integers(0, 3)), 66, 46, rng.uniform(2, 9, 3)) for _ in range(LIST + 4)]
    args = _soup(tris, 70, 50)
    assert (MR.box_pixels(_boxes(args)) > HUGE).all() and len(_boxes(args)) == LIST + 4
    cases["huge_faces_overflow"] = args
    # two frames of one mesh under two cameras: huge in the first, pushed half out of the second (a list per frame)
    args = _soup([box_triangle(2, 1, 66, 46), box_triangle(5, 5, 6, 4, (3.0, 3.0, 3.0))], 70, 50)
    args["cams"] = np.stack([R.cam_row(far=100.0), R.cam_row(far=100.0, cx=40.0, cy=-20.0)])
    cases["huge_in_one_frame_of_two"] = args
    rng = np.random.default_rng(5)
    for n in (65, 129):                                          # a wave's ballot full, then one face in the next wave
        tris = [box_triangle(int(rng.integers(0, 30)), int(rng.integers(0, 18)), 6, 4, rng.uniform(2, 9, 3)) for _ in range(n)]
        args = _soup(tris, 37, 23)
        assert (MR.box_pixels(_boxes(args)) > SMALL).all() and len(_boxes(args)) == n
        cases[f"large_faces_{n}"] = args
    return cases


@functools.lru_cache(maxsize=None)
def edge_case_answers():
    """name -> (arguments, depth, winner), the rule's answer computed once."""
    out = {}
    for name, args in edge_cases().items():
        depth, winner = MR.raster_rule(**args)
        assert (winner >= 0).any(), name
        out[name] = (args,) + _frozen(depth, winner)
    sub = out["subpixel_grid"]
    seen = np.unique(sub[2][sub[2] >= 0])
    assert 0 < len(seen) < 0.5 * sub[0]["faces"].shape[1], "most sub-pixel triangles cover no pixel centre"
    return out


EDGE_NAMES = sorted(edge_cases())


def planar_fan(n=7, centre=(8.5, 7.5), radius=5.0):
    """A closed fan of n triangles around a vertex that IS a pixel centre, rim vertices on the 1/256 grid."""
    ang = 2 * np.pi * (np.arange(n) + 0.3) / n
    rim = np.round((np.stack([np.cos(ang), np.sin(ang)], 1) * radius + centre) * 256) / 256
    tris = [[[*centre, 2.0], [*rim[i], 2.0], [*rim[(i + 1) % n], 2.0]] for i in range(n)]
    return _soup(tris, 18, 16)


def planar_grid():
    """4 x 3 cells of 2 x 2 pixels with their corners ON pixel centres, split along alternating diagonals: centres fall on
    shared vertices, on horizontal, vertical and diagonal shared edges."""
    tris = []
    for i in range(4):
        for j in range(3):
            x0, y0, x1, y1 = 2.5 + 2 * i, 1.5 + 2 * j, 4.5 + 2 * i, 3.5 + 2 * j
            a, b, c, d = [x0, y0, 3.0], [x1, y0, 3.0], [x1, y1, 3.0], [x0, y1, 3.0]
            tris += [[a, b, c], [a, c, d]] if (i + j) % 2 == 0 else [[a, b, d], [b, c, d]]
    return _soup(tris, 14, 10)

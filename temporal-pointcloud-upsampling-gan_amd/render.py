"""Pictures of point clouds on the GPU: cameras, colours, PNG files.

    python -m tpgan_amd.render --frames 'bunny_demo/pcd_{i}.npy' --count 800 --out PNGDIR
        [--size 3 --width 768 --height 768 --mode pinhole --color depth|density|free_surface
         --cutoff 0.0775 --direction x y z --frames_per_call T
         --style points|surface|surface_mesh --particle_radius 0.025 --smooth_iters 3 --smooth_half_width 2
         --solids obstacles.ply|icosphere:2 --solids_color 150 150 150
         --translucent --absorption 0.2 0.07 0.03 --thickness_iters 2]

The reference looks at its results through an Open3D window (train_utils.py:224-238) and hands its demo frames to an
external renderer; neither works on a display-less GPU node.  Here a picture is one op, `ops.render_points`
(csrc/render.hip): a z-buffered square splat, many frames per call, the same bits on every run.  This file is the thin
layer above it: `Camera` (host maths in float64, rounded to fp32 once), the colour of a point (its depth, or the
density / free surface / speed the project already computes on the device), a closed-form colour ramp and a PNG writer
on the standard library.  `--style surface` draws the fluid's surface instead of its particles, `ops.render_surface`
(csrc/surface.hip): spheres, a depth image smoothed within silhouettes, normals, shading -- what the reference leaves to
an external renderer; `--translucent` adds the technique's second half, a thickness image (`ops.render_thickness`) and a
Beer-Lambert composite over what lies behind the fluid (`ops.absorb_layers`).  Triangle meshes -- the surface
`mesh.surface_mesh` builds (`--style surface_mesh`), the solids of a simulated scene (`--solids`), any .obj / .ply file
-- are drawn by `ops.render_mesh` (csrc/mesh_render.hip) and composed with the
fluid by depth, `ops.compose_layers`.  The look is this project's own: no parity with Open3D's or any renderer's picture
is claimed.
"""
import argparse
import os
import struct
import zlib

import numpy as np
import torch

from . import analysis, ops

PADDING = 900.0                # rows with any |coordinate| >= this are the 999 padding of hard masking, not points
FRAMES_PER_CALL = 16
MODES = {"ortho": ops.RENDER_ORTHO, "pinhole": ops.RENDER_PINHOLE}
STYLES = ("points", "surface", "surface_mesh")
SOLIDS_COLOR = (150, 150, 150)
# --translucent: absorption per particle diameter (red, green, blue).  Red goes first, as in water: one diameter still
# transmits 0.82 / 0.93 / 0.97, twenty diameters 0.018 / 0.25 / 0.55.
ABSORPTION = (0.20, 0.07, 0.03)
THICKNESS_DIAMETERS = 40.0     # the absorption table's last level: this many particle diameters of fluid


def _unit(v, what):
    v = np.asarray(v, dtype=np.float64).reshape(3)
    n = np.linalg.norm(v)
    if not np.isfinite(n) or n == 0.0:
        raise ValueError(f"{what} must be a finite non-zero vector")
    return v / n


def _frame(direction, up):
    """-> rows r, d, f (image-right, image-DOWN, forward), orthonormal, float64."""
    f = _unit(direction, "direction")
    r = np.cross(f, np.asarray(up, dtype=np.float64).reshape(3))
    if np.linalg.norm(r) < 1e-9:
        raise ValueError("up must not be parallel to the viewing direction")
    r = _unit(r, "up")
    return r, np.cross(f, r), f


class Camera:
    """eye, the rows r / d / f, mode, scale, cx, cy, near, far (the 18 floats of include/tpgan_ops.h) and the picture's
    width and height.  Everything is kept in float64; `row()` rounds to fp32 once."""

    def __init__(self, eye, r, d, f, mode, scale, cx, cy, near, far, width, height):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {sorted(MODES)}")
        self.eye, self.r, self.d, self.f = (np.asarray(a, dtype=np.float64).reshape(3) for a in (eye, r, d, f))
        self.mode, self.scale, self.cx, self.cy = mode, float(scale), float(cx), float(cy)
        self.near, self.far, self.width, self.height = float(near), float(far), int(width), int(height)
        if mode == "pinhole" and not self.near > 0:
            raise ValueError("a pinhole camera needs near > 0")
        if not self.far > self.near:
            raise ValueError("far must exceed near")

    def row(self):
        return np.concatenate([self.eye, self.r, self.d, self.f,
                               [self.scale, self.cx, self.cy, self.near, self.far, MODES[self.mode]]]).astype(np.float32)

    def project(self, points):
        """(N,3) -> (u, v, t) float64 with the fp32-rounded camera: where the kernel puts the points, up to its rounding."""
        c = self.row().astype(np.float64)
        q = np.asarray(points, dtype=np.float64).reshape(-1, 3) - c[0:3]
        xv, yv, zv = q @ c[3:6], q @ c[6:9], q @ c[9:12]
        if self.mode == "pinhole":
            xv, yv = xv / zv, yv / zv
        return xv * c[12] + c[13], yv * c[12] + c[14], zv - c[15]

    @classmethod
    def look_at(cls, eye, target, up=(0.0, 1.0, 0.0), mode="pinhole", width=768, height=768, scale=None, near=None,
                far=None):
        """A camera at `eye` looking at `target`, which lands on the picture's centre.  scale: pixels per unit length in
        the plane through the target, the same in both modes (default: that plane's unit square fills the smaller
        picture edge); near / far default to 0.01 x / 2 x the distance to the target."""
        eye, target = np.asarray(eye, dtype=np.float64).reshape(3), np.asarray(target, dtype=np.float64).reshape(3)
        dist = float(np.linalg.norm(target - eye))
        r, d, f = _frame(target - eye, up)
        scale = float(min(width, height)) if scale is None else float(scale)
        return cls(eye, r, d, f, mode, scale * dist if mode == "pinhole" else scale, width / 2.0, height / 2.0,
                   0.01 * dist if near is None else near, 2.0 * dist if far is None else far, width, height)

    @classmethod
    def fit(cls, points, lengths=None, direction=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), mode="pinhole", width=768,
            height=768, margin=0.05):
        """A camera that looks along `direction` and holds the bounding box of the valid rows of one cloud (N,3), a batch
        (F,N,3) with optional lengths (F,), or a list of clouds: every valid point lands at least margin x the half
        extent away from the picture's edges, and near .. far is the box's depth range.  Rows that are not finite, or
        have any |coordinate| >= 900 (the 999 padding of hard masking), are ignored."""
        if not 0.0 <= margin < 1.0:
            raise ValueError("margin must be in [0, 1)")
        lo, hi = bounding_box(points, lengths)
        centre, radius = (lo + hi) / 2.0, float(np.linalg.norm(hi - lo)) / 2.0
        radius = radius if radius > 0 else 1.0
        r, d, f = _frame(direction, up)
        dist = 3.0 * radius
        eye = centre - dist * f
        corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])]) - eye
        xv, yv, zv = corners @ r, corners @ d, corners @ f
        near, far = float(zv.min()) - 0.01 * radius, float(zv.max()) + 0.01 * radius
        if mode == "pinhole":
            xv, yv = xv / zv, yv / zv                       # zv >= dist - radius > 0
        ext_x, ext_y = max(float(np.abs(xv).max()), 1e-12), max(float(np.abs(yv).max()), 1e-12)
        scale = (1.0 - margin) * min(width / 2.0 / ext_x, height / 2.0 / ext_y)
        return cls(eye, r, d, f, mode, scale, width / 2.0, height / 2.0, near, far, width, height)


def bounding_box(points, lengths=None):
    """(lo (3,), hi (3,)) float64 of the valid rows (finite, every |coordinate| < 900, below the frame's length) of a
    cloud, a batch or a list of clouds; the reduction runs where the points live."""
    if isinstance(points, (list, tuple)):
        if lengths is not None:
            raise ValueError("lengths go with one (F,N,3) batch, not with a list of clouds")
        boxes = [bounding_box(p) for p in points]
        return np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)
    p = torch.as_tensor(points).detach().float()
    p = p.reshape(1, -1, 3) if p.dim() == 2 else p
    if p.dim() != 3 or p.shape[2] != 3:
        raise ValueError("points must be (N,3) or (F,N,3)")
    valid = torch.isfinite(p).all(-1) & (p.abs() < PADDING).all(-1)
    if lengths is not None:
        n = torch.as_tensor(lengths, device=p.device).view(-1, 1)
        valid &= torch.arange(p.shape[1], device=p.device).view(1, -1) < n
    if not bool(valid.any()):
        raise ValueError("no valid point to fit a camera to")
    v = valid.unsqueeze(-1)
    lo = torch.where(v, p, torch.full_like(p, float("inf"))).amin((0, 1))
    hi = torch.where(v, p, torch.full_like(p, float("-inf"))).amax((0, 1))
    return lo.double().cpu().numpy(), hi.double().cpu().numpy()


def default_lut():
    """(256,3) uint8: blue - cyan - green - yellow - red, each channel the closed form clamp(1.5 - |4x - k|, 0, 1) with
    k = 3, 2, 1 for red, green, blue and x = level / 255."""
    x = np.arange(256, dtype=np.float64) / 255.0
    rgb = np.stack([np.clip(1.5 - np.abs(4.0 * x - k), 0.0, 1.0) for k in (3.0, 2.0, 1.0)], axis=1)
    return np.floor(rgb * 255.0 + 0.5).astype(np.uint8)


def _finite_range(s, lengths):
    """(min, max) of the finite values of the valid rows of s (F,N); (0, 1) if there is none."""
    ok = torch.isfinite(s)
    if lengths is not None:
        ok &= torch.arange(s.shape[1], device=s.device).view(1, -1) < torch.as_tensor(lengths, device=s.device).view(-1, 1)
    if not bool(ok.any()):
        return 0.0, 1.0
    return float(s[ok].min()), float(s[ok].max())


def point_scalar(points, color, lengths=None, cutoff=None, radius=analysis.BASE_RADIUS, velocity=None):
    """The per-point value (F,N) fp32 behind a named colour: "density" (`analysis.particle_density_batch` within
    `cutoff`), "free_surface" (1 on the free surface of `analysis.free_surface_mask` at `radius`, else 0) or "speed"
    (|velocity|, velocity (F,N,3))."""
    F, N, _ = points.shape
    if color == "density":
        if cutoff is None:
            raise ValueError('color="density" needs a cutoff')
        return analysis.particle_density_batch(points, cutoff, lengths)
    if color == "free_surface":
        num = analysis.neighbor_num_batch(points, radius, lengths)
        lens = [N] * F if lengths is None else [int(v) for v in torch.as_tensor(lengths).tolist()]
        out = torch.zeros((F, N), dtype=torch.float32, device=points.device)
        for t in range(F):
            out[t, :lens[t]] = analysis.free_surface_mask(num[t, :lens[t]]).float()
        return out
    if color == "speed":
        if velocity is None or tuple(velocity.shape) != (F, N, 3):
            raise ValueError(f'color="speed" needs velocity of shape {(F, N, 3)}')
        v = velocity.to(points.device).float()
        return torch.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]).contiguous()
    raise ValueError(f"unknown color {color!r}")


def _prepare(points, camera, color, lengths, lo, hi, cutoff, radius, velocity):
    """What `render` and `render_surface` do with their common arguments -> (single, points (F,N,3) fp32, cameras,
    scalar (F,N) or None, lo, hi)."""
    single = points.dim() == 2
    pts = points.detach().float().contiguous()
    pts = pts.unsqueeze(0) if single else pts
    cams = [camera] if isinstance(camera, Camera) else list(camera)
    if any((c.width, c.height) != (cams[0].width, cams[0].height) for c in cams):
        raise ValueError("the cameras of one call share the picture's size")
    scalar = None
    if color is not None and not (isinstance(color, str) and color == "depth"):
        if isinstance(color, str):
            scalar = point_scalar(pts, color, lengths, cutoff, radius,
                                  None if velocity is None else velocity.reshape(pts.shape))
            if color == "free_surface":
                lo, hi = 0.0 if lo is None else lo, 1.0 if hi is None else hi
        else:
            scalar = color.detach().to(pts.device).float().reshape(pts.shape[:2])
        scalar = scalar.contiguous()
        if lo is None or hi is None:
            a, b = _finite_range(scalar, lengths)
            lo, hi = a if lo is None else lo, b if hi is None else hi
        if not hi > lo:
            hi = lo + 1.0
    return single, pts, cams, scalar, lo, hi


def render(points, camera, color=None, size=3, lengths=None, lo=None, hi=None, cutoff=None, radius=analysis.BASE_RADIUS,
           velocity=None, lut=None, background=(255, 255, 255), return_winner=False,
           max_key_bytes=ops.RENDER_KEY_BYTES, return_depth=False, solids=None, solids_color=SOLIDS_COLOR):
    """Pictures of a cloud (N,3) -> (H,W,3) uint8, or of a batch (F,N,3) with optional lengths (F,) -> (F,H,W,3), on the
    points' device.  camera: one `Camera` for all frames or a list of F.  color: None / "depth" (the distance from the
    near plane, range 0 .. far - near), "density", "free_surface", "speed" (`point_scalar`), or a tensor (F,N) / (N,)
    of values per point.  lo / hi: the values that map to the ramp's ends; taken from the finite values when not
    given.  return_winner: also the (F,H,W) int32 map of the visible point per pixel (-1: background).  return_depth:
    also the (F,H,W) fp32 depth of what is seen (+inf: background).  solids: a mesh (`render_mesh`'s single forms) drawn
    in every frame in `solids_color` and composed with the points by depth; the winner map stays the points' own."""
    single, pts, cams, scalar, lo, hi = _prepare(points, camera, color, lengths, lo, hi, cutoff, radius, velocity)
    rows = np.stack([c.row() for c in cams])
    out = ops.render_points(pts, rows, cams[0].width, cams[0].height, default_lut() if lut is None else lut, size,
                            lengths, scalar, lo, hi, background, max_key_bytes,
                            return_depth=return_depth or solids is not None)
    image, winner, depth = out if len(out) == 3 else out + (None,)
    if solids is not None:
        image, depth = _with_solids(image, depth, solids, solids_color, rows, cams[0], pts.shape[0], background,
                                    max_key_bytes)
    if single:
        image, winner, depth = image[0], winner[0], None if depth is None else depth[0]
    extra = ((winner,) if return_winner else ()) + ((depth,) if return_depth else ())
    return (image,) + extra if extra else image


def render_surface(points, camera, particle_radius=analysis.BASE_RADIUS, color=None, lengths=None, lo=None, hi=None,
                   cutoff=None, radius=analysis.BASE_RADIUS, velocity=None, lut=None, background=(255, 255, 255),
                   half_width=2, iters=3, delta=None, light=None, return_depth=False, return_winner=False,
                   max_key_bytes=ops.RENDER_KEY_BYTES, solids=None, solids_color=SOLIDS_COLOR, translucent=False,
                   absorption=None, thickness_iters=2, return_thickness=False):
    """Pictures of the fluid's SURFACE (`ops.render_surface`: every point a sphere of `particle_radius`, the nearest
    fronts smoothed `iters` times over a window of half-width `half_width` without crossing depth steps above `delta`,
    default 2 x particle_radius, then shaded).  points, camera, color, lengths, lo, hi, cutoff, radius, velocity, lut
    and background are `render`'s and give the surface's base colour.  light: the direction towards the light in view
    coordinates (x right, y down, z forward; None: `ops.surface_shade()`'s).  return_depth / return_winner: also the
    smoothed depth (F,H,W) fp32 (+inf: background) / the (F,H,W) int32 map of the point in front.  solids: a mesh
    (`render_mesh`'s single forms) drawn in every frame in `solids_color` under the same light and composed with the
    fluid by depth; the depth returned is then the composed one, the winner map stays the fluid's own.
    translucent: the fluid absorbs light instead of hiding what is behind it: the solids (or the bare background) are
    drawn first, `ops.render_thickness` measures the fluid in front of them per pixel, that image is blurred
    `thickness_iters` times with the window of `half_width`, and `ops.absorb_layers` mixes the shaded surface with what
    lies behind it.  absorption: three coefficients (red, green, blue) per particle DIAMETER, default `ABSORPTION`; the
    table reaches `THICKNESS_DIAMETERS` diameters, thicker fluid absorbs like that much.  return_thickness: also the
    blurred thickness (F,H,W) fp32 in world units, after depth and winner (with `translucent` only)."""
    single, pts, cams, scalar, lo, hi = _prepare(points, camera, color, lengths, lo, hi, cutoff, radius, velocity)
    if return_thickness and not translucent:
        raise ValueError("return_thickness goes with translucent=True")
    rows = np.stack([c.row() for c in cams])
    shade = None if light is None else ops.surface_shade(light)
    out = ops.render_surface(pts, rows, cams[0].width, cams[0].height, default_lut() if lut is None else lut,
                             particle_radius, lengths, scalar, lo, hi, half_width, iters, delta, shade, background,
                             max_key_bytes)
    if translucent:
        F, (W, H) = pts.shape[0], (cams[0].width, cams[0].height)
        if solids is not None:
            behind, limit = _solid_layer(out[0].device, solids, solids_color, rows, cams[0], F, background, max_key_bytes,
                                         shade)
        else:
            behind = torch.tensor([int(c) for c in background], dtype=torch.uint8, device=pts.device)
            behind, limit = behind.view(1, 1, 1, 3).expand(F, H, W, 3).contiguous(), None
        thickness = ops.render_thickness(pts, rows, W, H, particle_radius, lengths, limit, max_key_bytes)
        thickness = ops.surface_smooth(thickness, half_width, None, thickness_iters)
        diameter = 2.0 * float(particle_radius)
        th_max = THICKNESS_DIAMETERS * diameter
        sigma = np.asarray(ABSORPTION if absorption is None else absorption, dtype=np.float64).reshape(-1) / diameter
        if limit is None:
            limit = torch.full((F, H, W), float("inf"), dtype=torch.float32, device=pts.device)
        out = ops.absorb_layers(out[0], out[1], thickness, behind, limit, ops.absorb_table(sigma, th_max), th_max) + \
            (out[2], thickness)
    elif solids is not None:
        out = _with_solids(out[0], out[1], solids, solids_color, rows, cams[0], pts.shape[0], background, max_key_bytes,
                           shade) + (out[2],)
    out = tuple(o[0] for o in out) if single else out
    image, depth, winner = out[:3]
    extra = ((depth,) if return_depth else ()) + ((winner,) if return_winner else ()) + \
        ((out[3],) if return_thickness else ())
    return (image,) + extra if extra else image


def _mesh_parts(mesh, device):
    """A `mesh.Mesh`, or (vertices, faces[, normals]) of arrays / tensors -> (vertices (V,3) fp32, faces (T,3) int32,
    normals (V,3) fp32 or None) on `device` (None: where the vertices are)."""
    if hasattr(mesh, "_fields"):
        mesh = (mesh.vertices, mesh.faces, mesh.normals)
    if not isinstance(mesh, tuple) or len(mesh) not in (2, 3):
        raise ValueError("a mesh is a mesh.Mesh or a tuple (vertices, faces[, normals])")
    v = torch.as_tensor(mesh[0]).detach()
    device = v.device if device is None else torch.device(device)
    v = v.to(device).float().reshape(-1, 3)
    f = torch.as_tensor(mesh[1]).detach().to(device).to(torch.int32).reshape(-1, 3)
    n = None if len(mesh) < 3 or mesh[2] is None else torch.as_tensor(mesh[2]).detach().to(device).float().reshape(-1, 3)
    if n is not None and n.shape != v.shape:
        raise ValueError("normals go with the vertices, one each")
    return v, f, n


def pad_meshes(meshes, device=None):
    """list of F meshes (`_mesh_parts`' forms) -> the ragged batch `ops.render_mesh` takes: (vertices (F,max V,3) fp32,
    faces (F,max T,3) int32, normals (F,max V,3) or None unless every mesh has them, vlengths (F,), flengths (F,)); rows
    beyond a mesh's own are zero and never read."""
    parts = [_mesh_parts(m, device) for m in meshes]
    device = parts[0][0].device
    vl, fl = [p[0].shape[0] for p in parts], [p[1].shape[0] for p in parts]
    vertices = torch.zeros((len(parts), max(max(vl), 1), 3), dtype=torch.float32, device=device)
    faces = torch.zeros((len(parts), max(max(fl), 1), 3), dtype=torch.int32, device=device)
    normals = torch.zeros_like(vertices) if all(p[2] is not None for p in parts) else None
    for m, (v, f, n) in enumerate(parts):
        vertices[m, :vl[m]], faces[m, :fl[m]] = v.to(device), f.to(device)
        if normals is not None:
            normals[m, :vl[m]] = n.to(device)
    return (vertices, faces, normals, torch.tensor(vl, dtype=torch.int64, device=device),
            torch.tensor(fl, dtype=torch.int64, device=device))


def render_mesh(mesh, camera, color=None, base=None, lo=None, hi=None, lut=None, background=(255, 255, 255), light=None,
                return_depth=False, return_winner=False, max_key_bytes=ops.RENDER_KEY_BYTES, device=None):
    """Pictures of triangle meshes (`ops.render_mesh`: a z-buffered rasteriser, both sides lit).  mesh: a `mesh.Mesh`,
    a tuple (vertices (V,3), faces (T,3)[, normals (V,3)]) of tensors or arrays, or a LIST of F of either, one per frame
    (padded into a ragged batch).  camera: one `Camera`, or a list of F; one mesh under F cameras gives F pictures.  One
    mesh under one camera -> (H,W,3) uint8, else (F,H,W,3), on the vertices' device (arrays go to `device`).  The base
    colour: `base` (3 values 0..255), else the ramp of `color`, a tensor (V,) / (F,V) of values per vertex with lo / hi
    (taken from the finite values when not given), else of the depth.  Vertex normals shade smoothly; without them
    every face has its own.  light: as for `render_surface`.  return_depth / return_winner: also the depth (+inf:
    background) / the face index per pixel (-1: background)."""
    cams = [camera] if isinstance(camera, Camera) else list(camera)
    if any((c.width, c.height) != (cams[0].width, cams[0].height) for c in cams):
        raise ValueError("the cameras of one call share the picture's size")
    many = isinstance(mesh, list)
    vertices, faces, normals, vlengths, flengths = pad_meshes(mesh if many else [mesh], device)
    single = not many and len(cams) == 1
    scalar = None
    if color is not None and not (isinstance(color, str) and color == "depth"):
        if isinstance(color, str):
            raise ValueError('a mesh is coloured by "depth", by values per vertex, or by `base`')
        scalar = torch.zeros(vertices.shape[:2], dtype=torch.float32, device=vertices.device)
        values = color if isinstance(color, (list, tuple)) else ([color] if not many else list(color))
        for m, c in enumerate(values):
            scalar[m, :int(vlengths[m])] = torch.as_tensor(c).detach().to(vertices.device).float().reshape(-1)
        if lo is None or hi is None:
            a, b = _finite_range(scalar, vlengths)
            lo, hi = a if lo is None else lo, b if hi is None else hi
        if not hi > lo:
            hi = lo + 1.0
    image, depth, winner = ops.render_mesh(
        vertices, faces, np.stack([c.row() for c in cams]), cams[0].width, cams[0].height,
        default_lut() if lut is None else lut, vlengths, flengths, normals, scalar, lo, hi, base,
        None if light is None else ops.surface_shade(light), background, max_key_bytes)
    if single:
        image, depth, winner = image[0], depth[0], winner[0]
    extra = ((depth,) if return_depth else ()) + ((winner,) if return_winner else ())
    return (image,) + extra if extra else image


def _solid_layer(device, solids, color, rows, camera, F, background, max_key_bytes, shade=None):
    """`solids` drawn over `background` under the cameras of F frames -> (image, depth)."""
    v, f, n = _mesh_parts(solids, device)
    rows = rows if rows.shape[0] == F else np.repeat(rows, F, axis=0)          # one mesh, F frames
    solid = ops.render_mesh(v.unsqueeze(0).contiguous(), f.unsqueeze(0).contiguous(), rows, camera.width, camera.height,
                            default_lut(), normals=None if n is None else n.unsqueeze(0).contiguous(),
                            base=tuple(int(c) for c in color), shade=shade, background=background,
                            max_key_bytes=max_key_bytes)
    return solid[0], solid[1]


def _with_solids(image, depth, solids, color, rows, camera, F, background, max_key_bytes, shade=None):
    """The fluid's layer (image, depth) of F frames composed with `solids` drawn under the same cameras -> (image,
    depth).  On equal depth the fluid shows."""
    return ops.compose_layers([(image, depth), _solid_layer(image.device, solids, color, rows, camera, F, background,
                                                            max_key_bytes, shade)])


def write_png(path, image):
    """(H,W,3) uint8 (tensor or array) -> an 8-bit RGB PNG, every scanline with filter type 0; standard library only.
    Deflate level 1: the encoding is most of what a picture costs, and level 6 takes about three times as
    long for files a third smaller."""
    a = image.detach().cpu().numpy() if isinstance(image, torch.Tensor) else np.asarray(image)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("image must be (H,W,3) uint8")
    h, w = a.shape[:2]
    rows = np.concatenate([np.zeros((h, 1), np.uint8), np.ascontiguousarray(a).reshape(h, w * 3)], axis=1)

    def chunk(kind, data):
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(rows.tobytes(), 1)) + chunk(b"IEND", b""))


def pad_frames(frames, device):
    """list of (n_t,3) arrays / tensors -> ((T,max n,3) fp32 on `device`, zero rows beyond a frame's own, lengths (T,))."""
    frames = [torch.as_tensor(f).detach().float().reshape(-1, 3) for f in frames]
    lens = [f.shape[0] for f in frames]
    batch = torch.zeros((len(frames), max(max(lens), 1), 3), dtype=torch.float32, device=device)
    for t, f in enumerate(frames):
        batch[t, :lens[t]] = f.to(device)
    return batch, torch.tensor(lens, dtype=torch.int64, device=device)


class SequenceRenderer:
    """Pictures of a sequence, `pcd_{i:04d}.png` in `out_dir`, under ONE camera: fitted to the frames of the first
    `push` unless `camera` is given.  The range of a "density" colour is that of the first `push` as well, so the
    pictures of a sequence are comparable.  `push(frames, first)`: frames = list of (n_t,3) clouds, first = index of
    the first one; they are rendered in one call.  style: "points" (`render`, squares of `size` pixels) or "surface"
    (`render_surface`: spheres of `particle_radius`, `smooth_iters` passes of half-width `half_width`) or "surface_mesh" (every
    frame meshed by `mesh.surface_mesh(**mesh_options)` and drawn with its vertex normals by `render_mesh`, coloured by
    depth).  solids: a mesh (`render_mesh`'s single forms) drawn into every picture in `solids_color`; the camera is
    still fitted to the frames alone.  translucent, absorption, thickness_iters: `render_surface`'s, style "surface"
    only."""

    def __init__(self, out_dir, size=3, width=768, height=768, mode="pinhole", color="depth", cutoff=None,
                 direction=(0.0, 0.0, -1.0), camera=None, device="cuda", style="points",
                 particle_radius=analysis.BASE_RADIUS, smooth_iters=3, half_width=2, solids=None,
                 solids_color=SOLIDS_COLOR, mesh_options=None, translucent=False, absorption=None, thickness_iters=2):
        if color not in ("depth", "density", "free_surface"):
            raise ValueError("color must be depth, density or free_surface")
        if style not in STYLES:
            raise ValueError(f"style must be one of {STYLES}")
        if style == "surface_mesh" and color != "depth":
            raise ValueError('style "surface_mesh" colours the surface by depth')
        if translucent and style != "surface":
            raise ValueError(f'translucent goes with style "surface", not with "{style}"')
        if absorption is not None:
            absorption = tuple(float(c) for c in absorption)
            if len(absorption) != 3 or not all(np.isfinite(c) and c >= 0.0 for c in absorption):
                raise ValueError("absorption must be 3 finite values >= 0")
        if int(thickness_iters) < 0:
            raise ValueError("thickness_iters must not be negative")
        self.translucent, self.absorption, self.thickness_iters = bool(translucent), absorption, int(thickness_iters)
        self.solids, self.solids_color, self.mesh_options = solids, tuple(solids_color), dict(mesh_options or {})
        self.style, self.particle_radius = style, float(particle_radius)
        self.smooth_iters, self.half_width = int(smooth_iters), int(half_width)
        self.out_dir, self.size, self.width, self.height, self.mode = out_dir, int(size), int(width), int(height), mode
        self.color, self.cutoff, self.direction, self.camera = color, cutoff, tuple(direction), camera
        self.device, self.range = torch.device(device), (None, None)
        os.makedirs(out_dir, exist_ok=True)

    def _translucent(self):
        """`render_surface`'s extra arguments; none without `translucent`: that route is the one of before."""
        if not self.translucent:
            return {}
        return dict(translucent=True, absorption=self.absorption, thickness_iters=self.thickness_iters)

    def fit(self, frames):
        self.camera = Camera.fit(list(frames), direction=self.direction, mode=self.mode, width=self.width,
                                 height=self.height)
        return self.camera

    def push(self, frames, first):
        if self.camera is None:
            self.fit(frames)
        batch, lengths = pad_frames(frames, self.device)
        lo, hi = self.range
        if self.color == "density" and lo is None:
            s = point_scalar(batch, "density", lengths, self.cutoff)
            self.range = lo, hi = 0.0, max(_finite_range(s, lengths)[1], 1e-12)
        solids = {} if self.solids is None else dict(solids=self.solids, solids_color=self.solids_color)
        if self.style == "surface_mesh":
            from . import mesh                      # mesh imports this module
            meshes = [mesh.surface_mesh(batch[t, :int(lengths[t])], **self.mesh_options) for t in range(len(frames))]
            images, depth = render_mesh(meshes, self.camera, return_depth=True)
            if self.solids is not None:
                images, _ = _with_solids(images, depth, self.solids, self.solids_color, self.camera.row()[None],
                                         self.camera, len(frames), (255, 255, 255), ops.RENDER_KEY_BYTES)
        elif self.style == "surface":
            images = render_surface(batch, self.camera, self.particle_radius, self.color, lengths, lo, hi, self.cutoff,
                                    half_width=self.half_width, iters=self.smooth_iters, **solids, **self._translucent())
        else:
            images = render(batch, self.camera, self.color, self.size, lengths, lo, hi, self.cutoff, **solids)
        images = images.cpu().numpy()
        for t, image in enumerate(images):
            write_png(os.path.join(self.out_dir, f"pcd_{first + t:04d}.png"), image)


def add_render_options(ap):
    ap.add_argument("--size", type=int, default=3, help="edge of a point's square in pixels, 1..16")
    ap.add_argument("--width", type=int, default=768)
    ap.add_argument("--height", type=int, default=768)
    ap.add_argument("--mode", choices=sorted(MODES), default="pinhole")
    ap.add_argument("--color", choices=("depth", "density", "free_surface"), default="depth")
    ap.add_argument("--cutoff", type=float, default=0.0775, help="density cutoff of --color density")
    ap.add_argument("--direction", type=float, nargs=3, default=(0.0, 0.0, -1.0), metavar=("X", "Y", "Z"),
                    help="viewing direction (y is up)")
    ap.add_argument("--style", choices=STYLES, default="points",
                    help="points: a square per point; surface: the shaded fluid surface; surface_mesh: the meshed surface")
    ap.add_argument("--particle_radius", type=float, default=analysis.BASE_RADIUS,
                    help="--style surface: a point's sphere radius in world units")
    ap.add_argument("--smooth_iters", type=int, default=3, help="--style surface: smoothing passes over the depth")
    ap.add_argument("--smooth_half_width", type=int, default=2,
                    help="--style surface: half-width of the smoothing window, 1..4")
    ap.add_argument("--translucent", action="store_true",
                    help="--style surface: the fluid absorbs light by its thickness and shows what is behind it")
    ap.add_argument("--absorption", type=float, nargs=3, default=None, metavar=("R", "G", "B"),
                    help=f"--translucent: absorption per particle diameter (default {' '.join(map(str, ABSORPTION))})")
    ap.add_argument("--thickness_iters", type=int, default=2, metavar="K",
                    help="--translucent: blur passes over the thickness image")
    ap.add_argument("--solids", default=None, metavar="PATH|SPEC",
                    help="a mesh drawn into every picture: an .obj / .ply file (a scene's obstacles.ply), icosphere:N or "
                         "torus:R,r,nu,nv")
    ap.add_argument("--solids_color", type=int, nargs=3, default=SOLIDS_COLOR, metavar=("R", "G", "B"))


def check_render_options(ap, a):
    """The argument errors of `add_render_options`' translucency options, raised at parse time."""
    if a.translucent and a.style != "surface":
        ap.error(f"--translucent needs --style surface: it is the fluid's surface that absorbs light, not --style {a.style}")
    if a.thickness_iters < 0:
        ap.error("--thickness_iters must not be negative")
    if a.absorption is not None and not all(np.isfinite(c) and c >= 0.0 for c in a.absorption):
        ap.error("--absorption takes three finite values >= 0")


MESH_OPTIONS = ("spacing", "support", "step", "iso", "kernel", "cov_radius", "smooth_lambda")    # mesh.add_mesh_options'


def renderer_from(a, out_dir, device):
    """The renderer of the options `add_render_options` added; --style surface_mesh takes the mesher's options where the parser
    has them too (`mesh.add_mesh_options`), and `mesh.surface_mesh`'s defaults otherwise."""
    solids = None
    if getattr(a, "solids", None):
        from . import mesh                          # mesh imports this module
        solids = mesh.load_spec(a.solids)
    return SequenceRenderer(out_dir, a.size, a.width, a.height, a.mode, a.color, a.cutoff, a.direction, device=device,
                            style=a.style, particle_radius=a.particle_radius, smooth_iters=a.smooth_iters,
                            half_width=a.smooth_half_width, solids=solids,
                            solids_color=getattr(a, "solids_color", SOLIDS_COLOR),
                            translucent=getattr(a, "translucent", False), absorption=getattr(a, "absorption", None),
                            thickness_iters=getattr(a, "thickness_iters", 2),
                            mesh_options={k: getattr(a, k) for k in MESH_OPTIONS if hasattr(a, k)})


def load_frame(path):
    """`evaluate.load_frame` (.npy, or .npz with `pos`), and the action demo's .npz files, whose entry is `pred`."""
    from .evaluate import load_frame as load
    if path.endswith(".npz"):
        with np.load(path) as data:
            if "pos" not in data.files and "pred" in data.files:
                return np.ascontiguousarray(data["pred"], dtype=np.float32).reshape(-1, 3)
    return load(path)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tpgan_amd.render", description="Render a sequence of frames to PNG files.")
    ap.add_argument("--frames", required=True, help="frame files, '{i}' = frame index, e.g. 'out/pcd_{i}.npy'")
    ap.add_argument("--count", type=int, required=True, help="frames 0 .. count-1")
    ap.add_argument("--out", required=True, help="output directory for pcd_{i:04d}.png")
    add_render_options(ap)
    ap.add_argument("--frames_per_call", type=int, default=FRAMES_PER_CALL, help="frames rendered per call")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    if "{i}" not in a.frames:
        ap.error("--frames must contain '{i}'")
    if a.count < 1 or a.frames_per_call < 1:
        ap.error("--count and --frames_per_call must be at least 1")
    check_render_options(ap, a)
    seq = renderer_from(a, a.out, torch.device(a.device))
    # one camera for the whole sequence: the union box of the first, the middle and the last frame
    seq.fit([load_frame(a.frames.format(i=i)) for i in sorted({0, a.count // 2, a.count - 1})])
    for i in range(0, a.count, a.frames_per_call):
        idx = range(i, min(i + a.frames_per_call, a.count))
        seq.push([load_frame(a.frames.format(i=j)) for j in idx], i)
    print(f"wrote {a.count} pictures to {a.out}")


if __name__ == "__main__":
    main()

"""Host-side operator layer: torch tensors in, C-ABI calls out, autograd glue.

The functional API here is what the import-compatible modules in ``compat/``
(pointnet2_ops, pytorch3d.ops, frnn, chamferdist) and the model code call.

Device dispatch: CUDA/HIP tensors go to libtpgan_hip.so.  CPU tensors raise --
like upstream's "CPU not supported" -- unless a test or the bench's cpu_baseline
leg has explicitly registered a checker backend with ``register_backend('cpu',
...)``; the product never registers one itself and never imports ``oracle``.
"""
import ctypes as C

import os

import numpy as np
import torch

from . import _lib

_BACKENDS = {}


class OpTimer:
    """Per-kernel timing with HIP events recorded on the stream each kernel is launched on
    (torch's current stream).  Used by bench.py for the roofline leg; off by default."""

    def __init__(self):
        self.pending = {}   # name -> [(start_evt, end_evt, algorithmic_bytes)]

    def record(self, name, nbytes, stream_of, launch, flops=0):
        st = torch.cuda.current_stream(stream_of.device)
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record(st)
        out = launch()
        b.record(st)
        self.pending.setdefault(name, []).append((a, b, nbytes, flops))
        return out

    def summary(self):
        """name -> dict(launches, total_ms, avg_us, bytes_per_launch, gbps, flops_per_launch, tflops);
        call after a sync."""
        out = {}
        for name, recs in self.pending.items():
            ms = [a.elapsed_time(b) for a, b, _, _ in recs]
            by = [n for _, _, n, _ in recs]
            fl = [f for _, _, _, f in recs]
            tot = sum(ms)
            out[name] = dict(launches=len(recs), total_ms=tot, avg_us=1e3 * tot / len(recs),
                             bytes_per_launch=sum(by) / len(by),
                             gbps=(sum(by) / 1e9) / (tot / 1e3) if tot > 0 else 0.0,
                             flops_per_launch=sum(fl) / len(fl),
                             tflops=(sum(fl) / 1e12) / (tot / 1e3) if tot > 0 else 0.0)
        return out


_timer = None


def set_timer(timer):
    """Install (or remove with None) an OpTimer; returns the previous one."""
    global _timer
    prev, _timer = _timer, timer
    return prev


def _run(name, nbytes, t, launch, flops=0):
    if _timer is None:
        return launch()
    return _timer.record(name, nbytes, t, launch, flops)


def timed(name, nbytes, flops, t, launch):
    """Run `launch()` (a library GEMM of the host layer) under the per-kernel timer, if one is installed."""
    return _run(name, nbytes, t, launch, flops)


def register_backend(device_type, impl):
    """Install an op backend for a non-HIP device type (tests / cpu_baseline only)."""
    if device_type == "cuda":
        raise ValueError("the cuda backend is the HIP library and cannot be replaced")
    _BACKENDS[device_type] = impl


def unregister_backend(device_type):
    _BACKENDS.pop(device_type, None)


def radius_sq(r):
    """python float radius -> fp32 r*r, the value both backends compare against."""
    r32 = np.float32(r)
    return float(np.float32(r32 * r32))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(t):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


class _DeviceGuard:
    """Make `t.device` current for the duration of a launch (no-op when it already is)."""

    def __init__(self, t):
        self.idx = t.device.index
        self.prev = None

    def __enter__(self):
        cur = torch.cuda.current_device()
        if self.idx is not None and cur != self.idx:
            self.prev = cur
            torch.cuda.set_device(self.idx)

    def __exit__(self, *a):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)


class HipBackend:
    """Raw (non-autograd) ops on HIP tensors through the C-ABI (include/tpgan_ops.h).

    Every method allocates its outputs with torch, launches on torch's current stream and
    returns without synchronising.  `_call` adds the optional per-kernel HIP-event timing
    (algorithmic bytes per launch are the SURVEY.md section 8d figures)."""

    name = "hip"

    def __init__(self):
        self.lib = _lib.load()
        self._ws = {}
        self._ws_retired = []   # outgrown workspaces: captured graphs may still hold their addresses
        self._sn_plans = {}

    def _retire(self, ws):
        """A workspace that is being replaced by a larger one stays allocated: a hipGraph captured earlier has its
        address baked in, and replaying that graph after the tensor went back to the allocator would scribble on
        whoever got the memory next.  (Sizes grow monotonically per (kind, stream): a handful of buffers at most.)"""
        if ws is not None:
            self._ws_retired.append(ws)

    def _workspace(self, kind, ref, need, dtype=torch.float32, zeroed=False):
        """The grow-only scratch buffer of `kind` (>= need elements of dtype) on ref's device and current stream.
        One buffer per (kind, device, stream), reused by every call: launches on a stream are ordered, so the next
        call cannot start before the previous one has consumed it.  zeroed: filled with zeros when it is created."""
        key = (kind, ref.device, torch.cuda.current_stream(ref.device).cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            self._retire(ws)
            ws = (torch.zeros if zeroed else torch.empty)(need, dtype=dtype, device=ref.device)
            self._ws[key] = ws
        return ws

    def _call(self, symbol, op, nbytes, ref, *args, flops=0):
        fn = getattr(self.lib, symbol)
        with _DeviceGuard(ref):
            _lib.check(_run(op, nbytes, ref, lambda: fn(*args, _stream(ref)), flops), symbol)

    # A radius search goes to the uniform grid (csrc/frnn_grid.hip) from GRID_MIN_PAIRS query x point
    # pairs on (and GRID_MIN_POINTS searched points per cloud); below, the exhaustive wave-per-query
    # kernel wins.  Measured on MI355X, tools/tune_frnn.py, B = 8, K = 16 self search: 2048 points 40 / 40 us,
    # 4096: 105 / 60 us, 16384: 1176 / 169 us, 131072 (B = 1): 8267 / 383 us (exhaustive / grid); the grid
    # costs ~30 us of build launches whatever the size.
    GRID_MIN_POINTS = 1024
    GRID_MIN_PAIRS = 6.0e7

    KNN_GRID_MIN_POINTS = 2048
    CHAMFER_GRID_MIN_POINTS = 8192

    def _use_grid(self, B, Nq, Np, min_points=None):
        """The size switch of every op that has a grid form: enough searched points per cloud (GRID_MIN_POINTS, or the
        op's own floor) and enough query x point pairs in the call."""
        floor = self.GRID_MIN_POINTS if min_points is None else min_points
        return Np >= floor and float(B) * Nq * Np >= self.GRID_MIN_PAIRS

    def _grid_ws(self, ref, B, P2):
        return self._workspace("frnn", ref, self.lib.tpg_frnn_grid_workspace_bytes(B, P2), dtype=torch.uint8)

    def knn(self, p1, p2, len1, len2, K, r2, r=None):
        B, P1, D = p1.shape
        P2 = p2.shape[1]
        dist = torch.empty((B, P1, K), dtype=torch.float32, device=p1.device)
        idx = torch.empty((B, P1, K), dtype=torch.int64, device=p1.device)
        if r is not None and r2 is not None and D == 3 and K <= 64 and self._use_grid(B, P1, P2) and float(r) > 0:
            self._call("tpg_frnn_grid_f32", "frnn_grid", 4 * B * D * (P1 + P2) + 12 * B * P1 * K, p1,
                       _ptr(p1), _ptr(p2), _ptr(len1), _ptr(len2), B, P1, P2, K, float(np.float32(r)), _ptr(dist),
                       _ptr(idx), _ptr(self._grid_ws(p1, B, P2)))
            return dist, idx
        if r2 is None and D == 3 and K <= 64 and self._use_grid(B, P1, P2, self.KNN_GRID_MIN_POINTS):
            # plain 3-D kNN on the uniform grid (first EdgeConv at cfg5 / rollout sizes, Chamfer at 16384 points):
            # measured (tools/tune_frnn.py) B = 40, 4096 points, K = 20: 431 us exhaustive
            self._call("tpg_knn_grid_f32", "knn_grid", 4 * B * D * (P1 + P2) + 12 * B * P1 * K, p1,
                       _ptr(p1), _ptr(p2), _ptr(len1), _ptr(len2), B, P1, P2, K, _ptr(dist), _ptr(idx),
                       _ptr(self._grid_ws(p1, B, P2)))
            return dist, idx
        # (the library takes the matrix-core filter by itself under exactly this condition, csrc/knn.hip: the name
        # and the executed flops -- two sweeps, three split products -- are for the per-kernel timer only)
        mfma = r2 is None and D in (32, 64) and 1 < K <= 24 and P2 >= 2048 and os.environ.get("TPG_KNN_MFMA", "1")[:1] != "0"
        self._call("tpg_knn_f32", "knn_mfma" if mfma else "knn", 4 * B * D * (P1 + P2) + 12 * B * P1 * K, p1,
                   _ptr(p1), _ptr(p2), _ptr(len1), _ptr(len2), B, P1, P2, D, K,
                   -1.0 if r2 is None else r2, _ptr(dist), _ptr(idx), flops=12.0 * B * P1 * P2 * D if mfma else 0)
        return dist, idx

    def _knn_filter(self, symbol, op, flops, p1, p2, len1, len2, K, redo):
        B, P1, D = p1.shape
        P2 = p2.shape[1]
        dist = torch.zeros((B, P1, K), dtype=torch.float32, device=p1.device)
        idx = torch.zeros((B, P1, K), dtype=torch.int64, device=p1.device)
        self._call(symbol, op, 4 * B * D * (P1 + P2) + 12 * B * P1 * K, p1, _ptr(p1), _ptr(p2), _ptr(len1), _ptr(len2),
                   B, P1, P2, D, K, _ptr(dist), _ptr(idx), 1 if redo else 0, flops=flops * B * P1 * P2 * D)
        return dist, idx

    def knn_mfma(self, p1, p2, len1, len2, K, redo=True):
        """The matrix-core filter path of tpg_knn_f32 called directly (D = 32 / 64, 2 <= K <= 24): what
        tpg_knn_f32 runs by itself on clouds of >= 2048 points.  redo=False leaves idx[..., 0] = -2 on the
        queries the filter could not settle (tests and tuning count them)."""
        return self._knn_filter("tpg_knn_mfma_f32", "knn_mfma", 12.0, p1, p2, len1, len2, K, redo)

    def knn_small(self, p1, p2, len1, len2, K, redo=True):
        """The one-sweep filter path of tpg_knn_f32 called directly (D = 32 / 64, 2 <= K <= 24, P2 <= 1024): what
        tpg_knn_f32 runs by itself on small feature-space clouds (csrc/knn_small.hpp).  redo=False leaves
        idx[..., 0] = -2 on the queries the filter could not settle (tests and tuning count them)."""
        return self._knn_filter("tpg_knn_small_f32", "knn", 0, p1, p2, len1, len2, K, redo)

    def cubic_interp(self, query, pos, field, cutoff):
        B, Nq, _ = query.shape
        Np, F_ = pos.shape[1], field.shape[2]
        plain = torch.empty((B, Nq, F_), dtype=torch.float32, device=query.device)
        pad = torch.empty_like(plain)
        hits = torch.empty((B, Nq), dtype=torch.int32, device=query.device)
        self._call("tpg_cubic_interp_f32", "cubic_interp", 12 * B * (Nq + Np) + 4 * B * Np * F_ + 8 * B * Nq * F_,
                   query, _ptr(query), _ptr(pos), _ptr(field), B, Nq, Np, F_, float(cutoff), _ptr(plain),
                   _ptr(pad), _ptr(hits))
        return plain, pad, hits

    def radius_reduce(self, query, pos, lenq, lenp, r, kernel, want_count=True, want_sum=True, grid=None):
        """csrc/radius_reduce.hip: (count (B,Nq) int32, sum (B,Nq) f32) over every stored point with d2 <= r2; the grid
        from the sizes of the radius search's switch on, the exhaustive shape of the same kernel below (same bits
        either way; `grid` forces one, for tests and tuning)."""
        B, Nq, _ = query.shape
        Np = pos.shape[1]
        count = torch.empty((B, Nq), dtype=torch.int32, device=query.device) if want_count else None
        total = torch.empty((B, Nq), dtype=torch.float32, device=query.device) if want_sum else None
        if grid is None:
            grid = self._use_grid(B, Nq, Np)
        nbytes = 12 * B * (Nq + Np) + 4 * B * Nq * (int(want_count) + int(want_sum))
        args = (_ptr(query), _ptr(pos), _ptr(lenq), _ptr(lenp), B, Nq, Np, float(np.float32(r)), int(kernel),
                _ptr(count), _ptr(total))
        if grid and B > 0 and Nq > 0 and Np > 0:
            self._call("tpg_radius_reduce_f32", "radius_reduce_grid", nbytes, query, *args,
                       _ptr(self._grid_ws(query, B, Np)))
        else:
            self._call("tpg_radius_reduce_exhaustive_f32", "radius_reduce", nbytes, query, *args)
        return count, total

    # Auction matching (csrc/emd.hip).  A cloud takes wide rounds (two launches each) while more than `narrow_at` of its
    # persons are unassigned and the narrow path (EMD_NARROW_ROUNDS rounds per launch, one workgroup per cloud) below;
    # the host reads the per-cloud records once per batch of EMD_CHECK_EVERY wide rounds + one narrow launch.  On the
    # narrow path the workgroup's 16 waves scan the n objects once per bidder, so its cost per round grows as
    # bidders x n while a wide round spreads the bidders over the chip: the threshold is a bound on that WORK,
    # narrow_at = EMD_NARROW_WORK / n, but never below one bidder per wave.  The values are tuning only -- the results
    # do not depend on them -- and come from the sweep in profiles/metrics.txt (tools/metrics_time.py).
    EMD_NARROW_WORK = 256 * 1024
    EMD_NARROW_MIN = 16
    EMD_CHECK_EVERY = 8
    EMD_NARROW_ROUNDS = 256

    def emd_narrow_at(self, n):
        return max(0, min(n, max(self.EMD_NARROW_MIN, self.EMD_NARROW_WORK // max(n, 1))))

    def emd_begin(self, xyz1, xyz2, phases):
        """tpg_emd_init_f32 -> the handle the next two steps take (outputs and workspace of one matching)."""
        B, n, _ = xyz1.shape
        dev = xyz1.device
        st = {"xyz1": xyz1, "B": B, "n": n, "phases": int(phases),
              "dist": torch.empty((B, n), dtype=torch.float32, device=dev),
              "assignment": torch.empty((B, n), dtype=torch.int32, device=dev),
              "price": torch.empty((B, n), dtype=torch.float32, device=dev),
              "rounds": torch.zeros((B,), dtype=torch.int32, device=dev)}
        st["ws"] = self._workspace("emd", xyz1, self.lib.tpg_emd_workspace_bytes(B, n), dtype=torch.uint8)
        self._call("tpg_emd_init_f32", "emd_init", 16 * B * n, xyz1, _ptr(xyz2), B, n, xyz2.shape[1], int(phases),
                   _ptr(st["assignment"]), _ptr(st["ws"]))
        return st

    def emd_batch(self, st, eps, iters, scaling, narrow_at, wide):
        """tpg_emd_rounds_f32 once, then the per-cloud records on the host (the one synchronisation per batch):
        -> (B,8) int32 {phase, rounds, unassigned, status, ..}, the number of kernel launches issued."""
        B, n = st["B"], st["n"]
        self._call("tpg_emd_rounds_f32", "emd_rounds", 16 * B * n, st["xyz1"], _ptr(st["xyz1"]), B, n, float(eps),
                   float(scaling), st["phases"], int(iters), int(wide), self.EMD_NARROW_ROUNDS, int(narrow_at),
                   _ptr(st["assignment"]), _ptr(st["ws"]))
        launches = (2 * int(wide) if narrow_at < n else 0) + (1 if narrow_at > 0 else 0)
        return st["ws"][:32 * B].view(torch.int32).view(B, 8).cpu(), launches

    def emd_end(self, st):
        B, n = st["B"], st["n"]
        self._call("tpg_emd_finish_f32", "emd_finish", 16 * B * n, st["xyz1"], _ptr(st["xyz1"]), B, n,
                   _ptr(st["assignment"]), _ptr(st["ws"]), _ptr(st["dist"]), _ptr(st["price"]), _ptr(st["rounds"]))
        return st["dist"], st["assignment"], st["price"], st["rounds"]

    def emd_match(self, xyz1, xyz2, eps, iters, phases, scaling, narrow_at=None, check_every=None):
        """-> dist (B,n) f32, assignment (B,n) i32, price (B,n) f32, rounds (B,) i32; RuntimeError at the round cap."""
        B, n, _ = xyz1.shape
        if B == 0 or n == 0:
            dev = xyz1.device
            return (torch.empty((B, n), dtype=torch.float32, device=dev),
                    torch.empty((B, n), dtype=torch.int32, device=dev),
                    torch.empty((B, n), dtype=torch.float32, device=dev),
                    torch.zeros((B,), dtype=torch.int32, device=dev))
        narrow_at = self.emd_narrow_at(n) if narrow_at is None else max(0, min(int(narrow_at), n))
        wide = self.EMD_CHECK_EVERY if check_every is None else int(check_every)
        st = self.emd_begin(xyz1, xyz2, phases)
        while True:
            rec, _ = self.emd_batch(st, eps, iters, scaling, narrow_at, wide)
            status = rec[:, 3]
            if bool((status == 2).any()):
                b = int(torch.nonzero(status == 2)[0])
                raise RuntimeError(f"emd_match: cloud {b} still has {int(rec[b, 2])} unassigned persons after "
                                   f"{int(rec[b, 1])} rounds (iters = {int(iters)})")
            if bool((status == 1).all()):
                return self.emd_end(st)

    def gaussian_row_sums(self, a, b, lena, lenb, sigma):
        """csrc/gauss_sum.hip: (B,N) float64 sums of exp(-c / (2 sigma^2)) over the points of b."""
        B, N, _ = a.shape
        M = b.shape[1]
        out = torch.empty((B, N), dtype=torch.float64, device=a.device)
        self._call("tpg_gaussian_row_sums_f32", "gaussian_row_sums", 12 * B * (N + M) + 8 * B * N, a, _ptr(a), _ptr(b),
                   _ptr(lena), _ptr(lenb), B, N, M, float(np.float32(sigma)), _ptr(out))
        return out

    def render_points(self, points, lengths, scalar, cams, W, H, size, lo, hi, lut, background, max_key_bytes):
        """csrc/render.hip: cams (1 or F, 18) is a host fp32 array (numpy); -> (image (F,H,W,3) uint8, winner (F,H,W)
        int32).  The 64-bit key buffer is a per-stream workspace of at most `max_key_bytes` (one frame's at least): F is
        rendered in chunks of that many frames, each chunk one call."""
        F, N, _ = points.shape
        image = torch.empty((F, H, W, 3), dtype=torch.uint8, device=points.device)
        winner = torch.empty((F, H, W), dtype=torch.int32, device=points.device)
        chunk = max(1, min(65535, int(max_key_bytes) // (8 * H * W)))
        keys = self._workspace("render_keys", points, min(chunk, max(F, 1)) * H * W, dtype=torch.int64)
        for f0 in range(0, F, chunk):
            f1 = min(F, f0 + chunk)
            c = cams if cams.shape[0] == 1 else np.ascontiguousarray(cams[f0:f1])
            self._call("tpg_render_points_f32", "render_points",
                       (f1 - f0) * (12 * N + (4 * N if scalar is not None else 0) + 23 * H * W), points,
                       _ptr(points[f0:f1]), _ptr(None if lengths is None else lengths[f0:f1]),
                       _ptr(None if scalar is None else scalar[f0:f1]), f1 - f0, N, c.ctypes.data, c.shape[0], W, H, size,
                       lo, hi, _ptr(lut), _ptr(background), _ptr(keys), _ptr(image[f0:f1]), _ptr(winner[f0:f1]))
        return image, winner

    def render_surface(self, points, lengths, scalar, cams, W, H, radius, lo, hi, lut, background, half_width, iters,
                       delta, shade, max_key_bytes):
        """csrc/surface.hip: sphere fronts, `iters` smoothing passes, shading; cams and shade are host fp32 arrays.
        -> (image (F,H,W,3) uint8, depth (F,H,W) fp32, winner (F,H,W) int32).  Frames go in chunks as in
        `render_points`; the keys and the two depth buffers the passes alternate between are per-stream workspaces, and
        the last pass of a chunk writes into the returned depth."""
        F, N, _ = points.shape
        dev = points.device
        image = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
        depth = torch.empty((F, H, W), dtype=torch.float32, device=dev)
        winner = torch.empty((F, H, W), dtype=torch.int32, device=dev)
        chunk = max(1, min(65535, int(max_key_bytes) // (8 * H * W)))
        held = min(chunk, F) * H * W
        keys = self._workspace("render_keys", points, held, dtype=torch.int64)
        ping = [self._workspace(f"surface_depth{j}", points, held) for j in range(2)] if iters > 0 else []
        for f0 in range(0, F, chunk):
            f1 = min(F, f0 + chunk)
            n, pix = f1 - f0, (f1 - f0) * H * W
            c = cams if cams.shape[0] == 1 else np.ascontiguousarray(cams[f0:f1])
            src = ping[0] if iters > 0 else depth[f0:f1]
            self._call("tpg_render_spheres_f32", "render_spheres", 12 * n * N + 24 * pix, points, _ptr(points[f0:f1]),
                       _ptr(None if lengths is None else lengths[f0:f1]), n, N, c.ctypes.data, c.shape[0], W, H, radius,
                       _ptr(keys), _ptr(src), _ptr(winner[f0:f1]))
            for it in range(iters):
                dst = depth[f0:f1] if it == iters - 1 else ping[(it + 1) % 2]
                self._call("tpg_surface_smooth_f32", "surface_smooth", 8 * pix, points, _ptr(src), n, W, H, half_width,
                           delta, _ptr(dst))
                src = dst
            self._call("tpg_surface_shade_f32", "surface_shade", 11 * pix + (4 * pix if scalar is not None else 0), points,
                       _ptr(depth[f0:f1]), _ptr(winner[f0:f1]), _ptr(None if scalar is None else scalar[f0:f1]), n, N,
                       c.ctypes.data, c.shape[0], W, H, lo, hi, _ptr(lut), _ptr(background), shade.ctypes.data,
                       _ptr(image[f0:f1]))
        return image, depth, winner

    def render_thickness(self, points, lengths, cams, W, H, radius, limit, max_key_bytes):
        """csrc/surface.hip: the fluid a pixel looks through, up to `limit` (F,H,W) or None -> (F,H,W) fp32.  Frames go
        in chunks as in `render_points`; the 64-bit sums live on the same key workspace."""
        F, N, _ = points.shape
        thickness = torch.empty((F, H, W), dtype=torch.float32, device=points.device)
        chunk = max(1, min(65535, int(max_key_bytes) // (8 * H * W)))
        acc = self._workspace("render_keys", points, min(chunk, F) * H * W, dtype=torch.int64)
        for f0 in range(0, F, chunk):
            f1 = min(F, f0 + chunk)
            n, pix = f1 - f0, (f1 - f0) * H * W
            c = cams if cams.shape[0] == 1 else np.ascontiguousarray(cams[f0:f1])
            self._call("tpg_render_thickness_f32", "render_thickness", 12 * n * N + (24 if limit is None else 28) * pix,
                       points, _ptr(points[f0:f1]), _ptr(None if lengths is None else lengths[f0:f1]), n, N,
                       c.ctypes.data, c.shape[0], W, H, radius, _ptr(None if limit is None else limit[f0:f1]), _ptr(acc),
                       _ptr(thickness[f0:f1]))
        return thickness

    def surface_smooth(self, image, half_width, delta, iters):
        """csrc/surface.hip: `iters` >= 1 passes of tpg_surface_smooth_f32 over image (F,H,W) -> a new (F,H,W); the
        passes alternate between the result and one per-stream workspace."""
        F, H, W = image.shape
        out = torch.empty_like(image)
        other = self._workspace("surface_depth0", image, F * H * W) if iters > 1 else None
        src = image
        for it in range(iters):
            dst = out if (iters - 1 - it) % 2 == 0 else other
            self._call("tpg_surface_smooth_f32", "surface_smooth", 8 * F * H * W, image, _ptr(src), F, W, H, half_width,
                       delta, _ptr(dst))
            src = dst
        return out

    def absorb_layers(self, fluid, fdepth, thickness, behind, bdepth, table, th_max):
        """csrc/surface.hip: the absorption composite; table is a host fp32 array (256,3) -> (image, depth)."""
        F, H, W = fdepth.shape
        image, depth = torch.empty_like(fluid), torch.empty_like(fdepth)
        self._call("tpg_surface_absorb_u8", "surface_absorb", 22 * F * H * W, fluid, _ptr(fluid), _ptr(fdepth),
                   _ptr(thickness), _ptr(behind), _ptr(bdepth), F, W, H, th_max, table.ctypes.data, _ptr(image), _ptr(depth))
        return image, depth

    def render_mesh(self, vertices, vlengths, faces, flengths, normals, scalar, cams, F, W, H, lo, hi, lut, base,
                    background, shade, max_key_bytes):
        """csrc/mesh_render.hip: raster + resolve, then the deferred shading; cams and shade are host fp32 arrays,
        vertices (M,V,3) / faces (M,T,3) with M = 1 (one mesh in every frame) or F.  -> (image (F,H,W,3) uint8, depth
        (F,H,W) fp32, winner (F,H,W) int32).  Frames go in chunks as in `render_points`, on the same key workspace."""
        M, V, _ = vertices.shape
        T = faces.shape[1]
        dev = vertices.device
        image = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
        depth = torch.empty((F, H, W), dtype=torch.float32, device=dev)
        winner = torch.empty((F, H, W), dtype=torch.int32, device=dev)
        chunk = max(1, min(65535, int(max_key_bytes) // (8 * H * W)))
        keys = self._workspace("render_keys", vertices, min(chunk, F) * H * W, dtype=torch.int64)
        huge = self._workspace("mesh_list", vertices, min(chunk, F) * (1 + MESH_LIST), dtype=torch.int32)

        def part(t, f0, f1):                        # the rows of a per-mesh tensor that frames f0 .. f1-1 read
            return None if t is None else (t if M == 1 else t[f0:f1])
        for f0 in range(0, F, chunk):
            f1 = min(F, f0 + chunk)
            n, pix = f1 - f0, (f1 - f0) * H * W
            c = cams if cams.shape[0] == 1 else np.ascontiguousarray(cams[f0:f1])
            m = 1 if M == 1 else n
            mesh = (_ptr(part(vertices, f0, f1)), _ptr(part(vlengths, f0, f1)), _ptr(part(faces, f0, f1)),
                    _ptr(part(flengths, f0, f1)))
            self._call("tpg_render_mesh_f32", "render_mesh", n * (48 * T + 24 * H * W), vertices, *mesh, m, V, T, n,
                       c.ctypes.data, c.shape[0], W, H, _ptr(keys), _ptr(huge), _ptr(depth[f0:f1]), _ptr(winner[f0:f1]))
            self._call("tpg_mesh_shade_f32", "mesh_shade", 59 * pix, vertices, _ptr(depth[f0:f1]), _ptr(winner[f0:f1]),
                       *mesh, _ptr(part(normals, f0, f1)), _ptr(part(scalar, f0, f1)), m, V, T, n, c.ctypes.data,
                       c.shape[0], W, H, lo, hi, _ptr(lut), _ptr(base), _ptr(background), shade.ctypes.data,
                       _ptr(image[f0:f1]))
        return image, depth, winner

    # ---- the fluid simulator's launch kinds (csrc/pbf.hip); box (B,6) and gravity (3) are host fp32 arrays ----------
    def pbf_ws(self, ref, B, N):
        return self._workspace("pbf", ref, max(int(self.lib.tpg_pbf_workspace_bytes(B, N)), 1), dtype=torch.uint8)

    def pbf_predict(self, x, v, lengths, box, dt, prm, p_out, v_out):
        B, N, _ = x.shape
        g = np.asarray(prm.gravity, dtype=np.float32)
        self._call("tpg_pbf_predict_f32", "pbf_predict", 48 * B * N, x, _ptr(x), _ptr(v), _ptr(lengths), box.ctypes.data,
                   B, N, dt, prm.radius, g.ctypes.data, _ptr(p_out), _ptr(v_out))

    def pbf_grid(self, p, lengths, prm, ws):
        B, N, _ = p.shape
        self._call("tpg_pbf_grid_f32", "pbf_grid", 36 * B * N, p, _ptr(p), _ptr(lengths), B, N, prm.h, _ptr(ws))

    def pbf_lambda(self, p, lengths, prm, ws, lam, C_out=None):
        B, N, _ = p.shape
        self._call("tpg_pbf_lambda_f32", "pbf_lambda", 16 * B * N, p, _ptr(p), _ptr(lengths), B, N, prm.h, prm.S0, prm.eps,
                   _ptr(ws), _ptr(lam), _ptr(C_out))

    def pbf_dp(self, p, lam, lengths, box, prm, ws, p_out, dp_out=None):
        B, N, _ = p.shape
        self._call("tpg_pbf_dp_f32", "pbf_dp", 28 * B * N, p, _ptr(p), _ptr(lam), _ptr(lengths), box.ctypes.data, B, N,
                   prm.h, prm.radius, prm.wq, prm.k, prm.dp_scale, _ptr(ws), _ptr(p_out), _ptr(dp_out))

    def pbf_finish(self, p, x, lengths, dt, prm, ws, x_out, v_out):
        B, N, _ = p.shape
        self._call("tpg_pbf_finish_f32", "pbf_finish", 48 * B * N, p, _ptr(p), _ptr(x), _ptr(lengths), B, N, prm.h, dt,
                   prm.cs, _ptr(ws), _ptr(x_out), _ptr(v_out))

    def pbf_finish_ex(self, p, x, lengths, dt, prm, ws, x_out, v_out, cs_tab=None, omega_out=None):
        """finish with a per-particle XSPH table cs_tab (B,N) and / or the curl into omega_out (B,N,4)."""
        B, N, _ = p.shape
        extra = (8 if cs_tab is not None else 0) + (16 if omega_out is not None else 0)
        self._call("tpg_pbf_finish_ex_f32", "pbf_finish_ex", (48 + extra) * B * N, p, _ptr(p), _ptr(x), _ptr(lengths), B, N,
                   prm.h, dt, prm.cs, _ptr(cs_tab), _ptr(ws), _ptr(x_out), _ptr(v_out), _ptr(omega_out))

    def pbf_vorticity(self, p, omega, v, lengths, dt, prm, ws, v_out):
        """v_out = v + confinement force (v_out may be v), on the grid and the omega the finish pass left."""
        B, N, _ = p.shape
        self._call("tpg_pbf_vorticity_f32", "pbf_vorticity", 68 * B * N, p, _ptr(p), _ptr(omega), _ptr(v), _ptr(lengths),
                   B, N, prm.h, dt, prm.vs, prm.delta, _ptr(ws), _ptr(v_out))

    def pbf_collide(self, p, lengths, box, obstacles, prm, p_out, hit_out=None):
        """p_out = collide(p) (p_out may be p): the obstacles (B,M,16) in index order, then the box clamp."""
        B, N, _ = p.shape
        self._call("tpg_pbf_collide_f32", "pbf_collide", (24 + (4 if hit_out is not None else 0)) * B * N, p, _ptr(p),
                   _ptr(lengths), box.ctypes.data, _ptr(obstacles), B, N, obstacles.shape[1], prm.radius, _ptr(p_out),
                   _ptr(hit_out))

    def pbf_collide_sdf(self, p, lengths, box, table, fields, prm, p_out, hit_out=None):
        """p_out = collide_sdf(p) (p_out may be p): the mesh obstacles (B,M,24) in index order, then the box clamp."""
        B, N, _ = p.shape
        self._call("tpg_pbf_collide_sdf_f32", "pbf_collide_sdf", (24 + (4 if hit_out is not None else 0)) * B * N, p,
                   _ptr(p), _ptr(lengths), box.ctypes.data, _ptr(table), _ptr(fields), fields.numel(), B, N, table.shape[1],
                   prm.radius, _ptr(p_out), _ptr(hit_out))

    def pbf_substep(self, x, v, lengths, box, dt, prm, x_out, v_out, obstacles=None, sdf_obstacles=None, xsph=None):
        """One substep of every scene: predict | iters x (grid | lambda | dp) | grid | finish.  x_out / v_out receive the
        rows below lengths; p and lambda are per-stream workspaces, the dp pass updates p in place.  obstacles (B,M,16):
        a collide launch in place after predict and after every dp; None: no such launch.  sdf_obstacles (table, fields):
        a collide_sdf launch in the same places, behind collide; None: no such launch.  xsph (B,N): the per-particle XSPH
        table; with it or with prm.vorticity > 0 the tail is grid | finish_ex | vorticity (the last only for vorticity
        > 0, in place on v_out, reading the per-stream workspace omega that finish_ex wrote)."""
        B, N, _ = x.shape
        ws = self.pbf_ws(x, B, N)
        p = self._workspace("pbf_p", x, B * N * 3)[:B * N * 3].view(B, N, 3)
        lam = self._workspace("pbf_lam", x, B * N)

        def solids():
            if obstacles is not None:
                self.pbf_collide(p, lengths, box, obstacles, prm, p)
            if sdf_obstacles is not None:
                self.pbf_collide_sdf(p, lengths, box, sdf_obstacles[0], sdf_obstacles[1], prm, p)
        self.pbf_predict(x, v, lengths, box, dt, prm, p, v_out)
        solids()
        for _ in range(prm.iters):
            self.pbf_grid(p, lengths, prm, ws)
            self.pbf_lambda(p, lengths, prm, ws, lam)
            self.pbf_dp(p, lam, lengths, box, prm, ws, p)
            solids()
        self.pbf_grid(p, lengths, prm, ws)
        if xsph is None and prm.vorticity == 0.0:
            self.pbf_finish(p, x, lengths, dt, prm, ws, x_out, v_out)
            return x_out, v_out
        omega = self._workspace("pbf_omega", x, B * N * 4)[:B * N * 4].view(B, N, 4) if prm.vorticity > 0.0 else None
        self.pbf_finish_ex(p, x, lengths, dt, prm, ws, x_out, v_out, xsph, omega)
        if omega is not None:
            self.pbf_vorticity(p, omega, v_out, lengths, dt, prm, ws, v_out)
        return x_out, v_out

    # ---- signed distance to a triangle mesh (csrc/mesh_sdf.hip; the rule: include/tpgan_ops.h)
    def mesh_sdf(self, query, vertices, faces, box, inv_unit):
        Q, V, F = query.shape[0], vertices.shape[0], faces.shape[0]
        dist = torch.empty(Q, dtype=torch.float32, device=query.device)
        face = torch.empty(Q, dtype=torch.int32, device=query.device)
        self._call("tpg_mesh_sdf_f32", "mesh_sdf", 20 * Q + 12 * (V + F), query, _ptr(query), _ptr(vertices), _ptr(faces),
                   Q, V, F, box.ctypes.data, inv_unit, _ptr(dist), _ptr(face), flops=150 * Q * F)
        return dist, face

    # ---- isosurfaces (csrc/isosurface.hip; the rule: include/tpgan_ops.h)
    def iso_count(self, field, iso):
        """Masks, triangle counts and their prefix sums into the per-stream workspace -> (ws, V, F): the ONE host read."""
        nx, ny, nz = field.shape
        ws = self._workspace("iso", field, self.lib.tpg_iso_workspace_bytes(nx, ny, nz), dtype=torch.uint8)
        counts = torch.empty(2, dtype=torch.int64, device=field.device)
        self._call("tpg_iso_count_f32", "iso_count", 14 * field.numel(), field, _ptr(field), nx, ny, nz, iso, _ptr(ws),
                   _ptr(counts))
        V, F = counts.tolist()
        return ws, int(V), int(F)

    def iso_emit(self, field, origin, step, iso, ws, V_cap, F_cap, vertices, normals, faces):
        """Vertices, normals (or None) and faces of the field `iso_count` has just classified; nothing is written at or
        beyond V_cap vertices / F_cap faces."""
        nx, ny, nz = field.shape
        self._call("tpg_iso_emit_f32", "iso_emit", 14 * field.numel() + 12 * (2 * V_cap + F_cap), field, _ptr(field), nx,
                   ny, nz, C.c_void_p(origin.ctypes.data), step, iso, _ptr(ws), int(V_cap), int(F_cap), _ptr(vertices),
                   _ptr(normals), _ptr(faces))

    def iso_surface(self, field, origin, step, iso, normals):
        ws, V, F = self.iso_count(field, iso)
        vertices = torch.empty((V, 3), dtype=torch.float32, device=field.device)
        faces = torch.empty((F, 3), dtype=torch.int32, device=field.device)
        nrm = torch.empty((V, 3), dtype=torch.float32, device=field.device) if normals else None
        if V > 0:
            self.iso_emit(field, origin, step, iso, ws, V, F, vertices, nrm, faces)
        return vertices, faces, nrm

    # ---- anisotropic kernels (csrc/aniso.hip; the rule: include/tpgan_ops.h)
    def _aniso_ws(self, ref, B, N):
        return self._workspace("aniso", ref, max(int(self.lib.tpg_aniso_workspace_bytes(B, N)), 1), dtype=torch.uint8)

    def aniso_kernels(self, pos, lengths, prm, grid=None, stages=3, out=None):
        """Stage A -> (centres (B,N,3), G (B,N,6), det (B,N), count (B,N) int32).  The grid from the sizes of the radius
        search's switch on, the exhaustive shape below (same bits; `grid` forces one).  stages / out: the walk (1) and
        the finish (2) as calls of their own into the tensors of an earlier call, for timing."""
        B, N, _ = pos.shape
        rc, lam, ks, kr, s_min, s_max, kn, n_eps = prm
        if out is None:
            out = (torch.empty((B, N, 3), dtype=torch.float32, device=pos.device),
                   torch.empty((B, N, 6), dtype=torch.float32, device=pos.device),
                   torch.empty((B, N), dtype=torch.float32, device=pos.device),
                   torch.empty((B, N), dtype=torch.int32, device=pos.device))
        if grid is None:
            grid = self._use_grid(B, N, N)
        symbol = "tpg_aniso_kernels_f32" if grid else "tpg_aniso_kernels_exhaustive_f32"
        self._call(symbol, "aniso_kernels", 12 * B * N + 44 * B * N, pos, _ptr(pos), _ptr(lengths), B, N, rc, lam, ks, kr,
                   s_min, s_max, kn, int(n_eps), int(stages), *[_ptr(t) for t in out], _ptr(self._aniso_ws(pos, B, N)))
        return out

    def aniso_field(self, query, centres, G, det, lenq, lenp, support, reach, grid=None):
        """Stage B -> sum (B,Nq) f32; the launch shapes as for `aniso_kernels`."""
        B, Nq, _ = query.shape
        Np = centres.shape[1]
        total = torch.empty((B, Nq), dtype=torch.float32, device=query.device)
        if grid is None:
            grid = self._use_grid(B, Nq, Np)
        args = (_ptr(query), _ptr(centres), _ptr(G), _ptr(det), _ptr(lenq), _ptr(lenp), B, Nq, Np, support, reach,
                _ptr(total))
        nbytes = 12 * B * Nq + 44 * B * Np + 4 * B * Nq
        if grid and B > 0 and Nq > 0 and Np > 0:
            self._call("tpg_aniso_field_f32", "aniso_field_grid", nbytes, query, *args, _ptr(self._aniso_ws(query, B, Np)))
        else:
            self._call("tpg_aniso_field_exhaustive_f32", "aniso_field", nbytes, query, *args)
        return total

    def chamfer_fwd(self, src, tgt):
        B, N, _ = src.shape
        M = tgt.shape[1]
        d1 = torch.empty((B, N), dtype=torch.float32, device=src.device)
        i1 = torch.empty((B, N), dtype=torch.int64, device=src.device)
        if min(N, M) >= self.CHAMFER_GRID_MIN_POINTS and float(B) * N * M >= self.GRID_MIN_PAIRS:
            # both directions on the uniform grid (loss.py:125-127 at cfg5's 16384-point clouds: 2.9 ms exhaustive,
            # 0.3 ms on the grid; at 4096 points the two exhaustive K = 1 launches (0.17 ms) cost what the grid's
            # twelve do, so the switch sits above that size)
            d1, i1 = self.knn(src, tgt, None, None, 1, None)
            d2, i2 = self.knn(tgt, src, None, None, 1, None)
            return d1.view(B, N), i1.view(B, N), d2.view(B, M), i2.view(B, M)
        d2 = torch.empty((B, M), dtype=torch.float32, device=src.device)
        i2 = torch.empty((B, M), dtype=torch.int64, device=src.device)
        self._call("tpg_chamfer_fwd_f32", "chamfer_fwd", 24 * B * (N + M), src,
                   _ptr(src), _ptr(tgt), B, N, M, _ptr(d1), _ptr(i1), _ptr(d2), _ptr(i2))
        return d1, i1, d2, i2

    def chamfer_bwd(self, src, tgt, i1, i2, g1, g2):
        B, N, _ = src.shape
        M = tgt.shape[1]
        gs, gt = torch.empty_like(src), torch.empty_like(tgt)
        # scratch for the two inverted nearest-neighbour indices (the gather form of the scatter: no float atomics)
        ws = torch.empty(self.lib.tpg_chamfer_bwd_workspace_bytes(B, N, M) // 4, dtype=torch.int32, device=src.device)
        self._call("tpg_chamfer_bwd_f32", "chamfer_bwd", 40 * B * (N + M), src,
                   _ptr(src), _ptr(tgt), B, N, M, _ptr(i1), _ptr(i2), _ptr(g1), _ptr(g2), _ptr(gs), _ptr(gt), _ptr(ws))
        return gs, gt

    def fps_prefix(self, xyz, m, prefix_in=None):
        """pointnet2's FPS + the per-cloud flag the next level's sampling of these centres may shortcut on
        (tpg_fps_prefix_f32); prefix_in: the flags of the launch that PRODUCED xyz's order, or None."""
        B, N, _ = xyz.shape
        idx = torch.empty((B, m), dtype=torch.int32, device=xyz.device)
        flag = torch.empty((B,), dtype=torch.int32, device=xyz.device)
        temp = torch.empty((B, N), dtype=torch.float32, device=xyz.device) if N > 16384 else None
        self._call("tpg_fps_prefix_f32", "fps" if prefix_in is None else "fps_prefix", 12 * B * N + 4 * B * m, xyz,
                   _ptr(xyz), B, N, m, _ptr(temp), _ptr(idx), _ptr(prefix_in), _ptr(flag))
        return idx, flag

    def replace_dummy_centres(self, xyz, centres, draw_key, site, prefix_flag=None):
        """tpg_replace_dummy_centres: -> (out (B,S) int32, short (1,) int32); prefix_flag (B,) int32 is cleared in place
        where a cloud's centres were replaced."""
        B, N, _ = xyz.shape
        S = centres.shape[1]
        out = torch.empty_like(centres)
        short = torch.empty((1,), dtype=torch.int32, device=xyz.device)
        self._call("tpg_replace_dummy_centres", "replace_dummy_centres", 8 * B * S, xyz, _ptr(xyz), _ptr(centres),
                   _ptr(draw_key), int(site), B, N, S, _ptr(out), _ptr(prefix_flag), _ptr(short))
        return out, short

    def context_expand(self, pos, edge, mask, state, t0):
        """Hard-masked expansion of T rollout frames with the running mask average (tpg_context_expand_f32):
        -> (points (T*N*r, 3): frame t is rows offsets[t]..offsets[t+1], offsets (T+1,) int64); `state` is updated."""
        T, N, _ = pos.shape
        r = edge.shape[1] // max(N, 1)
        out = torch.empty((T * N * r, 3), dtype=torch.float32, device=pos.device)
        offsets = torch.empty((T + 1,), dtype=torch.int64, device=pos.device)
        ws = torch.empty((max(self.lib.tpg_context_expand_workspace_bytes(T, N), 8) + 7) // 8, dtype=torch.int64,
                         device=pos.device)
        self._call("tpg_context_expand_f32", "context_expand", 4 * T * N * (2 * 3 * r + 3 + 1) + 16 * N, pos,
                   _ptr(pos), _ptr(edge), _ptr(mask), T, N, r, int(t0), _ptr(state), _ptr(out), _ptr(offsets),
                   _ptr(ws))
        return out, offsets

    def patch_select(self, points, first, count, seed, K):
        """tpg_patch_select_f32: first / count / seed are host int32 arrays (numpy); -> idx (B,K) int32."""
        B = len(first)
        idx = torch.empty((B, K), dtype=torch.int32, device=points.device)
        need = self.lib.tpg_patch_select_workspace_bytes(B, int(count.max()) if B else 0, K)
        ws = torch.empty((max(need, 8) + 7) // 8, dtype=torch.int64, device=points.device)
        self._call("tpg_patch_select_f32", "patch_select", 12 * int(count.sum()) + 4 * B * K, points,
                   _ptr(points), points.shape[0], first.ctypes.data, count.ctypes.data, seed.ctypes.data, B, K,
                   _ptr(idx), _ptr(ws))
        return idx

    def clip_gather_high(self, pos, vel, frame_first, count, centroids, centroid_row, patch):
        """tpg_clip_gather_high_f32: frame_first (T,B) / count (B) / centroid_row (B) are host int32 arrays (numpy)."""
        T, B = frame_first.shape
        K = patch.shape[1]
        high_pos = torch.empty((T, B, K, 3), dtype=torch.float32, device=pos.device)
        high_vel = torch.empty_like(high_pos) if vel is not None else None
        self._call("tpg_clip_gather_high_f32", "clip_gather_high", (1 if vel is None else 2) * 24 * T * B * K, pos,
                   _ptr(pos), _ptr(vel), pos.shape[0], frame_first.ctypes.data, count.ctypes.data, _ptr(centroids),
                   centroids.shape[0], centroid_row.ctypes.data, _ptr(patch), T, B, K, _ptr(high_pos), _ptr(high_vel))
        return high_pos, high_vel

    def clip_gather_low(self, high_pos, fps_idx, noise, jitter, vel, frame_first, count):
        T, B, K, _ = high_pos.shape
        M = fps_idx.shape[1]
        low_pos = torch.empty((T, B, M, 3), dtype=torch.float32, device=high_pos.device)
        low_vel = torch.empty_like(low_pos) if vel is not None else None
        self._call("tpg_clip_gather_low_f32", "clip_gather_low", (1 if vel is None else 2) * 24 * T * B * M, high_pos,
                   _ptr(high_pos), _ptr(fps_idx), _ptr(noise), float(jitter), _ptr(vel),
                   0 if vel is None else vel.shape[0], None if vel is None else frame_first.ctypes.data,
                   None if vel is None else count.ctypes.data, T, B, K, M, _ptr(low_pos), _ptr(low_vel))
        return low_pos, low_vel

    def frame_subset(self, count, seed, K, device):
        """tpg_frame_subset: count (F,) int32 / seed (F,) uint64 are host arrays (numpy); -> idx (F,K) int32 on `device`."""
        F = len(count)
        idx = torch.empty((F, K), dtype=torch.int32, device=device)
        self._call("tpg_frame_subset", "frame_subset", 4 * F * K, idx, count.ctypes.data, seed.ctypes.data, F, K, _ptr(idx))
        return idx

    def action_gather(self, points, frame_first, count, idx, scale, per_frame):
        """tpg_action_gather_f32: frame_first / count (T,B) int32 and scale (B,3) float64 (or None) are host arrays
        (numpy); per_frame selects the test split.  -> (high (T,B,K,3), centre (T,B,3) or None)."""
        T, B, K = idx.shape
        high = torch.empty((T, B, K, 3), dtype=torch.float32, device=points.device)
        centre = torch.empty((T, B, 3), dtype=torch.float32, device=points.device) if per_frame else None
        self._call("tpg_action_gather_f32", "action_gather", 28 * T * B * K, points,
                   _ptr(points), points.shape[0], frame_first.ctypes.data, count.ctypes.data, _ptr(idx),
                   None if scale is None else scale.ctypes.data, 1 if per_frame else 0, T, B, K, _ptr(high), _ptr(centre))
        return high, centre

    def fps(self, xyz, m, start=None, skip_origin=True):
        B, N, _ = xyz.shape
        idx = torch.empty((B, m), dtype=torch.int32, device=xyz.device)
        temp = torch.empty((B, N), dtype=torch.float32, device=xyz.device) if N > 16384 else None
        if start is None and skip_origin:
            self._call("tpg_fps_f32", "fps", 12 * B * N + 4 * B * m, xyz, _ptr(xyz), B, N, m, _ptr(temp), _ptr(idx))
        else:
            self._call("tpg_fps_start_f32", "fps", 12 * B * N + 4 * B * m, xyz, _ptr(xyz), _ptr(start),
                       int(bool(skip_origin)), B, N, m, _ptr(temp), _ptr(idx))
        return idx

    def gather_fwd(self, feat, idx):
        B, Cc, N = feat.shape
        S = idx.shape[1]
        out = torch.empty((B, Cc, S), dtype=torch.float32, device=feat.device)
        self._call("tpg_gather_fwd_f32", "gather_fwd", 4 * B * (Cc * N + S + Cc * S), feat,
                   _ptr(feat), _ptr(idx), B, Cc, N, S, _ptr(out))
        return out

    def gather_bwd(self, gout, idx, N):
        B, Cc, S = gout.shape
        g = torch.empty((B, Cc, N), dtype=torch.float32, device=gout.device)
        self._call("tpg_gather_bwd_f32", "gather_bwd", 4 * B * (Cc * N + S + Cc * S), gout,
                   _ptr(gout), _ptr(idx), B, Cc, N, S, _ptr(g))
        return g

    def gather_rows_fwd(self, rows, idx):
        B, N, Cc = rows.shape
        S = idx.shape[1]
        out = torch.empty((B, S, Cc), dtype=torch.float32, device=rows.device)
        self._call("tpg_gather_rows_fwd_f32", "gather_fwd", 4 * B * S * (2 * Cc + 1), rows,
                   _ptr(rows), _ptr(idx), B, N, S, Cc, _ptr(out))
        return out

    def gather_rows_bwd(self, gout, idx, N):
        B, S, Cc = gout.shape
        g = torch.empty((B, N, Cc), dtype=torch.float32, device=gout.device)
        self._call("tpg_gather_rows_bwd_f32", "gather_bwd", 4 * B * (Cc * N + S + 2 * Cc * S), gout,
                   _ptr(gout), _ptr(idx), B, N, S, Cc, _ptr(g))
        return g

    def ball_query(self, radius, nsample, xyz, new_xyz):
        B, N, _ = xyz.shape
        S = new_xyz.shape[1]
        idx = torch.empty((B, S, nsample), dtype=torch.int32, device=xyz.device)
        self._call("tpg_ball_query_f32", "ball_query", 12 * B * (N + S) + 4 * B * S * nsample, xyz,
                   _ptr(xyz), _ptr(new_xyz), B, N, S, float(radius), nsample, _ptr(idx))
        return idx

    def group_fwd(self, feat, idx):
        B, Cc, N = feat.shape
        _, S, K = idx.shape
        out = torch.empty((B, Cc, S, K), dtype=torch.float32, device=feat.device)
        self._call("tpg_group_fwd_f32", "group_fwd", 4 * B * (Cc * N + S * K + Cc * S * K), feat,
                   _ptr(feat), _ptr(idx), B, Cc, N, S, K, _ptr(out))
        return out

    def group_bwd(self, gout, idx, N):
        B, Cc, S, K = gout.shape
        g = torch.empty((B, Cc, N), dtype=torch.float32, device=gout.device)
        self._call("tpg_group_bwd_f32", "group_bwd", 4 * B * (Cc * N + S * K + Cc * S * K), gout,
                   _ptr(gout), _ptr(idx), B, Cc, N, S, K, _ptr(g))
        return g

    def three_nn(self, unknown, known):
        B, n, _ = unknown.shape
        m = known.shape[1]
        d2 = torch.empty((B, n, 3), dtype=torch.float32, device=unknown.device)
        idx = torch.empty((B, n, 3), dtype=torch.int32, device=unknown.device)
        self._call("tpg_three_nn_f32", "three_nn", 12 * B * (n + m) + 24 * B * n, unknown,
                   _ptr(unknown), _ptr(known), B, n, m, _ptr(d2), _ptr(idx))
        return d2, idx

    def three_interp_fwd(self, feat, idx, w):
        B, Cc, m = feat.shape
        n = idx.shape[1]
        out = torch.empty((B, Cc, n), dtype=torch.float32, device=feat.device)
        self._call("tpg_three_interp_fwd_f32", "three_interp_fwd", 4 * B * (Cc * m + 6 * n + Cc * n), feat,
                   _ptr(feat), _ptr(idx), _ptr(w), B, Cc, m, n, _ptr(out))
        return out

    def three_interp_bwd(self, gout, idx, w, m):
        B, Cc, n = gout.shape
        g = torch.empty((B, Cc, m), dtype=torch.float32, device=gout.device)
        self._call("tpg_three_interp_bwd_f32", "three_interp_bwd", 4 * B * (Cc * m + 6 * n + Cc * n), gout,
                   _ptr(gout), _ptr(idx), _ptr(w), B, Cc, m, n, _ptr(g))
        return g

    # ---- channels-last row combine (csrc/rowgather.hip) --------------------------------
    def rowcombine_fwd(self, U, QE, idx, mode, slope, out_dtype):
        B, N, Cc = U.shape
        _, S, K = idx.shape
        out = torch.empty((B, S, K, Cc), dtype=out_dtype, device=U.device)
        nbytes = (U.element_size() * B * Cc * (N + (S if QE is not None else 0)) + 4 * B * S * K
                  + out.element_size() * B * S * K * Cc)
        self._call("tpg_rowcombine_fwd", "rowcombine_fwd", nbytes, U,
                   _ptr(U), _ptr(QE), _ptr(idx), mode, _DTYPE_CODE[U.dtype], _DTYPE_CODE[out_dtype],
                   B, N, S, K, Cc, float(slope), _ptr(out))
        return out

    def invert_index(self, idx, N):
        B = idx.shape[0]
        SK = idx[0].numel()
        offs = torch.empty((B, N + 1), dtype=torch.int32, device=idx.device)
        lst = torch.empty((B, SK), dtype=torch.int32, device=idx.device)
        tmp = torch.empty((B, SK), dtype=torch.int32, device=idx.device) if N > 256 else None   # radix scratch
        self._call("tpg_invert_index", "invert_index", 4 * B * (2 * SK + N + 1), idx,
                   _ptr(idx), B, N, SK, _ptr(offs), _ptr(lst), _ptr(tmp))
        return offs, lst

    def rowcombine_bwd(self, gout, idx, E, mode, N, slope, in_dtype, inverse=None):
        B, S, K, Cc = gout.shape
        if inverse is None:
            inverse = self.invert_index(idx, N)
        offs, lst = inverse
        gU = torch.empty((B, N, Cc), dtype=in_dtype, device=gout.device)
        gQE = torch.empty((B, S, Cc), dtype=in_dtype, device=gout.device) if mode != 0 else None
        nbytes = (gout.element_size() * B * S * K * Cc * (2 if mode == 1 else 1) + 8 * B * S * K
                  + gU.element_size() * B * Cc * (N + (S if mode else 0)))
        self._call("tpg_rowcombine_bwd", "rowcombine_bwd", nbytes, gout,
                   _ptr(gout), _ptr(idx), _ptr(offs), _ptr(lst), _ptr(E), mode, _DTYPE_CODE[in_dtype],
                   _DTYPE_CODE[gout.dtype], B, N, S, K, Cc, float(slope), _ptr(gU), _ptr(gQE))
        return gU, gQE


    def rowcombine_edge_fwd(self, Y, idx, slope_a, slope_e, out_dtype):
        """Y (B,N,2C) = f [We; Wn]^T -> lrelu(Y[idx, C:], slope_a) + lrelu(Y[idx, :C] - Y[n, :C], slope_e), (B,N,K,C)."""
        B, N, C2 = Y.shape
        Cc, K = C2 // 2, idx.shape[2]
        out = torch.empty((B, N, K, Cc), dtype=out_dtype, device=Y.device)
        nbytes = Y.element_size() * B * N * C2 + 4 * B * N * K + out.element_size() * B * N * K * Cc
        self._call("tpg_rowcombine_edge_fwd", "rowcombine_fwd", nbytes, Y,
                   _ptr(Y), _ptr(idx), _DTYPE_CODE[Y.dtype], _DTYPE_CODE[out_dtype], B, N, K, Cc, float(slope_a),
                   float(slope_e), _ptr(out))
        return out

    def rowcombine_edge_bwd(self, gout, idx, Y, slope_a, slope_e, inverse=None):
        B, N, K, Cc = gout.shape
        if inverse is None:
            inverse = self.invert_index(idx, N)
        offs, lst = inverse
        gY = torch.empty_like(Y)
        nbytes = gout.element_size() * B * N * K * Cc * 2 + 8 * B * N * K + 2 * Y.element_size() * B * N * 2 * Cc
        self._call("tpg_rowcombine_edge_bwd", "rowcombine_bwd", nbytes, gout,
                   _ptr(gout), _ptr(idx), _ptr(offs), _ptr(lst), _ptr(Y), _DTYPE_CODE[Y.dtype], _DTYPE_CODE[gout.dtype],
                   B, N, K, Cc, float(slope_a), float(slope_e), _ptr(gY))
        return gY

    # ---- BatchNorm1d + LeakyReLU + dropout mask of a classification head (csrc/head.hip) ----
    def head_bn_act_fwd(self, h, gamma, beta, running_mean, running_var, nbt, momentum, eps, slope, mask):
        B, Cc = h.shape
        y = torch.empty_like(h)
        mean = torch.empty(Cc, dtype=torch.float32, device=h.device)
        rstd = torch.empty(Cc, dtype=torch.float32, device=h.device)
        self._call("tpg_head_bn_act_fwd", "head_bn_act", 4 * B * Cc * (3 if mask is not None else 2), h,
                   _ptr(h), B, Cc, _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), _ptr(nbt),
                   float(momentum), float(eps), float(slope), _ptr(mask), _ptr(y), _ptr(mean), _ptr(rstd))
        return y, mean, rstd

    def head_bn_act_bwd(self, gy, h, mean, rstd, gamma, beta, slope, mask, need_affine):
        B, Cc = h.shape
        dh = torch.empty_like(h)
        dg = torch.empty(Cc, dtype=torch.float32, device=h.device) if need_affine else None
        db = torch.empty(Cc, dtype=torch.float32, device=h.device) if need_affine else None
        self._call("tpg_head_bn_act_bwd", "head_bn_act_bwd", 4 * B * Cc * (4 if mask is not None else 3), h,
                   _ptr(gy), _ptr(h), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), float(slope), _ptr(mask), B, Cc,
                   _ptr(dh), _ptr(dg), _ptr(db))
        return dh, dg, db

    # ---- fused BatchNorm + LeakyReLU (+ max over K) on rows (csrc/rowbn.hip) -------------
    def _bn_ws(self, x, C_, nseg=1):
        need = self.lib.tpg_rowbn_workspace_bytes(max(C_, 256), max(nseg, 1)) // 4
        return self._workspace("rowbn", x, need, zeroed=True)

    def rowbn_fwd(self, x, K, eps, momentum, training, running_mean, running_var, gamma, beta, slope,
                  mean, rstd, out_dtype, num_batches_tracked=None, nseg=1, mean_shift=None):
        P, Cc = x.shape
        rows = P // K if K else P
        y = torch.empty((rows, Cc), dtype=out_dtype, device=x.device)
        arg = torch.empty((rows, Cc), dtype=torch.uint8, device=x.device) if K else None
        ws = self._bn_ws(x, Cc, nseg)
        args = (_ptr(x), _DTYPE_CODE[x.dtype], P, K, Cc, float(eps), float(momentum), int(training),
                _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked), _ptr(mean_shift), _ptr(gamma),
                _ptr(beta),
                float(slope), _ptr(mean),
                _ptr(rstd), _ptr(y), _DTYPE_CODE[out_dtype], _ptr(arg), _ptr(ws), int(nseg))
        b_stats = x.element_size() * P * Cc
        b_apply = x.element_size() * P * Cc + y.element_size() * rows * Cc + (rows * Cc if K else 0)
        if _timer is None:
            self._call("tpg_rowbn_fwd", "rowbn_fwd", b_stats + b_apply, x, *args, 0)
        else:       # time the reduction and the streaming kernel separately (one kernel each + finalize)
            if training:
                self._call("tpg_rowbn_fwd", "rowbn_fwd_stats", b_stats, x, *args, 1)
            self._call("tpg_rowbn_fwd", "rowbn_fwd_apply_max" if K else "rowbn_fwd_apply", b_apply, x, *args, 2)
        return y, arg

    def rowbn_bwd(self, gy, x, arg, K, training, mean, rstd, gamma, beta, slope, need_affine, y=None, nseg=1):
        P, Cc = x.shape
        dx = torch.empty_like(x)
        dgamma = torch.empty(Cc, dtype=torch.float32, device=x.device) if need_affine else None
        dbeta = torch.empty(Cc, dtype=torch.float32, device=x.device) if need_affine else None
        ws = self._bn_ws(x, Cc, nseg)
        if y is not None and (not K or y.dtype != gy.dtype):
            y = None
        args = (_ptr(gy), _DTYPE_CODE[gy.dtype], _ptr(x), _DTYPE_CODE[x.dtype], _ptr(arg), _ptr(y),
                _DTYPE_CODE[y.dtype] if y is not None else 0, P, K, Cc,
                int(training), _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta), float(slope), _ptr(dgamma),
                _ptr(dbeta), _ptr(dx), _ptr(ws), int(nseg))
        b_gy = gy.element_size() * gy.numel() + (gy.numel() if K else 0)
        b_reduce = (2 * gy.element_size() * gy.numel() if y is not None
                    else b_gy + x.element_size() * (gy.numel() if K else P * Cc))
        b_apply = b_gy + 2 * x.element_size() * P * Cc
        if _timer is None:
            self._call("tpg_rowbn_bwd", "rowbn_bwd", b_reduce + b_apply, x, *args, 0)
        else:
            self._call("tpg_rowbn_bwd", "rowbn_bwd_reduce", b_reduce, x, *args, 1)
            self._call("tpg_rowbn_bwd", "rowbn_bwd_apply", b_apply, x, *args, 2)
        return dx, dgamma, dbeta


    # ---- fused MLP tail layer on MFMA tiles (csrc/mlp_fused.hip) ---------------------------
    def _mlp_ws(self, x, C_, nseg):
        need = self.lib.tpg_mlp_workspace_bytes(max(C_, 256), max(nseg, 1)) // 4
        return self._workspace("mlp", x, need, zeroed=True)

    def mlp_fwd(self, x, ss_in, slope_in, W, nseg, eps=0.0, momentum=0.0, running_mean=None, running_var=None,
                num_batches_tracked=None, mean_shift=None, gamma_out=None, beta_out=None, stats=True, mean_rstd=False):
        """y = W . lrelu(sc * x + sh) on bf16 rows [+ batch statistics of y].
        ss_in: None (identity) or a tensor whose per-segment blocks START with sc | sh of the input
        BatchNorm -- (nseg,2,Cin) or a ci block (nseg,4,Cin).
        -> y (P,Cout) bf16, ci_out (nseg,4,Cout) = sc | sh | mu | rs of the OUTPUT BatchNorm (None if not stats)
        [, mean, rstd (nseg,Cout) as tensors of their own (mean_rstd: the finalize launch writes them anyway)]."""
        P, Cin = x.shape
        w_per_seg = int(W.dim() == 3 and W.shape[0] == nseg and nseg > 1)
        Cout = W.shape[-2]
        y = torch.empty((P, Cout), dtype=torch.bfloat16, device=x.device)
        ci_out = torch.empty((nseg, 4, Cout), dtype=torch.float32, device=x.device) if stats else None
        ws = self._mlp_ws(x, max(Cin, Cout), nseg)
        mr = torch.empty((2, nseg, Cout), dtype=torch.float32, device=x.device) if (stats and mean_rstd) else None
        ss_stride = 0 if ss_in is None else ss_in.shape[1] * ss_in.shape[2]
        self._call("tpg_mlp_fwd", "mlp_fwd", 2 * P * (Cin + Cout), x,
                   _ptr(x), P, Cin, Cout, nseg, _ptr(ss_in), ss_stride, float(slope_in), _ptr(W), w_per_seg, _ptr(y),
                   float(eps), float(momentum), _ptr(running_mean), _ptr(running_var), _ptr(num_batches_tracked),
                   _ptr(mean_shift), _ptr(gamma_out), _ptr(beta_out), _ptr(None if mr is None else mr[0]),
                   _ptr(None if mr is None else mr[1]), _ptr(ci_out), _ptr(ws), flops=2 * P * Cin * Cout)
        if mr is not None:
            return y, ci_out, mr[0], mr[1]
        return y, ci_out

    def mlp_infer(self, U, Q, idx, packed, scales, shifts, slopes):
        """One launch of the eval-mode tail (csrc/mlp_infer.hip): U (B,N,C0), Q (B,S,C0) fp32 or bf16, idx (B,S,K) int32,
        packed: the L bf16 weights in fragment order (`pack_infer_weight`), scales / shifts: L fp32 vectors,
        slopes: L+1 floats -> (B,S,C_L) bf16."""
        B, N, C0 = U.shape
        _, S, K = idx.shape
        L = len(packed)
        chans = [C0] + [int(a.numel()) for a in scales]
        out = torch.empty((B, S, chans[-1]), dtype=torch.bfloat16, device=U.device)
        nbytes = U.element_size() * B * C0 * (N + S) + 4 * B * S * K + 2 * B * S * chans[-1]
        flops = 2 * B * S * K * sum(a * b for a, b in zip(chans[:-1], chans[1:]))
        two = L == 2
        self._call("tpg_mlp_infer_fwd", "mlp_infer", nbytes, U,
                   _ptr(U), _ptr(Q), _ptr(idx), _DTYPE_CODE[U.dtype], B, N, S, K, C0, chans[1], chans[2] if two else 0,
                   _ptr(packed[0]), _ptr(packed[1] if two else None), _ptr(scales[0]), _ptr(shifts[0]),
                   _ptr(scales[1] if two else None), _ptr(shifts[1] if two else None),
                   float(slopes[0]), float(slopes[1]), float(slopes[2]) if two else 1.0, _ptr(out), flops=flops)
        return out

    def rowbn_stats(self, x, eps, momentum, running_mean, running_var, num_batches_tracked, nseg, mean_shift,
                    consts=None):
        """Training-mode batch statistics of x (P,C) alone (the reduction half of rowbn_fwd): mean, rstd
        (nseg,C); running statistics / batch counter updated like nn.BatchNorm's forward.
        consts = (gamma, beta): also ci (nseg,4,C) = sc | sh | mu | rs from the same finalize launch -> (mean, rstd, ci)."""
        P, Cc = x.shape
        mean = torch.empty((nseg, Cc), dtype=torch.float32, device=x.device)
        rstd = torch.empty((nseg, Cc), dtype=torch.float32, device=x.device)
        ws = self._bn_ws(x, Cc, nseg)
        if consts is not None:
            ci = torch.empty((nseg, 4, Cc), dtype=torch.float32, device=x.device)
            self._call("tpg_rowbn_stats_consts", "rowbn_fwd_stats", x.element_size() * P * Cc, x,
                       _ptr(x), _DTYPE_CODE[x.dtype], P, Cc, float(eps), float(momentum), _ptr(running_mean),
                       _ptr(running_var), _ptr(num_batches_tracked), _ptr(mean_shift), _ptr(consts[0]), _ptr(consts[1]),
                       _ptr(mean), _ptr(rstd), _ptr(ci), _ptr(ws), int(nseg))
            return mean, rstd, ci
        self._call("tpg_rowbn_fwd", "rowbn_fwd_stats", x.element_size() * P * Cc, x,
                   _ptr(x), _DTYPE_CODE[x.dtype], P, 0, Cc, float(eps), float(momentum), 1, _ptr(running_mean),
                   _ptr(running_var), _ptr(num_batches_tracked), _ptr(mean_shift), None, None, 1.0, _ptr(mean),
                   _ptr(rstd), _ptr(x), _DTYPE_CODE[x.dtype], None, _ptr(ws), int(nseg), 1)
        return mean, rstd

    def rowbn_apply_max(self, x, K, mean, rstd, gamma, beta, slope, out_dtype, nseg):
        """The streaming half of rowbn_fwd with GIVEN training-mode statistics: lrelu(BN(x)) [+ max over K]."""
        P, Cc = x.shape
        rows = P // K if K else P
        y = torch.empty((rows, Cc), dtype=out_dtype, device=x.device)
        arg = torch.empty((rows, Cc), dtype=torch.uint8, device=x.device) if K else None
        ws = self._bn_ws(x, Cc, nseg)
        self._call("tpg_rowbn_fwd", "rowbn_fwd_apply_max" if K else "rowbn_fwd_apply",
                   x.element_size() * P * Cc + y.element_size() * rows * Cc + (rows * Cc if K else 0), x,
                   _ptr(x), _DTYPE_CODE[x.dtype], P, K, Cc, 0.0, 0.0, 1, None, None, None, None, _ptr(gamma), _ptr(beta),
                   float(slope), _ptr(mean), _ptr(rstd), _ptr(y), _DTYPE_CODE[out_dtype], _ptr(arg), _ptr(ws), int(nseg), 2)
        return y, arg

    def rowbn_bwd_sums(self, gy, x, arg, y, K, mean, rstd, gamma, beta, slope, need_affine, nseg, want_cb=False):
        """Backward sums of a training-mode BatchNorm (+LeakyReLU, + max over K): c12 (nseg,2,C) and, if
        wanted, dgamma / dbeta [want_cb: and cb (nseg,4,C) = a | f*mu | e | f from the same finalize launch, and ag =
        mlp_max_prep's output (or None where the reduction cannot make it: no y of gy's type), appended]."""
        P, Cc = x.shape
        c12 = torch.empty((nseg, 2, Cc), dtype=torch.float32, device=x.device)
        dgamma = torch.empty(Cc, dtype=torch.float32, device=x.device) if need_affine else None
        dbeta = torch.empty(Cc, dtype=torch.float32, device=x.device) if need_affine else None
        ws = self._bn_ws(x, Cc, nseg)
        if y is not None and (not K or y.dtype != gy.dtype):
            y = None
        if want_cb:
            cb = torch.empty((nseg, 4, Cc), dtype=torch.float32, device=x.device)
            ag = torch.empty_like(gy) if (K and y is not None) else None
            self._call("tpg_rowbn_bwd_sums_consts", "rowbn_bwd_reduce", (3 if ag is not None else 2) * gy.element_size() * gy.numel(), x,
                       _ptr(gy), _DTYPE_CODE[gy.dtype], _ptr(x), _DTYPE_CODE[x.dtype], _ptr(arg), _ptr(y),
                       _DTYPE_CODE[y.dtype] if y is not None else 0, P, K, Cc, 1, _ptr(mean), _ptr(rstd), _ptr(gamma),
                       _ptr(beta), float(slope), _ptr(dgamma), _ptr(dbeta), _ptr(c12), _ptr(cb), _ptr(ag), _ptr(ws), int(nseg))
            return c12, dgamma, dbeta, cb, ag
        self._call("tpg_rowbn_bwd_sums", "rowbn_bwd_reduce", 2 * gy.element_size() * gy.numel(), x,
                   _ptr(gy), _DTYPE_CODE[gy.dtype], _ptr(x), _DTYPE_CODE[x.dtype], _ptr(arg), _ptr(y),
                   _DTYPE_CODE[y.dtype] if y is not None else 0, P, K, Cc, 1, _ptr(mean), _ptr(rstd), _ptr(gamma),
                   _ptr(beta), float(slope), _ptr(dgamma), _ptr(dbeta), _ptr(c12), _ptr(ws), int(nseg))
        return c12, dgamma, dbeta

    def mlp_consts(self, mean, rstd, gamma, beta, c12, want_ci, want_cb):
        nseg, Cc = mean.shape
        ci = torch.empty((nseg, 4, Cc), dtype=torch.float32, device=mean.device) if want_ci else None
        cb = torch.empty((nseg, 4, Cc), dtype=torch.float32, device=mean.device) if want_cb else None
        self._call("tpg_mlp_consts", "mlp_consts", 32 * nseg * Cc, mean, _ptr(mean), _ptr(rstd), _ptr(gamma), _ptr(beta),
                   _ptr(c12), Cc, nseg, _ptr(ci), _ptr(cb))
        return ci, cb

    def mlp_max_prep(self, gout, y, cb_out, slope_out, nseg):
        """a * lrelu'(y) * gout per (group, channel): the MODE_MAX operand of mlp_dgrad / mlp_wgrad."""
        rows, Cc = gout.shape
        ag = torch.empty_like(gout)
        self._call("tpg_mlp_max_prep", "mlp_max_prep", 6 * rows * Cc, gout, _ptr(gout), _ptr(y), _ptr(cb_out),
                   float(slope_out), rows, Cc, nseg, _ptr(ag))
        return ag

    def mlp_dgrad(self, x_out, g_out, arg, K, cb_out, x_in, ci_in, slope_in, W, nseg, need_affine, sums=True):
        """-> g_in (P,Cin) bf16, c12_in (nseg,2,Cin), cb_in (nseg,4,Cin), dgamma_in, dbeta_in
        (sums=False: BN_in is the identity -- nothing but g_in)."""
        P, Cout = x_out.shape
        Cin = x_in.shape[1]
        mode = 1 if arg is not None else 0
        w_per_seg = int(W.dim() == 3 and W.shape[0] == nseg and nseg > 1)
        dev = x_out.device
        g_in = torch.empty((P, Cin), dtype=torch.bfloat16, device=dev)
        c12 = torch.empty((nseg, 2, Cin), dtype=torch.float32, device=dev) if sums else None
        cb_in = torch.empty((nseg, 4, Cin), dtype=torch.float32, device=dev) if sums else None
        dgamma = torch.empty(Cin, dtype=torch.float32, device=dev) if (need_affine and sums) else None
        dbeta = torch.empty(Cin, dtype=torch.float32, device=dev) if (need_affine and sums) else None
        ws = self._mlp_ws(x_out, max(Cin, Cout), nseg)
        self._call("tpg_mlp_dgrad", "mlp_dgrad", 2 * P * (Cout + 2 * Cin) + (0 if mode else 2 * P * Cout), x_out,
                   _ptr(x_out), _ptr(g_out), _ptr(arg), int(K), _ptr(cb_out), _ptr(x_in), _ptr(ci_in),
                   float(slope_in), _ptr(W), w_per_seg, P, Cin, Cout, nseg, mode, _ptr(g_in), _ptr(c12), _ptr(dgamma),
                   _ptr(dbeta), _ptr(cb_in), _ptr(ws), flops=2 * P * Cin * Cout)
        return g_in, c12, cb_in, dgamma, dbeta

    def mlp_wgrad(self, x_out, g_out, arg, K, cb_out, x_in, ci_in, slope_in, nseg):
        """-> dW (nseg,Cout,Cin) f32."""
        P, Cout = x_out.shape
        Cin = x_in.shape[1]
        mode = 1 if arg is not None else 0
        dW = torch.empty((nseg, Cout, Cin), dtype=torch.float32, device=x_out.device)
        ws = self._workspace("wgrad", x_out, self.lib.tpg_mlp_wgrad_workspace_bytes(P, Cin, Cout, nseg) // 4)
        self._call("tpg_mlp_wgrad", "mlp_wgrad", 2 * P * (Cout + Cin) + (0 if mode else 2 * P * Cout), x_out,
                   _ptr(x_out), _ptr(g_out), _ptr(arg), int(K), _ptr(cb_out), _ptr(x_in), _ptr(ci_in),
                   float(slope_in), P, Cin, Cout, nseg, mode, _ptr(dW), _ptr(ws), flops=2 * P * Cin * Cout)
        return dW

    def small_tail_fwd(self, h, W1, W2, s1, s2, K):
        """h (P*K, 16) bf16 / f32 -> out (P, 32) of h's dtype, arg (P, 32) u8 (csrc/mlp_small.hip)."""
        E, H = h.shape
        P = E // K
        C1, C2 = W1.shape[0], W2.shape[0]
        out = torch.empty((P, C2), dtype=h.dtype, device=h.device)
        arg = torch.empty((P, C2), dtype=torch.uint8, device=h.device)
        self._call("tpg_small_tail_fwd", "small_tail_fwd", h.element_size() * (E * H + P * C2) + P * C2, h,
                   _ptr(h), 1 if h.dtype == torch.bfloat16 else 0, _ptr(W1), _ptr(W2), float(s1), float(s2), P, int(K),
                   H, C1, C2, _ptr(out), _ptr(arg), flops=2 * E * (H * C1 + C1 * C2))
        return out, arg

    def small_tail_bwd(self, h, out, gout, arg, W1, W2, s1, s2, K):
        """-> gh (P*K, 16) of h's dtype, dW1 (16,16) f32, dW2 (32,16) f32."""
        E, H = h.shape
        P = E // K
        C1, C2 = W1.shape[0], W2.shape[0]
        gh = torch.empty_like(h)
        dW1 = torch.empty((C1, H), dtype=torch.float32, device=h.device)
        dW2 = torch.empty((C2, C1), dtype=torch.float32, device=h.device)
        ws = self._workspace("small_tail", h, max(16, self.lib.tpg_small_tail_workspace_bytes(P, int(K)) // 4))
        self._call("tpg_small_tail_bwd", "small_tail_bwd", h.element_size() * (2 * E * H + 2 * P * C2) + P * C2, h,
                   _ptr(h), _ptr(out), _ptr(gout), _ptr(arg), 1 if h.dtype == torch.bfloat16 else 0, _ptr(W1), _ptr(W2),
                   float(s1), float(s2), P, int(K), H, C1, C2, _ptr(gh), _ptr(dW1), _ptr(dW2), _ptr(ws),
                   flops=2 * E * (2 * H * C1 + 2 * C1 * C2 + H * C1))
        return gh, dW1, dW2

    def mlp_bn_bwd_apply(self, g, x, ci, c12, nseg, K=0):
        """dx of the tail's first BatchNorm; K > 0: also qneg (P/K, C) f32 = -sum over each group of K rows of dx
        (the ROW_SUB gather's gradient of Q, see _GatherMlpTail.backward) -> (dx, qneg)."""
        P, Cc = x.shape
        dx = torch.empty_like(x)
        if K:
            qneg = torch.empty((P // K, Cc), dtype=torch.float32, device=x.device)
            self._call("tpg_mlp_bn_bwd_apply_rowsum", "mlp_bn_bwd_apply", 6 * P * Cc + 4 * (P // K) * Cc, x, _ptr(g),
                       _ptr(x), _ptr(ci), _ptr(c12), P, K, Cc, nseg, _ptr(dx), _ptr(qneg))
            return dx, qneg
        self._call("tpg_mlp_bn_bwd_apply", "mlp_bn_bwd_apply", 6 * P * Cc, x, _ptr(g), _ptr(x), _ptr(ci), _ptr(c12), P,
                   Cc, nseg, _ptr(dx))
        return dx

    # ---- fused spectral norm (csrc/spectral.hip) ------------------------------------------
    def spectral_norm_fwd(self, W, u, v, iterate, eps):
        R, Cn = W.shape
        Wsn = torch.empty_like(W)
        sigma = torch.empty(1, dtype=torch.float32, device=W.device)
        self._call("tpg_spectral_norm_fwd", "spectral_norm_fwd", 4 * (2 * R * Cn + 2 * (R + Cn)), W,
                   _ptr(W), _ptr(u), _ptr(v), R, Cn, int(iterate), float(eps), _ptr(Wsn), _ptr(sigma))
        return Wsn, sigma

    def spectral_norm_bwd(self, G, Wsn, u, v, sigma):
        R, Cn = Wsn.shape
        dW = torch.empty_like(Wsn)
        self._call("tpg_spectral_norm_bwd", "spectral_norm_bwd", 4 * 3 * R * Cn, G,
                   _ptr(G), _ptr(Wsn), _ptr(u), _ptr(v), _ptr(sigma), R, Cn, _ptr(dW))
        return dW


    def _sn_plan(self, Ws, us, vs, uses):
        """Static description of a batched spectral-norm call (cached per parameter set): device
        descriptor arrays for forward and backward + buffer layouts.  Nothing in it depends on a
        per-call allocation, so no host->device copy happens after the first call (capture-safe)."""
        key = tuple(t.data_ptr() for t in (*Ws, *us, *vs)) + tuple(uses)
        plan = self._sn_plans.get(key)
        if plan is None:
            _need(max(int(n) for n in uses) <= 64, "at most 64 uses of one spectrally-normalised weight per forward")
            dev = Ws[0].device
            fwd, bwd, layout, goffs, dwoffs = [], [], [], [], []
            out_total = g_total = dw_total = 0
            for W, u, v, n in zip(Ws, us, vs, uses):
                R, Cn = W.shape
                st = sn_multi_stride(R, Cn)
                fwd += [W.data_ptr(), u.data_ptr(), v.data_ptr(), R, Cn, n, out_total]
                bwd += [R, Cn, n, out_total, g_total, dw_total]
                layout.append((out_total, st))
                goffs.append(g_total)
                dwoffs.append(dw_total)
                out_total += st * n
                g_total += R * Cn * n
                dw_total += R * Cn
            # split form (training mode, csrc/spectral.hip): rows of a weight over several workgroups, one exchange per use
            rows, split = self.lib.tpg_spectral_norm_split_rows(), None
            if (SN_SPLIT[0] and max(W.shape[1] for W in Ws) <= self.lib.tpg_spectral_norm_split_max_cn()
                    and max(W.shape[0] for W in Ws) <= self.lib.tpg_spectral_norm_split_max_rows()):
                sd, pmap, words, off = [], [], 0, 0
                for m, (W, u, v, n) in enumerate(zip(Ws, us, vs, uses)):
                    R, Cn = W.shape
                    parts = (R + rows - 1) // rows
                    sd += [W.data_ptr(), u.data_ptr(), v.data_ptr(), R, Cn, n, off, parts, words]
                    pmap += [(m, g) for g in range(parts)]
                    words += 2 * parts * (Cn + 1)
                    off += sn_multi_stride(R, Cn) * n
                words = (words + 1 + 1) & ~1                      # + the timeout word, whole 16-byte units
                split = dict(desc=torch.tensor(sd, dtype=torch.int64).to(dev),
                             pmap=torch.tensor(pmap, dtype=torch.int32).to(dev).contiguous(), parts=len(pmap),
                             xws=torch.zeros(words, dtype=torch.int64, device=dev), words=words,
                             max_cn=max(W.shape[1] for W in Ws))
            plan = dict(split=split,
                        fwd=torch.tensor(fwd, dtype=torch.int64).to(dev), bwd=torch.tensor(bwd, dtype=torch.int64).to(dev),
                        layout=layout, goffs=goffs, dwoffs=dwoffs, out_total=out_total, g_total=g_total,
                        dw_total=dw_total, max_rc=max(W.shape[0] + W.shape[1] for W in Ws), M=len(Ws),
                        max_uses=max(int(n) for n in uses))
            self._sn_plans[key] = plan
        return plan

    # ---- row-wise linear layers of any small channel count (csrc/rowlinear.hip) -------------
    def rowlinear_fwd(self, x, W, bias, nseg, slope, out_dtype):
        P, Cin = x.shape
        Cout = W.shape[-2]
        y = torch.empty((P, Cout), dtype=out_dtype, device=x.device)
        self._call("tpg_rowlinear_fwd", "rowlinear_fwd", x.element_size() * P * Cin + y.element_size() * P * Cout + 4 * W.numel(), x,
                   _ptr(x), _DTYPE_CODE[x.dtype], _ptr(W), _ptr(bias), P, int(nseg), Cin, Cout, float(slope), _ptr(y),
                   _DTYPE_CODE[out_dtype], flops=2 * P * Cin * Cout)
        return y

    def rowlinear_dgrad(self, gy, y, W, nseg, slope, x_dtype):
        P, Cout = gy.shape
        Cin = W.shape[-1]
        dx = torch.empty((P, Cin), dtype=x_dtype, device=gy.device)
        self._call("tpg_rowlinear_dgrad", "rowlinear_dgrad", gy.element_size() * P * Cout * (2 if y is not None else 1)
                   + dx.element_size() * P * Cin + 4 * W.numel(), gy,
                   _ptr(gy), _ptr(y), _DTYPE_CODE[gy.dtype], _ptr(W), P, int(nseg), Cin, Cout, float(slope), _ptr(dx),
                   _DTYPE_CODE[x_dtype], flops=2 * P * Cin * Cout)
        return dx

    def rowlinear_wgrad(self, x, gy, y, nseg, slope, need_bias):
        P, Cin = x.shape
        Cout = gy.shape[1]
        dW = torch.empty((nseg, Cout, Cin), dtype=torch.float32, device=x.device)
        db = torch.empty(Cout, dtype=torch.float32, device=x.device) if need_bias else None
        need = self.lib.tpg_rowlinear_wgrad_workspace_bytes(P, int(nseg), Cin, Cout, int(bool(need_bias))) // 4 + 4
        ws = self._workspace("rowlinear", x, need)
        self._call("tpg_rowlinear_wgrad", "rowlinear_wgrad", x.element_size() * P * Cin + gy.element_size() * P * Cout
                   * (2 if y is not None else 1), x,
                   _ptr(x), _DTYPE_CODE[x.dtype], _ptr(gy), _ptr(y), _DTYPE_CODE[gy.dtype], P, int(nseg), Cin, Cout,
                   float(slope), _ptr(dW), _ptr(db), _ptr(ws), flops=2 * P * Cin * Cout)
        return dW, db

    def spectral_norm_multi_fwd(self, Ws, us, vs, uses, iterate, eps):
        """-> (flat output buffer, plan); output layout in include/tpgan_ops.h."""
        plan = self._sn_plan(Ws, us, vs, uses)
        out = torch.empty(plan["out_total"], dtype=torch.float32, device=Ws[0].device)
        nbytes = 4 * sum((1 + n) * W.numel() for W, n in zip(Ws, uses))
        sp = plan["split"]
        if iterate and sp is not None:
            self._call("tpg_spectral_norm_multi_fwd_split", "spectral_norm_fwd", nbytes, out,
                       _ptr(sp["desc"]), _ptr(sp["pmap"]), sp["parts"], sp["max_cn"], _ptr(out), _ptr(sp["xws"]),
                       sp["words"], float(eps))
            return out, plan
        self._call("tpg_spectral_norm_multi_fwd", "spectral_norm_fwd", nbytes, out,
                   _ptr(plan["fwd"]), plan["M"], plan["max_rc"], _ptr(out), int(iterate), float(eps))
        return out, plan

    def spectral_norm_multi_bwd(self, out, plan, gflat):
        dw = torch.empty(plan["dw_total"], dtype=torch.float32, device=out.device)
        maxu = plan["max_uses"]
        scratch = torch.empty(self.lib.tpg_spectral_norm_multi_bwd_scratch(plan["M"], maxu), dtype=torch.float32,
                              device=out.device)
        self._call("tpg_spectral_norm_multi_bwd", "spectral_norm_bwd", 4 * (3 * plan["g_total"] + plan["dw_total"]),
                   out, _ptr(plan["bwd"]), plan["M"], maxu, _ptr(gflat), _ptr(out), _ptr(dw), _ptr(scratch))
        return dw


# spectral norm of a forward's weights with every weight's rows split over several workgroups (False: the
# one-workgroup-per-weight kernel; set by tests and tools/tune_sn.py)
SN_SPLIT = [True]


def sn_multi_stride(R, Cn):
    return (R * Cn + R + Cn + 1 + 3) & ~3


_DTYPE_CODE = {torch.float32: 0, torch.bfloat16: 1}
_hip = None


def backend_for(t):
    global _hip
    if t.is_cuda:
        if _hip is None:
            _hip = HipBackend()  # raises HipLibraryMissing loudly if the .so is absent
        return _hip
    impl = _BACKENDS.get(t.device.type)
    if impl is None:
        raise RuntimeError(
            f"tpgan_amd ops: {t.device.type} tensors are not supported (HIP only); "
            "the product has no CPU fallback")
    return impl


# ----------------------------------------------------------------- validation
def _need(cond, msg):
    if not cond:
        raise RuntimeError(msg)


def _check_float(t, name, ndim):
    _need(isinstance(t, torch.Tensor), f"{name} must be a tensor")
    _need(t.dim() == ndim, f"{name} must have {ndim} dims, got {tuple(t.shape)}")
    _need(t.dtype == torch.float32, f"{name} must be a float tensor, got {t.dtype}")
    _need(t.is_contiguous(), f"{name} must be a contiguous tensor")


def _check_int(t, name, ndim):
    _need(isinstance(t, torch.Tensor), f"{name} must be a tensor")
    _need(t.dim() == ndim, f"{name} must have {ndim} dims, got {tuple(t.shape)}")
    _need(t.dtype == torch.int32, f"{name} must be an int tensor, got {t.dtype}")
    _need(t.is_contiguous(), f"{name} must be a contiguous tensor")


def _same_device(*ts):
    d = ts[0].device
    for t in ts[1:]:
        _need(t.device == d, "all tensors must be on the same device")


# --------------------------------------------------------- pointnet2-style ops
def furthest_point_sample(xyz, npoint):
    """(B,N,3) fp32 -> (B,npoint) int32.  Reference call site discriminator.py:114."""
    _check_float(xyz, "xyz", 3)
    _need(xyz.shape[2] == 3, "xyz must be (B,N,3)")
    _need(int(npoint) > 0 and xyz.shape[1] > 0, "npoint and N must be positive")
    with torch.no_grad():
        return backend_for(xyz).fps(xyz.detach(), int(npoint))


def furthest_point_sample_prefix(xyz, npoint, prefix_flag=None):
    """`furthest_point_sample` for a chain of set-abstraction levels: -> (idx (B,npoint) int32, flag (B,) int32).
    `prefix_flag` = the flag returned by the call that sampled the centres `xyz` consists of (xyz must be those centres
    in pick order): clouds whose flag is set are answered with 0..npoint-1 at once -- the exact result, see
    csrc/fps.hip -- the others by the full algorithm.  Backends without the entry fall back to the plain op."""
    _check_float(xyz, "xyz", 3)
    _need(xyz.shape[2] == 3 and int(npoint) > 0 and xyz.shape[1] > 0, "xyz must be (B,N,3), npoint and N positive")
    be = backend_for(xyz)
    with torch.no_grad():
        if hasattr(be, "fps_prefix"):
            return be.fps_prefix(xyz.detach(), int(npoint), prefix_flag)
        return be.fps(xyz.detach(), int(npoint)), None


# ------------------------------------ dummy-centre replacement on the device (csrc/dummy_centres.hip)
_U32 = 0xFFFFFFFF


def _mix32(h):
    """include/tpgan_ops.h's mix on int64 tensors that hold uint32 values (int64 products wrap; the low words are right)."""
    h = h ^ (h >> 16)
    h = (h * 0x7FEB352D) & _U32
    h = h ^ (h >> 15)
    h = (h * 0x846CA68B) & _U32
    return h ^ (h >> 16)


def _replace_dummy_centres_torch(xyz, centres, draw_key, site, prefix_flag=None):
    """`replace_dummy_centres` composed of torch ops (backends without the kernel): the rule of include/tpgan_ops.h,
    cloud by cloud (it reads the hit counts on the host, which the kernel never does)."""
    B, N, _ = xyz.shape
    S = centres.shape[1]
    dev = xyz.device
    hit = torch.abs(torch.gather(xyz[:, :, 0], 1, centres.long()) - 999) < 1e-4
    out = centres.clone()
    short = torch.zeros((1,), dtype=torch.int32, device=dev)
    seed, n_iter = draw_key[0], draw_key[1]
    j = torch.arange(N, dtype=torch.int64, device=dev)
    lo = _mix32((seed & _U32) ^ _mix32((((n_iter & _U32) * 0x9E3779B1) + site) & _U32))
    for b, k in enumerate(hit.sum(1).tolist()):
        if k == 0:
            continue
        pool = torch.ones(N, dtype=torch.bool, device=dev)
        pool[:S] = ~hit[b, :N]
        if int(pool.sum()) < k:
            short[0] = 1
            continue
        hi = _mix32(((seed >> 32) & _U32) ^ _mix32((b * 0x85EBCA6B + site) & _U32))
        key = _mix32(_mix32((j * 0x9E3779B1 + lo) & _U32) ^ hi)
        picks = j[pool][torch.argsort(key[pool])[:k]]      # key() is a bijection: distinct keys, j never decides
        out[b] = torch.cat((centres[b][~hit[b]], picks.to(centres.dtype)))
        if prefix_flag is not None:
            prefix_flag[b] = 0
    return out, short


def replace_dummy_centres(xyz, centres, draw_key, site, prefix_flag=None):
    """The discriminators' dummy-centre replacement (discriminator.py:115-130) with no host involvement: centres that
    point at a 999-padded row of their cloud are dropped, the survivors keep their order and as many other points,
    drawn by tpg_frame_subset's keyed order, follow them (the rule: include/tpgan_ops.h).

    xyz (B,N,3) fp32, centres (B,S) int32; draw_key: a DEVICE int64 tensor (2,) holding [seed, n_iter], read
    by the kernel (a captured step rewrites it before each replay); site: a host int >= 0, the ordinal of the call within
    the step.  prefix_flag: the (B,) int32 flags of `furthest_point_sample_prefix` or None; cleared IN PLACE for every
    cloud whose centres were replaced.  -> (centres_out (B,S) int32, short (1,) int32: set if a cloud had fewer
    candidates than dummies -- where the reference's choice() raises -- and kept its row)."""
    _check_float(xyz, "xyz", 3)
    _check_int(centres, "centres", 2)
    _need(xyz.shape[2] == 3 and centres.shape[0] == xyz.shape[0], "xyz must be (B,N,3) and centres (B,S)")
    _need(xyz.shape[1] > 0 or centres.shape[1] == 0, "an empty cloud has no centres")
    _need(isinstance(draw_key, torch.Tensor) and draw_key.dtype == torch.int64 and tuple(draw_key.shape) == (2,)
          and draw_key.is_contiguous(), "draw_key must be an int64 tensor [seed, n_iter]")
    _need(int(site) >= 0, "site must be >= 0")
    _same_device(xyz, centres, draw_key)
    if prefix_flag is not None:
        _check_int(prefix_flag, "prefix_flag", 1)
        _need(prefix_flag.shape[0] == xyz.shape[0], "prefix_flag must hold one flag per cloud")
        _same_device(xyz, prefix_flag)
    if centres.numel() == 0:
        return centres.clone(), torch.zeros((1,), dtype=torch.int32, device=xyz.device)
    be = backend_for(xyz)
    with torch.no_grad():
        if hasattr(be, "replace_dummy_centres"):
            if xyz.is_cuda:
                _need(centres.shape[1] <= frame_subset_max_k(),
                      f"S = {centres.shape[1]} exceeds the selection's capacity ({frame_subset_max_k()})")
            return be.replace_dummy_centres(xyz.detach(), centres, draw_key, int(site), prefix_flag)
        return _replace_dummy_centres_torch(xyz.detach(), centres, draw_key, int(site), prefix_flag)


# --------------------------------------------------- rollout: running mask average (upsampling_network.py:159-174)
CONTEXT_WINDOW = 25            # frames in the reference's running mask average
CONTEXT_NONE = -2 ** 31        # state value "no such frame" (TPG_CTX_NONE)


def context_state(N, device):
    """The (2, N) int32 rollout state of a fresh sequence: no frame with a hit, no frame with a NaN."""
    return torch.full((2, N), CONTEXT_NONE, dtype=torch.int32, device=device)


def context_keep(mask, state, t0):
    """Keep decisions of T frames (t0 .. t0+T-1) from the raw masks (T, N) and the carried state (torch ops; updates
    `state` in place) -> (T, N) bool.  keep_t(i) <=> a frame of the window [t-24, t] has m >= 0.6 and none has NaN:
    what the reference's clamp to {0, 0.6}, 25-frame mean and `> 0.01` decide (0.6 / 25 > 0.01, NaN poisons the mean)."""
    T = mask.shape[0]
    t = torch.arange(t0, t0 + T, dtype=torch.int32, device=mask.device).view(T, 1)
    none = torch.full_like(mask, CONTEXT_NONE, dtype=torch.int32)
    hit = torch.cummax(torch.cat([state[:1], torch.where(mask >= 0.6, t, none)]), 0).values[1:]
    nan = torch.cummax(torch.cat([state[1:], torch.where(torch.isnan(mask), t, none)]), 0).values[1:]
    lo = t - (CONTEXT_WINDOW - 1)
    state.copy_(torch.stack([hit[-1], nan[-1]]))
    return (hit >= lo) & (nan < lo)


def _context_expand_torch(pos, edge, mask, state, t0):
    """`context_expand` composed of torch ops (backends without the fused kernel): the reference's
    expand_pos_with_masking(hard_masking=True) per frame on the keep decisions of `context_keep`."""
    T, N, _ = pos.shape
    r = edge.shape[1] // N
    keep = context_keep(mask, state, t0).view(T, N, 1)
    expanded = pos.repeat(1, 1, r).view(T, -1, 3) + (edge.view(T, N, 3 * r) * keep.float()).view(T, -1, 3)
    hard = keep.repeat(1, 1, r)
    hard[:, :, 0] = True
    counts = hard.view(T, -1).sum(1)
    offsets = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])
    return expanded[hard.view(T, -1)], offsets


def context_expand(pos, edge, mask, state, t0):
    """Hard-masked position expansion of T consecutive frames of one rollout with the reference's 25-frame running
    mask average (upsampling_network.py:159-174), all frames at once.

    pos (T,N,3), edge (T,N*r,3), mask (T,N) raw mask-head outputs, fp32; state (2,N) int32 from `context_state`,
    updated in place (carry it to the next call with t0 advanced by T); t0 = index of the chunk's first frame in the
    sequence.  -> (points (P,3), offsets (T+1,) int64 on the device): frame t's surviving points are
    points[offsets[t]:offsets[t+1]], point-major, slot-minor, as the reference's `expanded[hard]`."""
    _check_float(pos, "pos", 3)
    _check_float(edge, "edge", 3)
    _check_int(state, "state", 2)
    if mask.dim() == 3 and mask.shape[2] == 1:
        mask = mask.view(mask.shape[0], mask.shape[1])
    _check_float(mask, "mask", 2)
    _same_device(pos, edge, mask, state)
    T, N, _ = pos.shape
    _need(pos.shape[2] == 3 and edge.shape[2] == 3, "pos and edge must hold 3-D points")
    _need(N > 0 and edge.shape[0] == T and edge.shape[1] % N == 0, "edge must be (T, N*r, 3)")
    _need(tuple(mask.shape) == (T, N) and tuple(state.shape) == (2, N), "mask must be (T, N) and state (2, N)")
    _need(2 <= edge.shape[1] // N <= 16, "upsampling ratio must be 2..16")
    _need(int(t0) >= 0, "t0 must be >= 0")
    be = backend_for(pos)
    with torch.no_grad():
        if hasattr(be, "context_expand"):
            return be.context_expand(pos.detach(), edge.detach(), mask.detach(), state, int(t0))
        return _context_expand_torch(pos.detach(), edge.detach(), mask.detach(), state, int(t0))


# ------------------------------------------- training clips from device-resident sequences (csrc/clip_sample.hip)
PATCH_SELECT_NAN_KEY = 0x7FC00000      # the bit pattern every NaN distance ranks as (after +inf)
CLIP_MAX_T = 8                         # frames per clip the gathers take: csrc/tpg_select.hpp's TPG_CLIP_MAX_T says the same


def _host_ints(a, name, shape):
    """A small per-clip table kept on the HOST (list / numpy / CPU tensor) -> contiguous int32 numpy array."""
    if isinstance(a, torch.Tensor):
        _need(not a.is_cuda, f"{name} is a host table (the sampler draws it on the host): pass a CPU tensor or a list")
        a = a.numpy()
    a = np.asarray(a)
    _need(a.dtype.kind in "iu", f"{name} must hold integers, got {a.dtype}")
    _need(a.ndim == len(shape) and all(s in (None, n) for s, n in zip(shape, a.shape)),    # None: any extent, the table's
          f"{name} must have shape {tuple(shape)}, got {a.shape}")
    _need(a.size == 0 or (a.min() >= -2 ** 31 and a.max() < 2 ** 31), f"{name} does not fit int32")
    return np.ascontiguousarray(a, dtype=np.int32)


def _check_frames(first, count, rows, what):
    """Every frame (scene) is a non-empty slice of the `rows` stored rows of `what`; count broadcasts over first."""
    _need(bool((count > 0).all() and (first >= 0).all() and (first.astype(np.int64) + count <= rows).all()),
          f"every frame must be a non-empty slice of {what}")


def _patch_select_torch(points, first, count, seed, K):
    """`patch_select` composed of torch ops (backends without the kernel): the rule, scene by scene."""
    out = []
    for f, n, s in zip(first.tolist(), count.tolist(), seed.tolist()):
        x = points[f:f + n]
        d = x - x[s]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        bits = d2.view(torch.int32).long()             # a non-negative fp32 orders like its bit pattern
        bits = torch.where(torch.isnan(d2), torch.full_like(bits, PATCH_SELECT_NAN_KEY), bits)
        key = (bits << 32) | torch.arange(n, device=points.device)
        out.append((torch.sort(key).values[:K] & 0xFFFFFFFF).int())
    return torch.stack(out)


def patch_select(points, first, count, seed, K):
    """The K nearest stored points of one seed point per scene, for a ragged batch of scenes: the reference's
    `KDTree(input_pos).query(input_pos[seed], K)` (train_utils.py:118-123) on the device.

    points (P,3) fp32: the scenes back to back; first / count / seed: (B,) HOST integers (list, numpy or CPU tensor) --
    scene b is points[first[b] : first[b] + count[b]], its seed point is row seed[b] of that slice.
    -> idx (B,K) int32 on points' device, scene-local, ascending in (d2, index) with the canonical fp32
    d2 = (dx*dx + dy*dy) + dz*dz; a NaN d2 ranks after +inf (include/tpgan_ops.h)."""
    _check_float(points, "points", 2)
    _need(points.shape[1] == 3, "points must be (P,3)")
    B = len(first)
    first, count, seed = (_host_ints(a, n, (B,)) for a, n in ((first, "first"), (count, "count"), (seed, "seed")))
    K = int(K)
    _need(B > 0, "patch_select needs at least one scene")
    _need(K > 0, "K must be positive")
    _check_frames(first, count, points.shape[0], "points")
    _need(bool((count >= K).all()), f"K = {K} exceeds a scene's particle count ({int(count.min())})")
    _need(bool(((seed >= 0) & (seed < count)).all()), "seed must index a point of its scene")
    be = backend_for(points)
    with torch.no_grad():
        if hasattr(be, "patch_select"):
            return be.patch_select(points.detach(), first, count, seed, K)
        return _patch_select_torch(points.detach(), first, count, seed, K)


def clip_gather_high(pos, vel, frame_first, count, centroids, centroid_row, patch):
    """Every high-resolution array of a batch of clips at once (tempo_dataset.py:69-87):
    high_pos[t,b,k] = pos[frame_first[t,b] + patch[b,k]] - centroids[centroid_row[b]], high_vel the plain gather of `vel`
    (None: no velocities).  pos / vel (P,3) fp32: every frame back to back; frame_first (T,B), count (B), centroid_row (B):
    HOST integers; centroids (F,3) fp32; patch (B,K) int32.  -> (high_pos (T,B,K,3), high_vel or None)."""
    _check_float(pos, "pos", 2)
    _check_float(centroids, "centroids", 2)
    _check_int(patch, "patch", 2)
    _same_device(pos, centroids, patch)
    _need(pos.shape[1] == 3 and centroids.shape[1] == 3, "pos and centroids must hold 3-D points")
    if vel is not None:
        _check_float(vel, "vel", 2)
        _same_device(pos, vel)
        _need(vel.shape == pos.shape, "vel must have pos's shape")
    B = patch.shape[0]
    frame_first = _host_ints(frame_first, "frame_first", (None, B))
    T = frame_first.shape[0]
    count = _host_ints(count, "count", (B,))
    centroid_row = _host_ints(centroid_row, "centroid_row", (B,))
    _need(1 <= T <= CLIP_MAX_T, f"a clip has 1..{CLIP_MAX_T} frames")
    _need(B > 0 and patch.shape[1] > 0, "patch must be (B,K) with B, K positive")
    _check_frames(frame_first, count, pos.shape[0], "pos")
    _need(bool(((centroid_row >= 0) & (centroid_row < centroids.shape[0])).all()), "centroid_row out of range")
    be = backend_for(pos)
    with torch.no_grad():
        if hasattr(be, "clip_gather_high"):
            return be.clip_gather_high(pos.detach(), None if vel is None else vel.detach(), frame_first, count,
                                       centroids.detach(), centroid_row, patch)
        rows = torch.as_tensor(frame_first, dtype=torch.long, device=pos.device).view(T, B, 1) + patch.long().view(1, B, -1)
        c = centroids[torch.as_tensor(centroid_row, dtype=torch.long, device=pos.device)].view(1, B, 1, 3)
        return pos[rows] - c, None if vel is None else vel[rows]


def clip_gather_low(high_pos, fps_idx, noise=None, jitter=0.0, vel=None, frame_first=None, count=None):
    """Every low-resolution array of the batch at once (tempo_dataset.py:89-100):
    low_pos[t,b,j] = high_pos[t,b,fps_idx[b,j]] + noise[t,b,j] * jitter (noise None: the plain gather) and, if `vel` is
    given, low_vel[t,b,j] = vel[frame_first[t,b] + fps_idx[b,j]] -- the reference's rows, quirk included: it indexes the
    whole scene's velocities with the patch-local sampling (include/tpgan_ops.h).  high_pos (T,B,K,3) fp32, fps_idx (B,M)
    int32, noise (T,B,M,3) fp32, vel (P,3) fp32, frame_first (T,B) / count (B) HOST integers as in `clip_gather_high`.
    -> (low_pos (T,B,M,3), low_vel or None)."""
    _check_float(high_pos, "high_pos", 4)
    _check_int(fps_idx, "fps_idx", 2)
    _same_device(high_pos, fps_idx)
    T, B, K, _ = high_pos.shape
    M = fps_idx.shape[1]
    _need(high_pos.shape[3] == 3 and fps_idx.shape[0] == B and min(T, B, K, M) > 0, "high_pos (T,B,K,3), fps_idx (B,M)")
    _need(T <= CLIP_MAX_T, f"a clip has 1..{CLIP_MAX_T} frames")
    if noise is not None:
        _check_float(noise, "noise", 4)
        _same_device(high_pos, noise)
        _need(tuple(noise.shape) == (T, B, M, 3), "noise must be (T,B,M,3)")
    if vel is not None:
        _check_float(vel, "vel", 2)
        _same_device(high_pos, vel)
        _need(vel.shape[1] == 3, "vel must be (P,3)")
        _need(frame_first is not None and count is not None, "low-resolution velocities need frame_first and count")
        frame_first = _host_ints(frame_first, "frame_first", (T, B))
        count = _host_ints(count, "count", (B,))
        _check_frames(frame_first, count, vel.shape[0], "vel")
    be = backend_for(high_pos)
    with torch.no_grad():
        if hasattr(be, "clip_gather_low"):
            return be.clip_gather_low(high_pos.detach(), fps_idx, noise, float(jitter),
                                      None if vel is None else vel.detach(), frame_first, count)
        sel = fps_idx.long().view(1, B, M, 1).expand(T, B, M, 3)
        low = torch.gather(high_pos, 2, sel)
        if noise is not None:
            low = low + noise * float(np.float32(jitter))
        if vel is None:
            return low, None
        lim = torch.as_tensor(count, dtype=torch.long, device=vel.device).view(1, B, 1) - 1
        rows = torch.as_tensor(frame_first, dtype=torch.long, device=vel.device).view(T, B, 1) \
            + torch.minimum(fps_idx.long().view(1, B, M), lim)
        return low, vel[rows]


# --------------------------------------------- action clips from device-resident depth videos (csrc/action_sample.hip)
def frame_subset_max_k():
    return _lib.load().tpg_patch_select_max_k()


def frame_subset(count, seeds, K, device="cuda"):
    """A uniformly random ordered subset of K points of every frame of a ragged batch: the reference's
    `np.random.choice(n, K, replace=False)` per frame (msr_dataset.py:69-74) on the device.

    count / seeds: (F,) HOST integers (list, numpy or CPU tensor): points per frame, and one 64-bit seed per frame
    (0 <= seed < 2^64).  -> idx (F,K) int32 on `device`, frame-local: by ascending (key, j) with the hash key of
    include/tpgan_ops.h, the K smallest if a frame has more than K points, else 0..n-1 repeated K // n times followed by
    the K % n smallest.  A pure function of (count, seeds, K)."""
    F = len(count)
    count = _host_ints(count, "count", (F,))
    if isinstance(seeds, torch.Tensor):
        _need(not seeds.is_cuda, "seeds is a host table (the sampler draws it on the host): pass a CPU tensor or a list")
        seeds = seeds.numpy()
    seeds = np.asarray(seeds, dtype=object)              # Python ints: a list may hold values above 2^63
    _need(seeds.shape == (F,), f"seeds must have shape {(F,)}, got {seeds.shape}")
    _need(all(isinstance(s, (int, np.integer)) and 0 <= s < 2 ** 64 for s in seeds),
          "seeds must hold integers in [0, 2^64)")
    seeds = np.array([int(s) for s in seeds], dtype=np.uint64)
    K = int(K)
    _need(F > 0, "frame_subset needs at least one frame")
    _need(K > 0, "K must be positive")
    _need(bool((count > 0).all()), "every frame must hold at least one point")
    device = torch.device(device)
    be = backend_for(torch.empty(0, device=device))
    _need(hasattr(be, "frame_subset"), f"the {device.type} backend has no frame_subset")
    if device.type == "cuda":
        _need(K <= frame_subset_max_k(), f"K = {K} exceeds the selection's capacity ({frame_subset_max_k()})")
    with torch.no_grad():
        return be.frame_subset(count, seeds, K, device)


def action_gather(points, frame_first, count, idx, scale=None, mode="train"):
    """Every high-resolution cloud of a batch of action clips at once (msr_dataset.py:67-91 / :105-127): with
    q = (double)points[frame_first[t,b] + idx[t,b,k]], y negated, and v = (q * scale[b]) / 300.0 in fp64,
        mode "train": high[t,b,k] = (float)(v - c[b]), c[b] the fp64 mean of v over frame T // 2's K rows;
        mode "test":  high[t,b,k] = (float)(v - c[t,b]), c[t,b] the mean per frame, also returned; no scale.
    points (P,3) fp32: every stored frame back to back; frame_first / count (T,B): HOST integers; idx (T,B,K) int32
    (`frame_subset`; entries are clamped into the frame); scale (B,3) HOST float64 or None (ones).
    -> (high (T,B,K,3) fp32, centres (T,B,3) fp32 in test mode, else None)."""
    _check_float(points, "points", 2)
    _check_int(idx, "idx", 3)
    _same_device(points, idx)
    _need(points.shape[1] == 3, "points must be (P,3)")
    _need(mode in ("train", "test"), 'mode must be "train" or "test"')
    T, B, K = idx.shape
    _need(1 <= T <= CLIP_MAX_T, f"a clip has 1..{CLIP_MAX_T} frames")
    _need(B > 0 and K > 0, "idx must be (T,B,K) with B, K positive")
    frame_first = _host_ints(frame_first, "frame_first", (T, B))
    count = _host_ints(count, "count", (T, B))
    _check_frames(frame_first, count, points.shape[0], "points")
    if scale is not None:
        _need(mode == "train", "the test split has no scale")
        scale = np.ascontiguousarray(scale.numpy() if isinstance(scale, torch.Tensor) else scale, dtype=np.float64)
        _need(scale.shape == (B, 3) and bool(np.isfinite(scale).all()), "scale must be (B,3) finite float64 values")
    be = backend_for(points)
    _need(hasattr(be, "action_gather"), f"the {points.device.type} backend has no action_gather")
    with torch.no_grad():
        return be.action_gather(points.detach(), frame_first, count, idx, scale, mode == "test")


def farthest_point_sampling(pts, k, initial_idx=None):
    """Dataset-side FPS (sampling.py:50-106, used by train_utils.py:126, tempo_dataset.py:78,
    msr_dataset.py:94,130 through numba on the host): every point eligible, first pick
    `initial_idx` (None = random, np.random like the reference).  pts (N,3) or (B,N,3) on the
    GPU -> indices (k,) / (B,k) int64."""
    single = pts.dim() == 2
    x = (pts.unsqueeze(0) if single else pts).detach().float().contiguous()
    _need(x.dim() == 3 and x.shape[2] == 3, "pts must be (N,3) or (B,N,3)")
    B, N, _ = x.shape
    if initial_idx is None:
        initial_idx = [int(np.random.randint(N)) for _ in range(B)]
    start = torch.as_tensor(initial_idx, dtype=torch.int32).reshape(-1).expand(B).contiguous().to(x.device)
    idx = backend_for(x).fps(x, int(k), start, False).long()
    return idx[0] if single else idx


def sample_patch_with_fps(input_pos, patch_num, ds_ratio=0.125, seed_idx=None, initial_idx=None,
                          return_free_surface_particles=False, h=None):
    """train_utils.py:98-139 on the GPU: the `patch_num` nearest neighbours of a random seed
    point (the reference queries a KD-tree) and their FPS down-sampling to `ds_ratio` of the patch.
    input_pos (N,3) -> dict(patch_pos, ds_pos, patch_idx, fps_idx).  The K = thousands
    selection is one `torch.topk` over the N distances to the seed (a single query: nothing to
    tile), FPS is the HIP kernel.  return_free_surface_particles=True (the reference's default; needs its
    scale `h`) adds `surface_points`: the patch's free-surface points at radius 3.1 * 0.025 / h
    (train_utils.py:132-134, analysis.get_free_surface_particles)."""
    if return_free_surface_particles:
        _need(h is not None and float(h) > 0.0, "return_free_surface_particles needs the scale h > 0")
    x = input_pos.detach().float()
    N = x.shape[0]
    if seed_idx is None:
        seed_idx = int(np.random.choice(N))
    d = ((x - x[seed_idx]) ** 2).sum(-1)
    patch = torch.topk(d, min(int(patch_num), N), largest=False, sorted=True).indices
    patch_pos = x[patch].contiguous()
    fps_idx = farthest_point_sampling(patch_pos, int(ds_ratio * patch_pos.shape[0]), initial_idx)
    out = {"patch_pos": patch_pos, "ds_pos": patch_pos[fps_idx], "patch_idx": patch, "fps_idx": fps_idx}
    if return_free_surface_particles:
        from .analysis import get_free_surface_particles
        out["surface_points"] = get_free_surface_particles(patch_pos, 3.1 * 0.025 / float(h))
    return out


class _Gather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx):
        _check_float(features, "features", 3)
        _check_int(idx, "idx", 2)
        _same_device(features, idx)
        ctx.save_for_backward(idx)
        ctx.N = features.shape[2]
        return backend_for(features).gather_fwd(features, idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        g = backend_for(grad_out).gather_bwd(grad_out.contiguous().float(), idx, ctx.N)
        return g, None


def gather_operation(features, idx):
    """(B,C,N),(B,S) int32 -> (B,C,S).  Reference call site discriminator.py:131-137."""
    return _Gather.apply(features, idx)


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, idx):
        _check_float(rows, "rows", 3)
        _check_int(idx, "idx", 2)
        _same_device(rows, idx)
        ctx.save_for_backward(idx)
        ctx.N = rows.shape[1]
        return backend_for(rows).gather_rows_fwd(rows, idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        return backend_for(grad_out).gather_rows_bwd(grad_out.contiguous().float(), idx, ctx.N), None


def gather_rows(rows, idx):
    """(B,N,C) rows, (B,S) int32 -> (B,S,C): gather_operation (discriminator.py:131-137) in the layout the rows path
    keeps its clouds in -- one launch each way instead of transpose copy + gather + transpose copy."""
    return _GatherRows.apply(rows, idx)


def ball_query(radius, nsample, xyz, new_xyz):
    """-> (B,S,nsample) int32.  Inside QueryAndGroup, discriminator.py:190."""
    _check_float(xyz, "xyz", 3)
    _check_float(new_xyz, "new_xyz", 3)
    _same_device(xyz, new_xyz)
    _need(xyz.shape[0] == new_xyz.shape[0], "batch mismatch")
    with torch.no_grad():
        return backend_for(xyz).ball_query(float(radius), int(nsample), xyz.detach(), new_xyz.detach())


class _Group(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx):
        _check_float(features, "features", 3)
        _check_int(idx, "idx", 3)
        _same_device(features, idx)
        _need(features.shape[0] == idx.shape[0], "batch mismatch")
        ctx.save_for_backward(idx)
        ctx.N = features.shape[2]
        return backend_for(features).group_fwd(features, idx)

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        g = backend_for(grad_out).group_bwd(grad_out.contiguous().float(), idx, ctx.N)
        return g, None


def grouping_operation(features, idx):
    """(B,C,N),(B,S,K) int32 -> (B,C,S,K).  gcn_lib/pointnet/gcn.py:207,261; discriminator.py:270,273."""
    return _Group.apply(features, idx)


def three_nn(unknown, known):
    """-> (dist (B,n,3) = sqrt of squared distance, idx (B,n,3) int32)."""
    _check_float(unknown, "unknown", 3)
    _check_float(known, "known", 3)
    _same_device(unknown, known)
    with torch.no_grad():
        d2, idx = backend_for(unknown).three_nn(unknown.detach(), known.detach())
    return torch.sqrt(d2), idx


class _ThreeInterpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, idx, weight):
        _check_float(features, "features", 3)
        _check_int(idx, "idx", 3)
        _check_float(weight, "weight", 3)
        _same_device(features, idx, weight)
        ctx.save_for_backward(idx, weight)
        ctx.m = features.shape[2]
        return backend_for(features).three_interp_fwd(features, idx, weight)

    @staticmethod
    def backward(ctx, grad_out):
        idx, weight = ctx.saved_tensors
        g = backend_for(grad_out).three_interp_bwd(grad_out.contiguous().float(), idx, weight, ctx.m)
        return g, None, None


def three_interpolate(features, idx, weight):
    return _ThreeInterpolate.apply(features, idx, weight)


# ------------------------------------------------------------- kNN / FRNN
def _lengths(t, B, P, device):
    if t is None:
        return None
    t = torch.as_tensor(t, device=device).to(torch.int64).contiguous()
    _need(t.shape == (B,), "lengths must have shape (B,)")
    return t


def neighbour_search(p1, p2, K, lengths1=None, lengths2=None, r=None):
    """Raw search: (dists (B,P1,K) f32, idx (B,P1,K) i64); r=None -> kNN, else d < r^2.

    dists/idx carry no autograd history (callers add it, see knn_points)."""
    _need(p1.dim() == 3 and p2.dim() == 3, "p1, p2 must be (B,P,D)")
    _need(p1.shape[0] == p2.shape[0] and p1.shape[2] == p2.shape[2], "p1/p2 batch or dim mismatch")
    _need(int(K) >= 1, "K must be >= 1")
    _same_device(p1, p2)
    a = p1.detach().float().contiguous()
    b = a if p2 is p1 else p2.detach().float().contiguous()       # a cloud searched in itself: one cast, not two
    B = a.shape[0]
    l1 = _lengths(lengths1, B, a.shape[1], a.device)
    l2 = _lengths(lengths2, B, b.shape[1], a.device)
    r2 = None if r is None else radius_sq(r)
    be = backend_for(a)
    if r is not None and getattr(be, "name", "") == "hip":
        return be.knn(a, b, l1, l2, int(K), r2, r=r)        # large clouds: uniform grid, same results
    return be.knn(a, b, l1, l2, int(K), r2)


RADIUS_KERNELS = {"cubic": 0, "linear": 1}


def radius_reduce(query, pos, r, kernel="cubic", lengths_q=None, lengths_p=None, _grid=None):
    """Neighbourhood sums with no cap on the number of neighbours (csrc/radius_reduce.hip): per query the number of
    points of `pos` within `r` (d2 <= r2, inclusive like scipy's query_ball_point, the query itself included when it is
    a stored point) and the sum of a radial kernel over them -> (count int32, sum float32).

    query (B,Nq,3), pos (B,Np,3) float tensors on the GPU, or unbatched (Nq,3) / (Np,3) (-> (Nq,) results); lengths
    (B,) or None as in `neighbour_search` (queries beyond their length get 0 / 0).  kernel: "cubic"
    (analysis_helper.py:102-113, coefficient 1), "linear" (train_utils.py:258-266) or None (counts only: sum is None).
    Deterministic: the same bits whatever the order in which the grid hands out the neighbours.  No gradient."""
    _need(isinstance(query, torch.Tensor) and isinstance(pos, torch.Tensor), "query and pos must be tensors")
    squeeze, same = query.dim() == 2, pos is query
    if squeeze:
        _need(pos.dim() == 2, "query (Nq,3) needs pos (Np,3)")
        query, pos = query.unsqueeze(0), pos.unsqueeze(0)
    _need(query.dim() == 3 and pos.dim() == 3, "query (B,Nq,3), pos (B,Np,3)")
    _need(query.shape[2] == 3 and pos.shape[2] == 3 and query.shape[0] == pos.shape[0], "query (B,Nq,3), pos (B,Np,3)")
    _need(query.is_floating_point() and pos.is_floating_point(), "query and pos must be float tensors")
    _need(kernel is None or kernel in RADIUS_KERNELS, f"kernel must be one of {sorted(RADIUS_KERNELS)} or None")
    _need(float(r) > 0.0, "r must be positive")
    _same_device(query, pos)
    q = query.detach().float().contiguous()
    p = q if same else pos.detach().float().contiguous()       # a cloud measured in itself: one cast, not two
    be = backend_for(q)
    _need(hasattr(be, "radius_reduce"), "this backend has no radius_reduce")
    B = q.shape[0]
    lq = _lengths(lengths_q, B, q.shape[1], q.device)
    lp = _lengths(lengths_p, B, p.shape[1], q.device)
    with torch.no_grad():
        count, total = be.radius_reduce(q, p, lq, lp, float(r), RADIUS_KERNELS.get(kernel, 0), True,
                                        kernel is not None, _grid)
    if squeeze:
        return count[0], None if total is None else total[0]
    return count, total


# ------------------------------------------------- earth mover's distance, Gaussian sums
EMD_DEFAULTS = dict(eps=1e-4, iters=1_000_000, phases=3, scaling=4.0)


class _Emd(torch.autograd.Function):
    """dist of the auction's assignment with the gradient of |x1 - x2[a]|^2 attached; the assignment is a constant."""

    @staticmethod
    def forward(ctx, xyz1, xyz2, eps, iters, phases, scaling, narrow_at, check_every):
        dist, assignment, price, rounds = backend_for(xyz1).emd_match(xyz1, xyz2, eps, iters, phases, scaling,
                                                                      narrow_at, check_every)
        ctx.save_for_backward(xyz1, xyz2, assignment)
        ctx.mark_non_differentiable(assignment, price, rounds)
        return dist, assignment, price, rounds

    @staticmethod
    def backward(ctx, g, _ga, _gp, _gr):
        xyz1, xyz2, assignment = ctx.saved_tensors
        a = assignment.long().unsqueeze(-1).expand(-1, -1, 3)
        g1 = 2.0 * g.unsqueeze(-1) * (xyz1 - torch.gather(xyz2, 1, a))
        g2 = torch.empty_like(g1).scatter_(1, a, -g1)          # a is a permutation: the gather by its inverse
        return g1, g2, None, None, None, None, None, None


def emd_match(xyz1, xyz2, eps=EMD_DEFAULTS["eps"], iters=EMD_DEFAULTS["iters"], phases=EMD_DEFAULTS["phases"],
              scaling=EMD_DEFAULTS["scaling"], _narrow_at=None, _check_every=None):
    """One-to-one assignment of the points of xyz1 to the points of xyz2 (both (B,n,3)) that approximately minimises
    the sum of squared distances: a forward auction with Jacobi rounds and epsilon scaling (csrc/emd.hip;
    include/tpgan_ops.h states the rule, which is reproduced bit for bit).  `eps` is the final epsilon -- the sum of
    costs ends within n * eps of the optimum -- the phases run at eps * scaling^k, k = phases .. 0; `iters` caps the
    rounds per cloud (RuntimeError beyond it).

    -> dist (B,n) f32 squared distance of every point of xyz1 to its partner, differentiable wrt both clouds with the
    assignment held fixed; assignment (B,n) int32; price (B,n) f32; rounds (B,) int32.  A cloud's results do not
    depend on the rest of the batch.  `_narrow_at` / `_check_every` force the launch arrangement (tests, tuning)."""
    _need(isinstance(xyz1, torch.Tensor) and isinstance(xyz2, torch.Tensor), "xyz1 and xyz2 must be tensors")
    _need(xyz1.dim() == 3 and xyz2.dim() == 3 and xyz1.shape[2] == 3 and xyz2.shape[2] == 3, "clouds must be (B,n,3)")
    _need(xyz1.shape[0] == xyz2.shape[0], "batch mismatch")
    _need(xyz1.shape[1] == xyz2.shape[1], f"emd_match needs equal-size clouds, got {xyz1.shape[1]} and {xyz2.shape[1]}")
    _need(xyz1.is_floating_point() and xyz2.is_floating_point(), "xyz1 and xyz2 must be float tensors")
    _need(float(eps) > 0.0, "eps must be positive")
    _need(int(iters) >= 1, "iters must be >= 1")
    _need(0 <= int(phases) <= 64, "phases must be in [0, 64]")
    _need(float(scaling) >= 1.0, "scaling must be >= 1")
    _need(_narrow_at is None or int(_narrow_at) >= 0, "_narrow_at must be >= 0")
    _need(_check_every is None or 1 <= int(_check_every) <= 4096, "_check_every must be in [1, 4096]")
    _same_device(xyz1, xyz2)
    be = backend_for(xyz1)
    _need(hasattr(be, "emd_match"), "this backend has no emd_match")
    return _Emd.apply(xyz1.float().contiguous(), xyz2.float().contiguous(), float(eps), int(iters), int(phases),
                      float(scaling), _narrow_at, _check_every)


def gaussian_row_sums(a, b, sigma, lengths_a=None, lengths_b=None):
    """(B,N,3), (B,M,3) -> (B,N) float64: entry i is sum_j exp(-|a_i - b_j|^2 / (2 sigma^2)) over the points of b
    (csrc/gauss_sum.hip; lengths (B,) or None as in `neighbour_search`, rows beyond lengths_a get 0).  Summed in
    fixed point: the same bits on every run and at every batch position.  No gradient."""
    _need(isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor), "a and b must be tensors")
    _need(a.dim() == 3 and b.dim() == 3 and a.shape[2] == 3 and b.shape[2] == 3 and a.shape[0] == b.shape[0],
          "a (B,N,3), b (B,M,3)")
    _need(a.is_floating_point() and b.is_floating_point(), "a and b must be float tensors")
    _need(float(sigma) > 0.0, "sigma must be positive")
    _need(b.shape[1] < (1 << 17), "gaussian_row_sums: at most 2^17 - 1 points per cloud")
    _same_device(a, b)
    x = a.detach().float().contiguous()
    y = x if b is a else b.detach().float().contiguous()
    be = backend_for(x)
    _need(hasattr(be, "gaussian_row_sums"), "this backend has no gaussian_row_sums")
    B = x.shape[0]
    with torch.no_grad():
        return be.gaussian_row_sums(x, y, _lengths(lengths_a, B, x.shape[1], x.device),
                                    _lengths(lengths_b, B, y.shape[1], x.device), float(sigma))


# ------------------------------------------------------------------------ point-cloud pictures (csrc/render.hip)
RENDER_CAM_FLOATS = 18                 # eye, r, d, f, scale, cx, cy, near, far, mode: include/tpgan_ops.h
RENDER_ORTHO, RENDER_PINHOLE = 0, 1
RENDER_MAX_SIZE = 16
RENDER_MAX_EXTENT = 16384
RENDER_KEY_BYTES = 256 << 20           # cap of the 64-bit key buffer; more frames than fit are rendered in chunks
_KEY_FLIP = -2 ** 63                   # unsigned 64-bit order on int64: flip the top bit


def _render_points_torch(points, lengths, scalar, cams, W, H, size, lo, hi, lut, background):
    """`render_points` composed of torch ops (backends without the kernel): the rule of include/tpgan_ops.h frame by
    frame -- fp32 operations in the stated order, the cull before any conversion to an integer, one `amin` scatter of
    the 64-bit keys per splat offset (kept as int64 with the top bit flipped, which orders them as unsigned)."""
    F, N, _ = points.shape
    dev = points.device
    image = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    winner = torch.empty((F, H, W), dtype=torch.int32, device=dev)
    lo_t = torch.tensor(np.float32(lo), device=dev)
    inv = torch.tensor(np.float32(255.0) / (np.float32(hi) - np.float32(lo)), device=dev)
    lens = [N] * F if lengths is None else [min(max(int(v), 0), N) for v in lengths.tolist()]
    for f in range(F):
        cam = torch.from_numpy(cams[f if cams.shape[0] > 1 else 0]).to(dev)
        p = points[f, :lens[f]]
        q = p - cam[0:3]

        def dot(b):
            return (q[:, 0] * b[0] + q[:, 1] * b[1]) + q[:, 2] * b[2]
        xv, yv, zv = dot(cam[3:6]), dot(cam[6:9]), dot(cam[9:12])
        if float(cam[17]) != 0.0:
            u, v = (xv / zv) * cam[12] + cam[13], (yv / zv) * cam[12] + cam[14]
        else:
            u, v = xv * cam[12] + cam[13], yv * cam[12] + cam[14]
        t = zv - cam[15]
        keep = (t >= 0) & (zv <= cam[16]) & (u >= -size) & (u < W + size) & (v >= -size) & (v < H + size)
        index = torch.nonzero(keep).view(-1)
        px, py = torch.floor(u[index]).long(), torch.floor(v[index]).long()
        key = (((t[index].view(torch.int32).long() & 0xFFFFFFFF) << 32) | index) ^ _KEY_FLIP
        keys = torch.full((H * W,), 2 ** 63 - 1, dtype=torch.int64, device=dev)
        for dy in range(size):
            for dx in range(size):
                x, y = px - size // 2 + dx, py - size // 2 + dy
                ok = (x >= 0) & (x < W) & (y >= 0) & (y < H)
                keys.scatter_reduce_(0, (y * W + x)[ok], key[ok], "amin")
        hit = keys != 2 ** 63 - 1
        ukey = keys ^ _KEY_FLIP
        win = torch.where(hit, ukey & 0xFFFFFFFF, torch.full_like(keys, -1))
        if scalar is None:
            s = ((ukey >> 32) & 0xFFFFFFFF).to(torch.int32).view(torch.float32)
        else:
            s = scalar[f][win.clamp(min=0)] if N > 0 else torch.zeros_like(keys, dtype=torch.float32)
        c = (s - lo_t) * inv
        c = torch.where(c > 0, c, torch.zeros_like(c)).clamp(max=255.0)         # NaN: c > 0 is false, level 0
        level = torch.where(c >= 255.0, torch.full_like(keys, 255), (c + 0.5).long())
        image[f] = torch.where(hit.view(-1, 1), lut[level], background.view(1, 3)).view(H, W, 3)
        winner[f] = win.to(torch.int32).view(H, W)
    return image, winner


def _picture_args(points, cams, width, height, lut, lengths, scalar, lo, hi, background, max_key_bytes):
    """What `render_points` and `render_surface` ask of their common arguments; -> F, N, W, H, cams (host fp32 (1 or
    F, 18)), scalar, lo, hi (rounded to fp32), lut and background (uint8 on the points' device), lengths."""
    _check_float(points, "points", 3)
    _need(points.shape[2] == 3, "points must be (F,N,3)")
    F, N, _ = points.shape
    W, H = int(width), int(height)
    _need(1 <= W <= RENDER_MAX_EXTENT and 1 <= H <= RENDER_MAX_EXTENT, f"width and height must be 1..{RENDER_MAX_EXTENT}")
    _need(int(max_key_bytes) > 0, "max_key_bytes must be positive")
    if isinstance(cams, torch.Tensor):
        _need(not cams.is_cuda, "cams is a host table: pass a CPU tensor or a numpy array")
        cams = cams.numpy()
    cams = np.ascontiguousarray(np.asarray(cams, dtype=np.float32).reshape(-1, RENDER_CAM_FLOATS))
    _need(cams.shape[0] in (1, F) or F == 0, f"cams must hold 1 or {F} cameras, got {cams.shape[0]}")
    _need(bool(np.isfinite(cams).all()), "cams must be finite")
    _need(bool(np.isin(cams[:, 17], (RENDER_ORTHO, RENDER_PINHOLE)).all()), "camera mode must be 0 (ortho) or 1 (pinhole)")
    _need(bool((cams[cams[:, 17] == RENDER_PINHOLE, 15] > 0).all()), "a pinhole camera needs near > 0")
    if scalar is not None:
        _check_float(scalar, "scalar", 2)
        _same_device(points, scalar)
        _need(tuple(scalar.shape) == (F, N), f"scalar must be ({F}, {N})")
        _need(lo is not None and hi is not None, "a scalar colour needs its range lo / hi")
    if lo is None:
        lo = 0.0
    if hi is None:
        hi = float(np.float32(cams[0, 16]) - np.float32(cams[0, 15]))
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    _need(hi > lo and np.isfinite(np.float32(255.0) / (np.float32(hi) - np.float32(lo))) and np.isfinite(lo),
          f"the colour range needs finite lo < hi, got {lo} .. {hi}")
    lut = torch.as_tensor(lut)
    _need(lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3), "lut must be (256,3) uint8")
    lut = lut.to(points.device).contiguous()
    bg = np.asarray(background)
    _need(bg.shape == (3,) and bg.dtype.kind in "iu" and 0 <= bg.min() and bg.max() <= 255, "background must be 3 values 0..255")
    background = torch.tensor(bg.tolist(), dtype=torch.uint8).to(points.device)
    lengths = _lengths(lengths, F, N, points.device)
    return F, N, W, H, cams, scalar, lo, hi, lut, background, lengths


def _winner_depth_torch(points, cams, winner):
    """The depth layer of a splat picture: t = zv - near of the winner point per pixel, by the projection of
    `_render_points_torch` (the same fp32 operations in the same order), +inf where winner is -1 -> (F,H,W) fp32."""
    F = points.shape[0]
    depth = torch.full(winner.shape, float("inf"), dtype=torch.float32, device=points.device)
    for f in range(F):
        cam = torch.from_numpy(cams[f if cams.shape[0] > 1 else 0]).to(points.device)
        hit = winner[f] >= 0
        q = points[f][winner[f][hit].long()] - cam[0:3]
        zv = (q[:, 0] * cam[9] + q[:, 1] * cam[10]) + q[:, 2] * cam[11]
        depth[f][hit] = zv - cam[15]
    return depth


def render_points(points, cams, width, height, lut, size=1, lengths=None, scalar=None, lo=None, hi=None,
                  background=(255, 255, 255), max_key_bytes=RENDER_KEY_BYTES, return_depth=False):
    """One picture per cloud of a ragged batch: a z-buffered square splat (csrc/render.hip; the rule in full:
    include/tpgan_ops.h).

    points (F,N,3) fp32; lengths (F,) or None: rows at or beyond lengths[f] are never read; scalar (F,N) fp32 or None:
    what a point is coloured by (None: its depth t = zv - near).  cams: HOST fp32, (18,) / (1,18) shared by all frames
    or (F,18) one per frame: eye, the rows r / d / f (image-right, image-DOWN, forward), scale, cx, cy, near, far, mode
    (`render.Camera.row()` builds one).  lut (256,3) uint8 and background (3 values 0..255); the colour is lut[level]
    with c = (s - lo) * (255 / (hi - lo)), level = 0 unless c > 0, 255 from c >= 255, else int(c + 0.5); lo / hi
    default to 0 and far - near of the first camera when the colour is the depth, and must be given with `scalar`.
    size: the splat's edge in pixels, 1..16.  max_key_bytes: cap of the kernel's 64-bit key buffer; F is rendered in
    chunks that stay under it (the pictures do not depend on it).
    -> (image (F,height,width,3) uint8, winner (F,height,width) int32: the visible point's index, -1 = background).
    return_depth: also depth (F,height,width) fp32, the winner's t (torch ops after the kernel, `_winner_depth_torch`),
    +inf = background: what `compose_layers` orders the splat by.
    Bit-identical from run to run and at every batch position; no gradient."""
    size = int(size)
    _need(1 <= size <= RENDER_MAX_SIZE, f"size must be 1..{RENDER_MAX_SIZE}")
    F, N, W, H, cams, scalar, lo, hi, lut, background, lengths = _picture_args(
        points, cams, width, height, lut, lengths, scalar, lo, hi, background, max_key_bytes)
    if F == 0 or N == 0:
        out = (background.view(1, 1, 1, 3).expand(F, H, W, 3).contiguous(),
               torch.full((F, H, W), -1, dtype=torch.int32, device=points.device))
        if return_depth:
            out += (torch.full((F, H, W), float("inf"), dtype=torch.float32, device=points.device),)
        return out
    be = backend_for(points)
    with torch.no_grad():
        args = (points.detach(), lengths, None if scalar is None else scalar.detach(), cams, W, H, size, lo, hi, lut,
                background)
        if hasattr(be, "render_points"):
            out = be.render_points(*args, int(max_key_bytes))
        else:
            out = _render_points_torch(*args)
        return out + (_winner_depth_torch(points.detach(), cams, out[1]),) if return_depth else out


# ---------------------------------------------------------------------- fluid surface pictures (csrc/surface.hip)
SURFACE_MAX_RADIUS = 64                # pixels: a nearer or larger sphere is drawn as a disc of this radius
SURFACE_MAX_HALF = 4                   # the smoothing window's half-width, 1..4
SURFACE_SHADE_FLOATS = 11              # L, Hh, ka, kd, ks, kf, p: include/tpgan_ops.h


def surface_shade(light=(-0.4, -0.6, -0.7), ka=0.25, kd=0.65, ks=0.35, kf=0.25, p=5):
    """The 11 floats `render_surface` shades with: `light` is the direction TOWARDS the light in view coordinates (x
    right, y down, z forward; the default comes from up, left and in front of the surface) and is normalised here, Hh
    is the unit half vector of it and the direction to the viewer (0,0,-1); ambient ka, diffuse kd, specular ks with
    the exponent 2^p (p an integer 0..8), kf the weight of the Fresnel rim (1 - max(-nz, 0))^5.  Host maths in
    float64, rounded to fp32 once."""
    L = np.asarray(light, dtype=np.float64).reshape(3)
    n = float(np.linalg.norm(L))
    _need(np.isfinite(n) and n > 0.0, "light must be a finite non-zero vector")
    L = L / n
    half = L + np.array([0.0, 0.0, -1.0])
    h = float(np.linalg.norm(half))
    _need(h > 1e-9, "the light must not shine from straight behind the surface")
    _need(int(p) == p and 0 <= int(p) <= 8, "p must be an integer 0..8")
    table = np.concatenate([L, half / h, [ka, kd, ks, kf, float(int(p))]]).astype(np.float32)
    _need(bool(np.isfinite(table).all()), "the shading table must be finite")
    return table


def render_surface(points, cams, width, height, lut, radius, lengths=None, scalar=None, lo=None, hi=None, half_width=2,
                   iters=3, delta=None, shade=None, background=(255, 255, 255), max_key_bytes=RENDER_KEY_BYTES):
    """One picture of the fluid's SURFACE per cloud of a ragged batch: screen-space fluid rendering (csrc/surface.hip;
    the rule in full: include/tpgan_ops.h).  Every point is a sphere of `radius` world units; the nearest sphere front
    per pixel is kept, that depth image is smoothed `iters` times (a binomial window of half-width `half_width` = 1..4
    that leaves out neighbours further than `delta` in depth, default 2 x radius, so silhouettes stay sharp and the
    background stays background; iters = 0 shades the raw sphere fronts), normals are taken from the smoothed depth and
    it is shaded with `shade` (`surface_shade()`: 11 host floats) over the colour lut[level] of `scalar` (None: of the
    depth).  points, cams, width, height, lut, lengths, scalar, lo, hi, background and max_key_bytes are
    `render_points`'s.  Needs the HIP backend: there is no composition of torch ops for it.
    -> (image (F,height,width,3) uint8, depth (F,height,width) fp32: the smoothed front's distance from the near plane,
    +inf = background, winner (F,height,width) int32: the point whose sphere is in front, -1 = background).
    Bit-identical from run to run, at every batch position and under every chunking; no gradient."""
    F, N, W, H, cams, scalar, lo, hi, lut, background, lengths = _picture_args(
        points, cams, width, height, lut, lengths, scalar, lo, hi, background, max_key_bytes)
    radius = float(np.float32(radius))
    _need(np.isfinite(radius) and radius > 0.0, "radius must be positive and finite")
    half_width, iters = int(half_width), int(iters)
    _need(1 <= half_width <= SURFACE_MAX_HALF, f"half_width must be 1..{SURFACE_MAX_HALF}")
    _need(iters >= 0, "iters must not be negative")
    delta = float(np.float32(2.0 * radius if delta is None else delta))
    _need(np.isfinite(delta) and delta > 0.0, "delta must be positive and finite")
    shade = surface_shade() if shade is None else np.ascontiguousarray(np.asarray(shade, dtype=np.float32).reshape(-1))
    _need(shade.shape == (SURFACE_SHADE_FLOATS,) and bool(np.isfinite(shade).all()),
          f"shade must be {SURFACE_SHADE_FLOATS} finite floats (surface_shade() builds them)")
    _need(shade[10] == int(shade[10]) and 0 <= shade[10] <= 8, "p must be an integer 0..8")
    if F == 0 or N == 0:
        return (background.view(1, 1, 1, 3).expand(F, H, W, 3).contiguous(),
                torch.full((F, H, W), float("inf"), dtype=torch.float32, device=points.device),
                torch.full((F, H, W), -1, dtype=torch.int32, device=points.device))
    be = backend_for(points)
    _need(hasattr(be, "render_surface"), "this backend has no render_surface")
    with torch.no_grad():
        return be.render_surface(points.detach(), lengths, None if scalar is None else scalar.detach(), cams, W, H,
                                 radius, lo, hi, lut, background, half_width, iters, delta, shade, int(max_key_bytes))


# -------------------------------------------------------------------------- mesh pictures (csrc/mesh_render.hip)
MESH_GUARD = 32768.0                   # a face with a vertex at or beyond this many pixels from the origin is not drawn
MESH_SMALL = 16                        # the kernel's class edge (tuning, not part of the rule): include/tpgan_ops.h
MESH_HUGE = 2048                       # a box of more pixels is drawn by the tile launch, from a list of
MESH_LIST = 256                        # this many faces per frame (tuning as well)
MESH_MAX_ROWS = 715827882              # vertices or faces per mesh: 2^31 / 3
_MESH_EDGES = ((1, 2), (2, 0), (0, 1))  # w_i is the edge function of the edge opposite vertex i


def _mesh_edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _mesh_faces_torch(vertices, faces, cam_row, vlen, tlen):
    """The kept faces of one mesh (V,3) / (T,3) under one camera (host fp32 (18,)), by the rule of include/tpgan_ops.h:
    -> None if there is none, else a dict of index (K,), tri (K,3), X, Y (K,3) int64, d (K,3) fp32 (zv under a pinhole
    camera, else t), area = |A| and sign (K,) int64, own (K,3) bool, view (vlen,3) fp32 (xv, yv, zv of every vertex)."""
    if vlen == 0 or tlen == 0:
        return None
    cam = torch.from_numpy(cam_row).to(vertices.device)
    q = vertices[:vlen] - cam[0:3]

    def dot(b):
        return (q[:, 0] * b[0] + q[:, 1] * b[1]) + q[:, 2] * b[2]
    xv, yv, zv = dot(cam[3:6]), dot(cam[6:9]), dot(cam[9:12])
    pinhole = float(cam_row[17]) != 0.0
    if pinhole:
        u, v = (xv / zv) * cam[12] + cam[13], (yv / zv) * cam[12] + cam[14]
    else:
        u, v = xv * cam[12] + cam[13], yv * cam[12] + cam[14]
    t = zv - cam[15]
    good = (t >= 0) & (zv <= cam[16]) & (u.abs() < MESH_GUARD) & (v.abs() < MESH_GUARD)      # false for NaN and inf
    zero = torch.zeros_like(u)
    X = torch.floor(torch.where(good, u, zero) * 256.0 + 0.5).long()          # only rows that passed are converted
    Y = torch.floor(torch.where(good, v, zero) * 256.0 + 0.5).long()
    tri = faces[:tlen].long()
    ok = ((tri >= 0) & (tri < vlen)).all(1)
    ok = ok & good[torch.where(ok.unsqueeze(1), tri, torch.zeros_like(tri))].all(1)
    index = torch.nonzero(ok).view(-1)
    tri = tri[index]
    X, Y = X[tri], Y[tri]
    A = _mesh_edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    keep = A != 0
    if not bool(keep.any()):
        return None
    index, tri, X, Y, A = index[keep], tri[keep], X[keep], Y[keep], A[keep]
    sign = torch.sign(A)
    own = []
    for a, b in _MESH_EDGES:
        dx, dy = sign * (X[:, b] - X[:, a]), sign * (Y[:, b] - Y[:, a])
        own.append((dy < 0) | ((dy == 0) & (dx > 0)))
    return dict(index=index, tri=tri, X=X, Y=Y, d=(zv if pinhole else t)[tri], area=A.abs(), sign=sign,
                own=torch.stack(own, 1), view=torch.stack([xv, yv, zv], 1), pinhole=pinhole, near=float(cam_row[15]))


def _mesh_weights_torch(fc, rows, px, py):
    """w0..w2 (int64) and l0..l2 (float64) of the kept faces `rows` at the points (px, py) (1/256 pixel), broadcast."""
    X, Y, s, area = fc["X"][rows], fc["Y"][rows], fc["sign"][rows], fc["area"][rows].double()
    if px.dim() == 2:                               # (1, pixels) against (faces, 1); else one face per point
        X, Y, s, area = X.unsqueeze(-1), Y.unsqueeze(-1), s.unsqueeze(-1), area.unsqueeze(-1)
    w = [s * _mesh_edge(X[:, a], Y[:, a], X[:, b], Y[:, b], px, py) for a, b in _MESH_EDGES]
    return w, [wi.double() / area for wi in w]


def _mesh_depth_torch(fc, rows, lam):
    d = fc["d"][rows].double()
    d = [d[:, k].unsqueeze(-1) if lam[0].dim() == 2 else d[:, k] for k in range(3)]
    if fc["pinhole"]:
        Z = 1.0 / ((lam[0] / d[0] + lam[1] / d[1]) + lam[2] / d[2])
        t = (Z - float(np.float32(fc["near"]))).float()
    else:
        t = ((lam[0] * d[0] + lam[1] * d[1]) + lam[2] * d[2]).float()
    return torch.where(t > 0, t, torch.zeros_like(t))


def _render_mesh_torch(vertices, vlengths, faces, flengths, cams, F, W, H, pairs_per_chunk=1 << 22):
    """Entry (a) of the mesh pictures composed of torch ops (backends without the kernel): every kept face against every
    pixel centre, `pairs_per_chunk` face x pixel pairs at a time -> (depth (F,H,W) fp32, winner (F,H,W) int32).  The
    candidate box of the rule is not needed: a covered pixel always lies in it."""
    M, V, _ = vertices.shape
    T = faces.shape[1]
    dev = vertices.device
    depth = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    winner = torch.empty((F, H, W), dtype=torch.int32, device=dev)
    vl = [V] * M if vlengths is None else [min(max(int(v), 0), V) for v in vlengths.tolist()]
    fl = [T] * M if flengths is None else [min(max(int(v), 0), T) for v in flengths.tolist()]
    at = torch.arange(H * W, device=dev)
    px, py = (256 * (at % W) + 128).view(1, -1), (256 * (at // W) + 128).view(1, -1)
    step = max(1, int(pairs_per_chunk) // (H * W))
    for f in range(F):
        m = f if M > 1 else 0
        fc = _mesh_faces_torch(vertices[m], faces[m], cams[f if cams.shape[0] > 1 else 0], vl[m], fl[m])
        keys = torch.full((H * W,), 2 ** 63 - 1, dtype=torch.int64, device=dev)
        for k0 in range(0, 0 if fc is None else fc["index"].shape[0], step):
            rows = torch.arange(k0, min(k0 + step, fc["index"].shape[0]), device=dev)
            w, lam = _mesh_weights_torch(fc, rows, px, py)
            inside = torch.ones_like(w[0], dtype=torch.bool)
            for k in range(3):
                inside &= (w[k] > 0) | ((w[k] == 0) & fc["own"][rows, k].unsqueeze(-1))
            t = _mesh_depth_torch(fc, rows, lam)
            key = (((t.view(torch.int32).long() & 0xFFFFFFFF) << 32) | fc["index"][rows].unsqueeze(-1)) ^ _KEY_FLIP
            key = torch.where(inside, key, torch.full_like(key, 2 ** 63 - 1))
            keys = torch.minimum(keys, key.amin(0))
        hit = keys != 2 ** 63 - 1
        ukey = keys ^ _KEY_FLIP
        winner[f] = torch.where(hit, ukey & 0xFFFFFFFF, torch.full_like(keys, -1)).to(torch.int32).view(H, W)
        bits = ((ukey >> 32) & 0xFFFFFFFF).to(torch.int32).view(torch.float32)
        depth[f] = torch.where(hit, bits, torch.full_like(bits, float("inf"))).view(H, W)
    return depth, winner


def _mesh_shade_torch(depth, winner, vertices, vlengths, faces, flengths, normals, scalar, cams, lo, hi, lut, base,
                      background, shade):
    """Entry (b) of the mesh pictures composed of torch ops -> image (F,H,W,3) uint8."""
    F, H, W = depth.shape
    M, V, _ = vertices.shape
    T = faces.shape[1]
    dev = vertices.device
    vl = [V] * M if vlengths is None else [min(max(int(v), 0), V) for v in vlengths.tolist()]
    fl = [T] * M if flengths is None else [min(max(int(v), 0), T) for v in flengths.tolist()]
    sh = torch.from_numpy(np.ascontiguousarray(shade, dtype=np.float32)).to(dev)
    lo_t = torch.tensor(np.float32(lo), device=dev)
    inv = torch.tensor(np.float32(255.0) / (np.float32(hi) - np.float32(lo)), device=dev)
    image = background.view(1, 1, 3).expand(F, H * W, 3).contiguous()
    at = torch.arange(H * W, device=dev)
    for f in range(F):
        m = f if M > 1 else 0
        cam_row = cams[f if cams.shape[0] > 1 else 0]
        fc = _mesh_faces_torch(vertices[m], faces[m], cam_row, vl[m], fl[m])
        if fc is None:
            continue
        cam = torch.from_numpy(cam_row).to(dev)
        slot = torch.full((T + 1,), -1, dtype=torch.int64, device=dev)
        slot[fc["index"]] = torch.arange(fc["index"].shape[0], device=dev)
        win = winner[f].view(-1).long()
        k = torch.where((win >= 0) & (win < fl[m]), slot[win.clamp(0, T)], torch.full_like(win, -1))
        pix = at[k >= 0]
        rows = k[pix]
        _, lam = _mesh_weights_torch(fc, rows, 256 * (pix % W) + 128, 256 * (pix // W) + 128)
        tri = fc["tri"][rows]

        def mix(a):                                 # a (V,) fp32 -> the pixel's value, float64 and rounded once
            a = a.double()
            return ((lam[0] * a[tri[:, 0]] + lam[1] * a[tri[:, 1]]) + lam[2] * a[tri[:, 2]]).float()
        if normals is not None:
            nw = [mix(normals[m][:, j]) for j in range(3)]
            n = [(nw[0] * cam[3 + 3 * r] + nw[1] * cam[4 + 3 * r]) + nw[2] * cam[5 + 3 * r] for r in range(3)]
        else:
            P = fc["view"]
            a, b = P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]]
            n = [a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                 a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]]
        length = torch.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        ok = length > 0
        n = [torch.where(ok, c / length, torch.full_like(c, d)) for c, d in zip(n, (0.0, 0.0, -1.0))]
        back = n[2] > 0
        n = [torch.where(back, -c, c) for c in n]
        zero = torch.zeros_like(length)
        dif = torch.fmax((n[0] * sh[0] + n[1] * sh[1]) + n[2] * sh[2], zero)
        sp = torch.fmax((n[0] * sh[3] + n[1] * sh[4]) + n[2] * sh[5], zero)
        for _ in range(int(shade[10])):
            sp = sp * sp
        mm = 1.0 - torch.fmax(-n[2], zero)
        m2 = mm * mm
        fr = (m2 * m2) * mm
        lit, gloss = sh[6] + sh[7] * dif, 255.0 * (sh[8] * sp + sh[9] * fr)
        if base is not None:
            col = base.view(1, 3).expand(pix.shape[0], 3)
        else:
            s = mix(scalar[m]) if scalar is not None else depth[f].view(-1)[pix]
            c = (s - lo_t) * inv
            c = torch.where(c > 0, c, torch.zeros_like(c)).clamp(max=255.0)     # NaN: c > 0 is false, level 0
            col = lut[torch.where(c >= 255.0, torch.full_like(pix, 255), (c + 0.5).long())]
        val = col.float() * lit.unsqueeze(1) + gloss.unsqueeze(1)
        val = torch.where(val > 0, val, torch.zeros_like(val)).clamp(max=255.0)
        image[f, pix] = torch.where(val >= 255.0, torch.full_like(val, 255.0), torch.floor(val + 0.5)).to(torch.uint8)
    return image.view(F, H, W, 3)


def render_mesh(vertices, faces, cams, width, height, lut, vlengths=None, flengths=None, normals=None, scalar=None,
                lo=None, hi=None, base=None, shade=None, background=(255, 255, 255), max_key_bytes=RENDER_KEY_BYTES):
    """One picture per frame of indexed triangle meshes: a z-buffered rasteriser with deferred shading
    (csrc/mesh_render.hip; the rule in full: include/tpgan_ops.h, "mesh pictures").

    vertices (M,V,3) fp32 and faces (M,T,3) int32 with M = 1 (one mesh drawn under every camera, as an obstacle) or M =
    the number of cameras F (mesh f in frame f); vlengths / flengths (M,) or None: vertices and faces at or beyond them
    are never read.  A face with an index outside its mesh's vertices, a vertex that is not finite, behind the near
    plane, beyond far or beyond 32768 pixels, or no area is not drawn; there is NO clipping.  cams: HOST fp32 (18,) /
    (F,18) as for `render_points`; with one camera F = M.  normals (M,V,3) fp32 or None (the face's own normal);
    scalar (M,V) fp32 with lo / hi, or None (the depth, 0 .. far - near): the base colour lut[level], interpolated in
    screen space; base: 3 values 0..255 that replace it.  shade: `surface_shade()`'s table.  Both sides are lit.
    -> (image (F,height,width,3) uint8, depth (F,height,width) fp32: the nearest face's distance from the near plane,
    perspective-correct, +inf = background, winner (F,height,width) int32: that face's index, -1 = background).
    Bit-identical from run to run, at every batch position and under every chunking, and equal to `_render_mesh_torch`
    + `_mesh_shade_torch`, which backends without the kernel run.  No gradient."""
    _check_float(vertices, "vertices", 3)
    _check_int(faces, "faces", 3)
    _same_device(vertices, faces)
    _need(vertices.shape[2] == 3 and faces.shape[2] == 3, "vertices must be (M,V,3) and faces (M,T,3)")
    M, V, _ = vertices.shape
    T = faces.shape[1]
    _need(faces.shape[0] == M, f"vertices and faces must hold the same number of meshes, got {M} and {faces.shape[0]}")
    _need(V <= MESH_MAX_ROWS and T <= MESH_MAX_ROWS, f"at most {MESH_MAX_ROWS} vertices and faces per mesh")
    ncam = (cams.numel() if isinstance(cams, torch.Tensor) else int(np.size(cams))) // RENDER_CAM_FLOATS
    F = max(M, ncam)
    _need(M in (1, F), f"{M} meshes do not go with {ncam} cameras: one mesh, or one per camera")
    proxy = torch.empty((F, 0, 3), dtype=torch.float32, device=vertices.device)     # the frames `_picture_args` counts
    if scalar is not None:
        _check_float(scalar, "scalar", 2)
        _same_device(vertices, scalar)
        _need(tuple(scalar.shape) == (M, V), f"scalar must be ({M}, {V})")
        _need(lo is not None and hi is not None, "a scalar colour needs its range lo / hi")
    _, _, W, H, cams, _, lo, hi, lut, background, _ = _picture_args(
        proxy, cams, width, height, lut, None, None, 0.0 if lo is None else lo, hi, background, max_key_bytes)
    if normals is not None:
        _check_float(normals, "normals", 3)
        _same_device(vertices, normals)
        _need(tuple(normals.shape) == (M, V, 3), f"normals must be ({M}, {V}, 3)")
    if base is not None:
        bs = np.asarray(base)
        _need(bs.shape == (3,) and bs.dtype.kind in "iu" and 0 <= bs.min() and bs.max() <= 255, "base must be 3 values 0..255")
        base = torch.tensor(bs.tolist(), dtype=torch.uint8).to(vertices.device)
    shade = surface_shade() if shade is None else np.ascontiguousarray(np.asarray(shade, dtype=np.float32).reshape(-1))
    _need(shade.shape == (SURFACE_SHADE_FLOATS,) and bool(np.isfinite(shade).all()),
          f"shade must be {SURFACE_SHADE_FLOATS} finite floats (surface_shade() builds them)")
    _need(shade[10] == int(shade[10]) and 0 <= shade[10] <= 8, "p must be an integer 0..8")
    vlengths, flengths = _lengths(vlengths, M, V, vertices.device), _lengths(flengths, M, T, vertices.device)
    if F == 0 or T == 0 or V == 0:
        return (background.view(1, 1, 1, 3).expand(F, H, W, 3).contiguous(),
                torch.full((F, H, W), float("inf"), dtype=torch.float32, device=vertices.device),
                torch.full((F, H, W), -1, dtype=torch.int32, device=vertices.device))
    be = backend_for(vertices)
    with torch.no_grad():
        vertices, faces = vertices.detach(), faces.detach()
        normals, scalar = None if normals is None else normals.detach(), None if scalar is None else scalar.detach()
        if hasattr(be, "render_mesh"):
            return be.render_mesh(vertices, vlengths, faces, flengths, normals, scalar, cams, F, W, H, lo, hi, lut, base,
                                  background, shade, int(max_key_bytes))
        depth, winner = _render_mesh_torch(vertices, vlengths, faces, flengths, cams, F, W, H)
        image = _mesh_shade_torch(depth, winner, vertices, vlengths, faces, flengths, normals, scalar, cams, lo, hi, lut,
                                  base, background, shade)
        return image, depth, winner


def compose_layers(layers):
    """[(image (...,H,W,3) uint8, depth (...,H,W) fp32), ...] -> (image, depth): per pixel the layer of smallest depth
    (+inf: background, which every surface is in front of); on equality the EARLIER layer.  Every picture op writes such a
    depth: `render_surface`, `render_mesh`, `render_points(return_depth=True)`.  Plain torch, no kernel."""
    layers = list(layers)
    _need(len(layers) >= 1, "compose_layers needs at least one layer")
    image, depth = layers[0]
    for img, dep in layers[1:]:
        _need(img.shape == image.shape and dep.shape == depth.shape and tuple(img.shape[:-1]) == tuple(dep.shape),
              "the layers of one picture share its shape")
        take = dep < depth
        image = torch.where(take.unsqueeze(-1), img, image)
        depth = torch.where(take, dep, depth)
    return image, depth


# --------------------------------------------------------------- fluid thickness and absorption (csrc/surface.hip)
THICKNESS_MAX_RADIUS = 1024.0          # world units: a chord stays at or below 2^35 units of 2^-24
THICKNESS_MAX_N = 1 << 27              # points per frame: the 64-bit sum cannot overflow
THICKNESS_UNIT = 16777216.0            # 2^24 units per world unit
SMOOTH_ALL = float(np.finfo(np.float32).max)      # the delta that makes `surface_smooth` a plain blur: FLT_MAX


def _render_thickness_torch(points, lengths, cams, W, H, radius, limit, pairs_per_chunk=1 << 22):
    """`render_thickness` composed of torch ops (backends without the kernel): every kept point against every pixel
    centre, `pairs_per_chunk` point x pixel pairs at a time, the contributions summed as int64 -> (F,H,W) fp32.  The
    candidate box of the rule is not needed: a covered pixel always lies in it."""
    F, N, _ = points.shape
    dev = points.device
    out = torch.empty((F, H, W), dtype=torch.float32, device=dev)
    lens = [N] * F if lengths is None else [min(max(int(v), 0), N) for v in lengths.tolist()]
    at = torch.arange(H * W, device=dev)
    cx, cy = ((at % W).float() + 0.5).view(1, -1), ((at // W).float() + 0.5).view(1, -1)
    rad = torch.tensor(np.float32(radius), device=dev)
    step = max(1, int(pairs_per_chunk) // (H * W))
    for f in range(F):
        row = cams[f if cams.shape[0] > 1 else 0]
        cam = torch.from_numpy(row).to(dev)
        q = points[f, :lens[f]] - cam[0:3]

        def dot(b):
            return (q[:, 0] * b[0] + q[:, 1] * b[1]) + q[:, 2] * b[2]
        xv, yv, zv = dot(cam[3:6]), dot(cam[6:9]), dot(cam[9:12])
        if float(row[17]) != 0.0:
            u, v = (xv / zv) * cam[12] + cam[13], (yv / zv) * cam[12] + cam[14]
            rp = (rad / zv) * cam[12]
        else:
            u, v = xv * cam[12] + cam[13], yv * cam[12] + cam[14]
            rp = (rad * cam[12]).expand_as(zv)
        rp = torch.fmin(rp, torch.full_like(rp, float(SURFACE_MAX_RADIUS)))
        t = zv - cam[15]
        keep = (t >= 0) & (zv <= cam[16]) & (rp > 0) & (u >= -rp) & (u < W + rp) & (v >= -rp) & (v < H + rp)
        index = torch.nonzero(keep).view(-1)
        lim = None if limit is None else limit[f].reshape(1, -1)
        acc = torch.zeros((H * W,), dtype=torch.int64, device=dev)
        for k0 in range(0, index.shape[0], step):
            rows = index[k0:k0 + step]
            pu, pv, pt, pr = (a[rows].view(-1, 1) for a in (u, v, t, rp))
            dx, dy = (cx - pu) / pr, (cy - pv) / pr
            s = dx * dx + dy * dy
            covered = s < 1.0
            # sqrtf: torch's vectorised fp32 sqrt is not correctly rounded on every backend; the float64 root rounded to
            # fp32 is (53 bits are more than twice 24 plus two: the second rounding cannot change the answer)
            half = rad * torch.sqrt(torch.where(covered, 1.0 - s, torch.zeros_like(s)).double()).float()
            tp, tb = pt - half, pt + half
            a = torch.where(tp > 0, tp, torch.zeros_like(tp))
            b = tb if lim is None else torch.where(lim < tb, lim.expand_as(tb), tb)      # false for a NaN: the whole chord
            term = b - a
            units = (torch.where(covered & (term > 0), term, torch.zeros_like(term)) * THICKNESS_UNIT).long()
            acc += units.sum(0)
        out[f] = (acc.to(torch.float32) * (1.0 / THICKNESS_UNIT)).view(H, W)
    return out


def render_thickness(points, cams, width, height, radius, lengths=None, limit=None, max_key_bytes=RENDER_KEY_BYTES):
    """How much fluid every pixel looks through (csrc/surface.hip; the rule in full: include/tpgan_ops.h, "fluid
    thickness and absorption"): every point is a sphere of `radius` world units (at most 1024) as in `render_surface`,
    and a pixel's value is the sum over the spheres that cover it of the ray's chord through the sphere, in front of the
    near plane and in front of `limit` (F,height,width) fp32 or None: the opaque scene's depth, +inf where there is
    nothing.  points, cams, width, height, lengths and max_key_bytes are `render_points`'s.
    -> thickness (F,height,width) fp32 in world units, 0 where there is no fluid.
    The chords are summed as 64-bit integers of 2^-24 units: bit-identical from run to run, at every batch position and
    under every chunking, and equal to `_render_thickness_torch`, which backends without the kernel run.  No
    gradient."""
    dummy = torch.zeros((256, 3), dtype=torch.uint8)
    F, N, W, H, cams, _, _, _, _, _, lengths = _picture_args(points, cams, width, height, dummy, lengths, None, None, None,
                                                             (0, 0, 0), max_key_bytes)
    radius = float(np.float32(radius))
    _need(np.isfinite(radius) and 0.0 < radius <= THICKNESS_MAX_RADIUS,
          f"radius must be positive and at most {THICKNESS_MAX_RADIUS:g}")
    _need(N <= THICKNESS_MAX_N, f"at most {THICKNESS_MAX_N} points per frame")
    if limit is not None:
        _check_float(limit, "limit", 3)
        _same_device(points, limit)
        _need(tuple(limit.shape) == (F, H, W), f"limit must be ({F}, {H}, {W})")
    if F == 0 or N == 0:
        return torch.zeros((F, H, W), dtype=torch.float32, device=points.device)
    be = backend_for(points)
    with torch.no_grad():
        args = (points.detach(), lengths, cams, W, H, radius, None if limit is None else limit.detach())
        if hasattr(be, "render_thickness"):
            return be.render_thickness(*args, int(max_key_bytes))
        return _render_thickness_torch(*args)


def _surface_smooth_torch(image, half_width, delta):
    """One pass of entry (b) of the fluid surface pictures composed of torch ops -> (F,H,W) fp32."""
    F, H, W = image.shape
    k = half_width
    bw = [1]
    for _ in range(2 * k):
        bw = [a + b for a, b in zip([0] + bw, bw + [0])]
    pad = torch.full((F, H + 2 * k, W + 2 * k), float("inf"), dtype=torch.float32, device=image.device)
    pad[:, k:k + H, k:k + W] = image
    acc, ws = torch.zeros_like(image), torch.zeros_like(image)
    for oy in range(2 * k + 1):
        for ox in range(2 * k + 1):
            zj = pad[:, oy:oy + H, ox:ox + W]
            ok = (zj - image).abs() <= delta        # false for background, NaN and what lies outside
            w = float(bw[oy] * bw[ox])
            acc = torch.where(ok, acc + w * zj, acc)
            ws = torch.where(ok, ws + w, ws)
    return torch.where(torch.isfinite(image), acc / ws, image)


def surface_smooth(image, half_width=2, delta=None, iters=1):
    """`iters` passes of the surface renderer's smoothing (tpg_surface_smooth_f32) over any image (F,H,W) fp32: a
    binomial window of half-width `half_width` = 1..4 that leaves out pixels outside the image, pixels that are not finite
    and neighbours further than `delta` from the centre.  delta None: FLT_MAX, a plain blur, which is how a thickness
    image is smoothed (its zeros are finite and take part).  -> a new (F,H,W) fp32; iters = 0 returns `image` itself.
    The kernel on the HIP backend, `_surface_smooth_torch` elsewhere; the two are equal.  No gradient."""
    _check_float(image, "image", 3)
    half_width, iters = int(half_width), int(iters)
    _need(1 <= half_width <= SURFACE_MAX_HALF, f"half_width must be 1..{SURFACE_MAX_HALF}")
    _need(iters >= 0, "iters must not be negative")
    delta = float(np.float32(SMOOTH_ALL if delta is None else delta))
    _need(np.isfinite(delta) and delta > 0.0, "delta must be positive and finite")
    F, H, W = image.shape
    _need(1 <= W <= RENDER_MAX_EXTENT and 1 <= H <= RENDER_MAX_EXTENT, f"width and height must be 1..{RENDER_MAX_EXTENT}")
    if iters == 0 or F == 0:
        return image
    with torch.no_grad():
        image = image.detach()
        if image.is_cuda:
            return backend_for(image).surface_smooth(image, half_width, delta, iters)
        for _ in range(iters):
            image = _surface_smooth_torch(image, half_width, delta)
        return image


def absorb_table(sigma, th_max):
    """The (256,3) fp32 transmittance table `absorb_layers` looks thickness up in: table[l][c] = exp(-sigma_c * th_max *
    l / 255) (Beer-Lambert), sigma: 3 finite absorption coefficients >= 0 per world unit, th_max > 0: the thickness of
    level 255.  Host maths in float64, rounded to fp32 once."""
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    th_max = float(th_max)
    _need(sigma.shape == (3,) and bool(np.isfinite(sigma).all()) and bool((sigma >= 0).all()),
          "sigma must be 3 finite values >= 0")
    _need(np.isfinite(th_max) and th_max > 0.0, "th_max must be positive and finite")
    level = np.arange(256, dtype=np.float64).reshape(256, 1)
    return np.exp(-sigma.reshape(1, 3) * th_max * level / 255.0).astype(np.float32)


def _absorb_torch(fluid, fdepth, thickness, behind, bdepth, table, th_max):
    """`absorb_layers` in plain torch -> (image, depth)."""
    dev = fluid.device
    tab = torch.tensor(table, dtype=torch.float32, device=dev)
    inv = torch.tensor(np.float32(255.0) / np.float32(th_max), device=dev)
    c = thickness * inv
    c = torch.where(c > 0, c, torch.zeros_like(c)).clamp(max=255.0)             # NaN: c > 0 is false, level 0
    level = torch.where(c >= 255.0, torch.full_like(c, 255.0), torch.floor(c + 0.5)).long()
    T = tab[level]
    val = fluid.float() * (1.0 - T) + behind.float() * T
    val = torch.where(val > 0, val, torch.zeros_like(val)).clamp(max=255.0)
    mixed = torch.where(val >= 255.0, torch.full_like(val, 255.0), torch.floor(val + 0.5)).to(torch.uint8)
    back = ~torch.isfinite(fdepth) | (bdepth < fdepth)
    return torch.where(back.unsqueeze(-1), behind, mixed), torch.where(back, bdepth, fdepth)


def absorb_layers(fluid_image, fluid_depth, thickness, behind_image, behind_depth, table, th_max):
    """The translucent fluid over what lies behind it (csrc/surface.hip; the rule in full: include/tpgan_ops.h, "fluid
    thickness and absorption").  fluid_image (F,H,W,3) uint8 and fluid_depth (F,H,W) fp32: the shaded fluid
    (`render_surface`); thickness (F,H,W) fp32 (`render_thickness`, smoothed or not); behind_image / behind_depth: the
    opaque scene, e.g. `render_mesh`'s picture, or the background colour with +inf.  Where there is no fluid, or the
    opaque scene is nearer, the pixel is behind's; elsewhere per channel fluid * (1 - T) + behind * T with T =
    table[level][c], level = thickness * 255 / th_max rounded, 0 .. 255.  table: `absorb_table(sigma, th_max)`, HOST
    (256,3) fp32 in [0,1].  -> (image (F,H,W,3) uint8, depth (F,H,W) fp32: fluid_depth where the fluid shows).
    The kernel on the HIP backend, `_absorb_torch` elsewhere; the two are equal.  No gradient."""
    for t, name, ndim in ((fluid_depth, "fluid_depth", 3), (thickness, "thickness", 3), (behind_depth, "behind_depth", 3)):
        _check_float(t, name, ndim)
    F, H, W = fluid_depth.shape
    for t, name in ((fluid_image, "fluid_image"), (behind_image, "behind_image")):
        _need(isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and tuple(t.shape) == (F, H, W, 3) and
              t.is_contiguous(), f"{name} must be a contiguous uint8 tensor ({F}, {H}, {W}, 3)")
    _need(thickness.shape == fluid_depth.shape and behind_depth.shape == fluid_depth.shape,
          "the layers of one picture share its shape")
    _same_device(fluid_image, fluid_depth, thickness, behind_image, behind_depth)
    _need(1 <= W <= RENDER_MAX_EXTENT and 1 <= H <= RENDER_MAX_EXTENT, f"width and height must be 1..{RENDER_MAX_EXTENT}")
    if isinstance(table, torch.Tensor):
        _need(not table.is_cuda, "table is a host table: pass a CPU tensor or a numpy array")
        table = table.numpy()
    table = np.ascontiguousarray(np.asarray(table, dtype=np.float32))
    _need(table.shape == (256, 3) and bool(((table >= 0) & (table <= 1)).all()), "table must be (256,3) values in [0,1]")
    th_max = float(np.float32(th_max))
    with np.errstate(all="ignore"):
        _need(np.isfinite(th_max) and th_max > 0.0 and np.isfinite(np.float32(255.0) / np.float32(th_max)),
              "th_max must be positive and finite")
    if F == 0:
        return torch.empty_like(fluid_image), torch.empty_like(fluid_depth)
    with torch.no_grad():
        args = (fluid_image.detach(), fluid_depth.detach(), thickness.detach(), behind_image.detach(),
                behind_depth.detach(), table, th_max)
        if fluid_image.is_cuda:
            return backend_for(fluid_image).absorb_layers(*args)
        return _absorb_torch(*args)


# ------------------------------------------------------------------- particle fluid simulator (csrc/pbf.hip)
PBF_RADIUS = 0.0125                    # the reference's particle radius a; spacing s = 2a, support h = 4a
PBF_GRAVITY = (0.0, -9.81, 0.0)
PBF_ITERS = 4                          # Jacobi iterations per substep
# Tuned on the host statement (tests/test_simulate_cpu.py holds the properties they were tuned to):
PBF_EPS = 0.25                         # relaxation, in units of sum |G|^2 (0.47 in a lattice): half a Jacobi step, no overshoot
PBF_K = 0.2                            # tensile term: at 0.1 and below a splash still drives pairs into one box corner, where
#                                        the clamp merges them for good (d2 == 0 has no gradient); 0.2 keeps the nearest pair
#                                        above 0.4 s while a pool at rest stays within 2 % of the lattice density
PBF_XSPH = 0.05                        # XSPH c: a pool's rms speed falls below 0.02 m/s within 2 s, splashes are not damped
PBF_MAX_N = 1 << 22                    # particles per scene: the fixed-point sums' headroom (csrc/pbf.hip)
PBF_XSPH_MAX = 0.5                     # cap of c(viscosity): one XSPH application scales a velocity deviation by
#                                        1 - c n / S0, a contraction while c n / S0 < 2: at 0.5 up to 4 x the rest density
PBF_VISCOSITY = 0.01                   # the viscosity whose coefficient is PBF_XSPH: the liquid of every scene so far
PBF_VORTICITY = 0.4                    # shipped confinement strength in m/s: the largest rung of 0.0125 * 2^k, k = 0..5, at
#                                        which a dropped body keeps the bounds of tests/test_simulate_cpu.py and comes to
#                                        rest as without it (the ladder and the energy it adds: DESIGN.md, section 4s)
PBF_VORT_DELTA = 2.0 ** -13            # N = eta / (|eta| + delta).  Smallest power of two that keeps |N| < 2^-10 on every
#                                        interior particle of a rigidly rotating lattice, where eta is exactly 0 in exact
#                                        arithmetic: the rounding noise measured there (7^3 particles, 3 rad/s,
#                                        tests/pbf_vort_cases.py) is |eta| <= 8.6e-8 against m = 0.16, so 2^-14 fails
_F32 = np.float32


def pbf_lattice_sum():
    """S0: the sum of W = (1 - |z|^2 / 4)^3 over the points z of Z^3 with |z| < 2 -- an infinite cubic lattice of
    spacing s = h / 2 seen from one of its points, self included -- in float64."""
    r = np.arange(-2, 3, dtype=np.float64)
    z2 = (r[:, None, None] ** 2 + r[None, :, None] ** 2) + r[None, None, :] ** 2
    return float((np.clip(1.0 - z2 / 4.0, 0.0, None) ** 3).sum())


def pbf_lattice_curl():
    """R0 = (1/3) sum of ((2 - |z|) / 2)^2 |z| over the points z of Z^3 with 0 < |z| < 2 (26 of them), in float64: in a
    cubic lattice of spacing s = h / 2 that rotates rigidly at Omega, the curl of the rule (include/tpgan_ops.h,
    "vorticity confinement") is s * R0 * 2 Omega."""
    r = np.arange(-2, 3, dtype=np.float64)
    z = np.sqrt((r[:, None, None] ** 2 + r[None, :, None] ** 2) + r[None, None, :] ** 2)
    return float((np.clip((2.0 - z) / 2.0, 0.0, None) ** 2 * z).sum() / 3.0)


class PbfParams:
    """The constants of one simulation, each rounded to fp32 once (include/tpgan_ops.h): radius a, h = 4a, S0, wq,
    dp_scale = -7 h S0 / 64, cs = c / S0, eps, k, gravity, and the iteration count.  vorticity: the confinement strength
    in m/s (0: none, and no launch for it), carried as vs = vorticity / (s R0) with s = 2a, beside delta."""

    def __init__(self, radius=PBF_RADIUS, iters=PBF_ITERS, eps=PBF_EPS, k=PBF_K, c=PBF_XSPH, gravity=PBF_GRAVITY,
                 vorticity=0.0):
        S0 = pbf_lattice_sum()
        self.vorticity = float(vorticity)
        self.vs = float(_F32(float(vorticity) / (2.0 * float(radius) * pbf_lattice_curl())))
        self.delta = float(_F32(PBF_VORT_DELTA))
        _need(np.isfinite(self.vs) and self.vs >= 0.0, "vorticity must be finite and not negative")
        self.radius = float(_F32(radius))
        self.h = float(_F32(4.0 * float(radius)))
        self.S0 = float(_F32(S0))
        self.wq = float(_F32((1.0 - 0.2 ** 2) ** 3))
        self.dp_scale = float(_F32(-7.0 * 4.0 * float(radius) * S0 / 64.0))
        self.c = float(c)
        self.cs = float(_F32(float(c) / S0))
        self.eps, self.k = float(_F32(eps)), float(_F32(k))
        self.gravity = tuple(float(_F32(g)) for g in gravity)
        self.iters = int(iters)
        _need(np.isfinite(self.radius) and self.radius > 0.0, "radius must be positive and finite")
        _need(self.iters >= 0 and self.eps >= 0.0 and self.k >= 0.0 and self.cs >= 0.0 and len(self.gravity) == 3,
              "iters, eps, k and c must not be negative; gravity has 3 components")
        _need(all(np.isfinite(v) for v in (self.eps, self.k, self.cs) + self.gravity), "parameters must be finite")

    def as_dict(self):
        d = dict(radius=self.radius, iters=self.iters, eps=self.eps, k=self.k, c=self.c, gravity=list(self.gravity))
        if self.vorticity != 0.0:                           # without confinement: the dict of before
            d["vorticity"] = self.vorticity
        return d


def _pbf_candidates_torch(p, h):
    """Candidate pairs (i, j) of one cloud p (n,3): every pair with d < h and more (self pairs included), from a cell
    list with edge 1.001 h in float64.  Any superset gives the same sums: membership is decided by the canonical d2."""
    n = p.shape[0]
    q = p.double()
    c = torch.floor((q - q.amin(0)) / (1.001 * h)).long() + 1                  # cells from 1: the offsets below stay >= 0
    dims = c.amax(0) + 2
    key = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
    skey, order = torch.sort(key)
    ii, jj = [], []
    ar = torch.arange(n, device=p.device)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            row = ((c[:, 2] + dz) * dims[1] + (c[:, 1] + dy)) * dims[0] + c[:, 0]       # 3 x-adjacent cells: one run
            lo, hi = torch.searchsorted(skey, row - 1), torch.searchsorted(skey, row + 1, right=True)
            cnt = hi - lo
            i = torch.repeat_interleave(ar, cnt)
            off = torch.arange(int(cnt.sum()), device=p.device) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
            ii.append(i)
            jj.append(order[lo[i] + off])
    return torch.cat(ii), torch.cat(jj)


class _PbfPairs:
    """The pairs of one cloud with d2 < h2 and what the passes share: W, and G where d2 > 0."""

    def __init__(self, p, prm, neighbours):
        f = lambda v: torch.tensor(v, dtype=torch.float32, device=p.device)      # noqa: E731
        h, h2 = f(prm.h), f(radius_sq(prm.h))
        i, j = neighbours(p, prm.h)
        d = p[i] - p[j]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        keep = d2 < h2
        self.n = p.shape[0]
        self.i, self.j, d, d2 = i[keep], j[keep], d[keep], d2[keep]
        u = (h2 - d2) / h2
        self.W = (u * u) * u
        self.off = d2 != 0                                                        # pairs that have a gradient
        # sqrtf of the rule is correctly rounded; torch's fp32 sqrt on the CPU goes to a vector maths library that is an
        # ulp off now and then.  The float64 root rounded once IS the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits).
        dist = torch.sqrt(d2[self.off].double()).float()
        t = (h - dist) / h
        self.G = (t * t).unsqueeze(1) * (d[self.off] / dist.unsqueeze(1))
        self.gi, self.gj = self.i[self.off], self.j[self.off]

    def total(self, index, terms):
        """sum of int64 `terms` (m,) or (m,3) per particle."""
        return torch.zeros((self.n,) + terms.shape[1:], dtype=torch.int64, device=terms.device).index_add_(0, index, terms)


_PBF_U32, _PBF_U30 = 4294967296.0, 1073741824.0


def _pbf_fix30(t):
    return (t.clamp(-1024.0, 1024.0) * _PBF_U30).to(torch.int64)


def _pbf_clamp(p, lo, hi, a):
    lo_c, hi_c = lo + a, hi - a
    p = torch.where(p < lo_c, lo_c, p)
    return torch.where(p > hi_c, hi_c, p)


def _pbf_lambda_torch(p, prm, neighbours=_pbf_candidates_torch):
    """The lambda pass for one cloud (n,3) -> (lambda (n,), C (n,), pairs)."""
    pr = _PbfPairs(p, prm, neighbours)
    n = pr.total(pr.i, (pr.W * _PBF_U32).to(torch.int64)).to(torch.float32) * (1.0 / _PBF_U32)
    g2 = (pr.G[:, 0] * pr.G[:, 0] + pr.G[:, 1] * pr.G[:, 1]) + pr.G[:, 2] * pr.G[:, 2]
    sg2 = pr.total(pr.gi, (g2 * _PBF_U32).to(torch.int64)).to(torch.float32) * (1.0 / _PBF_U32)
    S = pr.total(pr.gi, (pr.G * _PBF_U32).to(torch.int64)).to(torch.float32) * (1.0 / _PBF_U32)
    C = n / torch.tensor(prm.S0, dtype=torch.float32, device=p.device) - 1.0
    C = torch.where(C > 0, C, torch.zeros_like(C))
    eps = torch.tensor(prm.eps, dtype=torch.float32, device=p.device)
    lam = -(C / ((sg2 + ((S[:, 0] * S[:, 0] + S[:, 1] * S[:, 1]) + S[:, 2] * S[:, 2])) + eps))
    return lam, C, pr


def _pbf_dp_torch(p, lam, pr, lo, hi, prm):
    """The dp pass for one cloud on the pairs of its lambda pass -> (clamped p + dp, dp)."""
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=p.device)          # noqa: E731
    r = pr.W[pr.off] / f(prm.wq)
    r2 = r * r
    co = (lam[pr.gi] + lam[pr.gj]) + -(f(prm.k) * (r2 * r2))
    acc = pr.total(pr.gi, _pbf_fix30(co.unsqueeze(1) * pr.G))
    dp = f(prm.dp_scale) * (acc.to(torch.float32) * (1.0 / _PBF_U30))
    return _pbf_clamp(p + dp, lo, hi, f(prm.radius)), dp


def _pbf_finish_torch(p, x, dt, prm, neighbours=_pbf_candidates_torch, cs_tab=None, curl=False, pairs=None):
    """Velocity and XSPH for one cloud -> v.  cs_tab (n,): the per-particle table of finish_ex (the pair's mean inside the
    term, no outer factor); curl: -> (v, omega (n,4)) with omega = sum u x G on the velocities before XSPH and its length
    in the last column; pairs: the `_PbfPairs` of p, when the caller has them."""
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=p.device)          # noqa: E731
    pr = _PbfPairs(p, prm, neighbours) if pairs is None else pairs
    v = (p - x) / f(dt)
    uw = (v[pr.j] - v[pr.i]) * pr.W.unsqueeze(1)
    if cs_tab is None:
        out = v + f(prm.cs) * (pr.total(pr.i, _pbf_fix30(uw)).to(torch.float32) * (1.0 / _PBF_U30))
    else:
        cij = 0.5 * (cs_tab[pr.i] + cs_tab[pr.j])
        out = v + pr.total(pr.i, _pbf_fix30(cij.unsqueeze(1) * uw)).to(torch.float32) * (1.0 / _PBF_U30)
    if not curl:
        return out
    u, G = v[pr.gj] - v[pr.gi], pr.G
    cross = torch.stack([u[:, 1] * G[:, 2] - u[:, 2] * G[:, 1], u[:, 2] * G[:, 0] - u[:, 0] * G[:, 2],
                         u[:, 0] * G[:, 1] - u[:, 1] * G[:, 0]], 1)
    om = pr.total(pr.gi, _pbf_fix30(cross)).to(torch.float32) * (1.0 / _PBF_U30)
    m = torch.sqrt(((om[:, 0] * om[:, 0] + om[:, 1] * om[:, 1]) + om[:, 2] * om[:, 2]).double()).float()
    return out, torch.cat([om, m.unsqueeze(1)], 1)


def _pbf_vorticity_torch(p, omega, v, dt, prm, neighbours=_pbf_candidates_torch, pairs=None):
    """Vorticity confinement for one cloud: p (n,3) the final positions, omega (n,4) of `_pbf_finish_torch(curl=True)`,
    v (n,3) the velocities after XSPH -> v + (dt vs) (N x omega), N = eta / (|eta| + delta), eta = sum (m_i - m_j) G."""
    f = lambda s: torch.tensor(s, dtype=torch.float32, device=p.device)          # noqa: E731
    pr = _PbfPairs(p, prm, neighbours) if pairs is None else pairs
    m = omega[:, 3]
    eta = pr.total(pr.gi, _pbf_fix30((m[pr.gi] - m[pr.gj]).unsqueeze(1) * pr.G)).to(torch.float32) * (1.0 / _PBF_U30)
    length = torch.sqrt(((eta[:, 0] * eta[:, 0] + eta[:, 1] * eta[:, 1]) + eta[:, 2] * eta[:, 2]).double()).float()
    n = eta / (length + f(prm.delta)).unsqueeze(1)
    force = torch.stack([n[:, 1] * omega[:, 2] - n[:, 2] * omega[:, 1], n[:, 2] * omega[:, 0] - n[:, 0] * omega[:, 2],
                         n[:, 0] * omega[:, 1] - n[:, 1] * omega[:, 0]], 1)
    return v + (f(dt) * f(prm.vs)) * force


def _pbf_collide_torch(p, lo, hi, table, prm, hit=None):
    """collide of include/tpgan_ops.h ("solid obstacles") for one cloud p (n,3) against the rows of table (M,16), in
    torch ops: the same fp32 operations in the same order as pbf_collide_kernel, so the results are EQUAL to its.
    hit: an int32 (n,) tensor that gains bit o for the particles obstacle o moved -> the new p."""
    f = lambda s: torch.tensor(s, dtype=torch.float32, device=p.device)          # noqa: E731
    root = lambda t: torch.sqrt(t.double()).float()                               # noqa: E731  (see _PbfPairs)
    a = f(prm.radius)
    side = lambda q, E: torch.where(q < 0, -E, E)                                 # noqa: E731
    P = [p[:, 0], p[:, 1], p[:, 2]]
    for o in range(table.shape[0]):
        row = table[o].to(device=p.device, dtype=torch.float32)
        kind = float(row[0])
        if kind not in (1.0, 2.0, 3.0) or not bool(torch.isfinite(row[1:]).all()):
            continue
        c, R, s = row[1:4], row[4:13].view(3, 3), row[13:16]
        d = [P[0] - c[0], P[1] - c[1], P[2] - c[2]]
        q = [(d[0] * R[0, k] + d[1] * R[1, k]) + d[2] * R[2, k] for k in range(3)]
        zeros = torch.zeros_like(q[0])
        if kind == 1.0:
            E = s[0] + a
            d2 = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]
            inside = d2 < E * E
            dist = root(d2)
            new = [torch.where(d2 == 0, E if k == 1 else zeros, (q[k] / dist) * E) for k in range(3)]
        elif kind == 2.0:
            E = [s[k] + a for k in range(3)]
            mag = [q[k].abs() for k in range(3)]
            inside = (mag[0] < E[0]) & (mag[1] < E[1]) & (mag[2] < E[2])
            pen = [E[k] - mag[k] for k in range(3)]
            k1 = pen[1] < pen[0]
            k2 = pen[2] < torch.where(k1, pen[1], pen[0])
            axis = torch.where(k2, 2, torch.where(k1, 1, 0))
            new = [torch.where(axis == k, side(q[k], E[k]), q[k]) for k in range(3)]
        else:
            Er, Eh = s[0] + a, s[1] + a
            r2 = q[0] * q[0] + q[2] * q[2]
            inside = (r2 < Er * Er) & (q[1].abs() < Eh)
            r = root(r2)
            cap = (Eh - q[1].abs()) <= (Er - r)
            new = [torch.where(cap, q[0], torch.where(r2 == 0, Er, (q[0] / r) * Er)),
                   torch.where(cap, side(q[1], Eh), q[1]),
                   torch.where(cap, q[2], torch.where(r2 == 0, zeros, (q[2] / r) * Er))]
        P = [torch.where(inside, c[k] + ((R[k, 0] * new[0] + R[k, 1] * new[1]) + R[k, 2] * new[2]), P[k]) for k in range(3)]
        if hit is not None:
            hit |= inside.to(torch.int32) << o
    return _pbf_clamp(torch.stack(P, 1), lo, hi, a)


def _pbf_substep_torch(x, v, lengths, box, dt, prm, neighbours=_pbf_candidates_torch, obstacles=None,
                       sdf_obstacles=None, xsph=None):
    """`pbf_substep` composed of torch ops, scene by scene: the same fp32 operations in the same order and the same
    fixed-point sums as csrc/pbf.hip (the rule: include/tpgan_ops.h), so the results are EQUAL to the kernels'.
    `neighbours(p, h) -> (i, j)` supplies candidate pairs (any superset of the pairs within h).  obstacles (B,M,16) or
    None: collide after predict and after every dp; sdf_obstacles (table (B,M,24), fields) or None: collide_sdf in the
    same places, behind collide.  xsph (B,N) or None: the per-particle XSPH table of finish_ex; prm.vorticity > 0: the
    curl in the finish pass and the confinement pass behind it."""
    B, N, _ = x.shape
    x_out, v_out = x.clone(), v.clone()
    lens = [N] * B if lengths is None else [min(max(int(n), 0), N) for n in lengths.tolist()]
    f = lambda s: torch.tensor(s, dtype=torch.float32, device=x.device)          # noqa: E731
    for b in range(B):
        n = lens[b]
        if n == 0:
            continue
        lo, hi = torch.from_numpy(box[b, :3].copy()).to(x.device), torch.from_numpy(box[b, 3:].copy()).to(x.device)
        xb = x[b, :n]
        vb = v[b, :n] + f(dt) * torch.tensor(prm.gravity, dtype=torch.float32, device=x.device)
        def solids(p):
            if obstacles is not None:
                p = _pbf_collide_torch(p, lo, hi, obstacles[b], prm)
            if sdf_obstacles is not None:
                p = _pbf_collide_sdf_torch(p, lo, hi, sdf_obstacles[0][b], sdf_obstacles[1], prm)
            return p
        p = solids(_pbf_clamp(xb + f(dt) * vb, lo, hi, f(prm.radius)))
        for _ in range(prm.iters):
            lam, _, pr = _pbf_lambda_torch(p, prm, neighbours)
            p, _ = _pbf_dp_torch(p, lam, pr, lo, hi, prm)
            p = solids(p)
        if xsph is None and prm.vorticity == 0.0:
            v_out[b, :n] = _pbf_finish_torch(p, xb, dt, prm, neighbours)
        else:
            pr = _PbfPairs(p, prm, neighbours)
            tab = None if xsph is None else xsph[b, :n]
            if prm.vorticity > 0.0:
                vb, omega = _pbf_finish_torch(p, xb, dt, prm, neighbours, tab, True, pr)
                vb = _pbf_vorticity_torch(p, omega, vb, dt, prm, neighbours, pr)
            else:
                vb = _pbf_finish_torch(p, xb, dt, prm, neighbours, tab, False, pr)
            v_out[b, :n] = vb
        x_out[b, :n] = p
    return x_out, v_out


def pbf_box(box_lo, box_hi, B):
    """box_lo, box_hi: 3 values shared by the batch, or (B,3) -> the host table (B,6) fp32 of include/tpgan_ops.h."""
    lo = np.broadcast_to(np.asarray(box_lo, dtype=np.float32).reshape(-1, 3), (B, 3))
    hi = np.broadcast_to(np.asarray(box_hi, dtype=np.float32).reshape(-1, 3), (B, 3))
    box = np.ascontiguousarray(np.concatenate([lo, hi], 1))
    _need(bool(np.isfinite(box).all()) and bool((box[:, :3] < box[:, 3:]).all()), "the box needs finite lo < hi on every axis")
    return box


PBF_MAX_OBSTACLES = 8                  # obstacles per scene (include/tpgan_ops.h)
PBF_OBSTACLE_KINDS = {"ball": 1, "box": 2, "cylinder": 3}
_PBF_OBSTACLE_SIZES = {"ball": 1, "box": 3, "cylinder": 2}


def _pbf_obstacle_row(ob):
    """One validated table row (16 float32) of an obstacle dict."""
    _need(isinstance(ob, dict) and ob.get("shape") in PBF_OBSTACLE_KINDS,
          f"an obstacle is a dict whose shape is one of {sorted(PBF_OBSTACLE_KINDS)}")
    _need("centre" in ob and "size" in ob, "an obstacle needs a centre and a size")
    shape = ob["shape"]
    centre = np.asarray(ob["centre"], dtype=np.float64).reshape(-1)
    rot = np.asarray(ob.get("rotation", np.eye(3)), dtype=np.float64).reshape(-1)
    size = np.asarray(ob["size"], dtype=np.float64).reshape(-1)
    _need(centre.size == 3 and rot.size == 9, "an obstacle's centre has 3 values, its rotation 9")
    _need(size.size == _PBF_OBSTACLE_SIZES[shape], f"a {shape}'s size has {_PBF_OBSTACLE_SIZES[shape]} value(s)")
    row = np.zeros(16, np.float32)
    row[0], row[1:4], row[4:13], row[13:13 + size.size] = PBF_OBSTACLE_KINDS[shape], centre, rot, size
    _need(bool(np.isfinite(row).all()), "an obstacle's centre, rotation and size must be finite")
    _need(bool((row[13:13 + size.size] > 0).all()), "an obstacle's sizes must be positive")
    R = rot.reshape(3, 3)
    _need(float(np.abs(R @ R.T - np.eye(3)).max()) <= 1e-5, "an obstacle's rotation must be orthonormal within 1e-5")
    return row


def pbf_obstacles(obstacles, B=None, device="cuda"):
    """The device table (B,M,16) fp32 of include/tpgan_ops.h ("solid obstacles") from obstacle dicts, validated on the
    host: `shape` ("ball" | "box" | "cylinder"), `centre` (3), `rotation` (9 values, row-major, default the identity) and
    `size`: a radius for a ball, 3 half extents for a box, (radius, half height) for a cylinder along its local y axis.

    obstacles: one list of dicts shared by the batch (B: how many scenes, default 1), or one list per scene (B: their
    number), padded to the longest with kind-0 rows; None: no obstacles (M = 0).  Raises on a non-finite value, a size
    that is not positive, more than PBF_MAX_OBSTACLES per scene, a rotation that is not orthonormal within 1e-5."""
    obstacles = [] if obstacles is None else list(obstacles)
    if all(isinstance(o, dict) for o in obstacles):
        per_scene = [obstacles] * (1 if B is None else int(B))
    else:
        per_scene = [[] if o is None else list(o) for o in obstacles]
        _need(B is None or int(B) == len(per_scene), "one obstacle list per scene")
    M = max([len(s) for s in per_scene] + [0])
    _need(M <= PBF_MAX_OBSTACLES, f"at most {PBF_MAX_OBSTACLES} obstacles per scene")
    table = np.zeros((len(per_scene), M, 16), np.float32)
    for b, scene in enumerate(per_scene):
        for o, ob in enumerate(scene):
            table[b, o] = _pbf_obstacle_row(ob)
    return torch.from_numpy(table).to(device)


def _pbf_check_obstacles(obstacles, ref, B):
    _check_float(obstacles, "obstacles", 3)
    _need(obstacles.shape[0] == B and obstacles.shape[2] == 16, "obstacles must be (B,M,16)")
    _need(obstacles.shape[1] <= PBF_MAX_OBSTACLES, f"at most {PBF_MAX_OBSTACLES} obstacles per scene")
    _same_device(ref, obstacles)


def pbf_collide(p, lengths, box_lo, box_hi, obstacles, params=None, return_hit=False):
    """The simulator's collide launch kind on its own (include/tpgan_ops.h, "solid obstacles"): every particle projected
    out of the obstacles of its scene in index order, then clamped into the box.

    p (B,N,3) fp32; lengths, box_lo, box_hi as in `pbf_substep`; obstacles: the DEVICE table (B,M,16) of `pbf_obstacles`
    (its values are not checked here; M = 0 applies the clamp alone); params: a `PbfParams` for the particle radius.
    -> p (a new tensor; rows at or beyond lengths[b] come back unchanged), and with return_hit an int32 (B,N) whose bit o
    is set iff obstacle o moved the particle (0 beyond the lengths).  Equal to `_pbf_collide_torch`.  No gradient."""
    _check_float(p, "p", 3)
    _need(p.shape[2] == 3, "p must be (B,N,3)")
    B, N, _ = p.shape
    _need(B <= 65535 and N <= PBF_MAX_N, f"at most 65535 scenes of {PBF_MAX_N} particles")
    _pbf_check_obstacles(obstacles, p, B)
    prm = PbfParams() if params is None else params
    box = pbf_box(box_lo, box_hi, B)
    lengths = _lengths(lengths, B, N, p.device)
    be = backend_for(p)
    with torch.no_grad():
        out = p.detach().clone()
        hit = torch.zeros((B, N), dtype=torch.int32, device=p.device) if return_hit else None
        if hasattr(be, "pbf_collide"):
            be.pbf_collide(p.detach(), lengths, box, obstacles.detach(), prm, out, hit)
        else:
            lens = [N] * B if lengths is None else [min(max(int(n), 0), N) for n in lengths.tolist()]
            for b, n in enumerate(lens):
                lo, hi = torch.from_numpy(box[b, :3].copy()).to(p.device), torch.from_numpy(box[b, 3:].copy()).to(p.device)
                out[b, :n] = _pbf_collide_torch(p[b, :n].detach(), lo, hi, obstacles[b], prm, None if hit is None else hit[b, :n])
    return (out, hit) if return_hit else out


def pbf_xsph_coefficient(viscosity):
    """c(nu) = min(PBF_XSPH * nu / PBF_VISCOSITY, PBF_XSPH_MAX) in float64, elementwise.  nu is a knob of THIS solver (the
    XSPH blend of a particle's velocity with its neighbours'), not a physical viscosity and not SPlisHSPlasH's."""
    return np.minimum(PBF_XSPH * np.asarray(viscosity, np.float64) / PBF_VISCOSITY, PBF_XSPH_MAX)


def pbf_xsph(viscosity, params=None, device="cuda"):
    """The per-particle XSPH table of `pbf_substep(xsph=)`: viscosity (B,N), a host array or a tensor of nu per
    particle (finite, not negative; rows beyond a scene's length hold anything valid, 0 say) -> cs = fp32(c(nu) / S0),
    a (B,N) fp32 tensor on `device` (a tensor's own device when `viscosity` is one).  Build it once per batch."""
    if isinstance(viscosity, torch.Tensor):
        device, viscosity = viscosity.device, viscosity.detach().cpu().numpy()
    nu = np.asarray(viscosity, np.float64)
    _need(nu.ndim == 2, "viscosity must be (B,N)")
    _need(bool(np.isfinite(nu).all()) and bool((nu >= 0.0).all()), "viscosity must be finite and not negative")
    prm = PbfParams() if params is None else params
    cs = (pbf_xsph_coefficient(nu) / prm.S0).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(cs)).to(device)


def pbf_substep(x, v, lengths, box_lo, box_hi, dt, params=None, obstacles=None, sdf_obstacles=None, xsph=None):
    """One substep of the particle fluid simulator (Position Based Fluids, Jacobi, gather form; csrc/pbf.hip, the rule
    in full: include/tpgan_ops.h) for every scene of a ragged batch.

    x, v (B,N,3) fp32; lengths (B,) or None: rows at or beyond lengths[b] are never read and come back unchanged
    (the values stay on the device and are not checked: each counts as min(max(lengths[b], 0), N) of the int64 it is);
    box_lo, box_hi: HOST values, 3 shared by the batch or (B,3); dt > 0; params: a `PbfParams` (None: the defaults);
    obstacles: the device table (B,M,16) of `pbf_obstacles`: static solids, applied after predict and after every dp
    pass (None: no obstacles, and no launch for them); sdf_obstacles: the (table, fields) pair of `pbf_sdf_obstacles`:
    mesh obstacles as sampled distance fields, applied in the same places behind the analytic ones (None: no launch);
    xsph: the (B,N) device table of `pbf_xsph`, an XSPH coefficient per particle in place of params.c (None: params.c).
    With xsph or params.vorticity > 0 the substep ends grid | finish_ex | vorticity (include/tpgan_ops.h, "vorticity
    confinement and per-particle viscosity"); with neither it is the substep of before, launch for launch.
    -> (x, v) new tensors.  Bit-identical from run to run, at every batch position, and equal to `_pbf_substep_torch`,
    which backends without the kernels run (CPU tensors need a registered checker, as everywhere).  No gradient."""
    _check_float(x, "x", 3)
    _check_float(v, "v", 3)
    _need(x.shape[2] == 3 and v.shape == x.shape, "x and v must be (B,N,3)")
    _same_device(x, v)
    B, N, _ = x.shape
    _need(B <= 65535 and N <= PBF_MAX_N, f"at most 65535 scenes of {PBF_MAX_N} particles")
    if obstacles is not None:
        _pbf_check_obstacles(obstacles, x, B)
        obstacles = obstacles.detach()
    if sdf_obstacles is not None:
        sdf_obstacles = _pbf_check_sdf_obstacles(sdf_obstacles, x, B)
    prm = PbfParams() if params is None else params
    dt = float(_F32(dt))
    _need(np.isfinite(dt) and dt > 0.0, "dt must be positive and finite")
    box = pbf_box(box_lo, box_hi, B)
    lengths = _lengths(lengths, B, N, x.device)
    if xsph is not None:
        _check_float(xsph, "xsph", 2)
        _need(xsph.shape == (B, N), "xsph must be (B,N)")
        _same_device(x, xsph)
        xsph = xsph.detach()
    be = backend_for(x)
    with torch.no_grad():
        if xsph is not None or prm.vorticity != 0.0:
            if hasattr(be, "pbf_finish_ex"):
                return be.pbf_substep(x.detach(), v.detach(), lengths, box, dt, prm, x.clone(), v.clone(), obstacles,
                                      sdf_obstacles, xsph)
            # a backend without finish_ex (the CPU checker): the whole substep as torch ops, as for sdf_obstacles below
            return _pbf_substep_torch(x.detach(), v.detach(), lengths, box, dt, prm, obstacles=obstacles,
                                      sdf_obstacles=sdf_obstacles, xsph=xsph)
        if sdf_obstacles is None:                       # the calls of before, argument for argument
            if hasattr(be, "pbf_substep"):
                return be.pbf_substep(x.detach(), v.detach(), lengths, box, dt, prm, x.clone(), v.clone(), obstacles)
            return _pbf_substep_torch(x.detach(), v.detach(), lengths, box, dt, prm, obstacles=obstacles)
        if hasattr(be, "pbf_collide_sdf"):
            return be.pbf_substep(x.detach(), v.detach(), lengths, box, dt, prm, x.clone(), v.clone(), obstacles,
                                  sdf_obstacles)
        # a backend without the new launch kind (the CPU checker): the whole substep as torch ops, with the backend's own
        # neighbour search where it has one
        return _pbf_substep_torch(x.detach(), v.detach(), lengths, box, dt, prm, obstacles=obstacles,
                                  sdf_obstacles=sdf_obstacles)


# ------------------------------------------------------------------------ mesh obstacles (csrc/pbf.hip)
PBF_MAX_SDF_OBSTACLES = 4              # include/tpgan_ops.h
PBF_SDF_MAX_DIM = 4096
PBF_SDF_KIND = 4
_PBF_SDF_WORDS = 24


def _pbf_sdf_row_host(row):
    """One table row (24 words, a float32 array) -> (floats[17], (nx, ny, nz), offset) with the integer words decoded."""
    row = np.ascontiguousarray(row, dtype=np.float32)
    words = row.view(np.int32)
    offset = (int(words[21]) << 32) | (int(words[20]) & 0xFFFFFFFF)
    return row[:17], (int(words[17]), int(words[18]), int(words[19])), offset


def _pbf_sdf_row_ok(fl, dims, offset, fields_len):
    with np.errstate(all="ignore"):
        ok = float(fl[0]) == float(PBF_SDF_KIND) and bool((np.abs(fl[1:]) <= np.finfo(np.float32).max).all())
    ok = ok and float(fl[16]) > 0.0 and all(2 <= n <= PBF_SDF_MAX_DIM for n in dims)
    return ok and 0 <= offset <= fields_len and dims[0] * dims[1] * dims[2] <= fields_len - offset


def _pbf_collide_sdf_torch(p, lo, hi, table, fields, prm, hit=None):
    """collide_sdf of include/tpgan_ops.h ("mesh obstacles") for one cloud p (n,3) against the rows of table (M,24) and
    the buffer fields (L,), in torch ops: the same fp32 operations in the same order as pbf_collide_sdf_kernel, so the
    results are EQUAL to its.  hit: an int32 (n,) tensor that gains bit o for the particles row o moved -> the new p."""
    f = lambda s: torch.tensor(s, dtype=torch.float32, device=p.device)          # noqa: E731
    a = f(prm.radius)
    rows = table.detach().cpu().numpy().reshape(-1, _PBF_SDF_WORDS)
    fields = fields.reshape(-1)
    P = [p[:, 0].clone(), p[:, 1].clone(), p[:, 2].clone()]
    for o in range(rows.shape[0]):
        fl, (nx, ny, nz), off = _pbf_sdf_row_host(rows[o])
        if not _pbf_sdf_row_ok(fl, (nx, ny, nz), off, fields.numel()):
            continue
        t = torch.from_numpy(fl.copy()).to(p.device)
        c, R, org, step = t[1:4], t[4:13].view(3, 3), t[13:16], t[16]
        d = [P[0] - c[0], P[1] - c[1], P[2] - c[2]]
        q = [(d[0] * R[0, k] + d[1] * R[1, k]) + d[2] * R[2, k] for k in range(3)]
        g = [(q[k] - org[k]) / step for k in range(3)]
        n = (nx, ny, nz)
        inl = torch.ones_like(g[0], dtype=torch.bool)
        for k in range(3):
            inl &= (g[k] >= 0) & (g[k] <= float(n[k] - 1))
        sel = torch.nonzero(inl).squeeze(1)
        if sel.numel() == 0:
            continue
        q, g = [v[sel] for v in q], [v[sel] for v in g]
        i = [torch.clamp(torch.floor(g[k]).long(), max=n[k] - 2) for k in range(3)]
        tx, ty, tz = (g[k] - i[k].to(torch.float32) for k in range(3))
        base = off + (i[0] * ny + i[1]) * nz + i[2]
        F = lambda da, db, dc: fields[base + (da * ny + db) * nz + dc]             # noqa: E731
        x00, x10, x01, x11 = F(1, 0, 0) - F(0, 0, 0), F(1, 1, 0) - F(0, 1, 0), F(1, 0, 1) - F(0, 0, 1), F(1, 1, 1) - F(0, 1, 1)
        c00, c10, c01, c11 = F(0, 0, 0) + tx * x00, F(0, 1, 0) + tx * x10, F(0, 0, 1) + tx * x01, F(0, 1, 1) + tx * x11
        y0, y1 = c10 - c00, c11 - c01
        c0, c1 = c00 + ty * y0, c01 + ty * y1
        gz = c1 - c0
        phi = c0 + tz * gz
        gx0, gx1 = x00 + ty * (x10 - x00), x01 + ty * (x11 - x01)
        gx = gx0 + tz * (gx1 - gx0)
        gy = y0 + tz * (y1 - y0)
        n2 = (gx * gx + gy * gy) + gz * gz
        moved = (phi < a) & (n2 > 0) & torch.isfinite(n2)
        length = torch.sqrt(n2.double()).float()                                  # correctly rounded (see _PbfPairs)
        s = a - phi
        new = [q[0] + s * (gx / length), q[1] + s * (gy / length), q[2] + s * (gz / length)]
        for k in range(3):
            world = c[k] + ((R[k, 0] * new[0] + R[k, 1] * new[1]) + R[k, 2] * new[2])
            P[k][sel] = torch.where(moved, world, P[k][sel])
        if hit is not None:
            hit[sel] |= moved.to(torch.int32) << o
    return _pbf_clamp(torch.stack(P, 1), lo, hi, a)


def _pbf_sdf_obstacle_row(ob, offsets, chunks, total):
    _need(isinstance(ob, dict) and all(k in ob for k in ("field", "origin", "step", "centre")),
          "a mesh obstacle is a dict with field, origin, step and centre")
    field = ob["field"]
    key = id(field)
    if key not in offsets:
        arr = field.detach().cpu().numpy() if isinstance(field, torch.Tensor) else np.asarray(field)
        _need(arr.ndim == 3 and arr.dtype == np.float32, "a field is a float32 (nx,ny,nz) lattice")
        _need(all(2 <= n <= PBF_SDF_MAX_DIM for n in arr.shape), f"a field has 2 .. {PBF_SDF_MAX_DIM} nodes per axis")
        _need(bool(np.isfinite(arr).all()), "a field must be finite")
        offsets[key] = (total[0], arr.shape)
        chunks.append(np.ascontiguousarray(arr).reshape(-1))
        total[0] += arr.size
    offset, dims = offsets[key]
    centre = np.asarray(ob["centre"], dtype=np.float64).reshape(-1)
    rot = np.asarray(ob.get("rotation", np.eye(3)), dtype=np.float64).reshape(-1)
    origin = np.asarray(ob["origin"], dtype=np.float64).reshape(-1)
    _need(centre.size == 3 and rot.size == 9 and origin.size == 3, "centre and origin have 3 values, rotation 9")
    row = np.zeros(_PBF_SDF_WORDS, np.float32)
    row[0], row[1:4], row[4:13], row[13:16], row[16] = PBF_SDF_KIND, centre, rot, origin, ob["step"]
    _need(bool(np.isfinite(row[:17]).all()) and row[16] > 0, "a mesh obstacle's values must be finite, its step positive")
    R = rot.reshape(3, 3)
    _need(float(np.abs(R @ R.T - np.eye(3)).max()) <= 1e-5, "an obstacle's rotation must be orthonormal within 1e-5")
    words = row.view(np.int32)
    words[17:20] = dims
    words[20:22] = np.array([offset], dtype=np.int64).view(np.int32)
    return row


def pbf_sdf_obstacles(obstacles, B=None, device="cuda"):
    """The device pair (table (B,M,24), fields (L,)) of include/tpgan_ops.h ("mesh obstacles") from obstacle dicts,
    validated on the host: `field` (a float32 (nx,ny,nz) lattice of signed distances in the obstacle's frame, negative
    inside: `mesh_sdf` at the nodes), `origin` (3: the position of node (0,0,0) in that frame), `step`, `centre` (3) and
    `rotation` (9 values, row-major, default the identity).  Dicts that hold the SAME field object share one copy in
    `fields`, at any number of poses.

    obstacles: one list shared by the batch (B scenes, default 1) or one list per scene, padded with kind-0 rows; None:
    M = 0.  Raises on a non-finite value, a step that is not positive, an extent outside 2 .. 4096, more than
    PBF_MAX_SDF_OBSTACLES per scene, a rotation that is not orthonormal within 1e-5."""
    obstacles = [] if obstacles is None else list(obstacles)
    if all(isinstance(o, dict) for o in obstacles):
        per_scene = [obstacles] * (1 if B is None else int(B))
    else:
        per_scene = [[] if o is None else list(o) for o in obstacles]
        _need(B is None or int(B) == len(per_scene), "one obstacle list per scene")
    M = max([len(s) for s in per_scene] + [0])
    _need(M <= PBF_MAX_SDF_OBSTACLES, f"at most {PBF_MAX_SDF_OBSTACLES} mesh obstacles per scene")
    table = np.zeros((len(per_scene), M, _PBF_SDF_WORDS), np.float32)
    offsets, chunks, total = {}, [], [0]
    for b, scene in enumerate(per_scene):
        for o, ob in enumerate(scene):
            table[b, o] = _pbf_sdf_obstacle_row(ob, offsets, chunks, total)
    fields = np.concatenate(chunks) if chunks else np.zeros(0, np.float32)
    return torch.from_numpy(table).to(device), torch.from_numpy(fields).to(device)


def _pbf_check_sdf_obstacles(sdf_obstacles, ref, B):
    _need(isinstance(sdf_obstacles, (tuple, list)) and len(sdf_obstacles) == 2, "sdf_obstacles is the pair (table, fields)")
    table, fields = sdf_obstacles
    _check_float(table, "table", 3)
    _check_float(fields, "fields", 1)
    _need(table.shape[0] == B and table.shape[2] == _PBF_SDF_WORDS, f"the table must be (B,M,{_PBF_SDF_WORDS})")
    _need(table.shape[1] <= PBF_MAX_SDF_OBSTACLES, f"at most {PBF_MAX_SDF_OBSTACLES} mesh obstacles per scene")
    _same_device(ref, table, fields)
    return table.detach(), fields.detach()


def pbf_collide_sdf(p, lengths, box_lo, box_hi, table, fields, params=None, return_hit=False):
    """The simulator's collide_sdf launch kind on its own (include/tpgan_ops.h, "mesh obstacles"): every particle pushed
    out of the sampled distance fields of its scene in index order, then clamped into the box.

    p (B,N,3) fp32; lengths, box_lo, box_hi as in `pbf_substep`; table (B,M,24), fields (L,): the DEVICE pair of
    `pbf_sdf_obstacles` (the values are not checked here: a row that fails the rule's tests is skipped in the kernel;
    M = 0 applies the clamp alone); params: a `PbfParams` for the particle radius.
    -> p (a new tensor; rows at or beyond lengths[b] come back unchanged), and with return_hit an int32 (B,N) whose bit o
    is set iff row o moved the particle.  Equal to `_pbf_collide_sdf_torch`, which backends without the kernel run.  No
    gradient."""
    _check_float(p, "p", 3)
    _need(p.shape[2] == 3, "p must be (B,N,3)")
    B, N, _ = p.shape
    _need(B <= 65535 and N <= PBF_MAX_N, f"at most 65535 scenes of {PBF_MAX_N} particles")
    table, fields = _pbf_check_sdf_obstacles((table, fields), p, B)
    prm = PbfParams() if params is None else params
    box = pbf_box(box_lo, box_hi, B)
    lengths = _lengths(lengths, B, N, p.device)
    be = backend_for(p)
    with torch.no_grad():
        out = p.detach().clone()
        hit = torch.zeros((B, N), dtype=torch.int32, device=p.device) if return_hit else None
        if hasattr(be, "pbf_collide_sdf"):
            be.pbf_collide_sdf(p.detach(), lengths, box, table, fields, prm, out, hit)
        else:
            lens = [N] * B if lengths is None else [min(max(int(n), 0), N) for n in lengths.tolist()]
            for b, n in enumerate(lens):
                lo, hi = torch.from_numpy(box[b, :3].copy()).to(p.device), torch.from_numpy(box[b, 3:].copy()).to(p.device)
                out[b, :n] = _pbf_collide_sdf_torch(p[b, :n].detach(), lo, hi, table[b], fields, prm,
                                                    None if hit is None else hit[b, :n])
    return (out, hit) if return_hit else out


# ------------------------------------------------------------------------ signed distance to a mesh (csrc/mesh_sdf.hip)
MESH_SDF_GRID = 65536
MESH_SDF_MAX = 1 << 30


def mesh_sdf_grid(vertices):
    """The snap grid of the sign (include/tpgan_ops.h) of HOST vertices (V,3) float32 -> (box (6,) float32: lo, hi;
    inv_unit): unit the smallest power of two with unit >= largest extent / 2^16 (1 where the box has no extent)."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    _need(v.shape[0] > 0 and bool(np.isfinite(v).all()), "vertices must be finite and at least one")
    lo, hi = v.min(0), v.max(0)
    ext = float((hi.astype(np.float64) - lo.astype(np.float64)).max())
    if ext == 0.0:
        unit = 1.0
    else:
        m, e = np.frexp(ext / MESH_SDF_GRID)                 # ext / 2^16 = m * 2^e, 0.5 <= m < 1
        unit = float(np.ldexp(1.0, int(e) - 1 if m == 0.5 else int(e)))
    _need(2.0 ** -100 <= unit <= 2.0 ** 100, "the mesh's extent is outside what the snap grid holds")
    return np.ascontiguousarray(np.concatenate([lo, hi]).astype(np.float32)), float(1.0 / unit)


def _mesh_sdf_torch(query, vertices, faces, box, inv_unit, pairs_per_chunk=1 << 20):
    """`mesh_sdf` as vectorised torch ops: the same fp32 operations in the same order and the same integer sign as
    csrc/mesh_sdf.hip (the rule: include/tpgan_ops.h), so the results are EQUAL to the kernel's."""
    dev = query.device
    Q, F = query.shape[0], faces.shape[0]
    V = vertices.shape[0]
    lo = torch.from_numpy(np.asarray(box[:3], dtype=np.float32).copy()).to(dev)
    hi = torch.from_numpy(np.asarray(box[3:], dtype=np.float32).copy()).to(dev)
    iu = torch.tensor(inv_unit, dtype=torch.float32, device=dev)

    def snap(x):                                            # (..., 3) f32 -> int64
        t = torch.floor((x - lo) * iu + 0.5)
        t = torch.where(t >= 0, t, torch.zeros_like(t))
        t = torch.where(t <= float(MESH_SDF_GRID), t, torch.full_like(t, float(MESH_SDF_GRID)))
        return t.long()

    def dot(s, t):
        return (s[..., 0] * t[..., 0] + s[..., 1] * t[..., 1]) + s[..., 2] * t[..., 2]
    inbox = ((query >= lo) & (query <= hi)).all(1)
    qi = torch.where(inbox.unsqueeze(1), snap(torch.where(inbox.unsqueeze(1), query, lo.expand_as(query))),
                     torch.zeros((Q, 3), dtype=torch.int64, device=dev))
    best = torch.full((Q,), float("inf"), dtype=torch.float32, device=dev)
    best_f = torch.full((Q,), -1, dtype=torch.int64, device=dev)
    count = torch.zeros((Q,), dtype=torch.int64, device=dev)
    step = max(1, int(pairs_per_chunk) // max(Q, 1))
    inf = torch.tensor(float("inf"), dtype=torch.float32, device=dev)
    zero, one = torch.zeros((), dtype=torch.float32, device=dev), torch.ones((), dtype=torch.float32, device=dev)
    P = query.unsqueeze(1)                                  # (Q,1,3)
    for f0 in range(0, F, step):
        fc = faces[f0:f0 + step].long().clamp(0, V - 1)
        a, b, c = vertices[fc[:, 0]], vertices[fc[:, 1]], vertices[fc[:, 2]]            # (Fc,3)
        u, w_ = b - a, c - a
        valid = ~((u[:, 1] * w_[:, 2] - u[:, 2] * w_[:, 1] == 0) & (u[:, 2] * w_[:, 0] - u[:, 0] * w_[:, 2] == 0)
                  & (u[:, 0] * w_[:, 1] - u[:, 1] * w_[:, 0] == 0))
        # ---- the sign
        A, B_, C_ = snap(a), snap(b), snap(c)
        area = (B_[:, 1] - A[:, 1]) * (C_[:, 2] - A[:, 2]) - (B_[:, 2] - A[:, 2]) * (C_[:, 1] - A[:, 1])
        swap = (area < 0).unsqueeze(1)
        B_, C_ = torch.where(swap, C_, B_), torch.where(swap, B_, C_)
        e1, e2 = B_ - A, C_ - A
        nx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
        ny = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
        nz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
        counts = valid & (area != 0)
        qy, qz = qi[:, 1:2], qi[:, 2:3]                     # (Q,1)
        covers = torch.ones((Q, fc.shape[0]), dtype=torch.bool, device=dev)
        for U, W in ((B_, C_), (C_, A), (A, B_)):
            dy, dz = W[:, 1] - U[:, 1], W[:, 2] - U[:, 2]
            e = dy * (qz - U[:, 2]) - dz * (qy - U[:, 1])
            own = (dy > 0) | ((dy == 0) & (dz > 0))
            covers &= (e > 0) | ((e == 0) & own)
        det = (nx * (qi[:, 0:1] - A[:, 0]) + ny * (qy - A[:, 1])) + nz * (qz - A[:, 2])
        count += (covers & (det < 0) & counts & inbox.unsqueeze(1)).sum(1)
        # ---- the magnitude
        ab, ac = (b - a).unsqueeze(0), (c - a).unsqueeze(0)                 # (1,Fc,3)
        ap, bp, cp = P - a, P - b, P - c                                    # (Q,Fc,3)
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        sm = (va + vb) + vc
        v, w = vb / sm, vc / sm
        rbc = (va <= 0) & (e43 >= 0) & (e56 >= 0)
        wbc = e43 / (e43 + e56)
        v, w = torch.where(rbc, one - wbc, v), torch.where(rbc, wbc, w)
        rac = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        v, w = torch.where(rac, zero, v), torch.where(rac, d2 / (d2 - d6), w)
        rc = (d6 >= 0) & (d5 <= d6)
        v, w = torch.where(rc, zero, v), torch.where(rc, one, w)
        rab = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        v, w = torch.where(rab, d1 / (d1 - d3), v), torch.where(rab, zero, w)
        rb = (d3 >= 0) & (d4 <= d3)
        v, w = torch.where(rb, one, v), torch.where(rb, zero, w)
        ra = (d1 <= 0) & (d2 <= 0)
        v, w = torch.where(ra, zero, v), torch.where(ra, zero, w)
        r = ap - (v.unsqueeze(2) * ab + w.unsqueeze(2) * ac)
        dd = dot(r, r)
        dd = torch.where(valid.unsqueeze(0) & ~torch.isnan(dd), dd, inf)
        val = dd.amin(1)
        ids = torch.arange(f0, f0 + fc.shape[0], device=dev)
        first = torch.where(dd == val.unsqueeze(1), ids.unsqueeze(0), torch.full_like(ids, F).unsqueeze(0)).amin(1)
        better = val < best
        best, best_f = torch.where(better, val, best), torch.where(better, first, best_f)
    d = torch.sqrt(best.double()).float()                   # correctly rounded (see _PbfPairs)
    return torch.where(count % 2 == 1, -d, d), best_f.to(torch.int32)


def mesh_sdf(query, vertices, faces):
    """The signed distance from every query point to a triangle mesh, brute force over all triangles (csrc/mesh_sdf.hip;
    the rule in full: include/tpgan_ops.h): the exact closest point on every triangle in fp32, the sign by ray parity in
    exact integer arithmetic on a 2^16 snap grid over the mesh's box.

    query (Q,3) f32, vertices (V,3) f32, faces (F,3) int32, one device.  -> (dist (Q,) f32, negative inside;
    face (Q,) int32, the nearest triangle, ties to the lowest).  The sign needs a CLOSED mesh (`mesh.check_closed`); its
    orientation does not matter.  Triangles whose fp32 normal is exactly zero are skipped; if all are, dist = +inf and
    face = -1.  One host read (the mesh: faces in range, finite vertices, the bounding box): the op is meant to be called
    once per mesh, not per frame.  Equal to `_mesh_sdf_torch`, which backends without the kernel run (CPU tensors need a
    registered checker).  No gradient."""
    _check_float(query, "query", 2)
    _check_float(vertices, "vertices", 2)
    _check_int(faces, "faces", 2)
    _need(query.shape[1] == 3 and vertices.shape[1] == 3 and faces.shape[1] == 3, "query, vertices and faces are (., 3)")
    _same_device(query, vertices, faces)
    Q, V, F = query.shape[0], vertices.shape[0], faces.shape[0]
    _need(V > 0 and F > 0, "a mesh needs vertices and faces")
    _need(max(Q, V, F) <= MESH_SDF_MAX, "at most 2^30 queries, vertices or faces")
    be = backend_for(query)
    vh, fh = vertices.detach().cpu().numpy(), faces.detach().cpu().numpy()
    _need(bool(np.isfinite(vh).all()), "vertices must be finite")
    _need(int(fh.min()) >= 0 and int(fh.max()) < V, "a face names a vertex that does not exist")
    box, inv_unit = mesh_sdf_grid(vh)
    if Q == 0:
        return (torch.zeros(0, dtype=torch.float32, device=query.device),
                torch.zeros(0, dtype=torch.int32, device=query.device))
    with torch.no_grad():
        if hasattr(be, "mesh_sdf"):
            return be.mesh_sdf(query.detach(), vertices.detach(), faces.detach(), box, inv_unit)
        return _mesh_sdf_torch(query.detach(), vertices.detach(), faces.detach(), box, inv_unit)


# ------------------------------------------------------------------------ isosurfaces (csrc/isosurface.hip)
ISO_DIRECTIONS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1))
ISO_PERMUTATIONS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
ISO_MAX_NODES = 1 << 27


def iso_tetrahedra():
    """The corner offsets v0..v3 of the six tetrahedra of the Kuhn split: [p][a] = (dx, dy, dz)."""
    out = []
    for perm in ISO_PERMUTATIONS:
        v, path = [0, 0, 0], [(0, 0, 0)]
        for axis in perm:
            v[axis] += 1
            path.append(tuple(v))
        out.append(path)
    return out


def iso_case_triangles(case):
    """The triangles of a tetrahedron whose corner at path position a is inside iff bit a of `case` is set, in the
    rule's listed order, before winding: each three edges (lo, hi) of path positions."""
    ins = [a for a in range(4) if case >> a & 1]
    outs = [a for a in range(4) if not case >> a & 1]
    if len(ins) == 1 or len(outs) == 1:
        s = ins[0] if len(ins) == 1 else outs[0]
        return [[(min(s, o), max(s, o)) for o in range(4) if o != s]]
    if len(ins) == 2:
        (a, b), (c, d) = ins, outs
        e = lambda u, v: (min(u, v), max(u, v))  # noqa: E731
        return [[e(a, c), e(a, d), e(b, d)], [e(a, c), e(b, d), e(b, c)]]
    return []


def iso_winding_table():
    """flip[p][case]: the triangles of that case of tetrahedron p are listed with their last two vertices exchanged.
    Generated in exact integer arithmetic (include/tpgan_ops.h): every edge vertex at its midpoint in doubled lattice
    coordinates, the sign of (q-p) x (r-p) . (sum of outside corners - sum of inside corners)."""
    flip = []
    for path in iso_tetrahedra():
        row = [False] * 16
        for case in range(1, 15):
            for tri in iso_case_triangles(case):
                p, q, r = ([path[a][x] + path[b][x] for x in range(3)] for a, b in tri)
                u, v = [q[x] - p[x] for x in range(3)], [r[x] - p[x] for x in range(3)]
                n = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
                side = [sum((-2 if case >> a & 1 else 2) * path[a][x] for a in range(4)) for x in range(3)]
                s = sum(n[x] * side[x] for x in range(3))
                _need(s != 0, "a degenerate tetrahedron")
                row[case] = s < 0
        flip.append(row)
    return flip


def _iso_surface_torch(field, origin, step, iso, normals=True):
    """The isosurface rule as vectorised torch ops (fp32, one rounding per operation): what backends without the
    kernels run.  field (nx,ny,nz) f32 with every extent >= 2, origin 3 host floats, step and iso fp32-exact floats."""
    f, dev = field, field.device
    nx, ny, nz = f.shape
    inside = f >= iso                                                        # NaN: outside
    active = torch.zeros((nx, ny, nz, 7), dtype=torch.bool, device=dev)
    for d, (dx, dy, dz) in enumerate(ISO_DIRECTIONS):
        active[:nx - dx, :ny - dy, :nz - dz, d] = inside[:nx - dx, :ny - dy, :nz - dz] != inside[dx:, dy:, dz:]
    flat = active.reshape(-1)
    vid = (torch.cumsum(flat, 0) - flat.long()).view(nx, ny, nz, 7)          # the vertex number of edge 7 n + d
    keys = torch.nonzero(flat).squeeze(1)
    node, d = torch.div(keys, 7, rounding_mode="floor"), keys % 7
    ij = torch.div(node, nz, rounding_mode="floor")
    ia = torch.stack([torch.div(ij, ny, rounding_mode="floor"), ij % ny, node % nz], 1)
    ib = ia + torch.tensor(ISO_DIRECTIONS, dtype=torch.int64, device=dev)[d]

    def at(table, idx):
        return table[idx[:, 0], idx[:, 1], idx[:, 2]]
    fa, fb = at(f, ia), at(f, ib)
    t = ((iso - fa) / (fb - fa)).unsqueeze(1)
    org = torch.from_numpy(np.asarray(origin, dtype=np.float32)).to(dev).view(1, 3)
    pa, pb = org + ia.float() * step, org + ib.float() * step
    vertices = pa + t * (pb - pa)
    nrm = None
    if normals:
        g = []
        for a, n in enumerate((nx, ny, nz)):
            idx = torch.arange(n, device=dev)
            g.append(f.index_select(a, (idx + 1).clamp(max=n - 1)) - f.index_select(a, (idx - 1).clamp(min=0)))
        g = torch.stack(g, -1)
        ga, gb = at(g, ia), at(g, ib)
        gv = ga + t * (gb - ga)
        # (sqrtf of the rule is correctly rounded, torch's fp32 sqrt on the CPU is not always: through float64, as the
        # simulator's statement does)
        sq = (gv[:, 0] * gv[:, 0] + gv[:, 1] * gv[:, 1]) + gv[:, 2] * gv[:, 2]
        length = torch.sqrt(sq.double()).float().unsqueeze(1)
        nrm = torch.where(length == 0, torch.zeros_like(gv), -gv / length)

    paths, flip = iso_tetrahedra(), iso_winding_table()
    cx, cy, cz = nx - 1, ny - 1, nz - 1
    cells = torch.arange(nx * ny * nz, device=dev).view(nx, ny, nz)[:cx, :cy, :cz]
    faces, order = [], []
    for p, path in enumerate(paths):
        corner = [inside[o[0]:o[0] + cx, o[1]:o[1] + cy, o[2]:o[2] + cz] for o in path]
        case = sum(corner[a].long() << a for a in range(4))
        for c in range(1, 15):
            where = torch.nonzero(case == c)
            if where.shape[0] == 0:
                continue
            for number, tri in enumerate(iso_case_triangles(c)):
                if flip[p][c]:
                    tri = [tri[0], tri[2], tri[1]]
                cols = []
                for a, b in tri:
                    direction = ISO_DIRECTIONS.index(tuple(path[b][x] - path[a][x] for x in range(3)))
                    owner = where + torch.tensor(path[a], dtype=torch.int64, device=dev)
                    cols.append(vid[owner[:, 0], owner[:, 1], owner[:, 2], direction])
                faces.append(torch.stack(cols, 1))
                order.append((at(cells, where) * 6 + p) * 2 + number)
    if not faces:
        return vertices, torch.zeros((0, 3), dtype=torch.int32, device=dev), nrm
    faces = torch.cat(faces)[torch.argsort(torch.cat(order))]               # the keys are distinct
    return vertices, faces.to(torch.int32), nrm


def iso_surface(field, origin, step, iso, normals=True):
    """The surface field >= iso of a scalar field on a regular lattice as a triangle mesh: marching tetrahedra on the Kuhn
    split of every lattice cube (csrc/isosurface.hip; the rule in full: include/tpgan_ops.h).  This project's own mesher:
    no parity with any external reconstruction tool is claimed.

    field (nx,ny,nz) fp32, node (i,j,k) at origin + (i,j,k) * step; origin: 3 HOST floats; step > 0; iso finite.
    -> (vertices (V,3) f32, faces (F,3) int32 wound so that the normals point to lower values, normals (V,3) f32 from
    the field's central differences, or None).  Where every boundary node is below iso the mesh is closed and
    consistently oriented.  One host read (the two counts) between the two launches' groups.  At most 2^27 nodes; an
    extent below 2 gives an empty mesh.  Bit-identical from run to run, order included, and equal to
    `_iso_surface_torch`, which backends without the kernels run (CPU tensors need a registered checker).  No gradient."""
    _check_float(field, "field", 3)
    origin = np.ascontiguousarray(np.asarray(origin, dtype=np.float32).reshape(-1))
    _need(origin.shape == (3,) and bool(np.isfinite(origin).all()), "origin must be 3 finite values")
    step, iso = float(_F32(step)), float(_F32(iso))
    _need(np.isfinite(step) and step > 0.0, "step must be positive and finite")
    _need(np.isfinite(iso), "iso must be finite")
    nx, ny, nz = field.shape
    _need(nx * ny * nz <= ISO_MAX_NODES, f"a lattice holds at most 2^27 nodes, got {nx} x {ny} x {nz}")
    be = backend_for(field)
    dev = field.device
    if min(nx, ny, nz) < 2:
        return (torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.int32, device=dev),
                torch.zeros((0, 3), dtype=torch.float32, device=dev) if normals else None)
    with torch.no_grad():
        if hasattr(be, "iso_surface"):
            return be.iso_surface(field.detach(), origin, step, iso, bool(normals))
        return _iso_surface_torch(field.detach(), origin, step, iso, bool(normals))


def _radius_cubic_sums_torch(query, pos, r, pairs_per_chunk=1 << 24):
    """`radius_reduce(query, pos, r, "cubic")[1]` for one cloud as torch ops, the same bits: the canonical fp32 distance,
    members d2 <= r2, every term truncated to 64-bit fixed point (unit 2^-32), integer sums, one conversion back
    (csrc/radius_reduce.hip).  query (Nq,3), pos (Np,3) fp32 -> (Nq,) fp32.  What backends without the kernel run."""
    r32 = float(_F32(r))
    r2 = float(_F32(r32) * _F32(r32))
    out = torch.zeros(query.shape[0], dtype=torch.float32, device=query.device)
    if pos.shape[0] == 0 or query.shape[0] == 0:
        return out
    rows = max(1, pairs_per_chunk // pos.shape[0])
    px, py, pz = pos[:, 0].unsqueeze(0), pos[:, 1].unsqueeze(0), pos[:, 2].unsqueeze(0)
    for a in range(0, query.shape[0], rows):
        q = query[a:a + rows]
        dx, dy, dz = q[:, 0:1] - px, q[:, 1:2] - py, q[:, 2:3] - pz
        d2 = dx * dx
        d2 = d2 + dy * dy
        d2 = d2 + dz * dz
        u = torch.clamp(torch.sqrt(d2.double()).float() / r32, max=1.0)      # a correctly rounded fp32 sqrt
        u2 = u * u
        near = 6.0 * (u2 * u - u2) + 1.0
        v = 1.0 - u
        far = 2.0 * (v * v * v)
        w = torch.clamp(torch.where(u <= 0.5, near, far), min=0.0)
        units = torch.where(d2 <= r2, (w * 4294967296.0).to(torch.int64), torch.zeros((), dtype=torch.int64, device=w.device))
        out[a:a + rows] = units.sum(1).to(torch.float32) * 2.3283064365386963e-10
    return out


# ------------------------------------------------- anisotropic kernels (csrc/aniso.hip; the rule: include/tpgan_ops.h)
def _aniso_params(cov_radius, ks, smooth_lambda, kr, s_min, s_max, kn, n_eps):
    """The stage-A parameters, validated and each rounded to fp32 once -> (rc, lambda, ks, kr, s_min, s_max, kn, n_eps)."""
    vals = [float(_F32(v)) for v in (cov_radius, smooth_lambda, ks, kr, s_min, s_max, kn)]
    rc, lam, ks, kr, s_min, s_max, kn = vals
    for name, v in (("cov_radius", rc), ("ks", ks), ("s_min", s_min), ("s_max", s_max), ("kn", kn)):
        _need(np.isfinite(v) and v > 0.0, f"{name} must be positive and finite")
    _need(np.isfinite(kr) and kr >= 1.0, "kr must be finite and at least 1")
    _need(0.0 <= lam <= 1.0, "smooth_lambda must lie in [0, 1]")
    _need(s_min <= s_max, "s_min must not exceed s_max")
    _need(int(n_eps) == n_eps and n_eps >= 0, "n_eps must be a non-negative integer")
    return rc, lam, ks, kr, s_min, s_max, kn, int(n_eps)


def _sqrt64(t):
    """A correctly rounded float64 square root of a float64 tensor: torch's own on the CPU is not (about one value in
    150 is an ulp off), numpy's is, and the statements below must give the device's bits.  Through host memory: the
    statements serve checkers, not a hot path."""
    return torch.from_numpy(np.sqrt(t.detach().cpu().numpy())).to(t.device)


def _aniso_rotate_torch(app, aqq, apq, arp, arq, vp, vq):
    """One Jacobi rotation of the rule, float64, on every particle at once."""
    zero = apq == 0.0
    theta = (aqq - app) / torch.where(zero, torch.ones_like(apq), 2.0 * apq)
    sg = torch.where(theta >= 0.0, 1.0, -1.0).to(theta.dtype)
    t = sg / (theta.abs() + _sqrt64(theta * theta + 1.0))
    t = torch.where(zero, torch.zeros_like(t), t)
    c = 1.0 / _sqrt64(t * t + 1.0)
    s = t * c
    h = t * apq
    new_vp = [c * a - s * e for a, e in zip(vp, vq)]
    new_vq = [s * a + c * e for a, e in zip(vp, vq)]
    return app - h, aqq + h, torch.zeros_like(apq), c * arp - s * arq, s * arp + c * arq, new_vp, new_vq


def _aniso_kernels_torch(points, prm, pairs_per_chunk=1 << 22):
    """Stage A of the anisotropic kernels for one cloud as torch ops, the same bits as the kernels: points (N,3) fp32 ->
    (centres (N,3), G (N,6), det (N,) fp32, count (N,) int32).  What backends without the kernels run."""
    rc, lam, ks, kr, s_min, s_max, kn, n_eps = prm
    N, dev = points.shape[0], points.device
    rc2 = float(_F32(rc) * _F32(rc))
    S = torch.zeros((10, N), dtype=torch.int64, device=dev)
    count = torch.zeros(N, dtype=torch.int32, device=dev)
    px, py, pz = points[:, 0].unsqueeze(0), points[:, 1].unsqueeze(0), points[:, 2].unsqueeze(0)
    rows = max(1, pairs_per_chunk // max(N, 1))
    for a in range(0, N, rows):
        qx, qy, qz = points[a:a + rows, 0:1], points[a:a + rows, 1:2], points[a:a + rows, 2:3]
        dx, dy, dz = qx - px, qy - py, qz - pz
        d2 = dx * dx
        d2 = d2 + dy * dy
        d2 = d2 + dz * dz
        member = d2 <= rc2
        d = torch.sqrt(d2.double()).float()                                   # a correctly rounded fp32 sqrt
        rho = torch.fmin(d / rc, torch.ones((), dtype=torch.float32, device=dev))
        w = 1.0 - (rho * rho) * rho
        ux, uy, uz = (px - qx) / rc, (py - qy) / rc, (pz - qz) / rc
        wx, wy, wz = w * ux, w * uy, w * uz
        terms = (w, wx, wy, wz, wx * ux, wx * uy, wx * uz, wy * uy, wy * uz, wz * uz)
        for k, term in enumerate(terms):
            units = (torch.where(member, term, torch.zeros_like(term)) * 4294967296.0).to(torch.int64)
            S[k, a:a + rows] = units.sum(1)
        count[a:a + rows] = member.sum(1).to(torch.int32)
    Sd = S.double()
    S0 = torch.where(Sd[0] > 0.0, Sd[0], torch.ones_like(Sd[0]))
    m = [Sd[1] / S0, Sd[2] / S0, Sd[3] / S0]
    lr = float(np.float64(_F32(lam)) * np.float64(_F32(rc)))
    centres = torch.stack([(points[:, a].double() + lr * m[a]).float() for a in range(3)], 1)
    a00, a01, a02 = Sd[4] / S0 - m[0] * m[0], Sd[5] / S0 - m[0] * m[1], Sd[6] / S0 - m[0] * m[2]
    a11, a12, a22 = Sd[7] / S0 - m[1] * m[1], Sd[8] / S0 - m[1] * m[2], Sd[9] / S0 - m[2] * m[2]
    one, nil = torch.ones_like(a00), torch.zeros_like(a00)
    V = [[one, nil, nil], [nil, one, nil], [nil, nil, one]]                   # V[k][column]

    def col(j):
        return [V[0][j], V[1][j], V[2][j]]

    def put(j, v):
        for k in range(3):
            V[k][j] = v[k]
    for _ in range(5):
        a00, a11, a01, a02, a12, vp, vq = _aniso_rotate_torch(a00, a11, a01, a02, a12, col(0), col(1))
        put(0, vp), put(1, vq)
        a00, a22, a02, a01, a12, vp, vq = _aniso_rotate_torch(a00, a22, a02, a01, a12, col(0), col(2))
        put(0, vp), put(2, vq)
        a11, a22, a12, a01, a02, vp, vq = _aniso_rotate_torch(a11, a22, a12, a01, a02, col(1), col(2))
        put(1, vp), put(2, vq)
    top = torch.where(a00 > a11, a00, a11)
    top = torch.where(top > a22, top, a22)
    few = (count <= n_eps) | ~(top > 0.0)
    fl = top / kr
    e = []
    for sig in (a00, a11, a22):
        x = ks * torch.where(sig > fl, sig, fl)
        x = torch.where(x < s_min, torch.full_like(x, s_min), x)
        e.append(torch.where(x > s_max, torch.full_like(x, s_max), x))
    inv = [1.0 / x for x in e]
    inv_kn = 1.0 / np.float64(kn)
    G = []
    for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)):
        g = ((V[a][0] * inv[0]) * V[b][0] + (V[a][1] * inv[1]) * V[b][1]) + (V[a][2] * inv[2]) * V[b][2]
        G.append(torch.where(few, torch.full_like(g, float(inv_kn) if a == b else 0.0), g).float())
    det = 1.0 / ((e[0] * e[1]) * e[2])
    det = torch.where(few, torch.full_like(det, float(1.0 / ((np.float64(kn) * kn) * kn))), det).float()
    return centres, torch.stack(G, 1), det, count


def _aniso_field_torch(query, centres, G, det, support, reach, pairs_per_chunk=1 << 22, query_rows=8192):
    """Stage B of the anisotropic kernels for one cloud as torch ops, the same bits as the kernels: query (Nq,3), centres
    (Np,3), G (Np,6), det (Np,) fp32 -> (Nq,) fp32.  A chunk of queries meets only the centres within reach of its
    bounding box (with a margin): every other centre is no member and would add exactly 0."""
    R, reach = float(_F32(support)), float(_F32(reach))
    reach2 = float(_F32(reach) * _F32(reach))
    dev = query.device
    out = torch.zeros(query.shape[0], dtype=torch.float32, device=dev)
    if centres.shape[0] == 0 or query.shape[0] == 0:
        return out
    one = torch.ones((), dtype=torch.float32, device=dev)
    nil = torch.zeros((), dtype=torch.float32, device=dev)
    for first in range(0, query.shape[0], query_rows):
        chunk = query[first:first + query_rows]
        finite = torch.isfinite(chunk).all(1)
        if not bool(finite.any()):
            continue
        lo, hi = chunk[finite].amin(0) - 1.001 * reach, chunk[finite].amax(0) + 1.001 * reach
        keep = ((centres >= lo) & (centres <= hi)).all(1)
        c, g, dt = centres[keep], G[keep], det[keep].unsqueeze(0)
        if c.shape[0] == 0:
            continue
        cx, cy, cz = c[:, 0].unsqueeze(0), c[:, 1].unsqueeze(0), c[:, 2].unsqueeze(0)
        g = [g[:, k].unsqueeze(0) for k in range(6)]
        rows = max(1, pairs_per_chunk // c.shape[0])
        for a in range(0, chunk.shape[0], rows):
            q = chunk[a:a + rows]
            t0, t1, t2 = q[:, 0:1] - cx, q[:, 1:2] - cy, q[:, 2:3] - cz
            d2 = t0 * t0
            d2 = d2 + t1 * t1
            d2 = d2 + t2 * t2
            y0 = (g[0] * t0 + g[1] * t1) + g[2] * t2
            y1 = (g[1] * t0 + g[3] * t1) + g[4] * t2
            y2 = (g[2] * t0 + g[4] * t1) + g[5] * t2
            yy = (y0 * y0 + y1 * y1) + y2 * y2
            u = torch.fmin(torch.sqrt(yy.double()).float() / R, one)
            u2 = u * u
            near = 6.0 * (u2 * u - u2) + 1.0
            v = 1.0 - u
            far = 2.0 * (v * v * v)
            w = torch.fmax(torch.where(u <= 0.5, near, far), nil)
            dw = torch.fmin(torch.fmax(dt * w, nil), 512.0 * one)
            units = torch.where(d2 <= reach2, (dw * 4194304.0).to(torch.int64),
                                torch.zeros((), dtype=torch.int64, device=dev))
            out[first + a:first + a + q.shape[0]] = units.sum(1).to(torch.float32) * 2.384185791015625e-7
    return out


def anisotropic_kernels(points, cov_radius, ks, smooth_lambda=0.9, kr=4.0, s_min=0.125, s_max=2.0, kn=0.5, n_eps=25,
                        lengths=None, _grid=None):
    """Stage A of the anisotropic surface kernels (Yu and Turk; csrc/aniso.hip, the rule in full: include/tpgan_ops.h):
    per particle the smoothed centre and the symmetric matrix G = V diag(1/s) V^T of the ellipsoid fitted to the weighted
    covariance of its neighbours within `cov_radius` -> (centres (B,N,3) f32, G (B,N,6) f32 as xx xy xz yy yz zz,
    det (B,N) f32 = 1 / (s0 s1 s2), count (B,N) int32, the neighbours within cov_radius, the particle included).

    points (B,N,3) float tensor on the GPU, or unbatched (N,3); lengths (B,) or None (rows beyond get zeros).  ks scales
    the extents (1 / `mesh.lattice_covariance` makes a full lattice's kernel the isotropic one); a particle with at most
    n_eps neighbours is a ball of extent kn.  Deterministic: the same bits from run to run, at every batch position and
    from both launch shapes, and equal to `_aniso_kernels_torch`, which backends without the kernels run (CPU tensors
    need a registered checker).  No gradient."""
    _need(isinstance(points, torch.Tensor) and points.is_floating_point(), "points must be a float tensor")
    squeeze = points.dim() == 2
    if squeeze:
        points = points.unsqueeze(0)
    _need(points.dim() == 3 and points.shape[2] == 3, "points must be (B,N,3) or (N,3)")
    prm = _aniso_params(cov_radius, ks, smooth_lambda, kr, s_min, s_max, kn, n_eps)
    p = points.detach().float().contiguous()
    be = backend_for(p)
    B, N = p.shape[:2]
    ln = _lengths(lengths, B, N, p.device)
    with torch.no_grad():
        if hasattr(be, "aniso_kernels"):
            out = be.aniso_kernels(p, ln, prm, _grid)
        else:
            out = (torch.zeros((B, N, 3)), torch.zeros((B, N, 6)), torch.zeros((B, N)), torch.zeros((B, N), dtype=torch.int32))
            out = tuple(t.to(p.device) for t in out)
            for b in range(B):
                n = N if ln is None else min(max(int(ln[b]), 0), N)
                for dst, src in zip(out, _aniso_kernels_torch(p[b, :n], prm)):
                    dst[b, :n] = src
    return tuple(t[0] for t in out) if squeeze else out


def anisotropic_field(query, centres, G, det, support, s_max=2.0, lengths_q=None, lengths_p=None, _grid=None):
    """Stage B of the anisotropic surface kernels: at every query the sum over the centres within s_max * support of
    det_j * W(|G_j (x - centre_j)| / support), W the cubic kernel of `radius_reduce` -> (B,Nq) f32.

    query (B,Nq,3), centres (B,Np,3), G (B,Np,6), det (B,Np) float tensors on the GPU (what `anisotropic_kernels`
    returned), or all unbatched; lengths as in `radius_reduce`.  Deterministic like stage A and equal to
    `_aniso_field_torch`.  No gradient."""
    tensors = (query, centres, G, det)
    _need(all(isinstance(t, torch.Tensor) and t.is_floating_point() for t in tensors),
          "query, centres, G and det must be float tensors")
    squeeze = query.dim() == 2
    if squeeze:
        _need(centres.dim() == 2 and G.dim() == 2 and det.dim() == 1, "query (Nq,3) needs centres (Np,3), G (Np,6), det (Np,)")
        query, centres, G, det = (t.unsqueeze(0) for t in tensors)
    _need(query.dim() == 3 and query.shape[2] == 3 and centres.dim() == 3 and centres.shape[2] == 3,
          "query (B,Nq,3), centres (B,Np,3)")
    B, Np = centres.shape[:2]
    _need(query.shape[0] == B and tuple(G.shape) == (B, Np, 6) and tuple(det.shape) == (B, Np),
          "centres (B,Np,3) need G (B,Np,6) and det (B,Np)")
    _same_device(query, centres, G, det)
    support32, smax32 = float(_F32(support)), float(_F32(s_max))
    _need(np.isfinite(support32) and support32 > 0.0, "support must be positive and finite")
    _need(np.isfinite(smax32) and smax32 > 0.0, "s_max must be positive and finite")
    reach = float(_F32(smax32) * _F32(support32))
    q, c, g, d = (t.detach().float().contiguous() for t in (query, centres, G, det))
    be = backend_for(q)
    Nq = q.shape[1]
    lq, lp = _lengths(lengths_q, B, Nq, q.device), _lengths(lengths_p, B, Np, q.device)
    with torch.no_grad():
        if hasattr(be, "aniso_field"):
            total = be.aniso_field(q, c, g, d, lq, lp, support32, reach, _grid)
        else:
            total = torch.zeros((B, Nq), dtype=torch.float32, device=q.device)
            for b in range(B):
                nq = Nq if lq is None else min(max(int(lq[b]), 0), Nq)
                n = Np if lp is None else min(max(int(lp[b]), 0), Np)
                total[b, :nq] = _aniso_field_torch(q[b, :nq], c[b, :n], g[b, :n], d[b, :n], support32, reach)
    return total[0] if squeeze else total


def cubic_interpolation(query_pos, field, pos, cutoff):
    """Bicubic-kernel interpolation of `field` (given at `pos`) at `query_pos` within `cutoff`:
    gcn_lib/interpolation.py:107-123 for a whole batch in one launch (the reference loops over
    frames and samples in Python, train_step_final.py:51-66, building a DGL graph per call).

    query_pos (B,Nq,3), field (B,Np,F), pos (B,Np,3) -> (B,Nq,F); unbatched 2-D inputs are
    accepted like the reference's and return (Nq,F).  No gradient (the reference calls it under
    no_grad).  Includes the reference's kNN-padding rule: in a cloud where some query has no
    field point within the cutoff, every query with fewer than 32 hits counts its 4 nearest hits
    twice (include/tpgan_ops.h)."""
    squeeze = query_pos.dim() == 2
    if squeeze:
        query_pos, field, pos = query_pos.unsqueeze(0), field.unsqueeze(0), pos.unsqueeze(0)
    _need(query_pos.dim() == 3 and pos.dim() == 3 and field.dim() == 3, "query (B,Nq,3), field (B,Np,F), pos (B,Np,3)")
    _need(query_pos.shape[2] == 3 and pos.shape[2] == 3 and field.shape[:2] == pos.shape[:2]
          and query_pos.shape[0] == pos.shape[0], "shape mismatch")
    _same_device(query_pos, pos)
    q = query_pos.detach().float().contiguous()
    p = pos.detach().float().contiguous()
    f = field.detach().float().contiguous()
    plain, pad, hits = backend_for(q).cubic_interp(q, p, f, float(cutoff))
    padded_cloud = (hits == 0).any(dim=1, keepdim=True)                  # some query without any hit
    out = torch.where((padded_cloud & (hits < 32)).unsqueeze(-1), pad, plain)
    return out[0] if squeeze else out


class _KnnDists(torch.autograd.Function):
    """Attaches the analytic gradient of squared distances to searched dists."""

    @staticmethod
    def forward(ctx, p1, p2, dists, idx, valid):
        ctx.save_for_backward(p1, p2, idx, valid)
        return dists.clone()

    @staticmethod
    def backward(ctx, g):
        p1, p2, idx, valid = ctx.saved_tensors
        B, P1, K = idx.shape
        D = p1.shape[2]
        safe = idx.clamp(min=0)
        nb = torch.gather(p2.unsqueeze(1).expand(B, P1, p2.shape[1], D), 2,
                          safe.unsqueeze(-1).expand(B, P1, K, D))
        diff = (p1.unsqueeze(2) - nb) * (2.0 * g * valid).unsqueeze(-1)
        g1 = diff.sum(2)
        g2 = torch.zeros_like(p2)
        g2.scatter_add_(1, safe.reshape(B, P1 * K, 1).expand(B, P1 * K, D), -diff.reshape(B, P1 * K, D))
        return g1, g2, None, None, None


def attach_dist_grad(p1, p2, dists, idx, lengths1=None, lengths2=None):
    """dists (B,P1,K) of a search of p1 in p2 -> the same values with the gradient of |p1 - p2[idx]|^2 attached.
    A slot the search did not fill is a constant and takes no gradient: the -1 / -1 slots of a radius search, and
    the 0 / 0 slots of a kNN search (include/tpgan_ops.h: k >= the cloud's length, rows beyond lengths1) -- those
    cannot be told from a hit by their index, so pass the lengths the search was given."""
    if torch.is_grad_enabled() and (p1.requires_grad or p2.requires_grad):
        B, P1, K = idx.shape
        valid = idx >= 0
        if lengths2 is not None or K > p2.shape[1]:
            n2 = (torch.full((B,), p2.shape[1], device=idx.device) if lengths2 is None
                  else torch.as_tensor(lengths2, device=idx.device))
            valid = valid & (torch.arange(K, device=idx.device)[None, None, :] < n2[:, None, None])
        if lengths1 is not None:
            n1 = torch.as_tensor(lengths1, device=idx.device)
            valid = valid & (torch.arange(P1, device=idx.device)[None, :, None] < n1[:, None, None])
        return _KnnDists.apply(p1.float(), p2.float(), dists, idx, valid)
    return dists


# ------------------------------------------------------------------ Chamfer
class _ChamferNN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, tgt):
        d1, i1, d2, i2 = backend_for(src).chamfer_fwd(src, tgt)
        ctx.save_for_backward(src, tgt, i1, i2)
        ctx.mark_non_differentiable(i1, i2)
        return d1, d2, i1, i2

    @staticmethod
    def backward(ctx, g1, g2, _gi1, _gi2):
        src, tgt, i1, i2 = ctx.saved_tensors
        gs, gt = backend_for(src).chamfer_bwd(src, tgt, i1, i2, g1.contiguous().float(),
                                              g2.contiguous().float())
        return gs, gt


def chamfer_nn(src, tgt):
    """(B,N,3),(B,M,3) -> d1 (B,N), d2 (B,M), i1, i2; differentiable wrt both clouds."""
    _need(src.dim() == 3 and tgt.dim() == 3 and src.shape[2] == 3 and tgt.shape[2] == 3,
          "clouds must be (B,N,3)")
    _need(src.shape[0] == tgt.shape[0], "batch mismatch")
    _same_device(src, tgt)
    return _ChamferNN.apply(src.float().contiguous(), tgt.float().contiguous())


# ------------------------------------------------------- channels-last row combine
ROW_GATHER, ROW_SUB, ROW_EDGE = 0, 1, 2


class _RowCombine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, U, QE, idx, mode, slope, out_dtype, inverse):
        be = backend_for(U)
        out = be.rowcombine_fwd(U, QE, idx, mode, slope, out_dtype)
        ctx.save_for_backward(idx, QE if mode == ROW_EDGE else None)
        ctx.inverse = inverse          # (offs, lst) int32 tensors prepared ahead of time, or None
        ctx.mode, ctx.slope, ctx.N, ctx.in_dtype = mode, slope, U.shape[1], U.dtype
        ctx.has_q = QE is not None
        return out

    @staticmethod
    def backward(ctx, gout):
        idx, E = ctx.saved_tensors
        gout = gout.contiguous()
        if gout.dtype not in _DTYPE_CODE:
            gout = gout.float()
        kw = {} if ctx.inverse is None else {"inverse": ctx.inverse}
        gU, gQE = backend_for(gout).rowcombine_bwd(gout, idx, E, ctx.mode, ctx.N, ctx.slope, ctx.in_dtype, **kw)
        return gU, (gQE if ctx.has_q else None), None, None, None, None, None


_DEFERRED_INVERSES = []        # stack of lists: inside `deferred_inverses()` NeighbourList.with_inverse only notes the list


class NeighbourList:
    """A neighbour list as the row gathers take it: idx (B,S,K) contiguous int32 into `n_src` source rows per cloud,
    and `inverse` = (offs, lst), the inverted index (tpg_invert_index) a row gather's BACKWARD reads, or None while
    nobody has prepared it (the backward then launches the inversion itself)."""
    __slots__ = ("idx", "n_src", "inverse")

    def __init__(self, idx, n_src, inverse=None):
        _need(idx.dtype == torch.int32 and idx.dim() == 3 and idx.is_contiguous(), "idx must be contiguous (B,S,K) int32")
        self.idx, self.n_src, self.inverse = idx, int(n_src), inverse

    def clouds(self, lo, hi):
        """Clouds lo..hi (a view: the clouds are the leading, contiguous axis), without an inverse."""
        return NeighbourList(self.idx[lo:hi], self.n_src)

    @staticmethod
    def cat(lists):
        """Lists into the same number of source rows, stacked along the cloud axis (no inverse yet)."""
        _need(all(l.n_src == lists[0].n_src for l in lists), "neighbour lists into different numbers of source rows")
        return NeighbourList(torch.cat([l.idx for l in lists], 0), lists[0].n_src)

    def with_inverse(self):
        """Prepare the inverted index NOW (on the current stream) -- index-only work like FPS and the ball query, so an
        index plan can take it off the critical path -- or, inside `deferred_inverses()`, note the list for
        `run_inverses`.  Returns self."""
        if _DEFERRED_INVERSES:
            _DEFERRED_INVERSES[-1].append(self)
            return self
        be = backend_for(self.idx)
        if hasattr(be, "invert_index"):
            self.inverse = be.invert_index(self.idx, self.n_src)
        return self

    def tensors(self):
        return [self.idx] + list(self.inverse or ())


def neighbour_list(idx, n_src):
    """What a row gather over `n_src` source rows was handed as its list -> NeighbourList: a bare (B,S,K) int32 tensor
    is a list without a prepared inverse; a NeighbourList must be one into that many rows (its inverse would be the
    inverse of another gather: a caller error, not a reason to invert again)."""
    if isinstance(idx, NeighbourList):
        _need(idx.n_src == n_src, f"neighbour list into {idx.n_src} source rows used on {n_src}")
        return idx
    _need(torch.is_tensor(idx) and idx.dim() == 3 and idx.dtype == torch.int32, "idx must be (B,S,K) int32")
    return NeighbourList(idx.contiguous(), n_src)


def row_combine(U, QE, idx, mode, slope=0.2, out_dtype=None):
    """Channels-last gather of first-layer rows (include/tpgan_ops.h, tpg_rowcombine_fwd).

    U (B,N,C); QE (B,S,C) or None; idx (B,S,K) int32 or a NeighbourList into N rows -> (B,S,K,C).
      ROW_GATHER: U[idx]      ROW_SUB: U[idx] - QE[s]      ROW_EDGE: U[idx] + lrelu(QE[idx] - QE[s])
    U/QE fp32 or bf16; out_dtype defaults to U.dtype (fp32 in -> bf16 out is supported)."""
    _need(U.dim() == 3, "U (B,N,C), idx (B,S,K) int32")
    nl = neighbour_list(idx, U.shape[1])
    idx = nl.idx
    _need(U.dtype in _DTYPE_CODE, f"row_combine supports fp32/bf16, got {U.dtype}")
    _need(U.shape[0] == idx.shape[0], "batch mismatch")
    out_dtype = out_dtype or U.dtype
    U = U.contiguous()
    if mode == ROW_GATHER:
        QE = None
    else:
        _need(QE is not None and QE.shape == (U.shape[0], idx.shape[1], U.shape[2]), "QE must be (B,S,C)")
        QE = QE.to(U.dtype).contiguous()
        if mode == ROW_EDGE:
            _need(idx.shape[1] == U.shape[1], "EDGE mode needs S == N")
    ne = 4 if (U.dtype == torch.float32 and out_dtype == torch.float32) else 8
    _need(U.shape[2] % ne == 0, f"channel count {U.shape[2]} must be a multiple of {ne}")
    return _RowCombine.apply(U, QE, idx, mode, float(slope), out_dtype, nl.inverse)


class deferred_inverses:
    """with deferred_inverses() as pending: ... -- `NeighbourList.with_inverse` calls inside launch nothing;
    `run_inverses(pending)` launches them later (on the stream current then).  The inverted index is read by a row
    gather's BACKWARD only, so an index plan can hand its lists to the forward first and build the inverses behind
    that (gan_step_graph: ~150 us earlier start of a discriminator update)."""

    def __enter__(self):
        self.pending = []
        _DEFERRED_INVERSES.append(self.pending)
        return self.pending

    def __exit__(self, *exc):
        _DEFERRED_INVERSES.pop()
        return False


def run_inverses(pending):
    for nl in pending:
        nl.with_inverse()
    del pending[:]


def attach_inverse(idx, N):
    """A bare neighbour list idx (B,S,K) contiguous int32 into N source rows -> the NeighbourList that carries its
    inverted index (`NeighbourList.with_inverse`): `row_combine` hands it to its backward, which then skips its own
    tpg_invert_index launch."""
    return NeighbourList(idx, N).with_inverse()


# ------------------------------------------------ head: BatchNorm1d + LeakyReLU + dropout mask
class _HeadBNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, gamma, beta, running_mean, running_var, nbt, momentum, eps, slope, mask):
        be = backend_for(h)
        y, mean, rstd = be.head_bn_act_fwd(h, gamma, beta, running_mean, running_var, nbt, momentum, eps, slope, mask)
        ctx.save_for_backward(h, mean, rstd, gamma, beta, mask)
        ctx.slope = slope
        return y

    @staticmethod
    def backward(ctx, gy):
        h, mean, rstd, gamma, beta, mask = ctx.saved_tensors
        need_affine = (gamma is not None and ctx.needs_input_grad[1]) or (beta is not None and ctx.needs_input_grad[2])
        dh, dg, db = backend_for(gy).head_bn_act_bwd(gy.contiguous().float(), h, mean, rstd, gamma, beta, ctx.slope, mask,
                                                     need_affine)
        return (dh, dg if gamma is not None else None, db if beta is not None else None, None, None, None, None, None,
                None, None)


def head_bn_act(h, bn, slope, mask=None):
    """Training-mode nn.BatchNorm1d `bn` (running statistics and batch counter updated like the module does) + LeakyReLU
    (slope) + the product with a dropout's scaled keep mask, on the (B,C) fp32 rows of a head: one launch each way
    (include/tpgan_ops.h, tpg_head_bn_act_*)."""
    _need(h.dim() == 2 and h.dtype == torch.float32, "h must be (B,C) fp32")
    _need(bn.momentum is not None and bn.track_running_stats, "needs a BatchNorm1d with a fixed momentum and running statistics")
    _need(h.shape[0] > 1, "Expected more than 1 value per channel when training")
    return _HeadBNAct.apply(h.contiguous(), bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                            float(bn.momentum), float(bn.eps), float(slope),
                            None if mask is None else mask.contiguous().float())


# ------------------------------------------------ fused BatchNorm + LeakyReLU (+ max over K)
class _RowBNAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, slope, K, out_dtype,
                num_batches_tracked, nseg, mean_shift):
        be = backend_for(x)
        C_ = x.shape[1]
        if training:
            mean = torch.empty((nseg, C_), dtype=torch.float32, device=x.device)
            rstd = torch.empty((nseg, C_), dtype=torch.float32, device=x.device)
        elif running_mean is None:                  # identity statistics: activation (+max) only
            mean = rstd = None
        else:
            mean = running_mean.float().contiguous()
            if mean_shift is not None:
                mean = mean - mean_shift.float()
            rstd = torch.rsqrt(running_var.float() + eps)
        y, arg = be.rowbn_fwd(x, K, eps, momentum, training, running_mean if training else None,
                              running_var if training else None, gamma, beta, slope, mean, rstd, out_dtype,
                              num_batches_tracked if training else None, **({"nseg": nseg} if nseg != 1 else {}),
                              **({"mean_shift": mean_shift} if mean_shift is not None and training else {}))
        # K > 0: the (small) output doubles as the backward's source of the arg-max pre-activations
        ctx.save_for_backward(x, gamma, beta, mean, rstd, arg, y if K else None)
        ctx.cfg = (training, slope, K, nseg)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, gamma, beta, mean, rstd, arg, y = ctx.saved_tensors
        training, slope, K, nseg = ctx.cfg
        gy = gy.contiguous()
        if gy.dtype not in _DTYPE_CODE:
            gy = gy.float()
        need_affine = gamma is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        dx, dgamma, dbeta = backend_for(x).rowbn_bwd(gy, x, arg, K, training, mean, rstd, gamma, beta, slope,
                                                    need_affine, y, **({"nseg": nseg} if nseg != 1 else {}))
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None, None, None, None


def row_bn_act(x, gamma, beta, running_mean, running_var, training, momentum, eps, slope=1.0, K=0,
               out_dtype=None, num_batches_tracked=None, nseg=1, mean_shift=None):
    """Fused BatchNorm (+LeakyReLU, + max over groups of K rows) on rows (include/tpgan_ops.h).

    x (P,C) fp32/bf16 -> (P,C) or (P/K,C).  slope: 1.0 = no activation, 0.0 = ReLU.  In training mode
    the running statistics are updated in place (momentum, unbiased variance) like nn.BatchNorm,
    and `num_batches_tracked` (int64 scalar tensor, optional) is incremented by the same launch.
    Eval mode with running_mean = running_var = None means identity statistics.
    nseg > 1 (training): the rows are nseg equal consecutive blocks, each normalised with its own
    batch statistics -- nseg calls of the same module in one launch, running statistics updated
    block after block (see include/tpgan_ops.h).
    mean_shift (C) fp32, no gradient: a per-channel constant (the preceding conv's bias) that was
    left out of x; only the running mean needs it (BatchNorm(x + b) == BatchNorm(x))."""
    _need(x.dim() == 2 and x.dtype in _DTYPE_CODE, "x must be (P,C) fp32/bf16")
    _need(K == 0 or (0 < K <= 256 and x.shape[0] % K == 0), "K must divide the row count (<= 256)")
    _need(nseg >= 1 and x.shape[0] % nseg == 0 and (K == 0 or (x.shape[0] // nseg) % K == 0),
          "nseg must divide the rows (and K the rows of a segment)")
    if not training:
        nseg = 1                                      # fixed statistics: segments are meaningless
    out_dtype = out_dtype or x.dtype
    ne = 4 if (x.dtype == torch.float32 and out_dtype == torch.float32) else 8
    _need(x.shape[1] % ne == 0 and x.shape[1] <= 1024, f"channels must be a multiple of {ne}, <= 1024")
    if not training:
        _need((running_mean is None) == (running_var is None), "eval mode: both running statistics or neither")
    if num_batches_tracked is not None:
        _need(num_batches_tracked.dtype == torch.int64 and num_batches_tracked.numel() == 1
              and num_batches_tracked.device == x.device, "num_batches_tracked must be an int64 scalar on x's device")
    g = None if gamma is None else gamma.float().contiguous()
    b = None if beta is None else beta.float().contiguous()
    return _RowBNAct.apply(x.contiguous(), g, b, running_mean, running_var, bool(training), float(momentum),
                           float(eps), float(slope), int(K), out_dtype, num_batches_tracked, int(nseg),
                           None if mean_shift is None else mean_shift.detach().float().contiguous())


def row_act_max(x, slope, K, out_dtype=None):
    """max over each group of K consecutive rows of LeakyReLU(x): the [activation -> max over
    the k neighbours] tail of an EdgeConv MLP (gcn_lib/pointnet/gcn.py:211) in one pass, with a
    one-pass backward (same kernels as row_bn_act with identity statistics)."""
    return row_bn_act(x, None, None, None, None, False, 0.0, 0.0, slope, K, out_dtype)


# ------------------------------------------------------ fused MLP tail on MFMA tiles (bf16 rows)
MLP_CHANNELS = ((64, 64), (64, 128), (128, 64), (128, 128), (128, 256), (256, 128), (256, 256))


def _mlp_tail_fwd(x0, cfg, tensors):
    """Forward body of the fused tail (`_MlpTail`): -> (out, the tensors its backward body reads)."""
    nseg, K, slopes, eps, moms, states, shifts = cfg
    be = backend_for(x0)
    L = (len(tensors) - 2) // 3
    gam = [tensors[0]] + [tensors[3 * l + 3] for l in range(L)]
    bet = [tensors[1]] + [tensors[3 * l + 4] for l in range(L)]
    Ws = [tensors[3 * l + 2] for l in range(L)]
    xs, cis = [x0], []
    rm, rv, nbt = states[0]
    cis.append(be.rowbn_stats(x0, eps[0], moms[0], rm, rv, nbt, nseg, shifts[0], consts=(gam[0], bet[0]))[2])  # sc | sh | mu | rs
    for l in range(L):
        rm, rv, nbt = states[l + 1]
        y, ci, *mr = be.mlp_fwd(xs[-1], cis[-1], slopes[l], Ws[l], nseg, eps[l + 1], moms[l + 1], rm, rv, nbt,
                                shifts[l + 1], gam[l + 1], bet[l + 1], mean_rstd=(l == L - 1))
        xs.append(y)
        cis.append(ci)
    mean_L, rstd_L = mr                          # of the last BatchNorm, written by the same finalize launch
    out, arg = be.rowbn_apply_max(xs[-1], K, mean_L, rstd_L, gam[-1], bet[-1], slopes[L], torch.bfloat16, nseg)
    return out, (*xs, *cis, *gam, *bet, *Ws, mean_L, rstd_L, out, *([arg] if arg is not None else []))


def _mlp_tail_bwd(saved, cfg, gout, need, want_dx, want_sums=False):
    """Backward body of the fused tail on what `_mlp_tail_fwd` saved; cfg = (nseg, K, slopes); need: which of gamma_0,
    beta_0, [W_l, gamma_l, beta_l]*L want a gradient; want_dx: so does x_0; want_sums: the launch that writes dx0 also
    writes qneg (P/K, C_0) f32 = -(its sum over each group of K rows) -> (dx0, qneg, the gradients in `need`'s order)."""
    (nseg, K, slopes), t = cfg, list(saved)
    n = len(slopes)
    L = n - 1
    xs, cis, gam, bet = t[:n], t[n:2 * n], t[2 * n:3 * n], t[3 * n:4 * n]
    Ws = t[4 * n:4 * n + L]
    mean_L, rstd_L, out = t[4 * n + L:4 * n + L + 3]
    arg = t[4 * n + L + 3] if K else None
    be = backend_for(xs[0])
    gout = gout.contiguous()
    if gout.dtype != torch.bfloat16:
        gout = gout.to(torch.bfloat16)
    need_aff = [need[0] or need[1]] + [need[3 * l + 3] or need[3 * l + 4] for l in range(L)]
    need_w = [need[3 * l + 2] for l in range(L)]
    grads_aff = [None] * n
    grads_w = [None] * L
    # the last BatchNorm (+ act, + max): its sums come from (gout, out) alone
    c12, dg, db, cb, ag = be.rowbn_bwd_sums(gout, xs[L], arg, out if K else None, K, mean_L, rstd_L, gam[L], bet[L],
                                            slopes[L], need_aff[L], nseg, want_cb=True)
    grads_aff[L] = (dg, db)
    # the arriving gradient lives on each group's arg-max row: a * lrelu'(y) * gout per (group, channel)
    # (normally a by-product of the reduction above)
    g_next, arg_next, K_next = (ag if ag is not None else be.mlp_max_prep(gout, out, cb, slopes[L], nseg)), arg, K
    for l in range(L, 0, -1):                    # layer l: x_{l-1} -> x_l
        if need_w[l - 1]:
            grads_w[l - 1] = be.mlp_wgrad(xs[l], g_next, arg_next, K_next, cb, xs[l - 1], cis[l - 1], slopes[l - 1],
                                          nseg)
        g_in, c12, cb, dg, db = be.mlp_dgrad(xs[l], g_next, arg_next, K_next, cb, xs[l - 1], cis[l - 1],
                                             slopes[l - 1], Ws[l - 1], nseg, need_aff[l - 1])
        grads_aff[l - 1] = (dg, db)
        g_next, arg_next, K_next = g_in, None, 0
    dx0 = qneg = None
    if want_dx and want_sums:
        dx0, qneg = be.mlp_bn_bwd_apply(g_next, xs[0], cis[0], c12, nseg, K)
    elif want_dx:
        dx0 = be.mlp_bn_bwd_apply(g_next, xs[0], cis[0], c12, nseg)
    grads = [grads_aff[0][0], grads_aff[0][1]]
    for l in range(L):
        gw = grads_w[l]
        if gw is not None and Ws[l].dim() == 2:
            gw = gw.sum(0) if gw.shape[0] > 1 else gw[0]
        elif gw is not None and Ws[l].shape[0] != gw.shape[0]:
            gw = gw.sum(0, keepdim=True)
        grads += [gw, grads_aff[l + 1][0], grads_aff[l + 1][1]]
    return dx0, qneg, grads


class _MlpTail(torch.autograd.Function):
    """[BN_0 + act] -> W_1 -> [BN_1 + act] -> ... -> W_L -> [BN_L + act (+ max over K)] on bf16 rows, every
    BatchNorm in training mode, `nseg` calls of the tail in one pass (csrc/mlp_fused.hip).

    forward : statistics of x_0 (one read), then per layer ONE fused launch (BatchNorm + LeakyReLU in the
              MFMA operand prologue, statistics of the product in the epilogue), then the final apply / max.
    backward: per layer a data-gradient launch (dx_{l+1} rebuilt in the prologue, BN_l's backward sums in
              the epilogue) and -- only where a weight needs its gradient -- a weight-gradient launch on
              the same saved rows; nothing but the bf16 pre-BatchNorm rows x_l was ever stored.
    tensors = gamma_0, beta_0, [W_l, gamma_l, beta_l]*L;  bns = the L+1 BatchNorm modules' state."""

    @staticmethod
    def forward(ctx, x0, cfg, *tensors):
        out, saved = _mlp_tail_fwd(x0, cfg, tensors)
        ctx.save_for_backward(*saved)
        ctx.cfg = cfg[:3]
        return out

    @staticmethod
    def backward(ctx, gout):
        need = ctx.needs_input_grad                  # (x0, cfg, gamma_0, beta_0, [W, gamma, beta]*L)
        dx0, _, grads = _mlp_tail_bwd(ctx.saved_tensors, ctx.cfg, gout, need[2:], need[0])
        return (dx0, None, *grads)


class _GatherMlpTail(torch.autograd.Function):
    """The ROW_SUB gather of (U, Q, idx) into bf16 rows and the fused tail (`_MlpTail`) on them as ONE node: the tail's
    last backward launch writes the rows' gradient dx0 group by group with each group's sum in registers, and those sums
    are the gather's gradient of Q (gQ[s] = -sum_k dx0[s,k]): dx0 is read once, by the plain gather's scatter."""

    @staticmethod
    def forward(ctx, U, Q, idx, inverse, cfg, *tensors):
        rows = backend_for(U).rowcombine_fwd(U, Q, idx, ROW_SUB, 0.0, torch.bfloat16)
        out, saved = _mlp_tail_fwd(rows.view(-1, rows.shape[3]), cfg, tensors)
        ctx.save_for_backward(idx, *saved)
        ctx.inverse = inverse          # (offs, lst) int32 tensors prepared ahead of time, or None
        ctx.cfg, ctx.N, ctx.in_dtype = cfg[:3], U.shape[1], U.dtype
        return out.view(idx.shape[0], idx.shape[1], -1)

    @staticmethod
    def backward(ctx, gout):
        idx, *saved = ctx.saved_tensors
        need = ctx.needs_input_grad                  # (U, Q, idx, inverse, cfg, gamma_0, beta_0, [W, gamma, beta]*L)
        want_dx = need[0] or need[1]
        sums = ctx.in_dtype == torch.float32         # (fp32 tables: the sums are gQ as they are; bf16: the SUB backward)
        dx0, qneg, grads = _mlp_tail_bwd(saved, ctx.cfg, gout.reshape(-1, gout.shape[-1]), need[5:], want_dx, sums)
        gU = gQ = None
        if want_dx:
            kw = {} if ctx.inverse is None else {"inverse": ctx.inverse}
            gU, gQ = backend_for(dx0).rowcombine_bwd(dx0.view(*idx.shape, -1), idx, None, ROW_GATHER if sums else ROW_SUB,
                                                     ctx.N, 0.0, ctx.in_dtype, **kw)
            if sums:
                gQ = qneg.view(idx.shape[0], idx.shape[1], -1)
        return (gU, gQ, None, None, None, *grads)


_IDENT = {}


def _ident_consts(C_, device):
    """(cb, ci) of an identity BatchNorm with zero backward sums: dx = gg, a = 1, xhat terms 0."""
    key = (C_, device)
    if key not in _IDENT:
        cb = torch.zeros((1, 4, C_), dtype=torch.float32, device=device)
        cb[0, 0] = 1.0                              # a | f*mu | e | f
        ci = torch.zeros((1, 4, C_), dtype=torch.float32, device=device)
        ci[0, 0] = 1.0                              # sc | sh | mu | rs
        ci[0, 3] = 1.0
        _IDENT[key] = (cb, ci)
    return _IDENT[key]


class _MlpTailPlain(torch.autograd.Function):
    """x_0 -> [act_0] -> W_1 -> act_1 -> ... -> W_L -> act_L -> max over K on bf16 rows, NO BatchNorm: the MLP of
    the generator's EdgeConv (gcn_lib/pointnet/gcn.py:207-211, norm == 'none') on the same fused MFMA kernels
    with identity statistics -- no statistics passes, no finalize launches, dx never stored."""

    @staticmethod
    def forward(ctx, x0, K, slopes, *Ws):
        be = backend_for(x0)
        L = len(Ws)
        xs = [x0]
        for l in range(L):
            y, _ = be.mlp_fwd(xs[-1], None, slopes[l], Ws[l], 1, stats=False)
            xs.append(y)
        out, arg = be.rowbn_fwd(xs[-1], K, 0.0, 0.0, False, None, None, None, None, slopes[L], None, None, torch.bfloat16)
        ctx.save_for_backward(*xs, *Ws, out, arg)
        ctx.cfg = (K, slopes, L)
        return out

    @staticmethod
    def backward(ctx, gout):
        K, slopes, L = ctx.cfg
        t = list(ctx.saved_tensors)
        xs, Ws, out, arg = t[:L + 1], t[L + 1:2 * L + 1], t[2 * L + 1], t[2 * L + 2]
        be = backend_for(xs[0])
        gout = gout.contiguous()
        if gout.dtype != torch.bfloat16:
            gout = gout.to(torch.bfloat16)
        need = ctx.needs_input_grad                  # (x0, K, slopes, W_1..W_L)
        grads_w = [None] * L
        cb = _ident_consts(out.shape[1], out.device)[0]
        g_next, arg_next, K_next = be.mlp_max_prep(gout, out, cb, slopes[L], 1), arg, K
        for l in range(L, 0, -1):
            cb = _ident_consts(xs[l].shape[1], out.device)[0]
            ci = _ident_consts(xs[l - 1].shape[1], out.device)[1]
            if need[3 + l - 1]:
                grads_w[l - 1] = be.mlp_wgrad(xs[l], g_next, arg_next, K_next, cb, xs[l - 1], ci, slopes[l - 1], 1)[0]
            if l > 1 or need[0]:
                g_next = be.mlp_dgrad(xs[l], g_next, arg_next, K_next, cb, xs[l - 1], ci, slopes[l - 1], Ws[l - 1], 1,
                                      False, sums=False)[0]
            arg_next, K_next = None, 0
        return (g_next if need[0] else None, None, None) + tuple(grads_w)


def mlp_tail_plain(x0, weights, slopes, K):
    """max_K act_L(W_L ... act_1(W_1 act_0(x0))) on bf16 rows x0 (P, C_0), no BatchNorm: (P/K, C_L) bf16.
    weights: L tensors (C_l, C_{l-1}) fp32; slopes: L+1 LeakyReLU slopes in [0, 1] (1.0 = no activation)."""
    L = len(weights)
    _need(len(slopes) == L + 1 and L >= 1, "mlp_tail_plain: L weights, L+1 slopes")
    _need(all(0.0 <= float(sl) <= 1.0 for sl in slopes), "mlp_tail_plain: LeakyReLU slopes in [0, 1]")
    _need(all(w.dtype == torch.float32 and w.dim() == 2 for w in weights), "mlp_tail_plain: 2-D fp32 weights")
    return _MlpTailPlain.apply(x0.contiguous(), int(K), tuple(float(s) for s in slopes), *[w.contiguous() for w in weights])


SMALL_TAIL_CHANNELS = (16, 16, 32)


class _SmallTail(torch.autograd.Function):
    """max_K lrelu(W2 lrelu(W1 h)) at the (16, 16, 32) channels of the IDGCN EdgeConvs, one launch each way
    (csrc/mlp_small.hip); only h, the output and the arg-max bytes are kept for the backward."""

    @staticmethod
    def forward(ctx, h, W1, W2, s1, s2, K):
        be = backend_for(h)
        w1, w2 = W1.detach().float().contiguous(), W2.detach().float().contiguous()
        out, arg = be.small_tail_fwd(h, w1, w2, s1, s2, K)
        ctx.save_for_backward(h, out, arg, w1, w2)
        ctx.cfg = (s1, s2, K, W1.dtype, W2.dtype)
        return out

    @staticmethod
    def backward(ctx, gout):
        h, out, arg, w1, w2 = ctx.saved_tensors
        s1, s2, K, t1, t2 = ctx.cfg
        be = backend_for(h)
        gh, dW1, dW2 = be.small_tail_bwd(h, out, gout.to(h.dtype).contiguous(), arg, w1, w2, s1, s2, K)
        return (gh if ctx.needs_input_grad[0] else None, dW1.to(t1) if ctx.needs_input_grad[1] else None,
                dW2.to(t2) if ctx.needs_input_grad[2] else None, None, None, None)


def small_tail_supported(h, channels, K):
    return (h.is_cuda and h.dtype in (torch.bfloat16, torch.float32) and tuple(channels) == SMALL_TAIL_CHANNELS
            and 0 < K <= 255)


def small_tail(h, W1, W2, slope1, slope2, K):
    """h (P*K, 16) rows (bf16 or fp32) of K consecutive edges per point -> (P, 32):
    max over the K edges of lrelu(W2 lrelu(W1 h)); W1 (16,16), W2 (32,16), no bias, slopes in [0, 1]."""
    _need(0.0 <= float(slope1) <= 1.0 and 0.0 <= float(slope2) <= 1.0, "small_tail: LeakyReLU slopes in [0, 1]")
    _need(h.dim() == 2 and h.shape[0] % int(K) == 0, "small_tail: (P*K, 16) rows")
    return _SmallTail.apply(h.contiguous(), W1, W2, float(slope1), float(slope2), int(K))


def mlp_tail_supported(x, channels, K, rows_dtype=None):
    """Can `mlp_tail` run this tail on the rows x (`gather_mlp_tail`: on rows of `rows_dtype` gathered from the table
    x)?  bf16 rows on the GPU, supported channel pairs, a max over K."""
    if not (x.is_cuda and (rows_dtype or x.dtype) == torch.bfloat16 and 0 < K <= 255 and len(channels) >= 2):
        return False
    return all((a, b) in MLP_CHANNELS for a, b in zip(channels[:-1], channels[1:]))


def _mlp_tail_args(bns, weights, slopes, K, nseg, shifts):
    """The validated (cfg, tensors) of `_mlp_tail_fwd` from what `mlp_tail` is given."""
    L = len(weights)
    _need(len(bns) == L + 1 and len(slopes) == L + 1 and L >= 1, "mlp_tail: L weights, L+1 BatchNorms / slopes")
    _need(all(0.0 <= float(sl) <= 1.0 for sl in slopes), "mlp_tail: LeakyReLU slopes in [0, 1] (lrelu = max(z, slope*z))")
    shifts = list(shifts) if shifts is not None else [None] * (L + 1)
    states, eps, moms = [], [], []
    for bn in bns:
        _need(bn.training and bn.momentum is not None, "mlp_tail needs training-mode BatchNorm with a fixed momentum")
        track = bn.track_running_stats and bn.running_mean is not None
        states.append((bn.running_mean if track else None, bn.running_var if track else None,
                       bn.num_batches_tracked if (track and bn.num_batches_tracked is not None) else None))
        eps.append(float(bn.eps))
        moms.append(float(bn.momentum))
    tensors = [bns[0].weight.float(), bns[0].bias.float()]
    for l in range(L):
        w = weights[l]
        _need(w.dtype == torch.float32, "mlp_tail weights are fp32 (rounded to bf16 inside the kernel)")
        tensors += [w.contiguous(), bns[l + 1].weight.float(), bns[l + 1].bias.float()]
    cfg = (int(nseg), int(K), tuple(float(s) for s in slopes), tuple(eps), tuple(moms), tuple(states),
           tuple(None if s is None else s.detach().float().contiguous() for s in shifts))
    return cfg, tensors


def mlp_tail(x0, bns, weights, slopes, K, nseg=1, shifts=None):
    """The tail of a shared MLP on bf16 rows x0 (P, C_0), fused on MFMA tiles (csrc/mlp_fused.hip):

        out = max_K lrelu(BN_L(W_L ... lrelu(BN_1(W_1 lrelu(BN_0(x0))))))          (P/K, C_L) bf16

    bns: the L+1 BatchNorm modules (training mode, fixed momentum; state updated like their own forward),
    weights: L tensors (C_l, C_{l-1}) or (nseg, C_l, C_{l-1}) fp32 (e.g. successive spectral-norm iterates),
    slopes: L+1 LeakyReLU slopes, nseg: calls of the tail on equal consecutive row blocks,
    shifts: per BatchNorm an optional bias of the preceding conv that was left out of its input."""
    cfg, tensors = _mlp_tail_args(bns, weights, slopes, K, nseg, shifts)
    return _MlpTail.apply(x0.contiguous(), cfg, *tensors)


def gather_mlp_tail(U, Q, idx, bns, weights, slopes, nseg=1, shifts=None):
    """The training-mode counterpart of `gather_mlp_max`: `mlp_tail` (K = idx's last axis) on the bf16 rows
    U[b,idx[b,s,j],:] - Q[b,s,:] of `row_combine` (ROW_SUB) as ONE autograd node -> (B,S,C_L) bf16.
    U (B,N,C_0) fp32 or bf16, Q (B,S,C_0), idx (B,S,K) int32 or a NeighbourList into N rows (its prepared inverse goes
    to the backward); the rest as `mlp_tail` takes it.  The launches and bits of the two ops one after the other, except
    that with fp32 tables the backward's last tail launch is tpg_mlp_bn_bwd_apply_rowsum (see _GatherMlpTail)."""
    _need(U.dim() == 3 and U.dtype in _DTYPE_CODE, "U (B,N,C) fp32/bf16, idx (B,S,K) int32")
    nl = neighbour_list(idx, U.shape[1])
    idx = nl.idx
    _need(U.shape[0] == idx.shape[0], "batch mismatch")
    _need(Q is not None and Q.shape == (U.shape[0], idx.shape[1], U.shape[2]), "Q must be (B,S,C)")
    _need(U.shape[2] % 8 == 0, f"channel count {U.shape[2]} must be a multiple of 8")
    cfg, tensors = _mlp_tail_args(bns, weights, slopes, idx.shape[2], nseg, shifts)
    return _GatherMlpTail.apply(U.contiguous(), Q.to(U.dtype).contiguous(), idx, nl.inverse, cfg, *tensors)


# ------------------------------------------- eval-mode tail in one launch (csrc/mlp_infer.hip)
def gather_mlp_max_supported(U, channels, K, rows_dtype=None):
    """Can `gather_mlp_max` run this tail?  Tables on the GPU, bf16 rows, one of the channel chains (C_0, .., C_L) and a K
    the library is built for (tpg_mlp_infer_supported: the one list).  rows_dtype: the dtype the per-layer path would
    store the grouped rows in (default: U's own); fp32 rows stay on that path -- the kernel's operands are bf16.
    Everything it refuses stays on the per-layer path (row_combine, rows_matmul, row_bn_act)."""
    if not (torch.is_tensor(U) and U.is_cuda and U.dtype in _DTYPE_CODE and (rows_dtype or U.dtype) == torch.bfloat16):
        return False
    chans = [int(c) for c in channels]
    if len(chans) not in (2, 3):
        return False
    return bool(_lib.load().tpg_mlp_infer_supported(chans[0], chans[1], chans[2] if len(chans) == 3 else 0, int(K)))


def pack_infer_weight(W):
    """(Cout,Cin) weight -> bf16 in the MFMA B-fragment order of csrc/mlp_infer.hip (include/tpgan_ops.h):
    packed[t, s, lq, li, e] = W[li*T + t, 32*s + 8*lq + e], T = Cout/16."""
    Cout, Cin = W.shape
    _need(Cout % 16 == 0 and Cin % 32 == 0, "pack_infer_weight: Cout % 16 == 0 and Cin % 32 == 0")
    w = W.detach().to(torch.bfloat16).view(16, Cout // 16, Cin // 32, 4, 8)          # li, t, s, lq, e
    return w.permute(1, 2, 3, 0, 4).contiguous()


def gather_mlp_max(U, Q, idx, weights, scales, shifts, slopes, out_dtype=torch.bfloat16):
    """The eval-mode tail behind a row gather, in one forward-only launch:

        out[b,s,:] = max_{j<K} act_L(a_L * (W_L ... act_1(a_1 * (W_1 act_0(U[b,idx[b,s,j],:] - Q[b,s,:])) + c_1) ...) + c_L)
        act_l(z) = max(z, slope_l * z)

    U (B,N,C_0), Q (B,S,C_0) both fp32 or both bf16 (the difference is taken in fp32 on their own values: fp32 tables
    are not rounded before it); idx (B,S,K) int32 or a NeighbourList into N rows; weights: L = 1 or 2 tensors
    (C_l, C_{l-1}) (rounded to bf16); scales / shifts: L per-channel vectors a_l / c_l (fp32); slopes: L+1 floats in
    [0,1] (slope_0 first) -> (B,S,C_L) bf16.  Not differentiable: raises when grad is enabled and an input requires it."""
    L = len(weights)
    _need(L in (1, 2) and len(scales) == L and len(shifts) == L and len(slopes) == L + 1,
          "gather_mlp_max: 1 or 2 weights, as many scales / shifts, one slope more")
    _need(out_dtype == torch.bfloat16, "gather_mlp_max writes bf16 rows")
    _need(all(0.0 <= float(sl) <= 1.0 for sl in slopes), "gather_mlp_max: LeakyReLU slopes in [0, 1]")
    _need(torch.is_tensor(U) and U.dim() == 3 and torch.is_tensor(Q) and Q.dim() == 3, "U (B,N,C), Q (B,S,C)")
    idx = neighbour_list(idx, U.shape[1]).idx
    B, N, C0 = U.shape
    _need(Q.shape[0] == B and Q.shape[2] == C0 and idx.shape[:2] == Q.shape[:2], "Q must be (B,S,C), idx (B,S,K)")
    _need(U.dtype in _DTYPE_CODE and Q.dtype == U.dtype, "gather_mlp_max: U and Q are both fp32 or both bf16")
    chans = [C0]
    for W, a, c in zip(weights, scales, shifts):
        _need(W.dim() == 2 and W.shape[1] == chans[-1], f"weight {tuple(W.shape)} does not follow {chans[-1]} channels")
        _need(a.shape == (W.shape[0],) and c.shape == (W.shape[0],), "one scale and one shift per output channel")
        chans.append(int(W.shape[0]))
    _need(gather_mlp_max_supported(U, chans, idx.shape[2], out_dtype),
          f"gather_mlp_max: chain {tuple(chans)} with K = {idx.shape[2]} is not built (see gather_mlp_max_supported)")
    tensors = [U, Q, idx] + list(weights) + list(scales) + list(shifts)
    _same_device(*tensors)
    _need(not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors)),
          "gather_mlp_max is forward-only: run it under no_grad or take the per-layer path")
    packed = [pack_infer_weight(W) for W in weights]
    return backend_for(U).mlp_infer(U.contiguous(), Q.contiguous(), idx.contiguous(), packed,
                                    [a.detach().float().contiguous() for a in scales],
                                    [c.detach().float().contiguous() for c in shifts], [float(sl) for sl in slopes])


# ---------------------------------------------------------------------- row-wise linear layers
class _RowLinear(torch.autograd.Function):
    """y = lrelu_slope(x @ W[seg]^T + bias) on rows (csrc/rowlinear.hip); backward from the saved OUTPUT (the sign
    of y is the sign of the pre-activation), one launch for dx, two (slabs + ordered reduce) for dW / db."""

    @staticmethod
    def forward(ctx, x, W, bias, nseg, slope, out_dtype):
        be = backend_for(x)
        Wf = W if W.dtype == torch.float32 else W.float()
        Wf = Wf.contiguous()
        bf = None if bias is None else bias.float().contiguous()
        y = be.rowlinear_fwd(x, Wf, bf, nseg, slope, out_dtype)
        ctx.save_for_backward(x, Wf, y if slope != 1.0 else None)
        ctx.cfg = (int(nseg), float(slope), W.dtype, W.shape, None if bias is None else bias.dtype)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, Wf, y = ctx.saved_tensors
        nseg, slope, w_dtype, w_shape, b_dtype = ctx.cfg
        be = backend_for(x)
        gy = gy.contiguous()
        if gy.dtype not in _DTYPE_CODE:
            gy = gy.float()
        if y is not None and y.dtype != gy.dtype:
            gy = gy.to(y.dtype)
        dx = dW = db = None
        if ctx.needs_input_grad[0]:
            dx = be.rowlinear_dgrad(gy, y, Wf, nseg, slope, x.dtype)
        if ctx.needs_input_grad[1] or (b_dtype is not None and ctx.needs_input_grad[2]):
            dW, db = be.rowlinear_wgrad(x, gy, y, nseg, slope, b_dtype is not None and ctx.needs_input_grad[2])
            dW = dW.view(w_shape).to(w_dtype) if ctx.needs_input_grad[1] else None
            if db is not None:
                db = db.to(b_dtype)
        return dx, dW, db, None, None, None


# Off by default (round 3 measurement, tools/tune_rowlinear.py -> profiles/r03_tune_rowlinear.txt, hipGraph replay,
# MI355X): the hand-written kernels are correct on every shape of the step (tests/test_mlp_gpu.py) and win the FORWARD at
# the small channel counts (12288 x 3 -> 64: 6.0 against 7.6 us; 196608 x 6 -> 64 in six segments: 22 against 38 us) but lose
# forward + backward everywhere (12288 x 128 -> 128 bf16: 95 against 39 us; 8192 x 515 -> 256 in four segments: 847 against
# 132 us): the f32 matrix rate bounds the wide layers (the pre-gather layers must stay fp32), the weight is staged per 128
# rows and once per 16-column pass when K is large, and the weight gradient walks its slabs on too few CUs.  The ~5 us
# saved per fused bias / activation / cast / partial-sum launch do not pay for that: the library route stays.
ROW_LINEAR = [False]


def row_linear_supported(x, W, nseg=1):
    """Can `row_linear` take this product?  fp32 / bf16 rows on the GPU, fp32 / bf16 weights, equal 64-row-aligned
    segments."""
    if not (ROW_LINEAR[0] and x.is_cuda and x.dtype in _DTYPE_CODE and W.dtype in (torch.float32, torch.bfloat16)):
        return False
    P = x.numel() // x.shape[-1] if x.numel() else 0
    if P == 0 or not _lib.load().tpg_rowlinear_supported(int(x.shape[-1]), int(W.shape[-2]), 1):
        return False
    return nseg == 1 or (P % nseg == 0 and (P // nseg) % 128 == 0)


def row_linear(x, W, bias=None, slope=1.0, nseg=1, out_dtype=None):
    """x (..., Cin) rows (fp32 / bf16) -> lrelu_slope(x @ W^T + bias) (..., Cout) of `out_dtype` (default x.dtype).
    W (Cout, Cin), or (nseg, Cout, Cin) with the leading rows in nseg equal blocks, block s using W[s].
    slope 1.0 = no activation.  Reference: the 1x1 convolutions of gcn_lib/pointnet/gcn.py:96-147 and
    discriminator.py:63-78 that are not inside a fused tail."""
    _need(x.dtype in _DTYPE_CODE, f"row_linear supports fp32/bf16 rows, got {x.dtype}")
    _need(0.0 <= float(slope) <= 1.0, "row_linear: LeakyReLU slope in [0, 1]")
    lead = x.shape[:-1]
    x2 = x.reshape(-1, x.shape[-1]).contiguous()
    if x2.data_ptr() % 16:
        x2 = x2.clone()                                    # (a row slice at an odd offset: the kernels take 16-byte rows)
    _need((W.dim() == 2 and nseg == 1) or (W.dim() == 3 and W.shape[0] == nseg), "W (Cout,Cin) or (nseg,Cout,Cin)")
    _need(W.shape[-1] == x2.shape[1], "row_linear: channel mismatch")
    y = _RowLinear.apply(x2, W, bias, int(nseg), float(slope), out_dtype or x.dtype)
    return y.view(*lead, W.shape[-2])


# ---------------------------------------------------------------------- fused spectral norm
class _SpectralNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, W, u, v, iterate, eps):
        Wsn, sigma = backend_for(W).spectral_norm_fwd(W, u, v, iterate, eps)
        # u, v as they are AFTER the power iteration (the constants of the backward)
        ctx.save_for_backward(Wsn, u.clone(), v.clone(), sigma)
        return Wsn

    @staticmethod
    def backward(ctx, G):
        Wsn, u, v, sigma = ctx.saved_tensors
        return backend_for(Wsn).spectral_norm_bwd(G.float().contiguous(), Wsn, u, v, sigma), None, None, None, None


def spectral_normalize(weight_orig, u, v, training, eps=1e-12):
    """W / sigma with one in-place power iteration of (u, v) in training mode -- the result of
    torch.nn.utils.spectral_norm's forward pre-hook, in one kernel (include/tpgan_ops.h).
    weight_orig (R, ...) fp32; returns a tensor of the same shape."""
    _need(weight_orig.dtype == torch.float32 and u.dtype == torch.float32 and v.dtype == torch.float32,
          "spectral_normalize works on fp32 parameters")
    W2 = weight_orig.reshape(weight_orig.shape[0], -1).contiguous()
    _need(u.numel() == W2.shape[0] and v.numel() == W2.shape[1] and u.is_contiguous() and v.is_contiguous(),
          "u / v do not match the weight")
    return _SpectralNorm.apply(W2, u, v, bool(training), float(eps)).view_as(weight_orig)


class _SpectralNormMulti(torch.autograd.Function):
    """All spectrally-normalised weights of one forward pass, each used `uses[m]` times."""

    @staticmethod
    def forward(ctx, training, eps, uses, *tensors):
        n = len(uses)
        Ws, us, vs = tensors[:n], tensors[n:2 * n], tensors[2 * n:]
        flat, plan = backend_for(Ws[0]).spectral_norm_multi_fwd(list(Ws), list(us), list(vs), list(uses),
                                                                training, eps)
        outs = []
        for W, (off, st), k in zip(Ws, plan["layout"], uses):
            R, Cn = W.shape
            for t in range(k):
                outs.append(flat[off + t * st: off + t * st + R * Cn].view(R, Cn))
        ctx.flat, ctx.plan, ctx.uses = flat, plan, tuple(uses)
        ctx.shapes = [tuple(W.shape) for W in Ws]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        parts, i = [], 0
        for (R, Cn), k in zip(ctx.shapes, ctx.uses):
            for _ in range(k):
                g = grads[i]
                i += 1
                parts.append(torch.zeros(R * Cn, dtype=torch.float32, device=ctx.flat.device) if g is None
                             else g.reshape(-1).float())
        gflat = torch.cat(parts)
        dw = backend_for(ctx.flat).spectral_norm_multi_bwd(ctx.flat, ctx.plan, gflat)
        dWs = [dw[off:off + R * Cn].view(R, Cn) for (R, Cn), off in zip(ctx.shapes, ctx.plan["dwoffs"])]
        n = len(ctx.uses)
        return (None, None, None) + tuple(dWs) + (None,) * (2 * n)


def spectral_normalize_many(modules, uses, training, eps=1e-12):
    """For every spectrally-normalised module m (attributes weight_orig / weight_u / weight_v) the
    `uses[m]` successive weights W / sigma its forward pre-hook would produce over that many calls
    (one power iteration per call in training mode) -- all modules in ONE launch.
    Returns a list (per module) of lists (per use) of 2-D weights (R, prod(rest))."""
    Ws = [m.weight_orig.reshape(m.weight_orig.shape[0], -1) for m in modules]
    for W in Ws:
        _need(W.dtype == torch.float32 and W.is_contiguous(), "spectral norm works on contiguous fp32 weights")
    us = [m.weight_u for m in modules]
    vs = [m.weight_v for m in modules]
    outs = _SpectralNormMulti.apply(bool(training), float(eps), tuple(int(k) for k in uses), *Ws, *us, *vs)
    res, i = [], 0
    for k in uses:
        res.append(list(outs[i:i + k]))
        i += k
    return res

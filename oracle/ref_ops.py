"""numpy front-end of libtpgref.so (the CPU restatement).  TEST INFRASTRUCTURE ONLY.

Every function takes/returns numpy arrays with the layouts of include/tpgan_ops.h.
"""
import ctypes as C

import numpy as np
import torch

from . import build

_lib = None

_F = C.POINTER(C.c_float)
_I32 = C.POINTER(C.c_int32)
_I64 = C.POINTER(C.c_int64)


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(build())
    return _lib


def _f(a):
    return a.ctypes.data_as(_F)


def _i32(a):
    return a.ctypes.data_as(_I32)


def _i64(a):
    return None if a is None else a.ctypes.data_as(_I64)


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _chk(rc, name):
    if rc != 0:
        raise RuntimeError(f"oracle {name} failed with status {rc}")


def radius_sq(r):
    """r (python float) -> fp32 r*r exactly as the product's host code does."""
    r32 = np.float32(r)
    return float(np.float32(r32 * r32))


def knn(p1, p2, K, lengths1=None, lengths2=None, r=None):
    p1, p2 = _c(p1, np.float32), _c(p2, np.float32)
    B, P1, D = p1.shape
    P2 = p2.shape[1]
    l1 = None if lengths1 is None else _c(lengths1, np.int64)
    l2 = None if lengths2 is None else _c(lengths2, np.int64)
    dist = np.empty((B, P1, K), np.float32)
    idx = np.empty((B, P1, K), np.int64)
    r2 = -1.0 if r is None else radius_sq(r)
    _chk(lib().tpgref_knn_f32(_f(p1), _f(p2), _i64(l1), _i64(l2), B, P1, P2, D, K,
                              C.c_float(r2), _f(dist), _i64(idx)), "knn")
    return dist, idx


def cubic_interp(query, pos, field, cutoff):
    """-> (out_plain (B,Nq,F), out_pad (B,Nq,F), hits (B,Nq) i32); include/tpgan_ops.h."""
    query, pos, field = _c(query, np.float32), _c(pos, np.float32), _c(field, np.float32)
    B, Nq, _ = query.shape
    Np, F = pos.shape[1], field.shape[2]
    plain, pad = np.empty((B, Nq, F), np.float32), np.empty((B, Nq, F), np.float32)
    hits = np.empty((B, Nq), np.int32)
    _chk(lib().tpgref_cubic_interp_f32(_f(query), _f(pos), _f(field), B, Nq, Np, F, C.c_float(cutoff),
                                       _f(plain), _f(pad), _i32(hits)), "cubic_interp")
    return plain, pad, hits


def chamfer_fwd(src, tgt):
    src, tgt = _c(src, np.float32), _c(tgt, np.float32)
    B, N, _ = src.shape
    M = tgt.shape[1]
    d1, i1 = np.empty((B, N), np.float32), np.empty((B, N), np.int64)
    d2, i2 = np.empty((B, M), np.float32), np.empty((B, M), np.int64)
    _chk(lib().tpgref_chamfer_fwd_f32(_f(src), _f(tgt), B, N, M, _f(d1), _i64(i1),
                                      _f(d2), _i64(i2)), "chamfer_fwd")
    return d1, i1, d2, i2


def chamfer_bwd(src, tgt, i1, i2, g1, g2):
    src, tgt = _c(src, np.float32), _c(tgt, np.float32)
    i1, i2 = _c(i1, np.int64), _c(i2, np.int64)
    g1, g2 = _c(g1, np.float32), _c(g2, np.float32)
    B, N, _ = src.shape
    M = tgt.shape[1]
    gs, gt = np.empty_like(src), np.empty_like(tgt)
    _chk(lib().tpgref_chamfer_bwd_f32(_f(src), _f(tgt), B, N, M, _i64(i1), _i64(i2),
                                      _f(g1), _f(g2), _f(gs), _f(gt)), "chamfer_bwd")
    return gs, gt


def fps(xyz, m):
    xyz = _c(xyz, np.float32)
    B, N, _ = xyz.shape
    temp = np.empty((B, N), np.float32)
    idx = np.empty((B, m), np.int32)
    _chk(lib().tpgref_fps_f32(_f(xyz), B, N, m, _f(temp), _i32(idx)), "fps")
    return idx


def fps_start(xyz, m, start=None, skip_origin=False):
    xyz = _c(xyz, np.float32)
    B, N, _ = xyz.shape
    temp = np.empty((B, N), np.float32)
    idx = np.empty((B, m), np.int32)
    st = None if start is None else _c(start, np.int32)
    _chk(lib().tpgref_fps_start_f32(_f(xyz), None if st is None else _i32(st), int(bool(skip_origin)), B, N, m,
                                    _f(temp), _i32(idx)), "fps_start")
    return idx


def gather_fwd(feat, idx):
    feat, idx = _c(feat, np.float32), _c(idx, np.int32)
    B, Cc, N = feat.shape
    S = idx.shape[1]
    out = np.empty((B, Cc, S), np.float32)
    _chk(lib().tpgref_gather_fwd_f32(_f(feat), _i32(idx), B, Cc, N, S, _f(out)), "gather_fwd")
    return out


def gather_bwd(gout, idx, N):
    gout, idx = _c(gout, np.float32), _c(idx, np.int32)
    B, Cc, S = gout.shape
    g = np.empty((B, Cc, N), np.float32)
    _chk(lib().tpgref_gather_bwd_f32(_f(gout), _i32(idx), B, Cc, N, S, _f(g)), "gather_bwd")
    return g


def gather_rows_fwd(rows, idx):
    """tpg_gather_rows_fwd_f32 = gather_fwd on the transposed tensors."""
    return np.ascontiguousarray(gather_fwd(np.ascontiguousarray(np.transpose(rows, (0, 2, 1))), idx).transpose(0, 2, 1))


def gather_rows_bwd(gout, idx, N):
    return np.ascontiguousarray(gather_bwd(np.ascontiguousarray(np.transpose(gout, (0, 2, 1))), idx, N).transpose(0, 2, 1))


def ball_query(radius, nsample, xyz, new_xyz):
    xyz, new_xyz = _c(xyz, np.float32), _c(new_xyz, np.float32)
    B, N, _ = xyz.shape
    S = new_xyz.shape[1]
    idx = np.empty((B, S, nsample), np.int32)
    _chk(lib().tpgref_ball_query_f32(_f(xyz), _f(new_xyz), B, N, S, C.c_float(radius),
                                     nsample, _i32(idx)), "ball_query")
    return idx


def group_fwd(feat, idx):
    feat, idx = _c(feat, np.float32), _c(idx, np.int32)
    B, Cc, N = feat.shape
    _, S, K = idx.shape
    out = np.empty((B, Cc, S, K), np.float32)
    _chk(lib().tpgref_group_fwd_f32(_f(feat), _i32(idx), B, Cc, N, S, K, _f(out)), "group_fwd")
    return out


def group_bwd(gout, idx, N):
    gout, idx = _c(gout, np.float32), _c(idx, np.int32)
    B, Cc, S, K = gout.shape
    g = np.empty((B, Cc, N), np.float32)
    _chk(lib().tpgref_group_bwd_f32(_f(gout), _i32(idx), B, Cc, N, S, K, _f(g)), "group_bwd")
    return g


def three_nn(unknown, known):
    unknown, known = _c(unknown, np.float32), _c(known, np.float32)
    B, n, _ = unknown.shape
    m = known.shape[1]
    d2 = np.empty((B, n, 3), np.float32)
    idx = np.empty((B, n, 3), np.int32)
    _chk(lib().tpgref_three_nn_f32(_f(unknown), _f(known), B, n, m, _f(d2), _i32(idx)), "three_nn")
    return d2, idx


def three_interp_fwd(feat, idx, w):
    feat, idx, w = _c(feat, np.float32), _c(idx, np.int32), _c(w, np.float32)
    B, Cc, m = feat.shape
    n = idx.shape[1]
    out = np.empty((B, Cc, n), np.float32)
    _chk(lib().tpgref_three_interp_fwd_f32(_f(feat), _i32(idx), _f(w), B, Cc, m, n, _f(out)),
         "three_interp_fwd")
    return out


def three_interp_bwd(gout, idx, w, m):
    gout, idx, w = _c(gout, np.float32), _c(idx, np.int32), _c(w, np.float32)
    B, Cc, n = gout.shape
    g = np.empty((B, Cc, m), np.float32)
    _chk(lib().tpgref_three_interp_bwd_f32(_f(gout), _i32(idx), _f(w), B, Cc, m, n, _f(g)),
         "three_interp_bwd")
    return g


def rowcombine_fwd(U, QE, idx, mode, slope=0.2):
    U, idx = _c(U, np.float32), _c(idx, np.int32)
    QE = None if QE is None else _c(QE, np.float32)
    B, N, Cc = U.shape
    _, S, K = idx.shape
    out = np.empty((B, S, K, Cc), np.float32)
    _chk(lib().tpgref_rowcombine_fwd_f32(_f(U), None if QE is None else _f(QE), _i32(idx), mode, B, N, S,
                                         K, Cc, C.c_float(slope), _f(out)), "rowcombine_fwd")
    return out


def rowcombine_bwd(gout, idx, E, mode, N, slope=0.2):
    gout, idx = _c(gout, np.float32), _c(idx, np.int32)
    E = None if E is None else _c(E, np.float32)
    B, S, K, Cc = gout.shape
    gU = np.empty((B, N, Cc), np.float32)
    gQE = np.empty((B, S, Cc), np.float32) if mode != 0 else None
    _chk(lib().tpgref_rowcombine_bwd_f32(_f(gout), _i32(idx), None if E is None else _f(E), mode, B, N, S, K,
                                         Cc, C.c_float(slope), _f(gU), None if gQE is None else _f(gQE)),
         "rowcombine_bwd")
    return gU, gQE


def rowcombine_edge_fwd(Y, idx, slope_a=0.2, slope_e=0.2):
    """The EdgeConv front end on one product (include/tpgan_ops.h, tpg_rowcombine_edge_fwd; reference
    gcn_lib/pointnet/gcn.py:176-180,207-210): Y (B,N,2C) = f [We; Wn]^T; restated over rowcombine_fwd(mode EDGE)."""
    Y = _c(Y, np.float32)
    Cc = Y.shape[2] // 2
    A = Y[:, :, Cc:]
    A = np.where(A > 0, A, A * np.float32(slope_a)).astype(np.float32)
    return rowcombine_fwd(A, Y[:, :, :Cc], idx, 2, slope_e)


def rowcombine_edge_bwd(gout, idx, Y, slope_a=0.2, slope_e=0.2):
    Y = _c(Y, np.float32)
    Cc = Y.shape[2] // 2
    gU, gE = rowcombine_bwd(gout, idx, Y[:, :, :Cc], 2, Y.shape[1], slope_e)
    gA = np.where(Y[:, :, Cc:] > 0, gU, gU * np.float32(slope_a)).astype(np.float32)
    return np.concatenate([gE, gA], axis=2)


# ---- a head's BatchNorm1d + LeakyReLU + dropout mask (include/tpgan_ops.h, tpg_head_bn_act_*): numpy restatement
# (float64 inside) of nn.BatchNorm1d in training mode -> nn.LeakyReLU -> x * mask, reference discriminator.py:503-516.
def head_bn_act_fwd(h, gamma, beta, running_mean, running_var, momentum, eps, slope, mask):
    h64 = np.asarray(h, np.float64)
    B = h64.shape[0]
    mean = h64.mean(0)
    var = h64.var(0)
    rstd = 1.0 / np.sqrt(var + eps)
    z = (h64 - mean) * rstd * (1.0 if gamma is None else np.asarray(gamma, np.float64)) + \
        (0.0 if beta is None else np.asarray(beta, np.float64))
    y = np.where(z > 0, z, z * slope)
    if mask is not None:
        y = y * np.asarray(mask, np.float64)
    new_rm = None if running_mean is None else (1 - momentum) * np.asarray(running_mean, np.float64) + momentum * mean
    new_rv = None if running_var is None else \
        (1 - momentum) * np.asarray(running_var, np.float64) + momentum * var * B / (B - 1)
    f = lambda a: None if a is None else a.astype(np.float32)
    return f(y), f(mean), f(rstd), f(new_rm), f(new_rv)


def head_bn_act_bwd(gy, h, mean, rstd, gamma, beta, slope, mask):
    h64, g64 = np.asarray(h, np.float64), np.asarray(gy, np.float64)
    B = h64.shape[0]
    ga = 1.0 if gamma is None else np.asarray(gamma, np.float64)
    be = 0.0 if beta is None else np.asarray(beta, np.float64)
    xh = (h64 - np.asarray(mean, np.float64)) * np.asarray(rstd, np.float64)
    gz = g64 if mask is None else g64 * np.asarray(mask, np.float64)
    gz = np.where(xh * ga + be > 0, gz, gz * slope)
    db, dg = gz.sum(0), (gz * xh).sum(0)
    dh = ga * np.asarray(rstd, np.float64) * (gz - db / B - xh * dg / B)
    return dh.astype(np.float32), dg.astype(np.float32), db.astype(np.float32)


# ---- fused BatchNorm + LeakyReLU (+ max over K) on rows: numpy restatement (float64 inside) of the
# build's own fused form of [BatchNorm2d -> (Leaky)ReLU -> max over nsample]
# (reference discriminator.py:63-78,145-150,279-282); equality with the reference is pinned at
# model level by tests/golden.
def _bn_preact32(x, mean, rstd, gamma, beta):
    """z = (x - mean) * (gamma * rstd) + beta in fp32, op for op as csrc/rowbn.hip::bn_z, so the
    sign of z (the LeakyReLU mask) is the one the kernel sees."""
    x32 = np.asarray(x, np.float32)
    Cc = x32.shape[1]
    g = np.ones(Cc, np.float32) if gamma is None else np.asarray(gamma, np.float32)
    b = np.zeros(Cc, np.float32) if beta is None else np.asarray(beta, np.float32)
    a = g * np.asarray(rstd, np.float32)
    return (x32 - np.asarray(mean, np.float32)) * a + b


def rowbn_fwd(x, K, eps, gamma, beta, slope, training=True, mean=None, rstd=None):
    x64 = np.asarray(x, np.float64)
    P, Cc = x64.shape
    if training:
        mean = x64.mean(0)
        rstd = 1.0 / np.sqrt(x64.var(0) + eps)
    mean, rstd = np.asarray(mean, np.float32), np.asarray(rstd, np.float32)
    z = _bn_preact32(x, mean, rstd, gamma, beta)
    y = np.where(z > 0, z, z * np.float32(slope))
    arg = None
    if K:
        yk = y.reshape(P // K, K, Cc)
        arg = yk.argmax(1).astype(np.uint8)          # first maximum
        y = yk.max(1)
    return y.astype(np.float32), mean, rstd, arg


def rowbn_bwd(gy, x, arg, K, training, mean, rstd, gamma, beta, slope):
    x64 = np.asarray(x, np.float64)
    P, Cc = x64.shape
    g_ = np.ones(Cc) if gamma is None else np.asarray(gamma, np.float64)
    z = _bn_preact32(x, mean, rstd, gamma, beta)
    mean, rstd = np.asarray(mean, np.float64), np.asarray(rstd, np.float64)
    xhat = (x64 - mean) * rstd
    gy64 = np.asarray(gy, np.float64)
    if K:
        full = np.zeros((P // K, K, Cc))
        gi, ci = np.meshgrid(np.arange(P // K), np.arange(Cc), indexing="ij")
        full[gi, arg.astype(np.int64), ci] = gy64
        gy64 = full.reshape(P, Cc)
    g = gy64 * np.where(z > 0, 1.0, slope)
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    if training:
        dx = g_ * rstd * (g - dbeta / P - xhat * dgamma / P)
    else:
        dx = g_ * rstd * g
    return dx.astype(np.float32), dgamma.astype(np.float32), dbeta.astype(np.float32)


# ---- spectral norm (torch.nn.utils.spectral_norm's forward pre-hook, n_power_iterations = 1) ----
def spectral_norm_fwd(W, u, v, iterate, eps=1e-12):
    W64, u64, v64 = np.asarray(W, np.float64), np.asarray(u, np.float64), np.asarray(v, np.float64)
    if iterate:
        t = W64.T @ u64
        v64 = t / max(np.linalg.norm(t), eps)
        s = W64 @ v64
        u64 = s / max(np.linalg.norm(s), eps)
    sigma = u64 @ (W64 @ v64)
    return (W64 / sigma).astype(np.float32), u64.astype(np.float32), v64.astype(np.float32), np.float32(sigma)


def spectral_norm_bwd(G, Wsn, u, v, sigma):
    G64, W64 = np.asarray(G, np.float64), np.asarray(Wsn, np.float64)
    d = (G64 * W64).sum()
    return ((G64 - d * np.outer(u, v)) / float(sigma)).astype(np.float32)


# ---- the fused MLP tail's backward (csrc/mlp_fused.hip): per-launch restatements ------------------------------------
# Unlike the numpy functions above, these take and return torch tensors: float64 carriers on any device (the GPU tests
# run the 65535-row contractions on the GPU in float64).  The build uses -ffp-contract=off, so the kernels' only fused
# operations are the explicit __builtin_fmaf calls and every other fp32 operation rounds once: `Arith(True)` restates
# that arithmetic exactly, `Arith(False)` is the same formula with every rounding switched off (the algebra alone, for
# the comparison with torch.autograd).
U32 = 2.0 ** -24          # unit roundoff of fp32
BF16_REL = 2.0 ** -8      # one round-to-nearest-even to bf16 moves a value by at most 2^-8 of itself


def _f64(t, like=None):
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(np.asarray(t))
    return t.to(device=like.device if like is not None else t.device, dtype=torch.float64)


def r32(v):
    """Round float64 values to fp32 (round to nearest even), kept in float64."""
    return v.to(torch.float32).to(torch.float64)


def rbf16(v):
    """pack_bf16x2 (csrc/mlp_fused.hip:45): round-to-nearest-even of fp32 values to bf16, kept in float64."""
    return v.to(torch.float32).to(torch.bfloat16).to(torch.float64)


def fma32(a, b, c):
    """__builtin_fmaf on fp32 values held in float64, exact: p = a*b is exact in fp64 (24 + 24 significand bits);
    s = p + c rounds once in fp64 and t is its TwoSum error.  Rounding s to fp32 is then right unless s lies exactly
    halfway between two fp32 values while t != 0: s is then moved one fp64 ulp towards t first."""
    p = a * b
    s = p + c
    bb = s - p
    t = (p - (s - bb)) + (c - bb)
    half = (s.contiguous().view(torch.int64) & ((1 << 29) - 1)) == (1 << 28)      # fp32 normal range: 29 extra bits
    inf = torch.full_like(s, float("inf"))
    s = torch.where(half & (t != 0), torch.nextafter(s, torch.where(t > 0, inf, -inf)), s)
    return r32(s)


class Arith:
    """The kernels' fp32 operations on float64 carriers (emulate=True), or exact float64 (emulate=False)."""

    def __init__(self, emulate):
        self.emulate = emulate

    def r(self, v):
        return r32(v) if self.emulate else v

    def mul(self, a, b):
        return self.r(a * b)

    def sub(self, a, b):
        return self.r(a - b)

    def add(self, a, b):
        return self.r(a + b)

    def fma(self, a, b, c):
        return fma32(a, b, c) if self.emulate else a * b + c

    def bf16(self, v):
        return rbf16(v) if self.emulate else v


FP32, FP64 = Arith(True), Arith(False)


def _rows(c, P):
    """(nseg, C) per-segment constants -> one row per row of the (nseg*P, C) tensor."""
    return c.repeat_interleave(P, 0)


def _cb(a, mu, rs, c12, ar):
    c1, c2 = c12[:, 0], c12[:, 1]
    f = ar.mul(ar.mul(a, rs), c2)                                  # a * rs * c2, left to right
    return torch.stack([a, ar.mul(f, mu), ar.mul(-a, c1), f], 1)   # a | f*mu | e = -a*c1 | f


def mlp_consts(mean, rstd, gamma, beta, c12, ar=FP32):
    """tpg_mlp_consts, op for op as csrc/mlp_fused.hip:797-817 (mlp_consts_kernel): mean, rstd (nseg,C), gamma, beta
    (C) or None, c12 (nseg,2,C) or None -> ci (nseg,4,C) = sc | sh | mu | rs, cb (nseg,4,C) = a | f*mu | e | f with
    a = gamma*rs, f = (a*rs)*c2, e = -a*c1 (cb None without c12)."""
    mu, rs = _f64(mean), _f64(rstd)
    a = rs if gamma is None else ar.mul(_f64(gamma, mu)[None], rs)
    bz = ar.sub(torch.zeros_like(mu) if beta is None else _f64(beta, mu)[None].expand_as(mu), ar.mul(mu, a))
    ci = torch.stack([a, bz, mu, rs], 1)
    return ci, (None if c12 is None else _cb(a, mu, rs, _f64(c12, mu), ar))


def mlp_finalize_cb(ci, c12, ar=FP32):
    """The cb that mlp_bwd_finalize_kernel (csrc/mlp_fused.hip:778-785) derives from its own c12 and the ci of the same
    BatchNorm: a = ci[0], mu = ci[2], f = (a*ci[3])*c2."""
    ci = _f64(ci)
    return _cb(ci[:, 0], ci[:, 2], ci[:, 3], _f64(c12, ci), ar)


def mlp_max_prep(g, y, cb, slope, nseg, ar=FP32):
    """tpg_mlp_max_prep, csrc/mlp_fused.hip:419-442: ag = bf16(a * (y > 0 ? g : g*slope)) per (group, channel)."""
    g, y, cb = _f64(g), _f64(y), _f64(cb)
    a = _rows(cb[:, 0], g.shape[0] // nseg)
    s = float(np.float32(slope)) if ar.emulate else float(slope)       # the launch takes the slope as a float
    return ar.bf16(ar.mul(a, torch.where(y > 0, g, ar.mul(g, s))))


def mlp_bn_bwd_apply(g, x, ci, c12, nseg, K=0, ar=FP32):
    """tpg_mlp_bn_bwd_apply (csrc/mlp_fused.hip:1010-1067): f = (a*rs)*c2, e = a*(((mu*rs)*c2) - c1),
    dx = bf16(fma(a, g, fma(-f, x, e))).  K > 0: tpg_mlp_bn_bwd_apply_rowsum (1073-1134) -> (dx, qneg) with
    qneg = -sum_k dx_bf16 over each group of K rows, fp32, k ascending."""
    g, x, ci, c12 = _f64(g), _f64(x), _f64(ci), _f64(c12)
    P = x.shape[0] // nseg
    a, mu, rs, c1, c2 = ci[:, 0], ci[:, 2], ci[:, 3], c12[:, 0], c12[:, 1]
    f = ar.mul(ar.mul(a, rs), c2)
    e = ar.mul(a, ar.sub(ar.mul(ar.mul(mu, rs), c2), c1))
    dx = ar.bf16(ar.fma(_rows(a, P), g, ar.fma(-_rows(f, P), x, _rows(e, P))))
    if not K:
        return dx
    dk = dx.view(-1, K, x.shape[1])
    q = torch.zeros_like(dk[:, 0])
    for k in range(K):
        q = ar.sub(q, dk[:, k])
    return dx, q


def mlp_bwd_operands(x_out, g_out, arg, K, cbo, x_in, cbi, slope_in, nseg, ar=FP32, round_d=True):
    """The MFMA operands of tpg_mlp_dgrad / tpg_mlp_wgrad as the kernels define them (both read the same).

    d = dx_out - e per row and output channel (d_out8<MODE>, csrc/mlp_fused.hip:390-414):
        DENSE  fma(a, g, fma(-f, x, f*mu))       MAX  fma(-f, x, f*mu) + (arg == row % K ? ag : 0)
      round_d=True: in the kernel's fp32 and rounded to bf16 (the `emulated` level); round_d=False: exact in float64
      (the `contract` level), with R_d bounding what the kernel's fp32 steps and bf16 rounding may move each element:
      |d_kernel - d| <= 2^-8 |d| + 2^-22 (|c| + |d|), c = -f (x - mu) (one rounding of c, one of c + a g, one to bf16).
    z_in = fma(x_in, sc, sh) in fp32, the lrelu' mask m = z_in > 0 ? 1 : slope_in, a_in = bf16(max(z, z*slope_in))
    (the mlp_wgrad_kernel prologue, 921-937); W is rounded to bf16 by the consumers below."""
    x_out, x_in, cbo, cbi = _f64(x_out), _f64(x_in), _f64(cbo), _f64(cbi)
    P = x_out.shape[0] // nseg
    a, fm, e, f = (_rows(cbo[:, i], P) for i in range(4))
    if round_d:
        c = ar.fma(-f, x_out, fm)
    else:
        c = fm - f * x_out
    if arg is None:
        g_out = _f64(g_out, x_out)
        d = ar.fma(a, g_out, c) if round_d else a * g_out + c
    else:
        rows = torch.arange(x_out.shape[0], device=x_out.device)
        grp = rows // K                                  # segments hold whole groups: global group = row // K
        hit = arg.to(x_out.device).long()[grp] == (rows % P % K)[:, None]
        gg = torch.where(hit, _f64(g_out, x_out)[grp], torch.zeros_like(x_out))
        d = ar.add(c, gg) if round_d else c + gg
    if round_d:
        d, R = ar.bf16(d), torch.zeros_like(d)
    else:
        R = BF16_REL * d.abs() + 2.0 ** -22 * (c.abs() + d.abs())
    s = float(np.float32(slope_in)) if ar.emulate else float(slope_in)
    sc, sh, mu = (_rows(cbi[:, i], P) for i in range(3))
    z = ar.fma(x_in, sc, sh)
    m = torch.where(z > 0, torch.ones_like(z), torch.full_like(z, s))
    a_in = ar.bf16(torch.where(z > 0, z, ar.mul(z, s)))
    xm = ar.sub(x_in, mu)                                # x_in - mu in fp32, as the dgrad epilogue's sums take it
    return dict(d=d, R=R, e=_f64(cbo[:, 2]), m=m, a_in=a_in, xm=xm, rs=cbi[:, 3], nseg=nseg, P=P, ar=ar)


def mlp_dgrad_ref(ops, W, round_w=True):
    """tpg_mlp_dgrad from mlp_bwd_operands: g_in = ((d + e) . W_bf) * m before its rounding to bf16 (the kernel adds
    e^T W as a bias in its epilogue, 494-500 and 639-659), the magnitude M = (|d| |W_bf| + |e| |W_bf|) |m| and the
    contract level's allowance R = (R_d |W_bf|) |m| of every element; then BN_in's backward sums of the launch's
    finalize (730-792): c12 = (sum g / P | rs * sum g (x - mu) / P), dbeta = sum over segments of sum g, dgamma = of
    rs * sum g (x - mu).  The kernel sums the UNROUNDED fp32 g of its epilogue, not the stored bf16 rows: so does this.
    S1 / S2 (nseg, C): sum (M + |g|) resp. rs * sum (M + |g|) |x - mu| per segment, what the sums' bounds scale with."""
    nseg, P, ar = ops["nseg"], ops["P"], ops["ar"]
    Wb = ar.bf16(_f64(W, ops["d"])) if round_w else _f64(W, ops["d"])
    Wb = Wb.view(-1, *Wb.shape[-2:])
    g, M, R = [], [], []
    for s in range(nseg):
        w = Wb[s if Wb.shape[0] > 1 else 0]
        sl = slice(s * P, (s + 1) * P)
        d, m, e = ops["d"][sl], ops["m"][sl], ops["e"][s]
        g.append((d @ w + (e @ w)[None]) * m)
        M.append((d.abs() @ w.abs() + (e.abs() @ w.abs())[None]) * m.abs())
        R.append((ops["R"][sl] @ w.abs()) * m.abs())
    g, M, R = torch.cat(g), torch.cat(M), torch.cat(R)
    rs, xm = ops["rs"], ops["xm"]
    Cin = g.shape[1]
    s1 = g.view(nseg, P, Cin).sum(1)
    sx = (g * xm).view(nseg, P, Cin).sum(1) * rs
    w1 = M + g.abs()
    S1 = w1.view(nseg, P, Cin).sum(1)
    S2 = (w1 * xm.abs()).view(nseg, P, Cin).sum(1) * rs
    return dict(g=g, M=M, R=R, c12=ar.r(torch.stack([s1 / P, sx / P], 1)), dbeta=ar.r(s1.sum(0)),
                dgamma=ar.r(sx.sum(0)), S1=S1, S2=S2)


def mlp_wgrad_ref(ops):
    """tpg_mlp_wgrad from mlp_bwd_operands (mlp_wgrad_kernel 845-980 + mlp_wgrad_reduce_kernel 984-1006):
    dW[s] = d^T a_in + e (x) sum_rows a_in per segment, M = |d|^T |a_in| + |e| (x) sum |a_in|, R = R_d^T |a_in|."""
    nseg, P = ops["nseg"], ops["P"]
    dW, M, R = [], [], []
    for s in range(nseg):
        sl = slice(s * P, (s + 1) * P)
        d, A, e = ops["d"][sl], ops["a_in"][sl], ops["e"][s]
        dW.append(d.t() @ A + e[:, None] * A.sum(0)[None])
        M.append(d.abs().t() @ A.abs() + e.abs()[:, None] * A.abs().sum(0)[None])
        R.append(ops["R"][sl].t() @ A.abs())
    return dict(dW=torch.stack(dW), M=torch.stack(M), R=torch.stack(R))


# The fp32 accumulation bound: a sum of n terms computed in fp32 along a summation tree of depth h, in any order, is
# within h * 2^-24 * sum |terms| of the exact sum (to first order).  The deepest chains of these launches are the data
# gradient's Cout + 2 (the MFMA k-loop over the output channels, the e^T W bias summed sequentially, its addition, the
# lrelu' product) and the weight gradient's rows of a workgroup + 1 + ceil(G/4) + 3 (a workgroup's row tiles into one
# accumulator, the rank-one fma, then mlp_wgrad_reduce_kernel's four strided groups of slabs and their combination):
# at most ~340 for every launch geometry of the tests (which assert h <= 512), so kappa = 512 * 2^-24 = 2^-15.
MLP_KAPPA = 2.0 ** -15


def mlp_bwd_case(Cin, Cout, P, nseg, per_seg, K, mode_max, slope_out, seed, device="cpu", mu_channel=5):
    """Inputs of one dgrad / wgrad launch: bf16 rows x_in (nseg*P, Cin), x_out (nseg*P, Cout) with per-channel offsets,
    x_out's channel `mu_channel` at |mu| / sigma ~ 1e3 (1 +- 2^-7 on one row in 61); fp32 mean / rstd of the rows' own
    fp64 statistics per segment (eps 1e-5), gamma / beta; c12_out of the arriving gradient gg in fp64.
    DENSE: g_out (nseg*P, Cout) bf16, on the |mu| >> sigma channel correlated with xhat (so that c2, and with it the
    f*(x - mu) term that the centring protects, is O(1) there).  MAX: gout, y = lrelu(.) of slope_out, arg (nseg*P/K,
    Cout); gg = gout * lrelu'(y) on each group's arg-max row.  W (nseg or 1, Cout, Cin) fp32.  All on `device`."""
    g = torch.Generator().manual_seed(seed)
    N = nseg * P
    x_in = (torch.randn(N, Cin, generator=g) * 0.8 + 0.5 * torch.randn(Cin, generator=g)).bfloat16()
    x_out = (torch.randn(N, Cout, generator=g) + torch.randn(Cout, generator=g)).bfloat16()
    r = torch.arange(N) % P
    k = torch.where(r % 122 == 0, 1.0, torch.where(r % 122 == 61, -1.0, 0.0))
    x_out[:, mu_channel] = (1.0 + k * 2.0 ** -7).bfloat16()

    def stats(x):
        xv = x.double().view(nseg, P, -1)
        return xv.mean(1).float(), (1.0 / torch.sqrt(xv.var(1, unbiased=False) + 1e-5)).float()
    mean_in, rstd_in = stats(x_in)
    mean_out, rstd_out = stats(x_out)
    gamma_in, beta_in = torch.rand(Cin, generator=g) + 0.5, 0.3 * torch.randn(Cin, generator=g)
    gamma_out, beta_out = torch.rand(Cout, generator=g) + 0.5, 0.3 * torch.randn(Cout, generator=g)
    xhat = (x_out.double() - mean_out.double().repeat_interleave(P, 0)) * rstd_out.double().repeat_interleave(P, 0)
    case = dict(x_in=x_in, x_out=x_out, mean_in=mean_in, rstd_in=rstd_in, mean_out=mean_out, rstd_out=rstd_out,
                gamma_in=gamma_in, beta_in=beta_in, gamma_out=gamma_out, beta_out=beta_out, K=K if mode_max else 0)
    if mode_max:
        G = P // K
        gout = torch.randn(nseg * G, Cout, generator=g).bfloat16()
        y = torch.randn(nseg * G, Cout, generator=g)
        y = torch.where(y > 0, y, y * slope_out).bfloat16()
        arg = torch.randint(0, K, (nseg * G, Cout), generator=g).to(torch.uint8)
        gg = torch.zeros(nseg * G, K, Cout, dtype=torch.float64)
        gg.scatter_(1, arg.long()[:, None], (gout.double() * torch.where(y > 0, 1.0, float(slope_out)).double())[:, None])
        gg = gg.view(N, Cout)
        case.update(gout=gout, y=y, arg=arg)
    else:
        g_out = torch.randn(N, Cout, generator=g)
        g_out[:, mu_channel] = 0.5 * xhat[:, mu_channel].float() + 0.5 * g_out[:, mu_channel]
        g_out = g_out.bfloat16()
        gg = g_out.double()
        case.update(g_out=g_out, arg=None)
    c12 = torch.stack([gg.view(nseg, P, -1).mean(1), (gg * xhat).view(nseg, P, -1).mean(1)], 1).float()
    W = torch.randn(nseg if per_seg else 1, Cout, Cin, generator=g) / Cin ** 0.5
    case.update(c12_out=c12, W=W if (per_seg or nseg == 1) else W[0])
    return {n: (v.to(device) if isinstance(v, torch.Tensor) else v) for n, v in case.items()}


# comparison helpers shared by tests/test_oracle_cpu.py (planted defects) and tests/test_mlp_gpu.py (the kernels)
def gin_bound(ref, M, R, kappa):
    """A bf16-stored g_in: one RNE rounding (2^-8 of the fp32 value, itself within kappa*M + R of ref) plus the fp32
    accumulation (kappa*M) plus, at the contract level, the rounding allowance of d carried through W (R)."""
    return BF16_REL * ref.abs() + (1.0 + BF16_REL) * (kappa * M + R)


def dw_bound(M, R, kappa):
    """An fp32 dW: the accumulation over rows, slabs and the rank-one term (kappa*M) plus R (contract level)."""
    return kappa * M + R


def sums_bound(S, ref, kappa):
    """BN_in's backward sums: each summed g within kappa*M of the reference, summed in fp32 at a depth that kappa also
    bounds (kappa * (1 + kappa) * S, S = sum (M + |g|) times the sum's weight), then rounded once to fp32."""
    return kappa * (1.0 + kappa) * S + U32 * ref.abs()


def err_ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound (0 where equal, inf where bound == 0 and they differ): <= 1 passes."""
    err = (_f64(got) - _f64(ref, _f64(got))).abs()
    bound = _f64(bound, err)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max()) if r.numel() else 0.0


# ---- the fused MLP tail's forward (mlp_fwd_kernel + mlp_stats_finalize_kernel): geometry, restatement, bounds --------
# The launcher's constants, copied: a retuned constant must be copied here too (tests/test_oracle_cpu.py holds the
# restated G equal to tpg_mlp_fwd_blocks, and every GPU case re-asserts which launch edge it still reaches).
TPG_ML_WAVES = 4              # csrc/mlp_fused.hip, ML_THREADS / 64
TPG_ML_MAX_BLOCKS = 512       # csrc/mlp_fused.hip
TPG_ML_WPAD = 8               # csrc/mlp_fused.hip
MLP_FWD_SAFETY = 2.0          # second-order terms of the first-order statistics bounds, once (as SMALL_SAFETY)


def mlp_fwd_geometry(P, nseg, Cin, Cout):
    """The integer decisions of one tpg_mlp_fwd call with P rows per segment (fwd_strips, fwd_smem, the `slots` rule of
    fwd_launch, fwd_blocks; tpg_bn::split and the `fits` test of mlp_stats_finalize_kernel) -> dict: STRIPS, BM (rows
    per tile), smem, slots, tiles, G (workgroups = partials per segment), tiles_wg (G,) tiles of each workgroup (it
    walks tiles b, b + G, ...), n_wave (G, 4) valid rows of each wave over its workgroup's tiles, n_wg (G,), lane_rows
    (most rows one lane accumulates), last_wg (the workgroup of the last tile), fin_SP / fin_L, fits, sweeps, dead
    (lane groups without a segment in the last sweep)."""
    strips = 2 if (Cout <= 128 and Cin <= 128) else 1
    rows_wave = strips * 16
    bm = TPG_ML_WAVES * rows_wave
    w, red = Cout * (Cin + TPG_ML_WPAD) * 2, 4 * TPG_ML_WAVES * 3 * Cout
    smem = max(w, red) + 4 * 2 * Cin
    slots = 256 if 2 * smem > 160 * 1024 else TPG_ML_MAX_BLOCKS
    tiles = -(-P // bm)
    G = min(tiles, max(16, slots // nseg))
    b = np.arange(G)
    tiles_wg = (tiles - b + G - 1) // G
    r = np.arange(P)
    slot = ((r // bm) % G) * TPG_ML_WAVES + (r % bm) // rows_wave
    n_wave = np.bincount(slot, minlength=G * TPG_ML_WAVES).reshape(G, TPG_ML_WAVES)
    sp, L = _bn_split(nseg)
    return dict(P=P, nseg=nseg, Cin=Cin, Cout=Cout, STRIPS=strips, BM=bm, smem=smem, slots=slots, tiles=tiles, G=G,
                tiles_wg=tiles_wg, n_wave=n_wave, n_wg=n_wave.sum(1), lane_rows=int(tiles_wg.max()) * strips * 4,
                last_wg=(tiles - 1) % G, fin_SP=sp, fin_L=L, fits=G <= L * TPG_BN_FIN_R, sweeps=-(-nseg // sp),
                dead=-(-nseg // sp) * sp - nseg)


MLP_FWD_MU_CHANNEL = 5        # the output channel of mlp_fwd_case with |mean| / sigma ~ 1e3


def mlp_fwd_case(Cin, Cout, P, nseg, per_seg, ss_kind, seed, device="cpu"):
    """Inputs of one tpg_mlp_fwd call: bf16 rows x (nseg*P, Cin) with per-channel and per-segment offsets; ss_kind None
    (no input BatchNorm), "ss" ((nseg,2,Cin) = sc | sh) or "ci" (a (nseg,4,Cin) block whose last two rows the forward
    must not read); W fp32 (nseg, Cout, Cin) (per_seg) or (1, Cout, Cin), / sqrt(Cin); gamma, beta, mean_shift (Cout);
    running_mean / running_var away from 0 / 1, num_batches_tracked = 3; eps, momentum.
    Output channel MLP_FWD_MU_CHANNEL is 8 + lrelu(x0): input channel 1 is exactly 1 after the prologue (sc = 0,
    sh = 1; without ss the rows hold 1) and carries a weight of 8, input channel 0 is +-2^-4 on one row in 61 (0
    elsewhere, sc = 1, sh = 0) with weight 1: |mean| / sigma ~ 1e3 in the stored bf16 values."""
    g = torch.Generator().manual_seed(seed)
    N = nseg * P
    x = torch.randn(N, Cin, generator=g) * 0.7 + 0.3 * torch.randn(Cin, generator=g)
    x = x + (0.2 * torch.randn(nseg, Cin, generator=g)).repeat_interleave(P, 0)
    r = torch.arange(N) % P
    x[:, 0] = torch.where(r % 122 == 0, 1.0, torch.where(r % 122 == 61, -1.0, 0.0)) * 2.0 ** -4
    if ss_kind is None:
        ss = None
        x[:, 1] = 1.0
    else:
        ss = torch.stack([torch.rand(nseg, Cin, generator=g) + 0.5, 0.3 * torch.randn(nseg, Cin, generator=g)], 1)
        ss[:, 0, 0], ss[:, 1, 0] = 1.0, 0.0
        ss[:, 0, 1], ss[:, 1, 1] = 0.0, 1.0
        if ss_kind == "ci":
            ss = torch.cat([ss, 1e3 * torch.randn(nseg, 2, Cin, generator=g)], 1)
        else:
            assert ss_kind == "ss", ss_kind
    W = torch.randn(nseg if per_seg else 1, Cout, Cin, generator=g) / Cin ** 0.5
    W[:, MLP_FWD_MU_CHANNEL] = 0.0
    W[:, MLP_FWD_MU_CHANNEL, 0], W[:, MLP_FWD_MU_CHANNEL, 1] = 1.0, 8.0
    case = dict(x=x.bfloat16(), ss=ss, W=W, nseg=nseg, P=P, per_seg=per_seg,
                gamma=torch.rand(Cout, generator=g) + 0.5, beta=0.3 * torch.randn(Cout, generator=g),
                mean_shift=torch.randn(Cout, generator=g), running_mean=0.5 * torch.randn(Cout, generator=g),
                running_var=torch.rand(Cout, generator=g) + 0.5, num_batches_tracked=torch.tensor(3, dtype=torch.int64),
                eps=1e-5, momentum=0.1)
    return {n: (v.to(device) if isinstance(v, torch.Tensor) else v) for n, v in case.items()}


def mlp_fwd_operand(case, slope):
    """The MFMA A operand of mlp_fwd_kernel, bit for bit: a = bf16(max(t, fp32(t * slope))), t = fma(x, sc, sh) (sc = 1,
    sh = 0 without ss: t = x), float64 carriers (nseg*P, Cin)."""
    x = _f64(case["x"])
    P = case["P"]
    if case["ss"] is None:
        t = x
    else:
        ss = _f64(case["ss"], x)
        t = fma32(x, _rows(ss[:, 0], P), _rows(ss[:, 1], P))
    return rbf16(torch.maximum(t, r32(t * slope32(slope))))


def mlp_fwd_ref(case, slope, a=None, W=None):
    """y64 = a . bf16(W)^T per segment in float64 and M = |a| . |bf16(W)|^T, (nseg*P, Cout) each (a, W: overrides of the
    operand and the weight, for the planted defects)."""
    a = mlp_fwd_operand(case, slope) if a is None else a
    Wb = rbf16(_f64(case["W"] if W is None else W, a))
    Wb = Wb.view(-1, *Wb.shape[-2:])
    P, nseg = case["P"], case["nseg"]
    y, M = [], []
    for s in range(nseg):
        w = Wb[s if Wb.shape[0] > 1 else 0]
        y.append(a[s * P:(s + 1) * P] @ w.t())
        M.append(a[s * P:(s + 1) * P].abs() @ w.abs().t())
    return dict(y=torch.cat(y), M=torch.cat(M), a=a)


def mlp_fwd_stored_interval(ref, kappa):
    """The kernel's fp32 accumulator lies within kappa * M of y64 and rounding is monotone: the stored bf16 value lies
    in [bf16(y64 - kappa M), bf16(y64 + kappa M)] -> (lo, hi); where they coincide the check is bit for bit."""
    return rbf16(ref["y"] - kappa * ref["M"]), rbf16(ref["y"] + kappa * ref["M"])


def mlp_fwd_stored_ratio(got, ref, kappa):
    """The stored bf16 y against mlp_fwd_stored_interval: the largest distance from the interval's centre over its
    half-width (0 where both ends coincide and the bits match, inf where they coincide and the bits differ)."""
    lo, hi = mlp_fwd_stored_interval(ref, kappa)
    return err_ratio(got, 0.5 * (lo + hi), 0.5 * (hi - lo))


def _mlp_fwd_slots(geo, device):
    P, bm, G = geo["P"], geo["BM"], geo["G"]
    r = torch.arange(P, device=device)
    slot = ((r // bm) % G) * TPG_ML_WAVES + (r % bm) // (geo["STRIPS"] * 16)
    piv_row = (torch.arange(G, device=device)[:, None] * bm +
               torch.arange(TPG_ML_WAVES, device=device)[None] * geo["STRIPS"] * 16).reshape(-1)
    return slot, piv_row


def mlp_fwd_stats(y, case, geo):
    """The statistics of the STORED rows y (nseg*P, Cout; bf16 values, exact in float64) and how far the kernels' may
    lie from them, from the geometry alone.
    Per wave (workgroup b, wave w; pivot = its first row, d = y - pivot): s1 = sum d and s2 = sum d^2 run down a lane's
    rows (tiles_wg * STRIPS * 4) and two shuffles, h = that depth; d rounds once, the fma once per row:
        E_s1 = (h + 1) u A,  E_s2 = (h + 3) u Q                       A = sum |d|, Q = sum d^2
        m = s1 / n,  mean_w = pivot + m:  E_mean_w = E_s1 / n + u |m| + u |mean_w|
        M2_w = s2 - s1 m:                 E_M2_w = E_s2 + 2 |m| E_s1 + 2u |s1 m| + u M2_w
    Chan's combination of the waves with rows, in wave order, fp32 (nothing rounds for the first one):
        delta = mean_w - mean,  r = n_w / tot,  mean' = mean + delta r,  M2' = M2 + (M2_w + delta^2 (n n_w / tot))
        E_mean' = (1 - r) E_mean + r E_mean_w + 3u |delta| r + u |mean'|
        E_M2'   = E_M2 + E_M2_w + 2 |delta| c (E_mean + E_mean_w + u |delta|) + 4u |term| + u |M2_w + term| + u M2'
    The finalize is fp64: mean = sum n_g mean_g / N, var = sum (M2_g + n_g (mean_g - mean)^2) / N carry the partials'
    bounds, then round once; rstd moves by 0.5 dvar / (var + eps) of itself, plus its rounding.  The running statistics
    follow the kernel's chain (fp64, one fp32 rounding per segment, call order, mean_shift in the mean only, unbiased
    variance where N > 1), their bounds E' = (1 - mom) E + mom E_new + u |running'|.  u = MLP_FWD_SAFETY * 2^-24.
    -> dict: part_n, part_mean, part_M2 with E_part_mean, E_part_M2 (nseg, G, Cout); mean, var, rstd with E_mean,
    E_rstd (nseg, Cout); running_mean, running_var with E_running_mean, E_running_var (Cout) if the case has them."""
    y = _f64(y)
    dev = y.device
    nseg, P = case["nseg"], case["P"]
    C = y.shape[1]
    G, nwv = geo["G"], TPG_ML_WAVES
    u = MLP_FWD_SAFETY * U32
    yv = y.view(nseg, P, C)
    slot, piv_row = _mlp_fwd_slots(geo, dev)
    n = torch.as_tensor(geo["n_wave"], dtype=torch.float64, device=dev).reshape(1, G * nwv, 1)
    piv = yv[:, piv_row.clamp(max=P - 1)]                           # (nseg, G*4, C); unused where n == 0
    d = yv - piv[:, slot]

    def per_wave(t):
        return torch.zeros(nseg, G * nwv, C, dtype=torch.float64, device=dev).index_add_(1, slot, t)
    s1, A, Q = per_wave(d), per_wave(d.abs()), per_wave(d * d)
    del d
    h = torch.as_tensor(geo["tiles_wg"] * geo["STRIPS"] * 4 + 2, dtype=torch.float64, device=dev)
    h = h.repeat_interleave(nwv).reshape(1, G * nwv, 1)
    n1 = n.clamp_min(1.0)
    m = s1 / n1
    mean_w = piv + m
    M2_w = (Q - s1 * m).clamp_min(0.0)
    E_s1, E_s2 = (h + 1.0) * u * A, (h + 3.0) * u * Q
    E_mean_w = E_s1 / n1 + u * m.abs() + u * mean_w.abs()
    E_M2_w = E_s2 + 2.0 * m.abs() * E_s1 + 2.0 * u * (s1 * m).abs() + u * M2_w

    def wv(t, w):
        return t.view(t.shape[0], G, nwv, -1)[:, :, w]
    zero = torch.zeros(nseg, G, C, dtype=torch.float64, device=dev)
    na, mean, M2, Em, Eq = zero[..., :1].clone(), zero.clone(), zero.clone(), zero.clone(), zero.clone()
    for w in range(nwv):
        nw_, mw, qw, Emw, Eqw = wv(n, w), wv(mean_w, w), wv(M2_w, w), wv(E_mean_w, w), wv(E_M2_w, w)
        act, first = nw_ > 0, na == 0
        tot = (na + nw_).clamp_min(1.0)
        r = nw_ / tot
        delta = mw - mean
        c = na * nw_ / tot
        term = delta * delta * c
        mean_n = mean + delta * r
        M2_n = M2 + (qw + term)
        Em_n = (1.0 - r) * Em + r * Emw + torch.where(first, zero, 3.0 * u * delta.abs() * r + u * mean_n.abs())
        Eq_n = Eq + Eqw + torch.where(first, zero, 2.0 * delta.abs() * c * (Em + Emw + u * delta.abs()) +
                                      4.0 * u * term + u * (qw + term) + u * M2_n)
        mean, M2 = torch.where(act, mean_n, mean), torch.where(act, M2_n, M2)
        Em, Eq = torch.where(act, Em_n, Em), torch.where(act, Eq_n, Eq)
        na = na + nw_
    eps, mom = slope32(case["eps"]), slope32(case["momentum"])
    N = float(P)
    mean64, var = yv.mean(1), yv.var(1, unbiased=False)
    E_m64 = (na * Em).sum(1) / N
    E_var = (Eq + 2.0 * na * (mean - mean64[:, None]).abs() * (Em + E_m64[:, None])).sum(1) / N
    rstd = 1.0 / torch.sqrt(var + eps)
    out = dict(part_n=na.expand(nseg, G, C), part_mean=mean, part_M2=M2, E_part_mean=Em, E_part_M2=Eq,
               mean=mean64, var=var, rstd=rstd, E_mean=E_m64 + u * mean64.abs(),
               E_rstd=rstd * (0.5 * E_var / (var + eps)) + u * rstd, E_var=E_var)
    if case.get("running_mean") is not None:
        rm, rv = _f64(case["running_mean"], y).clone(), _f64(case["running_var"], y).clone()
        sh = 0.0 if case.get("mean_shift") is None else _f64(case["mean_shift"], y)
        sc = N / (N - 1.0) if P > 1 else 1.0
        Erm, Erv = torch.zeros_like(rm), torch.zeros_like(rv)
        for s in range(nseg):
            rm = r32((1.0 - mom) * rm + mom * (mean64[s] + sh))
            rv = r32((1.0 - mom) * rv + mom * var[s] * sc)
            Erm = (1.0 - mom) * Erm + mom * E_m64[s] + u * rm.abs()
            Erv = (1.0 - mom) * Erv + mom * E_var[s] * sc + u * rv.abs()
        out.update(running_mean=rm, running_var=rv, E_running_mean=Erm, E_running_var=Erv)
    return out


def mlp_fwd_stats_ratios(st, part=None, mean=None, rstd=None, running_mean=None, running_var=None):
    """error / bound of whatever is given against st = mlp_fwd_stats(...): part (nseg, G, 3, C) = mean | M2 | n (n must
    be equal: ratio 0 or inf), mean / rstd (nseg, C), the running statistics (C) -> dict of floats, <= 1 passes."""
    out = {}
    if part is not None:
        part = _f64(part, st["mean"])
        out["part_n"] = 0.0 if torch.equal(part[:, :, 2], st["part_n"]) else float("inf")
        out["part_mean"] = err_ratio(part[:, :, 0], st["part_mean"], st["E_part_mean"])
        out["part_M2"] = err_ratio(part[:, :, 1], st["part_M2"], st["E_part_M2"])
    for name, got in (("mean", mean), ("rstd", rstd), ("running_mean", running_mean), ("running_var", running_var)):
        if got is not None:
            out[name] = err_ratio(_f64(got, st["mean"]), st[name], st["E_" + name])
    return out


def mlp_fwd_partials_emulated(y, case, geo, pivot_zero=False):
    """The (nseg, G, 3, Cout) partials mean | M2 | n as mlp_fwd_kernel's epilogue computes them from the stored rows y,
    op for op in fp32 (a lane's rows in tile, strip, register order, the two shuffles, the per-wave mean and M2, Chan's
    combination in wave order); rows past P add an exact 0.  pivot_zero: the planted defect of tests/test_oracle_cpu.py
    (no pivot: s1 = sum y, s2 = sum y^2 in fp32).  For the CPU tests: it shows the bounds of mlp_fwd_stats hold for the
    arithmetic the kernel is written in, and that they reject the defect."""
    ar = FP32
    y = _f64(y)
    dev = y.device
    nseg, P = case["nseg"], case["P"]
    C = y.shape[1]
    G, nwv, S, bm = geo["G"], TPG_ML_WAVES, geo["STRIPS"], geo["BM"]
    T = int(geo["tiles_wg"].max())
    yv = y.view(nseg, P, C)
    _, piv_row = _mlp_fwd_slots(geo, dev)
    n = torch.as_tensor(geo["n_wave"], dtype=torch.float64, device=dev).reshape(1, G, nwv, 1)
    piv = yv[:, piv_row.clamp(max=P - 1)].view(nseg, G, nwv, 1, C)
    if pivot_zero:
        piv = torch.zeros_like(piv)
    b, w, lq = (torch.arange(k, device=dev) for k in (G, nwv, 4))
    s1 = torch.zeros(nseg, G, nwv, 4, C, dtype=torch.float64, device=dev)
    s2 = torch.zeros_like(s1)
    for j in range(T):
        for st in range(S):
            for r in range(4):
                row = ((b[:, None, None] + j * G) * bm + (w[None, :, None] * S + st) * 16 + 4 * lq[None, None, :] + r)
                valid = (row < P) & ((b[:, None, None] + j * G) < geo["tiles"])
                v = yv[:, row.clamp(max=P - 1).reshape(-1)].view(nseg, G, nwv, 4, C)
                dd = torch.where(valid[None, ..., None], ar.sub(v, piv), torch.zeros_like(v))
                s1 = ar.add(s1, dd)
                s2 = ar.fma(dd, dd, s2)

    def lanes(t):                                   # + shfl_xor 16, + shfl_xor 32: lq pairs (0,1) (2,3), then both
        p01, p23 = ar.add(t[..., 0, :], t[..., 1, :]), ar.add(t[..., 2, :], t[..., 3, :])
        return ar.add(p01, p23)
    s1, s2 = lanes(s1), lanes(s2)                   # (nseg, G, 4, C)
    n1 = n.clamp_min(1.0)
    has = (n > 0).expand_as(s1)
    m = torch.where(has, ar.r(s1 / n1), torch.zeros_like(s1))
    mean_w = ar.add(piv[..., 0, :].expand_as(m), m)
    M2_w = torch.where(has, ar.sub(s2, ar.mul(s1, m)), torch.zeros_like(s1))
    zero = torch.zeros(nseg, G, C, dtype=torch.float64, device=dev)
    na, mean, M2 = zero.clone(), zero.clone(), zero.clone()
    for k in range(nwv):
        nw_ = n[:, :, k].expand(nseg, G, C)
        act = nw_ > 0
        tot = (na + nw_).clamp_min(1.0)
        delta = ar.sub(mean_w[:, :, k], mean)
        mean_n = ar.add(mean, ar.mul(delta, ar.r(nw_ / tot)))
        M2_n = ar.add(M2, ar.add(M2_w[:, :, k], ar.mul(ar.mul(delta, delta), ar.r(ar.mul(na, nw_) / tot))))
        mean, M2, na = torch.where(act, mean_n, mean), torch.where(act, M2_n, M2), torch.where(act, tot, na)
    return torch.stack([mean, M2, na], 2)


def mlp_fwd_finalize(part, case, order=None):
    """mlp_stats_finalize_kernel on given partials (nseg, G, 3, C): fp64 mean = sum n_g mean_g / N and biased var =
    sum (M2_g + n_g (mean_g - mean)^2) / N (the order of the fp64 additions is not restated: 2^-53 relative), mean and
    rstd rounded to fp32, the running chain over the segments in `order` (default: call order) -> dict."""
    part = _f64(part)
    n, pm, pq = part[:, :, 2], part[:, :, 0], part[:, :, 1]
    N = n.sum(1)
    m = (n * pm).sum(1) / N
    var = ((pq + n * (pm - m[:, None]) ** 2) * (n > 0)).sum(1) / N
    var = var.clamp_min(0.0)
    eps, mom = slope32(case["eps"]), slope32(case["momentum"])
    out = dict(mean=r32(m), rstd=r32(1.0 / torch.sqrt(var + eps)))
    if case.get("running_mean") is not None:
        rm, rv = _f64(case["running_mean"], part).clone(), _f64(case["running_var"], part).clone()
        sh = 0.0 if case.get("mean_shift") is None else _f64(case["mean_shift"], part)
        for s in (range(part.shape[0]) if order is None else order):
            unb = torch.where(N[s] > 1.0, var[s] * N[s] / (N[s] - 1.0).clamp_min(1.0), var[s])
            rm = r32((1.0 - mom) * rm + mom * (m[s] + sh))
            rv = r32((1.0 - mom) * rv + mom * unb)
        out.update(running_mean=rm, running_var=rv)
    return out


# ---- the 16 -> 16 -> 32 small tails (csrc/mlp_small.hip): restatements and derived per-element bounds ---------------
# out[n] = max_j lrelu_s2(W2 . lrelu_s1(W1 . h[n, j])) and its backward, exact in float64 on any device.  The kernels
# compute in fp32 on v_mfma_f32_16x16x4_f32 (fmaf chains) whatever the row type, so every bound below is a first-order
# running-error bound in u = U32, propagated through the magnitudes |W| . |x|; SMALL_SAFETY = 2 covers the second-order
# terms, once, by doubling u everywhere (the z1-sign threshold included).  Nothing here is measured on a kernel.
SMALL_SAFETY = 2.0


def slope32(s):
    """A LeakyReLU slope as the launch receives it: a C float."""
    return float(np.float32(s))


def small_tail_geometry(P):
    """(tiles, workgroups) of tpg_small_tail_bwd (small_bwd_blocks): 16 points per tile, 4 waves per workgroup, at
    most 1024 workgroups; a wave takes tiles wave, wave + 4 * workgroups, ..."""
    tiles = -(-P // 16)
    return tiles, max(1, min(1024, -(-tiles // 4)))


def small_tail_depth(P, K):
    """h_w, the deepest fp32 chain of a weight-gradient element: a wave's trips x 16 k-steps per edge slot x K into one
    accumulator, the reduce kernel's strided groups of slabs, the 16 group sums."""
    tiles, blocks = small_tail_geometry(P)
    return -(-tiles // (4 * blocks)) * 16 * K + -(-(4 * blocks) // 16) + 16


def _small_hidden(h, W1, s1, u):
    z1 = h @ W1.t()
    a1 = torch.where(z1 > 0, z1, z1 * s1)
    M1 = h.abs() @ W1.abs().t()
    E1 = 16 * u * M1                               # a 16-term fmaf chain
    return z1, a1, M1, E1, E1 + u * a1.abs()       # lrelu is 1-Lipschitz for slopes in [0, 1]; z1 * s1 rounds once


def small_tail_fwd_ref(h, W1, W2, s1, s2, K):
    """h (P*K, 16), W1 (16, 16), W2 (32, 16) -> dict of float64 tensors: the exact z1, a1 (P*K, 16), z2 (P*K, 32),
    best = max_j z2, out = lrelu_s2(best) before the store's rounding (P, 32), arg (P, 32) uint8 = the FIRST maximum
    (lowest j); the magnitudes M1 = |W1| . |h|, M2 = |W2| . |a1| and the bounds
        E1 = 16u M1,  Ea1 = E1 + u |a1|,  E2 = |W2| . Ea1 + 16u M2,  E2max = max_j E2,  Eout = E2max + u |out|
    (max over j and lrelu are 1-Lipschitz; a bf16 store: small_stored_bound)."""
    h = _f64(h)
    W1, W2 = _f64(W1, h), _f64(W2, h)
    s1, s2, u = slope32(s1), slope32(s2), SMALL_SAFETY * U32
    P = h.shape[0] // K
    z1, a1, M1, E1, Ea1 = _small_hidden(h, W1, s1, u)
    z2 = a1 @ W2.t()
    M2 = a1.abs() @ W2.abs().t()
    E2 = Ea1 @ W2.abs().t() + 16 * u * M2
    z2v = z2.view(P, K, W2.shape[0])
    best = z2v.max(1)[0]
    ks = torch.arange(K, device=h.device)[None, :, None]
    arg = torch.where(z2v == best[:, None], ks, K).min(1)[0]
    out = torch.where(best > 0, best, best * s2)
    E2max = E2.view(P, K, W2.shape[0]).max(1)[0]
    return dict(z1=z1, a1=a1, z2=z2, best=best, out=out, arg=arg.to(torch.uint8), M1=M1, M2=M2, E1=E1, Ea1=Ea1, E2=E2,
                E2max=E2max, Eout=E2max + u * out.abs())


def small_tail_bwd_ref(h, out_sign, gout, arg, W1, W2, s1, s2, K, h_w=None):
    """The backward as the kernel defines it, `arg` (P, 32) and the sign of `out` (any tensor positive where out is)
    taken as given, exactly as the kernel reads them back:
        gp = out > 0 ? gout : gout s2,  gz2[n, j, c] = (arg[n, c] == j) gp[n, c],  ga1 = W2^T gz2,
        gz1 = ga1 (z1 > 0 ? 1 : s1),  gh = W1^T gz1,  dW1 = sum_edges gz1 (x) h,  dW2 = sum_edges gz2 (x) a1.
    -> dict: the exact float64 values, the magnitude sums S1 / S2 of the weight gradients' terms, and the bounds
        Egz2 = u |gz2|                                               (gout s2 rounds once)
        Ega1 = 32u |W2|^T |gz2| + |W2|^T Egz2                        (a 32-term chain)
        Egz1 = Ega1 lrelu'(z1) + u |gz1|; where |z1| <= E1 (`flip`: the recomputed sign may differ there)
               Ega1 + u |gz1| + (1 - s1) |ga1|
        Egh  = |W1|^T Egz1 + 16u |W1|^T |gz1|                        (a bf16 store: small_stored_bound)
        EdW1 = h_w u S1 + sum Egz1 (x) |h|,   EdW2 = h_w u S2 + sum (Egz2 (x) |a1| + |gz2| (x) Ea1)
    with h_w = small_tail_depth(P, K) unless given."""
    h = _f64(h)
    W1, W2, gout = _f64(W1, h), _f64(W2, h), _f64(gout, h)
    s1, s2, u = slope32(s1), slope32(s2), SMALL_SAFETY * U32
    P = h.shape[0] // K
    h_w = small_tail_depth(P, K) if h_w is None else h_w
    z1, a1, _, E1, Ea1 = _small_hidden(h, W1, s1, u)
    gp = torch.where(out_sign.to(h.device) > 0, gout, gout * s2)
    hit = arg.to(h.device).long()[:, None, :] == torch.arange(K, device=h.device)[None, :, None]
    gz2 = torch.where(hit, gp[:, None, :], torch.zeros_like(gp[:, None, :])).reshape(P * K, W2.shape[0])
    Egz2 = u * gz2.abs()
    ga1 = gz2 @ W2
    Ega1 = 32 * u * (gz2.abs() @ W2.abs()) + Egz2 @ W2.abs()
    dz1 = torch.where(z1 > 0, torch.ones_like(z1), torch.full_like(z1, s1))
    gz1 = ga1 * dz1
    flip = z1.abs() <= E1
    Egz1 = Ega1 * torch.where(flip, torch.ones_like(dz1), dz1) + u * gz1.abs() + \
        torch.where(flip, (1.0 - s1) * ga1.abs(), torch.zeros_like(ga1))
    gh = gz1 @ W1
    Egh = Egz1 @ W1.abs() + 16 * u * (gz1.abs() @ W1.abs())
    S1, S2 = gz1.abs().t() @ h.abs(), gz2.abs().t() @ a1.abs()
    return dict(z1=z1, a1=a1, gz2=gz2, ga1=ga1, gz1=gz1, gh=gh, dW1=gz1.t() @ h, dW2=gz2.t() @ a1, S1=S1, S2=S2,
                flip=flip, Egz1=Egz1, Egh=Egh, h_w=h_w, EdW1=h_w * u * S1 + Egz1.t() @ h.abs(),
                EdW2=h_w * u * S2 + Egz2.t() @ a1.abs() + gz2.abs().t() @ Ea1)


def small_stored_bound(ref, E, bf16):
    """A stored row value: within E of ref in fp32, then one round-to-nearest-even to bf16 of that value."""
    return E + BF16_REL * (ref.abs() + E) if bf16 else E


# ---- fused BatchNorm + LeakyReLU (+ max over K) on rows (csrc/rowbn.hip): geometry, per-launch restatements, bounds --
# The launcher's tunables, copied: a retuned constant must be copied here too, and tests/test_rowbn_cpu.py then
# re-asserts which launch edge each case of tests/rowbn_cases.py still reaches.
TPG_BN_THREADS = 256          # csrc/rowbn.hip, BN_THREADS
TPG_BN_MAX_BLOCKS = 256       # csrc/rowbn.hip
TPG_BN_STATS_ROWS = 8         # csrc/rowbn.hip
TPG_BN_YRED_ROWS = 4          # csrc/rowbn.hip
TPG_BN_STATS_U = 8            # csrc/rowbn.hip
TPG_BN_APPLY_CAP = 256        # csrc/rowbn.hip
TPG_BN_APPLY_ROWS = 8         # csrc/rowbn.hip
TPG_BN_GROUP_CAP = 512        # csrc/rowbn.hip
TPG_BN_UNROLL = 4             # csrc/rowbn.hip
TPG_BN_BWD_U = 2              # csrc/rowbn.hip
TPG_BN_SEG_DIV = 4            # csrc/rowbn.hip
TPG_BN_FIN_R = 8              # csrc/tpg_bn_finalize.hpp, FIN_R
ROWBN_SAFETY = 2.0            # second-order terms of the first-order bounds below, once (as SMALL_SAFETY)


def _bn_row_blocks(rows, rpi, per_thread, cap):
    return max(1, min(cap, -(-rows // (rpi * per_thread))))


def _bn_seg_blocks(blocks, nseg):
    return max(1, -(-blocks // min(nseg, TPG_BN_SEG_DIV)))


def _bn_group_cap(nseg, cap_div):
    return (2 * TPG_BN_GROUP_CAP if nseg <= 3 else TPG_BN_GROUP_CAP) // cap_div


def _bn_group_unroll(K):
    return 4 if K % 4 == 0 else (2 if K % 2 == 0 else 1)


def _bn_group_runs(Gp, K, cpr, nseg, room):
    L = 1
    while K % (2 * L) == 0 and (K // (2 * L)) % 4 == 0 and Gp * L * cpr * nseg < 65536 and \
            (room == 0 or Gp * 2 * L <= room):
        L *= 2
    return L


def _bn_split(nseg):
    sp = 1
    while sp < nseg and sp < 64:
        sp <<= 1
    return sp, 64 // sp


def _is_bf16(dt):
    return dt in (torch.bfloat16, "bf16")


def rowbn_geometry(P, K, C, dtype_in, dtype_other, nseg=1):
    """The integer decisions of tpg_rowbn_fwd / tpg_rowbn_bwd (csrc/rowbn.hip: row_blocks, stats_blocks, seg_blocks,
    group_cap, group_unroll, group_runs with the forward's `room`; csrc/tpg_bn_finalize.hpp: split, pair_sums) for P
    rows per segment.  dtype_other: the output's type for the forward, the arriving gradient's for the backward.
    -> dict: *_stats the statistics walk (the INPUT type's vector width), the others the apply / backward walks:
    ne, cpr (chunks per row), rpi (rows per workgroup iteration), idle (threads of a workgroup without a column chunk),
    G_stats / G_bwd (workgroups = partials per segment of the reductions), fin_L (lanes per segment of a finalize
    wave) and fin_blocks_* (trips of pair_sums' outer loop), L_* (runs per group), U_* (rows per pipeline stage),
    grid_* (workgroups per segment of the streaming launch), per_* = (fewest, most) rows (K = 0: statistics, apply,
    reduce), groups (max-variant reduce) or runs (max-variant apply) a thread that has any walks."""
    bf_in, bf_any = _is_bf16(dtype_in), _is_bf16(dtype_in) or _is_bf16(dtype_other)
    ne_s, ne = (8 if bf_in else 4), (8 if bf_any else 4)
    assert C > 0 and C % ne == 0 and C // 4 <= TPG_BN_THREADS and 0 <= K <= 256 and (K == 0 or P % K == 0)
    cpr_s, cpr = C // ne_s, C // ne
    rpi_s, rpi = TPG_BN_THREADS // cpr_s, TPG_BN_THREADS // cpr
    cap_div = min(nseg, TPG_BN_SEG_DIV)
    sp, fl = _bn_split(nseg)

    def per(rows, threads):
        return (rows // threads if rows >= threads else 1, -(-rows // threads))
    G_stats = _bn_seg_blocks(_bn_row_blocks(P, rpi_s, TPG_BN_STATS_ROWS, TPG_BN_MAX_BLOCKS), nseg)
    rows_g = P // K if K else P
    G_bwd = _bn_seg_blocks(_bn_row_blocks(rows_g, rpi, TPG_BN_YRED_ROWS if K else TPG_BN_STATS_ROWS,
                                          TPG_BN_MAX_BLOCKS), nseg)
    if K:
        L_fwd = _bn_group_runs(rows_g, K, cpr, nseg, TPG_BN_MAX_BLOCKS * 8 // 5)
        L_bwd = _bn_group_runs(rows_g, K, cpr, nseg, 0)
        grid_fwd = _bn_row_blocks(rows_g * L_fwd, rpi, 1, _bn_group_cap(nseg, cap_div))
        grid_bwd = _bn_row_blocks(rows_g * L_bwd, rpi, 1, _bn_group_cap(nseg, cap_div))
        U_fwd, U_bwd = _bn_group_unroll(K // L_fwd), _bn_group_unroll(K // L_bwd)
        per_fwd, per_bwd = per(rows_g * L_fwd, grid_fwd * rpi), per(rows_g * L_bwd, grid_bwd * rpi)
    else:
        L_fwd = L_bwd = 1
        grid_fwd = grid_bwd = _bn_row_blocks(P, rpi, TPG_BN_APPLY_ROWS, TPG_BN_APPLY_CAP // cap_div)
        U_fwd, U_bwd = TPG_BN_UNROLL, TPG_BN_BWD_U
        per_fwd = per_bwd = per(P, grid_fwd * rpi)
    return dict(P=P, K=K, C=C, nseg=nseg, ne_stats=ne_s, cpr_stats=cpr_s, rpi_stats=rpi_s,
                idle_stats=TPG_BN_THREADS - cpr_s * rpi_s, G_stats=G_stats, per_stats=per(P, G_stats * rpi_s),
                fin_SP=sp, fin_L=fl, fin_blocks_stats=-(-G_stats // (fl * TPG_BN_FIN_R)),
                ne=ne, cpr=cpr, rpi=rpi, idle=TPG_BN_THREADS - cpr * rpi, G_bwd=G_bwd,
                per_reduce=per(rows_g, G_bwd * rpi), fin_blocks_bwd=-(-G_bwd // (fl * TPG_BN_FIN_R)),
                L_fwd=L_fwd, L_bwd=L_bwd, U_fwd=U_fwd, U_bwd=U_bwd, grid_fwd=grid_fwd, grid_bwd=grid_bwd,
                per_fwd=per_fwd, per_bwd=per_bwd)


def _bn_partials(t, G, rpi, ar):
    """Per-workgroup partial column sums of the rows t (n, C) as the reduction kernels take them: thread (workgroup b,
    rsub) adds its rows b*rpi + rsub + j*G*rpi in ascending order into one fp32 accumulator, block_column_reduce adds
    the rpi accumulators of a column in ascending rsub -> (G, C).  (A missing row adds +0: exact.)"""
    n, C = t.shape
    step = G * rpi
    J = -(-n // step)
    if J * step != n:
        t = torch.cat([t, torch.zeros(J * step - n, C, dtype=t.dtype, device=t.device)])
    t = t.view(J, G, rpi, C)
    acc = torch.zeros_like(t[0])
    for j in range(J):
        acc = ar.add(acc, t[j])
    s = torch.zeros_like(acc[:, 0])
    for r in range(rpi):
        s = ar.add(s, acc[:, r])
    return s


def _bn_consts(C, nseg, mean, rstd, gamma, beta, like):
    """mean / rstd (nseg or 1, C) or None, gamma / beta (C) or None -> float64 mu, rs (nseg, C), gm, b (C): absent
    constants read as the kernels' ld_consts defaults (0, 1, 1, 0)."""
    mu = torch.zeros(1, C, dtype=torch.float64, device=like.device) if mean is None else _f64(mean, like).reshape(-1, C)
    rs = torch.ones(1, C, dtype=torch.float64, device=like.device) if rstd is None else _f64(rstd, like).reshape(-1, C)
    gm = torch.ones(C, dtype=torch.float64, device=like.device) if gamma is None else _f64(gamma, like)
    b = torch.zeros(C, dtype=torch.float64, device=like.device) if beta is None else _f64(beta, like)
    return mu.expand(nseg, C), rs.expand(nseg, C), gm, b


def rowbn_stats_ref(x, nseg, eps, momentum, dtype_in, running_mean=None, running_var=None, num_batches_tracked=None,
                    mean_shift=None, ar=FP32):
    """rowbn_stats_kernel + rowbn_stats_finalize_kernel: x (nseg*P, C) -> dict(mean, rstd (nseg, C), running_mean,
    running_var (C) after the chain over the segments in call order, num_batches_tracked, and per segment the
    magnitudes S1 = sum |d|, S2 = sum d^2, m = sum d / P, var of the bound).  d = x - pivot (the segment's first row)
    and d*d round once each, the sums are _bn_partials, everything from the partials on is fp64 as in the kernel
    (the ORDER of the fp64 additions is not restated: 2^-53 relative), mean = fp32(pivot + m),
    rstd = fp32(1 / sqrt(var + eps)), running = fp32((1 - momentum) * running + momentum * new) with the unbiased
    variance for P > 1.  ar = FP64: the same algebra, no rounding.  eps and momentum are the launch's C floats."""
    x = _f64(x)
    N, C = x.shape
    P = N // nseg
    geo = rowbn_geometry(P, 0, C, dtype_in, dtype_in, nseg)
    G, rpi = geo["G_stats"], geo["rpi_stats"]
    eps, mom = slope32(eps), slope32(momentum)
    rm = None if running_mean is None else _f64(running_mean, x).clone()
    rv = None if running_var is None else _f64(running_var, x).clone()
    sh = 0.0 if mean_shift is None else _f64(mean_shift, x)
    out = {k: [] for k in ("mean", "rstd", "S1", "S2", "m", "var", "mean64")}
    for s in range(nseg):
        xs = x[s * P:(s + 1) * P]
        piv = xs[0]
        d = ar.sub(xs, piv[None])
        dd = ar.mul(d, d)
        p0, p1 = _bn_partials(d, G, rpi, ar), _bn_partials(dd, G, rpi, ar)
        m = p0.sum(0) / P
        var = (p1.sum(0) / P - m * m).clamp_min(0.0)
        pm = piv + m
        out["mean"].append(ar.r(pm))
        out["rstd"].append(ar.r(1.0 / torch.sqrt(var + eps)))
        out["mean64"].append(pm)
        out["S1"].append(d.abs().sum(0))
        out["S2"].append(dd.sum(0))
        out["m"].append(m)
        out["var"].append(var)
        if rm is not None:
            unbiased = var * P / (P - 1) if P > 1 else var
            rm = ar.r((1.0 - mom) * rm + mom * (pm + sh))
            rv = ar.r((1.0 - mom) * rv + mom * unbiased)
    out = {k: torch.stack(v) for k, v in out.items()}
    out.update(running_mean=rm, running_var=rv, geo=geo, P=P, eps=eps, momentum=mom,
               num_batches_tracked=None if num_batches_tracked is None else int(num_batches_tracked) + nseg)
    return out


def rowbn_stats_bound(ref, running_mean=None, running_var=None):
    """|kernel - FP64 twin| of mean, rstd (nseg, C) and the running statistics (C), from the twin `ref` =
    rowbn_stats_ref(..., ar=FP64) alone.  h = rows per thread + rpi LDS additions (_bn_partials' chain), fp64 after.
      sum d   : each d rounds once (u |d|), the chain adds h u sum |d|                  -> Em = (h + 1) u S1 / P
      sum d^2 : d's rounding twice, the product once, the chain                        -> Ess = (h + 3) u S2 / P
      var = ss/P - m^2                                                                 -> Ev = Ess + 2 |m| Em
      mean = fp32(pivot + m): Em + u |mean|;  rstd is monotone in var: the larger one-sided change of
      (var +- Ev + eps)^-1/2 (var - Ev clamped at 0, as the kernel clamps), + u rstd for its rounding
      running' = fp32((1 - mom) running + mom new): E' = (1 - mom) E + mom E_new + u |running'| along the chain, the
      unbiased variance scaling Ev by P / (P - 1).
    u = ROWBN_SAFETY * 2^-24."""
    geo, P, eps, mom = ref["geo"], ref["P"], ref["eps"], ref["momentum"]
    u = ROWBN_SAFETY * U32
    h = geo["per_stats"][1] + geo["rpi_stats"]
    Em = (h + 1) * u * ref["S1"] / P
    Ev = (h + 3) * u * ref["S2"] / P + 2.0 * ref["m"].abs() * Em
    var, rstd = ref["var"], ref["rstd"]
    up = 1.0 / torch.sqrt((var - Ev).clamp_min(0.0) + eps) - rstd
    dn = rstd - 1.0 / torch.sqrt(var + Ev + eps)
    out = dict(mean=Em + u * ref["mean"].abs(), rstd=torch.maximum(up, dn) + u * rstd, h=h)
    if running_mean is not None:
        rm, rv = _f64(running_mean, var), _f64(running_var, var)
        sc = P / (P - 1) if P > 1 else 1.0
        Erm, Erv = torch.zeros_like(rm), torch.zeros_like(rv)
        for s in range(var.shape[0]):
            rm = (1.0 - mom) * rm + mom * ref["mean64"][s]          # magnitudes only: mean_shift moves no bound
            rv = (1.0 - mom) * rv + mom * var[s] * sc
            Erm = (1.0 - mom) * Erm + mom * Em[s] + u * (rm.abs() + Erm)
            Erv = (1.0 - mom) * Erv + mom * Ev[s] * sc + u * (rv.abs() + Erv)
        out.update(running_mean=Erm, running_var=Erv)
    return out


def _bn_z(xs, mu, a, b, ar):
    """bn_z of csrc/rowbn.hip: (v - mu) * a + beta, each operation rounded once."""
    return ar.add(ar.mul(ar.sub(xs, mu), a), b)


def rowbn_apply_ref(x, K, mean, rstd, gamma, beta, slope, nseg=1, ar=FP32):
    """rowbn_apply_kernel / rowbn_apply_max_kernel (+ rowbn_max_combine_kernel) with GIVEN statistics: a = gamma * rstd,
    z = bn_z, v = z > 0 ? z : z * slope, all (nseg*P, C); K > 0: y = max over each group of K rows, arg = the FIRST
    maximum (lowest k; the runs of a cut group and the first-run-wins combine define the same) -> dict(z, v, y, arg):
    y before the store's rounding (rowbn_stored).  The slope is the launch's C float."""
    x = _f64(x)
    N, C = x.shape
    P = N // nseg
    mu, rs, gm, b = _bn_consts(C, nseg, mean, rstd, gamma, beta, x)
    a = ar.mul(gm[None], rs)
    z = _bn_z(x, _rows(mu, P), _rows(a, P), b[None], ar)
    s = slope32(slope)
    v = torch.where(z > 0, z, ar.mul(z, s))
    if not K:
        return dict(z=z, v=v, y=v, arg=None, a=a)
    vk = v.view(N // K, K, C)
    y = vk.max(1)[0]
    ks = torch.arange(K, device=x.device)[None, :, None]
    arg = torch.where(vk == y[:, None], ks, K).min(1)[0].to(torch.uint8)
    return dict(z=z, v=v, y=y, arg=arg, a=a)


def rowbn_stored(v, bf16):
    """A row element as the kernels store it: fp32, or one round-to-nearest-even of that fp32 value to bf16."""
    return rbf16(r32(v)) if bf16 else r32(v)


def rowbn_guard(gamma, beta, C, like, fixed=True):
    """The per-channel choice of rowbn_bwd_reduce_max_kernel's (gy, y) form: |beta| <= 4 |gamma| in fp32 and (fixed) a
    finite non-zero fp32 1 / gamma -> (inv (C) bool, ig = fp32(1 / gamma), float64; 0 where not inv)."""
    gm = torch.ones(C, dtype=torch.float64, device=like.device) if gamma is None else _f64(gamma, like)
    b = torch.zeros(C, dtype=torch.float64, device=like.device) if beta is None else _f64(beta, like)
    inv = b.abs() <= r32(4.0 * gm.abs())
    ig = r32(1.0 / gm)
    if fixed:
        inv = inv & torch.isfinite(ig) & (ig != 0)
    return inv, torch.where(inv, ig, torch.zeros_like(ig))


def rowbn_bwd_sums_ref(gy, x, arg, y, K, mean, rstd, gamma, beta, slope, nseg, dtype_in, dtype_g, training=True,
                       ar=FP32, fixed_guard=True):
    """The backward reductions + rowbn_bwd_finalize_kernel, per segment of P rows.
    K == 0 (rowbn_bwd_reduce_kernel) and the gather form of K > 0 (rowbn_bwd_reduce_max_kernel, y None or the guard
    false: x read at the arg-max row): gg = bn_z(v) > 0 ? g : g * slope, xhat = (v - mu) * rstd, terms gg | gg * xhat.
    Stored-output form (y given, channels where rowbn_guard holds): pos = y > 0, gg = pos ? g : g * slope,
    z = pos ? y : y * fp32(1 / slope) (slope 0: * 0), xhat = (z - beta) * fp32(1 / gamma).
    Sums: _bn_partials over the rows (K == 0) or the groups, then fp64: c12 (nseg, 2, C) = fp32(s / P | sx / P) with P
    the ROWS of a segment (zero in eval mode), dbeta = fp32(sum over segments of s), dgamma = of sx.
    ar = FP64: the same algebra without rounding (the guard and 1 / gamma stay those of the kernel's fp32 inputs).
    -> dict(c12, dgamma, dbeta, inv, and for the bounds S0 = sum |gg|, S1 = sum |gg xhat|, gg, xhat per summed row)."""
    x, gy = _f64(x), _f64(gy)
    N, C = x.shape
    P = N // nseg
    geo = rowbn_geometry(P, K, C, dtype_in, dtype_g, nseg)
    G, rpi = geo["G_bwd"], geo["rpi"]
    mu, rs, gm, b = _bn_consts(C, nseg, mean, rstd, gamma, beta, x)
    a = ar.mul(gm[None], rs)
    s = slope32(slope)
    rows = P // K if K else P
    if K:
        v = x.view(-1, K, C).gather(1, arg.to(x.device).long()[:, None])[:, 0]
    else:
        v = x
    z = _bn_z(v, _rows(mu, rows), _rows(a, rows), b[None], ar)
    gg = torch.where(z > 0, gy, ar.mul(gy, s))
    xh = ar.mul(ar.sub(v, _rows(mu, rows)), _rows(rs, rows))
    inv = torch.zeros(C, dtype=torch.bool, device=x.device)
    if K and y is not None:
        y = _f64(y, x)
        inv, ig = rowbn_guard(gamma, beta, C, x, fixed_guard)
        isl = (float(np.float32(1.0) / np.float32(s)) if ar.emulate else 1.0 / s) if s != 0.0 else 0.0
        igv = ig if ar.emulate else torch.where(inv, 1.0 / gm, ig)
        pos = y > 0
        gg_y = torch.where(pos, gy, ar.mul(gy, s))
        zz = torch.where(pos, y, ar.mul(y, isl))
        xh_y = ar.mul(ar.sub(zz, b[None]), igv[None])
        gg, xh = torch.where(inv[None], gg_y, gg), torch.where(inv[None], xh_y, xh)
    t1 = ar.mul(gg, xh)
    s0 = torch.stack([_bn_partials(gg[i * rows:(i + 1) * rows], G, rpi, ar).sum(0) for i in range(nseg)])
    s1 = torch.stack([_bn_partials(t1[i * rows:(i + 1) * rows], G, rpi, ar).sum(0) for i in range(nseg)])
    c12 = ar.r(torch.stack([s0 / P, s1 / P], 1)) if training else torch.zeros(nseg, 2, C, dtype=torch.float64, device=x.device)
    return dict(c12=c12, dbeta=ar.r(s0.sum(0)), dgamma=ar.r(s1.sum(0)), inv=inv, geo=geo, P=P, gg=gg, xhat=xh, g=gy, z=z,
                S0=gg.abs().view(nseg, rows, C).sum(1), S1=t1.abs().view(nseg, rows, C).sum(1))


def rowbn_kink(ref_apply, x, mean, nseg):
    """Where the FP64 twin's pre-activation z is too close to 0 for its sign to be the fp32 one: |z| <= the first-order
    error of bn_z, u (3 |(x - mu) a| + |z|) with u = ROWBN_SAFETY * 2^-24 (a's, the difference's and the product's
    rounding, the sum's) -> bool (N, C)."""
    x = _f64(x)
    P = x.shape[0] // nseg
    mu = _f64(mean, x).reshape(-1, x.shape[1]).expand(nseg, -1) if mean is not None else \
        torch.zeros(nseg, x.shape[1], dtype=torch.float64, device=x.device)
    t = ((x - _rows(mu, P)) * _rows(ref_apply["a"], P)).abs()
    return ref_apply["z"].abs() <= ROWBN_SAFETY * U32 * (3.0 * t + ref_apply["z"].abs())


def rowbn_bwd_sums_bound(ref, slope, flip=None, stored=None):
    """|kernel - FP64 twin| of the gather-form sums, from the twin `ref` = rowbn_bwd_sums_ref(..., y=None, ar=FP64):
    h = rows (groups) per thread + rpi LDS additions; gg rounds once (g * slope), xhat twice, their product once:
      s  : (h + 1) u S0,   sx : (h + 4) u S1,   then dbeta / dgamma sum them over the segments and round once,
      c1 = fp32(s / P), c2 = fp32(sx / P) round once.
    flip (rows, C) bool: summed rows whose lrelu' the fp32 sign of z may take from the other side (rowbn_kink at the
    summed rows): each allows (1 - slope) |g| resp. (1 - slope) |g xhat| more.
    stored = dict(gamma, beta, bf16): the stored-output form, judged against the SAME gather-form twin.  On the
    channels of rowbn_guard xhat is recovered from the stored y instead: z' = y or y * fp32(1/slope) carries y's own
    distance from the exact z (the forward's fp32 bn_z, 3u (|z - beta| + |z|) generously, its bf16 store 2^-8 |z| as in
    tests/test_autograd_ops.py::_stored_y_allowance) plus 3u |z| for the two roundings of the inversion, z' - beta
    rounds once and 1 / gamma once more (3u |z - beta|): Exhat = (6u |z - beta| + (6u [+ 2^-8]) |z|) / |gamma|, and
    sx allows sum |gg| Exhat more (the guard |beta| <= 4 |gamma| keeps |z| / |gamma| within |xhat| / rstd + 4)."""
    geo, P = ref["geo"], ref["P"]
    u = ROWBN_SAFETY * U32
    h = geo["per_reduce"][1] + geo["rpi"]
    nseg, C = ref["S0"].shape
    E0, E1 = (h + 1) * u * ref["S0"], (h + 4) * u * ref["S1"]
    s = slope32(slope)
    if flip is not None:
        f = flip.to(torch.float64) * abs(1.0 - s) * ref["g"].abs()
        E0 = E0 + f.view(nseg, -1, C).sum(1)
        E1 = E1 + (f * ref["xhat"].abs()).view(nseg, -1, C).sum(1)
    if stored is not None:
        gmv = torch.ones(C, dtype=torch.float64) if stored["gamma"] is None else _f64(stored["gamma"])
        bv = torch.zeros(C, dtype=torch.float64) if stored["beta"] is None else _f64(stored["beta"])
        zt = ref["z"]                                               # the twin's z at the summed rows
        rel = 6.0 * u + (BF16_REL if stored["bf16"] else 0.0)
        Ex = (6.0 * u * (zt - bv[None]).abs() + rel * zt.abs()) / gmv.abs()[None]
        inv = rowbn_guard(stored["gamma"], stored["beta"], C, zt)[0]
        Ex = torch.where(inv[None], Ex, torch.zeros_like(Ex))
        E1 = E1 + (ref["gg"].abs() * Ex).view(nseg, -1, C).sum(1)
    c12 = torch.stack([E0 / P, E1 / P], 1)
    c12 = c12 + u * (ref["c12"].abs() + c12)
    Eb, Eg = E0.sum(0), E1.sum(0)
    return dict(c12=c12, dbeta=Eb + u * (ref["dbeta"].abs() + Eb), dgamma=Eg + u * (ref["dgamma"].abs() + Eg), h=h)


def rowbn_bwd_apply_ref(gy, x, arg, K, mean, rstd, gamma, beta, slope, c12, nseg, ar=FP32):
    """rowbn_bwd_apply_kernel / rowbn_bwd_apply_max_kernel: a = gamma * rstd, gg = bn_z(x) > 0 ? g : g * slope (K > 0:
    only on the row k == arg of its group, else 0), dx = a * ((gg - c1) - ((x - mu) * rstd) * c2), c12 (nseg, 2, C) or
    None (absent constants read as zero) -> dict(dx before the store's rounding, and E: the first-order bound of
    |fp32 - FP64 twin| per element, u |a| (|gg| + 2 |gg - c1| + 4 |xhat c2| + 2 |inner|) with u = ROWBN_SAFETY * 2^-24:
    g * slope, the difference twice counted through the outer one, xhat's two roundings, its product, the product
    with a and a's own rounding)."""
    x, gy = _f64(x), _f64(gy)
    N, C = x.shape
    P = N // nseg
    mu, rs, gm, b = _bn_consts(C, nseg, mean, rstd, gamma, beta, x)
    a = ar.mul(gm[None], rs)
    s = slope32(slope)
    c12 = torch.zeros(nseg, 2, C, dtype=torch.float64, device=x.device) if c12 is None else _f64(c12, x)
    z = _bn_z(x, _rows(mu, P), _rows(a, P), b[None], ar)
    if K:
        rows = torch.arange(N, device=x.device)
        hit = arg.to(x.device).long()[rows // K] == (rows % K)[:, None]
        g = torch.where(hit, gy[rows // K], torch.zeros_like(x))
    else:
        g = gy
    gg = torch.where(z > 0, g, ar.mul(g, s))
    xh = ar.mul(ar.sub(x, _rows(mu, P)), _rows(rs, P))
    t = ar.mul(xh, _rows(c12[:, 1], P))
    e = ar.sub(gg, _rows(c12[:, 0], P))
    inner = ar.sub(e, t)
    dx = ar.mul(_rows(a, P), inner)
    E = ROWBN_SAFETY * U32 * _rows(a, P).abs() * (gg.abs() + 2.0 * e.abs() + 4.0 * t.abs() + 2.0 * inner.abs())
    E = E + 2.0 ** -149 * (1.0 + inner.abs())        # a denormal a (gamma 2^-130) and a denormal product round absolutely
    return dict(dx=dx, E=E, a=a, xhat=xh, gg=gg, z=z)


def rowbn_dx_bound(ref, Ec12, nseg, bf16):
    """dx of one tpg_rowbn_bwd call (reduce + apply): the apply's own bound E plus what the kernel's c12 (within Ec12 of
    the twin's, rowbn_bwd_sums_bound) moves it, |a| (Ec1 + |xhat| Ec2); a bf16 store on top (small_stored_bound)."""
    P = ref["dx"].shape[0] // nseg
    E = ref["E"] if Ec12 is None else \
        ref["E"] + _rows(ref["a"], P).abs() * (_rows(Ec12[:, 0], P) + ref["xhat"].abs() * _rows(Ec12[:, 1], P))
    return small_stored_bound(ref["dx"], E, bf16) + (2.0 ** -134 if bf16 else 0.0)    # half a bf16 denormal step


# ---- the row-gather kernels (csrc/rowgather.hip): geometry, FP64 twins, per-element bounds --------------------------
# The launcher's constants, copied (tests/test_rowgather_cpu.py reads the #define defaults out of csrc/rowgather.hip and
# fails when they differ, and re-asserts which launch edge every case of tests/rowgather_cases.py still reaches).
TPG_RC_FWD_U = 1                  # csrc/rowgather.hip
TPG_RC_FWD_CAP = 16384            # csrc/rowgather.hip
TPG_RC_BWD_CAP = 4096             # csrc/rowgather.hip
TPG_RC_BWD_WAVE_CAP = 16384       # csrc/rowgather.hip
TPG_RC_ROWSUM_CAP = 16384         # csrc/rowgather.hip, grid_for's default cap (rowsum_neg_kernel)
ROW_GATHER, ROW_SUB, ROW_EDGE = 0, 1, 2


def rowcombine_geometry(mode, B, N, S, K, C, dtype_in, dtype_out):
    """The integer decisions of fwd_go / bwd_go (csrc/rowgather.hip) -> dict: ne, cpr; forward: total (chunks), wgs,
    wgs_launched (rounded up to a multiple of 8 under the XCD ordering), xcd, idle (workgroups without a chunk),
    passes_fwd; backward: form ("wave" / "thread"), G (64 / cpr, wave form only), grid_bwd, passes_bwd; passes_rowsum
    (SUB's rowsum_neg launch, else 0)."""
    ne = 8 if (_is_bf16(dtype_in) or _is_bf16(dtype_out)) else 4
    assert C > 0 and C % ne == 0 and (mode != ROW_EDGE or S == N)
    cpr = C // ne
    total = B * S * K * cpr
    wgs = max(1, min(TPG_RC_FWD_CAP, -(-total // (256 * TPG_RC_FWD_U))))
    xcd = wgs >= 64
    launched = (wgs + 7) & ~7 if xcd else wgs
    rows = B * N
    wave = cpr <= 32 and 64 % cpr == 0 and not (mode == ROW_EDGE and cpr <= 2)
    if wave:
        grid = max(1, min(TPG_RC_BWD_WAVE_CAP, -(-rows // 4)))
        passes = -(-rows // (4 * grid))
    else:
        grid = max(1, min(TPG_RC_BWD_CAP, -(-rows * cpr // 256)))
        passes = -(-rows * cpr // (256 * grid))
    totq = B * S * cpr
    pq = -(-totq // (256 * max(1, min(TPG_RC_ROWSUM_CAP, -(-totq // 256))))) if mode == ROW_SUB else 0
    return dict(ne=ne, cpr=cpr, total=total, wgs=wgs, wgs_launched=launched, xcd=xcd,
                idle=launched - -(-total // 256), passes_fwd=-(-total // (launched * 256 * TPG_RC_FWD_U)),
                form="wave" if wave else "thread", G=64 // cpr if wave else None, grid_bwd=grid, passes_bwd=passes,
                passes_rowsum=pq)


def rowcombine_clamp(idx, N):
    """tpg_clamp_idx: anything outside [0, N) reads row N - 1 -> int64 indices.  (oracle/tpgref.c does not clamp.)"""
    i = idx.long()
    return torch.where((i >= 0) & (i < N), i, torch.full_like(i, N - 1))


def _rc_gather(T, idxc):
    B, S, K = idxc.shape
    Cc = T.shape[2]
    return torch.gather(T, 1, idxc.reshape(B, S * K, 1).expand(-1, -1, Cc)).view(B, S, K, Cc)


def rowcombine_fwd_twin(U, QE, idx, mode, slope=0.2, slope_u=1.0, dt=torch.float64):
    """tpg_rowcombine_fwd on values of the row type, before the store's rounding.  dt = float64: the exact value (the
    LeakyReLU's branch from the fp32 difference, whose sign is the exact one's; the slope as the launch's C float).
    dt = float32: the kernel op for op -- one rounding per subtraction, product and sum, nothing contracted.
    slope_u != 1: the front end's LeakyReLU of the gathered U row (tpg_rowcombine_edge_fwd)."""
    idxc = rowcombine_clamp(idx, U.shape[1])
    u = _rc_gather(U.to(dt).contiguous(), idxc)
    if mode == ROW_GATHER:
        return u
    QE = QE.to(dt).contiguous()
    if mode == ROW_SUB:
        return u - QE[:, :, None]
    d = _rc_gather(QE, idxc) - QE[:, :, None]
    a = u if slope_u == 1.0 else torch.where(u > 0, u, u * slope32(slope_u))
    return a + torch.where(d > 0, d, d * slope32(slope))


def rowcombine_edge_fwd_twin(Y, idx, slope_a=0.2, slope_e=0.2, dt=torch.float64):
    Cc = Y.shape[2] // 2
    return rowcombine_fwd_twin(Y[:, :, Cc:], Y[:, :, :Cc], idx, ROW_EDGE, slope_e, slope_a, dt)


def rowcombine_bwd_twin(g, idx, E, mode, N, slope=0.2, Uraw=None, slope_u=1.0, defect=None):
    """tpg_rowcombine_bwd in float64 -> {name: dict(v, n, A, depth)} per output element: the exact value, its number of
    terms, the sum of |term| and the factor of the fp32 bound depth * 2^-24 * A (rowcombine_bound):
      gU   (B,N,C)  sum over the destination's list (L entries; indices clamped as the forward reads them)    depth L
      gQE  SUB  (B,S,C): -sum_k g                                                                            depth K
           EDGE (B,N,C): sum over the list of g lrelu'(E[n] - E[s]) - sum_k g lrelu'(E[idx[n,k]] - E[n]);
                lrelu' = 1 where the fp32 difference is > 0, else the slope -- at 0 too, on BOTH sides; one more
                rounding for the slope's product                                                     depth L + K + 1
      gA   (Uraw given: the front end) gU * lrelu'(Uraw), the slope at 0                                  depth L + 1
    and L (B,N), the list lengths.  defect (tests/test_rowgather_cpu.py): "nbr_ge" takes >= on the neighbour side only,
    "a_zero" leaves slope_u out where Uraw == 0."""
    g = g.double()
    B, S, K, Cc = g.shape
    idxc = rowcombine_clamp(idx, N)
    flat = idxc.reshape(B, S * K)

    def scatter(v):
        out = torch.zeros(B, N, Cc, dtype=torch.float64, device=g.device)
        return out.scatter_add_(1, flat[:, :, None].expand(-1, -1, Cc), v.reshape(B, S * K, Cc))
    L = torch.zeros(B, N, dtype=torch.float64, device=g.device).scatter_add_(1, flat, torch.ones_like(flat, dtype=torch.float64))
    Ln = L[:, :, None].expand(B, N, Cc)
    r = dict(L=L, gU=dict(v=scatter(g), n=Ln, A=scatter(g.abs()), depth=Ln))
    if mode == ROW_SUB:
        kk = torch.full((B, S, Cc), float(K), dtype=torch.float64, device=g.device)
        r["gQE"] = dict(v=-g.sum(2), n=kk, A=g.abs().sum(2), depth=kk)
    elif mode == ROW_EDGE:
        E = E.double().contiguous()
        d = _rc_gather(E, idxc) - E[:, :, None]
        s = slope32(slope)
        gs = g * s
        ge_n = torch.where((d >= 0) if defect == "nbr_ge" else (d > 0), g, gs)
        ge_c = torch.where(d > 0, g, gs)
        r["gQE"] = dict(v=scatter(ge_n) - ge_c.sum(2), n=Ln + K, A=scatter(ge_n.abs()) + ge_c.abs().sum(2),
                        depth=Ln + (K + 1))
        if Uraw is not None:
            Ur = Uraw.double()
            f = torch.where((Ur >= 0) if defect == "a_zero" else (Ur > 0), 1.0, slope32(slope_u))
            r["gA"] = dict(v=r["gU"]["v"] * f, n=Ln, A=r["gU"]["A"] * f, depth=Ln + 1)
    return r


def rowcombine_edge_bwd_twin(g, idx, Y, slope_a=0.2, slope_e=0.2, defect=None):
    """tpg_rowcombine_edge_bwd: gY = [gE | gA] -> the twin's dict with gE (= gQE of mode EDGE) and gA."""
    Cc = Y.shape[2] // 2
    r = rowcombine_bwd_twin(g, idx, Y[:, :, :Cc], ROW_EDGE, Y.shape[1], slope_e, Y[:, :, Cc:], slope_a, defect)
    r["gE"] = r.pop("gQE")
    return r


def rowcombine_bound(t, bf16):
    """A gradient element summed in fp32 in ANY order, every term rounded at most once before: within depth * u * A of the
    exact sum (first order in u = 2^-24; depth terms meet at most depth roundings on their way).  Stored as bf16: one
    round-to-nearest-even of that fp32 value on top.  No additive slack: an element without terms is exactly 0."""
    fb = t["depth"] * U32 * t["A"]
    return fb + BF16_REL * (t["v"].abs() + fb) if bf16 else fb


def rowcombine_lists(idx, N):
    """tpg_invert_index of one cloud: idx (S*K) -> (offs (N + 1), list (S*K)) numpy, a stable sort by clamped destination."""
    ic = rowcombine_clamp(torch.as_tensor(idx).reshape(-1), N).cpu().numpy()
    return np.concatenate([[0], np.cumsum(np.bincount(ic, minlength=N))]), np.argsort(ic, kind="stable")

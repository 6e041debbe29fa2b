"""The anisotropic kernels' rule (include/tpgan_ops.h, "anisotropic kernels") stated in numpy, written from the header's
text: the yardstick for csrc/aniso.hip and for the torch statements in tpgan_amd.ops.  Every fp32 operation is a numpy
float32 operation (each rounded on its own), every float64 one a float64 operation; sums are 64-bit integers.

`kernels_eigh` states the same stages in float64 throughout with numpy.linalg.eigh in place of the Jacobi sweeps: not a
yardstick for bits, but the measure of what the rule's fp32 terms, fixed-point sums and fixed sweeps cost in accuracy."""
import collections

import numpy as np

F32, F64 = np.float32, np.float64
Params = collections.namedtuple("Params", "rc lam ks kr s_min s_max kn n_eps")


def params(rc, ks, lam=0.9, kr=4.0, s_min=0.125, s_max=2.0, kn=0.5, n_eps=25):
    """Every parameter rounded to fp32 once, as the entries take them."""
    return Params(F32(rc), F32(lam), F32(ks), F32(kr), F32(s_min), F32(s_max), F32(kn), int(n_eps))


def sq3(a, b):
    """The canonical fp32 distance: t = a - b per axis; d = t0*t0; d = d + t1*t1; d = d + t2*t2.  a (n,1,3), b (1,m,3)."""
    t = a - b
    d = t[..., 0] * t[..., 0]
    d = d + t[..., 1] * t[..., 1]
    d = d + t[..., 2] * t[..., 2]
    return d


def stage_a_sums(x, rc, rows=512):
    """x (N,3) fp32 -> (S (10,N) int64, count (N,) int32)."""
    N = x.shape[0]
    S = np.zeros((10, N), np.int64)
    count = np.zeros(N, np.int32)
    rc2 = rc * rc
    with np.errstate(invalid="ignore"):
        for a in range(0, N, rows):
            xi = x[a:a + rows, None, :]
            d2 = sq3(xi, x[None, :, :])
            member = d2 <= rc2
            d = np.sqrt(np.where(member, d2, F32(0)))
            rho = np.fmin(d / rc, F32(1))
            w = F32(1) - (rho * rho) * rho
            u = (x[None, :, :] - xi) / rc
            wu = w[..., None] * u
            terms = [w, wu[..., 0], wu[..., 1], wu[..., 2], wu[..., 0] * u[..., 0], wu[..., 0] * u[..., 1],
                     wu[..., 0] * u[..., 2], wu[..., 1] * u[..., 1], wu[..., 1] * u[..., 2], wu[..., 2] * u[..., 2]]
            for k, term in enumerate(terms):
                assert term.dtype == F32
                units = np.trunc(np.where(member, term, F32(0)) * F32(4294967296.0)).astype(np.int64)
                S[k, a:a + rows] = units.sum(1)
            count[a:a + rows] = member.sum(1)
    return S, count


def rotate(app, aqq, apq, arp, arq, vp, vq):
    """One rotation of the header, float64, for every particle at once.  vp, vq: lists of the three entries of V's
    columns p and q."""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        zero = apq == 0.0
        theta = (aqq - app) / np.where(zero, 1.0, 2.0 * apq)
        sg = np.where(theta >= 0.0, 1.0, -1.0)
        t = sg / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
        t = np.where(zero, 0.0, t)
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        h = t * apq
        new_p = [c * a - s * e for a, e in zip(vp, vq)]
        new_q = [s * a + c * e for a, e in zip(vp, vq)]
        return app - h, aqq + h, np.zeros_like(apq), c * arp - s * arq, s * arp + c * arq, new_p, new_q


def jacobi(C):
    """C: dict of the six float64 arrays 00 01 02 11 12 22 -> (sigma [3], V[k][column]) after 5 sweeps."""
    a00, a01, a02, a11, a12, a22 = (C[k].astype(F64) for k in ("00", "01", "02", "11", "12", "22"))
    one, nil = np.ones_like(a00), np.zeros_like(a00)
    V = [[one, nil, nil], [nil, one, nil], [nil, nil, one]]

    def col(j):
        return [V[0][j], V[1][j], V[2][j]]

    def put(j, v):
        for k in range(3):
            V[k][j] = v[k]
    for _ in range(5):
        a00, a11, a01, a02, a12, p, q = rotate(a00, a11, a01, a02, a12, col(0), col(1))      # (0,1), r = 2
        put(0, p), put(1, q)
        a00, a22, a02, a01, a12, p, q = rotate(a00, a22, a02, a01, a12, col(0), col(2))      # (0,2), r = 1
        put(0, p), put(2, q)
        a11, a22, a12, a01, a02, p, q = rotate(a11, a22, a12, a01, a02, col(1), col(2))      # (1,2), r = 0
        put(1, p), put(2, q)
    return [a00, a11, a22], V


PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def shape_matrices(sigma, V, count, prm):
    """Extents, G (N,6) and det (N,) in float64 from the eigen-decomposition, by the header's sequence."""
    ks, kr, lo, hi, kn = (F64(v) for v in (prm.ks, prm.kr, prm.s_min, prm.s_max, prm.kn))
    top = np.where(sigma[0] > sigma[1], sigma[0], sigma[1])
    top = np.where(top > sigma[2], top, sigma[2])
    few = (count <= prm.n_eps) | ~(top > 0.0)
    fl = top / kr
    e = []
    for s in sigma:
        x = ks * np.where(s > fl, s, fl)
        x = np.where(x < lo, lo, x)
        e.append(np.where(x > hi, hi, x))
    inv = [1.0 / x for x in e]
    G = np.zeros((count.shape[0], 6), F64)
    for n, (a, b) in enumerate(PAIRS):
        g = ((V[a][0] * inv[0]) * V[b][0] + (V[a][1] * inv[1]) * V[b][1]) + (V[a][2] * inv[2]) * V[b][2]
        G[:, n] = np.where(few, (1.0 / kn) if a == b else 0.0, g)
    det = np.where(few, 1.0 / ((kn * kn) * kn), 1.0 / ((e[0] * e[1]) * e[2]))
    return G, det


def kernels(x, prm):
    """Stage A: x (N,3) fp32, one cloud -> (centres (N,3) f32, G (N,6) f32, det (N,) f32, count (N,) int32)."""
    x = np.ascontiguousarray(x, dtype=F32)
    N = x.shape[0]
    if N == 0:
        return np.zeros((0, 3), F32), np.zeros((0, 6), F32), np.zeros(0, F32), np.zeros(0, np.int32)
    S, count = stage_a_sums(x, prm.rc)
    Sd = S.astype(F64)
    S0 = np.where(Sd[0] > 0.0, Sd[0], 1.0)
    m = [Sd[1] / S0, Sd[2] / S0, Sd[3] / S0]
    lr = F64(prm.lam) * F64(prm.rc)
    centres = np.stack([(x[:, a].astype(F64) + lr * m[a]).astype(F32) for a in range(3)], 1)
    C = {"00": Sd[4] / S0 - m[0] * m[0], "01": Sd[5] / S0 - m[0] * m[1], "02": Sd[6] / S0 - m[0] * m[2],
         "11": Sd[7] / S0 - m[1] * m[1], "12": Sd[8] / S0 - m[1] * m[2], "22": Sd[9] / S0 - m[2] * m[2]}
    sigma, V = jacobi(C)
    G, det = shape_matrices(sigma, V, count, prm)
    return centres, G.astype(F32), det.astype(F32), count


def kernels_eigh(x, prm):
    """The same stages in float64 with numpy.linalg.eigh: the fp32 membership (so that the neighbour sets agree), then
    float64 weights, plain float64 sums, eigh -> (centres, G, det) float64, count."""
    x = np.ascontiguousarray(x, dtype=F32)
    N = x.shape[0]
    rc = F64(prm.rc)
    with np.errstate(invalid="ignore"):
        member = sq3(x[:, None, :], x[None, :, :]) <= prm.rc * prm.rc
    X = x.astype(F64)
    centres, G, det = np.zeros((N, 3)), np.zeros((N, 6)), np.zeros(N)
    count = member.sum(1).astype(np.int32)
    sig, vec = np.zeros((N, 3)), np.zeros((N, 3, 3))
    for i in range(N):
        u = (X[member[i]] - X[i]) / rc
        w = 1.0 - np.minimum(np.linalg.norm(u, axis=1), 1.0) ** 3
        if w.sum() > 0:
            m = (w[:, None] * u).sum(0) / w.sum()
            C = (w[:, None, None] * u[:, :, None] * u[:, None, :]).sum(0) / w.sum() - np.outer(m, m)
        else:
            m, C = np.zeros(3), np.zeros((3, 3))
        centres[i] = X[i] + F64(prm.lam) * rc * m
        sig[i], vec[i] = np.linalg.eigh(C)
    sigma = [sig[:, k] for k in range(3)]
    V = [[vec[:, a, k] for k in range(3)] for a in range(3)]
    G, det = shape_matrices(sigma, V, count, prm)
    return centres, G, det, count


def cubic(q):
    """The cubic of tpg_radius_reduce_f32 in fp32."""
    q2 = q * q
    near = F32(6) * (q2 * q - q2) + F32(1)
    v = F32(1) - q
    far = F32(2) * (v * v * v)
    return np.fmax(np.where(q <= F32(0.5), near, far), F32(0))


def field(query, centres, G, det, support, reach, rows=256):
    """Stage B: query (Nq,3), centres (Np,3), G (Np,6), det (Np,) fp32, one cloud -> (Nq,) fp32."""
    query, centres = np.ascontiguousarray(query, dtype=F32), np.ascontiguousarray(centres, dtype=F32)
    G, det = np.ascontiguousarray(G, dtype=F32), np.ascontiguousarray(det, dtype=F32)
    R, reach = F32(support), F32(reach)
    reach2 = reach * reach
    out = np.zeros(query.shape[0], F32)
    if centres.shape[0] == 0:
        return out
    g = [G[None, :, k] for k in range(6)]
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(0, query.shape[0], rows):
            q = query[a:a + rows, None, :]
            member = sq3(q, centres[None, :, :]) <= reach2
            t = q - centres[None, :, :]
            t0, t1, t2 = t[..., 0], t[..., 1], t[..., 2]
            y0 = (g[0] * t0 + g[1] * t1) + g[2] * t2
            y1 = (g[1] * t0 + g[3] * t1) + g[4] * t2
            y2 = (g[2] * t0 + g[4] * t1) + g[5] * t2
            u = np.fmin(np.sqrt((y0 * y0 + y1 * y1) + y2 * y2) / R, F32(1))
            dw = np.fmin(np.fmax(det[None, :] * cubic(u), F32(0)), F32(512))
            assert dw.dtype == F32
            units = np.where(member, np.trunc(dw * F32(4194304.0)).astype(np.uint64), np.uint64(0))
            out[a:a + rows] = units.sum(1, dtype=np.uint64).astype(F32) * F32(2.384185791015625e-7)
    return out


def extents(G):
    """The three extents of every particle, ascending, from G (N,6): the reciprocals of G's eigenvalues (float64)."""
    G = np.asarray(G, dtype=F64)
    M = np.zeros((G.shape[0], 3, 3))
    for n, (a, b) in enumerate(PAIRS):
        M[:, a, b] = M[:, b, a] = G[:, n]
    return np.sort(1.0 / np.linalg.eigvalsh(M), axis=1)

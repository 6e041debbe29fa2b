"""The k-nearest-neighbour rule (csrc/knn_select.hpp, oracle/tpgref.c) stated in numpy.

  distance  sum_d (q_d - p_d)^2 in dimension order, every operation rounded to fp32, no FMA;
  order     ascending (distance, index); every NaN distance ranks after +Inf, NaN among themselves by index -- the
            unsigned order of the kernels' (dist_bits << 32 | idx) keys when a query's NaN distances carry one bit pattern;
  padding   (0, 0) for queries at or past len1 and for slots past len2.

The rule has no tolerance: what is compared with it must be EQUAL to it (distances with NaN == NaN)."""
import numpy as np

F32 = np.float32


def sqdist(q, p):
    """(nq, D), (np, D) fp32 -> (nq, np) fp32 canonical distances."""
    q, p = np.asarray(q, F32), np.asarray(p, F32)
    acc = np.zeros((q.shape[0], p.shape[0]), F32)
    with np.errstate(all="ignore"):
        for d in range(q.shape[1]):
            t = q[:, d, None] - p[None, :, d]
            acc = acc + t * t
    return acc


def order_keys(dist):
    """uint32 keys whose unsigned order is the rule's order of the (non-negative or NaN) fp32 distances."""
    dist = np.ascontiguousarray(dist, F32)
    keys = dist.view(np.uint32).copy()
    keys[np.isnan(dist)] = 0xFFFFFFFF
    return keys


def knn(p1, p2, K, lengths1=None, lengths2=None, chunk=256):
    """p1 (B, P1, D), p2 (B, P2, D) -> dist (B, P1, K) fp32, idx (B, P1, K) int64."""
    p1, p2 = np.asarray(p1, F32), np.asarray(p2, F32)
    B, P1, _ = p1.shape
    P2 = p2.shape[1]
    dist, idx = np.zeros((B, P1, K), F32), np.zeros((B, P1, K), np.int64)
    for b in range(B):
        n1 = P1 if lengths1 is None else min(int(lengths1[b]), P1)
        n2 = P2 if lengths2 is None else min(int(lengths2[b]), P2)
        kk = min(K, n2)
        if kk == 0:
            continue
        for q0 in range(0, n1, chunk):
            d = sqdist(p1[b, q0:min(q0 + chunk, n1)], p2[b, :n2])
            order = np.argsort(order_keys(d), axis=1, kind="stable")[:, :kk]       # stable: ties by index
            idx[b, q0:q0 + d.shape[0], :kk] = order
            dist[b, q0:q0 + d.shape[0], :kk] = np.take_along_axis(d, order, axis=1)
    return dist, idx

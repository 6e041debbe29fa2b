"""Measurements of upsampled frames on the GPU: particle density and free surface.

    python -m tpgan_amd.analysis --frames 'out/pcd_{i}.npy' --count 200 --cutoff 0.0775 --out stats.npz

The reference measures its `pcd_{i}.npy` frames on the host (train_fluid/analysis_helper.py:143-161,275-294 and
train_utils.py:269-286: a scipy KD-tree, `query_ball_tree`, a ragged list padded to a dense array, a numba loop).
Here they are a thin layer over one op, `ops.radius_reduce` (csrc/radius_reduce.hip): the number of points within a
radius and the sum of a radial kernel over them, with no cap on the number of neighbours, on the uniform grid the radius
searches already use.  Same signatures as the reference's functions; a GPU tensor in gives a GPU tensor out, a numpy
array in is moved to the current device and numpy comes back (float64 densities, int64 counts, as the reference returns).
The `*_batch` forms take (T,N,3) with lengths, so that a chunk of rollout frames is one call.  Forward only.
"""
import argparse

import numpy as np
import torch

from . import ops

BASE_RADIUS = 0.025            # train_utils.py:10: the fluid clips' particle spacing
FRAMES_PER_CALL = 8


def _in(x):
    """-> (float tensor on the GPU, came-as-numpy)"""
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.device("cuda")), True
    ops._need(isinstance(x, torch.Tensor), "positions must be a tensor or a numpy array")
    return x.detach(), False


def _cloud(x, name):
    t, host = _in(x)
    ops._need(t.dim() == 2 and t.shape[1] == 3, f"{name} must be (N,3), got {tuple(t.shape)}")
    return t, host


# ------------------------------------------------------------------------------------------------ density
def particle_density_batch(pos, cutoff, lengths=None, query=None, lengths_q=None):
    """(T,N,3) [lengths (T,)] -> (T,N) f32: per particle the sum of the cubic kernel over ALL particles of its frame
    within `cutoff`, itself included (entries beyond a frame's length are 0).  query (T,M,3): the density of `pos`
    sampled at other points instead -> (T,M)."""
    q = pos if query is None else query
    return ops.radius_reduce(q, pos, cutoff, "cubic", lengths if query is None else lengths_q, lengths)[1]


def get_particle_density(pos, cutoff):
    """analysis_helper.py:143-150: (N,3) -> (N,1)."""
    p, host = _cloud(pos, "pos")
    dns = ops.radius_reduce(p, p, cutoff, "cubic")[1].unsqueeze(1)
    return dns.double().cpu().numpy() if host else dns


def get_particle_density_of_two_pcd(pos_src, pos_dst, cutoff):
    """analysis_helper.py:153-161: the density of the cloud `pos_dst` at the points `pos_src`: (Ns,3), (Nd,3) -> (Ns,1)."""
    s, host = _cloud(pos_src, "pos_src")
    d, _ = _cloud(pos_dst, "pos_dst")
    dns = ops.radius_reduce(s, d.to(s.device), cutoff, "cubic")[1].unsqueeze(1)
    return dns.double().cpu().numpy() if host else dns


def particle_dns2grid_dns(grid_pos, pcd_pos, cutoff):
    """analysis_helper.py:291-294: the particle density on each grid point."""
    return get_particle_density_of_two_pcd(grid_pos, pcd_pos, cutoff)


# ------------------------------------------------------------------------------------------- free surface
def neighbor_num_batch(pos, radius, lengths=None):
    """(T,N,3) [lengths (T,)] -> (T,N) int32: particles of the same frame with d <= radius, itself included."""
    return ops.radius_reduce(pos, pos, radius, None, lengths, lengths)[0]


def fixed_radius_neighbor_num(pos, radius):
    """train_utils.py:269-272: (N,3) -> (N,) counts."""
    p, host = _cloud(pos, "pos")
    num = ops.radius_reduce(p, p, radius, None)[0]
    return num.cpu().numpy().astype(np.int64) if host else num


def free_surface_mask(nbr_num):
    """The rank rule of train_utils.py:283-285 on one frame's neighbour counts (n,) -> (n,) bool, on the device:
    a particle is at the free surface when its count is below 0.85 x the mean of the sorted counts between the 95 %
    and the 99 % rank (both ranks truncated by int() as there).  Below 100 particles the reference's slice is empty,
    its mean NaN, and nothing is selected; the same here."""
    n = nbr_num.shape[0]
    lo, cut = int(n * 0.95), int(n * 0.01)
    if n == 0 or cut == 0 or n - cut <= lo:
        return torch.zeros(n, dtype=torch.bool, device=nbr_num.device)
    ranked = torch.sort(nbr_num).values[lo:n - cut]
    threshold = ranked.double().mean()                      # integer counts: exact in float64, as numpy's mean
    return nbr_num.double() < 0.85 * threshold


def get_free_surface_particles(pos, radius):
    """train_utils.py:281-286: (N,3) -> the (S,3) free-surface particles, in their order in `pos`."""
    p, host = _cloud(pos, "pos")
    mask = free_surface_mask(ops.radius_reduce(p, p, radius, None)[0])
    return pos[mask.cpu().numpy()] if host else p[mask]


def free_surface_count_batch(pos, radius, lengths=None):
    """(T,N,3) [lengths (T,)] -> (T,) int64 on the device: the number of free-surface particles of every frame (one
    launch for the counts; the rank rule per frame is a device sort)."""
    num = neighbor_num_batch(pos, radius, lengths)
    T, N = num.shape
    lens = [N] * T if lengths is None else [int(v) for v in torch.as_tensor(lengths).tolist()]
    return torch.stack([free_surface_mask(num[t, :lens[t]]).sum() for t in range(T)]) if T else num.new_zeros(0).long()


def free_surface_particle_loss(pos_pred, pos_gt):
    """analysis_helper.py:275-281: |difference of the two free-surface sizes| at radius 0.025 -> int."""
    a = get_free_surface_particles(_cloud(pos_pred, "pos_pred")[0], BASE_RADIUS)
    b = get_free_surface_particles(_cloud(pos_gt, "pos_gt")[0], BASE_RADIUS)
    return abs(int(a.shape[0]) - int(b.shape[0]))


# ---------------------------------------------------------------------------------------------------- CLI
def first_difference(y):
    """d/dt of a per-frame series in units of one frame: central differences, one-sided at both ends (what the
    reference's get_1st_derivative, analysis_helper.py:164-166, is used for)."""
    y = np.asarray(y, dtype=np.float64)
    return np.gradient(y) if y.shape[0] > 1 else np.zeros_like(y)


def sequence_stats(frames, cutoff, radius=BASE_RADIUS, device="cuda", frames_per_call=FRAMES_PER_CALL):
    """frames: list of (N_t,3) arrays -> dict of per-frame series (density mean / std, free-surface count, point
    count) and their first differences; `frames_per_call` frames are padded to one (T,N,3) batch per launch."""
    dev = torch.device(device)
    mean, std, surf, npts = [], [], [], []
    for i in range(0, len(frames), frames_per_call):
        chunk = [np.ascontiguousarray(f, dtype=np.float32).reshape(-1, 3) for f in frames[i:i + frames_per_call]]
        lens = [c.shape[0] for c in chunk]
        batch = torch.zeros((len(chunk), max(max(lens), 1), 3), dtype=torch.float32)
        for t, c in enumerate(chunk):
            batch[t, :lens[t]] = torch.from_numpy(c)
        batch = batch.to(dev)
        lengths = torch.tensor(lens, dtype=torch.int64, device=dev)
        dns = particle_density_batch(batch, cutoff, lengths).double()
        free = free_surface_count_batch(batch, radius, lens)
        for t, n in enumerate(lens):
            d = dns[t, :n]
            mean.append(float(d.mean()) if n else 0.0)
            std.append(float(d.std(unbiased=False)) if n else 0.0)
        surf += [int(v) for v in free.tolist()]
        npts += lens
    out = {"density_mean": np.array(mean), "density_std": np.array(std),
           "free_surface_count": np.array(surf, dtype=np.int64), "point_count": np.array(npts, dtype=np.int64)}
    for k in list(out):
        out["d_" + k] = first_difference(out[k])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tpgan_amd.analysis",
                                 description="Particle density and free-surface statistics of a sequence of frames.")
    ap.add_argument("--frames", required=True, help="frame files, '{i}' = frame index, e.g. 'out/pcd_{i}.npy'")
    ap.add_argument("--count", type=int, required=True, help="frames 0 .. count-1")
    ap.add_argument("--cutoff", type=float, required=True, help="density cutoff (the reference uses 2.2 / 3.1 spacings)")
    ap.add_argument("--radius", type=float, default=BASE_RADIUS, help="free-surface neighbour radius")
    ap.add_argument("--out", required=True, help="output .npz")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    if "{i}" not in a.frames:
        ap.error("--frames must contain '{i}'")
    frames = []
    for i in range(a.count):
        data = np.load(a.frames.format(i=i))
        frames.append(data["pos"] if hasattr(data, "files") else data)
    stats = sequence_stats(frames, a.cutoff, a.radius, a.device)
    np.savez(a.out, cutoff=np.float64(a.cutoff), radius=np.float64(a.radius), **stats)
    print(f"wrote {a.out}: {a.count} frames, mean density {stats['density_mean'].mean():.4f}, "
          f"free-surface particles {int(stats['free_surface_count'].sum())}")


if __name__ == "__main__":
    main()

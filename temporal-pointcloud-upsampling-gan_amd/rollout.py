"""Sequence upsampling with a trained generator: the demo notebooks' rollout, T frames per network call.

The reference's `train_fluid/demo.ipynb` (cell 3) upsamples a simulated sequence one frame at a time with
`SRNet.forward_with_context` (upsampling_network.py:159-174) at B = 1.  Frames are independent through the network
body; only the 25-frame running mask average links them.  `SequenceUpsampler` runs a chunk of T frames through the body
as one batch of T and takes the masking decisions of all T frames in one fused launch (`ops.context_expand`,
csrc/rollout.hip), carrying the running-average state across chunks and `push` calls.

Reference semantics, kept on purpose: the body is called as `net.body(feature, None)` -- the reference's
`forward_with_context` passes no `pos` to the feature extractor, so with in_feats = 6 the first EdgeConv searches its
neighbours in the 6-D feature space (this project's `SRNet.forward_with_context` differs there: INTEGRATION.md).

    python -m tpgan_amd.rollout --checkpoint X.ckpt --frames 'dir/data_{i}.npz' --count 800 [--in-feats 6] --out DIR
        [--render PNGDIR --size 3 --width 768 --height 768 --mode pinhole --color depth --direction 0 0 -1
         --style points|surface --particle_radius 0.025 --smooth_iters 3 --smooth_half_width 2]
        [--mesh MESHDIR --format ply|obj --spacing 0.025 --support 0.05 --step 0.0125 --iso 0.5
         --kernel isotropic|anisotropic --cov_radius 0.1 --smooth_lambda 0.9]

--render writes one picture per frame (render.SequenceRenderer) from each chunk's outputs while they are still on the
device; the camera is fitted to the first chunk.  --mesh writes one surface mesh per frame (mesh.SequenceMesher) in the
same way.
"""
import argparse
import os

import numpy as np
import torch

from . import mesh, ops, render

# Default chunk: this many low-resolution points per chunk (T = CHUNK_POINTS // N frames, 1 <= T <= MAX_CHUNK), from
# tools/rollout_chunks.py on MI355X (profiles/rollout_chunks.txt, DESIGN.md "Sequence upsampling").
CHUNK_POINTS = 262144
MAX_CHUNK = 64


def default_chunk(n_points):
    """Frames per chunk for clouds of `n_points` low-resolution points."""
    return max(1, min(MAX_CHUNK, CHUNK_POINTS // max(1, int(n_points))))


class SequenceUpsampler:
    """Upsample the frames of ONE sequence in order, in chunks of `chunk` frames (None: `default_chunk`).

    `push(features (T,N,C), positions (T,N,3))` -> list of T tensors (1, M_t, 3): for an `SRNet`, what T successive
    reference `forward_with_context` calls return (hard masking with the running mask average over the frames pushed
    so far); for a `NoMaskSRNet`, its `forward_frames` positions (1, N*r, 3).  The tensors of a chunk are views of one
    packed buffer; each chunk costs one host read (its offsets).  `reset()` starts a new sequence."""

    def __init__(self, net, chunk=None):
        if chunk is not None and int(chunk) < 1:
            raise ValueError("chunk must be >= 1")
        self.net = net
        self.chunk = None if chunk is None else int(chunk)
        self.masked = hasattr(net, "filter_block")
        self.reset()

    def reset(self):
        self.frames = 0             # frames pushed since the last reset: the next frame's index in the sequence
        self.state = None           # (2, N) int32 running-average state (ops.context_state)

    def push(self, features, positions):
        if features.dim() != 3 or positions.dim() != 3 or positions.shape[2] != 3:
            raise ValueError("features must be (T,N,C) and positions (T,N,3)")
        if features.shape[:2] != positions.shape[:2]:
            raise ValueError(f"features {tuple(features.shape)} and positions {tuple(positions.shape)} disagree")
        T, N = positions.shape[:2]
        chunk = self.chunk or default_chunk(N)
        outs = []
        with torch.no_grad():
            for s in range(0, T, chunk):
                f = features[s:s + chunk].contiguous()
                p = positions[s:s + chunk].float().contiguous()
                outs += self._chunk(f, p) if self.masked else self._chunk_nomask(f, p)
        return outs

    def _chunk(self, f, p):
        T, N = p.shape[:2]
        if self.state is None:
            self.state = ops.context_state(N, p.device)
        elif self.state.shape[1] != N or self.state.device != p.device:
            raise ValueError(f"a sequence keeps its point count and device: {self.state.shape[1]} points on "
                             f"{self.state.device}, got {N} on {p.device} (reset() starts a new sequence)")
        edge, mask = self.net.body(f, None)
        pts, offsets = ops.context_expand(p, edge.float().reshape(T, -1, 3).contiguous(),
                                          mask.float().reshape(T, N).contiguous(), self.state, self.frames)
        self.frames += T
        o = offsets.tolist()
        return [pts[o[t]:o[t + 1]].unsqueeze(0) for t in range(T)]

    def _chunk_nomask(self, f, p):
        self.frames += p.shape[0]
        return [out for out, _ in self.net.forward_frames(list(f.split(1)), list(p.split(1)))]


def upsample_sequence(net, features, positions, chunk=None):
    """One-shot form of `SequenceUpsampler(net, chunk).push(features, positions)`."""
    return SequenceUpsampler(net, chunk).push(features, positions)


# ----------------------------------------------------------------------------------------------------------- CLI
def normalize_point_cloud(pcd_pos):
    """train_fluid/demo.ipynb cell 2: subtract the centroid, scale h = 1."""
    centroid = np.mean(pcd_pos, axis=0, keepdims=True)
    h = np.float32(1.0)
    return (pcd_pos - centroid) / h, centroid, h


def load_frames(pattern, indices, in_feats):
    """Frames `pattern.format(i=i)` (.npz with 'pos' and, for in_feats = 6, 'vel') -> (features (T,N,C) fp32,
    positions (T,N,3) fp32, centroids, scales), as the demo notebook builds its per-frame inputs."""
    feats, poss, cents, hs = [], [], [], []
    for i in indices:
        data = np.load(pattern.format(i=i))
        pos, centroid, h = normalize_point_cloud(np.asarray(data["pos"], dtype=np.float32))
        feat = pos if in_feats == 3 else np.concatenate([pos, np.asarray(data["vel"], np.float32) * 0.025], axis=1)
        feats.append(feat)
        poss.append(pos)
        cents.append(centroid)
        hs.append(h)
    return torch.from_numpy(np.stack(feats)), torch.from_numpy(np.stack(poss)), cents, hs


def load_generator(checkpoint, in_feats, device):
    """`SRNet(in_feats, 128)` with the reference checkpoint's 'sr_net' weights, in eval mode on `device`."""
    from .srnet import SRNet
    ckpt = torch.load(checkpoint, map_location="cpu", weights_only=True)
    net = SRNet(in_feats, 128)
    net.load_state_dict(ckpt["sr_net"])
    return net.to(device).eval()


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tpgan_amd.rollout",
                                 description="Upsample a sequence of frames with a trained TPU-GAN generator.")
    ap.add_argument("--checkpoint", required=True, help="reference checkpoint (.ckpt) holding 'sr_net'")
    ap.add_argument("--frames", required=True, help="frame files, '{i}' = frame index, e.g. 'dir/data_{i}.npz'")
    ap.add_argument("--count", type=int, required=True, help="frames 0 .. count-1")
    ap.add_argument("--in-feats", type=int, default=3, choices=(3, 6), help="3: positions; 6: positions + velocities")
    ap.add_argument("--chunk", type=int, default=None, help="frames per network call (default: by point count)")
    ap.add_argument("--out", required=True, help="output directory for pcd_{i}.npy")
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--render", default=None, metavar="PNGDIR", help="also write pcd_{i:04d}.png pictures there")
    render.add_render_options(ap)
    ap.add_argument("--mesh", default=None, metavar="MESHDIR", help="also write pcd_{i:04d}.ply surface meshes there")
    mesh.add_mesh_options(ap)
    a = ap.parse_args(argv)
    if "{i}" not in a.frames:
        ap.error("--frames must contain '{i}'")
    render.check_render_options(ap, a)
    dev = torch.device(a.device)
    net = load_generator(a.checkpoint, a.in_feats, dev)
    os.makedirs(a.out, exist_ok=True)
    pictures = render.renderer_from(a, a.render, dev) if a.render else None
    meshes = mesh.mesher_from(a, a.mesh, dev) if a.mesh else None
    up = SequenceUpsampler(net, a.chunk)
    step = a.chunk
    i = 0
    while i < a.count:
        if step is None:            # the first frame's point count picks the default chunk
            step = default_chunk(np.load(a.frames.format(i=0))["pos"].shape[0])
        idx = range(i, min(i + step, a.count))
        feats, poss, cents, hs = load_frames(a.frames, idx, a.in_feats)
        outs = up.push(feats.to(dev), poss.to(dev))
        if pictures is not None or meshes is not None:     # the frames' own coordinates, as the .npy files below hold them
            own = [out[0] * float(hs[j - i]) + torch.from_numpy(cents[j - i]).to(dev) for j, out in zip(idx, outs)]
            if pictures is not None:
                pictures.push(own, i)
            if meshes is not None:
                meshes.push(own, i)
        for j, out in zip(idx, outs):
            pcd = out[0].cpu().numpy()
            pcd *= hs[j - i]
            pcd += cents[j - i]
            np.save(os.path.join(a.out, f"pcd_{j}.npy"), pcd)
        i = idx.stop
    print(f"wrote {a.count} frames to {a.out}")


if __name__ == "__main__":
    main()

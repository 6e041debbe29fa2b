"""Training clips from simulation sequences kept on the device (train_fluid/tempo_dataset.py on the GPU).

The reference feeds its step from two host workers: per clip three `np.load`, a KD-tree over the scene, a query for the
4096 / 9216 nearest particles, a numba FPS and a pinned upload of 13 arrays.  A fluid training set is a few GB and fits
in HBM many times over, so here every frame is loaded ONCE (`FluidSequences`) and a batch is four launches whatever its
size (`ClipSampler`): ops.patch_select, ops.clip_gather_high, the dataset-side FPS on the centre frame's patch,
ops.clip_gather_low -- plus the draw of the jitter noise.  `prefetch` prepares batch n+1 on a side stream while the
step consumes batch n.
"""
import os

import numpy as np
import torch

from . import ops

MIN_PATCH = 4096          # train_utils.py:113-116: the patch size of a scene that has no more than `sample_num` particles


class FluidSequences:
    """`case{c}/{prefix}_{s}.npz` (arrays `pos`, `vel`, (N,3)) for c in [case_to_start, case_to_start + case_num) and
    s in [0, case_steps), loaded once: positions / velocities of all frames back to back on `device`, with the frames'
    offsets and centroids (float64 mean rounded to fp32 once: normalize_point_cloud, train_utils.py:214-221).

    `len()` and `clip(idx)` are SiamData's (tempo_dataset.py:40-41,59-63), quirk included: the case is
    idx // case_steps, the first step idx % (case_steps - 2)."""

    def __init__(self, root, case_num, case_steps, case_prefix="data", case_to_start=1, device="cuda"):
        if case_num < 1 or case_steps < 3:
            raise ValueError("need at least one case of at least 3 steps")
        self.root, self.case_num, self.case_steps = root, int(case_num), int(case_steps)
        self.case_prefix, self.case_to_start = case_prefix, int(case_to_start)
        self.device = torch.device(device)
        pos, vel, cen = [], [], []
        self.count = np.zeros(self.case_num, np.int64)                       # particles per case
        self.frame_first = np.zeros((self.case_num, self.case_steps), np.int64)
        total = 0
        for c in range(self.case_num):
            for s in range(self.case_steps):
                path = os.path.join(root, self.key(c, s))
                with np.load(path) as f:
                    p, v = f["pos"].astype(np.float32), f["vel"].astype(np.float32)
                if p.ndim != 2 or p.shape[1] != 3 or v.shape != p.shape:
                    raise ValueError(f"{path}: pos and vel must be (N,3) arrays of one shape, got {p.shape} / {v.shape}")
                if s == 0:
                    self.count[c] = p.shape[0]
                elif p.shape[0] != self.count[c]:
                    raise ValueError(f"{path}: {p.shape[0]} particles, but the case's first frame has {self.count[c]}: "
                                     "the frames of a case are indexed with one patch and must hold the same particles")
                self.frame_first[c, s] = total
                total += p.shape[0]
                pos.append(p)
                vel.append(v)
                cen.append(p.astype(np.float64).mean(0).astype(np.float32))
        if total >= 2 ** 31:
            raise ValueError(f"{total} points: frame offsets must fit int32")
        self.pos = torch.from_numpy(np.concatenate(pos)).to(self.device)
        self.vel = torch.from_numpy(np.concatenate(vel)).to(self.device)
        self.centroids = torch.from_numpy(np.stack(cen)).to(self.device)     # row c * case_steps + s

    def key(self, case, step):
        """File of frame `step` of the case-th loaded case (0-based)."""
        return f"case{case + self.case_to_start}/{self.case_prefix}_{step}.npz"

    def __len__(self):
        return self.case_num * (self.case_steps - 2)

    def clip(self, idx):
        """Clip index -> (case, first step), both 0-based; the clip is steps first .. first + 2, centre first + 1."""
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        return idx // self.case_steps, idx % (self.case_steps - 2)

    def keys(self, idx):
        case, step = self.clip(idx)
        return tuple(self.key(case, step + t) for t in range(3))


class ClipSampler:
    """Batches of training clips in the reference's 13-tuple (tempo_dataset.py:102-105, batched by `my_collate`):
    (highres_pos_left, highres_pos, highres_pos_right, highres_vel_*, lowres_pos_*, lowres_vel_*, h) with (B,K,3) high-
    and (B,K/8,3) low-resolution tensors on the sequences' device and h = ones (B,) on the host.

    Patch size per clip: `sample_num` if the scene has more particles, else 4096 (train_utils.py:113-116); a batch holds one
    patch size (my_collate, tempo_dataset.py:108-112: the clips of size `sample_num`, or, if at most one is left, those of
    size 4096).  All randomness -- clip indices, seed points, FPS starts, the jitter's seed -- comes from ONE host
    torch.Generator; the jitter noise itself is drawn on the device from that seed."""

    def __init__(self, sequences, batch_size, sample_num, jitter=0.003, frames=3, generator=None):
        if frames != 3:
            raise NotImplementedError("the reference's clips have 3 frames")
        self.seq, self.batch_size, self.sample_num = sequences, int(batch_size), int(sample_num)
        self.jitter, self.frames = float(jitter), 3
        self.generator = generator if generator is not None else torch.Generator().manual_seed(0)
        self.device = sequences.device
        self._noise_gen = torch.Generator(device=self.device)

    def _draw(self, high):
        return int(torch.randint(int(high), (1,), generator=self.generator))

    def patch_size(self, case):
        n = int(self.seq.count[case])
        k = self.sample_num if n > self.sample_num else MIN_PATCH
        if n < k:
            raise ValueError(f"{self.seq.key(case, 0)}: a scene of {n} particles cannot give a patch of {k} "
                             f"(sample_num = {self.sample_num}; scenes with no more particles than that need >= {MIN_PATCH})")
        return k

    def sample(self, indices=None, seed_idx=None, initial_idx=None, patch_idx=None):
        """One batch.  indices: clip indices (default: batch_size draws); seed_idx: the seed particle per clip (default:
        drawn); initial_idx: the FPS' first pick per clip, a position in the patch (default: drawn).  Given values replace
        the draws, clip for clip, before the collate rule drops any.  patch_idx (B,K) int32 on the device: patch lists that
        replace the selection itself (a comparison with another implementation's patch ORDER; no clip may be dropped)."""
        seq = self.seq
        if indices is None:
            indices = torch.randint(len(seq), (self.batch_size,), generator=self.generator).tolist()
        clips = [seq.clip(int(i)) for i in indices]
        sizes = [self.patch_size(c) for c, _ in clips]
        seeds = [self._draw(seq.count[c]) for c, _ in clips] if seed_idx is None else [int(s) for s in seed_idx]
        starts = [self._draw(k) for k in sizes] if initial_idx is None else [int(s) for s in initial_idx]
        noise_seed = self._draw(2 ** 62) if self.jitter != 0.0 else None
        if len(seeds) != len(clips) or len(starts) != len(clips):
            raise ValueError("seed_idx and initial_idx need one entry per clip")
        keep = [i for i, k in enumerate(sizes) if k == self.sample_num]
        if len(keep) <= 1:
            keep = [i for i, k in enumerate(sizes) if k == MIN_PATCH]
        if not keep:
            raise ValueError("no clip of the batch has a usable patch size")
        K = sizes[keep[0]]
        M = K // 8
        T, B = self.frames, len(keep)
        case = np.array([clips[i][0] for i in keep])
        step = np.array([clips[i][1] for i in keep])
        frame_first = np.stack([seq.frame_first[case, step + t] for t in range(T)])             # (T,B)
        count = seq.count[case]
        centre = T // 2
        if patch_idx is None:
            patch = ops.patch_select(seq.pos, frame_first[centre], count, [seeds[i] for i in keep], K)
        else:
            if tuple(patch_idx.shape) != (len(clips), K) or B != len(clips):
                raise ValueError(f"patch_idx must be ({len(clips)}, {K}) and every clip must be kept")
            patch = patch_idx
        high_pos, high_vel = ops.clip_gather_high(seq.pos, seq.vel, frame_first, count, seq.centroids,
                                                  case * seq.case_steps + step + centre, patch)
        start = torch.tensor([starts[i] for i in keep], dtype=torch.int32).to(self.device, non_blocking=True)
        fps_idx = ops.backend_for(high_pos).fps(high_pos[centre], M, start, False)
        noise = None
        if noise_seed is not None:
            self._noise_gen.manual_seed(noise_seed)
            noise = torch.randn((T, B, M, 3), dtype=torch.float32, device=self.device, generator=self._noise_gen)
        low_pos, low_vel = ops.clip_gather_low(high_pos, fps_idx, noise, self.jitter, seq.vel, frame_first, count)
        self.last = {"patch_idx": patch, "fps_idx": fps_idx, "indices": [int(indices[i]) for i in keep]}
        return (*high_pos.unbind(0), *high_vel.unbind(0), *low_pos.unbind(0), *low_vel.unbind(0),
                torch.ones(B, dtype=torch.float32))

    def __iter__(self):
        while True:
            yield self.sample()


class prefetch:
    """Iterator over `sampler`'s batches that prepares batch n+1 on `stream` while batch n is consumed (two batches in
    flight).  The hand-off is per batch: an event recorded on the side stream after the batch's last launch, waited for
    by the consumer's current stream, and `record_stream` on every tensor so that the allocator does not hand the memory
    out again before the consumer's work on it has run; nothing synchronises the device.  The batches are those of
    `sampler.sample()` called in a loop, bit for bit: the host generator is consumed in the same order.

    `resume_state`: the sampler generator's state from which the NEXT batch this iterator yields is (was) drawn -- what a
    checkpoint stores, since the generator itself is already one batch ahead.  On a device without streams (CPU tensors
    under a registered checker backend) the batches are produced one ahead in the same way, without a stream."""

    def __init__(self, sampler, stream=None):
        self.sampler = sampler
        self.cuda = sampler.device.type == "cuda"
        self.stream = stream if stream is not None or not self.cuda else torch.cuda.Stream(sampler.device)
        if self.cuda:
            self.stream.wait_stream(torch.cuda.current_stream(sampler.device))   # the sequences' upload
        self._next = self._produce()

    def _produce(self):
        state = self.sampler.generator.get_state()
        if not self.cuda:
            return state, self.sampler.sample(), None
        with torch.cuda.stream(self.stream):
            batch = self.sampler.sample()
            done = torch.cuda.Event()
            done.record(self.stream)
        return state, batch, done

    @property
    def resume_state(self):
        return self._next[0]

    def __iter__(self):
        return self

    def __next__(self):
        _, batch, done = self._next
        self._next = self._produce()
        if self.cuda:
            cur = torch.cuda.current_stream(self.sampler.device)
            cur.wait_event(done)
            for t in batch:
                if t.is_cuda:
                    t.record_stream(cur)
        return batch

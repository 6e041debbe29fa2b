"""Training clips from simulation sequences kept on the device (train_fluid/tempo_dataset.py on the GPU).

The reference feeds its step from two host workers: per clip three `np.load`, a KD-tree over the scene, a query for the
4096 / 9216 nearest particles, a numba FPS and a pinned upload of 13 arrays.  A fluid training set is a few GB and fits
in HBM many times over, so here every frame is loaded ONCE (`FluidSequences`) and a batch is four launches whatever its
size (`ClipSampler`): ops.patch_select, ops.clip_gather_high, the dataset-side FPS on the centre frame's patch,
ops.clip_gather_low -- plus the draw of the jitter noise.  `prefetch` prepares batch n+1 on a side stream while the
step consumes batch n.

The action upsampler's clips (train_action/msr_dataset.py) come the same way from depth videos whose frames are ragged:
`ActionSequences` and `ActionClipSampler` (ops.frame_subset, ops.action_gather, one FPS over all frames,
ops.clip_gather_low), under the same `prefetch`.
"""
import os
import re

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


# ---------------------------------------------------------------------------------------------------------------------
# Action clips from depth videos (train_action/msr_dataset.py on the GPU)
_ACTION_FILE = re.compile(r"^a(\d+)_s(\d+)_e(\d+)_sdepth\.npz$")


class ActionSequences:
    """Depth videos `a{label}_s{subject}_e{..}_sdepth.npz` under `root` (key `point_clouds`: an object array of (n_i,3)
    frames, every frame with its own point count), loaded once: all frames cast to fp32 and stored back to back on
    `device`, with per-frame `first` / `count` (host int64) and per-video `video_first` (index of its first frame).

    The split, the labels, `num_classes` and `index_map` are MSRAction3D's (msr_dataset.py:26-52): train = subject <= 5,
    test = subject > 5, label = the file's action number - 1, one clip per start frame t in
    range(0, nframes - step_between_clips * (frames_per_clip - 1), step_between_clips).  DEVIATION: the files are read
    in SORTED name order (the reference's `os.listdir` order is the file system's), so a video's index does not depend on
    the machine.  Other files in the directory are ignored."""

    def __init__(self, root, train=True, frames_per_clip=3, step_between_clips=1, device="cuda"):
        if frames_per_clip < 1 or step_between_clips < 1:
            raise ValueError("frames_per_clip and step_between_clips must be positive")
        self.root, self.train = root, bool(train)
        self.frames_per_clip, self.step_between_clips = int(frames_per_clip), int(step_between_clips)
        self.device = torch.device(device)
        self.names, self.labels, self.index_map = [], [], []
        frames, counts, video_first = [], [], []
        for name in sorted(os.listdir(root)):
            m = _ACTION_FILE.match(name)
            if m is None or (int(m.group(2)) <= 5) != self.train:
                continue
            with np.load(os.path.join(root, name), allow_pickle=True) as f:
                video = f["point_clouds"]
            index = len(self.names)
            self.names.append(name)
            self.labels.append(int(m.group(1)) - 1)
            video_first.append(len(frames))
            for i, p in enumerate(video):
                p = np.asarray(p)
                if p.ndim != 2 or p.shape[1] != 3:
                    raise ValueError(f"{os.path.join(root, name)}: frame {i} must be an (n,3) array, got {p.shape}")
                if p.shape[0] == 0:
                    raise ValueError(f"{os.path.join(root, name)}: frame {i} is empty: a clip cannot sample from it")
                frames.append(p.astype(np.float32))
                counts.append(p.shape[0])
            span = self.step_between_clips * (self.frames_per_clip - 1)
            for t in range(0, len(video) - span, self.step_between_clips):
                self.index_map.append((index, t))
        if not self.names:
            raise ValueError(f"{root}: no {'train' if self.train else 'test'} video (a*_s*_e*_sdepth.npz)")
        self.count = np.array(counts, np.int64)
        self.first = np.concatenate([[0], np.cumsum(self.count)[:-1]]).astype(np.int64)
        self.video_first = np.array(video_first, np.int64)
        total = int(self.count.sum())
        if total >= 2 ** 31:
            raise ValueError(f"{total} points: frame offsets must fit int32")
        self.points = torch.from_numpy(np.concatenate(frames)).to(self.device)
        self.num_classes = max(self.labels) + 1

    def __len__(self):
        return len(self.index_map)

    def clip(self, idx):
        """Clip index -> (video, first frame); the clip is frames t, t + step, ... of that video."""
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        return self.index_map[idx]

    def frame_rows(self, idx):
        """Rows of the clip's frames in `first` / `count`."""
        video, t = self.clip(idx)
        return self.video_first[video] + t + self.step_between_clips * np.arange(self.frames_per_clip)


class ActionClipSampler:
    """Batches of action clips in the reference's layout (msr_dataset.py:98,133-135, default collate): a flat tuple of
    T high-resolution (B,K,3) and T low-resolution (B,K/16,3) tensors on the sequences' device and `label` (B,) int64 on
    the host; for test sequences additionally the T per-frame centres (B,3) before the label and the video index (B,)
    int64 on the host after it.

    Per frame the high-resolution cloud is a uniformly random ordered subset of `num_points` points (a frame with no
    more points than that is repeated and padded with a random residue), y negated, scaled per clip (train) and divided
    by 300, centred on the middle frame's mean (train) or its own (test); every frame gets its own FPS down to K / 16.
    A batch is four launches whatever its size: ops.frame_subset, ops.action_gather, ONE FPS over all T * B clouds,
    ops.clip_gather_low.  All randomness -- clip indices, one 64-bit subset seed per frame, the scales ~ U(0.9, 1.1) in
    float64 per clip (train only), one FPS start per frame -- comes from ONE host torch.Generator, in that order.

    return_lowres=False (the reference's flag of that name, msr_dataset.py:92,128): no FPS and no low-resolution gather,
    and the T low-resolution tensors are left out of the tuple.  The FPS starts are then NOT drawn, as in the reference,
    whose FPS draws its own start: the draws of a batch are clip indices, subset seeds, scales (train), in that order.
    The high-resolution tensors of a batch are those of return_lowres=True from the same generator state, bit for bit;
    the state after the batch differs (one draw less), so later batches do."""

    def __init__(self, sequences, batch_size, num_points=2048, generator=None, return_lowres=True):
        if num_points < 16 or num_points % 16:
            raise ValueError("num_points must be a positive multiple of 16 (the low resolution is num_points / 16)")
        self.seq, self.batch_size, self.num_points = sequences, int(batch_size), int(num_points)
        self.frames = sequences.frames_per_clip
        self.generator = generator if generator is not None else torch.Generator().manual_seed(0)
        self.device = sequences.device
        self.return_lowres = bool(return_lowres)

    def sample(self, indices=None, subset_idx=None, scales=None, initial_idx=None):
        """One batch.  indices: clip indices (default: batch_size draws); scales: (B,3) float64 per clip (train only;
        default: drawn); initial_idx: (T,B) the FPS' first pick per frame, a position in the subset (default: drawn).
        Given values replace the draws (the generator advances as if they had been drawn).  subset_idx (T,B,K) int32 on the device: frame-local point lists that replace
        the selection itself (a comparison with another implementation's subsets)."""
        seq, K, T, g = self.seq, self.num_points, self.frames, self.generator
        if indices is None:
            indices = torch.randint(len(seq), (self.batch_size,), generator=g).tolist()
        indices = [int(i) for i in indices]
        B = len(indices)
        rows = np.stack([seq.frame_rows(i) for i in indices], 1)                                 # (T,B)
        frame_first, count = seq.first[rows], seq.count[rows]
        halves = torch.randint(2 ** 32, (T * B, 2), generator=g).numpy().astype(np.uint64)
        if seq.train:
            drawn = 0.9 + 0.2 * torch.rand((B, 3), dtype=torch.float64, generator=g).numpy()
            scales = drawn if scales is None else np.asarray(scales, np.float64).reshape(B, 3)
        elif scales is not None:
            raise ValueError("the test split has no scales")
        if initial_idx is not None and not self.return_lowres:
            raise ValueError("return_lowres=False runs no FPS: there is no first pick to give")
        if self.return_lowres:
            starts = torch.randint(K, (T, B), generator=g)
            if initial_idx is not None:
                starts = torch.as_tensor(np.asarray(initial_idx)).reshape(T, B)
        if subset_idx is None:
            subset = ops.frame_subset(count.reshape(-1), (halves[:, 1] << np.uint64(32)) | halves[:, 0], K,
                                      device=self.device).view(T, B, K)
        else:
            if tuple(subset_idx.shape) != (T, B, K):
                raise ValueError(f"subset_idx must be ({T}, {B}, {K})")
            subset = subset_idx
        high, centres = ops.action_gather(seq.points, frame_first, count, subset, scales,
                                          "train" if seq.train else "test")
        label = torch.tensor([seq.labels[seq.clip(i)[0]] for i in indices], dtype=torch.int64)
        video = torch.tensor([seq.clip(i)[0] for i in indices], dtype=torch.int64)
        if not self.return_lowres:
            self.last = {"subset_idx": subset, "indices": indices, "scales": scales}
            if seq.train:
                return (*high.unbind(0), label)
            return (*high.unbind(0), *centres.unbind(0), label, video)
        start = starts.to(torch.int32).reshape(T * B).to(self.device, non_blocking=True)
        fps_idx = ops.backend_for(high).fps(high.view(T * B, K, 3), K // 16, start, False)
        low, _ = ops.clip_gather_low(high.view(1, T * B, K, 3), fps_idx)
        low = low.view(T, B, K // 16, 3)
        self.last = {"subset_idx": subset, "fps_idx": fps_idx.view(T, B, K // 16), "indices": indices, "scales": scales}
        if seq.train:
            return (*high.unbind(0), *low.unbind(0), label)
        return (*high.unbind(0), *low.unbind(0), *centres.unbind(0), label, video)

    def __iter__(self):
        while True:
            yield self.sample()


# ---------------------------------------------------------------------------------------------------------------------
# Held-out clips for the trainers' test pass (train.run): drawn ONCE from a generator of their own, only the chosen
# frames go to the device, and nothing of numpy's, torch's or the device's global RNG is touched.
TEST_PATCH_MAX = 9216          # train_utils.py:106-111, the rule of sample_num=None: the test data loader's
TEST_PATCH_SCENE = 10000


def held_out_fluid_clips(root, case_num, case_steps, n, generator, device, use_vel=False, jitter=0.003, case_prefix="data",
                         case_to_start=1):
    """`n` test clips as the reference's test loader makes them (tempo_dataset.py:118, SiamData with sample_num=None),
    centre frame only -- the test pass reads nothing else: a list of dicts with `gt` (K,3), `input` (K/8,3) and
    `feature` (1,K/8,3), or (1,K/8,6) = position and 0.025 x velocity under `use_vel`.  K = 9216 if the scene has more
    than 10000 particles, else (count // 1024) * 1024; the low resolution is the dataset-side FPS plus `jitter` x noise
    from a device generator of this function's own.  Clip indices, seed particles, FPS starts and noise seeds come from
    `generator`, clip by clip in that order."""
    device = torch.device(device)
    if case_num < 1 or case_steps < 3:
        raise ValueError("need at least one case of at least 3 steps")
    noise_gen = torch.Generator(device=device)
    clips = []
    for idx in torch.randint(case_num * (case_steps - 2), (int(n),), generator=generator).tolist():
        case, step = idx // case_steps, idx % (case_steps - 2)                 # SiamData's rule, quirk included
        path = os.path.join(root, f"case{case + case_to_start}/{case_prefix}_{step + 1}.npz")
        with np.load(path) as f:
            p, v = f["pos"].astype(np.float32), f["vel"].astype(np.float32)
        if p.ndim != 2 or p.shape[1] != 3 or v.shape != p.shape:
            raise ValueError(f"{path}: pos and vel must be (N,3) arrays of one shape, got {p.shape} / {v.shape}")
        count = p.shape[0]
        K = TEST_PATCH_MAX if count > TEST_PATCH_SCENE else count // 1024 * 1024
        if K == 0:
            raise ValueError(f"{path}: a test scene needs at least 1024 particles, got {count}")
        seed, start, noise_seed = (int(torch.randint(int(high), (1,), generator=generator)) for high in (count, K, 2 ** 62))
        pos, vel = torch.from_numpy(p).to(device), torch.from_numpy(v).to(device)
        centroid = torch.from_numpy(p.astype(np.float64).mean(0).astype(np.float32)).view(1, 3).to(device)
        zero = np.zeros((1, 1), np.int64)
        patch = ops.patch_select(pos, [0], [count], [seed], K)
        high, _ = ops.clip_gather_high(pos, None, zero, [count], centroid, [0], patch)               # (1,1,K,3)
        fps_idx = ops.backend_for(high).fps(high[0], K // 8, torch.tensor([start], dtype=torch.int32).to(device), False)
        noise_gen.manual_seed(noise_seed)
        noise = torch.randn((1, 1, K // 8, 3), dtype=torch.float32, device=device, generator=noise_gen)
        low, low_vel = ops.clip_gather_low(high, fps_idx, noise, jitter, vel, zero, [count])
        feature = torch.cat([low[0], low_vel[0] * 0.025], dim=2) if use_vel else low[0]
        clips.append({"gt": high[0, 0], "input": low[0, 0], "feature": feature.contiguous()})
    return clips


def held_out_action_clips(root, n, generator, device, num_points=2048):
    """`n` clips of the test subjects under `root`, first frame only (train_msr.py:249-254): a list of dicts with `gt`
    (num_points,3) and `input` = `feature` (num_points/16,3), prepared as `ActionClipSampler` prepares the test split.
    The videos are read into HOST memory; only the chosen frames go to the device.  Clip indices, subset seeds and FPS
    starts come from `generator`, in that order."""
    device, n, K = torch.device(device), int(n), int(num_points)
    seq = ActionSequences(root, train=False, frames_per_clip=3, device="cpu")
    indices = torch.randint(len(seq), (n,), generator=generator).tolist()
    halves = torch.randint(2 ** 32, (n, 2), generator=generator).numpy().astype(np.uint64)
    starts = torch.randint(K, (n,), generator=generator)
    rows = np.array([int(seq.frame_rows(i)[0]) for i in indices])
    count = seq.count[rows]
    points = torch.cat([seq.points[f:f + c] for f, c in zip(seq.first[rows].tolist(), count.tolist())]).to(device)
    first = np.concatenate([[0], np.cumsum(count)[:-1]]).astype(np.int64)
    subset = ops.frame_subset(count, (halves[:, 1] << np.uint64(32)) | halves[:, 0], K, device=device).view(1, n, K)
    high, _ = ops.action_gather(points, first.reshape(1, n), count.reshape(1, n), subset, None, "test")
    fps_idx = ops.backend_for(high).fps(high.view(n, K, 3), K // 16, starts.to(torch.int32).to(device), False)
    low, _ = ops.clip_gather_low(high.view(1, n, K, 3), fps_idx)
    return [{"gt": high[0, j], "input": low[0, j], "feature": low[0, j:j + 1].contiguous()} for j in range(n)]


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

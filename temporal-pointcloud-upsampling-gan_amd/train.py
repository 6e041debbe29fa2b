"""Adversarial training of the fluid upsampler from sequences on disk (train_fluid/train_tempo.py).

    python -m tpgan_amd.train --train_dataset_path DATA --train_sequence_num 20 --sequence_length 200 --log_dir runs/a

Data layout: DATA/case{c}/data_{s}.npz for c = 1 .. train_sequence_num, s = 0 .. sequence_length - 1, each holding
`pos` and `vel`, (N,3), the same particles in every frame of a case.  Every frame is loaded to the device once
(data.FluidSequences); the batches come from data.ClipSampler through data.prefetch on a side stream.

The loop is the reference's: SRNet + FluidTempoDis(3) + FluidSpatialDis, Adam(lr) and 2 x Adam(0.33 lr), StepLR(10000,
0.7) x 3, the EAGER step gan_step.tempo_gan_step (the one with the reference's regimes: n_iter <= 10, closed gate,
999-padding), a checkpoint when (n_iter - 1) % ckpt_every == 0 or at the end.  Under --graph the step is
gan_step_graph.GraphedFluidStep(padded=True), captured from the first batch: steps whose frames keep every slot or pad
replay from hipGraphs, every other step (n_iter <= 10, a closed gate, a frame that compresses, a ragged batch) falls back
to that eager step with the same draws; a padded step that replays draws its replacement centres from the keyed device
rule instead of numpy's stream.  Instead of tensorboardX one JSON line per --log_every iterations
goes to stdout (under --graph with `replayed`, the replays in the window).  Checkpoints hold the reference's ten keys
plus `tpgan_amd`: the sampler's generator state and the numpy / torch RNG states, which make a resumed run repeat the
uninterrupted one bit for bit.
Under torch.distributed.run every rank samples its own clips (seed + 1000 * rank), gradients are averaged by
ddp.GradSync and rank 0 writes the checkpoints.

The test pass (train_tempo.py:259-297): under --samples N (or --dump_visualization = --samples 4) N clips of
--test_dataset_path / --test_sequence_num are drawn once at start-up from a generator of their own, and whenever a
checkpoint is written rank 0 upsamples them in eval mode, writes LOG/samples/{gt,input,pred}_iter:{n_iter}_{j}.png
(render.py instead of the reference's Open3D window) and prints one JSON line with `test_cd` and `test_points`.  The
pass touches no random stream of the training: a run with and a run without it write the same checkpoints, bit for bit.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

from . import ddp
from .data import ClipSampler, FluidSequences, held_out_fluid_clips, prefetch
from .gan_step import tempo_gan_step
from .set_abstraction import FluidSpatialDis, FluidTempoDis
from .srnet import SRNet

CKPT_KEYS = ("sr_net", "tempo_dis", "spatial_dis", "n_iter", "sr_optim", "tempo_optim", "spatial_optim", "sr_sched",
             "tempo_sched", "spatial_sched", "tpgan_amd")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tpgan_amd.train", description="Train the temporally coherent upsampler.")
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--resume", action="store_true", help="resume from --path_to_resume")
    ap.add_argument("--path_to_resume", type=str, help="checkpoint file, or a directory with latest_checkpoint.txt")
    ap.add_argument("--iters", type=int, default=80000)
    ap.add_argument("--log_dir", type=str, default="./")
    ap.add_argument("--ckpt_every", type=int, default=5000)
    ap.add_argument("--in_node_feats", type=int, default=3)
    ap.add_argument("--R", type=float, default=0.10, help="radius of the temporal discriminator's flow embedding")
    ap.add_argument("--train_dataset_path", type=str, default="../../data/train_data_0.025_fine")
    ap.add_argument("--train_sequence_num", type=int, default=20)
    ap.add_argument("--sequence_length", type=int, default=200)
    ap.add_argument("--batch_size", type=int, default=4)
    ap.add_argument("--small_batch", action="store_true")
    ap.add_argument("--w", type=float, default=0.5, help="weight of the position loss")
    ap.add_argument("--cutoff", type=float, default=0.025, help="cutoff distance of the masking loss")
    ap.add_argument("--use_vel", action="store_true")
    ap.add_argument("--freeze_D", action="store_true")
    # not in the reference
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--amp", choices=("bf16", "none"), default="bf16")
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--log_every", type=int, default=100)
    ap.add_argument("--sample_num", type=int, default=None,
                    help="patch size (default, as the reference: 9216 if batch_size <= 4 and not --small_batch, else 4096)")
    # the test pass: held-out clips upsampled and rendered at every checkpoint (the reference's --dump_visualization)
    ap.add_argument("--test_dataset_path", type=str, default="../../data/test_data_0.025_fine")
    ap.add_argument("--test_sequence_num", type=int, default=4)
    ap.add_argument("--dump_visualization", action="store_true", help="--samples 4, unless --samples is given")
    add_sample_options(ap, default=None)
    add_graph_option(ap)
    opt = ap.parse_args(argv)
    check_graph_option(ap, opt)
    check_sample_options(ap, opt)
    if opt.samples is None:
        opt.samples = 4 if opt.dump_visualization else 0
    return opt


def add_sample_options(ap, default=0):
    ap.add_argument("--samples", type=int, default=default,
                    help="held-out clips upsampled at every checkpoint: LOG/samples/{gt,input,pred}_iter:{n}_{j}.png and "
                         "one JSON line with their Chamfer distances (0: off)")
    ap.add_argument("--samples_width", type=int, default=512, help="width of the sample pictures")
    ap.add_argument("--samples_height", type=int, default=512, help="height of the sample pictures")
    ap.add_argument("--solids", default=None, metavar="PATH|SPEC",
                    help="a mesh drawn into every sample picture: an .obj / .ply file (a scene's obstacles.ply), "
                         "icosphere:N or torus:R,r,nu,nv")
    ap.add_argument("--solids_color", type=int, nargs=3, default=(150, 150, 150), metavar=("R", "G", "B"))
    ap.add_argument("--samples_style", choices=("points", "surface"), default="points",
                    help="points: a square per point; surface: the shaded fluid surface (render.render_surface)")
    ap.add_argument("--particle_radius", type=float, default=0.025,
                    help="--samples_style surface: a point's sphere radius in the clips' units")
    ap.add_argument("--translucent", action="store_true",
                    help="--samples_style surface: the fluid absorbs light by its thickness and shows what is behind it")
    ap.add_argument("--absorption", type=float, nargs=3, default=None, metavar=("R", "G", "B"),
                    help="--translucent: absorption per particle diameter (default: render.ABSORPTION)")
    ap.add_argument("--thickness_iters", type=int, default=2, metavar="K",
                    help="--translucent: blur passes over the thickness image")


def check_sample_options(ap, opt):
    """The sample pictures' argument errors, raised at parse time."""
    if opt.translucent and opt.samples_style != "surface":
        ap.error("--translucent needs --samples_style surface: it is the fluid's surface that absorbs light, not "
                 f"--samples_style {opt.samples_style}")
    if opt.thickness_iters < 0:
        ap.error("--thickness_iters must not be negative")
    if opt.absorption is not None and not all(np.isfinite(c) and c >= 0.0 for c in opt.absorption):
        ap.error("--absorption takes three finite values >= 0")
    if not (np.isfinite(opt.particle_radius) and opt.particle_radius > 0.0):
        ap.error("--particle_radius must be positive")


def sample_surface_options(opt):
    """`HeldOutPass`'s `surface`: None for --samples_style points, else `render.render_surface`'s arguments."""
    if getattr(opt, "samples_style", "points") != "surface":
        return None
    surface = dict(particle_radius=opt.particle_radius)
    if opt.translucent:
        surface.update(translucent=True, absorption=opt.absorption, thickness_iters=opt.thickness_iters)
    return surface


def add_graph_option(ap):
    ap.add_argument("--graph", action="store_true",
                    help="replay the step from hipGraphs captured on the first batch (gan_step_graph); steps outside the "
                         "captured regime fall back to the eager step")


def check_graph_option(ap, opt):
    """--graph's argument errors, raised at parse time."""
    if not opt.graph:
        return
    if getattr(opt, "use_vel", False) or opt.in_node_feats == 6:
        ap.error("--graph cannot be combined with --use_vel or --in_node_feats 6: the captured step has no velocities")
    if torch.device(opt.device).type != "cuda":
        ap.error("--graph needs a cuda --device")


def _rng_state(device, sampler_state):
    """Everything a bit-exact resume needs beyond the reference's ten keys, in types torch.load(weights_only=True) takes."""
    kind, keys, pos, has_gauss, gauss = np.random.get_state()
    st = {"sampler_generator": sampler_state, "torch_rng": torch.get_rng_state(),
          "numpy_rng": {"kind": kind, "keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos),
                        "has_gauss": int(has_gauss), "cached_gaussian": float(gauss)}}
    if device.type == "cuda":
        st["device_rng"] = torch.cuda.get_rng_state(device)
    return st


def _set_rng_state(st, device, generator):
    generator.set_state(st["sampler_generator"])
    torch.set_rng_state(st["torch_rng"])
    n = st["numpy_rng"]
    np.random.set_state((n["kind"], n["keys"].numpy().astype(np.uint32), n["pos"], n["has_gauss"], n["cached_gaussian"]))
    if device.type == "cuda" and "device_rng" in st:
        torch.cuda.set_rng_state(st["device_rng"], device)


def save_checkpoint(state, path):
    """torch.save + the newest name on top of latest_checkpoint.txt beside it (utils.py:7-30)."""
    torch.save(state, path)
    listing = os.path.join(os.path.dirname(path), "latest_checkpoint.txt")
    old = open(listing).readlines() if os.path.exists(listing) else []
    with open(listing, "w") as f:
        f.writelines([os.path.basename(path) + "\n"] + old)


def load_checkpoint(path):
    if os.path.isdir(path):
        with open(os.path.join(path, "latest_checkpoint.txt")) as f:
            path = os.path.join(path, f.readline().strip())
    return torch.load(path, map_location="cpu", weights_only=True)


class HeldOutPass:
    """The reference's test pass (train_tempo.py:259-297, train_msr.py:230-262) without a window: at every checkpoint
    the SAME held-out clips -- `clips`, a list of dicts with `gt` (K,3), `input` (M,3) and `feature`, drawn once at
    start-up -- are upsampled by `predict(sr_net, clip) -> (P,3)` in eval mode and written as
    `{gt,input,pred}_iter:{n_iter}_{j}.png` into `sample_dir` (the reference's names): coloured by depth, one camera per
    clip fitted to its ground truth, so that the three pictures of a clip and those of successive checkpoints compare;
    splats of 3 pixels, 5 for the sparse input; `solids` (a mesh, `render.render`'s) is drawn into all of them; with
    `surface` (a dict of `render.render_surface`'s arguments, `sample_surface_options`) the fluid's surface is drawn
    instead of splats.  -> {"n_iter", "test_cd": Chamfer distance of prediction against ground truth per clip
    (losses.chamfer_distance), "test_points": predicted points per clip}.

    The pass draws no random number, runs on the current stream like the step (the prefetcher's hand-off is untouched)
    and puts the generator back into the mode it found it in."""

    def __init__(self, clips, predict, sample_dir, width, height, amp_dtype=None, solids=None,
                 solids_color=(150, 150, 150), surface=None):
        from . import render
        self.surface = surface
        self.clips, self.predict, self.sample_dir, self.amp_dtype = clips, predict, sample_dir, amp_dtype
        self.solids = {} if solids is None else dict(solids=solids, solids_color=tuple(solids_color))
        self.cameras = [render.Camera.fit(c["gt"], width=width, height=height) for c in clips]
        os.makedirs(sample_dir, exist_ok=True)
        for j, (clip, cam) in enumerate(zip(clips, self.cameras)):           # what does not change is rendered once
            clip["pictures"] = {"gt": self._draw(clip["gt"], cam, 3).cpu(), "input": self._draw(clip["input"], cam, 5).cpu()}

    def _draw(self, points, cam, size):
        from . import render
        if self.surface is None:
            return render.render(points, cam, size=size, **self.solids)
        return render.render_surface(points, cam, **self.surface, **self.solids)

    def __call__(self, sr_net, n_iter):
        from . import render
        from .gan_step import _autocast
        from .losses import chamfer_distance
        was_training = sr_net.training
        sr_net.eval()
        cds, counts = [], []
        try:
            with torch.no_grad():
                for j, (clip, cam) in enumerate(zip(self.clips, self.cameras)):
                    with _autocast(self.amp_dtype, clip["gt"].device):
                        pred = self.predict(sr_net, clip).float().reshape(-1, 3).contiguous()
                    cds.append(float(chamfer_distance(pred[None], clip["gt"][None])))
                    counts.append(int(pred.shape[0]))
                    pictures = dict(clip["pictures"], pred=self._draw(pred, cam, 3).cpu())
                    for name, image in pictures.items():
                        render.write_png(os.path.join(self.sample_dir, f"{name}_iter:{n_iter}_{j}.png"), image)
        finally:
            sr_net.train(was_training)
        return {"n_iter": n_iter, "test_cd": cds, "test_points": counts}


def run(opt, nets_of, sched_of, sampler_of, step, samples_of=None, graph_step_of=None):
    """The training loop both trainers share (--seed, --device, --lr, --amp, --freeze_D, --iters, --resume,
    --path_to_resume, --log_dir, --log_every, --ckpt_every and --samples of `opt`); what differs comes as callables:
    nets_of(dev) -> (sr_net, tempo_dis, spatial_dis) on the device; sched_of(optimiser) -> its scheduler;
    sampler_of(dev, seed) -> the clip sampler, its `generator` seeded with `seed`;
    step((sr_net, tempo_dis, spatial_dis), (sr_optim, tempo_optim, spatial_optim), batch, n_iter, freeze_D, sync,
    amp_dtype) -> the losses of one adversarial step; the last three go to the step function under those names;
    samples_of(dev, generator, n) -> (the n held-out clips of `HeldOutPass`, drawn from `generator`, and its `predict`):
    called once, on rank 0, and only under --samples n > 0; the pass then runs whenever a checkpoint is written.
    Under --graph, graph_step_of((nets), (optims), batch, sync, amp_dtype, draw_seed) -> (a gan_step_graph stepper
    captured from that batch, clouds_of(batch) -> its (low, high) lists) replaces `step`: it is called once, on the first
    batch and after any --resume load.  The optimisers are then capturable and their learning rate is a device tensor,
    which the schedulers fill in place: the captured Adam follows the schedule."""
    rank, world, local = ddp.init_from_env(backend=os.environ.get("TPGAN_DDP_BACKEND"))
    dev = torch.device(opt.device)
    if dev.type == "cuda":
        torch.backends.cudnn.enabled = False         # hipBLASLt GEMMs + native BatchNorm, as bench.py and the tests
        if dev.index is None:
            dev = torch.device("cuda", local)
        torch.cuda.set_device(dev)
    np.random.seed(opt.seed + 1000 * rank)
    torch.manual_seed(opt.seed)                      # same initial weights on every rank; broadcast below anyway

    nets = nets_of(dev)
    graph = bool(getattr(opt, "graph", False))
    if graph and graph_step_of is None:
        raise ValueError("--graph needs the trainer's graph_step_of")
    adam = (lambda p, lr: torch.optim.Adam(p, lr=torch.tensor(lr, device=dev), capturable=True)) if graph else \
        (lambda p, lr: torch.optim.Adam(p, lr=lr))
    optims = tuple(adam(net.parameters(), lr) for net, lr in zip(nets, (opt.lr, 0.33 * opt.lr, 0.33 * opt.lr)))
    scheds = [sched_of(o) for o in optims]
    sync = ddp.GradSync()
    sync.broadcast_state(*nets)
    torch.manual_seed(opt.seed + 1000 * rank)
    sampler = sampler_of(dev, opt.seed + 1000 * rank)

    held = {"sr_net": nets[0], "tempo_dis": nets[1], "spatial_dis": nets[2],
            "sr_optim": optims[0], "tempo_optim": optims[1], "spatial_optim": optims[2],
            "sr_sched": scheds[0], "tempo_sched": scheds[1], "spatial_sched": scheds[2]}

    n_iter = 0
    if opt.resume:
        ckpt = load_checkpoint(opt.path_to_resume)
        for k, x in held.items():
            x.load_state_dict(ckpt[k])
        n_iter = int(ckpt["n_iter"])
        if "tpgan_amd" in ckpt and world == 1:       # (the file holds rank 0's streams; other ranks keep their seeds)
            _set_rng_state(ckpt["tpgan_amd"], dev, sampler.generator)
        if graph:                                    # (the file's learning rates were mapped to the host)
            for o in optims:
                for g in o.param_groups:
                    g["lr"] = torch.as_tensor(g["lr"], dtype=torch.float32).to(dev)

    ckpt_dir = os.path.join(opt.log_dir, "model_ckpt")
    if rank == 0:
        os.makedirs(ckpt_dir, exist_ok=True)
    amp_dtype = torch.bfloat16 if opt.amp == "bf16" else None
    held_out = None
    if rank == 0 and getattr(opt, "samples", 0) > 0:
        if samples_of is None:
            raise ValueError("--samples needs the trainer's samples_of")
        # before the prefetcher starts: its side stream waits for what the current stream has been given so far
        clips, predict = samples_of(dev, torch.Generator().manual_seed(opt.seed), opt.samples)
        solids = None
        if getattr(opt, "solids", None):
            from . import mesh
            solids = mesh.load_spec(opt.solids)
        held_out = HeldOutPass(clips, predict, os.path.join(opt.log_dir, "samples"), opt.samples_width,
                               opt.samples_height, amp_dtype, solids, getattr(opt, "solids_color", (150, 150, 150)),
                               sample_surface_options(opt))
    batches = prefetch(sampler)
    for net in nets:
        net.train()
    window_start, window_iters, window_replays = time.time(), 0, 0
    stepper = None
    while n_iter < opt.iters:
        data = next(batches)
        n_iter += 1
        if graph:
            if stepper is None:
                stepper, clouds_of = graph_step_of(nets, optims, data, sync, amp_dtype, opt.seed + 1000 * rank)
            losses = stepper(*clouds_of(data), n_iter, freeze_D=opt.freeze_D)
        else:
            losses = step(nets, optims, data, n_iter, opt.freeze_D, sync, amp_dtype)
        for s in scheds:
            s.step()
        window_iters += 1
        if rank == 0 and (n_iter % opt.log_every == 0 or n_iter >= opt.iters):
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            now = time.time()
            replayed = {"replayed": stepper.replays - window_replays} if graph else {}
            print(json.dumps({"n_iter": n_iter, "steps_per_s": window_iters / max(now - window_start, 1e-9), **replayed,
                              **{k: float(v) for k, v in losses.items()}}), flush=True)
            window_start, window_iters, window_replays = now, 0, stepper.replays if graph else 0
        if rank == 0 and ((n_iter - 1) % opt.ckpt_every == 0 or n_iter >= opt.iters):
            if held_out is not None:
                print(json.dumps(held_out(nets[0], n_iter)), flush=True)
            state = {k: x.state_dict() for k, x in held.items()}
            state.update(n_iter=n_iter, tpgan_amd=_rng_state(dev, batches.resume_state))
            save_checkpoint({k: state[k] for k in CKPT_KEYS}, os.path.join(ckpt_dir, f"tpugan_checkpoint{n_iter}.ckpt"))
    ddp.barrier()
    return 0


def main(argv=None):
    opt = parse_args(argv)

    def nets_of(dev):
        return SRNet(opt.in_node_feats, 128).to(dev), FluidTempoDis(3).to(dev), FluidSpatialDis().to(dev)

    def sampler_of(dev, seed):
        sequences = FluidSequences(opt.train_dataset_path, opt.train_sequence_num, opt.sequence_length, device=dev)
        sample_num = opt.sample_num or (9216 if opt.batch_size <= 4 and not opt.small_batch else 4096)
        return ClipSampler(sequences, opt.batch_size, sample_num, generator=torch.Generator().manual_seed(seed))

    def step(nets, optims, data, n_iter, freeze_D, sync, amp_dtype):
        sr_net, tempo_dis, spatial_dis = nets
        high_pos, high_vel, low_pos, low_vel = list(data[0:3]), list(data[3:6]), list(data[6:9]), list(data[9:12])
        return tempo_gan_step(sr_net, spatial_dis, tempo_dis, low_pos, low_vel, high_pos, high_vel, 1., opt, n_iter,
                              *optims, freeze_D=freeze_D, sync=sync, amp_dtype=amp_dtype)

    def graph_step_of(nets, optims, data, sync, amp_dtype, draw_seed):
        from .gan_step_graph import GraphedFluidStep
        sr_net, tempo_dis, spatial_dis = nets

        def clouds_of(data):
            return list(data[6:9]), list(data[0:3])
        low, high = clouds_of(data)
        return GraphedFluidStep(sr_net, spatial_dis, tempo_dis, optims, opt, low, high, 1., amp_dtype, sync, padded=True,
                                draw_seed=draw_seed), clouds_of

    def samples_of(dev, generator, n):
        clips = held_out_fluid_clips(opt.test_dataset_path, opt.test_sequence_num, opt.sequence_length, n, generator, dev,
                                     use_vel=opt.use_vel and opt.in_node_feats == 6)
        return clips, lambda sr_net, clip: sr_net(clip["feature"], clip["input"][None], hard_masking=True)[2]

    return run(opt, nets_of, lambda o: torch.optim.lr_scheduler.StepLR(o, 10000, gamma=0.7), sampler_of, step, samples_of,
               graph_step_of)


if __name__ == "__main__":
    sys.exit(main())

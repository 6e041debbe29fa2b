"""Adversarial training of the action upsampler from depth videos on disk (train_action/train_msr.py).

    python -m tpgan_amd.train_action --data_dir DATA/MSR-Action3D --log_dir runs/msr

Data layout: DATA/MSR-Action3D/a{label}_s{subject}_e{..}_sdepth.npz, each holding `point_clouds`, an object array of
(n_i,3) depth frames; subjects 1-5 train.  Every frame is loaded to the device once (data.ActionSequences); the batches
come from data.ActionClipSampler through data.prefetch on a side stream.

The loop is the reference's: NoMaskSRNet(in, emb, upsample_ratio=16) + ActionTempoDis(3) + ActionSpatialDis, Adam(lr) and
2 x Adam(0.33 lr), StepLR(iters // 10, 0.72) x 3, the eager step gan_step.tempo_gan_step_no_mask, a checkpoint when
(n_iter - 1) % ckpt_every == 0 or at the end.  Logging, the checkpoint's keys (the reference's ten plus `tpgan_amd`),
the bit-exact --resume and the multi-process rules are train.py's, whose helpers are imported.  --dump_visualization is
accepted and ignored.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

from . import ddp
from .data import ActionClipSampler, ActionSequences, prefetch
from .gan_step import tempo_gan_step_no_mask
from .set_abstraction import ActionSpatialDis, ActionTempoDis
from .srnet import NoMaskSRNet
from .train import CKPT_KEYS, _rng_state, _set_rng_state, load_checkpoint, save_checkpoint  # noqa: F401


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tpgan_amd.train_action", description="Train the action upsampler.")
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--resume", action="store_true", help="resume from --path_to_resume")
    ap.add_argument("--path_to_resume", type=str, default="", help="checkpoint file, or a directory with latest_checkpoint.txt")
    ap.add_argument("--iters", type=int, default=80000)
    ap.add_argument("--log_dir", type=str, default="./")
    ap.add_argument("--ckpt_every", type=int, default=5000)
    ap.add_argument("--batch_size", type=int, default=4)
    ap.add_argument("--data_dir", type=str, default="../../data/MSR-Action3D")
    ap.add_argument("--in_node_feats", type=int, default=3)
    ap.add_argument("--node_embedding", type=int, default=128)
    ap.add_argument("--R", type=float, default=2.0, help="radius of the temporal discriminator's flow embedding")
    ap.add_argument("--w", type=float, default=2.0, help="weight of the temporal loss")
    ap.add_argument("--freeze_D", action="store_true")
    ap.add_argument("--dump_visualization", action="store_true", help="accepted for the reference's command lines; ignored")
    # not in the reference
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--amp", choices=("bf16", "none"), default="bf16")
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--log_every", type=int, default=100)
    ap.add_argument("--num_points", type=int, default=2048, help="points per high-resolution frame (low: 1/16 of it)")
    return ap.parse_args(argv)


def main(argv=None):
    opt = parse_args(argv)
    rank, world, local = ddp.init_from_env(backend=os.environ.get("TPGAN_DDP_BACKEND"))
    dev = torch.device(opt.device)
    if dev.type == "cuda":
        torch.backends.cudnn.enabled = False         # hipBLASLt GEMMs + native BatchNorm, as bench.py and the tests
        if dev.index is None:
            dev = torch.device("cuda", local)
        torch.cuda.set_device(dev)
    np.random.seed(opt.seed + 1000 * rank)
    torch.manual_seed(opt.seed)                      # same initial weights on every rank; broadcast below anyway

    sr_net = NoMaskSRNet(opt.in_node_feats, opt.node_embedding, upsample_ratio=16).to(dev)
    tempo_dis = ActionTempoDis(3).to(dev)
    spatial_dis = ActionSpatialDis().to(dev)
    sr_optim = torch.optim.Adam(sr_net.parameters(), lr=opt.lr)
    tempo_optim = torch.optim.Adam(tempo_dis.parameters(), lr=0.33 * opt.lr)
    spatial_optim = torch.optim.Adam(spatial_dis.parameters(), lr=0.33 * opt.lr)
    scheds = [torch.optim.lr_scheduler.StepLR(o, max(opt.iters // 10, 1), gamma=0.72)
              for o in (sr_optim, tempo_optim, spatial_optim)]
    sync = ddp.GradSync()
    sync.broadcast_state(sr_net, tempo_dis, spatial_dis)
    torch.manual_seed(opt.seed + 1000 * rank)

    sequences = ActionSequences(opt.data_dir, train=True, frames_per_clip=3, device=dev)
    generator = torch.Generator().manual_seed(opt.seed + 1000 * rank)
    sampler = ActionClipSampler(sequences, opt.batch_size, opt.num_points, generator=generator)

    n_iter = 0
    if opt.resume:
        ckpt = load_checkpoint(opt.path_to_resume)
        sr_net.load_state_dict(ckpt["sr_net"])
        tempo_dis.load_state_dict(ckpt["tempo_dis"])
        spatial_dis.load_state_dict(ckpt["spatial_dis"])
        sr_optim.load_state_dict(ckpt["sr_optim"])
        tempo_optim.load_state_dict(ckpt["tempo_optim"])
        spatial_optim.load_state_dict(ckpt["spatial_optim"])
        for s, k in zip(scheds, ("sr_sched", "tempo_sched", "spatial_sched")):
            s.load_state_dict(ckpt[k])
        n_iter = int(ckpt["n_iter"])
        if "tpgan_amd" in ckpt and world == 1:       # (the file holds rank 0's streams; other ranks keep their seeds)
            _set_rng_state(ckpt["tpgan_amd"], dev, generator)

    ckpt_dir = os.path.join(opt.log_dir, "model_ckpt")
    if rank == 0:
        os.makedirs(ckpt_dir, exist_ok=True)
    amp_dtype = torch.bfloat16 if opt.amp == "bf16" else None
    batches = prefetch(sampler)
    sr_net.train(), tempo_dis.train(), spatial_dis.train()
    window_start, window_iters = time.time(), 0
    while n_iter < opt.iters:
        data = next(batches)
        high_pos, low_pos = list(data[0:3]), list(data[3:6])
        n_iter += 1
        losses = tempo_gan_step_no_mask(sr_net, spatial_dis, tempo_dis, low_pos, high_pos, opt, n_iter, sr_optim,
                                        tempo_optim, spatial_optim, freeze_D=opt.freeze_D, sync=sync, amp_dtype=amp_dtype)
        for s in scheds:
            s.step()
        window_iters += 1
        if rank == 0 and (n_iter % opt.log_every == 0 or n_iter >= opt.iters):
            if dev.type == "cuda":
                torch.cuda.synchronize(dev)
            now = time.time()
            print(json.dumps({"n_iter": n_iter, "steps_per_s": window_iters / max(now - window_start, 1e-9),
                              **{k: float(v) for k, v in losses.items()}}), flush=True)
            window_start, window_iters = now, 0
        if rank == 0 and ((n_iter - 1) % opt.ckpt_every == 0 or n_iter >= opt.iters):
            save_checkpoint({
                "sr_net": sr_net.state_dict(), "tempo_dis": tempo_dis.state_dict(),
                "spatial_dis": spatial_dis.state_dict(), "n_iter": n_iter,
                "sr_optim": sr_optim.state_dict(), "tempo_optim": tempo_optim.state_dict(),
                "spatial_optim": spatial_optim.state_dict(),
                "sr_sched": scheds[0].state_dict(), "tempo_sched": scheds[1].state_dict(),
                "spatial_sched": scheds[2].state_dict(),
                "tpgan_amd": _rng_state(dev, batches.resume_state),
            }, os.path.join(ckpt_dir, f"tpugan_checkpoint{n_iter}.ckpt"))
    ddp.barrier()
    return 0


if __name__ == "__main__":
    sys.exit(main())

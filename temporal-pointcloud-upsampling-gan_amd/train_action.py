"""Adversarial training of the action upsampler from depth videos on disk (train_action/train_msr.py).

    python -m tpgan_amd.train_action --data_dir DATA/MSR-Action3D --log_dir runs/msr

Data layout: DATA/MSR-Action3D/a{label}_s{subject}_e{..}_sdepth.npz, each holding `point_clouds`, an object array of
(n_i,3) depth frames; subjects 1-5 train.  Every frame is loaded to the device once (data.ActionSequences); the batches
come from data.ActionClipSampler through data.prefetch on a side stream.

The loop is the reference's: NoMaskSRNet(in, emb, upsample_ratio=16) + ActionTempoDis(3) + ActionSpatialDis, Adam(lr) and
2 x Adam(0.33 lr), StepLR(iters // 10, 0.72) x 3, the eager step gan_step.tempo_gan_step_no_mask (under --graph its
replay from hipGraphs, gan_step_graph.GraphedActionStep, captured from the first batch), a checkpoint when
(n_iter - 1) % ckpt_every == 0 or at the end.  The loop itself is train.run: optimisers, logging, the checkpoint's keys
(the reference's ten plus `tpgan_amd`), the bit-exact --resume and the multi-process rules are written there once; this
file says only what the action trainer's flags, networks, scheduler, sampler, step and held-out clips are.
--dump_visualization is accepted and ignored; the test pass it stood for (train_msr.py:230-262) is --samples N: the first
frames of N clips of the test subjects under --data_dir, upsampled and rendered whenever a checkpoint is written.
"""
import argparse
import sys

import torch

from .data import ActionClipSampler, ActionSequences, held_out_action_clips
from .gan_step import tempo_gan_step_no_mask
from .set_abstraction import ActionSpatialDis, ActionTempoDis
from .srnet import NoMaskSRNet
from .train import add_graph_option, add_sample_options, check_graph_option, check_sample_options, run


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
    ap.add_argument("--dump_visualization", action="store_true",
                    help="accepted for the reference's command lines; ignored (the test pass is --samples N)")
    # not in the reference
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--amp", choices=("bf16", "none"), default="bf16")
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--log_every", type=int, default=100)
    ap.add_argument("--num_points", type=int, default=2048, help="points per high-resolution frame (low: 1/16 of it)")
    add_sample_options(ap)
    add_graph_option(ap)
    opt = ap.parse_args(argv)
    check_graph_option(ap, opt)
    check_sample_options(ap, opt)
    return opt


def main(argv=None):
    opt = parse_args(argv)

    def nets_of(dev):
        return (NoMaskSRNet(opt.in_node_feats, opt.node_embedding, upsample_ratio=16).to(dev), ActionTempoDis(3).to(dev),
                ActionSpatialDis().to(dev))

    def sampler_of(dev, seed):
        sequences = ActionSequences(opt.data_dir, train=True, frames_per_clip=3, device=dev)
        return ActionClipSampler(sequences, opt.batch_size, opt.num_points, generator=torch.Generator().manual_seed(seed))

    def step(nets, optims, data, n_iter, freeze_D, sync, amp_dtype):
        sr_net, tempo_dis, spatial_dis = nets
        high_pos, low_pos = list(data[0:3]), list(data[3:6])
        return tempo_gan_step_no_mask(sr_net, spatial_dis, tempo_dis, low_pos, high_pos, opt, n_iter, *optims,
                                      freeze_D=freeze_D, sync=sync, amp_dtype=amp_dtype)

    def graph_step_of(nets, optims, data, sync, amp_dtype, draw_seed):
        from .gan_step_graph import GraphedActionStep
        sr_net, tempo_dis, spatial_dis = nets

        def clouds_of(data):
            return list(data[3:6]), list(data[0:3])
        low, high = clouds_of(data)
        return GraphedActionStep(sr_net, spatial_dis, tempo_dis, optims, opt, low, high, 1., amp_dtype, sync), clouds_of

    def samples_of(dev, generator, n):
        clips = held_out_action_clips(opt.data_dir, n, generator, dev, opt.num_points)
        return clips, lambda sr_net, clip: sr_net(clip["feature"], clip["feature"])[0]

    return run(opt, nets_of, lambda o: torch.optim.lr_scheduler.StepLR(o, max(opt.iters // 10, 1), gamma=0.72), sampler_of,
               step, samples_of, graph_step_of)


if __name__ == "__main__":
    sys.exit(main())

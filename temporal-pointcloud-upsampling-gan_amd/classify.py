"""Action classification on the frozen temporal features of a trained discriminator (train_action/eval_tempo_feat.py).

    python -m tpgan_amd.classify --data_path DATA/MSR-Action3D --pretrained_ckpt runs/msr/model_ckpt --log_dir runs/cls

What it measures: how much a trained ActionTempoDis has learned about motion.  Its two set-abstraction levels and its
flow module are copied into set_abstraction.ActionCls and frozen (`init_feature_extractor`, the reference's quirks
included); the pooling level and a 512 -> 256 -> 64 -> 20 head are trained for 20-way action recognition on the train
subjects, and every --eval_every epochs the test subjects' clips vote per video.

The loop is the reference's: clips of 3 frames without the low resolution (ActionClipSampler(return_lowres=False)), an
epoch = one torch.randperm of the train clips in batches of --batch_size with the last partial batch dropped,
NLLLoss(log_softmax(model(clip, 2.0))), Adam(lr, weight_decay = --decay_rate) over the trainable parameters only (any
other --optimizer: SGD(0.01, momentum 0.9)), StepLR(20, 0.7).  Evaluation runs the test clips in order (last partial
batch kept) with model.eval() under no_grad -- the forward that takes the one-launch eval tails (ops.gather_mlp_max)
under --amp bf16 -- writes every clip's probabilities into ONE device buffer and transfers it once; `video_vote` then
sums them per video like eval_tempo_feat.test.  Output: one JSON line per epoch; on evaluation epochs the checkpoint
LOG/checkpoints/model_epoch:{e}.pth with the reference's four keys.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from .data import ActionClipSampler, ActionSequences
from .set_abstraction import ActionCls, ActionTempoDis
from .train import load_checkpoint

CKPT_KEYS = ("epoch", "total_acc", "model_state_dict", "optimizer_state_dict")
FLOW_RADIUS = 2.0            # eval_tempo_feat.model_wrapper


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m tpgan_amd.classify",
                                 description="Train and test an action classifier on frozen temporal features.")
    ap.add_argument("--data_path", type=str, required=True, help="directory of a*_s*_e*_sdepth.npz depth videos")
    ap.add_argument("--pretrained_ckpt", type=str, required=True,
                    help="checkpoint of tpgan_amd.train_action (file, or directory with latest_checkpoint.txt)")
    ap.add_argument("--epoch", type=int, default=201)
    ap.add_argument("--learning_rate", type=float, default=3e-4)
    ap.add_argument("--optimizer", type=str, default="Adam")
    ap.add_argument("--log_dir", type=str, default="./")
    ap.add_argument("--decay_rate", type=float, default=1e-4)
    # not in the reference
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--amp", choices=("bf16", "none"), default="bf16")
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--num_points", type=int, default=2048)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--test_batch_size", type=int, default=128)
    ap.add_argument("--eval_every", type=int, default=10)
    ap.add_argument("--npoints", type=int, nargs=2, default=(512, 256), help=argparse.SUPPRESS)   # centres per level (tests)
    return ap.parse_args(argv)


def video_vote(prob, label, video):
    """Video-level accuracy from clip probabilities, as eval_tempo_feat.test computes it: prob (n,C) float32, label (n,)
    and video (n,) integers, all in clip order -> (accuracy over the videos, accuracy per class as a list of C floats).
    A video's score is the float32 sum of its clips' probabilities, added one clip after the other in clip order; its
    prediction is the first arg-max, its label the label of its first clip.  A class without a video has accuracy nan
    (the reference divides by zero there)."""
    prob = np.ascontiguousarray(np.asarray(prob, dtype=np.float32))
    label, video = np.asarray(label).astype(np.int64), np.asarray(video).astype(np.int64)
    ids, first, slot = np.unique(video, return_index=True, return_inverse=True)
    score = np.zeros((len(ids), prob.shape[1]), np.float32)
    np.add.at(score, slot, prob)                       # unbuffered: one float32 addition per clip, in clip order
    pred, truth = score.argmax(1), label[first]
    hit = pred == truth
    count = np.bincount(truth, minlength=prob.shape[1])[:prob.shape[1]]
    right = np.bincount(truth[hit], minlength=prob.shape[1])[:prob.shape[1]]
    class_acc = [float(r) / float(c) if c else float("nan") for r, c in zip(right, count)]
    return float(np.mean(hit)), class_acc


def _autocast(dev, amp_dtype):
    return torch.autocast(device_type=dev.type, dtype=amp_dtype or torch.bfloat16, enabled=amp_dtype is not None)


def clip_probabilities(model, sampler, batch_size, amp_dtype=None):
    """Class probabilities of every clip of the sampler's sequences in order: (n,C) float32 on the device (written
    batch by batch, no host synchronisation), labels and video indices (n,) int64 on the host."""
    seq, T, dev = sampler.seq, sampler.frames, sampler.device
    model.eval()
    prob, labels, videos = None, [], []
    with torch.no_grad():
        for lo in range(0, len(seq), batch_size):
            hi = min(lo + batch_size, len(seq))
            batch = sampler.sample(indices=range(lo, hi))
            with _autocast(dev, amp_dtype):
                logits = model(list(batch[:T]), FLOW_RADIUS)
            p = torch.exp(F.log_softmax(logits.float(), dim=-1))
            if prob is None:
                prob = torch.empty((len(seq), p.shape[1]), dtype=torch.float32, device=dev)
            prob[lo:hi] = p
            labels.append(batch[-2])
            videos.append(batch[-1])
    return prob, torch.cat(labels), torch.cat(videos)


def train_epoch(model, sampler, optimizer, amp_dtype=None):
    """One pass over the train clips: a random permutation from the sampler's generator in batches, the last partial one
    dropped -> mean loss (None without a full batch)."""
    seq, T, dev, B = sampler.seq, sampler.frames, sampler.device, sampler.batch_size
    model.train()
    order = torch.randperm(len(seq), generator=sampler.generator).tolist()
    total, nb = torch.zeros((), device=dev), 0
    for lo in range(0, len(order) - B + 1, B):
        batch = sampler.sample(indices=order[lo:lo + B])
        optimizer.zero_grad()
        with _autocast(dev, amp_dtype):
            logits = model(list(batch[:T]), FLOW_RADIUS)
        loss = F.nll_loss(F.log_softmax(logits.float(), dim=-1), batch[-1].to(dev))
        loss.backward()
        optimizer.step()
        total += loss.detach()
        nb += 1
    return float(total) / nb if nb else None


def main(argv=None):
    opt = parse_args(argv)
    dev = torch.device(opt.device)
    if dev.type == "cuda":
        torch.backends.cudnn.enabled = False         # hipBLASLt GEMMs + native BatchNorm, as train.run
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        torch.cuda.set_device(dev)
    amp_dtype = torch.bfloat16 if (opt.amp == "bf16" and dev.type == "cuda") else None
    np.random.seed(opt.seed)
    torch.manual_seed(opt.seed)

    gen = torch.Generator().manual_seed(opt.seed)
    train_set = ActionSequences(opt.data_path, train=True, frames_per_clip=3, device=dev)
    test_set = ActionSequences(opt.data_path, train=False, frames_per_clip=3, device=dev)
    train_sampler = ActionClipSampler(train_set, opt.batch_size, opt.num_points, generator=gen, return_lowres=False)
    test_sampler = ActionClipSampler(test_set, opt.test_batch_size, opt.num_points,
                                     generator=torch.Generator().manual_seed(opt.seed + 1), return_lowres=False)

    model = ActionCls(3, npoints=tuple(opt.npoints))
    trained = ActionTempoDis(3, sn=True)
    trained.load_state_dict(load_checkpoint(opt.pretrained_ckpt)["tempo_dis"])
    model.init_feature_extractor(trained)
    del trained
    model = model.to(dev)
    params = [p for p in model.parameters() if p.requires_grad]
    if opt.optimizer == "Adam":
        optimizer = torch.optim.Adam(params, lr=opt.learning_rate, betas=(0.9, 0.999), eps=1e-8, weight_decay=opt.decay_rate)
    else:
        optimizer = torch.optim.SGD(params, lr=0.01, momentum=0.9)
    scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=20, gamma=0.7)

    ckpt_dir = os.path.join(opt.log_dir, "checkpoints")
    os.makedirs(ckpt_dir, exist_ok=True)
    for epoch in range(opt.epoch):
        line = {"epoch": epoch, "lr": scheduler.get_last_lr()[0],
                "train_loss": train_epoch(model, train_sampler, optimizer, amp_dtype)}
        scheduler.step()
        if epoch % opt.eval_every == 0:
            prob, label, video = clip_probabilities(model, test_sampler, opt.test_batch_size, amp_dtype)
            total_acc, class_acc = video_vote(prob.cpu().numpy(), label.numpy(), video.numpy())
            path = os.path.join(ckpt_dir, f"model_epoch:{epoch}.pth")
            torch.save({"epoch": epoch, "total_acc": total_acc, "model_state_dict": model.state_dict(),
                        "optimizer_state_dict": optimizer.state_dict()}, path)
            line.update(video_acc=total_acc, class_acc=class_acc, checkpoint=path)
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())

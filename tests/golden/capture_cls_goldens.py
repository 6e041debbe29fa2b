"""Generates tests/golden/action_cls.npz by running the REFERENCE's own ActionCls and evaluation vote in the build container.

    TPGAN_REFERENCE=<checkout of the reference> python tests/golden/capture_cls_goldens.py

Same recipe as capture_goldens.py: the reference checkout (read-only, imported unmodified; never copied, never shipped)
on `sys.path` in this container only, `pointnet2_ops` / `pytorch3d` / `frnn` / `chamferdist` resolved to this repo's
import-compatible modules whose CPU tensors are served by the oracle, the inert import shims of
tests/golden/_import_shims, `.cuda()` patched to identity.  Never run by a test; the tests read the committed .npz.

What is stored (arrays only; weights by seed + per-tensor checksums):
  clip                    action_clip(2, 1024, 16, 3, seed=41), the three high-resolution frames
  cls/w, cls/w_after      checksums of discriminator.ActionCls(3) built under torch.manual_seed(51), before / after
  cls/train, cls/eval     its logits in .train() (dropout draws under torch.manual_seed(151)) and then in .eval()
  src/w                   checksums of ActionTempoDis(3, sn=True) built under torch.manual_seed(52)
  init/w, init/w_after    checksums of the classifier after init_feature_extractor(source), before / after the passes
  init/names, init/requires_grad   the parameter names and their requires_grad flags after it
  init/train, init/eval   logits as above (dropout draws under torch.manual_seed(152))
  vote/*                  train_action/eval_tempo_feat.test() run on a stub model that returns recorded logits for 40
                          clips of 6 videos in batches of 16: the logits, labels and video indices per clip, the
                          returned total_acc and the class accuracies it logged
"""
import ast
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFERENCE = os.environ.get("TPGAN_REFERENCE") or (sys.argv[1] if len(sys.argv) > 1 else None)
if not REFERENCE:
    raise SystemExit("set TPGAN_REFERENCE (or pass the path) to a checkout of the reference")

sys.dont_write_bytecode = True
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "_import_shims"))

import tpgan_amd  # noqa: E402

tpgan_amd.install_compat()
sys.path.insert(2, REFERENCE)
sys.path.insert(3, os.path.join(REFERENCE, "train_action"))
from oracle import torch_backend  # noqa: E402

torch_backend.install()
torch.Tensor.cuda = lambda self, *a, **k: self
torch.nn.Module.cuda = lambda self, *a, **k: self
warnings.simplefilter("ignore")

import discriminator as ref_dis  # noqa: E402

from tpgan_amd.synthetic import action_clip  # noqa: E402

torch.set_num_threads(8)


def checksums(module):
    out = {}
    for k, v in module.state_dict().items():
        v = v.detach().double()
        out[k] = np.array([v.sum().item(), v.abs().sum().item(), float(v.numel())])
    return out


def pack(prefix, d):
    return {f"{prefix}/{k}": v for k, v in d.items()}


def n(t):
    return t.detach().cpu().numpy()


def passes(m, clip, prefix, seed, out):
    m.train()
    torch.manual_seed(seed)
    out[f"{prefix}/train"] = n(m(list(clip), 2.0))
    out.update(pack(f"{prefix}/w_after", checksums(m)))
    m.eval()
    out[f"{prefix}/eval"] = n(m(list(clip), 2.0))


def capture_vote(out):
    try:
        import eval_tempo_feat as ref_eval
    except Exception as e:                                   # noqa: BLE001
        print(f"eval_tempo_feat does not import here ({e!r}): no vote/* arrays")
        return
    g = torch.Generator().manual_seed(61)
    n_clips, n_classes = 40, 5
    video = torch.sort(torch.randint(0, 6, (n_clips,), generator=g))[0]          # clips of a video are consecutive
    video_label = torch.tensor([0, 1, 2, 3, 4, 2])
    label = video_label[video]
    logits = torch.randn(n_clips, n_classes, generator=g)
    logits[torch.arange(n_clips), label] += 0.8                                   # right more often than not, not always

    class Loader(list):
        pass

    loader = Loader()
    loader.dataset = type("D", (), {"num_classes": n_classes})()
    for lo in range(0, n_clips, 16):
        hi = min(lo + 16, n_clips)
        loader.append(([torch.zeros(hi - lo, 4, 3)] * 3, None, None, label[lo:hi], video[lo:hi]))

    class Stub(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.at = 0

        def forward(self, pos_lst, cutoff):
            b = pos_lst[0].shape[0]
            self.at += b
            return logits[self.at - b:self.at]

    lines = []
    total = ref_eval.test(Stub(), loader, lines.append)
    logged = [s for s in lines if "Class Acc@1" in s][0].split("Class Acc@1", 1)[1].strip()
    class_acc = ast.literal_eval(logged.replace("np.float64(", "("))             # numpy 2 prints its scalars' type
    out["vote/logits"], out["vote/label"], out["vote/video"] = n(logits), n(label), n(video)
    out["vote/total_acc"] = np.float64(total)
    out["vote/class_acc"] = np.array(class_acc, np.float64)
    print(f"vote: total_acc {float(total):.4f}, class_acc {class_acc}")


def main():
    out = {}
    _, clip = action_clip(2, 1024, 16, 3, seed=41)
    out["clip"] = np.stack([n(h) for h in clip])
    torch.manual_seed(51)
    m = ref_dis.ActionCls(3)
    out.update(pack("cls/w", checksums(m)))
    passes(m, clip, "cls", 151, out)
    torch.manual_seed(52)
    src = ref_dis.ActionTempoDis(3, sn=True)
    out.update(pack("src/w", checksums(src)))
    m.init_feature_extractor(src)
    out.update(pack("init/w", checksums(m)))
    names = [k for k, _ in m.named_parameters()]
    out["init/names"] = np.array(names)
    out["init/requires_grad"] = np.array([p.requires_grad for _, p in m.named_parameters()])
    passes(m, clip, "init", 152, out)
    capture_vote(out)
    path = os.path.join(HERE, "action_cls.npz")
    np.savez_compressed(path, **{k: np.asarray(v) for k, v in out.items()})
    print(f"action_cls: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()

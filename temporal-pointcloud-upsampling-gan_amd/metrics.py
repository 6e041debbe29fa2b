"""Evaluation metrics between predicted and true clouds: Chamfer distance, earth mover's distance, Gaussian MMD.

The reference scores its results with `position_loss` / `cycle_consistency` (train_fluid/analysis_helper.py:175-262),
`position_loss` of the action model (train_action/analysis_helper.py:60-68) and trains with
`earth_mover_distance_loss` (loss.py:294-316).  Those rest on two third-party packages: the `emd` auction-matching
extension and `geomloss.SamplesLoss`.  Here they are a thin layer over three ops: `ops.chamfer_nn`,
`ops.emd_match` (csrc/emd.hip) and `ops.gaussian_row_sums` (csrc/gauss_sum.hip).  Same signatures as the reference's
functions; GPU tensors in, GPU tensors out; CPU tensors raise like every other op (no CPU fallback).

Two deliberate differences: no function modifies its inputs (the reference shifts `pos_pred`, `pos_gt` and
`masked_pos` in place), and a batch is normalised cloud by cloud, each by its own furthest distance `h` (the
reference divides `masked_pos` by the first cloud's; the two agree at B = 1, the only size it is called with).
"""
import torch

from . import ops
from .losses import chamfer_distance


# The auction's phases run at eps * scaling^k, k = phases .. 0.  The metrics pass final epsilons between 1e-4 and 0.05
# on clouds normalised to about unit size; a phase whose epsilon is far above the costs themselves only shuffles the
# assignment (in the numpy statement of the rule, eps = 0.03 on a normalised 1024-point fluid pair: 100 rounds with no
# scaling phase, 4084 with three), so the schedule starts at the largest eps * scaling^k that is not above START_EPS.
START_EPS = 0.01


def schedule_phases(eps, scaling=ops.EMD_DEFAULTS["scaling"], most=ops.EMD_DEFAULTS["phases"]):
    k = 0
    while k < most and float(eps) * float(scaling) ** (k + 1) <= START_EPS:
        k += 1
    return k


# The reference passes `iters` = 3000 (2000 in the loss) to its extension for clouds of 1024 and 2048 points.  Here
# `iters` caps the auction's ROUNDS, a cloud that needs more raises, and the rounds grow with the cloud: at the metrics'
# settings 3522 for a 4096-point action pair, 6539 at 16384 points, 6154 for a 79 872-point fluid frame
# (profiles/metrics.txt), in every measurement below n.  The functions below therefore keep the reference's figure up
# to 2048 points and scale it with the size beyond; every one of them takes `iters` to set the cap outright.
REFERENCE_POINTS = 2048


def round_cap(n, reference_iters):
    return int(reference_iters) * max(1, -(-int(n) // REFERENCE_POINTS))


class emdModule(torch.nn.Module):
    """The reference's `emdModule()(x1, x2, eps, iters) -> (dist, assignment)`: dist (B,n) squared distance of every
    point of x1 to its partner in x2, assignment (B,n) int32.  `eps` is the final epsilon of the auction (the sum of
    squared distances ends within n * eps of the optimum), `iters` the cap on the rounds per cloud: a cloud that
    needs more raises.  Unlike the reference's, n need not be a multiple of 1024.  The number of scaling phases follows
    from `eps` (`schedule_phases`)."""

    def forward(self, input1, input2, eps, iters):
        dist, assignment, _, _ = ops.emd_match(input1, input2, eps=eps, iters=iters, phases=schedule_phases(eps))
        return dist, assignment


def earth_mover_distance(x1, x2, eps=ops.EMD_DEFAULTS["eps"], iters=ops.EMD_DEFAULTS["iters"]):
    """(B,n,3), (B,n,3) -> (B,): the mean distance between matched points of each pair of clouds."""
    dist, _ = emdModule()(x1, x2, eps, iters)
    return torch.sqrt(dist).mean(dim=1)


def gaussian_mmd(x, y, blur=0.01):
    """(B,N,3), (B,M,3) -> (B,) float64, per pair of clouds

        0.5 * mean_ii' k(x_i, x_i') + 0.5 * mean_jj' k(y_j, y_j') - mean_ij k(x_i, y_j),   k = exp(-d^2 / (2 blur^2))

    with uniform weights 1/N and 1/M.  This is the project's own statement of `SamplesLoss('gaussian', blur=blur)`;
    that package is not available to compare against, so parity with it is NOT pinned by any test.  No gradient."""
    ops._need(x.dim() == 3 and y.dim() == 3 and x.shape[0] == y.shape[0], "x (B,N,3), y (B,M,3)")
    ops._need(x.shape[1] > 0 and y.shape[1] > 0, "gaussian_mmd needs non-empty clouds")
    N, M = x.shape[1], y.shape[1]
    xx = ops.gaussian_row_sums(x, x, blur).sum(dim=1) / float(N * N)
    yy = ops.gaussian_row_sums(y, y, blur).sum(dim=1) / float(M * M)
    xy = ops.gaussian_row_sums(x, y, blur).sum(dim=1) / float(N * M)
    return 0.5 * xx + 0.5 * yy - xy


def _batched(*clouds):
    ops._need(all(isinstance(c, torch.Tensor) and c.dim() == 3 and c.shape[2] == 3 for c in clouds),
              "clouds must be (B,N,3) tensors")
    ops._need(all(c.shape[0] == clouds[0].shape[0] for c in clouds), "batch mismatch")


def _joint_frame(a, b):
    """The reference's normalisation of a pair of clouds: shift both to their joint minimum corner, scale by the larger
    of the two furthest distances from it -> (corner (B,1,3), h (B,1,1))."""
    corner = torch.minimum(a.min(dim=1, keepdim=True)[0], b.min(dim=1, keepdim=True)[0])
    h1 = torch.amax(torch.sqrt(torch.sum((a - corner) ** 2, dim=-1)), dim=1)
    h2 = torch.amax(torch.sqrt(torch.sum((b - corner) ** 2, dim=-1)), dim=1)
    return corner, torch.maximum(h1, h2).view(-1, 1, 1)


def position_loss(masked_pos, pos_pred, pos_gt, iters=None):
    """train_fluid/analysis_helper.py:232-262 -> (cd / N, mean sqrt(emd), mean mmd): Chamfer distance of `pos_pred`
    against `pos_gt` per point of `pos_gt`; EMD (eps 0.03, at most `iters` rounds, default `round_cap(N, 3000)`:
    3000 up to 2048 points, a RuntimeError beyond the cap) between the two, shifted to their
    joint minimum corner and scaled by the larger furthest distance h; Gaussian MMD (blur 0.01) of `masked_pos`
    against `pos_gt` in the same frame.  pos_pred and pos_gt must have the same number of points."""
    _batched(masked_pos, pos_pred, pos_gt)
    cd = chamfer_distance(pos_pred, pos_gt) / pos_gt.shape[1]
    corner, h = _joint_frame(pos_pred, pos_gt)
    gt = (pos_gt - corner) / h
    emd = earth_mover_distance((pos_pred - corner) / h, gt, eps=0.03,
                               iters=round_cap(pos_gt.shape[1], 3000) if iters is None else iters)
    mmd = gaussian_mmd((masked_pos - corner) / h, gt, blur=0.01)
    return cd, emd.mean(), mmd.mean()


def action_position_loss(pos_pred, pos_gt, iters=None):
    """train_action/analysis_helper.py:60-68 -> (cd / N, 2 * mean sqrt(emd of the halved clouds)); eps 0.002, at most
    `iters` rounds (default `round_cap(N, 3000)`).  (The reference divides by its fixed 2048 points.)"""
    _batched(pos_pred, pos_gt)
    cd = chamfer_distance(pos_pred, pos_gt) / pos_gt.shape[1]
    emd = earth_mover_distance(pos_pred / 2.0, pos_gt / 2.0, eps=0.002,
                               iters=round_cap(pos_gt.shape[1], 3000) if iters is None else iters)
    return cd, emd.mean() * 2.0


def cycle_consistency(lowres_pos_left, lowres_pos_right, highres_advection, highres_pos_left, cutoff, sr_net,
                      use_vel=False, lowres_vel_left=None, lowres_vel_right=None, iters=None):
    """train_fluid/analysis_helper.py:175-229: upsample the left frame and advect it with the true high-resolution
    displacement (interpolated at the predicted points within 1.6 * cutoff), upsample the right frame, and compare the
    two -> (cd / N, mean sqrt(emd), mmd) as in `position_loss` (`iters` as there)."""
    def upsample(pos, vel):
        feature = torch.cat([pos, vel * 0.025], dim=2) if use_vel else pos
        return sr_net(feature, pos)[0]

    with torch.no_grad():
        left = upsample(lowres_pos_left, lowres_vel_left)
        advected = left + ops.cubic_interpolation(left, highres_advection, highres_pos_left, 1.6 * cutoff)
        right = upsample(lowres_pos_right, lowres_vel_right)
        _batched(right, advected)
        cd = chamfer_distance(right, advected) / right.shape[1]
        corner, h = _joint_frame(right, advected)
        a, b = (right - corner) / h, (advected - corner) / h
        emd = earth_mover_distance(a, b, eps=0.03, iters=round_cap(a.shape[1], 3000) if iters is None else iters)
        mmd = gaussian_mmd(a, b, blur=0.01)
    return cd, emd.mean(), mmd.mean()


def earth_mover_distance_loss(pred, target, generator=None, iters=None):
    """loss.py:294-316: (N,3), (M,3) -> the sum over a random subset of min(N, M) // 1024 * 1024 indices (the same for
    both clouds, drawn from `generator`, a CPU torch.Generator) of the distance between matched points.  The
    matching is taken without gradient on the clouds in their joint frame (eps 0.05, at most `iters` rounds, default
    `round_cap(subset size, 2000)`); the result
    is differentiable through the distances of the matched pairs."""
    ops._need(pred.dim() == 2 and target.dim() == 2 and pred.shape[1] == 3 and target.shape[1] == 3,
              "pred (N,3), target (M,3)")
    n = min(pred.shape[0], target.shape[0])
    k = n // 1024 * 1024
    ops._need(k > 0, f"earth_mover_distance_loss needs at least 1024 points in both clouds, got {n}")
    idx = torch.randperm(n, generator=generator)[:k].to(pred.device)
    p, t = pred[idx], target[idx]
    with torch.no_grad():
        corner, h = _joint_frame(pred[None], target[None])
        _, assignment = emdModule()((p[None] - corner) / h, (t[None] - corner) / h, eps=0.05,
                                    iters=round_cap(k, 2000) if iters is None else iters)
    matched = t[assignment[0].long()]
    return torch.sqrt(torch.sum((p - matched) ** 2, dim=-1)).sum()

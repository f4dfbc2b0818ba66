#!/usr/bin/env python3
"""A minimal fine-tuning loop for the correspondence extractor on the sequence it is used on: PointNet2Msg2(64) with the seeded
weights of reart_amd.synthetic.extractor_state (the reference ships no way to train corr_model.pth.tar), descriptors with
grad=True, the contrastive loss networks.loss.DescriptorInfoNCE between consecutive frames, positives from
utils.flow_utils.correspondence_targets on the ground-truth tracks (every point of frame t carried to frame t + 1 by its
part's true motion, matched to the nearest observed point within --max_dist), stepped with reart_amd.optim.Adam.  Prints the
loss and the share of used rows whose best column is the positive, per step.  Not a training recipe: BatchNorm stays in
eval mode (running statistics), no schedule, no validation split.  Without a GPU it fails."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def tracked(seq, t):
    """Frame t's points where the true motion puts them in frame t + 1 (make_sequence's per-part world transforms)."""
    import numpy as np

    W0, W1 = seq["world"](t), seq["world"](t + 1)
    pts = seq["complete"][t].astype(np.float64)
    out = np.empty_like(pts)
    for e in range(W0.shape[0]):
        m = seq["part"] == e
        M = W1[e] @ np.linalg.inv(W0[e])
        out[m] = pts[m] @ M[:3, :3].T + M[:3, 3]
    return out.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--parts", type=int, default=4)
    ap.add_argument("--pts_per_part", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--tau", type=float, default=0.07)
    ap.add_argument("--max_dist", type=float, default=0.02)
    ap.add_argument("--symmetric", action="store_true")
    ap.add_argument("--seed", type=int, default=2)
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F

    from reart_amd.networks.feature_extractor import PointNet2Msg2
    from reart_amd.networks.loss import DescriptorInfoNCE
    from reart_amd.optim import Adam
    from reart_amd.synthetic import extractor_state, make_sequence
    from reart_amd.utils.flow_utils import correspondence_targets

    if not torch.cuda.is_available():
        raise SystemExit("finetune_extractor.py needs an MI355X")
    dev = torch.device("cuda:0")
    seq = make_sequence(T=20, n_parts=args.parts, pts_per_part=args.pts_per_part, seed=args.seed, with_flow=False)
    T = args.frames
    frames = torch.from_numpy(seq["complete"][:T]).to(dev)
    pred = torch.from_numpy(np.stack([tracked(seq, t) for t in range(T - 1)])).to(dev)
    pos = correspondence_targets(pred, frames[1:], args.max_dist)
    print(f"{T - 1} pairs of {frames.shape[1]} points, {(pos >= 0).float().mean().item():.1%} of the rows have a positive")
    net = PointNet2Msg2(64)
    net.load_state_dict(extractor_state(net))
    net = net.to(dev).eval()
    opt = Adam(net.parameters(), lr=args.lr)
    loss_fn = DescriptorInfoNCE(tau=args.tau, symmetric=args.symmetric)
    xyz = frames.transpose(1, 2).contiguous()
    for step in range(args.steps):
        opt.zero_grad(set_to_none=True)
        desc = F.normalize(net(xyz, grad=True).transpose(1, 2), dim=2)          # cosine logits: autograd carries the normalisation
        loss = loss_fn(desc[:-1], desc[1:], pos)
        loss.backward()
        opt.step()
        print(f"step {step:3d}  loss {loss.item():.5f}  accuracy {loss_fn.accuracy().item():.4f}")


if __name__ == "__main__":
    main()

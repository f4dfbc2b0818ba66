#!/usr/bin/env python3
"""Golden vectors for one iteration's flow term (reference run_robot.py:194-209), produced by the reference's own
``blend_anchor_motion`` (utils/flow_utils.py:147-170) and ``flow_loss`` (networks/loss.py:10-21) under torch-CPU autograd:

    python tests/golden/make_golden_flow_term.py  ->  tests/golden/flow_term.npz

``knn_cuda.KNN`` is the brute-force stand-in of make_golden.py.  B = 3 frame pairs of N = 100 points against ragged reference
sets of 3, 17 and 130 points; every cano_idx in {0, 1, 3} with and without the robust (Huber) loss.  Stored: the inputs, and
per case gt_flow, mask, neighbour indices, loss and d loss / d pc_trans."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (stand-ins + reference on sys.path)

B, N, LENS = 3, 100, (3, 17, 130)


def inputs():
    rng = np.random.default_rng(41)
    base = rng.uniform(-0.3, 0.3, (N, 3))
    frames = [base + rng.normal(0, 0.01, (N, 3)) + 0.02 * f for f in range(B + 1)]       # four complete frames
    refs, flows = [], []
    for f, n in enumerate(LENS):
        pick = rng.integers(0, N, n)
        refs.append(base[pick] + rng.normal(0, 0.02, (n, 3)) + 0.02 * f)
        fl = rng.normal(0, 0.02, (n, 3))
        fl[::7] = rng.normal(0, 2.0, fl[::7].shape)      # large flows: Huber's linear branch
        flows.append(fl)
    pc = np.stack(frames[:B])
    pc[:, ::10, 0] += 1.0                                # far from every reference point: masked out
    f32 = lambda x: torch.from_numpy(np.asarray(x, dtype=np.float32))
    return f32(pc), f32(frames[B]), [f32(r) for r in refs], [f32(f) for f in flows]


def main():
    pc_trans, cano, refs, flows = inputs()
    knn = mg.KNN(k=3, transpose_mode=True)
    out = {"pc_trans": pc_trans, "cano": cano}
    for f in range(B):
        out[f"ref{f}"], out[f"flow{f}"] = refs[f], flows[f]
    for c in (0, 1, 3):
        for robust in (0, 1):
            pc = pc_trans.clone().requires_grad_(True)
            with torch.no_grad():
                query = torch.cat((pc[:c], cano[None], pc[c:]), dim=0)[:-1]
                bl = [mg.blend_anchor_motion(q, r, fl, knn, return_mask=True) for q, r, fl in zip(query, refs, flows)]
                idx = torch.stack([knn(r[None], q[None])[1][0] for q, r in zip(query, refs)])
            gt, mask = torch.stack([b[0] for b in bl]), torch.stack([b[1] for b in bl])
            comp = torch.cat((pc[:c], cano[None], pc[c:]), dim=0)
            loss = mg.flow_loss(gt, comp[1:] - comp[:-1], flow_mask_list=mask, robust=bool(robust))
            loss.backward()
            tag = f"c{c}_r{robust}"
            out.update({f"gt_{tag}": gt, f"mask_{tag}": mask, f"idx_{tag}": idx, f"loss_{tag}": loss.detach(), f"grad_{tag}": pc.grad})
            print(tag, "loss", float(loss), "masked in", float(mask.float().mean()))
    mg.save("flow_term", **out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/loss_terms.npz by IMPORTING the reference (read-only checkout, REART_REFERENCE) with the stand-ins of
make_golden.py: the float32 values of the reference's own structure_loss and compute_connection_loss (networks/loss.py:32-78)
with their autograd gradients.  Run once where the reference is; the .npz is committed.

    python tests/golden/make_golden_loss_terms.py

Stored: expected outputs, and the inputs of the two small synthetic cases (tests/structure_loss_ref.make_case).  The large
inputs stay in structure.npz.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (installs the stand-ins and puts the reference on sys.path)
from networks.loss import structure_loss, compute_connection_loss  # noqa: E402
from utils.graph_utils import compute_relative_trans  # noqa: E402
from utils.chamfer import ChamferDistance  # noqa: E402
from tests import structure_loss_ref as slr  # noqa: E402

# name -> (T, P, edges, kinds, seed, big) of structure_loss_ref.make_case
SYNTHETIC = {
    "synA": (5, 4, [(0, 1), (1, 2), (2, 3)], "irpp", 3, ()),
    "synB": (4, 5, [(0, 1), (2, 1), (3, 2), (3, 4), (0, 4)], "qqrrr", 4, (2,)),
}


def structure_case(trans, edges):
    tl = torch.from_numpy(np.asarray(trans, np.float32)).clone().requires_grad_(True)
    el = torch.from_numpy(np.asarray(edges, np.int64))
    axis, moment, theta, distance, rel = compute_relative_trans(tl, return_trans=True)
    loss = structure_loss(rel, axis, moment, theta, distance, el)
    loss.backward()
    th, d = theta[:, el[:, 0], el[:, 1]].detach(), distance[:, el[:, 0], el[:, 1]].detach()
    pris = d.abs().mean(dim=0) > th.abs().mean(dim=0)
    return np.float32(loss.item()), tl.grad[:, :, :3].numpy().copy(), pris.numpy()


def main():
    torch.set_num_threads(8)
    z = np.load(os.path.join(HERE, "structure.npz"))
    out = {}
    for tag, tk, ek in (("raw", "trans0", "joint_connection_raw"), ("new", "new_trans", "new_conn")):
        out[f"{tag}_loss"], out[f"{tag}_grad"], out[f"{tag}_pris"] = structure_case(z[tk], z[ek])
    for tag, (T, P, edges, kinds, seed, big) in SYNTHETIC.items():
        c = slr.make_case(T, P, edges, kinds, seed, big)
        out[f"{tag}_trans"], out[f"{tag}_pairs"] = c["trans"], c["pairs"]
        out[f"{tag}_loss"], out[f"{tag}_grad"], out[f"{tag}_pris"] = structure_case(c["trans"], c["pairs"])
        assert out[f"{tag}_pris"].any() and not out[f"{tag}_pris"].all(), tag

    # compute_connection_loss at k = 10 on the fixture's cloud, labels, tree and predicted frames
    k = 10
    cano, seg = torch.from_numpy(z["cano"]), torch.from_numpy(z["new_seg"])
    conn = torch.from_numpy(z["new_conn"])
    pred = torch.from_numpy(z["pred"]).clone().requires_grad_(True)
    cd = ChamferDistance()
    loss = compute_connection_loss(cano, seg, conn, pred, cd, k=k)
    loss.backward()
    src_all, tgt_all = [], []
    for edge in conn:                                   # the selection again, to record it and to rule ties out
        sm, tm = seg == edge[0], seg == edge[1]
        d, nn = cd(cano[sm][None], cano[tm][None], return_index=True)
        d, nn = d[0], nn[0]
        srt = torch.sort(d).values
        assert srt[k] > srt[k - 1], "tie at the k-th place"
        _, si = torch.topk(d, k=k, largest=False)
        src_all.append(torch.where(sm)[0][si].numpy())
        tgt_all.append(torch.where(tm)[0][nn[si].long()].numpy())
    src_all, tgt_all = np.stack(src_all), np.stack(tgt_all)
    rows = np.unique(np.concatenate([src_all.ravel(), tgt_all.ravel()]))
    g = pred.grad.numpy()
    rest = np.delete(g, rows, axis=1)
    assert not rest.any()
    out.update(conn_loss=np.float32(loss.item()), conn_src=src_all, conn_tgt=tgt_all, conn_rows=rows, conn_grad_rows=g[:, rows],
               conn_k=np.int64(k))
    mg.save("loss_terms", **out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generate tests/golden/scdm_long.npz by running the REAL reference's SCDM_Attention and rnn_recalibration_layer
(model/networks/attention.py, model/components/VideoEncoder.py) on the CPU at sentence lengths above 32 words.

Runs only where the reference is checked out (``--ref``: its grounding/ directory), with the shims of oracle/make_golden.py that
matter here (``.cuda()`` -> identity: RNN.py hard-codes it; ``h5py`` stub).  The reference is imported, never copied.  Stored per case
(N = 40 and N = 48, small widths): inputs, weights (``<case>.att.w.*`` / ``<case>.rec.w.*``), the attention output C and the gated
output of the recalibration layer, with the gradients of one backward each.

Usage:  python tools/make_golden_scdm_long.py --ref REFERENCE/grounding
"""
import argparse
import logging
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "scdm_long.npz")
# case -> (B, T, N, video width Dv, word width Ds, attention hidden H or None, recalibration hidden h)
CASES = {"n40": (2, 19, 40, 24, 16, 20, 8), "n48": (2, 37, 48, 32, 24, None, 12)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout's grounding/ directory")
    a = ap.parse_args()
    torch.Tensor.cuda = lambda self, *x, **k: self
    nn.Module.cuda = lambda self, *x, **k: self
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    sys.path.insert(0, a.ref)
    from model.networks.attention import SCDM_Attention
    from model.components.VideoEncoder import rnn_recalibration_layer

    torch.set_num_threads(4)
    npy = lambda t: t.detach().cpu().numpy()
    arrs = {}
    for tag, (B, T, N, Dv, Ds, H, h) in CASES.items():
        torch.manual_seed(4000 + N)
        att = SCDM_Attention(Dv, Ds, H)
        video = torch.randn(B, T, Dv, requires_grad=True)
        sent = torch.randn(B, N, Ds, requires_grad=True)
        C = att(video, sent)
        gC = torch.randn_like(C)
        C.backward(gC)
        arrs.update({f"{tag}.video": npy(video), f"{tag}.sent": npy(sent), f"{tag}.C": npy(C), f"{tag}.gC": npy(gC),
                     f"{tag}.gvideo": npy(video.grad), f"{tag}.gsent": npy(sent.grad)})
        arrs.update({f"{tag}.att.w.{k}": npy(v) for k, v in att.state_dict().items()})
        arrs.update({f"{tag}.att.gw.{k}": npy(p.grad) for k, p in att.named_parameters()})

        rec = rnn_recalibration_layer(Dv, Ds, h, 2, "sigmoid", 0.0, logging.getLogger("golden"))
        rec.train()
        rv = torch.randn(B, T, Dv, requires_grad=True)
        rw = torch.randn(B, N, Ds, requires_grad=True)
        out = rec(rv, rw)
        g = torch.randn_like(out)
        out.backward(g)
        arrs.update({f"{tag}.rec.video": npy(rv), f"{tag}.rec.word": npy(rw), f"{tag}.rec.out": npy(out), f"{tag}.rec.g": npy(g),
                     f"{tag}.rec.gvideo": npy(rv.grad), f"{tag}.rec.gword": npy(rw.grad)})
        arrs.update({f"{tag}.rec.w.{k}": npy(v) for k, v in rec.state_dict().items()})
        arrs.update({f"{tag}.rec.gw.{k}": npy(p.grad) for k, p in rec.named_parameters()})
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **arrs)
    print(f"{OUT}: {len(CASES)} cases, {len(arrs)} arrays, {os.path.getsize(OUT) / 1024:.1f} kB")


if __name__ == "__main__":
    main()

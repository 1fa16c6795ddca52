#!/usr/bin/env python3
"""Generate tests/golden/tall_head.npz by running the REAL reference's ``TALL`` + ``MLP_predictor`` and ``OnlyVideo`` + ``MLP_predictor``
(model/components/CrossModalInteraction.py, SpanPredictor.py) the way ``GMD`` calls them (SpanGroundMatchDisc.py:86: the matching logits
gate the fused feature, ``mask_logits`` with the video mask), forward and backward, fp32 on the CPU.

Runs only where the reference is checked out (``--ref``: its grounding/ directory), with the ``h5py`` stub of oracle/make_golden.py.  The
reference is imported, never copied.  One shape, [B, T, d, Hm] = [2, 32, 32, 256] -- the smallest the fused head kernels take, so the GPU
tests can hold the fused forms against the same file -- with a gate of N(0,1) x 2 and a mask that cuts the second item.  Stored: the inputs,
the cotangents of (start, end), and per CMI ('tall', 'video') the predictor's weights, both outputs and every gradient.

Usage:  python tools/make_golden_tall_head.py --ref REFERENCE/grounding
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "tall_head.npz")
B, T, D, HM = 2, 32, 32, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout's grounding/ directory")
    a = ap.parse_args()
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    sys.path.insert(0, a.ref)
    from model.components import CrossModalInteraction, SpanPredictor

    torch.manual_seed(20240923)
    video = torch.randn(B, T, D)
    sent = torch.randn(B, D)
    gate = torch.randn(B, T) * 2
    mask = torch.ones(B, T, dtype=torch.int64)
    mask[1, 23:] = 0
    ct_s, ct_e = torch.randn(B, T), torch.randn(B, T)
    out = dict(video=video.numpy(), sent=sent.numpy(), gate=gate.numpy(), mask=mask.numpy().astype(np.int32), ct_start=ct_s.numpy(),
               ct_end=ct_e.numpy())
    for kind, cls in (("tall", CrossModalInteraction.TALL), ("video", CrossModalInteraction.OnlyVideo)):
        cmi = cls(D, D)
        pred = SpanPredictor.MLP_predictor(cmi.cross_dim(), HM)
        v, s, g = (t.clone().requires_grad_(True) for t in (video, sent, gate))
        ps, pe = pred(g.unsqueeze(dim=2) * cmi(v, None, s), v_mask=mask)
        ((ps * ct_s).sum() + (pe * ct_e).sum()).backward()
        out[f"{kind}.start"], out[f"{kind}.end"] = ps.detach().numpy(), pe.detach().numpy()
        out[f"{kind}.g.video"], out[f"{kind}.g.gate"] = v.grad.numpy(), g.grad.numpy()
        if s.grad is not None:
            out[f"{kind}.g.sent"] = s.grad.numpy()
        for n, p in pred.named_parameters():
            out[f"{kind}.w.{n}"], out[f"{kind}.gw.{n}"] = p.detach().numpy(), p.grad.numpy()
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {len(out)} arrays, {os.path.getsize(OUT) / 1024:.1f} kB")


if __name__ == "__main__":
    main()

"""Float64 ground truth of the boundary head on TALL's fusion and on the clips alone, for tests/test_tall_head_cpu.py and
tests/test_tall_head_gpu.py.

``concat_form`` is the reference's own formula (CrossModalInteraction.py:49-67 / 35-36, the gate of SpanGroundMatchDisc.py:86 multiplied into the
fused feature, then ``oracle.mlp_predictor`` = SpanPredictor.py:71-85) in float64 with autograd on the CPU.  ``split_form`` restates what the
fused kernel computes -- Wv = W_a + W_d, W_c in place, cs = s (W_b + W_d)^T, z = gate (v Wv^T + (v * s) W_c^T + cs) + b1 -- also in float64:
the two must agree to rounding.  ``f32s_form`` restates the DESIGNED arithmetic of tsg_boundary_head_tall_gemm in torch: fp32 sums of the
weight blocks, the fp32 product v * s (one rounding), every operand split into bf16 hi + lo, hi hi + hi lo + lo hi accumulated (here in
float64: the kernel's fp32 accumulation is not what is being bounded), the tail in float64."""
import torch

from oracle import tsg_oracle as O

NAMES = [f"{n}_mlp_{i}.{k}" for n in ("start", "end") for i in (1, 2) for k in ("weight", "bias")]


def make_case(B, T, d, Hm, kind="tall", seed=0, gate=True, mask=True, gate_scale=2.0):
    """Seeded fp32 inputs: video [B,T,d], sent [B,d], the predictor's parameters (first Linears [Hm, 4d] for 'tall', [Hm, d] for 'video'),
    gate N(0,1) x gate_scale or None, a mask with a ragged tail per item or None, and cotangents of (start, end)."""
    g = torch.Generator().manual_seed(1000 * seed + B * T + d + Hm)
    D = 4 * d if kind == "tall" else d
    p = {}
    for n in ("start", "end"):
        p[f"{n}_mlp_1.weight"] = torch.randn(Hm, D, generator=g) / D ** 0.5
        p[f"{n}_mlp_1.bias"] = torch.randn(Hm, generator=g) * 0.1
        p[f"{n}_mlp_2.weight"] = torch.randn(1, Hm, generator=g) / Hm ** 0.5
        p[f"{n}_mlp_2.bias"] = torch.randn(1, generator=g) * 0.1
    c = dict(kind=kind, p=p, video=torch.randn(B, T, d, generator=g), sent=torch.randn(B, d, generator=g),
             gate=torch.randn(B, T, generator=g) * gate_scale if gate else None, mask=None,
             ct=(torch.randn(B, T, generator=g), torch.randn(B, T, generator=g)))
    if mask:
        n = torch.randint(max(1, T // 2), T + 1, (B,), generator=g)
        c["mask"] = (torch.arange(T)[None, :] < n[:, None]).int()
    return c


def fuse(kind, video, sent):
    if kind == "video":
        return video
    s = sent.unsqueeze(1).expand(-1, video.size(1), -1)
    return torch.cat((video, s, video * s, video + s), -1)


def concat_form(c, dtype=torch.float64):
    """-> dict(start, end, g.video, g.sent, g.gate, gw.<parameter>) of the reference's formula in ``dtype``."""
    p = {k: v.to(dtype).requires_grad_(True) for k, v in c["p"].items()}
    v = c["video"].to(dtype).requires_grad_(True)
    s = c["sent"].to(dtype).requires_grad_(True)
    g = c["gate"].to(dtype).requires_grad_(True) if c["gate"] is not None else None
    x = fuse(c["kind"], v, s)
    if g is not None:
        x = g.unsqueeze(2) * x
    ps, pe = O.mlp_predictor(x, p, c["mask"])
    ((ps * c["ct"][0].to(dtype)).sum() + (pe * c["ct"][1].to(dtype)).sum()).backward()
    out = {"start": ps.detach(), "end": pe.detach(), "g.video": v.grad}
    if c["kind"] == "tall":
        out["g.sent"] = s.grad
    if g is not None:
        out["g.gate"] = g.grad
    for k, w in p.items():
        out["gw." + k] = w.grad
    return out


def _tail(z, p, n, mask, dtype):
    l = (torch.tanh(z) @ p[f"{n}_mlp_2.weight"].to(dtype).t()).squeeze(2) + p[f"{n}_mlp_2.bias"].to(dtype)
    if mask is not None:
        l = O.mask_logits(l, mask)
    return torch.softmax(l, dim=1)


def split_form(c):
    """The fused kernel's algebra in float64 -> (start, end, pre-activation z of both heads [B,T,2Hm])."""
    f = torch.float64
    v, s = c["video"].to(f), c["sent"].to(f)
    d = v.size(2)
    g = c["gate"].to(f).unsqueeze(2) if c["gate"] is not None else 1.0
    out, zs = [], []
    for n in ("start", "end"):
        W, b = c["p"][f"{n}_mlp_1.weight"].to(f), c["p"][f"{n}_mlp_1.bias"].to(f)
        Wa, Wb, Wc, Wd = W[:, :d], W[:, d:2 * d], W[:, 2 * d:3 * d], W[:, 3 * d:]
        y = v @ (Wa + Wd).t() + (v * s.unsqueeze(1)) @ Wc.t()
        cs = s @ (Wb + Wd).t()
        z = g * (y + cs.unsqueeze(1)) + b
        zs.append(z)
        out.append(_tail(z, c["p"], n, c["mask"], f))
    return out[0], out[1], torch.cat(zs, 2)


def _split(x32):
    hi = x32.to(torch.bfloat16).to(torch.float32)
    lo = (x32 - hi).to(torch.bfloat16).to(torch.float32)
    return hi.double(), lo.double()


def _mm3(a32, b32):
    """a [.., K] x b [N, K]^T with the three split products."""
    ah, al = _split(a32)
    bh, bl = _split(b32)
    return ah @ bh.t() + ah @ bl.t() + al @ bh.t()


def f32s_form(c):
    """The designed f32s arithmetic -> (start, end, z)."""
    f = torch.float64
    v, s = c["video"], c["sent"]
    d = v.size(2)
    g = c["gate"].to(f).unsqueeze(2) if c["gate"] is not None else 1.0
    vs = v * s.unsqueeze(1)                                              # fp32, one rounding
    out, zs = [], []
    for n in ("start", "end"):
        W, b = c["p"][f"{n}_mlp_1.weight"], c["p"][f"{n}_mlp_1.bias"].to(f)
        Wv = W[:, :d] + W[:, 3 * d:]                                     # fp32
        Wbd = W[:, d:2 * d] + W[:, 3 * d:]
        y = _mm3(v, Wv) + _mm3(vs, W[:, 2 * d:3 * d])
        cs = (s @ Wbd.t()).to(f)                                         # the per-item row: a plain fp32 GEMM
        z = g * (y + cs.unsqueeze(1)) + b
        zs.append(z)
        out.append(_tail(z, c["p"], n, c["mask"], f))
    return out[0], out[1], torch.cat(zs, 2)

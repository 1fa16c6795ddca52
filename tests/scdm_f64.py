"""float64 ground truth for K1 / K1g (plain helper module of tests/test_scdm_f64_cpu.py and tests/test_scdm_f64_gpu.py).

``reference`` is the operation itself -- e = sum_k w_k tanh(a + s), P = softmax_n e, C = P V, gate-fused out = r sigmoid(P V + gbias) -- on the
CPU with autograd, in float64 (the truth) or in float32 (``E32``: the same formula in the kernels' own precision, the yardstick of the bound).
``family`` builds the operand sets: unit scale up to the clamp edge of the contract DESIGN 4.1 / 4.1a states (|a| <= 39 and |s| <= 39 for
sentences of up to 32 words), and ``scale30`` beyond it (in contract for the long kernels only)."""
import functools

import torch

BF = torch.bfloat16
CLAMP = 39.0                       # in-contract operand range of the 32-word kernels (the q-form clamps to [-39, 40])
FLOOR = 64.0 * 2.0 ** -24          # x max|want|: the floor of the bound, for tensors on which the fp32 formula happens to be exact
MARGIN = 16.0                      # x E32
FAMILIES = ("scale1", "scale4", "scale12", "scale19", "pinned", "mixed", "edge", "tiny_w", "equal")      # in contract for every kernel
ALL_FAMILIES = FAMILIES + ("scale30",)                                                                   # scale30: the long kernels only


def _alternating(a, s, v):
    """+-v against -+v with alternating sign along k, some words flipped: a + s = 0 and +-2v side by side in neighbouring k elements."""
    H = a.shape[-1]
    sign = torch.where(torch.arange(H) % 2 == 0, 1.0, -1.0)
    a[:] = v * sign; a[:, 1::2] *= -1.0
    s[:] = -v * sign; s[:, ::5] *= -1.0


def family(kind, B, T, N, H, seed=0):
    """(a [B,T,H], s [B,N,H], w [H]) of one operand family, fp32.  a and s hold bf16-exact values where the family pins them."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, T, H, generator=g); s = torch.randn(B, N, H, generator=g); w = torch.randn(H, generator=g) / H ** 0.5
    if kind.startswith("scale"):
        a, s = a * float(kind[5:]), s * float(kind[5:])
    elif kind == "pinned":                       # rows pinned at a + s = +-40 (and 0), from +-20 and +-20
        a[:, ::2] = 20.0; a[:, 1::2] = -20.0
        s[:, ::3] = 20.0; s[:, 1::3] = -20.0
    elif kind == "mixed":
        _alternating(a, s, 30.0)
    elif kind == "edge":                         # the same pattern at the clamp edge; every seventh column of s moved so that the scores differ
        _alternating(a, s, CLAMP)
        s[..., ::7] += 0.25
    elif kind == "tiny_w":                       # weights of 0 and 1e-7 on scale-12 operands
        w[::2] = 0.0; w[1::4] = 1e-7
        a, s = a * 12.0, s * 12.0
    elif kind == "equal":                        # every word the same: all scores equal, P = 1/N
        s[:] = s[:, :1].clone()
    else:
        raise ValueError(kind)
    if kind != "scale30":
        a, s = a.clamp(-CLAMP, CLAMP), s.clamp(-CLAMP, CLAMP)
    return a.contiguous(), s.contiguous(), w.contiguous()


def extras(B, T, N, Ds, seed=0):
    """(V [B,N,Ds], gC [B,T,Ds], gbias [Ds], r [B,T,Ds]): the word rows (sent, or VW gate-fused), the output's gradient and the gate's operands."""
    g = torch.Generator().manual_seed(seed + 1000)
    return (torch.randn(B, N, Ds, generator=g), torch.randn(B, T, Ds, generator=g), torch.randn(Ds, generator=g) * 0.1,
            torch.randn(B, T, Ds, generator=g))


def reference(a, s, w, V, gC, gate=None, dtype=torch.float64):
    """The operation and all its gradients in ``dtype`` on the CPU, one batch item at a time (no [B,T,N,H] tensor).
    -> dict: P, C (or out with gate = (gbias, r)), da, ds, dw, dV (and dgbias, dr)."""
    a, s, V, gC = (x.detach().to(dtype) for x in (a, s, V, gC))
    w = w.detach().to(dtype).clone().requires_grad_(True)
    if gate is not None:
        gb = gate[0].detach().to(dtype).clone().requires_grad_(True)
        r = gate[1].detach().to(dtype)
    per_item = {k: [] for k in ("P", "out", "da", "ds", "dV", "dr")}
    for b in range(a.shape[0]):                  # the item's rows are leaves of their own: their gradients are not summed into [B, ...] tensors
        ab, sb, vb = (x[b].clone().requires_grad_(True) for x in (a, s, V))
        e = torch.matmul(torch.tanh(ab.unsqueeze(1) + sb.unsqueeze(0)), w)               # [T,N]
        P = torch.softmax(e, dim=-1)
        out = P @ vb
        if gate is not None:
            rb = r[b].clone().requires_grad_(True)
            out = rb * torch.sigmoid(out + gb)
            (out * gC[b]).sum().backward()
            per_item["dr"].append(rb.grad)
        else:
            (out * gC[b]).sum().backward()
        for k, v in (("P", P.detach()), ("out", out.detach()), ("da", ab.grad), ("ds", sb.grad), ("dV", vb.grad)):
            per_item[k].append(v)
    res = {k: torch.stack(v) for k, v in per_item.items() if v}
    res["dw"] = w.grad
    if gate is not None:
        res["dgbias"] = gb.grad
    else:
        res["C"] = res.pop("out")
    return res


def rule(e32, S):
    """The bound on a quantity the kernels compute in fp32 arithmetic: elementwise |got - float64| <= max(16 E32, 64 2^-24 S), E32 = max error
    of the float32 run of ``reference`` on that tensor, S = max|want|.  16: the kernels form tanh with three roundings and two 1-ulp hardware
    approximations (v_exp_f32, v_rcp_f32) where torch rounds one correctly rounded call, ~4x per term; a lane-strided summation order adds no
    more than that again; 16x leaves 4x of headroom."""
    return max(MARGIN * e32, FLOOR * S)


def bf16_valued(t):
    return t.to(BF).float()


@functools.lru_cache(maxsize=24)
def truth(kind, B, T, N, H, Ds, bf=False, gate=False, seed=0):
    """Operands, the float64 result and E32 per tensor, computed once per (family, shape, storage, form) and shared by every test that needs
    them (read-only).  bf: the activations hold bf16 values (the weights w, gbias stay fp32).
    -> (ins dict of fp32 CPU tensors, want dict of float64 tensors, e32 dict of floats)."""
    a, s, w = family(kind, B, T, N, H, seed)
    V, gC, gb, r = extras(B, T, N, Ds, seed)
    if bf:
        a, s, V, gC, r = (bf16_valued(x) for x in (a, s, V, gC, r))
    g = (gb, r) if gate else None
    want = reference(a, s, w, V, gC, g, torch.float64)
    f32 = reference(a, s, w, V, gC, g, torch.float32)
    e32 = {k: float((f32[k].double() - want[k]).abs().max()) for k in want}
    return dict(a=a, s=s, w=w, V=V, gC=gC, gbias=gb, r=r), want, e32

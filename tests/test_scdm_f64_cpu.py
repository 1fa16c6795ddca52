"""The float64 tier of K1 / K1g on the CPU (tests/scdm_f64.py): the float64 reference against the pinned oracle and the reference's goldens, the
operand families against the contract's range, and a torch-fp32 restatement of the two score forms of csrc/scdm_attn.hip -- the per-element
triple w rcp(Ea Es + 1) and the q-form (one reciprocal per four k elements) -- over every family: the range claims the kernel's comments make,
and P against float64 within the bound the GPU tests apply.  When a GPU case of tests/test_scdm_f64_gpu.py fails, this file tells "the arithmetic
as designed is wrong" (it fails too) from "the kernel implements it wrongly" (it passes)."""
import pytest
import torch

from oracle import tsg_oracle as O
import scdm_f64 as R

TOL = dict(atol=2e-6, rtol=1e-5)                 # tests/test_oracle_golden.py
K2LOG2E = 2.0 * 1.4426950408889634
LOG2E = 1.4426950408889634
KQU = 2.0 ** -26                                 # csrc/scdm_attn.hip: kQU
KQHALF = 13.0                                    # ... kQHalfExp
MIN_NORMAL = 2.0 ** -126


def test_reference_matches_the_fp32_oracle():
    a, s, w = R.family("scale1", 3, 17, 20, 40, seed=1)
    V, gC, _, _ = R.extras(3, 17, 20, 24, seed=1)
    want = R.reference(a, s, w, V, gC)
    al, sl, wl, vl = (x.clone().requires_grad_(True) for x in (a, s, w, V))
    C, P = O.scdm_core(al, sl, wl, vl)
    C.backward(gC)
    for name, got in (("P", P.detach()), ("C", C.detach()), ("da", al.grad), ("ds", sl.grad), ("dw", wl.grad), ("dV", vl.grad)):
        torch.testing.assert_close(got, want[name].float(), **TOL, msg=lambda m, n=name: f"{n}: {m}")


def test_gated_reference_matches_the_unfused_formula():
    a, s, w = R.family("scale4", 2, 9, 5, 24, seed=2)
    V, gC, gb, r = R.extras(2, 9, 5, 24, seed=2)
    want = R.reference(a, s, w, V, gC, gate=(gb, r))
    lv = [x.double().requires_grad_(True) for x in (a, s, w, V, gb, r)]
    _, P = O.scdm_core(lv[0], lv[1], lv[2], lv[3])
    out = lv[5] * torch.sigmoid(torch.bmm(P, lv[3]) + lv[4])
    out.backward(gC.double())
    torch.testing.assert_close(out.detach(), want["out"], atol=1e-13, rtol=1e-12)
    for name, x in zip(("da", "ds", "dw", "dV", "dgbias", "dr"), lv):
        torch.testing.assert_close(x.grad, want[name], atol=1e-12, rtol=1e-11, msg=lambda m, n=name: f"{n}: {m}")


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_reference_matches_the_goldens(golden, tag):
    """C and the input gradients the real reference produced (tests/golden/scdm_*.npz), through the float64 reference and the projections."""
    g = golden("scdm_" + tag)
    wt = g.weights
    video, sent = g.t("video"), g.t("sent")
    a = torch.nn.functional.linear(video.double(), wt["W_a.weight"].double(), wt["W_a.bias"].double())
    s = torch.nn.functional.linear(sent.double(), wt["W_s.weight"].double())
    res = R.reference(a, s, wt["w.weight"].reshape(-1), sent, g.t("gC"))
    torch.testing.assert_close(res["C"].float(), g.t("C"), **TOL)
    torch.testing.assert_close((res["da"] @ wt["W_a.weight"].double()).float(), g.t("gvideo"), **TOL)
    torch.testing.assert_close((res["ds"] @ wt["W_s.weight"].double() + res["dV"]).float(), g.t("gsent"), **TOL)
    torch.testing.assert_close(res["dw"].float().reshape(1, -1), g.wgrads["w.weight"], **TOL)


@pytest.mark.parametrize("kind", R.ALL_FAMILIES)
def test_families_respect_the_contract(kind):
    a, s, w = R.family(kind, 2, 20, 26, 256)
    assert a.shape == (2, 20, 256) and s.shape == (2, 26, 256) and w.shape == (256,)
    assert all(bool(torch.isfinite(x).all()) for x in (a, s, w))
    if kind == "scale30":
        assert float(a.abs().max()) > 40 and float(s.abs().max()) > 40          # the point of the family: beyond the clamp
        return
    assert float(a.abs().max()) <= R.CLAMP and float(s.abs().max()) <= R.CLAMP
    x = a.unsqueeze(2) + s.unsqueeze(1)
    if kind == "pinned":                          # the pinned values survive bf16 storage
        assert torch.equal(R.bf16_valued(a), a) and torch.equal(R.bf16_valued(s[:, ::3]), s[:, ::3])
        assert float(x.max()) == 40.0 and float(x.min()) == -40.0 and bool((x == 0).any())
    if kind in ("mixed", "edge"):
        assert torch.equal(R.bf16_valued(a), a) and torch.equal(R.bf16_valued(s), s)
        v = 30.0 if kind == "mixed" else R.CLAMP
        assert float(x.max()) == 2 * v and float(x.min()) == -2 * v and bool((x == 0).any())
        assert bool(((x[..., :-1] == 2 * v) & (x[..., 1:] == -2 * v)).any())      # saturated high and saturated low in neighbouring k elements
    if kind == "equal":
        assert torch.equal(s, s[:, :1].expand_as(s))
    if kind == "tiny_w":
        assert float(w[::2].abs().max()) == 0.0 and bool((w[1::4] == 1e-7).all())


def _fma(x, y, z):
    """fp32 fused multiply-add: the product of two fp32 numbers is exact in float64, one rounding at the end"""
    return (x.double() * y.double() + z.double()).float()


def _softmax_fp32(z):
    m = z.max(-1, keepdim=True).values
    p = torch.exp2((z - m) * LOG2E)
    return p * (1.0 / p.sum(-1, keepdim=True))


def _triple_scores(a, s, w):
    """scdm_chunk_step: e'[t,n] = sum_k (-2 w_k) rcp(Ea Es + 1), Ea = exp(2 clamp(a, +-40)), all fp32.  -> (e', Ea, Es, denominators)"""
    Ea = torch.exp2(a.clamp(-40.0, 40.0) * K2LOG2E); Es = torch.exp2(s.clamp(-40.0, 40.0) * K2LOG2E)
    d = _fma(Ea.unsqueeze(2), Es.unsqueeze(1), torch.ones(()))                  # [B,T,N,H]; an overflowing product -> inf -> r = 0
    r = 1.0 / d
    acc = torch.zeros(d.shape[:-1] + (d.shape[-1] // 4,))
    for c in range(4):                                                           # the lane's four k elements in order, then over the lanes
        acc = _fma((-2.0 * w[c::4]).expand_as(acc), r[..., c::4], acc)
    return acc.sum(-1), Ea, Es, d


def _q_scores(a, s, w):
    """scdm_chunk_step_q: operands pre-scaled by 2^-13 each, d' = clamp01(Ea' Es' + u), u = 2^-26, four consecutive k share one reciprocal,
    w2 = -2 w u.  -> (e', Ea', Es', products of four denominators)"""
    Ea = torch.exp2(_fma(a.clamp(-39.0, 40.0), torch.tensor(K2LOG2E), torch.tensor(-KQHALF)))
    Es = torch.exp2(_fma(s.clamp(-39.0, 40.0), torch.tensor(K2LOG2E), torch.tensor(-KQHALF)))
    d = _fma(Ea.unsqueeze(2), Es.unsqueeze(1), torch.tensor(KQU)).clamp(0.0, 1.0)          # the FMA's output modifier
    w2 = (-2.0 * KQU) * w
    d0, d1, d2, d3 = (d[..., c::4] for c in range(4))
    w0, w1, w2_, w3 = (w2[c::4] for c in range(4))
    n01 = _fma(w1.expand_as(d0), d0, w0 * d1); p01 = d0 * d1
    n23 = _fma(w3.expand_as(d2), d2, w2_ * d3); p23 = d2 * d3
    num = _fma(n23, p01, n01 * p23)
    den = p01 * p23
    terms = num * (1.0 / den)                                                              # [B,T,N,H/4]
    return terms.sum(-1), Ea, Es, den


@pytest.mark.parametrize("H", [64, 256, 1024])
@pytest.mark.parametrize("kind", R.ALL_FAMILIES)
def test_score_forms_restated_in_fp32(kind, H):
    """Both score forms on every family: finite, the q-form's scaled exponentials normal numbers and its denominator products >= 2^-104 (the
    range claims of csrc/scdm_attn.hip), and -- inside the contract -- P within the GPU tests' bound of float64."""
    B, T, N = 2, 20, 20
    a, s, w = R.family(kind, B, T, N, H)
    x = a.double().unsqueeze(2) + s.double().unsqueeze(1)
    want = torch.softmax(torch.matmul(torch.tanh(x), w.double()), -1)
    e32 = float((O.scdm_core(a, s, w, torch.zeros(B, N, 1))[1].double() - want).abs().max())
    bound = min(R.rule(e32, float(want.max())), 1e-4)
    for form, fn in (("triple", _triple_scores), ("q", _q_scores)):
        e, Ea, Es, den = fn(a, s, w)
        assert bool(torch.isfinite(e).all()), form
        assert bool(torch.isfinite(Ea).all()) and bool(torch.isfinite(Es).all()), form
        assert float(Ea.min()) >= MIN_NORMAL and float(Es.min()) >= MIN_NORMAL, f"{form}: a scaled exponential is not a normal number"
        assert not bool(torch.isnan(den).any()), form
        if form == "q":
            assert float(den.min()) >= 2.0 ** -104 and float(den.max()) <= 1.0
        P = _softmax_fp32(e)
        assert bool(torch.isfinite(P).all()), form
        assert float((P.sum(-1) - 1).abs().max()) <= N * 2.0 ** -23
        err = float((P.double() - want).abs().max())
        print(f"  {kind} H={H} {form}: P err {err:.2e}  E32 {e32:.2e}  bound {bound:.2e}  ratio {err / bound:.2f}")
        if kind != "scale30":                    # scale30 is outside the 32-word kernels' contract: finite, nothing more
            assert err <= bound, f"{form} form on {kind}, H={H}: P error {err:.3e} > {bound:.3e}"

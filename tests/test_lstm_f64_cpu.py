"""The float64 tier of the BiLSTM recurrence on the CPU (tests/lstm_f64.py): the float64 reference against torch.nn.LSTM in float64 -- with
h_n carrying gradient, which pins where dHn enters -- and against the reference project's golden vectors; the operand families against what
each is built to reach; the activation formulas of csrc/lstm.hip (sigmoid_f, tanh_f) restated in torch fp32 over every family, within the
bound the GPU tests apply; and the part of the f32s and bf16 bounds that the designed roundings alone use up.  When a GPU case of
tests/test_lstm_f64_gpu.py fails, this file tells "the arithmetic as designed is wrong" (it fails too) from "the kernel implements it wrongly"
(it passes)."""
import pytest
import torch

import lstm_f64 as R

TOL = dict(atol=2e-6, rtol=1e-5)                 # tests/test_oracle_golden.py
LOG2E = 1.4426950408889634
B0, T0 = 20, 12                                  # the base shape of the GPU tests


def test_reference_matches_nn_lstm_in_float64():
    """out, h_n, c_n and the gradient with respect to the input gates.  nn.LSTM takes no pre-computed gates, so it gets x = Gx as its input with
    W_ih = (1 0) for the forward direction and (0 1) for the reverse one and zero biases: x.grad IS dG.  h_n carries gradient: the reverse
    direction's h_n is its state after t = 0, so this pins dHn to t = T-1 (forward) and t = 0 (reverse)."""
    B, T, h = 3, 7, 8
    Gx, W = R.family("unit", B, T, h, seed=3)
    dOut, dHn = R.extras(B, T, h, seed=3)
    want = R.reference(Gx, W, dOut, dHn)
    m = torch.nn.LSTM(8 * h, h, bidirectional=True).double()
    eye = torch.eye(4 * h, dtype=torch.float64); zero = torch.zeros(4 * h, 4 * h, dtype=torch.float64)
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.cat((eye, zero), 1)); m.weight_ih_l0_reverse.copy_(torch.cat((zero, eye), 1))
        m.weight_hh_l0.copy_(W[0].double()); m.weight_hh_l0_reverse.copy_(W[1].double())
        for b in (m.bias_ih_l0, m.bias_hh_l0, m.bias_ih_l0_reverse, m.bias_hh_l0_reverse):
            b.zero_()
    x = Gx.double().reshape(T, B, 8 * h).requires_grad_(True)
    out, (hn, cn) = m(x)
    ((out * dOut.double()).sum() + (hn * dHn.double()).sum()).backward()
    tight = dict(atol=1e-13, rtol=1e-12)
    torch.testing.assert_close(want["out"], out.detach(), **tight)
    torch.testing.assert_close(want["hn"], hn.detach(), **tight)
    torch.testing.assert_close(want["cn"], cn.detach(), **tight)
    torch.testing.assert_close(want["dG"], x.grad.reshape(T, B, 2, 4 * h), **tight)
    torch.testing.assert_close(want["dbias"], x.grad.reshape(T * B, 2, 4 * h).sum(0), **tight)
    assert torch.equal(want["hn"][0], want["out"][T - 1, :, :h]) and torch.equal(want["hn"][1], want["out"][0, :, h:])
    assert torch.equal(want["cn"][0], want["Cs"][T - 1, 0]) and torch.equal(want["cn"][1], want["Cs"][0, 1])
    # dHn is not the same as more dOut at the other end of the sequence
    other = R.reference(Gx, W, dOut, None)
    assert float((other["dG"] - want["dG"]).abs().max()) > 1e-3


def test_hand_written_backward_equals_autograd():
    """``backward_from_saved`` (the formulas the kernels use, from R and Cs) against autograd on the same float64 forward, with and without dHn."""
    Gx, W = R.family("scale4", 5, 9, 12, seed=4)
    dOut, dHn = R.extras(5, 9, 12, seed=4)
    for hn in (None, dHn):
        want = R.reference(Gx, W, dOut, hn)
        dG, db = R.backward_from_saved(W, want["R"], want["Cs"], dOut, hn)
        torch.testing.assert_close(dG, want["dG"], atol=1e-13, rtol=1e-11)
        torch.testing.assert_close(db, want["dbias"], atol=1e-12, rtol=1e-11)


def test_reference_matches_the_goldens(golden):
    """The two-layer BiLSTM the real reference ran (tests/golden/bilstm.npz), through the float64 reference and the input projections: outputs, final
    states, the input gradient and every parameter gradient (h_n of both layers carries gradient there)."""
    g = golden("bilstm")
    w = {k: v.double() for k, v in g.weights.items()}
    x = g.t("x").double().transpose(0, 1)                         # time-major [T,B,I]
    go, gh = g.t("g").double().transpose(0, 1), g.t("gh").double()
    T, B, _ = x.shape
    h = 8
    sufs = ("", "_reverse")

    def gates(inp, k):
        return torch.stack([inp @ w[f"lstm.weight_ih_l{k}{s}"].t() + w[f"lstm.bias_ih_l{k}{s}"] + w[f"lstm.bias_hh_l{k}{s}"] for s in sufs], 2)

    def whh(k):
        return torch.stack([w[f"lstm.weight_hh_l{k}{s}"] for s in sufs])

    zero = torch.zeros(T, B, 2 * h, dtype=torch.float64)
    l0 = R.reference(gates(x, 0), whh(0), zero)                   # forward of layer 0 (its gradients follow below)
    l1 = R.reference(gates(l0["out"], 1), whh(1), go, gh[2:4])
    torch.testing.assert_close(l1["out"].transpose(0, 1).float(), g.t("out"), **TOL)
    torch.testing.assert_close(torch.cat((l0["hn"], l1["hn"])).float(), g.t("hn"), **TOL)
    torch.testing.assert_close(torch.cat((l0["cn"], l1["cn"])).float(), g.t("cn"), **TOL)
    d_out0 = sum(l1["dG"][:, :, d] @ w[f"lstm.weight_ih_l1{s}"] for d, s in enumerate(sufs))
    l0 = R.reference(gates(x, 0), whh(0), d_out0, gh[0:2])
    gx = sum(l0["dG"][:, :, d] @ w[f"lstm.weight_ih_l0{s}"] for d, s in enumerate(sufs))
    torch.testing.assert_close(gx.transpose(0, 1).float(), g.t("gx"), **TOL)
    wg = g.wgrads
    for k, layer, inp in ((0, l0, x), (1, l1, l0["out"])):
        for d, s in enumerate(sufs):
            dg = layer["dG"][:, :, d]                                                # [T,B,4h]
            hprev = torch.zeros(T, B, h, dtype=torch.float64)                        # h_(t-1) in the direction's own order
            hd = layer["out"][:, :, d * h:(d + 1) * h]
            if d == 0:
                hprev[1:] = hd[:-1]
            else:
                hprev[:-1] = hd[1:]
            tol = dict(atol=5e-6, rtol=1e-5)
            torch.testing.assert_close(torch.einsum("tbg,tbi->gi", dg, inp).float(), wg[f"lstm.weight_ih_l{k}{s}"], **tol)
            torch.testing.assert_close(torch.einsum("tbg,tbi->gi", dg, hprev).float(), wg[f"lstm.weight_hh_l{k}{s}"], **tol)
            torch.testing.assert_close(layer["dbias"][d].float(), wg[f"lstm.bias_ih_l{k}{s}"], **tol)
            torch.testing.assert_close(layer["dbias"][d].float(), wg[f"lstm.bias_hh_l{k}{s}"], **tol)


@pytest.mark.parametrize("kind", R.ALL_FAMILIES)
def test_families_do_what_they_say(kind):
    T = 128 if kind == "remember" else T0
    h = 128
    ins, want, e32, _ = R.truth(kind, B0, T, h)
    Gx, W = ins["Gx"], ins["W"]
    assert Gx.shape == (T, B0, 2, 4 * h) and W.shape == (2, 4 * h, h)
    for k, v in want.items():
        assert bool(torch.isfinite(v).all()), k
    uGx, uW = R.family("unit", B0, T, h)
    Z, Rg, Cs, out = want["Z"], want["R"], want["Cs"], want["out"]
    if kind == "unit":                           # today's operands (tests/test_lstm_gpu.py)
        g = torch.Generator().manual_seed(0)
        assert torch.equal(Gx, torch.randn(T, B0, 2, 4 * h, generator=g) * 0.5) and torch.equal(W, torch.randn(2, 4 * h, h, generator=g) / h ** 0.5)
    elif kind == "small":                        # gates at 0.5, tanh arguments of about 1e-3
        assert float(out.abs().max()) < 1e-2 and float((Rg[..., (0, 1, 3)] - 0.5).abs().max()) < 1e-2
        assert float(Z[..., 2].abs().max()) < 1e-2 and float(Cs.abs().max()) < 1e-2
    elif kind == "scale4":                       # saturated and unsaturated gates side by side
        assert float((Z.abs() > 8).double().mean()) > 0.04 and float((Z.abs() < 1).double().mean()) > 0.1
    elif kind == "w2":
        assert torch.equal(Gx, uGx) and torch.equal(W, 2 * uW)
    elif kind == "saturated":                    # exp2 overflows in sigmoid_f (z < -128 ln 2 = -88.7), tanh_f clamps (|z| > 44)
        assert float((Z.abs() > 20).double().mean()) > 0.5
        assert float(Z.min()) < -100 and float(Z[..., 2].abs().max()) > 100
    elif kind == "remember":                     # the cell state integrates: about 1 per step
        assert float(Cs.max()) >= 0.9 * T
        assert float(Rg[..., 0].min()) > 0.999 and float(Rg[..., 1].min()) > 0.999
    elif kind == "forget":                       # c_t = i g
        assert float(Rg[..., 1].max()) < 1e-9
        assert float((Cs - Rg[..., 0] * Rg[..., 2]).abs().max()) < 1e-9
    elif kind == "zero_w":                       # every (t, b, direction, unit) on its own: gate order i, f, g, o; direction d in columns d h .. d h + h
        gz = Gx.double().view(T, B0, 2, 4, h)
        i, g_, o = torch.sigmoid(gz[..., 0, :]), torch.tanh(gz[..., 2, :]), torch.sigmoid(gz[..., 3, :])
        assert not bool(W.any())
        torch.testing.assert_close(out[T - 1, :, h:], o[T - 1, :, 1] * torch.tanh(i[T - 1, :, 1] * g_[T - 1, :, 1]), atol=1e-14, rtol=0)   # reverse, first step
        torch.testing.assert_close(out[0, :, :h], o[0, :, 0] * torch.tanh(i[0, :, 0] * g_[0, :, 0]), atol=1e-14, rtol=0)                   # forward, first step
    elif kind == "beyond":
        assert float(Z.abs().max()) > 300


def _sigmoid_f(x):
    """csrc/lstm.hip sigmoid_f: rcp(1 + exp2(-x log2 e)), in the tensor's precision (fp32 here)"""
    return 1.0 / (1.0 + torch.exp2(-x * LOG2E))


def _tanh_f(x):
    """csrc/lstm.hip tanh_f: 1 - 2 rcp(exp2(2 log2 e clamp(x, +-44)) + 1)"""
    e = torch.exp2(x.clamp(-44.0, 44.0) * (2.0 * LOG2E))
    return 1.0 - 2.0 / (e + 1.0)


@pytest.mark.parametrize("kind", R.ALL_FAMILIES)
@pytest.mark.parametrize("T", [T0, 128])
def test_activation_formulas_restated_in_fp32(kind, T):
    """The kernels' formulas for sigmoid and tanh, in torch fp32 with correctly rounded exp2 and division, through the whole recurrence and the
    hand-written backward: finite on every family (``beyond`` included: exp2 overflows to inf, rcp(inf) = 0), and -- inside the contract --
    within the fp32 bound of the GPU tests.  (Measured: at most 0.16 of the bound, dbias at T = 128 on ``w2``; 0.11 at T = 12.)"""
    h = 128
    ins, want, e32, _ = R.truth(kind, B0, T, h)
    with torch.no_grad():
        fw = R.forward(ins["Gx"], ins["W"], torch.float32, sigmoid=_sigmoid_f, tanh=_tanh_f)
        dG, db = R.backward_from_saved(ins["W"], fw["R"], fw["Cs"], ins["dOut"], ins["dHn"], tanh=_tanh_f)
    got = dict(out=fw["out"], R=fw["R"], Cs=fw["Cs"], dG_hn=dG, dbias_hn=db)
    worst = {}
    for k, v in got.items():
        assert v.dtype == torch.float32 and bool(torch.isfinite(v).all()), f"{kind}: {k} not finite"
        worst[k] = float(((v.double() - want[k]).abs() / R.bound_fp32(e32[k], want[k])).max())
    print(f"\n  {kind} T={T}: error / bound " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    if kind != "beyond":
        assert max(worst.values()) <= 1.0, f"{kind}: {worst}"


# ---- conditions on the bounds: what the designed roundings alone use of them ---------------------------------------------------------------------
_SHAPES = [(20, 12, 128, R.FAMILIES), (20, 128, 128, R.SHORT), (20, 128, 512, R.SHORT), (144, 8, 512, R.SHORT)]
_PARAMS = [pytest.param(B, T, h, kind, id=f"{B}-{T}-{h}-{kind}") for B, T, h, kinds in _SHAPES for kind in kinds]


@pytest.mark.parametrize("B,T,h,kind", _PARAMS)
def test_split_emulation_uses_at_most_half_of_the_f32s_bound(B, T, h, kind):
    """hi hi + hi lo + lo hi of bf16 halves in both products, everything else float64, against float64: at most half of 2e-5 max(1, S)
    on every tensor.  A bound the designed rounding alone nearly fills would hide nothing.  (Measured: out <= 0.33, R <= 0.42, Cs <= 0.23, dG <= 0.22,
    dbias <= 0.2.)"""
    ins, want, _, _ = R.truth(kind, B, T, h)
    got = R.emulate_split(ins["Gx"], ins["W"], ins["dOut"], ins["dHn"])
    share = {}
    for k, wk in (("out", "out"), ("R", "R"), ("Cs", "Cs"), ("dG", "dG_hn"), ("dbias", "dbias_hn")):
        S = float(want[wk].abs().max())
        share[k] = float((got[k] - want[wk]).abs().max()) / (2e-5 * max(1.0, S))
    print(f"\n  split [{B},{T},{h}] {kind}: share of 2e-5 max(1,S) " + " ".join(f"{k} {v:.3f}" for k, v in share.items()))
    assert max(share.values()) <= 0.5, share


@pytest.mark.parametrize("B,T,h,kind", _PARAMS)
def test_bf16_emulation_uses_at_most_half_of_the_storage_bound(B, T, h, kind):
    """The roundings of the bf16 storage mode (W_hh once, h fed back as stored, R as stored) against float64 on bf16-valued operands: at most half
    of ``_close`` at rel = 1e-2 on out and Cs.  (Measured: <= 0.25 / 0.12; R <= 0.29.)  The gradients' bound is derived from this emulation's own error in
    tests/test_lstm_f64_gpu.py; it is printed here."""
    ins, want, _, ebf = R.truth(kind, B, T, h, bf=True)
    got = R.emulate_bf16(ins["Gx"], ins["W"], ins["dOut"], None)
    share = {k: float(((got[k] - want[k]).abs() / R.bound_close(want[k], 1e-2)).max()) for k in ("out", "R", "Cs")}
    grad = {k: ebf[k] / max(1.0, float(want[k].abs().max())) for k in ("dG", "dbias", "dG_hn", "dbias_hn")}
    print(f"\n  bf16 [{B},{T},{h}] {kind}: share of _close(1e-2) " + " ".join(f"{k} {v:.3f}" for k, v in share.items())
          + " | EBF / scale " + " ".join(f"{k} {v:.2e}" for k, v in grad.items()))
    assert share["out"] <= 0.5 and share["Cs"] <= 0.5, share

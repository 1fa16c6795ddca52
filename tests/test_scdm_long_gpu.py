"""K1 / K1g for sentences of more than 32 words (tsg_scdm_long_*, csrc/scdm_long.hip) on the GPU: kernel parity against the CPU oracle in
the strict-fp32, f32s and bf16-storage modes, chunk boundaries, saturation, the reference's own outputs (tests/golden/scdm_long.npz), the
modules and models at sent_len = 48, graph replay and the error paths.

Tolerances are the project's existing ones: outputs 1e-4 (tests/test_scdm_gpu.py TOL); K1 gradients atol 2e-4 max(1, max|g|), rtol 1e-3
(_run there); model-level gradients atol 3e-4, rtol 3e-3 (tests/test_models_gpu.py); bf16 storage the per-kernel bounds of
tests/test_bf16_storage_gpu.py (_close: stored bf16 tensors 1e-2 max(1, max|want|) / 1e-2, P 1e-4, dw and dgbias 2e-3)."""
import logging

import pytest
import torch

from oracle import tsg_oracle as O

pytestmark = pytest.mark.gpu
TOL = dict(atol=1e-4, rtol=1e-4)
BF = torch.bfloat16
LOG = logging.getLogger("t")
lin = torch.nn.functional.linear

SHAPES = [(2, 9, 33, 24, 24), (3, 17, 40, 40, 24), (1, 1, 33, 8, 8), (2, 64, 48, 512, 512), (2, 40, 50, 1024, 1024),
          (2, 128, 64, 1024, 1024), (1, 33, 128, 260, 516),
          (130, 100, 40, 256, 256)]      # the full grid with ragged tiles: 520 forward workgroups, T = 100 = 3 x 32 + 4
MODES = [None, "f32s", "bf16"]


def _r(t):
    return t.to(BF).float()


def _mode(request, mode):
    from shufflingvideosfortsg_amd import engine
    engine.set_precision(mode if mode == "f32s" else None)     # bf16 storage is selected by the tensors' dtype at this level
    request.addfinalizer(lambda: engine.set_precision(None))


def _grad_close(got, want, name):
    atol = 2e-4 * max(1.0, float(want.abs().max()))
    err = float((got.float().cpu() - want).abs().max())
    print(f"    d{name}: max err {err:.3e} (max|g| {float(want.abs().max()):.3e}, atol {atol:.3e})")
    torch.testing.assert_close(got.cpu(), want, atol=atol, rtol=1e-3, msg=lambda m: f"d{name}: {m}")


def _bf_close(got, want, name, rel=1e-2, tight=None):
    rel = tight if tight is not None else rel
    scale = max(1.0, float(want.abs().max()))
    print(f"    {name}: max err {float((got.float().cpu() - want).abs().max()):.3e} (atol {rel * scale:.3e})")
    torch.testing.assert_close(got.float().cpu(), want, atol=rel * scale, rtol=rel, msg=lambda m: f"{name}: {m}")


def _plain_case(a, s, w, sent, gC, bf):
    """One forward + backward of scdm_attn_long against O.scdm_core on the given CPU fp32 operands (bf16-valued where bf)."""
    from shufflingvideosfortsg_amd import functional as F
    a, s, w, sent = (x.detach().clone().requires_grad_(True) for x in (a, s, w, sent))
    C0, P0 = O.scdm_core(a, s, w, sent)
    C0.backward(gC)
    cast = (lambda x: x.detach().to(BF).cuda().requires_grad_(True)) if bf else (lambda x: x.detach().cuda().requires_grad_(True))
    ad, sd, vd = cast(a), cast(s), cast(sent)
    wd = w.detach().cuda().requires_grad_(True)
    C1, P1 = F.scdm_attn_long(ad, sd, wd, vd, return_p=True)
    C1.backward(gC.to(BF).cuda() if bf else gC.cuda())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(C1.float()).all()) and bool(torch.isfinite(P1).all())
    print(f"    P: max err {float((P1.cpu() - P0.detach()).abs().max()):.3e}   C: max err {float((C1.float().cpu() - C0.detach()).abs().max()):.3e}")
    if bf:
        assert C1.dtype == BF and P1.dtype == torch.float32
        _bf_close(P1, P0.detach(), "P", tight=1e-4)
        _bf_close(C1, C0.detach(), "C")
        for got, want, name in ((ad.grad, a.grad, "da"), (sd.grad, s.grad, "ds"), (vd.grad, sent.grad, "dsent")):
            assert got.dtype == BF
            _bf_close(got, want, name)
        _bf_close(wd.grad, w.grad, "dw", tight=2e-3)
    else:
        torch.testing.assert_close(P1.cpu(), P0.detach(), **TOL)
        torch.testing.assert_close(C1.detach().cpu(), C0.detach(), **TOL)
        for got, want, name in zip((ad, sd, wd, vd), (a, s, w, sent), "a s w sent".split()):
            _grad_close(got.grad, want.grad, name)
    C2, P2 = F.scdm_attn_long(ad.detach(), sd.detach(), wd.detach(), vd.detach(), return_p=True)     # bitwise run-to-run
    assert torch.equal(C2, C1.detach()) and torch.equal(P2, P1)
    return C1.detach(), P1.detach()


def _plain_inputs(B, T, N, H, Ds, seed=0, scale=1.0, bf=False):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, T, H, generator=g) * scale
    s = torch.randn(B, N, H, generator=g) * scale
    w = torch.randn(H, generator=g) / H ** 0.5
    sent = torch.randn(B, N, Ds, generator=g)
    gC = torch.randn(B, T, Ds, generator=g)
    if bf:
        a, s, sent, gC = _r(a), _r(s), _r(sent), _r(gC)
    return a, s, w, sent, gC


def _gate_case(a, s, w, VW, gb, r, go, bf):
    """scdm_gate_long against the oracle tail on the projected operands: out = r * sigmoid(P @ VW + gbias), all six gradients."""
    from shufflingvideosfortsg_amd import functional as F
    a, s, w, VW, gb, r = (x.detach().clone().requires_grad_(True) for x in (a, s, w, VW, gb, r))
    _, P0 = O.scdm_core(a, s, w, VW)
    out0 = r * torch.sigmoid(torch.bmm(P0, VW) + gb)
    out0.backward(go)
    cast = (lambda x: x.detach().to(BF).cuda().requires_grad_(True)) if bf else (lambda x: x.detach().cuda().requires_grad_(True))
    ad, sd, vd, rd = cast(a), cast(s), cast(VW), cast(r)
    wd, gd = w.detach().cuda().requires_grad_(True), gb.detach().cuda().requires_grad_(True)
    out1 = F.scdm_gate_long(ad, sd, wd, vd, gd, rd)
    out1.backward(go.to(BF).cuda() if bf else go.cuda())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out1.float()).all())
    print(f"    out: max err {float((out1.float().cpu() - out0.detach()).abs().max()):.3e}")
    if bf:
        assert out1.dtype == BF
        _bf_close(out1, out0.detach(), "out")
        for got, want, name in ((ad.grad, a.grad, "da"), (sd.grad, s.grad, "ds"), (vd.grad, VW.grad, "dVW"), (rd.grad, r.grad, "dr")):
            assert got.dtype == BF
            _bf_close(got, want, name)
        _bf_close(wd.grad, w.grad, "dw", tight=2e-3)
        _bf_close(gd.grad, gb.grad, "dgbias", tight=2e-3)
    else:
        torch.testing.assert_close(out1.detach().cpu(), out0.detach(), **TOL)
        for got, want, name in zip((ad, sd, wd, vd, gd, rd), (a, s, w, VW, gb, r), "a s w VW gbias r".split()):
            _grad_close(got.grad, want.grad, name)
    out2 = F.scdm_gate_long(ad.detach(), sd.detach(), wd.detach(), vd.detach(), gd.detach(), rd.detach())
    assert torch.equal(out2, out1.detach())
    return out1.detach()


def _gate_inputs(B, T, N, d, seed=4, scale=1.0, bf=False):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, T, d, generator=g) * scale
    r = torch.randn(B, T, d, generator=g)
    s = torch.randn(B, N, d, generator=g) * scale
    VW = torch.randn(B, N, d, generator=g)
    w = torch.randn(d, generator=g) / d ** 0.5
    gb = torch.randn(d, generator=g) * 0.1
    go = torch.randn(B, T, d, generator=g)
    if bf:
        a, r, s, VW, go = _r(a), _r(r), _r(s), _r(VW), _r(go)
    return a, s, w, VW, gb, r, go


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_long_parity(shape, mode, request):
    """tsg_scdm_long_fwd / _bwd against O.scdm_core: C, P and the four gradients; a second forward is bitwise the same."""
    _mode(request, mode)
    print(f"\n  plain {shape} mode={mode}")
    _plain_case(*_plain_inputs(*shape, bf=mode == "bf16"), bf=mode == "bf16")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_long_gate_parity_on_projected_operands(shape, mode, request):
    """tsg_scdm_long_gate_fwd / _bwd (Ds = H) against the oracle's tail with sent_linear reassociated onto the word rows: the output and
    all six gradients (da, ds, dw, dVW, dgbias, dr)."""
    _mode(request, mode)
    B, T, N, H, _ = shape
    print(f"\n  gate {(B, T, N, H)} mode={mode}")
    _gate_case(*_gate_inputs(B, T, N, H, bf=mode == "bf16"), bf=mode == "bf16")


@pytest.mark.parametrize("mode", [None, "f32s"])
@pytest.mark.parametrize("shape", SHAPES[:7])
def test_long_gate_against_the_unfused_oracle_tail(shape, mode, request):
    """The gate-fused form inside the module's arithmetic -- VW = sent W_l^T on the device, then scdm_gate_long -- against the UN-fused
    oracle tail sigmoid(linear(C, W_l, b_l)) * r with C = P @ sent: output and the gradients of every leaf (dVW shows in dsent and dW_l).
    (The 130-item shape is covered on projected operands above; here W_l's gradient would sum 5 200 word rows in a rocBLAS GEMM.)"""
    from shufflingvideosfortsg_amd import functional as F
    _mode(request, mode)
    B, T, N, d, _ = shape
    g = torch.Generator().manual_seed(24)
    a = torch.randn(B, T, d, generator=g).requires_grad_(True); r = torch.randn(B, T, d, generator=g).requires_grad_(True)
    s = torch.randn(B, N, d, generator=g).requires_grad_(True); sent = torch.randn(B, N, d, generator=g).requires_grad_(True)
    w = (torch.randn(d, generator=g) / d ** 0.5).requires_grad_(True)
    Wl = (torch.randn(d, d, generator=g) / d ** 0.5).requires_grad_(True); bl = (torch.randn(d, generator=g) * 0.1).requires_grad_(True)
    go = torch.randn(B, T, d, generator=g)
    leaves = (a, s, w, sent, Wl, bl, r)
    C0, _ = O.scdm_core(a, s, w, sent)
    out0 = torch.sigmoid(lin(C0, Wl, bl)) * r
    out0.backward(go)
    dev = [x.detach().cuda().requires_grad_(True) for x in leaves]
    ad, sd, wd, vd, Wd, bd, rd = dev
    out1 = F.scdm_gate_long(ad, sd, wd, lin(vd, Wd), bd, rd)
    out1.backward(go.cuda())
    torch.cuda.synchronize()
    print(f"\n  gate un-fused {(B, T, N, d)} mode={mode}: out max err {float((out1.cpu() - out0.detach()).abs().max()):.3e}")
    torch.testing.assert_close(out1.detach().cpu(), out0.detach(), **TOL)
    for got, want, name in zip(dev, leaves, "a s w sent W_l b_l r".split()):
        _grad_close(got.grad, want.grad, name)


@pytest.mark.parametrize("N", [31, 32, 33, 63, 64, 65, 96, 127, 128])
def test_long_chunk_boundaries(N, request):
    """Sentence lengths around the 16-word chunk, the 32-word routing limit, the softmax's second 64-lane half and NMAX, plain and
    gate-fused.  For N <= 32 the long entry points also run against the existing ones on the same inputs; the largest difference on
    P and C is printed (recorded in DESIGN 4.1a, not bounded: the two kernels sum in different orders)."""
    from shufflingvideosfortsg_amd import functional as F
    _mode(request, None)
    print(f"\n  chunk boundary N={N}")
    ins = _plain_inputs(2, 20, N, 128, 128, seed=N)
    C1, P1 = _plain_case(*ins, bf=False)
    _gate_case(*_gate_inputs(2, 20, N, 128, seed=100 + N), bf=False)
    if N <= 32:
        a, s, w, sent, _ = (x.cuda() for x in ins)
        C2, P2 = F.scdm_attn(a, s, w, sent, return_p=True)
        print(f"    long vs 32-word kernels at N={N}: max |dP| {float((P1 - P2).abs().max()):.3e}  max |dC| {float((C1 - C2).abs().max()):.3e}")


def _saturated(kind, B=2, T=16, N=40, H=64, seed=3):
    """(a, s, w) of a saturation case; a and s hold bf16-exact values where the case pins them."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(B, T, H, generator=g); s = torch.randn(B, N, H, generator=g); w = torch.randn(H, generator=g) / H ** 0.5
    if kind == "scale12":
        a, s = a * 12.0, s * 12.0
    elif kind == "scale30":
        a, s = a * 30.0, s * 30.0
    elif kind == "pinned":                       # rows pinned at a + s = +-40
        a[:, ::2] = 20.0; a[:, 1::2] = -20.0
        s[:, ::3] = 20.0; s[:, 1::3] = -20.0
    elif kind == "mixed":                        # mixed-sign extremes: a + s = 0 from +-30, and +-60 beside them
        sign = torch.where(torch.arange(H) % 2 == 0, 1.0, -1.0)
        a[:] = 30.0 * sign; a[:, 1::2] *= -1.0
        s[:] = -30.0 * sign; s[:, ::5] *= -1.0
    elif kind == "tiny_w":                       # weights of 0 and 1e-7
        w[::2] = 0.0; w[1::4] = 1e-7
        a, s = a * 12.0, s * 12.0
    elif kind == "equal":                        # every word the same: all scores equal, P = 1/N
        s[:] = s[:, :1].clone()
    return a, s, w


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["scale12", "scale30", "pinned", "mixed", "tiny_w", "equal"])
def test_long_saturation(kind, bf, request):
    """|a + s| far into tanh's flat part, in the plain and the gate-fused kernels: finite, and inside the unchanged tolerances.

    ``scale30`` (a, s ~ 30 N(0,1)) puts |a| or |s| ALONE beyond 40 in 18 % of the elements, where the product form exp(2a) exp(2s) with its
    separate clamps is no longer exact (a = 90, s = -90.3 would score as tanh(0)): the kernels switch to the sum form there (rcp_sum_form in
    csrc/scdm_long.hip).  Measured: max |dP| 4.5e-8 in fp32 (3.1e-2 before that path existed)."""
    _mode(request, None)
    print(f"\n  saturation {kind} bf16={bf}")
    B, T, N, H = 2, 16, 40, 64
    a, s, w = _saturated(kind)
    g = torch.Generator().manual_seed(9)
    sent = torch.randn(B, N, H, generator=g); gC = torch.randn(B, T, H, generator=g)
    r = torch.randn(B, T, H, generator=g); gb = torch.randn(H, generator=g) * 0.1
    if bf:
        a, s, sent, gC, r = _r(a), _r(s), _r(sent), _r(gC), _r(r)
    _, P = _plain_case(a, s, w, sent, gC, bf)
    if kind == "equal":
        torch.testing.assert_close(P, torch.full_like(P, 1.0 / N), atol=1e-6, rtol=1e-5)
    _gate_case(a, s, w, sent, gb, r, gC, bf)


@pytest.mark.parametrize("tag", ["n40", "n48"])
def test_long_modules_reproduce_the_reference(golden, tag):
    """SCDM_Attention and rnn_recalibration_layer with the weights of tests/golden/scdm_long.npz against the real reference's outputs and
    gradients at N = 40 and 48 (both routed to the long kernels)."""
    from shufflingvideosfortsg_amd.model.networks.attention import SCDM_Attention
    from shufflingvideosfortsg_amd.model.components.VideoEncoder import rnn_recalibration_layer
    g = golden("scdm_long")
    wts = g.group(f"{tag}.att.w.")
    H, Dv = wts["W_a.weight"].shape
    Ds = wts["W_s.weight"].shape[1]
    m = SCDM_Attention(Dv, Ds, H)
    m.load_state_dict(wts)
    m.cuda()
    v = g.t(f"{tag}.video").cuda().requires_grad_(True); s = g.t(f"{tag}.sent").cuda().requires_grad_(True)
    assert s.shape[1] > 32
    C = m(v, s)
    torch.testing.assert_close(C.cpu(), g.t(f"{tag}.C"), **TOL)
    C.backward(g.t(f"{tag}.gC").cuda())
    torch.testing.assert_close(v.grad.cpu(), g.t(f"{tag}.gvideo"), atol=3e-4, rtol=3e-3)
    torch.testing.assert_close(s.grad.cpu(), g.t(f"{tag}.gsent"), atol=3e-4, rtol=3e-3)
    for k, p in m.named_parameters():
        torch.testing.assert_close(p.grad.cpu(), g.group(f"{tag}.att.gw.")[k], atol=3e-4, rtol=3e-3, msg=lambda m_, k=k: f"att {k}: {m_}")
    rw = g.group(f"{tag}.rec.w.")
    h = rw["sent_linear.weight"].shape[0] // 2                 # visual_dim = 2 h
    rec = rnn_recalibration_layer(Dv, Ds, h, 2, "sigmoid", 0.0, LOG)
    rec.load_state_dict(rw)
    rec.cuda().train()
    rv = g.t(f"{tag}.rec.video").cuda().requires_grad_(True); rwd = g.t(f"{tag}.rec.word").cuda().requires_grad_(True)
    out = rec(rv, rwd)
    torch.testing.assert_close(out.cpu(), g.t(f"{tag}.rec.out"), **TOL)
    out.backward(g.t(f"{tag}.rec.g").cuda())
    torch.testing.assert_close(rv.grad.cpu(), g.t(f"{tag}.rec.gvideo"), atol=3e-4, rtol=3e-3)
    torch.testing.assert_close(rwd.grad.cpu(), g.t(f"{tag}.rec.gword"), atol=3e-4, rtol=3e-3)
    for k, p in rec.named_parameters():
        torch.testing.assert_close(p.grad.cpu(), g.group(f"{tag}.rec.gw.")[k], atol=3e-4, rtol=3e-3, msg=lambda m_, k=k: f"rec {k}: {m_}")


def _small_params(**over):
    from shufflingvideosfortsg_amd import engine
    p = dict(video_feature_dim=40, video_rnn_hiddendim=32, sent_rnn_hiddendim=32, dropout=0.0, video_len=36, sent_len=48,
             mlp_hidden_dim=24, m_pred_hidden=32)
    p.update(over)
    return engine.default_params(**p)


def _param_grads_close(model, sd):
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        torch.testing.assert_close(p.grad.cpu(), sd[k].grad, atol=3e-4, rtol=3e-3, msg=lambda m, k=k: f"grad {k}: {m}")


@pytest.mark.parametrize("gemm", [None, "f32s"])
def test_query_aware_encoder_at_48_words(gemm, request):
    from shufflingvideosfortsg_amd import engine
    from shufflingvideosfortsg_amd.model.components.VideoEncoder import QueryAwareEncoder
    engine.set_precision(gemm)
    request.addfinalizer(lambda: engine.set_precision(None))
    torch.manual_seed(0)
    vs = dict(name="query_aware_encoder", input_dim=40, rnn_hidden_dim=32, rnn_layers=2, rnn_cell="lstm", mask=False, drop_out=0.0, T=36,
              nblocks=2, query_dim=64)
    m = QueryAwareEncoder(vs, LOG)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    video = torch.randn(3, 36, 40, generator=g).requires_grad_(True); word = torch.randn(3, 48, 64, generator=g).requires_grad_(True)
    go = torch.randn(3, 36, 64, generator=g)
    ref = O.query_aware_encoder(video, word, sd)
    ref.backward(go)
    m.cuda().train()
    vd, wd = video.detach().cuda().requires_grad_(True), word.detach().cuda().requires_grad_(True)
    out = m(vd, wd)
    out.backward(go.cuda())
    torch.testing.assert_close(out.detach().cpu(), ref.detach(), **TOL)
    torch.testing.assert_close(vd.grad.cpu(), video.grad, atol=3e-4, rtol=3e-3)
    torch.testing.assert_close(wd.grad.cpu(), word.grad, atol=3e-4, rtol=3e-3)
    _param_grads_close(m, sd)


@pytest.mark.parametrize("gemm", [None, "f32s"])
@pytest.mark.parametrize("mask", [False, True], ids=["nomask", "mask"])
def test_baseline_at_sent_len_48(mask, gemm, request):
    """Baseline (QAVE) forward + span_ground_loss + backward at sent_len = 48 against O.baseline_forward: outputs, loss, every parameter gradient."""
    from shufflingvideosfortsg_amd import data, engine
    engine.set_precision(gemm)
    request.addfinalizer(lambda: engine.set_precision(None))
    params = _small_params(mask=mask)
    torch.manual_seed(0)
    model = engine.build_model("qave", params)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    b = data.synthetic_batch(3, 36, 48, video_dim=40, seed=11)
    ref = O.baseline_forward(sd, b["video"], b["query"], b["video_mask"], use_mask=mask)
    ref_loss = O.span_ground_loss(ref["start"], ref["end"], b["gt"]["framestps"])
    ref_loss.backward()
    model = model.cuda().train()
    d = data.synthetic_batch(3, 36, 48, video_dim=40, seed=11, device="cuda")
    loss, out = engine.baseline_step(model, d)
    loss.backward()
    torch.testing.assert_close(out["start"].detach().cpu(), ref["start"].detach(), **TOL)
    torch.testing.assert_close(out["end"].detach().cpu(), ref["end"].detach(), **TOL)
    torch.testing.assert_close(loss.detach().cpu(), ref_loss.detach(), **TOL)
    _param_grads_close(model, sd)


@pytest.mark.parametrize("gemm", [None, "f32s"])
def test_gmd_at_sent_len_48(gemm, request):
    """The full GMD step at sent_len = 48 against O.gmd_forward / O.gmd_losses: span scores, loss, every parameter gradient."""
    from shufflingvideosfortsg_amd import data, engine
    engine.set_precision(gemm)
    request.addfinalizer(lambda: engine.set_precision(None))
    params = _small_params()
    torch.manual_seed(0)
    model = engine.build_model("gmd", params)
    sd = {k: v.detach().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    b = data.synthetic_batch(3, 36, 48, video_dim=40, seed=7, pair=True)
    g, pg = b["gt"], b["pseudo_gt"]
    ref = O.gmd_forward(sd, b["query"], b["video"], b["video_mask"], b["pseudo_video"], b["video_mask"],
                        g["temporal_labels"], g["fore_masks"], g["back_masks"], pg["temporal_labels"], pg["fore_masks"], pg["back_masks"])
    ref_loss, _ = O.gmd_losses(ref, b["video_mask"], b["video_mask"], g, pg)
    ref_loss.backward()
    model = model.cuda().train()
    model.tod.dropout.p = 0.0
    d = data.synthetic_batch(3, 36, 48, video_dim=40, seed=7, pair=True, device="cuda")
    loss, _, span = engine.gmd_step(model, d, params)
    loss.backward()
    torch.testing.assert_close(span["start"].detach().cpu(), ref[0]["start"].detach(), **TOL)
    torch.testing.assert_close(span["end"].detach().cpu(), ref[0]["end"].detach(), **TOL)
    torch.testing.assert_close(loss.detach().cpu(), ref_loss.detach(), **TOL)
    _param_grads_close(model, sd)


def test_gmd_step_and_update_at_48_words_in_f32s_and_bf16():
    """One engine.gmd_step + optimizer step at [B=8, T=128, N=48, d=1024] in the f32s and the bf16 storage modes: finite loss and gradients,
    probabilities summing to 1, bf16 within the existing bf16-vs-f32s bound, no skipped update."""
    from shufflingvideosfortsg_amd import data, engine, functional as TF
    params = engine.default_params(video_rnn_hiddendim=512, sent_rnn_hiddendim=512, video_len=128, sent_len=48, dropout=0.0)
    torch.manual_seed(0)
    model = engine.build_model("gmd", params).cuda().train()
    for m_ in model.modules():
        if isinstance(m_, torch.nn.Dropout):
            m_.p = 0.0
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    batch = data.synthetic_batch(8, 128, 48, seed=5, pair=True, device="cuda")
    engine.skipped_updates(reset=True)
    outs = {}
    for md in ("f32s", "bf16"):
        model.load_state_dict(state)
        TF.invalidate_shadows(model)
        opt = engine.make_optimizer(model, params)
        b = dict(batch)
        if md == "bf16":
            b["video"] = batch["video"].to(BF); b["pseudo_video"] = batch["pseudo_video"].to(BF)
        model.zero_grad(set_to_none=True)
        with engine.precision(md):
            loss, _, span = engine.gmd_step(model, b, params)
            loss.backward()
            engine.optimizer_step(opt, loss)
        torch.cuda.synchronize()
        TF.check_kernel_errors()
        assert bool(torch.isfinite(loss)), md
        assert span["start"].dtype == torch.float32
        torch.testing.assert_close(span["start"].sum(1), torch.ones(8, device="cuda"), atol=1e-4, rtol=1e-4)
        torch.testing.assert_close(span["end"].sum(1), torch.ones(8, device="cuda"), atol=1e-4, rtol=1e-4)
        for k, p in model.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (md, k)
            assert bool(torch.isfinite(p).all()), (md, k)
        outs[md] = span["start"].detach().float().clone()
    torch.testing.assert_close(outs["bf16"], outs["f32s"], atol=1e-2, rtol=5e-2)
    assert engine.skipped_updates() == 0


@pytest.mark.parametrize("mode", ["bf16", "f32s"])
def test_graphed_train_step_replays_at_48_words(mode):
    """engine.GraphedTrainStep at N = 48 (dropout off, lr = 0): every replay reproduces the eager step's gradients within the bound of
    test_graph_replay_gradients_match_the_eager_step (2e-5 of the parameter's max |g|: the order of the float atomics in dw / dgbias)."""
    from shufflingvideosfortsg_amd import data, engine, functional as TF
    params = engine.default_params(video_rnn_hiddendim=512, sent_rnn_hiddendim=512, video_len=128, sent_len=48)
    params["dropout"] = 0.0
    params["lr"] = 0.0
    torch.manual_seed(0)
    model = engine.build_model("gmd", params).cuda().train()
    for m_ in model.modules():
        if isinstance(m_, torch.nn.Dropout):
            m_.p = 0.0
    batch = data.synthetic_batch(16, 128, 48, seed=1234, pair=True, device="cuda")
    engine.set_precision(mode)
    engine.skipped_updates(reset=True)
    try:
        step = lambda m, b: engine.gmd_step(m, b, params)[0]
        model.zero_grad(set_to_none=True)
        step(model, batch).backward()
        torch.cuda.synchronize()
        ref = {k: p.grad.detach().float().clone() for k, p in model.named_parameters() if p.grad is not None}
        model.zero_grad(set_to_none=True)
        opt = engine.make_optimizer(model, params, capturable=True)
        g = engine.GraphedTrainStep(model, opt, step, batch, warmup=3)
        rtol = 2e-5
        for it in range(20):
            loss = g()
            if it % 10 == 9:
                torch.cuda.synchronize()
                TF.check_kernel_errors()
                assert bool(torch.isfinite(loss))
                for k, p in model.named_parameters():
                    if k not in ref:
                        continue
                    a, b = p.grad.detach().float(), ref[k]
                    scale = float(b.abs().max())
                    err = float((a - b).abs().max())
                    assert err <= rtol * scale + 1e-7, f"replay {it}: gradient of {k} deviates from the eager step by {err:.3e} (max |g| = {scale:.3e})"
        assert engine.skipped_updates() == 0
    finally:
        engine.set_precision(None)


def test_long_errors():
    from shufflingvideosfortsg_amd import functional as F
    from shufflingvideosfortsg_amd.model.networks.attention import SCDM_Attention
    nmax = F.scdm_long_max_words()
    assert nmax >= 128
    m = SCDM_Attention(8, 8).cuda()
    with pytest.raises(RuntimeError, match=f"N={nmax + 1}"):
        m(torch.randn(1, 4, 8).cuda(), torch.randn(1, nmax + 1, 8).cuda())
    a = torch.randn(1, 4, 8); s = torch.randn(1, 40, 8); w = torch.randn(8); v = torch.randn(1, 40, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        F.scdm_attn_long(a, s, w, v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SCDM_Attention(8, 8)(a, v)
    with pytest.raises(RuntimeError, match="H=1028"):
        F.scdm_attn_long(torch.randn(1, 4, 1028).cuda(), torch.randn(1, 40, 1028).cuda(), torch.randn(1028).cuda(), torch.randn(1, 40, 8).cuda())
    # the 32-word functions keep their limit
    with pytest.raises(RuntimeError, match="N=40"):
        F.scdm_attn(a.cuda(), s.cuda(), w.cuda(), v.cuda())

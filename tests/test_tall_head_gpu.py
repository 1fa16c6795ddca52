"""The boundary head on TALL's fusion (tsg_boundary_head_tall_gemm, tsg_tall_bwd_combine, functional.boundary_head_tall_params) and on the
clips alone (functional.boundary_head_video_params), on the GPU in the f32s mode: the C entry points and the modules against the float64
reference of tests/tall_head_f64.py at the project's tolerances, and Baseline / GMD with ``cross_name`` 'c' and 'a' against
the same model on the torch path.

Shapes [B, T, Dv, Hm] are the smallest at which each mechanism can go wrong:
  [2, 32, 32, 256]    one chunk per segment of the virtual contraction; a 64-row tile spanning two items
  [8, 40, 96, 256]    three chunks per segment: the segment switch falls on the odd buffer; items cut the staging passes at odd rows
  [16, 20, 64, 256]   a 32-row MFMA tile over three items: the epilogue's slow branch and the loader's row -> item map
  [4, 64, 64, 512]    two N tiles per head: the ticket reduction
  plus one shape per row tile the entry point can choose (128, 64), derived from the CU count."""
import functools
import logging

import pytest
import torch

import tall_head_f64 as R

pytestmark = pytest.mark.gpu
P_TOL = dict(atol=1e-4, rtol=1e-4)              # probabilities
A_TOL = dict(atol=3e-4, rtol=2e-3)              # dx, dsent, dgate
SHAPES = [(2, 32, 32, 256), (8, 40, 96, 256), (16, 20, 64, 256), (4, 64, 64, 512)]
PAD = 64                                        # floats of NaN in front of and behind every output buffer


@pytest.fixture
def f32s(request):
    from shufflingvideosfortsg_amd import engine
    engine.set_precision("f32s")
    request.addfinalizer(lambda: engine.set_precision(None))


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def plan_tm(M, N, cus):
    """The row tile tsg_boundary_head_tall_gemm plans (csrc/gemm_f32s.hip: pick_tm over {128, 64})."""
    best = None
    for tm in (128, 64):
        if M % tm:
            continue
        tiles = (M // tm) * (N // 256)
        cost = -(-tiles // cus) * (17.0 + 0.22 * tm)
        if best is None or cost < best[0]:
            best = (cost, tm)
    return best[1]


def _tile_shapes():
    """-> [(B, T, Dv, Hm, planned tile)]: one full round of 128-row tiles where 64-row tiles would need two; and a shape 128 does not divide."""
    cus = _cus()
    return [(cus // 4 + 1, 128, 32, 256, 128), (3, 64, 32, 256, 64)]


@functools.lru_cache(maxsize=None)
def _case(B, T, d, Hm, kind, on):
    c = R.make_case(B, T, d, Hm, kind=kind, gate=on, mask=on)
    return c, R.concat_form(c)


def _nan_buf(n):
    full = torch.full((n + 2 * PAD,), float("nan"), device="cuda")
    return full, full[PAD:PAD + n]


def _pads_untouched(full, n):
    bits = full.view(torch.int32)
    want = torch.full((1,), float("nan"), device="cuda").view(torch.int32)
    return bool((bits[:PAD] == want).all()) and bool((bits[PAD + n:] == want).all())


def _run_entry(c, want_y):
    """tsg_boundary_head_tall_gemm through ctypes on the case's fp32 inputs -> (p_start, p_end, y or None), with the buffer checks."""
    from shufflingvideosfortsg_amd import _lib
    from shufflingvideosfortsg_amd._lib import ptr
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    v, s = c["video"].cuda().contiguous(), c["sent"].cuda().contiguous()
    B, T, d = v.shape
    Ws, We = c["p"]["start_mlp_1.weight"].cuda(), c["p"]["end_mlp_1.weight"].cuda()
    Hm = Ws.shape[0]
    M, J = B * T, 2 * Hm
    Wv = torch.cat([Ws[:, :d] + Ws[:, 3 * d:], We[:, :d] + We[:, 3 * d:]], 0).contiguous()
    Wbd = torch.cat([Ws[:, d:2 * d] + Ws[:, 3 * d:], We[:, d:2 * d] + We[:, 3 * d:]], 0)
    cs = (s @ Wbd.t()).contiguous()
    b1 = torch.cat([c["p"]["start_mlp_1.bias"], c["p"]["end_mlp_1.bias"]]).cuda()
    w2 = torch.cat([c["p"]["start_mlp_2.weight"].reshape(-1), c["p"]["end_mlp_2.weight"].reshape(-1)]).cuda()
    b2 = torch.cat([c["p"]["start_mlp_2.bias"], c["p"]["end_mlp_2.bias"]]).cuda()
    gate = c["gate"].cuda().contiguous() if c["gate"] is not None else None
    mask = c["mask"].cuda().to(torch.int32).contiguous() if c["mask"] is not None else None
    nb = int(lib.tsg_head_gemm_ws_bytes(M, J, 2))
    ws = torch.empty(max(nb, 16), device="cuda", dtype=torch.uint8)
    ps_f, ps = _nan_buf(M)
    pe_f, pe = _nan_buf(M)
    y_f, y = _nan_buf(M * J) if want_y else (None, None)
    rc = lib.tsg_boundary_head_tall_gemm(ptr(v), d, ptr(Wv), ptr(Ws) + 8 * d, ptr(We) + 8 * d, 4 * d, ptr(s), ptr(cs), ptr(b1), ptr(w2), ptr(b2),
                                         ptr(gate) if gate is not None else None, ptr(mask) if mask is not None else None,
                                         ptr(y) if want_y else None, ptr(ps), ptr(pe), ptr(ws), nb, B, T, Hm, d, st)
    assert rc == 0, lib.tsg_last_error()
    torch.cuda.synchronize()
    assert _pads_untouched(ps_f, M) and _pads_untouched(pe_f, M), "the entry point wrote outside p_start / p_end"
    assert bool(torch.isfinite(ps).all()) and bool(torch.isfinite(pe).all())
    if want_y:
        assert _pads_untouched(y_f, M * J), "the entry point wrote outside y"
        assert bool(torch.isfinite(y).all())
    return ps.view(B, T).cpu(), pe.view(B, T).cpu(), (y.view(B, T, J).cpu() if want_y else None)


def _check_probs(c, ref, ps, pe):
    B, T = ps.shape
    for got, key in ((ps, "start"), (pe, "end")):
        err = (got.double() - ref[key]).abs() / (1e-4 + 1e-4 * ref[key].abs())
        print(f"{key}: {float(err.max()):.3f} of the output tolerance")
        torch.testing.assert_close(got.double(), ref[key], **P_TOL)
        assert float((got.double().sum(1) - 1).abs().max()) <= T * 2.0 ** -23, "rows must sum to 1 within T ulp"
        if c["mask"] is not None:
            assert float(got[c["mask"] == 0].abs().max()) == 0.0, "masked positions must be exactly 0"


def _check_y(c, y):
    """y is the GEMM output in front of gate / cs / b1: against the float64 split form, 2e-5 x scale (the f32s product bound of DESIGN section 2)."""
    f = torch.float64
    v, s = c["video"].to(f), c["sent"].to(f)
    d = v.size(2)
    want = torch.cat([v @ (W[:, :d] + W[:, 3 * d:]).t() + (v * s.unsqueeze(1)) @ W[:, 2 * d:3 * d].t()
                      for W in (c["p"]["start_mlp_1.weight"].to(f), c["p"]["end_mlp_1.weight"].to(f))], 2)
    scale = float(want.abs().max())
    assert float((y.double() - want).abs().max()) <= 2e-5 * scale


@pytest.mark.parametrize("want_y", [True, False], ids=["y", "no_y"])
@pytest.mark.parametrize("on", [True, False], ids=["gate_mask", "plain"])
@pytest.mark.parametrize("B,T,d,Hm", SHAPES)
def test_entry_point_vs_float64(B, T, d, Hm, on, want_y):
    c, ref = _case(B, T, d, Hm, "tall", on)
    ps, pe, y = _run_entry(c, want_y)
    _check_probs(c, ref, ps, pe)
    if want_y:
        _check_y(c, y)


@pytest.mark.parametrize("which", [0, 1], ids=["tile128", "tile64"])
def test_entry_point_on_each_row_tile(which):
    B, T, d, Hm, tm = _tile_shapes()[which]
    assert plan_tm(B * T, 2 * Hm, _cus()) == tm, "this shape must plan the tile it is here for"
    c, ref = _case(B, T, d, Hm, "tall", True)
    ps, pe, y = _run_entry(c, True)
    _check_probs(c, ref, ps, pe)
    _check_y(c, y)


@pytest.mark.parametrize("B,T,D", [(3, 1, 4), (2, 37, 100), (5, 8, 256), (2, 64, 132)])
def test_tall_bwd_combine_vs_float64(B, T, D):
    from shufflingvideosfortsg_amd import _lib
    from shufflingvideosfortsg_amd._lib import ptr
    lib = _lib.load()
    g = torch.Generator().manual_seed(B * T + D)
    u, v, dv = (torch.randn(B, T, D, generator=g) for _ in range(3))
    s = torch.randn(B, D, generator=g)
    u_f, ud = _nan_buf(B * T * D)
    dv_f, dvd = _nan_buf(B * T * D)
    ds_f, dsd = _nan_buf(B * D)
    ud.copy_(u.reshape(-1)); dvd.copy_(dv.reshape(-1))
    vd, sd = v.cuda(), s.cuda()
    rc = lib.tsg_tall_bwd_combine(ptr(ud), ptr(vd), ptr(sd), ptr(dvd), ptr(dsd), B, T, D, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.tsg_last_error()
    torch.cuda.synchronize()
    assert _pads_untouched(u_f, B * T * D) and _pads_untouched(dv_f, B * T * D) and _pads_untouched(ds_f, B * D)
    f = torch.float64
    want_dv = dv.to(f) + u.to(f) * s.to(f).unsqueeze(1)
    want_ds = (u.to(f) * v.to(f)).sum(1)
    want_u = v.to(f) * s.to(f).unsqueeze(1)
    # fp32 arithmetic: one fma per element of dv (2 ulp of the larger term), one rounding for v * s, a T-term fp32 sum for ds
    torch.testing.assert_close(dvd.view(B, T, D).cpu().double(), want_dv, atol=2 ** -22 * float(want_dv.abs().max()), rtol=0)
    torch.testing.assert_close(ud.view(B, T, D).cpu().double(), want_u, atol=0, rtol=2 ** -23)
    bound = T * 2 ** -23 * float((u.to(f) * v.to(f)).abs().sum(1).max())
    assert float((dsd.view(B, D).cpu().double() - want_ds).abs().max()) <= bound
    assert torch.equal(vd.cpu(), v) and torch.equal(sd.cpu(), s)


def _grad_tol(want):
    return dict(atol=5e-4 * max(1.0, float(want.abs().max())), rtol=5e-3)


@pytest.mark.parametrize("kind", ["tall", "video"])
@pytest.mark.parametrize("on", [True, False], ids=["gate_mask", "plain"])
@pytest.mark.parametrize("B,T,d,Hm", SHAPES)
def test_predictor_fused_forms_vs_float64(B, T, d, Hm, on, kind, f32s):
    """MLP_predictor.forward_fused: forward under grad and under no_grad, every gradient."""
    from shufflingvideosfortsg_amd import functional as TF
    from shufflingvideosfortsg_amd.model.components.SpanPredictor import MLP_predictor
    c, ref = _case(B, T, d, Hm, kind, on)
    m = MLP_predictor(4 * d if kind == "tall" else d, Hm)
    m.load_state_dict(c["p"])
    m.cuda()
    assert m.fused_form(kind, B, T, d, d) == kind
    calls = []
    orig = TF._call
    TF._call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
    try:
        v = c["video"].cuda().requires_grad_(True)
        s = c["sent"].cuda().requires_grad_(True)
        g = c["gate"].cuda().requires_grad_(True) if on else None
        mk = c["mask"].cuda() if on else None
        ps, pe = m.forward_fused(kind, v, s, g, mk)
        ((ps * c["ct"][0].cuda()).sum() + (pe * c["ct"][1].cuda()).sum()).backward()
        with torch.no_grad():
            ps2, pe2 = m.forward_fused(kind, v.detach(), s.detach(), g.detach() if on else None, mk)
    finally:
        TF._call = orig
    torch.cuda.synchronize()
    entry = "tsg_boundary_head_tall_gemm" if kind == "tall" else "tsg_boundary_head_gemm"
    assert calls.count(entry) == 2 and "tsg_boundary_score_fwd" not in calls, calls
    assert (calls.count("tsg_tall_bwd_combine") == 1) == (kind == "tall")
    _check_probs(c, ref, ps.detach().cpu(), pe.detach().cpu())
    assert torch.equal(ps2, ps.detach()) and torch.equal(pe2, pe.detach()), "the no_grad launch (y never written) must give the same bits"
    torch.testing.assert_close(v.grad.cpu().double(), ref["g.video"], **A_TOL)
    if kind == "tall":
        torch.testing.assert_close(s.grad.cpu().double(), ref["g.sent"], **A_TOL)
    else:
        assert s.grad is None
    if on:
        torch.testing.assert_close(g.grad.cpu().double(), ref["g.gate"], **A_TOL)
    for k, prm in m.named_parameters():
        want = ref["gw." + k]
        torch.testing.assert_close(prm.grad.cpu().double(), want, **_grad_tol(want), msg=lambda t, k=k: f"d{k}: {t}")


def test_fused_heads_vs_golden(golden, f32s):
    """OnlyVideo + MLP_predictor (tsg_boundary_head_gemm with a zero sentence row) and TALL + MLP_predictor as the real reference ran them
    (tools/make_golden_tall_head.py)."""
    from shufflingvideosfortsg_amd.model.components.SpanPredictor import MLP_predictor
    for kind in ("video", "tall"):
        gd = golden("tall_head")
        v = gd.t("video").cuda().requires_grad_(True)
        s = gd.t("sent").cuda().requires_grad_(True)
        g = gd.t("gate").cuda().requires_grad_(True)
        m = MLP_predictor(v.size(2) * (4 if kind == "tall" else 1), 256)
        m.load_state_dict(gd.group(f"{kind}.w."))
        m.cuda()
        ps, pe = m.forward_fused(kind, v, s, g, gd.t("mask").cuda())
        ((ps * gd.t("ct_start").cuda()).sum() + (pe * gd.t("ct_end").cuda()).sum()).backward()
        torch.testing.assert_close(ps.detach().cpu(), gd.t(f"{kind}.start"), **P_TOL)
        torch.testing.assert_close(pe.detach().cpu(), gd.t(f"{kind}.end"), **P_TOL)
        torch.testing.assert_close(v.grad.cpu(), gd.t(f"{kind}.g.video"), **A_TOL)
        torch.testing.assert_close(g.grad.cpu(), gd.t(f"{kind}.g.gate"), **A_TOL)
        for k, prm in m.named_parameters():
            want = gd.t(f"{kind}.gw.{k}")
            torch.testing.assert_close(prm.grad.cpu(), want, **_grad_tol(want), msg=lambda t, k=k: f"{kind} d{k}: {t}")


# ---- Baseline / GMD with cross_name 'c' and 'a' ------------------------------------------------------------------------------------------
def _params(cross, **over):
    from shufflingvideosfortsg_amd import engine
    return engine.default_params(video_rnn_hiddendim=128, sent_rnn_hiddendim=128, mlp_hidden_dim=256, m_pred_hidden=256, dropout=0.0,
                                 video_feature_dim=256, video_len=32, sent_len=15, crossmodal=cross, **over)


def _model(kind, params):
    from shufflingvideosfortsg_amd import engine
    torch.manual_seed(0)
    m = engine.build_model(kind, params, logging.getLogger("t")).cuda().train()
    for m_ in m.modules():
        if isinstance(m_, torch.nn.Dropout):
            m_.p = 0.0
    return m


def _step(kind, model, batch, params):
    from shufflingvideosfortsg_amd import engine
    if kind == "gmd":
        loss, _, span = engine.gmd_step(model, batch, params)
    else:
        loss, span = engine.baseline_step(model, batch)
    return loss, span


@pytest.mark.parametrize("cross", ["c", "a"])
@pytest.mark.parametrize("kind", ["qave", "gmd"])
def test_models_fused_vs_torch_path(kind, cross):
    """The same model, the same batch: the f32s step (fused head: the CMI module is not called) against the step outside the f32s mode (the
    torch path: concat, gate, Linear, K3)."""
    from shufflingvideosfortsg_amd import data, engine, functional as TF
    params = _params(cross)
    model = _model(kind, params)
    assert model._fused_head
    batch = data.synthetic_batch(8, 32, 15, video_dim=256, seed=3, pair=(kind == "gmd"), device="cuda")
    res = {}
    for mode in (None, "f32s"):
        calls = []
        orig = TF._call
        TF._call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
        model.zero_grad(set_to_none=True)
        try:
            with engine.precision(mode):
                loss, span = _step(kind, model, batch, params)
            loss.backward()
        finally:
            TF._call = orig
        torch.cuda.synchronize()
        fused = "tsg_boundary_head_tall_gemm" if cross == "c" else "tsg_boundary_head_gemm"
        assert (fused in calls) == (mode == "f32s"), (mode, sorted(set(calls)))
        res[mode] = (loss.detach().double().cpu(), span["start"].detach().double().cpu(), span["end"].detach().double().cpu(),
                     {k: p.grad.detach().double().cpu() for k, p in model.named_parameters()})
    TF.check_kernel_errors()
    want, got = res[None], res["f32s"]
    torch.testing.assert_close(got[1], want[1], **P_TOL)
    torch.testing.assert_close(got[2], want[2], **P_TOL)
    torch.testing.assert_close(got[0], want[0], **P_TOL)
    assert set(got[3]) == set(want[3])
    for k, w in want[3].items():
        torch.testing.assert_close(got[3][k], w, **_grad_tol(w), msg=lambda t, k=k: f"{k}: {t}")


def test_f32s_step_never_builds_the_concat(monkeypatch, f32s):
    """TALL.forward replaced by a function that raises: the f32s GMD step still runs (forward and backward); outside the f32s mode it raises."""
    from shufflingvideosfortsg_amd import data, engine
    from shufflingvideosfortsg_amd.model.components import CrossModalInteraction as CMI
    params = _params("c")
    model = _model("gmd", params)
    batch = data.synthetic_batch(8, 32, 15, video_dim=256, seed=3, pair=True, device="cuda")

    def boom(self, *a):
        raise AssertionError("the [B,T,4d] concat was built")
    monkeypatch.setattr(CMI.TALL, "forward", boom)
    loss, _, span = engine.gmd_step(model, batch, params)
    loss.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    with engine.precision(None), pytest.raises(AssertionError, match="concat was built"):
        engine.gmd_step(model, batch, params)


def test_graph_replay_of_the_tall_step_equals_eager(f32s):
    """One replay of the captured 'c' GMD step (lr = 0: the parameters do not move) reproduces the eager step's gradients up to the order of the
    float atomics a few sums of the step use (the bound of tests/test_models_gpu.py::test_graph_replay_gradients_match_the_eager_step)."""
    from shufflingvideosfortsg_amd import data, engine, functional as TF
    params = _params("c", lr=0.0)
    model = _model("gmd", params)
    batch = data.synthetic_batch(8, 32, 15, video_dim=256, seed=3, pair=True, device="cuda")
    engine.skipped_updates(reset=True)
    step = lambda m, b: engine.gmd_step(m, b, params)[0]
    model.zero_grad(set_to_none=True)
    loss = step(model, batch)
    loss.backward()
    torch.cuda.synchronize()
    eager = float(loss.detach())
    ref = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    # the eager step's autograd state (the loss and its graph, .grad, AccumulateGrad nodes bound to the eager stream) is dropped before the
    # capture: kept alive it breaks the capture (HISTORY, round 3)
    del loss
    model.zero_grad(set_to_none=True)
    opt = engine.make_optimizer(model, params, capturable=True)
    g = engine.GraphedTrainStep(model, opt, step, batch, warmup=3)
    loss = g()
    torch.cuda.synchronize()
    TF.check_kernel_errors()
    assert abs(float(loss.detach()) - eager) <= 2e-6 * max(1.0, abs(eager))
    for k, p in model.named_parameters():
        if k in ref:
            scale = float(ref[k].abs().max())
            err = float((p.grad.detach() - ref[k]).abs().max())
            assert err <= 2e-5 * scale + 1e-7, f"{k}: {err:.3e} against max |g| = {scale:.3e}"
    assert engine.skipped_updates() == 0

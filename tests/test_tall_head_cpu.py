"""The boundary head on TALL's fusion and on the clips alone, without a GPU: the float64 reference against the real reference's recorded run
(tests/golden/tall_head.npz, tools/make_golden_tall_head.py), the split algebra the kernel uses against the concat form, the error budget of
the designed f32s arithmetic, the argument checks of the two new entry points, and the modules' choice of the fused form."""
import ctypes

import pytest
import torch

import tall_head_f64 as R


def _golden_case(golden, kind):
    g = golden("tall_head")
    c = dict(kind=kind, p=g.group(f"{kind}.w."), video=g.t("video"), sent=g.t("sent"), gate=g.t("gate"), mask=g.t("mask"),
             ct=(g.t("ct_start"), g.t("ct_end")))
    return g, c


@pytest.mark.parametrize("kind", ["tall", "video"])
def test_float64_reference_matches_the_recorded_reference(golden, kind):
    """The reference's own fp32 run (TALL / OnlyVideo + MLP_predictor, gate and mask as GMD applies them), outputs and every gradient, at
    2e-6 (+ 2e-6 of the tensor's largest entry: an fp32 run of a 128-term contraction)."""
    g, c = _golden_case(golden, kind)
    out = R.concat_form(c)
    keys = ["start", "end", "g.video", "g.gate"] + (["g.sent"] if kind == "tall" else []) + ["gw." + n for n in R.NAMES]
    assert set(k for k in g.a if k.startswith(kind + ".") and ".w." not in k) == {f"{kind}.{k}" for k in keys}
    for k in keys:
        want = g.t(f"{kind}.{k}").double()
        scale = max(1.0, float(want.abs().max()))
        torch.testing.assert_close(out[k], want, atol=2e-6 * scale, rtol=2e-6, msg=lambda s, k=k: f"{kind}.{k}: {s}")
    masked = c["mask"] == 0
    assert masked.any() and float(out["start"][masked].abs().max()) == 0.0


@pytest.mark.parametrize("B,T,d,Hm,gate,mask", [(2, 32, 32, 256, True, True), (4, 128, 1024, 256, True, False), (3, 7, 20, 16, False, True)])
def test_split_form_equals_concat_form(B, T, d, Hm, gate, mask):
    """W1 [v, s, v*s, v+s] = (W_a + W_d) v + W_c (v*s) + (W_b + W_d) s in float64: 1e-12 x the scale of the pre-activation."""
    c = R.make_case(B, T, d, Hm, gate=gate, mask=mask)
    f = torch.float64
    x = R.fuse("tall", c["video"].to(f), c["sent"].to(f))
    if gate:
        x = c["gate"].to(f).unsqueeze(2) * x
    z_ref = torch.cat([x @ c["p"][f"{n}_mlp_1.weight"].to(f).t() + c["p"][f"{n}_mlp_1.bias"].to(f) for n in ("start", "end")], 2)
    ps, pe, z = R.split_form(c)
    scale = float(z_ref.abs().max())
    assert float((z - z_ref).abs().max()) <= 1e-12 * scale
    ref = R.concat_form(c)
    assert float((ps - ref["start"]).abs().max()) <= 1e-12 and float((pe - ref["end"]).abs().max()) <= 1e-12


def test_designed_f32s_arithmetic_uses_at_most_half_the_output_tolerance():
    """fp32 W_a + W_d, fp32 v * s, bf16 hi / lo splits with three products, at [4,128,1024,Hm 256] with a gate of N(0,1) x 2: the
    probabilities must stay within half of the project's 1e-4 abs + 1e-4 rel of float64 (measured: about a tenth)."""
    c = R.make_case(4, 128, 1024, 256, gate=True, mask=True, gate_scale=2.0)
    ref = R.concat_form(c)
    ps, pe, _ = R.f32s_form(c)
    worst = 0.0
    for got, want in ((ps, ref["start"]), (pe, ref["end"])):
        worst = max(worst, float(((got - want).abs() / (1e-4 + 1e-4 * want.abs())).max()))
    print(f"designed f32s arithmetic: {worst:.3f} of the output tolerance")
    assert worst <= 0.5


@pytest.fixture(scope="module")
def lib():
    from shufflingvideosfortsg_amd import _lib, build
    build.build()
    return _lib.load()


def test_tall_gemm_argument_errors(lib):
    """tsg_boundary_head_tall_gemm returns before a launch on every bad argument (no device is touched)."""
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    B, T, Hm, K = 2, 32, 256, 32
    ws = lib.tsg_head_gemm_ws_bytes(B * T, 2 * Hm, 2)
    assert ws > 0

    def call(x=p, ldx=K, wv=p, wsc=p, wec=p, ldw=4 * K, sent=p, cs=p, b1=p, w2=p, b2=p, gate=None, mask=None, y=None, ps=p, pe=p, wsp=p,
             ws_bytes=ws, B=B, T=T, Hm=Hm, K=K):
        return lib.tsg_boundary_head_tall_gemm(x, ldx, wv, wsc, wec, ldw, sent, cs, b1, w2, b2, gate, mask, y, ps, pe, wsp, ws_bytes, B, T, Hm, K, None)
    for name in ("x", "wv", "wsc", "wec", "sent", "cs", "b1", "w2", "b2", "ps", "pe", "wsp"):
        assert call(**{name: None}) == -1, name
        assert b"NULL" in lib.tsg_last_error()
        assert call(**{name: p + 4}) == -3, name
    assert call(y=p + 8) == -3
    assert call(K=48, ldx=48, ldw=192) == -2, "Dv % 32"
    assert call(K=16, ldx=16, ldw=64) == -2, "Dv = 16: the virtual contraction 2 Dv = 32 is whole chunks, a segment is not"
    assert call(Hm=128) == -2 and call(Hm=384) == -2, "Hm % 256"
    assert call(B=3, T=21) == -2, "M % 64"
    assert call(B=0) == -2 and call(T=0) == -2 and call(B=1 << 16, T=128) == -2, "B T > 2^22"
    assert call(ldx=K - 4) == -3 and call(ldw=K - 4) == -3 and call(ldx=K + 2) == -3
    assert call(ws_bytes=ws - 1) == -2
    assert b"workspace" in lib.tsg_last_error()
    assert call(B=1, T=8256, ws_bytes=1 << 30) == -2, "T > 8192"
    # (M % T != 0 cannot be passed through this signature: the entry point forms M = B * T itself, as tsg_boundary_head_gemm does)


def test_tall_bwd_combine_argument_errors(lib):
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    for i in range(5):
        a = [p] * 5
        a[i] = None
        assert lib.tsg_tall_bwd_combine(*a, 2, 3, 4, None) == -1
        a[i] = p + 4
        assert lib.tsg_tall_bwd_combine(*a, 2, 3, 4, None) == -3
    for B, T, D in ((0, 3, 4), (2, 0, 4), (2, 3, 0), (2, 3, 6), (2, 3, -4)):
        assert lib.tsg_tall_bwd_combine(p, p, p, p, p, B, T, D, None) == -2, (B, T, D)


def test_modules_choose_the_fused_form_exactly_when_the_kernel_takes_the_shape():
    from shufflingvideosfortsg_amd import engine, functional as TF
    from shufflingvideosfortsg_amd.model.components import CrossModalInteraction as CMI
    from shufflingvideosfortsg_amd.model.components.SpanPredictor import MLP_predictor
    assert (CMI.OnlyVideo.kind, CMI.VideoSentenceConcat.kind, CMI.TALL.kind) == ("video", "vs", "tall")
    shapes = [(2, 32, 32, 256), (8, 40, 96, 256), (16, 20, 64, 256), (4, 64, 64, 512), (64, 128, 1024, 256),     # taken
              (2, 32, 16, 256), (2, 32, 48, 256), (2, 32, 32, 128), (3, 21, 32, 256), (1, 8256, 32, 256), (2, 32, 36, 256)]
    want = [True] * 5 + [False] * 6
    try:
        for mode in ("f32s", None, "bf16", torch.bfloat16):
            engine.set_precision(mode)
            for (B, T, d, Hm), ok in zip(shapes, want):
                ok = ok and mode == "f32s"
                assert TF.tall_head_ok(B, T, d, d, Hm) == ok, (mode, B, T, d, Hm)
                assert not TF.tall_head_ok(B, T, d, d + 32, Hm)
                m = MLP_predictor(4 * d, Hm)
                assert m.fused_form("tall", B, T, d, d) == ("tall" if ok else None), (mode, B, T, d, Hm)
                assert m.fused_form("tall", B, T, d, d + 32) is None
                mv = MLP_predictor(d, Hm)
                ok_v = TF.head_gemm_ok(B * T, 2 * Hm, d, T, Hm)
                assert mv.fused_form("video", B, T, d, d) == ("video" if ok_v else None)
                assert ok_v == (mode == "f32s" and d % 32 == 0 and Hm % 256 == 0 and (B * T) % 64 == 0 and T <= 8192)
    finally:
        engine.set_precision(None)
    # CPU tensors never reach a kernel: no fused form
    m = MLP_predictor(128, 256)
    assert m.forward_fused("tall", torch.zeros(2, 32, 32), torch.zeros(2, 32)) is None

"""K1 / K1g against float64 across operand magnitudes, on every kernel path (tests/scdm_f64.py; the arithmetic restated on the CPU:
tests/test_scdm_f64_cpu.py).

One case = one path at one small shape on one operand family, forward and backward, plain (``scdm_attn``) and gate-fused (``scdm_gate``);
sentences of more than 32 words through ``scdm_attn_long`` / ``scdm_gate_long``.  The contract under test is the one DESIGN 4.1 / 4.1a states:
up to 32 words the product form is exact while |a| <= 39 and |s| <= 39 (every family but ``scale30``); the long kernels switch to the sum form
beyond the clamp (``scale30`` is in contract there); outside the contract the only promise is "finite".

Bounds.  A quantity the kernels compute in fp32 arithmetic -- P in every mode; C / out and every gradient in strict fp32; the gradients in
f32s (its backward is the fp32 kernel); everything the long kernels compute in f32s (they have no matrix-pipe phase) -- is held elementwise to
``max(16 E32, 64 2^-24 S)`` against float64 (scdm_f64.rule), never looser than the tolerance tests/test_scdm_gpu.py has for the same tensor
(1e-4 on outputs, 2e-4 / 3e-4 x max(1, S) on plain / gate-fused gradients).  Matrix-pipe outputs of the f32s mode (C, out of
scdm_fwd_ws_kernel): 2e-5 S (tests/test_gemm_f32s_gpu.py).  bf16-stored tensors: ``_close`` of tests/test_bf16_storage_gpu.py.
No bound here is set by argument: all follow the rule.

Every measured error, bound and ratio is printed, one ``k1f64 | case | tensor error/bound=ratio ...`` line per case and form (``pytest -s``; the
lines of one run: profiles/k1_f64/errors.txt)."""
import pytest
import torch

import scdm_f64 as R
from test_bf16_storage_gpu import _close

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
OUT_TOL = 1e-4                      # tests/test_scdm_gpu.py TOL (its absolute part)
B0, T0 = 2, 20                      # two full 8-row sub-tiles and a ragged one of 4


def _lib():
    from shufflingvideosfortsg_amd import _lib
    return _lib.load()


def _set_mode(request, mode):
    from shufflingvideosfortsg_amd import engine
    engine.set_precision("f32s" if mode == "f32s" else None)       # bf16 storage is selected by the tensors' dtype
    request.addfinalizer(lambda: engine.set_precision(None))


class _Report:
    """collects (tensor, error, bound) of one case, prints them as one line, fails at the end with every tensor that exceeded its bound"""

    def __init__(self, tag):
        self.tag, self.bad, self.cells = tag, [], []

    def check(self, name, got, want, bound, how):
        got = got.detach().double().cpu()
        assert bool(torch.isfinite(got).all()), f"{self.tag} {name}: not finite"
        err = float((got - want).abs().max())
        self.cells.append(f"{name} {err:.2e}/{bound:.2e}={err / bound:.3f} {how}")
        if not err <= bound:
            self.bad.append(f"{name}: error {err:.3e} > bound {bound:.3e} ({how})")

    def bf16(self, name, got, want, tight=None):
        """a bf16-stored tensor (or dw / dgbias of the bf16 mode, tight = 2e-3): _close of tests/test_bf16_storage_gpu.py, unchanged"""
        assert bool(torch.isfinite(got.float()).all()), f"{self.tag} {name}: not finite"
        rel = tight if tight is not None else 1e-2
        atol = rel * max(1.0, float(want.abs().max()))
        err = float((got.detach().float().cpu() - want.float()).abs().max())
        self.cells.append(f"{name} {err:.2e}/{atol:.2e}={err / atol:.3f} bf16")
        try:
            _close(got.detach(), want.float(), name, tight=tight)
        except AssertionError as e:
            self.bad.append(str(e))

    def done(self):
        print(f"\nk1f64 | {self.tag} | " + " | ".join(self.cells))            # tensor error/bound=ratio kind-of-bound
        assert not self.bad, f"{self.tag}:\n  " + "\n  ".join(self.bad)


def _p_checks(rep, P, want_P, e32_P, N, kind):
    S = float(want_P.max())
    rep.check("P", P, want_P, min(R.rule(e32_P, S), OUT_TOL), "rule")
    rowsum = float((P.double().sum(-1) - 1.0).abs().max())
    assert rowsum <= N * 2.0 ** -23, f"{rep.tag}: a P row sums to 1 + {rowsum:.3e}"
    if kind == "equal":
        dev = float((P.double().cpu() - 1.0 / N).abs().max())
        assert dev <= R.FLOOR / N, f"{rep.tag}: equal words, P differs from 1/N by {dev:.3e}"


def _run_case(kind, N, H, Ds, mode, B=B0, T=T0, long=False, accuracy=True, note=""):
    """Plain and gate-fused forward + backward of one (family, shape, mode) against float64.  accuracy = False (operands outside the
    contract): finiteness and the row sums of P only."""
    from shufflingvideosfortsg_amd import functional as F
    bf = mode == "bf16"
    mm = mode == "f32s" and not long and H == Ds and Ds in (256, 512, 1024)        # C / out come off the matrix pipe (scdm_fwd_ws_kernel)
    fwd_plain, fwd_gate = (F.scdm_attn_long, F.scdm_gate_long) if long else (F.scdm_attn, F.scdm_gate)
    dev = (lambda x: x.to(BF).cuda().requires_grad_(True)) if bf else (lambda x: x.cuda().requires_grad_(True))
    par = lambda x: x.cuda().requires_grad_(True)
    for gate in (False, True):
        if gate and long and Ds != H:
            continue                                                               # (the long gate-fused kernels take Ds = H)
        tag = f"{'long' if long else 'k1'} {mode or 'fp32'} {'gate' if gate else 'plain'} [{B},{T},{N},{H},{Ds}] {kind}{note}"
        ins, want, e32 = R.truth(kind, B, T, N, H, Ds, bf=bf, gate=gate)
        rep = _Report(tag)
        a, s, V = dev(ins["a"]), dev(ins["s"]), dev(ins["V"])
        w = par(ins["w"])
        gC = ins["gC"].to(BF).cuda() if bf else ins["gC"].cuda()
        if gate:
            gb, r = par(ins["gbias"]), dev(ins["r"])
            out = fwd_gate(a, s, w, V, gb, r)
            with torch.no_grad():                                                  # P of the same operands (the gate-fused entry point keeps its own)
                _, P = fwd_plain(a.detach(), s.detach(), w.detach(), V.detach(), return_p=True)
            grads = dict(da=a, ds=s, dw=w, dV=V, dgbias=gb, dr=r)
            oname, gtol = "out", 3e-4
        else:
            out, P = fwd_plain(a, s, w, V, return_p=True)
            grads = dict(da=a, ds=s, dw=w, dV=V)
            oname, gtol = "C", 2e-4
        out.backward(gC)
        torch.cuda.synchronize()
        F.check_kernel_errors()
        assert P.dtype == torch.float32 and out.dtype == (BF if bf else torch.float32)
        for k, x in grads.items():
            assert x.grad is not None and bool(torch.isfinite(x.grad.float()).all()), f"{tag}: {k} not finite"
        assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(P).all()), f"{tag}: output not finite"
        if not accuracy:
            rowsum = float((P.double().sum(-1) - 1.0).abs().max())
            assert rowsum <= N * 2.0 ** -23, f"{tag}: a P row sums to 1 + {rowsum:.3e}"
            continue
        _p_checks(rep, P, want["P"], e32["P"], N, kind)
        S = float(want[oname].abs().max())
        if bf:
            rep.bf16(oname, out, want[oname])
        elif mm:
            rep.check(oname, out, want[oname], min(2e-5 * S, OUT_TOL), "2e-5S")
        else:
            rep.check(oname, out, want[oname], min(R.rule(e32[oname], S), OUT_TOL), "rule")
        for k, x in grads.items():
            S = float(want[k].abs().max())
            if bf:
                rep.bf16(k, x.grad, want[k], tight=2e-3 if k in ("dw", "dgbias") else None)
            else:
                rep.check(k, x.grad, want[k], min(R.rule(e32[k], S), gtol * max(1.0, S)), "rule")
        rep.done()


def _fused_ok(B, T, N, H, Ds):
    ok = int(_lib().tsg_scdm_bwd_fused_ok(B, T, N, H, Ds))
    print(f"\ntsg_scdm_bwd_fused_ok({B},{T},{N},{H},{Ds}) = {ok}")
    return ok


# ---- the 32-word kernels, automatic backward (the one-launch kernel: asserted) --------------------------------------------------------------
_LIMITED = ("scale12", "mixed", "edge")
CASES = []                                                         # (id, mode, N, H, Ds, families)
CASES += [(f"fp32-N{n}", None, n, 256, 256, R.FAMILIES) for n in (5, 20, 32)]                     # strict fp32: scdm_fwd_kernel
CASES += [("fp32-N32-H260-Ds516", None, 32, 260, 516, ("scale12", "edge"))]
CASES += [(f"f32s-N{n}", "f32s", n, 256, 256, R.FAMILIES) for n in (5,             # q-form, 4 + 4 waves (8 slots)
                                                                    12,            # q-form, 8 + 8 waves, one 32x32x16 k step
                                                                    20, 24,        # q-form, 8 + 8 waves, + the 32x32x8 step
                                                                    25, 26,        # triple form, fp32 tail words (XW = 1, 2)
                                                                    28, 32)]       # triple form, 4 + 4 waves, two k steps
CASES += [(f"f32s-N20-H{h}", "f32s", 20, h, h, _LIMITED) for h in (512, 1024)]                   # CT = 2, 4 (CT = 1 above)
CASES += [("f32s-N8-H64", "f32s", 8, 64, 64, R.FAMILIES)]                                         # a width the ws kernel does not take: VALU kernel
CASES += [(f"bf16-N{n}", "bf16", n, 256, 256, R.FAMILIES) for n in (5, 20, 25, 32)]              # bf16 storage: q-form / 8 + 8 at 28 slots / triple
PARAMS = [pytest.param(mode, N, H, Ds, kind, id=f"{cid}-{kind}") for cid, mode, N, H, Ds, kinds in CASES for kind in kinds]


@pytest.mark.parametrize("mode,N,H,Ds,kind", PARAMS)
def test_k1_f64(mode, N, H, Ds, kind, request):
    _set_mode(request, mode)
    assert _fused_ok(B0, T0, N, H, Ds) == 1, "the automatic backward of this shape is expected to be the one-launch kernel"
    _run_case(kind, N, H, Ds, mode)


@pytest.mark.parametrize("kind", ["scale12", "edge"])
@pytest.mark.parametrize("mode", ["f32s", "bf16"])
def test_k1_f64_full_grid(mode, kind, request):
    """64-row workgroups with a ragged last tile (T = 70 = 64 + 6; 260 tiles)."""
    _set_mode(request, mode)
    assert _fused_ok(130, 70, 20, 256, 256) == 1
    _run_case(kind, 20, 256, 256, mode, B=130, T=70)


@pytest.mark.parametrize("kind", R.FAMILIES)
@pytest.mark.parametrize("N", [5, 20, 32])
@pytest.mark.parametrize("bwd_mode", [1, 2], ids=["two-kernel", "fused-valu-rows"])
def test_k1_f64_backward_paths(bwd_mode, N, kind, request):
    """The backward's other two paths (tsg_scdm_bwd_mode 1: the two kernels; 2: one launch with the row phase on the VALU), strict fp32."""
    _set_mode(request, None)
    lib = _lib()
    prev = lib.tsg_scdm_bwd_mode(bwd_mode)
    try:
        assert _fused_ok(B0, T0, N, 256, 256) == (0 if bwd_mode == 1 else 1)
        _run_case(kind, N, 256, 256, None, note=f" bwd_mode={bwd_mode}")
    finally:
        lib.tsg_scdm_bwd_mode(prev)


# ---- the long kernels: scale30 is in contract (the sum form beyond the clamp) -----------------------------------------------------------------
@pytest.mark.parametrize("kind", R.ALL_FAMILIES)
@pytest.mark.parametrize("mode", [None, "f32s", "bf16"], ids=["fp32", "f32s", "bf16"])
@pytest.mark.parametrize("H", [256, 64])
@pytest.mark.parametrize("N", [33, 48])
def test_long_f64(N, H, mode, kind, request):
    _set_mode(request, mode)
    _run_case(kind, N, H, H, mode, long=True)


# ---- outside the contract -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [None, "f32s", "bf16"], ids=["fp32", "f32s", "bf16"])
def test_k1_beyond_the_clamp_is_finite(mode, request):
    """``scale30`` on the 32-word kernels: |a| or |s| alone exceeds the clamp in 18 % of the elements.  This is OUTSIDE the contract (DESIGN
    4.1a: the product form with separate clamps is exact only within them, and only the long kernels switch form), so nothing is asked of the
    accuracy: outputs and gradients are finite and the P rows sum to 1."""
    _set_mode(request, mode)
    _run_case("scale30", 20, 256, 256, mode, accuracy=False)

"""The f32s GEMMs against float64, per element, on every tile path (tests/gemm_f64.py; its arithmetic on the CPU: tests/test_gemm_f64_cpu.py).

One case = one entry point (tsg_gemm_f32s_ld, tsg_gemm_f32s_nn, tsg_gemm_f32s_nn_acc, tsg_match_head_gemm, tsg_boundary_head_gemm,
tsg_wgrad_f32s, tsg_wgrad_f32s_out2) at one shape on one operand family, through the C ABI on buffers the test owns: the output -- and its
padding when the row stride exceeds the row, and the padding of strided operands -- holds one NaN bit pattern before the launch; afterwards
every element of the result is finite and every padding element still holds that pattern, so a tile that is never written, or a store outside
the tile, fails.  The result is held to the two rules of gemm_f64: |Y - D| <= 64 2^-24 A per element against the designed value, and
max|Y - ref| <= 2e-5 max|ref| (not for ``cancel``).  Where rule 1 is exceeded, the library's fp32 product of the same operands is measured
against ref; only if ITS error is above 16 2^-24 A does the case get 4 x that error, and its line says so.  A bias joins D and, by magnitude, A.
tsg_gemm_f32s_nn_acc adds onto a random P: (Y - P) by rule 1 plus 2^-23 |P + D| for the fp32 add -- a tile visited twice leaves P + 2 D.
``perm`` (W = a permutation matrix): |Y[i, j] - (hi + lo)(x[i, pi(j)])| <= 2^-23 |x|: placement, row / column swaps, which plane was read.

Shapes come from the device's CU count through gemm_f64.plan (pick_tm, the placement test and the persistent walk restated); each case names
the plan it is there for and FAILS if the library would plan otherwise, and test_census_reaches_every_cell holds the case list to: row tiles of
64 / 128 / 256, both placement branches, one / two / three rounds, xcd_remap's ragged tail, 1..5 chunks, and head widths of 1..5 column tiles.

The heads: gemm_f64.head_logits / head_probs (the formula of include/tsg_hip.h on D, exact activations, the bound written out term by term
there); logits / probabilities bit-equal with ``y`` requested (workspace zeroed) and with y = NULL (workspace of 0xFF bytes); masked positions
exactly 0; rows summing to 1 within T 2^-23; ``y`` by the two rules.

Every measured error, bound and ratio is printed, one ``gemmf64 | entry path [M,N,K] family | tensor error/bound=ratio rule`` line per case
(``pytest -s``; the largest ratios of one run: profiles/gemm_f64/errors.txt).  Out of scope: tsg_gemm_bf16, tsg_wgrad_bf16, tsg_linear_fwd,
the heads' backward kernels, any timing."""
import pytest
import torch

import gemm_f64 as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
CUS = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
NAN_BITS = 0x7FC0BEEF                                   # a quiet NaN no arithmetic produces


def _lib():
    from shufflingvideosfortsg_amd import _lib
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc, tag):
    assert rc == 0, f"{tag}: rc={rc} {_lib().tsg_last_error()}"


def _p(t):
    return t.data_ptr() if t is not None else None


# ---- the launches (each through the C entry point) ---------------------------------------------------------------------------------------
def _gemm_nt(x, ldx, w, ldw, bias, y, ldy, M, N, K, tag):
    _ok(_lib().tsg_gemm_f32s_ld(_p(x), ldx, _p(w), ldw, _p(bias), _p(y), ldy, M, N, K, _st()), tag)
    torch.cuda.synchronize()


def _gemm_nn(x, ldx, w0, w1, kseg, ldw, bias, y, ldy, M, N, K, acc, tag):
    if acc:
        _ok(_lib().tsg_gemm_f32s_nn_acc(_p(x), ldx, _p(w0), _p(w1), kseg, ldw, _p(y), ldy, M, N, K, _st()), tag)
    else:
        _ok(_lib().tsg_gemm_f32s_nn(_p(x), ldx, _p(w0), _p(w1), kseg, ldw, _p(bias), _p(y), ldy, M, N, K, _st()), tag)
    torch.cuda.synchronize()


def _match(x, w, cs, w2, b2, y, logits, ws, M, T, N, K, act, tag):
    _ok(_lib().tsg_match_head_gemm(_p(x), K, _p(w), K, _p(cs), _p(w2), _p(b2), _p(y), _p(logits), _p(ws), ws.numel() * ws.element_size(),
                                   M, T, N, K, act, _st()), tag)
    torch.cuda.synchronize()


def _boundary(x, w_s, w_e, cs, b1, w2, b2, gate, mask, y, ps, pe, ws, Bn, T, Hm, K, tag):
    _ok(_lib().tsg_boundary_head_gemm(_p(x), K, _p(w_s), _p(w_e), K, _p(cs), _p(b1), _p(w2), _p(b2), _p(gate), _p(mask), _p(y), _p(ps), _p(pe),
                                      _p(ws), ws.numel() * ws.element_size(), Bn, T, Hm, K, _st()), tag)
    torch.cuda.synchronize()


def _head_ws_bytes(M, N, heads):
    return int(_lib().tsg_head_gemm_ws_bytes(M, N, heads))


def _wgrad_ws_bytes(M, N, K0, K1, groups):
    return int(_lib().tsg_wgrad_f32s_ws_bytes(M, N, K0, K1, groups))


def _wgrad(A, a_gs, B0, K0, B1, b1_gs, K1, shift, period, C, ldc, c_gs, C1, ldc1, c1_gs, ws, M, N, groups, tag):
    lib = _lib()
    nb = ws.numel() if ws is not None else 0
    ldb1 = B1.stride(0) if B1 is not None else 0
    if C1 is None:
        rc = lib.tsg_wgrad_f32s(_p(A), A.stride(0), a_gs, _p(B0), B0.stride(0), K0, _p(B1), ldb1, b1_gs, K1, shift, period,
                                _p(C), ldc, c_gs, _p(ws), nb, M, N, groups, _st())
    else:
        rc = lib.tsg_wgrad_f32s_out2(_p(A), A.stride(0), a_gs, _p(B0), B0.stride(0), K0, _p(B1), ldb1, b1_gs, K1, shift, period,
                                     _p(C), ldc, c_gs, _p(C1), ldc1, c1_gs, _p(ws), nb, M, N, groups, _st())
    _ok(rc, tag)
    torch.cuda.synchronize()


def _set_stream_k(mode):
    _lib().tsg_wgrad_set_stream_k(mode)


# ---- buffers the test owns -----------------------------------------------------------------------------------------------------------------
def _nan(rows, ld):
    """[rows, ld] fp32 holding NAN_BITS everywhere"""
    return torch.full((rows, ld), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def _strided(t, ld):
    """a copy of fp32 [r, c] t with row stride ld >= c, NAN_BITS in the padding: a kernel that reads past a row poisons its result"""
    if ld == t.shape[1]:
        return t.contiguous()
    buf = _nan(t.shape[0], ld)
    buf[:, :t.shape[1]] = t
    return buf


def _padding_intact(buf, n):
    return bool((buf.view(torch.int32)[..., n:] == NAN_BITS).all())


class _Report:
    """collects (tensor, error, bound, rule) of one case, prints them as one line, fails at the end with every cell above its bound"""

    def __init__(self, entry, path, shape, kind):
        self.tag = f"{entry} {path} [{','.join(str(s) for s in shape)}] {kind}"
        self.bad, self.cells = [], []

    def cell(self, name, err, bound, how):
        r = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        self.cells.append(f"{name} {err:.2e}/{bound:.2e}={r:.3f} {how}")
        if not r <= 1.0:
            self.bad.append(f"{name}: error {err:.3e} > bound {bound:.3e} ({how})")

    def elementwise(self, name, err, bound, how):
        """the cell shows the error and the bound at the element with the largest error / bound"""
        r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
        i = int(r.argmax())
        self.cell(name, float(err.reshape(-1)[i]), float(bound.reshape(-1)[i]), how)

    def require(self, cond, what):
        if not cond:
            self.bad.append(what)

    def done(self):
        print(f"\ngemmf64 | {self.tag} | " + " | ".join(self.cells))
        assert not self.bad, f"{self.tag}:\n  " + "\n  ".join(self.bad)


def _rules(rep, name, Y, ref, D, A, kind, lib_product=None, extra=None, rule2=True):
    """Y (fp32 view of the result) by rule 1 (elementwise against D; ``extra``: a further elementwise allowance) and rule 2 (against ref)"""
    rep.require(bool(torch.isfinite(Y).all()), f"{name}: an element of the result is not finite (never written?)")
    Y = torch.nan_to_num(Y.double(), nan=float("inf"), posinf=float("inf"), neginf=float("inf"))
    err = (Y - D).abs()
    bound = G.rule1(A) + (extra if extra is not None else 0.0)
    how = "rule1"
    if lib_product is not None and not bool((err <= bound).all()):
        el = G.ratio((lib_product().double() - ref).abs(), A)             # the library's fp32 product of the same operands, over A
        if el > G.LIB_OK:
            bound = 4.0 * el * A + (extra if extra is not None else 0.0)
            how = f"rule1-library-allowance(4x{el:.2e}A)"
    rep.elementwise(name, err, bound, how)
    if rule2 and kind != "cancel":
        rep.cell(name, float((Y - ref).abs().max()), G.RULE2 * float(ref.abs().max()), "rule2")


def _perm_check(rep, Y, X, N, K):
    hi, lo = G.split(X)
    pi = G.perm_of(N, K).to(X.device)
    want = (hi + lo)[:, pi]
    rep.elementwise("Y", (Y.double() - want).abs(), 2.0 ** -23 * X.double().abs()[:, pi], "perm")


# ---- the census -------------------------------------------------------------------------------------------------------------------------
CENSUS = set()
WANTED = ({("tm", t) for t in (64, 128, 256)} | {("branch", b) for b in "AB"} | {("rounds", r) for r in (1, 2, 3)} | {("tail", True)}
          | {("nk", n) for n in (1, 2, 3, 4, 5)} | {("tiles_h", n) for n in (1, 2, 3, 4, 5)}
          | {("head_tm", t) for t in (64, 128, 256)} | {("head_rounds", 2)} | {("nn_rounds", 2), ("nn_branch", "A"), ("nn_tail", True)})


def _note(M, N, K, prefix="", tm=None, tiles_h=None):
    p = G.plan(M, N, CUS, tm)
    if prefix == "":
        CENSUS.update({("tm", p["tm"]), ("branch", p["branch"]), ("rounds", p["rounds"]), ("tail", 0 < p["tail"] < p["tiles"]), ("nk", K // 32)})
    elif prefix == "head":
        CENSUS.update({("head_tm", p["tm"]), ("head_rounds", p["rounds"]), ("tiles_h", tiles_h)})
    else:
        CENSUS.update({("nn_rounds", p["rounds"]), ("nn_branch", p["branch"]), ("nn_tail", 0 < p["tail"] < p["tiles"])})
    return p


def _planned(case, got):
    """the plan the case is in the list for, or a loud failure"""
    for k, v in case.get("plan", {}).items():
        assert got[k] == v, f"{case}: the library plans {k} = {got[k]} on {CUS} CUs, the case is there for {v}"


# ---- tsg_gemm_f32s_ld ------------------------------------------------------------------------------------------------------------------------
c4, c8 = CUS // 4, CUS // 8
NT = []


def _nt(path, M, N, K, kinds, plan=None, **kw):
    NT.extend(dict(path=path, M=M, N=N, K=K, kind=k, plan=plan or {}, **kw) for k in kinds)


_nt("one-tile", 64, 256, 32, G.FAMILIES, dict(tm=64, tiles=1))
for K_ in (64, 96, 128, 160):                                                     # the tail pipelines: both buffer parities at the end
    _nt(f"tail-nk{K_ // 32}", 64, 256, K_, G.FAMILIES, dict(tm=64))
_nt("tm64-two-rounds-ragged", 64 * (c4 + 1), 1024, 64, G.FAMILIES, dict(tm=64, rounds=2, branch="B", tail=4))
_nt("long-k", 256, 256, 4096, G.FAMILIES, dict(tm=64))
_nt("tm128-ragged", 128 * (c8 + 1), 1024, 96, G.LARGE, dict(tm=128, rounds=1, branch="B", tail=4))
_nt("tm128-neighbours", 128 * c4, 1024, 96, G.LARGE, dict(tm=128, rounds=1, branch="A"))
_nt("tm128-three-rounds", 128 * 3 * c8, 2048, 32, G.LARGE, dict(tm=128, rounds=3, branch="A"))
_nt("tm256-ragged", 256 * (c8 + 1), 1024, 64, G.LARGE, dict(tm=256, rounds=1, branch="B", tail=4))
_nt("tm256-neighbours", 256 * c4, 1024, 64, G.LARGE, dict(tm=256, rounds=1, branch="A"))
_nt("tm256-two-rounds", 256 * c4, 2048, 64, G.LARGE, dict(tm=256, rounds=2, branch="A"))
for bias_ in (False, True):                                                       # strided operands and output, the padding untouched
    _nt("strides" + ("-bias" if bias_ else ""), 256, 512, 96, ("randn", "rows", "lomax", "perm"), dict(tm=64), ldx=96 + 32, ldw=96 + 64, ldy=512 + 64, bias=bias_)
for c_ in NT:
    _note(c_["M"], c_["N"], c_["K"])


def _id(c):
    return "-".join(str(c[k]) for k in ("path", "M", "N", "K", "kind") if k in c)


@pytest.mark.parametrize("case", [pytest.param(c, id=_id(c)) for c in NT])
def test_gemm_f32s(case):
    M, N, K, kind = case["M"], case["N"], case["K"], case["kind"]
    _planned(case, G.plan(M, N, CUS))
    t = G.truth(kind, M, N, K, DEV)
    rep = _Report("tsg_gemm_f32s_ld", case["path"], (M, N, K), kind)
    ldx, ldw, ldy = case.get("ldx", K), case.get("ldw", K), case.get("ldy", N)
    x, w = _strided(t["X"], ldx), _strided(t["W"], ldw)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(N)).to(DEV) * float(t["ref"].abs().mean()) if case.get("bias") else None
    y = _nan(M, ldy)
    _gemm_nt(x, ldx, w, ldw, bias, y, ldy, M, N, K, rep.tag)
    rep.require(_padding_intact(y, N), "the padding of y was written")
    ref, D, A = t["ref"], t["D"], t["A"]
    if bias is not None:
        ref, D, A = ref + bias.double(), D + bias.double(), A + bias.double().abs()
    _rules(rep, "Y", y[:, :N], ref, D, A, kind, lib_product=lambda: torch.mm(t["X"], t["W"].t()) + (bias if bias is not None else 0.0))
    if kind == "perm" and bias is None:
        _perm_check(rep, y[:, :N], t["X"], N, K)
    rep.done()


# ---- tsg_gemm_f32s_nn / _nn_acc -----------------------------------------------------------------------------------------------------------
NN = []


def _nn(path, M, N, K, kinds, plan=None, **kw):
    NN.extend(dict(path=path, M=M, N=N, K=K, kind=k, plan=plan or {}, **kw) for k in kinds)


for acc_ in (False, True):
    s_ = "-acc" if acc_ else ""
    _nn("one-tile" + s_, 256, 256, 32, G.LARGE, dict(tiles=1), acc=acc_)
    _nn("two-rounds" + s_, 256 * (c4 + 1), 1024, 64, G.LARGE, dict(rounds=2, branch="B", tail=4), acc=acc_)
_nn("column-slice", 512, 256, 96, G.LARGE, ldw=256 + 64, offset=32)
_nn("two-segments-32", 512, 256, 128, G.LARGE, ldw=256 + 64, offset=32, kseg=32)
_nn("two-segments-96", 512, 256, 128, G.LARGE, ldw=256 + 64, offset=32, kseg=96)
_nn("neighbours", 256 * c4, 1024, 64, G.LARGE, dict(rounds=1, branch="A"))
_nn("bias", 512, 256, 96, ("randn", "lomax"), bias=True, ldy=256 + 64)
for c_ in NN:
    _note(c_["M"], c_["N"], c_["K"], "nn", tm=256)


@pytest.mark.parametrize("case", [pytest.param(c, id=_id(c)) for c in NN])
def test_gemm_f32s_nn(case):
    """y = x w with w [K,N] contraction-major: as a column slice (row stride N + 64, offset 32), as two row segments in two allocations, with a
    bias, and accumulating onto P; without accumulation bit-equal to tsg_gemm_f32s_ld on the transposed weight (the same products in the same order)"""
    M, N, K, kind, acc = case["M"], case["N"], case["K"], case["kind"], case.get("acc", False)
    _planned(case, G.plan(M, N, CUS, tm=256))
    t = G.truth(kind, M, N, K, DEV)
    rep = _Report("tsg_gemm_f32s_nn_acc" if acc else "tsg_gemm_f32s_nn", case["path"], (M, N, K), kind)
    ldw, off, kseg, ldy = case.get("ldw", N), case.get("offset", 0), case.get("kseg", K), case.get("ldy", N)
    wt = t["W"].t()                                                                 # [K, N]
    wide = _nan(K, ldw)
    wide[:, off:off + N] = wt
    w0, w1 = wide[:, off:off + N], None
    if kseg < K:                                                                    # the second segment lives in another allocation
        other = _nan(K - kseg, ldw)
        other[:, off:off + N] = wt[kseg:]
        wide[kseg:] = _nan(K - kseg, ldw)                                           # ... and the first one's rows behind kseg are poison
        w1 = other[:, off:off + N]
    bias = torch.randn(N, generator=torch.Generator().manual_seed(N)).to(DEV) if case.get("bias") else None
    y = _nan(M, ldy)
    ref, D, A = t["ref"], t["D"], t["A"]
    if acc:
        P = torch.randn(M, N, generator=torch.Generator().manual_seed(M)).to(DEV) * float(ref.abs().mean())
        y[:, :N] = P
    _gemm_nn(t["X"], K, w0, w1, kseg, ldw, bias, y, ldy, M, N, K, acc, rep.tag)
    rep.require(_padding_intact(y, N), "the padding of y was written")
    if acc:
        rep.require(bool(torch.isfinite(y[:, :N]).all()), "Y: not finite")
        _rules(rep, "Y-P", (y[:, :N].double() - P.double()), ref, D, A, kind, extra=2.0 ** -23 * (P.double() + D).abs(), rule2=False,
               lib_product=lambda: torch.mm(t["X"], wt.contiguous()))
    else:
        if bias is not None:
            ref, D, A = ref + bias.double(), D + bias.double(), A + bias.double().abs()
        _rules(rep, "Y", y[:, :N], ref, D, A, kind, lib_product=lambda: torch.mm(t["X"], wt.contiguous()) + (bias if bias is not None else 0.0))
        if kind == "perm" and bias is None:
            _perm_check(rep, y[:, :N], t["X"], N, K)
        y_nt = _nan(M, N)
        _gemm_nt(t["X"], K, t["W"], K, bias, y_nt, N, M, N, K, rep.tag)
        rep.require(torch.equal(y[:, :N], y_nt), "not bit-equal to tsg_gemm_f32s_ld on the transposed weight")
    rep.done()


# ---- the heads as epilogues -----------------------------------------------------------------------------------------------------------------
MATCH, BOUNDARY = [], []
for act_ in G.ACTS:
    for kind_ in G.HEAD_FAMILIES:
        MATCH.append(dict(path="T20-per-row-cs", Bn=16, T=20, H=256, K=64, act=act_, kind=kind_, plan=dict(tm=64)))
        MATCH.append(dict(path="T100-three-tiles", Bn=16, T=100, H=768, K=96, act=act_, kind=kind_, plan=dict(tm=64)))
        MATCH.append(dict(path="T100-five-tiles", Bn=16, T=100, H=1280, K=32, act=act_, kind=kind_, plan=dict(tm=64)))
for act_, kind_ in (("relu", "randn"), ("tanh", "lomax"), ("sigmoid", "rows"), ("relu", "ones")):
    MATCH.append(dict(path="two-rounds-tickets", Bn=64, T=c4 + 1, H=1024, K=64, act=act_, kind=kind_, plan=dict(tm=64, rounds=2)))
for act_, kind_ in (("tanh", "randn"), ("relu", "rows")):
    MATCH.append(dict(path="tm128", Bn=c8 + 1, T=128, H=1024, K=32, act=act_, kind=kind_, plan=dict(tm=128)))
for act_, kind_ in (("relu", "randn"), ("sigmoid", "ones"), ("tanh", "lomax")):
    MATCH.append(dict(path="tm256", Bn=2 * c4, T=128, H=1024, K=64, act=act_, kind=kind_, plan=dict(tm=256)))
for Hm_ in (256, 512, 768):
    for gate_, mask_, kind_ in ((0, 0, "randn"), (0, 1, "randn"), (1, 0, "randn"), (1, 1, "randn"), (1, 1, "rows"), (1, 1, "ones"), (1, 1, "lomax")):
        BOUNDARY.append(dict(path="tm64", Bn=16, T=100, Hm=Hm_, K=64, gate=gate_, mask=mask_, kind=kind_, plan=dict(tm=64)))
for Hm_, Bn_ in ((256, 4 * c4), (512, 2 * c4), (768, c4)):                       # 256-row tiles need more than half a round of them
    for kind_ in ("randn", "lomax"):
        BOUNDARY.append(dict(path="tm256", Bn=Bn_, T=128, Hm=Hm_, K=32, gate=1, mask=1, kind=kind_, plan=dict(tm=256)))
for c_ in MATCH:
    _note(c_["Bn"] * c_["T"], c_["H"], c_["K"], "head", tiles_h=c_["H"] // 256)
for c_ in BOUNDARY:
    _note(c_["Bn"] * c_["T"], 2 * c_["Hm"], c_["K"], "head", tiles_h=c_["Hm"] // 256)


def _head_id(c):
    return "-".join(str(c[k]) if k in ("path", "act", "kind") else f"{k}{c[k]}"
                    for k in ("path", "Bn", "T", "H", "Hm", "K", "act", "gate", "mask", "kind") if k in c)


def _ws(nbytes, byte):
    return torch.full((max(nbytes, 16),), byte, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("case", [pytest.param(c, id=_head_id(c)) for c in MATCH])
def test_match_head_gemm(case):
    Bn, T, H, K, act, kind = (case[k] for k in ("Bn", "T", "H", "K", "act", "kind"))
    M = Bn * T
    _planned(case, G.plan(M, H, CUS))
    t = G.truth(kind, M, H, K, DEV)
    rep = _Report("tsg_match_head_gemm", f"{case['path']} {act}", (M, H, K), kind)
    cs, _, w2, b2 = (v.to(DEV) for v in G.head_extras(Bn, H, 1))
    nws = _head_ws_bytes(M, H, 1)
    y = _nan(M, H)
    runs = []
    for want_y, fill in ((True, 0), (False, 0xFF)):
        logits = _nan(1, M)
        _match(t["X"], t["W"], cs, w2, b2, y if want_y else None, logits, _ws(nws, fill), M, T, H, K, G.ACTS.index(act), rep.tag)
        runs.append(logits.reshape(M))
    rep.require(torch.equal(runs[0], runs[1]), "logits differ between y requested / workspace zeroed and y = NULL / workspace of 0xFF bytes")
    rep.require(bool(torch.isfinite(runs[0]).all()), "logits: not finite")
    rows = cs[torch.arange(M, device=DEV) // T]
    want, bound = G.head_logits(t["D"], t["A"], rows, torch.zeros(H, device=DEV), w2, float(b2[0]), None, act)
    rep.elementwise("logits", (torch.nan_to_num(runs[0].double(), nan=float("inf")) - want).abs(), bound, "head")
    _rules(rep, "y", y, t["ref"], t["D"], t["A"], kind, lib_product=lambda: torch.mm(t["X"], t["W"].t()))
    rep.done()


@pytest.mark.parametrize("case", [pytest.param(c, id=_head_id(c)) for c in BOUNDARY])
def test_boundary_head_gemm(case):
    Bn, T, Hm, K, kind = (case[k] for k in ("Bn", "T", "Hm", "K", "kind"))
    M, N = Bn * T, 2 * Hm
    _planned(case, G.plan(M, N, CUS))
    t = G.truth(kind, M, N, K, DEV)
    rep = _Report("tsg_boundary_head_gemm", f"{case['path']} gate={case['gate']} mask={case['mask']}", (M, N, K), kind)
    cs, b1, w2, b2 = (v.to(DEV) for v in G.head_extras(Bn, N, 2))
    g = torch.Generator().manual_seed(M + Hm)
    gate = torch.randn(M, generator=g).to(DEV) if case["gate"] else None
    mask = None
    if case["mask"]:
        n = torch.randint(max(1, T // 2), T + 1, (Bn,), generator=g)
        mask = (torch.arange(T)[None, :] < n[:, None]).int().reshape(M).to(DEV)
    w_s, w_e = t["W"][:Hm].clone(), t["W"][Hm:].clone()                             # the two heads' first Linears, two allocations
    nws = _head_ws_bytes(M, N, 2)
    y = _nan(M, N)
    runs = []
    for want_y, fill in ((True, 0), (False, 0xFF)):
        ps, pe = _nan(Bn, T), _nan(Bn, T)
        _boundary(t["X"], w_s, w_e, cs, b1, w2, b2, gate, mask, y if want_y else None, ps, pe, _ws(nws, fill), Bn, T, Hm, K, rep.tag)
        runs.append((ps, pe))
    rows = cs[torch.arange(M, device=DEV) // T]
    for h, name in ((0, "p_start"), (1, "p_end")):
        got = runs[0][h]
        rep.require(torch.equal(got, runs[1][h]), f"{name} differs between y requested / workspace zeroed and y = NULL / workspace of 0xFF bytes")
        rep.require(bool(torch.isfinite(got).all()), f"{name}: not finite")
        sl = slice(h * Hm, (h + 1) * Hm)
        logit, lb = G.head_logits(t["D"][:, sl], t["A"][:, sl], rows[:, sl], b1[sl], w2[sl], float(b2[h]), gate, "tanh")
        want, bound = G.head_probs(logit, lb, mask, T)
        rep.elementwise(name, (torch.nan_to_num(got.double(), nan=float("inf")) - want).abs(), bound, "head-softmax")
        if mask is not None:
            rep.require(float(got.reshape(M)[mask == 0].abs().max()) == 0.0, f"{name}: a masked position has a non-zero probability")
        rep.cell(name + ".sum", float((got.double().sum(1) - 1.0).abs().max()), T * 2.0 ** -23, "rows-sum-to-1")
    _rules(rep, "y", y, t["ref"], t["D"], t["A"], kind, lib_product=lambda: torch.mm(t["X"], t["W"].t()))
    rep.done()


def test_census_reaches_every_cell():
    """the case lists above, planned for THIS device: a changed cost model or CU count that empties a cell fails here instead of testing less"""
    missing = sorted(WANTED - CENSUS, key=str)
    assert not missing, f"no case reaches {missing} on {CUS} CUs"
    assert G.plan(64 * (c4 + 1), 1024, CUS)["rounds"] == 2 and G.plan(256 * (c4 + 1), 1024, CUS, tm=256)["rounds"] == 2


# ---- tsg_wgrad_f32s / _out2 ------------------------------------------------------------------------------------------------------------------
WGRAD = []
for kind_ in G.WGRAD_FAMILIES:
    WGRAD.append(dict(path="one-range", M=32, N=256, K=128, kind=kind_))
    WGRAD.append(dict(path="row-ranges-reduce", M=2560, N=1024, K=1024, kind=kind_, ws=True))
    WGRAD.append(dict(path="long-m", M=16384, N=256, K=128, kind=kind_, ws=True))
    WGRAD.append(dict(path="stream-k-two-contributors", M=512, N=2048, K=2048, kind=kind_, sk=1, ws=True))
    WGRAD.append(dict(path="stream-k-ragged", M=1056, N=1536, K=3072, kind=kind_, sk=1, ws=True))


def _wgrad_id(c):
    return "-".join(str(c[k]) for k in ("path", "M", "N", "K", "Bn", "T", "layout", "out2", "kind") if k in c)


@pytest.mark.parametrize("case", [pytest.param(c, id=_wgrad_id(c)) for c in WGRAD])
def test_wgrad_f32s(case, request):
    """C[n][k] = sum_m A[m][n] B[m][k]: one row range, row ranges + the reduce launch, a long contraction, stream-K (switched on for fp32 operands,
    restored afterwards); C (row stride K + 32) and the workspace full of NaN before the launch"""
    M, N, K, kind = case["M"], case["N"], case["K"], case["kind"]
    rep = _Report("tsg_wgrad_f32s", case["path"], (M, N, K), kind)
    if "sk" in case:
        request.addfinalizer(lambda: _set_stream_k(-1))
        _set_stream_k(0)
        nb_ranges = _wgrad_ws_bytes(M, N, K, 0, 1)
        _set_stream_k(case["sk"])
        assert _wgrad_ws_bytes(M, N, K, 0, 1) != nb_ranges, f"{rep.tag}: the plan with stream-K switched on is that of the row ranges: not a stream-K shape"
    A_, B_ = (v.to(DEV) for v in G.family_wgrad(kind, M, N, K))
    nb = _wgrad_ws_bytes(M, N, K, 0, 1)
    assert (nb > 0) == bool(case.get("ws")), f"{rep.tag}: workspace of {nb} bytes: another scheme than the case is there for"
    ldc = K + 32
    C = _nan(N, ldc)
    _wgrad(A_, 0, B_, K, None, 0, 0, 0, 0, C, ldc, N * ldc, None, 0, 0, _ws(nb, 0xFF) if nb else None, M, N, 1, rep.tag)
    rep.require(_padding_intact(C, K), "the padding of C was written")
    ref, D, A = G.products(A_.t(), B_)
    _rules(rep, "C", C[:, :K], ref, D, A, kind, lib_product=lambda: torch.mm(A_.t(), B_))
    rep.done()


LSTM = []
for Bn_, T_ in ((4, 40), (4, 64)):
    for layout_ in ("batch-major", "time-major"):
        for out2_ in (0, 1):
            for kind_ in (("randn", "ones", "lomax") if not out2_ else ("randn",)):
                LSTM.append(dict(path="shifted-segment", Bn=Bn_, T=T_, layout=layout_, out2=out2_, kind=kind_))


@pytest.mark.parametrize("case", [pytest.param(c, id=_wgrad_id(c)) for c in LSTM])
def test_wgrad_f32s_lstm_operands(case):
    """Two groups, B = [x | h_(t-1)] / [x | h_(t+1)] read from ``out`` with a row shift, in both sequence layouts, with sequence lengths that are
    whole chunks (64) and that are not (40: chunks straddle sequences), to one output and to two (tsg_wgrad_f32s_out2)"""
    Bn, T, kind = case["Bn"], case["T"], case["kind"]
    I = h = 128
    M, N = Bn * T, 4 * h
    bm = case["layout"] == "batch-major"
    rep = _Report("tsg_wgrad_f32s_out2" if case["out2"] else "tsg_wgrad_f32s", f"shifted {case['layout']}", (M, N, I + h), kind)
    dG, Bfull = (v.to(DEV) for v in G.family_wgrad(kind, M, 2 * N, I + 2 * h))
    x, out = Bfull[:, :I].contiguous(), Bfull[:, I:].contiguous()
    shift, period = (1, T) if bm else (Bn, 0)
    nb = _wgrad_ws_bytes(M, N, I, h, 2)
    ws = _ws(nb, 0xFF) if nb else None
    if case["out2"]:
        C0, C1 = _nan(2 * N, I + 32), _nan(2 * N, h + 32)
        _wgrad(dG, N, x, I, out, h, h, shift, period, C0, I + 32, N * (I + 32), C1, h + 32, N * (h + 32), ws, M, N, 2, rep.tag)
        rep.require(_padding_intact(C0, I) and _padding_intact(C1, h), "the padding of C / C1 was written")
        got = torch.cat([C0[:, :I], C1[:, :h]], 1).view(2, N, I + h)
    else:
        ldc = I + h + 32
        C = _nan(2 * N, ldc)
        _wgrad(dG, N, x, I, out, h, h, shift, period, C, ldc, N * ldc, None, 0, 0, ws, M, N, 2, rep.tag)
        rep.require(_padding_intact(C, I + h), "the padding of C was written")
        got = C[:, :I + h].view(2, N, I + h)
    o3 = out.view(Bn, T, 2 * h) if bm else out.view(T, Bn, 2 * h)
    prev, nxt = torch.zeros_like(o3), torch.zeros_like(o3)
    if bm:
        prev[:, 1:] = o3[:, :-1]; nxt[:, :-1] = o3[:, 1:]
    else:
        prev[1:] = o3[:-1]; nxt[:-1] = o3[1:]
    for d, hs in ((0, prev.reshape(M, 2 * h)[:, :h]), (1, nxt.reshape(M, 2 * h)[:, h:])):
        Ad, Bd = dG[:, d * N:(d + 1) * N], torch.cat([x, hs], 1)
        ref, D, A = G.products(Ad.t(), Bd)
        _rules(rep, f"C[{d}]", got[d], ref, D, A, kind, lib_product=lambda: torch.mm(Ad.t().contiguous(), Bd))
    rep.done()

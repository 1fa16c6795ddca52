"""The BiLSTM recurrence against float64 across gate magnitudes, on every kernel path (tests/lstm_f64.py; the arithmetic restated on the CPU:
tests/test_lstm_f64_cpu.py).

One case = one path at one small shape on one operand family, through the C ABI (tsg_lstm_fwd_ws / tsg_lstm_fwd_bias, tsg_lstm_bwd_ws_layout /
tsg_lstm_bwd): the forward's out, R (activated gates, order i, f, g, o) and Cs, then the backward TWICE from the forward's own saved state --
without dHn and with it -- for dG and dbias (the persistent backward's fused sum, or dG.sum on the step kernels).  dHn is the gradient of each
direction's last hidden state: it joins at t = T-1 for the forward direction and at t = 0 for the reverse one.  Paths are selected with
tsg_lstm_set_persist / _ring / _wide (restored afterwards) and with B (the 16-unit workgroups); every launch's error words must be 0, and the
arrival counter of the start barrier (sync word 1: 2 directions x 16-row slices x workgroups per slice, of the last chunk) must be that of the
intended kernel -- a case whose path the library did not take FAILS.

Bounds.  fp32 arithmetic (TSG_F32 everywhere; TSG_F32S on the step kernels and at hidden sizes off the split path): elementwise
``max(16 E32, 64 2^-24 max(1, S))`` against float64 (lstm_f64.rule), never looser than TOL of tests/test_lstm_gpu.py.  f32s (persistent kernels,
h in {128, 256, 384, 512}): 2e-5 max(1, S) on all five tensors, end to end from its own forward.  bf16 storage: out, R, Cs by
``_close`` of tests/test_bf16_storage_gpu.py at rel = 1e-2; dG and dbias by ``_close`` at rel = min(5e-2, max(1e-2, 3 EBF / max(1, S))), EBF = the
error against float64 of the designed roundings alone (lstm_f64.emulate_bf16; 3: rounding ties that fall the other way; 5e-2: the bound of
test_bilstm_bf16_storage).  ``beyond`` is outside the contract: finite, nothing more.

Every measured error, bound and ratio is printed, one ``lstmf64 | case | tensor error/bound=ratio ...`` line per case (``pytest -s``; the lines of
one run: profiles/lstm_f64/errors.txt)."""
import pytest
import torch

import lstm_f64 as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DT = {"fp32": 0, "bf16": 1, "f32s": 2}                # TSG_F32, TSG_BF16, TSG_F32S
B0, T0 = 20, 12                                        # one full 16-row slice and a ragged one of 4; persistent, six ring generations of the backward
STALE = (0x3f800000, 0x3f800001)                       # 1.0f with the even / the odd generation tag of the backward's ring


def _lib():
    from shufflingvideosfortsg_amd import _lib
    return _lib.load()


class _Report:
    """collects (tensor, error, bound) of one case, prints them as one line, fails at the end with every tensor that exceeded its bound"""

    def __init__(self, tag):
        self.tag, self.bad, self.cells = tag, [], []

    def finite(self, name, got):
        assert bool(torch.isfinite(got.float()).all()), f"{self.tag} {name}: not finite"

    def check(self, name, got, want, bound, how):
        """bound: a number or an elementwise tensor; the cell shows the largest error / bound, with the error and the bound at that element"""
        self.finite(name, got)
        err = (got.detach().double().cpu().reshape(want.shape) - want).abs()
        ratio = err / bound
        i = int(ratio.argmax())
        e = float(err.reshape(-1)[i]); b = float(bound.reshape(-1)[i]) if torch.is_tensor(bound) else float(bound)
        self.cells.append(f"{name} {e:.2e}/{b:.2e}={e / b:.3f} {how}")
        if not bool((err <= bound).all()):
            self.bad.append(f"{name}: error {e:.3e} > bound {b:.3e} ({how})")

    def done(self):
        print(f"\nlstmf64 | {self.tag} | " + " | ".join(self.cells))            # tensor error/bound=ratio kind-of-bound
        assert not self.bad, f"{self.tag}:\n  " + "\n  ".join(self.bad)


def _switches(request, persist, ring=-1, wide=-1):
    lib = _lib()
    request.addfinalizer(lambda: (lib.tsg_lstm_set_persist(-1), lib.tsg_lstm_set_ring(-1), lib.tsg_lstm_set_wide(-1)))
    lib.tsg_lstm_set_persist(persist); lib.tsg_lstm_set_ring(ring); lib.tsg_lstm_set_wide(wide)
    return lib


def _last_chunk(B, wgs, per_cu=1):
    """(16-row slices of the last launch, launches) of a persistent layer of B rows with `wgs` workgroups per (direction, slice): csrc/lstm.hip
    persist_chunk_rows with one (16-unit workgroups: two) workgroup per CU"""
    cap = torch.cuda.get_device_properties(0).multi_processor_count * per_cu
    max_slices = cap // (2 * wgs)
    assert max_slices > 0
    slices = -(-B // 16)
    chunks = -(-slices // max_slices)
    rows = -(-slices // chunks) * 16
    return -(-(B - (B - 1) // rows * rows) // 16), chunks


def _check_mode(rep, name, got, want, e32, ebf, arith, grad):
    if arith == "fp32":
        rep.check(name, got, want, R.bound_fp32(e32, want), f"rule(E32 {e32:.1e})")
    elif arith == "f32s":
        rep.check(name, got, want, 2e-5 * max(1.0, float(want.abs().max())), "2e-5S")
    elif not grad:
        rep.check(name, got, want, R.bound_close(want, 1e-2), "bf16")
    else:
        rel = min(5e-2, max(1e-2, 3.0 * ebf / max(1.0, float(want.abs().max()))))
        rep.check(name, got, want, R.bound_close(want, rel), f"bf16 rel {rel:.2e} (EBF {ebf:.2e})")


def _forward(lib, path, dev, B, T, h, dt, bm, ring, tag):
    """-> (out, R, Cs) of one forward through the path's entry point; error word and arrival counter asserted"""
    from shufflingvideosfortsg_amd._lib import ptr
    st = torch.cuda.current_stream().cuda_stream
    seq = BF if dt == 1 else torch.float32
    out = torch.full((B, T, 2 * h) if bm else (T, B, 2 * h), 9.0, device="cuda", dtype=seq)
    Rg = torch.full((T, 2, B, h, 4), float("nan"), device="cuda", dtype=seq); Cs = torch.full((T, 2, B, h), float("nan"), device="cuda")
    if path in ("persist", "wide"):                        # workspace with room for the exchange ring, full of stale data
        nws = lib.tsg_lstm_fwd_ws_bytes(B, T, h)
        assert nws > 2048, f"{tag}: no ring workspace for this hidden size"
        ws = torch.full((nws // 4,), STALE[0], dtype=torch.int32, device="cuda")
        rc = lib.tsg_lstm_fwd_ws(ptr(dev["Gx"]), None, ptr(dev["W"]), ptr(out), ptr(Rg), ptr(Cs), ptr(ws), nws, B, T, h, dt, bm, st)
    else:                                                  # step kernels / the generic persistent kernel: the sync words only
        ws = torch.zeros(512, dtype=torch.int32, device="cuda")
        rc = lib.tsg_lstm_fwd_bias(ptr(dev["Gx"]), None, ptr(dev["W"]), ptr(out), ptr(Rg), ptr(Cs), ptr(ws), B, T, h, dt, bm, st)
    assert rc == 0, f"{tag}: {lib.tsg_last_error()}"
    torch.cuda.synchronize()
    assert int(ws[0]) == 0, f"{tag}: the forward's bounded wait expired"
    if path == "step":
        want_arrivals = 0                                  # no persistent launch touched the sync words
    else:
        nw4 = path == "persist" and B <= 32 and h == 512 and (dt == 2 or (dt == 1 and ring == 1))        # 16-unit workgroups (csrc/lstm.hip)
        wgs = h // 64 if path == "wide" else h // 16 if nw4 else h // 32
        last, _ = _last_chunk(B, wgs, 2 if nw4 else 1)
        want_arrivals = 2 * last * wgs
    assert int(ws[1]) == want_arrivals, f"{tag}: {int(ws[1])} workgroups arrived at the forward's start barrier, {want_arrivals} expected: another kernel ran"
    return out, Rg, Cs


def _backward(lib, persistent, dev, saved, hn, B, T, h, dt, bm, tag, ws=None):
    """-> (dG, dbias [2,4h]) of one backward from the forward's saved state; persistent: tsg_lstm_bwd_ws_layout with the ring workspace (path and
    error word asserted, dbias fused), else the step kernels (tsg_lstm_bwd, or _layout without a workspace for the batch-major layout)"""
    from shufflingvideosfortsg_amd._lib import ptr
    st = torch.cuda.current_stream().cuda_stream
    Rg, Cs = saved
    dG = torch.full_like(dev["Gx"], float("nan")); dC = torch.zeros(2, B, h, device="cuda")
    nb = lib.tsg_lstm_bwd_ws_bytes(B, T, h)
    hp = ptr(hn) if hn is not None else None
    if persistent:
        assert nb > 0 and lib.tsg_lstm_bwd_ws_persistent(B, T, h, nb) == 1, f"{tag}: the persistent backward does not take this shape"
        if ws is None:
            ws = torch.zeros(nb // 4 + 4, dtype=torch.int32, device="cuda")
        db = torch.full((8 * h,), float("nan"), device="cuda")
        rc = lib.tsg_lstm_bwd_ws_layout(ptr(dev["WT"]), ptr(Rg), ptr(Cs), ptr(dev["dOut"]), hp, ptr(dG), ptr(dC), ptr(ws), nb, ptr(db), B, T, h, dt, bm, st)
        assert rc == 0, f"{tag}: {lib.tsg_last_error()}"
        torch.cuda.synchronize()
        assert int(ws[0]) == 0, f"{tag}: the backward's bounded wait expired"
        last, _ = _last_chunk(B, h // 32)
        assert int(ws[1]) == 2 * last * (h // 32), f"{tag}: {int(ws[1])} workgroups arrived at the backward's start barrier"
        return dG, db.view(2, 4 * h)
    assert nb == 0 or lib.tsg_lstm_bwd_ws_persistent(B, T, h, nb) == 0, f"{tag}: the step kernels were meant to run"
    if bm:
        rc = lib.tsg_lstm_bwd_ws_layout(ptr(dev["WT"]), ptr(Rg), ptr(Cs), ptr(dev["dOut"]), hp, ptr(dG), ptr(dC), None, 0, None, B, T, h, dt, bm, st)
    else:
        rc = lib.tsg_lstm_bwd(ptr(dev["WT"]), ptr(Rg), ptr(Cs), ptr(dev["dOut"]), hp, ptr(dG), ptr(dC), B, T, h, dt, st)
    assert rc == 0, f"{tag}: {lib.tsg_last_error()}"
    torch.cuda.synchronize()
    return dG, dG.float().sum((0, 1))


def _operands(ins, bm, bf):
    seq = (lambda x: x.transpose(0, 1).contiguous()) if bm else (lambda x: x)
    to = (lambda x: x.to(BF)) if bf else (lambda x: x)
    return dict(Gx=to(seq(ins["Gx"]).cuda()), dOut=to(seq(ins["dOut"]).cuda()), W=ins["W"].cuda(), WT=ins["W"].transpose(1, 2).contiguous().cuda(),
                dHn=ins["dHn"].cuda())


def _run_case(request, path, mode, B, T, h, kind, ring=-1, bm=0):
    """path: "step" (persist 0: launch-per-step kernels, forward and backward), "generic" (persistent forward for any h % 32 == 0, polling out;
    backward on the step kernels), "persist" (tsg_lstm_fwd_ws with the ring off / on, persistent backward), "wide" (the 64-unit forward)."""
    bf = mode == "bf16"
    dt = DT[mode]
    lib = _switches(request, 0 if path == "step" else 1, ring, 1 if path == "wide" else 0)
    persistent_bwd = path in ("persist", "wide")
    arith = "bf16" if bf else "f32s" if (mode == "f32s" and persistent_bwd) else "fp32"
    tag = f"{path} {mode}{' ring=%d' % ring if ring >= 0 else ''}{' bm' if bm else ''} [{B},{T},{h}] {kind}"
    ins, want, e32, ebf = R.truth(kind, B, T, h, bf)
    dev = _operands(ins, bm, bf)
    rep = _Report(tag)
    out, Rg, Cs = _forward(lib, path, dev, B, T, h, dt, bm, ring, tag)
    got = dict(out=out.transpose(0, 1) if bm else out, R=Rg, Cs=Cs)
    for k in ("out", "R", "Cs"):
        if kind == "beyond":
            rep.finite(k, got[k])
        else:
            _check_mode(rep, k, got[k], want[k], e32[k], ebf[k] if bf else None, arith, grad=False)
    for hn, suf in ((None, ""), (dev["dHn"], "_hn")):
        dG, db = _backward(lib, persistent_bwd, dev, (Rg, Cs), hn, B, T, h, dt, bm, tag)
        for k, v in (("dG" + suf, dG.transpose(0, 1) if bm else dG), ("dbias" + suf, db)):
            if kind == "beyond":
                rep.finite(k, v)
            else:
                _check_mode(rep, k, v, want[k], e32[k], ebf[k] if bf else None, arith, grad=True)
    rep.done()


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------
MODES = ("fp32", "f32s", "bf16")
CASES = []


def _add(path, mode, B, T, h, kinds, **kw):
    CASES.extend(dict(path=path, mode=mode, B=B, T=T, h=h, kind=k, **kw) for k in kinds)


# launch-per-step kernels, forward and backward: h not a multiple of 16 and a multiple of 128; one step (no recurrent term), an odd count, the base
for h_ in (36, 128):
    for T_ in (1, 5, T0):
        _add("step", "fp32", B0, T_, h_, R.ALL_FAMILIES if (h_, T_) == (128, T0) else R.SHORT)
_add("step", "f32s", B0, T0, 96, R.SHORT)                             # f32s on the step kernels: the fp32 arithmetic, held to the fp32 bound
for h_ in (96, 160):                                                  # the generic persistent forward (HJ = 0)
    _add("generic", "fp32", B0, T0, h_, R.SHORT)
for h_ in (128, 256, 384, 512):                                       # persistent forward polling out / through the ring; persistent backward
    for ring_ in (0, 1):                                              # (h = 512 at B = 20: f32s, and bf16 through the ring, run the 16-unit workgroups)
        for mode_ in MODES:
            _add("persist", mode_, B0, T0, h_, R.ALL_FAMILIES if h_ == 128 else R.SHORT, ring=ring_)
for ring_ in (0, 1):                                                  # 32-unit workgroups at h = 512 in f32s: more than 32 rows
    _add("persist", "f32s", 36, T0, 512, R.SHORT, ring=ring_)
for B_ in (B0, 100):                                                  # the 64-unit forward
    _add("wide", "bf16", B_, T0, 512, R.SHORT, ring=1)
for mode_ in ("fp32", "bf16"):                                        # nine slices: more than the eight of one launch on 256 CUs -> two launches
    _add("persist", mode_, 144, 8, 512, R.SHORT, ring=1)
for mode_ in MODES:                                                   # long recurrence
    _add("persist", mode_, B0, 128, 128, R.ALL_FAMILIES, ring=1)
    _add("persist", mode_, B0, 128, 512, R.SHORT, ring=1)
# batch-major layout: one case of each row above
_add("step", "fp32", B0, 5, 36, ("scale4",), bm=1)
_add("step", "f32s", B0, T0, 96, ("scale4",), bm=1)
_add("generic", "fp32", B0, T0, 96, ("scale4",), bm=1)
_add("persist", "f32s", B0, T0, 256, ("scale4",), ring=0, bm=1)
_add("persist", "bf16", B0, T0, 384, ("scale4",), ring=1, bm=1)
_add("persist", "f32s", B0, T0, 512, ("scale4",), ring=1, bm=1)
_add("persist", "f32s", 36, T0, 512, ("scale4",), ring=1, bm=1)
_add("wide", "bf16", 100, T0, 512, ("scale4",), ring=1, bm=1)
_add("persist", "bf16", 144, 8, 512, ("scale4",), ring=1, bm=1)
_add("persist", "fp32", 144, 8, 512, ("scale4",), ring=1, bm=1)
_add("persist", "fp32", B0, 128, 128, ("scale4",), ring=1, bm=1)
# one truth serves the cases that follow it: ordered by (shape, family, storage)
CASES.sort(key=lambda c: (c["B"], c["T"], c["h"], c["kind"], c["mode"] == "bf16"))


def _id(c):
    return (f"{c['path']}-{c['mode']}" + (f"-ring{c['ring']}" if "ring" in c else "") + ("-bm" if c.get("bm") else "")
            + f"-B{c['B']}-T{c['T']}-h{c['h']}-{c['kind']}")


@pytest.mark.parametrize("case", [pytest.param(c, id=_id(c)) for c in CASES])
def test_lstm_f64(case, request):
    _run_case(request, **case)


def test_chunked_shape_needs_more_than_one_launch():
    """[144, 8, 512] is in the list as the case of consecutive launches over row chunks (with dHn offset by the chunk's first row): on this
    device it must need them, forward (32-unit workgroups) and backward."""
    assert _last_chunk(144, 512 // 32)[1] > 1


@pytest.mark.parametrize("mode", MODES)
def test_backward_ring_survives_stale_generations(mode, request):
    """The persistent backward on a ring workspace pre-filled with stale data of the even generation tag (0x3f800000), then -- on the same
    buffers -- of the odd one (0x3f800001): a consumer that accepted a stale block for a fresh one would add 1.0s to dh.  Both runs are held to
    the case's bound against float64 and give the same dG bit for bit."""
    B, T, h, kind = B0, T0, 256, "unit"
    bf = mode == "bf16"
    dt = DT[mode]
    lib = _switches(request, 1, 1, 0)
    ins, want, e32, ebf = R.truth(kind, B, T, h, bf)
    dev = _operands(ins, 0, bf)
    arith = "bf16" if bf else mode
    tag = f"stale ring {mode} [{B},{T},{h}] {kind}"
    out, Rg, Cs = _forward(lib, "persist", dev, B, T, h, dt, 0, 1, tag)
    nb = lib.tsg_lstm_bwd_ws_bytes(B, T, h)
    ws = torch.empty(nb // 4 + 4, dtype=torch.int32, device="cuda")
    rep = _Report(tag)
    runs = []
    for fill in STALE:
        ws.fill_(fill)
        dG, db = _backward(lib, True, dev, (Rg, Cs), dev["dHn"], B, T, h, dt, 0, tag, ws=ws)
        for k, v in (("dG_hn", dG), ("dbias_hn", db)):
            _check_mode(rep, k, v, want[k], e32[k], ebf[k] if bf else None, arith, grad=True)
        runs.append(dG)
    rep.done()
    assert torch.equal(runs[0], runs[1])

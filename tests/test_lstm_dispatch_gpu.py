"""Which kernel the BiLSTM host dispatch picks, at the smallest shapes on either side of every boundary of its forward and backward plans
(csrc/lstm.hip: lstm_fwd_plan / lstm_bwd_plan; include/tsg_hip.h, "BiLSTM host dispatch").  Through the C ABI, like tests/test_lstm_f64_gpu.py,
whose operands, float64 truth, bounds and ``_last_chunk`` arithmetic are reused.

The kernel that ran is identified by two observations on the caller's workspace, whose sync words start zeroed and whose ring region starts
full of a fill pattern:
  * sync word 1, the start barrier's arrival counter: 0 after the launch-per-step kernels (they never touch the workspace),
    2 directions x 16-row slices of the LAST launch x workgroups per slice after a persistent layer;
  * the ring region: still the fill pattern (step kernels, kernels that poll `out`) or changed (ring kernels).
Sync word 0 (expired bounded wait) must be 0 after every launch.  Paths the header declares bit-identical (ring / polling `out`, 64- / 32-unit
workgroups) are compared with torch.equal; everything is held to the float64 bounds of test_lstm_f64_gpu.py."""
import pytest
import torch

import lstm_f64 as R
import test_lstm_f64_gpu as F

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
FILL = 0x3f800000                                     # 1.0f: a stale value that would show in dh / h if a ring kernel accepted it
SYNC_WORDS = 2048 // 4                                # TSG_LSTM_SYNC_BYTES
KIND = "scale4"
E_SHAPE = -2


def _workspace(ring_bytes):
    """sync words zeroed, everything behind them the fill pattern; at least the sync words"""
    ws = torch.full((max(ring_bytes, 2048) // 4 + 4,), FILL, dtype=torch.int32, device="cuda")
    ws[:SYNC_WORDS] = 0
    return ws


def _observe(ws, tag):
    """-> (arrivals at the start barrier, ring region changed)"""
    torch.cuda.synchronize()
    assert int(ws[0]) == 0, f"{tag}: a bounded wait expired"
    return int(ws[1]), not bool((ws[SYNC_WORDS:] == FILL).all())


def _arrivals(B, wgs, per_cu=1):
    last, launches = F._last_chunk(B, wgs, per_cu)
    return 2 * last * wgs, launches


def _arith(mode, h, persistent):
    """the arithmetic a path runs in: f32s only on the persistent kernels of h in {128, 256, 384, 512}"""
    return "bf16" if mode == "bf16" else "f32s" if (mode == "f32s" and persistent and h % 128 == 0 and h <= 512) else "fp32"


def _run_forward(lib, dev, mode, B, T, h, ws_bytes="full", bm=0, tag=""):
    """-> (rc, out, R, Cs, arrivals, ring changed) of one tsg_lstm_fwd_ws call.  ws_bytes: "full" = tsg_lstm_fwd_ws_bytes (the sync words alone
    where there is no ring), or a byte count"""
    from shufflingvideosfortsg_amd._lib import ptr
    st = torch.cuda.current_stream().cuda_stream
    dt = F.DT[mode]
    seq = BF if mode == "bf16" else torch.float32
    out = torch.full((B, T, 2 * h) if bm else (T, B, 2 * h), 9.0, device="cuda", dtype=seq)
    Rg = torch.full((T, 2, B, h, 4), float("nan"), device="cuda", dtype=seq); Cs = torch.full((T, 2, B, h), float("nan"), device="cuda")
    need = max(int(lib.tsg_lstm_fwd_ws_bytes(B, T, h)), 2048)
    ws = _workspace(need)
    rc = lib.tsg_lstm_fwd_ws(ptr(dev["Gx"]), None, ptr(dev["W"]), ptr(out), ptr(Rg), ptr(Cs), ptr(ws), need if ws_bytes == "full" else ws_bytes,
                             B, T, h, dt, bm, st)
    if rc != 0:
        return rc, None, None, None, None, None
    arrived, ring = _observe(ws, tag)
    return rc, out, Rg, Cs, arrived, ring


# ---- forward ----------------------------------------------------------------------------------------------------------------------------------
# wgs: workgroups per (direction, 16-row slice) of the expected persistent kernel (h / 32; 16-unit workgroups h / 16, two per CU; 64-unit
# h / 64), None = the step kernels.  ring: whether the exchange ring is used.  launches: how many persistent launches on a 256-CU device
# (derived from the device's CU count, asserted only there).  twin: a second run whose out / R / Cs must be the same bit for bit.
def _f(name, mode, B, T, h, wgs, ring=False, per_cu=1, launches=1, persist=-1, wide=-1, ws_bytes="full", twin=None):
    return pytest.param(dict(mode=mode, B=B, T=T, h=h, wgs=wgs, ring=ring, per_cu=per_cu, launches=launches, persist=persist, wide=wide,
                             ws_bytes=ws_bytes, twin=twin), id=f"{name}-{mode}-B{B}-T{T}-h{h}")


FWD = [
    # T: the automatic rule takes sequences of >= 8 steps; one step never runs persistently; bf16 storage ignores the rule
    _f("T7-step", "fp32", 20, 7, 128, None),
    _f("T8-persist", "fp32", 20, 8, 128, 4),
    _f("T1-forced-step", "fp32", 20, 1, 128, None, persist=1),
    _f("T2-bf16-persist", "bf16", 20, 2, 128, 4, ring=True),
    # h: multiples of 32 up to 512
    _f("h100-step", "fp32", 20, 8, 100, None),
    _f("h96-generic", "fp32", 20, 8, 96, 3),
    _f("h160-generic", "fp32", 20, 8, 160, 5),
    _f("h544-step", "fp32", 20, 8, 544, None),
    # 16-unit workgroups: up to 32 rows at h = 512, f32s or bf16 through the ring
    _f("nw4", "f32s", 32, 8, 512, 32, per_cu=2),
    _f("nw8", "f32s", 33, 8, 512, 16),
    _f("nw4-ring", "bf16", 32, 8, 512, 32, ring=True, per_cu=2),
    _f("nw8-poll", "bf16", 33, 8, 512, 16),
    _f("h384-nw8", "f32s", 32, 8, 384, 12),
    _f("h384-nw8", "bf16", 32, 8, 384, 12, ring=True),
    # ring: from 96 rows (bf16 storage: also up to 32), when the workspace holds one
    _f("no-ring", "fp32", 95, 8, 128, 4),
    _f("ring", "fp32", 96, 8, 128, 4, ring=True, twin=dict(ws_bytes=-16, ring=False)),
    # 64-unit workgroups: bf16 storage, h = 512, more than 128 rows
    _f("narrow", "bf16", 128, 8, 512, 16, ring=True),
    _f("wide", "bf16", 129, 8, 512, 8, ring=True, twin=dict(wide=0, wgs=16, launches=2)),
]


def _forward_case(request, c, dev, want, e32, ebf, tag):
    lib = F._switches(request, c["persist"], -1, c["wide"])
    B, T, h, mode = c["B"], c["T"], c["h"], c["mode"]
    wsb = c["ws_bytes"]
    if isinstance(wsb, int) and wsb < 0:                                         # relative to the full size
        wsb = int(lib.tsg_lstm_fwd_ws_bytes(B, T, h)) + wsb
    rc, out, Rg, Cs, arrived, ring = _run_forward(lib, dev, mode, B, T, h, wsb, tag=tag)
    assert rc == 0, f"{tag}: {lib.tsg_last_error()}"
    if c["wgs"] is None:
        assert arrived == 0, f"{tag}: {arrived} workgroups arrived at a start barrier: a persistent kernel ran, the step kernels were expected"
    else:
        want_arrived, launches = _arrivals(B, c["wgs"], c["per_cu"])
        assert arrived == want_arrived, f"{tag}: {arrived} workgroups arrived at the start barrier, {want_arrived} expected: another kernel ran"
        if torch.cuda.get_device_properties(0).multi_processor_count == 256:
            assert launches == c["launches"], f"{tag}: {launches} launches"
    assert ring == c["ring"], f"{tag}: ring region {'changed' if ring else 'untouched'}"
    rep = F._Report(tag)
    arith = _arith(mode, h, c["wgs"] is not None)
    for k, v in (("out", out), ("R", Rg), ("Cs", Cs)):
        F._check_mode(rep, k, v, want[k], e32[k], ebf[k] if ebf else None, arith, grad=False)
    rep.done()
    return out, Rg, Cs


@pytest.mark.parametrize("c", FWD)
def test_lstm_dispatch_edges(c, request):
    bf = c["mode"] == "bf16"
    ins, want, e32, ebf = R.truth(KIND, c["B"], c["T"], c["h"], bf)
    dev = F._operands(ins, 0, bf)
    tag = f"fwd {c['mode']} [{c['B']},{c['T']},{c['h']}]"
    first = _forward_case(request, c, dev, want, e32, ebf, tag)
    if c["twin"]:
        second = _forward_case(request, dict(c, **c["twin"]), dev, want, e32, ebf, tag + f" twin {c['twin']}")
        for k, a, b in zip(("out", "R", "Cs"), first, second):
            assert torch.equal(a, b), f"{tag}: {k} differs between the two paths"


def test_lstm_dispatch_short_sync_workspace():
    """a workspace smaller than the sync words is an argument error, not a fallback"""
    lib = F._lib()
    ins, _, _, _ = R.truth(KIND, 96, 8, 128, False)
    rc = _run_forward(lib, F._operands(ins, 0, False), "fp32", 96, 8, 128, 2048 - 1)[0]
    assert rc == E_SHAPE and b"smaller than TSG_LSTM_SYNC_BYTES" in lib.tsg_last_error()


# ---- backward ---------------------------------------------------------------------------------------------------------------------------------
# persistent: what runs.  answer: what tsg_lstm_bwd_ws_persistent says (it has no dtype argument and follows the T >= 8 rule, which bf16 storage
# ignores: the one case where the two differ).  ws: "full", "none" (NULL) or a byte count relative to the full size.
def _b(name, mode, B, T, h, persistent, answer=None, ws="full", launches=1, bm=0, error=None):
    return pytest.param(dict(mode=mode, B=B, T=T, h=h, persistent=persistent, answer=persistent if answer is None else answer, ws=ws,
                             launches=launches, bm=bm, error=error), id=f"{name}-{mode}-B{B}-T{T}-h{h}" + ("-bm" if bm else ""))


BF16_NEEDS = b"dtype TSG_BF16 needs the persistent kernel (ring workspace of tsg_lstm_bwd_ws_bytes"
BWD = [
    _b("T7-step", "fp32", 20, 7, 128, False),
    _b("T8-persist", "fp32", 20, 8, 128, True),
    _b("T2-bf16-persist", "bf16", 20, 2, 128, True, answer=False),
    _b("h96-step", "fp32", 20, 8, 96, False),
    _b("no-ws-step", "fp32", 20, 8, 128, False, ws="none"),
    _b("short-ws-step", "fp32", 20, 8, 128, False, ws=-16),
    _b("no-ws-error", "bf16", 20, 8, 128, False, ws="none", error=BF16_NEEDS),
    _b("short-ws-error", "bf16", 20, 8, 128, False, ws=-16, error=BF16_NEEDS),
    _b("two-launches", "fp32", 144, 8, 512, True, launches=2),
    _b("two-launches", "bf16", 144, 8, 512, True, launches=2, bm=1),
]


@pytest.mark.parametrize("c", BWD)
def test_lstm_dispatch_edges_backward(c, request):
    from shufflingvideosfortsg_amd._lib import ptr
    lib = F._switches(request, -1)
    B, T, h, mode, bm = c["B"], c["T"], c["h"], c["mode"], c["bm"]
    bf = mode == "bf16"
    tag = f"bwd {mode}{' bm' if bm else ''} [{B},{T},{h}] ws={c['ws']}"
    ins, want, e32, ebf = R.truth(KIND, B, T, h, bf)
    dev = F._operands(ins, bm, bf)
    rc, _, Rg, Cs, arrived, _ = _run_forward(lib, dev, mode, B, T, h, bm=bm, tag=tag)           # the saved state, from the automatic forward
    assert rc == 0, f"{tag}: {lib.tsg_last_error()}"
    fwd_persistent = arrived > 0
    st = torch.cuda.current_stream().cuda_stream
    need = int(lib.tsg_lstm_bwd_ws_bytes(B, T, h))
    ws = None if c["ws"] == "none" else _workspace(need)
    nb = 0 if ws is None else need if c["ws"] == "full" else need + c["ws"]
    if ws is not None and need == 0:
        nb = 2048                                                                # no ring for this hidden size: the sync words alone
    assert lib.tsg_lstm_bwd_ws_persistent(B, T, h, nb) == int(c["answer"]), f"{tag}: tsg_lstm_bwd_ws_persistent"
    dG = torch.full_like(dev["Gx"], float("nan")); dC = torch.zeros(2, B, h, device="cuda")
    db = torch.full((8 * h,), float("nan"), device="cuda")
    rc = lib.tsg_lstm_bwd_ws_layout(ptr(dev["WT"]), ptr(Rg), ptr(Cs), ptr(dev["dOut"]), ptr(dev["dHn"]), ptr(dG), ptr(dC),
                                    ptr(ws) if ws is not None else None, nb, ptr(db), B, T, h, F.DT[mode], bm, st)
    if c["error"]:
        assert rc == E_SHAPE and c["error"] in lib.tsg_last_error(), f"{tag}: rc {rc} {lib.tsg_last_error()}"
        return
    assert rc == 0, f"{tag}: {lib.tsg_last_error()}"
    if ws is None:
        torch.cuda.synchronize()
        arrived, ring = 0, False
    else:
        arrived, ring = _observe(ws, tag)
    if c["persistent"]:
        want_arrived, launches = _arrivals(B, h // 32)
        assert arrived == want_arrived, f"{tag}: {arrived} workgroups arrived at the backward's start barrier, {want_arrived} expected"
        if torch.cuda.get_device_properties(0).multi_processor_count == 256:
            assert launches == c["launches"], f"{tag}: {launches} launches"
        assert ring, f"{tag}: the partial-dh ring is untouched"
        assert bool(torch.isfinite(db).all()), f"{tag}: the persistent backward did not fill dbias"
        dbias = db.view(2, 4 * h)
    else:
        assert arrived == 0 and not ring, f"{tag}: the workspace was touched ({arrived} arrivals): the persistent kernel ran"
        assert bool(torch.isnan(db).all()), f"{tag}: the step kernels wrote dbias"
        dbias = dG.float().sum((0, 1))
    rep = F._Report(tag)
    arith = _arith(mode, h, fwd_persistent and c["persistent"])
    for k, v in (("dG_hn", dG.transpose(0, 1) if bm else dG), ("dbias_hn", dbias)):
        F._check_mode(rep, k, v, want[k], e32[k], ebf[k] if bf else None, arith, grad=True)
    rep.done()

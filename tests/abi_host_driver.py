#!/usr/bin/env python3
"""Host-side checks of the C ABI that need no GPU: argument errors, workspace planners, tile / range arithmetic.  Two users:
  * tests/test_abi_cpu.py calls ``run_checks(lib)`` on the product library;
  * the same file, run as a script with a library path, is the driver of the host SANITIZER build: an AddressSanitizer +
    UndefinedBehaviorSanitizer build of the host layer without device code (``python tools/build_host_sanitized.py``),
    loaded into a python that has the ASAN runtime preloaded.  It imports neither torch nor the package (an uninstrumented torch under a
    preloaded ASAN runtime is slow and noisy): the ctypes signature table is read out of _lib.py with a placeholder in torch's place.
Every call here returns before a kernel launch.  Never run on a GPU box."""
import ctypes
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TSG_F32, TSG_BF16, TSG_F32S = 0, 1, 2


def signatures():
    """(_SIGNATURES, _RESTYPE) of shufflingvideosfortsg_amd/_lib.py without importing torch."""
    src = open(os.path.join(ROOT, "shufflingvideosfortsg_amd", "_lib.py")).read()
    had = sys.modules.get("torch")
    if had is None:
        sys.modules["torch"] = types.ModuleType("torch")
    try:
        ns = {"__name__": "_lib_signatures", "__file__": os.path.join(ROOT, "shufflingvideosfortsg_amd", "_lib.py")}
        exec(compile(src, ns["__file__"], "exec"), ns)
    finally:
        if had is None:
            del sys.modules["torch"]
    return ns["_SIGNATURES"], ns["_RESTYPE"]


def load_standalone(path):
    ctypes.CDLL("/opt/rocm/lib/libamdhip64.so", mode=ctypes.RTLD_GLOBAL)
    lib = ctypes.CDLL(path)
    sig, res = signatures()
    for name, argtypes in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = res.get(name, ctypes.c_int)
    return lib


def run_checks(lib):
    """Argument errors and planners; returns the number of calls made."""
    n = [0]

    def eq(got, want, what=""):
        n[0] += 1
        assert got == want, f"{what}: got {got}, want {want} ({lib.tsg_last_error()})"
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    # K1
    eq(lib.tsg_scdm_attn_fwd(None, p, p, p, p, p, 1, 1, 1, 4, 4, TSG_F32, None), -1, "NULL")
    assert b"NULL" in lib.tsg_last_error()
    eq(lib.tsg_scdm_attn_fwd(p, p, p, p, p, p, 1, 1, 33, 4, 4, TSG_F32, None), -2, "N > 32")
    eq(lib.tsg_scdm_attn_fwd(p, p, p, p, None, p, 1, 1, 33, 6, 4, 7, None), -1, "wrong four ways: the NULL pointer is reported")
    assert b"NULL" in lib.tsg_last_error()
    eq(lib.tsg_scdm_gate_bwd(*([p] * 15), 1 << 40, 1, 1, 33, 6, 4, 7, None), -4, "dtype, N > 32 and H % 4: the dtype is reported")
    eq(lib.tsg_scdm_attn_bwd(*([p] * 11), 1 << 40, 1, 1, 33, 6, 4, TSG_F32, None), -2, "N > 32 and H % 4: N is reported")
    assert b"N=33" in lib.tsg_last_error()
    eq(lib.tsg_scdm_attn_fwd(p, p, p, p, p, p, 1, 1, 1, 6, 4, TSG_F32, None), -3, "H % 4")
    eq(lib.tsg_scdm_attn_fwd(p, p, p, p, p, p, 1, 1, 1, 4, 4, 7, None), -4, "dtype")
    eq(lib.tsg_scdm_attn_fwd(p + 4, p, p, p, p, p, 1, 1, 1, 4, 4, TSG_F32, None), -3, "misaligned")
    for dims in ((0, 1, 1, 4, 4), (1, 0, 1, 4, 4), (1, 1, 0, 4, 4), (1, 1, 1, 0, 4), (1, 1, 1, 4, 0), (-3, 1, 1, 4, 4), (1, 1, 1, 4, -8)):
        eq(lib.tsg_scdm_attn_fwd(p, p, p, p, p, p, *dims, TSG_F32, None), -2, f"dims {dims}")
    # K2 / K3 / K5 / LSTM
    eq(lib.tsg_mha_fwd(p, p, p, p, None, None, p, 1, 4, 4, 8, 8, 3, 1.0, 0, 0.0, 0, 0, TSG_F32, None), -2, "8 % 3")
    eq(lib.tsg_mha_fwd(p, p, p, p, None, None, p, 1, 4, 4, 8, 8, 2, 1.0, 0, 1.0, 0, 0, TSG_F32, None), -2, "dropout p")
    eq(lib.tsg_boundary_score_fwd(p, p, p, p, p, None, None, p, p, 1, 4, 3, TSG_F32, None), -2, "2 Hm % 4")
    eq(lib.tsg_mha_bwd(p, p, p, p, p, p, p, p, p, p, 1, 4, 4, 8, 8, 2, 1.0, 0, 0.0, 0, 0, 7, None), -4, "dtype")
    eq(lib.tsg_mha_fwd(p, p, p, p, p, None, p, 1, 4, 4, 64, 64, 2, 1.0, 0, 0.0, 0, 0, TSG_BF16, None), -2, "A_sum in bf16")
    eq(lib.tsg_mha_fwd(p, p, p, p, None, None, p, 1, 4, 4, 40, 40, 2, 1.0, 0, 0.0, 0, 0, TSG_BF16, None), -2, "head width 20")
    eq(lib.tsg_mha_bwd(p, p, p, p, p, p, p, p, p, p, 1, 4, 4, 512, 512, 2, 1.0, 0, 0.0, 0, 0, TSG_BF16, None), -2, "head width 256")
    # K2 calls that are wrong in several ways at once: the code and the text of the FIRST failing check, in the order NULL / alignment ->
    # dtype -> dimensions -> divisibility -> head widths -> dropout -> scale (forward only) -> bf16 shape
    def k2(rc, want, text, what):
        eq(rc, want, what)
        assert text in lib.tsg_last_error(), f"{what}: {lib.tsg_last_error()}"

    def fwd(Q=p, A=None, B=1, dk=8, dv=8, H=2, scale=1.0, pd=0.0, dt=TSG_F32):
        return lib.tsg_mha_fwd(Q, p, p, p, A, None, p, B, 4, 4, dk, dv, H, scale, 0, pd, 0, 0, dt, None)

    def bwd(ws=p, dk=64, H=2, dt=TSG_BF16):
        return lib.tsg_mha_bwd(p, p, p, p, p, p, p, p, p, ws, 1, 4, 4, dk, dk, H, 1.0, 0, 0.0, 0, 0, dt, None)
    k2(fwd(Q=None, dt=7), -1, b"tsg_mha_fwd: NULL pointer argument", "NULL Q and dtype 7")
    k2(fwd(Q=p + 4, B=0), -3, b"is not 16-byte aligned", "misaligned Q and B = 0")
    k2(fwd(B=0, dt=7), -4, b"tsg_mha_fwd: dtype 7 not supported", "dtype 7 and B = 0")
    k2(fwd(H=3, pd=1.0), -2, b"d_key=8 / d_value=8 not divisible by n_heads=3", "8 % 3 and p_drop = 1")
    k2(fwd(pd=1.0, scale=0.0), -2, b"dropout probability 1 outside [0, 1)", "p_drop = 1 and scale = 0")
    k2(fwd(A=p, dk=64, dv=64, scale=0.0, dt=TSG_BF16), -2, b"tsg_mha_fwd: scale must be positive", "scale = 0, bf16 and A_sum")
    k2(fwd(dk=12, dv=12), -3, b"head widths 6 / 6 must be multiples of 4", "head width 6")
    k2(fwd(dv=1032), -2, b"value head width 516 > 512 not supported", "value head width 516")
    k2(bwd(ws=None), -2, b"tsg_mha_bwd: dtype TSG_BF16 needs delta_ws, d_key == d_value and head widths 32 .. 128 in steps of 32 "
       b"(head width 32 / 32)", "bf16 backward without delta_ws")
    k2(bwd(dk=320), -2, b"in steps of 32 (head width 160 / 160)", "bf16 backward at head width 160")
    k2(lib.tsg_mha_fwd_rng(None, p, p, p, None, None, p, 1, 4, 4, 8, 8, 2, 1.0, 0, 0.5, None, TSG_F32, None), -1,
       b"tsg_mha_fwd_rng: rng_dev is NULL", "fwd_rng: p_drop > 0, no rng_dev, NULL Q")
    k2(lib.tsg_mha_bwd_rng(None, p, p, p, p, p, p, p, p, p, 1, 4, 4, 8, 8, 2, 1.0, 0, 0.5, None, TSG_F32, None), -1,
       b"tsg_mha_bwd_rng: rng_dev is NULL", "bwd_rng: p_drop > 0, no rng_dev, NULL Q")
    eq(lib.tsg_lstm_fwd_bias(p, None, p, p, p, p, p, 4, 16, 100, TSG_BF16, 1, None), -2, "h = 100")
    eq(lib.tsg_lstm_fwd_bias(p, None, p, p, p, p, None, 4, 16, 128, TSG_BF16, 1, None), -2, "no sync workspace")
    eq(lib.tsg_lstm_bwd_ws_layout(p, p, p, p, None, p, p, None, 0, None, 4, 16, 128, TSG_BF16, 1, None), -2, "no ring workspace")
    # BiLSTM: one argument check for the forward, the step backward and the persistent backward.  Order on the forward (reported under the name
    # tsg_lstm_fwd): the workspace size (tsg_lstm_fwd_ws only) -> bias alignment -> each pointer's NULL / alignment in argument order ->
    # workspace alignment -> dtype -> dimensions -> h % 4 -> the bf16 shape.  tsg_lstm_bwd: pointers -> dtype -> dimensions -> h % 4.
    # tsg_lstm_bwd_ws_layout: the bf16 shape / workspace FIRST (a misaligned workspace counts as none), then -- no GPU here, so the step
    # kernels' checks under the name tsg_lstm_bwd -- pointers (dC_ws among them) -> dtype -> dimensions -> h % 4.
    def lf(Gx=p, bias=None, Whh=p, Cs=p, ws=p, nws=2048, B=4, T=16, h=128, dt=TSG_BF16):
        return lib.tsg_lstm_fwd_ws(Gx, bias, Whh, p, p, Cs, ws, nws, B, T, h, dt, 1, None)

    def lb(WhhT=p, dG=p, B=4, T=16, h=128, dt=TSG_F32):
        return lib.tsg_lstm_bwd(WhhT, p, p, p, None, dG, p, B, T, h, dt, None)

    def lw(WhhT=p, dOut=p, dC=p, ws=None, nws=0, B=4, T=16, h=128, dt=TSG_F32):
        return lib.tsg_lstm_bwd_ws_layout(WhhT, p, p, dOut, None, p, dC, ws, nws, None, B, T, h, dt, 1, None)
    nb = lib.tsg_lstm_bwd_ws_bytes(4, 16, 128)
    needs_fwd = b"tsg_lstm_fwd: dtype TSG_BF16 needs the persistent kernel (sync_ws given, TSG_LSTM_PERSIST != 0, T > 1, h in {128,256,384,512}); got "
    needs_bwd = b"tsg_lstm_bwd_ws: dtype TSG_BF16 needs the persistent kernel (ring workspace of tsg_lstm_bwd_ws_bytes, T > 1, h in {128,256,384,512}, " \
                b"TSG_LSTM_PERSIST != 0); got "
    k2(lf(Gx=None), -1, b"tsg_lstm_fwd: NULL pointer argument", "lstm fwd: NULL Gx")
    k2(lf(Whh=p + 4), -3, b"tsg_lstm_fwd: pointer", "lstm fwd: misaligned Whh")
    k2(lf(bias=p + 4), -3, b"tsg_lstm_fwd: bias", "lstm fwd: misaligned bias")
    k2(lf(ws=p + 4), -3, b"tsg_lstm_fwd: workspace", "lstm fwd: misaligned workspace")
    k2(lf(nws=2047), -2, b"tsg_lstm_fwd_ws: workspace of 2047 bytes is smaller than TSG_LSTM_SYNC_BYTES", "lstm fwd: short workspace")
    k2(lf(nws=2047, dt=TSG_F32), -2, b"smaller than TSG_LSTM_SYNC_BYTES", "lstm fwd: short workspace, fp32")
    k2(lf(dt=7), -4, b"tsg_lstm_fwd: dtype 7 not supported (TSG_F32, TSG_F32S or TSG_BF16)", "lstm fwd: dtype")
    for dims in ((0, 16, 128), (4, 0, 128), (4, 16, 0), (-4, 16, 128)):
        k2(lf(B=dims[0], T=dims[1], h=dims[2], dt=TSG_F32), -2, b"tsg_lstm_fwd: non-positive dimension", f"lstm fwd: dims {dims}")
    k2(lf(h=6, dt=TSG_F32), -3, b"tsg_lstm_fwd: hidden size 6 must be a multiple of 4", "lstm fwd: h % 4")
    k2(lf(T=1), -2, needs_fwd + b"T=1 h=128", "lstm fwd: bf16, T = 1")
    k2(lf(h=96), -2, needs_fwd + b"T=16 h=96", "lstm fwd: bf16, h = 96")
    k2(lf(ws=None, nws=0), -2, needs_fwd + b"T=16 h=128", "lstm fwd: bf16, no workspace")
    k2(lf(Gx=None, dt=7), -1, b"NULL pointer argument", "lstm fwd: NULL Gx and dtype 7")
    k2(lf(bias=p + 4, Gx=None), -3, b"tsg_lstm_fwd: bias", "lstm fwd: misaligned bias and NULL Gx")
    k2(lf(Gx=p + 4, Cs=None), -3, b"tsg_lstm_fwd: pointer", "lstm fwd: misaligned Gx and NULL Cs: argument order")
    k2(lf(Gx=None, ws=p + 4), -1, b"NULL pointer argument", "lstm fwd: NULL Gx and misaligned workspace")
    k2(lf(ws=p + 4, dt=7), -3, b"tsg_lstm_fwd: workspace", "lstm fwd: misaligned workspace and dtype 7")
    k2(lf(dt=7, B=0), -4, b"dtype 7 not supported", "lstm fwd: dtype 7 and B = 0")
    k2(lf(B=0, h=6, dt=TSG_F32), -2, b"non-positive dimension", "lstm fwd: B = 0 and h % 4")
    k2(lf(Gx=None, h=96), -1, b"NULL pointer argument", "lstm fwd: bf16 at h = 96 and NULL Gx")
    k2(lf(Gx=None, nws=2047), -2, b"smaller than TSG_LSTM_SYNC_BYTES", "lstm fwd: short workspace and NULL Gx")
    k2(lf(T=1, h=6), -3, b"must be a multiple of 4", "lstm fwd: bf16, T = 1 and h % 4")
    k2(lb(WhhT=None), -1, b"tsg_lstm_bwd: NULL pointer argument", "lstm bwd: NULL WhhT")
    k2(lb(dG=p + 4), -3, b"tsg_lstm_bwd: pointer", "lstm bwd: misaligned dG")
    k2(lb(dt=7), -4, b"tsg_lstm_bwd: dtype 7 not supported", "lstm bwd: dtype")
    k2(lb(T=0), -2, b"tsg_lstm_bwd: non-positive dimension B=4 T=0 h=128", "lstm bwd: T = 0")
    k2(lb(h=6), -3, b"tsg_lstm_bwd: hidden size 6 must be a multiple of 4", "lstm bwd: h % 4")
    k2(lb(WhhT=None, dt=7), -1, b"NULL pointer argument", "lstm bwd: NULL WhhT and dtype 7")
    k2(lb(dt=7, h=6), -4, b"dtype 7 not supported", "lstm bwd: dtype 7 and h % 4")
    k2(lw(WhhT=None), -1, b"tsg_lstm_bwd: NULL pointer argument", "lstm bwd_ws: NULL WhhT, no workspace")
    k2(lw(WhhT=None, ws=p, nws=nb), -1, b"NULL pointer argument", "lstm bwd_ws: NULL WhhT")
    k2(lw(dOut=p + 4), -3, b"is not 16-byte aligned", "lstm bwd_ws: misaligned dOut")
    k2(lw(dC=None, ws=p + 4, nws=nb), -1, b"tsg_lstm_bwd: NULL pointer argument", "lstm bwd_ws: misaligned workspace -> the step kernels' check of dC_ws")
    k2(lw(dC=None, ws=p, nws=2047), -1, b"tsg_lstm_bwd: NULL pointer argument", "lstm bwd_ws: short workspace -> the step kernels' check of dC_ws")
    k2(lw(dt=7), -4, b"dtype 7 not supported", "lstm bwd_ws: dtype")
    k2(lw(B=0), -2, b"tsg_lstm_bwd: non-positive dimension", "lstm bwd_ws: B = 0")
    k2(lw(h=6), -3, b"tsg_lstm_bwd: hidden size 6 must be a multiple of 4", "lstm bwd_ws: h % 4")
    k2(lw(ws=p, nws=nb, T=1, dt=TSG_BF16), -2, needs_bwd + b"T=1 h=128 ws=%d" % nb, "lstm bwd_ws: bf16, T = 1")
    k2(lw(ws=p, nws=lib.tsg_lstm_bwd_ws_bytes(4, 16, 96), h=96, dt=TSG_BF16), -2, needs_bwd + b"T=16 h=96 ws=0", "lstm bwd_ws: bf16, h = 96")
    k2(lw(dt=TSG_BF16), -2, needs_bwd + b"T=16 h=128 ws=0", "lstm bwd_ws: bf16, no workspace")
    k2(lw(ws=p, nws=nb - 16, dt=TSG_BF16), -2, needs_bwd + b"T=16 h=128 ws=%d" % (nb - 16), "lstm bwd_ws: bf16, short workspace")
    k2(lw(ws=p + 4, nws=nb, dt=TSG_BF16), -2, needs_bwd, "lstm bwd_ws: bf16, misaligned workspace")
    k2(lw(WhhT=None, ws=p, nws=nb, T=1, dt=TSG_BF16), -2, needs_bwd, "lstm bwd_ws: bf16 at T = 1 and NULL WhhT: the shape is reported")
    k2(lw(WhhT=None, B=0, dt=TSG_BF16), -2, needs_bwd, "lstm bwd_ws: bf16, B = 0 and NULL WhhT: the shape is reported")
    k2(lw(WhhT=None, dt=7), -1, b"NULL pointer argument", "lstm bwd_ws: NULL WhhT and dtype 7")
    k2(lw(dOut=p + 4, B=0), -3, b"is not 16-byte aligned", "lstm bwd_ws: misaligned dOut and B = 0")
    eq(lib.tsg_match_head_fwd(p, p, p, p, p, 1, 4, 8, 0, 7, None), -4, "dtype")
    eq(lib.tsg_boundary_score_fwd(p, p, p, p, p, None, None, p, p, 1, 4, 4, 7, None), -4, "dtype")
    eq(lib.tsg_error_word(None), 0); eq(lib.tsg_error_sink(None), 0)
    eq(lib.tsg_wgrad_bf16(p, 256, 0, p, 100, 128, None, 0, 0, 0, 0, 0, p, 128, 0, None, 0, 64, 256, 1, None), -2, "ldb0 < K0")
    # weight-gradient GEMM: plan and argument checks
    eq(lib.tsg_wgrad_f32s_ws_bytes(16384, 1024, 1024, 0, 1), 8 * 4 * 1024 * 1024, "32 tiles -> 8 row ranges")
    eq(lib.tsg_wgrad_f32s_ws_bytes(16384, 2048, 1024, 512, 2), 4 * 4 * 2 * 2048 * 1536, "LSTM shape")
    eq(lib.tsg_wgrad_f32s_ws_bytes(32, 256, 128, 0, 1), 0, "one chunk")
    eq(lib.tsg_wgrad_f32s_ws_bytes(48, 256, 128, 0, 1), -1, "M % 32")
    eq(lib.tsg_wgrad_f32s_ws_bytes(64, 128, 128, 0, 1), -1, "N % 256")
    eq(lib.tsg_wgrad_f32s(p, 256, 0, p, 128, 128, None, 0, 0, 0, 0, 0, p, 128, 0, None, 0, 64, 256, 3, None), -2, "groups")
    eq(lib.tsg_wgrad_f32s(p, 256, 0, p, 100, 128, None, 0, 0, 0, 0, 0, p, 128, 0, None, 0, 64, 256, 1, None), -2, "ldb0 < K0")
    eq(lib.tsg_wgrad_f32s(None, 256, 0, p, 128, 128, None, 0, 0, 0, 0, 0, p, 128, 0, None, 0, 64, 256, 1, None), -1, "NULL")
    # the heads as GEMM epilogues: the row -> batch-item map is exact for M <= 2^22 only ((2^22, 2^23] used to pass the check)
    for M, want in ((1 << 22, None), ((1 << 22) + 64, -2), (1 << 23, -2), ((1 << 23) + 64, -2)):
        rc = lib.tsg_match_head_gemm(p, 1024, p, 1024, p, p, p, None, p, p, 1 << 40, M, 128, 1024, 1024, 0, None)
        n[0] += 1
        assert (rc == want) if want is not None else (rc != -2 or b"M=" not in lib.tsg_last_error()), f"match head M={M}: rc {rc} {lib.tsg_last_error()}"
    eq(lib.tsg_boundary_head_gemm(p, 1024, p, p, 1024, p, p, p, p, None, None, None, p, p, p, 1 << 40, 1 << 16, 128, 256, 1024, None), -2, "B T > 2^22")
    # planners over a sweep of shapes: no overflow, no UB, monotone in the batch
    for T in (1, 7, 64, 128, 512, 4096):
        for N in (1, 15, 20, 25, 32):
            for H in (8, 260, 512, 1024):
                prev = -1
                for B in (1, 3, 64, 128, 4096):
                    for gate in (0, 1):
                        v = lib.tsg_scdm_bwd_ws_bytes(B, T, N, H, H, gate); n[0] += 1
                        assert v >= 0, (B, T, N, H, gate, v)
                    assert v >= prev; prev = v
                    assert lib.tsg_scdm_bwd_fused_ok(B, T, N, H, H) in (0, 1); n[0] += 1
    eq(lib.tsg_scdm_bwd_ws_bytes(1 << 30, 1 << 30, 32, 1024, 1024, 1), 0, "B T >= 2^31: rejected (the plan used to overflow a long long here)")
    eq(lib.tsg_scdm_attn_fwd(p, p, p, p, p, p, 1 << 16, 1 << 15, 1, 4, 4, TSG_F32, None), -2, "B T = 2^31")
    for B in (1, 16, 64, 256, 1 << 20):
        for T in (1, 2, 128, 512, 1 << 16):
            for h in (32, 100, 128, 256, 384, 512, 544):
                a, b2 = lib.tsg_lstm_fwd_ws_bytes(B, T, h), lib.tsg_lstm_bwd_ws_bytes(B, T, h); n[0] += 2
                assert a >= 0 and b2 >= 0, (B, T, h, a, b2)
                assert lib.tsg_lstm_bwd_ws_persistent(B, T, h, b2) in (0, 1); n[0] += 1
    for rows in (1, 63, 8192, 1 << 24, 1 << 33):
        for d in (4, 512, 1024, 4096):
            assert lib.tsg_layer_norm_bwd_ws_bytes(rows, d) >= 0; n[0] += 1
    for Bq in (1, 64, 1 << 14):
        for Tq in (1, 128, 1 << 12):
            for Hm in (2, 128, 256):
                assert lib.tsg_boundary_score_bwd_ws_bytes(Bq, Tq, Hm) >= 0; n[0] += 1
    for M in (64, 8192, 16384, 1 << 22, 100):
        for N in (128, 256, 512, 1024):
            for heads in (1, 2):
                v = lib.tsg_head_gemm_ws_bytes(M, N, heads); n[0] += 1
                assert (v >= 0) if (M % 64 == 0 and N % (256 * heads) == 0) else (v == -1), (M, N, heads, v)
    for M in (32, 16384, 1 << 26):
        for N in (256, 2048):
            for K0, K1, g in ((128, 0, 1), (1024, 512, 2), (4096, 0, 1)):
                assert lib.tsg_wgrad_f32s_ws_bytes(M, N, K0, K1, g) >= 0; n[0] += 1
    # timing hook and gradient check (ABI 7)
    us = ctypes.c_float(-1.0)
    eq(lib.tsg_time_next_launch(4096), -2); eq(lib.tsg_time_next_launch(-1), 0)
    eq(lib.tsg_timed_launch_us(7, ctypes.byref(us)), -2); eq(lib.tsg_timed_launch_us(7, None), -1)
    one = (ctypes.c_void_p * 1)(p); cnt = (ctypes.c_longlong * 1)(8)
    eq(lib.tsg_grads_nonfinite(0, one, cnt, p, None), -1); eq(lib.tsg_grads_nonfinite(1, one, cnt, None, None), -1)
    eq(lib.tsg_grads_nonfinite(1, (ctypes.c_void_p * 1)(None), cnt, p, None), -1)
    eq(lib.tsg_grads_nonfinite(1, one, (ctypes.c_longlong * 1)(0), p, None), -2)
    eq(lib.tsg_grads_nonfinite(1, (ctypes.c_void_p * 1)(p + 2), cnt, p, None), -3)
    eq(lib.tsg_adam_step(0, one, one, one, one, cnt, 1e-3, 0.9, 0.999, 1e-6, 0.0, 1.0, p, None, None), -1, "n = 0")
    eq(lib.tsg_adam_step(1, one, one, one, one, cnt, 1e-3, 1.0, 0.999, 1e-6, 0.0, 1.0, p, None, None), -2, "beta1 = 1")
    return n[0]


if __name__ == "__main__":
    made = run_checks(load_standalone(sys.argv[1]))
    print(f"abi_host_driver: {made} host-side calls clean")

#!/usr/bin/env python3
"""Host-side checks of the long-sentence K1 entry points (tsg_scdm_long_*) that need no GPU: argument errors and the workspace planner.
Two users, as with tests/abi_host_driver.py (whose loader this reuses): tests/test_scdm_long_cpu.py calls ``run_checks(lib)`` on the
product library, and the same file run as a script with a library path drives the host SANITIZER build.  Every call returns before
a kernel launch.  Never run on a GPU box."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_host_driver as base  # noqa: E402

TSG_F32, TSG_BF16, TSG_F32S = 0, 1, 2
E_NULL, E_SHAPE, E_ALIGN, E_DTYPE = -1, -2, -3, -4


def run_checks(lib):
    """-> number of calls made."""
    n = [0]

    def eq(got, want, what=""):
        n[0] += 1
        assert got == want, f"{what}: got {got}, want {want} ({lib.tsg_last_error()})"
    buf = (ctypes.c_float * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15
    nmax = lib.tsg_scdm_long_max_words()
    assert nmax >= 128, nmax
    n[0] += 1
    # (entry point, number of pointer arguments, does it take (ws, ws_bytes))
    entries = (("tsg_scdm_long_fwd", 6, False), ("tsg_scdm_long_bwd", 11, True),
               ("tsg_scdm_long_gate_fwd", 8, False), ("tsg_scdm_long_gate_bwd", 15, True))
    big = 1 << 40
    for name, nptr, has_ws in entries:
        fn = getattr(lib, name)

        def call(ptrs, dims, dtype=TSG_F32):
            return fn(*ptrs, *((big,) if has_ws else ()), *dims, dtype, None)
        ok = [p] * nptr
        good = (1, 1, 40, 8, 8)
        for i in range(nptr):                                           # every pointer: NULL, then misaligned
            eq(call(ok[:i] + [None] + ok[i + 1:], good), E_NULL, f"{name} NULL #{i}")
            assert b"NULL" in lib.tsg_last_error()
            eq(call(ok[:i] + [p + 4] + ok[i + 1:], good), E_ALIGN, f"{name} misaligned #{i}")
        eq(call(ok, (1, 1, 0, 8, 8)), E_SHAPE, f"{name} N=0")
        eq(call(ok, (1, 1, nmax + 1, 8, 8)), E_SHAPE, f"{name} N=NMAX+1")
        assert f"N={nmax + 1}".encode() in lib.tsg_last_error(), lib.tsg_last_error()
        eq(call([None] + ok[1:], (1, 1, nmax + 1, 8, 8)), E_NULL, f"{name} NULL and N=NMAX+1")    # wrong twice: the pointer check comes first
        assert b"NULL" in lib.tsg_last_error()
        for dims in ((0, 1, 40, 8, 8), (1, 0, 40, 8, 8), (1, 1, 40, 0, 8), (1, 1, 40, 8, 0), (-2, 1, 40, 8, 8), (1, 1, -40, 8, 8)):
            eq(call(ok, dims), E_SHAPE, f"{name} dims {dims}")
        eq(call(ok, good, 7), E_DTYPE, f"{name} dtype 7")
        eq(call(ok, (1, 1, 40, 6, 8)), E_ALIGN, f"{name} H=6")
        eq(call(ok, (1, 1, 40, 8, 6)), E_ALIGN, f"{name} Ds=6")
        eq(call(ok, (1 << 16, 1 << 15, 40, 8, 8)), E_SHAPE, f"{name} B*T = 2^31")
        eq(call(ok, (1 << 30, 1 << 30, 40, 8, 8)), E_SHAPE, f"{name} B = T = 2^30")
        eq(call(ok, (1, 1, 40, 1028, 8)), E_SHAPE, f"{name} H=1028")
        assert b"H=1028" in lib.tsg_last_error()
        eq(call(ok, (1, 1, 40, 8, 1028)), E_SHAPE, f"{name} Ds=1028")
        assert b"Ds=1028" in lib.tsg_last_error()
        for dt in (TSG_BF16, TSG_F32S):                                  # the dtypes are accepted: the next check is what fails
            eq(call(ok, (1, 1, nmax + 1, 8, 8), dt), E_SHAPE, f"{name} dtype {dt}")
        if has_ws:                                                      # too small a workspace: refused before any launch
            eq(fn(*ok, 16, 2, 64, 48, 64, 64, TSG_F32, None), E_SHAPE, f"{name} small workspace")
            assert b"workspace" in lib.tsg_last_error()
    # the planner
    ws = lib.tsg_scdm_long_ws_bytes
    for gate in (0, 1):
        for dims in ((1, 1, 1, 4, 4), (2, 64, 48, 512, 512), (128, 128, nmax, 1024, 1024), (2, 20, 32, 128, 128), (1, 33, 128, 260, 516)):
            B, T, N, H, Ds = dims
            got = ws(*dims, gate)
            n[0] += 1
            assert got >= 4 * B * T * N and got > 0, (dims, gate, got)
        for dims in ((1, 1, 0, 4, 4), (1, 1, nmax + 1, 4, 4), (0, 1, 40, 4, 4), (1, 1, 40, 6, 4), (1, 1, 40, 4, 6), (1, 1, 40, 1028, 4),
                     (1, 1, 40, 4, 1028), (1 << 16, 1 << 15, 40, 8, 8), (1 << 30, 1 << 30, 40, 8, 8), (-1, 1, 40, 4, 4)):
            eq(ws(*dims, gate), 0, f"ws_bytes {dims}")
    big_rows = ws((1 << 31) - 1, 1, nmax, 1024, 1024, 1)                 # the largest accepted plan stays a positive long long
    n[0] += 1
    assert big_rows == 4 * ((1 << 31) - 1) * (nmax + 1024), big_rows
    # the 32-word entry points keep their limit
    eq(lib.tsg_scdm_attn_fwd(p, p, p, p, p, p, 1, 1, 33, 4, 4, TSG_F32, None), E_SHAPE, "tsg_scdm_attn_fwd N=33")
    assert b"N=33" in lib.tsg_last_error()
    eq(lib.tsg_scdm_gate_fwd(p, p, p, p, p, p, p, p, 1, 1, 33, 4, 4, TSG_F32, None), E_SHAPE, "tsg_scdm_gate_fwd N=33")
    eq(lib.tsg_scdm_attn_fwd(None, p, p, p, p, p, 1, 1, 33, 4, 4, TSG_F32, None), E_NULL, "tsg_scdm_attn_fwd NULL and N=33")
    assert b"NULL" in lib.tsg_last_error()
    eq(lib.tsg_scdm_bwd_ws_bytes(1, 1, 33, 4, 4, 0), 0, "tsg_scdm_bwd_ws_bytes N=33")
    return n[0]


if __name__ == "__main__":
    lib_ = base.load_standalone(sys.argv[1])
    print(f"{run_checks(lib_)} long-sentence host-side calls clean")

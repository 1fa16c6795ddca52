#!/usr/bin/env python3
"""Event-timed long-sentence K1 / K1g (tsg_scdm_long_*) at [B, T=128, H=Ds=1024] for N in {32, 48, 64, 128}: forward and backward, plain
and gate-fused, fp32 and bf16 storage -- beside the existing 32-word entry points (tsg_scdm_attn_* / tsg_scdm_gate_*, TSG_F32) at N = 32,
the yardstick.  The two families alternate inside each repetition; operands are allocated once (cached operands, event pairs around `iters`
back-to-back launches after a warm-up), so a figure holds launch gaps of a few microseconds per launch (the backward of the long family is
five launches + one zero-fill).

    python tools/k1_long_time.py [--B 128] [--iters 20] [--reps 3] [--out FILE]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from shufflingvideosfortsg_amd import _lib  # noqa: E402
from shufflingvideosfortsg_amd._lib import ptr, TSG_F32, TSG_BF16  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=128)
ap.add_argument("--T", type=int, default=128)
ap.add_argument("--d", type=int, default=1024)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("k1_long_time.py needs a GPU: a time measured elsewhere says nothing")
B, T, d = args.B, args.T, args.d
lib = _lib.load()
dev = "cuda"
st = torch.cuda.current_stream().cuda_stream


def timeit(fn):
    for _ in range(3):
        assert fn() == 0, lib.tsg_last_error()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.iters * 1e3


def operands(N, dt):
    td = torch.bfloat16 if dt == TSG_BF16 else torch.float32
    g = torch.Generator(device=dev).manual_seed(N)
    r_ = lambda *sh: torch.randn(*sh, device=dev, generator=g)
    o = dict(A=r_(B, T, d).to(td), S=r_(B, N, d).to(td), w=r_(d) / d ** 0.5, V=r_(B, N, d).to(td), gb=r_(d) * 0.1, r=r_(B, T, d).to(td),
             dY=r_(B, T, d).to(td))
    o.update(out=torch.empty_like(o["A"]), P=torch.empty(B, T, N, device=dev), da=torch.empty_like(o["A"]), ds=torch.empty_like(o["S"]),
             dw=torch.empty(d, device=dev), dV=torch.empty_like(o["V"]), dgb=torch.empty(d, device=dev), dr=torch.empty_like(o["A"]))
    return o


def calls(o, N, dt, long_):
    """{name: zero-argument launcher} of one family on one operand set."""
    p = {k: ptr(v) for k, v in o.items()}
    if long_:
        nb = max(int(lib.tsg_scdm_long_ws_bytes(B, T, N, d, d, 1)), 16)
        fwd, bwd, gfwd, gbwd = lib.tsg_scdm_long_fwd, lib.tsg_scdm_long_bwd, lib.tsg_scdm_long_gate_fwd, lib.tsg_scdm_long_gate_bwd
    else:
        nb = max(int(lib.tsg_scdm_bwd_ws_bytes(B, T, N, d, d, 1)), int(lib.tsg_scdm_bwd_ws_bytes(B, T, N, d, d, 0)), 16)
        fwd, bwd, gfwd, gbwd = lib.tsg_scdm_attn_fwd, lib.tsg_scdm_attn_bwd, lib.tsg_scdm_gate_fwd, lib.tsg_scdm_gate_bwd
    ws = torch.empty(nb // 4 + 4, device=dev)
    o["ws"] = ws
    return {
        "fwd": lambda: fwd(p["A"], p["S"], p["w"], p["V"], p["out"], p["P"], B, T, N, d, d, dt, st),
        "bwd": lambda: bwd(p["A"], p["S"], p["w"], p["V"], p["P"], p["dY"], p["da"], p["ds"], p["dw"], p["dV"], ptr(ws), nb, B, T, N, d, d, dt, st),
        "gate fwd": lambda: gfwd(p["A"], p["S"], p["w"], p["V"], p["gb"], p["r"], p["out"], p["P"], B, T, N, d, d, dt, st),
        "gate bwd": lambda: gbwd(p["A"], p["S"], p["w"], p["V"], p["gb"], p["r"], p["P"], p["dY"], p["da"], p["ds"], p["dw"], p["dV"], p["dgb"],
                                 p["dr"], ptr(ws), nb, B, T, N, d, d, dt, st),
    }


KINDS = ("fwd", "bwd", "gate fwd", "gate bwd")
lines = [f"# tools/k1_long_time.py  B={B} T={T} H=Ds={d}  iters={args.iters} reps={args.reps}  device={torch.cuda.get_device_name(0)}",
         "# microseconds per call (median of the repetitions; min..max in brackets)"]
res = {}
base_o = operands(32, TSG_F32)
base = calls(base_o, 32, TSG_F32, False)
for N in (32, 48, 64, 128):
    for dt, dname in ((TSG_F32, "fp32"), (TSG_BF16, "bf16")):
        o = operands(N, dt)
        c = calls(o, N, dt, True)
        acc = {k: [] for k in KINDS}
        bacc = {k: [] for k in KINDS}
        for _ in range(args.reps):                         # the two families alternate
            for k in KINDS:
                acc[k].append(timeit(c[k]))
                if N == 32 and dt == TSG_F32:
                    bacc[k].append(timeit(base[k]))
        for k in KINDS:
            v = sorted(acc[k])
            res[(N, dname, k)] = v[len(v) // 2]
            lines.append(f"long      N={N:3d} {dname} {k:8s}: {v[len(v) // 2]:9.1f}  [{v[0]:.1f} .. {v[-1]:.1f}]")
        if bacc["fwd"]:
            for k in KINDS:
                v = sorted(bacc[k])
                res[("base", k)] = v[len(v) // 2]
                lines.append(f"existing  N= 32 fp32 {k:8s}: {v[len(v) // 2]:9.1f}  [{v[0]:.1f} .. {v[-1]:.1f}]   (tsg_scdm_attn_* / tsg_scdm_gate_*, TSG_F32)")
        del o, c
        torch.cuda.empty_cache()
lines.append("# ratios against the existing strict-fp32 kernels at N = 32 (work scales with N: the allowance at N is 2 x N / 32)")
for N in (32, 48, 64, 128):
    for dname in ("fp32", "bf16"):
        lines.append(f"long N={N:3d} {dname}: " + "   ".join(f"{k} {res[(N, dname, k)] / res[('base', k)]:.2f}x (allowance {2 * N / 32:.1f}x)" for k in KINDS))
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")

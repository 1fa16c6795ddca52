#!/usr/bin/env python3
"""A/B of the shuffling-augmentation kernels between two builds of libtsg_hip.so at [64, 128, 1024] fp32: tsg_moment_translate
(insert positions given) and tsg_moment_augment (mode gt_translate, the same positions as plans).  Spans end before nfeats -- the
inputs every existing caller passes -- so both builds must produce the same bytes; the output's SHA-1 is reported to show it.

Each measurement is one fresh process (--lib PATH): 200 back-to-back launches through ctypes between two events, median of 5.
--ab A B --rounds R alternates the two libraries A, B, A, B, ... in R rounds and prints one JSON line per run and a summary.

Usage:  python tools/translate_ab_time.py --ab tools/_ablate/parent.so shufflingvideosfortsg_amd/libtsg_hip.so --rounds 4
"""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys

B, T, D, REPS = 64, 128, 1024, 200


def measure(path):
    import numpy as np
    import torch
    lib = ctypes.CDLL(path)
    P, I = ctypes.c_void_p, ctypes.c_int
    lib.tsg_moment_translate.argtypes = [P] * 4 + [ctypes.c_uint64, P, P] + [I] * 4 + [P]
    lib.tsg_moment_augment.argtypes = [P, P, P, I, ctypes.c_double, ctypes.c_uint64] + [P] * 5 + [I] * 4 + [P]
    rs = np.random.RandomState(0)
    nf = rs.randint(T // 2, T + 1, size=B)
    s = np.array([rs.randint(0, k - 1) for k in nf]); e = np.array([rs.randint(a + 1, k) for a, k in zip(s, nf)])
    c = np.array([rs.randint(0, k - (b - a + 1) + 1) for a, b, k in zip(s, e, nf)])
    dev = torch.device("cuda")
    video = torch.randn(B, T, D, generator=torch.Generator().manual_seed(1)).to(dev)
    spans = torch.from_numpy(np.stack([s, e], 1).astype(np.int32)).to(dev)
    nfd, cd = (torch.from_numpy(x.astype(np.int32)).to(dev) for x in (nf, c))
    plan = torch.from_numpy(np.stack([np.ones(B), c, 0 * c, 0 * c], 1).astype(np.int32)).to(dev)
    out, new_sp, new_nf, plan_out = torch.empty_like(video), torch.empty(B, 2, dtype=torch.int32, device=dev), \
        torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, 4, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    calls = {
        "tsg_moment_translate": lambda: lib.tsg_moment_translate(video.data_ptr(), spans.data_ptr(), nfd.data_ptr(), cd.data_ptr(), 0,
                                                                 out.data_ptr(), new_sp.data_ptr(), B, T, D, 0, st),
        "tsg_moment_augment": lambda: lib.tsg_moment_augment(video.data_ptr(), spans.data_ptr(), nfd.data_ptr(), 0, 1.0, 0,
                                                             plan.data_ptr(), plan_out.data_ptr(), out.data_ptr(), new_sp.data_ptr(),
                                                             new_nf.data_ptr(), B, T, D, 0, st),
    }
    res = {"lib": path, "shape": [B, T, D]}
    for name, fn in calls.items():
        for _ in range(20):
            assert fn() == 0, name
        ts = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                fn()
            e1.record(); torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / REPS)
        res[name + "_us"] = round(float(np.median(ts)), 3)
        res[name + "_sha1"] = hashlib.sha1(out.cpu().numpy().tobytes() + new_sp.cpu().numpy().tobytes()).hexdigest()[:16]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib")
    ap.add_argument("--ab", nargs=2)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.lib:
        return measure(a.lib)
    runs = []
    for r in range(a.rounds):
        for tag, path in zip("AB", a.ab):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", path], capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"run {tag}{r} failed (rc {p.returncode}):\n{p.stderr[-2000:]}")
            res = dict(json.loads(p.stdout.strip().splitlines()[-1]), run=f"{tag}{r}")
            print(json.dumps(res), flush=True)
            runs.append(res)
    summary = {"summary": True}
    for k in ("tsg_moment_translate", "tsg_moment_augment"):
        for tag in "AB":
            summary[f"{k}_{tag}_us"] = sorted(x[k + "_us"] for x in runs if x["run"][0] == tag)
        summary[f"{k}_same_output"] = len({x[k + "_sha1"] for x in runs}) == 1
    print(json.dumps(summary), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(x) + "\n" for x in runs + [summary])


if __name__ == "__main__":
    main()

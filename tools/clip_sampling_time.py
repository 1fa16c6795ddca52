#!/usr/bin/env python3
"""Time tsg_sample_clips per mode at the user shapes (ANet [64, 240, 1024] / [64, 240, 500], Charades [64, 128, 1024]; clip
counts 1 .. ~10 T): one launch (CUDA events, median of --reps), algorithmic bytes = the raw rows the windows read + B*T*D
written, the fraction of 8 TB/s; against the same output built in torch (a precomputed window index, gather, masked mean) and,
as context only, the reference-style per-sample numpy loop on the host with 16 threads.  One JSON line per (shape, mode).

Usage:  python tools/clip_sampling_time.py [--reps 50] [--out profiles/sampling/clip_sampling_time.jsonl]
The kernel's own duration: run the tool under `rocprofv3 --kernel-trace --stats -d DIR -o sampling -- python
tools/clip_sampling_time.py --reps 5`, then join that trace with the byte counts:
        python tools/clip_sampling_time.py --join-trace DIR/sampling_results.db --reps 5 --timing T.jsonl --out-dir profiles/sampling
which writes clip_sampling_kernel_times.jsonl (median kernel duration per shape / mode / dtype, fraction of 8 TB/s) and
rocprofv3_kernel_stats.csv (calls and durations per kernel name).
"""
import collections
import sqlite3
import statistics
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from shufflingvideosfortsg_amd import data  # noqa: E402

SHAPES = [(64, 240, 1024), (64, 240, 500), (64, 128, 1024)]


def batch(B, T, D, seed):
    rs = np.random.RandomState(seed)
    n = rs.randint(1, 10 * T + 1, size=B)
    off = np.concatenate([[0], np.cumsum(n)])
    dur = np.round(n / np.exp(rs.uniform(np.log(0.3), np.log(12.0), size=B)), 2)
    ts = np.sort(rs.uniform(0.0, 1.0, size=(B, 2)) * dur[:, None], axis=1)
    return torch.randn(int(off[-1]), D, generator=torch.Generator().manual_seed(seed)), off, n, dur, ts


def windows(raw, off, n, dur, ts, T, mode, spos):
    """(lo [B,T], cnt [B,T]) of every output row, from the numpy mirrors' rules (row index = the window's first raw row)."""
    B = len(n)
    lo, cnt = np.zeros((B, T), np.int64), np.zeros((B, T), np.int64)
    for b in range(B):
        k = int(n[b])
        for t in range(T):
            if mode == "pair" and 2 * t < k:
                lo[b, t], cnt[b, t] = 2 * t, min(2, k - 2 * t)
            elif mode == "triple" and 3 * t < k:
                lo[b, t], cnt[b, t] = 3 * t, min(3, k - 3 * t)
            elif mode == "1to1" and t < k:
                lo[b, t], cnt[b, t] = t, 1
            elif mode in ("f2s", "f2s_114") and t < dur[b]:
                rate = k / dur[b]
                if mode == "f2s":
                    lo[b, t], cnt[b, t] = min(k - 1, int(np.floor(t * rate))), 1
                else:
                    s, e = min(k - 1, int(t * rate + 0.5)), int((t + 1) * rate + 0.5)
                    lo[b, t], cnt[b, t] = (s, 1) if e > k or e <= s else (s, e - s)
        if mode == "lg":
            s = data.lg_positions(k, T, int(spos[b]))
            lo[b, :len(s)], cnt[b, :len(s)] = s, 1
    return lo + off[:-1, None], cnt


def event_time(fn, reps):
    """Mean time of one call over ``reps`` back-to-back calls between two events (median of 5 such runs), in us.  The host
    issues a call in ~20 us; where the kernel is shorter this is the issue rate -- the rocprofv3 run beside it
    (profiles/sampling/) has the kernel's own duration."""
    for _ in range(5):
        fn()
    ts = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / reps)
    return float(np.median(ts))


def join_trace(db, timing, reps, out_dir):
    """The rocprofv3 trace of one run of this tool (--reps ``reps``) joined with the byte counts of ``timing`` (this tool's JSON
    lines at the same shapes and seeds).  sample_clips_kernel dispatches come in the tool's order: per (shape, mode), fp32 then
    bf16, each 5 warm-up calls + 5 x reps timed ones; the warm-up calls are dropped."""
    c = sqlite3.connect(db)
    rows = c.execute("select name, duration from kernels order by start").fetchall()
    runs = [json.loads(x) for x in open(timing)]
    per, samp = 5 + 5 * reps, [r for r in rows if "sample_clips_kernel" in r[0]]
    assert len(samp) == 2 * per * len(runs), (len(samp), len(runs))
    out, i = [], 0
    for t in runs:
        B, T, D = t["shape"]
        for dt in ("fp32", "bf16"):
            chunk = samp[i:i + per]; i += per
            assert all(("bf16" in r[0]) == (dt == "bf16") for r in chunk), (t["mode"], dt)
            d = [r[1] / 1000 for r in chunk[5:]]
            wb = t["bytes"] - (B * T * D * 2 if dt == "bf16" else 0)
            med = statistics.median(d)
            out.append(dict(shape=t["shape"], mode=t["mode"], dtype=dt, kernel_us_median=round(med, 2), kernel_us_min=round(min(d), 2),
                            bytes=wb, frac_8TBps=round(wb / (med * 1e-6) / 8e12, 3), torch_build_us=t["torch_us"],
                            host_numpy16_us=t["host_numpy16_us"]))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "clip_sampling_kernel_times.jsonl"), "w") as f:
        f.writelines(json.dumps(r) + "\n" for r in out)
    agg = collections.defaultdict(list)
    for n, d in rows:
        agg[n].append(d)
    tot = sum(sum(v) for v in agg.values())
    with open(os.path.join(out_dir, "rocprofv3_kernel_stats.csv"), "w") as f:
        f.write('"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs"\n')
        for n, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
            f.write(f'"{n}",{len(v)},{sum(v)},{sum(v) / len(v):.1f},{100 * sum(v) / tot:.2f},{min(v)},{max(v)}\n')
    for r in out:
        print(json.dumps(r))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--join-trace", default=None, help="rocprofv3 results .db of a run of this tool with the same --reps")
    ap.add_argument("--timing", default=None, help="with --join-trace: this tool's JSON lines (byte counts)")
    ap.add_argument("--out-dir", default="profiles/sampling")
    a = ap.parse_args()
    if a.join_trace:
        return join_trace(a.join_trace, a.timing, a.reps, a.out_dir)
    lines = []
    for B, T, D in SHAPES:
        raw, off, n, dur, ts = batch(B, T, D, seed=T + D)
        rd = raw.cuda()
        offd, tsd, dud = (torch.as_tensor(x).cuda() for x in (off, ts, dur))              # resident: no copy inside the timing
        for mode in data.SAMPLE_MODES:
            spos = data.lg_spos_draws(1, n, T) if mode == "lg" else np.zeros(B, np.int32)
            lo, cnt = windows(raw, off, n, dur, ts, T, mode, spos)
            nbytes = (int(cnt.sum()) + B * T) * D * 4
            res = {"shape": [B, T, D], "mode": mode, "bytes": nbytes}
            for dt, key in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
                us = event_time(lambda: data.sample_clips_device(rd, offd, T, mode, tsd, dud, train=mode == "lg", seed=1, out_dtype=dt), a.reps)
                wb = nbytes - (B * T * D * 2 if dt == torch.bfloat16 else 0)
                res[f"{key}_us"] = round(us, 2)
                res[f"{key}_frac_8TBps"] = round(wb / (us * 1e-6) / 8e12, 3)
            W = max(1, int(cnt.max()))
            idx = torch.from_numpy(lo[..., None] + np.arange(W)).cuda()                       # [B,T,W] precomputed window index
            valid = torch.from_numpy(np.arange(W) < cnt[..., None]).cuda()
            c = torch.from_numpy(np.maximum(cnt, 1)).float().cuda()
            idx = torch.where(valid, idx, torch.zeros_like(idx))

            def torch_build():
                g = rd[idx.reshape(-1)].reshape(B, T, W, D) * valid[..., None]
                return g.sum(2) / c[..., None]
            res["torch_us"] = round(event_time(torch_build, max(5, a.reps // 5)), 2)
            rawn = raw.numpy()

            def host():
                with ThreadPoolExecutor(16) as ex:
                    list(ex.map(lambda b: data.sample_clips_numpy(rawn[off[b]:off[b + 1]], ts[b].tolist(), float(dur[b]), T, mode,
                                                                  int(spos[b])), range(B)))
            t0 = time.perf_counter(); host(); res["host_numpy16_us"] = round((time.perf_counter() - t0) * 1e6, 1)
            print(json.dumps(res), flush=True)
            lines.append(res)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in lines)


if __name__ == "__main__":
    main()

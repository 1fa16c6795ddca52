#!/usr/bin/env python3
"""Developer tool: tsg_moment_augment (csrc/augment.hip) per mode vs a torch gather baseline with identical output.

    python tools/augment_time.py [--iters N] [--reps R]

Shapes: [B=64, T=128, D=1024] (Charades) fp32 and bf16, and ANet's T=240.  One process, device events, warm-up first.  Per shape and
mode, in alternating repetitions of N back-to-back launches each:
  * own    tsg_moment_augment through its raw ctypes entry point (buffers preallocated, plans drawn by the kernel);
  * gather the same outputs by torch.gather from a video with one zero row appended, with the [B,T,D] int64 index precomputed
           from the plans the kernel drew (the row map of op 0-3; the zero row for deleted / padding rows).
The outputs are compared once (bit-exact).  Also printed: the kernel alone, bracketed by its own event pair (tsg_time_next_launch).
Bytes = source rows actually read + B*T*D written, times the element size; fraction of the 8 TB/s HBM peak.  Prints one line per
(shape, dtype, mode) and a JSON summary line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from shufflingvideosfortsg_amd import _lib, data  # noqa: E402

PEAK = 8.0e12
MODES = ["gt_translate", "gt_crop", "prot_gt_crop", "gt_cropout", "all", None]


def row_map(spans, nfeats, plans, T):
    """[B,T] source row of every output row (-1: zero row), from the plans through the numpy functions."""
    src = np.empty((len(plans), T), np.int64)
    rows = np.arange(1, T + 1, dtype=np.float64)[None, :, None]
    for b, pl in enumerate(plans):
        _, _, o = data.apply_plan(list(spans[b]), int(nfeats[b]), rows, pl)
        src[b] = o[0, :, 0].astype(np.int64) - 1
    return src


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    lib = _lib.load()
    fn = lib.tsg_moment_augment
    results = []
    for B, T, D, dt in ((64, 128, 1024, torch.float32), (64, 128, 1024, torch.bfloat16), (64, 240, 1024, torch.float32),
                        (64, 240, 1024, torch.bfloat16)):
        host = data.synthetic_batch(B, T, 4, video_dim=D, seed=17)
        spans = np.array(host["gt"]["framestps"], np.int32); nfs = np.asarray(host["nfeats"], np.int32)
        video = host["video"].to(dt).cuda()
        sp, nf = torch.from_numpy(spans).cuda(), torch.from_numpy(nfs).cuda()
        out = torch.empty_like(video)
        new_sp = torch.empty(B, 2, dtype=torch.int32, device="cuda"); new_nf = torch.empty(B, dtype=torch.int32, device="cuda")
        plan = torch.empty(B, 4, dtype=torch.int32, device="cuda")
        vpad = torch.cat([video, torch.zeros(B, 1, D, dtype=dt, device="cuda")], 1)
        gout = torch.empty_like(video)
        dtype = _lib.TSG_F32 if dt == torch.float32 else _lib.TSG_BF16
        stream = torch.cuda.current_stream().cuda_stream
        esize = video.element_size()
        for mode in MODES:
            code = data.aug_mode_code(mode)

            def own():
                rc = fn(video.data_ptr(), sp.data_ptr(), nf.data_ptr(), code, 1.0, 5, None, plan.data_ptr(), out.data_ptr(),
                        new_sp.data_ptr(), new_nf.data_ptr(), B, T, D, dtype, stream)
                assert rc == 0, rc
            own(); torch.cuda.synchronize()
            plans = plan.cpu().numpy()
            src = row_map(spans, nfs, plans, T)
            idx = torch.from_numpy(np.where(src < 0, T, src)).cuda()[:, :, None].expand(B, T, D).contiguous()

            def gather():
                torch.gather(vpad, 1, idx, out=gout)
            gather(); torch.cuda.synchronize()
            assert torch.equal(out, gout), (mode, dt, T)
            for _ in range(3):
                own(); gather()
            torch.cuda.synchronize()
            t_own, t_gather = [], []
            for _ in range(a.reps):                             # alternating repetitions
                t_own.append(timed(own, a.iters)); t_gather.append(timed(gather, a.iters))
            alone = []
            for _ in range(a.reps):
                assert lib.tsg_time_next_launch(0) == 0
                own()
                us = ctypes.c_float()
                assert lib.tsg_timed_launch_us(0, ctypes.byref(us)) == 0
                alone.append(us.value)
            rows_read = int((src >= 0).sum())
            nbytes = (rows_read + B * T) * D * esize
            r = dict(B=B, T=T, D=D, dtype=str(dt).replace("torch.", ""), mode=str(mode), own_us=statistics.median(t_own),
                     own_alone_us=statistics.median(alone), gather_us=statistics.median(t_gather), mbytes=nbytes / 1e6)
            r["hbm_fraction"] = nbytes / (r["own_us"] * 1e-6) / PEAK
            r["hbm_fraction_alone"] = nbytes / (r["own_alone_us"] * 1e-6) / PEAK
            r["speedup_vs_gather"] = r["gather_us"] / r["own_us"]
            results.append(r)
            print(f"[{B},{T},{D}] {r['dtype']:8s} {str(mode):12s}  own {r['own_us']:7.2f} us (alone {r['own_alone_us']:7.2f})  "
                  f"gather {r['gather_us']:7.2f} us  x{r['speedup_vs_gather']:.2f}  {r['mbytes']:.1f} MB  "
                  f"{r['hbm_fraction']:.3f} of 8 TB/s (alone {r['hbm_fraction_alone']:.3f})", flush=True)
    print(json.dumps({"device": torch.cuda.get_device_name(0), "results": results}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Developer tool: the boundary head on TALL's fusion (cross_name 'c'), fused (tsg_boundary_head_tall_gemm) against the routing it replaces
(the [B,T,4d] concat, the gated copy, Linear over 4d, K3), in the f32s mode on one MI355X.

    python tools/tall_head_time.py --ab 3 [--out FILE]            alternating fresh processes: parent, fused, parent, fused, ...
    python tools/tall_head_time.py --route fused|parent            one process, one JSON line per (shape, measurement)

Per shape [B, T, d, Hm] ([64,128,1024,256] and [64,240,1024,256]): `fwd` the head's forward under no_grad, `fwd_bwd` the head alone forward +
backward, `gmd_step` the full GMD forward + backward with cross_name 'c' (B pairs; default widths, dropout off).  Each window is >= 0.2 s of
device events over rotating operand sets (4 sets: 134 MB of clips each at the first shape, so no set is warm in the caches); `fused`
lines also carry the new GEMM's share of the nominal bf16 peak, counted as 3 x 2 M 2Hm 2Dv over the event time of the entry point alone
(GEMM + softmax launch).  'parent' makes ``MLP_predictor.forward_fused`` decline, which is the code path of the commit before the fused form."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(64, 128, 1024, 256), (64, 240, 1024, 256)]
PEAK_BF16 = 2.5e15            # nominal dense bf16 matrix rate of one MI355X, FLOP/s


def _events(fn, min_s=0.2, reps=5):
    """Median over ``reps`` windows of the mean time of fn(i) in ms (device events; each window runs for at least min_s)."""
    import torch
    for i in range(4):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter(); fn(0); torch.cuda.synchronize()
    n = max(4, int(min_s / max(time.perf_counter() - t0, 1e-5)))
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(n):
            fn(i)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / n)
    out.sort()
    return out[len(out) // 2], out[0], out[-1], n


def run(route):
    sys.path.insert(0, ROOT)
    import torch
    from shufflingvideosfortsg_amd import data, engine, functional as TF
    from shufflingvideosfortsg_amd.model.components import CrossModalInteraction as CMI
    from shufflingvideosfortsg_amd.model.components.SpanPredictor import MLP_predictor, SpanPredictor_Boundary
    if not torch.cuda.is_available():
        raise SystemExit("tall_head_time: no GPU visible (there is nothing to time on a CPU)")
    if route == "parent":
        MLP_predictor.forward_fused = lambda self, kind, *a, **k: self.forward_split(*a, **k) if kind == "vs" else None
    engine.set_precision("f32s")
    for B, T, d, Hm in SHAPES:
        torch.manual_seed(0)
        head = SpanPredictor_Boundary(4 * d, dict(name="mlp", mlp_hidden_dim=Hm), 0.0, None).cuda()
        cmi = CMI.TALL(d, d)
        sets = [(torch.randn(B, T, d, device="cuda"), torch.randn(B, d, device="cuda"), torch.randn(B, T, device="cuda") * 2) for _ in range(4)]
        assert head.predictor.fused_form("tall", B, T, d, d) == "tall", "the timed shapes must be ones the fused form takes"

        def emit(what, t, **extra):
            print(json.dumps(dict(route=route, shape=[B, T, d, Hm], what=what, ms=round(t[0], 4), ms_min=round(t[1], 4), ms_max=round(t[2], 4),
                                  calls_per_window=t[3], **extra)), flush=True)

        def fwd(i):
            v, s, g = sets[i % 4]
            with torch.no_grad():
                return head.forward_cmi(cmi, v, None, s, g, None)
        emit("fwd", _events(fwd))
        leaves = [(v.clone().requires_grad_(True), s.clone().requires_grad_(True), g.clone().requires_grad_(True)) for v, s, g in sets]

        def fwd_bwd(i):
            v, s, g = leaves[i % 4]
            ps, pe = head.forward_cmi(cmi, v, None, s, g, None)
            (ps[:, 0].sum() + pe[:, -1].sum()).backward()
            for t in (v, s, g, *head.parameters()):
                t.grad = None
        emit("fwd_bwd", _events(fwd_bwd))
        if route == "fused":                                   # the entry point alone: its share of the nominal peak
            from shufflingvideosfortsg_amd._lib import load, ptr
            lib, st = load(), torch.cuda.current_stream().cuda_stream
            Ws, We = head.predictor.start_mlp_1.weight.detach(), head.predictor.end_mlp_1.weight.detach()
            Wv = torch.cat([Ws[:, :d] + Ws[:, 3 * d:], We[:, :d] + We[:, 3 * d:]], 0).contiguous()
            cs = torch.zeros(B, 2 * Hm, device="cuda"); vec = torch.randn(2 * Hm, device="cuda")
            nb = int(lib.tsg_head_gemm_ws_bytes(B * T, 2 * Hm, 2)); ws = torch.empty(max(nb, 16), device="cuda", dtype=torch.uint8)
            ps, pe = torch.empty(B, T, device="cuda"), torch.empty(B, T, device="cuda")

            def entry(i):
                v, s, g = sets[i % 4]
                rc = lib.tsg_boundary_head_tall_gemm(ptr(v), d, ptr(Wv), ptr(Ws) + 8 * d, ptr(We) + 8 * d, 4 * d, ptr(s), ptr(cs), ptr(vec), ptr(vec),
                                                     ptr(vec), ptr(g), None, None, ptr(ps), ptr(pe), ptr(ws), nb, B, T, Hm, d, st)
                assert rc == 0, lib.tsg_last_error()
            t = _events(entry)
            flop = 3 * 2 * (B * T) * (2 * Hm) * (2 * d)
            emit("entry_point", t, bf16_flop=flop, share_of_nominal_bf16_peak=round(flop / (t[0] * 1e-3) / PEAK_BF16, 4))
        del sets, leaves
        params = engine.default_params(video_rnn_hiddendim=d // 2, sent_rnn_hiddendim=d // 2, mlp_hidden_dim=Hm, dropout=0.0, video_len=T,
                                       sent_len=20, crossmodal="c")
        torch.manual_seed(0)
        model = engine.build_model("gmd", params).cuda().train()
        for m_ in model.modules():
            if isinstance(m_, torch.nn.Dropout):
                m_.p = 0.0
        batches = [data.synthetic_batch(B, T, 20, seed=5 + k, pair=True, device="cuda") for k in range(2)]

        def step(i):
            loss = engine.gmd_step(model, batches[i % 2], params)[0]
            loss.backward()
            for p in model.parameters():
                p.grad = None
        emit("gmd_step", _events(step, min_s=0.5, reps=3))
        TF.check_kernel_errors()
        del model, batches
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=["fused", "parent"])
    ap.add_argument("--ab", type=int, default=0, help="rounds of (parent, fused) in fresh processes")
    ap.add_argument("--out", default=None, help="append the raw lines to this file as well")
    a = ap.parse_args()
    if a.route:
        return run(a.route)
    if a.ab < 1:
        ap.error("give --route or --ab N")
    for r in range(a.ab):
        for route in ("parent", "fused"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--route", route], capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"tall_head_time: the {route} process of round {r} ended with {p.returncode}")
            lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
            for l in lines:
                l = json.dumps(dict(json.loads(l), round=r))
                print(l, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(l + "\n")


if __name__ == "__main__":
    main()

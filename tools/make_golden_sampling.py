#!/usr/bin/env python3
"""Generate tests/golden/clip_sampling.npz by running the REAL reference's clip samplers (dataset/charades.py, dataset/anet.py).

Runs only where the reference is checked out (``--ref``: its grounding/ directory), with the ``h5py`` stub of
oracle/make_golden.py.  The reference is imported, never copied.  Its six samplers are called UNBOUND with a stub ``self``
(SAMPLE_LEN, split, vfeat_fname) -- no annotation or feature file is read.  LG's training draw goes through a wrapper around
``np.random.random_integers`` that records the inclusive range asked for and forces or records the value returned.
Stored per case: mode (TSG_SAMPLE_*), T, n, duration, timestamps, the raw clips (float32, D = 8), the spos used and its
range, and the reference's outputs (video [T, D], framestamps, nfeats).  Also stored: ``_lg_frame2sec`` on the collate's
dtypes, and ``DataAugmentForTSG.gt_moment_translate`` (insert position forced) and the crop family (gt_crop, prot_gt_crop,
gt_cropout; draws recorded) on LG spans that end past nfeats.

Usage:  python tools/make_golden_sampling.py --ref REFERENCE/grounding
"""
import argparse
import os
import random
import sys
import types

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "clip_sampling.npz")
MODE = {"pair": 0, "triple": 1, "1to1": 2, "f2s": 3, "f2s_114": 4, "lg": 5}
D = 8

# (mode, T, n, duration, timestamps, split, forced spos or None = drawn)
CASES = (
    [("pair", 8, n, 30.0, [1.5, 6.2], "train", None) for n in (1, 2, 3, 4, 5, 15, 16, 17, 40)]      # n mod 2; n below / at / above 2T
    + [("triple", 8, n, 30.0, [0.0, 3.9], "train", None) for n in (1, 2, 3, 4, 5, 6, 23, 24, 25, 40)]   # n mod 3; at / above 3T
    + [("1to1", 8, n, 30.0, [2.0, 7.0], "train", None) for n in (3, 8, 20)]
    + [("f2s", 8, 4, 10.0, [1.0, 9.5], "train", None),       # rate < 1
       ("f2s", 8, 20, 6.5, [0.4, 5.7], "train", None),       # fractional duration
       ("f2s", 8, 30, 12.0, [3.0, 11.0], "train", None),     # duration above T
       ("f2s", 8, 40, 5.0, [-2.5, 3.0], "train", None),      # n > T, negative timestamp
       ("f2s", 8, 7, 7.0, [3.0, 50.0], "train", None)]       # timestamp beyond the duration
    + [("f2s_114", 8, 4, 10.0, [1.0, 9.5], "train", None),   # rate < 1: end <= start -> copies
       ("f2s_114", 8, 9, 7.3, [0.4, 5.7], "train", None),    # end > n on the last row, fractional duration
       ("f2s_114", 8, 30, 12.0, [3.0, 11.0], "train", None), # duration above T, nfeats = n = 30 > T
       ("f2s_114", 8, 13, 4.0, [-1.5, 3.0], "train", None),  # windows of 3-4 clips, negative timestamp
       ("f2s_114", 8, 5, 5.0, [2.0, 60.0], "train", None),   # rate 1, timestamp beyond the duration
       ("f2s_114", 8, 57, 9.7, [2.0, 8.0], "train", None)]   # n > T, windows of ~6 clips
    + [("lg", 8, 5, 4.0, [1.0, 4.0], "test", None),          # n < T; start exactly on s[1], moment ending at the video's end
       ("lg", 8, 8, 16.0, [2.0, 10.0], "test", None),        # n == T
       ("lg", 8, 100, 50.0, [12.3, 31.9], "test", None),     # n >> T, test split: spos 0
       ("lg", 8, 100, 50.0, [12.3, 31.9], "train", 11),      # stride 12.5: random_end 12 integral -> [0, 11], spos at the top
       ("lg", 8, 12, 6.0, [1.0, 5.0], "train", None),        # stride 1.5: random_end 1 integral -> [0, 0]
       ("lg", 8, 21, 10.0, [2.0, 7.0], "train", 2),          # stride 2.625 -> [0, 2], spos at the top
       ("lg", 8, 5, 4.0, [0.5, 3.0], "train", None),         # n < T in training: random_integers(0, 0.5) -> 0
       ("lg", 8, 60, 20.0, [-3.0, 25.0], "train", None),     # timestamps outside [0, duration]
       ("lg", 6, 17, 8.0, [1.0, 6.0], "train", 2),           # arange's start + i*((start+step)-start) != start + i*step at i=3
       ("lg", 6, 23, 8.0, [1.0, 6.0], "train", 1),           # ... (rint differs)
       ("lg", 30, 303, 100.0, [10.0, 90.0], "train", 6),     # a fused start + i*delta rounds element 25 the other way
       ("lg", 8, 41, 13.0, [4.0, 13.0], "train", None)]      # drawn spos
)
LG_F2S = [  # _lg_frame2sec: pred (float32, as test.py passes pred_time.float()), durations, nfeats
    ([[0, 7], [3, 5], [1, 1], [2, 7]], [31.7, 12.25, 100.0, 7.3], [8, 5, 8, 3])]
# gt_moment_translate on LG spans that end at or past nfeats: (T, [s, e], nfeats, cropin)
TRANSLATE = [(16, [7, 15], 10, 1), (16, [5, 15], 12, 0), (16, [5, 15], 12, 1), (16, [9, 15], 12, 2), (16, [3, 12], 10, 1),
             (16, [3, 9], 10, 2)]                            # the last one: e < nfeats, the ordinary case
# the crop family on LG spans that end past nfeats: (function, [s, e], nfeats, forced random.randint values, None = drawn); T = 16
CROP = [("gt_crop", [7, 15], 10, []), ("prot_gt_crop", [7, 15], 10, []), ("gt_cropout", [7, 15], 10, []),
        ("gt_crop", [5, 15], 12, []), ("prot_gt_crop", [5, 15], 12, []), ("gt_cropout", [5, 15], 12, [None, None, 0]),
        ("gt_crop", [9, 15], 12, [4, 12]),                  # the widest crop at its last start: deletes rows 12..15
        ("prot_gt_crop", [9, 15], 12, []), ("gt_cropout", [9, 15], 12, []),
        ("gt_cropout", [6, 15], 8, [2]),                     # e far past nfeats: candidates on the left only
        ("gt_cropout", [3, 15], 8, [2])]                     # ... and none: the crop fallback with the drawn (w, start)
CROP_FN = {"gt_crop": 1, "prot_gt_crop": 2, "gt_cropout": 3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout's grounding/ directory")
    a = ap.parse_args()
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    sys.path.insert(0, a.ref)
    import torch
    from dataset.anet import ANetDataSentence
    from dataset.charades import CharadesDataSentence
    from dataset.data_augment import DataAugmentForTSG
    fn = {"pair": CharadesDataSentence.generate_video_fts_data, "triple": CharadesDataSentence.lg_generate_video_fts_data,
          "1to1": ANetDataSentence.sample_1to1_video_feat, "f2s": ANetDataSentence.sample_frame2second,
          "f2s_114": ANetDataSentence.sample_frame2second_114, "lg": ANetDataSentence.lg_get_fixed_length_feat}

    real_ri = np.random.random_integers
    draw_src = np.random.RandomState(5)
    vid_src = np.random.RandomState(17)
    f = {k: [] for k in ("mode", "T", "n", "dur", "ts", "spos", "spos_hi", "fs", "nfeats", "raw_off", "out_off")}
    raws, outs = [], []
    f["raw_off"].append(0); f["out_off"].append(0)
    for mode, T, n, dur, ts, split, forced in CASES:
        rec = {}

        def random_integers(lo, hi):
            rec["hi"] = int(hi)
            v = forced if forced is not None else int(draw_src.randint(int(lo), int(hi) + 1))
            assert lo <= v <= int(hi), (mode, n, T, lo, hi, v)
            rec["v"] = v
            return np.int64(v)

        stub = types.SimpleNamespace(SAMPLE_LEN=T, split=split, vfeat_fname="lg" if mode == "lg" else mode)
        raw = vid_src.randn(n, D).astype(np.float32)
        np.random.random_integers = random_integers
        try:
            out, fs, nf = fn[mode](stub, raw, list(ts), dur)
        finally:
            np.random.random_integers = real_ri
        out = np.asarray(out)[0]
        assert np.array_equal(out.astype(np.float32).astype(np.float64), out)   # float32 values stored in float64
        f["mode"].append(MODE[mode]); f["T"].append(T); f["n"].append(n); f["dur"].append(dur); f["ts"].append(list(ts))
        f["spos"].append(rec.get("v", 0)); f["spos_hi"].append(rec.get("hi", -1))
        f["fs"].append([int(fs[0]), int(fs[1])]); f["nfeats"].append(int(nf))
        raws.append(raw); outs.append(out.astype(np.float32).reshape(-1))
        f["raw_off"].append(f["raw_off"][-1] + n); f["out_off"].append(f["out_off"][-1] + T * D)

    pred, durs, nfs = LG_F2S[0]
    stub = types.SimpleNamespace(vfeat_fname="lg")
    sec = ANetDataSentence._lg_frame2sec(stub, torch.tensor(pred).float(), torch.from_numpy(np.array(durs)),
                                         torch.from_numpy(np.array(nfs)))
    sec_ch = CharadesDataSentence._lg_frame2sec(stub, torch.tensor(pred).float(), torch.from_numpy(np.array(durs)),
                                                torch.from_numpy(np.array(nfs)))
    assert torch.equal(sec, sec_ch) and sec.dtype == torch.float64

    real_randint = random.randint
    tr = {k: [] for k in ("fs", "nfeats", "cropin", "video", "out_fs", "out_video")}
    aug = DataAugmentForTSG(0, 1.0, "gt_translate")
    for T, fs, nf, c in TRANSLATE:
        video = np.zeros((1, T, D))
        video[0] = vid_src.randn(T, D).astype(np.float32)      # rows past nfeats carry content too (the BiLSTM reads them)
        random.randint = lambda lo, hi, c=c: (c if lo <= c <= hi else (_ for _ in ()).throw(AssertionError((lo, hi, c))))
        try:
            ofs, onf, ov = aug.gt_moment_translate(list(fs), nf, video.copy())
        finally:
            random.randint = real_randint
        assert onf == nf
        tr["fs"].append(fs); tr["nfeats"].append(nf); tr["cropin"].append(c); tr["video"].append(video[0])
        tr["out_fs"].append([int(ofs[0]), int(ofs[1])]); tr["out_video"].append(np.asarray(ov)[0])

    cr = {k: [] for k in ("fn", "fs", "nfeats", "draws", "video", "out_fs", "out_nfeats", "out_video")}
    crop_src, crop_vid = random.Random(31), np.random.RandomState(23)
    for name, fs, nf, forced in CROP:
        forced, draws = list(forced), []

        def randint(lo, hi):
            want = forced.pop(0) if forced else None
            v = want if want is not None else crop_src.randint(int(lo), int(hi))
            assert lo <= v <= hi, (name, fs, lo, hi, v)
            draws.append(int(v))
            return v

        video = crop_vid.randn(1, 16, D).astype(np.float32).astype(np.float64)
        random.randint = randint
        try:
            ofs, onf, ov = getattr(aug, {"gt_crop": "gt_moment_crop", "prot_gt_crop": "protected_gt_moment_crop",
                                         "gt_cropout": "gt_moment_cropout"}[name])(list(fs), nf, video.copy())
        finally:
            random.randint = real_randint
        assert not forced and len(draws) <= 4, (name, fs, draws)
        cr["fn"].append(CROP_FN[name]); cr["fs"].append(fs); cr["nfeats"].append(nf); cr["draws"].append(draws + [-1] * (4 - len(draws)))
        cr["video"].append(video[0]); cr["out_fs"].append([int(ofs[0]), int(ofs[1])]); cr["out_nfeats"].append(int(onf))
        cr["out_video"].append(np.asarray(ov)[0])

    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(
        OUT, mode=np.array(f["mode"], np.int32), T=np.array(f["T"], np.int32), n=np.array(f["n"], np.int32),
        duration=np.array(f["dur"]), timestamps=np.array(f["ts"]), spos=np.array(f["spos"], np.int32),
        spos_hi=np.array(f["spos_hi"], np.int32), framestps=np.array(f["fs"], np.int32), nfeats=np.array(f["nfeats"], np.int32),
        raw=np.concatenate(raws), raw_off=np.array(f["raw_off"], np.int64), out=np.concatenate(outs),
        out_off=np.array(f["out_off"], np.int64),
        f2s_pred=np.array(pred, np.float32), f2s_dur=np.array(durs), f2s_nfeats=np.array(nfs, np.int64), f2s_sec=sec.numpy(),
        tr_fs=np.array(tr["fs"], np.int32), tr_nfeats=np.array(tr["nfeats"], np.int32), tr_cropin=np.array(tr["cropin"], np.int32),
        tr_video=np.stack(tr["video"]), tr_out_fs=np.array(tr["out_fs"], np.int32), tr_out_video=np.stack(tr["out_video"]),
        crop_fn=np.array(cr["fn"], np.int32), crop_fs=np.array(cr["fs"], np.int32), crop_nfeats=np.array(cr["nfeats"], np.int32),
        crop_draws=np.array(cr["draws"], np.int32), crop_video=np.stack(cr["video"]), crop_out_fs=np.array(cr["out_fs"], np.int32),
        crop_out_nfeats=np.array(cr["out_nfeats"], np.int32), crop_out_video=np.stack(cr["out_video"]))
    print(f"{OUT}: {len(CASES)} sampling cases, {len(TRANSLATE)} translate cases, {os.path.getsize(OUT) / 1024:.1f} kB")


if __name__ == "__main__":
    main()

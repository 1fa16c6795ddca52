#!/usr/bin/env python3
"""Generate tests/golden/aug_modes.npz by running the REAL reference's DataAugmentForTSG (dataset/data_augment.py).

Runs only where the reference is checked out (``--ref``: its grounding/ directory), with the shims of
oracle/make_golden.py (``h5py`` stub; nothing else of them is needed here).  The reference is imported, never copied.
Every draw it makes is recorded through wrappers around ``np.random.rand`` (the apply gate) and ``random.randint`` (everything
else): kind, the (lo, hi) it asked for and the value returned.  A case may force some draws (a value inside the asked range,
checked) to reach an edge -- a crop that ends at row T-1, both cropout fallbacks, the gate at p = 0.5 -- the rest come from a
seeded generator.  Stored per case: inputs (mode, aug_percentage, [s, e], nfeats, video [1,T,D]), the draws, and the
reference's outputs ([s, e], nfeats, video).

Usage:  python tools/make_golden_augment.py --ref REFERENCE/grounding
"""
import argparse
import os
import random
import sys
import types

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "aug_modes.npz")
MODE_CODE = {"gt_translate": 0, "gt_crop": 1, "prot_gt_crop": 2, "gt_cropout": 3, "all": 4, None: 5}
T, D = 16, 4

# (mode, aug_percentage, [s, e], nfeats, forced gate value or None, forced randint values in call order (None = drawn))
CASES = [
    ("gt_crop", 1.0, [3, 9], 14, None, []),
    ("gt_crop", 1.0, [10, 15], 16, None, [3, 13]),        # widest crop, start e-w+1: deletes rows 13..15, the last one is T-1
    ("gt_crop", 1.0, [12, 15], 16, None, [2, 14]),        # ... and a 2-wide one at T-1
    ("gt_crop", 1.0, [0, 4], 10, None, [None, 0]),        # moment at row 0, crop at row 0
    ("gt_crop", 1.0, [5, 6], 12, None, []),               # 2-clip moment
    ("gt_crop", 1.0, [7, 9], 11, None, [None, 8]),        # 3-clip moment
    ("gt_crop", 1.0, [4, 4], 12, None, []),               # 1-clip moment: unchanged
    ("prot_gt_crop", 1.0, [6, 7], 16, None, []),          # 2 clips: protected width ceil(-0.5) = 0
    ("prot_gt_crop", 1.0, [6, 8], 12, None, [None, 8]),   # 3 clips: width 0, start at the top of its range
    ("prot_gt_crop", 1.0, [2, 12], 16, None, []),
    ("prot_gt_crop", 1.0, [5, 15], 16, None, [None, 12]), # nfeats = T, moment ends at T-1
    ("prot_gt_crop", 1.0, [0, 9], 13, None, []),          # moment at row 0
    ("gt_cropout", 1.0, [5, 12], 16, None, [1, None, 3]),  # candidates on both sides, pick from the right
    ("gt_cropout", 1.0, [5, 12], 16, None, [2, None, 0]),  # left side only (right block too narrow for w = 2)
    ("gt_cropout", 1.0, [0, 5], 12, None, []),            # moment at row 0: right side only
    ("gt_cropout", 1.0, [8, 15], 16, None, []),           # ends at T-1 (nfeats = T): left side only
    ("gt_cropout", 1.0, [4, 6], 12, None, []),            # width 0 -> gt_moment_crop with fresh draws
    ("gt_cropout", 1.0, [5, 6], 9, None, [None, None, 6]),  # 2 clips: width 0 -> crop, start at e
    ("gt_cropout", 1.0, [1, 12], 14, None, []),           # no outside block fits -> crop with the drawn (w, cropout start)
    ("gt_cropout", 1.0, [0, 15], 16, None, [3, 9]),       # whole sequence: no candidate -> crop ending at T-1's side
    ("gt_cropout", 1.0, [3, 3], 10, None, []),            # 1 clip: unchanged
    ("gt_translate", 1.0, [3, 6], 12, None, []),
    ("gt_translate", 1.0, [10, 15], 16, None, [0]),
    ("gt_translate", 1.0, [0, 11], 12, None, []),         # covers every clip: unchanged
    ("all", 1.0, [2, 10], 14, None, [0]),                 # -> prot_gt_crop
    ("all", 1.0, [2, 10], 14, None, [1]),                 # -> gt_cropout
    ("all", 1.0, [6, 15], 16, None, [1]),                 # -> gt_cropout at T-1
    ("all", 1.0, [4, 5], 10, None, [1]),                  # -> gt_cropout -> crop fallback
    (None, 1.0, [1, 9], 12, None, [0]),                   # -> gt_crop
    (None, 1.0, [1, 9], 12, None, [1]),                   # -> gt_cropout
    (None, 1.0, [9, 15], 16, None, [0, None, 12]),        # -> gt_crop ending at T-1
    (None, 1.0, [2, 4], 8, None, [1]),                    # -> gt_cropout -> crop fallback
    ("gt_crop", 0.0, [3, 9], 14, None, []),               # p = 0: skipped
    ("all", 0.0, [2, 10], 14, None, []),
    ("gt_crop", 0.5, [3, 9], 14, 0.3, []),                # gate: applied
    ("gt_crop", 0.5, [3, 9], 14, 0.7, []),                # gate: skipped
    ("gt_cropout", 0.5, [5, 12], 16, 0.5, []),            # u = p: applied (the test is u > p)
    (None, 0.5, [1, 9], 12, None, []),                    # gate drawn
    ("prot_gt_crop", 0.5, [2, 12], 16, None, []),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="the reference checkout's grounding/ directory")
    a = ap.parse_args()
    sys.modules.setdefault("h5py", types.ModuleType("h5py"))
    sys.path.insert(0, a.ref)
    from dataset.data_augment import DataAugmentForTSG

    real_randint, real_rand = random.randint, np.random.rand
    src = random.Random(20240611)
    gate_src = np.random.RandomState(7)
    vid_src = np.random.RandomState(11)
    rec = dict(kind=[], lo=[], hi=[], val=[], off=[0])
    fields = {k: [] for k in ("mode", "p", "fs", "nfeats", "video", "out_fs", "out_nfeats", "out_video")}
    for mode, p, fs, nf, gate, forced in CASES:
        forced = list(forced)

        def randint(lo, hi):
            want = forced.pop(0) if forced else None
            v = want if want is not None else src.randint(int(lo), int(hi))
            assert lo <= v <= hi, (mode, fs, lo, hi, v)
            rec["kind"].append(1); rec["lo"].append(float(lo)); rec["hi"].append(float(hi)); rec["val"].append(float(v))
            return v

        def rand(n):
            v = gate if gate is not None else float(gate_src.rand())
            rec["kind"].append(0); rec["lo"].append(0.0); rec["hi"].append(1.0); rec["val"].append(v)
            return np.array([v] * n)

        aug = DataAugmentForTSG(0, p, mode)
        video = np.zeros((1, T, D))
        video[0, :nf] = vid_src.randn(nf, D).astype(np.float32)      # float32 values: exact on the device
        random.randint, np.random.rand = randint, rand
        try:
            ofs, onf, ovid = aug.aug_data(list(fs), nf, video.copy())
        finally:
            random.randint, np.random.rand = real_randint, real_rand
        assert not forced, (mode, fs, "unused forced draws", forced)
        rec["off"].append(len(rec["kind"]))
        fields["mode"].append(MODE_CODE[mode]); fields["p"].append(p); fields["fs"].append(list(fs)); fields["nfeats"].append(nf)
        fields["video"].append(video[0]); fields["out_fs"].append([int(ofs[0]), int(ofs[1])]); fields["out_nfeats"].append(int(onf))
        fields["out_video"].append(np.asarray(ovid)[0])
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, mode=np.array(fields["mode"], np.int32), p=np.array(fields["p"]), fs=np.array(fields["fs"], np.int32),
                        nfeats=np.array(fields["nfeats"], np.int32), video=np.stack(fields["video"]),
                        out_fs=np.array(fields["out_fs"], np.int32), out_nfeats=np.array(fields["out_nfeats"], np.int32),
                        out_video=np.stack(fields["out_video"]), draw_kind=np.array(rec["kind"], np.int32),
                        draw_lo=np.array(rec["lo"]), draw_hi=np.array(rec["hi"]), draw_val=np.array(rec["val"]),
                        draw_off=np.array(rec["off"], np.int32))
    print(f"{OUT}: {len(CASES)} cases, {len(rec['kind'])} draws, {os.path.getsize(OUT) / 1024:.1f} kB")


if __name__ == "__main__":
    main()

"""Clip-feature sampling on the host (no GPU): the numpy mirrors of the reference's six samplers against the golden the real
reference produced (tests/golden/clip_sampling.npz, tools/make_golden_sampling.py), frame2sec, the shuffling augmentation on
LG spans that end past nfeats, the sampler / frame2sec selection table, the host mirror of LG's training draws, and argument
errors of the wrapper and of the C ABI."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from shufflingvideosfortsg_amd import data

NAMES = {v: k for k, v in data.SAMPLE_MODES.items()}


@pytest.fixture(scope="module")
def golden(request):
    from conftest import Golden
    return Golden("clip_sampling")


def cases(g):
    a = g.a
    for i in range(len(a["mode"])):
        T, D = int(a["T"][i]), a["raw"].shape[1]
        yield dict(mode=NAMES[int(a["mode"][i])], T=T, n=int(a["n"][i]), dur=float(a["duration"][i]),
                   ts=a["timestamps"][i].tolist(), spos=int(a["spos"][i]), spos_hi=int(a["spos_hi"][i]),
                   raw=a["raw"][a["raw_off"][i]:a["raw_off"][i + 1]], out=a["out"][a["out_off"][i]:a["out_off"][i + 1]].reshape(T, D),
                   fs=a["framestps"][i].tolist(), nfeats=int(a["nfeats"][i]))


def test_golden_covers_the_edges(golden):
    cs = list(cases(golden))
    by = {m: [c for c in cs if c["mode"] == m] for m in data.SAMPLE_MODES}
    assert {c["n"] % 2 for c in by["pair"]} == {0, 1} and {c["n"] % 3 for c in by["triple"]} == {0, 1, 2}
    for m in ("pair", "1to1", "lg"):
        assert any(c["nfeats"] < c["T"] for c in by[m]) and any(c["nfeats"] == c["T"] for c in by[m]), m
    assert any(c["nfeats"] > c["T"] for c in by["f2s_114"])                    # 114 does not clamp
    assert any(c["n"] / c["dur"] < 1 for c in by["f2s_114"]) and any(c["dur"] > c["T"] for c in by["f2s"])
    assert any(c["dur"] != int(c["dur"]) for c in by["f2s"])
    lg = by["lg"]
    assert any(c["spos_hi"] == 0 and c["n"] > c["T"] for c in lg)               # integral stride - 0.5: range [0, 0]
    assert any(c["spos"] == c["spos_hi"] > 0 for c in lg)                        # spos at the top of its range
    assert any(c["fs"][1] == c["T"] - 1 and c["n"] < c["T"] for c in lg)        # the T-1 default on a short video
    assert any(min(c["ts"]) < 0 for c in cs) and any(max(c["ts"]) > c["dur"] for c in cs)


def test_numpy_mirrors_equal_reference_golden(golden):
    for c in cases(golden):
        out, fs, nf = data.sample_clips_numpy(c["raw"], c["ts"], c["dur"], c["T"], c["mode"], c["spos"])
        assert np.array_equal(out.astype(np.float32), c["out"]) and np.array_equal(out.astype(np.float32).astype(np.float64), out), c["mode"]
        assert [int(x) for x in fs] == c["fs"] and nf == c["nfeats"], (c["mode"], c["n"], fs, nf)
        if c["mode"] == "lg" and c["spos_hi"] >= 0:
            assert data.lg_spos_range(c["n"], c["T"]) == (0, c["spos_hi"])


def test_lg_arange_and_contraction_cases_matter(golden):
    """The golden pins the arange arithmetic: start + i*step (or a fused start + i*delta) would round a position the other way."""
    from fractions import Fraction
    hits_naive = hits_fused = 0
    for c in cases(golden):
        if c["mode"] != "lg" or c["n"] <= c["T"]:
            continue
        s = data.lg_positions(c["n"], c["T"], c["spos"])
        stride = c["n"] / c["T"]
        a0 = float(c["spos"]); d = (a0 + stride) - a0
        naive = np.round(np.array([a0 + i * stride for i in range(len(s))]))
        fused = np.round(np.array([float(Fraction(a0) + i * Fraction(d)) for i in range(len(s))]))
        hits_naive += int((naive != s).any()); hits_fused += int((fused != s).any())
    assert hits_naive >= 1 and hits_fused >= 1


def test_frame2sec_equals_reference(golden):
    a = golden.a
    got = data.frame2sec(torch.from_numpy(a["f2s_pred"]), a["f2s_dur"].tolist(), a["f2s_nfeats"].tolist(), "lg")
    assert got.dtype == torch.float64 and torch.equal(got, torch.from_numpy(a["f2s_sec"]))
    p = torch.from_numpy(a["f2s_pred"])
    assert data.frame2sec(p, a["f2s_dur"], a["f2s_nfeats"], "identity") is p
    with pytest.raises(NotImplementedError):
        data.frame2sec(p, a["f2s_dur"], a["f2s_nfeats"], "unsupported")
    with pytest.raises(ValueError):
        data.frame2sec(p, a["f2s_dur"], a["f2s_nfeats"], "seconds")


def test_translate_past_nfeats_equals_reference(golden):
    a = golden.a
    for i in range(len(a["tr_nfeats"])):
        fs, nf, c = a["tr_fs"][i].tolist(), int(a["tr_nfeats"][i]), int(a["tr_cropin"][i])
        nfs, onf, out = data.gt_moment_translate(fs, nf, a["tr_video"][i][None], c)
        assert nfs == a["tr_out_fs"][i].tolist() and onf == nf
        assert np.array_equal(out[0], a["tr_out_video"][i]), (fs, nf, c)
    assert (a["tr_fs"][:, 1] >= a["tr_nfeats"]).sum() >= 4


def test_vfeat_mode_table():
    V = data.VfeatMode
    assert data.vfeat_mode("charades", "i3d", "raw") == V("pair", "identity")
    assert data.vfeat_mode("Charades", "i3d", "lg") == V("lg", "lg")
    assert data.vfeat_mode("charades", "i3d", "LG") == V("lg", "identity")             # sampler lower()s, frame2sec does not
    assert data.vfeat_mode("charades", "lgi3d", "raw") == V("triple", "identity")
    assert data.vfeat_mode("charades", "lgi3d", "lg") == V("lg", "lg")                 # lg is checked first
    assert data.vfeat_mode("anet", "i3d", "raw") == V("1to1", "identity")
    assert data.vfeat_mode("anet", "i3d", "lg") == V("1to1", "lg")                     # samples 1:1, converts as lg
    assert data.vfeat_mode("anet", "i3d", "other") == V("1to1", "unsupported")
    assert data.vfeat_mode("anet", "c3d", "raw") == V("f2s", "identity")
    assert data.vfeat_mode("anet", "c3d", "114") == V("f2s_114", "identity")
    assert data.vfeat_mode("anet", "c3d", "lg") == V("lg", "lg")
    assert data.vfeat_mode("activitynet", "c3d", "other") == V("f2s_114", "identity")
    with pytest.raises(ValueError):
        data.vfeat_mode("tacos", "c3d", "raw")


def test_host_spos_draws_cover_the_inclusive_range():
    T = 240
    for n in (100, 240, 241, 360, 600, 1000, 2400, 3000):
        lo, hi = data.lg_spos_range(n, T)
        d = np.stack([data.lg_spos_draws(seed, [n] * 4, T) for seed in range(300)])
        assert d.min() >= lo and d.max() <= hi, n
        assert d.min() == lo and d.max() == hi, (n, hi)
    assert data.lg_spos_range(360, 240) == (0, 0)          # stride 1.5: random_end 1.0 is integral -> 0
    assert data.lg_spos_range(600, 240) == (0, 1)          # stride 2.5: random_end 2.0 -> 1
    assert data.lg_spos_range(1000, 240) == (0, 3)         # stride 4.1667: floor(3.6667)
    assert not np.array_equal(data.lg_spos_draws(1, [3000] * 16, T), data.lg_spos_draws(2, [3000] * 16, T))


def test_wrapper_argument_errors():
    raw = torch.zeros(10, 8)
    with pytest.raises(ValueError, match="unknown sampling mode"):
        data.sample_clips_device(raw, [0, 10], 8, "c3d")
    with pytest.raises(ValueError, match="needs durations"):
        data.sample_clips_device(raw, [0, 10], 8, "f2s_114", timestamps=[[0, 1]])
    with pytest.raises(ValueError, match="needs timestamps"):
        data.sample_clips_device(raw, [0, 10], 8, "lg", durations=[5.0])
    with pytest.raises(TypeError):
        data.sample_clips_device(raw, [0, 10], 8, "pair", out_dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.sample_clips_device(raw, [0, 10], 8, "pair")


def test_c_abi_argument_errors_without_gpu():
    from shufflingvideosfortsg_amd import _lib, build
    build.build()
    lib = _lib.load()
    fn = lib.tsg_sample_clips
    P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(9)]      # 16-byte aligned stand-ins: every call returns before a launch
    names = ("raw", "offsets", "ts", "dur", "spos", "out", "nf", "fs", "spos_out")

    def call(**kw):
        a = dict(zip(names, P), mode=5, train=1, seed=0, B=4, T=16, D=8, dtype=_lib.TSG_F32)
        a.update(kw)
        return fn(a["raw"], a["offsets"], a["ts"], a["dur"], a["mode"], a["train"], a["seed"], a["spos"], a["out"], a["nf"],
                  a["fs"], a["spos_out"], a["B"], a["T"], a["D"], a["dtype"], None)
    E_NULL, E_SHAPE, E_ALIGN, E_DTYPE = -1, -2, -3, -4
    for k in ("raw", "offsets", "out", "nf"):
        assert call(**{k: None}) == E_NULL, k
    for dims in itertools.product((0, -1, 4), repeat=3):
        if min(dims) <= 0:
            assert call(B=dims[0], T=dims[1], D=dims[2] * 2) == E_SHAPE, dims
    for mode in (-1, 6, 100):
        assert call(mode=mode) == E_SHAPE, mode
    assert call(T=16385) == E_SHAPE
    assert call(D=6) == E_ALIGN and call(D=500, dtype=7) == E_DTYPE and call(dtype=_lib.TSG_F32S) == E_DTYPE
    for mode in (3, 4, 5):
        assert call(mode=mode, dur=None) == E_NULL, mode
    assert call(mode=5, ts=None, fs=None) == E_NULL                       # LG's labels need the timestamps
    assert call(ts=None) == E_NULL and call(fs=None) == E_NULL            # timestamps and framestps go together
    for k in ("raw", "out", "ts", "dur", "spos", "fs", "spos_out"):
        assert call(**{k: ctypes.c_void_p(0x10004)}) == E_ALIGN, k
    assert b"tsg_sample_clips" in lib.tsg_last_error()


class _Replay:
    """random.randint replaying recorded draws."""
    def __init__(self, draws):
        self.it = iter(int(x) for x in draws if x >= 0)

    def randint(self, lo, hi):
        v = next(self.it)
        assert lo <= v <= hi, (lo, hi, v)
        return v


def crop_plan(fn, fs, nf, d):
    """The (op, a, b, c) plan of a crop-family call from its recorded draws (moment_augment_device's plan format)."""
    if fn in (1, 2):
        return (2, d[0], d[1], 0)
    if d[0] <= 0:
        return (2, d[1], d[2], 0)
    cand = data.cropout_candidates(fs, nf, d[0])
    if not cand:
        return (2, d[0], d[1], 0)
    return (3, d[0], d[1], cand[d[2] if len(cand) > 1 else 0])


def test_crop_family_past_nfeats_equals_reference(golden):
    """gt_crop / prot_gt_crop / gt_cropout on LG spans that end at or past nfeats: the port agrees with the reference."""
    a = golden.a
    fns = {1: data.gt_moment_crop, 2: data.protected_gt_moment_crop, 3: data.gt_moment_cropout}
    assert (a["crop_fs"][:, 1] >= a["crop_nfeats"]).all() and set(a["crop_fn"].tolist()) == {1, 2, 3}
    for i in range(len(a["crop_fn"])):
        fn, fs, nf, d = int(a["crop_fn"][i]), a["crop_fs"][i].tolist(), int(a["crop_nfeats"][i]), a["crop_draws"][i].tolist()
        v = a["crop_video"][i][None]
        for got in (fns[fn](fs, nf, v, rng=_Replay(d)), data.apply_plan(fs, nf, v, crop_plan(fn, fs, nf, d))):
            assert list(got[0]) == a["crop_out_fs"][i].tolist() and got[1] == int(a["crop_out_nfeats"][i]), (i, got[:2])
            assert np.array_equal(got[2][0], a["crop_out_video"][i]), i

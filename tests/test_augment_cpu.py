"""The crop family of the augmentation (gt_crop, prot_gt_crop, gt_cropout, 'all', None) without a GPU: the numpy functions and
the host mirror of the device's plan draws against the real reference's recorded draws and outputs (tests/golden/aug_modes.npz,
tools/make_golden_augment.py), the legality and coverage of the hash draws, mode names, and the C ABI's argument errors."""
import ctypes
import itertools

import numpy as np
import pytest

from shufflingvideosfortsg_amd import data

MODES = ["gt_translate", "gt_crop", "prot_gt_crop", "gt_cropout", "all", None]
NAME = {data.AUG_MODES[m]: m for m in MODES}


def cases(golden):
    g = golden("aug_modes").a
    for i in range(len(g["mode"])):
        o0, o1 = g["draw_off"][i], g["draw_off"][i + 1]
        draws = [(int(k), lo, hi, v) for k, lo, hi, v in zip(g["draw_kind"][o0:o1], g["draw_lo"][o0:o1], g["draw_hi"][o0:o1],
                                                             g["draw_val"][o0:o1])]
        yield dict(mode=NAME[int(g["mode"][i])], p=float(g["p"][i]), fs=g["fs"][i].tolist(), nf=int(g["nfeats"][i]),
                   video=g["video"][i][None], out_fs=g["out_fs"][i].tolist(), out_nf=int(g["out_nfeats"][i]),
                   out_video=g["out_video"][i][None], draws=draws)


class Replay:
    """Hands out the reference's recorded draws in order and checks each request's inclusive (lo, hi) against the recorded one:
    ``randint(lo, hi)`` the numpy functions' interface, ``randint(slot, lo, hi)`` / ``unit(slot)`` the plan drawer's."""

    def __init__(self, draws):
        self.rand = [v for k, _, _, v in draws if k == 0]
        self.ints = [(lo, hi, v) for k, lo, hi, v in draws if k == 1]

    def randint(self, *a):
        lo, hi = a[-2:]
        assert self.ints, f"a draw randint({lo}, {hi}) the reference did not make"
        rlo, rhi, v = self.ints.pop(0)
        assert (lo, hi) == (rlo, rhi), f"randint({lo}, {hi}) where the reference drew randint({rlo}, {rhi})"
        return int(v)

    def unit(self, slot):
        return self.rand.pop(0)


FNS = {"gt_translate": [data.gt_moment_translate], "gt_crop": [data.gt_moment_crop], "prot_gt_crop": [data.protected_gt_moment_crop],
       "gt_cropout": [data.gt_moment_cropout], "all": [data.protected_gt_moment_crop, data.gt_moment_cropout],
       None: [data.gt_moment_crop, data.gt_moment_cropout]}


def aug_np(mode, fs, nf, video, rng, gate=None, p=1.0):
    """aug_data (data_augment.py:28-36) over the numpy functions."""
    if gate is not None and gate > p:
        return list(fs), nf, video
    fns = FNS[mode]
    fn = fns[rng.randint(0, len(fns) - 1)] if len(fns) > 1 else fns[0]
    return fn(fs, nf, video, rng=rng)


def test_golden_covers_the_edges(golden):
    cs = list(cases(golden))
    assert {c["mode"] for c in cs} == set(MODES)
    assert {c["p"] for c in cs} == {0.0, 0.5, 1.0}
    assert any(c["nf"] < 16 for c in cs) and any(c["nf"] == 16 for c in cs)
    assert any(c["fs"][1] == 15 and c["out_nf"] < c["nf"] for c in cs)                  # a crop ending at row T-1
    assert any(c["fs"][1] - c["fs"][0] == 1 for c in cs) and any(c["fs"][1] - c["fs"][0] == 2 for c in cs)
    assert any(c["fs"][0] == 0 for c in cs)
    # both cropout fallbacks, each ending as a crop (nfeats shrinks): width <= 0 -> fresh crop draws (first range is [0, 0] or
    # below); no outside block fits -> crop with the two draws already made (width, cropout start), no cropin draw
    crops = [[d for d in c["draws"] if d[0] == 1] for c in cs if c["mode"] == "gt_cropout" and c["out_nf"] < c["nf"]]
    assert any(d[0][2] <= 0 and len(d) == 3 for d in crops)
    assert any(d[0][2] > 0 and len(d) == 2 for d in crops)


def test_numpy_functions_equal_reference_golden(golden):
    for c in cases(golden):
        r = Replay(c["draws"])
        gate = r.rand[0] if r.rand else None
        fs, nf, v = aug_np(c["mode"], c["fs"], c["nf"], c["video"].copy(), r, gate, c["p"])
        assert not r.ints, (c["mode"], c["fs"], "reference drew more")
        assert [int(x) for x in fs] == c["out_fs"] and int(nf) == c["out_nf"], c
        np.testing.assert_array_equal(v, c["out_video"])


def test_host_plan_drawer_follows_reference_draws(golden):
    """The device's draw logic (mirrored on the host) asks for the reference's ranges in the reference's order; the plan it
    resolves, applied, gives the reference's output."""
    for c in cases(golden):
        r = Replay(c["draws"])
        plan = data._draw_plan(r, data.aug_mode_code(c["mode"]), c["p"], c["fs"][0], c["fs"][1], c["nf"])
        assert not r.ints, (c["mode"], c["fs"], "reference drew more")
        fs, nf, v = data.apply_plan(c["fs"], c["nf"], c["video"].copy(), plan)
        assert [int(x) for x in fs] == c["out_fs"] and int(nf) == c["out_nf"], (c, plan)
        np.testing.assert_array_equal(v, c["out_video"])


def reachable(mode, fs, nf, T):
    """Every outcome the reference can produce at p = 1: depth-first over every value of every randint it asks for.  An outcome
    is (span, nfeats, row map) with rows encoded as t+1 (0 = zero row)."""
    video = np.zeros((1, T, 1)); video[0, :nf, 0] = np.arange(1, nf + 1)
    seen, stack = set(), [[]]
    while stack:
        prefix = stack.pop()
        calls = []

        class R:
            def randint(self, lo, hi):
                i = len(calls)
                v = prefix[i] if i < len(prefix) else lo
                calls.append((lo, hi, v))
                return v
        s, n, v = aug_np(mode, list(fs), nf, video, R())
        seen.add((tuple(int(x) for x in s), int(n), tuple(v[0, :, 0].astype(int))))
        for i in range(len(prefix), len(calls)):
            lo, hi, _ = calls[i]
            stack += [[x[2] for x in calls[:i]] + [w] for w in range(lo + 1, hi + 1)]
    return seen


SMALL = [([2, 6], 9), ([0, 3], 10), ([5, 9], 10), ([3, 4], 8), ([1, 3], 7), ([4, 4], 6), ([0, 9], 10), ([2, 8], 10), ([6, 7], 10)]


@pytest.mark.parametrize("mode", MODES)
def test_hash_plans_are_legal_and_cover_every_legal_outcome(mode):
    T = 10
    spans, nfs = [c[0] for c in SMALL], [c[1] for c in SMALL]
    video = np.zeros((len(SMALL), T))
    for b, nf in enumerate(nfs):
        video[b, :nf] = np.arange(1, nf + 1)
    legal = [reachable(mode, fs, nf, T) for fs, nf in SMALL]
    hit = [set() for _ in SMALL]
    for seed in range(1500):
        for b, plan in enumerate(data.augment_plans(seed, spans, nfs, mode, 1.0)):
            s, n, v = data.apply_plan(spans[b], nfs[b], video[b][None, :, None], plan)
            out = (tuple(int(x) for x in s), int(n), tuple(v[0, :, 0].astype(int)))
            assert out in legal[b], (mode, SMALL[b], seed, plan.tolist())
            hit[b].add(out)
    for b in range(len(SMALL)):
        assert hit[b] == legal[b], (mode, SMALL[b], sorted(legal[b] - hit[b])[:3])


def test_hash_gate():
    spans, nfs = [[3, 9]] * 4000, [14] * 4000
    assert (data.augment_plans(5, spans, nfs, "gt_crop", 0.0)[:, 0] == 0).all()
    assert (data.augment_plans(5, spans, nfs, "gt_crop", 1.0)[:, 0] == 2).all()
    frac = (data.augment_plans(5, spans, nfs, "gt_crop", 0.3)[:, 0] != 0).mean()
    assert abs(frac - 0.3) < 5 * (0.3 * 0.7 / 4000) ** 0.5
    a, b = data.augment_plans(1, spans[:64], nfs[:64], None, 1.0), data.augment_plans(2, spans[:64], nfs[:64], None, 1.0)
    assert not np.array_equal(a, b) and np.array_equal(a, data.augment_plans(1, spans[:64], nfs[:64], None, 1.0))


def test_mode_names():
    assert [data.aug_mode_code(m) for m in MODES] == [0, 1, 2, 3, 4, 5]
    with pytest.raises(NotImplementedError, match="seg_len"):
        data.aug_mode_code("shuffle_temporal")
    with pytest.raises(ValueError, match="unknown aug_mode"):
        data.aug_mode_code("gt_shuffle")
    import torch
    v = torch.zeros(2, 8, 4)
    with pytest.raises(NotImplementedError):
        data.moment_augment_device(v, [[1, 3]] * 2, [8, 8], "shuffle_temporal")
    with pytest.raises(ValueError):
        data.moment_augment_device(v, [[1, 3]] * 2, [8, 8], "crop")
    with pytest.raises(ValueError, match="ops in 0..3"):
        data.moment_augment_device(v, [[1, 3]] * 2, [8, 8], None, plan=[[0, 0, 0, 0], [4, 0, 0, 0]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.moment_augment_device(v, [[1, 3]] * 2, [8, 8], None)


def test_c_abi_argument_errors_without_gpu():
    from shufflingvideosfortsg_amd import _lib, build
    build.build()
    lib = _lib.load()
    fn = lib.tsg_moment_augment
    P = [ctypes.c_void_p(0x10000 * (i + 1)) for i in range(8)]      # 16-byte aligned stand-ins: every call returns before a launch
    video, spans, nfeats, out, new_spans, new_nf, plan, plan_out = P

    def call(**kw):
        a = dict(video=video, spans=spans, nfeats=nfeats, mode=1, p=1.0, seed=0, plan=None, plan_out=plan_out, out=out,
                 new_spans=new_spans, new_nf=new_nf, B=4, T=16, D=8, dtype=_lib.TSG_F32)
        a.update(kw)
        return fn(a["video"], a["spans"], a["nfeats"], a["mode"], a["p"], a["seed"], a["plan"], a["plan_out"], a["out"],
                  a["new_spans"], a["new_nf"], a["B"], a["T"], a["D"], a["dtype"], None)
    E_NULL, E_SHAPE, E_ALIGN, E_DTYPE = -1, -2, -3, -4
    for k in ("video", "spans", "nfeats", "out", "new_spans", "new_nf"):
        assert call(**{k: None}) == E_NULL, k
    for dims in itertools.product((0, -1, 4), repeat=3):
        if min(dims) <= 0:
            assert call(B=dims[0], T=dims[1], D=dims[2] * 2) == E_SHAPE, dims
    assert call(D=6) == E_ALIGN
    assert call(D=12, dtype=_lib.TSG_BF16) == E_ALIGN
    assert call(dtype=_lib.TSG_F32S) == E_DTYPE and call(dtype=7) == E_DTYPE
    assert call(out=video) == E_SHAPE
    for mode in (-1, 6, 100):
        assert call(mode=mode) == E_SHAPE, mode
        assert call(mode=mode, plan=plan) == E_SHAPE, mode
    assert call(plan=ctypes.c_void_p(0x10004)) == E_ALIGN
    assert call(plan_out=ctypes.c_void_p(0x10008)) == E_ALIGN
    assert call(video=ctypes.c_void_p(0x10002)) == E_ALIGN
    assert b"tsg_moment_augment" in lib.tsg_last_error()

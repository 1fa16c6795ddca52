"""Input-side helpers of the grounding path: label masks, the shuffling augmentation and the
synthetic batches used by the benchmarks.

Two implementations of the same functions:
  * host / numpy, like the reference's dataset code (grounding/dataset/charades.py, data_augment.py): ``Sequence_mask``,
    ``gt_moment_translate``, ``synthetic_batch`` -- used for CPU tensors, by the CPU-side tests and to seed the benchmarks;
  * device (``*_device``, csrc/input_pipeline.hip through the C ABI): pair-mean pooling, the four masks and the shuffling
    augmentation for a whole batch on the GPU that consumes it, so that N ranks on one host do not queue behind numpy
    workers (the reference feeds ONE GPU from 8 DataLoader workers).  ``pair_batch_device`` assembles the GMD batch dict
    (train.py:50-91 keys) from resident features.

The clip samplers of the reference's Charades and ActivityNet datasets (raw clip features -> the [T, D] rows the model reads)
have numpy mirrors (``generate_video_fts_data`` ... ``lg_get_fixed_length_feat``, chosen by ``vfeat_mode``) and one device
kernel (``sample_clips_device``, csrc/input_pipeline.hip); ``clip_batch_device`` composes it with the masks / GMD pair."""
from __future__ import annotations

import collections
import math

import numpy as np
import torch


def Sequence_mask(max_len, temporal_boundary):
    """int32 mask with ones on [st, et] INCLUSIVE, clipped to the sequence (charades.py:12-18)."""
    st, et = temporal_boundary
    mask = np.zeros([max_len], dtype=np.int32)
    mask[max(0, st):min(et, max_len - 1) + 1] = 1
    return mask


def gt_moment_translate(framestps, nfeats, video_feat, cropin_start=None, rng=None):
    """The shuffling augmentation (data_augment.py:135-156): cut the ground-truth moment [s, e] out of
    the first ``nfeats`` clips, close the gap and re-insert it in front of position ``cropin_start``
    (uniform in [0, nfeats-len] when not given; ``rng`` = ``random.Random`` / ``np.random.RandomState``)
    of the gap-closed sequence.  ``video_feat`` is [1, T, D]; returns (new [s,e], nfeats, new feats).
    No-op for moments of length <= 1 or covering every clip."""
    s, e = framestps
    n = e - s + 1
    if n <= 1 or n >= nfeats:
        return list(framestps), nfeats, video_feat
    if cropin_start is None:
        if rng is None:
            import random as rng       # the reference draws from the unseeded global ``random``
        cropin_start = rng.randint(0, nfeats - n)
    order = np.concatenate([np.arange(0, s), np.arange(e + 1, nfeats)])           # gap closed
    order = np.concatenate([order[:cropin_start], np.arange(s, e + 1), order[cropin_start:]])
    out = np.zeros(video_feat.shape) + 0.0
    # nfeats rows -- or, for a moment ending at or past nfeats (LG's end label T-1), e+1 of them: the gap-closed sequence is
    # then rows [0, s) only, and the reference's np.insert keeps every row it produced up to T (data_augment.py:141-153)
    out[0, :len(order)] = video_feat[0, order]
    return [cropin_start, cropin_start + n - 1], nfeats, out


def _randint(rng):
    if rng is None:
        import random as rng           # the reference draws from the unseeded global ``random``
    return rng.randint


def _crop_rows(video_feat, crop_start, crop_width):
    """np.delete of rows [crop_start, crop_start + crop_width) along axis 1, then zero-filled back to T rows
    (data_augment.py:56-58).  Rows at or beyond T are not there to delete."""
    T = video_feat.shape[1]
    keep = [t for t in range(T) if not crop_start <= t < crop_start + crop_width]
    out = np.zeros(video_feat.shape) + 0.0
    out[0, :len(keep)] = video_feat[0, keep]
    return out


def gt_moment_crop(framestps, nfeats, video_feat, crop_width=None, crop_start=None, rng=None,
                   min_crop_width_ratio=0.2, max_crop_width_ratio=0.5):
    """``gt_crop`` (data_augment.py:38-63): delete ``crop_width`` clips starting at ``crop_start`` from inside the moment
    [s, e]; the rest shifts left over a zero tail.  Width drawn in [ceil(.2 len), ceil(.5 len)] when not given or >= len,
    start in [s, e - w + 1] when not given or outside [s, e] (``rng.randint``, inclusive).  Returns ([s, e - w], nfeats - w,
    new feats); moments of length <= 1 are returned unchanged."""
    s, e = framestps
    n = e - s + 1
    if n <= 1:
        return list(framestps), nfeats, video_feat
    randint = _randint(rng)
    if crop_width is None or crop_width >= n:
        crop_width = randint(int(np.ceil(n * min_crop_width_ratio)), int(np.ceil(n * max_crop_width_ratio)))
    if crop_start is None or crop_start < s or crop_start > e:
        crop_start = randint(s, e - crop_width + 1)
    return [s, e - crop_width], nfeats - crop_width, _crop_rows(video_feat, crop_start, crop_width)


def protected_gt_moment_crop(framestps, nfeats, video_feat, crop_width=None, crop_start=None, rng=None,
                             min_crop_width_ratio=0.2, max_crop_width_ratio=0.5, protected_ratio=0.2):
    """``prot_gt_crop`` (data_augment.py:65-93): ``gt_moment_crop`` inside the protected part [ps, pe] = [s + ceil(.2 len),
    e - ceil(.2 len)] of the moment: width in [ceil(.2 (pe - ps)), ceil(.5 (pe - ps))], start in [ps, pe - w + 1].  pe - ps
    is -1 or 0 for moments of 2-3 clips: width 0, a crop that deletes nothing."""
    s, e = framestps
    n = e - s + 1
    if n <= 1:
        return list(framestps), nfeats, video_feat
    randint = _randint(rng)
    ps, pe = s + int(np.ceil(n * protected_ratio)), e - int(np.ceil(n * protected_ratio))
    if crop_width is None or crop_width > n:
        crop_width = randint(int(np.ceil((pe - ps) * min_crop_width_ratio)), int(np.ceil((pe - ps) * max_crop_width_ratio)))
    if crop_start is None or crop_start < s or crop_start > e:
        crop_start = randint(ps, pe - crop_width + 1)
    return [s, e - crop_width], nfeats - crop_width, _crop_rows(video_feat, crop_start, crop_width)


def cropout_candidates(framestps, nfeats, crop_width, protected_ratio=0.2):
    """The cropin starts ``gt_moment_cropout`` chooses from (data_augment.py:118-122): [0, psl - 1] if psl >= w and
    [per, nfeats - w - 1] if nfeats - 1 - per >= w, where psl / per = s - ceil(.2 len) / e + ceil(.2 len)."""
    s, e = framestps
    c = int(np.ceil((e - s + 1) * protected_ratio))
    psl, per = s - c, e + c
    cand = list(range(psl)) if psl >= crop_width else []
    if nfeats - 1 - per >= crop_width:
        cand += list(range(per, nfeats - crop_width))
    return cand


def gt_moment_cropout(framestps, nfeats, video_feat, crop_width=None, cropout_start=None, cropin_start=None, rng=None,
                      min_crop_width_ratio=0.2, max_crop_width_ratio=0.5, protected_ratio=0.2):
    """``gt_cropout`` (data_augment.py:95-133): overwrite ``crop_width`` clips of the moment's protected part, starting at
    ``cropout_start``, with the clips starting at ``cropin_start`` outside the moment (read from the original video); span and
    nfeats stay.  Draws (``rng.randint``, inclusive) for what is not given: width in [ceil(.2 d), ceil(.5 d)] with
    d = (e - ceil(.2 len)) - (s + ceil(.2 len)), cropout start in [s + ceil(.2 len), e - ceil(.2 len) - w + 1], cropin start
    uniformly from ``cropout_candidates``.  Fallbacks as in the reference: w <= 0 -> ``gt_moment_crop`` with fresh draws; no
    candidate -> ``gt_moment_crop(w, cropout_start)``."""
    s, e = framestps
    n = e - s + 1
    if n <= 1:
        return list(framestps), nfeats, video_feat
    randint = _randint(rng)
    c = int(np.ceil(n * protected_ratio))
    psr, pel = s + c, e - c
    if crop_width is None:
        crop_width = randint(int(np.ceil((pel - psr) * min_crop_width_ratio)), int(np.ceil((pel - psr) * max_crop_width_ratio)))
    if crop_width <= 0:
        return gt_moment_crop(framestps, nfeats, video_feat, rng=rng, min_crop_width_ratio=min_crop_width_ratio,
                              max_crop_width_ratio=max_crop_width_ratio)
    if cropout_start is None:
        cropout_start = randint(psr, pel - crop_width + 1)
    cand = cropout_candidates(framestps, nfeats, crop_width, protected_ratio)
    if not cand:
        return gt_moment_crop(framestps, nfeats, video_feat, crop_width, cropout_start, rng=rng,
                              min_crop_width_ratio=min_crop_width_ratio, max_crop_width_ratio=max_crop_width_ratio)
    if cropin_start is None:
        cropin_start = cand[randint(0, len(cand) - 1) if len(cand) > 1 else 0]
    out = video_feat.copy()
    out[0, cropout_start:cropout_start + crop_width] = video_feat[0, cropin_start:cropin_start + crop_width]
    return list(framestps), nfeats, out


def apply_plan(framestps, nfeats, video_feat, plan):
    """One sample's resolved plan (op, a, b, c) -- see ``moment_augment_device`` -- applied with the numpy functions above."""
    op, a, b, c = (int(x) for x in plan)
    if op == 1:
        return gt_moment_translate(framestps, nfeats, video_feat, a)
    if op == 2:
        s, e = framestps
        return [s, e - a], nfeats - a, _crop_rows(video_feat, b, a)
    if op == 3:
        out = video_feat.copy()
        out[0, b:b + a] = video_feat[0, c:c + a]
        return list(framestps), nfeats, out
    return list(framestps), nfeats, video_feat


def synthetic_batch(B, T, N, video_dim=1024, word_dim=300, seed=1234, pair=False, device="cpu"):
    """Seeded synthetic (video, query, masks, labels) batch with the shapes and label conventions of
    the reference's collate functions; ``pair=True`` adds the shuffled pseudo video of the GMD step."""
    g = torch.Generator().manual_seed(seed)
    rs = np.random.RandomState(seed)
    video = torch.randn(B, T, video_dim, generator=g)
    query = torch.randn(B, N, word_dim, generator=g) * 0.4
    nfeats = rs.randint(max(2, T // 2), T + 1, size=B)
    fs = []
    for n in nfeats:
        s = rs.randint(0, n - 1); e = rs.randint(s + 1, n)
        fs.append([int(s), int(e)])

    def labels(fsl):
        return {"framestps": [list(f) for f in fsl],
                "temporal_labels": torch.from_numpy(np.stack([Sequence_mask(T, f) for f in fsl])),
                "fore_masks": torch.from_numpy(np.stack([Sequence_mask(T, [0, f[0]]) for f in fsl])),
                "back_masks": torch.from_numpy(np.stack([Sequence_mask(T, [f[1], int(n)]) for f, n in zip(fsl, nfeats)]))}
    out = {"video": video, "query": query, "nfeats": nfeats,
           "video_mask": torch.from_numpy(np.stack([Sequence_mask(T, [0, int(n)]) for n in nfeats])),
           "query_mask": torch.ones(B, N, dtype=torch.int32), "gt": labels(fs)}
    out["gt"]["timestps"] = torch.tensor(fs, dtype=torch.float32)
    if pair:
        pv, pfs = [], []
        for b in range(B):
            nf, _, nv = gt_moment_translate(fs[b], int(nfeats[b]), video[b:b + 1].double().numpy(), rng=rs)
            pv.append(torch.from_numpy(np.ascontiguousarray(nv[0])).float()); pfs.append([int(nf[0]), int(nf[1])])
        out["pseudo_video"] = torch.stack(pv)
        out["pseudo_gt"] = labels(pfs)
    return out if device == "cpu" else to_device(out, device)


def to_device(batch, device):
    """Move a (possibly sharded) host batch dict to ``device``; the collate's lists of [start, end] pairs become ONE resident
    index tensor per label group: the losses gather with it three times per step, and a list would be a blocking host-to-device
    copy each time."""
    out = dict(batch)
    for k, v in list(out.items()):
        if isinstance(v, torch.Tensor):
            out[k] = v.to(device)
    for gt in ("gt", "pseudo_gt"):
        if gt in out:
            out[gt] = dict(out[gt])
            for k, v in list(out[gt].items()):
                if isinstance(v, torch.Tensor):
                    out[gt][k] = v.to(device)
            fs = out[gt]["framestps"]
            out[gt]["framestps"] = (fs if isinstance(fs, torch.Tensor) else torch.tensor(fs, dtype=torch.long)).to(device)
    # The GMD step runs the original and the shuffled stream as ONE batch of 2B (model/SpanGroundMatchDisc.py): their tensors are
    # placed back to back in one device allocation, so the model's batch concatenation is a view (`adjacent_cat`), not a 64 MB copy
    # and four small ones per step.
    if "pseudo_video" in out and isinstance(out.get("video"), torch.Tensor):
        out["video"], out["pseudo_video"] = _adjacent(out["video"], out["pseudo_video"])
    if "gt" in out and "pseudo_gt" in out:
        for k in ("temporal_labels", "fore_masks", "back_masks"):
            a, b = out["gt"].get(k), out["pseudo_gt"].get(k)
            if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor):
                out["gt"][k], out["pseudo_gt"][k] = _adjacent(a, b)
    return out


def _adjacent(a, b):
    """Two equally shaped tensors as the two halves of one allocation (views)."""
    if a.shape != b.shape or a.dtype != b.dtype or a.device != b.device:
        return a, b
    both = torch.empty((2 * a.shape[0],) + tuple(a.shape[1:]), dtype=a.dtype, device=a.device)
    both[:a.shape[0]].copy_(a); both[a.shape[0]:].copy_(b)
    return both[:a.shape[0]], both[a.shape[0]:]


def adjacent_cat(a, b):
    """``torch.cat([a, b], 0)``; a VIEW when b starts where a ends in the same storage (see ``to_device``) and neither needs a gradient."""
    if (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype and a.device == b.device
            and a.dim() >= 1 and a.is_contiguous() and b.is_contiguous() and not a.requires_grad and not b.requires_grad
            and a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() and b.storage_offset() == a.storage_offset() + a.numel()
            and a.untyped_storage().nbytes() >= (b.storage_offset() + b.numel()) * a.element_size()):
        return torch.as_strided(a, (2 * a.shape[0],) + tuple(a.shape[1:]), a.stride(), a.storage_offset())
    return torch.cat([a, b], 0)


# ---------------------------------------------------------------------------------------------------------------------
# device-side pipeline (csrc/input_pipeline.hip); no CPU fallback: CPU tensors raise
# ---------------------------------------------------------------------------------------------------------------------

def _i32(t, device):
    return torch.as_tensor(t, device=device).to(torch.int32).contiguous()


def pool_clips_device(raw, offsets, T, timestamps=None):
    """Charades pair-mean pooling + zero pad of a batch (generate_video_fts_data, charades.py:177-196): ``raw`` [sum n_b, D]
    fp32 device tensor (the batch's clip features back to back), ``offsets`` [B+1] -> (video [B,T,D], nfeats [B] int32,
    framestps [B,2] int32 or None when no ``timestamps`` [B,2] (seconds) are given)."""
    from . import _lib
    from .functional import _call
    _lib.require_device(raw)
    raw = raw.contiguous()
    off = torch.as_tensor(offsets, device=raw.device).to(torch.int64).contiguous()
    B, D = off.numel() - 1, raw.shape[1]
    out = torch.empty(B, T, D, device=raw.device, dtype=torch.float32)
    nf = torch.empty(B, device=raw.device, dtype=torch.int32)
    ts = fs = None
    if timestamps is not None:
        ts = torch.as_tensor(timestamps, device=raw.device).to(torch.float64).contiguous()
        fs = torch.empty(B, 2, device=raw.device, dtype=torch.int32)
    _call("tsg_pool_clips", raw, raw.data_ptr(), off.data_ptr(), ts.data_ptr() if ts is not None else None, out.data_ptr(),
          nf.data_ptr(), fs.data_ptr() if fs is not None else None, B, T, D, _lib.TSG_F32)
    return out, nf, fs


def sequence_masks_device(nfeats, spans, T):
    """-> dict(video_mask, temporal_labels, fore_masks, back_masks), each int32 [B,T] (Sequence_mask as combined at
    charades.py:167-170) from device tensors nfeats [B] and spans [B,2]."""
    from . import _lib
    from .functional import _call
    _lib.require_device(nfeats, spans)
    nf, sp = _i32(nfeats, nfeats.device), _i32(spans, nfeats.device)
    B = nf.numel()
    vm, tl, fm, bm = (torch.empty(B, T, device=nf.device, dtype=torch.int32) for _ in range(4))
    _call("tsg_sequence_masks", nf, nf.data_ptr(), sp.data_ptr(), vm.data_ptr(), tl.data_ptr(), fm.data_ptr(), bm.data_ptr(), B, T)
    return {"video_mask": vm, "temporal_labels": tl, "fore_masks": fm, "back_masks": bm}


def gt_moment_translate_device(video, spans, nfeats, cropin_start=None, seed=0):
    """The shuffling augmentation for a whole batch on the device (gt_moment_translate, data_augment.py:135-156):
    video [B,T,D] fp32, spans [B,2], nfeats [B] -> (pseudo video [B,T,D], new spans [B,2] int32).  ``cropin_start`` [B]:
    insert positions (the reference draws them with random.randint(0, nfeats-len)); None: drawn on the device from a
    counter-based hash of (seed, sample index)."""
    from . import _lib
    from .functional import _call
    _lib.require_device(video)
    video = video.contiguous()
    B, T, D = video.shape
    sp, nf = _i32(spans, video.device), _i32(nfeats, video.device)
    ci = _i32(cropin_start, video.device) if cropin_start is not None else None
    out = torch.empty_like(video)
    new = torch.empty(B, 2, device=video.device, dtype=torch.int32)
    _call("tsg_moment_translate", video, video.data_ptr(), sp.data_ptr(), nf.data_ptr(), ci.data_ptr() if ci is not None else None,
          int(seed) & 0xFFFFFFFFFFFFFFFF, out.data_ptr(), new.data_ptr(), B, T, D, _lib.TSG_F32)
    return out, new


def cropin_positions(seed, spans, nfeats):
    """Host mirror of the device's insert-position draw (splitmix64 of (seed, b), multiply-high onto [0, nfeats-len]) --
    what ``gt_moment_translate_device(..., cropin_start=None, seed=seed)`` uses; for tests and for reproducing a batch."""
    M = (1 << 64) - 1

    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)
    out = []
    for b, ((s, e), nf) in enumerate(zip(np.asarray(spans).tolist(), np.asarray(nfeats).tolist())):
        n = e - s + 1
        if n <= 1 or n >= nf:
            out.append(s)
            continue
        h = mix((int(seed) & M) ^ ((0xD1B54A32D192ED03 * (b + 1)) & M))
        out.append(((h >> 32) * (nf - n + 1)) >> 32)
    return out


def pair_batch_device(video, nfeats, spans, query, seed=0, cropin_start=None, timestps=None):
    """The GMD training batch (keys of train.py:50-91 / charades_pair_aug.py:96-107) assembled on the device from resident
    tensors: video [B,T,D], nfeats [B], spans [B,2] (frame stamps), query [B,N,300].  Masks and the shuffled pseudo video
    come from the device kernels; nothing is copied to or from the host."""
    B, T, _ = video.shape
    sp, nf = _i32(spans, video.device), _i32(nfeats, video.device)
    pv, psp = gt_moment_translate_device(video, sp, nf, cropin_start, seed)
    m, pm = sequence_masks_device(nf, sp, T), sequence_masks_device(nf, psp, T)
    out = {"video": video, "query": query, "nfeats": nf, "video_mask": m.pop("video_mask"),
           "query_mask": torch.ones(query.shape[0], query.shape[1], dtype=torch.int32, device=video.device),
           "pseudo_video": pv, "gt": m, "pseudo_gt": pm}
    pm.pop("video_mask")                      # gt_translate keeps nfeats: the pseudo video shares the mask (engine.gmd_step)
    out["gt"]["framestps"], out["pseudo_gt"]["framestps"] = sp.long(), psp.long()
    out["gt"]["timestps"] = timestps if timestps is not None else sp.float()
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the crop family of the augmentation on the device (csrc/augment.hip)
# ---------------------------------------------------------------------------------------------------------------------

# DataAugmentForTSG's mode names (data_augment.py:13-26) -> TSG_AUG_* of include/tsg_hip.h; None is the reference's fall-through
# branch (argparse default of charades.py): gt_crop or gt_cropout per sample
AUG_MODES = {"gt_translate": 0, "gt_crop": 1, "prot_gt_crop": 2, "gt_cropout": 3, "all": 4, None: 5}


def aug_mode_code(mode):
    """TSG_AUG_* code of a reference mode name.  'shuffle_temporal' raises NotImplementedError: the reference's aug_data passes
    min_crop_width_ratio (0.2) as its seg_len (data_augment.py:36, :158-161), so that mode cannot run there either."""
    if isinstance(mode, str) and mode == "shuffle_temporal":
        raise NotImplementedError("aug_mode 'shuffle_temporal' is not supported: the reference's aug_data calls it with "
                                  "seg_len = min_crop_width_ratio = 0.2 and it fails there too")
    if mode not in AUG_MODES:
        raise ValueError(f"unknown aug_mode {mode!r}; expected one of {sorted(k for k in AUG_MODES if k)} or None")
    return AUG_MODES[mode]


_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


class _HashDraws:
    """The device's draws for one sample (csrc/augment.hip: aug_hash / draw_int / draw_unit), slot by slot."""
    GATE, FN, WIDTH, START, PICK, FB_WIDTH, FB_START = range(7)

    def __init__(self, seed, b):
        self.key = (int(seed) & _M64) ^ ((0xD1B54A32D192ED03 * (b + 1)) & _M64)

    def _h(self, slot):
        return _splitmix64(self.key ^ ((0xA0761D6478BD642F * (slot + 1)) & _M64))

    def randint(self, slot, lo, hi):
        return lo if hi <= lo else lo + (((self._h(slot) >> 32) * (hi - lo + 1)) >> 32)

    def unit(self, slot):
        return (self._h(slot) >> 11) * 2.0 ** -53


def _ceil(x, r):
    return math.ceil(x * r)


def _draw_plan(d, code, p, s, e, nf):
    """One sample's plan (op, a, b, c) as the device draws it (draw_plan in csrc/augment.hip)."""
    n = e - s + 1
    if not (p >= 1.0 or (p > 0.0 and not d.unit(_HashDraws.GATE) > p)):
        return (0, 0, 0, 0)
    fn = code
    if code == 4:
        fn = 3 if d.randint(_HashDraws.FN, 0, 1) else 2
    elif code == 5:
        fn = 3 if d.randint(_HashDraws.FN, 0, 1) else 1

    def crop(slot_w, slot_s):
        w = d.randint(slot_w, _ceil(n, 0.2), _ceil(n, 0.5))
        return (2, w, d.randint(slot_s, s, e - w + 1), 0)

    if n <= 1:
        return (0, 0, 0, 0)
    if fn == 0:
        return (1, d.randint(_HashDraws.WIDTH, 0, nf - n), 0, 0) if n < nf else (0, 0, 0, 0)
    if fn == 1:
        return crop(_HashDraws.WIDTH, _HashDraws.START)
    c = _ceil(n, 0.2)
    if fn == 2:
        ps, pe = s + c, e - c
        w = d.randint(_HashDraws.WIDTH, _ceil(pe - ps, 0.2), _ceil(pe - ps, 0.5))
        return (2, w, d.randint(_HashDraws.START, ps, pe - w + 1), 0)
    psl, psr, pel, per = s - c, s + c, e - c, e + c
    w = d.randint(_HashDraws.WIDTH, _ceil(pel - psr, 0.2), _ceil(pel - psr, 0.5))
    if w <= 0:
        return crop(_HashDraws.FB_WIDTH, _HashDraws.FB_START)
    out_start = d.randint(_HashDraws.START, psr, pel - w + 1)
    n_left = psl if psl >= w else 0
    n_right = nf - w - per if nf - 1 - per >= w else 0
    if n_left + n_right == 0:
        return (2, w, out_start, 0)
    k = d.randint(_HashDraws.PICK, 0, n_left + n_right - 1) if n_left + n_right > 1 else 0
    return (3, w, out_start, k if k < n_left else per + (k - n_left))


def augment_plans(seed, spans, nfeats, mode, aug_percentage):
    """Host mirror of the plans ``moment_augment_device(..., plan=None, seed=seed)`` draws: int32 [B,4] numpy.  For tests and
    for reproducing a batch (as ``cropin_positions`` is for the translate kernel)."""
    code = aug_mode_code(mode)
    sp = np.asarray(spans).reshape(-1, 2).tolist()
    nf = np.asarray(nfeats).reshape(-1).tolist()
    return np.array([_draw_plan(_HashDraws(seed, b), code, float(aug_percentage), int(s), int(e), int(n))
                     for b, ((s, e), n) in enumerate(zip(sp, nf))], dtype=np.int32).reshape(-1, 4)


def moment_augment_device(video, spans, nfeats, mode, aug_percentage=1.0, seed=0, plan=None):
    """``DataAugmentForTSG.aug_data`` for a whole batch on the device, one launch (csrc/augment.hip): video [B,T,D] fp32 or bf16,
    spans [B,2] frame stamps, nfeats [B] -> (out [B,T,D], new_spans [B,2] int32, new_nfeats [B] int32, plan [B,4] int32).

    ``mode``: a reference mode name ('gt_translate', 'gt_crop', 'prot_gt_crop', 'gt_cropout', 'all') or None (gt_crop or
    gt_cropout per sample).  Per sample the gate (applied with probability ``aug_percentage``), the candidate function and its
    draws come from a counter-based hash of (seed, sample index); ``augment_plans`` reproduces them on the host.  ``plan``
    [B,4] = (op, a, b, c) skips the draws: op 0 identity, 1 translate (a = cropin), 2 crop (a = width, b = start),
    3 cropout (a = width, b = out_start, c = in_start)."""
    from . import _lib
    from .functional import _call
    code = aug_mode_code(mode)
    if plan is not None:
        pl = np.asarray(plan.cpu() if isinstance(plan, torch.Tensor) else plan)
        if pl.ndim != 2 or pl.shape[1] != 4 or not np.isin(pl[:, 0], (0, 1, 2, 3)).all():
            raise ValueError(f"plan must be [B,4] with ops in 0..3, got shape {pl.shape}")
    _lib.require_device(video)
    dtype = {torch.float32: _lib.TSG_F32, torch.bfloat16: _lib.TSG_BF16}.get(video.dtype)
    if dtype is None:
        raise TypeError(f"moment_augment_device: video must be float32 or bfloat16, got {video.dtype}")
    video = video.contiguous()
    B, T, D = video.shape
    sp, nf = _i32(spans, video.device), _i32(nfeats, video.device)
    pin = _i32(plan, video.device) if plan is not None else None
    out = torch.empty_like(video)
    new_sp = torch.empty(B, 2, device=video.device, dtype=torch.int32)
    new_nf = torch.empty(B, device=video.device, dtype=torch.int32)
    pout = torch.empty(B, 4, device=video.device, dtype=torch.int32)
    _call("tsg_moment_augment", video, video.data_ptr(), sp.data_ptr(), nf.data_ptr(), code, float(aug_percentage),
          int(seed) & _M64, pin.data_ptr() if pin is not None else None, pout.data_ptr(), out.data_ptr(), new_sp.data_ptr(),
          new_nf.data_ptr(), B, T, D, dtype)
    return out, new_sp, new_nf, pout


def augment_batch_device(batch, mode, aug_percentage, seed):
    """A QAVE batch (``synthetic_batch`` / ``pair_batch_device`` keys) with the reference's per-sample augmentation applied
    (charades.py:164-170, anet.py:160-161): the video, ``nfeats``, ``video_mask`` and the gt masks and ``framestps`` (through
    ``tsg_sequence_masks``) are replaced; ``timestps`` stays as the reference leaves it.  Feeds ``engine.baseline_step``.

    nfeats > T (``sample_clips_device`` mode 'f2s_114' returns the clip count itself): the augmentation works on the T rows there
    are -- it gets min(nfeats, T), so every draw and every row it moves lies inside the video -- and the returned nfeats follows
    the reference's arithmetic on the full count (a crop subtracts its width, the other ops keep it).  The masks are the
    reference's wherever it does not raise: Sequence_mask clamps to T - 1.  For nfeats <= T this is the plain call."""
    video = batch["video"]
    T = video.shape[1]
    nf_full = _i32(batch["nfeats"], video.device)
    nf_in = torch.clamp(nf_full, max=T)
    out, sp, nf, _ = moment_augment_device(video, _i32(batch["gt"]["framestps"], video.device), nf_in, mode, aug_percentage,
                                           seed)
    nf = nf + (nf_full - nf_in)
    masks = sequence_masks_device(nf, sp, T)
    new = dict(batch)
    new["video"], new["nfeats"], new["video_mask"] = out, nf, masks.pop("video_mask")
    new["gt"] = dict(batch["gt"], **masks)
    new["gt"]["framestps"] = sp.long()
    return new


# ---------------------------------------------------------------------------------------------------------------------
# clip-feature sampling: the reference datasets' six samplers (raw clips -> [T, D] rows), numpy mirrors and the device
# kernel (csrc/input_pipeline.hip: tsg_sample_clips)
# ---------------------------------------------------------------------------------------------------------------------

# sampler names -> TSG_SAMPLE_* of include/tsg_hip.h
SAMPLE_MODES = {"pair": 0, "triple": 1, "1to1": 2, "f2s": 3, "f2s_114": 4, "lg": 5}
FRAME2SEC_RULES = ("identity", "lg", "unsupported")


def _framestamps(timestamps, T):
    """int(x) if int(x) < SAMPLE_LEN else SAMPLE_LEN - 1 (charades.py:178, anet.py:174)."""
    return [int(x) if int(x) < T else T - 1 for x in timestamps]


def generate_video_fts_data(video_fts, timestamps, T):
    """Charades' default sampler (generate_video_fts_data, charades.py:177-196): the mean of clips 2j, 2j+1 (np.mean over float32
    rows), a lone last clip copied, at most T rows.  -> (video [T,D] float64, framestamps, nfeats)."""
    n, D = np.shape(video_fts)
    out = np.zeros([T, D]) + 0.0
    add = 0
    for i in range(0, n, 2):
        out[add] = np.mean(video_fts[i:i + 2, :], 0) if i + 1 <= n - 1 else video_fts[i, :]
        add += 1
        if add == T:
            break
    return out, _framestamps(timestamps, T), add


def lg_generate_video_fts_data(video_fts, timestamps, T):
    """Charades lgi3d (lg_generate_video_fts_data, charades.py:245-269): the mean of clips 3j..3j+2, with the 2- and 1-clip
    tails.  -> (video [T,D], framestamps, nfeats)."""
    n, D = np.shape(video_fts)
    out = np.zeros([T, D]) + 0.0
    add = 0
    for i in range(0, n, 3):
        out[add] = np.mean(video_fts[i:i + 3, :], 0) if i + 1 <= n - 1 else video_fts[i, :]
        add += 1
        if add == T:
            break
    return out, _framestamps(timestamps, T), add


def sample_1to1_video_feat(video_fts, timestamps, T):
    """ANet i3d (sample_1to1_video_feat, anet.py:193-208): the first min(n, T) clips.  -> (video [T,D], framestamps, nfeats)."""
    n, D = np.shape(video_fts)
    out = np.zeros([T, D]) + 0.0
    add = min(n, T)
    out[:add] = video_fts[:add, :]
    return out, _framestamps(timestamps, T), add


def _f2s_rows(duration, T):
    """The output rows the frame2second samplers fill: i < duration and i < T (anet.py:185-186, :221-222)."""
    return [i for i in range(T) if i < duration]


def sample_frame2second(video_fts, timestamps, duration, T):
    """ANet c3d 'raw' (sample_frame2second, anet.py:173-191): rate = n / duration; row i < duration (and < T) is clip
    floor(i * rate).  -> (video [T,D], framestamps, nfeats = the number of such rows)."""
    n, D = np.shape(video_fts)
    rate = n / duration
    rows = _f2s_rows(duration, T)
    out = np.zeros([T, D])
    out[rows] = video_fts[[max(0, math.floor(i * rate)) for i in rows]]
    return out, _framestamps(timestamps, T), len(rows)


def _f2s_114_window(i, n, rate):
    """[start, end) of row i of sample_frame2second_114 (anet.py:223-228); a window of one clip where it copies."""
    start = min(n - 1, max(0, int(i * rate + 0.5)))
    end = int((i + 1) * rate + 0.5)
    return (start, start + 1) if end > n or end <= start else (start, end)


def sample_frame2second_114(video_fts, timestamps, duration, T):
    """ANet c3d '114' and any unknown name (sample_frame2second_114, anet.py:210-230): row i < duration (and < T) is the mean of
    clips [start, end) with start = min(n-1, int(i*rate + 0.5)), end = int((i+1)*rate + 0.5), or a copy of clip start when
    end > n or end <= start.  -> (video [T,D], framestamps, nfeats = n -- NOT clamped to T, as the reference returns it)."""
    n, D = np.shape(video_fts)
    rate = n / duration
    out = np.zeros([T, D])
    for i in _f2s_rows(duration, T):
        lo, hi = _f2s_114_window(i, n, rate)
        out[i] = video_fts[lo] if hi - lo == 1 else np.mean(video_fts[lo:hi, :], 0)
    return out, _framestamps(timestamps, T), n


def lg_spos_range(n, T):
    """The inclusive range [0, hi] of LG's training start position: the reference draws np.random.random_integers(0, r) with
    r = stride - 0.5, lowered by 1 when integral, and random_integers draws from [0, int(r)] (charades.py:209-215,
    anet.py:243-249).  n <= T (stride 1): [0, 0]."""
    stride = n / T if n > T else 1.0
    r = stride - 0.5
    return 0, int(r - 1.0 if r == math.floor(r) else r)


def lg_positions(n, T, spos):
    """The clips LG samples (charades.py:216-225, anet.py:250-259): rint of np.arange(spos, n - 0.5, stride), at most T of them.
    np.arange itself forms the values (start, start + step, then start + i*((start + step) - start)); min(n, T) entries on
    every input the reference accepts."""
    stride = n * 1.0 / T if n > T else 1
    return np.round(np.arange(spos, n - 0.5, stride)).astype(int)[:T]


def _lg_label(s, pos, default):
    """The i with s[i] <= pos < s[i+1] (the last such i; the positions are increasing, so there is at most one), else default."""
    hits = [i for i in range(len(s) - 1) if s[i] <= pos < s[i + 1]]
    return hits[-1] if hits else default


def lg_get_fixed_length_feat(feat, timestamps, duration, T, spos=0):
    """vfeat_fn 'lg' (lg_get_fixed_length_feat, charades.py:198-243 = anet.py:232-277) with the start position ``spos`` given
    (the reference: 0 outside training, a draw over ``lg_spos_range`` in training).  Rows feat[s[t]] for s = ``lg_positions``;
    the labels are the ``_lg_label`` of (n - 1) * clamp(timestamp / duration, 0, 1), defaults 0 and T - 1.
    -> (video [T,D], (start_index, end_index), nfeats = min(n, T))."""
    n = feat.shape[0]
    s = lg_positions(n, T, spos)
    ps, pe = (float(n - 1.0) * min(max(x / duration, 0), 1) for x in timestamps[:2])
    out = np.zeros((T, feat.shape[1]))
    out[:len(s)] = feat[s]
    return out, (_lg_label(s, ps, 0), _lg_label(s, pe, T - 1)), min(n, T)


VfeatMode = collections.namedtuple("VfeatMode", "sampler frame2sec")


def vfeat_mode(dataset, feature_type, vfeat_fn):
    """The reference's choice of sampler and of frame2sec rule from (dataset, feature_type, vfeat_fn) -> VfeatMode(sampler,
    frame2sec), sampler in SAMPLE_MODES, frame2sec in FRAME2SEC_RULES.

    Charades (charades.py:101-107, :275-279): vfeat_fn.lower() == 'lg' -> 'lg'; else feature_type 'lgi3d' -> 'triple'; else
    'pair'.  frame2sec converts only when vfeat_fn is exactly 'lg' (an 'LG' samples as lg but keeps frame indices).
    ActivityNet (anet.py:66-79, :283-289): feature_type 'i3d' -> '1to1' whatever vfeat_fn says; else 'raw' -> 'f2s', '114' ->
    'f2s_114', 'lg' -> 'lg', any other name -> 'f2s_114' (and the name becomes '114').  frame2sec keys on the NAME: ANet i3d
    with vfeat_fn 'lg' samples 1:1 but converts as lg; ANet i3d with an unknown name samples 1:1 and its frame2sec raises
    ('unsupported')."""
    ds = str(dataset).lower()
    if ds.startswith("charades"):
        if vfeat_fn.lower() == "lg":
            sampler = "lg"
        elif feature_type.lower() in ["lgi3d"]:
            sampler = "triple"
        else:
            sampler = "pair"
        return VfeatMode(sampler, "lg" if vfeat_fn in ["lg"] else "identity")
    if ds.startswith("anet") or ds.startswith("activitynet"):
        name = vfeat_fn
        if feature_type in ["i3d"]:
            sampler = "1to1"
        elif vfeat_fn in ["raw"]:
            sampler = "f2s"
        elif vfeat_fn in ["114"]:
            sampler = "f2s_114"
        elif vfeat_fn in ["lg"]:
            sampler = "lg"
        else:
            name, sampler = "114", "f2s_114"
        rule = "identity" if name in ["raw", "114"] else ("lg" if name in ["lg"] else "unsupported")
        return VfeatMode(sampler, rule)
    raise ValueError(f"unknown dataset {dataset!r}: expected Charades or ActivityNet")


def sample_clips_numpy(video_fts, timestamps, duration, T, mode, spos=0):
    """One sample through the numpy mirror of ``mode`` (a SAMPLE_MODES name) -> (video [T,D], framestps, nfeats)."""
    if mode == "pair":
        return generate_video_fts_data(video_fts, timestamps, T)
    if mode == "triple":
        return lg_generate_video_fts_data(video_fts, timestamps, T)
    if mode == "1to1":
        return sample_1to1_video_feat(video_fts, timestamps, T)
    if mode == "f2s":
        return sample_frame2second(video_fts, timestamps, duration, T)
    if mode == "f2s_114":
        return sample_frame2second_114(video_fts, timestamps, duration, T)
    if mode == "lg":
        return lg_get_fixed_length_feat(video_fts, timestamps, duration, T, spos)
    raise ValueError(f"unknown sampling mode {mode!r}; expected one of {sorted(SAMPLE_MODES)}")


def lg_spos_draws(seed, n_clips, T):
    """Host mirror of the device's LG training draws (``sample_clips_device(..., mode='lg', train=True, seed=seed)``): per sample
    a counter-based hash of (seed, b) mapped by multiply-high onto the inclusive range of ``lg_spos_range``.  int32 [B]."""
    out = []
    for b, n in enumerate(np.asarray(n_clips).reshape(-1).tolist()):
        _, hi = lg_spos_range(int(n), int(T))
        if hi <= 0:
            out.append(0)
            continue
        h = _splitmix64((int(seed) & _M64) ^ ((0xD1B54A32D192ED03 * (b + 1)) & _M64) ^ 0x8CB92BA72F3D8DD7)
        out.append(((h >> 32) * (hi + 1)) >> 32)
    return np.array(out, dtype=np.int32)


def sample_code(mode):
    if isinstance(mode, str) and mode in SAMPLE_MODES:
        return SAMPLE_MODES[mode]
    raise ValueError(f"unknown sampling mode {mode!r}; expected one of {sorted(SAMPLE_MODES)}")


def sample_clips_device(raw, offsets, T, mode, timestamps=None, durations=None, train=False, seed=0, spos=None,
                        out_dtype=torch.float32):
    """The reference's per-sample sampler for a whole batch in one launch (tsg_sample_clips): ``raw`` [sum n_b, D] fp32 device
    tensor (the batch's clips back to back), ``offsets`` [B+1], ``mode`` a SAMPLE_MODES name, ``timestamps`` [B,2] seconds,
    ``durations`` [B] seconds ('f2s', 'f2s_114', 'lg' need them; 'lg' needs timestamps).  'lg' draws its start position per
    sample in training (``train``; host mirror: ``lg_spos_draws``) unless ``spos`` [B] is given; 0 otherwise.
    -> (video [B,T,D] ``out_dtype`` (float32, or bfloat16 = the fp32 rows rounded to nearest-even), nfeats [B] int32,
    framestps [B,2] int32 or None without timestamps, spos [B] int32: the start positions used, 0 outside 'lg')."""
    from . import _lib
    from .functional import _call
    code = sample_code(mode)
    dt = {torch.float32: _lib.TSG_F32, torch.bfloat16: _lib.TSG_BF16}.get(out_dtype)
    if dt is None:
        raise TypeError(f"sample_clips_device: out_dtype must be float32 or bfloat16, got {out_dtype}")
    if mode in ("f2s", "f2s_114", "lg") and durations is None:
        raise ValueError(f"sampling mode {mode!r} needs durations")
    if mode == "lg" and timestamps is None:
        raise ValueError("sampling mode 'lg' needs timestamps")
    _lib.require_device(raw)
    if raw.dtype != torch.float32 or raw.dim() != 2:
        raise TypeError(f"sample_clips_device: raw must be a [sum n, D] float32 tensor, got {raw.dtype} {tuple(raw.shape)}")
    raw = raw.contiguous()
    dev = raw.device
    off = torch.as_tensor(offsets, device=dev).to(torch.int64).contiguous()
    B, D = off.numel() - 1, raw.shape[1]
    out = torch.empty(B, T, D, device=dev, dtype=out_dtype)
    nf = torch.empty(B, device=dev, dtype=torch.int32)
    sp_out = torch.empty(B, device=dev, dtype=torch.int32)
    ts = fs = du = sp_in = None
    if timestamps is not None:
        ts = torch.as_tensor(timestamps, device=dev).to(torch.float64).reshape(B, 2).contiguous()
        fs = torch.empty(B, 2, device=dev, dtype=torch.int32)
    if durations is not None:
        du = torch.as_tensor(durations, device=dev).to(torch.float64).reshape(B).contiguous()
    if spos is not None:
        sp_in = _i32(spos, dev).reshape(B)

    def p(t):
        return t.data_ptr() if t is not None else None
    _call("tsg_sample_clips", raw, raw.data_ptr(), off.data_ptr(), p(ts), p(du), code, int(bool(train)), int(seed) & _M64,
          p(sp_in), out.data_ptr(), nf.data_ptr(), p(fs), sp_out.data_ptr(), B, T, D, dt)
    return out, nf, fs, sp_out


def frame2sec(pred, durations, nfeats, rule):
    """The datasets' frame2sec on a batch of predicted [start, end] frame indices (charades.py:271-279, anet.py:279-289).
    'identity': returned as given; 'lg': _lg_frame2sec = pred / nfeats[:, None] * durations[:, None], on tensors with the
    dtypes of the reference's collate_fn and test loop (pred float32, durations float64, nfeats int64): the quotient is
    float32, the result float64; 'unsupported': NotImplementedError, as the reference's ANet frame2sec raises."""
    if rule == "identity":
        return pred
    if rule == "unsupported":
        raise NotImplementedError("frame2sec: the reference has no rule for this vfeat_fn")
    if rule != "lg":
        raise ValueError(f"unknown frame2sec rule {rule!r}; expected one of {FRAME2SEC_RULES}")
    pred = torch.as_tensor(pred).float()
    dur = durations if isinstance(durations, torch.Tensor) else torch.from_numpy(np.array(durations, dtype=np.float64))
    nf = nfeats if isinstance(nfeats, torch.Tensor) else torch.from_numpy(np.array(nfeats, dtype=np.int64))
    pos = pred / nf.to(pred.device).unsqueeze(1)
    return pos * dur.to(pred.device).unsqueeze(1)


def clip_batch_device(raw, offsets, T, mode, query, timestamps, durations=None, train=False, seed=0, spos=None, pair=False,
                      cropin_start=None, out_dtype=torch.float32, aug=None):
    """One batch from raw clip features on the device: ``sample_clips_device`` then the QAVE masks (``pair=False``: the keys of
    ``synthetic_batch``; ``aug`` = (aug_mode, aug_percentage) applies the trainers' augmentation through
    ``augment_batch_device`` with ``seed``) or the GMD pair (``pair=True``: ``pair_batch_device``, shuffled with the insert
    positions ``cropin_start`` or drawn from ``seed``; fp32 only).  query [B,N,300] device tensor.

    nfeats > T: 'f2s_114' returns clip counts above T (the reference's collate passes them on, and its shuffling augmentation
    raises on them).  The masks, the GMD shuffle and the augmentation get min(nfeats, T) -- Sequence_mask clamps to T - 1, so
    the masks are the reference's -- and batch['nfeats'] is the count as the reference computes it (``augment_batch_device``
    holds the same rule for the QAVE augmentation).  Adds 'durations' (float64) and gt 'timestps' (float32, as collate_fn)
    for ``engine.evaluate`` / ``frame2sec``."""
    if pair and aug is not None:
        raise ValueError("clip_batch_device: the GMD pair carries its own shuffle; aug applies to QAVE batches (pair=False)")
    dev = raw.device
    video, nf, fs, sp = sample_clips_device(raw, offsets, T, mode, timestamps, durations, train, seed, spos, out_dtype)
    nf_c = torch.clamp(nf, max=T)
    ts = torch.as_tensor(timestamps).to(torch.float64).reshape(-1, 2).float().to(dev)
    if pair:
        if out_dtype != torch.float32:
            raise TypeError("clip_batch_device: the GMD pair is built in float32")
        batch = pair_batch_device(video, nf_c, fs, query, seed=seed, cropin_start=cropin_start, timestps=ts)
    else:
        m = sequence_masks_device(nf_c, fs, T)
        batch = {"video": video, "query": query, "video_mask": m.pop("video_mask"),
                 "query_mask": torch.ones(query.shape[0], query.shape[1], dtype=torch.int32, device=dev), "gt": m}
        batch["gt"]["framestps"], batch["gt"]["timestps"] = fs.long(), ts
    batch["nfeats"], batch["spos"] = nf, sp
    if aug is not None:
        batch = augment_batch_device(batch, aug[0], aug[1], seed)
    if durations is not None:
        batch["durations"] = torch.as_tensor(durations).to(torch.float64).reshape(-1).to(dev)
    return batch

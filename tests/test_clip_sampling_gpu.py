"""tsg_sample_clips on the device: the reference golden (tests/golden/clip_sampling.npz) bit for bit, every mode at user shapes
against the numpy mirrors (fp32 bit-exact, bf16 = the fp32 rows rounded to nearest-even), PAIR == tsg_pool_clips, LG's training
draws, the translate kernels on spans past nfeats, GMD pair batches built on the device vs the host, one GMD train step from a
device-built ActivityNet-CD batch (T = 240), and evaluate's frame2sec."""
import numpy as np
import pytest
import torch

from shufflingvideosfortsg_amd import data

pytestmark = pytest.mark.gpu
NAMES = {v: k for k, v in data.SAMPLE_MODES.items()}


@pytest.fixture(scope="module")
def golden():
    from conftest import Golden
    return Golden("clip_sampling")


def test_golden_cases_through_the_kernel(golden):
    a = golden.a
    D = a["raw"].shape[1]
    for i in range(len(a["mode"])):
        mode, T = NAMES[int(a["mode"][i])], int(a["T"][i])
        raw = torch.from_numpy(a["raw"][a["raw_off"][i]:a["raw_off"][i + 1]]).cuda()
        n = raw.shape[0]
        spos = [int(a["spos"][i])] if mode == "lg" and int(a["spos_hi"][i]) >= 0 else None
        want = torch.from_numpy(a["out"][a["out_off"][i]:a["out_off"][i + 1]].reshape(1, T, D))
        for dt in (torch.float32, torch.bfloat16):
            out, nf, fs, sp = data.sample_clips_device(raw, [0, n], T, mode, a["timestamps"][i:i + 1], a["duration"][i:i + 1],
                                                       spos=spos, out_dtype=dt)
            w = want if dt == torch.float32 else want.to(torch.bfloat16)
            assert torch.equal(out.cpu(), w), (i, mode, n, T, dt)
            assert int(nf[0]) == int(a["nfeats"][i]) and fs[0].tolist() == a["framestps"][i].tolist(), (i, mode, fs, nf)
            assert int(sp[0]) == (int(a["spos"][i]) if mode == "lg" else 0)


def _user_batch(B, T, D, seed):
    rs = np.random.RandomState(seed)
    n = np.concatenate([[1, 2, 3, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T, 10 * T], rs.randint(1, 10 * T + 1, size=B - 10)])
    rs.shuffle(n)
    off = np.concatenate([[0], np.cumsum(n)])
    raw = torch.from_numpy(rs.randn(int(off[-1]), D).astype(np.float32))
    rate = np.exp(rs.uniform(np.log(0.3), np.log(12.0), size=B))        # clips per second: windows of 0 .. ~12 clips
    dur = np.round(n / rate, 2) + 0.0
    dur[:3] = [T + 0.5, 2.0 * T, T / 2 + 0.25]                          # durations above T
    ts = np.sort(rs.uniform(-2.0, 1.1, size=(B, 2)) * dur[:, None], axis=1)
    return raw, off, n, dur, ts


@pytest.mark.parametrize("B,T,D", [(64, 240, 1024), (64, 240, 500), (64, 128, 1024)])
def test_every_mode_at_user_shapes_equals_the_mirrors(B, T, D):
    raw, off, n, dur, ts = _user_batch(B, T, D, seed=T + D)
    raw_d = raw.cuda()
    rawn = raw.numpy()
    for mode in data.SAMPLE_MODES:
        train = mode == "lg"
        out, nf, fs, sp = data.sample_clips_device(raw_d, off, T, mode, ts, dur, train=train, seed=7)
        outb, nfb, fsb, spb = data.sample_clips_device(raw_d, off, T, mode, ts, dur, train=train, seed=7, out_dtype=torch.bfloat16)
        out, nf, fs, sp = out.cpu(), nf.cpu().numpy(), fs.cpu().numpy(), sp.cpu().numpy()
        assert torch.equal(outb.cpu(), out.to(torch.bfloat16)), mode
        assert np.array_equal(nfb.cpu().numpy(), nf) and np.array_equal(fsb.cpu().numpy(), fs) and np.array_equal(spb.cpu().numpy(), sp)
        if train:
            np.testing.assert_array_equal(sp, data.lg_spos_draws(7, n, T))
        for b in range(B):
            v, f, k = data.sample_clips_numpy(rawn[off[b]:off[b + 1]], ts[b].tolist(), float(dur[b]), T, mode, int(sp[b]))
            assert torch.equal(out[b], torch.from_numpy(v.astype(np.float32))), (mode, b, int(n[b]), float(dur[b]))
            assert [int(x) for x in f] == fs[b].tolist() and k == nf[b], (mode, b, f, fs[b], k, nf[b])


def test_pair_mode_is_pool_clips():
    raw, off, n, dur, ts = _user_batch(64, 128, 1024, seed=3)
    raw = raw.cuda()
    a = data.sample_clips_device(raw, off, 128, "pair", ts)
    b = data.pool_clips_device(raw, off, 128, ts)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


def test_lg_training_draws():
    raw, off, n, dur, ts = _user_batch(64, 240, 64, seed=5)
    raw = raw.cuda()
    r = {s: data.sample_clips_device(raw, off, 240, "lg", ts, dur, train=True, seed=s) for s in (11, 11, 12)}
    a, b = data.sample_clips_device(raw, off, 240, "lg", ts, dur, train=True, seed=11), r[11]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(r[11][3], r[12][3])
    np.testing.assert_array_equal(r[12][3].cpu().numpy(), data.lg_spos_draws(12, n, 240))
    for b_ in range(64):
        lo, hi = data.lg_spos_range(int(n[b_]), 240)
        assert lo <= int(r[12][3][b_]) <= hi
    given = np.array([data.lg_spos_range(int(k), 240)[1] for k in n], np.int32)            # the top of every range
    out, nf, fs, sp = data.sample_clips_device(raw, off, 240, "lg", ts, dur, spos=given)
    np.testing.assert_array_equal(sp.cpu().numpy(), given)
    rawn = raw.cpu().numpy()
    for b_ in range(64):
        v, f, k = data.lg_get_fixed_length_feat(rawn[off[b_]:off[b_ + 1]], ts[b_].tolist(), float(dur[b_]), 240, int(given[b_]))
        assert torch.equal(out[b_].cpu(), torch.from_numpy(v.astype(np.float32))) and list(f) == fs[b_].tolist() and k == int(nf[b_])
    test = data.sample_clips_device(raw, off, 240, "lg", ts, dur, train=False, seed=11)
    assert int(test[3].abs().sum()) == 0


def test_translate_kernels_past_nfeats_equal_golden(golden):
    a = golden.a
    v = torch.from_numpy(a["tr_video"]).float().cuda()
    sp, nf, c = a["tr_fs"], a["tr_nfeats"], a["tr_cropin"]
    out, new = data.gt_moment_translate_device(v, sp, nf, c)
    assert torch.equal(out.cpu().double(), torch.from_numpy(a["tr_out_video"])) and np.array_equal(new.cpu().numpy(), a["tr_out_fs"])
    plan = np.stack([np.ones_like(c), c, 0 * c, 0 * c], 1)
    for dt in (torch.float32, torch.bfloat16):
        out, new, nnf, _ = data.moment_augment_device(v.to(dt), sp, nf, "gt_translate", plan=plan)
        assert torch.equal(out.cpu(), torch.from_numpy(a["tr_out_video"]).to(dt)), dt
        assert np.array_equal(new.cpu().numpy(), a["tr_out_fs"]) and np.array_equal(nnf.cpu().numpy(), nf)


def _host_pair(raw, off, T, mode, ts, dur, spos, cropin):
    """The GMD pair built on the host: the mirrors, then data.gt_moment_translate on min(nfeats, T) with the given positions."""
    B = len(off) - 1
    v, pv, fs, pfs, nfs = [], [], [], [], []
    for b in range(B):
        x, f, k = data.sample_clips_numpy(raw[off[b]:off[b + 1]], ts[b].tolist(), float(dur[b]), T, mode, int(spos[b]))
        x = x.astype(np.float32)[None]
        nf2, _, px = data.gt_moment_translate([int(f[0]), int(f[1])], min(k, T), x, int(cropin[b]))
        v.append(x[0]); pv.append(px[0].astype(np.float32)); fs.append([int(f[0]), int(f[1])]); pfs.append(nf2); nfs.append(k)
    return np.stack(v), np.stack(pv), np.array(fs), np.array(pfs), np.array(nfs)


@pytest.mark.parametrize("mode,T", [("lg", 64), ("f2s_114", 64), ("pair", 64)])
def test_gmd_pair_batch_device_equals_host(mode, T):
    B, D = 16, 32
    raw, off, n, dur, ts = _user_batch(B, T, D, seed=21)
    ts = np.maximum(ts, 0.0)                                               # the augmentation takes frame stamps >= 0
    if mode == "lg":
        ts[:, 1] = dur + 1.0                                               # moments that reach the video's end: end label T - 1
    q = torch.randn(B, 25, 300).cuda()
    batch = data.clip_batch_device(raw.cuda(), off, T, mode, q, ts, dur, train=True, seed=9, pair=True)
    spos = batch["spos"].cpu().numpy()
    nf = batch["nfeats"].cpu().numpy()
    fs = batch["gt"]["framestps"].cpu().numpy()
    cropin = data.cropin_positions(9, fs, np.minimum(nf, T))
    v, pv, hfs, hpfs, hnf = _host_pair(raw.numpy(), off, T, mode, ts, dur, spos, cropin)
    assert torch.equal(batch["video"].cpu(), torch.from_numpy(v)) and torch.equal(batch["pseudo_video"].cpu(), torch.from_numpy(pv))
    np.testing.assert_array_equal(fs, hfs)
    np.testing.assert_array_equal(batch["pseudo_gt"]["framestps"].cpu().numpy(), hpfs)
    np.testing.assert_array_equal(nf, hnf)
    for k in ("temporal_labels", "fore_masks", "back_masks"):
        for g, f in (("gt", hfs), ("pseudo_gt", hpfs)):
            want = np.stack([data.Sequence_mask(T, fb if k == "temporal_labels" else ([0, fb[0]] if k == "fore_masks" else [fb[1], nb]))
                             for fb, nb in zip(f.tolist(), hnf.tolist())])
            np.testing.assert_array_equal(batch[g][k].cpu().numpy(), want, err_msg=f"{g}.{k}")
    np.testing.assert_array_equal(batch["video_mask"].cpu().numpy(), np.stack([data.Sequence_mask(T, [0, int(k)]) for k in hnf]))
    if mode == "lg":
        assert (hfs[:, 1] == T - 1).sum() >= 4 and (hfs[:, 1] >= np.minimum(hnf, T)).any()
    if mode == "f2s_114":
        assert (hnf > T).sum() >= 4


def test_gmd_step_from_device_anet_cd_batch(request):
    """The published ActivityNet-CD run (i3d, T = 240, N = 25, d = 512): one f32s GMD train step from a batch built on the device;
    at B = 2 the boundary scores match the CPU oracle."""
    from oracle import tsg_oracle as O
    from shufflingvideosfortsg_amd import engine, functional as TF
    T, N = 240, 25
    engine.set_precision("f32s")
    request.addfinalizer(lambda: engine.set_precision(None))
    params = engine.default_params(video_rnn_hiddendim=512, sent_rnn_hiddendim=512, dropout=0.0, video_len=T, sent_len=N)
    torch.manual_seed(0)
    model = engine.build_model("gmd", params)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model = model.cuda().train()
    model.tod.dropout.p = 0.0
    opt = engine.make_optimizer(model, params)
    engine.skipped_updates(reset=True)
    for B in (16, 2):
        raw, off, n, dur, ts = _user_batch(max(B, 10), T, 1024, seed=B)
        raw, off, dur, ts = raw[:int(off[B])], off[:B + 1], dur[:B], np.maximum(ts[:B], 0.0)   # real spans: frame stamps >= 0
        q = (torch.randn(B, N, 300) * 0.4).cuda()
        batch = data.clip_batch_device(raw.cuda(), off, T, "1to1", q, ts, dur, pair=True, seed=3)
        model.zero_grad(set_to_none=True)
        loss, _, span = engine.gmd_step(model, batch, params)
        loss.backward()
        torch.cuda.synchronize(); TF.check_lstm_errors()
        assert torch.isfinite(loss)
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
        assert (batch["gt"]["temporal_labels"].sum(1) > 0).all()                   # every sample has a non-empty moment
        if B == 16:
            engine.optimizer_step(opt, loss)
            torch.cuda.synchronize()
            assert engine.skipped_updates() == 0
            sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
            continue
        c = {k: v.cpu() for k, v in batch.items() if isinstance(v, torch.Tensor)}
        g, pg = ({k: v.cpu() for k, v in batch[x].items()} for x in ("gt", "pseudo_gt"))
        ref = O.gmd_forward(sd, c["query"], c["video"], c["video_mask"], c["pseudo_video"], c["video_mask"],
                            g["temporal_labels"], g["fore_masks"], g["back_masks"], pg["temporal_labels"], pg["fore_masks"], pg["back_masks"])
        torch.testing.assert_close(span["start"].detach().cpu(), ref[0]["start"].detach(), atol=1e-4, rtol=1e-4)
        torch.testing.assert_close(span["end"].detach().cpu(), ref[0]["end"].detach(), atol=1e-4, rtol=1e-4)


def test_evaluate_lg_seconds():
    from shufflingvideosfortsg_amd import engine
    from shufflingvideosfortsg_amd import loss as L
    T, B = 32, 4
    params = engine.default_params(video_rnn_hiddendim=64, sent_rnn_hiddendim=64, mlp_hidden_dim=64, m_pred_hidden=128,
                                   dropout=0.0, video_feature_dim=64, video_len=T)
    torch.manual_seed(0)
    model = engine.build_model("baseline", params).cuda()
    raw, off, n, dur, ts = _user_batch(10, T, 64, seed=8)
    raw, off, dur, ts = raw[:int(off[B])], off[:B + 1], dur[:B], ts[:B]
    q = (torch.randn(B, 10, 300) * 0.4).cuda()
    batch = data.clip_batch_device(raw.cuda(), off, T, "lg", q, ts, dur)
    plain = engine.evaluate(model, [batch])
    sec = engine.evaluate(model, [batch], vfeat_mode="lg")
    again = engine.evaluate(model, [batch], vfeat_mode=data.vfeat_mode("anet", "i3d", "lg"))
    with torch.no_grad():
        out = model(batch["video"], batch["query"], batch["video_mask"], batch["query_mask"])
        pred, _ = L.span_pred(out["start"], out["end"])
    frames = pred.float().cpu()
    want = data.frame2sec(frames, dur.tolist(), batch["nfeats"].cpu().long(), "lg").numpy()
    got = np.array([r["timestamp"] for r in sec["results"]["b0"]])
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(np.array([r["timestamp"] for r in again["results"]["b0"]]), want)
    np.testing.assert_array_equal(np.array([r["timestamp"] for r in plain["results"]["b0"]]), frames.numpy())


def test_crop_family_past_nfeats_on_the_device(golden):
    """tsg_moment_augment with the reference's recorded draws (as plans) on LG spans that end past nfeats equals the golden."""
    from test_clip_sampling_cpu import crop_plan
    a = golden.a
    fs, nf = a["crop_fs"], a["crop_nfeats"]
    plan = np.array([crop_plan(int(a["crop_fn"][i]), fs[i].tolist(), int(nf[i]), a["crop_draws"][i].tolist())
                     for i in range(len(nf))], np.int32)
    v = torch.from_numpy(a["crop_video"]).float().cuda()
    for dt in (torch.float32, torch.bfloat16):
        out, nsp, nnf, _ = data.moment_augment_device(v.to(dt), fs, nf, "gt_crop", plan=plan)
        assert torch.equal(out.cpu(), torch.from_numpy(a["crop_out_video"]).to(dt)), dt
        assert np.array_equal(nsp.cpu().numpy(), a["crop_out_fs"]) and np.array_equal(nnf.cpu().numpy(), a["crop_out_nfeats"])


@pytest.mark.parametrize("aug_mode", ["gt_translate", "gt_crop", "gt_cropout", None])
def test_qave_augmented_batch_with_nfeats_above_t(aug_mode):
    """An f2s_114 QAVE batch (nfeats > T) through the trainers' augmentation (clip_batch_device(aug=...) -> augment_batch_device):
    the augmentation sees min(nfeats, T); the result equals the host mirrors + data.augment_plans / apply_plan on min(nfeats, T),
    with the returned nfeats = the reference's count (a crop subtracts its width)."""
    B, T, D, seed = 16, 64, 32, 13
    raw, off, n, dur, ts = _user_batch(B, T, D, seed=29)
    ts = np.maximum(ts, 0.0)
    q = torch.randn(B, 25, 300).cuda()
    batch = data.clip_batch_device(raw.cuda(), off, T, "f2s_114", q, ts, dur, seed=seed, aug=(aug_mode, 1.0))
    rawn = raw.numpy()
    host = [data.sample_clips_numpy(rawn[off[b]:off[b + 1]], ts[b].tolist(), float(dur[b]), T, "f2s_114") for b in range(B)]
    fs = np.array([[int(x) for x in h[1]] for h in host])
    nf = np.array([h[2] for h in host])
    nf_in = np.minimum(nf, T)
    assert (nf > T).sum() >= 4
    plans = data.augment_plans(seed, fs, nf_in, aug_mode, 1.0)
    assert (plans[nf > T, 0] != 0).any()
    want_v, want_fs, want_nf = [], [], []
    for b in range(B):
        f2, k2, v2 = data.apply_plan(fs[b].tolist(), int(nf_in[b]), host[b][0][None].astype(np.float32), plans[b])
        want_v.append(v2[0].astype(np.float32)); want_fs.append([int(f2[0]), int(f2[1])])
        want_nf.append(int(nf[b]) + (int(k2) - int(nf_in[b])))
    assert torch.equal(batch["video"].cpu(), torch.from_numpy(np.stack(want_v)))
    np.testing.assert_array_equal(batch["gt"]["framestps"].cpu().numpy(), np.array(want_fs))
    np.testing.assert_array_equal(batch["nfeats"].cpu().numpy(), np.array(want_nf))
    assert (np.array(want_fs)[:, 1] < T).all()                              # every moment stays inside the video
    for k, want in (("video_mask", [[0, k] for k in want_nf]), ("temporal_labels", want_fs),
                    ("fore_masks", [[0, f[0]] for f in want_fs]), ("back_masks", [[f[1], k] for f, k in zip(want_fs, want_nf)])):
        got = batch[k] if k == "video_mask" else batch["gt"][k]
        np.testing.assert_array_equal(got.cpu().numpy(), np.stack([data.Sequence_mask(T, w) for w in want]), err_msg=k)

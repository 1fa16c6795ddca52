"""tests/gemm_f64.py on the CPU: the reference pinned to torch.mm in float64, the designed value hi hi' + hi lo' + lo hi' held to its provable
distance from it and to its share of the f32s contract on every operand family, the head epilogues' fp32 batch-index formula against integer
division up to the limit check_head enforces, and the tile plan of csrc/gemm_f32s.hip against a table for 256 CUs."""
import numpy as np
import pytest
import torch

import gemm_f64 as G

KS = (32, 96, 1024, 4096)


@pytest.fixture(scope="module")
def designed():
    """(family, K) -> (ref, D, A) of a 64 x 64 output, computed once"""
    out = {}
    for kind in G.FAMILIES:
        for K in KS:
            X, W = G.family(kind, 64, 64, K)
            out[kind, K] = (X, W) + G.products(X, W.t())
    return out


def test_reference_is_the_float64_product_and_the_split_is_exact(designed):
    for (kind, K), (X, W, ref, D, A) in designed.items():
        assert X.dtype == torch.float32 and W.dtype == torch.float32
        assert torch.equal(ref, torch.mm(X.double(), W.double().t())), (kind, K)
        assert torch.equal(A, torch.mm(X.double().abs(), W.double().abs().t())), (kind, K)
        for t in (X, W):
            mag = t[t != 0].abs()
            assert float(mag.min()) >= G.MAG_LO * (1 - 1e-6) and float(mag.max()) <= G.MAG_HI * (1 + 1e-6), (kind, K)
            hi, lo = G.split(t)
            assert torch.equal(hi, hi.to(G.BF).double()) and torch.equal(lo, lo.to(G.BF).double())      # both planes are bf16 values
            assert bool(((hi + lo - t.double()).abs() <= 2.0 ** -16 * t.double().abs()).all()), (kind, K)
            tiny = torch.finfo(G.BF).tiny
            assert bool(((lo == 0) | (lo.abs() >= tiny)).all()), (kind, K)                               # lo never reaches the subnormals
        Xh, Xl = G.split(X); Wh, Wl = G.split(W)
        want = torch.mm(Xh, Wh.t()) + torch.mm(Xh, Wl.t()) + torch.mm(Xl, Wh.t())
        assert torch.equal(D, want), (kind, K)


def test_families_are_what_they_claim():
    X, W = G.family("lomax", 64, 64, 96)
    for t in (X, W):
        hi, lo = G.split(t)
        assert bool((lo > 0).all()) and bool((lo >= 0.49 * 2.0 ** -8 * hi / 2.0).all())                 # lo at its largest (hi in [m, 2m)), one sign
    X, W = G.family("lomax_neg", 64, 64, 96)
    assert bool((X > 0).all()) and bool((W < 0).all())
    X, W = G.family("cancel", 64, 64, 96)
    ref, D, A = G.products(X, W.t())
    assert float(ref.abs().max()) <= 1e-12 * float(A.max()) and float(D.abs().max()) <= 1e-12 * float(A.max())
    X, W = G.family("zeros", 64, 64, 96)
    assert float(X[::3].abs().max()) == 0.0 and float(W[:, ::2].abs().max()) == 0.0
    X, W = G.family("perm", 64, 96, 96)
    pi = G.perm_of(96, 96)
    assert sorted(pi.tolist()) == list(range(96)) and not torch.equal(pi[pi], torch.arange(96))         # a permutation, not an involution
    assert torch.equal(W.sum(1), torch.ones(96)) and torch.equal(W[torch.arange(96), pi], torch.ones(96))
    hi, lo = G.split(X)
    assert torch.equal(G.products(X, W.t())[1], (hi + lo)[:, pi])                                        # D places (hi + lo)(x[i, pi(j)]) at [i, j]
    A, B = G.family_wgrad("rows", 64, 256, 128)
    assert A.shape == (64, 256) and B.shape == (64, 128)
    assert float(A[0].abs().max()) < 1e-4 * float(A[-1].abs().max())                                     # the scales run along m


@pytest.mark.parametrize("kind", G.FAMILIES)
def test_designed_value_bounds(kind, designed):
    """|D - ref| <= 3 2^-16 (1 + 2^-7) A elementwise (provable), and <= 0.6 x 2e-5 max|ref| (0.4 of the contract stays for the kernels) --
    not for ``cancel``, whose ref is rounding noise"""
    for K in KS:
        X, W, ref, D, A = designed[kind, K]
        err = (D - ref).abs()
        assert bool((err <= G.DESIGNED * A).all()), f"{kind} K={K}: {G.ratio(err, G.DESIGNED * A):.3f} of the provable bound"
        if kind != "cancel":
            S = float(ref.abs().max())
            assert float(err.max()) <= G.DESIGNED_SHARE * G.RULE2 * S, f"{kind} K={K}: {float(err.max()) / (G.RULE2 * S):.3f} of 2e-5 S"


def test_batch_index_formula_is_exact_below_2_22():
    """(int)((float(row) + 0.5f) (1 / T)) == row // T at the rows b T - 1 and b T (where the quotient changes) for every T <= 8192 and every row
    < 2^22: the M <= 1 << 22 limit of check_head"""
    limit = 1 << 22
    for T in range(1, 8193):
        b = np.arange(1, (limit - 1) // T + 1, dtype=np.int64)
        rows = np.concatenate([b * T - 1, b * T])
        rows = rows[rows < limit]
        got = G.batch_index(rows, T)
        if not np.array_equal(got, rows // T):
            bad = rows[got != rows // T][0]
            raise AssertionError(f"T={T} row={bad}: {G.batch_index(np.array([bad]), T)[0]} != {bad // T}")


def test_batch_index_formula_fails_beyond_the_limit():
    """the limit is not slack: an odd T has a row below 2^25 where the fp32 formula is off by one"""
    rows = np.arange(1 << 24, 1 << 25, dtype=np.int64)
    assert not np.array_equal(G.batch_index(rows, 7), rows // 7)


PLAN_256 = [   # (M, N) -> (tm, branch, rounds, tail) with 256 CUs
    ((64, 256), (64, "B", 1, 1)),
    ((256, 256), (64, "B", 1, 4)),
    ((256, 512), (64, "B", 1, 8)),
    ((4160, 1024), (64, "B", 2, 4)),
    ((4224, 1024), (128, "B", 1, 4)),
    ((8192, 1024), (128, "A", 1, 0)),
    ((12288, 2048), (128, "A", 3, 0)),
    ((8448, 1024), (256, "B", 1, 4)),
    ((16384, 1024), (256, "A", 1, 0)),
    ((16384, 2048), (256, "A", 2, 0)),
    ((2560, 1024), (64, "B", 1, 0)),
    ((16384, 512), (128, "B", 1, 0)),
]


@pytest.mark.parametrize("shape,want", PLAN_256)
def test_plan_for_256_cus(shape, want):
    p = G.plan(*shape, 256)
    assert (p["tm"], p["branch"], p["rounds"], p["tail"]) == want


def test_plan_with_a_fixed_row_tile():
    """tsg_gemm_f32s_nn always runs 256-row tiles"""
    p = G.plan(16640, 1024, 256, tm=256)
    assert (p["tiles"], p["branch"], p["rounds"], p["tail"]) == (260, "B", 2, 4)
    p = G.plan(16384, 1024, 256, tm=256)
    assert (p["tiles"], p["branch"], p["rounds"]) == (256, "A", 1)


def test_head_reference_against_plain_formulas():
    g = torch.Generator().manual_seed(1)
    M, H, T = 40, 8, 20
    D = torch.randn(M, H, generator=g).double(); A = D.abs() + 1.0
    cs, b1, w2, b2 = G.head_extras(M // T, H, 1)
    rows = cs[torch.arange(M) // T]
    gate = torch.randn(M, generator=g)
    logit, bound = G.head_logits(D, A, rows, b1, w2, float(b2[0]), gate, "tanh")
    want = (torch.tanh(gate.double()[:, None] * (D + rows.double()) + b1.double()) * w2.double()).sum(1) + float(b2[0])
    assert torch.allclose(logit, want, rtol=0, atol=1e-14) and bool((bound > 0).all())
    mask = (torch.arange(T)[None, :] < torch.tensor([[12], [20]])).int().reshape(-1)
    p, pb = G.head_probs(logit, bound, mask, T)
    assert float(p[0, 12:].abs().max()) == 0.0 and torch.allclose(p.sum(1), torch.ones(2, dtype=torch.float64))
    assert bool((pb >= G.FLOOR).all())

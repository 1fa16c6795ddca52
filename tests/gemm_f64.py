"""float64 ground truth for the f32s GEMMs (plain helper module of tests/test_gemm_f64_cpu.py and tests/test_gemm_f64_gpu.py).

csrc/gemm_f32s.hip and csrc/wgrad_split.hip split every fp32 operand element x into hi = rne_bf16(x), lo = rne_bf16(x - hi) and accumulate
hi hi' + hi lo' + lo hi' in fp32 on the bf16 MFMA.  For a product L [m,k] R [k,n] (``products``; on whatever device the operands are):
  ref  the float64 product of the fp32 operands;
  D    the DESIGNED value: the three plane products, each exact, summed in float64 -- what the kernels document, without their fp32 accumulation;
  A    |L| |R| in float64, the per-element scale.
Two rules hold a kernel's result Y:
  1.  |Y - D| <= 64 2^-24 A for every element (``rule1``): fp32 accumulation separates the kernel from D and nothing else; 64 2^-24 is the
      project's fp32 floor.  An addend that joins the sum in fp32 (a bias, the head's cs and b1) joins D and, by magnitude, A.
  2.  max|Y - ref| <= 2e-5 max|ref| (``RULE2``), the published f32s contract -- not for ``cancel``, whose ref is rounding noise.
The designed value itself is within 3 2^-16 (1 + 2^-7) A of ref (x = hi + lo + r, |lo| <= 2^-9 |x| (1 + 2^-8), |r| <= 2^-9 |lo|; the product
drops lo lo' and the two r terms), and uses at most 0.6 of rule 2 on every family here (tests/test_gemm_f64_cpu.py).

``family`` builds the operand sets from a seeded CPU generator; non-zero magnitudes stay within [1e-18, 1e18], so that lo never reaches the
bf16 subnormals and no product overflows.  ``plan`` restates the tile plan of csrc/gemm_f32s.hip (pick_tm, the placement test, the persistent
walk, xcd_remap's ragged tail); ``batch_index`` the fp32 row -> batch item formula of the head epilogues."""
import functools

import numpy as np
import torch

BF = torch.bfloat16
FLOOR = 64.0 * 2.0 ** -24          # rule 1, x A
RULE2 = 2e-5                       # rule 2, x max|ref|
LIB_OK = 16.0 * 2.0 ** -24         # the library's own fp32 product above this (x A) grants 4 x its error to the case
DESIGNED = 3.0 * 2.0 ** -16 * (1.0 + 2.0 ** -7)      # |D - ref| <= DESIGNED x A, provable
DESIGNED_SHARE = 0.6               # |D - ref| <= DESIGNED_SHARE x RULE2 x max|ref|: 0.4 of the contract is left to the kernels
FAMILIES = ("randn", "rows", "kscale", "kspike", "ones", "lomax", "lomax_neg", "cancel", "big", "tiny", "zeros", "perm")
LARGE = ("randn", "ones", "lomax", "rows", "perm")                      # the sweep of the large shapes
HEAD_FAMILIES = ("randn", "rows", "ones", "lomax")
WGRAD_FAMILIES = ("randn", "rows", "ones", "lomax", "cancel", "zeros")
MAG_LO, MAG_HI = 1e-18, 1e18


def perm_of(N, K):
    """pi(j) of the ``perm`` family: a bijection of [0, K) for K a multiple of 32 (gcd(5, K) = 1), not an involution (pi(pi(j)) = 25 j + 18)"""
    return (5 * torch.arange(N) + 3) % K


def _lomax(g, rows, cols):
    m = 1.0 + torch.randint(0, 128, (rows, cols), generator=g).double() / 128.0           # the bf16 grid in [1, 2)
    e = torch.randint(-3, 4, (rows, cols), generator=g).double()
    return ((m + 0.499 * 2.0 ** -8) * 2.0 ** e).float()                                     # lo just below half an ulp of hi, positive


def family(kind, M, N, K, seed=0):
    """(X [M,K], W [N,K]) of one operand family, fp32 on the CPU: Y = X W^T contracts the columns of both"""
    g = torch.Generator().manual_seed(seed + 7919 * FAMILIES.index(kind))
    rn = lambda *s: torch.randn(*s, generator=g)
    if kind == "lomax" or kind == "lomax_neg":
        X, W = _lomax(g, M, K), _lomax(g, N, K)
        if kind == "lomax_neg":
            W = -W
    elif kind == "ones":
        X, W = 1.0 + 1e-3 * rn(M, K), 1.0 + 1e-3 * rn(N, K)
    elif kind == "cancel":
        a, b = rn(M, K // 2), rn(N, K // 2)
        X, W = 1e3 * torch.cat([a, -a], 1), torch.cat([b, b], 1)
    elif kind == "perm":
        X = rn(M, K) * torch.logspace(-3, 3, K)[None, :]
        W = torch.zeros(N, K)
        W[torch.arange(N), perm_of(N, K)] = 1.0
    else:
        X, W = rn(M, K), rn(N, K) / K ** 0.5
        if kind == "randn":
            pass
        elif kind == "rows":
            X = X * torch.logspace(-6, 3, M)[:, None]; W = W * torch.logspace(3, -6, N)[:, None]
        elif kind == "kscale":
            s = torch.logspace(-4, 4, K)
            X = X * s[None, :]; W = W / s[None, :]
        elif kind == "kspike":
            X = X * torch.logspace(0, 6, K)[None, :]; W = W * K ** 0.5
        elif kind == "big":
            X = X * 1e15; W = W * K ** 0.5 * 1e15
        elif kind == "tiny":
            X = X * 1e-15; W = W * K ** 0.5 * 1e-15
        elif kind == "zeros":
            X[::3] = 0.0; W[:, ::2] = 0.0
        else:
            raise ValueError(kind)
    return _in_range(X.float()).contiguous(), _in_range(W.float()).contiguous()


def _in_range(t):
    """non-zero magnitudes into [MAG_LO, MAG_HI], signs and zeros kept"""
    return torch.where(t == 0, t, torch.sign(t) * t.abs().clamp(MAG_LO, MAG_HI))


def family_wgrad(kind, M, N, K, seed=0):
    """(A [M,N], B [M,K]) for C = A^T B: the same families with the contraction along the rows (``rows``: the scales run along m)"""
    if kind == "rows":
        g = torch.Generator().manual_seed(seed + 31)
        A = torch.randn(M, N, generator=g) * torch.logspace(-6, 3, M)[:, None]
        B = torch.randn(M, K, generator=g) / M ** 0.5 * torch.logspace(3, -6, M)[:, None]
        return _in_range(A).contiguous(), _in_range(B).contiguous()
    X, W = family(kind, N, K, M, seed)
    return X.t().contiguous(), W.t().contiguous()


def split(x):
    """(hi, lo) of fp32 x, as float64: hi = rne_bf16(x), lo = rne_bf16(x - hi), with torch's own bfloat16 conversion (x - hi is exact in fp32)"""
    x = x.float()
    hi = x.to(BF).float()
    return hi.double(), (x - hi).to(BF).double()


def products(L, R):
    """L [m,k], R [k,n] fp32 (any device) -> (ref, D, A), float64 [m,n]"""
    Lh, Ll = split(L); Rh, Rl = split(R)
    ref = L.double() @ R.double()
    D = Lh @ Rh + Lh @ Rl + Ll @ Rh
    A = L.double().abs() @ R.double().abs()
    return ref, D, A


def rule1(A):
    return FLOOR * A


def ratio(err, bound):
    """largest err / bound; an element with bound 0 must have err 0 (a zero row times anything is exactly zero)"""
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max())


# ---- the tile plan of csrc/gemm_f32s.hip -------------------------------------------------------------------------------------------------
def pick_tm(M, N, cus):
    best, best_cost = 0, np.float32(0)
    for tm in (256, 128, 64):
        if M % tm:
            continue
        tiles = (M // tm) * (N // 256)
        cost = np.float32((tiles + cus - 1) // cus) * (np.float32(17.0) + np.float32(0.22) * np.float32(tm))
        if not best or cost < best_cost:
            best, best_cost = tm, cost
    return best


def plan(M, N, cus, tm=None):
    """-> dict(tm, tiles, branch 'A' (8 x 4 neighbour tiles per XCD) / 'B' (the N tiles of an M tile per XCD), rounds of the persistent walk,
    tail = tiles xcd_remap leaves in natural order); tm: a kernel with a fixed row tile (tsg_gemm_f32s_nn: 256)"""
    tm = tm or pick_tm(M, N, cus)
    tiles_n = N // 256
    m_tiles = M // tm
    tiles = m_tiles * tiles_n
    a = tiles_n % 4 == 0 and m_tiles % 8 == 0 and tiles % 256 == 0
    group = 32 if a else tiles_n
    return dict(tm=tm, tiles=tiles, branch="A" if a else "B", rounds=-(-tiles // min(tiles, cus)), tail=tiles - tiles // (8 * group) * (8 * group))


def batch_index(rows, T):
    """(int)(((float)row + 0.5f) * (1.f / (float)T)) of the head epilogues, in numpy float32"""
    inv = np.float32(1.0) / np.float32(T)
    return ((rows.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int32)


# ---- the heads ------------------------------------------------------------------------------------------------------------------------------
ACTS = ("relu", "tanh", "sigmoid")
LIPSCHITZ = {"relu": 1.0, "tanh": 1.0, "sigmoid": 0.25}


def act64(name, z):
    return torch.relu(z) if name == "relu" else torch.tanh(z) if name == "tanh" else torch.sigmoid(z)


def head_extras(Bn, N, heads, seed=0):
    """cs [Bn,N] (+-30 in a tenth of the columns: saturated activations), b1 [N], w2 [N] of mixed magnitudes, b2 [heads]; fp32, CPU"""
    g = torch.Generator().manual_seed(seed + 555)
    cs = torch.randn(Bn, N, generator=g)
    sat = torch.arange(N) % 10 == 3
    cs[:, sat] = torch.where(torch.randn(Bn, int(sat.sum()), generator=g) > 0, 30.0, -30.0)
    b1 = 0.1 * torch.randn(N, generator=g)
    w2 = torch.randn(N, generator=g) / N ** 0.5 * 10.0 ** torch.randint(-3, 2, (N,), generator=g).float()
    b2 = torch.randn(heads, generator=g)
    return cs.contiguous(), b1, w2, b2


def head_logits(D, A, cs_rows, b1, w2, b2, gate, act):
    """The head's formula (include/tsg_hip.h) on the designed pre-activation, and its bound, per row of one head.
    D, A [M,H] float64; cs_rows [M,H] (cs of the row's item); b1, w2 [H]; b2 a float; gate [M] or None (1).
        z = g (D + cs) + b1            logit = sum_c w2_c act(z_c) + b2
    bound = sum_c |w2_c| L 64 2^-24 (|g| (A_c + |cs_c|) + |b1_c|)         rule 1 on the pre-activation (cs and b1 join its sum in fp32), through the
                                                                          activation's Lipschitz constant L (1; sigmoid 1/4)
          + sum_c 64 2^-24 |w2_c|                                         the fast tanh / sigmoid (absolute error); not for relu
          + 64 2^-24 (sum_c |w2_c act_c| + |b2|)                          the fp32 reduction
    -> (logit [M], bound [M]) float64"""
    g = gate.double()[:, None] if gate is not None else 1.0
    ga = gate.double().abs()[:, None] if gate is not None else 1.0
    cs_rows, b1, w2 = cs_rows.double(), b1.double(), w2.double()
    a = act64(act, g * (D + cs_rows) + b1)
    logit = (a * w2).sum(1) + b2
    bound = (w2.abs() * LIPSCHITZ[act] * FLOOR * (ga * (A + cs_rows.abs()) + b1.abs())).sum(1)
    if act != "relu":
        bound = bound + FLOOR * w2.abs().sum()
    bound = bound + FLOOR * ((a * w2).abs().sum(1) + abs(b2))
    return logit, bound


def head_probs(logit, bound, mask, T):
    """softmax over T of mask_logits(logit) per item, and its bound p (exp(2 delta) - 1) + 64 2^-24, delta = the largest logit bound among the
    item's unmasked rows (a shift of every logit by at most delta moves a probability by at most that factor).  -> (p [Bn,T], bound [Bn,T])"""
    l = logit.view(-1, T); d = bound.view(-1, T)
    if mask is not None:
        keep = mask.view(-1, T).bool()
        l = torch.where(keep, l, torch.full_like(l, -float("inf"))); d = torch.where(keep, d, torch.zeros_like(d))
    p = torch.softmax(l, 1)
    delta = d.max(1, keepdim=True).values
    return p, (p * torch.expm1(2.0 * delta)).clamp(max=1.0) + FLOOR


# ---- truths, computed once and shared (read-only) ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)            # (a [16384, 2048] entry holds 0.8 GB on the device; the cases that share one follow each other)
def truth(kind, M, N, K, device="cpu", seed=0):
    """-> dict X [M,K], W [N,K] (fp32), ref, D, A (float64 [M,N]) of Y = X W^T on ``device``"""
    X, W = family(kind, M, N, K, seed)
    X, W = X.to(device), W.to(device)
    ref, D, A = products(X, W.t())
    return dict(X=X, W=W, ref=ref, D=D, A=A)

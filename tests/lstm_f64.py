"""float64 ground truth for the BiLSTM recurrence (plain helper module of tests/test_lstm_f64_cpu.py and tests/test_lstm_f64_gpu.py).

``reference`` is the recurrence of csrc/lstm.hip on pre-computed input gates -- z_t = Gx_t + h_(t-1) W_hh^T, (i, f, o) = sigmoid, g = tanh,
c_t = f c_(t-1) + i g, h_t = o tanh(c_t), both directions, zero initial state -- on the CPU with autograd, in float64 (the truth) or in float32
(``E32``: the same formula in the kernels' own precision, the yardstick of the bound).  ``dHn`` enters as the gradient of the LAST hidden state of
each direction: h at t = T-1 for the forward direction, h at t = 0 for the reverse one.  ``family`` builds the operand sets, from unit scale up
to saturated gates and cell states of about T; ``beyond`` is outside any contract (finite, nothing more).  ``emulate_split`` and
``emulate_bf16`` restate in float64 the roundings the f32s arithmetic and the bf16 storage make by design: what they lose is the part of a
bound that the design itself uses up."""
import functools

import torch

BF = torch.bfloat16
FLOOR = 64.0 * 2.0 ** -24          # x max(1, max|want|): the floor of the bound
MARGIN = 16.0                      # x E32
FAMILIES = ("unit", "small", "scale4", "w2", "saturated", "remember", "forget", "zero_w")      # in contract
ALL_FAMILIES = FAMILIES + ("beyond",)
SHORT = ("unit", "scale4", "remember")                                                         # the sweep of the shapes beyond h = 128
TENSORS = ("out", "R", "Cs", "dG", "dbias")


def family(kind, B, T, h, seed=0):
    """(Gx [T,B,2,4h], W [2,4h,h]) of one operand family, fp32; gate order i, f, g, o."""
    g = torch.Generator().manual_seed(seed)
    Gx = torch.randn(T, B, 2, 4 * h, generator=g) * 0.5
    W = torch.randn(2, 4 * h, h, generator=g) / h ** 0.5
    gates = Gx.view(T, B, 2, 4, h)
    if kind == "unit":
        pass
    elif kind == "small":                        # gates at 0.5, tanh arguments near 1e-3: the cancellation in 1 - 2 / (e^2x + 1)
        Gx *= 2e-3
    elif kind == "scale4":                       # mixed saturation
        Gx *= 8.0
    elif kind == "w2":                           # stronger recurrence
        W *= 2.0
    elif kind == "saturated":                    # pre-activations to +-150: exp2 overflows in sigmoid_f, tanh_f clamps at +-44
        Gx *= 60.0
    elif kind == "remember":                     # i = f = 1, g > 0.96: c grows by about 1 per step
        gates[..., 0, :] += 15.0; gates[..., 1, :] += 15.0
        gates[..., 2, :] = 4.0 * gates[..., 2, :].abs() + 2.0
    elif kind == "forget":                       # f = 0: c_t = i g only
        gates[..., 1, :] -= 30.0
    elif kind == "zero_w":                       # pure elementwise: pins the gate order and the direction layout
        W.zero_()
    elif kind == "beyond":                       # out of contract
        Gx *= 200.0
    else:
        raise ValueError(kind)
    return Gx.contiguous(), W.contiguous()


def extras(B, T, h, seed=0):
    """(dOut [T,B,2h], dHn [2,B,h]): the gradients of the output and of each direction's last hidden state."""
    g = torch.Generator().manual_seed(seed + 1000)
    return torch.randn(T, B, 2 * h, generator=g), torch.randn(2, B, h, generator=g)


def bf16_valued(t):
    return t.to(BF).float()


def _times(T, d):
    return range(T) if d == 0 else range(T - 1, -1, -1)


def forward(Gx, W, dtype=torch.float64, mm=None, sigmoid=torch.sigmoid, tanh=torch.tanh, feed=None):
    """The recurrence with a graph: -> dict Gx (the leaf), out [T,B,2h], Z (pre-activations) and R (activated gates) [T,2,B,h,4], Cs [T,2,B,h],
    hn, cn [2,B,h].  mm(h_prev [B,h], W_d [4h,h], d) replaces the recurrent product, feed(h) the value fed back (and written to out)."""
    Gx = Gx.detach().to(dtype).clone().requires_grad_(True)
    W = W.detach().to(dtype)
    T, B, _, h4 = Gx.shape
    h = h4 // 4
    outs, Zs, Rs, Cs, hn, cn = [], [], [], [], [], []
    for d in range(2):
        Wt = W[d].t().contiguous()
        hp = torch.zeros(B, h, dtype=dtype); c = torch.zeros(B, h, dtype=dtype)
        o_t, z_t, r_t, c_t = [None] * T, [None] * T, [None] * T, [None] * T
        gx = Gx[:, :, d].unbind(0)               # (one stack in the backward instead of a [T,B,2,4h] scatter per step)
        for t in _times(T, d):
            z = gx[t] + (mm(hp, W[d], d) if mm is not None else hp @ Wt)
            zi, zf, zg, zo = z.split(h, 1)
            gi, gf, gg, go = sigmoid(zi), sigmoid(zf), tanh(zg), sigmoid(zo)
            c = gf * c + gi * gg
            hp = go * tanh(c)
            if feed is not None:
                hp = feed(hp)
            o_t[t], c_t[t] = hp, c
            z_t[t] = torch.stack((zi, zf, zg, zo), -1); r_t[t] = torch.stack((gi, gf, gg, go), -1)
        outs.append(torch.stack(o_t)); Zs.append(torch.stack(z_t)); Rs.append(torch.stack(r_t)); Cs.append(torch.stack(c_t))
        hn.append(hp); cn.append(c)
    return dict(Gx=Gx, out=torch.cat(outs, -1), Z=torch.stack(Zs, 1).detach(), R=torch.stack(Rs, 1).detach(), Cs=torch.stack(Cs, 1).detach(),
                hn=torch.stack(hn), cn=torch.stack(cn).detach())


def gate_gradients(fw, dOut, dHn=None, retain=False):
    """-> (dG [T,B,2,4h] = d loss / d Gx, dbias [2,4h] = dG.sum((0, 1))) of loss = <out, dOut> + <hn, dHn>, by autograd on ``forward``'s graph."""
    dtype = fw["out"].dtype
    loss = (fw["out"] * dOut.to(dtype)).sum()
    if dHn is not None:
        loss = loss + (fw["hn"] * dHn.to(dtype)).sum()
    dG, = torch.autograd.grad(loss, fw["Gx"], retain_graph=retain)
    return dG, dG.sum((0, 1))


def reference(Gx, W, dOut, dHn=None, dtype=torch.float64, **kw):
    """The recurrence and its gate gradients in ``dtype`` on the CPU.  -> dict: out, R, Cs, dG, dbias (and Z, hn, cn)."""
    fw = forward(Gx, W, dtype, **kw)
    dG, db = gate_gradients(fw, dOut, dHn)
    res = {k: fw[k].detach() for k in ("out", "Z", "R", "Cs", "hn", "cn")}
    res["dG"], res["dbias"] = dG, db
    return res


def backward_from_saved(W, R, Cs, dOut, dHn=None, tanh=torch.tanh, mm=None, stored=None):
    """The backward as the kernels run it: from the saved gates R and cell states Cs, the last forward step first,
    dh_t = dOut_t (+ dHn at the direction's last step) + dG_(t+1) W_hh, written out by hand (no autograd).  mm(dG [B,4h], W_d [4h,h], d)
    replaces the recurrent product; stored(dG_t) is the value written -- and multiplied in the next step --, dbias sums the unrounded one.
    -> (dG [T,B,2,4h], dbias [2,4h])"""
    T, _, B, h = Cs.shape
    dtype = Cs.dtype
    W, dOut = W.to(dtype), dOut.to(dtype)
    dG = torch.zeros(T, B, 2, 4 * h, dtype=dtype); db = torch.zeros(2, 4 * h, dtype=dtype)
    for d in range(2):
        order = list(_times(T, d))[::-1]
        dc_carry = torch.zeros(B, h, dtype=dtype)
        prev = None
        for n, t in enumerate(order):
            gi, gf, gg, go = R[t, d].unbind(-1)
            cp = Cs[order[n + 1], d] if n + 1 < T else torch.zeros(B, h, dtype=dtype)
            dh = dOut[t, :, d * h:(d + 1) * h].clone()
            if n == 0:
                if dHn is not None:
                    dh = dh + dHn[d].to(dtype)
            else:
                dh = dh + (mm(prev, W[d], d) if mm is not None else prev @ W[d])
            tc = tanh(Cs[t, d])
            dc = dh * go * (1.0 - tc * tc) + dc_carry
            dc_carry = dc * gf
            dg = torch.cat((dc * gg * gi * (1.0 - gi), dc * cp * gf * (1.0 - gf), dc * gi * (1.0 - gg * gg), dh * tc * go * (1.0 - go)), 1)
            db[d] += dg.sum(0)
            prev = stored(dg) if stored is not None else dg
            dG[t, :, d] = prev
    return dG, db


def rule(e32, S):
    """The bound on a quantity the kernels compute in fp32 arithmetic: elementwise |got - float64| <= max(16 E32, 64 2^-24 max(1, S)), E32 = max
    error of the float32 run of ``reference`` on that tensor, S = max|want|.  16, as in scdm_f64.rule: the kernels form an activation with
    three roundings and two 1-ulp hardware approximations (v_exp_f32, v_rcp_f32) where torch rounds one correctly rounded call, ~4x per term; the
    MFMA summation order adds no more than that again; 4x of headroom.  The floor uses max(1, S), not S: tanh_f = 1 - 2 rcp(e + 1) has an absolute
    error of an ulp of 1, not of its result, so a tensor of small values (the ``small`` family) is not held to an ulp of itself."""
    return max(MARGIN * e32, FLOOR * max(1.0, S))


def bound_fp32(e32, want):
    """``rule`` as an elementwise tensor, never looser than TOL of tests/test_lstm_gpu.py (atol = rtol = 1e-4)"""
    want = want.double()
    return (1e-4 + 1e-4 * want.abs()).clamp(max=rule(e32, float(want.abs().max())))


def bound_close(want, rel):
    """``_close`` of tests/test_bf16_storage_gpu.py as an elementwise tensor: rel max(1, S) + rel |want|"""
    want = want.double()
    return rel * max(1.0, float(want.abs().max())) + rel * want.abs()


# ---- the roundings the two reduced-precision modes make by design, in float64 --------------------------------------------------------------
def _bf_round(x):
    return x.float().to(BF).to(x.dtype)


def _split(x):
    x32 = x.float()
    hi = x32.to(BF).float()
    return hi.to(x.dtype), (x32 - hi).to(BF).to(x.dtype)


def _split_prod(a, bh, bl):
    ah, al = _split(a)
    return ah @ bh + ah @ bl + al @ bh


class _SplitMM(torch.autograd.Function):
    """h W_hh^T forward, dG W_hh backward, each as hi hi + hi lo + lo hi of bf16 halves (exact products, float64 sums); Wh, Wl: the halves of W_d"""

    @staticmethod
    def forward(ctx, x, Wh, Wl):
        ctx.save_for_backward(Wh, Wl)
        return _split_prod(x, Wh.t(), Wl.t())

    @staticmethod
    def backward(ctx, dz):
        Wh, Wl = ctx.saved_tensors
        return _split_prod(dz, Wh, Wl), None, None


def emulate_split(Gx, W, dOut, dHn=None):
    """float64 recurrence with every h W_hh and dG W_hh product evaluated as the f32s kernels do.  -> dict like ``reference``"""
    halves = [_split(Wd) for Wd in W.double()]                        # W_hh is split once (the kernels: in the prologue)

    def mm(x, Wd, d):
        return _SplitMM.apply(x, *halves[d])
    return reference(Gx, W, dOut, dHn, torch.float64, mm=mm)


def emulate_bf16(Gx, W, dOut, dHn=None):
    """float64 recurrence with the roundings of the bf16 storage mode (include/tsg_hip.h, tsg_lstm_fwd): W_hh rounded once, h_t fed back as
    the bf16 value stored to out, R rounded where stored (the backward reads that), dG rounded where stored (the next step multiplies that);
    the caller passes bf16-valued Gx and dOut.  Cs, dHn and dbias stay unrounded.  -> dict like ``reference``"""
    Wb = _bf_round(W.double())
    with torch.no_grad():
        fw = forward(Gx, Wb, torch.float64, feed=_bf_round)
    R = _bf_round(fw["R"])
    dG, db = backward_from_saved(Wb, R, fw["Cs"], dOut, dHn, stored=_bf_round)
    return dict(out=fw["out"].detach(), R=R, Cs=fw["Cs"], dG=dG, dbias=db)


def _err(a, b):
    return float((a.double() - b).abs().max())


@functools.lru_cache(maxsize=4)            # (a [20,128,512] entry holds 0.4 GB; the cases that share one follow each other)
def truth(kind, B, T, h, bf=False, seed=0):
    """Operands, the float64 result and E32 per tensor, computed once per (family, shape, storage) and shared by every test that needs them
    (read-only).  The gate gradients come twice: dG / dbias without dHn, dG_hn / dbias_hn with it.  bf: Gx, W, dOut and dHn hold bf16 values, and
    ``ebf`` has the error of ``emulate_bf16`` against float64 per tensor.
    -> (ins dict of fp32 CPU tensors, want dict of float64 tensors, e32 dict of floats, ebf dict of floats or None)"""
    Gx, W = family(kind, B, T, h, seed)
    dOut, dHn = extras(B, T, h, seed)
    if bf:
        Gx, W, dOut, dHn = (bf16_valued(x) for x in (Gx, W, dOut, dHn))
    res = []
    for dtype in (torch.float64, torch.float32):
        fw = forward(Gx, W, dtype)
        r = {k: fw[k].detach() for k in ("out", "R", "Cs", "Z")}
        r["dG"], r["dbias"] = gate_gradients(fw, dOut, None, retain=True)
        r["dG_hn"], r["dbias_hn"] = gate_gradients(fw, dOut, dHn)
        res.append(r)
    want, f32 = res
    e32 = {k: _err(f32[k], want[k]) for k in want if k != "Z"}
    ebf = None
    if bf:
        a, b = emulate_bf16(Gx, W, dOut, None), emulate_bf16(Gx, W, dOut, dHn)
        ebf = {k: _err(a[k], want[k]) for k in TENSORS}
        ebf.update(dG_hn=_err(b["dG"], want["dG_hn"]), dbias_hn=_err(b["dbias"], want["dbias_hn"]))
    return dict(Gx=Gx, W=W, dOut=dOut, dHn=dHn), want, e32, ebf

"""The row-wise checker has power (no GPU).  (a) A plain torch fp32 emulation of each kernel's documented chain, summed in a
different order from the kernel (torch's own reduction over the columns reversed), passes tests/rowwise_check.py with the final c
of every path.  (b) Each of the usual ways such a kernel goes wrong, applied to that emulation, is flagged -- by the per-element
bound, by an exact check, by the count, or by the guard bands.  (c) The case lists of tests/test_rowwise_contract_gpu.py cover
the launch variants: every norm_ch, both loop bodies of reduce_partials, both arg-max kernels.  The MoE expert fusion
(mm_expert_fuse, forward and backward = 1) has its emulation and its six planted mistakes in a section of its own."""
import pytest
import torch

from tests import gemm_check as GC
from tests import rowwise_check as RC
from tests import test_rowwise_contract_gpu as GPU
from tests.kernel_check import check_bits
from tests.rowwise_check import BF, F32, U32

DTYPES = [BF, F32]
ids = lambda d: RC.NAME[d]
M, H = 40, 136                      # three 16-row blocks (the last one ragged), 17 bf16 vectors per row


def rsum(t, dim=-1):
    """fp32 sum in an order of its own: the columns reversed, then torch's pairwise reduction."""
    return t.flip(dim).sum(dim)


# ---- emulations (mut names a deliberate mistake) ---------------------------------------------------------------------------------
def rms_fwd(x, w, eps, mut=None):
    T, xf = x.dtype, x.float()
    Hn = xf.shape[1]
    den = (Hn + 2047) // 2048 * 2048 if mut == "rstd_padded_H" else Hn
    rstd = torch.rsqrt(rsum(xf * xf) / den + eps)
    n = xf * rstd[:, None]
    if mut != "no_mid_round":
        n = n.to(T).float()
    y = (w.float()[None, :] * n).to(T)
    if mut == "zero_vector":
        y[3, 8:16] = 0
    if mut == "swap_rows":
        y[[16, 17]] = y[[17, 16]]
    return y, rstd


def rms_bwd(dy, x, w, rstd, dres, mut=None):
    g, xf, wf, rs = dy.float(), x.float(), w.float()[None, :], rstd[:, None]
    xh = xf * rs
    dot = rsum(g * wf * xh)[:, None] / xf.shape[1]
    dx = rs * (g * wf - xh * dot) + (dres.float() if dres is not None else 0.0)
    return dx.to(x.dtype), blocks(g * xh)


def blocks(t, mut=None):
    """the [nblk, H] partials of a per-row term: 16 rows per block, added in sequence."""
    Mm = t.shape[0]
    out = []
    for r0 in range(0, Mm, 16):
        r1 = min(Mm, r0 + 16)
        if mut == "drop_block_last_row" and r1 - r0 == 16 and r0 == 16:
            r1 -= 1
        out.append(t[r0:r1].flip(0).sum(0))
    return torch.stack(out)


def reduce(p, dtype, before=None, mut=None):
    s = p.flip(0).sum(0)
    if mut == "block_twice":
        s = s + p[p.shape[0] // 2]
    if before is not None:
        s = s + before.float()
    return s.to(dtype)


def ln_fwd(x, w, b, eps):
    xf = x.float()
    mu = rsum(xf) / xf.shape[1]
    xc = xf - mu[:, None]
    rstd = torch.rsqrt(rsum(xc * xc) / xf.shape[1] + eps)
    return (xc * rstd[:, None] * w.float()[None, :] + b.float()[None, :]).to(x.dtype), mu, rstd


def ln_bwd(dy, x, w, mean, rstd, dres, mut=None):
    g, wf, rs = dy.float(), w.float()[None, :], rstd[:, None]
    xh = (x.float() - mean[:, None]) * rs
    gw = g * wf
    s1, s2 = rsum(gw)[:, None] / x.shape[1], rsum(gw * xh)[:, None] / x.shape[1]
    dx = rs * (gw - s1 - xh * s2) + (dres.float() if dres is not None else 0.0)
    return dx.to(x.dtype), blocks(g * xh), blocks(g, mut)


def rope(x, cos, sin, nheads, D, inverse=False, mut=None):
    T, xf = x.dtype, x.float().clone()
    s = sin if (inverse and mut == "inverse_sign") or not inverse else -sin
    h = xf[:, : nheads * D].reshape(x.shape[0], nheads, D)
    lo, hi = h[..., : D // 2].clone(), h[..., D // 2:].clone()
    c, s = cos[:, None, :], s[:, None, :]
    xf[:, : nheads * D] = torch.cat([lo * c - hi * s, hi * c + lo * s], -1).reshape(x.shape[0], nheads * D)
    return xf.to(T)


def swiglu_fwd(gu, I, mut=None):
    g, u = gu[:, :I].float(), gu[:, I:].float()
    s = g * torch.sigmoid(g)
    if mut != "no_mid_round":
        s = s.to(gu.dtype).float()
    return (s * u).to(gu.dtype)


def swiglu_bwd(gu, dout, I):
    g, u, d = gu[:, :I].float(), gu[:, I:].float(), dout.float()
    sig = torch.sigmoid(g)
    return torch.cat([d * u * (sig * (1 + g * (1 - sig))), d * g * sig], 1).to(gu.dtype)


def gelu(x, kind, dy=None):
    xf = x.float().clone().requires_grad_(dy is not None)
    y = GC.act64(xf, RC.GELU_KINDS[kind])
    if dy is None:
        return y.detach().to(x.dtype)
    y.backward(dy.float())
    return xf.grad.to(x.dtype)


def ce(x, labels, ld, gscale=None, mut=None):
    T, V = x.shape
    xf = x.float()
    mx = xf.max(-1).values
    lse = mx + torch.log(rsum(torch.exp(xf - mx[:, None])))
    live = (labels >= 0) & (labels < V)
    lab = labels.clamp(0, V - 1)
    row = torch.where(live, lse - xf.gather(1, lab[:, None])[:, 0], torch.zeros_like(lse))
    count = float(T if mut == "count_ignored" else (labels >= 0).sum())
    lc = torch.tensor([float(rsum(row)) / max(count, 1.0), count])
    onehot = torch.zeros_like(xf)
    onehot.scatter_(1, ((lab + 1) % V if mut == "label_off_by_one" else lab)[:, None], 1.0)
    scale = torch.where(live, (1.0 if gscale is None else gscale) / max(count, 1.0), 0.0)[:, None]
    d = torch.zeros(T, ld)
    d[:, :V] = (torch.exp(xf - lse[:, None]) - onehot) * scale
    return lse, row, lc, d.to(x.dtype)


def argmax(x, temp, last=False):
    T = x.dtype
    s = (x.float() / temp).to(T).float()
    p = torch.softmax(s, -1).to(T).float()
    hit = p == p.max(-1, keepdim=True).values
    return (x.shape[1] - 1 - hit.flip(-1).int().argmax(-1)) if last else hit.int().argmax(-1)


@pytest.fixture(autouse=True)
def _own_ratio_paths():
    """the emulation's ratios go under rowwise_emulation.<kernel>.<dtype>, apart from what the kernels measure"""
    RC.PREFIX[0] = "rowwise_emulation"
    yield
    RC.PREFIX[0] = "rowwise"


def fails(fn):
    """fn must be flagged; what a deliberate mistake measures is kept out of the ratio log"""
    saved = dict(RC.RATIOS)
    with pytest.raises(AssertionError):
        fn()
    RC.RATIOS.clear()
    RC.RATIOS.update(saved)


# ---- (a) + (b) ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_rmsnorm_emulation_passes_and_mutations_fail(dtype):
    p = RC.norm_problem(M, H, dtype, "cpu", 1)
    x, w, dy, dres = p["x"], p["w"], p["dy"], p["dres"]
    y64, Ey, r64, Er = RC.rmsnorm_fwd_reference(x, w, 1e-5)

    def check_fwd(mut):
        y, rstd = rms_fwd(x, w, 1e-5, mut)
        RC.check_exact("chain", y, RC.rmsnorm_chain(x, w, rstd))
        RC.bound("rstd", "rmsnorm.rstd", dtype, rstd, r64, Er, u=U32)
        RC.bound("y", "rmsnorm.y", dtype, y, y64, Ey)
    check_fwd(None)
    for mut in ("zero_vector", "swap_rows", "rstd_padded_H") + (("no_mid_round",) if dtype == BF else ()):
        fails(lambda: check_fwd(mut))
    # the bound alone sees the misplaced data and the wrong statistic (the exact chain is not what catches them)
    for mut in ("zero_vector", "swap_rows"):
        fails(lambda: RC.bound("y", "rmsnorm.y", dtype, rms_fwd(x, w, 1e-5, mut)[0], y64, Ey))
    fails(lambda: RC.bound("rstd", "rmsnorm.rstd", dtype, rms_fwd(x, w, 1e-5, "rstd_padded_H")[1], r64, Er, u=U32))
    _, rstd = rms_fwd(x, w, 1e-5)
    for res in (None, dres):
        dx, dwp = rms_bwd(dy, x, w, rstd, res)
        dx64, Edx, dw64, Edw = RC.rmsnorm_bwd_reference(dy, x, w, rstd, res)
        RC.bound("dx", "rmsnorm.dx", dtype, dx, dx64, Edx)
        RC.bound("dw", "rmsnorm.dw", dtype, reduce(dwp, dtype), dw64, Edw)
    fails(lambda: RC.bound("dw", "rmsnorm.dw", dtype, reduce(dwp, dtype, mut="block_twice"), dw64, Edw))
    fails(lambda: RC.bound("dx", "rmsnorm.dx", dtype, rms_bwd(dy, x, w, rstd, None)[0], dx64, Edx))      # the residual left out


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_layernorm_emulation_passes_and_mutations_fail(dtype):
    p = RC.norm_problem(M, H, dtype, "cpu", 2, layer=True)
    x, w, b, dy, dres = p["x"], p["w"], p["b"], p["dy"], p["dres"]
    y, mean, rstd = ln_fwd(x, w, b, 1e-6)
    y64, Ey, m64, Em, r64, Er = RC.layernorm_fwd_reference(x, w, b, 1e-6)
    RC.bound("mean", "layernorm.mean", dtype, mean, m64, Em, u=U32)
    RC.bound("rstd", "layernorm.rstd", dtype, rstd, r64, Er, u=U32)
    RC.bound("y", "layernorm.y", dtype, y, y64, Ey)
    fails(lambda: RC.bound("mean", "layernorm.mean", dtype, mean * (1 + 2.0 ** -14), m64, Em, u=U32))
    fails(lambda: RC.bound("y", "layernorm.y", dtype, ln_fwd(x, w, b.roll(8), 1e-6)[0], y64, Ey))       # bias of the next vector
    dx, dwp, dbp = ln_bwd(dy, x, w, mean, rstd, dres)
    dx64, Edx, dw64, Edw, db64, Edb = RC.layernorm_bwd_reference(dy, x, w, mean, rstd, dres)
    RC.bound("dx", "layernorm.dx", dtype, dx, dx64, Edx)
    RC.bound("dw", "layernorm.dw", dtype, reduce(dwp, dtype), dw64, Edw)
    RC.bound("db", "layernorm.db", dtype, reduce(dbp, dtype), db64, Edb)
    bad = ln_bwd(dy, x, w, mean, rstd, dres, "drop_block_last_row")[2]
    fails(lambda: RC.bound("db", "layernorm.db", dtype, reduce(bad, dtype), db64, Edb))
    # the exact family of db: integer dy, every sum exact, one rounding
    g = torch.Generator().manual_seed(3)
    q = torch.exp2(torch.randint(-3, 4, (H,), generator=g).double())
    dyi = (torch.randint(-8, 9, (M, H), generator=g).double() * q)
    want = RC.rne(dyi.sum(0), dtype)
    RC.check_exact("db", reduce(ln_bwd(dyi.to(dtype), x, w, mean, rstd, None)[2], dtype), want)
    fails(lambda: RC.check_exact("db", reduce(ln_bwd(dyi.to(dtype), x, w, mean, rstd, None, "drop_block_last_row")[2], dtype), want))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_reduce_partials_exact_family(dtype):
    for nblk in (0, 1, 65, 257, 1000):
        p, before, q = RC.partials_problem(nblk, 12, "cpu", nblk)
        for b in (None, before):
            want = RC.rne(RC.partials_reference(p, q, b), dtype)
            RC.check_exact("reduce", reduce(p, dtype, b), want)
            if nblk > 1:
                fails(lambda: RC.check_exact("reduce", reduce(p, dtype, b, "block_twice"), want))
                fails(lambda: RC.check_exact("reduce", reduce(p[:-1], dtype, b), want))
    with pytest.raises(AssertionError, match="out of range"):
        RC.partials_reference(torch.full((3, 4), 2.0 ** 24), torch.ones(4))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_rope_emulation_passes_and_mutations_fail(dtype):
    D, nh, T = 64, 3, 9
    pos = torch.tensor(GPU.ROPE_POS + [7, 8, 9, 10])
    inv = 1.0 / (1e4 ** (torch.arange(0, D, 2).float() / D))
    ang = pos.float()[:, None] * inv[None, :]
    for rb in (False, True):
        c64, s64, Ec, Es, u = RC.rope_table_reference(pos, inv, rb)
        cos, sin = (t.to(BF).float() if rb else t for t in (torch.cos(ang), torch.sin(ang)))
        td = BF if rb else F32
        RC.bound("cos", "rope_table", td, cos, c64, Ec, u=u)
        RC.bound("sin", "rope_table", td, sin, s64, Es, u=u)
        # the angle taken in fp64 instead of the documented fp32 product: off by |pos| u32 at position 1 000 000
        fails(lambda: RC.bound("cos", "rope_table", td, torch.cos(pos.double()[:, None] * inv.double()[None, :]).float(), c64, Ec, u=u)
              if not rb else RC.bound("cos", "rope_table", td, -cos, c64, Ec, u=u))
    x = (torch.randn(T, (nh + 1) * D, generator=torch.Generator().manual_seed(4)) * 3).to(dtype)
    for inverse in (False, True):
        ref, E = RC.rope_reference(x, cos, sin, nh, D, inverse)
        RC.bound("rope", "rope", dtype, rope(x, cos, sin, nh, D, inverse), ref, E)
    fails(lambda: RC.bound("rope", "rope", dtype, rope(x, cos, sin, nh, D, True, "inverse_sign"), ref, E))
    fails(lambda: RC.bound("rope", "rope", dtype, rope(x, cos, sin, nh + 1, D, True), ref, E))             # one head too many


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_activation_emulations_pass_and_mutations_fail(dtype):
    I, Mm = 136, 30
    g = torch.Generator().manual_seed(5)
    gu = (torch.randn(Mm, 2 * I, generator=g) * 2).to(dtype)
    dout = torch.randn(Mm, I, generator=g).to(dtype)
    ref, E = RC.swiglu_fwd_reference(gu, I)
    RC.bound("swiglu_fwd", "swiglu_fwd", dtype, swiglu_fwd(gu, I), ref, E)
    if dtype == BF:
        RC.swiglu_chain_check("chain", gu, swiglu_fwd(gu, I), I)
        fails(lambda: RC.swiglu_chain_check("chain", gu, swiglu_fwd(gu, I, "no_mid_round"), I))
    bad = swiglu_fwd(gu, I)
    bad[5, 8:16] = 0
    fails(lambda: RC.bound("swiglu_fwd", "swiglu_fwd", dtype, bad, ref, E))
    ref, E = RC.swiglu_bwd_reference(gu, dout, I)
    RC.bound("swiglu_bwd", "swiglu_bwd", dtype, swiglu_bwd(gu, dout, I), ref, E)
    fails(lambda: RC.bound("swiglu_bwd", "swiglu_bwd", dtype, swiglu_bwd(gu, dout, I).roll(I, 1), ref, E))   # dgate and dup swapped
    x = RC.gelu_edge_values(dtype, "cpu", 1003)
    dy = torch.randn(1003, generator=g).to(dtype)
    for kind in (0, 1, 2):
        ref, E = RC.gelu_fwd_reference(x, kind)
        RC.bound("gelu_fwd", "gelu_fwd", dtype, gelu(x, kind), ref, E)
        fails(lambda: RC.bound("gelu_fwd", "gelu_fwd", dtype, gelu(x, (kind + 1) % 3), ref, E))
        ref, E = RC.gelu_bwd_reference(x, dy, kind)
        RC.bound("gelu_bwd", "gelu_bwd", dtype, gelu(x, kind, dy), ref, E)
        fails(lambda: RC.bound("gelu_bwd", "gelu_bwd", dtype, gelu(x, (kind + 1) % 3, dy), ref, E))


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_cross_entropy_emulation_passes_and_mutations_fail(dtype):
    T, V = 11, 1000
    ld = RC.pad64(V)
    x, labels = RC.ce_problem(T, V, dtype, "cpu", 6)
    x[0, 8:48] = float("-inf")                                  # a run of -inf: the reference and the chain stay finite
    for gscale in (None, 0.37):
        lse, row, lc, d = ce(x, labels, ld, gscale)
        RC.check_ce(dtype, x, labels, lse, lc, d, gscale, row)
    for mut in ("label_off_by_one", "count_ignored"):
        lse, row, lc, d = ce(x, labels, ld, None, mut)
        fails(lambda: RC.check_ce(dtype, x, labels, lse, lc, d, None, row))
    lse, row, lc, d = ce(x, labels, ld)
    d2 = d.clone()
    d2[1, V + 3] = 1.0
    fails(lambda: RC.check_ce(dtype, x, labels, lse, lc, d2, None, row))                        # a write into [V, ld)
    fails(lambda: RC.check_ce(dtype, x, labels, lse * (1 + 2.0 ** -15), lc, d, None, row))      # a wrong saved statistic
    # one rule for live / counted rows
    lab = torch.tensor([-100, -1, V, ld, 5, V - 1] + [7] * (T - 6))
    assert RC.live_rows(lab, V).tolist()[:6] == [False, False, False, False, True, True]
    assert RC.counted_rows(lab).tolist()[:6] == [False, False, True, True, True, True]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_argmax_chain_and_tie_order(dtype):
    for V in (130, 4097):
        spec = RC.argmax_tie_rows(V, dtype)
        x = torch.stack([RC.argmax_row(V, dtype, "cpu", 100 + i, t, fill, ninf) for i, (_, t, fill, ninf) in enumerate(spec)])
        want, robust = RC.argmax_chain(x, 0.7)
        assert bool(robust.all())
        assert want.tolist() == [t[0] if t else 0 for _, t, _, _ in spec]
        assert argmax(x, 0.7).tolist() == want.tolist()
        assert argmax(x, 0.7, last=True).tolist() != want.tolist()                               # last index on a tie is seen
    # a row whose runner-up is distinct in s but rounds to the same p is reported as not robust (no such row is used on the GPU)
    y = torch.full((1, 16), -30.0)
    y[0, 3], y[0, 9] = 2.0 ** -7 * (1 - (2.0 ** -8 if dtype == BF else 2.0 ** -20)), 2.0 ** -7
    idx, robust = RC.argmax_chain(y.to(dtype), 1.0)
    assert idx.tolist() == [3] and not bool(robust.all())


def test_guard_bands_see_a_write_past_the_row():
    for dtype in DTYPES:
        v, g = RC.guarded((4, H), dtype, ld=H + 8, extra_rows=1, device="cpu")
        v.fill_(1.0)
        g.verify("ok")
        g.buf[g.pad + H + 2] = 1.0                                                                # a write into [H, ld)
        fails(lambda: g.verify("row padding"))
        v2, g2 = RC.guarded((4, H), dtype, extra_rows=1, device="cpu")
        v2[:3].fill_(1.0)
        fails(lambda: g2.verify("last row never written"))


# ---- MoE expert fusion ---------------------------------------------------------------------------------------------------------------
def fuse_weights(gate, idx, mode, mut=None):
    cols = list(range(len(idx))) if mut == "gate_j" else list(idx)
    w = gate.float()[:, cols]
    if mode == 1:
        if mut == "softmax_all":                                # over all E experts in place of the listed J
            a = gate.float()
            e = torch.exp(a - a.max(-1, keepdim=True).values)
            return (e / e.sum(-1, keepdim=True))[:, cols]
        e = torch.exp(w - w.max(-1, keepdim=True).values)
        w = e / e.sum(-1, keepdim=True)
    return w


def fuse_fwd(X, gate, idx, mode, mut=None):
    """expert_fuse_kernel's forward: fp32 arithmetic (mode 0 adds the experts in idx order), one rounding"""
    n, J, L = X.shape[1], len(idx), X.shape[2]
    t = fuse_weights(gate, idx, mode, mut)[:, :, None] * X.float()[list(idx)].permute(1, 0, 2)       # [n, J, L]
    if mode == 0:
        acc = torch.zeros(n, L)
        for j in range(J - 1 if mut == "drop_last" else J):
            acc = acc + t[:, j]
        return acc.to(X.dtype)
    out = t.to(X.dtype)
    return out.permute(1, 0, 2).contiguous().view(n, J, L) if mut == "layout_jnl" else out


def fuse_bwd(dout, gate, idx, mode, E, mut=None):
    """the backward = 1 form into a NaN-filled [E, n, L]: only the listed slices are written"""
    w, d = fuse_weights(gate, idx, mode), dout.float()
    dX = torch.full((E, d.shape[0], d.shape[-1]), float("nan")).to(dout.dtype)
    for j, e in enumerate(idx):
        dj = d if mode == 0 else d[:, 0 if mut == "bwd_dout0" else j]
        dX[j if mut == "bwd_slice_j" else e] = (w[:, j, None] * dj).to(dout.dtype)
    return dX


FUSE_MUTATIONS = [  # (what, mutation, backward, mode)
    ("gate[:, j] read in place of gate[:, idx[j]]", "gate_j", False, 0), ("softmax over all E experts", "softmax_all", False, 1),
    ("the mode-1 output laid out [J, n, L]", "layout_jnl", False, 1), ("the backward reads dout[n, 0] for every j", "bwd_dout0", True, 1),
    ("the backward writes slice j in place of idx[j]", "bwd_slice_j", True, 0), ("mode 0 without the last expert", "drop_last", False, 0)]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_expert_fuse_emulation_passes_and_mutations_fail(dtype):
    c = RC.c_of("expert_fuse", dtype)
    cases = [(E, idx, n, L) for (E, idx) in GPU.FUSE_EXPERTS for n in GPU.FUSE_N for L in GPU.fuse_L(dtype)[:2]]

    def ratio(E, idx, n, L, mode, backward, mut=None, exact=False):
        """worst err / (u E) of the emulation (inf: a non-finite value, or a miss where E = 0); exact: the bits of the exact family"""
        X, gate, dout = RC.expert_fuse_problem(E, idx, n, L, dtype, mode, "cpu", E + n + L, exact=exact)
        if backward:
            got = RC.fuse_listed(fuse_bwd(dout, gate, idx, mode, E, mut), idx)
            ref, Er = (RC.fuse_listed(t, idx) for t in RC.expert_fuse_bwd_reference(dout, gate, idx, mode, E))
        else:
            got = fuse_fwd(X, gate, idx, mode, mut)
            ref, Er = RC.expert_fuse_reference(X, gate, idx, mode)
        try:
            if exact:
                check_bits("exact family", got, RC.rne(ref, dtype), zero_sign=False)
                return 0.0
            return RC.check_bound("expert_fuse", got, ref, Er, float("inf"), RC.U[dtype])
        except AssertionError:
            return float("inf")

    worst = max(ratio(*cs, mode, backward) for cs in cases for mode in (0, 1) for backward in (False, True))
    print(f"\n  [expert_fuse emulation {RC.NAME[dtype]}] worst err/(u E) = {worst:.3f} (c = {c})")
    assert worst < c
    assert all(ratio(*cs, mode, backward, exact=True) == 0.0 for cs in cases for mode in (0, 1) for backward in (False, True)
               if mode == 0 or len(cs[1]) in (1, 2, 16))
    for what, mut, backward, mode in FUSE_MUTATIONS:
        by_bound = max(ratio(*cs, mode, backward, mut) for cs in cases)
        by_bits = any(ratio(*cs, mode, backward, mut, exact=True) for cs in cases if mode == 0 or len(cs[1]) in (1, 2, 16))
        print(f"  [expert_fuse {RC.NAME[dtype]}: {what}] bound: {by_bound / c:.1f}x c; exact family flags it: {by_bits}")
        assert by_bound >= 4.0 * c or by_bits, what


# ---- (c) the case lists cover the edge matrix --------------------------------------------------------------------------------------
def test_case_lists_cover_the_launch_variants():
    for d in DTYPES:
        hs = [H_ for dd, H_ in GPU.NORM_CASES if dd == d]
        assert {RC.expected_ch(d, h) for h in hs} == set(range(1, 9))
        assert {RC.body_ch(d, h) for h in hs} == {1, 2, 4, 8}
        assert all(h % RC.VN[d] == 0 for h in hs)
        assert any(h % (256 * RC.VN[d]) for h in hs if RC.expected_ch(d, h) in (3, 5))          # a ragged last chunk in a wider body
        assert RC.expected_ch(d, 256 * RC.VN[d] * 8 + RC.VN[d]) == 9                             # the refusal case of the GPU file
        assert set(GPU.CROSS_H[d]) <= set(hs)
    assert {m for m, *_ in GPU.NORM_M} == {1, 16, 17, 130}
    seen = [RC.reduce_bodies(n) for n in GPU.REDUCE_NBLK]
    assert all(s in seen for s in (set(), {"tail"}, {"unrolled"}, {"unrolled", "tail"}))
    assert set(GPU.REDUCE_NBLK) >= {0, 1, 63, 64, 65, 192, 193, 255, 256, 257, 448, 449, 512, 513, 1000}
    assert any(h % 16 for h in GPU.REDUCE_H) and all(h % 4 == 0 for h in GPU.REDUCE_H)
    assert {RC.norm_blocks(m) for m in GPU.DB_M} >= {1, 2, 3, 513}
    names = {n for V in GPU.ARGMAX_V for d in DTYPES for n, *_ in RC.argmax_tie_rows(V, d)}
    assert {"ends", "vector", "stride", "chunk", "tail", "all_equal", "neg_inf"} <= names
    assert min(GPU.ARGMAX_V) < 16384 <= max(GPU.ARGMAX_V)            # both sides of the dispatch switch; both kernels run on all
    assert any(V % 8 for V in GPU.CE_V) and any(V % 8 == 0 for V in GPU.CE_V) and max(GPU.CE_V) > 256 * 8 * 8


def test_depths_are_the_kernels_not_H():
    assert RC.norm_depth(BF, 16384) == 73 and RC.norm_depth(F32, 8192) == 41 and RC.norm_depth(BF, 8) == 17
    assert RC.reduce_depth(512) == 14 and RC.reduce_depth(1) == 13
    assert RC.ce_iters(BF, 128258) == 63 and RC.ce_iters(F32, 130) == 1

"""Kernel contract of the row-wise kernels (csrc/mm_rowwise.hip) through the C ABI: bit-exact where the arithmetic allows it,
|got - ref| <= c u E per element against fp64 elsewhere (tests/rowwise_check.py), every output in a NaN-sentinel storage
(Guarded) with spare rows and, where the entry takes one, a padded leading dimension; inputs the contract says are not read hold
NaN sentinels.  Refusals are asserted by return code with the outputs untouched; no call passes a pointer or a size an entry
does not check.  The last two sections hold the MoE expert fusion (mm_expert_fuse, forward and backward = 1) and generate()'s eos
bookkeeping (mm_decode_select) the same way."""
import ctypes
import itertools

import pytest
import torch

from tests import gemm_check as GC
from tests import rowwise_check as RC
from tests.kernel_check import SENTINEL, Guarded, check_bits, dt, lib, rc
from tests.kernel_check import ptr as p_
from tests.rowwise_check import BF, F32, U32, VN, check_exact, guarded

pytestmark = pytest.mark.gpu
DTYPES = [BF, F32]
DEV = "cuda"

# the width matrix: every norm_ch value 1..8 by name, per dtype (test_width_matrix_covers_every_ch)
WIDTHS = [8, 64, 136, 1152, 2048, 2056, 2560, 3584, 4096, 4104, 5120, 6144, 7168, 8192, 8200, 10240, 12288, 14336, 16384]
NORM_CASES = [(d, H) for d in DTYPES for H in WIDTHS if RC.expected_ch(d, H) <= 8]
NORM_M = [(1, False, 1e-5), (16, True, 1e-6), (17, True, 1e-5), (130, False, 1e-6)]        # (M, dres, eps) at every width
CROSS_H = {BF: [136, 4104, 16384], F32: [136, 2056, 8192]}                                    # full M x dres x eps cross here
REDUCE_NBLK = [0, 1, 63, 64, 65, 192, 193, 255, 256, 257, 448, 449, 512, 513, 1000]
REDUCE_H = [4, 12, 16, 136, 1152, 4096, 4100]
DB_M = [1, 15, 16, 17, 31, 32, 33, 8195]
SWIGLU_I = [8, 136, 14336, 18944]
SWIGLU_M = [1, 7, 130]
CE_V = [2, 130, 1000, 32000, 128258, 152066]
ARGMAX_V = [130, 4096, 4097, 16384, 128258]
ROPE_POS = [0, 1, 4095, 131071, 1_000_000]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def sync():
    torch.cuda.synchronize()


def f(x):
    return ctypes.c_float(x)


def untouched(*guards):
    for g in guards:
        iv = g.buf.view(torch.int16 if g.dtype == BF else torch.int32)
        assert bool((iv == SENTINEL[g.dtype]).all()), "a refused or empty call wrote to its output"


def ids(v):
    return RC.NAME[v] if isinstance(v, torch.dtype) else None


# ---- norms ---------------------------------------------------------------------------------------------------------------------
def test_width_matrix_covers_every_ch():
    for d in DTYPES:
        assert {RC.expected_ch(d, H) for dd, H in NORM_CASES if dd == d} == set(range(1, 9)), d
        assert {RC.body_ch(d, H) for dd, H in NORM_CASES if dd == d} == {1, 2, 4, 8}


def rms_case(dtype, H, M, with_res, eps, seed):
    p = RC.norm_problem(M, H, dtype, DEV, seed)
    x, dy, dres, w = RC.rows_storage(p["x"]), RC.rows_storage(p["dy"]), RC.rows_storage(p["dres"]), GC.vec_storage(p["w"], dtype)
    tag = f"rmsnorm {RC.NAME[dtype]} H={H} ch={RC.expected_ch(dtype, H)} M={M}"
    y, gy = guarded((M, H), dtype, extra_rows=2)
    rstd, gr = guarded((M,), F32)
    assert rc("mm_rmsnorm_fwd", dt(dtype), p_(x), p_(w), M, H, f(eps), p_(y), p_(rstd)) == RC.OK
    sync()
    gy.verify(tag + " y")
    gr.verify(tag + " rstd")
    check_exact(tag + " y = T(w * f32(T(x * rstd)))", y, RC.rmsnorm_chain(x, w, rstd))
    y64, Ey, r64, Er = RC.rmsnorm_fwd_reference(x, w, eps)
    RC.bound(tag + " rstd", "rmsnorm.rstd", dtype, rstd, r64, Er, u=U32)
    RC.bound(tag + " y", "rmsnorm.y", dtype, y, y64, Ey)
    nblk = RC.norm_blocks(M)
    assert lib().mm_norm_bwd_blocks(M) == nblk
    dx, gdx = guarded((M, H), dtype, extra_rows=2)
    dwp, gdw = guarded((nblk, H), F32, extra_rows=1)
    res = dres if with_res else None
    assert rc("mm_rmsnorm_bwd", dt(dtype), p_(dy), p_(x), p_(w), p_(rstd), M, H, p_(dx), p_(dwp), p_(res)) == RC.OK
    dw, gw = guarded((H,), dtype)
    assert rc("mm_reduce_partials", dt(dtype), p_(dwp), nblk, H, p_(dw), 0) == RC.OK
    sync()
    gdx.verify(tag + " dx")
    gdw.verify(tag + " dw partials")
    gw.verify(tag + " dw")
    dx64, Edx, dw64, Edw = RC.rmsnorm_bwd_reference(dy, x, w, rstd, res)
    RC.bound(tag + " dx", "rmsnorm.dx", dtype, dx, dx64, Edx)
    RC.bound(tag + " dw", "rmsnorm.dw", dtype, dw, dw64, Edw)
    dx2, dwp2 = torch.empty_like(dx.contiguous()), torch.empty(nblk, H, device=DEV)
    assert rc("mm_rmsnorm_bwd", dt(dtype), p_(dy), p_(x), p_(w), p_(rstd), M, H, p_(dx2), p_(dwp2), p_(res)) == RC.OK
    sync()
    check_exact(tag + " dw partials rerun", dwp2, dwp)
    check_exact(tag + " dx rerun", dx2, dx)


def ln_case(dtype, H, M, with_res, eps, seed):
    p = RC.norm_problem(M, H, dtype, DEV, seed, layer=True)
    x, dy, dres = RC.rows_storage(p["x"]), RC.rows_storage(p["dy"]), RC.rows_storage(p["dres"])
    w, b = GC.vec_storage(p["w"], dtype), GC.vec_storage(p["b"], dtype)
    tag = f"layernorm {RC.NAME[dtype]} H={H} ch={RC.expected_ch(dtype, H)} M={M}"
    y, gy = guarded((M, H), dtype, extra_rows=2)
    mean, gm = guarded((M,), F32)
    rstd, gr = guarded((M,), F32)
    assert rc("mm_layernorm_fwd", dt(dtype), p_(x), p_(w), p_(b), M, H, f(eps), p_(y), p_(mean), p_(rstd)) == RC.OK
    sync()
    for n_, g_ in (("y", gy), ("mean", gm), ("rstd", gr)):
        g_.verify(f"{tag} {n_}")
    y64, Ey, m64, Em, r64, Er = RC.layernorm_fwd_reference(x, w, b, eps)
    RC.bound(tag + " mean", "layernorm.mean", dtype, mean, m64, Em, u=U32)
    RC.bound(tag + " rstd", "layernorm.rstd", dtype, rstd, r64, Er, u=U32)
    RC.bound(tag + " y", "layernorm.y", dtype, y, y64, Ey)
    nblk = RC.norm_blocks(M)
    dx, gdx = guarded((M, H), dtype, extra_rows=2)
    dwp, gdw = guarded((nblk, H), F32, extra_rows=1)
    dbp, gdb = guarded((nblk, H), F32, extra_rows=1)
    res = dres if with_res else None
    args = (dt(dtype), p_(dy), p_(x), p_(w), p_(mean), p_(rstd), M, H)
    assert rc("mm_layernorm_bwd", *args, p_(dx), p_(dwp), p_(dbp), p_(res)) == RC.OK
    dw, gw = guarded((H,), dtype)
    db, gb = guarded((H,), dtype)
    assert rc("mm_reduce_partials2", dt(dtype), p_(dwp), p_(dbp), nblk, H, p_(dw), p_(db), 0, 0) == RC.OK
    sync()
    for n_, g_ in (("dx", gdx), ("dw partials", gdw), ("db partials", gdb), ("dw", gw), ("db", gb)):
        g_.verify(f"{tag} {n_}")
    dx64, Edx, dw64, Edw, db64, Edb = RC.layernorm_bwd_reference(dy, x, w, mean, rstd, res)
    RC.bound(tag + " dx", "layernorm.dx", dtype, dx, dx64, Edx)
    RC.bound(tag + " dw", "layernorm.dw", dtype, dw, dw64, Edw)
    RC.bound(tag + " db", "layernorm.db", dtype, db, db64, Edb)
    dwp2, dbp2, dx2 = torch.empty(nblk, H, device=DEV), torch.empty(nblk, H, device=DEV), torch.empty(M, H, dtype=dtype, device=DEV)
    assert rc("mm_layernorm_bwd", *args, p_(dx2), p_(dwp2), p_(dbp2), p_(res)) == RC.OK
    sync()
    check_exact(tag + " dw partials rerun", dwp2, dwp)
    check_exact(tag + " db partials rerun", dbp2, dbp)
    check_exact(tag + " dx rerun", dx2, dx)


@pytest.mark.parametrize("dtype,H", NORM_CASES, ids=lambda v: ids(v) or str(v))
def test_rmsnorm_width_matrix(dtype, H):
    for M, with_res, eps in NORM_M:
        rms_case(dtype, H, M, with_res, eps, seed=H + M)


@pytest.mark.parametrize("dtype,H", NORM_CASES, ids=lambda v: ids(v) or str(v))
def test_layernorm_width_matrix(dtype, H):
    for M, with_res, eps in NORM_M:
        ln_case(dtype, H, M, with_res, eps, seed=H + 3 * M)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_norms_full_cross_of_rows_residual_eps(dtype):
    for H in CROSS_H[dtype]:
        for M in (1, 16, 17, 130):
            for with_res in (False, True):
                for eps in (1e-5, 1e-6):
                    rms_case(dtype, H, M, with_res, eps, seed=7 * H + M)
                    ln_case(dtype, H, M, with_res, eps, seed=5 * H + M)


# ---- reduce_partials: exact --------------------------------------------------------------------------------------------------------
def test_reduce_cases_reach_both_loop_bodies():
    seen = [RC.reduce_bodies(n) for n in REDUCE_NBLK]
    assert set() in seen and {"tail"} in seen and {"unrolled"} in seen and {"unrolled", "tail"} in seen


@pytest.mark.parametrize("H", REDUCE_H)
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_reduce_partials_exact(dtype, H):
    for nblk in REDUCE_NBLK:
        pfull, before, q = RC.partials_problem(nblk + 2, H, DEV, seed=nblk * 31 + H)
        pfull[nblk:] = float("nan")                              # rows past nblk are not read
        part = pfull[:nblk]
        for acc in (0, 1):
            out, g = guarded((H,), dtype)
            out.copy_(before.to(dtype))
            assert rc("mm_reduce_partials", dt(dtype), p_(pfull), nblk, H, p_(out), acc) == RC.OK
            sync()
            g.verify(f"reduce_partials nblk={nblk} H={H}")
            want = RC.rne(RC.partials_reference(part, q, before if acc else None), dtype)
            check_exact(f"reduce_partials {RC.NAME[dtype]} nblk={nblk} H={H} accumulate={acc}", out, want)


@pytest.mark.parametrize("H", REDUCE_H)
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_reduce_partials2_exact_with_different_flags_per_pair(dtype, H):
    for nblk in REDUCE_NBLK:
        for acc0, acc1 in ((0, 1), (1, 0), (1, 1)):
            pr = [RC.partials_problem(nblk + 2, H, DEV, seed=nblk * 17 + H + k) for k in (0, 1)]
            outs = []
            for pf, before, q in pr:
                pf[nblk:] = float("nan")
                o, g = guarded((H,), dtype)
                o.copy_(before.to(dtype))
                outs.append((o, g))
            assert rc("mm_reduce_partials2", dt(dtype), p_(pr[0][0]), p_(pr[1][0]), nblk, H, p_(outs[0][0]), p_(outs[1][0]), acc0,
                      acc1) == RC.OK
            sync()
            for k, acc in ((0, acc0), (1, acc1)):
                pf, before, q = pr[k]
                outs[k][1].verify(f"reduce_partials2 pair {k}")
                want = RC.rne(RC.partials_reference(pf[:nblk], q, before if acc else None), dtype)
                check_exact(f"reduce_partials2 {RC.NAME[dtype]} nblk={nblk} H={H} pair {k} accumulate={acc}", outs[k][0], want)


@pytest.mark.parametrize("M", DB_M)
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_layernorm_db_exact_end_to_end(dtype, M):
    """integer-valued dy (times a power of two per column): every partial and the reduction are exact, so a row skipped or
    repeated at the 16-rows-per-block boundary changes db by a whole dy."""
    H = 136
    p = RC.norm_problem(M, H, dtype, DEV, seed=M, layer=True)
    g = torch.Generator(device=DEV).manual_seed(M + 1)
    q = torch.exp2(torch.randint(-3, 4, (H,), generator=g, device=DEV).double())
    dy64 = torch.randint(-8, 9, (M, H), generator=g, device=DEV).double() * q
    assert float((dy64.abs().sum(0) / q).max()) < 2.0 ** 24
    dy, x = RC.rows_storage(dy64.to(dtype)), RC.rows_storage(p["x"])
    assert torch.equal(dy.double(), dy64)
    mean, rstd = x.float().mean(-1), torch.rsqrt(x.float().var(-1, unbiased=False) + 1e-5)
    nblk = RC.norm_blocks(M)
    dx = torch.empty(M, H, dtype=dtype, device=DEV)
    dwp, gdw = guarded((nblk, H), F32, extra_rows=1)
    dbp, gdb = guarded((nblk, H), F32, extra_rows=1)
    assert rc("mm_layernorm_bwd", dt(dtype), p_(dy), p_(x), p_(p["w"]), p_(mean), p_(rstd), M, H, p_(dx), p_(dwp), p_(dbp), None) == RC.OK
    db, gb = guarded((H,), dtype)
    dw = torch.empty(H, dtype=dtype, device=DEV)
    assert rc("mm_reduce_partials2", dt(dtype), p_(dwp), p_(dbp), nblk, H, p_(dw), p_(db), 0, 0) == RC.OK
    sync()
    gdw.verify("dw partials")
    gdb.verify("db partials")
    gb.verify("db")
    check_exact(f"layernorm db {RC.NAME[dtype]} M={M}", db, RC.rne(dy64.sum(0), dtype))


# ---- add / cast: exact -------------------------------------------------------------------------------------------------------------
def sizes(vn):
    return [1, vn - 1, vn, vn + 1, 256 * vn - 1, 256 * vn, 256 * vn + 1, 1000003]


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_add_exact(dtype):
    for n in sizes(VN[dtype]):
        g = torch.Generator(device=DEV).manual_seed(n)
        a = GC.vec_storage(torch.randn(n, generator=g, device=DEV) * 3, dtype)
        b = GC.vec_storage(torch.randn(n, generator=g, device=DEV) * 0.7, dtype)
        y, gy = guarded((n,), dtype)
        assert rc("mm_add", dt(dtype), p_(a), p_(b), n, p_(y)) == RC.OK
        sync()
        gy.verify(f"add n={n}")
        check_exact(f"add {RC.NAME[dtype]} n={n}", y, (a.float() + b.float()).to(dtype))     # fp32 sum of two bf16 is exact


@pytest.mark.parametrize("dst", DTYPES, ids=ids)
@pytest.mark.parametrize("src", DTYPES, ids=ids)
def test_cast_exact(src, dst):
    for n in sizes(VN[src]) + sizes(VN[dst]):
        x = GC.vec_storage(torch.randn(n, generator=torch.Generator(device=DEV).manual_seed(n + 1), device=DEV) * 5, src)
        y, gy = guarded((n,), dst)
        assert rc("mm_cast", dt(src), dt(dst), p_(x), p_(y), n) == RC.OK
        sync()
        gy.verify(f"cast n={n}")
        check_exact(f"cast {RC.NAME[src]} -> {RC.NAME[dst]} n={n}", y, x.to(dst))


# ---- RoPE ------------------------------------------------------------------------------------------------------------------------
def rope_tables(D, theta, round_bf16, T):
    pos = torch.arange(3, T + 3, device=DEV, dtype=torch.int64)
    pos[: len(ROPE_POS)] = torch.tensor(ROPE_POS, device=DEV)
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, device=DEV, dtype=torch.int64).float() / D))
    cos, gc = guarded((T, D // 2), F32, extra_rows=1)
    sin, gs = guarded((T, D // 2), F32, extra_rows=1)
    assert rc("mm_rope_table", p_(pos), p_(inv), T, D // 2, int(round_bf16), p_(cos), p_(sin)) == RC.OK
    sync()
    gc.verify("cos")
    gs.verify("sin")
    return pos, inv, cos.contiguous(), sin.contiguous()


@pytest.mark.parametrize("round_bf16", [False, True])
@pytest.mark.parametrize("theta", [1e4, 1e6])
@pytest.mark.parametrize("D", [64, 128])
def test_rope_table_fp64_of_the_fp32_angle(D, theta, round_bf16):
    pos, inv, cos, sin = rope_tables(D, theta, round_bf16, 37)
    c64, s64, Ec, Es, u = RC.rope_table_reference(pos, inv, round_bf16)
    dtype = BF if round_bf16 else F32
    RC.bound(f"cos D={D} theta={theta:g}", "rope_table", dtype, cos, c64, Ec, u=u)
    RC.bound(f"sin D={D} theta={theta:g}", "rope_table", dtype, sin, s64, Es, u=u)
    if round_bf16:
        assert torch.equal(cos, cos.to(BF).float()) and torch.equal(sin, sin.to(BF).float())


def rope_x(dtype, T, W, seed):
    """x [T, W] inside a guarded storage with row stride W + 2 VN; the storage's padding columns and spare rows stay sentinels."""
    ld = W + 2 * VN[dtype]
    x, g = guarded((T, W), dtype, ld=ld, extra_rows=2)
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x.copy_((torch.randn(T, W, generator=gen, device=DEV) * (0.2 + 3.0 * torch.rand(T, 1, generator=gen, device=DEV))).to(dtype))
    return x, g, ld


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_rope_apply_inverse_append(dtype, D):
    T, Hq, Hkv = 37, 4, 2
    nh, W = Hq + Hkv, (Hq + 2 * Hkv) * D
    _, _, cos, sin = rope_tables(D, 1e4, dtype == BF, T)
    for inverse in (False, True):
        x, gx, ld = rope_x(dtype, T, W, seed=D + inverse)
        x0 = x.clone()
        assert rc("mm_rope_apply", dt(dtype), p_(x), T, nh, D, ld, p_(cos), p_(sin), int(inverse)) == RC.OK
        sync()
        gx.verify("rope x")
        check_exact("columns past the rotated heads", x[:, nh * D:], x0[:, nh * D:])
        ref, E = RC.rope_reference(x0, cos, sin, nh, D, inverse)
        RC.bound(f"rope {RC.NAME[dtype]} D={D} inverse={inverse}", "rope", dtype, x, ref, E)
    # append: bit-identical to apply in place + the cache copy; only the cache row of this step is written
    B, Smax, step = 7, 5, 3
    row = Hkv * D
    dstride = Smax * row + 2 * VN[dtype]
    x, gx, ld = rope_x(dtype, B, W, seed=D + 9)
    a = x.clone()
    gx2 = RC.Guarded((B + 2) * ld, dtype, DEV)
    xa = gx2.view((B, W), (ld, 1))
    xa.copy_(x)
    caches = []
    for _ in range(2):
        gcache = RC.Guarded(B * dstride, dtype, DEV)
        caches.append((gcache.view((B, Smax * row), (dstride, 1)), gcache))
        caches[-1][0].zero_()
    kc, vc = caches[0][0], caches[1][0]
    assert rc("mm_rope_append", dt(dtype), p_(xa), B, Hq, Hkv, D, ld, p_(cos), p_(sin), p_(kc[:, step * row:]), p_(vc[:, step * row:]),
              dstride) == RC.OK
    assert rc("mm_rope_apply", dt(dtype), p_(x), B, nh, D, ld, p_(cos), p_(sin), 0) == RC.OK
    sync()
    gx2.verify("append x")
    caches[0][1].verify("k cache")
    caches[1][1].verify("v cache")
    check_exact("append x == apply in place", xa, x)
    check_exact("k cache row", kc[:, step * row:(step + 1) * row], x[:, Hq * D: nh * D])
    check_exact("v cache row", vc[:, step * row:(step + 1) * row], a[:, nh * D:])
    for cache in (kc, vc):
        assert not bool(cache[:, : step * row].any()) and not bool(cache[:, (step + 1) * row:].any())
    ref, E = RC.rope_reference(a, cos[:B], sin[:B], nh, D)
    RC.bound(f"rope_append {RC.NAME[dtype]} D={D}", "rope", dtype, xa, ref, E)


# ---- SwiGLU / GELU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", SWIGLU_I)
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_swiglu_fp64_bounds(dtype, I):
    for M in SWIGLU_M:
        g = torch.Generator(device=DEV).manual_seed(M + I)
        gu = torch.randn(M, 2 * I, generator=g, device=DEV) * (0.2 + 4.0 * torch.rand(M, 1, generator=g, device=DEV))
        gu[:, I:] *= torch.linspace(0.5, 2.0, I, device=DEV)
        gu, dout = RC.rows_storage(gu.to(dtype)), RC.rows_storage(torch.randn(M, I, generator=g, device=DEV).to(dtype))
        out, go = guarded((M, I), dtype, extra_rows=2)
        dgu, gd = guarded((M, 2 * I), dtype, extra_rows=2)
        assert rc("mm_swiglu_fwd", dt(dtype), p_(gu), M, I, p_(out)) == RC.OK
        assert rc("mm_swiglu_bwd", dt(dtype), p_(gu), p_(dout), M, I, p_(dgu)) == RC.OK
        sync()
        go.verify("swiglu out")
        gd.verify("swiglu dgu")
        ref, E = RC.swiglu_fwd_reference(gu, I)
        RC.bound(f"swiglu_fwd {RC.NAME[dtype]} M={M} I={I}", "swiglu_fwd", dtype, out, ref, E)
        if dtype == BF:
            RC.swiglu_chain_check(f"swiglu_fwd chain M={M} I={I}", gu, out, I)
        ref, E = RC.swiglu_bwd_reference(gu, dout, I)
        RC.bound(f"swiglu_bwd {RC.NAME[dtype]} M={M} I={I}", "swiglu_bwd", dtype, dgu, ref, E)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_gelu_fp64_bounds_edges_and_scalar_tail(dtype, kind):
    vn = VN[dtype]
    for n in (1, vn - 1, vn, vn + 1, 1003, 4099, 256 * vn + 3):
        x = GC.vec_storage(RC.gelu_edge_values(dtype, DEV, n), dtype)
        dy = GC.vec_storage(torch.randn(n, generator=torch.Generator(device=DEV).manual_seed(n), device=DEV), dtype)
        y, gy = guarded((n,), dtype)
        dx, gdx = guarded((n,), dtype)
        assert rc("mm_gelu_fwd", dt(dtype), kind, p_(x), n, p_(y)) == RC.OK
        assert rc("mm_gelu_bwd", dt(dtype), kind, p_(x), p_(dy), n, p_(dx)) == RC.OK
        sync()
        gy.verify("gelu y")
        gdx.verify("gelu dx")
        ref, E = RC.gelu_fwd_reference(x, kind)
        RC.bound(f"gelu_fwd kind={kind} {RC.NAME[dtype]} n={n}", "gelu_fwd", dtype, y, ref, E)
        ref, E = RC.gelu_bwd_reference(x, dy, kind)
        RC.bound(f"gelu_bwd kind={kind} {RC.NAME[dtype]} n={n}", "gelu_bwd", dtype, dx, ref, E)


# ---- cross entropy -----------------------------------------------------------------------------------------------------------------
def ce_run(dtype, x, labels, ld, gscale=None, tag="ce"):
    """forward + reduce + backward on logits [T, V] stored at row stride ld; -> dict of outputs (all guards verified)."""
    T, V = x.shape
    lg = RC.logits_storage(x, ld)
    lse, gl = guarded((T,), F32)
    row, gr = guarded((T,), F32)
    lc, gc = guarded((2,), F32)
    d, gd = guarded((T, ld), dtype, extra_rows=2)
    gs = torch.tensor([gscale], dtype=torch.float32, device=DEV) if gscale is not None else None
    assert rc("mm_ce_fwd", dt(dtype), p_(lg), T, V, ld, p_(labels), p_(lse), p_(row)) == RC.OK
    assert rc("mm_ce_reduce", p_(row), p_(labels), T, p_(lc)) == RC.OK
    assert rc("mm_ce_bwd", dt(dtype), p_(lg), T, V, ld, p_(labels), p_(lse), p_(lc), p_(gs), p_(d)) == RC.OK
    sync()
    for n_, g_ in (("lse", gl), ("loss_row", gr), ("loss, count", gc), ("dlogits", gd)):
        g_.verify(f"{tag} {n_}")
    return {"logits": lg, "lse": lse, "row": row, "lc": lc, "d": d}


def ce_check(dtype, x, labels, ld, gscale, tag):
    T, V = x.shape
    o = ce_run(dtype, x, labels, ld, gscale, tag)
    RC.check_ce(dtype, x, labels, o["lse"], o["lc"], o["d"], gscale, o["row"], tag)
    return o


@pytest.mark.parametrize("V", CE_V)
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_cross_entropy_fp64_bounds(dtype, V):
    T = 11
    x, labels = RC.ce_problem(T, V, dtype, DEV, seed=V)
    for ld, gscale in ((RC.pad64(V), None), (RC.ld_vn(V, dtype), 0.37)):
        tag = f"ce {RC.NAME[dtype]} V={V} ld={ld}"
        o = ce_check(dtype, x, labels, ld, gscale, tag)
        o2 = ce_run(dtype, x, labels, ld, gscale, tag)
        for k in ("lse", "row", "lc", "d"):
            check_exact(f"{tag} {k} rerun", o2[k], o[k])


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_cross_entropy_one_rule_for_live_and_counted_rows(dtype):
    """labels -100 and -1 are ignored and not counted; labels V and ld give no loss and no gradient but are counted by
    mm_ce_reduce (a caller error the header documents; the callers never produce it)."""
    V = 130
    ld = RC.pad64(V)
    x, _ = RC.ce_problem(6, V, dtype, DEV, seed=1)
    labels = torch.tensor([-100, -1, V, ld, 5, V - 1], device=DEV, dtype=torch.int64)
    o = ce_check(dtype, x, labels, ld, None, f"ce labels {RC.NAME[dtype]}")
    assert float(o["lc"][1]) == 4.0
    assert not bool(o["row"][:4].any()) and not bool(o["d"][:4].any())
    assert bool((o["row"][4:] > 0).all()) and bool(o["d"][4:, :V].any(-1).all())


@pytest.mark.parametrize("V", [130, 5000])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_cross_entropy_runs_of_minus_inf_logits(dtype, V):
    """A run of -inf longer than one thread's 16-byte vector, at the start of the row and in the middle: the finite fp64 loss and
    gradient (what torch gives).  Before the guard in ce_fwd_kernel a thread whose first vector was all -inf computed
    exp(-inf - -inf) = NaN; when the row is longer than one sweep (V > 256 VN: the 5000 case) that thread goes on to finite
    logits and the row's lse was NaN (a thread that never sees a finite logit was already discarded: the 130 case passed)."""
    vn = VN[dtype]
    x, labels = RC.ce_problem(8, V, dtype, DEV, seed=V + 5)
    run = 3 * vn + 3
    mid = (V // 2) // vn * vn
    x[0::2, :run] = float("-inf")
    x[1::2, mid:mid + run] = float("-inf")
    x[2, : 2 * vn] = float("-inf")
    at_label = x.float().gather(1, labels.clamp(min=0)[:, None])[:, 0]
    labels = torch.where((labels >= 0) & torch.isinf(at_label), torch.full_like(labels, V - 1), labels)      # a finite logit at every label
    assert bool(torch.isfinite(x.float().gather(1, labels.clamp(min=0)[:, None])[:, 0][labels >= 0]).all())
    ce_check(dtype, x, labels, RC.pad64(V), None, f"ce -inf {RC.NAME[dtype]} V={V}")


@pytest.mark.parametrize("T", [1, 255, 256, 257, 4099])
def test_ce_reduce_exact_on_integer_rows(T):
    g = torch.Generator(device=DEV).manual_seed(T)
    labels = torch.randint(0, 50, (T,), generator=g, device=DEV)
    labels[torch.rand(T, generator=g, device=DEV) < 0.3] = -100
    row = torch.where(labels >= 0, torch.randint(0, 17, (T,), generator=g, device=DEV), torch.zeros_like(labels)).float()
    lc, gc = guarded((2,), F32)
    assert rc("mm_ce_reduce", p_(row), p_(labels), T, p_(lc)) == RC.OK
    sync()
    gc.verify("loss, count")
    count = (labels >= 0).sum().float()
    want = torch.stack([row.sum() / torch.clamp(count, min=1.0), count])         # integer sums: exact; one fp32 division
    check_exact(f"ce_reduce T={T}", lc, want)


# ---- arg-max -----------------------------------------------------------------------------------------------------------------------
def test_argmax_cases_reach_both_kernels_and_every_boundary():
    names = {n for V in ARGMAX_V for d in DTYPES for n, *_ in RC.argmax_tie_rows(V, d)}
    assert {"ends", "vector", "stride", "chunk", "tail", "all_equal", "neg_inf"} <= names
    assert any(V % VN[d] for V in ARGMAX_V for d in DTYPES) and any(V > RC.ARGMAX_CHUNK for V in ARGMAX_V)


@pytest.mark.parametrize("V", ARGMAX_V)
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_argmax_constructed_ties_one_launch_and_split(dtype, V):
    spec = RC.argmax_tie_rows(V, dtype)
    x = torch.stack([RC.argmax_row(V, dtype, DEV, 100 + i, t, fill, ninf) for i, (_, t, fill, ninf) in enumerate(spec)])
    R = x.shape[0]
    first = [t[0] if t else 0 for _, t, _, _ in spec]
    ld16 = RC.pad64(V) + 64
    for ld in (ld16, ld16 + 1):                                   # a row stride that is / is not a multiple of 16 bytes
        lg = RC.logits_storage(x, ld)
        for temp in (1.0, 0.7):
            want, robust = RC.argmax_chain(x, temp)
            assert bool(robust.all()), "a constructed row is not robust to the last bit of the softmax"
            assert want.tolist() == first, (want.tolist(), first)
            outs = []
            for split in (False, True):
                out = torch.full((R + 2,), -7, dtype=torch.int64, device=DEV)
                if split:
                    nb = lib().mm_argmax_softmax_ws_bytes(R, V)
                    ws = torch.empty((nb + 7) // 8, dtype=torch.int64, device=DEV)
                    assert rc("mm_argmax_softmax_split", dt(dtype), p_(lg), R, V, ld, f(temp), p_(out), p_(ws)) == RC.OK
                else:
                    assert rc("mm_argmax_softmax", dt(dtype), p_(lg), R, V, ld, f(temp), p_(out)) == RC.OK
                sync()
                assert out[R:].tolist() == [-7, -7]
                got = out[:R].tolist()
                assert got == first, (f"argmax {RC.NAME[dtype]} V={V} ld={ld} temp={temp} split={split}",
                                      [(n, g_, w_) for (n, *_), g_, w_ in zip(spec, got, first) if g_ != w_])
                outs.append(got)
            assert outs[0] == outs[1]


# ---- refusals: the code, and nothing written -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_refusals_return_before_any_launch(dtype):
    vn, d = VN[dtype], dt(dtype)
    Hmax = 256 * vn * 8
    buf = lambda *s: torch.zeros(*s, dtype=dtype, device=DEV)
    st = torch.zeros(64, device=DEV)
    for H, code in ((vn + vn // 2, RC.ERR_ALIGN), (Hmax + vn, RC.ERR_UNSUPPORTED)):
        x, w = buf(4, H), buf(H)
        y, gy = guarded((4, H), dtype)
        s1, g1 = guarded((4,), F32)
        s2, g2 = guarded((4,), F32)
        pw, gp = guarded((1, H), F32)
        pb, gq = guarded((1, H), F32)
        assert rc("mm_rmsnorm_fwd", d, p_(x), p_(w), 4, H, f(1e-5), p_(y), p_(s1)) == code
        assert rc("mm_rmsnorm_bwd", d, p_(x), p_(x), p_(w), p_(st), 4, H, p_(y), p_(pw), None) == code
        assert rc("mm_layernorm_fwd", d, p_(x), p_(w), p_(w), 4, H, f(1e-5), p_(y), p_(s1), p_(s2)) == code
        assert rc("mm_layernorm_bwd", d, p_(x), p_(x), p_(w), p_(st), p_(st), 4, H, p_(y), p_(pw), p_(pb), None) == code
        sync()
        untouched(gy, g1, g2, gp, gq)
    # RoPE: (D/2) % VN, ld % VN
    T, D = 4, 16 * vn
    cs = torch.zeros(T, D, device=DEV)
    x, gx = guarded((T, 4 * D + vn), dtype)
    assert rc("mm_rope_apply", d, p_(x), T, 2, 3 * vn, 4 * D + vn, p_(cs), p_(cs), 0) == RC.ERR_ALIGN
    assert rc("mm_rope_apply", d, p_(x), T, 2, D, 4 * D + 1, p_(cs), p_(cs), 0) == RC.ERR_ALIGN
    assert rc("mm_rope_append", d, p_(x), T, 1, 1, 3 * vn, 4 * D + vn, p_(cs), p_(cs), p_(x), p_(x), 4 * D) == RC.ERR_ALIGN
    # SwiGLU: I % VN
    o, go = guarded((4, 64), dtype)
    assert rc("mm_swiglu_fwd", d, p_(buf(4, 128)), 4, vn + 1, p_(o)) == RC.ERR_ALIGN
    assert rc("mm_swiglu_bwd", d, p_(buf(4, 128)), p_(buf(4, 64)), 4, vn + 1, p_(o)) == RC.ERR_ALIGN
    # GELU: kind out of range
    for kind in (-1, 3):
        assert rc("mm_gelu_fwd", d, kind, p_(buf(64)), 64, p_(o)) == RC.ERR_ARG
        assert rc("mm_gelu_bwd", d, kind, p_(buf(64)), p_(buf(64)), 64, p_(o)) == RC.ERR_ARG
    # CE: ld % VN, ld < V
    V = 16 * vn
    lg, lab = buf(4, V + vn), torch.zeros(4, dtype=torch.int64, device=DEV)
    l1, g1 = guarded((4,), F32)
    l2, g2 = guarded((4,), F32)
    dl, gd = guarded((4, V + vn), dtype)
    for ld, code in ((V + 1, RC.ERR_ALIGN), (V - vn, RC.ERR_ARG)):
        assert rc("mm_ce_fwd", d, p_(lg), 4, V, ld, p_(lab), p_(l1), p_(l2)) == code
        assert rc("mm_ce_bwd", d, p_(lg), 4, V, ld, p_(lab), p_(st), p_(st), None, p_(dl)) == code
    # arg-max: temperature <= 0
    out = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    ws = torch.zeros(64, dtype=torch.int64, device=DEV)
    for temp in (0.0, -1.0):
        assert rc("mm_argmax_softmax", d, p_(lg), 4, V, V + vn, f(temp), p_(out)) == RC.ERR_ARG
        assert rc("mm_argmax_softmax_split", d, p_(lg), 4, V, V + vn, f(temp), p_(out), p_(ws)) == RC.ERR_ARG
    # empty problems: MM_OK, nothing written
    H = 16 * vn
    x, w = buf(4, H), buf(H)
    y, gy = guarded((4, H), dtype)
    assert rc("mm_rmsnorm_fwd", d, p_(x), p_(w), 0, H, f(1e-5), p_(y), p_(l1)) == RC.OK
    assert rc("mm_rmsnorm_bwd", d, p_(x), p_(x), p_(w), p_(st), 0, H, p_(y), p_(l2), None) == RC.OK
    assert rc("mm_layernorm_fwd", d, p_(x), p_(w), p_(w), 0, H, f(1e-5), p_(y), p_(l1), p_(l2)) == RC.OK
    assert rc("mm_layernorm_bwd", d, p_(x), p_(x), p_(w), p_(st), p_(st), 0, H, p_(y), p_(l1), p_(l2), None) == RC.OK
    assert rc("mm_swiglu_fwd", d, p_(x), 0, H // 2, p_(y)) == RC.OK
    assert rc("mm_swiglu_bwd", d, p_(x), p_(x), 0, H // 2, p_(y)) == RC.OK
    assert rc("mm_gelu_fwd", d, 0, p_(x), 0, p_(y)) == RC.OK
    assert rc("mm_gelu_bwd", d, 0, p_(x), p_(x), 0, p_(y)) == RC.OK
    assert rc("mm_add", d, p_(x), p_(x), 0, p_(y)) == RC.OK
    assert rc("mm_cast", d, d, p_(x), p_(y), 0) == RC.OK
    assert rc("mm_rope_apply", d, p_(y), 0, 2, D, 4 * D, p_(cs), p_(cs), 0) == RC.OK
    assert rc("mm_rope_table", p_(lab), p_(st), 0, 8, 0, p_(l1), p_(l2)) == RC.OK
    assert rc("mm_ce_fwd", d, p_(lg), 0, V, V + vn, p_(lab), p_(l1), p_(l2)) == RC.OK
    assert rc("mm_ce_bwd", d, p_(lg), 0, V, V + vn, p_(lab), p_(st), p_(st), None, p_(dl)) == RC.OK
    assert rc("mm_argmax_softmax", d, p_(lg), 0, V, V + vn, f(1.0), p_(out)) == RC.OK
    assert rc("mm_argmax_softmax_split", d, p_(lg), 0, V, V + vn, f(1.0), p_(out), p_(ws)) == RC.OK
    sync()
    untouched(gx, go, g1, g2, gd, gy)
    assert out.tolist() == [-7] * 4


# ---- MoE expert fusion (mm_expert_fuse, forward and backward = 1) ---------------------------------------------------------------------
FUSE_EXPERTS = [(3, (0, 1, 2)), (3, (2, 0)), (4, (3,)), (16, (5, 12, 0, 9, 15, 3, 7, 1, 14, 10, 2, 8, 13, 6, 11, 4))]
FUSE_N = [1, 3]


def fuse_L(dtype):
    """one 16-byte vector; 136; 257 vectors of bf16 -- with n = 3 the n x 257 threads end in a partial 256-thread block"""
    return [VN[dtype], 136, 257 * 8]


def cints(idx):
    return (ctypes.c_int * len(idx))(*idx)


def fuse_launch(dtype, mode, E, idx, n, L, X, gate, dout):
    """forward into a guarded out, backward into a guarded [E, n, L] storage whose views are the listed experts' slices.  The
    slices of X and the columns of gate that belong to unlisted experts hold NaN: they are not read.
    -> (out, dX listed [J, n, L], tag)"""
    J = len(idx)
    tag = f"expert_fuse {RC.NAME[dtype]} mode={mode} E={E} idx={list(idx)} n={n} L={L}"
    unlisted = [e for e in range(E) if e not in idx]
    X, gate = X.clone(), gate.clone()
    X[unlisted] = float("nan")
    gate[:, unlisted] = float("nan")
    oshape = (n, L) if mode == 0 else (n, J, L)
    go = Guarded(n * L * (1 if mode == 0 else J), dtype, DEV)
    out = go.view(oshape, (L, 1) if mode == 0 else (J * L, L, 1))
    assert rc("mm_expert_fuse", dt(dtype), 0, mode, p_(X), p_(gate), cints(idx), J, E, n, L, p_(out)) == RC.OK
    gd = Guarded(E * n * L, dtype, DEV)
    dX = [gd.view((n, L), (L, 1), e * n * L) for e in idx]
    assert rc("mm_expert_fuse", dt(dtype), 1, mode, p_(dout), p_(gate), cints(idx), J, E, n, L, p_(gd.buf[gd.pad:])) == RC.OK
    sync()
    go.verify(tag + " out")
    gd.verify(tag + " dX: the listed slices are written whole, the unlisted ones keep the sentinel")
    return out, torch.stack(dX), tag


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_expert_fuse_contract(dtype, mode):
    for (E, idx), n, L in itertools.product(FUSE_EXPERTS, FUSE_N, fuse_L(dtype)):
        X, gate, dout = RC.expert_fuse_problem(E, idx, n, L, dtype, mode, DEV, E + n + L)
        out, dX, tag = fuse_launch(dtype, mode, E, idx, n, L, X, gate, dout)
        ref, Eo = RC.expert_fuse_reference(X, gate, idx, mode)
        RC.bound(tag + " out", "expert_fuse", dtype, out, ref, Eo)
        ref, Ed = RC.expert_fuse_bwd_reference(dout, gate, idx, mode, E)
        RC.bound(tag + " dX", "expert_fuse", dtype, dX, RC.fuse_listed(ref, idx), RC.fuse_listed(Ed, idx))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_expert_fuse_exact(dtype, mode):
    """integer X / dout, every gate entry 0.25: mode 0, and mode 1 with J in {1, 2, 16} (softmax exactly 1 / J), have no fp32
    rounding, so every output is the one rounding of the fp64 result, bit for bit."""
    for (E, idx), n, L in itertools.product(FUSE_EXPERTS, FUSE_N, fuse_L(dtype)):
        if mode == 1 and len(idx) not in (1, 2, 16):
            continue
        X, gate, dout = RC.expert_fuse_problem(E, idx, n, L, dtype, mode, DEV, E + n + L, exact=True)
        out, dX, tag = fuse_launch(dtype, mode, E, idx, n, L, X, gate, dout)
        check_bits(tag + " out (exact family)", out, RC.rne(RC.expert_fuse_reference(X, gate, idx, mode)[0], dtype), zero_sign=False)
        ref = RC.expert_fuse_bwd_reference(dout, gate, idx, mode, E)[0]
        check_bits(tag + " dX (exact family)", dX, RC.rne(RC.fuse_listed(ref, idx), dtype), zero_sign=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_expert_fuse_return_codes(dtype):
    """every refusal by code with nothing written; n = 0 is MM_OK and writes nothing"""
    vn, E, n, L = VN[dtype], 20, 2, 16 * VN[dtype]
    X = torch.randn(E, n, L + vn, device=DEV).to(dtype)
    gate = torch.rand(n, E, device=DEV)
    out, go = guarded((E * n, L + vn), dtype)

    def attempt(want, idx=(0, 1), mode=0, n=n, L=L):
        for backward in (0, 1):
            assert rc("mm_expert_fuse", dt(dtype), backward, mode, p_(X), p_(gate), cints(idx), len(idx), E, n, L, p_(out)) == want, \
                (want, idx, mode, n, L, backward)

    attempt(RC.ERR_ARG, idx=tuple(range(17)))                # J = 17 > 16
    attempt(RC.ERR_ARG, idx=(0, E))                          # an index >= E
    attempt(RC.ERR_ARG, idx=(0, -1))
    attempt(RC.ERR_ARG, mode=2)
    attempt(RC.ERR_ALIGN, L=L + 1)
    attempt(RC.OK, n=0)
    sync()
    untouched(go)


# ---- generate()'s eos bookkeeping (mm_decode_select) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_decode_select(B):
    """Three chained steps (columns 0, 3, 6 of out [B, 7]) on the same `finished`, rows a mix of already finished, emitting eos
    now and live: every buffer, whole -- the other columns of out and the spare elements behind B of finished / next_ids
    included --, equals a torch rendering of the header's four assignments; a finished row keeps emitting eos."""
    EOS, LD, MARK, SPARE = 2, 7, -99, 5
    r = torch.arange(B, device=DEV)
    fin = torch.full((B + SPARE,), 0xAB, dtype=torch.uint8, device=DEV)
    fin[:B] = (r % 3 == 0).to(torch.uint8)
    out = torch.full((B + 2, LD), MARK, dtype=torch.int64, device=DEV)
    nxt = torch.full((B + SPARE,), MARK, dtype=torch.int64, device=DEV)
    fin_ref, out_ref, nxt_ref = fin.clone(), out.clone(), nxt.clone()
    g = RC._gen(DEV, B)
    for step, col in enumerate((0, 3, 6)):
        tok = torch.randint(3, 1000, (B + SPARE,), generator=g, device=DEV)
        tok[:B][(r + step) % 4 == 1] = EOS
        assert rc("mm_decode_select", p_(tok), p_(fin), EOS, B, p_(out), LD, col, p_(nxt)) == RC.OK
        was = fin_ref[:B] != 0
        chosen = torch.where(was, torch.full_like(tok[:B], EOS), tok[:B])
        fin_ref[:B] |= (chosen == EOS).to(torch.uint8)
        out_ref[:B, col] = chosen
        nxt_ref[:B] = chosen
        sync()
        assert torch.equal(fin, fin_ref), f"finished after step {step}"
        assert torch.equal(out, out_ref), f"out after step {step} (column {col})"
        assert torch.equal(nxt, nxt_ref), f"next_ids after step {step}"
        assert bool((chosen[was] == EOS).all())
    assert B < 3 or bool(((out[:B, 6] == EOS) >= (out[:B, 0] == EOS)).all())     # eos sticks
    # refusals change nothing; B = 0 is MM_OK and writes nothing
    args = lambda **kw: [kw.get("tok", p_(tok)), kw.get("fin", p_(fin)), EOS, kw.get("B", B), kw.get("out", p_(out)), LD, kw.get("col", 1),
                         kw.get("nxt", p_(nxt))]
    for bad in (dict(col=LD), dict(col=-1), dict(tok=None), dict(fin=None), dict(out=None), dict(nxt=None)):
        assert rc("mm_decode_select", *args(**bad)) == RC.ERR_ARG, bad
    assert rc("mm_decode_select", *args(B=0)) == RC.OK
    sync()
    assert torch.equal(fin, fin_ref) and torch.equal(out, out_ref) and torch.equal(nxt, nxt_ref)

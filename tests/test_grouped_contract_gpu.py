"""Kernel contract of the grouped launches (include/mm_hip.h, "grouped launches"): every problem of a launch against ITS fp64
reference -- bitwise in the exact family, per-element bounds under the stand-alone constants in the random one
(tests/gemm_check.py, tests/rowwise_check.py) -- at the sizes where a grouped kernel does what the small equality tests of
tests/test_grouped_kernels_gpu.py never reach:

  * a persistent workgroup WALKS: a grouped grid is (min(tiles, CUs), groups), so with more tiles per problem than CUs a workgroup
    takes tiles blockIdx.x, + gridDim.x, ...;
  * the SUBSTITUTION: a batch of more than 320 128x128 tiles runs the LDS-DMA 128x128 kernel where the stand-alone call of one
    problem takes the register-staged one (or, for a small problem, the 64x128 tile) -- promised to give the same bits;
  * both tile-count thresholds (96, 320) of the batch, on either side;
  * expert-major outputs, where a tile that overhangs M lands in the next problem's rows.

GEMM_CASES is the table; every case asserts the plan it claims (mm_gemm_plan on the device's CU count: kernel family, tile, grid,
and the stand-alone plan it is compared with) and tests/test_grouped_check_cpu.py asserts the same claims at 256 CUs without a GPU.
Outputs live in Guarded storages; operands hold NaN beyond the contract; a grouped launch is also required to equal the stand-alone
entry point bit for bit and, where it walks, to repeat itself bit for bit.  Refusals are asserted by return code with every
output untouched and "gemm_last_kernel" as it was; no call passes a pointer or a size that an entry point does not check."""
import ctypes
from contextlib import contextmanager

import pytest
import torch

from tests import gemm_check as GC
from tests import rowwise_check as RC
from tests.gemm_check import NN, NT, TN
from tests.kernel_check import dt, lib, options, rc
from tests.kernel_check import ptr as p_
from tests.rowwise_check import BF, F32, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"
QUICK = GC.EPI_QUICK_GELU
EPIS = {"plain": 0, "bias": GC.EPI_BIAS, "bias+residual": GC.EPI_BIAS | GC.EPI_RESIDUAL, "accumulate": GC.EPI_ACCUMULATE,
        "bias+quick": GC.EPI_BIAS | QUICK, "bias+quick+residual": GC.EPI_BIAS | QUICK | GC.EPI_RESIDUAL}
LAYOUT_NAME = {NT: "NT", NN: "NN", TN: "TN"}
LIN = [(NT, "bias+residual"), (NN, "bias"), (TN, "accumulate")]


def _case(name, M, N, K, g, tile, kid, alone, tiles, variants, kind=GC.KIND_PLAIN, opts=None, walk=False, batch128=None, dtype=BF):
    """one row of the table.  tile / kid: the grouped launch's (BM, BN) and kernel id; alone: the kernel id of the stand-alone call of
    ONE problem; tiles: tiles per problem; walk: the grid is smaller than that; batch128: the 128x128 tiles of the whole batch, the
    number the tile is chosen from; variants: (layout, epilogue) pairs the GPU test runs."""
    return dict(name=name, M=M, N=N, K=K, g=g, tile=tile, kid=kid, alone=alone, tiles=tiles, variants=variants, kind=kind, opts=opts or {},
                walk=walk, batch128=batch128, dtype=dtype)


GEMM_CASES = [
    # 17 x 21 = 357 tiles per problem on 256 CUs (a second round of 101); 714 in the batch: substituted LDS-DMA 128x128 where the
    # stand-alone call takes the register-staged kernel.  K = 200: three full K-steps and a ragged 8-wide one
    _case("walk+substitution", 2100, 2600, 200, 2, (128, 128), GC.DMA128, GC.V1, 357, walk=True, batch128=714,
          variants=[(NT, "plain"), (NT, "bias"), (NT, "bias+residual"), (NN, "plain"), (NN, "bias+residual"), (TN, "plain"), (TN, "accumulate")]),
    _case("walk 64x128", 1100, 2056, 200, 2, (64, 128), GC.DMA64x128, GC.DMA64x128, 306, LIN, opts=dict(gemm_kernel=5), walk=True),
    _case("walk 64x64", 1100, 1000, 200, 2, (64, 64), GC.DMA64, GC.DMA64, 288, LIN, opts=dict(gemm_kernel=6), walk=True),
    # ViT-L fc1 on 4 images: 9 x 32 tiles per expert
    _case("act_fwd walk", 1028, 4096, 264, 2, (128, 128), GC.DMA128, GC.DMA128, 288, [(NT, "bias+quick"), (NT, "bias+quick+residual")],
          kind=GC.KIND_ACT_FWD, walk=True, batch128=576),
    # the batch's tile count on either side of 96 and 320; a stand-alone call of one such problem takes 64x128
    _case("96 tiles", 257, 200, 72, 16, (64, 128), GC.DMA64x128, GC.DMA64x128, 10, [(NT, "bias")], batch128=96),
    _case("99 tiles", 257, 384, 72, 11, (128, 128), GC.DMA128, GC.DMA64x128, 9, [(NT, "bias")], batch128=99),
    _case("90 tiles", 257, 384, 72, 10, (64, 128), GC.DMA64x128, GC.DMA64x128, 15, [(NT, "bias")], batch128=90),
    _case("320 tiles", 600, 512, 72, 16, (128, 128), GC.DMA128, GC.DMA64x128, 20, [(NT, "bias")], batch128=320),
    _case("336 tiles", 300, 896, 72, 16, (128, 128), GC.DMA128, GC.DMA64x128, 21, [(NT, "bias")], batch128=336),
]
# group counts on one small ragged shape, bf16 (64x128 tiles: 3 x 2) and fp32 (64x64 tiles, one workgroup each: 3 x 3)
for _g in (1, 3, 16):
    GEMM_CASES.append(_case(f"groups {_g} bf16", 130, 136, 72, _g, (64, 128), GC.DMA64x128, GC.DMA64x128, 6, LIN + [(NT, "plain")]))
    GEMM_CASES.append(_case(f"groups {_g} f32", 130, 136, 72, _g, (0, 0), GC.F32, GC.F32, 9, LIN + [(NT, "plain")], dtype=F32))
CASE = {c["name"]: c for c in GEMM_CASES}
WALKS = [c["name"] for c in GEMM_CASES if c["walk"] and c["kind"] == GC.KIND_PLAIN]
THRESHOLDS = [c["name"] for c in GEMM_CASES if c["batch128"] is not None and not c["walk"]]
COUNTS = [c["name"] for c in GEMM_CASES if c["name"].startswith("groups")]


def assert_plan(c, layout, epi, ncu):
    """the case reaches the path it claims on `ncu` compute units (0: the current device's): the grouped plan's kernel family, tile, id
    and grid, and the stand-alone plan of one problem.  Host only."""
    M, N, K, g, dtype = c["M"], c["N"], c["K"], c["g"], c["dtype"]
    with options(**c["opts"]):
        pg = GC.plan(dtype, layout, c["kind"], g, M, N, K, epi, ncu)
        ps = GC.plan(dtype, layout, c["kind"], 0, M, N, K, epi, ncu)
    tag = (c["name"], LAYOUT_NAME[layout], epi, pg, ps)
    assert pg["rc"] == GC.OK and pg["last"] == c["kid"] and pg["grid_y"] == g and pg["tiles"] == c["tiles"], tag
    if dtype == BF:
        assert pg["family"] == GC.FAM_DMA and pg["tile"] == c["tile"], tag
        assert pg["tiles"] == -(-M // c["tile"][0]) * -(-N // c["tile"][1]), tag
    else:
        assert pg["family"] == GC.FAM_F32, tag
    if c["walk"]:
        assert pg["grid_x"] < pg["tiles"], tag              # a workgroup takes a second tile
    else:
        assert pg["grid_x"] == pg["tiles"], tag
    if c["batch128"] is not None:
        assert g * -(-M // 128) * -(-N // 128) == c["batch128"], tag
    assert ps["rc"] == GC.OK and ps["last"] == c["alone"] and ps["grid_y"] == 1, tag
    return pg, ps


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def sync():
    torch.cuda.synchronize()


def f(x):
    return ctypes.c_float(x)


def _seed(c, layout, epi):
    return c["M"] * 7 + c["N"] * 3 + c["K"] + 131 * layout + epi


# ---- 1. grouped GEMM -------------------------------------------------------------------------------------------------------------------
def run_linear(c, layout, epi_name, family, place, same_a=False, twice=False):
    """one grouped launch of the case against fp64, against the stand-alone call of every problem (bitwise), inside guards"""
    M, N, K, g, dtype = c["M"], c["N"], c["K"], c["g"], c["dtype"]
    epi = EPIS[epi_name]
    tag = f"{c['name']} {LAYOUT_NAME[layout]} {epi_name} {family} {place}"
    assert_plan(c, layout, epi, 0)
    probs = GC.grouped_problems(family, g, M, N, K, DEV, _seed(c, layout, epi), dtype, same_a)
    As, Bs, biases, res = GC.grouped_operands(layout, probs, epi, dtype, same_a)
    at = lambda ts, p: ts[p] if ts is not None else None

    def launch():
        outs, guards = GC.grouped_out(g, M, N, place, dtype)
        if epi & GC.EPI_ACCUMULATE:
            GC.fill_c0(outs, probs, dtype)
        assert GC.launch_batched(GC.batched_args(layout, M, N, K, As, Bs, outs, biases, res, epi, dtype)) == GC.OK, tag
        sync()
        assert GC.last_kernel() == c["kid"], (tag, GC.last_kernel())          # a successful grouped launch reports its tile
        GC.verify_all(tag, guards)
        return outs

    with options(**c["opts"]):
        alone = []
        for p in range(g):                                   # the stand-alone calls first: they leave THEIR kernel id behind
            (cp,), (gp,) = GC.grouped_out(1, M, N, "separate", dtype)
            if epi & GC.EPI_ACCUMULATE:
                GC.fill_c0([cp], [probs[p]], dtype)
            assert GC.gemm(layout, As[p], Bs[p], M, N, K, cp, at(biases, p), at(res, p), epi, dtype) == c["alone"], tag
            sync()
            gp.verify(f"{tag} stand-alone {p}")
            alone.append(cp)
        outs = launch()
        again = launch() if twice else None
    GC.check_grouped(tag, family, probs, epi, outs, dtype)
    for p in range(g):
        GC.check_exact(f"{tag}: grouped vs stand-alone, problem {p}", outs[p], alone[p])
        if again is not None:
            GC.check_exact(f"{tag}: second run vs first, problem {p}", again[p], outs[p])
    if g > 1 and not same_a:
        assert not torch.equal(outs[0], outs[1]), tag        # the problems really differ


@pytest.mark.parametrize("name", WALKS)
def test_walk_exact_and_bounded(name):
    """every persistent workgroup takes more than one tile; the first case also crosses the substitution"""
    c = CASE[name]
    for i, (layout, epi_name) in enumerate(c["variants"]):
        run_linear(c, layout, epi_name, "exact", GC.GROUPED_PLACEMENTS[i % 2], twice=True)
        run_linear(c, layout, epi_name, "random", GC.GROUPED_PLACEMENTS[(i + 1) % 2])


def run_act(c, epi_name, family, place, twice=False):
    M, N, K, g = c["M"], c["N"], c["K"], c["g"]
    epi = EPIS[epi_name]
    flags = epi & ~QUICK
    tag = f"{c['name']} {epi_name} {family} {place}"
    assert_plan(c, NT, epi, 0)
    probs = GC.grouped_problems(family, g, M, N, K, DEV, _seed(c, NT, epi))
    Xs, Ws, biases, res = GC.grouped_operands(NT, probs, flags)
    ldr = res[0].stride(0) if res is not None else 0

    def launch():
        pres, gpre = GC.grouped_out(g, M, N, place)
        acts, gact = GC.grouped_out(g, M, N, place)
        assert GC.launch_batched(GC.batched_args(NT, M, N, K, Xs, Ws, acts, biases, res, epi, BF, pres=pres)) == GC.OK, tag
        sync()
        assert GC.last_kernel() == c["kid"], (tag, GC.last_kernel())
        GC.verify_all(tag + " PRE", gpre)
        GC.verify_all(tag + " ACT", gact)
        return pres, acts

    with options(**c["opts"]):
        alone = []
        for p in range(g):
            (pre,), (gp,) = GC.grouped_out(1, M, N, "separate")
            (act,), (ga,) = GC.grouped_out(1, M, N, "separate")
            assert rc("mm_gemm_act_fwd", 0, M, N, K, p_(Xs[p]), Xs[p].stride(0), p_(Ws[p]), Ws[p].stride(0), p_(biases[p]), p_(pre),
                      pre.stride(0), p_(act), act.stride(0), p_(res[p]) if res is not None else None, ldr, epi) == GC.OK, tag
            sync()
            assert GC.last_kernel() == c["alone"], tag
            gp.verify(tag + " stand-alone PRE")
            ga.verify(tag + " stand-alone ACT")
            alone.append((pre, act))
        pres, acts = launch()
        again = launch() if twice else None
    GC.check_grouped_act(tag, family, probs, flags, "quick", pres, acts)
    for p in range(g):
        GC.check_exact(f"{tag}: PRE grouped vs stand-alone, problem {p}", pres[p], alone[p][0])
        GC.check_exact(f"{tag}: ACT grouped vs stand-alone, problem {p}", acts[p], alone[p][1])
        if again is not None:
            GC.check_exact(f"{tag}: PRE second run, problem {p}", again[0][p], pres[p])
            GC.check_exact(f"{tag}: ACT second run, problem {p}", again[1][p], acts[p])
    assert not torch.equal(acts[0], acts[1]), tag


@pytest.mark.parametrize("epi_name", ["bias+quick", "bias+quick+residual"])
def test_act_fwd_walk(epi_name):
    """mm_gemm_act_fwd_batched at ViT-L fc1's tile count: PRE exact, ACT from the kernel's own PRE, both equal to mm_gemm_act_fwd"""
    c = CASE["act_fwd walk"]
    assert (NT, epi_name) in c["variants"]
    run_act(c, epi_name, "exact", "expert_major", twice=True)
    run_act(c, epi_name, "random", "separate")


@pytest.mark.parametrize("name", THRESHOLDS)
def test_tile_count_thresholds(name):
    """the tile is chosen from the tile count of the WHOLE batch (64x128 up to 96, 128x128 beyond, the substituted 128x128 past
    320) while the stand-alone call of one problem takes 64x128: exact, and the same bits on either tile"""
    c = CASE[name]
    for layout, epi_name in c["variants"]:
        run_linear(c, layout, epi_name, "exact", "expert_major")


@pytest.mark.parametrize("name", COUNTS)
def test_group_counts(name):
    c = CASE[name]
    for i, (layout, epi_name) in enumerate(c["variants"]):
        run_linear(c, layout, epi_name, "exact", GC.GROUPED_PLACEMENTS[i % 2])
        run_linear(c, layout, epi_name, "random", GC.GROUPED_PLACEMENTS[(i + 1) % 2])


def test_shared_a_across_problems():
    """the patch embedding's form: every problem reads the same A"""
    run_linear(CASE["groups 3 bf16"], NT, "plain", "exact", "expert_major", same_a=True)
    run_linear(CASE["groups 3 bf16"], NT, "bias", "random", "separate", same_a=True)


def test_unevenly_spaced_operands():
    """all operands and outputs of a launch inside ONE allocation each, at spacings that differ from problem to problem"""
    c = CASE["groups 3 bf16"]
    M, N, K, g = c["M"], c["N"], c["K"], c["g"]
    epi = EPIS["bias+residual"]
    probs = GC.grouped_problems("exact", g, M, N, K, DEV, 77)
    lda, ldb, ldc, ldr = GC.grouped_lds(NT, M, N, K)
    gaps = [8 * (1 + (5 * i) % 7) for i in range(4 * g)]      # 8 .. 56 elements: 16-byte aligned, never the same twice in a row
    pool = GC.sentinel_fill(torch.empty(g * ((M + 8) * (lda + ldr) + (N + 8) * ldb + N + 64) + sum(gaps) + 64, dtype=BF, device=DEV))
    state = {"off": 0, "i": 0}

    def carve(vals, ld, zero_to=None):
        R, W = vals.shape
        state["off"] += gaps[state["i"]]
        state["i"] += 1
        v = pool.as_strided((R, W), (ld, 1), state["off"])
        if zero_to is not None:
            pool.as_strided((R, zero_to), (ld, 1), state["off"]).zero_()
        v.copy_(vals.to(BF))
        state["off"] += GC.pad8(R * ld)
        return v

    As = [carve(d["A"], lda, GC.pad8(K)) for d in probs]
    Bs = [carve(d["B"], ldb, GC.pad8(K)) for d in probs]
    res = [carve(d["res"], ldr) for d in probs]
    biases = [carve(d["bias"][None, :], GC.pad8(N))[0] for d in probs]
    assert len({As[p + 1].data_ptr() - As[p].data_ptr() for p in range(g - 1)}) == g - 1
    guard = GC.Guarded(g * (M + 4) * ldc + 512, BF, DEV)
    outs, off = [], 0
    for p in range(g):
        off += 8 * (1 + (3 * p) % 5) + 2 * ldc
        outs.append(guard.view((M, N), (ldc, 1), off))
        off += M * ldc
    assert GC.launch_batched(GC.batched_args(NT, M, N, K, As, Bs, outs, biases, res, epi)) == GC.OK
    sync()
    guard.verify("uneven outputs")
    GC.check_grouped("uneven", "exact", probs, epi, outs)


# ---- return codes ----------------------------------------------------------------------------------------------------------------------
def _pad(ts):
    """a pointer list long enough for any `groups` a refusal test passes"""
    return list(ts) + [ts[-1]] * (GC.GROUP_MAX + 1 - len(ts))


@contextmanager
def _refusals(guards):
    """inside: calls that must write nothing and leave "gemm_last_kernel" alone (set to a known id first)"""
    a = torch.ones(64, 64, dtype=BF, device=DEV)
    assert GC.gemm(NT, a, a, 64, 64, 64, torch.empty(64, 64, dtype=BF, device=DEV)) == GC.DMA64x128
    before = GC.last_kernel()

    def refused(args, want, what):
        got = GC.launch_batched(args)
        sync()
        assert got == want, f"{what}: returned {got}, expected {want}"
        GC.untouched(guards)
        assert GC.last_kernel() == before, f"{what}: gemm_last_kernel moved from {before} to {GC.last_kernel()}"

    yield refused


def _valid(layout, M, N, K, g, epi, act_fwd=False):
    probs = GC.grouped_problems("random", g, M, N, K, DEV, 5)
    As, Bs, biases, res = GC.grouped_operands(layout, probs, epi)
    outs, guards = GC.grouped_out(g, M, N, "expert_major")
    pres, gpre = GC.grouped_out(g, M, N, "separate") if act_fwd else (None, [])
    return GC.batched_args(layout, M, N, K, As, Bs, outs, biases, res, epi, BF, pres=pres), guards + gpre


def test_gemm_batched_refusals_write_nothing():
    M, N, K, g = 130, 136, 72, 3
    args, guards = _valid(NT, M, N, K, g, EPIS["bias+residual"])
    with _refusals(guards) as refused:
        wide = dict(args, **{k: _pad(args[k]) for k in ("A", "B", "C", "bias", "res")})
        refused(dict(wide, groups=0), GC.ERR_ARG, "groups = 0")
        refused(dict(wide, groups=GC.GROUP_MAX + 1), GC.ERR_ARG, "groups = MM_GROUP_MAX + 1")
        for k in ("A", "B", "C", "bias", "res"):
            refused(dict(args, **{k: None}), GC.ERR_ARG, f"NULL {k} table")
            refused(dict(args, **{k: args[k][:-1] + [None]}), GC.ERR_ARG, f"NULL {k} entry of the last problem")
        for k, step in (("lda", 4), ("ldb", 4), ("ldc", 2), ("ldr", 2)):
            refused(dict(args, **{k: args[k] + step}), GC.ERR_ALIGN, f"{k} + {step}")
        for k, step in (("A", 2), ("A", 8), ("B", 4), ("C", 2), ("C", 4)):                 # A, B: 16 bytes; C: 8 bytes
            moved = args[k][:-1] + [args[k][-1].data_ptr() + step]
            refused(dict(args, **{k: moved}), GC.ERR_ALIGN, f"{k} of the last problem only {step} bytes off")
        refused(dict(args, M=16), GC.ERR_UNSUPPORTED, "M = 16 in NT (the weight-streaming kernels' range)")
        with options(gemm_kernel=1):
            refused(args, GC.ERR_UNSUPPORTED, "gemm_kernel = 1 (the register-staged kernel by name)")
        refused(dict(args, M=0), GC.OK, "M = 0")
        refused(dict(args, N=0), GC.OK, "N = 0")
    nn, gnn = _valid(NN, M, N, K, g, EPIS["bias"])
    with _refusals(gnn) as refused:
        refused(dict(nn, epi=nn["epi"] | QUICK), GC.ERR_UNSUPPORTED, "an activation in NN")


def test_gemm_batched_refuses_256_wide_tiles():
    """4096 x 4096 x 256 fills the chip with 256-wide tiles on its own: MM_ERR_UNSUPPORTED before any launch (real-sized buffers)"""
    M = N = 4096
    K = 256
    a = torch.ones(M, K, dtype=BF, device=DEV)
    Bs = [torch.ones(N, K, dtype=BF, device=DEV) for _ in range(2)]
    outs, guards = GC.grouped_out(2, M, N, "separate")
    with _refusals(guards) as refused:
        refused(GC.batched_args(NT, M, N, K, [a, a], Bs, outs), GC.ERR_UNSUPPORTED, "256-wide tiles")


def test_gemm_act_fwd_batched_refusals_write_nothing():
    M, N, K, g = 130, 136, 72, 3
    args, guards = _valid(NT, M, N, K, g, EPIS["bias+quick+residual"], act_fwd=True)
    with _refusals(guards) as refused:
        wide = dict(args, **{k: _pad(args[k]) for k in ("A", "B", "C", "bias", "res", "PRE")})
        refused(dict(wide, groups=0), GC.ERR_ARG, "groups = 0")
        refused(dict(wide, groups=GC.GROUP_MAX + 1), GC.ERR_ARG, "groups = MM_GROUP_MAX + 1")
        for k in ("A", "B", "C", "bias", "res", "PRE"):
            refused(dict(args, **{k: None}), GC.ERR_ARG, f"NULL {k} table")
            refused(dict(args, **{k: args[k][:-1] + [None]}), GC.ERR_ARG, f"NULL {k} entry of the last problem")
        for k, step in (("lda", 4), ("ldb", 4), ("ldc", 2), ("ldr", 2), ("ldpre", 2)):
            refused(dict(args, **{k: args[k] + step}), GC.ERR_ALIGN, f"{k} + {step}")
        for k, step in (("A", 2), ("C", 2), ("PRE", 2), ("PRE", 4)):
            moved = args[k][:-1] + [args[k][-1].data_ptr() + step]
            refused(dict(args, **{k: moved}), GC.ERR_ALIGN, f"{k} of the last problem only {step} bytes off")
        refused(dict(args, dtype=1), GC.ERR_UNSUPPORTED, "fp32")
        refused(dict(args, M=16), GC.ERR_UNSUPPORTED, "M = 16")
        with options(gemm_kernel=1):
            refused(args, GC.ERR_UNSUPPORTED, "gemm_kernel = 1")
        refused(dict(args, epi=GC.EPI_BIAS), GC.ERR_ARG, "no activation")
        refused(dict(args, M=0), GC.OK, "M = 0")


# ---- 2. grouped LayerNorm, reduce, column sums -----------------------------------------------------------------------------------------
# widths per dtype: the lower edge (one vector), then norm_ch = 1, 2, 4, 8 at a width that is no multiple of the chunk
LN_H = {BF: [8, 136, 2056, 6152, 14344], F32: [4, 132, 1028, 3076, 7172]}
LN_ROWS = [1, RC.ROWS_PER_BLOCK, RC.ROWS_PER_BLOCK + 1, 257]
LN_GROUPS = [1, 4, 16]
LN_CASES = [(d, H) for d in (BF, F32) for H in LN_H[d]]


def ids(v):
    return RC.NAME[v] if isinstance(v, torch.dtype) else None


def test_layernorm_widths_cover_every_body():
    assert lib().mm_norm_bwd_blocks(RC.ROWS_PER_BLOCK) == 1 and lib().mm_norm_bwd_blocks(RC.ROWS_PER_BLOCK + 1) == 2
    for d in (BF, F32):
        assert [RC.expected_ch(d, H) for H in LN_H[d]] == [1, 1, 2, 4, 8], d
        assert LN_H[d][0] == RC.VN[d]


def ln_grouped_case(dtype, groups, R, H, with_res, eps, seed):
    p = RC.grouped_norm_problem(groups, R, H, dtype, DEV, seed)
    M = groups * R
    x, dy, dres = RC.rows_storage(p["x"]), RC.rows_storage(p["dy"]), RC.rows_storage(p["dres"])
    ws, bs = [GC.vec_storage(w, dtype) for w in p["ws"]], [GC.vec_storage(b, dtype) for b in p["bs"]]
    tag = f"grouped layernorm {RC.NAME[dtype]} groups={groups} R={R} H={H} ch={RC.expected_ch(dtype, H)}"
    y, gy = guarded((M, H), dtype, extra_rows=2)
    mean, gm = guarded((M,), F32)
    rstd, gr = guarded((M,), F32)
    assert rc("mm_layernorm_fwd_batched", dt(dtype), p_(x), GC.pa(ws), GC.pa(bs), groups, R, H, f(eps), p_(y), p_(mean), p_(rstd)) == RC.OK
    sync()
    for n_, g_ in (("y", gy), ("mean", gm), ("rstd", gr)):
        g_.verify(f"{tag} {n_}")
    RC.check_grouped_layernorm_fwd(tag, x, ws, bs, eps, R, y, mean, rstd)
    nb = RC.norm_blocks(R)
    dx, gdx = guarded((M, H), dtype, extra_rows=2)
    dwp, gdw = guarded((groups * nb, H), F32, extra_rows=2)
    dbp, gdb = guarded((groups * nb, H), F32, extra_rows=2)
    res = dres if with_res else None
    assert rc("mm_layernorm_bwd_batched", dt(dtype), p_(dy), p_(x), GC.pa(ws), groups, p_(mean), p_(rstd), R, H, p_(dx), p_(dwp), p_(dbp),
              p_(res)) == RC.OK
    dws, dbs = [guarded((H,), dtype) for _ in range(groups)], [guarded((H,), dtype) for _ in range(groups)]
    assert rc("mm_reduce_partials2_batched", dt(dtype), p_(dwp), p_(dbp), groups, nb, H, GC.pa([v for v, _ in dws]),
              GC.pa([v for v, _ in dbs]), 0, 0) == RC.OK
    sync()
    # expert g's blocks [g nb, (g + 1) nb) fully written, the rows past groups * nb still sentinels
    for n_, g_ in [("dx", gdx), ("dw partials", gdw), ("db partials", gdb)] + [(f"dw[{i}]", g_) for i, (_, g_) in enumerate(dws)] + \
            [(f"db[{i}]", g_) for i, (_, g_) in enumerate(dbs)]:
        g_.verify(f"{tag} {n_}")
    RC.check_grouped_layernorm_bwd(tag, dy, x, ws, mean, rstd, res, R, dx, [v for v, _ in dws], [v for v, _ in dbs])


@pytest.mark.parametrize("dtype,H", LN_CASES, ids=lambda v: ids(v) or str(v))
def test_layernorm_batched_against_fp64(dtype, H):
    """forward, backward and the reduction of the partial blocks, expert by expert against fp64.  The full groups x rows cross at the
    two narrow widths; every row count (16 experts up to one block of rows, 4 beyond) at the wide ones."""
    narrow = H <= 136
    i = 0
    for R in LN_ROWS:
        for groups in (LN_GROUPS if narrow else [16 if R <= RC.ROWS_PER_BLOCK else 4]):
            ln_grouped_case(dtype, groups, R, H, with_res=bool(i % 2), eps=1e-5 if i % 3 else 1e-6, seed=H + 3 * R + groups)
            i += 1
    if narrow:
        for R in LN_ROWS:                                  # the other dres setting
            ln_grouped_case(dtype, 4, R, H, with_res=not bool(R % 2), eps=1e-5, seed=H + R)


@pytest.mark.parametrize("dtype", [BF, F32], ids=ids)
def test_layernorm_batched_refusals_write_nothing(dtype):
    groups, R = 2, 3
    vn = RC.VN[dtype]
    hmax = 256 * 8 * vn
    for H, want, Rr in ((hmax + vn, RC.ERR_UNSUPPORTED, R), (136 + vn // 2, RC.ERR_ALIGN, R), (136, RC.OK, 0)):
        Hs = -(-H // vn) * vn                                   # real-sized buffers whatever the call claims
        p = RC.grouped_norm_problem(groups, R, Hs, dtype, DEV, 3)
        ws, bs = [GC.vec_storage(w, dtype) for w in p["ws"]], [GC.vec_storage(b, dtype) for b in p["bs"]]
        M = groups * R
        outs = [guarded((M, Hs), dtype), guarded((M,), F32), guarded((M,), F32)]
        (y, _), (mean, _), (rstd, _) = outs
        assert rc("mm_layernorm_fwd_batched", dt(dtype), p_(p["x"]), GC.pa(ws), GC.pa(bs), groups, Rr, H, f(1e-5), p_(y), p_(mean),
                  p_(rstd)) == want, (H, Rr)
        mean0 = torch.zeros(M, device=DEV)
        bouts = [guarded((M, Hs), dtype), guarded((groups, Hs), F32), guarded((groups, Hs), F32)]
        (dx, _), (dwp, _), (dbp, _) = bouts
        assert rc("mm_layernorm_bwd_batched", dt(dtype), p_(p["dy"]), p_(p["x"]), GC.pa(ws), groups, p_(mean0), p_(mean0), Rr, H, p_(dx),
                  p_(dwp), p_(dbp), None) == want, (H, Rr)
        sync()
        GC.untouched([g_ for _, g_ in outs + bouts])
    p = RC.grouped_norm_problem(groups, R, 136, dtype, DEV, 3)
    ws = [GC.vec_storage(w, dtype) for w in p["ws"]]
    y, gy = guarded((groups * R, 136), dtype)
    st = torch.zeros(groups * R, device=DEV)
    for g, tabs, what in ((0, (ws, ws), "groups = 0"), (GC.GROUP_MAX + 1, (ws, ws), "groups = 17"), (groups, (None, ws), "NULL w table"),
                          (groups, (ws, None), "NULL b table"), (groups, ([ws[0], None], ws), "NULL w entry"),
                          (groups, (ws, [ws[0], None]), "NULL b entry")):
        w_, b_ = (_pad(t) if t is not None and all(e is not None for e in t) else t for t in tabs)
        assert rc("mm_layernorm_fwd_batched", dt(dtype), p_(p["x"]), GC.pa(w_), GC.pa(b_), g, R, 136, f(1e-5), p_(y), p_(st), p_(st)) == RC.ERR_ARG, what
    sync()
    GC.untouched([gy])


REDUCE_NBLK = [0, 1, 65, 256, 300]
REDUCE_H = [4, 16, 1032]


def test_grouped_reduce_cases_reach_both_loop_bodies():
    seen = [RC.reduce_bodies(n) for n in REDUCE_NBLK]
    assert set() in seen and {"tail"} in seen and {"unrolled"} in seen and {"unrolled", "tail"} in seen


@pytest.mark.parametrize("H", REDUCE_H)
@pytest.mark.parametrize("dtype", [BF, F32], ids=ids)
def test_reduce_partials2_batched_exact(dtype, H):
    """expert g's nblk blocks into out0[g] / out1[g]: exact-family partials per expert and per pair, every accumulate combination"""
    combos = [(0, 1), (1, 0), (1, 1), (0, 0)]
    i = 0
    for groups, nblks in ((16, REDUCE_NBLK), (4, [300]), (1, [1, 300])):
        for nblk in nblks:
            for acc in (combos if nblk == 300 and groups == 16 else [combos[i % 4]]):
                i += 1
                pairs = [RC.grouped_partials_problem(groups, nblk, H, DEV, seed=nblk * 17 + H + 1000 * k + groups) for k in (0, 1)]
                outs = [[guarded((H,), dtype) for _ in range(groups)] for _ in (0, 1)]
                for k in (0, 1):
                    for g in range(groups):
                        outs[k][g][0].copy_(pairs[k][1][g].to(dtype))
                assert rc("mm_reduce_partials2_batched", dt(dtype), p_(pairs[0][0]), p_(pairs[1][0]), groups, nblk, H,
                          GC.pa([v for v, _ in outs[0]]), GC.pa([v for v, _ in outs[1]]), acc[0], acc[1]) == RC.OK
                sync()
                tag = f"reduce_partials2_batched {RC.NAME[dtype]} groups={groups} nblk={nblk} H={H} accumulate={acc}"
                for k in (0, 1):
                    for g in range(groups):
                        outs[k][g][1].verify(f"{tag} pair {k} expert {g}")
                    pfull, befores, qs = pairs[k]
                    RC.check_grouped_partials(f"{tag} pair {k}", pfull, befores, qs, nblk, acc[k], [v for v, _ in outs[k]], dtype)


COLSUM_R = [1, 31, 32, 33, 127, 128, 129, 1028]       # the 32 row lanes and the 4 x 32-row unroll, on either side
COLSUM_N = [3, 130, 1024, 1032]                       # ragged vectors (the scalar branch) and a partial last block


@pytest.mark.parametrize("N", COLSUM_N)
@pytest.mark.parametrize("groups", [1, 16])
@pytest.mark.parametrize("dtype", [BF, F32], ids=ids)
def test_colsum_batched_exact(dtype, groups, N):
    """exact-family rows, expert-major at a padded ldx (expert g + 1's first row follows expert g's last): out[g] = the ONE rounding
    of the fp64 column sum (+ what it held)"""
    for R in COLSUM_R:
        probs = GC.colsum_problems(groups, R, N, DEV, seed=R * 13 + N)
        xs = GC.colsum_storage(probs, dtype)
        for acc in (False, True):
            outs = [guarded((N,), dtype) for _ in range(groups)]
            wants = []
            for (o, _), d in zip(outs, probs):
                base, want = GC.colsum_want(d, acc, dtype)
                if acc:
                    o.copy_(base)
                wants.append(want)
            assert rc("mm_colsum_batched", dt(dtype), GC.pa(xs), groups, R, N, xs[0].stride(0), GC.pa([o for o, _ in outs]), int(acc)) == GC.OK
            sync()
            for g, ((o, go), want) in enumerate(zip(outs, wants)):
                go.verify(f"colsum out[{g}]")
                GC.check_exact(f"colsum_batched {RC.NAME[dtype]} groups={groups} R={R} N={N} accumulate={acc} expert {g}", o, want)


def test_colsum_batched_refusals_write_nothing():
    probs = GC.colsum_problems(2, 5, 130, DEV, 9)
    xs = GC.colsum_storage(probs, BF)
    outs = [guarded((130,), BF) for _ in range(2)]
    po = [o for o, _ in outs]
    ld = xs[0].stride(0)
    for args, want in (((_pad(xs), 0, 5, 130, ld, _pad(po)), GC.ERR_ARG), ((_pad(xs), GC.GROUP_MAX + 1, 5, 130, ld, _pad(po)), GC.ERR_ARG),
                       ((None, 2, 5, 130, ld, po), GC.ERR_ARG), ((xs, 2, 5, 130, ld, None), GC.ERR_ARG),
                       (([xs[0], None], 2, 5, 130, ld, po), GC.ERR_ARG), ((xs, 2, 5, 130, ld, [po[0], None]), GC.ERR_ARG),
                       ((xs, 2, 5, 130, ld + 4, po), GC.ERR_ALIGN), (([xs[0], xs[1].data_ptr() + 2], 2, 5, 130, ld, po), GC.ERR_ALIGN)):
        X, g, R, N, ldx, out = args
        assert rc("mm_colsum_batched", 0, GC.pa(X), g, R, N, ldx, GC.pa(out), 0) == want, args[1:5]
    sync()
    GC.untouched([g_ for _, g_ in outs])


# ---- 3. the autograd level at walk size ------------------------------------------------------------------------------------------------
@contextmanager
def _recorded():
    """names of the library calls made through multimeditron_amd.kernels inside the block"""
    from multimeditron_amd import kernels
    names, real = [], kernels.call

    def spy(name, *a):
        names.append(name)
        return real(name, *a)

    kernels.call = spy
    try:
        yield names
    finally:
        kernels.call = real


def test_grouped_linear_autograd_at_walk_size():
    """functional.grouped_linear with bias + quick_gelu + residual, E = 2 experts of 2100 rows, 2056 -> 2056: the forward (act_fwd),
    dgrad (NN) and wgrad (TN, accumulating) each count 17 x 17 = 289 tiles per expert, so every one walks on the substituted kernel.
    Bit for bit against E calls of functional.linear; the grouped entry points ran, not the per-problem loop."""
    from multimeditron_amd import functional as Fm
    from multimeditron_amd._lib import EPI_QUICK_GELU
    from multimeditron_amd.nn import grad_dummy
    E, R, D = 2, 2100, 2056
    for layout, kind, epi in ((NT, GC.KIND_ACT_FWD, EPIS["bias+quick+residual"]), (NN, GC.KIND_PLAIN, 0), (TN, GC.KIND_PLAIN, GC.EPI_ACCUMULATE)):
        M, N, K = (D, D, R) if layout == TN else (R, D, D)
        pg = GC.plan(BF, layout, kind, E, M, N, K, epi, 0, lds=(D, D, D, D))
        assert pg["rc"] == GC.OK and pg["last"] == GC.DMA128 and pg["tiles"] == 289 and pg["grid_x"] < 289 and pg["grid_y"] == E, pg
    gen = torch.Generator().manual_seed(31)
    rnd = lambda *s: (torch.randn(s, generator=gen) * 0.5).to(BF).cuda()
    x, dy, res = rnd(E * R, D), rnd(E * R, D), rnd(E * R, D)
    vals = [{"w": rnd(D, D) * 0.1, "b": rnd(D), "gw": rnd(D, D), "gb": rnd(D)} for _ in range(E)]

    def params():
        out = []
        for v in vals:
            w, b = torch.nn.Parameter(v["w"].clone()), torch.nn.Parameter(v["b"].clone())
            w.grad, b.grad = v["gw"].clone(), v["gb"].clone()      # the gradients accumulate: wgrad runs with MM_EPI_ACCUMULATE
            out.append((w, b))
        return out

    grouped, single = params(), params()
    rows = [slice(e * R, (e + 1) * R) for e in range(E)]
    xg, rg = x.clone().requires_grad_(), res.clone().requires_grad_()
    with _recorded() as names:
        yg = Fm.grouped_linear(xg, [w for w, _ in grouped], [b for _, b in grouped], residual=rg, act=EPI_QUICK_GELU,
                               dummy=grad_dummy(grouped[0][0]))
        yg.backward(dy)
    sync()
    assert names.count("mm_gemm_act_fwd_batched") == 1 and names.count("mm_gemm_batched") == 2 and names.count("mm_colsum_batched") == 1, names
    assert not {"mm_gemm", "mm_gemm_act_fwd", "mm_colsum"} & set(names), names      # no per-problem fallback loop
    xs = [x[sl].clone().requires_grad_() for sl in rows]
    rs = [res[sl].clone().requires_grad_() for sl in rows]
    ys = [Fm.linear(xs[e], single[e][0], single[e][1], residual=rs[e], act=EPI_QUICK_GELU, dummy=grad_dummy(single[e][0])) for e in range(E)]
    for e in range(E):
        ys[e].backward(dy[rows[e]])
    sync()
    GC.check_exact("y", yg, torch.cat(ys))
    GC.check_exact("dx", xg.grad, torch.cat([t.grad for t in xs]))
    GC.check_exact("dresidual", rg.grad, torch.cat([t.grad for t in rs]))
    for e in range(E):
        GC.check_exact(f"w.grad of expert {e}", grouped[e][0].grad, single[e][0].grad)
        GC.check_exact(f"b.grad of expert {e}", grouped[e][1].grad, single[e][1].grad)
    assert not torch.equal(grouped[0][0].grad, grouped[1][0].grad)

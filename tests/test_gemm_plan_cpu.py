"""The GEMM launch planner (csrc/mm_gemm_plan.h through mm_gemm_plan) without a GPU.

tests/golden/gemm_plan.jsonl records, per problem, option flip and CU count, what the dispatch decided before the planner existed
(kernel family and template arguments, grid, block, LDS bytes, the kernel-argument ints, the return code and the kernel id): the
planner must reproduce every row.  A policy change rewrites the table (tools/make_golden.py gemm_plan) and shows up as its diff."""
import ctypes
import json
import os

from multimeditron_amd import _lib
from tests import gemm_check as GC

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan.jsonl")
PLAN_INTS = 26
PLAN_FIELDS = ("rc", "last_kernel", "family", "t0", "t1", "t2", "t3", "t4", "t5", "t6", "t7", "grid_x", "grid_y", "block", "lds", "nbm", "nbn",
               "tail", "pipe", "stagger", "stagger_slots", "diag_epi", "shuffle", "group_m", "stream_epi", "rowmajor")
# name -> (a value to store, what reads back, a value out of range or None when every int is taken)
OPTIONS = {
    "adamw_blocks": (7, 7, -1), "gemm_tail": (5, 1, None), "gemm_skinny": (-3, 1, None), "gemv_stream": (2, 1, None), "gemv_nt": (9, 1, None),
    "gemv_wgs": (3, 3, None), "gemm_small": (5, 5, 6), "gemm_persist": (4, 1, None), "gemm_epi_pipe": (2, 1, None),
    "gemm_issue_waves": (8, 8, 6), "gemm_w4_rowmajor": (3, 1, None), "gemm_w4_big": (1, 1, 2), "gemm_w4_group_m": (4, 4, 0),
    "gemm_w4_stream": (7, 1, None), "gemm_w4_shuffle": (2, 1, None), "gemm_w4_diag_epi": (5, 5, None), "gemm_w4_stagger_slots": (32, 32, 33),
    "gemm_w4_stagger": (100, 100, -1), "gemm_w4": (6, 6, -1), "gemm_kernel": (6, 6, 7),
    # the attention kernels' switches (mm_attn.hip answers them): tests/kernel_check.options needs them to read back
    "attn_decode_mfma": (0, 0, None), "attn_decode_wgs": (8, 8, 0), "attn_q_prio": (0, 0, None), "attn_diag": (2, 2, None),
}


def rows():
    with open(TABLE) as f:
        next(f)                       # the header line names the fields
        return [json.loads(line) for line in f]


def plan(problem, ncu):
    out = (ctypes.c_int * PLAN_INTS)()
    assert _lib.lib().mm_gemm_plan(*problem, ncu, out) == 0, problem
    return list(out)


def by_option(table):
    """rows grouped by their option flip, so that each switch is set once"""
    groups = {}
    for r in table:
        groups.setdefault(tuple(r["opt"]) if r["opt"] else None, []).append(r)
    return groups


def set_option(name, value):
    return _lib.lib().mm_set_option(name.encode(), value)


def test_planner_reproduces_the_recorded_decisions():
    table = rows()
    assert PLAN_INTS == len(PLAN_FIELDS)
    # the table is the sweep: every return code, every kernel id and "unchanged", every kernel family and both CU counts are in it
    assert {r["plan"][0] for r in table} == {0, -1, -2, -3} and {r["plan"][2] for r in table} == {-1, 0, 1, 2, 3, 4, 5}
    assert {r["plan"][1] for r in table} == {-2, 0, 1, 2, 3, 4, 5, 10, 20, 21, 30} and {r["ncu"] for r in table} == {64, 256}
    bad = []
    for opt, rs in by_option(table).items():
        old = _lib.get_option(opt[0]) if opt else None
        if opt:
            assert set_option(*opt) == 0, opt
        try:
            for r in rs:
                got = plan(r["problem"], r["ncu"])
                if got != r["plan"]:
                    diff = {f: (w, g) for f, w, g in zip(PLAN_FIELDS, r["plan"], got) if w != g}
                    bad.append((opt, r["ncu"], r["problem"], diff))
        finally:
            if opt:
                assert set_option(opt[0], old) == 0
    assert not bad, f"{len(bad)} of {len(table)} rows differ (field: (recorded, planned)); first: {bad[:5]}"


def test_planner_agrees_with_the_tests_own_oracle():
    """plain stand-alone mm_gemm rows within the 32-bit offsets: the kernel id is gemm_check.expected_kernel's"""
    checked = set()
    for opt, rs in by_option(rows()).items():
        if opt and opt[0] not in ("gemm_kernel", "gemm_w4", "gemv_stream"):
            continue                                     # expected_kernel models these three switches
        kw = {} if not opt else {{"gemm_kernel": "forced", "gemm_w4": "w4", "gemv_stream": "gemv"}[opt[0]]: opt[1]}
        for r in rs:
            dtype, layout, kind, groups, M, N, K, lda, ldb, ldc, ldr, ldaux, epi, _, _ = r["problem"]
            rc, last = r["plan"][:2]
            if dtype != 0 or kind != 0 or groups != 0 or rc != 0:
                continue
            if max(N * ldb * 2, K * ldb * 2, K * lda * 2, 16 * lda * 2, max(ldc, ldr) * 256 + 2 * N) >= 1 << 31:
                continue                                 # every byte offset below 2^31: within each of the dispatch's 32-bit limits
            acts = bool(epi & (GC.EPI_GELU_ERF | GC.EPI_QUICK_GELU | GC.EPI_GELU_TANH))
            want = GC.expected_kernel(layout, M, N, K, acts=acts, ncu_tiles=192, **kw)
            assert last == want, (opt, r["problem"], last, want)
            checked.add(want)
    assert checked == {GC.V1, GC.DMA256x128, GC.DMA256x256, GC.DMA128, GC.DMA64x128, GC.DMA64, GC.W4, GC.SKINNY, GC.GEMV}      # every id the oracle knows


def test_every_option_reads_back_what_was_set():
    L = _lib.lib()
    for name, (value, stored, out_of_range) in OPTIONS.items():
        old = _lib.get_option(name)
        try:
            assert set_option(name, value) == 0 and _lib.get_option(name) == stored, name
            if out_of_range is not None:
                assert set_option(name, out_of_range) == -1 and _lib.get_option(name) == stored, name
        finally:
            assert set_option(name, old) == 0 and _lib.get_option(name) == old, name
    v = ctypes.c_int(0)
    assert L.mm_get_option(b"gemm_last_kernel", ctypes.byref(v)) == 0 and set_option("gemm_last_kernel", 3) == -1      # read-only
    assert L.mm_get_option(b"no_such_option", ctypes.byref(v)) == -1 and set_option("no_such_option", 1) == -1

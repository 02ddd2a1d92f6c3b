"""Kernel contract of the embedding, splice, ViT-glue and row-mover kernels (csrc/mm_embed.hip) through the C ABI: the embedding
gradient against fp64 per element and, on integer data, bit for bit (tests/embed_check.py), with run shapes placed on the chunk
edges by hand, the scratch poisoned with NaN sentinels and every case run twice; the sort, the splice map and every mover bit for
bit.  Outputs live in NaN-sentinel storages (Guarded); int32 outputs are fp32 storages seen as int32.  Refusals are asserted by
return code with nothing written."""
import ctypes

import pytest
import torch

from tests import embed_check as EC
from tests.embed_check import BF, F32, VN
from tests.kernel_check import SENTINEL, Guarded, check_bits, dt, lib, rc, sentinel_fill
from tests.kernel_check import ptr as p_

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [BF, F32]
WIDTHS = {BF: [8, 512, 520], F32: [4, 256, 260]}          # one short slice, exactly one slice, one slice and a ragged second
SORT_T = [1, 31, 32, 33, 63, 64, 65, 8191, 8192, 8193, 16385]
SPLICE_T = [1, 3, 4, 5, 8193]                              # 8193 rows: past the 2048-block cap of the row kernels
N_MOD = [0, 1, 8193]
CHECK_IDS_T = [1, 255, 256, 257]


def _every_third(ids):
    m = torch.full((ids.numel(),), -1, dtype=torch.int32)
    m[::3] = torch.arange(ids.numel(), dtype=torch.int32)[::3] % 7
    return m


def _all(ids):
    return torch.arange(ids.numel(), dtype=torch.int32) % 5


# name -> (run lengths, invalid tail, src_map builder or None): where the runs fall in the chunks of 32 sorted positions
DEMB_CASES = {
    "one full chunk": ([32], 0, None),
    "one id, two full chunks": ([64], 0, None),
    "one past the edge": ([33], 0, None),
    "run ends on the edge": ([31, 1, 32], 0, None),
    "one id, four chunks": ([100], 0, None),
    "run starts on the last slot": ([1] * 31 + [2], 0, None),
    "chunk continues one run and starts another": ([16, 32, 16], 0, None),
    "three runs over four chunks": ([40, 40, 40], 0, None),
    "one id, T = 200": ([200], 0, None),
    "invalid chunks behind 64 valid tokens": ([30, 34], 40, None),
    "T % 32 == 0, the last run meets the padding": ([10, 54], 0, None),
    "every token out of range": ([], 40, None),
    "every token under a splice": ([20, 20], 0, _all),
    "every third token under a splice": ([40, 40, 40], 7, _every_third),
    "T = 1": ([1], 0, None),
}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def sync():
    torch.cuda.synchronize()


def ids(v):
    return EC.NAME[v] if isinstance(v, torch.dtype) else None


def input_storage(x, pad=64):
    """x (contiguous) in front of `pad` sentinel elements: nothing behind x is read"""
    n = x.numel()
    if x.dtype in (BF, F32):
        buf = sentinel_fill(torch.empty(n + pad, dtype=x.dtype, device=DEV))
    else:
        buf = torch.full((n + pad,), -(2 ** 30), dtype=x.dtype, device=DEV)
    buf[:n] = x.reshape(-1)
    return buf[:n].view(x.shape)


def out_storage(shape, dtype, ld=None, extra=0):
    """-> (view, Guarded): a sentinel-filled output [.., W] (row stride ld for 2-D)"""
    if len(shape) == 2 and ld is not None:
        g = Guarded(shape[0] * ld + extra, dtype, DEV)
        return g.view(shape, (ld, 1)), g
    n = 1
    for s in shape:
        n *= s
    g = Guarded(n + extra, dtype, DEV)
    stride, acc = [], 1
    for s in reversed(shape):
        stride.append(acc)
        acc *= s
    return g.view(tuple(shape), tuple(reversed(stride))), g


def i32_storage(n, covered=None):
    """an int32 output: a guarded fp32 storage seen as int32; only the first `covered` elements are expected to be written"""
    g = Guarded(n, F32, DEV)
    g.view((n if covered is None else covered,), (1,))
    return g.buf[g.pad:g.pad + n].view(torch.int32), g


def bands_intact(name, g):
    """the guard bands alone (a storage whose inside is legitimately left partly unwritten, or pre-filled)"""
    iv = g.buf.view(torch.int16 if g.dtype == BF else torch.int32)
    bad = ~g.covered & (iv != SENTINEL[g.dtype])
    assert not bool(bad.any()), f"{name}: write outside the output ({int(bad.sum())} elements)"


def all_sentinel(*guards):
    sync()
    for g in guards:
        iv = g.buf.view(torch.int16 if g.dtype == BF else torch.int32)
        assert bool((iv == SENTINEL[g.dtype]).all()), "a refused or empty call wrote to its output"


def rnd(shape, dtype, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator(DEV).manual_seed(seed), device=DEV) * scale).to(dtype)


# ---- sort ----------------------------------------------------------------------------------------------------------------------------
def sort_call(idt, smap, vocab, tag):
    """mm_embed_sort into guarded storages, checked against the reference -> (order, skey) device int32 views (padded sizes)"""
    T = idt.numel()
    n_order, _ = EC.sizes(T, 8)
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib().mm_embed_sort_sizes(T, 8, ctypes.byref(a), ctypes.byref(b)) == EC.OK and (a.value, b.value) == EC.sizes(T, 8)
    ws, gws = i32_storage(T)
    order, gorder = i32_storage(n_order, covered=T)           # order[T:] is not written
    skey, gskey = i32_storage(n_order)
    assert rc("mm_embed_sort", p_(idt), p_(smap), T, vocab, p_(ws), p_(order), p_(skey)) == EC.OK, tag
    sync()
    gws.verify(tag + " key workspace")
    gorder.verify(tag + " order")
    gskey.verify(tag + " skey")
    o_ref, k_ref = EC.sort_reference(idt, smap, vocab)
    assert bool((order[:T] == o_ref).all()), f"{tag}: order is not the stable sort by (key, t)"
    assert bool((skey == k_ref).all()), f"{tag}: skey is not the sorted keys followed by the padding"
    return order, skey


def sort_distributions(T, seed):
    gen = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi: torch.randint(lo, hi, (T,), generator=gen)
    yield "all equal", torch.full((T,), 5, dtype=torch.int64), 10
    yield "all distinct", torch.randperm(T, generator=gen), T
    yield "vocab of one", torch.zeros(T, dtype=torch.int64), 1
    yield "heavy id 0", torch.where(torch.rand(T, generator=gen) < 0.9, torch.zeros(T, dtype=torch.int64), ri(0, 100)), 100
    yield "negative ids", ri(-3, 6), 6
    yield "ids past the vocabulary", ri(0, 12), 8


@pytest.mark.parametrize("T", SORT_T)
def test_embed_sort(T):
    for name, idc, vocab in sort_distributions(T, T):
        for with_map in (False, True):
            smap = None
            if with_map:
                smap = input_storage(torch.where(torch.rand(T, generator=torch.Generator().manual_seed(T + 1)) < 0.3,
                                                 torch.arange(T) % 11, torch.full((T,), -1)).to(torch.int32))
            sort_call(input_storage(idc), smap, vocab, f"sort T={T} {name} map={with_map}")


def test_embed_sort_refusals():
    idt = input_storage(torch.zeros(8, dtype=torch.int64))
    ws, gws = i32_storage(8)
    order, go = i32_storage(64)
    skey, gs = i32_storage(64)
    for bad in range(4):
        a = [p_(idt), p_(ws), p_(order), p_(skey)]
        a[bad] = None
        assert rc("mm_embed_sort", a[0], None, 8, 10, a[1], a[2], a[3]) == EC.ERR_ARG
    assert rc("mm_embed_sort", p_(idt), None, -1, 10, p_(ws), p_(order), p_(skey)) == EC.ERR_ARG
    assert rc("mm_embed_sort", p_(idt), None, 8, 0, p_(ws), p_(order), p_(skey)) == EC.ERR_ARG
    assert rc("mm_embed_sort", p_(idt), None, 0, 10, p_(ws), p_(order), p_(skey)) == EC.OK
    all_sentinel(gws, go, gs)


# ---- embedding gradient ----------------------------------------------------------------------------------------------------------------
def demb_call(dtype, dE, idt, smap, vocab, order, skey, old, accumulate, tag):
    T, H = dE.shape
    gd = Guarded(vocab * H, dtype, DEV)
    demb = gd.view((vocab, H), (H, 1))
    demb.copy_(old)
    gscr = Guarded(EC.sizes(T, H)[1], F32, DEV)              # poisoned: a slot nobody wrote reads as NaN
    scr = gscr.view((EC.sizes(T, H)[1],), (1,))
    assert rc("mm_embed_splice_bwd", dt(dtype), p_(dE), H, p_(idt), p_(smap), T, None, None, 0, T, None, p_(demb), vocab, p_(order),
              p_(skey), p_(scr), accumulate) == EC.OK, tag
    sync()
    bands_intact(tag + " demb", gd)
    bands_intact(tag + " scratch", gscr)
    return demb


def run_demb_case(dtype, H, name, accumulate, exact, seed=0):
    lengths, tail, mapper = DEMB_CASES[name]
    idc, vocab = EC.runs(lengths, tail, seed)
    T = idc.numel()
    idt = input_storage(idc)
    smap = input_storage(mapper(idc)) if mapper else None
    tag = f"demb {EC.NAME[dtype]} H={H} [{name}] acc={accumulate} {'exact' if exact else 'random'}"
    order, skey = sort_call(idt, smap, vocab, tag)
    dE, q = EC.exact_rows(T, H, dtype, DEV, seed + 1) if exact else (rnd((T, H), dtype, seed + 1), None)
    dE = input_storage(dE)
    old = EC.old_rows(vocab, H, dtype, DEV)
    demb = demb_call(dtype, dE, idt, smap, vocab, order, skey, old, accumulate, tag)
    EC.check_demb(tag, dE, idt, smap, vocab, old, accumulate, demb, q)
    check_bits(tag + " rerun", demb_call(dtype, dE, idt, smap, vocab, order, skey, old, accumulate, tag), demb)


@pytest.mark.parametrize("name", list(DEMB_CASES))
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_embed_grad_run_shapes(dtype, name):
    for H in WIDTHS[dtype]:
        for accumulate in (0, 1):
            for exact in (False, True):
                run_demb_case(dtype, H, name, accumulate, exact)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_embed_grad_second_key_block(dtype):
    """T = 8200 over three ids: the sort stages a second block of 8192 keys, and every run spans about 85 chunks"""
    T, V, H = 8200, 3, 8
    idt = input_storage(torch.randint(0, V, (T,), generator=torch.Generator().manual_seed(3)))
    order, skey = sort_call(idt, None, V, "T=8200")
    old = EC.old_rows(V, H, dtype, DEV)
    for exact in (False, True):
        dE, q = EC.exact_rows(T, H, dtype, DEV, 5, amp=2) if exact else (rnd((T, H), dtype, 5), None)
        dE = input_storage(dE)
        for accumulate in (0, 1):
            tag = f"demb {EC.NAME[dtype]} T=8200 acc={accumulate} exact={exact}"
            demb = demb_call(dtype, dE, idt, None, V, order, skey, old, accumulate, tag)
            EC.check_demb(tag, dE, idt, None, V, old, accumulate, demb, q)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_embed_grad_refusals(dtype):
    vn, T, V = VN[dtype], 40, 6
    H = 2 * vn
    idt = input_storage(torch.randint(0, V, (T,), generator=torch.Generator().manual_seed(1)))
    order, skey = sort_call(idt, None, V, "refusals")
    dE = input_storage(rnd((T + 1, H), dtype, 2))
    demb, gd = out_storage((V + 1, H), dtype)
    scr, gs = out_storage((EC.sizes(T, H)[1] + 8,), F32)
    es = dE.element_size()

    def call(dE_=p_(dE), H_=H, ids_=p_(idt), demb_=p_(demb), order_=p_(order), skey_=p_(skey), scr_=p_(scr)):
        return rc("mm_embed_splice_bwd", dt(dtype), dE_, H_, ids_, None, T, None, None, 0, T, None, demb_, V, order_, skey_, scr_, 0)

    assert call(dE_=None) == EC.ERR_ARG
    assert call(ids_=None) == EC.ERR_ARG
    assert call(order_=None) == EC.ERR_ARG
    assert call(skey_=None) == EC.ERR_ARG
    assert call(scr_=None) == EC.ERR_ARG
    assert call(H_=0) == EC.ERR_ARG
    assert call(H_=H - 1) == EC.ERR_ALIGN
    assert call(dE_=p_(dE) + es) == EC.ERR_ALIGN
    assert call(demb_=p_(demb) + es) == EC.ERR_ALIGN
    assert call(scr_=p_(scr) + 4) == EC.ERR_ALIGN
    all_sentinel(gd, gs)


# ---- splice: map, forward, dproj -------------------------------------------------------------------------------------------------------
def splice_problem(T, n_mod, seed):
    """batch rows of S = T / B tokens; sources at random positions (duplicates as they fall, every source index distinct), a few
    with a batch index of -1 or B: their position is outside [0, T) and they are dropped.  0 <= token_range < S throughout."""
    B = 3 if T % 3 == 0 else 1
    S = T // B
    gen = torch.Generator().manual_seed(seed)
    bi = torch.randint(0, B, (n_mod,), generator=gen)
    tr = torch.randint(0, S, (n_mod,), generator=gen)
    if n_mod > 4:
        bi[1::7] = -1
        bi[3::11] = B
        tr[-1], bi[-1], tr[0], bi[0] = tr[2], bi[2], tr[2], bi[2]      # a triple on one position: the last index wins
    return B, S, bi, tr


@pytest.mark.parametrize("n_mod", N_MOD)
@pytest.mark.parametrize("T", SPLICE_T)
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_splice_map_forward_dproj(dtype, T, n_mod):
    H, V = VN[dtype], 9
    B, S, bi, tr = splice_problem(T, n_mod, T + n_mod)
    tag = f"splice {EC.NAME[dtype]} T={T} n_mod={n_mod}"
    bid, trd = (input_storage(bi), input_storage(tr)) if n_mod else (None, None)
    smap, gmap = i32_storage(T)
    assert rc("mm_splice_build_map", p_(bid), p_(trd), n_mod, S, T, p_(smap)) == EC.OK
    sync()
    gmap.verify(tag + " src_map")
    m_ref = EC.build_map_reference(bi.to(DEV), tr.to(DEV), S, T)
    assert bool((smap == m_ref).all()), f"{tag}: src_map (the largest source index wins, positions outside [0, T) are dropped)"
    idc = torch.randint(0, V, (T,), generator=torch.Generator().manual_seed(T))
    idc[::5] = torch.tensor([-1, V, V + 100, -7])[torch.arange(idc[::5].numel()) % 4]      # read row 0, raise the flag
    idt = input_storage(idc)
    emb, proj = input_storage(rnd((V, H), dtype, 1)), input_storage(rnd((max(n_mod, 1), H), dtype, 2))
    out, gout = out_storage((T, H), dtype)
    use_map = n_mod > 0
    assert rc("mm_embed_splice_fwd", dt(dtype), p_(emb), V, H, p_(idt), p_(proj) if use_map else None, p_(smap) if use_map else None, T,
              p_(out)) == EC.OK
    sync()
    gout.verify(tag + " out")
    check_bits(tag + " out", out, EC.splice_fwd_reference(emb, idt, proj, smap if use_map else None))
    if use_map:
        dE = input_storage(rnd((T, H), dtype, 3))
        dproj, gdp = out_storage((n_mod, H), dtype)
        assert rc("mm_embed_splice_bwd", dt(dtype), p_(dE), H, p_(idt), p_(smap), T, p_(bid), p_(trd), n_mod, S, p_(dproj), None, V, None,
                  None, None, 0) == EC.OK
        sync()
        gdp.verify(tag + " dproj")
        check_bits(tag + " dproj", dproj, EC.dproj_reference(dE, bid, trd, S, smap))


def test_splice_refusals():
    T, H, V = 8, 8, 4
    idt = input_storage(torch.zeros(T, dtype=torch.int64))
    emb, proj = input_storage(rnd((V, H), BF, 1)), input_storage(rnd((2, H), BF, 2))
    smap, gmap = i32_storage(T)
    out, gout = out_storage((T, H), BF)
    bi = input_storage(torch.zeros(2, dtype=torch.int64))
    assert rc("mm_embed_splice_fwd", 0, p_(emb), V, H, p_(idt), None, p_(smap), T, p_(out)) == EC.ERR_ARG       # a map without proj
    assert rc("mm_embed_splice_fwd", 0, None, V, H, p_(idt), None, None, T, p_(out)) == EC.ERR_ARG
    assert rc("mm_embed_splice_fwd", 0, p_(emb), V, H, None, None, None, T, p_(out)) == EC.ERR_ARG
    assert rc("mm_embed_splice_fwd", 0, p_(emb), V, H, p_(idt), None, None, T, None) == EC.ERR_ARG
    assert rc("mm_embed_splice_fwd", 0, p_(emb), 0, H, p_(idt), None, None, T, p_(out)) == EC.ERR_ARG
    assert rc("mm_embed_splice_fwd", 0, p_(emb), V, 4, p_(idt), None, None, T, p_(out)) == EC.ERR_ALIGN
    assert rc("mm_embed_splice_fwd", 0, p_(emb) + 2, V, H, p_(idt), None, None, T, p_(out)) == EC.ERR_ALIGN
    assert rc("mm_embed_splice_fwd", 0, p_(emb), V, H, p_(idt), None, None, T, p_(out) + 2) == EC.ERR_ALIGN
    assert rc("mm_embed_splice_fwd", 0, p_(emb), V, H, p_(idt), p_(proj) + 2, p_(smap), T, p_(out)) == EC.ERR_ALIGN
    assert rc("mm_embed_splice_fwd", 0, p_(emb), V, H, p_(idt), None, None, 0, p_(out)) == EC.OK
    assert rc("mm_splice_build_map", p_(bi), p_(bi), 2, T, T, None) == EC.ERR_ARG
    assert rc("mm_splice_build_map", None, p_(bi), 2, T, T, p_(smap)) == EC.ERR_ARG
    assert rc("mm_splice_build_map", p_(bi), None, 2, T, T, p_(smap)) == EC.ERR_ARG
    assert rc("mm_splice_build_map", p_(bi), p_(bi), -1, T, T, p_(smap)) == EC.ERR_ARG
    dproj, gdp = out_storage((2, H), BF)
    dE = input_storage(rnd((T, H), BF, 3))
    assert rc("mm_embed_splice_bwd", 0, p_(dE), H, p_(idt), None, T, p_(bi), p_(bi), 2, T, p_(dproj), None, V, None, None, None,
              0) == EC.ERR_ARG                                                                                    # dproj without the map
    assert rc("mm_embed_splice_bwd", 0, p_(dE), H, p_(idt), p_(smap), T, None, p_(bi), 2, T, p_(dproj), None, V, None, None, None,
              0) == EC.ERR_ARG
    all_sentinel(gmap, gout, gdp)


@pytest.mark.parametrize("T", CHECK_IDS_T)
def test_embed_check_ids_flag_is_sticky(T):
    V = 50
    flag, gf = i32_storage(1)
    flag.zero_()
    good = input_storage(torch.randint(0, V, (T,), generator=torch.Generator().manual_seed(T)))
    for where, bad_id in ((T - 1, V), (0, -1), (T // 2, 2 ** 40)):
        bad = good.clone()
        bad[where] = bad_id
        bad = input_storage(bad)
        flag.zero_()
        assert rc("mm_embed_check_ids", p_(good), T, V, p_(flag)) == EC.OK
        sync()
        assert int(flag[0]) == 0 == EC.ids_flag_reference(good, V)
        assert rc("mm_embed_check_ids", p_(bad), T, V, p_(flag)) == EC.OK
        sync()
        assert int(flag[0]) == 1 == EC.ids_flag_reference(bad, V)
        assert rc("mm_embed_check_ids", p_(good), T, V, p_(flag)) == EC.OK          # a good call does not clear it
        sync()
        assert int(flag[0]) == 1
    bands_intact("flag", gf)
    assert rc("mm_embed_check_ids", None, T, V, p_(flag)) == EC.ERR_ARG
    assert rc("mm_embed_check_ids", p_(good), T, V, None) == EC.ERR_ARG
    assert rc("mm_embed_check_ids", p_(good), T, 0, p_(flag)) == EC.ERR_ARG
    assert rc("mm_embed_check_ids", p_(good), -1, V, p_(flag)) == EC.ERR_ARG


# ---- ViT glue ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kpad", [588, 640])
@pytest.mark.parametrize("hw", [(28, 42), (42, 28), (30, 44)], ids=lambda v: f"{v[0]}x{v[1]}")
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_patchify(dtype, hw, kpad):
    n, ps, (h, w) = 3, 14, hw
    pix = input_storage(rnd((n, 3, h, w), F32, h * w))
    rows = n * (h // ps) * (w // ps)
    out, go = out_storage((rows, kpad), dtype)
    assert rc("mm_patchify", dt(dtype), p_(pix), n, h, w, ps, kpad, p_(out)) == EC.OK
    sync()
    go.verify("patches")
    check_bits(f"patchify {h}x{w} kpad={kpad}", out, EC.patchify_reference(pix, ps, kpad, dtype))
    out2, go2 = out_storage((rows, kpad), dtype)
    assert rc("mm_patchify", dt(dtype), None, n, h, w, ps, kpad, p_(out2)) == EC.ERR_ARG
    assert rc("mm_patchify", dt(dtype), p_(pix), n, h, w, ps, 3 * ps * ps - 1, p_(out2)) == EC.ERR_ARG
    assert rc("mm_patchify", dt(dtype), p_(pix), n, ps - 1, w, ps, kpad, p_(out2)) == EC.ERR_ARG
    assert rc("mm_patchify", dt(dtype), p_(pix), 0, h, w, ps, kpad, p_(out2)) == EC.OK
    all_sentinel(go2)


@pytest.mark.parametrize("D", [8, 72])
@pytest.mark.parametrize("P", [1, 6])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_vit_embed(dtype, n, P, D):
    tag = f"vit_embed {EC.NAME[dtype]} n={n} P={P} D={D}"
    po, cls, pos = (input_storage(rnd(s, dtype, i)) for i, s in enumerate([(n, P, D), (D,), (P + 1, D)]))
    x, gx = out_storage((n, P + 1, D), dtype)
    assert rc("mm_vit_embed_fwd", dt(dtype), p_(po), p_(cls), p_(pos), n, P, D, p_(x)) == EC.OK
    sync()
    gx.verify(tag + " x")
    check_bits(tag + " x", x, EC.vit_embed_fwd_reference(po, cls, pos))
    dx = rnd((n, P + 1, D), dtype, 9)                                    # not integers: the order of the adds shows
    dx = input_storage(EC.plant_order_triple(dx) if n >= 3 else dx)
    old_pos, old_cls = rnd((P + 1, D), dtype, 10), rnd((D,), dtype, 11)
    for accumulate in (0, 1):
        for skip in (None, "dpatch", "dcls", "dpos"):
            outs = {"dpatch": out_storage((n, P, D), dtype), "dcls": out_storage((D,), dtype), "dpos": out_storage((P + 1, D), dtype)}
            if accumulate:                                               # without `accumulate` the old contents are sentinels: not read
                outs["dcls"][0].copy_(old_cls)
                outs["dpos"][0].copy_(old_pos)
            a = {k: (None if k == skip else p_(v[0])) for k, v in outs.items()}
            assert rc("mm_vit_embed_bwd", dt(dtype), p_(dx), n, P, D, a["dpatch"], a["dcls"], a["dpos"], accumulate) == EC.OK
            sync()
            want = dict(zip(("dpatch", "dcls", "dpos"), EC.vit_embed_bwd_reference(dx, old_pos, old_cls, accumulate)))
            for k, (v, g) in outs.items():
                if k == skip:
                    if not (accumulate and k != "dpatch"):
                        all_sentinel(g)
                    else:
                        check_bits(f"{tag} {k} not written", v, old_cls if k == "dcls" else old_pos)
                else:
                    g.verify(f"{tag} {k}")
                    check_bits(f"{tag} acc={accumulate} without {skip}: {k}", v, want[k])
    assert rc("mm_vit_embed_fwd", dt(dtype), None, p_(cls), p_(pos), n, P, D, p_(x)) == EC.ERR_ARG
    assert rc("mm_vit_embed_fwd", dt(dtype), p_(po), p_(cls), p_(pos), n, 0, D, p_(x)) == EC.ERR_ARG
    assert rc("mm_vit_embed_bwd", dt(dtype), None, n, P, D, None, None, None, 0) == EC.ERR_ARG
    assert rc("mm_vit_embed_bwd", dt(dtype), p_(dx), n, P, 0, None, None, None, 0) == EC.ERR_ARG


# ---- row movers ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_rows_select(dtype):
    vn = VN[dtype]
    for n_src, n_dst, D, ld_src, ld_dst in [(5, 7, vn, 2 * vn, 3 * vn), (40, 33, 72, 80, 72), (3, 1100, 72, 72, 88), (9, 4, 2 * vn, 2 * vn, 2 * vn)]:
        tag = f"rows_select {EC.NAME[dtype]} {n_src}->{n_dst} D={D} ld={ld_src},{ld_dst}"
        src = sentinel_fill(torch.empty(n_src, ld_src, dtype=dtype, device=DEV))      # the pad columns of src are not read
        src[:, :D] = rnd((n_src, D), dtype, n_dst)
        idx = torch.randint(0, n_src, (n_dst,), generator=torch.Generator().manual_seed(n_dst)).to(torch.int32)
        idx[::3] = torch.tensor([-1, n_src, n_src + 5])[torch.arange(idx[::3].numel()) % 3].to(torch.int32)   # zero rows
        idx = input_storage(idx)
        dst, gd = out_storage((n_dst, D), dtype, ld=ld_dst)
        assert rc("mm_rows_select", dt(dtype), p_(src), ld_src, p_(idx), n_src, n_dst, D, p_(dst), ld_dst) == EC.OK
        sync()
        gd.verify(tag)                                                                # the pad columns of dst stay untouched
        check_bits(tag, dst, EC.rows_select_reference(src[:, :D], idx, n_src))
    dst, gd = out_storage((4, 2 * vn), dtype)
    a = (p_(src), 2 * vn, p_(idx), 9, 4, 2 * vn, p_(dst), 2 * vn)
    rep = lambda i, v: a[:i] + (v,) + a[i + 1:]
    assert rc("mm_rows_select", dt(dtype), *rep(4, 0)) == EC.OK                       # n_dst = 0
    assert rc("mm_rows_select", dt(dtype), *rep(0, None)) == EC.ERR_ARG
    assert rc("mm_rows_select", dt(dtype), *rep(2, None)) == EC.ERR_ARG
    assert rc("mm_rows_select", dt(dtype), *rep(6, None)) == EC.ERR_ARG
    assert rc("mm_rows_select", dt(dtype), *rep(1, vn)) == EC.ERR_ALIGN                # ld_src < D
    assert rc("mm_rows_select", dt(dtype), *rep(7, vn)) == EC.ERR_ALIGN                # ld_dst < D
    assert rc("mm_rows_select", dt(dtype), *rep(5, 2 * vn - 1)) == EC.ERR_ALIGN
    assert rc("mm_rows_select", dt(dtype), *rep(6, p_(dst) + dst.element_size())) == EC.ERR_ALIGN
    all_sentinel(gd)


@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_drop_cls(dtype):
    for n, P, D in [(1, 1, VN[dtype]), (3, 6, 72), (2, 577, 8)]:
        tag = f"drop_cls {EC.NAME[dtype]} n={n} P={P} D={D}"
        x = input_storage(rnd((n, P + 1, D), dtype, P))
        y, gy = out_storage((n, P, D), dtype)
        assert rc("mm_drop_cls_fwd", dt(dtype), p_(x), n, P, D, p_(y)) == EC.OK
        d = input_storage(rnd((n, P, D), dtype, P + 1))
        dxx, gdx = out_storage((n, P + 1, D), dtype)
        assert rc("mm_drop_cls_bwd", dt(dtype), p_(d), n, P, D, p_(dxx)) == EC.OK
        sync()
        gy.verify(tag + " fwd")
        gdx.verify(tag + " bwd")
        check_bits(tag + " fwd", y, EC.drop_cls_fwd_reference(x))
        check_bits(tag + " bwd", dxx, EC.drop_cls_bwd_reference(d))
    y, gy = out_storage((n, P, D), dtype)
    for entry in ("mm_drop_cls_fwd", "mm_drop_cls_bwd"):
        assert rc(entry, dt(dtype), None, n, P, D, p_(y)) == EC.ERR_ARG
        assert rc(entry, dt(dtype), p_(x), n, P, D, None) == EC.ERR_ARG
        assert rc(entry, dt(dtype), p_(x), n, 0, D, p_(y)) == EC.ERR_ARG
        assert rc(entry, dt(dtype), p_(x), n, P, D - 1, p_(y)) == EC.ERR_ALIGN
        assert rc(entry, dt(dtype), p_(x) + x.element_size(), n, P, D, p_(y)) == EC.ERR_ALIGN
        assert rc(entry, dt(dtype), p_(x), 0, P, D, p_(y)) == EC.OK
    all_sentinel(gy)


@pytest.mark.parametrize("d,dpad", [(72, 128), (64, 64), (8, 16)])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_head_pad(dtype, d, dpad):
    rows, nh = 5, 3
    tag = f"head_pad {EC.NAME[dtype]} {d}->{dpad}"
    x = input_storage(rnd((rows, nh, d), dtype, d))
    wide, gw = out_storage((rows, nh, dpad), dtype)
    assert rc("mm_head_pad", dt(dtype), p_(x), rows, nh, d, dpad, p_(wide), 0) == EC.OK
    sync()
    gw.verify(tag)
    check_bits(tag, wide, EC.head_pad_reference(x, d, dpad, False))
    w_in = sentinel_fill(torch.empty(rows, nh, dpad, dtype=dtype, device=DEV))          # the pad of the wide side is not read back
    w_in[..., :d] = x
    back, gb = out_storage((rows, nh, d), dtype)
    assert rc("mm_head_pad", dt(dtype), p_(w_in), rows, nh, d, dpad, p_(back), 1) == EC.OK
    sync()
    gb.verify(tag + " inverse")
    check_bits(tag + " inverse", back, x)
    o, go = out_storage((rows, nh, dpad), dtype)
    assert rc("mm_head_pad", dt(dtype), p_(x), rows, nh, d, d - VN[dtype], p_(o), 0) == EC.ERR_ARG          # dpad < d
    assert rc("mm_head_pad", dt(dtype), None, rows, nh, d, dpad, p_(o), 0) == EC.ERR_ARG
    assert rc("mm_head_pad", 7, p_(x), rows, nh, d, dpad, p_(o), 0) == EC.ERR_UNSUPPORTED
    assert rc("mm_head_pad", dt(dtype), p_(x), rows, nh, d - 1, dpad, p_(o), 0) == EC.ERR_ALIGN
    assert rc("mm_head_pad", dt(dtype), p_(x), 0, nh, d, dpad, p_(o), 0) == EC.OK
    all_sentinel(go)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=ids)
def test_bcast_add(dtype, n):
    for L in (VN[dtype], 16 * 72):
        x, b = input_storage(rnd((n, L), dtype, L)), input_storage(rnd((L,), dtype, L + 1))
        y, gy = out_storage((n, L), dtype)
        assert rc("mm_bcast_add", dt(dtype), p_(x), p_(b), n, L, p_(y)) == EC.OK
        sync()
        gy.verify("bcast_add")
        check_bits(f"bcast_add {EC.NAME[dtype]} n={n} L={L}", y, EC.bcast_add_reference(x, b))
    y, gy = out_storage((n, L), dtype)
    assert rc("mm_bcast_add", 7, p_(x), p_(b), n, L, p_(y)) == EC.ERR_UNSUPPORTED
    assert rc("mm_bcast_add", dt(dtype), None, p_(b), n, L, p_(y)) == EC.ERR_ARG
    assert rc("mm_bcast_add", dt(dtype), p_(x), p_(b), n, 0, p_(y)) == EC.ERR_ARG
    assert rc("mm_bcast_add", dt(dtype), p_(x), p_(b), n, L - 1, p_(y)) == EC.ERR_ALIGN
    assert rc("mm_bcast_add", dt(dtype), p_(x), p_(b) + x.element_size(), n, L, p_(y)) == EC.ERR_ALIGN
    assert rc("mm_bcast_add", dt(dtype), p_(x), p_(b), 0, L, p_(y)) == EC.OK
    all_sentinel(gy)

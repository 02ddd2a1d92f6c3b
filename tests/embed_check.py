"""Embedding / splice / ViT-glue checker (csrc/mm_embed.hip): an fp64 reference with a per-row error scale for the embedding
gradient, and bit references for everything else -- the sort, the splice map, the row movers and the single-rounding adds.

Embedding gradient (mm_embed_sort + mm_embed_splice_bwd).  A token is VALID when it is not under a splice (src_map[t] < 0) and
0 <= id < vocab.  The reference is an fp64 index_add_ over the valid tokens.  The kernels sort the tokens by id, cut the sorted
positions into chunks of 32, sum each run of equal ids inside a chunk in fp32 in token order, and join the pieces of a run that
crosses chunks in ascending chunk order.  So a row touched by n tokens whose run starts at sorted position s has
  depth_row = min(n, 32) + (chunks the run spans - 1)
additions on its longest path, and
  E_row = depth_row * sum |dE_t| [U32] + |ref| [u of the output] + |old| [u] when accumulating.
A row no valid token touches keeps its previous BITS (E = 0): demb is filled with finite, recognisable values before the call,
not with the NaN sentinel, and only the bands around it are guarded.  The exact family (`exact_rows`): dE = small integers times a
power of two, below 2^24 quanta per row, so every fp32 partial sum is exact in any order and demb == RNE_T(sum) bit for bit -- the
test that catches a token dropped or counted twice at a chunk boundary.

`runs(lengths)` builds ids whose sorted run lengths are given, shuffled with a fixed seed, to place runs on chunk edges by hand.

Sort: order[:T] is the stable sort by (key, t) with key = id, or 0x7fffffff for a token that is not valid; skey[:Tpad] the sorted
keys followed by 0x7fffffff up to Tpad = (ceil(T / 32) + 1) * 32; order[T:] is not written.

c is in `C` (bf16, f32): the smallest power of two >= 2x the worst err / (u E) measured on the MI355X over
tests/test_embed_contract_gpu.py (MM_EMBED_RATIO_LOG writes the ratios)."""
import torch

from tests.kernel_check import U, U32, RatioLog, check_bits, check_bound

BF, F32 = torch.bfloat16, torch.float32
VN = {BF: 8, F32: 4}
NAME = {BF: "bf16", F32: "f32"}
OK, ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -3
R = 32                                # EMB_R: sorted positions per chunk
INVALID = 0x7FFFFFFF
RATIOS = RatioLog("MM_EMBED_RATIO_LOG")

# c (bf16, f32): the smallest power of two >= 2x the worst err / (u E) measured on the MI355X; the measured ratios in the comment
C = {
    "embed.demb": (2.0, 1.0),         # 0.996, 0.4997 (0.550 over the larger shapes of tests/test_kernels_gpu.py)
}
PREFIX = [""]                         # tests/test_embed_check_cpu.py records its emulation under "emulation." instead


def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def sizes(T, H):
    """mm_embed_sort_sizes: (order / skey elements, scratch floats)"""
    nch = -(-T // R)
    return (nch + 1) * R, nch * 2 * H


# ---- key structure -----------------------------------------------------------------------------------------------------------------
def runs(lengths, invalid_tail=0, seed=0):
    """-> (ids [T] int64, vocab): run i of the sorted order has lengths[i] tokens of id 1 + 2 i (the even rows stay untouched);
    `invalid_tail` more tokens are out of range (alternately -1 and vocab + 1).  Positions are shuffled with a fixed seed."""
    vocab = 2 * len(lengths) + 2
    ids = [1 + 2 * i for i, n in enumerate(lengths) for _ in range(n)]
    ids += [-1 if j % 2 == 0 else vocab + 1 for j in range(invalid_tail)]
    ids = torch.tensor(ids, dtype=torch.int64)
    return ids[torch.randperm(ids.numel(), generator=_gen("cpu", seed))], vocab


def valid_mask(ids, src_map, vocab):
    ok = (ids >= 0) & (ids < vocab)
    return ok & (src_map < 0) if src_map is not None else ok


def keys(ids, src_map, vocab):
    return torch.where(valid_mask(ids, src_map, vocab), ids, torch.full_like(ids, INVALID)).to(torch.int32)


def sort_reference(ids, src_map, vocab):
    """-> (order [T] int32, skey [Tpad] int32)"""
    T = ids.numel()
    k = keys(ids, src_map, vocab)
    sk, order = torch.sort(k, stable=True)
    pad = torch.full((sizes(T, 1)[0] - T,), INVALID, dtype=torch.int32, device=ids.device)
    return order.to(torch.int32), torch.cat([sk, pad])


# ---- embedding gradient ------------------------------------------------------------------------------------------------------------
def row_depth(ids, src_map, vocab):
    """[vocab] float64: additions on the longest path of each row (0 for an untouched row), and the token count per row"""
    ok = valid_mask(ids, src_map, vocab)
    cnt = torch.bincount(ids[ok], minlength=vocab)
    start = torch.cumsum(cnt, 0) - cnt
    last = start + cnt - 1
    spans = torch.div(last, R, rounding_mode="floor") - torch.div(start, R, rounding_mode="floor") + 1
    depth = torch.clamp(cnt, max=R) + spans - 1
    return torch.where(cnt > 0, depth, torch.zeros_like(depth)).double(), cnt


def demb_reference(dE, ids, src_map, vocab, old, accumulate):
    """-> (ref [V, H], E [V, H] in u of dE's dtype, touched [V] bool).  old: what demb held before the call (the output's dtype)."""
    dtype = dE.dtype
    ok = valid_mask(ids, src_map, vocab)
    d64 = dE.double()[ok]
    V, H = old.shape
    s = torch.zeros(V, H, dtype=torch.float64, device=dE.device).index_add_(0, ids[ok], d64)
    mag = torch.zeros_like(s).index_add_(0, ids[ok], d64.abs())
    depth, cnt = row_depth(ids, src_map, vocab)
    touched = cnt > 0
    o64 = old.double()
    ref = torch.where(touched[:, None], s + o64 if accumulate else s, o64)
    E = depth[:, None] * mag * (U32 / U[dtype]) + ref.abs() + (o64.abs() if accumulate else 0.0)
    return ref, torch.where(touched[:, None], E, torch.zeros_like(E)), touched


def exact_rows(T, H, dtype, device, seed, amp=4, shift=-3):
    """dE = integers in [-amp, amp] times 2^shift -> (dE, quantum)"""
    x = torch.randint(-amp, amp + 1, (T, H), generator=_gen(device, seed), device=device).double() * 2.0 ** shift
    return x.to(dtype), 2.0 ** shift


def old_rows(V, H, dtype, device, quantum=0.125):
    """finite, recognisable previous contents: row r, column j holds (3 r + j % 5 - 2) quanta (exact in bf16 for the rows used)"""
    r = torch.arange(V, device=device, dtype=torch.float64)[:, None]
    j = torch.arange(H, device=device, dtype=torch.float64)[None, :]
    out = ((3 * r + j % 5 - 2) * quantum).to(dtype)
    assert bool((out.double() == (3 * r + j % 5 - 2) * quantum).all())
    return out


def check_demb(tag, dE, ids, src_map, vocab, old, accumulate, got, quantum=None):
    """the bound per element, untouched rows bit for bit and, for the exact family (quantum given), every row bit for bit"""
    dtype = dE.dtype
    ref, E, touched = demb_reference(dE, ids, src_map, vocab, old, accumulate)
    check_bits(tag + " untouched rows keep their bits", got[~touched], old[~touched])
    worst = check_bound(tag + " demb", got, ref, E, C["embed.demb"][0 if dtype == BF else 1], U[dtype],
                        key=f"{PREFIX[0]}embed.demb.{NAME[dtype]}", log=RATIOS)
    if quantum is not None:
        ok = valid_mask(ids, src_map, vocab)
        mag = torch.zeros(old.shape, dtype=torch.float64, device=dE.device).index_add_(0, ids[ok], dE.double()[ok].abs())
        mag = mag + (old.double().abs() if accumulate else 0.0)
        assert float(mag.max()) / quantum < 2.0 ** 24, "exact family out of range"
        check_bits(tag + " demb (exact family)", got, ref.float().to(dtype), zero_sign=False)
    return worst


# ---- exact movers ------------------------------------------------------------------------------------------------------------------
def build_map_reference(bi, tr, S, T):
    """src_map [T] int32: the LARGEST source index that lands on a position wins; positions outside [0, T) are dropped"""
    m = torch.full((T,), -1, dtype=torch.int64, device=bi.device)
    pos = bi * S + tr
    ok = (pos >= 0) & (pos < T)
    idx = torch.arange(bi.numel(), device=bi.device)
    if bool(ok.any()):
        m.scatter_reduce_(0, pos[ok], idx[ok], "amax")
    return m.to(torch.int32)


def splice_fwd_reference(emb, ids, proj, src_map):
    """out [T, H]: proj[src_map[t]] where src_map[t] >= 0, else emb[id] (row 0 for an id out of range)"""
    V = emb.shape[0]
    safe = torch.where((ids >= 0) & (ids < V), ids, torch.zeros_like(ids))
    out = emb[safe]
    if src_map is not None:
        sp = src_map >= 0
        out = torch.where(sp[:, None], proj[src_map.clamp(min=0).long()], out)
    return out


def ids_flag_reference(ids, vocab):
    return int(bool(((ids < 0) | (ids >= vocab)).any()))


def dproj_reference(dE, bi, tr, S, src_map):
    """dproj [n_mod, H]: dE[pos] for the source that owns pos; a lost duplicate or a dropped position gets exactly zero"""
    T = dE.shape[0]
    pos = bi * S + tr
    ok = (pos >= 0) & (pos < T)
    idx = torch.arange(bi.numel(), device=bi.device)
    live = ok & (src_map[pos.clamp(0, max(T - 1, 0))].long() == idx)
    return torch.where(live[:, None], dE[pos.clamp(0, max(T - 1, 0))], torch.zeros((), dtype=dE.dtype, device=dE.device))


def rows_select_reference(src, idx, n_src):
    """dst[r] = src[idx[r]], or a zero row where idx[r] is outside [0, n_src)"""
    ok = (idx >= 0) & (idx < n_src)
    return torch.where(ok[:, None], src[idx.clamp(0, max(n_src - 1, 0)).long()], torch.zeros((), dtype=src.dtype, device=src.device))


def drop_cls_fwd_reference(x):
    return x[:, 1:].contiguous()


def drop_cls_bwd_reference(d):
    return torch.cat([torch.zeros_like(d[:, :1]), d], 1)


def head_pad_reference(x, d, dpad, inverse):
    """[rows, nheads, d] -> [rows, nheads, dpad] with zeros behind d, or back"""
    if inverse:
        return x[..., :d].contiguous()
    return torch.cat([x, torch.zeros(*x.shape[:-1], dpad - d, dtype=x.dtype, device=x.device)], -1)


def patchify_reference(pix, ps, kpad, dtype):
    """pix [n, 3, h, w] f32 -> [n * gh * g, kpad]: patch (py, px) in row py * g + px, column c ps^2 + y ps + x, one rounding to
    the dtype, zeros in [3 ps^2, kpad); a ragged border (h % ps rows, w % ps columns) is dropped"""
    n, _, h, w = pix.shape
    gh, g = h // ps, w // ps
    x = pix[:, :, :gh * ps, :g * ps].reshape(n, 3, gh, ps, g, ps).permute(0, 2, 4, 1, 3, 5).reshape(n * gh * g, 3 * ps * ps)
    return torch.cat([x.to(dtype), torch.zeros(n * gh * g, kpad - 3 * ps * ps, dtype=dtype, device=pix.device)], 1)


def bcast_add_reference(x, b):
    """x [n, L] + b [L]: the fp32 add rounded once (nothing to contract)"""
    return (x.float() + b.float()[None]).to(x.dtype)


def vit_embed_fwd_reference(patch_out, cls, pos):
    """x [n, 1 + P, D] = cat(cls, patch_out) + pos, the fp32 add rounded once"""
    n = patch_out.shape[0]
    base = torch.cat([cls.float().expand(n, 1, -1), patch_out.float()], 1)
    return (base + pos.float()[None]).to(patch_out.dtype)


def plant_order_triple(dx):
    """three bf16 values whose fp32 sum lands on either side of a bf16 tie depending on the order of the adds, written to the
    first element of the CLS row and of the last row of images 0, 1, 2: random bf16 data alone almost never tells the order, since
    the sum of three bf16 values is usually exact in fp32 or far from a tie."""
    assert dx.shape[0] >= 3
    t = torch.tensor([float.fromhex("0x1.a4p+0"), float.fromhex("0x1.8p-7"), float.fromhex("-0x1.02p-24")]).to(dx.dtype).to(dx.device)
    dx[:3, 0, 0] = t
    dx[:3, -1, 0] = -t
    return dx


def vit_embed_bwd_reference(dx, old_pos, old_cls, accumulate):
    """-> (dpatch, dcls, dpos): dpatch a bit copy of dx[:, 1:]; dpos / dcls the SEQUENTIAL fp32 sum over the images in index order
    (adds only), + old when accumulating, rounded once"""
    s = torch.zeros_like(dx[0], dtype=F32)
    for i in range(dx.shape[0]):
        s = s + dx[i].float()
    dpos = (s + (old_pos.float() if accumulate else 0.0)).to(dx.dtype)
    dcls = (s[0] + (old_cls.float() if accumulate else 0.0)).to(dx.dtype)
    return dx[:, 1:].contiguous(), dcls, dpos

"""mm_attn_decode_shared (n samples per prompt over one copy of the prompt's keys) on top of tests/attn_check.py: the cases, the
operands as generate passes them, the materialised concatenation that mm_attn_decode must reproduce bit for bit, and the guarded
launch."""
import torch

from tests import attn_check as AC
from tests.kernel_check import dt, ptr, sentinel_fill

BF16 = torch.bfloat16
D = 128


def shared_splits(B, n, Hkv, Skv, wgs=AC.DECODE_WGS):
    """mm_attn_decode_shared_splits: ceil(T / (B ceil(n / 4) Hkv)) slices with T = ceil(2 wgs / 3) -- the workgroups of G = 4, two per
    CU where the slice kernel holds three -- at least 64 keys each."""
    return max(1, min(-(-(-(-2 * wgs // 3)) // (B * -(-n // 4) * Hkv)), -(-Skv // 64)))


def case(B, Hq, Hkv, n, Sp, Ss, ns, mask=None):
    """ns: "lib" = the library's split count, or an explicit nsplit; mask: a kind of attn_check.decode_mask over the PREFIX"""
    return dict(B=B, Hq=Hq, Hkv=Hkv, n=n, Sp=Sp, Ss=Ss, ns=ns, mask=mask)


def case_id(c):
    return f"B{c['B']}-n{c['n']}-p{c['Sp']}-s{c['Ss']}-h{c['Hq']}x{c['Hkv']}-{c['mask'] or 'nomask'}-ns{c['ns']}"


def nsplit(c):
    return shared_splits(c["B"], c["n"], c["Hkv"], c["Sp"] + c["Ss"]) if c["ns"] == "lib" else int(c["ns"])


def slice_kinds(Sp, Ss, ns):
    """where the slices of the concatenation lie: a set of 'prefix', 'straddle', 'suffix', 'empty'"""
    Skv = Sp + Ss
    chunk = AC.decode_chunk(Skv, ns)
    kinds = set()
    for s in range(ns):
        lo, hi = s * chunk, min(Skv, (s + 1) * chunk)
        kinds.add("empty" if lo >= Skv else "prefix" if hi <= Sp else "suffix" if lo >= Sp else "straddle")
    return kinds


def operands(c, mask, seed=1):
    """q [B n, Hq, D], prefix kp / vp [B, Sp, Hkv, D], suffix ks / vs [B n, Ss, Hkv, D] in bf16 (CPU).  Masked prefix keys hold finite
    values about 1e3 times the visible ones (attn_check.decode_operands)."""
    B, n, Hq, Hkv, Sp, Ss = c["B"], c["n"], c["Hq"], c["Hkv"], c["Sp"], c["Ss"]
    g = torch.Generator().manual_seed(seed + 13 * Sp + 7 * Ss + Hq + 31 * n)
    q = torch.randn(B * n, Hq, D, generator=g)
    kp, vp = torch.randn(B, Sp, Hkv, D, generator=g), torch.randn(B, Sp, Hkv, D, generator=g)
    ks, vs = torch.randn(B * n, Ss, Hkv, D, generator=g), torch.randn(B * n, Ss, Hkv, D, generator=g)
    if mask is not None:
        big = torch.where(mask == 0, 1000.0, 1.0)[:, :, None, None]
        kp, vp = kp * big, vp * big
    return tuple(t.to(BF16) for t in (q, kp, vp, ks, vs))


def materialise(kp, vp, ks, vs, mask, n):
    """the cache of B n rows that holds every prompt n times: k / v [B n, Sp + Ss, Hkv, D] and the mask with ones over the suffix"""
    k = torch.cat([kp.repeat_interleave(n, 0), ks], 1)
    v = torch.cat([vp.repeat_interleave(n, 0), vs], 1)
    m = None if mask is None else torch.cat([mask.repeat_interleave(n, 0), torch.ones(ks.shape[0], ks.shape[1], dtype=mask.dtype)], 1)
    return k, v, m


def place(q, kp, vp, ks, vs, device="cuda"):
    """The operands as generate() passes them (attn_check.decode_place): q a strided view into a fused q|k|v row, every cache a view
    [:, :S] of a longer buffer whose tail holds the sentinel NaN."""
    R, Hq, _ = q.shape
    Hkv = kp.shape[2]
    row = sentinel_fill(torch.empty(R, (Hq + 2 * Hkv) * D, dtype=q.dtype))
    row[:, :Hq * D] = q.reshape(R, Hq * D)

    def longer(t):
        c = sentinel_fill(torch.empty(t.shape[0], t.shape[1] + 11, Hkv, D, dtype=t.dtype))
        c[:, :t.shape[1]] = t
        return c.to(device)[:, :t.shape[1]]

    return (row.to(device)[:, :Hq * D].view(R, Hq, D),) + tuple(longer(t) for t in (kp, vp, ks, vs))


def run(q, kp, vp, ks, vs, n, key_mask, scale, ns):
    """mm_attn_decode_shared with out and the workspace inside guarded storages (every slice's record must be written)
    -> (out [B n, Hq, D], [guards])"""
    from multimeditron_amd._lib import call
    R, Hq, _ = q.shape
    B, Sp, Hkv = kp.shape[0], kp.shape[1], kp.shape[2]
    out, ws, guards = AC.decode_buffers(R, Hq, D, ns, q.device)
    s3 = AC._s3
    call("mm_attn_decode_shared", dt(q.dtype), ptr(q), ptr(kp), ptr(vp), ptr(ks), ptr(vs), B, n, Sp, ks.shape[1], Hq, Hkv, D,
         q.stride(0), q.stride(1), *s3(kp), *s3(vp), *s3(ks), *s3(vs), ptr(key_mask), float(scale), ptr(out), ptr(ws), ns,
         torch.cuda.current_stream().cuda_stream)
    return out, guards

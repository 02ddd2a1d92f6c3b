"""mm_attn_decode_beam through the C ABI: mm_attn_decode_shared whose suffix keys are read through an ancestor table
(include/mm_hip.h).  Kernel: attn_decode_beam128_kernel<G> -- the body of attn_decode_shared128_kernel<G> with the suffix row looked up
and clamped -- + attn_decode_merge_kernel.

Every case runs four tables (identity, random inside each prompt, every row of a prompt pointing at one row, and the random one with
a tenth of its entries outside the prompt's rows: -1, base - 1, base + n, 2^20, INT32_MIN -- the kernel clamps an entry into
[base, base + n) before it forms an address, so the suffix it must read is the one gathered through the CLAMPED table) and is held to
  (a) the bits of mm_attn_decode_shared on the GATHERED suffix ks'[r, t] = ks[anc[t, r], t] with the same nsplit (for the identity
      table: on ks itself);
  (b) two runs giving the same bits;
  (c) intact guards around out and the workspace, every slice's record written.
Operands sit as generate passes them (tests/attn_shared_check.place); the table is a view of a wider int32 buffer whose padding
columns hold rows far outside the cache (never read: the kernel reads column r < B n only)."""
import pytest
import torch

from tests import attn_check as AC
from tests import attn_shared_check as SC
from tests.kernel_check import check_bits, dt, lib, ptr

pytestmark = pytest.mark.gpu


def _cases():
    out, i = [], 0
    sps, sss, nss = (1, 70, 150), (1, 17, 40), (1, 3, "lib")
    for Hq, Hkv in ((2, 2), (4, 2), (4, 1)):                       # G = 1, 2, 4
        G = Hq // Hkv
        for n in (16 // G, 16 // G + 1, 3):                        # a full column tile, a second tile, a partial one
            # every (Sp, Ss, nsplit) value with every G, every pair of values at least once over the nine cases of a G
            out.append(SC.case(2, Hq, Hkv, n, sps[i % 3], sss[(i // 3 + i) % 3], nss[(i // 3 + 2 * i) % 3], "leftpad"))
            i += 1
    return out


CASES = _cases()


def test_the_cases_cover_what_the_issue_lists():
    for G in (1, 2, 4):
        cs = [c for c in CASES if c["Hq"] // c["Hkv"] == G]
        assert {c["n"] for c in cs} == {16 // G, 16 // G + 1, 3}
        assert {c["Sp"] for c in cs} == {1, 70, 150} and {c["Ss"] for c in cs} == {1, 17, 40} and {c["ns"] for c in cs} == {1, 3, "lib"}
    assert all(c["B"] == 2 and c["mask"] == "leftpad" for c in CASES)
    # the out-of-range table: every case has entries outside its prompt's rows; every kind occurs below and above both prompts
    kinds = set()
    for c in CASES:
        B, n, Ss = c["B"], c["n"], c["Ss"]
        t = tables(B, n, Ss, 5 + c["Sp"] + Ss + n)
        assert set(t) == {"identity", "random", "one-row", "out-of-range"}
        oor, base = t["out-of-range"], (torch.arange(B * n) // n * n)[None, :].expand(Ss, B * n)
        out = (oor < base) | (oor >= base + n)
        assert bool(out.any()) and torch.equal(oor[~out], t["random"][~out]) and not torch.equal(clamped(oor, B, n), oor)
        for v, b0 in zip(oor[out].tolist(), base[out].tolist()):
            kinds.add(v if v in (-1, 1 << 20, -(1 << 31)) and not (v == -1 and b0 == 0) else ("below" if v < b0 else "above", b0 > 0))
    assert kinds >= {1 << 20, -(1 << 31), -1, ("below", False), ("below", True), ("above", False), ("above", True)}, kinds


def tables(B, n, Ss, seed):
    g = torch.Generator().manual_seed(seed)
    R = B * n
    base = (torch.arange(R) // n * n)[None, :]
    ident = torch.arange(R)[None, :].expand(Ss, R)
    rand = base + torch.randint(0, n, (Ss, R), generator=g)
    one = (base + (n - 1)).expand(Ss, R)
    hit = torch.rand(Ss, R, generator=g) < 0.1
    hit.view(-1)[int(torch.randint(0, Ss * R, (1,), generator=g))] = True          # at least one, however small the table
    kind = ((hit.view(-1).long().cumsum(0) - 1) % 5).view(Ss, R)
    vals = (torch.full((Ss, R), -1), (base - 1).expand(Ss, R), (base + n).expand(Ss, R), torch.full((Ss, R), 1 << 20),
            torch.full((Ss, R), -(1 << 31)))
    oor = rand.clone()
    for k, v in enumerate(vals):
        oor = torch.where(hit & (kind == k), v, oor)
    assert bool(((oor < base) | (oor >= base + n)).any())
    return {"identity": ident, "random": rand, "one-row": one, "out-of-range": oor}


def clamped(tab, B, n):
    base = (torch.arange(B * n) // n * n)[None, :]
    return torch.minimum(torch.maximum(tab, base), base + n - 1)


def run_beam(q, kp, vp, ks, vs, n, key_mask, scale, ns, anc):
    from multimeditron_amd._lib import call
    R, Hq, _ = q.shape
    B, Sp, Hkv = kp.shape[0], kp.shape[1], kp.shape[2]
    out, ws, guards = AC.decode_buffers(R, Hq, SC.D, ns, q.device)
    s3 = AC._s3
    call("mm_attn_decode_beam", dt(q.dtype), ptr(q), ptr(kp), ptr(vp), ptr(ks), ptr(vs), B, n, Sp, ks.shape[1], Hq, Hkv, SC.D,
         q.stride(0), q.stride(1), *s3(kp), *s3(vp), *s3(ks), *s3(vs), ptr(key_mask), float(scale), ptr(out), ptr(ws), ns, ptr(anc),
         anc.stride(0), torch.cuda.current_stream().cuda_stream)
    return out, guards


@pytest.mark.parametrize("c", CASES, ids=[SC.case_id(c) for c in CASES])
def test_beam_decode_contract(c):
    B, n, Hkv, Sp, Ss = c["B"], c["n"], c["Hkv"], c["Sp"], c["Ss"]
    R = B * n
    ns = SC.nsplit(c)
    if c["ns"] == "lib":
        assert lib().mm_attn_decode_shared_splits(B, n, Hkv, Sp + Ss) == ns
    mask = AC.decode_mask(c["mask"], B, Sp, ns)
    q, kp, vp, ks, vs = SC.operands(c, mask)
    scale = SC.D ** -0.5
    mg = mask.cuda()
    qd, kpd, vpd, ksd, vsd = SC.place(q, kp, vp, ks, vs)
    guards, outs = [], {}
    t_idx = torch.arange(Ss)[:, None]
    for name, tab in tables(B, n, Ss, 5 + Sp + Ss + n).items():
        wide = torch.full((Ss + 2, R + 3), 1 << 20, dtype=torch.int32)         # padding columns and rows: far outside the cache
        wide[:Ss, :R] = tab
        anc = wide.cuda()[:Ss, :R]
        got, g1 = run_beam(qd, kpd, vpd, ksd, vsd, n, mg, scale, ns, anc)
        again, g2 = run_beam(qd, kpd, vpd, ksd, vsd, n, mg, scale, ns, anc)
        # ks'[r, t] = ks[anc[t, r], t], every entry clamped into its prompt's rows as the kernel reads it
        tab = clamped(tab, B, n)
        ksg, vsg = ks[tab, t_idx].transpose(0, 1).contiguous(), vs[tab, t_idx].transpose(0, 1).contiguous()
        if name == "identity":
            assert torch.equal(ksg.view(torch.int16), ks.view(torch.int16))
        _, _, _, ksgd, vsgd = SC.place(q, kp, vp, ksg, vsg)
        want, g3 = SC.run(qd, kpd, vpd, ksgd, vsgd, n, mg, scale, ns)
        torch.cuda.synchronize()
        AC.verify_guards(g1 + g2 + g3)                                          # (c)
        check_bits(f"{name}: beam == mm_attn_decode_shared on the gathered suffix", got, want)      # (a)
        check_bits(f"{name}: rerun", again, got)                                # (b)
        assert bool(torch.isfinite(got.float()).all())
        outs[name] = got
    if n > 1 and Ss > 1:
        assert not torch.equal(outs["identity"].view(torch.int16), outs["one-row"].view(torch.int16))       # the table is read

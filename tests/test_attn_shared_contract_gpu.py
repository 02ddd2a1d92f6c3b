"""mm_attn_decode_shared through the C ABI: n samples per prompt over ONE copy of the prompt's keys (include/mm_hip.h).

Kernel: attn_decode_shared128_kernel<G> (16 / G samples per 16-column MFMA tile; a 16-key block in the prefix is one set of MFMAs for
the tile, a block with suffix keys one per sample) + attn_decode_merge_kernel.  Every case is held to
  (a) the bits of mm_attn_decode (two launches, attn_decode_mfma = 1, the same nsplit) on the materialised concatenation;
  (b) independently, the per-element fp64 bound of attn_check.decode_reference with C["bf16-decode-mfma"]["out"] = 2 (derived there
      from the kernel's single bf16 rounding);
  (c) two runs giving the same bits;
  (d) intact guards around out and the workspace, and every slice's record written.
Operands sit as generate passes them: q a strided view into a fused q|k|v row, the caches views of longer buffers with a NaN tail.
The cases are the smallest at which the kernel can go wrong: partial and several column tiles (n against 16 / G), prefix and suffix
lengths around the 16-key block, slices in the prefix, across Sp, in the suffix and empty, and every prefix mask."""
import pytest
import torch

from tests import attn_check as AC
from tests import attn_shared_check as SC
from tests.kernel_check import check_bits, lib, options

pytestmark = pytest.mark.gpu

SH = SC.case
CASES = [
    #  B  Hq Hkv n   Sp  Ss  ns
    SH(1, 4, 1, 1, 1, 1, 1),                          # one key each side, one live sample
    SH(3, 8, 2, 5, 130, 40, 7, "leftpad"),            # G 4, two tiles (4 + 1); chunk 25: prefix, straddle (125..150), suffix
    SH(1, 4, 1, 9, 15, 1, 7, "holes"),                # G 4, three tiles; chunk 3: prefix, suffix (15..16), an empty slice
    SH(3, 4, 2, 9, 47, 17, 3, "dead"),                # G 2, two tiles (8 + 1); chunk 22: prefix, prefix, straddle; prompt 0 sees its suffix only
    SH(1, 2, 1, 9, 16, 16, 2, "leftpad"),             # G 2; the slice edge on Sp, both a whole 16-key block
    SH(3, 2, 2, 3, 64, 15, "lib", "holes"),           # G 1, one partial tile; the library's 2 slices of 40: prefix, straddle
    SH(1, 1, 1, 9, 65, 40, 3, "dead"),                # G 1; every prefix key masked; chunk 35: prefix, straddle, suffix
    SH(3, 4, 1, 4, 65, 17, 2),                        # G 4, exactly one full tile
    SH(1, 4, 2, 2, 17, 15, 1, "holes"),               # G 2, one slice
    SH(3, 1, 1, 5, 1, 40, 7),                         # one prefix key, three suffix blocks; chunk 6
    SH(1, 8, 2, 9, 130, 16, "lib", "leftpad"),        # G 4, three tiles; the library's 3 slices of 49: prefix, prefix, straddle
    SH(3, 4, 1, 2, 16, 2, 3, "dead"),                 # G 4, half a tile; chunk 6: the last slice straddles
    SH(1, 4, 1, 5, 130, 40, 1, "holes"),              # one workgroup walks prefix blocks, the straddling block and suffix blocks
]


def test_the_cases_cover_what_the_kernel_distinguishes():
    seen = {k: {c[k] for c in CASES} for k in ("B", "Hkv", "n", "Sp", "Ss", "ns", "mask")}
    assert seen["B"] == {1, 3} and seen["Hkv"] == {1, 2} and {c["Hq"] // c["Hkv"] for c in CASES} == {1, 2, 4}
    assert seen["n"] == {1, 2, 3, 4, 5, 9}
    assert seen["Sp"] == {1, 15, 16, 17, 47, 64, 65, 130} and seen["Ss"] == {1, 2, 15, 16, 17, 40}
    assert seen["ns"] == {1, 2, 3, 7, "lib"} and seen["mask"] == {None, "leftpad", "holes", "dead"}
    many = set()                                       # slice positions met with more samples than one tile holds
    for c in CASES:
        if c["n"] > 16 // (c["Hq"] // c["Hkv"]):
            many |= SC.slice_kinds(c["Sp"], c["Ss"], SC.nsplit(c))
    assert many == {"prefix", "straddle", "suffix", "empty"}


@pytest.mark.parametrize("c", CASES, ids=[SC.case_id(c) for c in CASES])
def test_shared_decode_contract(c):
    B, n, Hq, Hkv, Sp, Ss = c["B"], c["n"], c["Hq"], c["Hkv"], c["Sp"], c["Ss"]
    ns = SC.nsplit(c)
    if c["ns"] == "lib":
        assert lib().mm_attn_decode_shared_splits(B, n, Hkv, Sp + Ss) == ns
    mask = AC.decode_mask(c["mask"], B, Sp, ns)
    q, kp, vp, ks, vs = SC.operands(c, mask)
    scale = SC.D ** -0.5
    mg = mask.cuda() if mask is not None else None
    qd, kpd, vpd, ksd, vsd = SC.place(q, kp, vp, ks, vs)
    got, g1 = SC.run(qd, kpd, vpd, ksd, vsd, n, mg, scale, ns)
    again, g2 = SC.run(qd, kpd, vpd, ksd, vsd, n, mg, scale, ns)
    # the cache of B n rows that holds the prompt n times, through mm_attn_decode's MFMA slice kernel with the same slices
    km, vm, mm = SC.materialise(kp, vp, ks, vs, mask, n)
    qm, kmd, vmd = AC.decode_place(q, km, vm)
    mmg = mm.cuda() if mm is not None else None
    with options(attn_decode_mfma=1):
        want, g3, _ = AC.run_decode(qm, kmd, vmd, mmg, scale, ns)
    torch.cuda.synchronize()
    AC.verify_guards(g1 + g2 + g3)                                    # (d)
    ref = AC.decode_reference(qm, kmd, vmd, mmg, scale)
    worst = AC.check_decode(got, ref, "bf16-decode-mfma")            # (b)
    print(f"{SC.case_id(c)}: err / (u E) = {worst:.3f}, bits equal = {torch.equal(got.view(torch.int16), want.view(torch.int16))}")
    assert bool(ref["rows"].all())                                    # a suffix key is always visible
    check_bits("shared == mm_attn_decode on the materialised cache", got, want)      # (a)
    check_bits("rerun", again, got)                                   # (c)


def test_b0_and_refusals_write_nothing():
    """B = 0 is MM_OK; a refused call returns its code; neither touches out or the workspace."""
    from tests.kernel_check import SENTINEL, rc, dt, ptr
    c = SH(2, 4, 2, 3, 20, 3, 2)
    q, kp, vp, ks, vs = SC.place(*SC.operands(c, None))
    out, ws, guards = AC.decode_buffers(6, 4, SC.D, 2, "cuda")
    s3 = AC._s3

    def attempt(want, B=2, n=3, Hq=4, D=SC.D, ns=2, dq=0):
        assert rc("mm_attn_decode_shared", dt(q.dtype), ptr(q) + dq, ptr(kp), ptr(vp), ptr(ks), ptr(vs), B, n, 20, 3, Hq, 2, D, q.stride(0),
                  q.stride(1), *s3(kp), *s3(vp), *s3(ks), *s3(vs), None, 0.1, ptr(out), ptr(ws), ns) == want

    attempt(0, B=0)
    attempt(-1, n=0)
    attempt(-1, ns=0)
    attempt(-3, D=64)
    attempt(-3, Hq=16)
    attempt(-2, dq=8)
    torch.cuda.synchronize()
    for _, g, *_ in guards:
        assert bool((g.buf.view(torch.int16 if g.dtype == torch.bfloat16 else torch.int32) == SENTINEL[g.dtype]).all())

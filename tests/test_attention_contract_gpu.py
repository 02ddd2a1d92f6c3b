"""Attention through the C ABI, by launch path, against the fp64 per-element bounds of tests/attn_check.py.

Paths (launch_bf16_fwd / launch_bf16_bwd / mm_attn_bwd): bf16 D = 128 (attn_fwd128q_kernel, attn_fwd128p_kernel above 256 Ki keys,
attn_bwd_dq128p_kernel, attn_bwd_dkv128_pairp_kernel), bf16 D = 64 (attn_fwd_kernel<64>, attn_bwd_dq_kernel<64>,
attn_bwd_dkv_kernel<64>), fp32 (attn_fwd_f32_kernel, attn_bwd_f32_kernel, both forms of attn_delta_kernel).  Every launch writes
into guarded storages (tests/kernel_check.py: Guarded) and every case checks the output contract.  Then the exact invariances:
the work mapping (batch split, KV-head permutation), masked padding keys, and repeat determinism with a GEMM running beside.
The last section holds mm_attn_decode (the VALU and MFMA slice kernels, the merge kernel and the single-launch merge) to the same
rule, to two exact families and to its return codes."""
import pytest
import torch

from tests import attn_check as AC
from tests.kernel_check import SENTINEL, check_bits, lib, options, rc

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from multimeditron_amd import kernels
    return kernels


def case(B, Sq, Skv, Hq, Hkv, D, causal, mask=None, mag="randn", layout="sep", dtype=BF):
    return dict(B=B, Sq=Sq, Skv=Skv, Hq=Hq, Hkv=Hkv, D=D, causal=causal, mask=mask, mag=mag, layout=layout, dtype=dtype)


def case_id(c):
    t = "f32" if c["dtype"] == F32 else "bf16"
    return (f"{t}-B{c['B']}-q{c['Sq']}-k{c['Skv']}-h{c['Hq']}x{c['Hkv']}-d{c['D']}-{'causal' if c['causal'] else 'full'}"
            f"-{c['mask'] or 'nomask'}-{c['mag']}-{c['layout']}")


CASES = [
    # ---- bf16 D = 128: work mapping (B*Hkv % 8 == 0 takes attn_work_item's XCD branch and the pair kernel's XCD order)
    case(4, 2048, 2048, 32, 8, 128, True, layout="fused"),                     # the benchmark geometry: B*Hkv 32, G 4
    case(2, 513, 513, 28, 4, 128, True, "holes", layout="fused"),              # Qwen2 28/4: B*Hkv 8, G 7; Sq%256 = 1, Skv%128 = 1
    case(8, 200, 200, 8, 1, 128, False, "holes", "big"),                       # B*Hkv 8, G 8
    case(16, 129, 129, 1, 1, 128, True, layout="prefix"),                      # B*Hkv 16, G 1
    case(4, 65, 257, 28, 4, 128, True, mag="maxlast"),                          # B*Hkv 16, G 7, 3 key blocks (partial partner), odd totals
    case(8, 256, 256, 32, 4, 128, False, mag="rising", layout="fused"),         # B*Hkv 32, G 8; Sq%256 = 0, Skv%128 = 0
    case(3, 255, 255, 8, 2, 128, True, "holes", layout="fused"),                # plain branch: B*Hkv 6; Skv%128 = 127
    case(3, 33, 64, 28, 4, 128, True, mag="maxlast"),                           # plain branch: B*Hkv 12, G 7; shift 31, one key block
    # ---- tile edges, causal shifts, Sq > Skv
    case(1, 31, 32, 4, 1, 128, True, layout="prefix"),                          # shift 1, Sq%256 = 31
    case(2, 1, 65, 8, 2, 128, True, "holes"),                                   # Sq = 1, Skv%128 = 65
    case(1, 256, 319, 4, 2, 128, True, mag="big"),                              # shift 63, Skv%128 = 63
    case(2, 32, 96, 2, 1, 128, True, "lead_dead"),                              # shift 64, Sq%256 = 32
    case(1, 512, 641, 2, 1, 128, True, mag="rising", layout="prefix"),          # shift 129, 6 key blocks
    case(2, 300, 200, 4, 2, 128, True),                                         # Sq > Skv: rows 0..99 see no key
    case(1, 70, 64, 7, 1, 128, True, mag="big"),                                # Sq > Skv, one key block, odd G
    # ---- masks
    case(2, 640, 640, 4, 2, 128, True, "holes"),                                # hole, a masked 64-key tile and a masked 128-key block
    case(2, 40, 200, 2, 1, 128, False, "last_only"),
    case(2, 130, 130, 4, 4, 128, True, "dead_sample", layout="fused"),
    case(2, 300, 300, 4, 1, 128, True, "lead_dead", "big"),
    # ---- bf16 D = 64
    case(2, 200, 200, 4, 2, 64, True, "holes", layout="fused"),
    case(8, 33, 129, 8, 1, 64, True, mag="big"),
    case(1, 300, 200, 2, 1, 64, True),                                          # Sq > Skv
    case(2, 1, 77, 4, 2, 64, True, "last_only"),
    case(3, 255, 255, 2, 2, 64, False, mag="rising", layout="prefix"),
    case(2, 130, 130, 2, 1, 64, True, "dead_sample", "maxlast"),
    # ---- fp32, D in {64, 72, 96, 128, 256}: delta kernel vector form (D 64, 128, 256) and one-wave-per-row form (72, 96)
    case(2, 130, 130, 4, 2, 64, True, "holes", layout="fused", dtype=F32),
    case(1, 77, 100, 2, 1, 72, True, mag="big", dtype=F32),
    case(2, 65, 65, 2, 1, 96, False, "lead_dead", "rising", layout="prefix", dtype=F32),
    case(2, 129, 129, 4, 2, 128, True, "dead_sample", dtype=F32),
    case(1, 40, 300, 2, 1, 256, True, mag="maxlast", dtype=F32),
    case(1, 100, 60, 2, 1, 64, True, dtype=F32),                                # Sq > Skv
]



def make_mask(kind, B, Skv):
    if kind is None:
        return None
    m = torch.ones(B, Skv, dtype=torch.long)
    if kind == "holes":
        m[0, min(70, Skv - 1):min(73, Skv)] = 0           # a hole inside one 64-key tile (Skv = 65: the last keys)
        if Skv > 200:
            m[0, 128:192] = 0                              # a fully masked 64-key tile between visible keys
        if Skv > 450:
            m[-1, 256:384] = 0                             # a fully masked 128-key block between visible keys
        if B > 1:
            m[1, : Skv // 3] = 0                           # left padding
    elif kind == "last_only":
        m[:, :-1] = 0
    elif kind == "dead_sample":
        m[0] = 0
    elif kind == "lead_dead":                              # with causal: the leading rows of sample 0 see no key
        m[0, : Skv // 3] = 0
    return m


def make_operands(c, seed=1):
    B, Sq, Skv, Hq, Hkv, D = c["B"], c["Sq"], c["Skv"], c["Hq"], c["Hkv"], c["D"]
    g = torch.Generator().manual_seed(seed + Sq * 7 + Skv + D)
    q = torch.randn(B, Sq, Hq, D, generator=g)
    k = torch.randn(B, Skv, Hkv, D, generator=g)
    v = torch.randn(B, Skv, Hkv, D, generator=g)
    do = torch.randn(B, Sq, Hq, D, generator=g)
    a = 40.0 / (4.0 * D ** -0.5)
    if c["mag"] == "big":                                  # scores up to about +-60 after scaling
        q, k = q * 2.8, k * 2.8
    elif c["mag"] == "rising":                             # scores rise along the keys: the running max moves in every tile
        q[..., 0] = 4.0
        k[..., 0] = torch.linspace(-1.0, 1.0, Skv)[None, :, None] * a
    elif c["mag"] == "maxlast":                            # every row's max sits on the last key (in the last partial tile)
        q[..., 0] = 4.0
        k[:, -1, :, 0] = a
    dt = c["dtype"]
    return q.to(dt), k.to(dt), v.to(dt), do.to(dt)


def place(c, q, k, v):
    """Device q/k/v in the case's layout: `fused` = views of one [B*S, (Hq + 2Hkv) D + guard columns] buffer (as the decoder
    uses them; the guard columns hold NaN), `sep` = contiguous tensors, `prefix` = K/V as prefix views of a longer cache whose
    rows past Skv are NaN (k_sb != Skv k_ss)."""
    B, Sq, Skv, Hq, Hkv, D = c["B"], c["Sq"], c["Skv"], c["Hq"], c["Hkv"], c["D"]
    dev = "cuda"
    if c["layout"] == "fused":
        assert Sq == Skv
        gc = 8
        W = Hq * D + 2 * Hkv * D + 4 * gc
        buf = torch.full((B, Sq, W), float("nan"), dtype=q.dtype)
        o_q, o_k = gc, gc + Hq * D + gc
        o_v = o_k + Hkv * D + gc
        buf[..., o_q:o_q + Hq * D] = q.reshape(B, Sq, -1)
        buf[..., o_k:o_k + Hkv * D] = k.reshape(B, Skv, -1)
        buf[..., o_v:o_v + Hkv * D] = v.reshape(B, Skv, -1)
        buf = buf.to(dev)
        return (buf[..., o_q:o_q + Hq * D].view(B, Sq, Hq, D), buf[..., o_k:o_k + Hkv * D].view(B, Skv, Hkv, D),
                buf[..., o_v:o_v + Hkv * D].view(B, Skv, Hkv, D))
    if c["layout"] == "prefix":
        Smax = Skv + 37
        kc = torch.full((B, Smax, Hkv, D), float("nan"), dtype=q.dtype)
        vc = torch.full((B, Smax, Hkv, D), float("nan"), dtype=q.dtype)
        kc[:, :Skv], vc[:, :Skv] = k, v
        kc, vc = kc.to(dev), vc.to(dev)
        return q.to(dev), kc[:, :Skv], vc[:, :Skv]
    return q.to(dev), k.to(dev), v.to(dev)


def run_case(c, qd, kd, vd, dod, mg, scale, stream=None):
    out, lse, g1 = AC.run_fwd(qd, kd, vd, mg, c["causal"], scale, stream)
    dq, dk, dv, g2 = AC.run_bwd(qd, kd, vd, out, dod, lse, mg, c["causal"], scale, stream)
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv), g1 + g2


def big_gemm(K, side):
    """A large GEMM on another stream (the overlap run of the determinism check)."""
    cur = torch.cuda.current_stream()
    a = torch.randn(4096, 4096, device="cuda").to(BF)
    b = torch.randn(4096, 4096, device="cuda").to(BF)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        K.gemm(0, a, b, 4096, 4096, 4096)
        K.gemm(0, a, b, 4096, 4096, 4096)
    return a, b


def check_case(K, c, repeats=True):
    B, Sq, Skv, D = c["B"], c["Sq"], c["Skv"], c["D"]
    dt = c["dtype"]
    q, k, v, do = make_operands(c)
    mask = make_mask(c["mask"], B, Skv)
    scale = D ** -0.5
    qd, kd, vd = place(c, q, k, v)
    dod = do.cuda()
    mg = mask.cuda() if mask is not None else None
    res, guards = run_case(c, qd, kd, vd, dod, mg, scale)
    torch.cuda.synchronize()
    AC.verify_guards(guards)
    ref = AC.reference(qd, kd, vd, dod, mg, c["causal"], scale)
    AC.check_contract(res, ref)
    AC.check_all(res, ref, dt, AC.path_of(dt, D, Skv))
    if repeats and dt == BF and D == 128:
        # two more runs, the second beside a large GEMM on another stream: bit for bit the same results
        side = torch.cuda.Stream()
        again, g = run_case(c, qd, kd, vd, dod, mg, scale)
        keep = big_gemm(K, side)
        third, g3 = run_case(c, qd, kd, vd, dod, mg, scale)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        del keep
        AC.verify_guards(g + g3)
        for n in ("out", "lse", "dq", "dk", "dv"):
            assert torch.equal(res[n], again[n]) and torch.equal(res[n], third[n]), f"{n} differs between repeated runs"
    return res


@pytest.mark.parametrize("c", CASES, ids=[case_id(c) for c in CASES])
def test_attention_contract(K, c):
    check_case(K, c)


# ---- exact invariances -------------------------------------------------------------------------------------------------
def _run_plain(c, q, k, v, do, mask, scale):
    qd, kd, vd = place(c, q, k, v)
    res, guards = run_case(c, qd, kd, vd, do.cuda(), mask.cuda() if mask is not None else None, scale)
    torch.cuda.synchronize()
    AC.verify_guards(guards)
    return res


@pytest.mark.parametrize("D", [128, 64])
def test_attention_batch_split(K, D):
    """B = 8, Hkv = 1 (B*Hkv % 8 == 0: the XCD-aware work order of the D = 128 kernels) == each sample alone (the plain order),
    bit for bit: the per-row arithmetic does not depend on which workgroup does it."""
    c = case(8, 200, 200, 4, 1, D, True, "holes")
    q, k, v, do = make_operands(c)
    mask = make_mask("holes", 8, 200)
    scale = D ** -0.5
    full = _run_plain(c, q, k, v, do, mask, scale)
    c1 = dict(c, B=1)
    for b in range(8):
        one = _run_plain(c1, q[b:b + 1], k[b:b + 1], v[b:b + 1], do[b:b + 1], mask[b:b + 1], scale)
        for n in ("out", "dq", "dk", "dv"):
            assert torch.equal(full[n][b:b + 1], one[n]), f"{n} of sample {b} differs from the sample run alone"
        assert torch.equal(full["lse"][b:b + 1], one["lse"]), f"lse of sample {b} differs from the sample run alone"


@pytest.mark.parametrize("D", [128, 64])
def test_attention_head_permutation(K, D):
    """Permuting the KV heads together with their query groups permutes the results, bit for bit (B = 2, Hkv = 4: XCD order)."""
    B, S, Hkv, G = 2, 160, 4, 2
    c = case(B, S, S, Hkv * G, Hkv, D, True, layout="fused")
    q, k, v, do = make_operands(c)
    scale = D ** -0.5
    perm = [2, 0, 3, 1]
    qperm = [p * G + g for p in perm for g in range(G)]
    base = _run_plain(c, q, k, v, do, None, scale)
    pr = _run_plain(c, q[:, :, qperm], k[:, :, perm], v[:, :, perm], do[:, :, qperm], None, scale)
    for n, idx in (("out", qperm), ("dq", qperm), ("dk", perm), ("dv", perm)):
        assert torch.equal(base[n][:, :, idx], pr[n]), f"{n} differs under a KV-head permutation"
    assert torch.equal(base["lse"][:, qperm], pr["lse"]), "lse differs under a KV-head permutation"


@pytest.mark.parametrize("npad", [1, 64, 200])
@pytest.mark.parametrize("path", [(BF, 128), (BF, 64), (F32, 64)], ids=["bf16-d128", "bf16-d64", "f32-d64"])
def test_attention_masked_padding_keys(K, npad, path):
    """Keys appended with key_mask = 0 (non-causal) change nothing: out, lse and dq are bit-identical, dk / dv are bit-identical on
    the original keys and exactly 0 on the appended ones.  A masked key gets p = exp2(-inf) = 0: the running max, l (times
    alpha = 1) and O (+ 0 * v) keep their bits, and so do dS and every dQ / dK / dV sum.  fp32: dk / dv are atomic sums (no
    fixed order), so only out, lse and dq are compared there."""
    dt, D = path
    B, Sq, Skv, Hq, Hkv = 2, 150, 150, 4, 2
    c = case(B, Sq, Skv, Hq, Hkv, D, False, dtype=dt)
    cp = dict(c, Skv=Skv + npad)
    q, k, v, do = make_operands(cp)
    scale = D ** -0.5
    base = _run_plain(c, q, k[:, :Skv], v[:, :Skv], do, None, scale)
    mask = torch.ones(B, Skv + npad, dtype=torch.long)
    mask[:, Skv:] = 0
    pad = _run_plain(cp, q, k, v, do, mask, scale)
    for n in ("out", "lse", "dq"):
        assert torch.equal(base[n], pad[n]), f"{n} changes when {npad} masked keys are appended"
    assert bool((pad["dk"][:, Skv:] == 0).all()) and bool((pad["dv"][:, Skv:] == 0).all()), "dk/dv of appended masked keys != 0"
    if dt == BF:
        assert torch.equal(base["dk"], pad["dk"][:, :Skv]) and torch.equal(base["dv"], pad["dv"][:, :Skv]), \
            f"dk/dv of the original keys change when {npad} masked keys are appended"


# ---- mm_attn_decode: one query token over a KV cache ---------------------------------------------------------------------------
# Kernels: attn_decode_partial_kernel<D, G> (VALU; keys per wave trip / workgroup trip: 16 / 64 at D = 128, 32 / 128 at D = 64),
# attn_decode_partial128_mfma_kernel<G> (D = 128, G <= 4, two-launch form; 16 / 64), attn_decode_merge_kernel, and the merge by
# the last slice through the `sync` counters.  Every case runs the three launch forms -- two launches with attn_decode_mfma = 1
# (MFMA where it applies), two launches with attn_decode_mfma = 0 (VALU), fused (VALU) -- each twice into fresh guards.
DC = AC.decode_case
DECODE_CASES = [
    # D = 128, G <= 4: every Skv through the MFMA and the VALU slice kernels
    DC(1, 1, 1, 1, 128),
    DC(3, 15, 4, 2, 128, "leftpad"),
    DC(1, 17, 4, 1, 128, "holes", ns=1),
    DC(3, 63, 2, 2, 128, "single"),
    DC(3, 65, 8, 2, 128, "dead"),
    DC(3, 129, 2, 1, 128, "slice", ns="lib8"),              # 3 slices of 43 keys
    DC(1, 200, 1, 1, 128, "holes", ns="lib8"),              # 4 slices of 50
    DC(3, 200, 8, 2, 128, "leftpad", ns=3),                 # chunk 67: a slice edge that is no multiple of 16
    DC(1, 10, 2, 1, 128, ns=8),                             # chunk 2: slices 5 .. 7 hold no key
    DC(3, 10, 4, 1, 128, "slice", ns=8),                    # ... and one more holds only masked keys
    DC(1, 2051, 4, 1, 128, "holes"),                        # the library's own count: 33 slices of 63
    # D = 128, G in {7, 8}: VALU in every form
    DC(1, 65, 7, 1, 128, "leftpad"),
    DC(3, 200, 16, 2, 128, "dead", ns=3),
    DC(1, 129, 14, 2, 128, "slice", ns="lib8"),
    # D = 64: every Skv, every G
    DC(1, 1, 2, 2, 64),
    DC(3, 15, 7, 1, 64, "leftpad"),
    DC(1, 17, 8, 1, 64, "holes", ns=1),
    DC(3, 63, 1, 1, 64, "single"),
    DC(3, 65, 4, 1, 64, "dead"),
    DC(3, 129, 4, 2, 64, "slice", ns="lib8"),
    DC(1, 200, 14, 2, 64, "holes", ns="lib8"),
    DC(3, 200, 2, 1, 64, "leftpad", ns=3),
    DC(1, 10, 8, 2, 64, ns=8),
    DC(1, 2051, 8, 1, 64, "holes"),
]
ONE_KEY_CASES = [DC(3, 200, 8, 2, 128, ns=3), DC(3, 10, 7, 1, 128, ns=8), DC(3, 2051, 4, 1, 128), DC(3, 200, 2, 1, 64, ns=3),
                 DC(3, 65, 14, 2, 64), DC(3, 17, 1, 1, 128, ns=1)]
UNIFORM_CASES = [DC(3, 200, 4, 2, 128, ns=3), DC(3, 200, 7, 1, 64, ns="lib8"), DC(3, 2051, 2, 1, 128), DC(3, 2051, 8, 1, 64),
                 DC(3, 200, 16, 2, 128, ns=8)]


def decode_nsplit(c):
    """the case's split count; the library's own value is asked of mm_attn_decode_splits and must match its mirror"""
    ns = AC.decode_nsplit(c)
    if c["ns"] in ("lib", "lib8"):
        with options(attn_decode_wgs=8 if c["ns"] == "lib8" else AC.DECODE_WGS):
            assert lib().mm_attn_decode_splits(c["B"], c["Hkv"], c["Skv"]) == ns
    return ns


def decode_forms(q, k, v, mask, scale, ns):
    """{path: out} of the three launch forms.  Each runs twice into fresh guards (the fused form on the same counters) and must
    repeat bit for bit; the fused form must equal the two-launch VALU form bit for bit and leave every counter zero."""
    B, Hq, D = q.shape
    G = Hq // k.shape[2]
    res, guards = {}, []
    for mfma in (1, 0):
        with options(attn_decode_mfma=mfma):
            a, g1, _ = AC.run_decode(q, k, v, mask, scale, ns)
            b, g2, _ = AC.run_decode(q, k, v, mask, scale, ns)
        path = AC.decode_path(D, G, mfma=bool(mfma))
        guards += g1 + g2
        check_bits(f"{path} rerun", b, a)
        if path in res:                                     # no MFMA kernel for this shape: the switch changes nothing
            check_bits(f"{path} with attn_decode_mfma = {mfma}", a, res[path])
        res[path] = a
    a, g1, sync = AC.run_decode(q, k, v, mask, scale, ns, fused=True)
    b, g2, _ = AC.run_decode(q, k, v, mask, scale, ns, fused=True, sync=sync)
    torch.cuda.synchronize()
    AC.verify_guards(guards + g1 + g2)
    AC.decode_sync_clean(sync)
    check_bits("fused rerun on the same counters", b, a)
    check_bits("fused == two-launch VALU", a, res["bf16-decode-valu"])
    res["bf16-decode-fused"] = a
    return res


@pytest.mark.parametrize("c", DECODE_CASES, ids=[AC.decode_case_id(c) for c in DECODE_CASES])
def test_decode_contract(K, c):
    ns = decode_nsplit(c)
    mask = AC.decode_mask(c["mask"], c["B"], c["Skv"], ns)
    q, k, v = AC.decode_place(*AC.decode_operands(c, mask))
    mg = mask.cuda() if mask is not None else None
    scale = c["D"] ** -0.5
    res = decode_forms(q, k, v, mg, scale, ns)
    if c["D"] == 128 and c["Hq"] // c["Hkv"] <= 4:
        assert set(res) == {"bf16-decode-mfma", "bf16-decode-valu", "bf16-decode-fused"}
    ref = AC.decode_reference(q, k, v, mg, scale)
    for path, out in res.items():
        AC.check_decode(out, ref, path)
        dead = out[~ref["rows"]]
        check_bits(f"{path}: rows with no visible key give 0", dead, torch.zeros_like(dead))


@pytest.mark.parametrize("c", ONE_KEY_CASES, ids=[AC.decode_case_id(c) for c in ONE_KEY_CASES])
def test_decode_one_key_exact(K, c):
    """One visible key per sequence (first of a slice, last of a slice, Skv - 1): p = 1, l = 1, out == that key's V row."""
    ns = decode_nsplit(c)
    q, k, v, mask, want = AC.decode_one_key(c, ns)
    qd, kd, vd = AC.decode_place(q, k, v)
    for path, out in decode_forms(qd, kd, vd, mask.cuda(), c["D"] ** -0.5, ns).items():
        check_bits(f"one_key {path}", out, want)


@pytest.mark.parametrize("c", UNIFORM_CASES, ids=[AC.decode_case_id(c) for c in UNIFORM_CASES])
def test_decode_uniform_exact(K, c):
    """q = 0, integer V, 128 / 64 / 32 visible keys spread over the slices: every sum is exact, out == mean of the visible V."""
    ns = decode_nsplit(c)
    q, k, v, mask, want = AC.decode_uniform(c)
    qd, kd, vd = AC.decode_place(q, k, v)
    for path, out in decode_forms(qd, kd, vd, mask.cuda(), c["D"] ** -0.5, ns).items():
        check_bits(f"uniform {path}", out, want, zero_sign=False)


def test_decode_return_codes(K):
    """Every refusal of mm_attn_decode by code, with out, the workspace and the counters bit-unchanged; B = 0 is MM_OK and
    writes nothing."""
    OK, ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -3
    B, Skv, Hq, Hkv, D, ns = 2, 40, 4, 2, 128, 2

    def attempt(want, B=B, Hq=Hq, Hkv=Hkv, D=D, ns=ns, dtype=BF, dq=0, dsb=0):
        q = torch.randn(max(B, 1), Hq, D + 8, device="cuda").to(dtype)[..., :D]
        k = torch.randn(max(B, 1), Skv, Hkv, D, device="cuda").to(dtype)
        v = torch.randn(max(B, 1), Skv, Hkv, D, device="cuda").to(dtype)
        out, ws, guards = AC.decode_buffers(max(B, 1), Hq, D, max(ns, 1), "cuda")
        sync = torch.full((max(B, 1) * Hkv + AC.SYNC_SPARE,), 77, dtype=torch.int32, device="cuda")
        for s in (None, sync):
            a = list(AC.decode_args(q, k, v, None, D ** -0.5, out, ws, ns, s))
            a[0], a[1], a[4], a[9] = (0 if dtype == BF else 1), a[1] + dq, B, a[9] + dsb
            assert rc("mm_attn_decode", *a) == want, (want, B, Hq, Hkv, D, ns, dtype, dq, dsb)
        torch.cuda.synchronize()
        for _, g, *_ in guards:
            assert bool((g.buf.view(torch.int16 if g.dtype == BF else torch.int32) == SENTINEL[g.dtype]).all()), \
                "a refused or empty call wrote to out or the workspace"
        assert bool((sync == 77).all()), "a refused or empty call touched the counters"

    attempt(ERR_UNSUPPORTED, dtype=F32)
    attempt(ERR_UNSUPPORTED, D=96)
    attempt(ERR_UNSUPPORTED, Hq=3, Hkv=1)                  # G = 3
    attempt(ERR_ARG, Hq=5, Hkv=2)                          # Hq % Hkv != 0
    attempt(ERR_ARG, ns=0)
    attempt(ERR_ALIGN, dsb=4)                              # q_sb not a multiple of 8 elements
    attempt(ERR_ALIGN, dq=2)                               # q not 16-byte aligned
    attempt(OK, B=0)

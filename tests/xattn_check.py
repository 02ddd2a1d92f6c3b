"""Cross-attention and dropout checker (csrc/mm_xattn.hip): the keep masks of the documented Philox indexing computed on the CPU,
an fp64 reference with per-element error scales, the cases of the GPU contract test, and guarded launches through the C ABI.

`keep_mask` / `dropout_keep` follow include/mm_hip.h and nothing else: Philox4x32-10 (tests/sampling_ref.py) keyed by `seed` with
counter (call, offset); attention weight (row, key), row = (image * H + head) * Nq + query, takes component key & 3 of call
row * KP/4 + key/4 with KP = Nkv rounded up to 32; element i of the flat stream takes component i & 3 of call i / 4; an element is
kept when its word >= float32(p) * 2^32.  No mask in these tests comes from mm_dropout_mask, which is code under test.

`reference` runs in float64 on the device of its operands, on the SAME bf16- or fp32-rounded q/k/v/dout the kernels read, with
the keep factor F = keep * float32(1 / (1 - float32(p))) carried through, and returns the error scale E of every element for
the rule of tests/kernel_check.py.  A, PA, Pw and kappa are those of tests/attn_check.py: A = sqrt(D) scale |Q|.|K|^T + |lse|
(the relative error of an fp32 probability in units of u32), PA = P o A, Pw = P + kappa PA, kappa = u32 / u.

The rounding points of the bf16 kernels (header comment of mm_xattn.hip) and the term of E that covers each:
  forward   S = Q.K^T in fp32 (exact bf16 products), p = exp(S*scale - m), sum in fp32, P_drop = bf16(p / sum * f) before
            O = P_drop.V in fp32, out = bf16(O)                                -> E_out = (Pw o F).|V| + kappa |O| rowsum(PA)
  backward  delta = rowsum(out * dO) from the bf16 `out`                        -> E_delta = sum_d E_out |dO|
            p = exp(S*scale - lse), dP = dO.V^T in fp32
            dV = bf16(p f)^T.dO                                                -> E_dv = (Pb o F)^T.|dO|
            dS = bf16(p (dP f - delta) scale)   -> E_dS = Pb o (F |dP| + |delta|) + P E_delta + kappa sqrt(D) P o F o (|dO|.|V|^T)
            dQ = dS.K, dK = dS^T.Q in fp32, every output rounded to bf16        -> E_dq = scale E_dS.|K|, E_dk = scale E_dS^T.|Q|
  lse (fp32 on both paths, checked with u32)                                  -> E_lse = |lse| + rowsum(PA) + sqrt(Nkv)
One term more than the attention checker's, found by the fp32 emulation (tests/test_xattn_check_cpu.py) on the `maxlast`
cases: the backward's p = exp(S*scale - lse) (xattn_bwd_q_kernel; xattn_f32_q_kernel mode 1) reads the forward's stored fp32 lse,
whose error u32 E_lse -- that of the row's largest score, about 380 u32 there -- moves EVERY probability of the row, while Pw
charges a probability with its own score's error and |lse| only.  So the backward scales (E_dv, E_dS) use
Pb = Pw + kappa P E_lse in place of Pw.  Without it the same emulation ran to 3.9 (dv) and 3.1 (dq) on those cases and under
0.9 with it; at kappa = 2^-16 the bf16 scales do not notice.
E = 0, where the rule demands equality, falls out of these terms: a query whose every key was dropped has F = 0 on its row, so
out = 0 with E_out = 0, delta = 0 with E_delta = 0 and dq = 0 with E_dq = 0; a key dropped by every query has dv = 0, E_dv = 0.

The constants.  bf16 out, dq, dk, dv: c = 4, derived, not measured.  Each term of E above bounds one bf16 rounding of the kernel
from above by u times itself: out and dv see two (P_drop -> bf16, and the output; E_out >= |out|, E_dv >= |dv|), dq and dk see
three (dS -> bf16, the bf16 `out` that enters delta, and the output), so the bf16 roundings amount to 3 u E at most; the fp32
steps enter E at kappa = 2^-16 and cannot fill the rest; 4 is the next power of two.  lse on both paths and every fp32-path
quantity: the smallest power of two >= 4x the worst err / (u E) of the CPU emulations of tests/test_xattn_check_cpu.py over
the cases below (4x and not the usual 2x: an emulation cannot model the hardware exp / log nor the MFMA's summation order).
No constant comes from kernel output; the ratios seen on the MI355X stand beside them as observations only."""
import ctypes
import functools
import math

import numpy as np
import torch

from tests.attn_check import grad_views
from tests.kernel_check import U, U32, Guarded, RatioLog, check_bound, coords, dt, lib, ptr, stream
from tests.sampling_ref import philox4x32_10

BF, F32 = torch.bfloat16, torch.float32
OK, ERR_ARG, ERR_ALIGN, ERR_UNSUPPORTED = 0, -1, -2, -3
QUANTITIES = ("out", "lse", "dq", "dk", "dv")

# c per path and quantity.  "emulation": worst err / (u E) of the CPU emulation over CASES, the (case, p) pairs the GPU test runs
# (tests/test_xattn_check_cpu.py asserts each constant against them and prints them with -s); "MI355X": what the GPU contract
# test saw, an observation.
C = {
    # out, dq, dk, dv derived (docstring); emulation 1.78, 1.49, 1.21, 1.84; MI355X observed 1.78, 1.49, 1.21, 1.84
    # lse: emulation 0.73 (x4 = 2.9); MI355X observed 0.42
    "bf16": {"out": 4.0, "lse": 4.0, "dq": 4.0, "dk": 4.0, "dv": 4.0},
    # out, lse, dq, dk, dv: emulation 0.72, 0.78, 0.52, 0.13, 0.58 (x4 = 2.9, 3.1, 2.1, 0.52, 2.3), each worst at
    # (1,70,33,3,72) maxlast p = 0.9; MI355X observed 0.72, 0.78, 0.52, 0.13, 0.58
    # (the fp32 kernels' fma chains are what the emulation computes: the same worst elements to 10 digits)
    "f32": {"out": 4.0, "lse": 4.0, "dq": 4.0, "dk": 1.0, "dv": 4.0},
}

# worst err / (u E) seen per (path, quantity) in this process; MM_XATTN_RATIO_LOG=<file> writes them out at exit
RATIOS = RatioLog("MM_XATTN_RATIO_LOG")


def path_of(dtype):
    return "f32" if dtype == F32 else "bf16"


# ---- the dropout streams of include/mm_hip.h, on the CPU ------------------------------------------------------------------
def drop_threshold(p):
    """keep <=> word >= this: float32(p) * 2^32 in double, truncated, clamped to 32 bits."""
    t = float(np.float32(p)) * 4294967296.0
    return 0xFFFFFFFF if t >= 4294967295.0 else (0 if t <= 0.0 else int(t))


def inv_keep(p):
    """float32(1 / (1 - float32(p))), computed in fp32 as the kernels do; 1 at p = 0."""
    p32 = np.float32(p)
    return float(np.float32(1.0) / (np.float32(1.0) - p32)) if p32 > 0 else 1.0


def _words(calls, seed, offset):
    """[len(calls), 4]: the four 32-bit words of every Philox call"""
    return np.stack(philox4x32_10(calls, offset, seed), axis=-1)


def dropout_keep(seed, offset, n_elems, p):
    """bool [n_elems]: the flat stream of mm_dropout -- element i takes component i & 3 of call i // 4."""
    w = _words(np.arange((n_elems + 3) // 4, dtype=np.uint64), seed, offset).reshape(-1)[:n_elems]
    return torch.from_numpy(w >= np.uint64(drop_threshold(p)))


def keep_mask(seed, offset, n, H, Nq, Nkv, p, kp_multiple=32):
    """bool [n, H, Nq, Nkv]: weight (row, key) takes component key & 3 of call row * KP/4 + key/4, KP = Nkv rounded up to 32
    (`kp_multiple` exists for the CPU test that shows another rounding is a different mask)."""
    KP = (Nkv + kp_multiple - 1) // kp_multiple * kp_multiple
    rows = n * H * Nq
    calls = np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(KP // 4) + np.arange(KP // 4, dtype=np.uint64)[None, :]
    w = _words(calls.reshape(-1), seed, offset).reshape(rows, KP)[:, :Nkv]
    return torch.from_numpy(np.ascontiguousarray(w >= np.uint64(drop_threshold(p)))).view(n, H, Nq, Nkv)


# ---- the reference ------------------------------------------------------------------------------------------------------------
def reference(q, k, v, dout, scale, keep, p):
    """fp64 on q's device.  q/dout [n,Nq,H,D], k/v [n,Nkv,H,D] (any strides), keep bool [n,H,Nq,Nkv] or None (p = 0).  Returns
    a dict with out, lse [n,H,Nq], dq, dk, dv (fp64, [n,N,H,D]) and E_out, E_lse, E_dq, E_dk, E_dv, plus rows [n,H,Nq] (the
    query kept at least one key) and keys [n,H,Nkv] (at least one query kept the key)."""
    n, Nq, H, D = q.shape
    Nkv = k.shape[1]
    dev = q.device
    kappa = U32 / U[q.dtype]
    rt = math.sqrt(D)
    scale = float(np.float32(scale))                                     # what crosses the C ABI
    hm = lambda t: t.double().permute(0, 2, 1, 3)                        # [n, H, N, D]
    Q, Kt, V, dO = hm(q), hm(k), hm(v), hm(dout)
    if keep is None:
        keep = torch.ones(n, H, Nq, Nkv, dtype=torch.bool)
    keep = keep.to(dev)
    F = keep.double() * inv_keep(p)
    S = Q @ Kt.transpose(2, 3) * scale
    m = S.amax(-1, keepdim=True)
    e = torch.exp(S - m)
    lsum = e.sum(-1, keepdim=True)
    P = e / lsum
    lse = m + torch.log(lsum)
    PA = P * (rt * scale * (Q.abs() @ Kt.abs().transpose(2, 3)) + lse.abs())
    Pw = P + kappa * PA
    PA_sum = PA.sum(-1, keepdim=True)
    E_lse = lse.abs() + PA_sum + math.sqrt(Nkv)
    Pd, PwF = P * F, Pw * F
    O = Pd @ V
    E_o = PwF @ V.abs() + kappa * O.abs() * PA_sum
    Pb = Pw + kappa * P * E_lse              # backward: p = exp(S*scale - lse) reads the stored fp32 lse, error u32 E_lse and all
    PbF = Pb * F
    dP = dO @ V.transpose(2, 3)
    delta = (O * dO).sum(-1, keepdim=True)
    E_delta = (E_o * dO.abs()).sum(-1, keepdim=True)
    dS = P * (F * dP - delta)
    E_dS = Pb * (F * dP.abs() + delta.abs()) + P * E_delta + kappa * rt * P * F * (dO.abs() @ V.abs().transpose(2, 3))
    back = lambda t: t.permute(0, 2, 1, 3)                                # [n, N, H, D]
    return {"out": back(O), "E_out": back(E_o),
            "lse": lse[..., 0], "E_lse": E_lse[..., 0],
            "dq": back(scale * dS @ Kt), "E_dq": back(scale * E_dS @ Kt.abs()),
            "dk": back(scale * dS.transpose(2, 3) @ Q), "E_dk": back(scale * E_dS.transpose(2, 3) @ Q.abs()),
            "dv": back(Pd.transpose(2, 3) @ dO), "E_dv": back(PbF.transpose(2, 3) @ dO.abs()),
            "rows": keep.any(-1), "keys": keep.any(2)}


def _where(kind, idx, shape):
    """the location of flat index idx: image, head, query row or key, d, and the 64-query / 16-key tile the kernels give it to"""
    if kind == "lse":
        b, h, row = coords(idx, shape)
        return f"(image={b}, head={h}, row={row}) [q64 tile {row // 64}]"
    b, row, h, d = coords(idx, shape)
    if kind == "q":
        return f"(image={b}, head={h}, row={row}, d={d}) [q64 tile {row // 64}, d64 slice {d // 64}]"
    return f"(image={b}, head={h}, key={row}, d={d}) [k16 tile {row // 16}, d64 slice {d // 64}]"


KIND = {"out": "q", "lse": "lse", "dq": "q", "dk": "k", "dv": "k"}


def check(name, got, ref, E, c, u, path=None):
    """The rule on one quantity, recorded in RATIOS[(path, name)]; a failure names image, head, row or key, and d."""
    return check_bound(name, got, ref, E, c, u, key=path and (path, name), log=RATIOS, where=functools.partial(_where, KIND[name]))


def check_all(res, ref, dtype, path=None, c=None):
    """Every quantity present in `res` (out, lse, dq, dk, dv) against `ref`; returns {name: worst ratio}."""
    c = c or C[path]
    return {nm: check(nm, res[nm], ref[nm], ref["E_" + nm], c[nm], U32 if nm == "lse" else U[dtype], path)
            for nm in QUANTITIES if nm in res}


# ---- the cases of tests/test_xattn_contract_gpu.py (the CPU emulations run the same ones) ---------------------------------------
BF16_SHAPES = [  # n, Nq, Nkv, H, D
    (2, 5, 7, 1, 8),          # KP 32: 2 key tiles of the 4-tile instantiation
    (1, 1, 1, 1, 8),
    (1, 64, 64, 2, 64),       # 4 tiles full, one query tile exactly
    (1, 65, 65, 2, 72),       # 8-tile instantiation partly used, two query tiles, an 8-wide tail slice
    (1, 70, 33, 3, 72),
    (2, 49, 196, 2, 96),      # the recipe geometry
    (1, 16, 256, 1, 128),     # 16 tiles full, two full slices
    (1, 17, 257, 1, 136),     # 32-tile instantiation, three slices
    (1, 130, 500, 2, 128),
    (1, 9, 512, 1, 96),
    (1, 65, 513, 2, 72),      # 64-tile instantiation
    (1, 17, 777, 1, 96),
    (1, 16, 1024, 1, 512),    # the largest LDS image
    (1, 64, 47, 2, 504),
    (2, 40, 40, 2, 96),       # Nq = Nkv: the fused q|k|v layout
]
F32_SHAPES = [(2, 5, 7, 1, 7), (1, 3, 1, 1, 5), (1, 70, 33, 3, 72), (2, 49, 196, 2, 96), (1, 9, 1000, 1, 40), (1, 17, 1024, 1, 100),
              (2, 40, 40, 2, 96)]
MAGNITUDE_SHAPES = {BF: [(1, 70, 33, 3, 72), (2, 49, 196, 2, 96), (1, 65, 513, 2, 72)],
                    F32: [(1, 70, 33, 3, 72), (2, 49, 196, 2, 96), (1, 9, 1000, 1, 40)]}
LAYOUTS = ["sep", "fused_kv", "headmajor", "prefix"]              # cycled; fused_qkv goes where Nq = Nkv
FUSED_QKV = {(2, 40, 40, 2, 96), (1, 65, 65, 2, 72)}
SEEDS = [(1234, 7), (2 ** 63 - 1, 2 ** 33 + 1), (0, 0)]            # (seed, offset), cycled
P_ALL, P_SHORT = (0.0, 0.1), (0.5, 0.9)                           # every case; the cases with Nkv <= 65 as well


def _cases():
    out = []
    for dtype, shapes in ((BF, BF16_SHAPES), (F32, F32_SHAPES)):
        variants = [(s, "randn") for s in shapes] + [(s, mag) for s in MAGNITUDE_SHAPES[dtype] for mag in ("big", "maxlast")]
        for i, (shape, mag) in enumerate(variants):
            layout = "fused_qkv" if shape in FUSED_QKV else LAYOUTS[i % len(LAYOUTS)]
            ps = P_ALL + (P_SHORT if shape[2] <= 65 else ())
            for j, p in enumerate(ps):
                seed, offset = SEEDS[(i + j) % len(SEEDS)]
                out.append(dict(shape=shape, dtype=dtype, mag=mag, layout=layout, p=p, seed=seed, offset=offset))
    return out


CASES = _cases()


def case_id(c):
    return (f"{path_of(c['dtype'])}-" + "x".join(map(str, c["shape"])) + f"-{c['mag']}-{c['layout']}-p{c['p']}"
            f"-s{c['seed'] % 1000}")


def make_operands(c):
    """CPU q, k, v, dout of the case, storage-rounded: test_attention_contract_gpu.make_operands (its `big` and `maxlast`)."""
    from tests.test_attention_contract_gpu import make_operands as attn_operands
    n, Nq, Nkv, H, D = c["shape"]
    return attn_operands(dict(B=n, Sq=Nq, Skv=Nkv, Hq=H, Hkv=H, D=D, mag=c["mag"], dtype=c["dtype"]))


def place(layout, q, k, v, device):
    """q/k/v on `device` in a layout (every spare element is NaN):
      sep        contiguous tensors
      fused_kv   k | v as column halves of one [n*Nkv, 2C] buffer (the model's fused projection)
      fused_qkv  q, k, v as column sections of one [n, N, 3C + guard columns] buffer (needs Nq = Nkv)
      headmajor  storage [n, H, N, D] viewed as [n, N, H, D]: head stride N*D, row stride D
      prefix     k, v as prefix views of a longer cache: batch stride != Nkv * row stride"""
    n, Nq, H, D = q.shape
    Nkv = k.shape[1]
    C_ = H * D
    nan = float("nan")
    if layout == "fused_kv":
        kv = torch.cat([k.reshape(n * Nkv, C_), v.reshape(n * Nkv, C_)], dim=1).to(device)
        return q.to(device), kv[:, :C_].view(n, Nkv, H, D), kv[:, C_:].view(n, Nkv, H, D)
    if layout == "fused_qkv":
        assert Nq == Nkv
        gc = 8
        buf = torch.full((n, Nq, 3 * C_ + 4 * gc), nan, dtype=q.dtype)
        offs = [gc, 2 * gc + C_, 3 * gc + 2 * C_]
        for o, t in zip(offs, (q, k, v)):
            buf[..., o:o + C_] = t.reshape(n, Nq, C_)
        buf = buf.to(device)
        return tuple(buf[..., o:o + C_].view(n, Nq, H, D) for o in offs)
    if layout == "headmajor":
        return tuple(t.permute(0, 2, 1, 3).contiguous().to(device).permute(0, 2, 1, 3) for t in (q, k, v))
    if layout == "prefix":
        caches = []
        for t in (k, v):
            cache = torch.full((n, Nkv + 37, H, D), nan, dtype=t.dtype)
            cache[:, :Nkv] = t
            caches.append(cache.to(device)[:, :Nkv])
        return (q.to(device), *caches)
    assert layout == "sep"
    return q.to(device), k.to(device), v.to(device)


# ---- guarded launches through the C ABI ---------------------------------------------------------------------------------------
def s3(t):
    return t.stride(0), t.stride(1), t.stride(2)


def ws_bytes(dtype, n, Nq, Nkv, H):
    nb = ctypes.c_int64(0)
    assert lib().mm_xattn_ws_bytes(dt(dtype), n, Nq, Nkv, H, ctypes.byref(nb)) == OK
    return nb.value


def run_fwd(q, k, v, scale, p, seed, offset):
    """mm_xattn_fwd with out / lse inside guarded storages; returns (out, lse, [guards])."""
    from multimeditron_amd._lib import call
    n, Nq, H, D = q.shape
    go = Guarded(n * Nq * H * D, q.dtype, q.device)
    gl = Guarded(n * H * Nq, F32, q.device)
    out = go.view((n, Nq, H, D), (Nq * H * D, H * D, D, 1))
    lse = gl.view((n, H, Nq), (H * Nq, Nq, 1))
    call("mm_xattn_fwd", dt(q.dtype), ptr(q), ptr(k), ptr(v), n, Nq, k.shape[1], H, D, *s3(q), *s3(k), *s3(v), float(scale), float(p),
         int(seed), int(offset), ptr(out), ptr(lse), stream())
    return out, lse, [("out", go), ("lse", gl)]


def run_bwd(q, k, v, out, dout, lse, scale, p, seed, offset):
    """mm_xattn_bwd with dq/dk/dv as guarded views mirroring q/k/v and a guarded workspace of exactly mm_xattn_ws_bytes; returns
    (dq, dk, dv, [guards]).  The bf16 kernels write every workspace cell; the fp32 ones only the (key < Nkv, query < Nq) cells,
    so there the guard bands are held and unwritten interior cells are allowed."""
    from multimeditron_amd._lib import call
    n, Nq, H, D = q.shape
    Nkv = k.shape[1]
    (dq, dk, dv), stores = grad_views([q, k, v])
    nb = ws_bytes(q.dtype, n, Nq, Nkv, H)
    gw = Guarded(nb // q.element_size(), q.dtype, q.device)
    ws = gw.view((nb // q.element_size(),), (1,))
    call("mm_xattn_bwd", dt(q.dtype), ptr(q), ptr(k), ptr(v), ptr(out), ptr(dout), ptr(lse), n, Nq, Nkv, H, D, *s3(q), *s3(k), *s3(v),
         float(scale), float(p), int(seed), int(offset), ptr(dq), ptr(dk), ptr(dv), ptr(ws), nb, stream())
    return dq, dk, dv, [(f"dq/dk/dv storage {i}", g) for i, g in enumerate(stores)] + [("workspace", gw, q.dtype == BF)]

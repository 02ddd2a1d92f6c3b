"""mm_cfg_combine (include/mm_hip.h; generate's guidance_scale) in float64 from the storage-rounded operands, with the error scale E
of tests/kernel_check.py's rule -- one term per rounding point of the kernel, never fitted to kernel output -- and the launcher the
GPU tests share.  A helper for tests/test_cfg_cpu.py, tests/test_cfg_combine_gpu.py and tests/test_generate_guidance_gpu.py, not a
test module.

The rounding points, in U32 units (everything the kernel computes is fp32):
  lse of either row   built the way rowwise_check.ce_fwd_reference builds E_lse, from THIS kernel's reduction: the relative error of
                      the sum is its depth -- 16 serial adds per thread, 6 of the wave's butterfly, 3 across the waves, then one
                      multiply and one add per chunk in chunk order (GPT + 9 + 2 C) -- plus expf twice on arguments of size up to R =
                      max - min (the term with its chunk's maximum, the chunk's rescale to the row's maximum), 2 R + 2 ulps each (the
                      argument's own rounding is R u); logf turns it into an absolute error and adds 2 |lse - max|; the add of the
                      maximum rounds |lse|
  y = x - lse         |y|, for both rows
  d = yc - yu         |d|
  t = scale d         |t|
  out = t + yu        |out|
and each incoming error carried through: E = |scale| (Ey_c + Ey_u + |d|) + |t| + Ey_u + |out| with Ey = E_lse + |y|."""
import torch

from tests.kernel_check import RatioLog, U, check_bound, dt, ptr, stream
from multimeditron_amd._lib import call, lib

CHUNK = 4096                  # vocabulary entries per workgroup of the kernel (csrc/mm_cfg.hip)
GPT = 16                      # contiguous entries per thread

# c of kernel_check's rule: the smallest power of two >= 2x the worst err / (u E) measured on the MI355X over
# tests/test_cfg_combine_gpu.py's contract cases (measured: see the figure beside it)
C = 1.0                       # measured worst ratio 0.291 (bf16, magnitudes of +-80); fp32 0.243; N(0, 4^2) logits 0.112
# the same rule for transformers' processor on the CPU (torch's fp32 log_softmax and three tensor operations, another reduction than
# the kernel's): tests/test_cfg_cpu.py holds the restatement to it
C_HF = 0.5                    # measured worst ratio 0.248 (scale 0.0, unconditional ids, first pass)
RATIOS = RatioLog("MM_CFG_RATIO_LOG")


def lse_reference(x):
    """x [rows, V] float64 (finite) -> (lse, E_lse) in U32 units."""
    V = x.shape[-1]
    chunks = -(-V // CHUNK)
    mx = x.max(-1).values
    lse = torch.logsumexp(x, -1)
    R = mx - x.min(-1).values
    return lse, lse.abs() + 2.0 * (lse - mx).abs() + (GPT + 9 + 2 * chunks) + 2.0 * (2.0 * R + 2.0)


def reference(cond, uncond, scale):
    """cond, uncond [rows, V] (the valid columns, bf16 or fp32 as stored) -> (out, E) float64, E in U32 units."""
    xc, xu = cond.double(), uncond.double()
    (lc, Ec), (lu, Eu) = lse_reference(xc), lse_reference(xu)
    yc, yu = xc - lc[:, None], xu - lu[:, None]
    d = yc - yu
    t = float(scale) * d
    out = t + yu
    Eyc, Eyu = Ec[:, None] + yc.abs(), Eu[:, None] + yu.abs()
    return out, abs(float(scale)) * (Eyc + Eyu + d.abs()) + t.abs() + Eyu + out.abs()


def check(name, got, cond, uncond, scale, key=None, c=None):
    """got fp32 [rows, V] against the reference of the operands' valid columns, under check_bound with C (or the path's own c)."""
    ref, E = reference(cond, uncond, scale)
    return check_bound(name, got.detach().cpu(), ref.cpu(), E.cpu(), C if c is None else c, U[torch.float32], key=key, log=RATIOS)


def ws_bytes(rows, V):
    import ctypes
    nb = ctypes.c_int64(0)
    call("mm_cfg_ws_bytes", int(rows), int(V), ctypes.byref(nb))
    return nb.value


def launch(cond, uncond, V, scale, out, ws, nbytes):
    """the raw return code of mm_cfg_combine on views cond / uncond [rows, V] (row strides = their ld) and out [rows, V] fp32."""
    import ctypes
    return lib().mm_cfg_combine(dt(cond.dtype), ptr(cond), cond.stride(0), ptr(uncond), uncond.stride(0), cond.shape[0], V,
                                ctypes.c_float(scale), ptr(out), out.stride(0), ptr(ws), nbytes, stream())

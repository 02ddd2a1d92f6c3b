"""What every kernel checker shares: the acceptance rule, bitwise equality, the ratio log, guarded storages and the C-ABI shims.
The checkers (attn_check, xattn_check, gemm_check, rowwise_check, conv_check) build the references and the error scales; nothing here knows a
kernel family.

The rule (`check_bound`).  A reference is computed in float64 from the SAME storage-rounded operands the kernel reads, together
with an error scale E per element: a sum of absolute values of fp64 terms, one per rounding point of the kernel, never fitted to
kernel output.  A result passes when |got - ref| <= c u E elementwise, with
  u   the unit roundoff of the output's dtype (`U`: 2^-8 bf16, 2^-24 fp32); fp32 terms enter a bf16 output's E scaled by U32 / u;
  c   a constant per launch path (each checker's `C`): the smallest power of two >= 2x the worst err / (u E) measured on the
      MI355X over that checker's contract tests (the measured ratios are written beside each constant);
  E = 0  means no rounding can occur there: the result must EQUAL the reference (the zeros of masked rows, keys and padding).
Every other element must be finite.  The bound is a worst case (sum of |terms|), so it is rigorous and loses power as 1/sqrt(n)
on long sums; each checker's test_*_check_cpu.py shows which kernel mistakes it flags at the sizes the GPU tests use.

Where c is DERIVED instead of measured (the kernel's only rounding to the output dtype is the store, so err / (u E) <= 1, times 2 of
margin; the measured ratio is then only recorded beside it): attn_check's bf16-decode-valu / bf16-decode-mfma / bf16-decode-fused
(mm_attn_decode) and rowwise_check's expert_fuse (mm_expert_fuse, forward and backward = 1).  mm_decode_select is integer
bookkeeping: tests/test_rowwise_contract_gpu.py compares every buffer whole."""
import atexit
import contextlib
import json
import os

import torch

from multimeditron_amd._lib import get_option, lib  # noqa: F401  (get_option: part of the C-ABI shims below)

U = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}
U32 = 2.0 ** -24
SENTINEL = {torch.bfloat16: 0x7FC1, torch.float32: 0x7FC10000}   # quiet NaNs with a payload no kernel produces


class RatioLog(dict):
    """Worst err / (u E) seen per key in this process.  When the environment variable `env` names a file, the log is written
    there as JSON at exit (a tuple key as "path/name")."""

    def __init__(self, env):
        super().__init__()
        if os.environ.get(env):
            atexit.register(self.dump, os.environ[env])

    def record(self, key, ratio):
        self[key] = max(self.get(key, 0.0), ratio)

    def dump(self, path):
        with open(path, "w") as f:
            json.dump({"/".join(k) if isinstance(k, tuple) else k: v for k, v in sorted(self.items())}, f, indent=1)


def coords(idx, shape):
    """flat index -> tuple of coordinates"""
    out = []
    for n in reversed(shape):
        out.append(idx % n)
        idx //= n
    return tuple(out[::-1])


def _first(mask):
    return int(mask.reshape(-1).nonzero()[0])


def check_bound(name, got, ref, E, c, u, *, key=None, log=None, where=None, exact=None):
    """The rule: got == ref where E = 0 or the bool mask `exact` is set (attention's lse, whose reference is +inf there), finite
    and |got - ref| <= c u E everywhere else.  Returns the worst err / (u E) and records it in `log` under `key` when a key is
    given.  `where(flat_index, shape) -> str` words the location of a failure (default: the coordinates)."""
    g = got.detach().to(ref.device, torch.float64)
    assert g.shape == ref.shape, f"{name}: shape {tuple(g.shape)} != {tuple(ref.shape)}"
    at = lambda i: (where or coords)(i, g.shape)
    val = lambda t, i: float(t.reshape(-1)[i])
    exact = E == 0 if exact is None else (E == 0) | exact
    nonfinite = ~torch.isfinite(g) & ~exact
    if bool(nonfinite.any()):
        i = _first(nonfinite)
        raise AssertionError(f"{name}: non-finite {val(g, i)} at {at(i)}, ref {val(ref, i):.6g} ({int(nonfinite.sum())} such elements)")
    bad_exact = exact & ~(g == ref)
    if bool(bad_exact.any()):
        i = _first(bad_exact)
        raise AssertionError(f"{name}: {val(g, i):.6g} where exactly {val(ref, i)} is required (E = 0) at {at(i)} "
                             f"({int(bad_exact.sum())} such elements)")
    ratio = torch.where(exact, torch.zeros_like(g), (g - ref).abs() / (u * torch.where(exact, torch.ones_like(E), E)))
    if ratio.numel() == 0:
        return 0.0
    i = int(ratio.reshape(-1).argmax())
    worst = val(ratio, i)
    if key is not None:
        log.record(key, worst)
    if not worst <= c:
        raise AssertionError(f"{name}: err/(u E) = {worst:.3g} > c = {c} at {at(i)}: got {val(g, i):.6g}, ref {val(ref, i):.6g}, "
                             f"c u E = {c * u * val(E, i):.3g} ({int((ratio > c).sum())} elements over the bound)")
    return worst


def _ints(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check_bits(name, got, want, *, where=None, zero_sign=True):
    """Bitwise equality of every element (got, want: the same dtype).  zero_sign=False compares values instead of the bits of a
    zero: equal values with equal sign bits, or both zero of either sign; a NaN then never matches."""
    g = got.detach()
    w = want.to(g.device)
    assert g.shape == w.shape, f"{name}: shape {tuple(g.shape)} != {tuple(w.shape)}"
    same = _ints(g.contiguous()) == _ints(w.contiguous())
    if not zero_sign:
        same = same & (g == w) | (g == 0) & (w == 0)
    if not bool(same.all()):
        i = _first(~same)
        raise AssertionError(f"{name}: {int((~same).sum())} of {same.numel()} elements differ from the exact result; first at "
                             f"{(where or coords)(i, g.shape)}: got {float(g.reshape(-1)[i])!r}, want {float(w.reshape(-1)[i])!r}")


# ---- guarded storages ------------------------------------------------------------------------------------------------------
def sentinel_fill(t):
    """fill a contiguous tensor with the sentinel NaN of its dtype"""
    _ints(t).fill_(SENTINEL[t.dtype])
    return t


class Guarded:
    """One storage of `numel` elements between guard bands of `pad` elements, all filled with the sentinel NaN.  `view`
    places a strided view at an element offset into the storage (as the operand it mirrors sits in its own storage);
    `verify` asserts that every element outside the views is bit-unchanged and that no sentinel is left inside them
    (require_written=False: only the former, for a scratch buffer whose interior a kernel may leave partly unwritten)."""

    def __init__(self, numel, dtype, device, pad=512):
        self.dtype, self.pad = dtype, pad
        self.buf = sentinel_fill(torch.empty(pad + numel + pad, dtype=dtype, device=device))
        self.covered = torch.zeros(self.buf.numel(), dtype=torch.bool, device=device)
        self.views = []

    def view(self, shape, stride, offset=0):
        v = self.buf.as_strided(shape, stride, self.pad + offset)
        self.covered.as_strided(shape, stride, self.pad + offset).fill_(True)
        self.views.append(v)
        return v

    def verify(self, name, require_written=True):
        iv = _ints(self.buf)
        s = SENTINEL[self.dtype]
        guard_bad = (~self.covered) & (iv != s)
        if bool(guard_bad.any()):
            i = int(guard_bad.nonzero()[0])
            raise AssertionError(f"{name}: write outside the output at storage element {i - self.pad} "
                                 f"(storage [0, {self.buf.numel() - 2 * self.pad}), {int(guard_bad.sum())} elements)")
        left = self.covered & (iv == s)
        if require_written and bool(left.any()):
            i = int(left.nonzero()[0])
            raise AssertionError(f"{name}: {int(left.sum())} output elements never written (first at storage element "
                                 f"{i - self.pad})")


def verify_guards(guards):
    """guards: (name, Guarded) or (name, Guarded, require_written) entries"""
    for name, g, *opt in guards:
        g.verify(name, *opt)


# ---- the C ABI: argument shims, raw return codes, option switches --------------------------------------------------------------
def dt(dtype):
    return 0 if dtype == torch.bfloat16 else 1


def ptr(t):
    return t.data_ptr() if t is not None else None


def stream():
    return torch.cuda.current_stream().cuda_stream


def rc(name, *args):
    """the raw return code of an entry point on the current stream (no exception)."""
    return getattr(lib(), name)(*args, stream())


@contextlib.contextmanager
def options(**kw):
    """Set mm_set_option switches for the block and restore what was there."""
    old = {}
    for k, v in kw.items():
        old[k] = get_option(k)
        assert lib().mm_set_option(k.encode(), int(v)) == 0, (k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            lib().mm_set_option(k.encode(), v)

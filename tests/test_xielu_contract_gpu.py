"""Kernel contract of the xIELU kernels (csrc/mm_xielu.hip) through the C ABI: |got - ref| <= c u E per element against fp64
(tests/xielu_check.py), every output in a NaN-sentinel storage (Guarded), inputs followed by NaN sentinels, two launches bit for bit,
frozen scalars (partials == NULL), refusals by return code with the outputs untouched."""
import ctypes

import pytest
import torch

from tests import xielu_check as XC
from tests.kernel_check import SENTINEL, Guarded, check_bits, dt, lib, rc, sentinel_fill
from tests.kernel_check import ptr as p_
from tests.xielu_check import BF, F32

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = XC.NS + (XC.N_REDUCE_PASSES, XC.N_ITERS2)


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def f(x):
    return ctypes.c_float(x)


def ids(v):
    return XC.NAME[v] if isinstance(v, torch.dtype) else None


def stored(t, spare=64):
    """an input in a storage whose elements past it are NaN sentinels (nothing past n is read)"""
    buf = sentinel_fill(torch.empty(t.numel() + spare, dtype=t.dtype, device=t.device))
    buf[: t.numel()] = t
    return buf[: t.numel()]


def out(n, dtype):
    g = Guarded(n, dtype, DEV)
    return g.view((n,), (1,)), g


def untouched(*guards):
    for g in guards:
        iv = g.buf.view(torch.int16 if g.dtype == BF else torch.int32)
        assert bool((iv == SENTINEL[g.dtype]).all()), "a refused or empty call wrote to its output"


def run_case(dtype, n, scale, case, acc):
    tag = f"xielu {XC.NAME[dtype]} n={n} scale={scale} alpha={case} acc={acc}"
    x, dy = XC.problem(n, dtype, DEV, scale, n)
    x, dy = stored(x), stored(dy)
    ap, an = XC.alphas(case, dtype, DEV)
    beta, eps = XC.BETA, XC.EPS[dtype]
    nb = XC.blocks(n)
    assert lib().mm_xielu_bwd_blocks(n) == nb
    y, gy = out(n, dtype)
    assert rc("mm_xielu_fwd", dt(dtype), p_(x), n, p_(ap), p_(an), f(beta), f(eps), p_(y)) == XC.OK
    dx, gdx = out(n, dtype)
    part, gpart = out(2 * nb, F32)
    assert rc("mm_xielu_bwd", dt(dtype), p_(x), p_(dy), n, p_(ap), p_(an), f(beta), f(eps), p_(dx), p_(part)) == XC.OK
    dp, gdp = out(1, dtype)
    dn, gdn = out(1, dtype)
    old_p = old_n = None
    if acc:
        old_p, old_n = XC.old_values(dtype, DEV)
        dp.copy_(old_p)
        dn.copy_(old_n)
    assert rc("mm_xielu_reduce", dt(dtype), p_(part), nb, p_(ap), p_(an), p_(dp), p_(dn), int(acc), int(acc)) == XC.OK
    torch.cuda.synchronize()
    for name, g in (("y", gy), ("dx", gdx), ("partials", gpart), ("dalpha_p", gdp), ("dalpha_n", gdn)):
        g.verify(f"{tag} {name}")
    ry, Ey = XC.fwd_reference(x, ap, an, beta, eps)
    XC.bound(tag + " y", "y", dtype, y, ry, Ey)
    rdx, Edx = XC.bwd_reference(x, dy, ap, an, beta, eps)
    XC.bound(tag + " dx", "dx", dtype, dx, rdx, Edx)
    (rp, Ep), (rn, En) = XC.dalpha_reference(x, dy, ap, an, beta, eps, old_p, old_n)
    XC.bound(tag + " dalpha_p", "dalpha_p", dtype, dp, rp, Ep)
    XC.bound(tag + " dalpha_n", "dalpha_n", dtype, dn, rn, En)
    # a second launch on the same inputs: the same bits (fixed summation order, no atomics)
    y2, dx2, part2 = torch.empty_like(y.contiguous()), torch.empty_like(dx.contiguous()), torch.empty(2 * nb, device=DEV)
    dp2, dn2 = (old_p.clone(), old_n.clone()) if acc else (torch.empty(1, dtype=dtype, device=DEV), torch.empty(1, dtype=dtype, device=DEV))
    assert rc("mm_xielu_fwd", dt(dtype), p_(x), n, p_(ap), p_(an), f(beta), f(eps), p_(y2)) == XC.OK
    assert rc("mm_xielu_bwd", dt(dtype), p_(x), p_(dy), n, p_(ap), p_(an), f(beta), f(eps), p_(dx2), p_(part2)) == XC.OK
    assert rc("mm_xielu_reduce", dt(dtype), p_(part2), nb, p_(ap), p_(an), p_(dp2), p_(dn2), int(acc), int(acc)) == XC.OK
    # frozen scalars: partials == NULL computes the same dx and nothing else
    dx3, gdx3 = out(n, dtype)
    assert rc("mm_xielu_bwd", dt(dtype), p_(x), p_(dy), n, p_(ap), p_(an), f(beta), f(eps), p_(dx3), None) == XC.OK
    torch.cuda.synchronize()
    gdx3.verify(tag + " dx (frozen)")
    for name, a, b in (("y", y2, y), ("dx", dx2, dx), ("partials", part2, part), ("dalpha_p", dp2, dp), ("dalpha_n", dn2, dn), ("dx frozen", dx3, dx)):
        check_bits(f"{tag} {name} rerun", a, b.contiguous())


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", [BF, F32], ids=ids)
def test_xielu_contract(dtype, n):
    for scale, case, acc in XC.contract_cases(n):
        run_case(dtype, n, scale, case, acc)


def test_sizes_cover_the_paths():
    assert {XC.blocks(n) for n in SIZES} >= {1, 2, 147, 601}
    assert XC.iters(XC.N_ITERS2) == 2 and -(-XC.blocks(XC.N_REDUCE_PASSES) // 256) == 3
    assert any(n % 8 and n > 8 for n in SIZES) and 8 in SIZES


@pytest.mark.parametrize("dtype", [BF, F32], ids=ids)
def test_frozen_scalars_through_the_wrapper(dtype):
    """kernels.xielu_bwd(want_dalpha=False) allocates no partials and the scalar gradients' storage stays as it was"""
    from multimeditron_amd import kernels as K
    x, dy = XC.problem(4100, dtype, DEV, 1.0, 3)
    ap, an = XC.alphas("init", dtype, DEV)
    dp, gdp = out(1, dtype)
    dx, partials = K.xielu_bwd(x, dy, ap, an, XC.BETA, XC.EPS[dtype], want_dalpha=False)
    dx_t, partials_t = K.xielu_bwd(x, dy, ap, an, XC.BETA, XC.EPS[dtype])
    torch.cuda.synchronize()
    assert partials is None and partials_t.shape == (XC.blocks(4100), 2)
    check_bits("dx frozen vs trained", dx, dx_t)
    untouched(gdp)


@pytest.mark.parametrize("dtype", [BF, F32], ids=ids)
def test_argument_errors_return_before_launch(dtype):
    n = 100
    x, dy = XC.problem(n, dtype, DEV, 1.0, 1)
    big_x = stored(torch.cat([x, x]))
    ap, an = XC.alphas("init", dtype, DEV)
    b, e = f(XC.BETA), f(XC.EPS[dtype])
    y, gy = out(n, dtype)
    dx, gdx = out(n, dtype)
    part, gpart = out(2, F32)
    dp, gdp = out(1, dtype)
    dn, gdn = out(1, dtype)
    d = dt(dtype)
    off = big_x[1: n + 1]                                             # not 16-byte aligned
    calls = [
        (("mm_xielu_fwd", d, None, n, p_(ap), p_(an), b, e, p_(y)), XC.ERR_ARG),
        (("mm_xielu_fwd", d, p_(x), n, None, p_(an), b, e, p_(y)), XC.ERR_ARG),
        (("mm_xielu_fwd", d, p_(x), n, p_(ap), None, b, e, p_(y)), XC.ERR_ARG),
        (("mm_xielu_fwd", d, p_(x), n, p_(ap), p_(an), b, e, None), XC.ERR_ARG),
        (("mm_xielu_fwd", d, p_(x), -1, p_(ap), p_(an), b, e, p_(y)), XC.ERR_ARG),
        (("mm_xielu_fwd", 2, p_(x), n, p_(ap), p_(an), b, e, p_(y)), XC.ERR_UNSUPPORTED),
        (("mm_xielu_fwd", d, p_(off), n, p_(ap), p_(an), b, e, p_(y)), XC.ERR_ALIGN),
        (("mm_xielu_fwd", d, p_(x), 0, p_(ap), p_(an), b, e, p_(y)), XC.OK),
        (("mm_xielu_bwd", d, None, p_(dy), n, p_(ap), p_(an), b, e, p_(dx), p_(part)), XC.ERR_ARG),
        (("mm_xielu_bwd", d, p_(x), None, n, p_(ap), p_(an), b, e, p_(dx), p_(part)), XC.ERR_ARG),
        (("mm_xielu_bwd", d, p_(x), p_(dy), n, p_(ap), p_(an), b, e, None, p_(part)), XC.ERR_ARG),
        (("mm_xielu_bwd", d, p_(x), p_(dy), -5, p_(ap), p_(an), b, e, p_(dx), p_(part)), XC.ERR_ARG),
        (("mm_xielu_bwd", 7, p_(x), p_(dy), n, p_(ap), p_(an), b, e, p_(dx), p_(part)), XC.ERR_UNSUPPORTED),
        (("mm_xielu_bwd", d, p_(off), p_(dy), n, p_(ap), p_(an), b, e, p_(dx), p_(part)), XC.ERR_ALIGN),
        (("mm_xielu_bwd", d, p_(x), p_(dy), 0, p_(ap), p_(an), b, e, p_(dx), p_(part)), XC.OK),
        (("mm_xielu_reduce", d, None, 1, p_(ap), p_(an), p_(dp), p_(dn), 0, 0), XC.ERR_ARG),
        (("mm_xielu_reduce", d, p_(part), 1, p_(ap), p_(an), None, p_(dn), 0, 0), XC.ERR_ARG),
        (("mm_xielu_reduce", d, p_(part), -1, p_(ap), p_(an), p_(dp), p_(dn), 0, 0), XC.ERR_ARG),
        (("mm_xielu_reduce", 2, p_(part), 1, p_(ap), p_(an), p_(dp), p_(dn), 0, 0), XC.ERR_UNSUPPORTED),
    ]
    for args, want in calls:
        assert rc(*args) == want, (args[0], want)
    torch.cuda.synchronize()
    untouched(gy, gdx, gpart, gdp, gdn)
    assert lib().mm_xielu_bwd_blocks(0) == 0 and lib().mm_xielu_bwd_blocks(-3) == 0

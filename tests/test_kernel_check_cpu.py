"""The shared rule of tests/kernel_check.py, held to its own definition on the CPU: what check_bound, check_bits, RatioLog and
Guarded accept and reject at the edges where the per-family copies they replace used to differ (an element just under / over
c u E, non-finite values, E = 0, an infinite reference, the sign of zero, a shape that merely broadcasts, the guard bands)."""
import json
import math

import pytest
import torch

from tests import kernel_check as KC

DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "f32"]
C = 8.0
I, Z = (1, 7), (2, 3)                    # a bounded element and an exact-required one (E = 0)


def problem(dtype):
    """ref, E [12, 32] fp64 with |ref| in 2 .. 6 and E = 1.25 |ref|; ref = E = 0 on one element in ten; got = dtype(ref): a pass."""
    g = torch.Generator().manual_seed(3)
    ref = torch.randn(12, 32, generator=g, dtype=torch.float64)
    ref = ref + 3.0 * torch.sign(ref)
    zero = torch.rand(12, 32, generator=g) < 0.1
    zero[Z], zero[I] = True, False
    ref[zero] = 0.0
    return ref, ref.abs() * 1.25, ref.to(dtype)


def put(t, at, value):
    t = t.clone()
    t[at] = value
    return t


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bound_accepts_up_to_c_and_rejects_past_it(dtype):
    ref, E, got = problem(dtype)
    u = KC.U[dtype]
    log = KC.RatioLog("MM_NO_SUCH_LOG")
    assert KC.check_bound("x", got, ref, E, C, u, key="p", log=log) <= 1.0 / 1.25               # one rounding: err <= u |ref|
    r = float(ref[I])
    # dtype(r (1 + k u)) is within u |r| (1 + k u) of r (1 + k u): err / (u E) lies in (k -+ 1.1) / 1.25
    worst = KC.check_bound("x", put(got, I, r * (1 + 8 * u)), ref, E, C, u, key="p", log=log)
    assert 6.9 / 1.25 <= worst <= 9.1 / 1.25 < C and log["p"] == worst
    with pytest.raises(AssertionError, match=r"err/\(u E\) = .* > c = 8.0 at \(1, 7\).*\(1 elements over the bound\)"):
        KC.check_bound("x", put(got, I, r * (1 + 12 * u)), ref, E, C, u, key="p", log=log)
    assert log["p"] > C                                           # the failing ratio is recorded before the check raises
    with pytest.raises(AssertionError, match="at tile 39"):
        KC.check_bound("x", put(got, I, r * (1 + 12 * u)), ref, E, C, u, where=lambda i, shape: f"tile {i}")
    assert KC.check_bound("x", got[:0], ref[:0], E[:0], C, u) == 0.0


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bound_non_finite_exact_and_shape(dtype):
    ref, E, got = problem(dtype)
    u = KC.U[dtype]
    for bad in (math.nan, math.inf):
        with pytest.raises(AssertionError, match=r"non-finite .* \(1 such elements\)"):
            KC.check_bound("x", put(got, I, bad), ref, E, math.inf, u)                   # no c lets a non-finite value through
    for bad in (1e-30, math.nan, -math.inf):
        with pytest.raises(AssertionError, match=r"where exactly 0.0 is required .* \(1 such elements\)"):
            KC.check_bound("x", put(got, Z, bad), ref, E, math.inf, u)
    KC.check_bound("x", put(got, Z, -0.0), ref, E, C, u)                                  # -0 == +0
    with pytest.raises(AssertionError, match="shape"):
        KC.check_bound("x", got[:1], ref[:1].expand(12, 32), E[:1].expand(12, 32), C, u)  # would broadcast to a pass
    # the `exact` mask: attention's lse, +inf on a row with no visible key -- accepted there and nowhere else
    ref_l, got_l, E = put(ref, Z, math.inf), put(got.float(), Z, math.inf), put(E, Z, 1.0)
    mask = torch.isinf(ref_l)
    with pytest.raises(AssertionError, match="non-finite inf"):
        KC.check_bound("lse", got_l, ref_l, E, C, u)                                      # without the mask +inf is non-finite
    assert KC.check_bound("lse", got_l, ref_l, E, C, u, exact=mask) <= 1.0 / 1.25
    for bad in (3.0e38, -math.inf, math.nan):
        with pytest.raises(AssertionError, match="where exactly inf is required"):
            KC.check_bound("lse", put(got_l, Z, bad), ref_l, E, C, u, exact=mask)
    with pytest.raises(AssertionError, match="non-finite inf"):
        KC.check_bound("lse", put(got_l, I, math.inf), ref_l, E, C, u, exact=mask)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bits_strict_and_zero_sign(dtype):
    want = problem(dtype)[2]
    ulp = want.clone()
    KC._ints(ulp)[I] += 1
    nan = put(want, I, math.nan)
    for zero_sign in (True, False):
        KC.check_bits("x", want, want, zero_sign=zero_sign)
        KC.check_bits("x", want.t(), want.clone().t(), zero_sign=zero_sign)                # strided views
        for bad in (ulp, nan, want.reshape(-1)):
            with pytest.raises(AssertionError):
                KC.check_bits("x", bad, want, zero_sign=zero_sign)
    with pytest.raises(AssertionError, match="1 of 384 elements differ from the exact result; first at tile 67"):
        KC.check_bits("x", put(want, Z, -0.0), want, where=lambda i, shape: f"tile {i}")
    KC.check_bits("x", put(want, Z, -0.0), want, zero_sign=False)
    KC.check_bits("x", nan, nan)                                                          # the same bits
    with pytest.raises(AssertionError):
        KC.check_bits("x", nan, nan, zero_sign=False)                                     # values: a NaN never matches


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_guard_bands_and_unwritten_elements(dtype):
    def guarded():
        g = KC.Guarded(200, dtype, "cpu", pad=64)
        g.view((10, 16), (20, 1), 3).fill_(1.0)
        return g
    guarded().verify("y")
    for at in (64 + 3 + 16, 5, 64 + 200):                       # the row padding, the band in front, the band behind
        g = guarded()
        g.buf[at] = 0.0
        with pytest.raises(AssertionError, match="write outside the output"):
            KC.verify_guards([("y", g)])
    g = guarded()
    KC.sentinel_fill(g.buf[64 + 3 + 20:64 + 3 + 21])
    with pytest.raises(AssertionError, match="1 output elements never written"):
        g.verify("y")
    g.verify("y", require_written=False)                        # a scratch buffer: only the bands are held
    KC.verify_guards([("y", g, False)])
    g.buf[5] = 0.0
    with pytest.raises(AssertionError, match="write outside the output"):
        KC.verify_guards([("y", g, False)])


def test_ratio_log_keeps_the_maximum_and_dumps_at_exit(tmp_path, monkeypatch):
    registered = []
    monkeypatch.setattr(KC.atexit, "register", lambda fn, *a: registered.append((fn, a)))
    assert KC.RatioLog("MM_NO_SUCH_LOG") == {} and not registered
    monkeypatch.setenv("MM_SOME_RATIO_LOG", str(tmp_path / "r.json"))
    for keys, want in (((("f32", "out"), ("f32", "out"), ("bf16", "dq")), {"bf16/dq": 1.5, "f32/out": 0.5}),       # "path/name"
                       (("linear", "act", "linear"), {"act": 0.25, "linear": 1.5})):                           # the plain path
        log = KC.RatioLog("MM_SOME_RATIO_LOG")
        for key, r in zip(keys, (0.5, 0.25, 1.5)):
            log.record(key, r)
        fn, args = registered.pop()
        fn(*args)
        assert json.load(open(tmp_path / "r.json")) == want and not registered

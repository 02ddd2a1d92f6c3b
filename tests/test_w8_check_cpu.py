"""The MXFP8 weight-only format as tests/w8_check.py restates it (CPU): the properties the decode path relies on, each derived from
the format and not from any kernel's output.

  * W' = element * 2^(byte - 127) is exactly a bf16 number: e4m3 carries at most 4 significant bits, and the lower clamp of the
    scale byte (27) keeps the product a normal number;
  * the scale rule puts the scaled amax in (224, 448], so no element saturates, and an element with |w| >= amax * 2^-13 has
    |w * 2^-e| >= 224 * 2^-13 > 2^-6, the smallest e4m3 normal: 3 mantissa bits, relative error <= 2^-4;
  * quantising W' again changes nothing (every W' element is representable under its block's scale);
  * the OCP "floor" rule (e = floor(log2 amax) - 8 always) would saturate a block's largest element when amax * 2^-e0 is in
    (448, 512): the counterexample that motivates the rule."""
import pytest
import torch

from tests import w8_check as W8

SHAPES = [(17, 256), (3, 4128), (64, 32)]


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def case(request):
    N, K = request.param
    w = W8.sample_matrix(N, K, seed=N + K)
    q, byte, scaled = W8.quant_ref(w, want_scaled=True)
    return w, q, byte, scaled


def _blocks(t):
    return t.reshape(t.shape[0], -1, W8.BLOCK)


def test_dequantised_matrix_is_exactly_bf16(case):
    w, q, byte, _ = case
    f = W8.dequant_f32(q, byte)
    assert torch.isfinite(f).all()
    assert torch.equal(f.to(torch.bfloat16).float(), f)
    nz = f != 0
    assert (f[nz].abs() >= 2.0 ** -126).all()                 # normal numbers: nothing depends on a denormal mode


def test_no_element_saturates_and_the_scaled_amax_fills_the_range(case):
    w, q, byte, scaled = case
    assert (scaled.abs() <= W8.E4M3_MAX).all()                # the clamp in front of the conversion is never active
    assert torch.isfinite(q.float()).all()
    amax_s = _blocks(scaled).abs().amax(dim=-1)
    free = (byte > 27) & (_blocks(w.float()).abs().amax(dim=-1) > 0)      # blocks the lower clamp of the byte did not touch
    assert free.any()
    assert (amax_s[free] > 224).all() and (amax_s[free] <= 448).all()


def test_relative_error_of_the_elements_that_matter(case):
    w, q, byte, _ = case
    wf, wd = w.float(), W8.dequant_f32(q, byte)
    amax = _blocks(wf).abs().amax(dim=-1, keepdim=True).expand(-1, -1, W8.BLOCK).reshape(wf.shape)
    free = (byte > 27).unsqueeze(-1).expand(-1, -1, W8.BLOCK).reshape(wf.shape)
    big = (wf.abs() >= amax * 2.0 ** -13) & (wf != 0) & free
    assert big.any()
    rel = ((wd - wf).abs() / wf.abs())[big]
    assert float(rel.max()) <= 2.0 ** -4, float(rel.max())
    assert torch.equal(torch.signbit(wd), torch.signbit(wf))  # signs, of zeros and of underflows too


def test_requantising_the_dequantised_matrix_reproduces_it(case):
    w, q, byte, _ = case
    wd = W8.dequant_ref(q, byte)
    wd2 = W8.roundtrip_ref(wd)
    assert torch.equal(wd2.view(torch.int16), wd.view(torch.int16))


def test_zero_blocks():
    w = torch.zeros(2, 64, dtype=torch.bfloat16)
    w[0, 3] = -0.0
    w[1, 40:] = -0.0
    w[1, 0] = 1.0
    q, byte = W8.quant_ref(w)
    assert byte.tolist() == [[127, 127], [127 - 8, 127]]      # amax = 1: e = -8, 1 * 2^8 = 256
    wd = W8.dequant_ref(q, byte)
    assert torch.equal(wd.view(torch.int16), w.view(torch.int16))


@pytest.mark.parametrize("shift", [-40, 0, 33])
def test_scale_rule_at_the_448_boundary(shift):
    """amax = m * 2^shift with m just below, at and just above 1.75: amax * 2^-e0 = m * 2^8 against 448 = 1.75 * 2^8."""
    e0 = shift - 8
    for m, want in ((1.7421875, e0), (1.75, e0), (1.7578125, e0 + 1)):
        w = torch.zeros(1, 32)
        w[0, 7] = -m * 2.0 ** shift
        w[0, 8] = 2.0 ** shift
        w = w.to(torch.bfloat16)
        assert float(w[0, 7]) == -m * 2.0 ** shift            # representable: 7 mantissa bits
        q, byte, scaled = W8.quant_ref(w, want_scaled=True)
        assert int(byte[0, 0]) - 127 == want, (m, int(byte[0, 0]) - 127, want)
        assert float(scaled.abs().max()) <= 448
        # the largest element is kept to e4m3's half-ulp, 2^-4 relative: the floor rule would have clamped 1.7578125 * 2^8 = 450 to 448
        wd = W8.dequant_ref(q, byte)
        assert abs(float(wd[0, 7]) - float(w[0, 7])) <= 2.0 ** -4 * abs(float(w[0, 7]))


def test_floor_rule_counterexample():
    """Under e = e0 always, a block whose amax * 2^-e0 is in (448, 512) loses its largest element to the clamp: up to 12 %."""
    amax = 1.9921875                                          # 0x7F mantissa: 510 after scaling by 2^8
    clamped = min(amax * 2.0 ** 8, 448.0) * 2.0 ** -8
    assert (amax - clamped) / amax > 0.12
    w = torch.zeros(1, 32, dtype=torch.bfloat16)
    w[0, 0] = amax
    q, byte = W8.quant_ref(w)
    assert int(byte[0, 0]) == 127 - 7                         # the rule here: e0 + 1
    assert float(W8.dequant_ref(q, byte)[0, 0]) == 2.0        # 255 is a tie of 240 | 256: to even -> 256, 0.4 % off, not 12 %


def test_lower_clamp_of_the_scale_byte():
    """Blocks below 2^-92 share the byte 27: their elements round on the 2^-109 grid of that scale, normal bf16 numbers or zero."""
    w = torch.zeros(1, 64, dtype=torch.bfloat16)
    w[0, 0] = 2.0 ** -100
    w[0, 1] = -2.0 ** -120                                   # below half the grid: -0
    w[0, 32] = 2.0 ** -130                                   # a bf16 subnormal
    q, byte = W8.quant_ref(w)
    assert byte.tolist() == [[27, 27]]
    wd = W8.dequant_ref(q, byte)
    assert float(wd[0, 0]) == 2.0 ** -100
    assert float(wd[0, 1]) == 0.0 and bool(torch.signbit(wd[0, 1]))
    assert float(wd[0, 32]) == 0.0

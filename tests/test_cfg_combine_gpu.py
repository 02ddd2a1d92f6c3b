"""mm_cfg_combine on the GPU against tests/cfg_check.py's fp64 reference under kernel_check's bound: the smallest shapes at which the
kernel can go wrong (V below one thread's 16 entries, one short of a chunk, a chunk, one over, three chunks and one entry; 1, 3 and 8
pairs; bf16 and fp32), rows of ld = V + 5 (the scalar path; NaN poison behind V in the inputs, the sentinel NaN behind V in the
output) and rows whose base and stride allow the 16-byte path, guarded storages around the output and the workspace; N(0, 4^2)
logits, a constant row, magnitudes of +-80, a pair of bit-equal rows (the same output bits at every scale); equal bits on a second
launch."""
import math

import pytest
import torch

from multimeditron_amd import kernels as K
from tests import cfg_check as CC
from tests.kernel_check import Guarded, check_bits, verify_guards

pytestmark = pytest.mark.gpu

VS, PAIRS, DTYPES, LAYOUTS = (3, 4095, 4096, 4097, 12289), (1, 3, 8), (torch.bfloat16, torch.float32), ("V+5", "aligned")
KINDS = ("normal", "constant", "pm80", "equal")
GRID = [(V, rows, dtype, lay) for V in VS for rows in PAIRS for dtype in DTYPES for lay in LAYOUTS]


def _ld(V, layout):
    return V + 5 if layout == "V+5" else (V + 63) // 64 * 64 + 64


def _values(kind, rows, V, gen):
    """(cond, uncond) fp32 [rows, V] on the host"""
    if kind == "constant":
        c = torch.full((rows, V), 2.5)
        return c, torch.randn(rows, V, generator=gen) * 4.0
    if kind == "pm80":
        sign = lambda: torch.where(torch.rand(rows, V, generator=gen) < 0.5, -1.0, 1.0)
        return 80.0 * sign(), 80.0 * sign() + torch.randn(rows, V, generator=gen)
    c = torch.randn(rows, V, generator=gen) * 4.0
    return c, (c.clone() if kind == "equal" else torch.randn(rows, V, generator=gen) * 4.0)


def _padded(x, ld, dtype):
    """[rows, ld] on the device in `dtype`, NaN behind V -> its [rows, V] view"""
    t = torch.full((x.shape[0], ld), float("nan"), dtype=dtype)
    t[:, :x.shape[1]] = x.to(dtype)
    return t.cuda()[:, :x.shape[1]]


def _run(cond, uncond, V, scale, ld_out):
    """one call into guarded storages -> (out [rows, V] view on the device, the guards)"""
    rows = cond.shape[0]
    nbytes = CC.ws_bytes(rows, V)
    g_out = Guarded(rows * ld_out, torch.float32, "cuda")
    g_ws = Guarded(max(4, nbytes // 4), torch.float32, "cuda")
    out = g_out.view((rows, V), (ld_out, 1))
    ws = g_ws.view((max(4, nbytes // 4),), (1,))
    assert CC.launch(cond, uncond, V, scale, out, ws, nbytes) == 0
    torch.cuda.synchronize()
    return out, [("out", g_out), ("workspace", g_ws, False)]


@pytest.mark.parametrize("n", range(len(GRID)), ids=[f"V{v}-r{r}-{str(d).split('.')[-1]}-{lay}" for v, r, d, lay in GRID])
def test_combine_is_within_the_bound(n):
    V, rows, dtype, layout = GRID[n]
    gen = torch.Generator().manual_seed(1000 + n)
    ld = _ld(V, layout)
    for kind in KINDS:
        c_host, u_host = _values(kind, rows, V, gen)
        cond, uncond = _padded(c_host, ld, dtype), _padded(u_host, ld, dtype)
        scale = {"normal": 1.5, "constant": -0.75, "pm80": 3.0, "equal": 1.5}[kind]
        out, guards = _run(cond, uncond, V, scale, ld)
        verify_guards(guards)                                  # nothing outside out[:, :V] and the workspace, every score written
        CC.check(f"{kind}", out, cond.cpu(), uncond.cpu(), scale, key=("cfg", f"{str(dtype).split('.')[-1]}-{kind}"))
        again, guards2 = _run(cond, uncond, V, scale, ld)
        verify_guards(guards2)
        check_bits(f"{kind}: the second launch", again, out)
        if kind == "constant":                                 # against itself at scale 0: out = y = -log V in every entry
            ref = CC.reference(cond.cpu(), cond.cpu(), 0.0)[0]
            assert float((ref + math.log(V)).abs().max()) < 1e-12
            CC.check("constant row alone", _run(cond, cond.clone(), V, 0.0, ld)[0], cond.cpu(), cond.cpu(), 0.0)
        if kind == "equal":                                    # yc - yu is exactly 0: the scale cannot show
            other, _ = _run(cond, uncond, V, 7.0, ld)
            check_bits("equal rows: scale 7.0 against scale 1.5", other, out)


def test_one_logits_tensor_through_the_wrapper():
    """K.cfg_combine: the conditional rows [0, B) and the unconditional rows [B, 2 B) of ONE padded logits tensor, as generate hands
    them over; V = 128 258 (32 chunks, the last one short), bf16, 2 pairs"""
    V, B = 128258, 2
    gen = torch.Generator().manual_seed(7)
    x = _padded(torch.randn(2 * B, V, generator=gen) * 4.0, (V + 63) // 64 * 64, torch.bfloat16)
    st = K.GuidanceState(B, V, "cuda")
    out = K.cfg_combine(x, st, 3.0)
    torch.cuda.synchronize()
    assert out.shape == (B, V) and out.dtype == torch.float32 and out.data_ptr() == st.out.data_ptr()
    CC.check("wrapper", out, x[:B].cpu(), x[B:].cpu(), 3.0, key=("cfg", "wrapper-128258"))


def test_the_cases_cover_the_chunk_edges_paths_and_values():
    assert {3, 4095, 4096, 4097, 12289} <= {g[0] for g in GRID} and {1, 3, 8} <= {g[1] for g in GRID}
    assert {torch.bfloat16, torch.float32} == {g[2] for g in GRID}
    assert any(V < CC.GPT for V in VS) and any(V % CC.CHUNK == CC.CHUNK - 1 for V in VS) and any(V % CC.CHUNK == 0 for V in VS)
    assert any(V % CC.CHUNK == 1 and V > 2 * CC.CHUNK for V in VS) and any(V % CC.CHUNK == 1 and V < 2 * CC.CHUNK for V in VS)
    for V in VS:
        for es in (2, 4):
            assert (_ld(V, "aligned") * es) % 16 == 0 and _ld(V, "aligned") % 4 == 0          # the 16-byte path
        assert _ld(V, "V+5") == V + 5 and ((V + 5) * 2 % 16 or V < CC.GPT)                      # the scalar path (V = 3: no full group)
    assert set(KINDS) == {"normal", "constant", "pm80", "equal"}

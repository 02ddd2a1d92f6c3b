"""Classifier-free guidance without a GPU: tests/cfg_check.py -- the fp64 restatement every GPU test of mm_cfg_combine is held to --
against transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor run on the CPU in fp32; the checker flags the mistakes a
combine kernel can make, at the GPU test's sizes; the two entry points are declared, exported, bound and refuse what they cannot run
before any launch; and the build's resource remarks of the new kernels show no scratch and no spills."""
import ctypes
import os
import re

import pytest
import torch

from multimeditron_amd import _lib
from tests import cfg_check as CC

BUILD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multimeditron_amd", "csrc", "build")
ARG, ALIGN = -1, -2
BF16, F32 = 0, 1


# ---- the restatement against transformers -----------------------------------------------------------------------------------------
class _Out(dict):
    logits = property(lambda self: self["logits"])


class _Stub:
    """a `model` for the processor: fixed logits per call, an empty cache, and a record of what it was asked"""

    def __init__(self, logits):
        self.logits, self.calls = logits, []

    def __call__(self, input_ids, attention_mask=None, use_cache=None, past_key_values=None):
        self.calls.append((input_ids.clone(), attention_mask.clone()))
        return _Out(logits=self.logits[len(self.calls) - 1], past_key_values=None)


@pytest.mark.parametrize("scale", [1.5, 0.0])
@pytest.mark.parametrize("with_ids", [False, True], ids=["default-negative", "unconditional-ids"])
def test_restatement_is_transformers_processor(scale, with_ids):
    tf = pytest.importorskip("transformers")
    from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor

    torch.manual_seed(11)
    B, V = 3, 4097
    prompt = torch.randint(0, V, (B, 5))
    uncond_ids = torch.randint(0, V, (B, 2)) if with_ids else None
    cond = [torch.randn(B, V) * 4.0 for _ in range(2)]
    # the model answers with every position's logits; the processor reads the last one
    uncond = [torch.randn(B, 2 if with_ids else 1, V) * 4.0, torch.randn(B, 1, V) * 4.0]
    stub = _Stub(uncond)
    proc = UnbatchedClassifierFreeGuidanceLogitsProcessor(scale, stub, unconditional_ids=uncond_ids)
    ids = prompt
    for step in range(2):                                    # its first pass and a later one
        got = proc(ids, cond[step])
        assert got.dtype == torch.float32
        CC.check(f"step {step}", got, cond[step], uncond[step][:, -1], scale, key=("hf", f"{scale}-{with_ids}-{step}"), c=CC.C_HF)
        ids = torch.cat([ids, torch.randint(0, V, (B, 1))], dim=1)
    first, later = stub.calls
    want = uncond_ids if with_ids else prompt[:, -1:]        # without unconditional ids: the last prompt id, one position
    assert torch.equal(first[0], want) and torch.equal(first[1], torch.ones_like(want))
    assert torch.equal(later[0], ids[:, -2:-1]) and later[1].shape == (B, want.shape[1] + 1) and bool(later[1].all())


# ---- the checker flags mistakes ---------------------------------------------------------------------------------------------------
SIZES = [(V, rows) for V in (3, 4095, 4096, 4097, 12289) for rows in (1, 3, 8)]


def _lsm(x, skip_chunk=None):
    if skip_chunk is not None:
        keep = torch.ones(x.shape[-1], dtype=torch.bool)
        keep[skip_chunk * CC.CHUNK:(skip_chunk + 1) * CC.CHUNK] = False
        return x - torch.logsumexp(x[:, keep], -1, keepdim=True)
    return x - torch.logsumexp(x, -1, keepdim=True)


def _mistakes(xc, xu, s, V, rows):
    yc, yu = _lsm(xc), _lsm(xu)
    out = {"swapped": s * (yu - yc) + yc, "scale-on-the-wrong-term": (yc - yu) + s * yu}
    if V > CC.CHUNK:
        out["chunk-left-out"] = s * (_lsm(xc, 0) - yu) + yu
    if rows > 1:
        wrong = xu - torch.logsumexp(xu, -1, keepdim=True).roll(1, 0)
        out["lse-of-the-wrong-row"] = s * (yc - wrong) + wrong
    return out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("V,rows", SIZES, ids=[f"V{v}-r{r}" for v, r in SIZES])
def test_checker_flags_mistakes(V, rows, dtype):
    torch.manual_seed(V * 31 + rows)
    cond, uncond = (torch.randn(rows, V) * 4.0).to(dtype), (torch.randn(rows, V) * 4.0).to(dtype)
    s = 1.5
    xc, xu = cond.double(), uncond.double()
    right = (s * (_lsm(xc) - _lsm(xu)) + _lsm(xu)).float()
    CC.check("the formula itself", right, cond, uncond, s)
    wrong = _mistakes(xc, xu, s, V, rows)
    assert {"swapped", "scale-on-the-wrong-term"} <= set(wrong)
    for name, got in wrong.items():
        with pytest.raises(AssertionError, match="err/"):
            CC.check(name, got.float(), cond, uncond, s)


def test_the_mistakes_cover_chunks_and_rows():
    assert any(V > CC.CHUNK for V, _ in SIZES) and any(r > 1 for _, r in SIZES)
    assert any(V % CC.CHUNK == 1 for V, _ in SIZES) and any(V == CC.CHUNK for V, _ in SIZES) and any(V < CC.GPT for V, _ in SIZES)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
NEW = ("mm_cfg_ws_bytes", "mm_cfg_combine")


def test_symbols_declared_exported_and_bound():
    protos = _lib.parse_header()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in protos, f"include/mm_hip.h does not declare {name}"
        assert hasattr(L, name), f"libmmhip.so does not export {name}"
    assert len(protos["mm_cfg_ws_bytes"][1]) == 3 and len(protos["mm_cfg_combine"][1]) == 13
    assert protos["mm_cfg_combine"][1][7] is ctypes.c_float and protos["mm_cfg_combine"][1][11] is ctypes.c_int64
    from multimeditron_amd import kernels as K
    assert callable(K.cfg_combine) and isinstance(K.GuidanceState, type)
    assert _lib.lib().mm_cfg_combine.argtypes == protos["mm_cfg_combine"][1]


def test_refusals_come_before_any_launch():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1 << 16)
    p = (ctypes.addressof(buf) + 15) & ~15
    a, b, o, w = p, p + 4096, p + 8192, p + 16384
    nb = ctypes.c_int64(0)
    assert L.mm_cfg_ws_bytes(3, 4097, ctypes.byref(nb)) == 0 and nb.value == 2 * 2 * 3 * 2 * 4
    need = nb.value
    assert L.mm_cfg_ws_bytes(0, 5, ctypes.byref(nb)) == 0 and nb.value == 0
    assert L.mm_cfg_ws_bytes(-1, 5, ctypes.byref(nb)) == ARG and L.mm_cfg_ws_bytes(1, 0, ctypes.byref(nb)) == ARG
    assert L.mm_cfg_ws_bytes(1, (1 << 24) + 1, ctypes.byref(nb)) == ARG and L.mm_cfg_ws_bytes(1, 5, None) == ARG
    assert L.mm_cfg_ws_bytes(1, 1 << 24, ctypes.byref(nb)) == 0

    def comb(dtype=BF16, cond=a, ld_c=4104, uncond=b, ld_u=4104, rows=3, V=4097, scale=1.5, out=o, ld_out=4104, ws=w, wb=need):
        return L.mm_cfg_combine(dtype, cond, ld_c, uncond, ld_u, rows, V, ctypes.c_float(scale), out, ld_out, ws, wb, None)

    assert comb(rows=-1) == ARG and comb(V=0) == ARG and comb(V=-3) == ARG
    assert comb(V=(1 << 24) + 1, ld_c=1 << 25, ld_u=1 << 25, ld_out=1 << 25, wb=1 << 30) == ARG
    assert comb(ld_c=4096) == ARG and comb(ld_u=4096) == ARG and comb(ld_out=4096) == ARG
    assert comb(scale=float("inf")) == ARG and comb(scale=float("-inf")) == ARG and comb(scale=float("nan")) == ARG
    for name in ("cond", "uncond", "out", "ws"):
        assert comb(**{name: None}) == ARG, name
    assert comb(wb=need - 1) == ARG and comb(wb=0) == ARG
    assert comb(out=a) == ARG and comb(out=b) == ARG
    assert comb(dtype=2) == ARG
    assert comb(ws=w + 4) == ALIGN and comb(ws=w + 8) == ALIGN
    assert comb(rows=-1, ws=w + 4) == ARG                       # the shape's code comes first
    assert comb(rows=0) == 0 and comb(rows=0, wb=0) == 0


# ---- the build ------------------------------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch_and_do_not_spill():
    path = os.path.join(BUILD, "mm_cfg.o.resources.txt")
    if not os.path.exists(path):
        pytest.skip("library not built in this tree (python multimeditron_amd/csrc/build.py)")
    out, cur = {}, None
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            cur = out.setdefault(m.group(1), {})
        for field, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
                           ("vgpr_spill", r"VGPRs Spill: (\d+)")):
            m = re.search(pat, ln)
            if m and cur is not None:
                cur[field] = int(m.group(1))
    new = {n: r for n, r in out.items() if "cfg_part_kernel" in n or "cfg_combine_kernel" in n}
    assert len(new) == 4, sorted(new)                           # two kernels, bf16 and fp32
    for name, r in sorted(new.items()):
        assert r == {"scratch": 0, "sgpr_spill": 0, "vgpr_spill": 0}, f"{name}: {r}"

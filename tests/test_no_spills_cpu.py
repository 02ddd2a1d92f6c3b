"""Build hygiene (CPU): the hot kernels must not spill.  `multimeditron_amd/csrc/build.py` keeps hipcc's per-kernel resource
remarks beside every object (`csrc/build/*.o.resources.txt`); a kernel on the step's critical path that starts to use scratch
loses far more than the change that caused it gains (round 2: an extra epilogue path put 528 bytes/lane of scratch into the
256x256 GEMM and cost 10 % of the step).  Skipped when the library has not been built in this tree."""
import os
import re

import pytest

BUILD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multimeditron_amd", "csrc", "build")
HOT = {
    "mm_gemm.o.resources.txt": ["gemm_bf16_dma_kernel", "gemm_bf16_kernel", "gemm_skinny_kernel"],
    "mm_attn.o.resources.txt": ["attn_fwd128q_kernel", "attn_fwd128p_kernel", "attn_bwd_dq128p_kernel", "attn_bwd_dkv128_pairp_kernel",
                                "attn_decode_partial_kernel", "attn_decode_partial128_mfma_kernel",
                                # every decode step of generate's samples, beams and prompt-lookup modes; the beam kernel sits at the 256
                                # VGPRs of its launch bounds
                                "attn_decode_shared128_kernel", "attn_decode_beam128_kernel", "attn_decode_verify128_kernel"],
    "mm_optim.o.resources.txt": ["adamw_kernel", "sumsq_kernel"],
}


def _kernels(path):
    out, name = [], None
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and name:
            out.append((name, int(m.group(1))))
    return out


@pytest.mark.parametrize("fname", sorted(HOT))
def test_hot_kernels_use_no_scratch(fname):
    path = os.path.join(BUILD, fname)
    if not os.path.exists(path):
        pytest.skip("library not built in this tree (python multimeditron_amd/csrc/build.py)")
    ks = _kernels(path)
    assert ks, path
    seen = set()
    for name, scratch in ks:
        for hot in HOT[fname]:
            if hot in name:
                seen.add(hot)
                assert scratch == 0, f"{name}: {scratch} bytes/lane of scratch"
    assert seen == set(HOT[fname]), sorted(set(HOT[fname]) - seen)


def test_plain_gemm_instantiations_spill_few_sgprs():
    """The instantiation every decoder GEMM runs (epilogue kind 0) must stay (nearly) free of scalar spills: with the GELU kinds
    compiled into it the 256x256 kernel spilt 13-14 SGPRs (v_writelane / v_readlane traffic) and ran 2.5 % slower, with nothing
    else to show for it.  Round 3's pipelined epilogue (two more buffer descriptors) costs it 2-4 spilt SGPRs; in the ISA they are
    written once in the kernel prologue and read back in the per-tile set-up and in front of the half-tile round, never inside
    the K loop (checked with `hipcc --cuda-device-only -S`), and the kernel measured faster, not slower (profiles/r03_*).  The
    rarely used instantiations (activation, SwiGLU) may spill more."""
    path = os.path.join(BUILD, "mm_gemm.o.resources.txt")
    if not os.path.exists(path):
        pytest.skip("library not built in this tree (python multimeditron_amd/csrc/build.py)")
    name, n = None, 0
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"SGPRs Spill: (\d+)", ln)
        if m and name and "gemm_bf16_dma_kernel" in name and name.endswith("ELi0EEEvNS_8GemmArgsE"):
            # round 4: GemmArgs grew by the 4-wave kernel's switches; the 8-wave 256x256 NT instantiation went from 4 to 5 spilt SGPRs
            # (still outside its K loop) -- and left the step's path: 256x256 tiles run on gemm_bf16_w4_kernel (zero scratch, below)
            assert int(m.group(1)) <= 6, f"{name}: {m.group(1)} SGPRs spilt"
            n += 1
    assert n >= 15, n


def test_w4_gemm_scratch_stays_outside_the_k_loop():
    """gemm_bf16_w4_kernel (round 4): the K loop of a tile is ONE asm statement with literal registers, so nothing the compiler spills
    can be touched inside it; what it does spill are a few values that live across that statement (only v0-v91 exist there).  Round 4
    measured what such reloads cost when they sat in the epilogue (every scratch reload's s_waitcnt vmcnt(0) waited out the stores
    before it: 21 000 cycles per tile): the bound keeps the count where the measured build has it."""
    path = os.path.join(BUILD, "mm_gemm.o.resources.txt")
    if not os.path.exists(path):
        pytest.skip("library not built in this tree (python multimeditron_amd/csrc/build.py)")
    n = 0
    for name, scratch in _kernels(path):
        if "gemm_bf16_w4_kernel" in name:
            assert scratch <= 64, f"{name}: {scratch} bytes/lane of scratch"
            n += 1
    assert n >= 6, n


def test_w4_generated_loop_is_current():
    """mm_gemm_w4.inc is generated: the committed file must be what gen_gemm_w4.py writes."""
    import subprocess, sys, tempfile, shutil
    csrc = os.path.join(os.path.dirname(BUILD))
    inc = os.path.join(csrc, "mm_gemm_w4.inc")
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(os.path.join(csrc, "gen_gemm_w4.py"), d)
        subprocess.run([sys.executable, os.path.join(d, "gen_gemm_w4.py")], check=True, stdout=subprocess.DEVNULL)
        assert open(os.path.join(d, "mm_gemm_w4.inc")).read() == open(inc).read()

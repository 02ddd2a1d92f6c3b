"""Build hygiene (CPU): the xIELU kernels (csrc/mm_xielu.hip) are HBM-bound streaming kernels and must use no scratch.  Read from
hipcc's per-kernel resource remarks that `multimeditron_amd/csrc/build.py` keeps beside the object, as tests/test_no_spills_cpu.py
does.  Skipped when the library has not been built in this tree."""
import os

import pytest

from tests.test_no_spills_cpu import BUILD, _kernels

KERNELS = ["xielu_fwd_kernel", "xielu_bwd_kernel", "xielu_reduce_kernel"]


def test_xielu_kernels_use_no_scratch():
    path = os.path.join(BUILD, "mm_xielu.o.resources.txt")
    if not os.path.exists(path):
        pytest.skip("library not built in this tree (python multimeditron_amd/csrc/build.py)")
    ks = _kernels(path)
    assert len(ks) == 8, ks          # forward x 2 dtypes, backward x 2 dtypes x (with / without the sums), the finishing sum x 2
    for name, scratch in ks:
        assert any(k in name for k in KERNELS), name
        assert scratch == 0, f"{name}: {scratch} bytes/lane of scratch"
    assert {k for k in KERNELS for name, _ in ks if k in name} == set(KERNELS)

"""Register / scratch audit of the 4-wave 256x256 GEMM (gemm_q.hip igemm_q_kernel) in the built gfx950 code objects
(CPU; reads build/*.o, no GPU).

Its ring of LDS stages is paced by a hand-counted `s_waitcnt vmcnt(16)`: a scratch spill is a vector-memory
instruction the count does not know about, and the kernel holds 256 accumulator AGPRs beside at most 256 VGPRs, so every
instance must have no private segment and no VGPR spills.
"""
import re
from pathlib import Path

import pytest

from tests.test_kernel_resources_cpu import ROOT, TOOLS, _kernels


@pytest.fixture(scope="module")
def q_kernels():
    if not all(t and Path(t).exists() for t in TOOLS):
        pytest.skip("objcopy / clang-offload-bundler / llvm-readelf / c++filt not available")
    if not list((ROOT / "build").glob("*.o")):
        pytest.skip("build/*.o absent: run make (or __graft_entry__.build()) first")
    k = {n: v for n, v in _kernels().items() if re.search(r"^_Z14igemm_q_kernelI", n[0])}
    assert k, "no igemm_q_kernel instance found in build/*.o"
    return k


def test_q_kernels_have_no_private_segment(q_kernels):
    bad = [f"{m[:110]}: private {priv} B" for (m, _), (priv, _, _) in q_kernels.items() if priv]
    assert not bad, "\n".join(bad)


def test_q_kernels_have_no_vgpr_spills(q_kernels):
    bad = [f"{m[:110]}: {vgpr} VGPR spills" for (m, _), (_, _, vgpr) in q_kernels.items() if vgpr]
    assert not bad, "\n".join(bad)

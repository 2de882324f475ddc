"""Register / scratch audit of the attention kernels (csrc/attention.hip) in the built gfx950 code object (CPU; reads
build/attention.o, no GPU).

The forward's bf16 instances are launch-bounded to 168 VGPRs (three waves per SIMD) and the register-staged one sits
exactly on that cap; the LDS-DMA kernels pace their prefetch with vmcnt(0) drains, which a scratch spill would join.
So no attention kernel may have a private segment or VGPR spills.  The set of kernels is pinned as well: the 16x16
backward pair is the f32 strict-parity path only (bf16 runs the 32x32x16 pair), so it has exactly one instance each.
"""
import re
from pathlib import Path

import pytest

from tests.test_kernel_resources_cpu import ROOT, TOOLS, _kernels

# demangled-name patterns; mangled-name prefixes where __bf16 is in the signature (c++filt cannot demangle it)
EXPECTED = [
    r"^_Z15attn_fwd_kernelIDF16bLb1EE",
    r"^_Z15attn_fwd_kernelIDF16bLb0EE",
    r"^void attn_fwd_kernel<float, false>\(",
    r"^_Z17attn_delta_kernelIDF16bE",
    r"^void attn_delta_kernel<float>\(",
    r"^attn_bwd_dkdv_kernel\(float const\*",
    r"^attn_bwd_dq_kernel\(float const\*",
    r"^_Z22attn_bwd_dkdv32_kernelILi4EE",
    r"^_Z20attn_bwd_dq32_kernelILi4EE",
]


@pytest.fixture(scope="module")
def attn_kernels():
    if not all(t and Path(t).exists() for t in TOOLS):
        pytest.skip("objcopy / clang-offload-bundler / llvm-readelf / c++filt not available")
    if not list((ROOT / "build").glob("*.o")):
        pytest.skip("build/*.o absent: run make (or __graft_entry__.build()) first")
    k = {n: v for n, v in _kernels().items() if re.search(r"attn_", n[0])}     # (the bias-sum fold is reduce.hpp's, shared with vit_ops.hip)
    assert k, "no attention kernel found in build/*.o"
    return k


def test_attn_kernels_have_no_private_segment(attn_kernels):
    bad = [f"{d[:110]}: private {priv} B" for (_, d), (priv, _, _) in attn_kernels.items() if priv]
    assert not bad, "\n".join(bad)


def test_attn_kernels_have_no_vgpr_spills(attn_kernels):
    bad = [f"{d[:110]}: {vgpr} VGPR spills" for (_, d), (_, _, vgpr) in attn_kernels.items() if vgpr]
    assert not bad, "\n".join(bad)


def test_attn_kernel_set_is_exact(attn_kernels):
    """each expected kernel once, nothing else -- in particular no bf16 instance of the 16x16 backward pair"""
    hits = {p: [d for m, d in attn_kernels if re.search(p, m) or re.search(p, d)] for p in EXPECTED}
    assert all(len(v) == 1 for v in hits.values()), {p: v for p, v in hits.items() if len(v) != 1}
    extra = [d for m, d in attn_kernels if not any(re.search(p, m) or re.search(p, d) for p in EXPECTED)]
    assert not extra, extra

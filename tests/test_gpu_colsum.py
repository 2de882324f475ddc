"""GPU: s3od_colsum (bias gradients: out += column sums of a [M, N] matrix) -- the two-pass form through the
caller-owned partial-sum workspace against fp32 torch, bit-identical run to run (fixed summation order), and the
per-block fp32-atomic form (no workspace) within fp32 summation-order tolerance; ragged M, N > 2048 (two column
block groups), N = 8 (a single column group: all 256 threads of a block are row phases of it, with too few rows
for the phases at M = 1000 and one 4-deep batch of 256-row strides plus a tail at M = 600000)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
BF16 = 1


@pytest.mark.parametrize("M,N", [(16 * 64 * 64, 256), (1000, 256), (65616, 768), (4099, 4096), (37, 64), (1000, 8),
                                 (600000, 8)])
def test_colsum_two_pass(M, N):
    from s3od_amd._lib import lib, stream
    g = torch.Generator(device="cuda").manual_seed(M + N)
    a = torch.randn(M, N, device="cuda", generator=g).bfloat16()
    base = torch.randn(N, device="cuda", generator=g)
    ref = base + a.float().sum(0)
    nb = ctypes.c_long(0)
    lib()("s3od_colsum_ws", M, N, ctypes.addressof(nb))
    assert nb.value > 0
    ws = torch.full((nb.value // 4,), float("nan"), device="cuda")          # dead contents: poisoned
    outs = []
    for _ in range(2):
        out = base.clone()
        lib()("s3od_colsum", BF16, a, N, M, N, out, ws, nb.value, stream())
        outs.append(out)
    atom = base.clone()
    lib()("s3od_colsum", BF16, a, N, M, N, atom, None, 0, stream())
    torch.cuda.synchronize()
    scale = float(a.float().abs().sum(0).max())
    assert torch.equal(outs[0], outs[1])
    assert float((outs[0] - ref).abs().max()) <= 1e-5 * scale
    assert float((atom - ref).abs().max()) <= 1e-5 * scale


@pytest.mark.parametrize("M,N", [(37, 64), (1000, 256)])
def test_colsum_one_pass(M, N):
    """The form without a workspace (every block adds its sums by fp32 atomics) against float64 column sums computed
    on the CPU; the test above holds it only to fp32 torch.  Same bound as the two-pass form: 1e-5 of the largest
    column's sum of magnitudes.  (37, 64): fewer rows than one block's row phases; (1000, 256): several row blocks."""
    from s3od_amd._lib import lib, stream
    g = torch.Generator(device="cuda").manual_seed(M + N)
    a = torch.randn(M, N, device="cuda", generator=g).bfloat16()
    base = torch.randn(N, device="cuda", generator=g)
    out = base.clone()
    lib()("s3od_colsum", BF16, a, N, M, N, out, None, 0, stream())
    torch.cuda.synchronize()
    a64 = a.double().cpu()
    ref = base.double().cpu() + a64.sum(0)
    scale = float(a64.abs().sum(0).max())
    err = float((out.double().cpu() - ref).abs().max())
    print(f"colsum one-pass M {M} N {N}: max err {err:.3e}, bound {1e-5 * scale:.3e}")
    assert err <= 1e-5 * scale

"""GPU parity of the 4-wave 256x256 GEMM's ring of k-step stages (gemm_q.hip igemm_q_kernel, S3OD_GEMM_CFG=6) through
the C ABI, at k-step counts around the ring depth (4) and its wrap.

A 64-deep K tile is two 32-deep k-steps, so K = 32 .. 544 gives 2, 2, 4, 4, 6, 10 and 18 k-steps (the ring's prologue
alone, one wrap, several) and K = 40 / 72 a last k-step that K cuts.  Every case is compared
  * against fp32 torch on the same bf16 operands, at the tolerances of tests/test_gpu_gemm_pp.py (rel-L2 <= 1e-5 for
    fp32 outputs, <= 4e-3 for bf16 outputs);
  * BIT FOR BIT against the same call on the ping-pong kernel (S3OD_GEMM_CFG=5): the MFMA chain per output element is
    the same (k order, operand order), only the staging differs;
  * BIT FOR BIT against itself over 20 calls on the same operands (a screen for the counted waits and the barrier).
"""
import pytest
import torch

from tests.test_gpu_gemm_pp import BF16, _lib, r, rel_l2

pytestmark = pytest.mark.gpu

KS = [32, 64, 96, 128, 160, 288, 544, 40, 72]
REPEAT = 20


def _run(monkeypatch, call, fresh):
    """call(*fresh()) under config 6 (REPEAT times) and config 5 (once); returns (q outputs, pp outputs)."""
    monkeypatch.setenv("S3OD_DGRAD_BLASLT", "0")        # the plain bf16 data gradients stay on our kernels
    monkeypatch.setenv("S3OD_GEMM_CFG", "6")
    first = None
    for _ in range(REPEAT):
        outs = fresh()
        call(*outs)
        torch.cuda.synchronize()
        if first is None:
            first = outs
        else:
            for a, b in zip(outs, first):
                assert torch.equal(a, b), "config 6 differs between two calls on the same operands"
    monkeypatch.setenv("S3OD_GEMM_CFG", "5")
    pp = fresh()
    call(*pp)
    torch.cuda.synchronize()
    for a, b in zip(first, pp):
        assert torch.equal(a, b), "config 6 differs from the ping-pong kernel"
    return first


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("form", ["plain", "residual_pre"])
def test_q_ring_linear_fwd(monkeypatch, K, form):
    L, s = _lib()
    for M in (256, 512):
        for N in (256, 512, 136):
            torch.manual_seed(M + N + K)
            x, w, b = r(M, K), r(N, K, scale=K ** -0.5), r(N, dt=torch.float32)
            ref_pre = x.float() @ w.float().t() + b
            if form == "plain":
                def call(out):
                    L("s3od_linear_fwd", BF16, M, N, K, x, K, w, b, None, None, 0, None, N, None, 0, 0, out, N, 0, None, N,
                      0, 0, 0, s)
                (out,) = _run(monkeypatch, call, lambda: (torch.zeros(M, N, device="cuda", dtype=torch.bfloat16),))
                assert rel_l2(out.float(), ref_pre) < 4e-3, (M, N, K)
            else:
                ls, res = r(N, dt=torch.float32), r(M, N, dt=torch.float32)

                def call(out, pre):
                    L("s3od_linear_fwd", BF16, M, N, K, x, K, w, b, ls, None, 0, res, N, None, 0, 1, out, N, 1, pre, N,
                      0, 0, 0, s)
                out, pre = _run(monkeypatch, call, lambda: (torch.zeros(M, N, device="cuda"),
                                                            torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)))
                assert rel_l2(out, ref_pre * ls + res) < 1e-5, (M, N, K)
                assert rel_l2(pre.float(), ref_pre) < 4e-3, (M, N, K)


@pytest.mark.parametrize("K", KS)
def test_q_ring_linear_dgrad(monkeypatch, K):
    """B operand N-contiguous (w [K][N]): bf16 output, and the fp32 in-place accumulate."""
    L, s = _lib()
    N = 256
    for M in (256, 512):
        torch.manual_seed(M + K)
        dy, w = r(M, K), r(K, N, scale=K ** -0.5)
        ref = dy.float() @ w.float()

        def call(dx):
            L("s3od_linear_dgrad", BF16, M, N, K, dy, K, w, 0, None, N, dx, N, 0, 0, 0, 0, None, s)
        (dx,) = _run(monkeypatch, call, lambda: (torch.zeros(M, N, device="cuda", dtype=torch.bfloat16),))
        assert rel_l2(dx.float(), ref) < 4e-3, (M, K)
        dx0 = r(M, N, dt=torch.float32)

        def call_acc(acc):
            L("s3od_linear_dgrad", BF16, M, N, K, dy, K, w, 0, acc, N, acc, N, 1, 0, 0, 0, None, s)
        (acc,) = _run(monkeypatch, call_acc, lambda: (dx0.clone(),))
        assert rel_l2(acc, dx0 + ref) < 1e-5, (M, K)


@pytest.mark.parametrize("share", [1, 2, 3, 4, 5, 9])
def test_q_ring_linear_wgrad_split(monkeypatch, share):
    """Forced split 2 over rows = 64 * ceil(share / 2) + 32 * share: split-K ranges are whole 64-row K tiles, so the
    first split gets ceil(share / 2) tiles and the last one `share` 32-row k-steps of data (an odd share ends in a
    k-step of zeros).  256 x 256 is one workgroup per split; both configs write their partials to slabs."""
    import ctypes
    L, s = _lib()
    Nout = Kin = 256
    rows = 64 * ((share + 1) // 2) + 32 * share
    torch.manual_seed(rows)
    dy, x = r(rows, Nout), r(rows, Kin)
    dw0 = r(Nout, Kin, dt=torch.float32)
    monkeypatch.setenv("S3OD_GEMM_CFG", "6")
    n = ctypes.c_long(0)
    L("s3od_linear_wgrad_ws", BF16, Nout, Kin, rows, 2, ctypes.addressof(n))
    assert n.value == 2 * Nout * Kin * 4
    ws = torch.full((n.value // 4,), float("nan"), device="cuda")

    def call(dw):
        L("s3od_linear_wgrad", BF16, Nout, Kin, rows, dy, Nout, x, Kin, dw, 2, ws, n.value, s)
    (dw,) = _run(monkeypatch, call, lambda: (dw0.clone(),))
    assert rel_l2(dw, dw0 + dy.float().t() @ x.float()) < 1e-5


def test_q_ring_production_rows(monkeypatch):
    """M = 16384 + 80, N = K = 768 (o_proj form): the 80 tail rows (skinny kernel) and the last full panel's rows
    (4-wave kernel) each equal the ping-pong result bit for bit."""
    torch.manual_seed(16464)
    L, s = _lib()
    M, N, K = 16384 + 80, 768, 768
    x, w = r(M, K), r(N, K, scale=K ** -0.5)
    b, ls, res = r(N, dt=torch.float32), r(N, dt=torch.float32), r(M, N, dt=torch.float32)
    got = {}
    for cfg in ("6", "5"):
        monkeypatch.setenv("S3OD_GEMM_CFG", cfg)
        out = torch.zeros(M, N, device="cuda")
        pre = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16)
        L("s3od_linear_fwd", BF16, M, N, K, x, K, w, b, ls, None, 0, res, N, None, 0, 1, out, N, 1, pre, N, 0, 0, 0, s)
        torch.cuda.synchronize()
        got[cfg] = (out, pre)
    for a, c in zip(got["6"], got["5"]):
        assert torch.equal(a[-80:], c[-80:])
        assert torch.equal(a[-80 - 256:-80], c[-80 - 256:-80])
        assert torch.equal(a, c)
    ref_pre = x.float() @ w.float().t() + b
    assert rel_l2(got["6"][0], ref_pre * ls + res) < 1e-5
    assert rel_l2(got["6"][1].float(), ref_pre) < 4e-3

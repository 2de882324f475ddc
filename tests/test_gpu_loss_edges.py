"""GPU: the fused mask loss (csrc/loss.hip: s3od_mask_loss_fwd / s3od_mask_loss_bwd) against the oracle
restatement (oracle/s3od_oracle.py: multi_mask_loss / single_mask_loss) evaluated in float64, at the edges
the goldens (B <= 2, M = 3, 64x64) never reach: more than 64 (b, m) entries, more than one loss_sums_kernel
block per map with a ragged tail, one-pixel-thin maps, an upstream gradient scale, soft targets, exact IoU
ties and saturated logits.

Tolerances are the project's (tests/test_gpu_loss.py): loss and parts <= 1e-4 relative, logit and pred_iou
gradients <= 2e-4 max-relative.  The oracle's own f32 and f64 evaluations agree to <= 1.4e-6 on the
gradients and <= 5e-8 on the loss at these shapes, so the float64 reference does not eat into them.
Each test prints its worst errors (pytest -s).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL_PART, TOL_GRAD = 1e-4, 2e-4
CFGS = ["focal_iou", "bce_iou_ssim"]
NAN = float("nan")


def _cfgs(name):
    from oracle import s3od_oracle as O
    from s3od_amd.loss import FOCAL_IOU, BCE_IOU_SSIM
    return (FOCAL_IOU, O.FOCAL_IOU) if name == "focal_iou" else (BCE_IOU_SSIM, O.BCE_IOU_SSIM)


def rel(a, b):
    """max-relative error of a against the float64 reference b"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-12))


def ellipses(B, H, W):
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    return torch.stack([(((yy - H / 2) / (H / 3)) ** 2 + ((xx - W / 2 - (b % 7 - 3)) / (W / 4)) ** 2 <= 1).float()
                        for b in range(B)])


def gpu_loss(cfgname, logits, pred_iou, masks, epoch=1, scale=None):
    """the product path: LossModule -> _MaskLossFn -> s3od_mask_loss_fwd/bwd"""
    from s3od_amd.loss import LossModule
    lm = LossModule(_cfgs(cfgname)[0], full_mask_lambda=0.1, decay_rate=0.2)
    lg = logits.cuda().requires_grad_(True)
    pi = pred_iou.cuda().requires_grad_(True)
    loss, parts = lm({"pred_masks": lg, "pred_iou": pi}, {"masks": masks.cuda()}, epoch)
    (loss if scale is None else loss * scale).backward()
    torch.cuda.synchronize()
    return loss, parts, lg.grad, pi.grad, lm


def direct_loss(cfgname, logits, pred_iou, masks, epoch=1):
    """the two entry points called directly, every output buffer NaN on entry"""
    from s3od_amd._lib import lib, stream
    from s3od_amd.loss import LossModule
    import math
    lm = LossModule(_cfgs(cfgname)[0], full_mask_lambda=0.1, decay_rate=0.2)
    w, lam = lm.w, 0.1 * math.exp(-0.2 * epoch)
    B, M, H, W = logits.shape
    HW, dev = H * W, "cuda"
    lg, pi, tg = logits.cuda().contiguous(), pred_iou.cuda().contiguous(), masks.cuda().contiguous()
    sums = torch.full((B * M * 8,), NAN, dtype=torch.float64, device=dev)      # cleared by the entry itself
    coef, iou_ws, diu = (torch.full((B * M * k,), NAN, device=dev) for k in (4, 2, 1))
    out = torch.full((16 + B * M + B,), NAN, device=dev)
    L, st = lib(), stream()
    L("s3od_mask_loss_fwd", lg, tg, pi, B, M, HW, W, w["focal"], w["iou"], w["bce"], w["ssim"], w["mse"], lam, 0.25, 2.0,
      sums, coef, iou_ws, diu, out, st)
    dl = torch.full_like(lg, NAN)
    di = torch.full((B, M), NAN, device=dev)
    L("s3od_mask_loss_bwd", lg, tg, coef, iou_ws, diu, None, dl, di, B, M, HW, W, int(w["ssim"] != 0.0), 0.25, 2.0, st)
    torch.cuda.synchronize()
    return out, dl, di


def oracle_loss(cfgname, logits, pred_iou, masks, epoch=1, dtype=torch.float64, scale=None):
    from oracle import s3od_oracle as O
    lg = logits.detach().to(dtype, copy=True).requires_grad_(True)
    pi = pred_iou.detach().to(dtype, copy=True).requires_grad_(True)
    rl, rparts, best, ious = O.multi_mask_loss({"pred_masks": lg, "pred_iou": pi}, masks.to(dtype), epoch, _cfgs(cfgname)[1])
    (rl if scale is None else rl * scale).backward()
    return rl.detach(), rparts, lg.grad, pi.grad, best, ious


def check(tag, got, ref, split=None):
    """got = (loss, parts, dlogits, dpred_iou) from the GPU, ref likewise from the oracle; split: also assert
    the pred_iou gradient over the flat entries [:split] and [split:] separately.  Prints, then asserts."""
    loss, parts, dl, di = got
    rl, rparts, rdl, rdi = ref
    e_loss = abs(float(loss) - float(rl)) / abs(float(rl))
    e_part = {n: abs(float(parts[n]) - float(rparts[n])) / max(abs(float(rparts[n])), 1e-6) for n in rparts}
    assert set(parts) == set(rparts)
    e_dl = rel(dl, rdl)
    di, rdi = di.flatten(), rdi.flatten()
    cuts = [(0, di.numel())] if split is None else [(0, split), (split, di.numel())]
    e_di = [rel(di[a:b], rdi[a:b]) for a, b in cuts]
    print(f"\n[{tag}] loss {e_loss:.2e}  worst part {max(e_part.values()):.2e}  dlogits {e_dl:.2e}  "
          f"dpred_iou {' / '.join(f'{e:.2e}' for e in e_di)}")
    assert torch.isfinite(dl).all() and torch.isfinite(di).all() and torch.isfinite(loss).all()
    assert e_loss <= TOL_PART, e_loss
    for n, e in e_part.items():
        assert e <= TOL_PART, (n, e)
    assert e_dl <= TOL_GRAD, e_dl
    for (a, b), e in zip(cuts, e_di):
        assert e <= TOL_GRAD, (f"pred_iou gradient entries [{a}:{b}]", e)


@pytest.mark.parametrize("cfgname", CFGS)
@pytest.mark.parametrize("B,M", [(21, 3), (22, 3), (32, 3)])
def test_batch_past_one_block_of_d_iou(cfgname, B, M):
    """B*M = 63 / 66 / 96 entries of the pred_iou gradient: the entries past the 64th were never written when
    loss_iou_grad_kernel was a single 64-thread block (that kernel gave 5.4e4 at 22x3 and 3.8e23 at 32x3 on the
    [64:] slice, profiles/loss_head_glue_gpu_tests.log).  The true gradient there is small but nonzero, so the
    two halves are asserted separately, through LossModule and through the entry points on NaN-filled buffers."""
    torch.manual_seed(B)
    logits, pred_iou, masks = torch.randn(B, M, 16, 16) * 2, torch.randn(B, M), ellipses(B, 16, 16)
    rl, rparts, rdl, rdi, best, ious = oracle_loss(cfgname, logits, pred_iou, masks)
    split = 64 if B * M > 64 else None
    assert split is None or float(rdi.flatten()[64:].abs().min()) > 0
    loss, parts, dl, di, _ = gpu_loss(cfgname, logits, pred_iou, masks)
    check(f"batch {cfgname} {B}x{M} module", (loss, parts, dl, di), (rl, rparts, rdl, rdi), split)
    out, dl2, di2 = direct_loss(cfgname, logits, pred_iou, masks)
    assert torch.isfinite(out[:12]).all() and torch.isfinite(out[16:]).all(), "packed result: [12:16] is padding, the rest is written"
    assert rel(out[16:16 + B * M], ious.flatten()) <= TOL_PART and out[16 + B * M:].long().tolist() == best.tolist()
    check(f"batch {cfgname} {B}x{M} direct", (out[0], parts, dl2, di2), (rl, rparts, rdl, rdi), split)


def test_single_mask_past_64_maps():
    """(B, M) = (70, 1): LossModule's single-mask path (lambda = 0, no aux MSE, pred_iou without gradient)."""
    from oracle import s3od_oracle as O
    torch.manual_seed(70)
    B, H, W = 70, 8, 8
    logits, pred_iou = torch.randn(B, 1, H, W) * 2, torch.randn(B, 1)
    masks = (torch.rand(B, H, W) > 0.5).float()
    loss, parts, dl, di, lm = gpu_loss("focal_iou", logits, pred_iou, masks)
    assert di is None and lm.last_best is None
    lg = logits.double().requires_grad_(True)
    rl, rparts = O.single_mask_loss({"pred_masks": lg, "pred_iou": pred_iou.double()}, masks.double(), O.FOCAL_IOU)
    rl.backward()
    e_loss = abs(float(loss) - float(rl)) / abs(float(rl))
    e_part = {n: abs(float(parts[n]) - float(rparts[n])) / max(abs(float(rparts[n])), 1e-6) for n in rparts}
    e_dl = rel(dl, lg.grad)
    print(f"\n[single 70x1] loss {e_loss:.2e}  worst part {max(e_part.values()):.2e}  dlogits {e_dl:.2e}")
    assert set(parts) == set(rparts) and torch.isfinite(dl).all()
    assert e_loss <= TOL_PART and max(e_part.values()) <= TOL_PART and e_dl <= TOL_GRAD
    ious = lm.last_gt_ious
    assert ious.shape == (B, 1) and torch.isfinite(ious).all()


@pytest.mark.parametrize("cfgname", CFGS)
@pytest.mark.parametrize("shape", [(1, 3, 130, 131), (2, 3, 1, 300), (1, 3, 300, 1)])
def test_many_sums_blocks_and_thin_maps(cfgname, shape):
    """HW = 17030: two loss_sums_kernel blocks per map, the second with 646 pixels; SSIM grid 5x5 tiles with a
    2- and 3-wide remainder.  1x300 and 300x1: SSIM tiles that are almost entirely zero padding."""
    torch.manual_seed(sum(shape))
    B, M, H, W = shape
    logits, pred_iou = torch.randn(B, M, H, W) * 2, torch.randn(B, M)
    masks = ellipses(B, H, W) if min(H, W) > 1 else (torch.rand(B, H, W) > 0.5).float()
    assert 0 < float(masks.mean()) < 1
    loss, parts, dl, di, _ = gpu_loss(cfgname, logits, pred_iou, masks)
    check(f"blocks {cfgname} {shape}", (loss, parts, dl, di), oracle_loss(cfgname, logits, pred_iou, masks)[:4])


@pytest.mark.parametrize("cfgname", CFGS)
def test_upstream_gradient_scale(cfgname):
    """(loss * 3.5).backward(): the gscale pointer of loss_grad_kernel, ssim_grad_kernel and loss_iou_grad_kernel."""
    torch.manual_seed(5)
    B, M, H, W = 2, 3, 33, 97
    logits, pred_iou, masks = torch.randn(B, M, H, W) * 2, torch.randn(B, M), ellipses(B, H, W)
    loss, parts, dl, di, _ = gpu_loss(cfgname, logits, pred_iou, masks, scale=3.5)
    ref = oracle_loss(cfgname, logits, pred_iou, masks, scale=3.5)
    unscaled = oracle_loss(cfgname, logits, pred_iou, masks)
    assert torch.allclose(ref[2], 3.5 * unscaled[2], rtol=1e-12, atol=0)
    check(f"gscale {cfgname}", (loss, parts, dl, di), ref[:4])


@pytest.mark.parametrize("cfgname", CFGS)
def test_soft_targets(cfgname):
    """targets uniform in [0, 1]: t*t != t in the IoU selection's union."""
    torch.manual_seed(6)
    B, M, H, W = 2, 3, 40, 40
    logits, pred_iou, masks = torch.randn(B, M, H, W) * 2, torch.randn(B, M), torch.rand(B, H, W)
    loss, parts, dl, di, _ = gpu_loss(cfgname, logits, pred_iou, masks)
    check(f"soft {cfgname}", (loss, parts, dl, di), oracle_loss(cfgname, logits, pred_iou, masks)[:4])


@pytest.mark.parametrize("cfgname", CFGS)
def test_exact_iou_ties(cfgname):
    """identical planes give bit-identical IoUs; the first maximum wins, as torch.argmax does."""
    torch.manual_seed(8)
    B, M, H, W = 3, 3, 32, 32
    masks = ellipses(B, H, W)
    good = 3.0 * (2 * masks - 1) + torch.randn(B, H, W)       # close to the target
    poor = torch.randn(B, H, W) * 2
    logits = torch.empty(B, M, H, W)
    logits[0, 0] = logits[0, 1] = good[0]; logits[0, 2] = poor[0]
    logits[1, 0] = poor[1]; logits[1, 1] = logits[1, 2] = good[1]
    logits[2, :] = good[2]
    pred_iou = torch.randn(B, M)
    loss, parts, dl, di, lm = gpu_loss(cfgname, logits, pred_iou, masks)
    rl, rparts, rdl, rdi, best, ious = oracle_loss(cfgname, logits, pred_iou, masks)
    assert ious[0, 0] == ious[0, 1] > ious[0, 2] and ious[1, 1] == ious[1, 2] > ious[1, 0] and ious[2, 0] == ious[2, 1] == ious[2, 2]
    assert best.tolist() == ious.argmax(1).tolist() == [0, 1, 0]
    got_best = lm.last_best.cpu().long().tolist()
    print(f"\n[ties {cfgname}] best {got_best} (oracle {best.tolist()})")
    assert got_best == best.tolist()
    check(f"ties {cfgname}", (loss, parts, dl, di), (rl, rparts, rdl, rdi))


@pytest.mark.parametrize("cfgname", CFGS)
def test_saturated_logits(cfgname):
    """logits from {0, +-0.5, +-8, +-12, +-25, +-40} against a random binary target, so about half of the
    saturated pixels are confidently wrong: the BCE log clamp at -100, p(1-p) underflowing to 0 and the
    max(p(1-p), 1e-12) of the BCE gradient.  FOCAL_IOU against the float64 oracle.  BCE_IOU_SSIM against the
    oracle in float32: torch.nn.BCELoss clamps the log of the *f32* sigmoid, which is exactly 1 from |x| ~ 17
    on, and the f64 oracle (no clamp reached until |x| ~ 37) differs from it by 30 % in the loss here.  The
    values keep clear of |x| in 16.6 .. 17.4, where an f32 sigmoid may or may not round to exactly 1."""
    torch.manual_seed(9)
    B, M, H, W = 2, 3, 32, 32
    vals = torch.tensor([0.0, 0.5, -0.5, 8, -8, 12, -12, 25, -25, 40, -40])
    logits = vals[torch.randint(0, len(vals), (B, M, H, W))]
    masks = (torch.rand(B, H, W) > 0.5).float()
    pred_iou = torch.randn(B, M)
    wrong = ((logits.abs() >= 25) & ((logits > 0) != (masks[:, None] > 0.5))).float().mean()
    assert 0.1 < float(wrong) < 0.3
    loss, parts, dl, di, _ = gpu_loss(cfgname, logits, pred_iou, masks)
    dtype = torch.float64 if cfgname == "focal_iou" else torch.float32
    ref = oracle_loss(cfgname, logits, pred_iou, masks, dtype=dtype)
    assert all(torch.isfinite(torch.as_tensor(float(v))) for v in parts.values())
    check(f"saturated {cfgname} vs {str(dtype)[6:]} oracle", (loss, parts, dl, di), ref[:4])

"""Shared by test_matte_ref_cpu.py and test_gpu_matte.py: the float64 numpy reference of s3od_matte_refine and
s3od_matte_foreground (csrc/matte.hip) and the images the kernels are tested on.

``box_mean(v, r)`` is the mean over the window [y-r, y+r] x [x-r, x+r] clipped to the image, divided by the number of
pixels inside it (He's boxfilter / N), by direct summation: one slice sum per row and per column, no running total.

``refine`` is the colour guided filter (He, Sun, Tang 2013) with I = src / 255:
    mI = box(I), mp = box(p), mIp = box(I p), mII = box(I_i I_j)
    Sigma = mII - mI mI^T + eps Id,  cov = mIp - mI mp,  a = Sigma^-1 cov (np.linalg.solve),  b = mp - a . mI
    q = clip(box(a) . I + box(b), 0, 1)

``foreground`` is the blur-fusion estimate (Forte & Pitie 2021), one pass, alpha = alpha[..., None]:
    F^ = box(I alpha) / (box(alpha) + 1e-5),  B^ = box(I (1 - alpha)) / (box(1 - alpha) + 1e-5)
    F = clip(F^ + alpha (I - alpha F^ - (1 - alpha) B^), 0, 1),  bytes = trunc(F 255 + 0.5)

``make_case(H, W, seed)``: a two-colour disc image with N(0, 12) noise whose top quarter is the constant 128 (there
Sigma is eps Id), and a soft mask: the disc plus N(0, 0.15) noise, Gaussian-blurred at sigma 3 and clipped, with a band
forced to exactly 0 and a block forced to exactly 1 (windows of the foreground estimate with alpha = 0 and alpha = 1
throughout).
"""
import numpy as np


def box_mean(v: np.ndarray, r: int) -> np.ndarray:
    """Clipped-window mean of the leading two axes of a float64 array [H, W, ...]."""
    v = np.asarray(v, np.float64)
    H, W = v.shape[:2]
    rows = np.stack([v[max(y - r, 0):min(y + r, H - 1) + 1].sum(axis=0) for y in range(H)], axis=0)
    both = np.stack([rows[:, max(x - r, 0):min(x + r, W - 1) + 1].sum(axis=1) for x in range(W)], axis=1)
    ny = np.array([min(y + r, H - 1) - max(y - r, 0) + 1 for y in range(H)], np.float64)
    nx = np.array([min(x + r, W - 1) - max(x - r, 0) + 1 for x in range(W)], np.float64)
    n = ny[:, None] * nx[None, :]
    return both / n.reshape(n.shape + (1,) * (v.ndim - 2))


def refine(mask: np.ndarray, src: np.ndarray, r: int, eps: float) -> np.ndarray:
    """float64 [H, W]: the guided filter of ``mask`` (float) against ``src`` (uint8 [H, W, 3])."""
    I = src.astype(np.float64) / 255.0
    p = mask.astype(np.float64)
    mI, mp = box_mean(I, r), box_mean(p, r)
    mIp = box_mean(I * p[..., None], r)
    mII = box_mean(I[..., :, None] * I[..., None, :], r)                     # [H, W, 3, 3]
    sigma = mII - mI[..., :, None] * mI[..., None, :] + eps * np.eye(3)
    cov = mIp - mI * mp[..., None]
    a = np.linalg.solve(sigma, cov[..., None])[..., 0]                       # [H, W, 3]
    b = mp - (a * mI).sum(-1)
    return np.clip((box_mean(a, r) * I).sum(-1) + box_mean(b, r), 0.0, 1.0)


def foreground(alpha: np.ndarray, src: np.ndarray, r: int) -> np.ndarray:
    """float64 [H, W, 3] in [0, 1]: the estimated foreground colours."""
    I = src.astype(np.float64) / 255.0
    a = alpha.astype(np.float64)[..., None]
    fh = box_mean(I * a, r) / (box_mean(a, r) + 1e-5)
    bh = box_mean(I * (1.0 - a), r) / (box_mean(1.0 - a, r) + 1e-5)
    return np.clip(fh + a * (I - a * fh - (1.0 - a) * bh), 0.0, 1.0)


def to_bytes(f: np.ndarray) -> np.ndarray:
    """(F 255 + 0.5) truncated, the foreground entry's rounding."""
    return (f * 255.0 + 0.5).astype(np.uint8)


def alpha_bytes(q: np.ndarray) -> np.ndarray:
    """(q 255) truncated, the product's alpha byte (predictor.py:127)."""
    return (q * 255.0).astype(np.uint8)


def _gauss_blur(v: np.ndarray, sigma: float) -> np.ndarray:
    k = int(3 * sigma + 0.5)
    w = np.exp(-0.5 * (np.arange(-k, k + 1) / sigma) ** 2)
    w /= w.sum()
    for axis in (0, 1):
        pad = [(k, k) if a == axis else (0, 0) for a in range(2)]
        vp = np.pad(v, pad, mode="edge")
        v = sum(w[j] * np.take(vp, np.arange(j, j + v.shape[axis]), axis=axis) for j in range(2 * k + 1))
    return v


def make_case(H: int, W: int, seed: int):
    """-> (src uint8 [H, W, 3], mask float32 [H, W])."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    disc = ((yy - 0.55 * H) / (0.3 * H)) ** 2 + ((xx - 0.45 * W) / (0.3 * W)) ** 2 <= 1.0
    inside, outside = np.array([200.0, 90.0, 60.0]), np.array([40.0, 110.0, 170.0])
    img = np.where(disc[..., None], inside, outside) + rng.normal(0.0, 12.0, (H, W, 3))
    img[:max(H // 4, 1)] = 128.0
    src = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    m = np.clip(_gauss_blur(disc.astype(np.float64) + rng.normal(0.0, 0.15, (H, W)), 3.0), 0.0, 1.0)
    m[:, :max(W // 8, 1)] = 0.0                                             # a band of exactly 0
    m[H // 2:H // 2 + max(H // 5, 1), W // 3:W // 3 + max(W // 5, 1)] = 1.0  # a block of exactly 1
    return src, m.astype(np.float32)

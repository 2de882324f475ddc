"""Device-side compositing and mask statistics over finished masks (s3od_compose, s3od_mask_stats).

``compose`` writes one of the demo's output formats from a device mask and the device source image: RGBA, the
visualizer's blend over a colour or over a background image (src/s3od/visualizer.py:17-21, byte for byte numpy's
float32 ``(mask * image + (1 - mask) * background).astype(uint8)``), or the mask as an 8-bit image.
``mask_stats`` counts, for every pair of masks, the pixels where both / either exceed 0.5 (the demo's pairwise IoU,
demo/app.py:38-56) and the area and bounding box of the best mask above a threshold; only the 288-byte counter block
comes back to the host.  There is no host fallback.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from .image_ops import MODE_MASK_U8, MODE_RGB_OVER_IMAGE, MODE_RGBA, STATS_WORDS

MAX_STAT_MASKS = 8
_BPP = (4, 3, 3, 1)


@dataclass
class MaskStats:
    """Exact integer statistics of one image's masks.  ``pair_inter[i, j]`` / ``pair_union[i, j]`` (symmetric; the
    diagonal is the plane's own count) are the pixel counts of ``m_i > 0.5 and m_j > 0.5`` / ``... or ...``;
    ``pair_ious`` is ``inter / (union + 1e-6)`` (demo/app.py:38-42); ``area`` counts the best mask's pixels above the
    call's ``threshold`` and ``bbox`` is their bounding box ``(x0, y0, x1, y1)``, x1 / y1 exclusive, None when empty."""
    pair_inter: np.ndarray
    pair_union: np.ndarray
    pair_ious: np.ndarray
    area: int
    bbox: Optional[Tuple[int, int, int, int]]

    def is_ambiguous(self, iou_threshold: float = 0.8) -> bool:
        """The demo's rule (demo/app.py:45-56): some pair of masks has IoU below ``iou_threshold``."""
        n = len(self.pair_ious)
        return any(self.pair_ious[i, j] < iou_threshold for i in range(n) for j in range(i + 1, n))

    @classmethod
    def from_words(cls, words: np.ndarray, num_masks: int) -> "MaskStats":
        """Decode a counter block (72 uint32, layout in include/s3od_hip.h at s3od_mask_stats)."""
        w = np.asarray(words, dtype=np.uint32).astype(np.int64)
        inter = np.zeros((num_masks, num_masks), np.int64)
        union = np.zeros((num_masks, num_masks), np.int64)
        for i in range(num_masks):
            inter[i, i] = union[i, i] = w[56 + i]
            for j in range(i + 1, num_masks):
                k = i * (15 - i) // 2 + j - i - 1
                inter[i, j] = inter[j, i] = w[k]
                union[i, j] = union[j, i] = w[28 + k]
        area = int(w[64])
        bbox = (int(w[65]), int(w[66]), int(w[67]), int(w[68])) if area > 0 else None
        return cls(inter, union, inter / (union + 1e-6), area, bbox)


def compose(mask: torch.Tensor, src: Optional[torch.Tensor], mode: int, color: int = 0, bg: Optional[torch.Tensor] = None,
            out: Optional[torch.Tensor] = None, out_offset: int = 0, pitch: Optional[int] = None) -> torch.Tensor:
    """s3od_compose on device tensors: fp32 mask [H0, W0], uint8 src [H0, W0, 3] -> uint8 output.  Without ``out`` a
    dense [H0, W0, C] tensor is returned; with it the rows go to ``out`` (flat uint8) from byte ``out_offset``,
    ``pitch`` bytes apart."""
    from ._lib import lib, stream
    H0, W0 = mask.shape
    if mask.dtype != torch.float32 or not mask.is_contiguous():
        raise ValueError("compose: the mask is a contiguous float32 tensor")
    bpp = _BPP[mode]
    if out is None:
        out = torch.empty((H0, W0, bpp) if bpp > 1 else (H0, W0), dtype=torch.uint8, device=mask.device)
        out_offset, pitch = 0, W0 * bpp
    elif out.numel() < out_offset + (H0 - 1) * pitch + W0 * bpp:
        raise ValueError("compose: the output buffer is too small for the tile")
    lib()("s3od_compose", mask, src, H0, W0, mode, color, bg if mode == MODE_RGB_OVER_IMAGE else None,
          out.data_ptr() + out_offset, pitch, stream())
    return out


def mask_stats_words(masks: torch.Tensor, best: int, threshold: float) -> torch.Tensor:
    """s3od_mask_stats on device masks [NM, H0, W0] -> the device counter block (72 int32-viewed words)."""
    from ._lib import lib, stream
    NM, H0, W0 = masks.shape
    if masks.dtype != torch.float32 or not masks.is_contiguous():
        raise ValueError("mask_stats: the masks are a contiguous float32 tensor")
    words = torch.empty(STATS_WORDS, dtype=torch.int32, device=masks.device)
    lib()("s3od_mask_stats", masks, NM, H0, W0, int(best), float(threshold), words, stream())
    return words


def mask_stats(masks: torch.Tensor, best: int, threshold: float = 0.5) -> MaskStats:
    words = mask_stats_words(masks, best, threshold)
    return MaskStats.from_words(words.cpu().numpy().view(np.uint32), masks.shape[0])


__all__ = ["MaskStats", "compose", "mask_stats", "mask_stats_words", "MODE_RGBA", "MODE_MASK_U8"]

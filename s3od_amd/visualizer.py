"""The reference's visualisation helpers (src/s3od/visualizer.py:8-48) on the device.

``visualize_removal`` blends the image over a background colour with the soft mask; ``visualize_all_masks`` tiles
``mask * image`` for every mask into a grid of at most 4 columns.  Both upload the masks they are given, run
s3od_compose (each grid tile is written in place through the row pitch) and download the uint8 result, which equals
the reference's numpy float32 evaluation byte for byte.  There is no host fallback: without a GPU they raise.
"""
from __future__ import annotations

from typing import Tuple, Union

import numpy as np
import torch
from PIL import Image

from .image_ops import MODE_RGB_OVER_COLOR, pack_color


def _upload(image, masks):
    if isinstance(image, Image.Image):
        image = np.array(image.convert("RGB"))
    image = np.ascontiguousarray(image, dtype=np.uint8)
    masks = np.ascontiguousarray(masks, dtype=np.float32)
    if image.ndim != 3 or image.shape[2] != 3 or masks.shape[-2:] != image.shape[:2]:
        raise ValueError(f"expected an H x W x 3 image and masks of its size, got {image.shape} and {masks.shape}")
    return torch.from_numpy(image).cuda(), torch.from_numpy(masks).cuda()


def visualize_removal(image: Union[np.ndarray, Image.Image], result, background_color: Tuple[int, int, int] = (0, 255, 0)) -> Image.Image:
    from .compose import compose
    color = pack_color(background_color)
    img, mask = _upload(image, result.predicted_mask)
    return Image.fromarray(compose(mask, img, MODE_RGB_OVER_COLOR, color).cpu().numpy())


def visualize_all_masks(image: Union[np.ndarray, Image.Image], result) -> Image.Image:
    from .compose import compose
    img, masks = _upload(image, result.all_masks)
    h, w = img.shape[:2]
    num_masks = len(masks)
    grid_width = min(num_masks, 4)
    grid_height = (num_masks + grid_width - 1) // grid_width
    grid = torch.zeros((h * grid_height, w * grid_width, 3), dtype=torch.uint8, device=img.device)
    pitch = w * grid_width * 3
    for idx in range(num_masks):
        row, col = idx // grid_width, idx % grid_width
        # mask * image is the blend over black: (1 - mask) * 0 adds a zero
        compose(masks[idx], img, MODE_RGB_OVER_COLOR, 0, out=grid.view(-1), out_offset=row * h * pitch + col * w * 3, pitch=pitch)
    return Image.fromarray(grid.cpu().numpy())


__all__ = ["visualize_removal", "visualize_all_masks"]

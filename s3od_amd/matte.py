"""Edge-aware alpha refinement and foreground colour estimation on device (s3od_matte_refine, s3od_matte_foreground).

``refine_alpha`` is the colour guided filter (He, Sun, Tang 2013) of a soft mask against the full-size source image:
the model's mask is resampled from S x S, so on a large photograph its edges are ramps that do not follow the image;
the filter makes them follow it.  ``estimate_foreground`` is the blur-fusion foreground estimate (Forte & Pitie 2021,
one pass): the colour a semi-transparent pixel would have without the old background, so a composite over a new one
carries no fringe.  ``Refine`` switches both on in ``BackgroundRemoval.remove_background`` / ``remove_background_many``.
Both are windowed means over the image (csrc/matte.hip); there is no host fallback.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional

import torch

MAX_RADIUS = 256
MIN_EPS, MAX_EPS = 1e-6, 1.0
MIN_SIDE, MAX_SIDE = 2, 32768


@dataclass(frozen=True)
class Refine:
    """``refine=`` of ``remove_background`` / ``remove_background_many``: the best mask is guided-filtered against the
    image (box ``radius``, regulariser ``eps``); with ``foreground`` the colours of ``rgba_image`` and ``composite``
    are the foreground estimated with box radius ``fg_radius``.  The ranges are those of the C entries."""
    radius: int = 16
    eps: float = 1e-4
    foreground: bool = True
    fg_radius: int = 64

    def __post_init__(self):
        for name in ("radius", "fg_radius"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= MAX_RADIUS:
                raise ValueError(f"Refine.{name} is an integer in 1..{MAX_RADIUS}, got {v!r}")
        if isinstance(self.eps, bool) or not isinstance(self.eps, (int, float)) or not MIN_EPS <= self.eps <= MAX_EPS:
            raise ValueError(f"Refine.eps is a number in {MIN_EPS}..{MAX_EPS}, got {self.eps!r}")
        if not isinstance(self.foreground, bool):
            raise ValueError(f"Refine.foreground is a bool, got {self.foreground!r}")


_WS = {}        # device -> the reusable scratch of both entries (uint8)


def workspace_bytes(H: int, W: int) -> int:
    """s3od_matte_ws: bytes of scratch both entries need for an H x W image."""
    from ._lib import lib
    need = ctypes.c_long(0)
    lib()("s3od_matte_ws", int(H), int(W), ctypes.addressof(need))
    return int(need.value)


def _workspace(H: int, W: int, device) -> torch.Tensor:
    """The scratch is shared by every call on a device: the calls are ordered by the stream they run on, so use one
    stream per device for them (``BackgroundRemoval`` does)."""
    need = workspace_bytes(H, W)
    ws = _WS.get(device)
    if ws is None or ws.numel() < need:
        ws = _WS[device] = torch.empty(need, dtype=torch.uint8, device=device)
    return ws


def _check(what: str, plane: torch.Tensor, src: torch.Tensor):
    if plane.dtype != torch.float32 or plane.dim() != 2 or not plane.is_contiguous():
        raise ValueError(f"{what}: the mask is a contiguous float32 [H, W] tensor")
    if src.dtype != torch.uint8 or tuple(src.shape) != (*plane.shape, 3) or not src.is_contiguous() or src.device != plane.device:
        raise ValueError(f"{what}: the source is a contiguous uint8 [H, W, 3] tensor of the mask's size and device")


def refine_alpha(mask: torch.Tensor, src: torch.Tensor, radius: int, eps: float,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """s3od_matte_refine on device tensors: fp32 mask [H, W], uint8 src [H, W, 3] -> the refined fp32 [H, W] in
    [0, 1].  ``out`` may be ``mask`` itself."""
    from ._lib import lib, stream
    _check("refine_alpha", mask, src)
    H, W = mask.shape
    if out is None:
        out = torch.empty_like(mask)
    elif out.dtype != torch.float32 or out.shape != mask.shape or not out.is_contiguous() or out.device != mask.device:
        raise ValueError("refine_alpha: out is a contiguous float32 tensor of the mask's size and device")
    ws = _workspace(H, W, mask.device)
    lib()("s3od_matte_refine", mask, src, H, W, int(radius), float(eps), ws, ws.numel(), out, stream())
    return out


def estimate_foreground(alpha: torch.Tensor, src: torch.Tensor, radius: int,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """s3od_matte_foreground on device tensors: fp32 alpha [H, W], uint8 src [H, W, 3] -> uint8 [H, W, 3], the
    estimated foreground colours.  ``out`` (not ``src``) receives them when given."""
    from ._lib import lib, stream
    _check("estimate_foreground", alpha, src)
    H, W = alpha.shape
    if out is None:
        out = torch.empty_like(src)
    elif out.dtype != torch.uint8 or out.shape != src.shape or not out.is_contiguous() or out.device != src.device:
        raise ValueError("estimate_foreground: out is a contiguous uint8 tensor of the source's size and device")
    ws = _workspace(H, W, alpha.device)
    lib()("s3od_matte_foreground", alpha, src, H, W, int(radius), ws, ws.numel(), out, stream())
    return out


__all__ = ["Refine", "refine_alpha", "estimate_foreground", "workspace_bytes"]

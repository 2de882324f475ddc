"""The Python side of csrc/image_ops.hip that both predictors, the batching engine, ``compose.py`` and
``visualizer.py`` share: the ctypes mirrors of the descriptor structs, the output modes, the ``background`` argument's
normalisation, ``BackgroundRemoval``'s letterbox geometry with the reference's odd-padding error, and the
single-image pipeline (upload -> ``s3od_preprocess`` -> forward -> ``s3od_sigmoid_unpad_resize``).

A geometry is ``(new_h, new_w, top, left, crop_pad_h, crop_pad_w)``: the letterbox placement of an image on the
S x S canvas and the padding cropped from the model output (h = LH - 2 crop_pad_h, w = LW - 2 crop_pad_w).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from .utils import get_pad_info


class PreDesc(ctypes.Structure):
    """Mirror of struct S3odPreDesc (csrc/image_ops.hip, include/s3od_hip.h)."""
    _fields_ = [("img_off", ctypes.c_long), ("H0", ctypes.c_int), ("W0", ctypes.c_int), ("new_h", ctypes.c_int),
                ("new_w", ctypes.c_int), ("pad_h", ctypes.c_int), ("pad_w", ctypes.c_int)]


class PostDesc(ctypes.Structure):
    """Mirror of struct S3odPostDesc (csrc/image_ops.hip, include/s3od_hip.h)."""
    _fields_ = [("img_off", ctypes.c_long), ("mask_off", ctypes.c_long), ("rgba_off", ctypes.c_long),
                ("tmp_off", ctypes.c_long), ("pad_h", ctypes.c_int), ("pad_w", ctypes.c_int), ("h", ctypes.c_int),
                ("w", ctypes.c_int), ("H0", ctypes.c_int), ("W0", ctypes.c_int)]


class OutDesc(ctypes.Structure):
    """Mirror of struct S3odOutDesc (csrc/image_ops.hip, include/s3od_hip.h)."""
    _fields_ = [("bg_off", ctypes.c_long), ("out_off", ctypes.c_long), ("stats_off", ctypes.c_long),
                ("scratch_off", ctypes.c_long), ("mode", ctypes.c_int), ("color", ctypes.c_int)]


# output modes of s3od_compose / S3odOutDesc.mode
MODE_RGBA, MODE_RGB_OVER_COLOR, MODE_RGB_OVER_IMAGE, MODE_MASK_U8, MODE_NONE = range(5)
STATS_WORDS = 72            # uint32 words of one image's counter block (s3od_mask_stats)


def pack_color(color) -> int:
    """(r, g, b) -> r | g << 8 | b << 16, the ``color`` argument of the C entries."""
    try:
        ok = len(color) == 3 and all(isinstance(c, (int, np.integer)) and not isinstance(c, bool) and 0 <= int(c) <= 255
                                     for c in color)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError(f"a background colour is three integers in 0..255, got {color!r}")
    r, g, b = (int(c) for c in color)
    return r | g << 8 | b << 16


def _is_color(v) -> bool:
    return isinstance(v, (tuple, list)) and len(v) == 3 and all(isinstance(c, (int, np.integer)) for c in v)


def normalize_background(background, shape, index: Optional[int] = None):
    """One image's ``background`` argument -> None, a packed colour (int) or a contiguous uint8 H0 x W0 x 3 array.
    ``shape`` is the image's (H0, W0); any other background size raises ``ValueError`` (backgrounds are not resized)."""
    where = "" if index is None else f"image {index}: "
    if background is None:
        return None
    if _is_color(background):
        return pack_color(background)
    if hasattr(background, "convert") and hasattr(background, "size"):        # a PIL image
        background = np.array(background.convert("RGB"))
    if isinstance(background, np.ndarray):
        if background.dtype != np.uint8:
            raise ValueError(f"{where}a background image is uint8, got {background.dtype}")
        if background.shape != (int(shape[0]), int(shape[1]), 3):
            raise ValueError(f"{where}a background image has the size of its image, {int(shape[0])} x {int(shape[1])} x 3, "
                             f"got {' x '.join(map(str, background.shape))}")
        return np.ascontiguousarray(background)
    raise ValueError(f"{where}background is None, an (r, g, b) tuple, a uint8 H x W x 3 array or a PIL image, got {background!r}")


def normalize_backgrounds(background, shapes):
    """``remove_background_many``'s ``background`` -> one normalised value per image: ``None``, one colour or one image
    for every image, or a list / tuple with one value per image (a wrong length raises ``ValueError``)."""
    if background is None:
        return [None] * len(shapes)
    if isinstance(background, (list, tuple)) and not _is_color(background):
        if len(background) != len(shapes):
            raise ValueError(f"background has {len(background)} values for {len(shapes)} images")
        return [normalize_background(v, s, i) for i, (v, s) in enumerate(zip(background, shapes))]
    return [normalize_background(background, s, i) for i, s in enumerate(shapes)]


def reference_geometry(h: int, w: int, S: int, exact_reference_quirks: bool = True,
                       index: Optional[int] = None) -> Tuple[tuple, bool]:
    """``BackgroundRemoval``'s geometry of an h x w image on the S x S canvas (``utils.get_pad_info``) -> (geometry,
    whether reference Quirk 2 applies: pad 0 but a resized side < S, so the model sees the unpadded image).  Under
    the quirks odd padding raises the reference's ``ValueError`` (predictor.py:83-89), naming ``index``."""
    info = get_pad_info(np.broadcast_to(np.uint8(0), (h, w)), S)
    nh, nw = info["resized_size"]
    ph, pw = info["height_pad"], info["width_pad"]
    if exact_reference_quirks and ((ph > 0 and S - nh != 2 * ph) or (pw > 0 and S - nw != 2 * pw)):
        where = "" if index is None else f"image {index}: "
        raise ValueError(f"{where}could not broadcast input array from shape ({nh},{nw},3) into the padded canvas "
                         f"(reference predictor.py:83-89 behaviour for odd padding)")
    return (nh, nw, ph, pw, ph, pw), exact_reference_quirks and ph == 0 and pw == 0 and (nh, nw) != (S, S)


def preprocess_single(image: np.ndarray, geom: tuple, S: int, device, unpadded: bool = False):
    """Upload + ``s3od_preprocess`` -> the model input [1, 3, S, S] and the uploaded uint8 image.  ``unpadded``
    (Quirk 2, ``padded = resized``): the model input is the new_h x new_w image, which sits at the canvas origin."""
    from ._lib import lib, stream
    nh, nw, top, left = geom[:4]
    img = torch.from_numpy(np.require(image, np.uint8, ["C", "W"])).to(device)
    x = torch.empty((1, 3, S, S), dtype=torch.float32, device=device)
    lib()("s3od_preprocess", img, image.shape[0], image.shape[1], nh, nw, top, left, S, x, stream())
    return (x[:, :, :nh, :nw] if unpadded else x), img


def run_single(model, image: np.ndarray, geom: tuple, S: int, device, unpadded: bool = False):
    """The single-image pipeline: ``preprocess_single`` -> forward -> ``s3od_sigmoid_unpad_resize`` over all masks
    -> the device masks fp32 [NM, H0, W0], the IoU logits [NM] and the uploaded uint8 image."""
    from ._lib import lib, stream
    x, img = preprocess_single(image, geom, S, device, unpadded)
    out = model(x)
    logits = out["pred_masks"][0].contiguous()                 # [NM, LH, LW]
    NM, LH, LW = logits.shape
    H0, W0 = image.shape[:2]
    ph, pw = geom[4:]
    h, w = LH - 2 * ph, LW - 2 * pw                             # masks[:, ph:-ph, pw:-pw]
    tmp = torch.empty((NM, h, W0), dtype=torch.float32, device=device)
    masks = torch.empty((NM, H0, W0), dtype=torch.float32, device=device)
    lib()("s3od_sigmoid_unpad_resize", logits, NM, LH, LW, ph, pw, h, w, H0, W0, tmp, masks, stream())
    return masks, out["pred_iou"][0], img

"""Drop-in inference API (src/s3od/predictor.py:16-139): ``BackgroundRemoval`` / ``RemovalResult``.

Same names, constructor and ``remove_background(image, threshold=0.5) -> RemovalResult``.
The whole path runs on the GPU: uint8 upload -> letterbox resize (cv2 INTER_LINEAR fixed-point
emulation) + ImageNet normalisation -> DINOv3/DPT forward -> sigmoid -> unpad -> antialiased
bilinear resize back to the original size, all in libs3od_hip.so; only the 3 IoU scores,
the masks and the RGBA composition come back to the host, as in the reference.

``remove_background_many(images, threshold, batch_size, return_all_masks)`` does the same for a list
of differently sized images, ``batch_size`` per forward (``infer_many.py``).

Both take ``background=`` (an (r, g, b) colour or an image of the source's size) and ``stats=True``: the subject
composited over the background (``RemovalResult.composite``, the reference visualizer's blend) and the pairwise
mask IoU counts, area and bounding box (``RemovalResult.stats``, a ``MaskStats``) are produced on the device, so
3 B/px and a 288-byte counter block come back in place of float masks (``compose.py``).

Model loading is offline-safe: a local checkpoint path is tried first (``torch.load`` with
``weights_only=True``; ``{"state_dict": ...}``, Lightning ``model.``-prefixed and both
transformers key layouts are accepted), then the Hugging Face cache (``local_files_only``).
``model_id="synthetic"`` builds the deterministic synthetic weights (tests / benchmarks).
Errors: ``ValueError`` when the model cannot be located (predictor.py:59-63).
Reference quirks kept under ``exact_reference_quirks=True`` (the default):
  1. when (image_size - new_h) or (image_size - new_w) is odd and the pad is > 0, the reference
     raises a numpy broadcast ValueError (predictor.py:83-89);
  2. when the pad is 0 but the resized side is < image_size (e.g. 1024x1023), the reference feeds
     the UNPADDED resized image (S x new_w) to the model (predictor.py:89-90: ``padded = resized``),
     whose output is then S x 16*floor(new_w/16) and is resized back from that.
``exact_reference_quirks=False`` pads asymmetrically / to S x S instead.
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from PIL import Image

from .utils import get_pad_info, remove_padding  # noqa: F401  (re-exported like the reference)
from .model import DPTSegmentation
from .compose import MaskStats


@dataclass
class RemovalResult:
    predicted_mask: np.ndarray
    all_masks: np.ndarray
    all_ious: np.ndarray
    rgba_image: Image.Image
    composite: Optional[Image.Image] = None     # the subject over ``background`` (RGB), when one was given
    stats: Optional[MaskStats] = None           # with ``stats=True``


class BackgroundRemoval:
    DEFAULT_MODEL_ID = "okupyn/s3od"
    DEFAULT_CHECKPOINT_NAME = "s3od.pt"

    def __init__(self, model_id: Optional[str] = None, image_size: int = 1024, device: Optional[str] = None,
                 compute_dtype: str = "bf16", exact_reference_quirks: bool = True):
        if image_size % 16 != 0:
            raise ValueError("image_size must be a multiple of 16")
        self.image_size = image_size
        self.device = device or "cuda"
        if not str(self.device).startswith("cuda"):
            raise RuntimeError("BackgroundRemoval runs on the MI355X HIP kernels only (device='cuda')")
        self.exact_reference_quirks = exact_reference_quirks
        model_id = model_id or self.DEFAULT_MODEL_ID
        self.model = self._load_model(model_id, compute_dtype)
        self.model.to(self.device)
        self.model.eval()
        self.mean = np.array([0.485, 0.456, 0.406])
        self.std = np.array([0.229, 0.224, 0.225])
        self._many = None           # staging buffers of remove_background_many, built on first use

    @classmethod
    def from_pretrained(cls, model_id: str, **kwargs):
        return cls(model_id=model_id, **kwargs)

    def _load_model(self, model_id: str, compute_dtype: str) -> torch.nn.Module:
        if model_id == "synthetic":
            return DPTSegmentation(compute_dtype=compute_dtype, init_seed=0)
        path = Path(model_id)
        if not path.exists():
            try:
                from huggingface_hub import hf_hub_download
                path = Path(hf_hub_download(repo_id=model_id, filename=self.DEFAULT_CHECKPOINT_NAME, local_files_only=True))
            except Exception as e:
                raise ValueError(f"Could not load model from {model_id}. Ensure model exists on HuggingFace or provide "
                                 f"valid local path. Error: {e}")
        try:
            ckpt = torch.load(str(path), map_location="cpu", weights_only=True)
        except Exception as e:
            raise ValueError(f"Could not load checkpoint {path} with a safe (weights_only) loader: {e}")
        model = DPTSegmentation(num_classes=1, num_outputs=3, encoder_name="dinov3_base", features=256, use_bn=True,
                                use_clstoken=False, compute_dtype=compute_dtype, init_seed=None)
        model.load_state_dict(ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt)
        return model

    # ------------------------------------------------------------------ pre / post
    def _pad_info(self, image: np.ndarray) -> Dict[str, Any]:
        info = get_pad_info(image, self.image_size)
        nh, nw = info["resized_size"]
        S = self.image_size
        if self.exact_reference_quirks and ((info["height_pad"] > 0 and S - nh != 2 * info["height_pad"]) or
                                            (info["width_pad"] > 0 and S - nw != 2 * info["width_pad"])):
            raise ValueError(f"could not broadcast input array from shape ({nh},{nw},3) into the padded canvas "
                             f"(reference predictor.py:83-89 behaviour for odd padding)")
        return info

    def _preprocess(self, image: np.ndarray) -> Tuple[torch.Tensor, Dict[str, Any]]:
        x, info, _ = self._preprocess_dev(image)
        return x, info

    def _preprocess_dev(self, image: np.ndarray) -> Tuple[torch.Tensor, Dict[str, Any], torch.Tensor]:
        """-> the model input, the padding info and the uploaded uint8 image."""
        from ._lib import lib, stream
        info = self._pad_info(image)
        S = self.image_size
        nh, nw = info["resized_size"]
        img = torch.from_numpy(np.ascontiguousarray(image, dtype=np.uint8)).to(self.device)
        x = torch.empty((1, 3, S, S), dtype=torch.float32, device=self.device)
        lib()("s3od_preprocess", img, image.shape[0], image.shape[1], nh, nw, info["height_pad"], info["width_pad"], S, x, stream())
        if self.exact_reference_quirks and info["height_pad"] == 0 and info["width_pad"] == 0 and (nh, nw) != (S, S):
            # Quirk 2: `padded = resized` -> the model sees the nh x nw image (it sits at the canvas origin)
            x = x[:, :, :nh, :nw]
        return x, info, img

    @torch.no_grad()
    def remove_background(self, image: Union[np.ndarray, Image.Image], threshold: float = 0.5, *, background=None,
                          stats: bool = False) -> RemovalResult:
        """``background``: None, an (r, g, b) tuple or a uint8 array / PIL image of the image's size (any other size
        raises ``ValueError``; backgrounds are not resized) -> ``result.composite``, the subject over it as a PIL RGB
        image.  ``stats=True`` -> ``result.stats`` (``MaskStats``); ``threshold`` sets its ``area`` and ``bbox`` and
        nothing else.  Both run on the device masks (s3od_compose, s3od_mask_stats)."""
        from ._lib import lib, stream
        from .compose import MAX_STAT_MASKS, compose, mask_stats_words
        from .infer_many import MODE_RGB_OVER_COLOR, MODE_RGB_OVER_IMAGE, normalize_background
        if isinstance(image, Image.Image):
            image_pil = image.convert("RGB")
            image = np.array(image_pil)
        else:
            image_pil = Image.fromarray(image)
        bg = normalize_background(background, image.shape[:2])
        x, pad, img_dev = self._preprocess_dev(image)
        out = self.model(x)
        H0, W0 = pad["original_size"]
        LH, LW = out["pred_masks"].shape[2], out["pred_masks"].shape[3]
        h, w = LH - 2 * pad["height_pad"], LW - 2 * pad["width_pad"]
        NM = out["pred_masks"].shape[1]
        tmp = torch.empty((NM, h, W0), dtype=torch.float32, device=x.device)
        masks = torch.empty((NM, H0, W0), dtype=torch.float32, device=x.device)
        lib()("s3od_sigmoid_unpad_resize", out["pred_masks"].contiguous(), NM, LH, LW, pad["height_pad"], pad["width_pad"], h, w,
              H0, W0, tmp, masks, stream())
        pred_ious = torch.sigmoid(out["pred_iou"]).squeeze(0).cpu().numpy()   # 3 floats
        all_masks = masks.cpu().numpy()
        best_idx = pred_ious.argmax()
        predicted_mask = all_masks[best_idx]
        alpha = (predicted_mask * 255).astype(np.uint8)
        rgba = np.dstack([image, alpha])
        composite = mask_stats = None
        if bg is not None:
            if isinstance(bg, int):
                comp = compose(masks[best_idx], img_dev, MODE_RGB_OVER_COLOR, bg)
            else:
                comp = compose(masks[best_idx], img_dev, MODE_RGB_OVER_IMAGE, 0, torch.from_numpy(bg).to(self.device))
            composite = Image.fromarray(comp.cpu().numpy())
        if stats:
            if NM > MAX_STAT_MASKS:
                raise ValueError(f"stats=True supports at most {MAX_STAT_MASKS} masks, the model predicts {NM}")
            words = mask_stats_words(masks, int(best_idx), threshold).cpu().numpy().view(np.uint32)
            mask_stats = MaskStats.from_words(words, NM)
        return RemovalResult(predicted_mask=predicted_mask, all_masks=all_masks, all_ious=pred_ious,
                             rgba_image=Image.fromarray(rgba, mode="RGBA"), composite=composite, stats=mask_stats)

    @torch.no_grad()
    def remove_background_many(self, images: Sequence[Union[np.ndarray, Image.Image]], threshold: float = 0.5,
                               batch_size: int = 8, return_all_masks: bool = True, background=None, stats: bool = False,
                               return_masks: bool = True, return_rgba: bool = True) -> List[RemovalResult]:
        """``remove_background`` over a list of differently sized images, ``batch_size`` per forward
        (s3od_preprocess_batch / s3od_postprocess_batch, see ``infer_many.BatchEngine``).  Results come back
        in input order.  ``return_all_masks=False`` leaves ``all_masks`` None and brings only the best mask
        and the RGBA image back from the device.  Under ``exact_reference_quirks`` every image is validated
        before any GPU work (odd padding raises, naming the image's index) and Quirk-2 images, which cannot
        share the S x S canvas, take the single-image path.

        ``background`` (None, one colour or image for every image, or a list with one value per image) and
        ``stats`` are those of ``remove_background``; the composite is written by the post-processing kernels
        where they write RGBA, the background images ride in the same staging buffer and upload as the sources,
        and the counters come from the device masks.  ``return_masks=False`` leaves ``predicted_mask`` and
        ``all_masks`` None (no float plane leaves the device) and ``return_rgba=False`` leaves ``rgba_image``
        None; asking for nothing at all raises ``ValueError``."""
        from .infer_many import BatchEngine, classify_geometry, normalize_backgrounds
        if batch_size < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        if not (return_masks or return_rgba or stats or background is not None):
            raise ValueError("nothing requested: return_masks, return_rgba, stats and background are all off")
        arrays = [np.array(im.convert("RGB")) if isinstance(im, Image.Image) else im for im in images]
        S = self.image_size
        classes = []
        for i, a in enumerate(arrays):
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"image {i}: expected an H x W x 3 array, got shape {a.shape}")
            classes.append(classify_geometry(a.shape[0], a.shape[1], S, self.exact_reference_quirks, index=i))
        bgs = normalize_backgrounds(background, [a.shape[:2] for a in arrays])
        extras = background is not None or stats or not return_masks or not return_rgba
        results: List[Optional[RemovalResult]] = [None] * len(arrays)
        batched = [i for i, c in enumerate(classes) if c == "batched"]
        geoms = []
        for i in batched:
            info = get_pad_info(arrays[i], S)
            nh, nw = info["resized_size"]
            geoms.append((nh, nw, info["height_pad"], info["width_pad"], info["height_pad"], info["width_pad"]))
        if self._many is None:
            self._many = BatchEngine(self.model, S, self.device)
        contiguous = [np.ascontiguousarray(arrays[i], dtype=np.uint8) for i in batched]
        NM = self.model.num_outputs
        if not extras:
            outs = self._many.run(contiguous, geoms, batch_size, NM, all_masks=return_all_masks)
            outs = [o + (None, None) for o in outs]
        else:
            outs = self._many.run(contiguous, geoms, batch_size, NM, all_masks=return_all_masks, want_rgba=return_rgba,
                                  want_masks=return_masks, backgrounds=[bgs[i] for i in batched], want_stats=stats,
                                  threshold=threshold)
        for i, (ious, best, masks, rgba, comp, words) in zip(batched, outs):   # the images wrap the arrays they own: no second copy
            results[i] = RemovalResult(
                predicted_mask=None if masks is None else (masks[best] if return_all_masks else masks[0]),
                all_masks=masks if return_all_masks else None, all_ious=ious,
                rgba_image=None if rgba is None else
                Image.frombuffer("RGBA", (rgba.shape[1], rgba.shape[0]), rgba, "raw", "RGBA", 0, 1),
                composite=comp,
                stats=None if words is None else MaskStats.from_words(words, NM))
        for i, c in enumerate(classes):
            if c == "single":
                bg = bgs[i]
                if isinstance(bg, int):
                    bg = (bg & 255, bg >> 8 & 255, bg >> 16 & 255)
                r = self.remove_background(arrays[i], threshold, background=bg, stats=stats)
                results[i] = RemovalResult(r.predicted_mask if return_masks else None,
                                           r.all_masks if return_masks and return_all_masks else None, r.all_ious,
                                           r.rgba_image if return_rgba else None, r.composite, r.stats)
        return results

    @torch.no_grad()
    def remove_background_batch(self, images: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Batched device entry (C2/C5 benchmarks): normalised [B,3,S,S] -> sigmoid masks + ious on device."""
        out = self.model(images)
        return {"masks": torch.sigmoid(out["pred_masks"]), "ious": torch.sigmoid(out["pred_iou"])}

"""Drop-in inference API (src/s3od/predictor.py:16-139): ``BackgroundRemoval`` / ``RemovalResult``.

Same names, constructor and ``remove_background(image, threshold=0.5) -> RemovalResult``.
The whole path runs on the GPU: uint8 upload -> letterbox resize (cv2 INTER_LINEAR fixed-point
emulation) + ImageNet normalisation -> DINOv3/DPT forward -> sigmoid -> unpad -> antialiased
bilinear resize back to the original size, all in libs3od_hip.so; only the 3 IoU scores,
the masks and the RGBA composition come back to the host, as in the reference.

``remove_background_many(images, threshold, batch_size, return_all_masks)`` does the same for a list
of differently sized images, ``batch_size`` per forward (``infer_many.py``).  Both take an image's geometry from
``_geometry`` (``image_ops.reference_geometry``, the one place that raises Quirk 1 and detects Quirk 2); the
single-image pipeline is ``image_ops.run_single``, which ``SODPredictor.predict`` shares, and Quirk-2 images of a
list go through it (``_remove_background``) because they cannot share the S x S canvas.

Both take ``background=`` (an (r, g, b) colour or an image of the source's size) and ``stats=True``: the subject
composited over the background (``RemovalResult.composite``, the reference visualizer's blend) and the pairwise
mask IoU counts, area and bounding box (``RemovalResult.stats``, a ``MaskStats``) are produced on the device, so
3 B/px and a 288-byte counter block come back in place of float masks (``compose.py``).  ``refine=Refine(...)``
(``matte.py``) guided-filters the best mask against the full-size image and estimates the foreground colours, on the
device: ``predicted_mask``, the alpha and the colours of ``rgba_image`` and ``composite`` are the refined ones, while
``all_masks``, ``all_ious`` and ``stats`` stay as the model produced them.  ``refine=None`` changes nothing.

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
from .compose import MAX_STAT_MASKS, MaskStats, compose, mask_stats_words
from .matte import Refine, estimate_foreground, refine_alpha
from .image_ops import (MODE_RGB_OVER_COLOR, MODE_RGB_OVER_IMAGE, normalize_background, normalize_backgrounds,
                        preprocess_single, reference_geometry, run_single)
from .infer_many import BatchEngine, Request


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
    def _geometry(self, h: int, w: int, index: Optional[int] = None) -> Tuple[tuple, bool]:
        """-> the geometry of an h x w image and whether Quirk 2 applies; odd padding raises (Quirk 1)."""
        return reference_geometry(h, w, self.image_size, self.exact_reference_quirks, index)

    def _preprocess(self, image: np.ndarray) -> Tuple[torch.Tensor, Dict[str, Any]]:
        geom, quirk2 = self._geometry(*image.shape[:2])
        x, _ = preprocess_single(image, geom, self.image_size, self.device, unpadded=quirk2)
        return x, get_pad_info(image, self.image_size)

    @torch.no_grad()
    def remove_background(self, image: Union[np.ndarray, Image.Image], threshold: float = 0.5, *, background=None,
                          stats: bool = False, refine: Optional[Refine] = None) -> RemovalResult:
        """``background``: None, an (r, g, b) tuple or a uint8 array / PIL image of the image's size (any other size
        raises ``ValueError``; backgrounds are not resized) -> ``result.composite``, the subject over it as a PIL RGB
        image.  ``stats=True`` -> ``result.stats`` (``MaskStats``); ``threshold`` sets its ``area`` and ``bbox`` and
        nothing else.  Both run on the device masks (s3od_compose, s3od_mask_stats).  ``refine``: a ``Refine``; the
        best mask is refined against the image (s3od_matte_refine) and, with ``Refine.foreground``, the colours of
        ``rgba_image`` and ``composite`` are the estimated foreground (s3od_matte_foreground)."""
        if isinstance(image, Image.Image):
            image = np.array(image.convert("RGB"))
        return self._remove_background(image, threshold, normalize_background(background, image.shape[:2]), stats, refine)

    def _remove_background(self, image: np.ndarray, threshold: float, bg, stats: bool,
                           refine: Optional[Refine] = None) -> RemovalResult:
        """``remove_background`` of an array with the background already normalised (``normalize_background``)."""
        if image.dtype != np.uint8:
            raise TypeError(f"an image array is uint8, got {image.dtype}")
        if refine is not None and not isinstance(refine, Refine):
            raise TypeError(f"refine is None or a Refine, got {refine!r}")
        geom, quirk2 = self._geometry(*image.shape[:2])
        masks, iou_logits, img_dev = run_single(self.model, image, geom, self.image_size, self.device, unpadded=quirk2)
        pred_ious = torch.sigmoid(iou_logits).cpu().numpy()   # 3 floats
        all_masks = masks.cpu().numpy()
        best_idx = pred_ious.argmax()
        predicted_mask, best_dev, colors, colors_dev = all_masks[best_idx], masks[best_idx], image, img_dev
        if refine is not None:                  # the planes of all_masks and the statistics stay the model's
            best_dev = refine_alpha(best_dev, img_dev, refine.radius, refine.eps)
            predicted_mask = best_dev.cpu().numpy()
            if refine.foreground:
                colors_dev = estimate_foreground(best_dev, img_dev, refine.fg_radius)
                colors = colors_dev.cpu().numpy()
        alpha = (predicted_mask * 255).astype(np.uint8)
        rgba = np.dstack([colors, alpha])
        composite = mask_stats = None
        if bg is not None:
            if isinstance(bg, int):
                comp = compose(best_dev, colors_dev, MODE_RGB_OVER_COLOR, bg)
            else:
                comp = compose(best_dev, colors_dev, MODE_RGB_OVER_IMAGE, 0, torch.from_numpy(bg).to(self.device))
            composite = Image.fromarray(comp.cpu().numpy())
        if stats:
            if len(masks) > MAX_STAT_MASKS:
                raise ValueError(f"stats=True supports at most {MAX_STAT_MASKS} masks, the model predicts {len(masks)}")
            words = mask_stats_words(masks, int(best_idx), threshold).cpu().numpy().view(np.uint32)
            mask_stats = MaskStats.from_words(words, len(masks))
        return RemovalResult(predicted_mask=predicted_mask, all_masks=all_masks, all_ious=pred_ious,
                             rgba_image=Image.fromarray(rgba, mode="RGBA"), composite=composite, stats=mask_stats)

    @torch.no_grad()
    def remove_background_many(self, images: Sequence[Union[np.ndarray, Image.Image]], threshold: float = 0.5,
                               batch_size: int = 8, return_all_masks: bool = True, background=None, stats: bool = False,
                               return_masks: bool = True, return_rgba: bool = True, *,
                               refine: Optional[Refine] = None) -> List[RemovalResult]:
        """``remove_background`` over a list of differently sized images, ``batch_size`` per forward
        (s3od_preprocess_batch / s3od_postprocess_batch_out, see ``infer_many.BatchEngine``).  Results come back
        in input order.  ``return_all_masks=False`` leaves ``all_masks`` None and brings only the best mask
        and the RGBA image back from the device.  Under ``exact_reference_quirks`` every image is validated
        before any GPU work (odd padding raises, naming the image's index) and Quirk-2 images, which cannot
        share the S x S canvas, take the single-image path.

        ``background`` (None, one colour or image for every image, or a list with one value per image) and
        ``stats`` are those of ``remove_background``; the composite is written by the post-processing kernels
        where they write RGBA, the background images ride in the same staging buffer and upload as the sources,
        and the counters come from the device masks.  ``return_masks=False`` leaves ``predicted_mask`` and
        ``all_masks`` None (no float plane leaves the device) and ``return_rgba=False`` leaves ``rgba_image``
        None; asking for nothing at all raises ``ValueError``.

        ``refine`` is that of ``remove_background`` and gives the same bytes: the best float plane stays on the device,
        the refinement, the foreground estimate and s3od_compose run per image on the compute stream and write into
        the packed outputs, so upload, compute and download overlap as without it."""
        if refine is not None and not isinstance(refine, Refine):
            raise TypeError(f"refine is None or a Refine, got {refine!r}")
        if batch_size < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        if not (return_masks or return_rgba or stats or background is not None):
            raise ValueError("nothing requested: return_masks, return_rgba, stats and background are all off")
        arrays = [np.array(im.convert("RGB")) if isinstance(im, Image.Image) else im for im in images]
        geoms = []
        for i, a in enumerate(arrays):
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError(f"image {i}: expected an H x W x 3 array, got shape {a.shape}")
            geoms.append(self._geometry(a.shape[0], a.shape[1], index=i))
        bgs = normalize_backgrounds(background, [a.shape[:2] for a in arrays])
        results: List[Optional[RemovalResult]] = [None] * len(arrays)
        batched = [i for i, (_, quirk2) in enumerate(geoms) if not quirk2]
        if self._many is None:
            self._many = BatchEngine(self.model, self.image_size, self.device)
        NM = self.model.num_outputs
        outs = self._many.run([np.ascontiguousarray(arrays[i], dtype=np.uint8) for i in batched],
                              [geoms[i][0] for i in batched], batch_size, NM,
                              Request(all_masks=return_all_masks, want_masks=return_masks, want_rgba=return_rgba,
                                      backgrounds=[bgs[i] for i in batched], want_stats=stats, threshold=threshold,
                                      refine=refine))
        for i, o in zip(batched, outs):     # the images wrap the arrays they own: no second copy
            results[i] = RemovalResult(
                predicted_mask=o.refined if refine is not None else
                None if o.masks is None else o.masks[o.best if return_all_masks else 0],
                all_masks=o.masks if return_all_masks else None, all_ious=o.ious,
                rgba_image=None if o.rgba is None else
                Image.frombuffer("RGBA", (o.rgba.shape[1], o.rgba.shape[0]), o.rgba, "raw", "RGBA", 0, 1),
                composite=o.composite,
                stats=None if o.stats_words is None else MaskStats.from_words(o.stats_words, NM))
        for i, (_, quirk2) in enumerate(geoms):
            if quirk2:                      # the single-image path, trimmed to what was asked for
                r = results[i] = self._remove_background(arrays[i], threshold, bgs[i], stats, refine)
                if not return_rgba:
                    r.rgba_image = None
                if not (return_masks and return_all_masks):
                    r.all_masks = None
                if not return_masks:
                    r.predicted_mask = None
        return results

    @torch.no_grad()
    def remove_background_batch(self, images: torch.Tensor) -> Dict[str, torch.Tensor]:
        """Batched device entry (C2/C5 benchmarks): normalised [B,3,S,S] -> sigmoid masks + ious on device."""
        out = self.model(images)
        return {"masks": torch.sigmoid(out["pred_masks"]), "ious": torch.sigmoid(out["pred_iou"])}

"""Flip-consistency scoring on the device: the operation under hard-sample mining
(``synth_sod/src/synth_sod/model_training/mine_samples.py:16-51`` ``eval_sample``) and the flip-consistency dataset
filter (``synth_sod/src/synth_sod/data_generation/filters/consistency_filter.py:49-95``).

Both predict an image and its horizontal mirror and compare the two masks with the ground truth and with each other:
mining through three S-measures, the filter through three binary IoUs.  Here the image is uploaded once, mirrored on
the device (``s3od_mirror_u8``, on the source image before the letterbox as ``cv2.flip(image, 1)`` + ``predict``
does; mirroring the letterboxed canvas is not the same, the fixed-point resize coordinates and the floor-of-half
padding are not symmetric), both go through one forward, and one ``s3od_flip_scores`` call reads the two soft masks
and the ground truth and returns the three S-measures and the six IoU counts.  The mirrored prediction is never
un-mirrored in memory: the kernel reads it through the mirror.  Nothing but the nine numbers per image comes back to
the host.

S semantics are those of three ``EvaluationMetrics(sm_only=True).step`` calls in a row on the same tensors: step 1
binarises the ground truth in place at 0.5 (unless its mean is 0 or 1), so step 2 scores against the binarised plane.
The caller's ``gt`` is not modified here.
"""
from __future__ import annotations

import ctypes
import math
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np
import torch

from ._lib import lib, stream

N_OUT = 9       # doubles s3od_flip_scores writes


class FlipScores(NamedTuple):
    s_orig: float           # S(prediction, gt)
    s_flip: float           # S(un-mirrored prediction of the mirror, gt as step 1 left it)
    s_cons: float           # S(prediction, un-mirrored prediction of the mirror); NaN kept
    iou_orig_gt: float      # binary IoUs; an empty union gives 1.0
    iou_flip_gt: float
    iou_orig_flip: float
    score: float            # eval_sample's mining score


def _iou(inter: float, union: float) -> float:
    return float(inter / union) if union > 0 else 1.0


def scores_from_out(v: Sequence[float]) -> FlipScores:
    """The nine doubles of ``s3od_flip_scores`` -> ``FlipScores`` (``eval_sample``'s NaN fallback and product)."""
    s_orig, s_flip, s_cons = float(v[0]), float(v[1]), float(v[2])
    s_cons_eff = (s_orig + s_flip) / 2 if math.isnan(s_cons) else s_cons
    return FlipScores(s_orig, s_flip, s_cons, _iou(v[3], v[4]), _iou(v[5], v[6]), _iou(v[7], v[8]),
                      (s_orig + s_flip) * s_cons_eff / 2)


def _ws_words() -> int:
    need = ctypes.c_long(0)
    lib()("s3od_flip_scores_ws", 2, 2, ctypes.addressof(need))      # the size does not depend on the image
    return (need.value + 7) // 8


def flip_scores_out(a: torch.Tensor, bm: torch.Tensor, gt: torch.Tensor, threshold: float = 0.5, out=None, ws=None):
    """``s3od_flip_scores`` on device planes fp32 [H, W] (``bm`` still mirrored) -> device float64 [9]."""
    if not (a.shape == bm.shape == gt.shape and a.dim() == 2):
        raise ValueError(f"planes differ: a {tuple(a.shape)}, bm {tuple(bm.shape)}, gt {tuple(gt.shape)}")
    for t in (a, bm, gt):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("flip_scores takes contiguous float32 planes")
    H, W = a.shape
    if out is None:
        out = torch.empty(N_OUT, dtype=torch.float64, device=a.device)
    if ws is None:
        ws = torch.empty(_ws_words(), dtype=torch.float64, device=a.device)
    lib()("s3od_flip_scores", a, bm, gt, H, W, float(threshold), ws, ws.numel() * 8, out, stream())
    return out


def _gt_array(gt):
    """A ground truth [H0, W0] (a leading 1-dim is accepted) as a host or device tensor, values as given."""
    t = torch.from_numpy(np.ascontiguousarray(gt)) if isinstance(gt, np.ndarray) else torch.as_tensor(gt)
    if t.dim() < 2 or t.numel() != t.shape[-2] * t.shape[-1]:
        raise ValueError(f"a ground truth is an [H, W] array, got shape {tuple(t.shape)}")
    return t.reshape(t.shape[-2], t.shape[-1])


class FlipScorer:
    """The mirror-pair path on one ``SODPredictor``: ``masks`` (the two device soft masks), ``score`` (one image) and
    ``score_many`` (``batch_size`` images, i.e. ``2 * batch_size`` canvases, per forward)."""

    def __init__(self, predictor, threshold: float = 0.5):
        self.predictor = predictor
        self.threshold = float(threshold)
        self._ws_words = None

    # ------------------------------------------------------------------ the pair of predictions
    def _image(self, image, index=None) -> np.ndarray:
        a = np.asarray(image)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            where = "" if index is None else f"image {index}: "
            raise ValueError(f"{where}expected a uint8 H x W x 3 array, got {a.dtype} {a.shape}")
        return np.require(a, np.uint8, ["C", "W"])      # torch.from_numpy wants a writable array (PIL's are not)

    @torch.no_grad()
    def _pairs(self, arrays: List[np.ndarray]) -> List[Tuple[torch.Tensor, torch.Tensor]]:
        """One forward over the images and their mirrors -> per image (a, bm), device fp32 [H0, W0]."""
        p = self.predictor
        S, dev, model = p.image_size, p.device, p.model
        L = lib()
        n = len(arrays)
        x = torch.empty((2 * n, 3, S, S), dtype=torch.float32, device=dev)
        geoms = []
        for i, im in enumerate(arrays):
            H0, W0 = im.shape[:2]
            pair = torch.empty((2, H0, W0, 3), dtype=torch.uint8, device=dev)
            pair[0].copy_(torch.from_numpy(im))                          # the one upload
            L("s3od_mirror_u8", pair[0], H0, W0, 3, pair[1], stream())
            g = p._geometry(H0, W0)
            geoms.append(g)
            nh, nw, top, left = g[:4]
            for k in range(2):
                L("s3od_preprocess", pair[k], H0, W0, nh, nw, top, left, S, x[2 * i + k], stream())
        out = model(x)
        logits, iou_logits = out["pred_masks"], out["pred_iou"]
        NM, LH, LW = logits.shape[1:]
        pairs = []
        for i, im in enumerate(arrays):
            H0, W0 = im.shape[:2]
            ph, pw = geoms[i][4:]
            h, w = LH - 2 * ph, LW - 2 * pw
            tmp = torch.empty((NM, h, W0), dtype=torch.float32, device=dev)
            planes = []
            for k in range(2):
                lg = logits[2 * i + k].contiguous()
                masks = torch.empty((NM, H0, W0), dtype=torch.float32, device=dev)
                L("s3od_sigmoid_unpad_resize", lg, NM, LH, LW, ph, pw, h, w, H0, W0, tmp, masks, stream())
                if NM == 1:
                    planes.append(masks[0])
                else:       # each prediction takes its own best plane, as two predict() calls would; no host read
                    best = torch.sigmoid(iou_logits[2 * i + k]).argmax().reshape(1)
                    planes.append(masks.index_select(0, best)[0])
            pairs.append((planes[0], planes[1]))
        return pairs

    def masks(self, image) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (a, bm): the soft mask of ``image`` and the soft mask of its mirror, still mirrored; device fp32 [H0, W0]."""
        return self._pairs([self._image(image)])[0]

    # ------------------------------------------------------------------ scores
    def _check(self, images, gts):
        if len(images) != len(gts):
            raise ValueError(f"{len(images)} images but {len(gts)} ground truths")
        arrays, planes = [], []
        for i, (im, gt) in enumerate(zip(images, gts)):
            a = self._image(im, i)
            g = _gt_array(gt)
            if tuple(g.shape) != a.shape[:2]:
                raise ValueError(f"image {i}: ground truth {tuple(g.shape)} does not match the image {a.shape[:2]}")
            if a.shape[0] < 2 or a.shape[1] < 2:
                raise ValueError(f"image {i}: the S-measure needs at least 2 x 2 pixels, got {a.shape[:2]}")
            arrays.append(a)
            planes.append(g)
        return arrays, planes

    @torch.no_grad()
    def _out_chunk(self, arrays, planes) -> np.ndarray:
        """One forward + one scoring pass per image -> host float64 [n, 9] (the chunk's one host read)."""
        dev = self.predictor.device
        if self._ws_words is None:
            self._ws_words = _ws_words()
        n = len(arrays)
        out = torch.empty((n, N_OUT), dtype=torch.float64, device=dev)
        ws = torch.empty((n, self._ws_words), dtype=torch.float64, device=dev)
        for i, (a, bm) in enumerate(self._pairs(arrays)):
            g = planes[i].to(device=dev, dtype=torch.float32).contiguous()
            flip_scores_out(a.contiguous(), bm.contiguous(), g, self.threshold, out[i], ws[i])
        return out.cpu().numpy()

    def raw_many(self, images, gts, batch_size: int = 4) -> np.ndarray:
        """``score_many``'s numbers as ``s3od_flip_scores`` wrote them: float64 [n, 9] = the three S-measures and the
        intersection / union counts of the three IoU pairs."""
        if batch_size < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        arrays, planes = self._check(list(images), list(gts))
        chunks = [self._out_chunk(arrays[i:i + batch_size], planes[i:i + batch_size])
                  for i in range(0, len(arrays), batch_size)]
        return np.concatenate(chunks) if chunks else np.zeros((0, N_OUT))

    def score(self, image, gt) -> FlipScores:
        """``gt``: numpy or torch [H0, W0]; floats in [0, 1] and uint8 {0, 1} are used as given.  A shape that does not
        match the image raises ``ValueError`` before the model runs."""
        return scores_from_out(self.raw_many([image], [gt], 1)[0])

    def score_many(self, images, gts, batch_size: int = 4) -> List[FlipScores]:
        """``score`` over lists, ``batch_size`` images (``2 * batch_size`` canvases) per forward; the images may differ in
        size; results in input order, one host read per chunk."""
        return [scores_from_out(v) for v in self.raw_many(images, gts, batch_size)]

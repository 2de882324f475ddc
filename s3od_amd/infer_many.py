"""Batched inference over a list of differently sized images (``remove_background_many`` / ``predict_many``).

Per chunk of ``batch_size`` images: the images and both descriptor tables are written into one pinned staging
buffer and uploaded with one async copy on a copy stream; ``s3od_preprocess_batch`` -> one batched forward ->
``s3od_best_index`` -> ``s3od_postprocess_batch`` run on the current stream with no host round trip; the packed
outputs (IoUs, best index, soft masks, RGBA) come back with one async copy into pinned memory, on a download
stream, and one event.  Chunk k+1 is staged and uploaded while chunk k computes, and chunk k is downloaded and
split on the host while chunk k+1 computes (two slots of every buffer; events order their reuse).  The arrays handed back are copies: they own
their memory.
"""
from __future__ import annotations

import ctypes
import time
from typing import List, Optional, Sequence, Tuple

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


def classify_geometry(h: int, w: int, image_size: int, exact_reference_quirks: bool = True, index: Optional[int] = None) -> str:
    """Pre-flight class of an h x w image for ``BackgroundRemoval.remove_background_many``.

    ``"batched"``: it shares the S x S canvas of its chunk.  ``"single"``: reference Quirk 2 (pad 0 but a resized
    side < S: the model sees the unpadded image), which goes through the single-image path.  Raises the
    reference's odd-padding ``ValueError`` (predictor.py:83-89), naming ``index``.  Without the quirks every
    image batches."""
    if not exact_reference_quirks:
        return "batched"
    S = image_size
    info = get_pad_info(np.broadcast_to(np.uint8(0), (h, w)), S)
    nh, nw = info["resized_size"]
    ph, pw = info["height_pad"], info["width_pad"]
    if (ph > 0 and S - nh != 2 * ph) or (pw > 0 and S - nw != 2 * pw):
        where = "" if index is None else f"image {index}: "
        raise ValueError(f"{where}could not broadcast input array from shape ({nh},{nw},3) into the padded canvas "
                         f"(reference predictor.py:83-89 behaviour for odd padding)")
    if ph == 0 and pw == 0 and (nh, nw) != (S, S):
        return "single"
    return "batched"


def _align(n: int, a: int = 16) -> int:
    return (n + a - 1) // a * a


class _Slot:
    """One set of staging buffers and the events that order their reuse."""

    def __init__(self):
        self.pin_in = self.dev_in = self.dev_out = self.pin_out = self.tmp = None
        self.h2d = torch.cuda.Event()      # upload of this slot finished (copy stream)
        self.done = torch.cuda.Event()     # kernels that read dev_in finished (compute stream)
        self.out = torch.cuda.Event()      # download into pin_out finished (download stream)
        self.used = False
        self.plan = None         # chunk staged in pin_in / dev_in
        self.out_plan = None     # chunk whose outputs are in dev_out / pin_out (the next chunk may already be staged)


class BatchEngine:
    """Chunked pre -> forward -> best index -> post over a list of uint8 HWC images.

    ``geoms[i] = (new_h, new_w, top, left, crop_pad_h, crop_pad_w)``: the letterbox placement of image i on the
    S x S canvas and the padding cropped from the model output (h = LH - 2 crop_pad_h, w = LW - 2 crop_pad_w)."""

    def __init__(self, model, image_size: int, device):
        self.model, self.S, self.device = model, int(image_size), device
        self.slots = None
        self.copy_stream = self.out_stream = None       # upload / download streams beside the compute stream
        self._inflight: list = []          # replaced buffers stay alive until the call that replaced them has finished
        self.host_seconds = None           # set to {} to accumulate host wall time per phase (tools/infer_many_bench.py)

    def _timed(self, phase, fn, *args):
        if self.host_seconds is None:
            return fn(*args)
        t0 = time.perf_counter()
        r = fn(*args)
        self.host_seconds[phase] = self.host_seconds.get(phase, 0.0) + time.perf_counter() - t0
        return r

    # ------------------------------------------------------------------ buffers
    def _ensure(self, slot: _Slot, name: str, nbytes: int, pinned: bool):
        cur = getattr(slot, name)
        if cur is None or cur.numel() < nbytes:
            if cur is not None:
                self._inflight.append(cur)
            n = max(int(nbytes), 1 << 16)
            n = n + n // 4 if cur is not None else n
            buf = torch.empty(n, dtype=torch.uint8, pin_memory=True) if pinned else \
                torch.empty(n, dtype=torch.uint8, device=self.device)
            setattr(slot, name, buf)
        return getattr(slot, name)

    # ------------------------------------------------------------------ one chunk
    def _plan(self, images, geoms, NM, LH, LW, all_masks, want_rgba):
        """Byte layout of the chunk's staging buffer and packed outputs."""
        B = len(images)
        pre_off = 0
        post_off = _align(pre_off + B * ctypes.sizeof(PreDesc))
        off = _align(post_off + B * ctypes.sizeof(PostDesc))
        pre, post = (PreDesc * B)(), (PostDesc * B)()
        planes = NM if all_masks else 1
        mask_floats = rgba_bytes = tmp_floats = 0
        for b, (img, g) in enumerate(zip(images, geoms)):
            H0, W0 = img.shape[:2]
            nh, nw, top, left, ph, pw = g
            pre[b] = PreDesc(off, H0, W0, nh, nw, top, left)
            h, w = LH - 2 * ph, LW - 2 * pw
            post[b] = PostDesc(off, mask_floats, rgba_bytes, tmp_floats, ph, pw, h, w, H0, W0)
            off = _align(off + H0 * W0 * 3)
            mask_floats += planes * H0 * W0
            rgba_bytes += H0 * W0 * 4 if want_rgba else 0
            tmp_floats += planes * h * W0
        ious_off = 0
        best_off = ious_off + B * NM * 4
        masks_off = _align(best_off + B * 4)
        rgba_off = _align(masks_off + mask_floats * 4)
        return dict(B=B, pre=pre, post=post, pre_off=pre_off, post_off=post_off, in_bytes=off, planes=planes,
                    ious_off=ious_off, best_off=best_off, masks_off=masks_off, rgba_off=rgba_off,
                    out_bytes=rgba_off + rgba_bytes, tmp_bytes=max(tmp_floats * 4, 16), want_rgba=want_rgba,
                    shapes=[img.shape[:2] for img in images])

    def _stage(self, slot: _Slot, images, plan):
        """Fill the pinned staging buffer and start its upload on the copy stream."""
        if slot.used:
            slot.h2d.synchronize()                      # the previous upload has left the pinned buffer
        pin = self._ensure(slot, "pin_in", plan["in_bytes"], True)
        dev = self._ensure(slot, "dev_in", plan["in_bytes"], False)
        ctypes.memmove(pin.data_ptr() + plan["pre_off"], plan["pre"], ctypes.sizeof(plan["pre"]))
        ctypes.memmove(pin.data_ptr() + plan["post_off"], plan["post"], ctypes.sizeof(plan["post"]))
        host = pin.numpy()
        for img, d in zip(images, plan["pre"]):
            n = img.shape[0] * img.shape[1] * 3
            host[d.img_off:d.img_off + n] = img.reshape(-1)
        with torch.cuda.stream(self.copy_stream):
            if slot.used:
                self.copy_stream.wait_event(slot.done)  # the kernels of the chunk that last used dev_in have read it
            dev[:plan["in_bytes"]].copy_(pin[:plan["in_bytes"]], non_blocking=True)
            slot.h2d.record(self.copy_stream)
        slot.plan = plan

    def _launch(self, slot: _Slot, NM, LH, LW, all_masks):
        from ._lib import lib, stream
        plan, S = slot.plan, self.S
        B = plan["B"]
        main = torch.cuda.current_stream()
        main.wait_event(slot.h2d)
        dev_in, pin_in = slot.dev_in, slot.pin_in
        dev_out = self._ensure(slot, "dev_out", plan["out_bytes"], False)
        pin_out = self._ensure(slot, "pin_out", plan["out_bytes"], True)
        tmp = self._ensure(slot, "tmp", plan["tmp_bytes"], False)
        x = torch.empty((B, 3, S, S), dtype=torch.float32, device=self.device)
        lib()("s3od_preprocess_batch", dev_in, dev_in.data_ptr() + plan["pre_off"], pin_in.data_ptr() + plan["pre_off"],
              B, S, x, stream())
        out = self.model(x)
        logits = out["pred_masks"].float().contiguous()
        if tuple(logits.shape) != (B, NM, LH, LW):
            raise RuntimeError(f"model output {tuple(logits.shape)} does not match the planned {(B, NM, LH, LW)}")
        iou_logits = out["pred_iou"].float().reshape(B, NM).contiguous()
        o = dev_out.data_ptr()
        lib()("s3od_best_index", iou_logits, B, NM, o + plan["ious_off"], o + plan["best_off"], stream())
        lib()("s3od_postprocess_batch", logits, B, NM, LH, LW, o + plan["best_off"], dev_in,
              dev_in.data_ptr() + plan["post_off"], pin_in.data_ptr() + plan["post_off"], 1 if all_masks else 0,
              o + plan["masks_off"], (o + plan["rgba_off"]) if plan["want_rgba"] else None, tmp, stream())
        slot.done.record(main)
        with torch.cuda.stream(self.out_stream):        # the download overlaps the next chunk's kernels
            self.out_stream.wait_event(slot.done)
            pin_out[:plan["out_bytes"]].copy_(dev_out[:plan["out_bytes"]], non_blocking=True)
            slot.out.record(self.out_stream)
        slot.out_plan = plan
        slot.used = True                                # x / logits live on the compute stream only: the allocator orders them

    def _collect(self, slot: _Slot, NM) -> List[Tuple[np.ndarray, int, np.ndarray, Optional[np.ndarray]]]:
        plan = slot.out_plan
        self._timed("wait", slot.out.synchronize)
        return self._timed("split", self._split, slot, plan, NM)

    @staticmethod
    def _split(slot: _Slot, plan, NM):
        B, planes = plan["B"], plan["planes"]
        host = slot.pin_out.numpy()
        ious = host[plan["ious_off"]:plan["ious_off"] + B * NM * 4].view(np.float32).reshape(B, NM).copy()
        best = host[plan["best_off"]:plan["best_off"] + B * 4].view(np.int32).copy()
        res = []
        for b, (H0, W0) in enumerate(plan["shapes"]):
            d = plan["post"][b]
            m0 = plan["masks_off"] + d.mask_off * 4
            masks = host[m0:m0 + planes * H0 * W0 * 4].view(np.float32).reshape(planes, H0, W0).copy()
            rgba = None
            if plan["want_rgba"]:
                r0 = plan["rgba_off"] + d.rgba_off
                rgba = host[r0:r0 + H0 * W0 * 4].reshape(H0, W0, 4).copy()
            res.append((ious[b], int(best[b]), masks, rgba))
        return res

    # ------------------------------------------------------------------ the list
    @torch.no_grad()
    def run(self, images: Sequence[np.ndarray], geoms: Sequence[tuple], batch_size: int, NM: int, all_masks: bool = True,
            want_rgba: bool = True):
        """-> per image (ious fp32 [NM], best index, masks fp32 [NM or 1, H0, W0], rgba uint8 [H0, W0, 4] or None)."""
        if not images:
            return []
        if self.slots is None:
            self.slots = [_Slot(), _Slot()]
            self.copy_stream = torch.cuda.Stream(device=self.device)
            self.out_stream = torch.cuda.Stream(device=self.device)
        LH = LW = 16 * (self.S // 16)
        chunks = [(images[i:i + batch_size], geoms[i:i + batch_size]) for i in range(0, len(images), batch_size)]
        results: list = []
        try:
            self._timed("stage", self._stage, self.slots[0], chunks[0][0], self._plan(*chunks[0], NM, LH, LW, all_masks, want_rgba))
            pending = None
            for k in range(len(chunks)):
                if k + 1 < len(chunks):
                    nxt = chunks[k + 1]
                    self._timed("stage", self._stage, self.slots[(k + 1) % 2], nxt[0],
                                self._plan(*nxt, NM, LH, LW, all_masks, want_rgba))
                self._timed("launch", self._launch, self.slots[k % 2], NM, LH, LW, all_masks)
                if pending is not None:
                    results += self._collect(self.slots[pending % 2], NM)
                pending = k
            results += self._collect(self.slots[pending % 2], NM)
        finally:
            # everything of this call has finished (or failed): uploads precede the kernels that were waited for
            self.copy_stream.synchronize()
            self.out_stream.synchronize()
            torch.cuda.current_stream().synchronize()
            self._inflight.clear()
        return results

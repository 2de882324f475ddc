"""Batched inference over a list of differently sized images (``remove_background_many`` / ``predict_many``).

Per chunk of ``batch_size`` images: the images and both descriptor tables are written into one pinned staging
buffer and uploaded with one async copy on a copy stream; ``s3od_preprocess_batch`` -> one batched forward ->
``s3od_best_index`` -> ``s3od_postprocess_batch`` run on the current stream with no host round trip; the packed
outputs (IoUs, best index, soft masks, RGBA) come back with one async copy into pinned memory, on a download
stream, and one event.  Chunk k+1 is staged and uploaded while chunk k computes, and chunk k is downloaded and
split on the host while chunk k+1 computes (two slots of every buffer; events order their reuse).  The arrays handed back are copies: they own
their memory.

With a background, mask statistics or without the float masks the chunk goes through ``s3od_postprocess_batch_out``
instead: an ``OutDesc`` table rides beside the other two, background images beside the sources, and the packed outputs
are IoUs | best | float masks (if wanted) | RGBA and composites | 288-byte counter blocks (``_plan_out``).
"""
from __future__ import annotations

import ctypes
import time
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

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
        self.pin_in = self.dev_in = self.dev_out = self.pin_out = self.tmp = self.scratch = None
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
    def _plan(self, images, geoms, NM, LH, LW, all_masks, want_rgba, opts=None):
        """Byte layout of the chunk's staging buffer and packed outputs."""
        if opts is not None:
            return self._plan_out(images, geoms, NM, LH, LW, all_masks, want_rgba, opts)
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

    def _plan_out(self, images, geoms, NM, LH, LW, all_masks, want_rgba, opts):
        """The layout for s3od_postprocess_batch_out: an S3odOutDesc table of ``n_out`` rows per image (RGBA, the
        composite) behind the other two tables, the background images behind the sources in the same staging buffer,
        and outputs packed as IoUs | best | float masks (if wanted) | RGBA and composites | counter blocks."""
        B = len(images)
        want_masks, want_stats, bgs = opts["want_masks"], opts["want_stats"], opts["backgrounds"]
        rows = ([MODE_RGBA] if want_rgba else []) + ([None] if any(bg is not None for bg in bgs) else [])
        n_out = max(len(rows), 1)
        pre_off = 0
        post_off = _align(pre_off + B * ctypes.sizeof(PreDesc))
        out_desc_off = _align(post_off + B * ctypes.sizeof(PostDesc))
        off = _align(out_desc_off + B * n_out * ctypes.sizeof(OutDesc))
        pre, post, outd = (PreDesc * B)(), (PostDesc * B)(), (OutDesc * (B * n_out))()
        planes = (NM if all_masks else 1) if want_masks else 0
        lplanes = NM if (all_masks or want_stats) else 1            # planes the kernels resample
        use_scratch = want_stats and not (all_masks and want_masks)
        mask_floats = out_bytes = tmp_floats = scratch_floats = 0
        bg_copies = []
        for b, (img, g, bg) in enumerate(zip(images, geoms, bgs)):
            H0, W0 = img.shape[:2]
            nh, nw, top, left, ph, pw = g
            pre[b] = PreDesc(off, H0, W0, nh, nw, top, left)
            h, w = LH - 2 * ph, LW - 2 * pw
            post[b] = PostDesc(off, mask_floats, 0, tmp_floats, ph, pw, h, w, H0, W0)
            off = _align(off + H0 * W0 * 3)
            for k in range(n_out):
                mode = rows[k] if k < len(rows) else MODE_NONE
                color = bg_off = 0
                if mode is None:
                    if bg is None:
                        mode = MODE_NONE
                    elif isinstance(bg, int):
                        mode, color = MODE_RGB_OVER_COLOR, bg
                    else:
                        mode, bg_off = MODE_RGB_OVER_IMAGE, off
                        bg_copies.append((off, bg))
                        off = _align(off + H0 * W0 * 3)
                bpp = (4, 3, 3, 1, 0)[mode]
                outd[b * n_out + k] = OutDesc(bg_off, out_bytes, b * STATS_WORDS * 4 if want_stats else -1,
                                              scratch_floats, mode, color)
                out_bytes = _align(out_bytes + H0 * W0 * bpp)
            mask_floats += planes * H0 * W0
            tmp_floats += lplanes * h * W0
            scratch_floats += NM * H0 * W0 if use_scratch else 0
        ious_off = 0
        best_off = ious_off + B * NM * 4
        masks_off = _align(best_off + B * 4)
        outs_off = _align(masks_off + mask_floats * 4)
        stats_off = _align(outs_off + out_bytes)
        return dict(B=B, pre=pre, post=post, outd=outd, n_out=n_out, rows=rows, pre_off=pre_off, post_off=post_off,
                    out_desc_off=out_desc_off, in_bytes=off, planes=planes, ious_off=ious_off, best_off=best_off,
                    masks_off=masks_off, outs_off=outs_off, stats_off=stats_off,
                    out_bytes=stats_off + (B * STATS_WORDS * 4 if want_stats else 0), tmp_bytes=max(tmp_floats * 4, 16),
                    scratch_bytes=max(scratch_floats * 4, 16) if use_scratch else 0, want_rgba=want_rgba,
                    want_stats=want_stats, threshold=float(opts["threshold"]), bg_copies=bg_copies,
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
        if "outd" in plan:
            ctypes.memmove(pin.data_ptr() + plan["out_desc_off"], plan["outd"], ctypes.sizeof(plan["outd"]))
            for o, bg in plan["bg_copies"]:
                host[o:o + bg.size] = bg.reshape(-1)
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
        if "outd" in plan:
            scratch = self._ensure(slot, "scratch", plan["scratch_bytes"], False) if plan["scratch_bytes"] else None
            lib()("s3od_postprocess_batch_out", logits, B, NM, LH, LW, o + plan["best_off"], dev_in,
                  dev_in.data_ptr() + plan["post_off"], pin_in.data_ptr() + plan["post_off"],
                  dev_in.data_ptr() + plan["out_desc_off"], pin_in.data_ptr() + plan["out_desc_off"], plan["n_out"],
                  1 if all_masks else 0, (o + plan["masks_off"]) if plan["planes"] else None, o + plan["outs_off"], tmp,
                  scratch, (o + plan["stats_off"]) if plan["want_stats"] else None, plan["threshold"], stream())
        else:
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
        if "outd" in plan:
            n_out, rows = plan["n_out"], plan["rows"]
            for b, (H0, W0) in enumerate(plan["shapes"]):
                d = plan["post"][b]
                masks = rgba = comp = words = None
                if planes:
                    m0 = plan["masks_off"] + d.mask_off * 4
                    masks = host[m0:m0 + planes * H0 * W0 * 4].view(np.float32).reshape(planes, H0, W0).copy()
                for k in range(len(rows)):
                    o = plan["outd"][b * n_out + k]
                    r0 = plan["outs_off"] + o.out_off
                    if o.mode == MODE_RGBA:
                        rgba = host[r0:r0 + H0 * W0 * 4].reshape(H0, W0, 4).copy()
                    elif o.mode != MODE_NONE:
                        # PIL keeps RGB as 4 bytes per pixel, so this unpacks into memory the image owns: the one
                        # copy out of the pinned buffer, made here while the next chunk computes
                        comp = Image.frombuffer("RGB", (W0, H0), host[r0:r0 + H0 * W0 * 3], "raw", "RGB", 0, 1)
                if plan["want_stats"]:
                    s0 = plan["stats_off"] + b * STATS_WORDS * 4
                    words = host[s0:s0 + STATS_WORDS * 4].view(np.uint32).copy()
                res.append((ious[b], int(best[b]), masks, rgba, comp, words))
            return res
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
            want_rgba: bool = True, *, want_masks: bool = True, backgrounds: Optional[Sequence] = None,
            want_stats: bool = False, threshold: float = 0.5):
        """-> per image (ious fp32 [NM], best index, masks fp32 [NM or 1, H0, W0], rgba uint8 [H0, W0, 4] or None).

        With ``want_masks=False``, ``backgrounds`` (one ``normalize_background`` value per image) or ``want_stats`` the
        chunk goes through s3od_postprocess_batch_out and the tuples are (ious, best, masks or None, rgba or None,
        composite (a PIL RGB image) or None, counter words uint32 [64] or None)."""
        if not images:
            return []
        opts = None
        if not want_masks or backgrounds is not None or want_stats:
            bgs = list(backgrounds) if backgrounds is not None else [None] * len(images)
            opts = dict(want_masks=want_masks, want_stats=want_stats, threshold=threshold)
            all_masks = all_masks and want_masks
        if self.slots is None:
            self.slots = [_Slot(), _Slot()]
            self.copy_stream = torch.cuda.Stream(device=self.device)
            self.out_stream = torch.cuda.Stream(device=self.device)
        LH = LW = 16 * (self.S // 16)
        chunks = [(images[i:i + batch_size], geoms[i:i + batch_size]) for i in range(0, len(images), batch_size)]
        copts = [None if opts is None else dict(opts, backgrounds=bgs[i:i + batch_size])
                 for i in range(0, len(images), batch_size)]
        results: list = []
        try:
            self._timed("stage", self._stage, self.slots[0], chunks[0][0], self._plan(*chunks[0], NM, LH, LW, all_masks, want_rgba, copts[0]))
            pending = None
            for k in range(len(chunks)):
                if k + 1 < len(chunks):
                    nxt = chunks[k + 1]
                    self._timed("stage", self._stage, self.slots[(k + 1) % 2], nxt[0],
                                self._plan(*nxt, NM, LH, LW, all_masks, want_rgba, copts[k + 1]))
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

"""Batched inference over a list of differently sized images (``remove_background_many`` / ``predict_many``).

Per chunk of ``batch_size`` images ``plan_chunk`` lays out one pinned staging buffer (the three descriptor tables,
the source images, the background images) and the packed outputs (IoUs | best | float masks | RGBA and composites |
288-byte counter blocks).  The staging buffer is uploaded with one async copy on a copy stream;
``s3od_preprocess_batch`` -> one batched forward -> ``s3od_best_index`` -> ``s3od_postprocess_batch_out`` run on the
current stream with no host round trip; the packed outputs come back with one async copy into pinned memory, on a
download stream, and one event.  Chunk k+1 is staged and uploaded while chunk k computes, and chunk k is downloaded
and split on the host while chunk k+1 computes (two slots of every buffer; events order their reuse).  Every call
takes this one path and gets one ``ImageOutputs`` per image; what a ``Request`` leaves out is ``None`` there and
never leaves the device.  The arrays handed back are copies: they own their memory.

With ``Request.refine`` (``matte.Refine``) the post-processing kernels write no RGBA or composite (their rows are
MODE_NONE) and leave the best float plane on the device; ``_refine`` then runs s3od_matte_refine, s3od_matte_foreground
and s3od_compose per image on the compute stream, into the same packed outputs at the planned offsets, before the
slot's ``done`` event: the upload and download overlap is that of the unrefined path.
"""
from __future__ import annotations

import ctypes
import time
from dataclasses import dataclass, replace
from typing import Any, List, NamedTuple, Optional, Sequence

import numpy as np
import torch
from PIL import Image

from .image_ops import (MODE_MASK_U8, MODE_NONE, MODE_RGB_OVER_COLOR, MODE_RGB_OVER_IMAGE, MODE_RGBA,  # noqa: F401
                        STATS_WORDS, OutDesc, PostDesc, PreDesc, normalize_background, normalize_backgrounds, pack_color,
                        reference_geometry)                     # the unused ones stay importable from here
from .matte import Refine


def classify_geometry(h: int, w: int, image_size: int, exact_reference_quirks: bool = True, index: Optional[int] = None) -> str:
    """Pre-flight class of an h x w image for ``BackgroundRemoval.remove_background_many``.

    ``"batched"``: it shares the S x S canvas of its chunk.  ``"single"``: reference Quirk 2, which goes through the
    single-image path.  Odd padding raises, naming ``index``; without the quirks every image batches
    (``image_ops.reference_geometry``)."""
    return "single" if reference_geometry(h, w, image_size, exact_reference_quirks, index)[1] else "batched"


def _align(n: int, a: int = 16) -> int:
    return (n + a - 1) // a * a


@dataclass(frozen=True)
class Request:
    """What a ``BatchEngine.run`` call brings back."""
    all_masks: bool = True          # every float plane, not only the best one
    want_masks: bool = True         # float planes at all
    want_rgba: bool = True
    backgrounds: Optional[Sequence] = None      # per image a ``normalize_background`` value: the composite over it
    want_stats: bool = False
    threshold: float = 0.5          # of the statistics' area and bounding box
    refine: Optional[Refine] = None     # the best mask is refined (and the foreground estimated) before the outputs are written


class ImageOutputs(NamedTuple):
    """One image's outputs; what was not requested is None."""
    ious: np.ndarray                        # fp32 [NM]
    best: int
    masks: Optional[np.ndarray]             # fp32 [NM or 1, H0, W0]
    rgba: Optional[np.ndarray]              # uint8 [H0, W0, 4]
    composite: Optional[Image.Image]        # RGB
    stats_words: Optional[np.ndarray]       # uint32 [STATS_WORDS]
    refined: Optional[np.ndarray] = None    # fp32 [H0, W0]: the refined best mask (``Request.refine`` with masks wanted)


@dataclass
class ChunkPlan:
    """Byte layout of one chunk.  Input offsets are bytes into the staging buffer; ``ious_off`` .. ``stats_off`` are
    bytes into the packed outputs, the descriptors' ``mask_off`` / ``tmp_off`` / ``scratch_off`` count floats from
    ``masks_off`` / the tmp / the scratch buffer and ``out_off`` / ``stats_off`` bytes from ``outs_off`` / ``stats_off``.
    ``rows`` holds what each image's output rows contain; ``outd`` is what the post-processing kernels are told to
    write, which is nothing (MODE_NONE) under ``refine``.  ``out_bytes`` of the packed outputs come back to the host;
    the buffer has ``dev_bytes``, and what lies beyond ``out_bytes`` stays on the device."""
    shapes: List[tuple]
    pre: Any                    # (PreDesc * B) at pre_off
    post: Any                   # (PostDesc * B) at post_off
    outd: Any                   # (OutDesc * (B * n_out)) at out_desc_off
    n_out: int
    rows: List[list]            # per image (mode, out_off, color, bg_off) of every row that is written
    pre_off: int
    post_off: int
    out_desc_off: int
    bg_copies: List[tuple]      # (offset, background image) behind the sources
    in_bytes: int
    all_masks: bool             # the C entry's flag: every plane is kept
    planes: int                 # float planes kept per image: NM, 1 or 0
    threshold: float
    ious_off: int
    best_off: int
    masks_off: int
    outs_off: int
    stats_off: Optional[int]    # None without statistics
    out_bytes: int
    tmp_bytes: int
    scratch_bytes: int          # 0 unless the statistics need planes that are not kept
    dev_planes: int = 0         # float planes the kernels store per image: ``planes``, or 1 when only ``refine`` needs one
    dev_bytes: int = 0
    refine: Optional[Refine] = None
    ref_off: Optional[List[int]] = None     # per image the byte offset of the refined plane in the packed outputs


def plan_chunk(shapes: Sequence[tuple], geoms: Sequence[tuple], NM: int, LH: int, LW: int, req: Request) -> ChunkPlan:
    """The layout of one chunk for s3od_preprocess_batch and s3od_postprocess_batch_out.  The S3odOutDesc table has
    ``n_out`` >= 1 rows per image: an RGBA row when wanted, a composite row when any image of the chunk has a
    background, MODE_NONE where an image has nothing to write."""
    B = len(shapes)
    bgs = [None] * B if req.backgrounds is None else req.backgrounds
    n_out = max(int(req.want_rgba) + int(any(bg is not None for bg in bgs)), 1)
    pre_off = 0
    post_off = _align(pre_off + B * ctypes.sizeof(PreDesc))
    out_desc_off = _align(post_off + B * ctypes.sizeof(PostDesc))
    off = _align(out_desc_off + B * n_out * ctypes.sizeof(OutDesc))
    pre, post, outd = (PreDesc * B)(), (PostDesc * B)(), (OutDesc * (B * n_out))()
    all_masks = req.all_masks and req.want_masks
    planes = (NM if all_masks else 1) if req.want_masks else 0
    dev_planes = max(planes, 1) if req.refine is not None else planes
    lplanes = NM if (all_masks or req.want_stats) else 1            # planes the kernels resample
    use_scratch = req.want_stats and not all_masks
    mask_floats = out_bytes = tmp_floats = scratch_floats = 0
    bg_copies, rows = [], []
    for b, ((H0, W0), g, bg) in enumerate(zip(shapes, geoms, bgs)):
        nh, nw, top, left, ph, pw = g
        pre[b] = PreDesc(off, H0, W0, nh, nw, top, left)
        h, w = LH - 2 * ph, LW - 2 * pw
        post[b] = PostDesc(off, mask_floats, 0, tmp_floats, ph, pw, h, w, H0, W0)
        off = _align(off + H0 * W0 * 3)
        modes = [MODE_RGBA] if req.want_rgba else []
        color = bg_off = 0
        if isinstance(bg, int):
            modes.append(MODE_RGB_OVER_COLOR)
            color = bg
        elif bg is not None:
            modes.append(MODE_RGB_OVER_IMAGE)
            bg_off = off
            bg_copies.append((off, bg))
            off = _align(off + H0 * W0 * 3)
        rows.append([])
        for k, mode in enumerate(modes + [MODE_NONE] * (n_out - len(modes))):
            outd[b * n_out + k] = OutDesc(bg_off if mode == MODE_RGB_OVER_IMAGE else 0, out_bytes,
                                          b * STATS_WORDS * 4 if req.want_stats else -1, scratch_floats,
                                          mode if req.refine is None else MODE_NONE,
                                          color if mode == MODE_RGB_OVER_COLOR else 0)
            if mode != MODE_NONE:
                rows[b].append((mode, out_bytes, color, bg_off))
            out_bytes = _align(out_bytes + H0 * W0 * (4, 3, 3, 1, 0)[mode])
        mask_floats += dev_planes * H0 * W0
        tmp_floats += lplanes * h * W0
        scratch_floats += NM * H0 * W0 if use_scratch else 0
    # packed outputs: IoUs | best | float planes | refined planes (beside every plane) | rows | counters, then what
    # stays on the device: the one plane per image that only the refinement reads
    ious_off = 0
    best_off = ious_off + B * NM * 4
    masks_off = _align(best_off + B * 4)
    ref_floats = sum(H0 * W0 for H0, W0 in shapes) if req.refine is not None and all_masks else 0
    refs_off = _align(masks_off + (mask_floats * 4 if planes else 0))
    outs_off = _align(refs_off + ref_floats * 4)
    stats_off = _align(outs_off + out_bytes)
    end = stats_off + (B * STATS_WORDS * 4 if req.want_stats else 0)
    if dev_planes and not planes:
        masks_off = _align(end)
    ref_off = None
    if req.refine is not None:          # with one plane per image the refinement is in place; otherwise beside the planes
        ref_off = [masks_off + d.mask_off * 4 for d in post]
        if all_masks:
            ref_off = [refs_off + 4 * sum(h * w for h, w in shapes[:b]) for b in range(B)]
    return ChunkPlan(shapes=[tuple(s) for s in shapes], pre=pre, post=post, outd=outd, n_out=n_out, rows=rows, pre_off=pre_off,
                     post_off=post_off, out_desc_off=out_desc_off, bg_copies=bg_copies, in_bytes=off, all_masks=all_masks,
                     planes=planes, threshold=float(req.threshold), ious_off=ious_off, best_off=best_off,
                     masks_off=masks_off, outs_off=outs_off, stats_off=stats_off if req.want_stats else None,
                     out_bytes=end, tmp_bytes=max(tmp_floats * 4, 16),
                     scratch_bytes=max(scratch_floats * 4, 16) if use_scratch else 0, dev_planes=dev_planes,
                     dev_bytes=max(end, masks_off + mask_floats * 4 if dev_planes else 0), refine=req.refine, ref_off=ref_off)


class _Slot:
    """One set of staging buffers and the events that order their reuse."""

    def __init__(self):
        self.pin_in = self.dev_in = self.dev_out = self.pin_out = self.tmp = self.scratch = self.fg = None
        self.h2d = torch.cuda.Event()      # upload of this slot finished (copy stream)
        self.done = torch.cuda.Event()     # kernels that read dev_in finished (compute stream)
        self.out = torch.cuda.Event()      # download into pin_out finished (download stream)
        self.used = False
        self.plan = None         # chunk staged in pin_in / dev_in
        self.out_plan = None     # chunk whose outputs are in dev_out / pin_out (the next chunk may already be staged)


class BatchEngine:
    """Chunked pre -> forward -> best index -> post over a list of uint8 HWC images, each with its geometry
    (``image_ops``: the letterbox placement on the S x S canvas and the padding cropped from the model output)."""

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
    def _stage(self, slot: _Slot, images, plan: ChunkPlan):
        """Fill the pinned staging buffer and start its upload on the copy stream."""
        if slot.used:
            slot.h2d.synchronize()                      # the previous upload has left the pinned buffer
        pin = self._ensure(slot, "pin_in", plan.in_bytes, True)
        dev = self._ensure(slot, "dev_in", plan.in_bytes, False)
        for off, table in ((plan.pre_off, plan.pre), (plan.post_off, plan.post), (plan.out_desc_off, plan.outd)):
            ctypes.memmove(pin.data_ptr() + off, table, ctypes.sizeof(table))
        host = pin.numpy()
        for o, a in [(d.img_off, img) for d, img in zip(plan.pre, images)] + plan.bg_copies:
            host[o:o + a.size] = a.reshape(-1)
        with torch.cuda.stream(self.copy_stream):
            if slot.used:
                self.copy_stream.wait_event(slot.done)  # the kernels of the chunk that last used dev_in have read it
            dev[:plan.in_bytes].copy_(pin[:plan.in_bytes], non_blocking=True)
            slot.h2d.record(self.copy_stream)
        slot.plan = plan

    def _launch(self, slot: _Slot, NM, LH, LW):
        from ._lib import lib, stream
        plan, S = slot.plan, self.S
        B = len(plan.shapes)
        main = torch.cuda.current_stream()
        main.wait_event(slot.h2d)
        dev_in, pin_in = slot.dev_in, slot.pin_in
        dev_out = self._ensure(slot, "dev_out", plan.dev_bytes, False)
        pin_out = self._ensure(slot, "pin_out", plan.out_bytes, True)
        tmp = self._ensure(slot, "tmp", plan.tmp_bytes, False)
        scratch = self._ensure(slot, "scratch", plan.scratch_bytes, False) if plan.scratch_bytes else None
        x = torch.empty((B, 3, S, S), dtype=torch.float32, device=self.device)
        lib()("s3od_preprocess_batch", dev_in, dev_in.data_ptr() + plan.pre_off, pin_in.data_ptr() + plan.pre_off,
              B, S, x, stream())
        out = self.model(x)
        logits = out["pred_masks"].float().contiguous()
        if tuple(logits.shape) != (B, NM, LH, LW):
            raise RuntimeError(f"model output {tuple(logits.shape)} does not match the planned {(B, NM, LH, LW)}")
        iou_logits = out["pred_iou"].float().reshape(B, NM).contiguous()
        o = dev_out.data_ptr()
        lib()("s3od_best_index", iou_logits, B, NM, o + plan.ious_off, o + plan.best_off, stream())
        lib()("s3od_postprocess_batch_out", logits, B, NM, LH, LW, o + plan.best_off, dev_in,
              dev_in.data_ptr() + plan.post_off, pin_in.data_ptr() + plan.post_off,
              dev_in.data_ptr() + plan.out_desc_off, pin_in.data_ptr() + plan.out_desc_off, plan.n_out,
              1 if plan.all_masks else 0, (o + plan.masks_off) if plan.dev_planes else None, o + plan.outs_off, tmp,
              scratch, None if plan.stats_off is None else o + plan.stats_off, plan.threshold, stream())
        if plan.refine is not None:
            self._refine(slot, NM)
        slot.done.record(main)
        with torch.cuda.stream(self.out_stream):        # the download overlaps the next chunk's kernels
            self.out_stream.wait_event(slot.done)
            pin_out[:plan.out_bytes].copy_(dev_out[:plan.out_bytes], non_blocking=True)
            slot.out.record(self.out_stream)
        slot.out_plan = plan
        slot.used = True                                # x / logits live on the compute stream only: the allocator orders them

    def _refine(self, slot: _Slot, NM):
        """Per image of the slot's chunk: the best plane (gathered by the device's best index when every plane is
        kept) is refined in place at ``ref_off``, the foreground is estimated into the slot's colour buffer, and
        s3od_compose writes the image's rows from them.  Everything is enqueued on the compute stream."""
        from .compose import compose
        from .matte import estimate_foreground, refine_alpha
        plan, rf, dev_in, dev_out = slot.plan, slot.plan.refine, slot.dev_in, slot.dev_out
        best = dev_out[plan.best_off:plan.best_off + 4 * len(plan.shapes)].view(torch.int32)
        if rf.foreground:
            fg = self._ensure(slot, "fg", max(H0 * W0 for H0, W0 in plan.shapes) * 3, False)
        for b, (H0, W0) in enumerate(plan.shapes):
            n = H0 * W0
            m = dev_out[plan.ref_off[b]:plan.ref_off[b] + 4 * n].view(torch.float32).view(H0, W0)
            if plan.all_masks:
                m0 = plan.masks_off + plan.post[b].mask_off * 4
                torch.index_select(dev_out[m0:m0 + 4 * NM * n].view(torch.float32).view(NM, n), 0, best[b:b + 1],
                                   out=m.view(1, n))
            src = dev_in[plan.pre[b].img_off:plan.pre[b].img_off + 3 * n].view(H0, W0, 3)
            refine_alpha(m, src, rf.radius, rf.eps, out=m)
            if rf.foreground:
                src = estimate_foreground(m, src, rf.fg_radius, out=fg[:3 * n].view(H0, W0, 3))
            for mode, out_off, color, bg_off in plan.rows[b]:
                compose(m, src, mode, color, dev_in[bg_off:bg_off + 3 * n].view(H0, W0, 3) if mode == MODE_RGB_OVER_IMAGE else None,
                        out=dev_out, out_offset=plan.outs_off + out_off, pitch=W0 * (4, 3, 3, 1)[mode])

    def _collect(self, slot: _Slot, NM) -> List[ImageOutputs]:
        self._timed("wait", slot.out.synchronize)
        return self._timed("split", self._split, slot.pin_out.numpy(), slot.out_plan, NM)

    @staticmethod
    def _split(host: np.ndarray, plan: ChunkPlan, NM) -> List[ImageOutputs]:
        B, planes = len(plan.shapes), plan.planes
        ious = host[plan.ious_off:plan.ious_off + B * NM * 4].view(np.float32).reshape(B, NM).copy()
        best = host[plan.best_off:plan.best_off + B * 4].view(np.int32).copy()
        res = []
        for b, (H0, W0) in enumerate(plan.shapes):
            masks = rgba = comp = words = refined = None
            if planes:
                m0 = plan.masks_off + plan.post[b].mask_off * 4
                masks = host[m0:m0 + planes * H0 * W0 * 4].view(np.float32).reshape(planes, H0, W0).copy()
            if planes and plan.ref_off is not None:
                refined = masks[0] if not plan.all_masks else \
                    host[plan.ref_off[b]:plan.ref_off[b] + H0 * W0 * 4].view(np.float32).reshape(H0, W0).copy()
            for mode, out_off, _, _ in plan.rows[b]:
                r0 = plan.outs_off + out_off
                if mode == MODE_RGBA:
                    rgba = host[r0:r0 + H0 * W0 * 4].reshape(H0, W0, 4).copy()
                else:
                    # PIL keeps RGB as 4 bytes per pixel, so this unpacks into memory the image owns: the one
                    # copy out of the pinned buffer, made here while the next chunk computes
                    comp = Image.frombuffer("RGB", (W0, H0), host[r0:r0 + H0 * W0 * 3], "raw", "RGB", 0, 1)
            if plan.stats_off is not None:
                s0 = plan.stats_off + b * STATS_WORDS * 4
                words = host[s0:s0 + STATS_WORDS * 4].view(np.uint32).copy()
            res.append(ImageOutputs(ious[b], int(best[b]), masks, rgba, comp, words, refined))
        return res

    # ------------------------------------------------------------------ the list
    @torch.no_grad()
    def run(self, images: Sequence[np.ndarray], geoms: Sequence[tuple], batch_size: int, NM: int,
            req: Request = Request()) -> List[ImageOutputs]:
        """One ``ImageOutputs`` per image, in input order; ``req.backgrounds`` holds one value per image of the list."""
        if not images:
            return []
        if self.slots is None:
            self.slots = [_Slot(), _Slot()]
            self.copy_stream = torch.cuda.Stream(device=self.device)
            self.out_stream = torch.cuda.Stream(device=self.device)
        LH = LW = 16 * (self.S // 16)

        def stage(k):
            i = k * batch_size
            chunk = images[i:i + batch_size]
            creq = req if req.backgrounds is None else replace(req, backgrounds=req.backgrounds[i:i + batch_size])
            plan = plan_chunk([im.shape[:2] for im in chunk], geoms[i:i + batch_size], NM, LH, LW, creq)
            self._timed("stage", self._stage, self.slots[k % 2], chunk, plan)
        n_chunks = (len(images) + batch_size - 1) // batch_size
        results: list = []
        try:
            stage(0)
            for k in range(n_chunks):
                if k + 1 < n_chunks:
                    stage(k + 1)
                self._timed("launch", self._launch, self.slots[k % 2], NM, LH, LW)
                if k > 0:
                    results += self._collect(self.slots[(k - 1) % 2], NM)
            results += self._collect(self.slots[(n_chunks - 1) % 2], NM)
        finally:
            # everything of this call has finished (or failed): uploads precede the kernels that were waited for
            self.copy_stream.synchronize()
            self.out_stream.synchronize()
            torch.cuda.current_stream().synchronize()
            self._inflight.clear()
        return results

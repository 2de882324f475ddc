"""Fused multi-tensor AdamW (one HIP launch per step for all parameters).

Semantics of torch.optim.AdamW as configured by the reference
(synth_sod/.../lightning_module.py:183-193): weight_decay=0.05, betas=(0.9, 0.999), eps=1e-8,
two param groups (encoder lr, seg_head lr*10).  Parameters whose ``.grad`` is None are skipped
(no decay, no step count change for them), like torch.  LR schedulers work unchanged because
each group's ``lr`` is re-read every step.

The kernel indexes a parameter, its gradient and both moments with one flat offset, so ``step`` checks on the
host that the four are laid out alike before it launches: a gradient (or loaded moment) with other strides, or with
overlapping elements, is stepped on through a copy laid out like the parameter; a parameter that is not float32 or
not non-overlapping and dense raises ``ValueError``.
"""
from __future__ import annotations

import torch

from ._lib import lib, stream

CHUNK = 65536


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self._tab = None
        self._tab_key = None

    def _table(self, items, dev, step, beta1, wd):
        key = tuple((p.data_ptr(), gr.data_ptr(), self.state[p]["exp_avg"].data_ptr(),
                     self.state[p]["exp_avg_sq"].data_ptr()) for p, _, gr in items)
        bc1 = 1.0 - beta1 ** step                 # Python doubles, rounded to f32 once (as torch)
        coef = torch.tensor([[1.0 - g["lr"] * wd, g["lr"] / bc1] for _, g, _ in items], dtype=torch.float32)
        if key != self._tab_key:
            ptrs, sizes, ct, co = [], [], [], []
            for t, (p, g, gr) in enumerate(items):
                st = self.state[p]
                ptrs.append([p.data_ptr(), gr.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()])
                n = p.numel()
                sizes.append(n)
                for o in range(0, n, CHUNK):
                    ct.append(t); co.append(o)
            self._tab = dict(ptrs=torch.tensor(ptrs, dtype=torch.int64, device=dev),
                             sizes=torch.tensor(sizes, dtype=torch.int64, device=dev),
                             ct=torch.tensor(ct, dtype=torch.int32, device=dev),
                             co=torch.tensor(co, dtype=torch.int64, device=dev), n=len(ct))
            self._tab_key = key
        self._tab["coef"] = coef.to(dev, non_blocking=True)
        return self._tab

    def load_state_dict(self, state_dict):
        """torch.optim.AdamW-compatible state (the device pointer table is rebuilt)."""
        super().load_state_dict(state_dict)
        self._tab, self._tab_key = None, None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # the kernel walks four raw pointers with one flat index: check every layout, and that one launch can serve
        # (one step count, one betas/eps/wd), before any state changes
        live, steps, hyper = [], set(), set()
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = self.state.get(p)
                live.append((p, g, _flat_compatible_grad(p)))
                steps.add(int(float(st["step"])) + 1 if st else 1)
                hyper.add((g["betas"], g["eps"], g["weight_decay"]))
        if not live:
            return loss
        if len(steps) != 1 or len(hyper) != 1:
            raise NotImplementedError("FusedAdamW: all stepped parameters must share step count and betas/eps/wd")
        step = steps.pop()
        for p, g, _ in live:
            st = self.state[p]
            if not st:
                # torch.optim.AdamW layout (step as a float tensor) so state_dicts interchange
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            else:
                for k in ("exp_avg", "exp_avg_sq"):      # a loaded state keeps the strides it was saved with
                    if not _same_layout(st[k], p):
                        st[k] = torch.empty_like(p).copy_(st[k])
            st["step"] = torch.tensor(float(step))
        (b1, b2), eps, wd = hyper.pop()
        tab = self._table(live, live[0][0].device, step, b1, wd)
        lib()("s3od_adamw_step", tab["ptrs"], tab["sizes"], tab["coef"], tab["ct"], tab["co"], tab["n"], CHUNK,
              step, float(b1), float(b2), float(eps), stream())
        # the kernel writes the masters through raw pointers: bump their version counters so
        # every consumer keyed on `_version` (DPTEngine's packed-weight cache) sees the update
        torch.autograd.graph.increment_version([p for p, _, _ in live])
        return loss


def _same_layout(a, b):
    """same shape and the same stride on every axis that has one (the stride of a size-1 axis addresses nothing)"""
    if a.shape != b.shape or a.dtype is not b.dtype:
        return False
    if a.is_contiguous() and b.is_contiguous():      # the usual case, decided without building tuples
        return True
    return all(sa == sb for n, sa, sb in zip(a.shape, a.stride(), b.stride()) if n > 1)


def _non_overlapping_and_dense(t):
    """every element of the storage span [0, numel) belongs to exactly one index: sorted by stride, the axes nest"""
    expect = 1
    for stride, n in sorted((st, n) for n, st in zip(t.shape, t.stride()) if n > 1):
        if stride != expect:
            return False
        expect *= n
    return True


def _flat_compatible_grad(p):
    """The gradient of ``p`` as a tensor that the kernel may index like ``p``: same strides, every element stored
    once.  ``p.grad`` itself where it already is (the engine's flat gradient views), else a copy laid out like ``p``
    (a transposed parameter with a contiguous gradient, an expanded stride-0 gradient).  Raises before any launch
    for a parameter whose own storage has gaps or overlaps, or is not float32: the kernel could only update it
    element-for-wrong-element or past its end."""
    gr = p.grad
    if p.dtype is not torch.float32 or gr.dtype is not torch.float32:
        raise ValueError(f"FusedAdamW: float32 parameters and gradients only, got {p.dtype} / {gr.dtype}")
    if gr.layout is not torch.strided:
        raise ValueError("FusedAdamW: sparse gradients are not supported")
    if p.is_contiguous() and gr.is_contiguous():     # the usual case (torch keeps a gradient's shape its parameter's)
        return gr
    if not _non_overlapping_and_dense(p):
        raise ValueError(f"FusedAdamW: parameter of shape {tuple(p.shape)} with strides {p.stride()} is not "
                         "non-overlapping and dense")
    if not _same_layout(gr, p) or not _non_overlapping_and_dense(gr):
        gr = torch.empty_like(p).copy_(gr)
    return gr


def reference_param_groups(model, lr):
    """lightning_module.py:185-188: encoder at lr, seg_head at lr*10."""
    return [{"params": list(model.encoder.parameters()), "lr": lr},
            {"params": list(model.seg_head.parameters()), "lr": lr * 10}]

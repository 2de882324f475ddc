"""GPU: FusedAdamW / s3od_adamw_step per element against torch.optim.AdamW(foreach=False) run in float64 on the CPU
from the same f32 gradients, at the edges of the chunk table (numel around CHUNK = 65536 and around the 256-thread
stride), with a learning rate that changes every step, gradients from 1e-12 to 1e7, exact zeros, gradients whose
square underflows, a parameter without gradient between stepped ones, re-allocated gradients, a resumed run at a large
step count and gradients laid out differently from their parameter.

Error units, per element:
    p           2^-24 (|p_ref| + lr)        (lr: the largest the element's group saw)
    exp_avg     2^-24 max over steps |g|    (it cancels, so a bound relative to its own value is wrong; a resumed
                                            run counts the loaded |exp_avg| as step 0's |g|)
    exp_avg_sq  2^-24 v_ref + 2^-126        (g = 1e-30: g^2 underflows in f32 and not in float64)
Where a unit is zero (an element whose gradient was always zero) the value has to be exact.

The tolerance is measured against the reference, not fixed: torch's own f32 AdamW(foreach=False) runs on the same
inputs, its worst error against the float64 run is taken in these units, and the kernel may be at most 2x that: both
are f32 evaluations of the same recurrence that differ only in rounding order.  Every test prints both figures.
Measured on the MI355X (worst over all elements, torch f32 / kernel, in units):
    12 steps, lr changing      p 13.29 / 13.29   exp_avg 0.90 / 0.90   exp_avg_sq 9.04 / 10.65
    resume at step 999 + 2     p 13.81 / 13.15   exp_avg 1.53 / 1.53   exp_avg_sq 4.06 /  4.57
    layouts, 3 steps           p  5.67 /  4.81   exp_avg 0.29 / 0.29   exp_avg_sq 5.23 /  5.23
(profiles/decoder_optim_parity_gpu_tests.log).  With eps moved inside the square root the kernel measures p 6.9e7
units on the first of these.
"""
import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 65536
WD, BETAS, EPS = 0.05, (0.9, 0.999), 1e-8
KEYS = ("exp_avg", "exp_avg_sq")


def _torch_adamw(groups):
    return torch.optim.AdamW(groups, weight_decay=WD, betas=BETAS, eps=EPS, foreach=False)


def _groups(params, split, lrs):
    return [{"params": params[:split], "lr": lrs[0]}, {"params": params[split:], "lr": lrs[1]}]


class Trio:
    """the same parameters under FusedAdamW on the GPU, torch AdamW in f32 on the CPU and torch AdamW in float64"""

    def __init__(self, p0, split, state=None):
        from s3od_amd.optim import FusedAdamW
        self.split = split
        self.pk = [torch.nn.Parameter(p.cuda()) for p in p0]          # .cuda() keeps a dense tensor's strides
        self.p32 = [torch.nn.Parameter(p.clone(memory_format=torch.preserve_format)) for p in p0]
        self.p64 = [torch.nn.Parameter(p.double()) for p in p0]
        self.ok = FusedAdamW(_groups(self.pk, split, (1.0, 1.0)), weight_decay=WD, betas=BETAS, eps=EPS)
        self.o32 = _torch_adamw(_groups(self.p32, split, (1.0, 1.0)))
        self.o64 = _torch_adamw(_groups(self.p64, split, (1.0, 1.0)))
        if state is not None:
            for o in (self.ok, self.o32, self.o64):
                o.load_state_dict(copy.deepcopy(state))               # casts the moments to the parameters' dtype and device
        # the magnitude exp_avg's error is measured in: the largest |g| so far, and a loaded exp_avg to begin with
        self.gmax = [torch.zeros_like(p, dtype=torch.float64) if state is None else self.o64.state[q]["exp_avg"].abs().clone()
                     for p, q in zip(p0, self.p64)]
        self.lrmax = [0.0, 0.0]

    def step(self, grads, lrs, grad_k=None):
        """grads: f32 CPU tensors or None per parameter; grad_k: what FusedAdamW's parameters get instead of a fresh
        .cuda() copy (the same values in another layout, or an in-place update)"""
        for o in (self.ok, self.o32, self.o64):
            for grp, lr in zip(o.param_groups, lrs):
                grp["lr"] = lr
        self.lrmax = [max(a, b) for a, b in zip(self.lrmax, lrs)]
        for i, g in enumerate(grads):
            self.p32[i].grad = None if g is None else g.clone(memory_format=torch.preserve_format)
            self.p64[i].grad = None if g is None else g.double()
            if grad_k is None:
                self.pk[i].grad = None if g is None else g.cuda()
            if g is not None:
                self.gmax[i] = torch.maximum(self.gmax[i], g.double().abs())
        if grad_k is not None:
            grad_k(self.pk, grads)
        self.ok.step(); self.o32.step(); self.o64.step()

    def stepped(self):
        return [i for i, p in enumerate(self.p64) if self.o64.state.get(p)]

    def worst(self):
        """{quantity: (torch f32 worst, kernel worst)} in the units of the module docstring, over all elements"""
        torch.cuda.synchronize()
        out = {k: [0.0, 0.0] for k in ("p",) + KEYS}
        for i in self.stepped():
            lr = self.lrmax[0 if i < self.split else 1]
            st64 = self.o64.state[self.p64[i]]
            ref = {"p": self.p64[i].detach(), **{k: st64[k] for k in KEYS}}
            unit = {"p": 2.0 ** -24 * (ref["p"].abs() + lr), "exp_avg": 2.0 ** -24 * self.gmax[i],
                    "exp_avg_sq": 2.0 ** -24 * ref["exp_avg_sq"] + 2.0 ** -126}
            for col, (p, o) in enumerate(((self.p32[i], self.o32), (self.pk[i], self.ok))):
                got = {"p": p.detach(), **{k: o.state[p][k] for k in KEYS}}
                for q in out:
                    err = (got[q].double().cpu() - ref[q]).abs()
                    ratio = torch.where(unit[q] > 0, err / unit[q], torch.where(err == 0, 0.0, math.inf))
                    out[q][col] = max(out[q][col], float(torch.nan_to_num(ratio, nan=math.inf).max()))
        return out

    def check(self, tag):
        w = self.worst()
        print(f"\n[adamw {tag}] worst error in units, torch f32 / kernel: "
              + "  ".join(f"{q} {a:.2f} / {b:.2f}" for q, (a, b) in w.items()))
        for i in self.stepped():
            assert float(self.ok.state[self.pk[i]]["step"]) == float(self.o64.state[self.p64[i]]["step"])
        for q, (a, b) in w.items():
            assert b <= 2.0 * a, (q, a, b)
        return w


# ------------------------------------------------------------------------------------------------ chunk edges, 12 steps
SHAPES = [(1,), (255,), (256,), (257,), (65535,), (65536,), (65537,), (2 * CHUNK + 123,), (3, 5, 17)]
FROZEN, SPLIT, STEPS = 3, 5, 12          # the frozen parameter is inserted at FROZEN; first SPLIT parameters form group 0
REALLOC_AT = (1, 5, 6, 11)


def _lr(k):
    return (1e-3 * (k + 1) / 4 if k < 4 else 1e-3 * 0.8 ** (k - 3), 1e-2 * (0.5 + 0.5 * math.cos(k)) + 1e-5)


def _edge_inputs():
    gen = torch.Generator().manual_seed(11)
    shapes = SHAPES[:FROZEN] + [(300,)] + SHAPES[FROZEN:]
    p0 = [torch.randn(s, generator=gen) for s in shapes]
    scale = [10.0 ** torch.randint(-12, 8, s, generator=gen).double() for s in shapes]
    alt = [torch.rand(s, generator=gen) + 0.5 for s in shapes]
    for p in p0:
        if p.numel() >= 500:
            p.view(-1)[:100] = 0.0                                    # parameters that start at zero
    grads = []
    for k in range(STEPS):
        gs = []
        for i, s in enumerate(shapes):
            if i == FROZEN:
                gs.append(None)
                continue
            g = (torch.randn(s, generator=gen).double() * scale[i]).float()
            g[torch.rand(s, generator=gen) < 0.2] = 0.0               # exact zeros, at other elements every step
            if g.numel() >= 500:
                f = g.view(-1)
                f[200:300] = 0.0                                      # never a gradient: p only decays, m = v = 0
                f[300:400] = 1e-30                                    # g^2 underflows in f32
                f[400:500] = alt[i].view(-1)[400:500] * (-1.0) ** k   # same magnitude, alternating sign: m cancels
            gs.append(g)
        grads.append(gs)
    return p0, grads


def test_adamw_chunk_edges_and_gradient_classes():
    """Tensor sizes 1, 255, 256, 257 (the thread stride), 65535, 65536, 65537, 2 * 65536 + 123 (the chunk) and a 3-d
    shape in two lr groups, 12 steps with both lrs changed before every step.  Per element, gradient scales 1e-12 ..
    1e7, 20 % exact zeros; in every tensor of 500 elements or more: parameters starting at 0, a block that never gets
    a gradient (p only decays, m and v stay exactly 0), a block of 1e-30 gradients, a block of alternating sign.
    A parameter whose grad is None sits between stepped ones: bit-unchanged, no state; giving it a gradient later
    raises the documented NotImplementedError and changes nothing.  A second FusedAdamW whose gradients are written in
    place (same pointers, table kept) must give bit-identical results to the first, whose gradients are re-allocated
    every step and at steps 1, 5, 6, 11 while the previous tensors are still alive (table rebuilt)."""
    from s3od_amd.optim import FusedAdamW
    p0, grads = _edge_inputs()
    trio = Trio(p0, SPLIT)
    # the in-place twin
    twin = [torch.nn.Parameter(p.cuda()) for p in p0]
    otwin = FusedAdamW(_groups(twin, SPLIT, (1.0, 1.0)), weight_decay=WD, betas=BETAS, eps=EPS)
    keep, tables = [], []
    for k in range(STEPS):
        lrs = _lr(k)
        if k in REALLOC_AT:
            keep.append([p.grad for p in trio.pk])                    # the old gradients stay allocated: new pointers
        trio.step(grads[k], lrs)
        for grp, lr in zip(otwin.param_groups, lrs):
            grp["lr"] = lr
        for p, g in zip(twin, grads[k]):
            if g is not None and p.grad is None:
                p.grad = g.cuda()
            elif g is not None:
                p.grad.copy_(g)
        otwin.step()
        tables.append(otwin._tab["ptrs"].data_ptr())
    assert len(set(tables)) == 1, "gradients updated in place: the pointer table is built once"
    trio.check("edges, 12 steps")
    n_checked = 0
    for i, (a, b) in enumerate(zip(trio.pk, twin)):
        if i == FROZEN:
            continue
        assert torch.equal(a, b), f"tensor {i}: re-allocated and in-place gradients must give the same bits"
        for key in KEYS:
            assert torch.equal(trio.ok.state[a][key], otwin.state[b][key]), (i, key)
        if a.numel() >= 500:
            m, v = (trio.ok.state[a][key].view(-1) for key in KEYS)
            assert int((m[200:300] != 0).sum()) == 0 and int((v[200:300] != 0).sum()) == 0
            decay = p0[i].view(-1)[200:300].double()
            for k in range(STEPS):
                decay = decay * (1.0 - _lr(k)[0 if i < SPLIT else 1] * WD)
            assert torch.equal(trio.p64[i].detach().view(-1)[200:300], decay), "reference: decay only"
            assert int((v[300:400] != 0).sum()) == 0 and int((m[300:400] <= 0).sum()) == 0    # 1e-30^2 underflows
            n_checked += 1
    assert n_checked == 4
    # the parameter without gradient
    fz = trio.pk[FROZEN]
    assert torch.equal(fz.detach().cpu(), p0[FROZEN]) and not trio.ok.state.get(fz)
    before = [p.detach().clone() for p in trio.pk]
    fz.grad = torch.ones_like(fz)
    with pytest.raises(NotImplementedError, match="share step count"):
        trio.ok.step()
    torch.cuda.synchronize()
    assert not trio.ok.state.get(fz)
    for i, (p, b) in enumerate(zip(trio.pk, before)):
        assert torch.equal(p.detach(), b)
        if i != FROZEN:
            assert float(trio.ok.state[p]["step"]) == STEPS


# ------------------------------------------------------------------------------------------------ resume
def test_adamw_resume_at_large_step():
    """load_state_dict of a state with step = 999 (bias corrections 1 - 0.9^1000 and 1 - 0.999^1000 = 0.632) into all
    three optimizers, then 2 steps."""
    gen = torch.Generator().manual_seed(12)
    shapes = [(257,), (CHUNK + 1,), (7, 33)]
    p0 = [torch.randn(s, generator=gen) for s in shapes]
    src = [torch.nn.Parameter(p.clone()) for p in p0]
    osrc = _torch_adamw(_groups(src, 1, (1e-3, 1e-2)))
    for p in src:
        g = torch.randn(p.shape, generator=gen) * 10.0 ** torch.randint(-4, 3, p.shape, generator=gen).float()
        osrc.state[p] = {"step": torch.tensor(999.0), "exp_avg": g * 0.7, "exp_avg_sq": g * g * torch.rand(p.shape, generator=gen)}
    trio = Trio(p0, 1, state=osrc.state_dict())
    for k in range(2):
        grads = [torch.randn(s, generator=gen) * 10.0 ** torch.randint(-4, 3, s, generator=gen).float() for s in shapes]
        trio.step(grads, (1e-3 * (1 - 0.1 * k), 1e-2))
    for p in trio.pk:
        assert float(trio.ok.state[p]["step"]) == 1001.0
    trio.check("resume at step 999, 2 steps")


# ------------------------------------------------------------------------------------------------ layouts
def test_adamw_gradient_layouts():
    """A transposed parameter with a contiguous gradient, and a stride-0 expanded gradient (torch.ones(1).expand(n)
    scaled, which torch lets one assign): FusedAdamW steps on a copy laid out like the parameter, so both match the
    float64 reference like any other tensor.  A contiguous parameter with a contiguous gradient rides along."""
    gen = torch.Generator().manual_seed(13)
    p0 = [torch.randn(70, 300, generator=gen).t(), torch.randn(1000, generator=gen), torch.randn(33, 9, generator=gen)]
    assert p0[0].stride() == (1, 300)
    trio = Trio(p0, 2)
    assert trio.pk[0].stride() == (1, 300) and trio.p32[0].stride() == (1, 300)

    def odd_layouts(pk, grads):
        pk[0].grad = grads[0].contiguous().cuda()                     # contiguous, the parameter is transposed
        pk[1].grad = grads[1][:1].cuda().expand(1000)                 # stride 0, one stored element
        pk[2].grad = grads[2].cuda()
        assert pk[0].grad.stride() == (70, 1) and pk[1].grad.stride() == (0,)

    for k in range(3):
        g1 = (torch.randn(1, generator=gen) * 0.37).expand(1000)
        grads = [torch.randn(300, 70, generator=gen) * 10.0 ** (k - 1), g1, torch.randn(33, 9, generator=gen)]
        trio.step(grads, (1e-3, 1e-2), grad_k=odd_layouts)
    for p in trio.pk:
        for key in KEYS:
            assert trio.ok.state[p][key].stride() == p.stride()
    trio.check("layouts, 3 steps")

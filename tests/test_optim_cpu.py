"""CPU (no kernel launch): the layout guard of FusedAdamW.  s3od_adamw_step walks the parameter, its gradient and
both moments through raw pointers with one flat index, so the four must store element k of the parameter at the same
offset.  FusedAdamW.step checks that on the host before it touches the library: a gradient laid out differently
from its parameter (or with overlapping elements, such as an expanded stride-0 one) is stepped on through a copy
laid out like the parameter, and a parameter that is itself not non-overlapping and dense (or not float32) raises
ValueError.  The library is replaced by a recorder here, so the tests see exactly which pointers would be launched on."""
import pytest
import torch

import s3od_amd.optim as optim
from s3od_amd.optim import FusedAdamW, _flat_compatible_grad, _non_overlapping_and_dense


class _Recorder:
    """stands in for lib(): keeps the arguments of every call (the tables are CPU tensors here)"""
    def __init__(self):
        self.calls = []

    def __call__(self, name, *args):
        self.calls.append((name, args))
        return 0


@pytest.fixture
def rec(monkeypatch):
    r = _Recorder()
    monkeypatch.setattr(optim, "lib", lambda: r)
    monkeypatch.setattr(optim, "stream", lambda: 0)
    return r


def _grad_ptrs(rec):
    name, args = rec.calls[-1]
    assert name == "s3od_adamw_step"
    return [int(v) for v in args[0][:, 1]]


def test_matching_layouts_pass_the_gradient_itself(rec):
    ps = [torch.nn.Parameter(torch.randn(5, 7)), torch.nn.Parameter(torch.randn(7, 5).t()),
          torch.nn.Parameter(torch.randn(1, 6))]
    ps[0].grad = torch.randn(5, 7)
    ps[1].grad = torch.randn(7, 5).t()                           # transposed like its parameter
    ps[2].grad = torch.randn(6, 1).t()                           # differs only in the stride of the size-1 axis
    for p in ps:
        assert _flat_compatible_grad(p) is p.grad
    FusedAdamW(ps, lr=1e-3).step()
    assert _grad_ptrs(rec) == [p.grad.data_ptr() for p in ps]


@pytest.mark.parametrize("case", ["transposed_param", "transposed_grad", "stride0_grad", "strided_grad", "channels_last_param"])
def test_mismatched_gradient_is_stepped_on_through_a_copy(rec, case):
    torch.manual_seed(len(case))
    if case == "transposed_param":
        p, g = torch.randn(7, 5).t(), torch.randn(5, 7)
    elif case == "transposed_grad":
        p, g = torch.randn(5, 7), torch.randn(7, 5).t()
    elif case == "stride0_grad":
        p, g = torch.randn(35), torch.ones(1).expand(35)
    elif case == "strided_grad":
        p, g = torch.randn(5, 7), torch.randn(5, 14)[:, ::2]
    else:
        p, g = torch.randn(2, 8, 3, 3).contiguous(memory_format=torch.channels_last), torch.randn(2, 8, 3, 3)
    p = torch.nn.Parameter(p)
    p.grad = g
    before = p.detach().clone()
    c = _flat_compatible_grad(p)
    assert c is not g and c.data_ptr() != g.data_ptr()
    assert c.stride() == p.stride() and _non_overlapping_and_dense(c) and torch.equal(c, g)
    assert c.untyped_storage().nbytes() >= 4 * p.numel()
    opt = FusedAdamW([p], lr=1e-3)
    opt.step()
    assert len(rec.calls) == 1 and _grad_ptrs(rec) != [g.data_ptr()], "the mismatched gradient's pointer must not be launched on"
    assert p.grad is g and torch.equal(p.detach(), before)       # the user's gradient tensor stays in place
    for k in ("exp_avg", "exp_avg_sq"):
        assert opt.state[p][k].stride() == p.stride()


@pytest.mark.parametrize("case", ["gaps", "overlapping", "bf16"])
def test_unsteppable_parameter_raises_before_the_library(monkeypatch, case):
    def no_lib():
        raise AssertionError("lib() reached")
    monkeypatch.setattr(optim, "lib", no_lib)
    good = torch.nn.Parameter(torch.randn(4))
    good.grad = torch.randn(4)
    if case == "gaps":
        bad = torch.nn.Parameter(torch.randn(4, 8)[:, ::2])
    elif case == "overlapping":
        bad = torch.nn.Parameter(torch.randn(1).expand(4))
    else:
        bad = torch.nn.Parameter(torch.randn(4).bfloat16())
    bad.grad = torch.ones_like(bad)
    opt = FusedAdamW([good, bad], lr=1e-3)
    with pytest.raises(ValueError, match="FusedAdamW"):
        opt.step()
    assert len(opt.state) == 0, "no state may be created (and no step counted) by a refused step"


def test_loaded_state_takes_the_parameters_layout(rec):
    p = torch.nn.Parameter(torch.randn(7, 5).t())
    p.grad = torch.randn(7, 5).t()
    opt = FusedAdamW([p], lr=1e-3)
    m, v = torch.randn(5, 7), torch.rand(5, 7)                   # contiguous: not the parameter's strides
    opt.state[p].update(step=torch.tensor(4.0), exp_avg=m.clone(), exp_avg_sq=v.clone())
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == 5.0
    assert st["exp_avg"].stride() == p.stride() and torch.equal(st["exp_avg"], m) and torch.equal(st["exp_avg_sq"], v)
    name, args = rec.calls[-1]
    assert [int(x) for x in args[0][0]] == [p.data_ptr(), p.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()]

"""CPU: the engine's conv geometry records and its side-stream runner (s3od_amd/engine.py; no GPU, no library load).

The geometry literals are the 11-number prefixes ``B, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad`` of s3od_conv_fwd /
s3od_conv_dgrad / s3od_conv_wgrad, written out by hand from the call sites the engine had before the records (one
layer stated up to three times there), for B = 2 and a NON-square 8 x 10 patch grid (a 128 x 160 image), 3 masks."""
import torch

from s3od_amd.engine import ConvGeom, DPTEngine, SideRunner, decoder_geometry

B, PH, PW, NM = 2, 8, 10, 3
# layer -> {use: prefix}.  A ConvTranspose2d runs forward as the conv view's data gradient (s3od_conv_dgrad) and
# backward as its forward (s3od_conv_fwd) and weight gradient; a conv the other way round.
PREFIX = {
    "rs0": {"fwd s3od_conv_dgrad": (2, 32, 40, 256, 8, 10, 256, 4, 4, 4, 0),       # resize_layers.0, ConvT k4 s4
            "bwd s3od_conv_fwd": (2, 32, 40, 256, 8, 10, 256, 4, 4, 4, 0),
            "bwd s3od_conv_wgrad": (2, 32, 40, 256, 8, 10, 256, 4, 4, 4, 0)},
    "rs1": {"fwd s3od_conv_dgrad": (2, 16, 20, 512, 8, 10, 512, 2, 2, 2, 0),       # resize_layers.1, ConvT k2 s2
            "bwd s3od_conv_fwd": (2, 16, 20, 512, 8, 10, 512, 2, 2, 2, 0),
            "bwd s3od_conv_wgrad": (2, 16, 20, 512, 8, 10, 512, 2, 2, 2, 0)},
    "rs3": {"fwd s3od_conv_fwd": (2, 8, 10, 1024, 4, 5, 1024, 3, 3, 2, 1),         # resize_layers.3, conv k3 s2 p1
            "bwd s3od_conv_dgrad": (2, 8, 10, 1024, 4, 5, 1024, 3, 3, 2, 1),
            "bwd s3od_conv_wgrad": (2, 8, 10, 1024, 4, 5, 1024, 3, 3, 2, 1)},
    "rn1": {"all": (2, 32, 40, 256, 32, 40, 256, 3, 3, 1, 1)},                      # scratch.layer{1..4}_rn
    "rn2": {"all": (2, 16, 20, 512, 16, 20, 256, 3, 3, 1, 1)},
    "rn3": {"all": (2, 8, 10, 1024, 8, 10, 256, 3, 3, 1, 1)},
    "rn4": {"all": (2, 4, 5, 1024, 4, 5, 256, 3, 3, 1, 1)},
    "rcu1": {"all": (2, 32, 40, 256, 32, 40, 256, 3, 3, 1, 1)},                     # both convs of both RCUs of refinenet r
    "rcu2": {"all": (2, 16, 20, 256, 16, 20, 256, 3, 3, 1, 1)},
    "rcu3": {"all": (2, 8, 10, 256, 8, 10, 256, 3, 3, 1, 1)},
    "rcu4": {"all": (2, 4, 5, 256, 4, 5, 256, 3, 3, 1, 1)},
    "oc1": {"all": (2, 64, 80, 256, 64, 80, 128, 3, 3, 1, 1)},                      # mask_head.output_conv1
    "up2x": {"fwd s3od_conv_dgrad": (2, 128, 160, 64, 64, 80, 128, 4, 4, 2, 1),    # mask_head.upsample_2x.0, ConvT k4 s2 p1
             "bwd s3od_conv_fwd": (2, 128, 160, 64, 64, 80, 128, 4, 4, 2, 1),
             "bwd s3od_conv_wgrad": (2, 128, 160, 64, 64, 80, 128, 4, 4, 2, 1)},
    "c64": {"all": (2, 128, 160, 64, 128, 160, 64, 3, 3, 1, 1)},                    # mask_head.upsample_2x.2
    "heads1": {"all": (2, 128, 160, 64, 128, 160, 96, 3, 3, 1, 1)},                 # the fused 3x3 of the 3 mask heads
}


def test_decoder_geometry_nonsquare():
    geo = decoder_geometry(B, PH, PW, NM)
    assert set(geo) == set(PREFIX)
    for name, uses in PREFIX.items():
        for use, want in uses.items():
            assert geo[name].abi == want, (name, use)
        g = geo[name]
        assert len(g.abi) == 11 and g.abi[7] == g.abi[8] == g.k
        # a planted swap of H and W (the mistake square test images cannot see) fails the same comparison
        swapped = g._replace(H=g.W, W=g.H)
        assert all(swapped.abi != want for want in uses.values()), name
    # the two constructors: a conv computes its output grid, a ConvTranspose2d in the module's own terms
    # (IH, IW, Cin_T, Cout_T) is turned into the conv view
    assert ConvGeom.conv(2, 8, 10, 1024, 1024, 3, 2, 1) == geo["rs3"]
    assert ConvGeom.convT(2, 64, 80, 128, 64, 4, 2, 1) == geo["up2x"]
    assert ConvGeom.convT(2, 8, 10, 256, 256, 4, 4, 0).abi[:7] == (2, 32, 40, 256, 8, 10, 256)


class _Stream:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def wait_event(self, e):
        self.log.append(("wait_event", self.name, e.id))

    def wait_stream(self, s):
        self.log.append(("wait_stream", self.name, s.name))


class _Tensor:
    def __init__(self, name, log):
        self.name, self.log = name, log

    def record_stream(self, s):
        self.log.append(("record_stream", self.name, s.name))


def _stub_cuda(monkeypatch):
    """torch.cuda.Event / torch.cuda.stream replaced by stubs that append to a log; returns (log, main, side)."""
    log, current = [], ["main"]

    class Event:
        n = 0

        def __init__(self):
            Event.n += 1
            self.id = Event.n
            log.append(("event", self.id))

        def record(self, s):
            log.append(("record", self.id, s.name))

    class under:
        def __init__(self, s):
            self.s = s

        def __enter__(self):
            current.append(self.s.name)

        def __exit__(self, *a):
            current.pop()

    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(torch.cuda, "stream", under)
    return log, _Stream("main", log), _Stream("side", log), current


def test_side_runner(monkeypatch):
    log, main, side, current = _stub_cuda(monkeypatch)
    fn = lambda: log.append(("fn", current[-1]))     # noqa: E731
    join_main = [("event", 1), ("record", 1, "main"), ("wait_event", "side", 1), ("fn", "side")]
    # ---- side mode, operands as tensors: record on main, side waits, fn under side, then record_stream each tensor
    run = SideRunner(main, side)
    run.run(fn, tensors=(_Tensor("dy", log), _Tensor("x", log)))
    assert log == join_main + [("record_stream", "dy", "side"), ("record_stream", "x", "side")]
    assert current == ["main"]
    # ---- side mode, operands as names of reused buffers: one free-event per name, recorded on side after fn
    del log[:]
    run.run(fn, names=("du", "dhp"))
    assert log == [("event", 2), ("record", 2, "main"), ("wait_event", "side", 2), ("fn", "side"),
                   ("event", 3), ("record", 3, "side"), ("event", 4), ("record", 4, "side")]
    # a later reader of the same name replaces the event: claim waits for exactly the LAST reader's, once
    run.run(fn, names=("du",))
    del log[:]
    run.claim("du")
    assert log == [("wait_event", "main", 6)]
    run.claim("du")            # already claimed
    run.claim("never_read")    # no side-stream reader at all
    assert log == [("wait_event", "main", 6)]
    run.claim("dhp")
    assert log == [("wait_event", "main", 6), ("wait_event", "main", 4)]
    # ---- hook: from the side stream after it has joined main; nothing to protect
    del log[:]
    run.hook(fn)
    assert log == [("event", 7), ("record", 7, "main"), ("wait_event", "side", 7), ("fn", "side")]
    # ---- join: main waits on side
    del log[:]
    run.join()
    assert log == [("wait_stream", "main", "side")]
    # ---- inline mode: the callable runs where it is, no event, no wait, no record_stream
    del log[:]
    inline = SideRunner(main, None)
    inline.run(fn, tensors=(_Tensor("dy", log),))
    inline.run(fn, names=("du",))
    inline.claim("du")
    inline.hook(fn)
    inline.join()
    assert log == [("fn", "main")] * 3


def test_weight_gradients_bound_at_the_call_site():
    """A weight gradient handed to the runner in a loop keeps its own iteration's operands, even if the runner invokes
    it after the loop has moved on."""
    class Deferred:
        def __init__(self):
            self.fns, self.tensors = [], []

        def run(self, fn, tensors=(), names=()):
            self.fns.append(fn)
            self.tensors.append(tensors)

    run, seen = Deferred(), []
    for i in range(3):
        dy, x = f"dy{i}", f"x{i}"
        DPTEngine._side_wgrad(run, lambda *a, **k: seen.append((a, k)), dy, x, i, relu_x=bool(i))
    dy = x = i = None
    for fn in run.fns:
        fn()
    assert seen == [((f"dy{i}", f"x{i}", i), {"relu_x": bool(i)}) for i in range(3)]
    assert run.tensors == [(f"dy{i}", f"x{i}") for i in range(3)]

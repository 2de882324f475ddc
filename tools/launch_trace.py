"""Host-side launch trace of the engine (dev tool): every C-ABI call and every stream operation (Event.record,
Stream.wait_event, Stream.wait_stream, Tensor.record_stream) of an eval forward and of one train step, one line each,
so two revisions of s3od_amd/engine.py can be compared call for call.

    python tools/launch_trace.py OUTDIR            # dinob, B = 2, 128 x 160 (non-square), f32 and bf16
    python tools/launch_trace.py --compare A B     # A = the older revision's OUTDIR, B = the newer one's

Line format.  Library call: the entry name and its arguments -- a device pointer as the ordinal of its first
appearance in the case (t0, t1, ...; the tool keeps every tensor argument alive until the case ends, so the caching
allocator cannot give one address to two tensors and an ordinal means one tensor in both revisions), the stream
argument as main / side, a host pointer as host, a null pointer as null, numbers as they are.  Stream operation: its
kind and the streams involved (``wait_event side<-main``: side waits for an event recorded on main).

Cases: eval forward and one train step (forward + loss + backward; S3OD_BWD_SIDE=1 and =0) per dtype.  OUTDIR also
gets summary.json: lines per case and a SHA-256 of the eval outputs (pred_masks, pred_iou, features) per dtype.

--compare: the traces must be equal line for line; in the S3OD_BWD_SIDE=0 train cases the stream operations whose
streams are all ``main`` (a stream waiting for itself) may be missing from B, and are counted."""
import hashlib
import json
import os
import sys
from pathlib import Path

B, H, W = 2, 128, 160
SELF_OPS = ("event_record main", "wait_event main<-main", "wait_stream main<-main")


def compare(a, b):
    a, b = Path(a), Path(b)
    sa, sb = (json.loads((d / "summary.json").read_text()) for d in (a, b))
    ok = True
    print(f"# launch traces of tools/launch_trace.py (dinob, B = {B}, {H} x {W}): A = {sa['label']}, B = {sb['label']}")
    for case in sa["lines"]:
        la, lb = ((d / f"{case}.txt").read_text().splitlines() for d in (a, b))
        calls = sum(1 for x in la if x.startswith("s3od_"))
        if la == lb:
            verdict = "identical"
        elif case.endswith("side0") and [x for x in la if x not in SELF_OPS] == lb:
            gone = [x for x in la if x in SELF_OPS]
            verdict = "identical but for A's self-waits on main, missing from B: " + ", ".join(
                f"{gone.count(k)} x '{k}'" for k in SELF_OPS if k in gone)
        else:
            ok = False
            first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            verdict = (f"DIFFERENT at line {first}: A '{la[first] if first < len(la) else '<end>'}' "
                       f"B '{lb[first] if first < len(lb) else '<end>'}'")
        print(f"{case}: {calls} library calls, {len(la) - calls} stream operations in A, {len(lb)} lines in B: {verdict}")
    for dt, h in sa["sha256"].items():
        same = h == sb["sha256"][dt]
        again = sa.get("sha256_rerun", {}).get(dt)
        note = "" if again is None else f" (A run twice: {'equal' if again == h else 'NOT equal, so bits are not comparable'})"
        if not same and (again is None or again == h):
            ok = False
        print(f"eval {dt} outputs sha256 {h[:16]}: B {'equal' if same else 'NOT equal ' + sb['sha256'][dt][:16]}{note}")
    return 0 if ok else 1


def main(out):
    import torch
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    from s3od_amd import _lib
    from s3od_amd.model import DPTSegmentation
    from s3od_amd.loss import LossModule, FOCAL_IOU

    out = Path(out)
    out.mkdir(parents=True, exist_ok=True)
    main_st = torch.cuda.current_stream()
    log, keep, ordinal, ev_on, depth = [], [], {}, {}, [0]

    def sname(s):
        return "main" if s.cuda_stream == main_st.cuda_stream else "side"

    def tname(t):
        keep.append(t)
        return f"t{ordinal.setdefault(t.data_ptr(), len(ordinal))}"

    orig_call = _lib._Lib.__call__

    def call(self, name, *args):
        types = self.fns[name][1]
        parts = []
        for i, (a, t) in enumerate(zip(args, types)):
            if not t.endswith("*"):
                parts.append(repr(a))
            elif a is None:
                parts.append("null")
            elif isinstance(a, torch.Tensor):
                parts.append(tname(a))
            elif i == len(types) - 1 and t == "void*":
                parts.append("main" if int(a) == main_st.cuda_stream else "side")
            else:
                parts.append("host")
        log.append(f"{name} " + " ".join(parts))
        return orig_call(self, name, *args)

    def wrap(cls, attr, line):
        orig = getattr(cls, attr)

        def f(self, *a, **k):
            if depth[0] == 0:          # wait_stream is built from record + wait_event: log the outermost only
                log.append(line(self, *a, **k))
            depth[0] += 1
            try:
                return orig(self, *a, **k)
            finally:
                depth[0] -= 1
        setattr(cls, attr, f)

    def rec(e, stream=None):
        keep.append(e)
        ev_on[id(e)] = sname(stream if stream is not None else torch.cuda.current_stream())
        return f"event_record {ev_on[id(e)]}"

    _lib._Lib.__call__ = call
    wrap(torch.cuda.Event, "record", rec)
    wrap(torch.cuda.Stream, "wait_event", lambda s, e: f"wait_event {sname(s)}<-{ev_on.get(id(e), '?')}")
    wrap(torch.cuda.Stream, "wait_stream", lambda s, o: f"wait_stream {sname(s)}<-{sname(o)}")
    wrap(torch.Tensor, "record_stream", lambda t, s: f"record_stream {sname(s)} {tname(t)}")

    def inputs():
        g = torch.Generator(device="cuda").manual_seed(5)
        x = torch.randn(B, 3, H, W, device="cuda", generator=g)
        return x, (torch.rand(B, H, W, device="cuda", generator=g) > 0.5).float()

    def case(name, fn):
        log.clear(); keep.clear(); ordinal.clear(); ev_on.clear()
        r = fn()
        torch.cuda.synchronize()
        (out / f"{name}.txt").write_text("\n".join(log) + "\n")
        lines[name] = len(log)
        print(f"{name}: {len(log)} lines", flush=True)
        return r

    def evaluate(dt):
        torch.manual_seed(0)
        m = DPTSegmentation(compute_dtype=dt).cuda().eval()
        x, _ = inputs()
        with torch.no_grad():
            o = m(x)
        h = hashlib.sha256()
        for k in ("pred_masks", "pred_iou", "features"):
            h.update(o[k].float().contiguous().cpu().numpy().tobytes())
        return h.hexdigest()

    def train(dt, side):
        os.environ["S3OD_BWD_SIDE"] = side
        torch.manual_seed(0)
        m = DPTSegmentation(compute_dtype=dt).cuda().train()
        m._rope_rescale = 1.0
        x, masks = inputs()
        loss, _ = LossModule(FOCAL_IOU, full_mask_lambda=0.1, decay_rate=0.2)(m(x), {"masks": masks}, 0)
        loss.backward()

    lines, sha, sha2 = {}, {}, {}
    for dt in ("f32", "bf16"):
        sha[dt] = case(f"eval_{dt}", lambda: evaluate(dt))
        sha2[dt] = evaluate(dt)
        for side in ("1", "0"):
            case(f"train_{dt}_side{side}", lambda: train(dt, side))
    os.environ.pop("S3OD_BWD_SIDE", None)
    label = os.environ.get("TRACE_LABEL", out.name)
    (out / "summary.json").write_text(json.dumps(dict(label=label, lines=lines, sha256=sha, sha256_rerun=sha2), indent=1) + "\n")
    print(json.dumps(sha))


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:4]))
    main(sys.argv[1])

"""S3OD MI355X benchmark (driver contract: one JSON line on rank 0).

Headline metric (BASELINE.json): "train images/sec (dinob 1024px bf16) at 1/2/4/8 GPU; infer masks/sec 1GPU".
Default workload = configs[2]: synth_sod train model=dinob, 1024x1024, bs=16 per GPU, bf16, forward +
focal_iou loss + backward + fused AdamW (which invalidates and re-packs the kernel-layout weights every
step), synthetic on-device data.  --gpus N runs data-parallel over RCCL, one rank per GPU, per-GPU batch
fixed ("weak" scaling): when the driver already launched the ranks (WORLD_SIZE in the environment) each
rank joins; a bare `python bench.py --gpus N` spawns `torch.distributed.run` itself (a child process,
started before anything touches the GPU) and exits with its status.  --mode infer measures configs[1].

A plain run (`--gpus N --steps K --warmup W`) sets up, warms up, times the K steps and prints the line (with the
`roofline` of the entry assumed to dominate, timed inside the K steps).  `--dump-outputs DIR` then writes arrays as
DIR/<name>.npy (float32) by which two builds can be compared output for output, and leaves the timed steps as they
are.  Images, masks, initial weights and the RoPE rescale draws are seeded.  --mode infer: `pred_masks` (a fixed
sample) and `pred_iou` of the last timed step.  Training: after the timed steps the same step function runs twice more,
untimed, from the seeded initial state: `step1_loss`, `step1_pred_masks` (a fixed sample), `step1_pred_iou`,
`step1_params` (4096 elements of every parameter after the first update) and `step2_loss`.  The timed training steps'
own outputs do not repeat from run to run (see `replay` in main) and are not written.
Everything below that takes a run of its own -- the profiling pass behind `breakdown` (which also picks the roofline
entry), `infer` / `infer_2048` / `c1`, every `cpu_baseline` -- is measured only with `--full`.

`roofline`: the dominant C-ABI entry point of the step (largest summed GPU time in an untimed profiling
pass) is timed live with HIP events on its launch stream around every call inside the timed region;
`achieved` = its ALGORITHMIC work (tools/costs.py, from the call arguments) / that time.
`breakdown`: per-class table (GEMM / attention / memory-bound) from a separate 2-step pass with every
entry timed, plus the whole-step MFMA fraction and the ViT-encoder ("attention block") fraction.
`cpu_baseline`: the oracle (oracle/s3od_oracle.py, the reference's CPU fp32 path restated) on this
host's cores (rank 0, N=1 only): 1 warm-up + --cpu-iters (3) timed iterations of one image (BASELINE.md
"CPU-baseline plan": 1 + >= 3), for the train step and for C2 (the `infer` object); the C5 baseline in
`infer_2048` is one timed 2048^2 image without warm-up (~80 s of CPU per image on the box's share).
`c1`: configs[0], `BackgroundRemoval.remove_background` on the reference's fixture image end to end (host
image in, RemovalResult out) beside the oracle's CPU restatement of the same pipeline (1 + --cpu-iters iterations).
Attention backward work follows SURVEY §8(d) (8*N^2*64 per (b,h), recompute not counted); the roofline
object also carries the executed figure (14*N^2*64) for that entry.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

import torch
import torch.distributed as dist

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

PEAK_BF16 = 2.5e15      # MI355X dense bf16 MFMA (MI355X_MICROARCH.md)
PEAK_F32 = 157.3e12     # f32 MFMA
PEAK_HBM = 8.0e12
TRAIN_TF_PER_IMG = {1024: 6.826e12}                 # SURVEY §8(d) / BASELINE.md (required work)
INFER_TF_PER_IMG = {1024: 2.2768e12, 2048: 15.908e12}
METRIC = "train images/sec (dinob 1024px bf16) at 1/2/4/8 GPU; infer masks/sec 1GPU"


def synthetic_batch(B, S, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    u8 = torch.randint(0, 256, (B, 3, S, S), generator=g, device=dev, dtype=torch.uint8)
    mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 3, 1, 1)
    x = ((u8.float() / 255.0) - mean) / std
    # 1-3 random filled ellipses per image
    yy = torch.arange(S, device=dev).view(1, S, 1).float()
    xx = torch.arange(S, device=dev).view(1, 1, S).float()
    masks = torch.zeros(B, S, S, device=dev)
    r = torch.rand(B, 3, 5, generator=g, device=dev)
    for k in range(3):
        cy, cx = (0.2 + 0.6 * r[:, k, 0]) * S, (0.2 + 0.6 * r[:, k, 1]) * S
        ry, rx = (0.08 + 0.22 * r[:, k, 2]) * S, (0.08 + 0.22 * r[:, k, 3]) * S
        inside = ((yy - cy.view(B, 1, 1)) / ry.view(B, 1, 1)) ** 2 + ((xx - cx.view(B, 1, 1)) / rx.view(B, 1, 1)) ** 2 <= 1
        use = (k == 0) | (r[:, k, 4] > 0.5)
        masks = torch.where(inside & use.view(B, 1, 1), torch.ones_like(masks), masks)
    return x.contiguous(), masks.contiguous()


def log(msg):
    """Progress on stderr (keeps long CPU-baseline phases visibly alive; stdout carries only the JSON line)."""
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


# ------------------------------------------------------------------------------------ CPU baseline
def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_threads():
    """BASELINE.md asks for os.cpu_count() threads; on the shared GPU box that count is the whole
    machine while the job's share is OMP_NUM_THREADS (16), so use the smaller of the two."""
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except AttributeError:
        pass
    omp = os.environ.get("OMP_NUM_THREADS")
    return min(n, int(omp)) if omp and omp.isdigit() and int(omp) > 0 else n


def cpu_baseline(S, mode, iters, warmup=1):
    """Oracle (reference CPU path restated in PyTorch fp32) on one image: `warmup` + `iters` timed."""
    from oracle import s3od_oracle as O
    from s3od_amd.weights import synthetic_state_dict
    threads = cpu_threads()
    torch.set_num_threads(threads)
    sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(0).items()}
    x, masks = synthetic_batch(1, S, 123, "cpu")
    if mode == "train":
        params = {k: v.requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}

        def run():
            for p in params.values():
                p.grad = None
            out = O.forward(x, sd, train=True, rope_rescale=1.0)
            loss, *_ = O.multi_mask_loss(out, masks, 0)
            loss.backward()
    else:
        def run():
            with torch.no_grad():
                O.forward(x, sd)
    for _ in range(warmup):
        log(f"cpu baseline {mode} {S}x{S}: warm-up ({threads} threads)")
        run()
    ts = []
    for it in range(iters):
        t0 = time.perf_counter()
        run()
        ts.append(time.perf_counter() - t0)
        log(f"cpu baseline {mode} {S}x{S}: iteration {it + 1}/{iters} {ts[-1]:.2f} s")
    dt = sum(ts) / len(ts)
    what = "fwd+focal_iou loss+bwd (no optimizer)" if mode == "train" else "eval fwd"
    return {"value": round(1.0 / dt, 5), "unit": "images/s" if mode == "train" else "masks/s", "cores": threads,
            "kind": "port", "cpu_model": _cpu_model(), "os_cpu_count": os.cpu_count(),
            "iter_s": [round(t, 3) for t in ts],
            "sample": f"1 image {S}x{S}, {what}, fp32 oracle (oracle/s3od_oracle.py), {warmup} warm-up + {iters} timed "
                      f"iterations, {threads} threads",
            "deviation": f"the oracle is a restatement, not the reference's executed path: like the GPU engine it skips the "
                         f"encoder layers past the last tap and the final LayerNorm, whose outputs the reference computes and "
                         f"discards ({_skipped_note(S)}); threads = the job's CPU share ({threads}), not os.cpu_count() "
                         f"({os.cpu_count()}) as BASELINE.md:76 says"}


def _skipped_note(S):
    if S == 1024:
        return "2.2768 of the reference's 2.3865 TF per 1024^2 forward, -4.6 %"
    return "layer 11 + final norm of dinob, about 4.6 % of the forward"


# ------------------------------------------------------------------------------------ profiling helpers
def _drain(timers):
    """{name: [(e0, e1, (kind, work), phase)]} -> per-call records (name, ms, kind, work, phase)."""
    torch.cuda.synchronize()
    rec = []
    for name, evs in timers.items():
        for e0, e1, c, ph in evs:
            kind, work = c if c is not None else ("other", 0.0)
            rec.append((name, e0.elapsed_time(e1), kind, work, ph))
    return rec


def breakdown(step, steps, peak):
    from s3od_amd import _lib
    from tools.costs import cost, klass
    lib = _lib.lib()
    lib.cost = cost
    lib.timers = {"*": []}
    for _ in range(steps):
        step()
    timers = lib.timers
    lib.timers = {}
    timers.pop("*", None)
    rec = _drain(timers)
    by_entry, by_class = {}, {}
    for name, ms, kind, work, ph in rec:
        for key, tab in ((name, by_entry), (klass(name), by_class)):
            d = tab.setdefault(key, {"ms": 0.0, "calls": 0, "kind": kind, "work": 0.0})
            d["ms"] += ms; d["calls"] += 1; d["work"] += work
            if kind != "other" and d["kind"] == "other":
                d["kind"] = kind
    tot = sum(d["ms"] for d in by_entry.values())

    def fmt(d):
        o = {"ms_per_step": round(d["ms"] / steps, 3), "pct": round(100 * d["ms"] / tot, 1), "calls_per_step": d["calls"] // steps}
        if d["kind"] == "mfma" and d["ms"] > 0:
            o["TFLOP/s"] = round(d["work"] / d["ms"] / 1e9, 1)
            o["frac_of_peak"] = round(d["work"] / (d["ms"] * 1e-3) / peak, 3)
        elif d["kind"] == "hbm" and d["ms"] > 0 and d["work"] > 0:
            o["GB/s"] = round(d["work"] / d["ms"] / 1e6, 1)
            o["frac_of_hbm"] = round(d["work"] / (d["ms"] * 1e-3) / PEAK_HBM, 3)
        return o
    mf = sum(w for _, _, k, w, _ in rec if k == "mfma")
    enc = [(ms, k, w) for _, ms, k, w, ph in rec if ph == "encoder"]
    enc_ms = sum(ms for ms, _, _ in enc)
    enc_fl = sum(w for ms, k, w in enc if k == "mfma")
    dom = max(by_entry.items(), key=lambda kv: kv[1]["ms"])[0]
    return dom, {
        "steps": steps, "kernel_ms_per_step": round(tot / steps, 3),
        "algorithmic_TF_per_step": round(mf / steps / 1e12, 3),
        "kernel_busy_mfma_frac": round(mf / (tot * 1e-3) / peak, 3),
        "vit_encoder": {"ms_per_step": round(enc_ms / steps, 3), "TF_per_step": round(enc_fl / steps / 1e12, 3),
                        "frac_of_peak": round(enc_fl / (enc_ms * 1e-3) / peak, 3) if enc_ms else None,
                        "note": "A4-A6 (11 ViT layers + patch embed) FLOPs over the time of every kernel the encoder "
                                "launches, memory-bound ones included (north_star 'attention block' target >= 0.40)"},
        "by_class": {k: fmt(v) for k, v in sorted(by_class.items(), key=lambda kv: -kv[1]["ms"])},
        "by_entry": {k: fmt(v) for k, v in sorted(by_entry.items(), key=lambda kv: -kv[1]["ms"])[:16]},
    }


def pmc_traffic(entry):
    """HBM bytes per launch of `entry`'s main kernel from the newest committed rocprofv3 PMC summary
    (profiles/<tag>_pmc.json, written by tools/collect_profiles.py from separate --pmc passes), or None."""
    for f in sorted((ROOT / "profiles").glob("*_pmc.json"), reverse=True):
        try:
            d = json.load(open(f))
        except Exception:
            continue
        if d.get("entry") == entry:
            return {"bytes": d["traffic_bytes_per_launch"], "source": f"profiles/{f.name}", "kernel": d.get("kernel")}
    return None


def infer_rate(model, B, S, steps, warmup, dev, cpu_iters):
    """Eval-forward throughput (configs[1] / configs[4]): one selected mask per image -> masks/s."""
    log(f"inference bs={B} {S}x{S}")
    x, _ = synthetic_batch(B, S, 7, dev)
    was_training = model.training
    model.eval()
    with torch.no_grad():
        for _ in range(warmup):
            model(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            out = model(x)["pred_masks"]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    model.train(was_training)
    ok = bool(torch.isfinite(out).all().item())
    del out, x
    value = B * steps / dt
    res = {"value": round(value, 3), "unit": "masks/s", "ms_per_step": round(dt / steps * 1e3, 3),
           "batch": B, "image_size": S, "steps": steps, "warmup": warmup, "finite": ok,
           "mfma_frac": round(value * INFER_TF_PER_IMG[S] / PEAK_BF16, 4)}
    if cpu_iters > 0:
        try:
            # one 2048^2 image is ~90 s of CPU on the box's 16-thread share: one timed pass, no warm-up
            res["cpu_baseline"] = cpu_baseline(S, "infer", cpu_iters if S <= 1024 else 1, warmup=1 if S <= 1024 else 0)
        except Exception as e:  # reported, never fatal for the GPU number
            res["cpu_baseline"] = {"value": None, "error": repr(e)[:200]}
    return res


def c1_plumbing(dev, cpu_iters, steps=10, warmup=2):
    """configs[0]: BackgroundRemoval.remove_background on the reference's fixture image end to end (PIL image in ->
    RemovalResult out: upload, device letterbox + normalise, eval forward, sigmoid/unpad/antialias resize, the masks'
    copy back, RGBA compose), synthetic weights.  Host round trips included, so this is a plumbing figure, not `value`.
    CPU leg: the oracle's restatement of the same pipeline (oracle/s3od_oracle.py get_pad_info / normalize / forward /
    postprocess = predictor.py:96-139), 1 warm-up + `cpu_iters` timed."""
    from PIL import Image
    from s3od_amd.predictor import BackgroundRemoval
    img = Image.open(Path(__file__).resolve().parent / "tests" / "fixture" / "image.jpg").convert("RGB")
    log(f"C1 remove_background on the fixture ({img.size[0]}x{img.size[1]})")
    br = BackgroundRemoval("synthetic", device=str(dev))
    for _ in range(warmup):
        br.remove_background(img)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        res = br.remove_background(img)
    dt = (time.perf_counter() - t0) / steps
    out = {"value": round(1.0 / dt, 3), "unit": "images/s", "ms_per_call": round(dt * 1e3, 3), "calls": steps,
           "warmup": warmup, "image": f"tests/fixture/image.jpg {img.size[0]}x{img.size[1]}", "dtype": "bf16",
           "best_idx": int(res.all_ious.argmax()),
           "config": "configs[0]: BackgroundRemoval.remove_background(fixture) end to end, host image in / masks out"}
    del br
    if cpu_iters > 0:
        try:
            import numpy as np
            from oracle import s3od_oracle as O
            from s3od_amd.weights import synthetic_state_dict
            threads = cpu_threads()
            torch.set_num_threads(threads)
            sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(0).items()}
            arr = np.array(img)

            def run():
                pad = O.get_pad_info(arr.shape[0], arr.shape[1], 1024)
                assert pad["resized_size"] == arr.shape[:2], "fixture is 1024^2: no resize step"
                x = O.normalize(arr)
                with torch.no_grad():
                    o = O.forward(x, sd)
                return O.postprocess(o["pred_masks"], o["pred_iou"], pad)
            run()
            ts = []
            for it in range(cpu_iters):
                t1 = time.perf_counter()
                run()
                ts.append(time.perf_counter() - t1)
                log(f"cpu baseline C1: iteration {it + 1}/{cpu_iters} {ts[-1]:.2f} s")
            ct = sum(ts) / len(ts)
            out["cpu_baseline"] = {"value": round(1.0 / ct, 5), "unit": "images/s", "cores": threads, "kind": "port",
                                   "iter_s": [round(t, 3) for t in ts],
                                   "sample": f"the fixture through the oracle's remove_background pieces (fp32), 1 warm-up + "
                                             f"{cpu_iters} timed, {threads} threads",
                                   "deviation": f"restatement: skips the encoder layers past the last tap and the final "
                                                f"LayerNorm ({_skipped_note(1024)}); {threads} threads of os.cpu_count() "
                                                f"{os.cpu_count()}"}
        except Exception as e:  # reported, never fatal for the GPU number
            out["cpu_baseline"] = {"value": None, "error": repr(e)[:200]}
    return out


# ------------------------------------------------------------------------------------ output dump
DUMP_MAX_ELEMS = 4 << 20        # per array: 16 MB of float32, the whole dump stays far below 64 MB


def _sample(t, n):
    """`t` flattened when it has at most `n` elements, else a fixed sample of n of them (indices seeded by the size)."""
    t = t.reshape(-1)
    if t.numel() <= n:
        return t.float()
    import numpy as np
    idx = np.sort(np.random.default_rng(t.numel()).integers(0, t.numel(), n))
    return t[torch.from_numpy(idx).to(t.device)].float()


def dump_outputs(path, arrays):
    """--dump-outputs: every array of the last timed step as <path>/<name>.npy, float32."""
    import numpy as np
    path = Path(path)
    path.mkdir(parents=True, exist_ok=True)
    for name, t in arrays.items():
        np.save(path / f"{name}.npy", _sample(t, DUMP_MAX_ELEMS).cpu().numpy().astype(np.float32))
    log(f"wrote {sorted(arrays)} to {path}")


# ------------------------------------------------------------------------------------ launcher
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: run N ranks under torch.distributed.run as a
    child process (no exec, no GPU touched in this process) and return its exit status."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", str(ROOT / "bench.py")] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


def dry_run(args, world, rank, local):
    """`--dry-run`: the rank layout the timed run would use, checked without a GPU — every rank joins a
    gloo group and all-reduces (rank, local rank, per-rank batch); rank 0 prints one JSON line."""
    if world > 1:
        dist.init_process_group("gloo")
    B = args.batch or (16 if args.mode == "train" else 8)
    t = torch.tensor([float(rank), float(local), float(B), 1.0], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t)
    if rank == 0:
        print(json.dumps({"dry_run": True, "world_size": world, "gpus_requested": args.gpus, "rank_sum": int(t[0]),
                          "local_rank_sum": int(t[1]), "global_batch": int(t[2]), "ranks_joined": int(t[3]),
                          "parallelism": f"dp{world}"}), flush=True)
    if world > 1:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mode", choices=["train", "infer"], default="train")
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (default 16 train / 8 infer)")
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--dtype", choices=["bf16", "f32"], default="bf16")
    ap.add_argument("--full", action="store_true",
                    help="also run the secondary measurements: per-class breakdown pass, inference lines (configs[1], "
                         "[4], [0]) and the CPU baselines; the --no-* options below trim a --full run")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the last step's outputs (rank 0) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-iters", type=int, default=3, help="timed CPU-baseline iterations (after 1 warm-up)")
    ap.add_argument("--no-infer", action="store_true", help="skip the secondary inference lines (train mode)")
    ap.add_argument("--no-breakdown", action="store_true", help="skip the per-class profiling pass")
    ap.add_argument("--single-stream", action="store_true",
                    help="profiling only: the whole run with the backward on one stream (S3OD_BWD_SIDE=0), so rocprofv3 "
                         "kernel durations are not stretched by the side-stream weight gradients sharing the CUs")
    ap.add_argument("--ddp", action="store_true",
                    help="use the RCCL data-parallel path even at world size 1 (rehearsal on one GPU)")
    ap.add_argument("--dry-run", action="store_true",
                    help="launch path only: spawn / join the ranks over gloo (no GPU call), rank 0 reports the world")
    args = ap.parse_args()
    if not args.full:
        args.no_cpu_baseline = args.no_infer = args.no_breakdown = True
    if args.single_stream:
        os.environ["S3OD_BWD_SIDE"] = "0"

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus and rank == 0:
        print(f"bench: --gpus {args.gpus} but WORLD_SIZE={world}; using the launcher's world size", file=sys.stderr)
    if args.dry_run:
        return dry_run(args, world, rank, local)
    use_dist = world > 1 or args.ddp
    torch.manual_seed(1000 + rank)      # the train forward draws its RoPE rescale from the CPU generator
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    if use_dist and "RANK" not in os.environ:       # --ddp rehearsal without a launcher: a world of one
        os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    if use_dist:
        dist.init_process_group("nccl", device_id=dev, timeout=__import__("datetime").timedelta(seconds=int(os.environ.get("S3OD_RCCL_TIMEOUT_S", "1800"))))

    from s3od_amd.model import DPTSegmentation
    from s3od_amd.loss import LossModule, FOCAL_IOU
    from s3od_amd.optim import FusedAdamW, reference_param_groups
    from s3od_amd import _lib

    B = args.batch or (16 if args.mode == "train" else 8)
    S = args.size
    model = DPTSegmentation(compute_dtype=args.dtype).to(dev)
    sync = None
    if use_dist:
        from s3od_amd.ddp import GradSync, broadcast_parameters
        broadcast_parameters(model)
        sync = GradSync(model)
    x, masks = synthetic_batch(B, S, 1000 + rank, dev)

    if args.mode == "train":
        model.train()
        crit = LossModule(FOCAL_IOU, full_mask_lambda=0.1, decay_rate=0.2)
        opt = FusedAdamW(reference_param_groups(model, 1e-5), weight_decay=0.05)

        def step(keep=None):
            out = model(x)
            loss, _ = crit(out, {"images": x, "masks": masks}, 0)
            loss.backward()
            opt.step()
            model.zero_grad(set_to_none=False)
            if keep is not None:
                keep.update(loss=loss.detach(), pred_masks=out["pred_masks"].detach(), pred_iou=out["pred_iou"].detach())
            return loss

        def replay(keep):
            """--dump-outputs, after the timed steps: two more (untimed) steps of the same `step` from the seeded initial
            state (weights and BatchNorm statistics regenerated from the seed, AdamW state dropped, RoPE draws reseeded).
            Step 1 gives the forward and the loss on known weights; the weights after its update and the loss of step 2
            carry the backward, the fused AdamW and the re-pack of the kernel-layout weights in float32.
            The outputs of the timed steps themselves cannot serve: the backward accumulates with float atomics, the
            bf16 forward turns the last-bit weight differences into rounding noise on every output one step later, and
            the run on synthetic weights amplifies it -- after 13 steps two runs differ by 6e-3 of the largest logit,
            after 33 steps by a quarter of the logits' rms and 5e-3 of the loss."""
            fresh = DPTSegmentation(compute_dtype=args.dtype).state_dict()
            model.load_state_dict(fresh)
            opt.state.clear()
            torch.manual_seed(2000 + rank)
            first, second = {}, {}
            step(first)
            keep["step1_params"] = torch.cat([_sample(p.detach(), 4096) for _, p in sorted(model.named_parameters())])
            step(second)
            keep.update(step1_loss=first["loss"], step1_pred_masks=first["pred_masks"], step1_pred_iou=first["pred_iou"],
                        step2_loss=second["loss"])
    else:
        model.eval()

        def step(keep=None):
            with torch.no_grad():
                out = model(x)
            if keep is not None:
                keep.update(pred_masks=out["pred_masks"], pred_iou=out["pred_iou"])
            return out["pred_masks"]

    peak = PEAK_BF16 if args.dtype == "bf16" else PEAK_F32
    log(f"{args.mode} bs={B} {S}x{S} {args.dtype}: warm-up")
    for _ in range(args.warmup):
        step()
    # untimed profiling pass: which entry point dominates (and the per-class table)
    bd = None
    dom = "s3od_attn_bwd_qkv" if args.mode == "train" else "s3od_attn_fwd"
    if not args.no_breakdown:
        # per-entry times are measured with the backward on ONE stream: beside the side-stream weight gradients every
        # kernel shares the CUs and its own duration stretches (the timed region below keeps the two streams)
        os.environ["S3OD_BWD_SIDE"] = "0"
        try:
            dom, bd = breakdown(step, 2, peak)
        finally:
            if not args.single_stream:
                os.environ.pop("S3OD_BWD_SIDE", None)
        bd["note"] = ("per-entry GPU times from a separate 2-step pass with the encoder backward on one stream (the timed "
                      "region runs the weight gradients on a side stream beside the data-gradient chain)")
    torch.cuda.synchronize()
    log(f"timed region: {args.steps} steps, roofline entry {dom}")
    from tools.costs import cost
    lib = _lib.lib()
    lib.cost = cost
    lib.timers = {dom: []}
    if sync is not None:
        sync.reset_timing(True)
    if use_dist:
        dist.barrier()
    kept = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        last = step(kept if args.dump_outputs and args.mode == "infer" and i == args.steps - 1 else None)
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    el = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([el], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    timers = lib.timers
    lib.timers = {}
    rec = _drain(timers)
    comm = None
    if sync is not None:
        comm = sync.timing_report()
        sync.reset_timing(False)
        if comm is not None and world > 1:
            t = torch.tensor([comm["comm_exposed_ms"], comm["allreduce_ms_per_step"]], device=dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            comm["comm_exposed_ms_max_over_ranks"], comm["allreduce_ms_per_step_max_over_ranks"] = \
                round(float(t[0]), 3), round(float(t[1]), 3)
    if args.dump_outputs:
        if args.mode == "train":
            kept.clear()
            replay(kept)
        if rank == 0:
            dump_outputs(args.dump_outputs, kept)
        kept.clear()
    kms = sum(r[1] for r in rec) / max(len(rec), 1)
    work = sum(r[3] for r in rec) / max(len(rec), 1)
    kind = rec[0][2] if rec else "mfma"
    ok = bool(torch.isfinite(last.float()).all().item())

    if rank == 0:
        total = B * world * args.steps
        value = total / el
        unit = "images/s" if args.mode == "train" else "masks/s"
        achieved = work / (kms * 1e-3) if kms > 0 else 0.0
        pk = peak if kind == "mfma" else PEAK_HBM
        tr = pmc_traffic(dom) if (B == 16 and S == 1024 and args.dtype == "bf16" and args.mode == "train") else None
        per_img = (TRAIN_TF_PER_IMG if args.mode == "train" else INFER_TF_PER_IMG).get(S)
        res = {
            "metric": METRIC, "value": round(value, 3), "unit": unit, "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(el / args.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": args.dtype,
            "data": "synthetic (seeded uint8 images, ImageNet-normalised; 1-3 ellipse masks), deterministic synthetic weights",
            "config": {"workload": ("synth_sod train model=dinob 1024px bs=16/GPU fwd+focal_iou loss+bwd+AdamW"
                                    if args.mode == "train" else "dinob inference bs=8 1024x1024 eval forward"),
                       "model": "dinob (DINOv3 ViT-B/16 + DPT + 3-mask head)", "global_batch": B * world,
                       "image_size": S, "parallelism": f"dp{world}",
                       "rccl_world_size": dist.get_world_size() if use_dist else 1},
            "roofline": {"entry": dom, "bound": "mfma" if kind == "mfma" else "hbm",
                         "achieved": round(achieved / (1e12 if kind == "mfma" else 1e9), 2),
                         "peak": round(pk / (1e12 if kind == "mfma" else 1e9), 1),
                         "unit": "TFLOP/s" if kind == "mfma" else "GB/s",
                         "frac": round(achieved / pk, 4),
                         "traffic": round(tr["bytes"]) if tr else None,
                         "traffic_unit": "HBM bytes/launch of the entry's main kernel (rocprofv3 FETCH_SIZE*2 + WRITE_SIZE, "
                                         "gfx950-corrected, separate --pmc passes)",
                         "traffic_source": tr["source"] if tr else None,
                         "work_per_launch": work, "mean_launch_ms": round(kms, 4), "launches": len(rec),
                         "note": ("dominant C-ABI entry point by summed GPU time" if bd is not None else
                                  "entry assumed dominant (measured only by the --full breakdown pass)") +
                                 "; HIP events on its launch stream around every call in the timed region; work = "
                                 "algorithmic (tools/costs.py)"},
            "mfma_frac_step": round(value / world * per_img / peak, 4) if per_img else None,
            "finite": ok,
        }
        if bd and dom in bd["by_entry"] and bd["by_entry"][dom].get("calls_per_step"):
            # the same entry in the single-stream breakdown pass: what a single-stream rocprofv3 trace of the step
            # (profiles/<tag>_ss_summary.md) reports for its kernels, without the side stream's CU sharing
            e = bd["by_entry"][dom]
            ms1 = e["ms_per_step"] / e["calls_per_step"]
            res["roofline"]["single_stream"] = {"mean_launch_ms": round(ms1, 4), "frac": e.get("frac_of_peak", e.get("frac_of_hbm")),
                                                "source": "breakdown pass (S3OD_BWD_SIDE=0), HIP events per call"}
        if dom.startswith("s3od_attn_bwd") and kms > 0:
            # what the kernels issue: S recomputed in the dK/dV pass, S and dP again in the dQ pass
            ex = work * 14.0 / 8.0
            res["roofline"]["executed_work_per_launch"] = ex
            res["roofline"]["executed_frac"] = round(ex / (kms * 1e-3) / pk, 4)
        if use_dist:
            res["comm"] = dict(comm or {}, backend=dist.get_backend(),
                               rccl_version=".".join(map(str, torch.cuda.nccl.version())) if hasattr(torch.cuda, "nccl") else None,
                               channels={k: os.environ[k] for k in ("NCCL_MIN_NCHANNELS", "NCCL_MAX_NCHANNELS") if k in os.environ}
                               or "RCCL default (NCCL_MIN/MAX_NCHANNELS unset)",
                               note="HIP events. buckets[].ms: bucket start on the comm stream -> the collective's end "
                                    "(event recorded behind Work.wait() on the comm stream); allreduce_ms_per_step: union of "
                                    "the step's bucket intervals; bus_GBps: 2(N-1)/N x bytes / that union; comm_exposed_ms: "
                                    "the compute stream's wait from backward end to GradSync.finish()'s join, per step")
        if bd is not None:
            res["breakdown"] = bd
        if args.mode == "train" and world == 1 and not args.no_infer and args.dtype == "bf16":
            ci = 0 if args.no_cpu_baseline else args.cpu_iters
            # the metric's second half ("infer masks/sec 1GPU"): configs[1] and configs[4]
            res["infer"] = dict(infer_rate(model, 8, 1024, 10, 3, dev, ci),
                                config="dinob inference bs=8 1024x1024 eval forward (configs[1])")
            res["infer_2048"] = dict(infer_rate(model, 4, 2048, 4, 2, dev, ci),
                                     config="high-res 2048x2048 eval forward bs=4 (configs[4])")
            try:
                res["c1"] = c1_plumbing(dev, ci)
            except Exception as e:  # reported, never fatal for the headline number
                res["c1"] = {"value": None, "error": repr(e)[:200]}
        if not args.no_cpu_baseline and world == 1:
            try:
                res["cpu_baseline"] = cpu_baseline(S, args.mode, args.cpu_iters)
            except Exception as e:  # reported, never fatal for the GPU number
                res["cpu_baseline"] = {"value": None, "error": repr(e)[:200]}
        print(json.dumps(res), flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

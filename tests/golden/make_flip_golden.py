"""Generate tests/golden/flip_scores.npz by running the REFERENCE itself on the CPU (this container only).

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_flip_golden.py

The reference (``/root/reference``, read-only) is imported with stubs for the modules it imports and this stack does
not have (``cv2``, ``tqdm``, ``fire``) and for its predictor module, which none of the code run here touches.  For
every case the reference's ``EvaluationMetrics(device=None, sm_only=True)`` goes through the three steps of
``eval_sample`` (mine_samples.py:34-51) on fresh copies of the tensors, in its order and with its dtypes (float32 soft
masks, float64 ground truth), so step 1's in-place binarisation of the ground truth carries into step 2; the
reference's ``calculate_iou`` (filter_dataset.py:398-427) gives the three IoUs.  ``calculate_new_samples`` and
``analyze_stability`` are recorded for a table of category scores.

The output is DATA: inputs + reference outputs.  Nothing under /root/reference is copied.
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference")


def _install_shims():
    sys.modules["cv2"] = types.ModuleType("cv2")
    tq = types.ModuleType("tqdm")
    tq.tqdm = lambda it, *a, **k: it
    sys.modules["tqdm"] = tq
    fire = types.ModuleType("fire")
    fire.Fire = lambda fn: None
    sys.modules["fire"] = fire
    pred = types.ModuleType("synth_sod.model_training.predictor")
    pred.SODPredictor = type("SODPredictor", (), {})
    sys.modules["synth_sod.model_training.predictor"] = pred
    sys.path.insert(0, str(REF / "synth_sod" / "src"))


def blob(H, W, cy, cx, ry, rx):
    yy, xx = np.mgrid[:H, :W]
    return (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1).astype(np.float32)


def pred_of(g, r, keep):
    """A soft prediction of the binary plane g: keep * g + (1 - keep) * noise, float32 in [0, 1].  keep < 0.5 lets
    both thresholds cut into either side; the noise has 256 levels so that the file compresses."""
    return np.clip(keep * g + (1 - keep) * r.integers(0, 256, g.shape) / 255.0, 0, 1).astype(np.float32)


def flip_cases(seed=23):
    """(name, a, bm, gt): float32 [H, W]; bm is the prediction of the mirrored image, still mirrored."""
    r = np.random.default_rng(seed)

    def pair(g):
        return pred_of(g, r, 0.45), np.ascontiguousarray(pred_of(g, r, 0.4)[:, ::-1])

    cases = []
    g = blob(33, 47, 15, 20, 9, 12)
    cases.append(("soft_gt_33x47", *pair(g), (0.9 * g + 0.05).astype(np.float32)))
    g = blob(40, 52, 20, 26, 11, 15)
    cases.append(("gt_const_0p2_40x52", *pair(g), np.full((40, 52), 0.2, np.float32)))
    cases.append(("gt_const_0p7_40x52", *pair(g), np.full((40, 52), 0.7, np.float32)))
    cases.append(("gt_zero_40x52", *pair(g), np.zeros((40, 52), np.float32)))
    a, _ = pair(g)
    cases.append(("bm_zero_40x52", a, np.zeros((40, 52), np.float32), g))
    cases.append(("bm_one_40x52", a, np.ones((40, 52), np.float32), g))
    bm = (0.4 * r.random((40, 52))).astype(np.float32)
    bm[17, 9] = 0.9
    cases.append(("bm_single_px_40x52", a, bm, g))
    g1 = np.zeros((33, 47), np.float32)
    g1[12, 0] = 1.0
    cases.append(("gt_px_col0_33x47", *pair(blob(33, 47, 12, 3, 5, 6)), g1))
    g = np.array([[1, 0], [0, 0]], np.float32)
    cases.append(("tiny_2x2", *pair(g), g))
    g = blob(65, 63, 30, 31, 20, 14)
    cases.append(("odd_65x63", *pair(g), g))
    g = np.maximum(blob(256, 300, 120, 140, 70, 50), blob(256, 300, 200, 60, 20, 30))
    cases.append(("two_blobs_256x300", *pair(g), g))
    return cases


def gen_cases(out):
    from synth_sod.model_training.metrics import EvaluationMetrics
    from synth_sod.data_generation.filter_dataset import calculate_iou
    names = []
    for name, a, bm, gt in flip_cases():
        b = np.ascontiguousarray(bm[:, ::-1])
        ta, tb = torch.tensor(a.copy()), torch.tensor(b.copy())
        tg = torch.tensor(gt.astype(np.float64))
        mc = EvaluationMetrics(device=None, sm_only=True)
        s = []
        for pred, mask in ((ta, tg), (tb, tg), (ta, tb)):        # eval_sample's order, the same tensors throughout
            mc.step(pred, mask)
            s.append(float(mc.compute_metrics()["Sm"]))
            mc.reset()
        s_orig, s_flip, s_cons = s
        cons = (s_orig + s_flip) / 2 if np.isnan(s_cons) else s_cons
        score = (s_orig + s_flip) * cons / 2
        ious = [calculate_iou(a, gt), calculate_iou(b, gt), calculate_iou(a, b)]
        out[f"{name}/a"], out[f"{name}/bm"], out[f"{name}/gt"] = a, bm, gt
        out[f"{name}/s"] = np.array([s_orig, s_flip, s_cons, score], np.float64)
        out[f"{name}/iou"] = np.array(ious, np.float64)
        names.append(name)
        print(name, out[f"{name}/s"], out[f"{name}/iou"])
    out["names"] = np.array(names)


def gen_table(out):
    import synth_sod.model_training.mine_samples as M
    scores = [0.0, 0.31, 0.5, 0.642, 0.79, 0.7999, 0.8, 0.8001, 0.83, 0.86, 0.875, 0.9, 0.93, 0.9499, 0.95, 0.9501,
              0.97, 0.99, 1.0, 0.7212, 0.9123]
    cats = {f"cat_{i:02d}": s for i, s in enumerate(scores)}
    out["table/names"] = np.array(list(cats))
    out["table/scores"] = np.array(scores, np.float64)
    for lo, hi in ((10, 50), (20, 100)):
        ns = M.calculate_new_samples(cats, lo, hi)
        out[f"table/new_samples_{lo}_{hi}"] = np.array([ns[c] for c in cats], np.int64)
    out["table/new_samples_default"] = np.array([M.calculate_new_samples(cats)[c] for c in cats], np.int64)
    for n in (15, 5):
        unstable, stable = M.analyze_stability(cats, n) if n != 15 else M.analyze_stability(cats)
        out[f"table/unstable_{n}"] = np.array(unstable)
        out[f"table/stable_{n}"] = np.array(stable)


def main():
    _install_shims()
    out = {}
    gen_cases(out)
    gen_table(out)
    np.savez_compressed(HERE / "flip_scores.npz", **out)
    print("wrote", HERE / "flip_scores.npz", (HERE / "flip_scores.npz").stat().st_size, "bytes")


if __name__ == "__main__":
    main()

"""Hard-sample mining — drop-in for ``synth_sod/src/synth_sod/model_training/mine_samples.py``: score every
validation image by how well the model predicts it and its horizontal mirror and how well the two predictions agree,
average per category, and turn the averages into "generate this many new samples per category".

The per-image score is ``FlipScorer`` (``flip_scores.py``): one upload, the mirror made on the device, both images in
one forward and one fused scoring pass, where the reference runs two batch-1 predictions, mirrors on the host and
takes three ``EvaluationMetrics`` steps.  ``metric_counter`` is accepted for the reference's signatures and unused.

Differences from the reference:
  * ``eval_category`` evaluates every sample once.  The reference evaluates it twice (mine_samples.py:71 for the NaN
    test and :75 for the value it keeps); the model is deterministic, so both give the same number.
  * ``eval_category`` goes through ``FlipScorer.score_many`` (several images per forward).
  * images are decoded with PIL, masks with ``metrics.read_gray_u8`` (cv2 is not part of this stack);
  * ``fire`` is not part of this stack either: the command line is argparse with the same parameter names,
    ``python -m synth_sod.model_training.mine_samples --input_dir D --model_path M [--img_size 1024] ...``.
"""
from __future__ import annotations

import argparse
import datetime
import json
import os
from collections import defaultdict
from typing import Dict, List, Tuple

import numpy as np

from .flip_scores import FlipScorer
from .metrics import read_gray_u8

BATCH_SIZE = 4      # images per forward in eval_category (8 canvases)


def _scorer(predictor) -> FlipScorer:
    sc = getattr(predictor, "_flip_scorer", None)
    if sc is None or sc.predictor is not predictor:
        sc = FlipScorer(predictor)
        predictor._flip_scorer = sc
    return sc


def eval_sample(predictor, image: np.ndarray, gt_mask: np.ndarray, metric_counter=None) -> float:
    """Evaluate single image with flips and consistency: (s_orig + s_flip) * s_cons / 2, where a NaN s_cons is
    replaced by the mean of the other two (mine_samples.py:16-51)."""
    return _scorer(predictor).score(image, gt_mask).score


def _load_pair(image_path: str):
    from PIL import Image
    image = np.asarray(Image.open(image_path).convert("RGB"))
    gt_mask = read_gray_u8(image_path.replace("images", "masks").replace(".jpg", ".png")) / 255.0
    return image, gt_mask


def eval_category(predictor, category_images: List[str], metric_counter=None) -> Tuple[float, List[float]]:
    """Evaluate category and return mean score and per-sample scores.  A NaN-score sample is reported and skipped;
    a category whose samples were all skipped has the mean ``np.mean([])`` = NaN."""
    scores = []
    sc = _scorer(predictor)
    for i in range(0, len(category_images), BATCH_SIZE):
        paths = category_images[i:i + BATCH_SIZE]
        pairs = [_load_pair(p) for p in paths]
        res = sc.score_many([im for im, _ in pairs], [gt for _, gt in pairs], batch_size=BATCH_SIZE)
        for image_path, r in zip(paths, res):
            if np.isnan(r.score):
                print(f"NaN score for {image_path}")
                continue
            scores.append(r.score)
    return np.mean(scores), scores


def calculate_new_samples(category_scores: Dict[str, float], min_samples: int = 10, max_samples: int = 50,
                          high_threshold: float = 0.95, low_threshold: float = 0.8) -> Dict[str, int]:
    """Number of new samples per category: a difficulty in [0.1, 1] from the score (0.1 at or above
    ``high_threshold``, 0.7 rising to 1 at or below ``low_threshold``, linear between), squashed by a logistic
    of slope 8 about 0.5 and mapped onto [min_samples, max_samples] (mine_samples.py:79-113)."""
    names = list(category_scores.keys())
    scores = np.array([category_scores[k] for k in names])
    difficulties = np.zeros_like(scores)
    for i, s in enumerate(scores):
        if s >= high_threshold:
            difficulties[i] = 0.1
        elif s <= low_threshold:
            difficulties[i] = 0.7 + 0.3 * (low_threshold - s) / low_threshold
        else:
            difficulties[i] = 0.1 + 0.6 * (high_threshold - s) / (high_threshold - low_threshold)
    scaled = 1 / (1 + np.exp(-8 * (difficulties - 0.5)))
    samples = min_samples + (max_samples - min_samples) * scaled
    return {cat: int(round(n)) for cat, n in zip(names, samples)}


def analyze_stability(scores: Dict[str, float], n_categories: int = 15) -> Tuple[List[str], List[str]]:
    """The ``n_categories`` lowest-scoring and the ``n_categories`` highest-scoring categories, each in
    ascending score order (mine_samples.py:116-124)."""
    ordered = [cat for cat, _ in sorted(scores.items(), key=lambda kv: kv[1])]
    return ordered[:n_categories], ordered[-n_categories:]


def save_results(results: dict, output_dir: str, prefix: str = ""):
    """Save evaluation results to ``<prefix>_eval_results_<timestamp>.json`` (mine_samples.py:127-152)."""
    timestamp = datetime.datetime.now().strftime("%Y%m%d_%H%M%S")
    output_path = os.path.join(output_dir, f"{prefix}_eval_results_{timestamp}.json")
    clean = {
        "category_scores": {k: float(v) for k, v in results["category_scores"].items()},
        "new_samples": results["new_samples"],
        "category_sample_scores": {k: [float(s) for s in v] for k, v in results["category_sample_scores"].items()},
        "stable_categories": results["stable_categories"],
        "unstable_categories": results["unstable_categories"],
    }
    os.makedirs(output_dir, exist_ok=True)
    with open(output_path, "w") as f:
        json.dump(clean, f, indent=4)
    print(f"Results saved to: {output_path}")
    return output_path


def main(input_dir: str, model_path, img_size: int = 1024, min_samples: int = 20, max_samples: int = 100,
         max_val_samples: int = 10, output_dir: str = "results"):
    from .sod_predictor import SODPredictor
    predictor = SODPredictor(model_path, img_size, device="cuda")

    splits_file = os.path.join(input_dir, "data_splits.json")
    if os.path.exists(splits_file):
        with open(splits_file, "r") as f:
            image_files = json.load(f)["val"]
    else:
        image_files = [f for f in os.listdir(os.path.join(input_dir, "images")) if f.endswith((".jpg", ".png"))]

    categories = defaultdict(list)
    for image_file in image_files:
        categories[image_file.rsplit("_", 1)[0]].append(os.path.join(input_dir, "images", image_file))

    category_scores, category_sample_scores = {}, {}
    for category, images in categories.items():
        eval_images = images[:max_val_samples] if max_val_samples else images
        category_scores[category], category_sample_scores[category] = eval_category(predictor, eval_images)

    new_samples = calculate_new_samples(category_scores, min_samples, max_samples)
    unstable_cats, stable_cats = analyze_stability(category_scores)

    print("\nResults:")
    print("\nMost Stable Categories:")
    for cat in stable_cats:
        print(f"{cat}: score={category_scores[cat]:.4f}, new_samples={new_samples[cat]}")
    print("\nLeast Stable Categories:")
    for cat in unstable_cats:
        print(f"{cat}: score={category_scores[cat]:.4f}, new_samples={new_samples[cat]}")

    save_results({"category_scores": category_scores, "new_samples": new_samples,
                  "category_sample_scores": category_sample_scores, "stable_categories": stable_cats,
                  "unstable_categories": unstable_cats}, output_dir)


def cli(argv=None):
    ap = argparse.ArgumentParser(description="Hard-sample mining: per-category flip-consistency scores -> new samples per category")
    ap.add_argument("--input_dir", required=True)
    ap.add_argument("--model_path", required=True)
    ap.add_argument("--img_size", type=int, default=1024)
    ap.add_argument("--min_samples", type=int, default=20)
    ap.add_argument("--max_samples", type=int, default=100)
    ap.add_argument("--max_val_samples", type=int, default=10)
    ap.add_argument("--output_dir", default="results")
    main(**vars(ap.parse_args(argv)))


if __name__ == "__main__":
    cli()

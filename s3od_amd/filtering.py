"""Dataset filtering — drop-in for the small framework of
``synth_sod/src/synth_sod/data_generation/filter_dataset.py`` (``Sample``, ``FilterResult``, ``BaseFilter``,
``DatasetLoader``, ``DatasetFilter``, ``calculate_iou``) and for the flip-consistency filter built on it,
``synth_sod/src/synth_sod/data_generation/filters/consistency_filter.py``.

``HorizontalFlipConsistencyFilter`` predicts a sample's image and its horizontal mirror, compares both binary masks
with the generated mask and with each other, and passes the sample when the two IoUs with the generated mask reach
``threshold`` and the IoU between the two predictions reaches ``consistency_threshold``.  The three IoUs come from
``FlipScorer`` (``flip_scores.py``): one upload, the mirror made on the device, one forward for both, one scoring
pass; the masks never reach the host.

Differences from the reference:
  * its filter ends in ``FilterResult(passes=...)``, a field that does not exist, so ``filter`` raises ``TypeError``
    as written; this one sets ``passed``;
  * ``save_fail_cases`` is accepted and recorded in the statistics, but the fail-case collage is not drawn;
  * pure-Python parts use numpy and PIL only.
"""
from __future__ import annotations

import logging
import shutil
from abc import ABC, abstractmethod
from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
from PIL import Image


@dataclass
class Sample:
    """One image-mask pair of a ``<class>/images/<id>.jpg`` + ``<class>/masks/<id>.png`` dataset."""
    image_path: Path
    mask_path: Path
    class_name: str
    sample_id: str

    def load_image(self) -> np.ndarray:
        """RGB uint8 [H, W, 3]."""
        return np.array(Image.open(self.image_path).convert("RGB"))

    def load_mask(self, binary: bool = True) -> np.ndarray:
        """The grey mask [H, W]: uint8 {0, 1} (``> 128``) when ``binary``, else the 8-bit values."""
        grey = np.array(Image.open(self.mask_path).convert("L"))
        return (grey > 128).astype(np.uint8) if binary else grey

    def get_relative_path(self) -> str:
        return f"{self.class_name}/images/{self.sample_id}.jpg"

    def get_mask_relative_path(self) -> str:
        return f"{self.class_name}/masks/{self.sample_id}.png"


@dataclass
class FilterResult:
    passed: bool
    reason: Optional[str] = None
    score: Optional[float] = None
    metadata: Optional[Dict[str, Any]] = None


class BaseFilter(ABC):
    """A named filter with pass / fail counters."""

    def __init__(self, name: str):
        self.name = name
        self.reset_stats()

    @abstractmethod
    def filter(self, sample: Sample) -> FilterResult:
        """Decide one sample."""

    def update_stats(self, result: FilterResult):
        self.stats["total_processed"] += 1
        self.stats["passed" if result.passed else "failed"] += 1

    def get_pass_rate(self) -> float:
        n = self.stats["total_processed"]
        return self.stats["passed"] / n if n else 0.0

    def reset_stats(self):
        self.stats = {"total_processed": 0, "passed": 0, "failed": 0}


class DatasetLoader:
    """Finds the image-mask pairs under ``dataset_path/<class>/{images,masks}``."""

    def __init__(self, dataset_path: str):
        self.dataset_path = Path(dataset_path)

    def load_samples(self) -> List[Sample]:
        samples = []
        for class_dir in self.dataset_path.iterdir():
            if not class_dir.is_dir():
                continue
            images_dir, masks_dir = class_dir / "images", class_dir / "masks"
            if not (images_dir.exists() and masks_dir.exists()):
                logging.warning(f"Skipping {class_dir.name}: missing images or masks directory")
                continue
            for image_path in images_dir.glob("*.jpg"):
                mask_path = masks_dir / f"{image_path.stem}.png"
                if not mask_path.exists():
                    logging.warning(f"Missing mask for {image_path}")
                    continue
                samples.append(Sample(image_path=image_path, mask_path=mask_path, class_name=class_dir.name,
                                      sample_id=image_path.stem))
        logging.info(f"Loaded {len(samples)} samples from {len(set(s.class_name for s in samples))} classes")
        return samples


class DatasetFilter:
    """Runs a list of filters over a dataset; a sample is dropped at the first filter it fails."""

    def __init__(self, filters: List[BaseFilter]):
        self.filters = filters
        self.global_stats = {"total_samples": 0, "passed_samples": 0, "failed_samples": 0, "filter_breakdown": {}}

    def filter_sample(self, sample: Sample) -> Tuple[bool, Dict[str, FilterResult]]:
        results = {}
        for f in self.filters:
            result = f.filter(sample)
            f.update_stats(result)
            results[f.name] = result
            if not result.passed:
                return False, results
        return True, results

    def filter_dataset(self, input_path: str, output_path: str, max_samples_per_class: Optional[int] = None,
                       save_fail_cases: bool = True) -> Dict[str, Any]:
        """Filter the dataset at ``input_path`` and copy the passing samples into the flat layout
        ``output_path/images/<class>_<id>.jpg`` + ``output_path/masks/<class>_<id>.png`` -> the statistics dict."""
        samples = DatasetLoader(input_path).load_samples()
        output_dir = Path(output_path)
        output_dir.mkdir(parents=True, exist_ok=True)
        by_class: Dict[str, List[Sample]] = {}
        for s in samples:
            by_class.setdefault(s.class_name, []).append(s)

        totals = {"processed": 0, "passed": 0, "failed": 0}
        class_stats = {}
        for class_name, class_samples in by_class.items():
            logging.info(f"Filtering class: {class_name} ({len(class_samples)} samples)")
            if max_samples_per_class:
                class_samples = class_samples[:max_samples_per_class]
            n_pass = 0
            for sample in class_samples:
                passed, results = self.filter_sample(sample)
                if passed:
                    self._copy_sample(sample, output_dir)
                    n_pass += 1
                    logging.debug(f"Passed: {sample.image_path.name}")
                else:
                    failed = next(name for name, r in results.items() if not r.passed)
                    logging.debug(f"Failed ({failed}): {sample.image_path.name} - {results[failed].reason or 'Unknown'}")
            n = len(class_samples)
            class_stats[class_name] = {"processed": n, "passed": n_pass, "failed": n - n_pass,
                                       "pass_rate": n_pass / n if n > 0 else 0.0}
            totals["processed"] += n
            totals["passed"] += n_pass
            totals["failed"] += n - n_pass

        self.global_stats.update({
            "total_samples": totals["processed"], "passed_samples": totals["passed"], "failed_samples": totals["failed"],
            "overall_pass_rate": totals["passed"] / totals["processed"] if totals["processed"] > 0 else 0.0,
            "class_stats": class_stats, "filter_breakdown": {f.name: f.stats for f in self.filters},
            "save_fail_cases": save_fail_cases})
        return self.global_stats

    def _copy_sample(self, sample: Sample, output_dir: Path):
        flat = f"{sample.class_name}_{sample.sample_id}"
        for sub, src, ext in (("images", sample.image_path, ".jpg"), ("masks", sample.mask_path, ".png")):
            (output_dir / sub).mkdir(parents=True, exist_ok=True)
            shutil.copy2(src, output_dir / sub / f"{flat}{ext}")

    def print_statistics(self):
        g = self.global_stats
        print("\n" + "=" * 60)
        print("DATASET FILTERING STATISTICS")
        print("=" * 60)
        print("Overall Results:")
        print(f"  Total Samples: {g['total_samples']}")
        print(f"  Passed: {g['passed_samples']}")
        print(f"  Failed: {g['failed_samples']}")
        print(f"  Pass Rate: {g.get('overall_pass_rate', 0.0):.2%}")
        print("\nPer-Filter Breakdown:")
        for name, st in g.get("filter_breakdown", {}).items():
            rate = st["passed"] / st["total_processed"] if st["total_processed"] > 0 else 0.0
            print(f"  {name}: {rate:.2%} pass rate ({st['passed']}/{st['total_processed']})")
        print("\nPer-Class Results:")
        for name, st in g.get("class_stats", {}).items():
            print(f"  {name}: {st['pass_rate']:.2%} ({st['passed']}/{st['processed']}) | Failed: {st.get('failed', 0)}")


def calculate_iou(mask1: np.ndarray, mask2: np.ndarray, threshold: float = 0.5) -> float:
    """IoU of two masks: boolean masks as they are, others binarised at ``> threshold``; arrays of more than two
    dimensions are squeezed; an empty union gives 1.0."""
    def binary(m):
        m = np.asarray(m)
        if m.ndim > 2:
            m = m.squeeze()
        return m if m.dtype == bool else m > threshold
    b1, b2 = binary(mask1), binary(mask2)
    union = np.logical_or(b1, b2).sum()
    if union == 0:
        return 1.0
    return float(np.logical_and(b1, b2).sum() / union)


class HorizontalFlipConsistencyFilter(BaseFilter):
    """Passes a sample when the model's masks of the image and of its horizontal mirror both match the generated
    mask (IoU >= ``threshold``) and each other (IoU >= ``consistency_threshold``).  ``model_path`` is a checkpoint
    path (loaded on first use) or a ready ``SODPredictor``."""

    def __init__(self, model_path, name: str = "horizontal_flip_consistency", threshold: float = 0.7,
                 consistency_threshold: float = 0.8, device: str = "cuda"):
        super().__init__(name)
        self.threshold = threshold
        self.consistency_threshold = consistency_threshold
        self.device = device
        self.model_path = model_path
        self.model = None
        self._model_loaded = False
        self._scorer = None

    def _load_model(self):
        if self._model_loaded:
            return
        if hasattr(self.model_path, "predict") and hasattr(self.model_path, "_geometry"):
            self.model = self.model_path
        else:
            from .sod_predictor import SODPredictor
            self.model = SODPredictor(checkpoint_path=self.model_path, device=self.device)
            logging.info(f"Loaded consistency model from {self.model_path}")
        self._model_loaded = True

    def filter(self, sample: Sample) -> FilterResult:
        from .flip_scores import FlipScorer
        self._load_model()
        if self._scorer is None or self._scorer.predictor is not self.model:
            self._scorer = FlipScorer(self.model, threshold=0.5)      # predict()'s binary_mask threshold
        r = self._scorer.score(sample.load_image(), sample.load_mask())
        avg_iou = (r.iou_orig_gt + r.iou_flip_gt) / 2
        passed = bool(r.iou_orig_gt >= self.threshold and r.iou_flip_gt >= self.threshold
                      and r.iou_orig_flip >= self.consistency_threshold)
        metadata = {"iou_orig_generated": r.iou_orig_gt, "iou_flipped_generated": r.iou_flip_gt,
                    "iou_orig_flipped": r.iou_orig_flip, "avg_iou": avg_iou}
        return FilterResult(passed=passed, score=avg_iou, metadata=metadata)

    def calculate_iou(self, mask1: np.ndarray, mask2: np.ndarray) -> float:
        """IoU of two masks binarised at ``> 0.5`` (the reference filter's own helper)."""
        return calculate_iou(np.asarray(mask1) > 0.5, np.asarray(mask2) > 0.5)

"""CPU-side checks of the mining and filtering surfaces (s3od_amd/mining.py, s3od_amd/filtering.py and their
synth_sod aliases): the sample-count rule and the stability lists against the reference golden, calculate_iou, the
filter framework's records and counters, the save_results layout and the FlipScores arithmetic.  No GPU."""
import json
import math

import numpy as np
import pytest
from PIL import Image

from conftest import GOLDEN


@pytest.fixture(scope="module")
def table():
    g = np.load(GOLDEN / "flip_scores.npz")
    names = [str(n) for n in g["table/names"]]
    return g, names, dict(zip(names, (float(s) for s in g["table/scores"])))


def test_calculate_new_samples_golden(table):
    from s3od_amd.mining import calculate_new_samples
    g, names, cats = table
    assert len(names) >= 20
    for lo, hi in ((10, 50), (20, 100)):
        got = calculate_new_samples(cats, lo, hi)
        assert list(got) == names
        assert [got[c] for c in names] == list(g[f"table/new_samples_{lo}_{hi}"]), (lo, hi)
        assert all(isinstance(v, int) for v in got.values())
    assert [calculate_new_samples(cats)[c] for c in names] == list(g["table/new_samples_default"])
    assert list(g["table/new_samples_default"]) == list(g["table/new_samples_10_50"])


def test_analyze_stability_golden(table):
    from s3od_amd.mining import analyze_stability
    g, names, cats = table
    unstable, stable = analyze_stability(cats)
    assert unstable == [str(n) for n in g["table/unstable_15"]] and stable == [str(n) for n in g["table/stable_15"]]
    unstable, stable = analyze_stability(cats, 5)
    assert unstable == [str(n) for n in g["table/unstable_5"]] and stable == [str(n) for n in g["table/stable_5"]]


def test_calculate_iou():
    from s3od_amd.filtering import calculate_iou
    a = np.array([[0.9, 0.6, 0.1], [0.5, 0.0, 0.7]], np.float32)
    b = np.array([[1, 0, 0], [1, 0, 1]], np.uint8)
    # a > 0.5: [[1,1,0],[0,0,1]]; b > 0.5: [[1,0,0],[1,0,1]] -> intersection 2, union 4
    assert calculate_iou(a, b) == 0.5
    assert calculate_iou(a > 0.5, b.astype(bool)) == 0.5
    assert calculate_iou(a, b.astype(bool)) == 0.5
    assert calculate_iou(a[None], b[..., None]) == 0.5                      # 3-D inputs are squeezed
    assert calculate_iou(a, b, threshold=0.8) == 1.0 / 3.0                  # a > 0.8: one pixel, b > 0.8: three
    assert calculate_iou(np.zeros((3, 3)), np.zeros((3, 3), bool)) == 1.0   # empty union
    assert isinstance(calculate_iou(a, b), float)


def _dataset(root):
    for cls, ids in (("apple", ("0", "1")), ("pear", ("7",))):
        (root / cls / "images").mkdir(parents=True)
        (root / cls / "masks").mkdir(parents=True)
        for i in ids:
            Image.fromarray(np.full((6, 8, 3), 20 * int(i) + 10, np.uint8)).save(root / cls / "images" / f"{i}.jpg")
            m = np.zeros((6, 8), np.uint8)
            m[1:4, 2:5] = 255
            m[5, 7] = 128                                                     # not > 128: background
            Image.fromarray(m).save(root / cls / "masks" / f"{i}.png")
    Image.fromarray(np.zeros((4, 4, 3), np.uint8)).save(root / "pear" / "images" / "nomask.jpg")
    (root / "empty_class").mkdir()
    (root / "readme.txt").write_text("not a class")


def test_sample_loader_filter_framework(tmp_path):
    from s3od_amd.filtering import BaseFilter, DatasetFilter, DatasetLoader, FilterResult, Sample
    _dataset(tmp_path / "in")
    samples = sorted(DatasetLoader(str(tmp_path / "in")).load_samples(), key=lambda s: (s.class_name, s.sample_id))
    assert [(s.class_name, s.sample_id) for s in samples] == [("apple", "0"), ("apple", "1"), ("pear", "7")]
    s = samples[1]
    assert isinstance(s, Sample) and s.get_relative_path() == "apple/images/1.jpg" and s.get_mask_relative_path() == "apple/masks/1.png"
    img, m, grey = s.load_image(), s.load_mask(), s.load_mask(binary=False)
    assert img.shape == (6, 8, 3) and img.dtype == np.uint8
    assert m.dtype == np.uint8 and m.sum() == 9 and set(np.unique(m)) == {0, 1} and m[5, 7] == 0
    assert grey.dtype == np.uint8 and grey[5, 7] == 128 and grey.max() == 255

    r = FilterResult(passed=True)
    assert (r.passed, r.reason, r.score, r.metadata) == (True, None, None, None)
    with pytest.raises(TypeError):
        FilterResult(passes=True)
    with pytest.raises(TypeError):
        BaseFilter("abstract")

    class OnlyApples(BaseFilter):
        def filter(self, sample):
            return FilterResult(passed=sample.class_name == "apple", reason="not an apple", score=1.0)

    class Never(BaseFilter):
        def filter(self, sample):
            raise AssertionError("a later filter ran after a failure")

    class OddIds(BaseFilter):
        def filter(self, sample):
            return FilterResult(passed=int(sample.sample_id) % 2 == 1)

    f = OnlyApples("apples")
    assert f.get_pass_rate() == 0.0
    ok, results = DatasetFilter([f, OddIds("odd")]).filter_sample(samples[0])
    assert ok is False and list(results) == ["apples", "odd"] and results["apples"].passed and not results["odd"].passed
    ok, results = DatasetFilter([f, Never("never")]).filter_sample(samples[2])
    assert ok is False and list(results) == ["apples"]
    assert f.stats == {"total_processed": 2, "passed": 1, "failed": 1} and f.get_pass_rate() == 0.5
    f.reset_stats()
    assert f.stats == {"total_processed": 0, "passed": 0, "failed": 0}

    df = DatasetFilter([f, OddIds("odd")])
    stats = df.filter_dataset(str(tmp_path / "in"), str(tmp_path / "out"), save_fail_cases=True)
    assert sorted(p.name for p in (tmp_path / "out" / "images").iterdir()) == ["apple_1.jpg"]
    assert sorted(p.name for p in (tmp_path / "out" / "masks").iterdir()) == ["apple_1.png"]
    assert not (tmp_path / "out" / "fail_cases").exists()                  # accepted, not drawn
    assert (stats["total_samples"], stats["passed_samples"], stats["failed_samples"]) == (3, 1, 2)
    assert stats["overall_pass_rate"] == 1 / 3 and stats["save_fail_cases"] is True
    assert stats["class_stats"]["apple"] == {"processed": 2, "passed": 1, "failed": 1, "pass_rate": 0.5}
    assert stats["class_stats"]["pear"] == {"processed": 1, "passed": 0, "failed": 1, "pass_rate": 0.0}
    assert stats["filter_breakdown"] == {"apples": {"total_processed": 3, "passed": 2, "failed": 1},
                                         "odd": {"total_processed": 2, "passed": 1, "failed": 1}}
    df.print_statistics()
    one = DatasetFilter([OddIds("odd")]).filter_dataset(str(tmp_path / "in"), str(tmp_path / "out1"), max_samples_per_class=1)
    assert one["total_samples"] == 2


def test_consistency_filter_is_lazy():
    from s3od_amd.filtering import BaseFilter, HorizontalFlipConsistencyFilter
    f = HorizontalFlipConsistencyFilter("no/such/checkpoint.ckpt")
    assert isinstance(f, BaseFilter) and f.name == "horizontal_flip_consistency"
    assert (f.threshold, f.consistency_threshold, f.device) == (0.7, 0.8, "cuda")
    assert f.model is None and f._model_loaded is False
    m = np.array([[0.2, 0.9], [0.6, 0.4]])
    assert f.calculate_iou(m, np.array([[0, 1], [0, 0]])) == 0.5


def test_save_results_layout(tmp_path, capsys):
    from s3od_amd.mining import save_results
    results = {"category_scores": {"a": np.float64(0.5), "b": np.float32(0.25), "c": float("nan")},
               "new_samples": {"a": 30, "b": 40, "c": 20},
               "category_sample_scores": {"a": [np.float64(0.5)], "b": [0.25, np.float32(0.25)], "c": []},
               "stable_categories": ["b", "a"], "unstable_categories": ["b", "a"]}
    path = save_results(results, str(tmp_path / "deep" / "dir"), prefix="run")
    assert path.startswith(str(tmp_path / "deep" / "dir" / "run_eval_results_")) and path.endswith(".json")
    assert "Results saved to:" in capsys.readouterr().out
    text = open(path).read()
    assert text.startswith('{\n    "category_scores": {')               # indent 4
    got = json.loads(text)
    assert list(got) == ["category_scores", "new_samples", "category_sample_scores", "stable_categories", "unstable_categories"]
    assert got["category_scores"]["a"] == 0.5 and got["category_scores"]["b"] == 0.25 and math.isnan(got["category_scores"]["c"])
    assert got["category_sample_scores"] == {"a": [0.5], "b": [0.25, 0.25], "c": []}
    assert got["new_samples"] == results["new_samples"] and got["stable_categories"] == ["b", "a"]


def test_flip_scores_record():
    from s3od_amd.flip_scores import FlipScores, scores_from_out
    r = scores_from_out([0.8, 0.6, 0.5, 3, 4, 0, 0, 1, 8])
    assert isinstance(r, FlipScores) and r._fields == ("s_orig", "s_flip", "s_cons", "iou_orig_gt", "iou_flip_gt",
                                                        "iou_orig_flip", "score")
    assert (r.iou_orig_gt, r.iou_flip_gt, r.iou_orig_flip) == (0.75, 1.0, 0.125)      # union 0 -> 1.0
    assert r.score == (0.8 + 0.6) * 0.5 / 2
    r = scores_from_out([0.8, 0.6, float("nan"), 0, 1, 0, 1, 0, 1])
    assert math.isnan(r.s_cons) and r.score == (0.8 + 0.6) * ((0.8 + 0.6) / 2) / 2     # the fallback
    assert math.isnan(scores_from_out([float("nan"), 0.6, 0.5, 0, 1, 0, 1, 0, 1]).score)


def test_alias_modules_import():
    import synth_sod.data_generation.filter_dataset as fd
    import synth_sod.data_generation.filters as filters
    import synth_sod.data_generation.filters.consistency_filter as cf
    import synth_sod.model_training.mine_samples as ms
    from s3od_amd import filtering, mining
    assert filters.__all__ == ["HorizontalFlipConsistencyFilter"]
    assert filters.HorizontalFlipConsistencyFilter is cf.HorizontalFlipConsistencyFilter is filtering.HorizontalFlipConsistencyFilter
    for name in ("Sample", "FilterResult", "BaseFilter", "DatasetLoader", "DatasetFilter", "calculate_iou"):
        assert getattr(fd, name) is getattr(filtering, name)
    for name in ("eval_sample", "eval_category", "calculate_new_samples", "analyze_stability", "save_results", "main"):
        assert getattr(ms, name) is getattr(mining, name)
    import inspect
    sig = inspect.signature(ms.main)
    assert [(p.name, p.default) for p in sig.parameters.values()][2:] == [
        ("img_size", 1024), ("min_samples", 20), ("max_samples", 100), ("max_val_samples", 10), ("output_dir", "results")]


def test_mining_cli_parses_the_reference_parameters(monkeypatch):
    from s3od_amd import mining
    seen = {}
    monkeypatch.setattr(mining, "main", lambda **kw: seen.update(kw))
    mining.cli(["--input_dir", "d", "--model_path", "m.ckpt", "--img_size", "512", "--max_val_samples", "3"])
    assert seen == {"input_dir": "d", "model_path": "m.ckpt", "img_size": 512, "min_samples": 20, "max_samples": 100,
                    "max_val_samples": 3, "output_dir": "results"}


def test_header_declares_the_new_entries():
    from s3od_amd._lib import lib
    L = lib()
    for name, nargs in (("s3od_mirror_u8", 6), ("s3od_flip_scores_ws", 3), ("s3od_flip_scores", 10)):
        assert name in L.decls and len(L.decls[name][1]) == nargs
    assert L.lib.s3od_abi_version() == 2

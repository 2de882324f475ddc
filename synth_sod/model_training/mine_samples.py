"""Alias of synth_sod/.../model_training/mine_samples.py (flip-consistency mining on MI355X).

    python -m synth_sod.model_training.mine_samples --input_dir D --model_path M
"""
from s3od_amd.mining import (analyze_stability, calculate_new_samples, cli, eval_category, eval_sample, main,  # noqa: F401
                             save_results)

if __name__ == "__main__":
    cli()

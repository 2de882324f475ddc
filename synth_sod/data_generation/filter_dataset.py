"""Alias of synth_sod/.../data_generation/filter_dataset.py's filtering framework."""
from s3od_amd.filtering import (BaseFilter, DatasetFilter, DatasetLoader, FilterResult, Sample,  # noqa: F401
                                calculate_iou)

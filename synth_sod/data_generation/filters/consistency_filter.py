"""Alias of synth_sod/.../data_generation/filters/consistency_filter.py (flip-consistency filter on MI355X)."""
from s3od_amd.filtering import HorizontalFlipConsistencyFilter  # noqa: F401

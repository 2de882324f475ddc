"""Alias of src/s3od/visualizer.py."""
from s3od_amd.visualizer import visualize_all_masks, visualize_removal  # noqa: F401

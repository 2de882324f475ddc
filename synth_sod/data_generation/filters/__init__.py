from .consistency_filter import HorizontalFlipConsistencyFilter

__all__ = ["HorizontalFlipConsistencyFilter"]

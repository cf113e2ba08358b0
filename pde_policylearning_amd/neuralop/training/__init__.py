"""The part of the reference's `neuralop.training` that runs on the engine: its losses (neuralop/training/losses.py)."""
from .losses import LpLoss, H1Loss, DissipativeLoss  # noqa: F401

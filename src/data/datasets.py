"""`src.data.datasets` import path of the reference (train.py:11), served by `aero_amd.data`."""
from aero_amd.data import LrHrSet  # noqa: F401

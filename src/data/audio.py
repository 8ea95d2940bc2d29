"""`src.data.audio` import path of the reference, served by `aero_amd.data` (the reader is `aero_amd.audio_io`, not torchaudio)."""
from aero_amd.data import Audioset  # noqa: F401

"""`src.models.seanet` import path of the reference (pickled class path `src.models.seanet.Seanet`), served by the MI355X-native implementation."""
from aero_amd.seanet import ResnetBlock, Seanet  # noqa: F401

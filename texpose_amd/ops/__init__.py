"""Thin torch-facing wrappers over the C ABI (include/texpose_amd.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; every computation on the hot
path is a hand-written gfx950 kernel in texpose_amd/csrc reached through ctypes.  All functions
require CUDA (ROCm) float32 tensors and raise if the library is unavailable -- there is no CPU or
eager fallback.

One module per stage over _base (the argument helpers and `_call`, the one place a launch is made), one namespace for callers:
``ops.name(...)``.  Tools and tests replace mlp_forward, mlp_backward, raygen, composite_fwd, patch_gather and step_inputs by assigning
to ``ops.<name>``: no module in here may call one of those six by its bare name or import it from a sibling.
"""
from .. import _lib  # noqa: F401
# the header's enumerators (TP_PIX_COORDS, ...) under their short names: tests and tools import them from here
from .._lib import (BOUNDS_AABB, BOUNDS_MAP, BOUNDS_NONE, JITTER_GIVEN, JITTER_MID, JITTER_PHILOX, MLP_F16, MLP_F16X3,  # noqa: F401
                    MLP_FP32, PACK_ALL, PACK_F16, PACK_F16X3, PACK_HEADS, PACK_RAYBIAS, PACK_TRUNK, PIX_COORDS, PIX_INDEX,
                    CompositeArgs, CompositeBwdArgs, MlpBwdArgs, MlpFwdArgs, MlpWeights, PatchGatherArgs, RaygenArgs)
from ._base import *  # noqa: F401,F403
from .render import *  # noqa: F401,F403
from .gan import *  # noqa: F401,F403
from .feat import *  # noqa: F401,F403
from .step import *  # noqa: F401,F403
from .scene import *  # noqa: F401,F403
from .pose import *  # noqa: F401,F403
from .refine import *  # noqa: F401,F403

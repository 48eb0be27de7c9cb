"""What icp.DepthRefiner and photo_align.PhotoRefiner share: the device check, the mesh on the device and a workspace per batch size."""
from typing import Dict

import torch

from . import ops

Tensor = torch.Tensor


class _MeshRefiner:
    _new_workspace = None                    # ops.<refiner>_workspace(B, H, W, device)

    def __init__(self, verts: Tensor, faces: Tensor, H: int, W: int, device, cull: bool = False):
        self.H, self.W, self.device = int(H), int(W), torch.device(device)
        self.cull = bool(cull)               # the loop's passes render with ops.mesh_raster(cull=True): the same bits (K34)
        if self.device.type != "cuda":
            raise ops._lib.TexposeLibraryError("%s runs the HIP kernels: a GPU device is needed (step_torch alone has a CPU route)"
                                               % type(self).__name__)
        self.verts = torch.as_tensor(verts).to(device=self.device, dtype=torch.float32).contiguous()
        self.faces = torch.as_tensor(faces).to(device=self.device, dtype=torch.int32).contiguous()
        self._workspaces: Dict[int, Tensor] = {}

    def _workspace(self, B: int) -> Tensor:
        if B not in self._workspaces:
            self._workspaces[B] = type(self)._new_workspace(B, self.H, self.W, self.device)
        return self._workspaces[B]

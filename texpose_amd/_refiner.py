"""What the refiner classes (icp.DepthRefiner, photo_align.PhotoRefiner, silhouette.SilhouetteRefiner, joint.JointRefiner) share: the
device check, the mesh (and its colours) on the device, a workspace per batch size and the measured masks' way to a distance field."""
from typing import Dict, Optional

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
        self._sdf_workspaces: Dict[int, Tensor] = {}

    def _workspace(self, B: int) -> Tensor:
        if B not in self._workspaces:                # (a refiner with lighting=True: its fit, K40, runs in the same bytes and may need more)
            extra = {"lighting": True} if getattr(self, "lighting", False) else {}
            self._workspaces[B] = type(self)._new_workspace(B, self.H, self.W, self.device, **extra)
        return self._workspaces[B]

    def _colours(self, vcolor, texels) -> None:
        """The mesh's colours on the device, checked: self.vcolor [V,3] and self.texels [F,T,3] (K35), each None where not given; how
        many of the two may be given is the subclass's rule."""
        up = lambda t: None if t is None else torch.as_tensor(t).to(device=self.device, dtype=torch.float32).contiguous()
        self.vcolor, self.texels = up(vcolor), up(texels)
        if self.texels is not None and (self.texels.dim() != 3 or self.texels.shape[0] != self.faces.shape[0] or self.texels.shape[2] != 3):
            raise ValueError("%s: texels [F,T,3] expected, T texels per face, got %s" % (type(self).__name__, tuple(self.texels.shape)))
        if self.vcolor is not None and tuple(self.vcolor.shape) != tuple(self.verts.shape):
            raise ValueError("%s: vcolor [V,3] expected, one colour per vertex, got %s" % (type(self).__name__, tuple(self.vcolor.shape)))

    def _field_of(self, mask_or_sdf: Tensor, known: Optional[Tensor]):
        """refine's measured masks [Ft,H,W] (uint8 or bool) as their distance field by ops.mask_sdf(known=), or their field (a float
        tensor) as it is -> (field [Ft,H,W], known [Ft,H,W] on the device or None)."""
        who = type(self).__name__
        planes = mask_or_sdf if mask_or_sdf.dim() == 3 else mask_or_sdf[None]
        if tuple(planes.shape[1:]) != (self.H, self.W):
            raise ValueError("%s.refine: planes of %d x %d expected, got %s" % (who, self.H, self.W, tuple(planes.shape)))
        if known is not None and planes.dtype.is_floating_point:
            raise ValueError("%s.refine: known= goes with masks; mask_or_sdf is a field (pass ops.mask_sdf(mask, known=known))" % who)
        if not planes.dtype.is_floating_point:
            Ft = planes.shape[0]
            if known is not None:
                known = (known if known.dim() == 3 else known[None]).to(self.device).contiguous()
            if Ft not in self._sdf_workspaces:
                self._sdf_workspaces[Ft] = ops.mask_sdf_workspace(Ft, self.H, self.W, self.device)
            planes = ops.mask_sdf(planes.to(self.device).contiguous(), workspace=self._sdf_workspaces[Ft], known=known)
        return planes, known

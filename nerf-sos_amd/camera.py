"""Learnable camera poses on the ray-gradient path: the reference's `models/camera.py::CameraTransformer` (:81-143).

A per-camera quaternion `rvec [C,4]` (x, y, z, w) and offset `tvec [C,3]` applied to rays that carry a camera id.  Constructor,
parameter / buffer names, shapes and initial values are the reference's, so its `state_dict()` loads.  Like the modules of
nerf_net.py this one holds parameters and sequences kernel launches (ops.camera_transform / ops.camera_transform_backward ->
csrc/camera.hip); it does no arithmetic and has no CPU path.

    cam = CameraTransformer(n_train_images, trainable=True).to(device)
    batch = scene.patch_batch(..., cam_id=True)
    ret = net(cam.transform(batch["rays_planar"], batch["cam_ids"].reshape(B, P, P)), (near, far))
    loss.backward()        # cam.rvec.grad / cam.tvec.grad next to the network's gradients

Rays that come out of a trainable module require a gradient, which `NeRFNet.render_rays` already serves (the generic fp32
kernels' input-gradient chain, nsos_ray_grad_reduce); the camera layer turns d loss / d rays into d loss / d (rvec, tvec).
"""
from __future__ import annotations

from typing import Tuple

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import ops


class _CameraTransform(torch.autograd.Function):
    """(rays_o, rays_d [...,3], ids [...] int32, rvec, tvec) -> [2,...,3] over nsos_camera_transform[_backward]."""

    @staticmethod
    def forward(ctx, rays_o, rays_d, ids, rvec, tvec, owner):
        rays_d = rays_d.contiguous()
        out = ops.camera_transform(rays_o, rays_d, ids, rvec, tvec, planar=True, ids_ready=True)
        ctx.save_for_backward(rays_d, ids, rvec)
        ctx.owner = owner
        return out

    @staticmethod
    @once_differentiable       # the kernels give first derivatives only: create_graph=True raises instead of returning constants
    def backward(ctx, g_out):
        rays_d, ids, rvec = ctx.saved_tensors
        need = ctx.needs_input_grad
        params, rays = need[3] or need[4], need[0] or need[1]
        g_out = g_out.contiguous()
        ws = ctx.owner._workspace_for(ids.numel(), rvec.device) if params else None
        g_rvec, g_tvec, g_o, g_d = ops.camera_transform_backward(g_out[0], g_out[1], rays_d, ids, rvec, workspace=ws, params=params,
                                                                 rays=rays, ids_ready=True)
        return (g_o if need[0] else None, g_d if need[1] else None, None, g_rvec if need[3] else None,
                g_tvec if need[4] else None, None)


class CameraTransformer(nn.Module):
    """models/camera.py:81-143.  `rvec` = [0,0,0,1] repeated, `tvec` = zeros: nn.Parameters when `trainable`, otherwise buffers
    of the same names."""

    def __init__(self, num_cams: int, trainable: bool = False):
        super().__init__()
        self.trainable = trainable
        identity_quat = torch.Tensor([0, 0, 0, 1]).repeat((num_cams, 1))
        identity_off = torch.Tensor([0, 0, 0]).repeat((num_cams, 1))
        if self.trainable:
            self.rvec = nn.Parameter(identity_quat)                # [N_cameras, 4]
            self.tvec = nn.Parameter(identity_off)                 # [N_cameras, 3]
        else:
            self.register_buffer('rvec', identity_quat)
            self.register_buffer('tvec', identity_off)
        # the backward's partial sums: one workspace per device, grown on demand, reused by every call (nothing allocated per step)
        self._ws = {}
        self._retired = []

    def _workspace_for(self, n_rays: int, device) -> torch.Tensor:
        need = ops.camera_workspace_bytes(n_rays, int(self.rvec.shape[0]))
        ws = self._ws.get(device)
        if ws is None or ws.numel() * 8 < need:
            if ws is not None:
                self._retired.append(ws)      # a graph captured at the smaller size still points into it
            ws = self._ws[device] = ops.camera_workspace(n_rays, int(self.rvec.shape[0]), device)
        return ws

    def _apply_layer(self, rays_o: torch.Tensor, rays_d: torch.Tensor, ids) -> torch.Tensor:
        if not (isinstance(rays_o, torch.Tensor) and rays_o.is_cuda and self.rvec.is_cuda):
            raise RuntimeError("nerf_sos_amd: CameraTransformer needs GPU tensors (module and rays) -- this package has no CPU path")
        ids = ops._cam_ids(ids, int(self.rvec.shape[0]), rays_o.device)
        return _CameraTransform.apply(rays_o, rays_d, ids, self.rvec, self.tvec, self)

    def rot_mats(self) -> torch.Tensor:
        """[C,3,3]: R(rvec[c]) (camera.py:103-118), read off the kernel by sending the three unit directions through camera c."""
        C = int(self.rvec.shape[0])
        if not self.rvec.is_cuda:
            raise RuntimeError("nerf_sos_amd: CameraTransformer needs GPU tensors (module and rays) -- this package has no CPU path")
        dev = self.rvec.device
        eye = torch.eye(3, device=dev).expand(C, 3, 3).contiguous()               # ray (c, j) = e_j  ->  R[c][:, j]
        ids = torch.arange(C, device=dev, dtype=torch.int32)[:, None].expand(C, 3).contiguous()
        cols = self._apply_layer(torch.zeros_like(eye), eye, ids)[1]
        return cols.transpose(1, 2)

    def forward(self, rays_o: torch.Tensor, rays_d: torch.Tensor, **render_kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        """The reference's format (camera.py:120-143): rays_o, rays_d [...,3+1] with the camera id as a float in the fourth column
        (the two id columns must agree) -> ([...,3], [...,3])."""
        if rays_o.shape[-1] != 4 or rays_d.shape[-1] != 4:
            raise ValueError(f"rays_o and rays_d must be [...,4] (xyz + camera id), got {tuple(rays_o.shape)} and {tuple(rays_d.shape)}")
        if not rays_o.is_cuda:
            raise RuntimeError("nerf_sos_amd: CameraTransformer needs GPU tensors (module and rays) -- this package has no CPU path")
        # camera.py:133 asserts on the host; inside a stream capture nothing may synchronise, so the check is skipped there
        if not torch.cuda.is_current_stream_capturing() and not torch.equal(rays_o[..., 3], rays_d[..., 3]):
            raise ValueError("the camera ids of rays_o and rays_d differ")
        # camera.py:134 `.type(torch.LongTensor)`: truncation toward zero (so -0.5 names camera 0, there as here).  The comparison is
        # made on the floats, before narrowing: NaN and anything the reference's indexing would refuse become -1 (NaN outputs)
        col = rays_o[..., 3].detach()
        ids = torch.where((col > -1) & (col < int(self.rvec.shape[0])), col, -1.0).to(torch.int32)
        out = self._apply_layer(rays_o[..., :3].contiguous(), rays_d[..., :3].contiguous(), ids)
        return out[0], out[1]

    def transform(self, rays: torch.Tensor, cam_ids) -> torch.Tensor:
        """This package's layout: rays [2,...,3] as NeRFNet takes them, cam_ids [...] integers (int32 on the device: nothing is
        converted or copied; a host sequence is range-checked and uploaded) -> [2,...,3]."""
        if rays.dim() < 2 or rays.shape[0] != 2 or rays.shape[-1] != 3:
            raise ValueError(f"rays must be [2,...,3], got {tuple(rays.shape)}")
        return self._apply_layer(rays[0], rays[1], cam_ids)

"""Torch restatement of the reference's camera layer (models/camera.py:103-143), in the dtype of its inputs: fp32 it is the
reference module's own ATen calls in its order (tests/golden/make_goldens_camera.py asserts bit-equality with the real module on
the CPU before it writes anything), fp64 it is the yardstick the kernels' accuracy bars are taken against.  Test infrastructure:
never imported by the package.  scripts/bench_camera.py imports it from here as the torch side of its comparison."""
import torch


def rot_mats(rvec: torch.Tensor) -> torch.Tensor:
    """camera.py:103-118: [C,4] (x, y, z, w) -> [C,3,3]."""
    theta = torch.sqrt(1e-5 + torch.sum(rvec ** 2, dim=1))
    rvec = rvec / theta[:, None]
    return torch.stack((
        1. - 2. * rvec[:, 1] ** 2 - 2. * rvec[:, 2] ** 2,
        2. * (rvec[:, 0] * rvec[:, 1] - rvec[:, 2] * rvec[:, 3]),
        2. * (rvec[:, 0] * rvec[:, 2] + rvec[:, 1] * rvec[:, 3]),

        2. * (rvec[:, 0] * rvec[:, 1] + rvec[:, 2] * rvec[:, 3]),
        1. - 2. * rvec[:, 0] ** 2 - 2. * rvec[:, 2] ** 2,
        2. * (rvec[:, 1] * rvec[:, 2] - rvec[:, 0] * rvec[:, 3]),

        2. * (rvec[:, 0] * rvec[:, 2] - rvec[:, 1] * rvec[:, 3]),
        2. * (rvec[:, 0] * rvec[:, 3] + rvec[:, 1] * rvec[:, 2]),
        1. - 2. * rvec[:, 0] ** 2 - 2. * rvec[:, 1] ** 2
    ), dim=1).view(-1, 3, 3)


def transform(rays_o: torch.Tensor, rays_d: torch.Tensor, ids: torch.Tensor, rvec: torch.Tensor, tvec: torch.Tensor):
    """camera.py:134-143 with the ids given apart: rays_o, rays_d [N,3], ids [N] integers -> (rays_o', rays_d')."""
    indx = ids.long()
    c2w = rot_mats(rvec)[indx]
    rays_d = torch.sum(rays_d[..., None, :3] * c2w[:, :3, :3], -1)
    rays_o = rays_o[..., :3] + tvec[indx]
    return rays_o, rays_d


def grads(rays_o, rays_d, ids, rvec, tvec, G_o, G_d):
    """Outputs and autograd gradients of sum(o' G_o) + sum(d' G_d) in the dtype of `rvec`: a dict of detached tensors."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (rays_o, rays_d, rvec, tvec)]
    with torch.enable_grad():
        o, d = transform(leaves[0], leaves[1], ids, leaves[2], leaves[3])
        ((o * G_o).sum() + (d * G_d).sum()).backward()
    return {"out_o": o.detach(), "out_d": d.detach(), "g_rays_o": leaves[0].grad, "g_rays_d": leaves[1].grad,
            "g_rvec": leaves[2].grad, "g_tvec": leaves[3].grad}


class Layer(torch.nn.Module):
    """The restatement as a module with the reference's parameter names (the refinement smoke's stand-in for the kernels)."""

    def __init__(self, num_cams: int, dtype=torch.float32):
        super().__init__()
        self.rvec = torch.nn.Parameter(torch.tensor([0., 0., 0., 1.], dtype=dtype).repeat(num_cams, 1))
        self.tvec = torch.nn.Parameter(torch.zeros(num_cams, 3, dtype=dtype))

    def transform(self, rays: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
        o, d = transform(rays[0].reshape(-1, 3), rays[1].reshape(-1, 3), ids.reshape(-1), self.rvec, self.tvec)
        return torch.stack([o.reshape(rays[0].shape), d.reshape(rays[1].shape)], 0)

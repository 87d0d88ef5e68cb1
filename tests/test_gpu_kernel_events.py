"""GPU: the ops.KERNEL_EVENTS contract bench.py times the MLP launches with: while it is a list, every ray wrapper appends exactly one
(n_points, start_event, end_event) per launch, recorded on the launch's stream; while it is None, nothing is recorded."""
import pytest
import torch

import nerf_sos_amd
from nerf_sos_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_kernel_events_one_entry_per_launch():
    torch.manual_seed(0)
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, use_semantics=True, sem_with_coord=True).to(DEV).eval()
    params = {k[len("nerf_fine.mlp."):]: v.detach() for k, v in net.state_dict().items() if k.startswith("nerf_fine.mlp.")}
    mode = ops.SEM_COORD
    R, S = 3, 5                                   # 15 points: one ragged tile
    o = torch.zeros(R, 3, device=DEV)
    d = torch.nn.functional.normalize(torch.randn(R, 3, device=DEV), dim=-1)
    z = torch.linspace(2.0, 6.0, S, device=DEV).repeat(R, 1).contiguous()
    fp32, fp16 = ops.pack_mlp(params, mode), ops.pack_mlp(params, mode, precision="fp16")
    calls = [lambda: ops.mlp_forward_rays(fp32, mode, o, d, d, z),
             lambda: ops.mlp_forward_rays_lp(fp16, mode, "fp16", o, d, d, z),
             lambda: ops.mlp_forward_rays_save(fp32, mode, o, d, d, z)]
    assert ops.KERNEL_EVENTS is None
    try:
        for call in calls:
            ops.KERNEL_EVENTS = []
            call()
            torch.cuda.synchronize()
            assert len(ops.KERNEL_EVENTS) == 1
            n_points, start, end = ops.KERNEL_EVENTS[0]
            assert n_points == R * S
            assert start.elapsed_time(end) >= 0.0
        last = ops.KERNEL_EVENTS                  # switched off: the list that was installed last gets nothing more
        ops.KERNEL_EVENTS = None
        for call in calls:
            call()
        torch.cuda.synchronize()
        assert ops.KERNEL_EVENTS is None and len(last) == 1
    finally:
        ops.KERNEL_EVENTS = None

"""CPU: the image models' wrappers live in nerf_sos_amd.image_ops; every name callers reach through `ops.` is still there."""
import pytest
import torch

import nerf_sos_amd  # noqa: F401
from nerf_sos_amd import image_ops, ops

# every `ops.dino* / ops.lpips* / ops.DINO* / ops.LPIPS*` the tree used before the move (bench.py, dino.py, lpips.py, metrics.py,
# tests/, scripts/)
MOVED = ["DINO_FULL_NHWC", "DINO_FULL_NORMALIZE", "DINO_NHWC", "DINO_PRECISIONS", "DINO_PREPARED", "DINO_STEP1", "LPIPS_CHANNELS",
         "LPIPS_CONV_KEYS", "LPIPS_LAYERS", "LPIPS_MIN_SIZE", "LPIPS_NHWC", "LPIPS_NORMALIZE", "dino_find_fg", "dino_forward",
         "dino_forward16", "dino_forward_full", "dino_full_workspace_floats", "dino_interp_pos", "dino_pack", "dino_pack16",
         "dino_resize_indices", "dino_workspace", "dino_workspace16", "dino_workspace16_floats", "dino_workspace_floats",
         "lpips_feature_sizes", "lpips_forward", "lpips_pack", "lpips_workspace_floats"]


def test_moved_names_resolve_on_ops_as_the_same_objects():
    assert len(MOVED) == len(set(MOVED)) == 29
    for name in MOVED:
        assert getattr(ops, name) is getattr(image_ops, name), name


@pytest.mark.parametrize("who", ["dino", "lpips"])
def test_buffer_errors_name_their_model(who):
    with pytest.raises(RuntimeError, match=f"nerf_sos_amd: {who} `packed` must be a contiguous float32 GPU tensor"):
        image_ops._buffer(torch.zeros(4), who, "packed", 16, torch.device("cpu"))

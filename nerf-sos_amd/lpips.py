"""LPIPS v0.1 with the AlexNet features (`lpips.LPIPS(net='alex')`, the default of every call site of the reference:
utils/image.py:149-160, engines/eval.py:87, utils/get_metrics.py:95) on the HIP kernels of csrc/lpips.hip.

The parameters carry the names and shapes of the published package's own state dict, so `LPIPS().load_state_dict(...)` takes
`lpips.LPIPS(net='alex').state_dict()`, and `LPIPS().load_pretrained(alexnet_state, lin_state)` takes the two files users actually
have: torchvision's AlexNet weights and the package's `alex.pth`.  Nothing here downloads anything.  Forward only (the reference
only evaluates with it); there is no CPU path.  Out of scope: net='vgg', spatial=True, gradients, 16-bit operands.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn as nn

from . import ops

SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)
_TV_KEYS = ("features.0", "features.3", "features.6", "features.8", "features.10")   # torchvision.models.alexnet


class _Holder(nn.Module):
    """Children under the checkpoint's numeric names (`slice2.3`, `model.1`): storage only."""

    def __init__(self, name: str, child: nn.Module):
        super().__init__()
        self.add_module(name, child)


class _Conv(nn.Module):
    def __init__(self, shape):
        super().__init__()
        fan_in = shape[1] * shape[2] * shape[3]
        self.weight = nn.Parameter(torch.randn(shape) * (2.0 / fan_in) ** 0.5, requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(shape[0]), requires_grad=False)


class _Lin(nn.Module):
    def __init__(self, channels: int):
        super().__init__()
        self.weight = nn.Parameter(torch.rand(1, channels, 1, 1), requires_grad=False)   # non-negative, as in the trained model


class _Scaling(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT).reshape(1, 3, 1, 1))
        self.register_buffer("scale", torch.tensor(SCALE).reshape(1, 3, 1, 1))


class _Alex(nn.Module):
    def __init__(self):
        super().__init__()
        for key, shape in zip(ops.LPIPS_CONV_KEYS, ops._LPIPS_CONV_SHAPES):
            _, slice_name, index = key.split(".")
            setattr(self, slice_name, _Holder(index, _Conv(shape)))


class LPIPS(nn.Module):
    """lpips.LPIPS(net='alex', lpips=True, spatial=False) in eval mode, frozen.  State dict: scaling_layer.{shift,scale} (buffers),
    net.slice{1..5}.{0,3,6,8,10}.{weight,bias}, lin{0..4}.model.1.weight."""

    def __init__(self, net: str = "alex"):
        super().__init__()
        if net != "alex":
            raise NotImplementedError(f"nerf_sos_amd.LPIPS: only net='alex' is built (every call site of the reference uses it), got {net!r}")
        self.scaling_layer = _Scaling()
        self.net = _Alex()
        for i, c in enumerate(ops.LPIPS_CHANNELS):
            setattr(self, f"lin{i}", _Holder("model", _Holder("1", _Lin(c))))
        self._packed = None
        self._packed_key = None
        self._workspace = {}
        self._retired = []

    # ---- loading
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """lpips.LPIPS's own state dict; its duplicate `lins.{i}.*` entries (the same tensors as `lin{i}.*`) are dropped."""
        sd = {k: v for k, v in state_dict.items() if not k.startswith("lins.")}
        ret = super().load_state_dict(sd, strict=strict, **kw)
        self.invalidate_packed()
        return ret

    def load_pretrained(self, alexnet_state: Dict[str, torch.Tensor], lin_state: Dict[str, torch.Tensor]) -> "LPIPS":
        """alexnet_state: torchvision's AlexNet state dict (`features.{0,3,6,8,10}.{weight,bias}`; the classifier's keys are
        ignored).  lin_state: the package's weights/v0.1/alex.pth (`lin{0..4}.model.1.weight`; `lins.*` duplicates are ignored).
        The scaling layer keeps its constants."""
        sd = {}
        for mine, theirs in zip(ops.LPIPS_CONV_KEYS, _TV_KEYS):
            for part in ("weight", "bias"):
                if f"{theirs}.{part}" not in alexnet_state:
                    raise KeyError(f"LPIPS.load_pretrained: the AlexNet state has no `{theirs}.{part}`")
                sd[f"{mine}.{part}"] = alexnet_state[f"{theirs}.{part}"]
        for i in range(ops.LPIPS_LAYERS):
            if f"lin{i}.model.1.weight" not in lin_state:
                raise KeyError(f"LPIPS.load_pretrained: the linear-layer state has no `lin{i}.model.1.weight`")
            sd[f"lin{i}.model.1.weight"] = lin_state[f"lin{i}.model.1.weight"]
        sd["scaling_layer.shift"], sd["scaling_layer.scale"] = self.scaling_layer.shift, self.scaling_layer.scale
        self.load_state_dict(sd)
        return self

    # ---- packed weights: once, and again when a tensor's storage or version changed (the pattern of DinoViT.packed_weights)
    def _tensors(self) -> Dict[str, torch.Tensor]:
        return {**dict(self.named_parameters()), **dict(self.named_buffers())}

    def _key(self):
        return tuple((t.data_ptr(), t._version) for t in self._tensors().values())

    def packed_weights(self) -> torch.Tensor:
        key = self._key()
        dev = self.scaling_layer.shift.device
        if self._packed is None or key != self._packed_key or self._packed.device != dev:
            if dev.type != "cuda":
                raise RuntimeError("nerf_sos_amd: LPIPS must live on a GPU -- this package has no CPU path")
            reuse = self._packed if self._packed is not None and self._packed.device == dev else None
            self._packed = ops.lpips_pack(self._tensors(), reuse)
            self._packed_key = key
        return self._packed

    def invalidate_packed(self):
        self._packed_key = None

    def _ws(self, batch: int, h: int, w: int, device) -> torch.Tensor:
        """ONE workspace per device, grown to the largest need seen and reused by every call, so that a captured call keeps valid
        pointers (the rule of DinoViT._ws: calls of one module on different streams at the same time would race on it)."""
        key = str(device)
        ws = self._workspace.get(key)
        need = ops.lpips_workspace_floats(batch, h, w)
        if ws is None or ws.numel() < need:
            if ws is not None:
                self._retired.append(ws)      # a graph captured at the smaller size still points into it
            ws = self._workspace[key] = torch.empty((need,), device=device, dtype=torch.float32)
        return ws

    def prepare(self, batch: int, h: int, w: int, device=None) -> None:
        """The first call's one-time work, done now (packed weights, workspace): a stream capture calls this beforehand."""
        device = self.scaling_layer.shift.device if device is None else torch.device(device)
        self.packed_weights()
        self._ws(int(batch), int(h), int(w), device)

    def _run(self, in0, in1, normalize=False, nhwc=False, **want) -> Dict[str, torch.Tensor]:
        for t in (in0, in1):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError("nerf_sos_amd: LPIPS needs GPU tensors -- this package has no CPU path")
        if in0.dim() != 4 or tuple(in0.shape) != tuple(in1.shape):
            raise ValueError(f"lpips needs two 4-d image batches of one shape, got {tuple(in0.shape)} and {tuple(in1.shape)}")
        N = int(in0.shape[0])
        h, w = (int(in0.shape[1]), int(in0.shape[2])) if nhwc else (int(in0.shape[2]), int(in0.shape[3]))
        flags = (ops.LPIPS_NORMALIZE if normalize else 0) | (ops.LPIPS_NHWC if nhwc else 0)
        packed = self.packed_weights()
        ws = self._ws(N, h, w, in0.device) if N > 0 and h >= ops.LPIPS_MIN_SIZE and w >= ops.LPIPS_MIN_SIZE else None
        with torch.no_grad():
            return ops.lpips_forward(in0.detach(), in1.detach(), packed, flags, ws, **want)

    # ---- the package's interface
    def forward(self, in0: torch.Tensor, in1: torch.Tensor, normalize: bool = False, nhwc: bool = False) -> torch.Tensor:
        """in0, in1 [N,3,H,W] in [-1,1] (normalize=True: in [0,1], mapped 2x-1 first) -> [N,1,1,1].  nhwc=True: [N,H,W,3] inputs
        (the renderer's layout), read as they are."""
        return self._run(in0, in1, normalize, nhwc)["lpips"]

    def layers(self, in0: torch.Tensor, in1: torch.Tensor, normalize: bool = False, nhwc: bool = False) -> torch.Tensor:
        """The five per-layer distances d_l, [N,5]; forward() is their sum in order 0..4."""
        return self._run(in0, in1, normalize, nhwc, want_layers=True)["layers"]

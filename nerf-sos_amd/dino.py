"""The frozen DINO ViT-S/16 feature extractor of the NeRF-SOS training step on the HIP kernels of csrc/dino_vit.hip.

Drop-in for the reference's `VitExtractor` as the trainer uses it (models/extractor.py:204-213 `get_vit_attn_feat`, called from
engines/trainer.py:101-109): the parameters carry the names and shapes of DINO's own checkpoint, so
`DinoViT().load_state_dict(torch.load("dino_deitsmall16_pretrain.pth"))` takes the file `torch.hub` would have fetched.  Nothing
here downloads anything.  The weights are frozen (the reference never trains DINO); the gradient with respect to the INPUT image is
there on request (`differentiable=True`, csrc/dino_vit_bwd.hip, fp32), as the reference's step back-propagates the contrastive term
through the class tokens into the rendered rgb.  There is no CPU path.

`DinoViT.precision` chooses the matrix pipe of the 224 x 224 path: "fp32" (default, csrc/dino_vit.hip) or "fp16" / "bf16"
(csrc/dino_vit16.hip: the operands of every matrix product in 16 bits, fp32 accumulation, everything else fp32).
"""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn as nn

from . import ops

DEPTH, WIDTH, HEADS, TOKENS, HIDDEN, PATCH, IMAGE = 12, 384, 6, 197, 1536, 16, 224


class _Affine(nn.Module):
    """A weight / bias pair under the checkpoint's name (nn.Linear, nn.LayerNorm or the patch convolution): storage only."""

    def __init__(self, w_shape, b_shape, ones=False):
        super().__init__()
        w = torch.ones(w_shape) if ones else nn.init.trunc_normal_(torch.empty(w_shape), std=0.02)
        self.weight = nn.Parameter(w, requires_grad=False)
        self.bias = nn.Parameter(torch.zeros(b_shape), requires_grad=False)


class _Attn(nn.Module):
    def __init__(self):
        super().__init__()
        self.qkv = _Affine((3 * WIDTH, WIDTH), (3 * WIDTH,))
        self.proj = _Affine((WIDTH, WIDTH), (WIDTH,))


class _Mlp(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc1 = _Affine((HIDDEN, WIDTH), (HIDDEN,))
        self.fc2 = _Affine((WIDTH, HIDDEN), (WIDTH,))


class _Block(nn.Module):
    def __init__(self):
        super().__init__()
        self.norm1 = _Affine((WIDTH,), (WIDTH,), ones=True)
        self.attn = _Attn()
        self.norm2 = _Affine((WIDTH,), (WIDTH,), ones=True)
        self.mlp = _Mlp()


class _PatchEmbed(nn.Module):
    def __init__(self):
        super().__init__()
        self.proj = _Affine((WIDTH, 3, PATCH, PATCH), (WIDTH,))


class _DinoFeatures(torch.autograd.Function):
    """feat / cls_ (/ attn, non-differentiable) of the fp32 224 x 224 path with the gradient to the input image: the forward is
    nsos_dino_forward_save (the launches of nsos_dino_forward plus one copy per block: the same output bits), the backward
    nsos_dino_backward on the block inputs kept in between (3.63 MB per image, freed with the graph)."""

    @staticmethod
    def forward(ctx, x, module, flags, patch_stride, want_attn):
        B = int(x.shape[0])
        saved = torch.empty((ops.dino_saved_floats(B),), device=x.device, dtype=torch.float32)
        out = ops.dino_forward(x.detach(), module.packed_weights(), flags, patch_stride, module._ws(B, x.device), want_attn=want_attn,
                               saved=saved)
        ctx.module, ctx.flags, ctx.patch_stride, ctx.shape = module, int(flags), int(patch_stride), tuple(x.shape)
        ctx.save_for_backward(saved)
        ctx.set_materialize_grads(False)      # an output the loss does not use arrives as None: the kernels' NULL, not a zeros tensor
        if want_attn:
            ctx.mark_non_differentiable(out["attn"])
            return out["feat"], out["cls_"], out["attn"]
        return out["feat"], out["cls_"]

    @staticmethod
    def backward(ctx, g_feat, g_cls, *_):
        m = ctx.module
        (saved,) = ctx.saved_tensors
        if g_feat is None and g_cls is None:
            return None, None, None, None, None
        g = ops.dino_backward(ctx.shape, ctx.flags, ctx.patch_stride, m.packed_weights(), m.packed_weights_backward(), saved, g_feat, g_cls,
                              m._ws_bwd(ctx.shape[0], saved.device))
        return g["g_input"], None, None, None, None


class DinoViT(nn.Module):
    """vit_small(patch_size=16) of models/vision_transformer.py, frozen.  150 state-dict tensors under DINO's names; `norm.*` is
    loaded and never applied (the reference reads block 11's output before the final norm).

    precision: "fp32" (default) | "fp16" | "bf16", a plain attribute like NeRFNet.mlp_precision, checked on assignment; it governs
    get_vit_attn_feat, patch_features and forward.  The 16-bit settings round the two operands of every matrix product once (weights
    at pack time, activations in their producer's epilogue) and accumulate in fp32; the residual stream, LayerNorm, softmax, bias,
    GELU and the outputs stay fp32, and the outputs are fp32 tensors with the same keys and shapes.  fp16 has no range check: an
    operand beyond 65504 becomes infinity (the largest 16-bit operand of the test weights is 162, tests/golden/
    dino_vit16.npz), so bf16 -- fp32's range at 8 bits of mantissa, about 8x fp16's error -- is the choice for a checkpoint whose
    activations are not known.  The full-image path (get_vit_attn_feat_noresize) is fp32 only, and so is the gradient to the input
    image (`differentiable=True` of get_vit_attn_feat / patch_features; the parameters never receive one)."""

    def __init__(self, precision: str = "fp32"):
        super().__init__()
        self.precision = precision
        self.cls_token = nn.Parameter(nn.init.trunc_normal_(torch.empty(1, 1, WIDTH), std=0.02), requires_grad=False)
        self.pos_embed = nn.Parameter(nn.init.trunc_normal_(torch.empty(1, TOKENS, WIDTH), std=0.02), requires_grad=False)
        self.patch_embed = _PatchEmbed()
        self.blocks = nn.ModuleList([_Block() for _ in range(DEPTH)])
        self.norm = _Affine((WIDTH,), (WIDTH,), ones=True)
        self._packed = None
        self._packed_key = None
        self._packed16 = {}          # precision -> (packed stream, key)
        self._packed_bwd = None      # the backward's stream (ops.dino_pack_backward), under the same key rule
        self._packed_bwd_key = None
        self._workspace_bwd = {}
        self._workspace = {}
        self._workspace16 = {}
        self._workspace_full = {}
        self._retired = []

    @property
    def precision(self) -> str:
        return self._precision

    @precision.setter
    def precision(self, value: str):
        if value not in ops.DINO_PRECISIONS:
            raise ValueError(f"DinoViT.precision must be one of {list(ops.DINO_PRECISIONS)}, got {value!r}")
        self._precision = value

    # ---- packed weights: once, and again when a parameter's storage or version changed (the pattern of NeRFMLP.packed_weights)
    def _key(self):
        # 150 (data_ptr, _version) pairs per call: a few tens of microseconds of host time, inside every eager timing
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def packed_weights(self) -> torch.Tensor:
        key = self._key()
        if self._packed is None or key != self._packed_key or self._packed.device != self.cls_token.device:
            if not self.cls_token.is_cuda:
                raise RuntimeError("nerf_sos_amd: DinoViT must live on a GPU -- this package has no CPU path")
            reuse = self._packed if self._packed is not None and self._packed.device == self.cls_token.device else None
            self._packed = ops.dino_pack(dict(self.named_parameters()), reuse)
            self._packed_key = key
        return self._packed

    def packed_weights_backward(self) -> torch.Tensor:
        """The stream of the backward to the input (the matrices as [out,in]), cached next to the forward's under the same rule."""
        key = self._key()
        if self._packed_bwd is None or key != self._packed_bwd_key or self._packed_bwd.device != self.cls_token.device:
            if not self.cls_token.is_cuda:
                raise RuntimeError("nerf_sos_amd: DinoViT must live on a GPU -- this package has no CPU path")
            reuse = self._packed_bwd if self._packed_bwd is not None and self._packed_bwd.device == self.cls_token.device else None
            self._packed_bwd = ops.dino_pack_backward(dict(self.named_parameters()), reuse)
            self._packed_bwd_key = key
        return self._packed_bwd

    def packed_weights16(self, precision: str) -> torch.Tensor:
        """The 16-bit stream of `precision`, cached next to the fp32 one under the same rule."""
        key = self._key()
        packed, have = self._packed16.get(precision, (None, None))
        if packed is None or key != have or packed.device != self.cls_token.device:
            if not self.cls_token.is_cuda:
                raise RuntimeError("nerf_sos_amd: DinoViT must live on a GPU -- this package has no CPU path")
            reuse = packed if packed is not None and packed.device == self.cls_token.device else None
            packed = ops.dino_pack16(dict(self.named_parameters()), precision, reuse)
            self._packed16[precision] = (packed, key)
        return packed

    def invalidate_packed(self):
        self._packed_key = self._packed_bwd_key = None
        self._packed16 = {p: (t, None) for p, (t, _) in self._packed16.items()}

    def _ws(self, batch: int, device) -> torch.Tensor:
        """ONE workspace per device, grown to the largest batch seen (3.6 MB per image) and reused by every call, so that a
        captured call keeps valid pointers.  Calls of one module on DIFFERENT streams at the same time would race on it: give each
        stream its own DinoViT (the packed weights are small) or order the streams.  That includes a captured training step that
        holds this module (GraphedPatchStep(dino=...)): while one of its replays is in flight, this DinoViT must not also be called
        from another stream -- the replay and the call would share the workspace."""
        key = str(device)
        ws = self._workspace.get(key)
        if ws is None or ws.numel() < ops.dino_workspace_floats(batch):
            if ws is not None:
                self._retired.append(ws)      # a graph captured at the smaller batch still points into it
            ws = self._workspace[key] = ops.dino_workspace(batch, device)
        return ws

    def _ws_bwd(self, batch: int, device) -> torch.Tensor:
        """The backward's workspace (4.25 MB per image), one per device, by the rule of _ws."""
        key = str(device)
        ws = self._workspace_bwd.get(key)
        if ws is None or ws.numel() < ops.dino_backward_workspace_floats(batch):
            if ws is not None:
                self._retired.append(ws)      # a graph captured at the smaller batch still points into it
            ws = self._workspace_bwd[key] = ops.dino_backward_workspace(batch, device)
        return ws

    def prepare(self, batch: int, device=None, backward: bool = False) -> None:
        """The first call's one-time work, done now: the packed weight stream of the current `precision` and the workspace for
        `batch` images on `device` (default: the parameters').  A stream capture calls this beforehand, so that the captured call
        packs nothing and allocates no workspace.  backward=True (fp32 only): also the backward's stream and workspace, for a
        capture that holds a `differentiable=True` call and its backward."""
        device = self.cls_token.device if device is None else torch.device(device)
        if backward:
            if self.precision != "fp32":
                raise ValueError(f"DinoViT: the backward to the input is fp32 only (precision is {self.precision!r})")
            self.packed_weights_backward()
            self._ws_bwd(int(batch), device)
        if self.precision == "fp32":
            self.packed_weights()
            self._ws(int(batch), device)
        else:
            self.packed_weights16(self.precision)
            self._ws16(int(batch), device)

    def _ws16(self, batch: int, device) -> torch.Tensor:
        """The 16-bit path's workspace (2.0 MB per image), one per device, by the rule of _ws; fp16 and bf16 share it."""
        key = str(device)
        ws = self._workspace16.get(key)
        if ws is None or ws.numel() < ops.dino_workspace16_floats(batch):
            if ws is not None:
                self._retired.append(ws)      # a graph captured at the smaller batch still points into it
            ws = self._workspace16[key] = ops.dino_workspace16(batch, device)
        return ws

    def _ws_full(self, batch: int, h: int, w: int, device) -> torch.Tensor:
        """The full-image path's workspace: ONE per device, grown to the largest need seen (the layout of a smaller (B, rows, cols)
        fits in a larger buffer) and reused by every call, so that a captured call keeps valid pointers (the pattern of _ws)."""
        key = str(device)
        ws = self._workspace_full.get(key)
        need = ops.dino_full_workspace_floats(batch, h, w)
        if ws is None or ws.numel() < need:
            if ws is not None:
                self._retired.append(ws)      # a graph captured at the smaller size still points into it
            ws = self._workspace_full[key] = torch.empty((need,), device=device, dtype=torch.float32)
        return ws

    def _run_full(self, x, flags, differentiable=False, **want) -> Dict[str, torch.Tensor]:
        if differentiable:
            raise ValueError("DinoViT: differentiable=True is not available on the full-image path (get_vit_attn_feat_noresize): the "
                             "backward to the input covers the 224 x 224 path only")
        if self.precision != "fp32":
            raise ValueError(f"DinoViT: the full-image path (get_vit_attn_feat_noresize) is fp32 only -- 16-bit precisions are out "
                             f"of its scope; set precision = 'fp32' (it is {self.precision!r})")
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("nerf_sos_amd: DinoViT needs a GPU tensor -- this package has no CPU path")
        if x.dim() != 4:
            raise ValueError(f"dino: expected a 4-d image batch, got {tuple(x.shape)}")
        h, w = (int(x.shape[1]), int(x.shape[2])) if flags & ops.DINO_FULL_NHWC else (int(x.shape[2]), int(x.shape[3]))
        packed = self.packed_weights()
        with torch.no_grad():
            return ops.dino_forward_full(x.detach(), packed, flags, self._ws_full(int(x.shape[0]), h, w, x.device), **want)

    def _run(self, x, flags, patch_stride=0, differentiable=False, **want) -> Dict[str, torch.Tensor]:
        precision = self.precision
        if differentiable:      # refused on the arguments alone, before any tensor is looked at
            if precision != "fp32":
                raise ValueError(f"DinoViT: differentiable=True needs precision 'fp32' -- the backward to the input has no 16-bit form "
                                 f"(precision is {precision!r})")
            if want.get("out") is not None:
                raise ValueError("DinoViT: out= together with differentiable=True -- autograd owns the outputs of a differentiable call")
            if want.get("want_prepared") or want.get("want_blocks"):
                raise ValueError("DinoViT: want_prepared / want_blocks are debug outputs of the plain forward, not of differentiable=True")
        if not isinstance(x, torch.Tensor) or not x.is_cuda:
            raise RuntimeError("nerf_sos_amd: DinoViT needs a GPU tensor -- this package has no CPU path")
        if differentiable and x.requires_grad and torch.is_grad_enabled():
            want_attn = bool(want.get("want_attn", True))
            res = _DinoFeatures.apply(x, self, int(flags), int(patch_stride), want_attn)
            out = {"feat": res[0], "cls_": res[1]}
            if want_attn:
                out["attn"] = res[2]
            return out
        with torch.no_grad():
            if precision == "fp32":
                return ops.dino_forward(x.detach(), self.packed_weights(), flags, patch_stride, self._ws(int(x.shape[0]), x.device), **want)
            return ops.dino_forward16(x.detach(), self.packed_weights16(precision), flags, precision, patch_stride,
                                      self._ws16(int(x.shape[0]), x.device), **want)

    # ---- the reference's interface
    def get_vit_attn_feat(self, x: torch.Tensor, prepared: bool = False, differentiable: bool = False, **want) -> Dict[str, torch.Tensor]:
        """models/extractor.py:204-213: x [B,3,h,w] -> nearest resize to 224x224, (x - mean) / std, the network;
        {'attn' [B,1,196], 'cls_' [B,384], 'feat' [B,196,384]}.  prepared=True: x is the [B,3,224,224] network input itself.
        out={"feat": ..., "cls_": ...}: contiguous float32 GPU tensors of those shapes that receive the two outputs instead of fresh
        allocations (ops.dino_forward checks them: ValueError); the returned dict holds the caller's tensors.
        differentiable=True (fp32 only, not with out=): if x requires grad, 'feat' and 'cls_' carry the gradient to x (HIP kernels,
        csrc/dino_vit_bwd.hip; 'attn' is marked non-differentiable); the output bits are those of the default call.  With False, or an
        x that does not require grad, exactly the default call's launches run and nothing is kept."""
        if prepared:
            if tuple(x.shape[1:]) != (3, IMAGE, IMAGE):
                raise ValueError(f"a prepared input is [B,3,{IMAGE},{IMAGE}], got {tuple(x.shape)}")
            return self._run(x, ops.DINO_PREPARED, differentiable=differentiable, **want)
        return self._run(x, 0, differentiable=differentiable, **want)

    def get_vit_attn_feat_noresize(self, x: torch.Tensor, **want) -> Dict[str, torch.Tensor]:
        """models/extractor.py:215-224: x [B,3,H,W] at full resolution -> (x - mean) / std (no resize), the network on the
        (H // 16) x (W // 16) patch grid with the position embedding interpolated; {'attn' [B,1,rows*cols], 'cls_' [B,384],
        'feat' [B,rows*cols,384]}.  H, W >= 16 and rows*cols <= 16384."""
        return self._run_full(x, 0, **want)

    def patch_features(self, rgb: torch.Tensor, patch_stride: int, differentiable: bool = False, **want) -> Dict[str, torch.Tensor]:
        """engines/trainer.py:103-109 from the rendered patches: rgb [B,P,P,3] (or [B,3,P,P]) -> resize to P*stride, normalise,
        then get_vit_attn_feat (which resizes to 224 and normalises again).  Returns get_vit_attn_feat's dict plus 'feats'
        [B,384,14,14] (the trainer's permuted view of 'feat': CorrelationLoss' orig_feats) and 'cls_tokens' (= 'cls_': similarity_negatives /
        NeRFContrastive).  out= as in get_vit_attn_feat: 'feat' / 'cls_' are then the caller's tensors, 'feats' / 'cls_tokens' the
        view of / the same storage, and with want_attn=False the call allocates nothing (what a captured training step relies on).
        differentiable=True: as in get_vit_attn_feat -- 'feat' / 'cls_' and their views 'feats' / 'cls_tokens' then carry the gradient
        to `rgb` (the reference's step: engines/trainer.py:103-108 runs the extractor on the render with autograd on)."""
        if patch_stride < 1:
            raise ValueError(f"patch_stride must be >= 1, got {patch_stride}")
        nhwc = rgb.dim() == 4 and rgb.shape[-1] == 3 and rgb.shape[1] != 3
        out = self._run(rgb, ops.DINO_STEP1 | (ops.DINO_NHWC if nhwc else 0), int(patch_stride), differentiable=differentiable, **want)
        B = out["feat"].shape[0]
        out["feats"] = out["feat"].reshape(B, 14, 14, WIDTH).permute(0, 3, 1, 2)   # engines/trainer.py:136-137
        out["cls_tokens"] = out["cls_"]
        return out

    def forward(self, x: torch.Tensor) -> Dict[str, torch.Tensor]:
        return self.get_vit_attn_feat(x)

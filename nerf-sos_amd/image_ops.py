"""The image models' wrappers over the C ABI (include/nerf_sos_hip.h): the DINO ViT-S/16 feature extractor (224 x 224 in fp32 and with
16-bit operands, the full-image path, find_fg) and LPIPS (AlexNet).  Same rules as ops.py, which re-exports every public name of this
module: PyTorch for device memory, streams and shapes only; contiguous fp32 GPU tensors; launches on the current stream."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib
from .ops import DTYPES, _dev, _p, _stream


# ------------------------------------------------------------------------------------------ what DINO and LPIPS share
def _buffer(t: torch.Tensor, who: str, name: str, nbytes: int, device) -> torch.Tensor:
    """A kernel-side buffer of `who` ("dino" / "lpips"): a contiguous float32 GPU tensor on `device` of at least nbytes."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"nerf_sos_amd: {who} `{name}` must be a contiguous float32 GPU tensor -- this package has no CPU path")
    if t.device != device:
        raise RuntimeError(f"{who}: `{name}` is on {t.device}, the data on {device}")
    if t.numel() * 4 < nbytes:
        raise ValueError(f"{who}: `{name}` holds {t.numel() * 4} bytes, {nbytes} needed")
    return t


def _image_dims(x: torch.Tensor, nhwc, who: str):
    """(B, h, w) of a 4-d batch of 3-channel images, [B,h,w,3] if `nhwc` else [B,3,h,w]."""
    if x.dim() != 4:
        raise ValueError(f"{who}: expected a 4-d image batch, got {tuple(x.shape)}")
    h, w, ch = (int(x.shape[1]), int(x.shape[2]), int(x.shape[3])) if nhwc else (int(x.shape[2]), int(x.shape[3]), int(x.shape[1]))
    if ch != 3:
        raise ValueError(f"{who}: expected 3 channels, got {tuple(x.shape)}")
    return int(x.shape[0]), h, w


def _floats(nbytes: int, refusal: str) -> int:
    """The answer of a `*_workspace_bytes` function as a count of float32 elements; 0 bytes = the kernels refuse the shape."""
    if nbytes == 0:
        raise ValueError(refusal)
    return int(nbytes) // 4


def _empty(floats: int, device) -> torch.Tensor:
    return torch.empty((floats,), device=device, dtype=torch.float32)


class _TensorTable:
    """The checkpoint tensors behind a pack call.  ptr(name): the tensor's address, after its shape (the pack kernels read exactly
    these extents) and its device (one GPU for all) are checked; the table keeps the tensors alive until the call is made."""

    def __init__(self, state: Dict[str, torch.Tensor], who: str, shape_of):
        self.state, self.who, self.shape_of, self.keep = state, who, shape_of, []

    def ptr(self, name: str) -> int:
        t = _dev(self.state[name].detach(), name)
        want = self.shape_of(name)
        if tuple(t.shape) != want:
            raise ValueError(f"{self.who}: `{name}` has shape {tuple(t.shape)}, the checkpoint's is {want}")
        if self.keep and t.device != self.keep[0].device:
            raise RuntimeError(f"{self.who}: `{name}` is on {t.device}, the other tensors on {self.keep[0].device}")
        self.keep.append(t)
        return t.data_ptr()

    def packed(self, packed: Optional[torch.Tensor], nbytes: int) -> torch.Tensor:
        """The stream the pack call writes: the caller's buffer, checked, or a fresh one on the tensors' device."""
        device = self.keep[0].device
        return _buffer(_empty(nbytes // 4, device) if packed is None else packed, self.who, "packed", nbytes, device)


# ------------------------------------------------------------------------------------------ DINO ViT-S/16 feature extractor
DINO_NHWC, DINO_STEP1, DINO_PREPARED = 1, 2, 4          # flags of nsos_dino_forward
DINO_DEPTH, DINO_WIDTH, DINO_TOKENS, DINO_IMAGE = 12, 384, 197, 224
_DINO_SHAPES = {"cls_token": (1, 1, 384), "pos_embed": (1, 197, 384), "patch_embed.proj.weight": (384, 3, 16, 16),
                "patch_embed.proj.bias": (384,), "norm1.weight": (384,), "norm1.bias": (384,), "attn.qkv.weight": (1152, 384),
                "attn.qkv.bias": (1152,), "attn.proj.weight": (384, 384), "attn.proj.bias": (384,), "norm2.weight": (384,),
                "norm2.bias": (384,), "mlp.fc1.weight": (1536, 384), "mlp.fc1.bias": (1536,), "mlp.fc2.weight": (384, 1536),
                "mlp.fc2.bias": (384,)}


_DINO_BLOCK_FIELDS = (("norm1_w", "norm1.weight"), ("norm1_b", "norm1.bias"), ("qkv_w", "attn.qkv.weight"), ("qkv_b", "attn.qkv.bias"),
                      ("proj_w", "attn.proj.weight"), ("proj_b", "attn.proj.bias"), ("norm2_w", "norm2.weight"), ("norm2_b", "norm2.bias"),
                      ("fc1_w", "mlp.fc1.weight"), ("fc1_b", "mlp.fc1.bias"), ("fc2_w", "mlp.fc2.weight"), ("fc2_b", "mlp.fc2.bias"))


def _dino_pack(state: Dict[str, torch.Tensor], packed: Optional[torch.Tensor], precision: str) -> torch.Tensor:
    table = _TensorTable(state, "dino", lambda name: _DINO_SHAPES[name.split(".", 2)[2] if name.startswith("blocks.") else name])
    ptr = table.ptr
    ts = _lib.DinoTensors()
    ts.cls_token, ts.pos_embed = ptr("cls_token"), ptr("pos_embed")
    ts.patch_w, ts.patch_b = ptr("patch_embed.proj.weight"), ptr("patch_embed.proj.bias")
    for i in range(DINO_DEPTH):
        for field, name in _DINO_BLOCK_FIELDS:
            setattr(ts.blocks[i], field, ptr(f"blocks.{i}.{name}"))
    L = _lib.lib()
    nbytes = {"fp32": L.nsos_dino_packed_bytes, "backward": L.nsos_dino_backward_packed_bytes}.get(precision, L.nsos_dino_packed16_bytes)()
    packed = table.packed(packed, int(nbytes))
    with torch.cuda.device(packed.device):
        if precision == "fp32":
            _lib.check(_lib.lib().nsos_dino_pack(C.byref(ts), _p(packed), packed.numel() * 4, _stream()), "nsos_dino_pack")
        elif precision == "backward":
            _lib.check(L.nsos_dino_pack_backward(C.byref(ts), _p(packed), packed.numel() * 4, _stream()), "nsos_dino_pack_backward")
        else:
            _lib.check(_lib.lib().nsos_dino_pack16(C.byref(ts), DTYPES[precision], _p(packed), packed.numel() * 4, _stream()),
                       "nsos_dino_pack16")
    return packed


def dino_pack(state: Dict[str, torch.Tensor], packed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """DINO's checkpoint tensors (state-dict names, on one GPU) -> the stream nsos_dino_forward reads (`nsos_dino_pack`)."""
    return _dino_pack(state, packed, "fp32")


def dino_pack_backward(state: Dict[str, torch.Tensor], packed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`nsos_dino_pack_backward`: the stream nsos_dino_backward reads beside dino_pack's -- the matrices in the state dict's own
    [out,in] layout, the operand of the data-gradient GEMMs."""
    return _dino_pack(state, packed, "backward")


DINO_PRECISIONS = ("fp32", "fp16", "bf16")


def _dino_precision16(precision: str) -> str:
    if precision not in ("fp16", "bf16"):
        raise ValueError(f"dino: the 16-bit entry points take precision 'fp16' or 'bf16', got {precision!r}")
    return precision


def dino_pack16(state: Dict[str, torch.Tensor], precision: str, packed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`nsos_dino_pack16`: the stream nsos_dino_forward16 reads at `precision` ("fp16" / "bf16"): an fp32 section (pos_embed, biases,
    LayerNorm vectors), then every matrix rounded once to 16 bits in its [out,in] layout.  Carried as a float32 tensor (raw bytes)."""
    return _dino_pack(state, packed, _dino_precision16(precision))


def dino_workspace_floats(batch: int) -> int:
    return _floats(_lib.lib().nsos_dino_workspace_bytes(int(batch)), f"dino: batch size {batch} outside what the kernels take")


def dino_workspace(batch: int, device) -> torch.Tensor:
    return _empty(dino_workspace_floats(batch), device)


def dino_workspace16_floats(batch: int) -> int:
    """The 16-bit path's workspace (`nsos_dino_workspace16_bytes`) as a count of float32 elements (the buffer is raw bytes)."""
    return _floats(_lib.lib().nsos_dino_workspace16_bytes(int(batch)), f"dino: batch size {batch} outside what the kernels take")


def dino_workspace16(batch: int, device) -> torch.Tensor:
    return _empty(dino_workspace16_floats(batch), device)


def _dino_out(out, batch: int) -> None:
    """The host-side half of the `out=` contract of dino_forward / dino_forward16: {"feat": [B,196,384], "cls_": [B,384]}, both
    contiguous float32 tensors.  (The device is compared with the input's once that is known to be a GPU tensor.)"""
    if not isinstance(out, dict) or set(out) != {"feat", "cls_"}:
        raise ValueError(f"dino: out= must be a dict with exactly the keys 'feat' and 'cls_', got "
                         f"{sorted(out) if isinstance(out, dict) else type(out).__name__}")
    for name, shape in (("feat", (batch, DINO_TOKENS - 1, DINO_WIDTH)), ("cls_", (batch, DINO_WIDTH))):
        t = out[name]
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"dino: out['{name}'] must be a tensor, got {type(t).__name__}")
        if tuple(t.shape) != shape:
            raise ValueError(f"dino: out['{name}'] has shape {tuple(t.shape)}, the call writes {shape}")
        if t.dtype != torch.float32:
            raise ValueError(f"dino: out['{name}'] must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"dino: out['{name}'] must be contiguous (strides {t.stride()}): the kernels write it densely")


def _dino_forward(x, packed, flags, patch_stride, workspace, want_attn, want_prepared, want_blocks, precision, out=None,
                  saved=None) -> Dict[str, torch.Tensor]:
    if saved is not None and (precision != "fp32" or want_prepared or want_blocks):
        raise ValueError("dino: saved= (nsos_dino_forward_save) is the fp32 forward without `prepared` / `blocks`")
    if out is not None:
        if not isinstance(x, torch.Tensor) or x.dim() != 4:
            raise ValueError(f"dino: expected a 4-d image batch, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
        _dino_out(out, int(x.shape[0]))
    L = _lib.lib()
    f32 = precision == "fp32"
    x = _dev(x, "x")
    B, h, w = _image_dims(x, flags & DINO_NHWC, "dino")
    dev = x.device
    ws_floats = dino_workspace_floats if f32 else dino_workspace16_floats
    if workspace is None:
        workspace = _empty(ws_floats(B), dev)
    _buffer(packed, "dino", "packed", int(L.nsos_dino_packed_bytes() if f32 else L.nsos_dino_packed16_bytes()), dev)
    _buffer(workspace, "dino", "workspace", ws_floats(B) * 4, dev)
    if saved is not None:
        _buffer(saved, "dino", "saved", dino_saved_floats(B) * 4, dev)
    if out is not None:
        for name in ("feat", "cls_"):
            if out[name].device != dev:
                raise ValueError(f"dino: out['{name}'] is on {out[name].device}, the data on {dev}")
        out = {"feat": out["feat"], "cls_": out["cls_"]}         # the caller's tensors; the optional outputs below are allocated
    else:
        out = {"feat": torch.empty((B, DINO_TOKENS - 1, DINO_WIDTH), device=dev, dtype=torch.float32),
               "cls_": torch.empty((B, DINO_WIDTH), device=dev, dtype=torch.float32)}
    if want_attn:
        out["attn"] = torch.empty((B, 1, DINO_TOKENS - 1), device=dev, dtype=torch.float32)
    if want_prepared:
        out["prepared"] = torch.empty((B, 3, DINO_IMAGE, DINO_IMAGE), device=dev, dtype=torch.float32)
    if want_blocks:
        out["blocks"] = torch.empty((DINO_DEPTH, B, DINO_TOKENS, DINO_WIDTH), device=dev, dtype=torch.float32)
    outs = (_p(out["feat"]), _p(out["cls_"]), _p(out.get("attn")), _p(out.get("prepared")), _p(out.get("blocks")), _stream())
    with torch.cuda.device(dev):
        if saved is not None:
            _lib.check(L.nsos_dino_forward_save(_p(x), B, h, w, int(patch_stride), int(flags), _p(packed), _p(workspace),
                                                workspace.numel() * 4, _p(out["feat"]), _p(out["cls_"]), _p(out.get("attn")), _p(saved),
                                                _stream()), "nsos_dino_forward_save")
        elif f32:
            _lib.check(L.nsos_dino_forward(_p(x), B, h, w, int(patch_stride), int(flags), _p(packed), _p(workspace), workspace.numel() * 4,
                                           *outs), "nsos_dino_forward")
        else:
            _lib.check(L.nsos_dino_forward16(_p(x), B, h, w, int(patch_stride), int(flags), DTYPES[precision], _p(packed), _p(workspace),
                                             workspace.numel() * 4, *outs), "nsos_dino_forward16")
    return out


def dino_forward(x: torch.Tensor, packed: torch.Tensor, flags: int, patch_stride: int = 0, workspace: Optional[torch.Tensor] = None,
                 want_attn: bool = True, want_prepared: bool = False, want_blocks: bool = False,
                 out: Optional[Dict[str, torch.Tensor]] = None, saved: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """`nsos_dino_forward`: x [B,h,w,3] (DINO_NHWC) or [B,3,h,w] -> {'feat' [B,196,384], 'cls_' [B,384], 'attn' [B,1,196]}
    (+ 'prepared' [B,3,224,224], 'blocks' [12,B,197,384] on request).  Launches only; capturable.
    out={"feat": ..., "cls_": ...}: contiguous float32 tensors of exactly those shapes on x's device that the kernels write instead of
    fresh ones (ValueError otherwise); the returned dict holds them.  With want_attn=False such a call allocates nothing.
    saved= (a buffer of dino_saved_floats(B) floats): `nsos_dino_forward_save` instead -- the same launches and the same output bits,
    and the input of every block kept in `saved` [12,B,197,384] for dino_backward."""
    return _dino_forward(x, packed, flags, patch_stride, workspace, want_attn, want_prepared, want_blocks, "fp32", out, saved)


def dino_saved_floats(batch: int) -> int:
    return _floats(_lib.lib().nsos_dino_saved_bytes(int(batch)), f"dino: batch size {batch} outside what the kernels take")


def dino_backward_workspace_floats(batch: int) -> int:
    return _floats(_lib.lib().nsos_dino_backward_workspace_bytes(int(batch)), f"dino: batch size {batch} outside what the kernels take")


def dino_backward_workspace(batch: int, device) -> torch.Tensor:
    return _empty(dino_backward_workspace_floats(batch), device)


def dino_backward(shape, flags: int, patch_stride: int, packed: torch.Tensor, packed_bwd: torch.Tensor, saved: torch.Tensor,
                  g_feat: Optional[torch.Tensor], g_cls: Optional[torch.Tensor], workspace: Optional[torch.Tensor] = None,
                  want_g_blocks: bool = False) -> Dict[str, torch.Tensor]:
    """`nsos_dino_backward`: the gradient of sum(feat * g_feat) + sum(cls_ * g_cls) with respect to the image of a dino_forward(...,
    saved=saved) call.  shape: that image's shape ([B,h,w,3] with DINO_NHWC in `flags`, else [B,3,h,w]); flags / patch_stride as given
    to the forward; packed from dino_pack, packed_bwd from dino_pack_backward; g_feat [B,196,384] / g_cls [B,384], either may be None
    (= zeros), not both.  Returns {'g_input': `shape`} (+ 'g_blocks' [12,B,197,384], the residual-stream gradient at every block's
    input, on request).  Launches only; capturable."""
    L = _lib.lib()
    if g_feat is None and g_cls is None:
        raise ValueError("dino: dino_backward needs g_feat or g_cls")
    first = g_feat if g_feat is not None else g_cls
    g_feat = None if g_feat is None else _dev(g_feat, "g_feat")
    g_cls = None if g_cls is None else _dev(g_cls, "g_cls")
    dev = first.device
    shape = tuple(int(n) for n in shape)
    if len(shape) != 4:
        raise ValueError(f"dino: expected the shape of a 4-d image batch, got {shape}")
    nhwc = bool(flags & DINO_NHWC)
    B, h, w, ch = (shape[0], shape[1], shape[2], shape[3]) if nhwc else (shape[0], shape[2], shape[3], shape[1])
    if ch != 3:
        raise ValueError(f"dino: expected 3 channels, got {shape}")
    for t, name, want in ((g_feat, "g_feat", (B, DINO_TOKENS - 1, DINO_WIDTH)), (g_cls, "g_cls", (B, DINO_WIDTH))):
        if t is not None and tuple(t.shape) != want:
            raise ValueError(f"dino: `{name}` has shape {tuple(t.shape)}, the gradient of that output is {want}")
        if t is not None and t.device != dev:
            raise RuntimeError(f"dino: `{name}` is on {t.device}, the data on {dev}")
    if workspace is None:
        workspace = dino_backward_workspace(B, dev)
    _buffer(packed, "dino", "packed", int(L.nsos_dino_packed_bytes()), dev)
    _buffer(packed_bwd, "dino", "packed_bwd", int(L.nsos_dino_backward_packed_bytes()), dev)
    _buffer(saved, "dino", "saved", dino_saved_floats(B) * 4, dev)
    _buffer(workspace, "dino", "workspace", dino_backward_workspace_floats(B) * 4, dev)
    out = {"g_input": torch.empty(shape, device=dev, dtype=torch.float32)}
    if want_g_blocks:
        out["g_blocks"] = torch.empty((DINO_DEPTH, B, DINO_TOKENS, DINO_WIDTH), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(L.nsos_dino_backward(B, h, w, int(patch_stride), int(flags), _p(packed), _p(packed_bwd), _p(saved), _p(g_feat), _p(g_cls),
                                        _p(workspace), workspace.numel() * 4, _p(out["g_input"]), _p(out.get("g_blocks")), _stream()),
                   "nsos_dino_backward")
    return out


def dino_forward16(x: torch.Tensor, packed: torch.Tensor, flags: int, precision: str, patch_stride: int = 0,
                   workspace: Optional[torch.Tensor] = None, want_attn: bool = True, want_prepared: bool = False,
                   want_blocks: bool = False, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """`nsos_dino_forward16`: dino_forward with the operands of every matrix product in `precision` ("fp16" / "bf16") and fp32
    accumulation; `packed` from dino_pack16 at the same precision, `workspace` from dino_workspace16.  Outputs are fp32 tensors of the
    same keys and shapes (`out=` as in dino_forward).  Launches only; capturable."""
    return _dino_forward(x, packed, flags, patch_stride, workspace, want_attn, want_prepared, want_blocks, _dino_precision16(precision), out)


def dino_resize_indices(in_size: int, patch_stride: int = 0):
    """The source index of each of the 224 rows / columns after the trainer's and the extractor's nearest resizes (host; the rule
    the prepare kernel evaluates).  patch_stride 0: the extractor's resize alone."""
    idx = (C.c_int32 * DINO_IMAGE)()
    _lib.check(_lib.lib().nsos_dino_resize_indices(int(in_size), int(patch_stride), idx), "nsos_dino_resize_indices")
    return list(idx)


# ---- DINO's full-image path (get_vit_attn_feat_noresize) and find_fg (engines/eval.py:133-144)
DINO_FULL_NHWC, DINO_FULL_NORMALIZE = 1, 2               # flags of nsos_dino_forward_full
DINO_FULL_MAX_PATCHES, DINO_PATCH = 16384, 16


def dino_full_workspace_floats(batch: int, h: int, w: int) -> int:
    return _floats(_lib.lib().nsos_dino_full_workspace_bytes(int(batch), int(h), int(w)),
                   f"dino: batch {batch} of {h}x{w} images is outside what the kernels take (H, W >= 16, "
                   f"(H // 16) * (W // 16) <= {DINO_FULL_MAX_PATCHES}, batch <= 1024)")


def dino_full_workspace(batch: int, h: int, w: int, device) -> torch.Tensor:
    return _empty(dino_full_workspace_floats(batch, h, w), device)


def dino_forward_full(x: torch.Tensor, packed: torch.Tensor, flags: int = 0, workspace: Optional[torch.Tensor] = None,
                      want_attn: bool = True, want_pos: bool = False) -> Dict[str, torch.Tensor]:
    """`nsos_dino_forward_full`: x [B,3,H,W] (or [B,H,W,3] with DINO_FULL_NHWC) at full resolution -> {'attn' [B,1,rows*cols],
    'cls_' [B,384], 'feat' [B,rows*cols,384]} with rows, cols = H // 16, W // 16 (+ 'pos' [1 + rows*cols, 384] on request).
    Launches only; capturable."""
    x = _dev(x, "x")
    B, h, w = _image_dims(x, flags & DINO_FULL_NHWC, "dino")
    dev = x.device
    nws = dino_full_workspace_floats(B, h, w) * 4
    if workspace is None:
        workspace = dino_full_workspace(B, h, w, dev)
    _buffer(packed, "dino", "packed", int(_lib.lib().nsos_dino_packed_bytes()), dev)
    _buffer(workspace, "dino", "workspace", nws, dev)
    n = (h // DINO_PATCH) * (w // DINO_PATCH)
    out = {"feat": torch.empty((B, n, DINO_WIDTH), device=dev, dtype=torch.float32),
           "cls_": torch.empty((B, DINO_WIDTH), device=dev, dtype=torch.float32)}
    if want_attn:
        out["attn"] = torch.empty((B, 1, n), device=dev, dtype=torch.float32)
    if want_pos:
        out["pos"] = torch.empty((n + 1, DINO_WIDTH), device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nsos_dino_forward_full(_p(x), B, h, w, int(flags), _p(packed), _p(workspace), workspace.numel() * 4,
                                                     _p(out["feat"]), _p(out["cls_"]), _p(out.get("attn")), _p(out.get("pos")),
                                                     _stream()), "nsos_dino_forward_full")
    return out


def dino_interp_pos(pos_embed, h: int, w: int):
    """The position table [1 + rows*cols, 384] nsos_dino_forward_full adds, from a CPU pos_embed [1,197,384] (host; the kernel's rule)."""
    pe = pos_embed.detach().reshape(DINO_TOKENS, DINO_WIDTH).to("cpu", torch.float32).contiguous()
    n = (int(h) // DINO_PATCH) * (int(w) // DINO_PATCH)
    out = torch.empty((n + 1, DINO_WIDTH), dtype=torch.float32)
    fp = C.POINTER(C.c_float)
    _lib.check(_lib.lib().nsos_dino_interp_pos(C.cast(pe.data_ptr(), fp), int(h), int(w), C.cast(out.data_ptr(), fp)), "nsos_dino_interp_pos")
    return out


_FG_WS: Dict[torch.device, torch.Tensor] = {}


def dino_find_fg(labels: torch.Tensor, attn: torch.Tensor, h: int, w: int) -> Dict[str, torch.Tensor]:
    """`nsos_dino_find_fg` for one image: labels int32 with H*W elements (e.g. [H,W,1]), attn float32 with (H//16)*(W//16)
    elements -> {'clustering' (labels' shape, int32, oriented), 'attn' [H,W,1] (nearest-upsampled), 'means' float64 [2]
    (cluster 0, cluster 1), 'flipped' int32 [1]}.  Launches only: no host synchronisation."""
    for t, name in ((labels, "clustering"), (attn, "attn")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError(f"nerf_sos_amd: `{name}` must be a GPU tensor -- this package has no CPU path")
    if labels.dtype != torch.int32:
        raise TypeError(f"find_fg: `clustering` must be int32, got {labels.dtype}")
    if attn.dtype != torch.float32:
        raise TypeError(f"find_fg: `attn` must be float32, got {attn.dtype}")
    if labels.device != attn.device:
        raise RuntimeError(f"find_fg: `clustering` is on {labels.device}, `attn` on {attn.device}")
    h, w = int(h), int(w)
    if h < DINO_PATCH or w < DINO_PATCH or labels.numel() != h * w or attn.numel() != (h // DINO_PATCH) * (w // DINO_PATCH):
        raise ValueError(f"find_fg: clustering {tuple(labels.shape)} / attn {tuple(attn.shape)} do not fit a {h}x{w} image")
    labels, attn = labels.contiguous(), attn.contiguous()
    dev = labels.device
    if dev not in _FG_WS:
        _FG_WS[dev] = torch.empty((int(_lib.lib().nsos_dino_find_fg_workspace_bytes()) + 15) // 16 * 4, device=dev, dtype=torch.float32)
    ws = _FG_WS[dev]
    out = {"clustering": torch.empty_like(labels), "attn": torch.empty((h, w, 1), device=dev, dtype=torch.float32),
           "means": torch.empty(2, device=dev, dtype=torch.float64), "flipped": torch.empty(1, device=dev, dtype=torch.int32)}
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nsos_dino_find_fg(_p(labels), _p(attn), h, w, _p(out["clustering"]), _p(out["attn"]), _p(out["means"]),
                                                _p(out["flipped"]), _p(ws), ws.numel() * 4, _stream()), "nsos_dino_find_fg")
    return out


# ------------------------------------------------------------------------------------------ LPIPS (AlexNet)
LPIPS_NHWC, LPIPS_NORMALIZE = 1, 2                       # flags of nsos_lpips_forward
LPIPS_LAYERS, LPIPS_MIN_SIZE = 5, 31
LPIPS_CHANNELS = (64, 192, 384, 256, 256)
LPIPS_CONV_KEYS = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")
_LPIPS_CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))


def lpips_key_shapes():
    """lpips.LPIPS(net='alex').state_dict() as this package keeps it: names and shapes, in the module's order."""
    out = [("scaling_layer.shift", (1, 3, 1, 1)), ("scaling_layer.scale", (1, 3, 1, 1))]
    for key, shp in zip(LPIPS_CONV_KEYS, _LPIPS_CONV_SHAPES):
        out += [(key + ".weight", shp), (key + ".bias", (shp[0],))]
    out += [(f"lin{i}.model.1.weight", (1, c, 1, 1)) for i, c in enumerate(LPIPS_CHANNELS)]
    return out


def lpips_feature_sizes(h: int, w: int):
    """[(H_l, W_l)] of the five feature maps of an h x w image."""
    a = ((h + 4 - 11) // 4 + 1, (w + 4 - 11) // 4 + 1)
    b = ((a[0] - 3) // 2 + 1, (a[1] - 3) // 2 + 1)
    c = ((b[0] - 3) // 2 + 1, (b[1] - 3) // 2 + 1)
    return [a, b, c, c, c]


def lpips_pack(state: Dict[str, torch.Tensor], packed: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LPIPS' tensors (the names of lpips_key_shapes, on one GPU) -> the stream nsos_lpips_forward reads (`nsos_lpips_pack`)."""
    table = _TensorTable(state, "lpips", dict(lpips_key_shapes()).__getitem__)
    ptr = table.ptr
    ts = _lib.LpipsTensors()
    ts.shift, ts.scale = ptr("scaling_layer.shift"), ptr("scaling_layer.scale")
    for i, key in enumerate(LPIPS_CONV_KEYS):
        ts.conv_w[i], ts.conv_b[i], ts.lin_w[i] = ptr(key + ".weight"), ptr(key + ".bias"), ptr(f"lin{i}.model.1.weight")
    packed = table.packed(packed, int(_lib.lib().nsos_lpips_packed_bytes()))
    with torch.cuda.device(packed.device):
        _lib.check(_lib.lib().nsos_lpips_pack(C.byref(ts), _p(packed), packed.numel() * 4, _stream()), "nsos_lpips_pack")
    return packed


def lpips_workspace_floats(batch: int, h: int, w: int) -> int:
    return _floats(_lib.lib().nsos_lpips_workspace_bytes(int(batch), int(h), int(w)),
                   f"lpips: {batch} pairs of {h}x{w} images are outside what the kernels take (H, W in {LPIPS_MIN_SIZE}..16384, "
                   f"1..1024 pairs)")


def lpips_workspace(batch: int, h: int, w: int, device) -> torch.Tensor:
    return _empty(lpips_workspace_floats(batch, h, w), device)


def lpips_forward(img0: torch.Tensor, img1: torch.Tensor, packed: torch.Tensor, flags: int = 0, workspace: Optional[torch.Tensor] = None,
                  want_layers: bool = False, want_feats: bool = False) -> Dict[str, torch.Tensor]:
    """`nsos_lpips_forward`: img0, img1 [N,3,H,W] (or [N,H,W,3] with LPIPS_NHWC) -> {'lpips' [N,1,1,1]} (+ 'layers' [N,5], 'feats': a
    list of five [2N,H_l,W_l,C_l] views, image 2b = img0[b], 2b+1 = img1[b], on request).  Launches only; capturable."""
    img0, img1 = _dev(img0, "img0"), _dev(img1, "img1")
    if img0.dim() != 4 or tuple(img0.shape) != tuple(img1.shape):
        raise ValueError(f"lpips needs two 4-d image batches of one shape, got {tuple(img0.shape)} and {tuple(img1.shape)}")
    if img0.device != img1.device:
        raise RuntimeError(f"lpips: img0 is on {img0.device}, img1 on {img1.device}")
    N, h, w = _image_dims(img0, flags & LPIPS_NHWC, "lpips")
    if h < LPIPS_MIN_SIZE or w < LPIPS_MIN_SIZE:
        raise ValueError(f"lpips: the smallest image AlexNet's second pool accepts is {LPIPS_MIN_SIZE}x{LPIPS_MIN_SIZE}, got {h}x{w}")
    dev = img0.device
    out = {"lpips": torch.empty((N, 1, 1, 1), device=dev, dtype=torch.float32)}
    if want_layers:
        out["layers"] = torch.empty((N, LPIPS_LAYERS), device=dev, dtype=torch.float32)
    if N == 0:
        if want_feats:
            out["feats"] = [torch.empty((0, a, b, c), device=dev) for (a, b), c in zip(lpips_feature_sizes(h, w), LPIPS_CHANNELS)]
        return out
    nws = lpips_workspace_floats(N, h, w) * 4
    if workspace is None:
        workspace = lpips_workspace(N, h, w, dev)
    _buffer(packed, "lpips", "packed", int(_lib.lib().nsos_lpips_packed_bytes()), dev)
    _buffer(workspace, "lpips", "workspace", nws, dev)
    flat = None
    if want_feats:
        sizes = [2 * N * a * b * c for (a, b), c in zip(lpips_feature_sizes(h, w), LPIPS_CHANNELS)]
        flat = torch.empty((sum(sizes),), device=dev, dtype=torch.float32)
        out["feats"] = [t.view(2 * N, a, b, c) for t, (a, b), c in zip(flat.split(sizes), lpips_feature_sizes(h, w), LPIPS_CHANNELS)]
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nsos_lpips_forward(_p(img0), _p(img1), N, h, w, int(flags), _p(packed), _p(out["lpips"]), _p(out.get("layers")),
                                                 _p(flat), _p(workspace), workspace.numel() * 4, _stream()), "nsos_lpips_forward")
    return out

"""A minimal torch restatement of the DINO ViT-S/16 feature path of the NeRF-SOS training step (test infrastructure and the GPU
timing baseline; the package never imports it).  Works in the dtype of its inputs (fp32, or fp64 for the error reference).

  step 1  engines/trainer.py:103-106        channels first, nearest resize to (P*stride, P*stride), (x - mean) / std
  step 2  models/extractor.py:204-208       nearest resize to 224x224, (x - mean) / std again
  step 3  models/vision_transformer.py      vit_small(patch_size=16): patch embedding, class token, pos_embed, 12 blocks
  step 4  models/extractor.py:109-117,209   block 11's output before the final norm -> cls_, feat; its softmax -> attn
"""
import torch
import torch.nn.functional as F

DEPTH, HEADS, EPS = 12, 6, 1e-6
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


_consts = {}


def normalize(x):
    key = (x.dtype, x.device)
    if key not in _consts:      # kept per dtype / device: a host-to-device copy per call could not be captured in a graph
        _consts[key] = (torch.tensor(MEAN, dtype=x.dtype, device=x.device).reshape(1, 3, 1, 1),
                        torch.tensor(STD, dtype=x.dtype, device=x.device).reshape(1, 3, 1, 1))
    mean, std = _consts[key]
    return (x - mean) / std


def trainer_step1(rgb, patch_stride):
    """rgb [B,P,P,3] as rendered -> the trainer's `dino_in` [B,3,P*stride,P*stride]."""
    x = rgb.permute(0, 3, 1, 2)
    x = F.interpolate(x, (rgb.shape[1] * patch_stride, rgb.shape[2] * patch_stride))
    return normalize(x)


def extractor_step2(x):
    """[B,3,h,w] -> the network input [B,3,224,224]."""
    return normalize(F.interpolate(x, size=(224, 224)))


def prepare(rgb, patch_stride):
    return extractor_step2(trainer_step1(rgb, patch_stride))


def network(sd, img, want_blocks=False):
    """img: prepared [B,3,224,224].  Returns {'attn' [B,1,196], 'cls_' [B,384], 'feat' [B,196,384]} (+ 'blocks': 12 x [B,197,384])."""
    B = img.shape[0]
    x = F.conv2d(img, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=16).flatten(2).transpose(1, 2)
    x = torch.cat((sd["cls_token"].expand(B, -1, -1), x), dim=1)
    x = x + sd["pos_embed"]
    C = x.shape[-1]
    N = x.shape[1]
    scale = (C // HEADS) ** -0.5
    blocks = []
    attn = None
    for i in range(DEPTH):
        p = f"blocks.{i}."
        y = F.layer_norm(x, (C,), sd[p + "norm1.weight"], sd[p + "norm1.bias"], EPS)
        qkv = F.linear(y, sd[p + "attn.qkv.weight"], sd[p + "attn.qkv.bias"]).reshape(B, N, 3, HEADS, C // HEADS).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        attn = ((q @ k.transpose(-2, -1)) * scale).softmax(dim=-1)
        y = (attn @ v).transpose(1, 2).reshape(B, N, C)
        x = x + F.linear(y, sd[p + "attn.proj.weight"], sd[p + "attn.proj.bias"])
        y = F.layer_norm(x, (C,), sd[p + "norm2.weight"], sd[p + "norm2.bias"], EPS)
        y = F.linear(F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
        x = x + y
        if want_blocks:
            blocks.append(x)
    out = {"attn": attn.mean(1).unsqueeze(1)[:, :, 0, 1:], "cls_": x[:, 0, :], "feat": x[:, 1:, :]}
    if want_blocks:
        out["blocks"] = blocks
    return out


def get_vit_attn_feat(sd, x, **kw):
    with torch.no_grad():
        return network(sd, extractor_step2(x), **kw)


def patch_features(sd, rgb, patch_stride, **kw):
    with torch.no_grad():
        return network(sd, prepare(rgb, patch_stride), **kw)


def similarity_argmin(cls_):
    """utils/image.py:187-190 get_similarity_matrix, then torch.min(sim, dim=0)[1] (:354): the negatives' indices."""
    sim = F.cosine_similarity(cls_.unsqueeze(0), cls_.unsqueeze(1), dim=2)
    return sim, torch.min(sim, dim=0)[1]

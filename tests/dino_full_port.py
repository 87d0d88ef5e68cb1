"""A torch restatement of DINO's full-image path of the NeRF-SOS evaluation (engines/eval.py:133-144 and :237-248): test
infrastructure and the GPU timing baseline; the package never imports it.  Works in the dtype of its inputs.

  eval.py:134-136            rgb [H,W,3] -> [1,3,H,W], normalize_batch (x - mean) / std
  extractor.py:215-224       get_vit_attn_feat_noresize: (x - mean) / std again, no resize, the network
  vision_transformer.py:174  interpolate_pos_encoding: bicubic resize of the 14x14 position grid to (H // 16, W // 16) unless
                             npatch == 196 and H == W
  eval.py:138-144            find_fg: nearest-upsample the class token's attention, flip the labels if cluster 1 looks darker
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import dino_port

DEPTH, HEADS, EPS, GRID, PATCH = 12, 6, 1e-6, 14, 16
normalize = dino_port.normalize


def grid_of(h, w):
    return h // PATCH, w // PATCH


def interpolate_pos(pos_embed, h, w):
    """models/vision_transformer.py:174-194 with the reference's own names: `w` there is the image HEIGHT (prepare_tokens unpacks
    B, nc, w, h = x.shape).  pos_embed [1,197,384] -> [1, 1 + rows*cols, 384]."""
    rows, cols = grid_of(h, w)
    N = pos_embed.shape[1] - 1
    if rows * cols == N and h == w:
        return pos_embed
    dim = pos_embed.shape[-1]
    w0, h0 = rows + 0.1, cols + 0.1
    p = F.interpolate(pos_embed[:, 1:].reshape(1, int(math.sqrt(N)), int(math.sqrt(N)), dim).permute(0, 3, 1, 2),
                      scale_factor=(w0 / math.sqrt(N), h0 / math.sqrt(N)), mode="bicubic")
    assert int(w0) == p.shape[-2] and int(h0) == p.shape[-1]
    return torch.cat((pos_embed[:, 0].unsqueeze(0), p.permute(0, 2, 3, 1).view(1, -1, dim)), dim=1)


def network(sd, img):
    """img: the network input [B,3,H,W] (already normalised).  {'attn' [B,1,rows*cols], 'cls_' [B,384], 'feat' [B,rows*cols,384]}."""
    B, _, h, w = img.shape
    x = F.conv2d(img, sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], stride=PATCH).flatten(2).transpose(1, 2)
    x = torch.cat((sd["cls_token"].expand(B, -1, -1), x), dim=1)
    x = x + interpolate_pos(sd["pos_embed"], h, w)
    C = x.shape[-1]
    N = x.shape[1]
    scale = (C // HEADS) ** -0.5
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
        x = x + F.linear(F.gelu(F.linear(y, sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"])), sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"])
    return {"attn": attn.mean(1).unsqueeze(1)[:, :, 0, 1:], "cls_": x[:, 0, :], "feat": x[:, 1:, :]}


def get_vit_attn_feat_noresize(sd, x):
    """models/extractor.py:215-224: x [B,3,H,W] -> (x - mean) / std -> the network."""
    with torch.no_grad():
        return network(sd, normalize(x))


def eval_dino_in(rgb):
    """engines/eval.py:134-136: rgb [B,H,W,3] as rendered -> normalize_batch of the channels-first image."""
    return normalize(rgb.permute(0, 3, 1, 2))


def upsample_attn(attn, h, w):
    """engines/eval.py:139-141: attn [1,1,rows*cols] -> nearest to (h, w) -> [h,w,1]."""
    rows, cols = grid_of(h, w)
    a = F.interpolate(attn.reshape(1, 1, rows, cols), (h, w))
    return a.permute(0, 2, 3, 1).squeeze(0)


def find_fg_numpy(attn_up, clustering):
    """engines/eval.py:142-144 as written: np.mean over each cluster, labels flipped by `1 - clustering` (2 -> -1).  An empty
    cluster's mean is NaN (numpy warns), the comparison is False, nothing flips."""
    attn_up, clustering = np.asarray(attn_up), np.asarray(clustering)
    with np.errstate(invalid="ignore", divide="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            flip = bool(np.mean(attn_up[clustering == 1]) < np.mean(attn_up[clustering == 0]))
    return (np.ones_like(clustering) - clustering if flip else clustering), flip


# ---- ATen's bicubic rule restated (float64), for the CPU test of the rule itself -----------------------------------------------
def _cubic_coeffs(t, A=-0.75):
    def c1(x):
        return ((A + 2) * x - (A + 3)) * x * x + 1

    def c2(x):
        return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
    return (c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t))


def bicubic_rule(grid, rows, cols):
    """grid [14,14,C] float64 -> [rows,cols,C] by upsample_bicubic2d(align_corners=False) with scale_factor (rows + 0.1) / 14:
    source coordinate (dst + 0.5) / scale_factor - 0.5, taps floor - 1 .. floor + 2 clamped to the grid, A = -0.75."""
    n = grid.shape[0]
    out = np.empty((rows, cols, grid.shape[2]))
    sy, sx = 1.0 / ((rows + 0.1) / math.sqrt(n * n)), 1.0 / ((cols + 0.1) / math.sqrt(n * n))
    for oy in range(rows):
        ry = sy * (oy + 0.5) - 0.5
        iy = math.floor(ry)
        cy = _cubic_coeffs(ry - iy)
        for ox in range(cols):
            rx = sx * (ox + 0.5) - 0.5
            ix = math.floor(rx)
            cx = _cubic_coeffs(rx - ix)
            acc = 0.0
            for i in range(4):
                yy = min(max(iy - 1 + i, 0), n - 1)
                r = sum(grid[yy, min(max(ix - 1 + j, 0), n - 1)] * cx[j] for j in range(4))
                acc = acc + r * cy[i]
            out[oy, ox] = acc
    return out

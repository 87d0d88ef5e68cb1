"""Evaluation metrics with the reference's call shapes, all on the device: SSIM (utils/image.py:139-147), sklearn's
adjusted_rand_score, segmap_cluster (utils/misc.py:40-52) and the metric blocks of engines/eval.py:31-93 (eval_one_view) and
engines/trainer.py:172-195 (the i_print logging), and LPIPS (utils/image.py:149-160) through a `nerf_sos_amd.LPIPS` model that holds
the user's weights.

The clustering is sklearn's KMeans(algorithm='lloyd') with greedy k-means++ seeding, but from this package's own counter-based
random stream (nsos_kmeans): sklearn's stream cannot be reproduced, so a seeded clustering is a different, equally valid local
optimum, and clus_ari moves inside the reference's own seed-to-seed spread.  With pinned initial centers the Lloyd loop follows
sklearn's step by step.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import ops


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True,
         format: str = "NCHW") -> torch.Tensor:
    """utils/image.py:139-147: format 'HWC' [H,W,C], 'NHWC' or 'NCHW'.  A 1-element fp32 tensor, or [N] without size_average."""
    if format == "HWC":
        img1, img2 = img1.permute(2, 0, 1)[None], img2.permute(2, 0, 1)[None]
    elif format == "NHWC":
        img1, img2 = img1.permute(0, 3, 1, 2), img2.permute(0, 3, 1, 2)
    elif format != "NCHW":
        raise ValueError(f"ssim: unknown format {format!r}")
    return ops.ssim(img1.contiguous(), img2.contiguous(), window_size, size_average)


def lpips(img1: torch.Tensor, img2: torch.Tensor, net: str = "alex", format: str = "NCHW", model=None) -> torch.Tensor:
    """utils/image.py:149-160 with the network handed in: `model` is a nerf_sos_amd.LPIPS holding the weights (the reference builds
    its own from the downloaded package).  format 'HWC' [H,W,3], 'NHWC' or 'NCHW'; images as the reference passes them (no 2x-1).
    [N,1,1,1] fp32.  The HWC / NHWC layouts are read in place: no permuted copy."""
    if net != "alex":
        raise NotImplementedError(f"lpips: only net='alex' is built (every call site of the reference uses it), got {net!r}")
    if model is None:
        raise ValueError("lpips: pass model=nerf_sos_amd.LPIPS() with its weights loaded -- nothing here downloads a network")
    if format == "HWC":
        return model(img1[None], img2[None], nhwc=True)
    if format == "NHWC":
        return model(img1, img2, nhwc=True)
    if format != "NCHW":
        raise ValueError(f"lpips: unknown format {format!r}")
    return model(img1, img2)


_lpips = lpips   # view_metrics' `lpips` argument shadows the function


def adjusted_rand_score(labels_true: torch.Tensor, labels_pred: torch.Tensor) -> torch.Tensor:
    """sklearn.metrics.adjusted_rand_score on device labelings: a 0-dim float64 tensor."""
    return ops.adjusted_rand_score(labels_true, labels_pred)[0]


def segmap_cluster(x: torch.Tensor, n_clusters: int = 2, seed: int = 0) -> torch.Tensor:
    """utils/misc.py:40-52: k-means of the [H,W,C] map's pixels -> int32 labels [H,W,1].  A leading batch dimension [B,H,W,C]
    clusters every slice on its own, in one launch ([B,H,W,1]); every slice draws from the same seed stream, so the batch equals
    per-slice calls (the trainer's loop, each with random_state=0)."""
    if x.dim() not in (3, 4):
        raise ValueError(f"segmap_cluster: x must be [H,W,C] or [B,H,W,C], got {tuple(x.shape)}")
    lead = tuple(x.shape[:-1])
    xb = x.float().reshape(1 if x.dim() == 3 else x.shape[0], -1, x.shape[-1])
    return ops.kmeans(xb, n_clusters, seed=seed, shared_stream=True)["labels"].reshape(*lead, 1)


def _labels_of(masks: torch.Tensor) -> torch.Tensor:
    if masks.dtype in ops.LABEL_DTYPES:
        return masks
    return masks.float()


def view_metrics(ret: Dict[str, torch.Tensor], target_s: Optional[torch.Tensor] = None, masks: Optional[torch.Tensor] = None,
                 N_cluster: int = 2, clus_no_sfm: bool = False, seed: int = 0, lpips=None) -> Dict[str, torch.Tensor]:
    """eval_one_view's metric_dict (mse psnr ssim clus_ari clus_ari_fg sem_ari sem_ari_fg, and lpips when a model is given) plus
    `sem` (argmax of the softmax, int32 [...,1]) and `clustering` (int32 [...,1]) on the device, from the render `ret` ('rgb' [H,W,3]
    and 'semantics' [H,W,C]; a ray list [R,3] / [R,C] works as well, except for SSIM and LPIPS, which need the image).  masks: the
    ground-truth labels (engines/eval.py:45 `batch['masks']`), fg = masks == 1.  The ARIs and SSIM are fp32 1-element tensors, as the
    reference's.  lpips: a nerf_sos_amd.LPIPS model -> out['lpips'] [1,1,1,1] (engines/eval.py:87 lpips(rgb, target_s,
    format='HWC')); None (the default): no 'lpips' key."""
    out: Dict[str, torch.Tensor] = {}
    sem = ret.get("semantics")
    rgb = ret.get("rgb")
    have_rgb = rgb is not None and target_s is not None
    pp = ops.eval_postprocess(sem, rgb if have_rgb else None, target_s if have_rgb else None)
    if have_rgb:
        out["mse"], out["psnr"] = pp["mse"], pp["psnr"]
        if rgb.dim() == 3:
            out["ssim"] = ssim(rgb, target_s.to(rgb.device), format="HWC")
            if lpips is not None:
                out["lpips"] = _lpips(rgb, target_s.to(rgb.device), format="HWC", model=lpips)
    if sem is not None:
        dev = sem.device
        feats = sem.float() if clus_no_sfm else pp["sem_prob"]   # engines/eval.py:49-54
        clus = ops.kmeans(feats.reshape(-1, feats.shape[-1]), N_cluster, seed=seed)["labels"]   # segmap_cluster, any layout
        out["sem"] = pp["sem"]
        out["clustering"] = clus.reshape(*feats.shape[:-1], 1)
        if masks is not None:
            gt = _labels_of(masks.to(dev)).reshape(-1)
            c = ops.adjusted_rand_score(gt, out["clustering"].reshape(-1).to(gt.dtype))
            s = ops.adjusted_rand_score(gt, out["sem"].reshape(-1).to(gt.dtype))
            vals = torch.cat([c, s]).float()
        else:
            vals = torch.zeros(4, device=dev, dtype=torch.float32)
        out["clus_ari"], out["clus_ari_fg"], out["sem_ari"], out["sem_ari_fg"] = vals[0:1], vals[1:2], vals[2:3], vals[3:4]
    return out


def patch_metrics(semantics: torch.Tensor, masks: torch.Tensor, N_cluster: int = 2, clus_no_sfm: bool = False,
                  seed: int = 0) -> Dict[str, torch.Tensor]:
    """engines/trainer.py:173-192 on the device: semantics [B,P,P,C], masks [B,P,P] or [B,P,P,1].  Every patch is clustered on
    its own (one launch for the batch); the four ARIs pool all patches.  Returns clus_ari, clus_ari_fg, sem_ari, sem_ari_fg as
    0-dim float64 tensors plus `sem` and `clustering` (int32 [B,P,P,1])."""
    if semantics.dim() != 4:
        raise ValueError(f"patch_metrics: semantics must be [B,P,P,C], got {tuple(semantics.shape)}")
    pp = ops.eval_postprocess(semantics)
    feats = semantics.float() if clus_no_sfm else pp["sem_prob"]
    clus = segmap_cluster(feats, N_cluster, seed)
    gt = _labels_of(masks.to(semantics.device)).reshape(-1)
    c = ops.adjusted_rand_score(gt, clus.reshape(-1).to(gt.dtype))
    s = ops.adjusted_rand_score(gt, pp["sem"].reshape(-1).to(gt.dtype))
    return {"clus_ari": c[0], "clus_ari_fg": c[1], "sem_ari": s[0], "sem_ari_fg": s[1], "sem": pp["sem"], "clustering": clus}


def find_fg(clustering: torch.Tensor, rgb: torch.Tensor, dino) -> Dict[str, torch.Tensor]:
    """engines/eval.py:133-144 (and :237-248) on the device: rgb [H,W,3] as rendered -> normalize_batch -> DINO's full-image path
    (`dino`: a DinoViT) -> the class token's attention nearest-upsampled to [H,W,1]; if its mean over cluster 1 is below its mean
    over cluster 0, clustering -> 1 - clustering.  clustering: int32 [H,W,1] as view_metrics returns it.  Returns {'clustering'
    (int32, oriented), 'attn' [H,W,1], 'flipped' (int32 [1])} plus 'means' (float64 [2]: clusters 0, 1); no host synchronisation."""
    if not isinstance(rgb, torch.Tensor) or not rgb.is_cuda:
        raise RuntimeError("nerf_sos_amd: find_fg needs a GPU tensor -- this package has no CPU path")
    if rgb.dim() != 3 or rgb.shape[-1] != 3:
        raise ValueError(f"find_fg: rgb must be [H,W,3], got {tuple(rgb.shape)}")
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    if not isinstance(clustering, torch.Tensor) or tuple(clustering.shape) not in ((H, W, 1), (H, W)):
        raise ValueError(f"find_fg: clustering must be [{H},{W},1], got {tuple(getattr(clustering, 'shape', ()))}")
    if clustering.device != rgb.device:
        raise RuntimeError(f"find_fg: clustering is on {clustering.device}, rgb on {rgb.device}")
    out = dino._run_full(rgb[None], ops.DINO_FULL_NHWC | ops.DINO_FULL_NORMALIZE)   # eval.py:134-137, fused
    return ops.dino_find_fg(clustering, out["attn"], H, W)

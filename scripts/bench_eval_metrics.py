"""Times the device evaluation metrics (nerf_sos_amd.metrics / ops) at C5 image size (1008x756) and for B = 8 patches of
64x64 (C = 2, K = 2), with the host path beside them (torch CPU SSIM as utils/ssim.py computes it, sklearn KMeans and
adjusted_rand_score, when sklearn is installed).  Prints one JSON line.

    python scripts/bench_eval_metrics.py [--reps 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nerf_sos_amd  # noqa: E402
from nerf_sos_amd import ops  # noqa: E402


def gpu_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def host_ms(fn, reps=3):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def torch_ssim_cpu(a, b, ws=11):
    g = torch.Tensor([np.exp(-(x - ws // 2) ** 2 / 4.5) for x in range(ws)])
    g = g / g.sum()
    C = a.shape[1]
    w = g[:, None].mm(g[None]).expand(C, 1, ws, ws).contiguous()
    conv = lambda t: F.conv2d(t, w, padding=ws // 2, groups=C)
    m1, m2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - m1 ** 2, conv(b * b) - m2 ** 2, conv(a * b) - m1 * m2
    return (((2 * m1 * m2 + 1e-4) * (2 * s12 + 9e-4)) / ((m1 ** 2 + m2 ** 2 + 1e-4) * (s1 + s2 + 9e-4))).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    H, W = 756, 1008
    img = torch.rand(1, 3, H, W, device=dev)
    img2 = (img + 0.05 * torch.randn_like(img)).clamp(0, 1)
    logits = torch.randn(H * W, 2, device=dev) * 2
    prob = torch.softmax(logits, -1)
    gt = (torch.rand(H * W, device=dev) < 0.3).to(torch.int32)
    pred = prob.argmax(-1).to(torch.int32)
    patches = prob[: 8 * 4096].reshape(8, 4096, 2).contiguous()
    iters = int(ops.kmeans(prob, 2, seed=0)["n_iter"])
    res = {
        "ssim_full_image_us": gpu_us(lambda: ops.ssim(img, img2), args.reps),
        "ari_pair_full_image_us": gpu_us(lambda: ops.adjusted_rand_score(gt, pred), args.reps),
        "kmeans_full_image_us": gpu_us(lambda: ops.kmeans(prob, 2, seed=0), max(5, args.reps // 5)),
        "kmeans_full_image_n_iter": iters,
        "kmeans_8_patches_64x64_us": gpu_us(lambda: ops.kmeans(patches, 2, seed=0, shared_stream=True), args.reps),
        "budgets_us": {"ssim": 50, "ari_pair": 30, "kmeans_full_image": 1500, "kmeans_8_patches": 300},
        "device": torch.cuda.get_device_name(0),
    }
    a, b = img.cpu(), img2.cpu()
    res["host_torch_cpu_ssim_ms"] = host_ms(lambda: torch_ssim_cpu(a, b))
    try:
        from sklearn.cluster import KMeans
        from sklearn.metrics import adjusted_rand_score
        p, g_, q = prob.cpu().numpy(), gt.cpu().numpy(), pred.cpu().numpy()
        pp = patches.cpu().numpy()
        res["host_sklearn_kmeans_full_ms"] = host_ms(lambda: KMeans(2, random_state=0).fit(p))
        res["host_sklearn_ari_pair_ms"] = host_ms(lambda: (adjusted_rand_score(g_, q), adjusted_rand_score(g_[g_ == 1], q[g_ == 1])))
        res["host_sklearn_kmeans_8_patches_ms"] = host_ms(lambda: [KMeans(2, random_state=0).fit(x) for x in pp])
    except ImportError:
        res["host_sklearn"] = "not installed"
    print(json.dumps(res))


if __name__ == "__main__":
    main()

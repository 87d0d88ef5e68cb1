"""LPIPS (AlexNet) on the HIP kernels against the same network as torch.nn.functional calls on the same GPU.

Two shapes: one 756x1008 pair (the evaluation image; 2 x 21.5 GFLOP) and eight 64x64 pairs (the training patch size), each eager and
captured in a graph.  Device events around `--iters` calls after `--warmup` calls; the median of `--repeats` windows and their
spread.  Prints one JSON line: ms, the speed-up over the torch modules, and for the large case the share of the fp32-MFMA peak
(157.3 TFLOP/s), which is a whole-call rate over peak, not a kernel's.  Weights are random (the timing does not depend on them).

    python scripts/bench_lpips.py [--iters 20] [--warmup 5] [--repeats 5] [--out profiles/lpips/bench_lpips.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nerf_sos_amd  # noqa: E402
from nerf_sos_amd import ops  # noqa: E402

PEAK_FP32_MFMA = 157.3e12
CONV = (("net.slice1.0", 4, 2), ("net.slice2.3", 1, 2), ("net.slice3.6", 1, 1), ("net.slice4.8", 1, 1), ("net.slice5.10", 1, 1))


def conv_flops(n_images, h, w):
    """2 * M * K * Cout of the five convolutions for n_images images (what the algorithm needs; padding taps counted)."""
    total = 0
    for (a, b), shp in zip(ops.lpips_feature_sizes(h, w), ops._LPIPS_CONV_SHAPES):
        total += 2 * n_images * a * b * shp[0] * shp[1] * shp[2] * shp[3]
    return total


def torch_lpips(sd, in0, in1):
    """The definition as torch.nn.functional calls (MIOpen / rocBLAS underneath), both images in one batch."""
    x = (torch.cat([in0, in1]) - sd["scaling_layer.shift"]) / sd["scaling_layer.scale"]
    n = in0.shape[0]
    val = None
    for i, (key, stride, pad) in enumerate(CONV):
        if i in (1, 2):
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, sd[key + ".weight"], sd[key + ".bias"], stride=stride, padding=pad))
        f = x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10)
        d = F.conv2d((f[:n] - f[n:]) ** 2, sd[f"lin{i}.model.1.weight"]).mean(dim=(2, 3), keepdim=True)
        val = d if val is None else val + d
    return val


def time_ms(fn, iters, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) / iters)
    return {"ms": statistics.median(windows), "min": min(windows), "max": max(windows)}


def captured(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g.replay, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = nerf_sos_amd.LPIPS().to(dev)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "cases": {}}
    for name, n, h, w in (("pair_756x1008", 1, 756, 1008), ("8_pairs_64x64", 8, 64, 64)):
        a = torch.rand(n, 3, h, w, device=dev)
        b = (a + 0.05 * torch.randn_like(a)).clamp(0, 1)
        model.prepare(n, h, w)
        with torch.no_grad():
            ours, theirs = model(a, b), torch_lpips(sd, a, b)
            diff = float((ours - theirs).abs().max() / theirs.abs().max())
            case = {"flop": conv_flops(2 * n, h, w), "rel_diff_vs_torch": diff}
            case["hip_eager"] = time_ms(lambda: model(a, b), args.iters, args.warmup, args.repeats)
            case["torch_eager"] = time_ms(lambda: torch_lpips(sd, a, b), args.iters, args.warmup, args.repeats)
            replay, _ = captured(lambda: model(a, b))
            case["hip_graph"] = time_ms(replay, args.iters, args.warmup, args.repeats)
            replay_t, _ = captured(lambda: torch_lpips(sd, a, b))
            case["torch_graph"] = time_ms(replay_t, args.iters, args.warmup, args.repeats)
        case["speedup_eager"] = case["torch_eager"]["ms"] / case["hip_eager"]["ms"]
        case["speedup_graph"] = case["torch_graph"]["ms"] / case["hip_graph"]["ms"]
        case["share_of_fp32_mfma_peak_graph"] = case["flop"] / (case["hip_graph"]["ms"] * 1e-3) / PEAK_FP32_MFMA
        result["cases"][name] = case
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Times the HIP DINO ViT-S/16 extractor (nerf_sos_amd.DinoViT.patch_features) against the torch restatement it replaces
(tests/dino_port.py, same weights, torch fp32 on the same GPU), eager and as a captured graph, for B in {1, 2, 8} patches of
64x64 at patch_stride 6 (the shipped recipe).  Device events around windows of many calls; hip and port windows alternate; the
median window and the spread (min .. max) are reported.  Prints one JSON line.

    python scripts/bench_dino.py [--iters 50] [--windows 7]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_dino.py --profile     # per-kernel times, B = 8, HIP path only
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nerf_sos_amd  # noqa: E402
import dino_port as port  # noqa: E402
import dino_weights as dw  # noqa: E402

PEAK_FP32_MFMA_TF = 157.3
C3_MS, C4_MS = 1.51, 2.70          # replayed C3 / C4 steps, DESIGN.md section 8 (quoted, not re-measured)
T, D, H = 197, 384, 1536


def useful_flop(B):
    """fp32 FLOP the algorithm needs (2 per multiply-add): patch embedding, 12 x (qkv, q.k, p.v, proj, fc1, fc2)."""
    gemm = 2.0 * B * 196 * 768 * D + 12 * 2.0 * B * T * (D * 3 * D + D * D + 2 * D * H)
    attn = 12 * 2.0 * B * 6 * (T * T * 64) * 2
    return gemm, attn


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def graphed(fn):
    fn()
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    return g.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dino needs a GPU (there is no CPU timing path)"
    dev = torch.device("cuda:0")
    sd = dw.make_state("wide", 11)
    model = nerf_sos_amd.DinoViT()
    model.load_state_dict(sd)
    model = model.to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    if args.profile:
        x = torch.rand(8, 64, 64, 3, device=dev)
        for _ in range(20):
            model.patch_features(x, 6)
        torch.cuda.synchronize()
        return
    res = {"bench": "dino_vit_s16", "device": torch.cuda.get_device_name(0), "P": 64, "patch_stride": 6, "iters": args.iters,
           "windows": args.windows, "peak_fp32_mfma_tflops": PEAK_FP32_MFMA_TF, "by_batch": {}}
    for B in (1, 2, 8):
        x = torch.rand(B, 64, 64, 3, device=dev, generator=torch.Generator(dev).manual_seed(B))
        fns = {"hip_eager": lambda: model.patch_features(x, 6), "port_eager": lambda: port.patch_features(sd_dev, x, 6)}
        fns["hip_graph"] = graphed(fns["hip_eager"])
        fns["port_graph"] = graphed(fns["port_eager"])
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in fns}
        for _ in range(args.windows):
            for k in ("hip_graph", "port_graph", "hip_eager", "port_eager"):       # alternating
                ts[k].append(window_ms(fns[k], args.iters))
        gemm, attn = useful_flop(B)
        row = {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in ts.items()}
        hip = row["hip_graph"]["median_ms"]
        row["useful_gflop"] = (gemm + attn) / 1e9
        row["hip_graph_tflops"] = (gemm + attn) / (hip * 1e-3) / 1e12
        row["hip_graph_fraction_of_fp32_mfma_peak"] = row["hip_graph_tflops"] / PEAK_FP32_MFMA_TF
        row["port_graph_over_hip_graph"] = row["port_graph"]["median_ms"] / hip
        row["share_of_c3_step"] = hip / C3_MS
        row["share_of_c4_step"] = hip / C4_MS
        res["by_batch"][str(B)] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()

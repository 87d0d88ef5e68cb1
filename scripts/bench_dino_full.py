"""Times DINO's full-image path (nerf_sos_amd.DinoViT.get_vit_attn_feat_noresize, what engines/eval.py:137 runs for find_fg)
against the torch restatement with the position-embedding interpolation (tests/dino_full_port.py, same weights, torch fp32 on the
same GPU: what the reference runs), eager and as a captured graph, B = 1 at 756 x 1008 (flower eval, 2 962 tokens) and 800 x 800
(Blender, 2 501 tokens).  Device events around windows of many calls; hip and port windows alternate; the median window and the
spread (min .. max) are reported.  Prints one JSON line (and writes it to --out).

    python scripts/bench_dino_full.py [--iters 20] [--windows 7] [--out profiles/dino/bench_dino_full.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_dino_full.py --profile     # per-kernel times, HIP path only
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
import dino_full_port as port  # noqa: E402
import dino_weights as dw  # noqa: E402

PEAK_FP32_MFMA_TF = 157.3
D, H = 384, 1536
SIZES = ((756, 1008), (800, 800))


def useful_flop(B, h, w):
    """fp32 FLOP the algorithm needs (2 per multiply-add): patch embedding, 12 x (qkv, proj, fc1, fc2) and 12 x (q.k, p.v)."""
    n = (h // 16) * (w // 16)
    T = n + 1
    gemm = 2.0 * B * n * 768 * D + 12 * 2.0 * B * T * (D * 3 * D + D * D + 2 * D * H)
    attn = 12 * 2.0 * 2.0 * B * T * T * D
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dino_full needs a GPU (there is no CPU timing path)"
    dev = torch.device("cuda:0")
    sd = dw.make_state("wide", 11)
    model = nerf_sos_amd.DinoViT()
    model.load_state_dict(sd)
    model = model.to(dev)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    if args.profile:
        for h, w in SIZES:
            x = torch.rand(1, 3, h, w, device=dev)
            for _ in range(10):
                model.get_vit_attn_feat_noresize(x)
        torch.cuda.synchronize()
        return
    res = {"bench": "dino_vit_s16_full_image", "device": torch.cuda.get_device_name(0), "B": 1, "iters": args.iters,
           "windows": args.windows, "peak_fp32_mfma_tflops": PEAK_FP32_MFMA_TF, "by_size": {}}
    for h, w in SIZES:
        x = torch.rand(1, 3, h, w, device=dev, generator=torch.Generator(dev).manual_seed(h))
        fns = {"hip_eager": lambda: model.get_vit_attn_feat_noresize(x), "port_eager": lambda: port.get_vit_attn_feat_noresize(sd_dev, x)}
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
        gemm, attn = useful_flop(1, h, w)
        row = {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in ts.items()}
        hip = row["hip_graph"]["median_ms"]
        row["tokens"] = (h // 16) * (w // 16) + 1
        row["useful_gflop"] = (gemm + attn) / 1e9
        row["attention_gflop"] = attn / 1e9
        row["hip_graph_tflops"] = (gemm + attn) / (hip * 1e-3) / 1e12
        row["hip_graph_fraction_of_fp32_mfma_peak"] = row["hip_graph_tflops"] / PEAK_FP32_MFMA_TF
        row["port_graph_over_hip_graph"] = row["port_graph"]["median_ms"] / hip
        res["by_size"][f"{h}x{w}"] = row
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

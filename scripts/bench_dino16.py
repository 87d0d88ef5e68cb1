"""Times the 16-bit DINO ViT-S/16 extractor (nerf_sos_amd.DinoViT with precision "fp16" / "bf16") against the fp32 HIP path (re-measured
in the same run) and against the torch restatement (tests/dino_port.py) run in the same 16-bit dtype on the same GPU (state and
prepared image cast; the port works in the dtype of its inputs), eager and as a captured graph, for B in {1, 2, 8} patches of 64x64
at patch_stride 6.  The method of scripts/bench_dino.py: device events around windows of many calls, the variants' windows alternate,
the median window and the spread (min .. max) are reported.  Prints one JSON line.

    python scripts/bench_dino16.py [--iters 50] [--windows 7]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_dino16.py --profile bf16     # per-kernel times, B = 8, HIP path only
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
from bench_dino import C3_MS, C4_MS, graphed, useful_flop, window_ms  # noqa: E402

PEAK_16BIT_MFMA_TF = 2500.0
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--profile", choices=list(DTYPES), default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dino16 needs a GPU (there is no CPU timing path)"
    dev = torch.device("cuda:0")
    sd = dw.make_state("wide", 11)
    models = {}
    for p in ("fp32",) + tuple(DTYPES):       # one module per precision: a captured graph keeps its module's buffers
        models[p] = nerf_sos_amd.DinoViT(precision=p)
        models[p].load_state_dict(sd)
        models[p] = models[p].to(dev)
    if args.profile:
        x = torch.rand(8, 64, 64, 3, device=dev)
        for _ in range(20):
            models[args.profile].patch_features(x, 6)
        torch.cuda.synchronize()
        return
    sd_dev = {p: {k: v.to(dev, dt) for k, v in sd.items()} for p, dt in DTYPES.items()}
    res = {"bench": "dino_vit_s16_16bit", "device": torch.cuda.get_device_name(0), "P": 64, "patch_stride": 6, "iters": args.iters,
           "windows": args.windows, "peak_16bit_mfma_tflops": PEAK_16BIT_MFMA_TF, "by_batch": {}}
    for B in (1, 2, 8):
        x = torch.rand(B, 64, 64, 3, device=dev, generator=torch.Generator(dev).manual_seed(B))
        fns = {}
        for p in models:
            fns[f"hip_{p}_eager"] = (lambda m: lambda: m.patch_features(x, 6))(models[p])
        for p, dt in DTYPES.items():           # the port in the same dtype: the prepared image is computed in fp32, then cast
            fns[f"port_{p}_eager"] = (lambda s, d: lambda: port.network(s, port.prepare(x, 6).to(d)))(sd_dev[p], dt)
        for k in list(fns):
            fns[k.replace("_eager", "_graph")] = graphed(fns[k])
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        order = sorted(fns, key=lambda k: (not k.endswith("_graph"), k))
        ts = {k: [] for k in fns}
        with torch.no_grad():
            for _ in range(args.windows):
                for k in order:                    # alternating
                    ts[k].append(window_ms(fns[k], args.iters))
        gemm, attn = useful_flop(B)
        row = {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))} for k, v in ts.items()}
        f32 = row["hip_fp32_graph"]
        row["useful_gflop"] = (gemm + attn) / 1e9
        for p in DTYPES:
            hip = row[f"hip_{p}_graph"]
            row[f"{p}_graph_speedup_over_fp32"] = f32["median_ms"] / hip["median_ms"]
            row[f"{p}_graph_slowest_over_fp32_fastest"] = hip["max_ms"] / f32["min_ms"]      # < 1: faster by more than the spread
            row[f"port_{p}_graph_over_hip_{p}_graph"] = row[f"port_{p}_graph"]["median_ms"] / hip["median_ms"]
            row[f"hip_{p}_graph_tflops"] = (gemm + attn) / (hip["median_ms"] * 1e-3) / 1e12
            row[f"{p}_share_of_c3_step"] = hip["median_ms"] / C3_MS
            row[f"{p}_share_of_c4_step"] = hip["median_ms"] / C4_MS
        res["by_batch"][str(B)] = row
    print(json.dumps(res))


if __name__ == "__main__":
    with torch.no_grad():
        main()

"""What the DINO extractor costs INSIDE the captured training step (GraphedPatchStep(dino=...)), against the two pieces it joins.

The step is the shipped frozen-backbone recipe of scripts/bench_train_step.py and bench.py's c3 / c4 (64 + 128 samples, semantic
head with coordinates, train-mode draws, both correlation losses, fused Adam; NeRF MLP in bf16; the contrastive term at weight 0.01
from two patches on, as in c4) on B patches of 64 x 64 at patch_stride 6: B = 1 (c3's batch), B = 2 (c4's per-GPU batch) and B = 8
(bench_train_step.py's).  The extractor carries tests/dino_weights.py's weights, at precision fp32 and fp16.  Per B and precision,
all three captured once and replayed:

  (a) the step on synthetic features (GraphedPatchStep(feat, cls_tokens) -- the ViT outside the path),
  (b) one DinoViT.patch_features(rgb [B,64,64,3], 6, want_attn=False) call on its own,
  (c) the step with dino=: render -> DINO on the rendered patches -> negatives -> losses -> backward -> Adam.

Device events around windows of `--iters` replays; the windows of (a), (b), (c) alternate; median and spread (min .. max) per item.
Reported: c - a (the extractor's cost in the step), a + b, and whether c <= a + b + the run's own window spread (the larger of the
three items' max - min).  Prints one JSON line; --out writes it to a file as well.

    python scripts/bench_train_step_dino.py [--iters 100] [--windows 7] [--batches 1,2,8] [--out profiles/dino/bench_train_step_dino.json]
"""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nerf_sos_amd  # noqa: E402
from nerf_sos_amd import synthetic as syn  # noqa: E402
import dino_weights as dw  # noqa: E402

PATCH, STRIDE = 64, 6


def loss_args():
    return types.SimpleNamespace(rand_neg=False, self_corr_w=0, use_sim_matrix=True, patch_stride=STRIDE,
                                 app_corr_params=["0.18", "1", "0.46", "1"], geo_corr_params=["0.5", "1", "3", "1"])


def make_step(B, dev, dino=None):
    torch.manual_seed(0)
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, use_semantics=True, sem_with_coord=True, perturb=1.0,
                               raw_noise_std=1.0, ray_chunk=1 << 20).to(dev)
    for n_, p_ in net.named_parameters():                      # run_nerf.py:307-318 (--fix_backbone)
        p_.requires_grad = "semantic_linear" in n_
    net.train()
    net.mlp_precision, net.rng, net.rng_seed = "bf16", "philox", 1
    opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)
    corr, geo = nerf_sos_amd.CorrelationLoss(loss_args()), nerf_sos_amd.GeoCorrelationLoss(loss_args())
    con = nerf_sos_amd.NeRFContrastive(device=dev) if B >= 2 else None
    rays = syn.synthetic_patches(B, PATCH, STRIDE, seed=0, device=dev)
    kw = dict(contrast_w=0.01, seed=0, warmup=3)
    if dino is not None:
        return nerf_sos_amd.GraphedPatchStep(net, opt, rays, (syn.NEAR, syn.FAR), None, None, corr, geo, con, dino=dino, patch_stride=STRIDE, **kw)
    gen = torch.Generator().manual_seed(1000 + B)
    feat = torch.randn(B, 384, 14, 14, generator=gen).to(dev)
    cls_ = (torch.randn(B, 384, generator=gen) + 3.0 * torch.randn(1, 384, generator=gen)).to(dev)   # one scene: a common component
    return nerf_sos_amd.GraphedPatchStep(net, opt, rays, (syn.NEAR, syn.FAR), feat, cls_, corr, geo, con, **kw)


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


def stat(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batches", default="1,2,8")
    ap.add_argument("--precisions", default="fp32,fp16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_train_step_dino needs a GPU (there is no CPU timing path)"
    dev = torch.device("cuda:0")
    sd = dw.make_state("wide", 11)
    res = {"bench": "train_step_dino", "device": torch.cuda.get_device_name(0), "P": PATCH, "patch_stride": STRIDE, "mlp_precision": "bf16",
           "iters": args.iters, "windows": args.windows, "cases": {}}
    for B in [int(b) for b in args.batches.split(",")]:
        for prec in args.precisions.split(","):
            dinos = []
            for _ in range(2):                                # (b) and (c) each own an extractor: one workspace per DinoViT
                m = nerf_sos_amd.DinoViT(prec)
                m.load_state_dict(sd)
                dinos.append(m.to(dev))
            step_a, step_c = make_step(B, dev), make_step(B, dev, dinos[1])
            if step_a.graph is None or step_c.graph is None:
                raise RuntimeError("the step was not captured")
            x = torch.rand(B, PATCH, PATCH, 3, device=dev, generator=torch.Generator(dev).manual_seed(B))
            fns = {"a_step_synthetic_features": step_a, "b_patch_features_alone": graphed(lambda: dinos[0].patch_features(x, STRIDE, want_attn=False)),
                   "c_step_with_dino": step_c}
            for fn in fns.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            ts = {k: [] for k in fns}
            for _ in range(args.windows):
                for k in fns:                                 # alternating
                    ts[k].append(window_ms(fns[k], args.iters))
            row = {k: stat(v) for k, v in ts.items()}
            a, b, c = (row[k]["median_ms"] for k in fns)
            spread = max(r["max_ms"] - r["min_ms"] for r in (row[k] for k in fns))
            row.update(dino_cost_in_step_ms=c - a, a_plus_b_ms=a + b, c_minus_a_plus_b_ms=c - (a + b), window_spread_ms=spread,
                       c_within_a_plus_b_plus_spread=bool(c <= a + b + spread),
                       loss_a=float(step_a.loss), loss_c=float(step_c.loss))
            res["cases"][f"B{B}_{prec}"] = row
            print(f"B={B} dino {prec}: a {a:.4f}  b {b:.4f}  c {c:.4f}  c-a {c - a:.4f}  c-(a+b) {c - a - b:+.4f}  spread {spread:.4f} ms",
                  file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

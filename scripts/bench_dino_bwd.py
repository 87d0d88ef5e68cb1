"""Times DINO's forward + backward to the input image (DinoViT.patch_features(differentiable=True) and its autograd backward:
csrc/dino_vit.hip + csrc/dino_vit_bwd.hip) for 8 patches of 64 x 64 at patch_stride 6 against the torch restatement
(tests/dino_port.py::network under torch autograd, same weights, fp32 on the same GPU), eager and as a captured graph, with the
forward-only call beside it.  Then the extractor's share of a contrastive training step: the eager sharded_patch_step of a field
that is not frozen (fp32, every parameter trainable, both correlation losses, NeRFContrastive at weight 1) with dino_grad=True
against the same step with dino_grad=False.  Device events around windows of calls; the items' windows alternate; median and spread
(min .. max) per item.  Prints one JSON line; --out writes it to a file as well.

    python scripts/bench_dino_bwd.py [--iters 20] [--windows 7] [--out profiles/dino/bench_dino_bwd.json]
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
from nerf_sos_amd import sharding  # noqa: E402
from nerf_sos_amd import synthetic as syn  # noqa: E402
import dino_port as port  # noqa: E402
import dino_weights as dw  # noqa: E402

B, PATCH, STRIDE = 8, 64, 6


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


def loss_args():
    return types.SimpleNamespace(rand_neg=False, self_corr_w=0, use_sim_matrix=True, patch_stride=STRIDE,
                                 app_corr_params=["0.18", "1", "0.46", "1"], geo_corr_params=["0.5", "1", "3", "1"])


def make_step(dev, dino, dino_grad):
    torch.manual_seed(0)
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, use_semantics=True, sem_with_coord=True, perturb=1.0,
                               raw_noise_std=1.0, ray_chunk=1 << 20).to(dev)
    net.train()
    net.rng, net.rng_seed = "philox", 1
    corr, geo, con = nerf_sos_amd.CorrelationLoss(loss_args()), nerf_sos_amd.GeoCorrelationLoss(loss_args()), nerf_sos_amd.NeRFContrastive(device=dev)
    rays = syn.synthetic_patches(B, PATCH, STRIDE, seed=0, device=dev)

    def step():
        for p in net.parameters():
            p.grad = None
        return sharding.sharded_patch_step(net, rays, (syn.NEAR, syn.FAR), B, None, None, corr, geo, step=0, seed=0, contrast_loss=con,
                                           contrast_w=1.0, dino=dino, patch_stride=STRIDE, dino_grad=dino_grad)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dino_bwd needs a GPU (there is no CPU timing path)"
    dev = torch.device("cuda:0")
    sd = dw.make_state("wide", 11)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    models = []
    for _ in range(3):                                        # eager, graph and the step each own an extractor: one workspace per DinoViT
        m = nerf_sos_amd.DinoViT()
        m.load_state_dict(sd)
        m = m.to(dev)
        m.prepare(B, backward=True)
        models.append(m)
    gen = torch.Generator(dev).manual_seed(B)
    x = torch.rand(B, PATCH, PATCH, 3, device=dev, generator=gen).requires_grad_()
    g_feat, g_cls = torch.randn(B, 196, 384, device=dev, generator=gen), torch.randn(B, 384, device=dev, generator=gen)

    def hip(m):
        def run():
            out = m.patch_features(x, STRIDE, differentiable=True, want_attn=False)
            return torch.autograd.grad((out["feat"] * g_feat).sum() + (out["cls_"] * g_cls).sum(), x)[0]
        return run

    def torch_port():
        out = port.network(sd_dev, port.prepare(x, STRIDE))
        return torch.autograd.grad((out["feat"] * g_feat).sum() + (out["cls_"] * g_cls).sum(), x)[0]

    a, b = hip(models[0])(), torch_port()
    agree = float((a - b).abs().max() / b.abs().max())
    fns = {"hip_forward_only_eager": lambda: models[0].patch_features(x.detach(), STRIDE, want_attn=False),
           "hip_fwd_bwd_eager": hip(models[0]), "port_fwd_bwd_eager": torch_port,
           "hip_fwd_bwd_graph": graphed(hip(models[1])), "port_fwd_bwd_graph": graphed(torch_port),
           "step_dino_grad_eager": make_step(dev, models[2], True), "step_forward_only_eager": make_step(dev, models[2], False)}
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(args.windows):
        for k in fns:                                         # alternating
            ts[k].append(window_ms(fns[k], args.iters))
    row = {k: stat(v) for k, v in ts.items()}
    med = {k: row[k]["median_ms"] for k in fns}
    res = {"bench": "dino_vit_s16_backward", "device": torch.cuda.get_device_name(0), "B": B, "P": PATCH, "patch_stride": STRIDE,
           "iters": args.iters, "windows": args.windows, "hip_vs_port_gradient_max_rel": agree, **row,
           "fwd_bwd_over_forward_eager": med["hip_fwd_bwd_eager"] / med["hip_forward_only_eager"],
           "port_over_hip_eager": med["port_fwd_bwd_eager"] / med["hip_fwd_bwd_eager"],
           "port_over_hip_graph": med["port_fwd_bwd_graph"] / med["hip_fwd_bwd_graph"],
           "extractor_fwd_bwd_share_of_contrastive_step": med["hip_fwd_bwd_eager"] / med["step_dino_grad_eager"],
           "dino_grad_cost_in_step_ms": med["step_dino_grad_eager"] - med["step_forward_only_eager"]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

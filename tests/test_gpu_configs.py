"""GPU (-m gpu): every BASELINE.json config that was not exercised at its own size / dtype in round 1.

  * C5: the full 1008x756 image in fp16 at 65 536-ray chunks -- finite, independent of the chunking, PSNR against the
    fp32 render of the same image, and a ray-sharded rank's block identical to the same rows of the full render;
  * C4: the per-GPU workload of the sharded training configuration (8192 rays = two 64x64 patches, train mode, semantic
    head with coordinates, both correlation losses, backward) on one GPU, in fp32 against the CPU port of the
    reference's losses evaluated on the rendered maps, and in bf16 against the fp32 step.
"""
import types

import numpy as np
import pytest
import torch

import nerf_sos_amd
from nerf_sos_amd import ops, sharding, synthetic as syn
from helpers import CFGS, ref_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 10.0 * np.log10(1.0 / max(mse, 1e-30))


FIELDS = {"fog (x1, +0.5)": (1.0, 0.5), "clumpy (x8, +0.5)": (8.0, 0.5), "default-init": None, "spiky (x40, -1.5)": (40.0, -1.5)}


@pytest.mark.parametrize("field,min_psnr", [("fog (x1, +0.5)", 55.0), ("clumpy (x8, +0.5)", 55.0), ("default-init", 40.0),
                                            ("spiky (x40, -1.5)", 40.0)])
def test_c5_full_image_fp16(manifest, field, min_psnr):
    """The whole 762 048-ray image in fp16 at 65 536-ray chunks: finite, independent of the chunking, a sharded rank's
    block identical to the same rows of the full render, and PSNR against the fp32 render of the same image.
    The PSNR bar depends on whether the field is well-posed at the far plane: the reference gives the LAST sample of a
    ray an interval of 1e10 (models/renderer.py:41), so its alpha is exactly 0 or 1 by the SIGN of that sample's sigma,
    and the ray's whole remaining transmittance goes with it.  Fields whose far-plane sigma has a robust sign (the two
    positive-bias fields) are held to >= 55 dB.  In the random-init field (sigma ~ +-0.01) and in the x40 head
    thresholded mid-distribution, 0.02-0.03 % of the rays have |sigma_last| below the fp16 error: those few rays change
    by O(1) -- in any reduced-precision implementation -- and cap the PSNR at 42-44 dB (asserted >= 40)."""
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, ray_chunk=65536, **CFGS["semcoord"]).to(DEV).eval()
    net.load_state_dict(ref_state("semcoord", manifest, peaky=False))
    if FIELDS[field]:
        syn.spiky_density_(net, *FIELDS[field])
    n = syn.H * syn.W
    assert n == 762048
    rays = syn.image_rays(DEV)
    keys = ("rgb", "depth", "acc", "semantics", "rgb0")
    with torch.no_grad():
        net.mlp_precision = "fp16"
        a = {k: v for k, v in net(rays, (syn.NEAR, syn.FAR), retraw=False).items() if k in keys}
        net.chunk = 32768 + 4096 + 7                              # ragged chunking of the same image
        b = {k: v for k, v in net(rays, (syn.NEAR, syn.FAR), retraw=False).items() if k in keys}
        net.chunk = 65536
        for k in keys:
            assert a[k].shape[0] == n
            assert torch.isfinite(a[k]).all() or k == "depth", f"{k} not finite"
            assert torch.equal(a[k], b[k]), f"fp16 {k}: result depends on the ray chunking"
        # a ray-sharded rank (rank 3 of 8) renders its block from pixel indices alone: identical rows
        s, e = sharding.shard_bounds(n, 3, 8)
        assert (s, e) == (3 * 95256, 4 * 95256)
        blk = net(syn.image_rays(DEV, (s, e)), (syn.NEAR, syn.FAR), retraw=False)
        for k in keys:
            assert torch.equal(blk[k], a[k][s:e]), f"shard != full for {k}"
        post = ops.eval_postprocess(semantics=a["semantics"])
        assert post["sem"].shape == (n, 1) and int(post["sem"].min()) >= 0 and int(post["sem"].max()) <= 1
        del b, blk
        net.mlp_precision = "fp32"
        ref = net(rays, (syn.NEAR, syn.FAR), retraw=False)
    p_rgb, p_rgb0 = _psnr(a["rgb"], ref["rgb"]), _psnr(a["rgb0"], ref["rgb0"])
    agree = float((ops.eval_postprocess(semantics=ref["semantics"])["sem"] == post["sem"]).float().mean())
    print(f"C5 fp16 vs fp32, full image, {field}: PSNR rgb {p_rgb:.1f} dB, rgb0 {p_rgb0:.1f} dB; labels agree on {agree:.5f}; "
          f"mean acc {float(ref['acc'].mean()):.3f}")
    assert p_rgb >= min_psnr and p_rgb0 >= min_psnr
    assert agree > 0.99, f"fp16 and fp32 label maps agree on {agree:.4f} of the pixels"


# measured (profiles/r06/b_c5_trained_image_tail.json; scripts/diag/lp_outliers.py explains the tail): of 762 048 rays, fp16 everywhere
# moves 837 by more than 0.01 (187 by more than 0.05, max 0.41 -- silhouette rays whose importance samples land elsewhere), bf16 1481;
# with the coarse pass in split fp16 the fp16 image has 9 such rays (max 0.026).  Bars = measurement + headroom for box-to-box noise.
C5_TRAINED = {
    ("fp16", None): dict(psnr=53.0, n01=1300, n05=320, within02=0.9990),
    ("bf16", None): dict(psnr=51.0, n01=2200, n05=420, within02=0.9985),
    ("fp16", "fp16x3"): dict(psnr=78.0, n01=30, n05=0, within02=0.9999),
}


@pytest.mark.parametrize("precision,coarse", list(C5_TRAINED))
def test_c5_full_image_trained_field(precision, coarse):
    """C5's workload on the TRAINED checkpoint (VERDICT r05 #1c): the whole 1008x756 image of held-out pose 0 in 65 536-ray chunks
    against the exact fp32 kernels (= the reference within 1e-4 on this field: test_gpu_trained.py): PSNR AND the tail -- counts of
    rays over 0.01 / 0.05, share within 0.02, depth -- plus label agreement and the PSNR against the analytic image."""
    import json
    import os
    from nerf_sos_amd import io as nio, quality
    scene = syn.ProceduralScene()
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, ray_chunk=65536, **CFGS["semcoord"]).to(DEV).eval()
    nio.load_checkpoint(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained_scene.ckpt"), net)
    for p_ in net.parameters():
        p_.requires_grad_(False)
    i = scene.i_test[0]
    H, W = syn.H, syn.W
    rays = ops.generate_rays(H, W, syn.intrinsics(H, W, scene.focal * W / scene.w), scene.poses[i, :3, :4], DEV).reshape(2, -1, 3)
    with torch.no_grad():
        net.mlp_precision, net.coarse_precision = precision, coarse
        lo = net(rays, (scene.NEAR, scene.FAR), retraw=False)
        lo = {k: lo[k].clone() for k in ("rgb", "depth", "semantics")}
        net.mlp_precision, net.coarse_precision = "fp32", None
        hi = net(rays, (scene.NEAR, scene.FAR), retraw=False)
    st = quality.tail_stats(lo["rgb"], hi["rgb"], lo["depth"], hi["depth"], lo["semantics"].argmax(-1), hi["semantics"].argmax(-1))
    gt = torch.from_numpy(scene.view(i, H, W)[0].reshape(-1, 3)).to(DEV)
    st["psnr_vs_analytic_image_db"] = {precision: round(_psnr(lo["rgb"], gt), 2), "fp32": round(_psnr(hi["rgb"], gt), 2)}
    os.makedirs("gpurun_out", exist_ok=True)
    path = "gpurun_out/c5_trained_image_tail.json"
    rec = json.load(open(path)) if os.path.exists(path) else {}
    rec[f"{precision}_coarse_{coarse or 'same'}"] = st
    json.dump(rec, open(path, "w"), indent=1, sort_keys=True)
    bar = C5_TRAINED[(precision, coarse)]
    assert torch.isfinite(lo["rgb"]).all()
    assert st["psnr_db"] >= bar["psnr"] and st["abs_rgb"]["n_gt_0.01"] <= bar["n01"] and st["abs_rgb"]["n_gt_0.05"] <= bar["n05"], st
    assert st["share_of_rays_within_0.02"] >= bar["within02"] and st["label_agreement"] >= 0.999, st
    assert abs(st["psnr_vs_analytic_image_db"][precision] - st["psnr_vs_analytic_image_db"]["fp32"]) < 0.3, st


def _loss_args():
    return types.SimpleNamespace(rand_neg=False, self_corr_w=0, use_sim_matrix=True, patch_stride=6,
                                 app_corr_params=["0.18", "1", "0.46", "1"], geo_corr_params=["0.5", "1", "3", "1"])


def _c4_step(precision, manifest, seed_draws=7, **step_kw):
    torch.manual_seed(0)
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, perturb=1.0, raw_noise_std=1.0, ray_chunk=1 << 20,
                               **CFGS["semcoord"]).to(DEV)
    net.load_state_dict(ref_state("semcoord", manifest, peaky=True))
    for n_, p_ in net.named_parameters():
        p_.requires_grad = "semantic_linear" in n_
    net.train()
    net.mlp_precision = precision
    B = 2
    rays = syn.synthetic_patches(B, 64, 6, seed=0, device=DEV)
    assert rays.shape == (2, B, 64, 64, 3) and rays[0].numel() // 3 == 8192
    feat = torch.randn(B, 384, 14, 14, generator=torch.Generator().manual_seed(1)).to(DEV)
    cls_ = torch.randn(B, 384, generator=torch.Generator().manual_seed(2)).to(DEV)
    corr, geo = nerf_sos_amd.CorrelationLoss(_loss_args()), nerf_sos_amd.GeoCorrelationLoss(_loss_args())
    torch.manual_seed(seed_draws)                                # the render's jitter / noise draws
    loss = sharding.sharded_patch_step(net, rays, (syn.NEAR, syn.FAR), B, feat, cls_, corr, geo, step=3, seed=11, **step_kw)
    grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.requires_grad}
    return net, rays, feat, cls_, loss, grads


def test_c4_per_gpu_workload_fp32_vs_port_losses(manifest):
    """8192 rays in train mode through render -> losses -> backward on one GPU; the loss value is re-derived on the CPU
    with the port of the reference's loss classes (oracle/losses_port.py, pinned to the real classes) from the maps the
    HIP path rendered and the same generator draws."""
    from oracle import losses_port as lp
    net, rays, feat, cls_, loss, grads = _c4_step("fp32", manifest)
    assert torch.isfinite(loss)
    assert len(grads) == 8 and all(torch.isfinite(g).all() and float(g.abs().max()) > 0 for g in grads.values())
    # replay: same render draws -> same maps; then the port's losses on the CPU with the generator's draws
    torch.manual_seed(7)
    with torch.no_grad():
        ret = net(rays, (syn.NEAR, syn.FAR), retraw=False)
    gen = sharding.loss_generator(torch.device(DEV), 3, 11)
    S = 11
    draws = list(torch.rand([2, 2, 2, S, S, 2], device=DEV, generator=gen).cpu().reshape(4, 2, S, S, 2))   # one launch: corr(s0) rand1, rand2, corr(s1) rand1, rand2
    sim = sharding.similarity_matrix(cls_).cpu()
    s0, s1 = ret["semantics0"].permute(0, 3, 1, 2).cpu(), ret["semantics"].permute(0, 3, 1, 2).cpu()
    depth = ret["depth"].permute(0, 3, 1, 2).cpu().contiguous()
    ro, rd = rays[0].permute(0, 3, 1, 2).cpu(), rays[1].permute(0, 3, 1, 2).cpu()
    neg = lp.neg_index(sim)
    pa = lp.CorrParams(self_shift=0.18, self_weight=1.0, neg_shift=0.46, neg_weight=1.0)
    pg = lp.CorrParams(self_shift=0.5, self_weight=1.0, neg_shift=3.0, neg_weight=1.0)
    c = [d_ * 2 - 1 for d_ in draws]                              # utils/image.py:343-344
    with torch.no_grad():
        want = (lp.correlation_loss(feat.cpu(), s0, neg, c[0], c[1], pa) + lp.correlation_loss(feat.cpu(), s1, neg, c[2], c[3], pa))
        want = want + 0.01 * (lp.geo_correlation_loss(depth.clone(), s0, ro, rd, neg, pg) +
                              lp.geo_correlation_loss(depth.clone(), s1, ro, rd, neg, pg))
    assert abs(float(loss) - float(want)) <= 1e-4 * (1 + abs(float(want))), (float(loss), float(want))
    # determinism of the whole step
    _, _, _, _, loss2, grads2 = _c4_step("fp32", manifest)
    assert float(loss2) == float(loss) and all(torch.equal(grads[k], grads2[k]) for k in grads)


def test_c4_per_gpu_workload_bf16_vs_fp32(manifest):
    _, _, _, _, loss32, g32 = _c4_step("fp32", manifest)
    _, _, _, _, loss16, g16 = _c4_step("bf16", manifest)
    assert torch.isfinite(loss16)
    assert abs(float(loss16) - float(loss32)) <= 3e-2 * (1 + abs(float(loss32))), (float(loss16), float(loss32))
    for k in g32:
        a, b = g32[k].flatten().double(), g16[k].flatten().double()
        cos = float((a @ b) / (a.norm() * b.norm() + 1e-300))
        # (a statistic of the step's 2 x 121 sample coordinates: 0.973-0.995 over the draws seen, per tensor)
        assert cos > 0.96, f"{k}: bf16 gradient direction differs from fp32 (cos {cos:.4f})"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_c4_direct_loss_gradients_equal_the_autograd_formulation(manifest, precision, monkeypatch):
    """The step sums the loss launches' gradients itself and enters autograd once, at the rendered semantic maps
    (sharding._losses_direct: weights on the kernels' weights, negatives from nsos_similarity_negatives); the formulation that
    mirrors the reference's trainer line by line (w * (L(s0) + L(s1)) + ..., loss.backward(); NSOS_STEP_AUTOGRAD_LOSSES=1) must
    give the same loss and parameter gradients up to the rounding of the folded weights."""
    _, _, _, _, loss_d, g_d = _c4_step(precision, manifest)
    monkeypatch.setenv("NSOS_STEP_AUTOGRAD_LOSSES", "1")
    _, _, _, _, loss_a, g_a = _c4_step(precision, manifest)
    assert abs(float(loss_d) - float(loss_a)) <= 2e-6 * (1 + abs(float(loss_a))), (float(loss_d), float(loss_a))
    for k in g_a:
        assert float((g_d[k] - g_a[k]).abs().max()) <= 2e-5 * float(g_a[k].abs().max()), k


def test_contrastive_gradient_reaches_the_class_tokens_on_both_loss_paths(manifest, monkeypatch):
    """engines/trainer.py:168-170 back-propagates contrast_l into the feature extractor through `cls_`: a `cls_tokens` that
    requires grad receives the same gradient from the direct path as from the line-by-line autograd formulation (ADVICE r03:
    the direct path evaluated the term under no_grad and dropped it)."""
    got = {}
    for mode in ("", "1"):
        monkeypatch.setenv("NSOS_STEP_AUTOGRAD_LOSSES", mode)
        torch.manual_seed(0)
        net = nerf_sos_amd.NeRFNet(N_samples=16, N_importance=16, perturb=1.0, raw_noise_std=1.0, **CFGS["semcoord"]).to(DEV)
        for n_, p_ in net.named_parameters():
            p_.requires_grad = "semantic_linear" in n_
        net.train()
        B = 3
        rays = syn.synthetic_patches(B, 64, 6, seed=0, device=DEV)
        feat = torch.randn(B, 384, 14, 14, generator=torch.Generator().manual_seed(1)).to(DEV)
        cls_ = torch.randn(B, 384, generator=torch.Generator().manual_seed(2)).to(DEV).requires_grad_(True)
        corr, geo = nerf_sos_amd.CorrelationLoss(_loss_args()), nerf_sos_amd.GeoCorrelationLoss(_loss_args())
        con = nerf_sos_amd.NeRFContrastive(device=DEV)
        torch.manual_seed(7)
        loss = sharding.sharded_patch_step(net, rays, (syn.NEAR, syn.FAR), B, feat, cls_, corr, geo, step=1, seed=3,
                                           contrast_loss=con, contrast_w=0.01)
        assert cls_.grad is not None and float(cls_.grad.abs().max()) > 0, f"mode {mode!r}: no gradient reached cls_"
        got[mode] = (float(loss), cls_.grad.clone())
    assert abs(got[""][0] - got["1"][0]) <= 2e-6 * (1 + abs(got["1"][0]))
    assert float((got[""][1] - got["1"][1]).abs().max()) <= 1e-6 * float(got["1"][1].abs().max())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_c4_loss_overlap_does_not_change_a_bit(manifest, precision):
    """The appearance loss on a stream of its own (in the shadow of the geometric one, forward and backward) against the same
    step on one stream: identical loss and gradients, bit for bit."""
    _, _, _, _, la, ga = _c4_step(precision, manifest, overlap_losses=True)
    _, _, _, _, lb, gb = _c4_step(precision, manifest, overlap_losses=False)
    assert torch.equal(la, lb)
    assert all(torch.equal(ga[k], gb[k]) for k in ga)


def _graphed(precision, manifest, capture, overlap, B=2, contrast=True):
    torch.manual_seed(0)
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, perturb=1.0, raw_noise_std=1.0, ray_chunk=1 << 20,
                               **CFGS["semcoord"]).to(DEV)
    net.load_state_dict(ref_state("semcoord", manifest, peaky=True))
    for n_, p_ in net.named_parameters():
        p_.requires_grad = "semantic_linear" in n_
    net.train()
    net.mlp_precision = precision
    net.rng, net.rng_seed = "philox", 5
    opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=5e-4, fused=True, capturable=True)
    rays = syn.synthetic_patches(B, 64, 6, seed=0, device=DEV)
    feat = torch.randn(B, 384, 14, 14, generator=torch.Generator().manual_seed(1)).to(DEV)
    cls_ = (torch.randn(B, 384, generator=torch.Generator().manual_seed(2)) + 3 * torch.randn(1, 384, generator=torch.Generator().manual_seed(3))).to(DEV)
    corr, geo = nerf_sos_amd.CorrelationLoss(_loss_args()), nerf_sos_amd.GeoCorrelationLoss(_loss_args())
    con = nerf_sos_amd.NeRFContrastive(device=DEV) if contrast and B >= 2 else None
    g = nerf_sos_amd.GraphedPatchStep(net, opt, rays, (syn.NEAR, syn.FAR), feat, cls_, corr, geo, con, contrast_w=0.01, seed=9,
                                      overlap_losses=overlap, warmup=2, capture=capture)
    return net, g, (rays, feat, cls_)


@pytest.mark.parametrize("precision,overlap", [("bf16", True), ("bf16", False), ("fp32", True)])
def test_whole_training_step_as_one_graph_equals_eager_bit_for_bit(manifest, precision, overlap):
    """GraphedPatchStep: render (train mode, SAVE kernels, Philox draws from a device counter) -> appearance + geometric +
    contrastive losses (torch draws from a generator registered with the graph) -> semantic-head backward -> fused capturable
    Adam, captured once and replayed.  Against the very same function run eagerly (same generator, same counter): after 2
    warm-up + 5 steps the losses of every step and all parameters are identical bit for bit; the step really trains (loss
    and parameters move); a new batch loaded into the static buffers is what the next replay renders."""
    net_g, g, batch = _graphed(precision, manifest, True, overlap)
    net_e, e, _ = _graphed(precision, manifest, False, overlap)
    assert g.graph is not None and e.graph is None
    e.eager_step(); e.eager_step()                       # the graphed instance's two warm-up steps
    p0 = {n: p.detach().clone() for n, p in net_g.named_parameters() if p.requires_grad}
    lg, le = [], []
    for k in range(5):
        if k == 3:                                       # a different batch through the static buffers
            rays2 = syn.synthetic_patches(2, 64, 6, seed=1, device=DEV)
            g.load(rays2, batch[1] * 0.5, batch[2])
            e.load(rays2, batch[1] * 0.5, batch[2])
        lg.append(g().clone())
        le.append(e().clone())
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(lg, le)), (lg, le)
    assert len({float(x) for x in lg}) == 5, "every step draws new numbers and sees updated weights: five different losses"
    for (n, a), (_, b) in zip(net_g.named_parameters(), net_e.named_parameters()):
        assert torch.equal(a, b), n
    assert any(not torch.equal(p0[n], p) for n, p in net_g.named_parameters() if p.requires_grad)
    assert int(net_g.rng_counter.item()) == 7 and int(net_e.rng_counter.item()) == 7       # one draw launch per step


def test_device_rng_counter_draws_equal_host_counter_draws():
    """nsos_render_draws_counted with the counter in device memory draws what nsos_render_draws draws for call = 1, 2, 3."""
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    for call in (1, 2, 3):
        a = ops.render_draws(77, call, 300, 64, 128, DEV)
        b = ops.render_draws(77, cnt, 300, 64, 128, DEV)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and int(cnt.item()) == call
    assert not torch.equal(ops.render_draws(77, 1, 300, 64, 128, DEV)[0], ops.render_draws(77, 2, 300, 64, 128, DEV)[0])


@pytest.mark.parametrize("cfg", ["nosem", "semcoord"])
def test_density_export_grid(manifest, cfg):
    """SURVEY 3.3 / engines/eval.py:285-300 at its own size: 256^3 grid points x 14, zero view directions, through the fine net's
    point-query entry.  A seeded sample of the grid against the CPU port's point query (fp32 band of the parity tests), the
    slab loop against one direct call, and the 16-bit precisions through the same entry (they used to fall back to fp32)."""
    from oracle import torch_port as tp
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, **CFGS[cfg]).to(DEV).eval()
    sd = ref_state(cfg, manifest, peaky=False)
    net.load_state_dict(sd)
    sigma = nerf_sos_amd.export_density(net)
    assert sigma.shape == (256, 256, 256) and torch.isfinite(sigma).all() and float(sigma.min()) >= 0 and float(sigma.max()) > 0
    lin = torch.linspace(-1, 1, 256)
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(0, 256, (8192, 3), generator=g)
    idx[:8] = torch.tensor([[0, 0, 0], [255, 255, 255], [0, 255, 0], [255, 0, 0], [0, 0, 255], [63, 64, 65], [64, 0, 0], [127, 128, 255]])
    pts = torch.stack([lin[idx[:, 0]], lin[idx[:, 1]], lin[idx[:, 2]]], -1) * 14
    pcfg = tp.PortConfig(use_semantics=CFGS[cfg]["use_semantics"], sem_with_coord=CFGS[cfg].get("sem_with_coord", False))
    with torch.no_grad():
        raw_ref = tp.point_query({k: v.cpu() for k, v in sd.items()}, "nerf_fine", pts[:, None, :], torch.zeros_like(pts)[:, None, :], pcfg)[:, 0]
        raw = net.nerf_fine(pts.to(DEV), viewdirs=torch.zeros(8192, 3, device=DEV))
    assert raw.shape == raw_ref.shape
    scale = 1 + raw_ref.abs()
    assert float(((raw.cpu() - raw_ref).abs() / scale).max()) <= 2e-5
    got = sigma[idx[:, 0].to(DEV), idx[:, 1].to(DEV), idx[:, 2].to(DEV)]
    assert torch.equal(got, raw[:, -1].clamp_min(0))            # the slab loop = one direct call of the same points
    for prec, tol in (("fp16x3", 2e-5), ("fp16", 2e-2), ("bf16", 1e-1)):
        net.mlp_precision = prec
        assert net.nerf_fine.mlp_precision == prec
        with torch.no_grad():
            lp = net.nerf_fine(pts.to(DEV), viewdirs=torch.zeros(8192, 3, device=DEV))
            z = torch.zeros(8192, 1, device=DEV)
            direct = ops.mlp_forward_rays_lp(net.nerf_fine.packed_weights(prec), net.nerf_fine.sem_mode, prec, pts.to(DEV),
                                             torch.zeros(8192, 3, device=DEV), torch.zeros(8192, 3, device=DEV), z)[:, 0]
        assert torch.equal(lp, direct)
        err = float(((lp - raw).abs() / (1 + raw.abs())).max())
        assert err <= tol, (prec, err)
        if prec != "fp16x3":
            assert not torch.equal(lp, raw)                     # it IS the 16-bit kernel now
    net.mlp_precision = "fp32"
    with pytest.raises(ValueError):
        net.mlp_precision = "fp8"


@pytest.mark.timeout(900)
def test_bench_plain_run_and_dump_outputs(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` (the headline, C2): ONE JSON line with the headline fields and none of what --full
    adds; `--dump-outputs DIR` writes the last timed step's render as float .npy files, bit for bit the same from run to run."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(d)], cwd=tmp_path, capture_output=True, text=True, timeout=800)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["dtype"] == "f32" and line["unit"] == "rays/s" and line["higher_is_better"] is True
        assert line["value"] > 0 and line["ms_per_step"] > 0 and line["metric"].startswith("rays/sec")
        assert not {"variants", "cpu_baseline", "parity", "replayed_as_hip_graph"} & set(line), sorted(line)
        assert not (tmp_path / "bench_detail.json").exists()
        arrays = {p.name[:-4]: np.load(p) for p in d.iterdir()}
        assert {"rgb", "depth", "acc", "rgb0", "depth0", "acc0"} <= set(arrays), sorted(arrays)
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(p.stat().st_size for p in d.iterdir()) <= 64 * 10**6
        assert arrays["rgb"].shape == (4096, 3) and np.isfinite(arrays["rgb"]).all()
        outs.append(arrays)
    for k, a in outs[0].items():
        assert np.array_equal(a, outs[1][k]), k

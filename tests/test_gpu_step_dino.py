"""GPU (-m gpu): the training step with the DINO extractor inside -- `sharding.sharded_patch_step(dino=...)`,
`GraphedPatchStep(dino=...)` and the `out=` buffers of `DinoViT.patch_features` that connect them.

Everything here is an identity: the step with `dino=` launches the same kernels on the same inputs as render -> patch_features ->
step-with-features, so losses, gradients, parameters and features are compared BIT FOR BIT (the two-rank comparison excepted: summing
the ranks' gradients re-orders fp32 additions; its tolerances are those of tests/test_gpu_sharded.py's two-rank test).

Shapes: the synthetic net and 16 x 16 patches of tests/test_gpu_sharded.py (64 + 128 samples), the extractor's weights from
tests/dino_weights.py, patch_stride = 2, B = 2 patches (the fewest with a negative) unless a test says why it needs another.
"""
import functools
import os
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import dino_weights as dw

pytestmark = pytest.mark.gpu
P, STRIDE = 16, 2
# tests/test_gpu_sharded.py::_worker, the two-rank step against the single-process one (shipped architecture): the loss within
# 1e-6 * (1 + |loss|), every gradient within 2e-5 of its largest entry
TWO_RANK_LOSS_RTOL, TWO_RANK_GRAD_OF_SCALE = 1e-6, 2e-5


def _loss_args():
    return types.SimpleNamespace(rand_neg=False, self_corr_w=0, use_sim_matrix=True, patch_stride=6,
                                 app_corr_params=["0.18", "1", "0.46", "1"], geo_corr_params=["0.5", "1", "3", "1"])


def _losses():
    import nerf_sos_amd
    return nerf_sos_amd.CorrelationLoss(_loss_args()), nerf_sos_amd.GeoCorrelationLoss(_loss_args())


def _net(dev, draws=False):
    """The shipped 8 x 256 net under the frozen-backbone recipe, as tests/test_gpu_sharded.py builds it; draws=True: train-mode
    jitter and noise from the package's Philox stream (what a captured step needs)."""
    import nerf_sos_amd
    torch.manual_seed(0)
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, perturb=0.0, raw_noise_std=0.0, ray_chunk=1 << 20,
                               use_semantics=True, sem_with_coord=True).to(dev)
    for n_, p_ in net.named_parameters():
        p_.requires_grad = "semantic_linear" in n_
    net.train()
    net.rng, net.rng_seed = "philox", 3
    if draws:
        net.perturb, net.raw_noise_std = 1.0, 1.0
        net.render_kwargs_train.update(perturb=1.0, raw_noise_std=1.0)
    return net


@functools.lru_cache(maxsize=None)
def _state():
    return dw.make_state("wide", 11)


def _dino(dev, precision="fp32"):
    import nerf_sos_amd
    m = nerf_sos_amd.DinoViT(precision)
    m.load_state_dict(_state())
    return m.to(dev)


def _rays(B, dev, seed=5):
    from nerf_sos_amd import synthetic as syn
    return syn.synthetic_patches(B, P, 6, seed=seed, device=dev)


def _bounds():
    from nerf_sos_amd import synthetic as syn
    return (syn.NEAR, syn.FAR)


def _adam(net):
    return torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=5e-3, fused=True, capturable=True)


# ------------------------------------------------------------------------------------------------ 1. the two-call form
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("autograd_losses", [False, True])
def test_step_with_dino_equals_render_then_features_then_step(monkeypatch, autograd_losses, precision):
    """perturb = 0 and no noise pin the render; then render -> patch_features -> step(feat, cls) and step(dino=) are the same launches
    on the same inputs: loss and every gradient bit-identical, on the direct and on the autograd loss path."""
    from nerf_sos_amd import sharding
    monkeypatch.setenv("NSOS_STEP_AUTOGRAD_LOSSES", "1" if autograd_losses else "0")
    dev, B = torch.device("cuda:0"), 2
    rays, dino = _rays(B, dev), _dino(dev, precision)
    corr, geo = _losses()
    assert sharding._direct_losses(corr, geo) == (not autograd_losses)
    net_a, net_b = _net(dev), _net(dev)
    ret = net_a(rays, _bounds())
    f = dino.patch_features(ret["rgb"].detach(), STRIDE)
    loss_a = sharding.sharded_patch_step(net_a, rays, _bounds(), B, f["feats"], f["cls_tokens"], corr, geo, step=4, seed=9)
    timings = {}
    loss_b = sharding.sharded_patch_step(net_b, rays, _bounds(), B, None, None, corr, geo, step=4, seed=9, timings=timings,
                                         dino=dino, patch_stride=STRIDE)
    torch.cuda.synchronize()
    print(f"loss: two calls {float(loss_a)!r}, dino= {float(loss_b)!r}")
    assert torch.isfinite(loss_a) and torch.equal(loss_a, loss_b)
    n_grads = 0
    for (n_, a), (_, b) in zip(net_a.named_parameters(), net_b.named_parameters()):
        assert (a.grad is None) == (b.grad is None) == (not a.requires_grad), n_
        if a.grad is not None:
            assert torch.equal(a.grad, b.grad), (n_, float((a.grad - b.grad).abs().max()))
            n_grads += int(bool(a.grad.abs().max() > 0))
    assert n_grads >= 4                                     # (both semantic heads received a gradient: the comparison is not 0 == 0)
    # 'dino' sits between 'render' and 'gather', and 'render' ends where it begins
    (r0, r1), (d0, d1), (g0, _) = timings["render"][0], timings["dino"][0], timings["gather"][0]
    assert r1 is d0 and d1 is g0 and d0.elapsed_time(d1) > 0 and r0.elapsed_time(r1) > 0


def test_step_without_dino_records_no_dino_timing():
    from nerf_sos_amd import sharding
    dev, B = torch.device("cuda:0"), 2
    corr, geo = _losses()
    feat, cls_ = torch.randn(B, 384, 14, 14, device=dev), torch.randn(B, 384, device=dev)
    timings = {}
    sharding.sharded_patch_step(_net(dev), _rays(B, dev), _bounds(), B, feat, cls_, corr, geo, step=4, seed=9, timings=timings)
    assert "dino" not in timings and timings["render"][0][1] is timings["gather"][0][0]


# ------------------------------------------------------------------------------------ 2. the features follow the render
def test_graphed_step_features_are_those_of_the_render_it_just_made():
    import nerf_sos_amd
    dev, B = torch.device("cuda:0"), 2
    r1, r2 = _rays(B, dev, seed=5), _rays(B, dev, seed=6)
    net, twin = _net(dev), _net(dev)                       # perturb = 0, no noise: the render has no draws
    corr, geo = _losses()
    g = nerf_sos_amd.GraphedPatchStep(net, _adam(net), r1, _bounds(), None, None, corr, geo, seed=21, warmup=2,
                                      dino=_dino(dev), patch_stride=STRIDE)
    assert g.graph is not None and g.capture_fallback is None
    assert tuple(g.feat.shape) == (B, 196, 384) and tuple(g.feats.shape) == (B, 384, 14, 14) and tuple(g.cls.shape) == (B, 384)
    assert g.feats.data_ptr() == g.feat.data_ptr()
    ptrs = (g.feat.data_ptr(), g.cls.data_ptr())
    other = _dino(dev)                                     # an extractor of its own: nothing shared with the graph's

    def independent(rays):
        # the backbone is frozen, so `twin` (never stepped) renders the rgb the stepped net renders
        return other.patch_features(twin(rays, _bounds())["rgb"].detach(), STRIDE, want_attn=False)

    g()
    e1 = independent(r1)
    assert torch.equal(g.feat, e1["feat"]) and torch.equal(g.cls, e1["cls_"]) and torch.equal(g.feats, e1["feats"])
    with pytest.raises(ValueError, match="rays alone"):
        g.load(r2, e1["feats"], e1["cls_"])
    g.load(r2)
    g()
    e2 = independent(r2)
    assert torch.equal(g.feat, e2["feat"]) and torch.equal(g.cls, e2["cls_"])
    assert not torch.equal(g.feat, e1["feat"]) and not torch.equal(g.cls, e1["cls_"])    # not the warm-up's features, baked in
    assert (g.feat.data_ptr(), g.cls.data_ptr()) == ptrs and torch.isfinite(g.loss)


# --------------------------------------------------------------------------- 3. replay == eager, 5. the extractor stays frozen
@functools.lru_cache(maxsize=None)
def _twins(precision):
    """Two identically seeded (net, optimizer, extractor) triples with train-mode draws, one captured and one eager; three steps
    each.  Returns what tests 3 and 5 compare."""
    import nerf_sos_amd
    dev, B, warmup = torch.device("cuda:0"), 2, 2
    rays = _rays(B, dev)
    steps, nets, dinos, before = [], [], [], []
    for capture in (True, False):
        net, dino = _net(dev, draws=True), _dino(dev, precision)
        before.append({k: v.detach().clone() for k, v in dino.state_dict().items()})     # (before the warm-up steps too)
        corr, geo = _losses()
        steps.append(nerf_sos_amd.GraphedPatchStep(net, _adam(net), rays, _bounds(), None, None, corr, geo, seed=21, warmup=warmup,
                                                   capture=capture, dino=dino, patch_stride=STRIDE))
        nets.append(net), dinos.append(dino)
    graphed, eager = steps
    for _ in range(warmup):                                 # the captured twin's warm-up steps
        eager.eager_step()
    rec = []
    for _ in range(3):
        la, lb = graphed().clone(), eager().clone()
        rec.append((la, lb, graphed.feat.clone(), eager.feat.clone(), graphed.cls.clone(), eager.cls.clone()))
    torch.cuda.synchronize()
    return dict(captured=graphed.graph is not None, fallback=graphed.capture_fallback, eager_graph=eager.graph, rec=rec, nets=nets,
                dinos=dinos, before=before)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_replayed_step_with_dino_equals_the_eager_step(precision):
    t = _twins(precision)
    assert t["captured"] and t["fallback"] is None and t["eager_graph"] is None
    for k, (la, lb, fa, fb, ca, cb) in enumerate(t["rec"]):
        print(f"step {k}: loss {float(la)!r} (replayed) vs {float(lb)!r} (eager)")
        assert torch.isfinite(la) and torch.equal(la, lb), k
        assert torch.equal(fa, fb) and torch.equal(ca, cb), k
    feats = [r[2] for r in t["rec"]]
    assert not torch.equal(feats[0], feats[1]) and not torch.equal(feats[1], feats[2])   # new draws, new render, new features
    moved = 0
    for (n_, a), (_, b) in zip(t["nets"][0].named_parameters(), t["nets"][1].named_parameters()):
        assert torch.equal(a, b), (n_, float((a.detach() - b.detach()).abs().max()))
        moved += int(a.requires_grad)
    assert moved >= 4


def test_extractor_stays_frozen_through_the_steps():
    t = _twins("fp32")
    for dino, before in zip(t["dinos"], t["before"]):
        after = dino.state_dict()
        assert list(after) == list(before) and len(before) == 150
        for k, v in before.items():
            assert torch.equal(after[k], v), k
        for n_, p_ in dino.named_parameters():
            assert p_.grad is None and not p_.requires_grad, n_


# ------------------------------------------------------------------------------------------------------------- 4. out=
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_patch_features_writes_into_the_callers_buffers(precision):
    dev, B = torch.device("cuda:0"), 2
    dino = _dino(dev, precision)
    x = torch.rand(B, P, P, 3, device=dev, generator=torch.Generator(dev).manual_seed(1))
    want = dino.patch_features(x, STRIDE)
    out = {"feat": torch.full((B, 196, 384), float("nan"), device=dev), "cls_": torch.full((B, 384), float("nan"), device=dev)}
    got = dino.patch_features(x, STRIDE, want_attn=False, out=out)
    assert got["feat"] is out["feat"] and got["cls_"] is out["cls_"] and got["cls_tokens"] is out["cls_"] and "attn" not in got
    assert got["feat"].data_ptr() == out["feat"].data_ptr() == got["feats"].data_ptr() and got["cls_"].data_ptr() == out["cls_"].data_ptr()
    assert torch.equal(out["feat"], want["feat"]) and torch.equal(out["cls_"], want["cls_"]) and torch.equal(got["feats"], want["feats"])
    via = dino.get_vit_attn_feat(x.permute(0, 3, 1, 2).contiguous(), out=out)     # the reference's entry point takes it too
    assert via["feat"] is out["feat"] and tuple(via["attn"].shape) == (B, 1, 196)
    good = lambda: {"feat": torch.empty(B, 196, 384, device=dev), "cls_": torch.empty(B, 384, device=dev)}   # noqa: E731
    bad = [dict(good(), feat=torch.empty(B + 1, 196, 384, device=dev)), dict(good(), cls_=torch.empty(B, 383, device=dev)),
           dict(good(), feat=torch.empty(B, 196, 384, device=dev, dtype=torch.float16)),
           dict(good(), cls_=torch.empty(B, 384, device=dev, dtype=torch.float64)),
           dict(good(), feat=torch.empty(B, 196, 384)), dict(good(), cls_=torch.empty(B, 384)),
           dict(good(), feat=torch.empty(B, 384, 196, device=dev).permute(0, 2, 1))]
    for o in bad:
        with pytest.raises(ValueError):
            dino.patch_features(x, STRIDE, out=o)


# ----------------------------------------------------------------------------------- 6. two ranks over gloo, one GPU
def _rank_worker(rank, world, port, q):
    """Both cases in one pair of processes.  B = 3: rank 0 owns patches 0 and 2, rank 1 patch 1; each rank passes dino=; loss and
    summed gradients against the single-process dino= step.  B = 1: rank 1 owns nothing, calls nothing on the extractor and
    contributes empty slots; the step completes with a finite loss on both ranks."""
    from nerf_sos_amd import sharding
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        why = {3: [], 1: []}
        solo = [dist.new_group([r]) for r in range(world)][rank]      # every rank creates every group, in the same order
        dino = _dino(dev)
        calls = []
        inner = dino.patch_features
        dino.patch_features = lambda *a, **k: (calls.append(int(a[0].shape[0])), inner(*a, **k))[1]
        for B in (3, 1):
            rays = _rays(B, dev)
            own = sharding.local_patches(B, rank, world)
            corr, geo = _losses()
            net = _net(dev)
            del calls[:]
            loss = sharding.sharded_patch_step(net, rays[:, own].contiguous(), _bounds(), B, None, None, corr, geo, step=4, seed=9,
                                               dino=dino, patch_stride=STRIDE)
            if calls != ([len(own)] if own else []):
                why[B].append(f"rank {rank} owns {len(own)} patches, extractor calls {calls}")
            if not bool(torch.isfinite(loss)):
                why[B].append(f"loss {float(loss)}")
            if B == 1:
                continue
            ref_net = _net(dev)
            ref_loss = sharding.sharded_patch_step(ref_net, rays, _bounds(), B, None, None, corr, geo, step=4, seed=9, group=solo,
                                                   dino=dino, patch_stride=STRIDE)
            if abs(float(loss) - float(ref_loss)) > TWO_RANK_LOSS_RTOL * (1 + abs(float(ref_loss))):
                why[B].append(f"loss {float(loss)!r} vs single-process {float(ref_loss)!r}")
            for (n_, p_), (_, r_) in zip(net.named_parameters(), ref_net.named_parameters()):
                if not p_.requires_grad:
                    continue
                scale = float(r_.grad.abs().max()) + 1e-30
                err = float((p_.grad - r_.grad).abs().max()) / scale
                if err > TWO_RANK_GRAD_OF_SCALE:
                    why[B].append(f"grad {n_}: {err:.2e} of scale")
        q.put((rank, {B: "; ".join(w) for B, w in why.items()}))
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def _two_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000) + 431
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=400) for _ in procs)
        for p in procs:
            p.join(60)
    finally:
        for p in procs:
            if p.is_alive():                               # a hung collective must not outlive the test (our own children)
                p.kill()
    return res


@pytest.mark.timeout(600)
def test_two_ranks_with_dino_equal_the_single_process_step():
    res = _two_ranks()
    assert {r: res[r][3] for r in (0, 1)} == {0: "", 1: ""}, res


@pytest.mark.timeout(600)
def test_rank_without_patches_skips_the_extractor_and_the_step_completes():
    res = _two_ranks()
    assert {r: res[r][1] for r in (0, 1)} == {0: "", 1: ""}, res

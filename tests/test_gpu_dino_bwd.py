"""GPU: DINO's backward to the input image (csrc/dino_vit_bwd.hip) against the fp64 autograd gradient of the real reference
(tests/golden/make_goldens_dino_bwd.py).

The bar is the project's (tests/dino_fixture.py::bar): max |gpu - fp64| <= max(4 * e32, 1e-6 * scale), e32 = the reference's own fp32
autograd distance from fp64 on that case, scale = max |fp64|, capped at 1e-4 * scale; every case, every element.  Each comparison
prints its figures (the ratio to e32 among them) before it asserts."""
import functools
import types

import numpy as np
import pytest
import torch

import dino_bwd_fixture as bfx
import dino_fixture as fx
import dino_weights as dw
from helpers import state_sha

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_models = {}


def state(kind):
    sd = dw.make_state(kind, fx.meta()["seeds"][kind])
    assert bfx.meta()["seeds"][kind] == fx.meta()["seeds"][kind] and state_sha(sd) == fx.meta()["state_sha256"][kind]
    return sd


def model(kind):
    import nerf_sos_amd
    if kind not in _models:
        m = nerf_sos_amd.DinoViT()
        m.load_state_dict(state(kind))
        _models[kind] = m.to(DEV)
    return _models[kind]


def features(m, x, c, **kw):
    if c["mode"] == "patch":
        return m.patch_features(x, c["stride"], **kw)
    return m.get_vit_attn_feat(x, prepared=c["mode"] == "prepared", **kw)


def flags_of(c, nhwc=True):
    from nerf_sos_amd import ops
    if c["mode"] == "patch":
        return ops.DINO_STEP1 | (ops.DINO_NHWC if nhwc else 0), c["stride"]
    return (ops.DINO_PREPARED if c["mode"] == "prepared" else 0), 0


def raw_backward(c, x=None, g_feat="case", g_cls="case", nhwc=True, want_g_blocks=False):
    """ops.dino_forward(saved=) then ops.dino_backward on a case's tensors (or on `x` / explicit upstream gradients)."""
    from nerf_sos_amd import ops
    m = model(c["kind"])
    x = torch.from_numpy(c["input"]).to(DEV) if x is None else x
    g_feat = torch.from_numpy(c["g_feat"]).to(DEV)[:x.shape[0]] if isinstance(g_feat, str) else g_feat
    g_cls = torch.from_numpy(c["g_cls"]).to(DEV)[:x.shape[0]] if isinstance(g_cls, str) else g_cls
    flags, stride = flags_of(c, nhwc)
    B = int(x.shape[0])
    saved = torch.empty(ops.dino_saved_floats(B), device=DEV)
    ops.dino_forward(x, m.packed_weights(), flags, stride, want_attn=False, saved=saved)
    return ops.dino_backward(tuple(x.shape), flags, stride, m.packed_weights(), m.packed_weights_backward(), saved, g_feat, g_cls,
                             want_g_blocks=want_g_blocks)


def worst(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())


# ------------------------------------------------------------------------------------------------ 1. every element against fp64
@pytest.mark.parametrize("ci", range(6))
def test_input_gradient_against_fp64(ci):
    c = bfx.case(ci)
    x = torch.from_numpy(c["input"]).to(DEV).requires_grad_()
    out = features(model(c["kind"]), x, c, differentiable=True)
    loss = (out["feat"] * torch.from_numpy(c["g_feat"]).to(DEV)).sum() + (out["cls_"] * torch.from_numpy(c["g_cls"]).to(DEV)).sum()
    loss.backward()
    got = x.grad.cpu().numpy()
    bar = bfx.bar(c["e32"], c["scale"])
    err = worst(got, c["g64"])
    print(f"case {ci} {c['kind']} {c['mode']}: |gpu-fp64| {err:.3e}, e32 {c['e32']:.3e}, scale {c['scale']:.3e}, bar {bar:.3e}, "
          f"ratio to e32 {err / c['e32']:.2f}")
    assert got.shape == c["g64"].shape and np.isfinite(got).all()
    assert bar <= 1e-4 * c["scale"]
    assert err <= bar, (err, bar)
    if ci == 4:   # source pixels that no pixel of the 224 x 224 image reads: exactly 0.0, and written
        unmapped = c["g64"] == 0.0
        assert unmapped.sum() > 0 and (got[unmapped] == 0.0).all()


# ------------------------------------------------------------------------------------------------ 2. the residual-stream gradient
def test_g_blocks_localise():
    c = bfx.case(0)
    g = raw_backward(c, want_g_blocks=True)
    assert g["g_blocks"].shape == (12, c["B"], 197, 384)
    gb = g["g_blocks"].cpu().numpy()
    assert worst(g["g_input"].cpu().numpy(), c["g64"]) <= bfx.bar(c["e32"], c["scale"])
    for k, (g64, e32, scale) in bfx.block_grads().items():
        err, bar = worst(gb[k][0][:g64.shape[0]], g64), bfx.bar(e32, scale)
        print(f"block {k}: |gpu-fp64| {err:.3e}, e32 {e32:.3e}, scale {scale:.3e}, bar {bar:.3e}, ratio to e32 {err / e32:.2f}")
        assert err <= bar, (k, err, bar)


# ------------------------------------------------------------------------------------------------ 3. one upstream gradient alone
def test_a_missing_upstream_gradient_is_zeros():
    c = bfx.case(0)
    zf, zc = torch.zeros(c["B"], 196, 384, device=DEV), torch.zeros(c["B"], 384, device=DEV)
    for a, b in ((dict(g_cls=None), dict(g_cls=zc)), (dict(g_feat=None), dict(g_feat=zf))):
        ga, gb = raw_backward(c, want_g_blocks=True, **a), raw_backward(c, want_g_blocks=True, **b)
        assert torch.equal(ga["g_input"], gb["g_input"]) and torch.equal(ga["g_blocks"], gb["g_blocks"])
        assert float(ga["g_input"].abs().max()) > 0
    # autograd hands None for an output that took no part in the loss: feat alone, then cls_ alone
    m = model(c["kind"])
    for key, gf, gc in (("feat", "case", zc), ("cls_", zf, "case")):
        x = torch.from_numpy(c["input"]).to(DEV).requires_grad_()
        out = m.patch_features(x, c["stride"], differentiable=True)
        up = torch.from_numpy(c["g_feat" if key == "feat" else "g_cls"]).to(DEV)
        (out[key] * up).sum().backward()
        assert torch.equal(x.grad, raw_backward(c, g_feat=gf, g_cls=gc)["g_input"]), key


# ------------------------------------------------------------------------------------------------ 4. determinism, batch invariance
def test_determinism_and_batch_invariance():
    c = bfx.case(2)                                            # B = 3
    x = torch.from_numpy(c["input"]).to(DEV)
    a = raw_backward(c, want_g_blocks=True)
    b = raw_backward(c, want_g_blocks=True)
    assert torch.equal(a["g_input"], b["g_input"]) and torch.equal(a["g_blocks"], b["g_blocks"])
    for i in (0, c["B"] - 1):
        one = raw_backward(c, x=x[i:i + 1].contiguous(), g_feat=torch.from_numpy(c["g_feat"][i:i + 1]).to(DEV),
                           g_cls=torch.from_numpy(c["g_cls"][i:i + 1]).to(DEV), want_g_blocks=True)
        assert torch.equal(one["g_input"][0], a["g_input"][i]), i
        assert torch.equal(one["g_blocks"][:, 0], a["g_blocks"][:, i]), i


# ------------------------------------------------------------------------------------------------ 5. autograd wiring
def _user_loss(out, contrast):
    return (out["feats"] ** 2).mean() + contrast(out["cls_tokens"])


def test_autograd_wiring_against_the_port():
    import nerf_sos_amd
    from oracle import losses_port
    c = bfx.case(0)
    m = model(c["kind"])
    x = torch.from_numpy(c["input"]).to(DEV).requires_grad_()
    plain = m.patch_features(x.detach(), c["stride"])
    out = m.patch_features(x, c["stride"], differentiable=True)
    for k in fx.OUTPUTS:
        assert torch.equal(out[k], plain[k]), k                # the same forward bits in both modes
    assert out["feat"].requires_grad and out["cls_"].requires_grad and out["feats"].requires_grad and not out["attn"].requires_grad
    assert not m.patch_features(x, c["stride"])["feat"].requires_grad            # the default stays detached
    assert not m.patch_features(x.detach(), c["stride"], differentiable=True)["feat"].requires_grad
    _user_loss(out, nerf_sos_amd.NeRFContrastive()).backward()
    sd = {k: v.to(DEV) for k, v in state(c["kind"]).items()}
    xr = torch.from_numpy(c["input"]).to(DEV).requires_grad_()
    ref = bfx.port_features(sd, xr, c)
    ref["feats"] = ref["feat"].reshape(c["B"], 14, 14, 384).permute(0, 3, 1, 2)
    ref["cls_tokens"] = ref["cls_"]
    _user_loss(ref, losses_port.nerf_contrastive).backward()
    scale = float(xr.grad.abs().max())
    bar = bfx.bar(c["e32"], c["scale"]) / c["scale"] * scale   # the bar of case 0, scaled to this gradient
    err = float((x.grad - xr.grad).abs().max())
    print(f"user loss: |hip - port autograd on the GPU| {err:.3e}, scale {scale:.3e}, bar {bar:.3e}")
    assert scale > 0 and err <= bar, (err, bar)


# ------------------------------------------------------------------------------------------------ 6. both layouts
def test_channels_first_gives_the_same_bits():
    c = bfx.case(0)
    x = torch.from_numpy(c["input"]).to(DEV)
    a = raw_backward(c)["g_input"]
    b = raw_backward(c, x=x.permute(0, 3, 1, 2).contiguous(), nhwc=False)["g_input"]
    assert b.shape == (c["B"], 3, c["P"], c["P"]) and torch.equal(a, b.permute(0, 2, 3, 1))
    xc = x.permute(0, 3, 1, 2).contiguous().requires_grad_()   # and through the module, which picks the layout from the shape
    out = model(c["kind"]).patch_features(xc, c["stride"], differentiable=True)
    ((out["feat"] * torch.from_numpy(c["g_feat"]).to(DEV)).sum() + (out["cls_"] * torch.from_numpy(c["g_cls"]).to(DEV)).sum()).backward()
    assert torch.equal(xc.grad, b)


# ------------------------------------------------------------------------------------------------ 7. capture
def test_capture_forward_and_backward():
    import nerf_sos_amd
    c = bfx.case(0)
    m = nerf_sos_amd.DinoViT()
    m.load_state_dict(state(c["kind"]))
    m = m.to(DEV)
    m.prepare(c["B"], backward=True)                           # both packed streams and both workspaces: the capture makes none
    ptrs = (m._packed.data_ptr(), m._packed_bwd.data_ptr(), m._ws(c["B"], torch.device(DEV)).data_ptr(),
            m._ws_bwd(c["B"], torch.device(DEV)).data_ptr())
    x, gf, gc = (torch.from_numpy(c[k]).to(DEV) for k in ("input", "g_feat", "g_cls"))
    sx, sgf, sgc = torch.zeros_like(x).requires_grad_(), torch.zeros_like(gf), torch.zeros_like(gc)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = m.patch_features(sx, c["stride"], differentiable=True, want_attn=False)
            (grad,) = torch.autograd.grad((out["feat"] * sgf).sum() + (out["cls_"] * sgc).sum(), sx)
    torch.cuda.current_stream().wait_stream(s)
    with torch.no_grad():
        sx.copy_(x), sgf.copy_(gf), sgc.copy_(gc)
    g.replay()
    torch.cuda.synchronize()
    replayed = grad.clone()
    assert ptrs == (m._packed.data_ptr(), m._packed_bwd.data_ptr(), m._ws(c["B"], torch.device(DEV)).data_ptr(),
                    m._ws_bwd(c["B"], torch.device(DEV)).data_ptr())
    xe = x.clone().requires_grad_()
    oe = m.patch_features(xe, c["stride"], differentiable=True, want_attn=False)
    ((oe["feat"] * gf).sum() + (oe["cls_"] * gc).sum()).backward()
    assert torch.equal(replayed, xe.grad) and torch.equal(out["feat"], oe["feat"])
    assert worst(replayed.cpu().numpy(), c["g64"]) <= bfx.bar(c["e32"], c["scale"])


# ------------------------------------------------------------------------------------------------ 8. the training step
P, STRIDE = 16, 2


def _loss_args():
    return types.SimpleNamespace(rand_neg=False, self_corr_w=0, use_sim_matrix=True, patch_stride=6,
                                 app_corr_params=["0.18", "1", "0.46", "1"], geo_corr_params=["0.5", "1", "3", "1"])


def _net(dev):
    """The shipped 8 x 256 net of tests/test_gpu_step_dino.py with EVERY parameter trainable (a field that is not frozen)."""
    import nerf_sos_amd
    torch.manual_seed(0)
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, perturb=0.0, raw_noise_std=0.0, ray_chunk=1 << 20,
                               use_semantics=True, sem_with_coord=True).to(dev)
    net.train()
    net.rng, net.rng_seed = "philox", 3
    return net


@functools.lru_cache(maxsize=None)
def _step_dino():
    import nerf_sos_amd
    m = nerf_sos_amd.DinoViT()
    m.load_state_dict(dw.make_state("wide", 11))
    return m.to(DEV)


def _step(B, **kw):
    import nerf_sos_amd
    from nerf_sos_amd import sharding
    from nerf_sos_amd import synthetic as syn
    dev = torch.device(DEV)
    net = _net(dev)
    rays = syn.synthetic_patches(B, P, 6, seed=5, device=dev)
    corr, geo = nerf_sos_amd.CorrelationLoss(_loss_args()), nerf_sos_amd.GeoCorrelationLoss(_loss_args())
    loss = sharding.sharded_patch_step(net, rays, (syn.NEAR, syn.FAR), B, None, None, corr, geo, step=4, seed=9,
                                       contrast_loss=nerf_sos_amd.NeRFContrastive(), contrast_w=1.0, dino=_step_dino(), patch_stride=STRIDE, **kw)
    return net, loss


def _rgb_weight(net):
    """The colour head of the FINE network: ret["rgb"] is the fine render, and no other loss of the step reaches this matrix."""
    return dict(net.named_parameters())["nerf_fine.mlp.rgb_linear.weight"]


@pytest.mark.parametrize("B", [2, 3])
def test_step_with_dino_grad(B):
    """B = 2 (the fewest patches with a negative): the step with dino_grad=True is the hand-written sequence bit for bit, and
    dino_grad=False is the call without the keyword.  Whether the gradient DIFFERS from the forward-only run cannot be asked at
    B = 2: with two patches the contrastive term's maximum and minimum are the same off-diagonal entry, -log(max / (max + min)) is the
    constant log 2 and its gradient is exactly zero (measured: max |rgb_linear.weight.grad| 0.0 with and without dino_grad).  B = 3 is
    the fewest at which the term has a gradient (measured: 1.545e-01 against 0.0), so the same checks run there with that one added."""
    import nerf_sos_amd
    from nerf_sos_amd import synthetic as syn
    net_t, loss_t = _step(B, dino_grad=True)
    net_f, loss_f = _step(B, dino_grad=False)
    net_d, loss_d = _step(B)
    # dino_grad=False is the call without the keyword, bit for bit
    assert torch.equal(loss_f, loss_d)
    for (n_, a), (_, b) in zip(net_f.named_parameters(), net_d.named_parameters()):
        assert (a.grad is None) == (b.grad is None) and (a.grad is None or torch.equal(a.grad, b.grad)), n_
    # dino_grad=True is render -> patch_features(differentiable=True) -> contrastive -> backward on the rgb branch
    dev = torch.device(DEV)
    net_h = _net(dev)
    ret = net_h(syn.synthetic_patches(B, P, 6, seed=5, device=dev), (syn.NEAR, syn.FAR), retraw=False)
    f = _step_dino().patch_features(ret["rgb"], STRIDE, differentiable=True, want_attn=False)
    (1.0 * nerf_sos_amd.NeRFContrastive()(f["cls_tokens"])).reshape(()).backward()
    gt, gh, gf = _rgb_weight(net_t).grad, _rgb_weight(net_h).grad, _rgb_weight(net_f).grad
    assert gt is not None and gh is not None and torch.isfinite(gt).all()
    print(f"B {B}: loss {float(loss_t)!r} (dino_grad) {float(loss_f)!r} (default); max |rgb_linear.weight.grad| {float(gt.abs().max()):.3e} "
          f"(dino_grad), {'None' if gf is None else format(float(gf.abs().max()), '.3e')} (default)")
    assert torch.equal(loss_t, loss_f)                          # the value of the loss does not depend on who differentiates it
    assert torch.equal(gt, gh)
    if B >= 3:                                                  # ... and it is not what the forward-only extractor leaves there
        assert float(gt.abs().max()) > 0 and (gf is None or not torch.equal(gt, gf))

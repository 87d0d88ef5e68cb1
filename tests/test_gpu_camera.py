"""The camera layer on the GPU (csrc/camera.hip, nerf_sos_amd.CameraTransformer): learnable per-camera poses that end the
ray-gradient path in rvec.grad / tvec.grad.  Goldens: tests/golden/camera.npz -- the REAL models/camera.py (fp32, CPU) and
tests/camera_port.py in fp64 (make_goldens_camera.py).

Accuracy bar (the one the DINO / LPIPS kernels carry): every element within max(4 e32, 1e-6 scale) of the fp64 result, capped at
1e-4 scale, where e32 is the fp32 reference's own distance from fp64 and scale the largest magnitude of that output."""
import os

import numpy as np
import pytest
import torch

import nerf_sos_amd
from nerf_sos_amd import io as nio, ops, synthetic as syn
from oracle import torch_port as tp
from helpers import CFGS, GENERIC_CASES, generic_state, ref_state
import camera_port as cp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
LAYER_CASES = ("n1_c1", "n63_c3_runs", "n64_c3_empty", "n64_c70_random", "n257_c3_one", "n257_c70_random", "n257_c3_farnorm",
               "n4099_c3_runs", "n4099_c70_random")
OUTS = ("out_o", "out_d", "g_rays_o", "g_rays_d", "g_rvec", "g_tvec")


def _case(g, name):
    ids = torch.from_numpy(g[f"{name}__ids"]).to(DEV)
    n = ids.numel()
    t = {k: torch.from_numpy(g[f"pool__{k}"][:n]).to(DEV) for k in ("rays_o", "rays_d", "G_o", "G_d")}
    t["ids"] = ids
    t["rvec"], t["tvec"] = torch.from_numpy(g[f"{name}__rvec"]).to(DEV), torch.from_numpy(g[f"{name}__tvec"]).to(DEV)
    return t


def _module(t, trainable=True):
    cam = nerf_sos_amd.CameraTransformer(t["rvec"].shape[0], trainable=trainable).to(DEV)
    cam.load_state_dict({"rvec": t["rvec"], "tvec": t["tvec"]})
    return cam


def _want64(g, name, k):
    if k in ("g_rvec", "g_tvec"):
        return g[f"{name}__ref64__{k}"]
    return g[f"{name}__ref32__{k}"].astype(np.float64) + g[f"{name}__res64__{k}"].astype(np.float64)


def _within_bar(got, g, name, k):
    want = _want64(g, name, k)
    scale = np.abs(want).max()
    e32 = float(g[f"{name}__e32"][OUTS.index(k)])
    bar = min(max(4 * e32, 1e-6 * scale), 1e-4 * scale)
    err = np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max()
    print(f"{name} {k}: err {err:.3e}  bar {bar:.3e}  (e32 {e32:.3e}, scale {scale:.3e})")
    assert err <= bar, f"{name}: {k} off by {err:.3e}, bar {bar:.3e} (e32 {e32:.3e}, scale {scale:.3e})"


def _run(cam, t, ray_grads=True, ids=None):
    """Forward + backward of sum(o' G_o) + sum(d' G_d) through cam.transform: (out [2,N,3], g_rays or None, g_rvec, g_tvec)."""
    rays = torch.stack([t["rays_o"], t["rays_d"]], 0).requires_grad_(ray_grads)
    out = cam.transform(rays, t["ids"] if ids is None else ids)
    grads = torch.autograd.grad(out, ([rays] if ray_grads else []) + [cam.rvec, cam.tvec], grad_outputs=torch.stack([t["G_o"], t["G_d"]], 0))
    return (out.detach(), grads[0], grads[1], grads[2]) if ray_grads else (out.detach(), None, grads[0], grads[1])


@pytest.mark.parametrize("name", LAYER_CASES)
def test_forward_and_backward_against_the_reference(golden, name):
    """rays_o' bit-equal to the reference's fp32 (one rounded add); rays_d', g_rvec, g_tvec, g_rays_d under the bar against fp64;
    g_rays_o is the upstream gradient itself; a camera without a ray gets exact zeros."""
    g = golden("camera")
    t = _case(g, name)
    cam = _module(t)
    out, g_rays, g_rvec, g_tvec = _run(cam, t)
    assert np.array_equal(out[0].cpu().numpy(), g[f"{name}__ref32__out_o"])
    _within_bar(out[1], g, name, "out_d")
    _within_bar(g_rvec, g, name, "g_rvec")
    _within_bar(g_tvec, g, name, "g_tvec")
    _within_bar(g_rays[1], g, name, "g_rays_d")
    assert torch.equal(g_rays[0], t["G_o"])
    absent = sorted(set(range(t["rvec"].shape[0])) - set(t["ids"].cpu().tolist()))
    if name in ("n64_c3_empty", "n257_c3_one", "n64_c70_random"):
        assert absent                                              # these cases exist for their empty cameras
    for c in absent:
        assert not g_rvec[c].any() and not g_tvec[c].any(), c
    # the parameter gradients do not depend on whether the rays asked for theirs
    _, none, g_rvec2, g_tvec2 = _run(cam, t, ray_grads=False)
    assert none is None and torch.equal(g_rvec2, g_rvec) and torch.equal(g_tvec2, g_tvec)
    # rot_mats(): the matrices the forward applied
    R = cam.rot_mats().detach()
    assert R.shape == (t["rvec"].shape[0], 3, 3)
    want = cp.rot_mats(t["rvec"].double().cpu())
    assert float((R.cpu().double() - want).abs().max()) <= 1e-6 * float(want.abs().max())


def test_identity_module_returns_its_input_bit_for_bit(golden):
    g = golden("camera")
    t = _case(g, "n4099_c70_random")
    for trainable in (False, True):
        cam = nerf_sos_amd.CameraTransformer(70, trainable=trainable).to(DEV)
        rays = torch.stack([t["rays_o"], t["rays_d"]], 0)
        out = cam.transform(rays, t["ids"])
        assert out.shape == rays.shape and torch.equal(out.detach(), rays)
        assert out.requires_grad == trainable
    assert torch.equal(cam.rot_mats().detach(), torch.eye(3, device=DEV).expand(70, 3, 3))


def test_two_calls_agree_and_a_camera_depends_on_its_own_rays_only(golden):
    """Determinism, and the reduction's invariant (include/nerf_sos_hip.h): the sums of camera c are taken over
    fixed chunks of the batch, so they depend on c's own rays AND their positions -- not on what any other ray holds or names.
    (A call given only c's rays moves them to other positions and chunks: its fp64 partial sums associate differently, so equality
    with it is not promised bit for bit and is held to the accuracy bar by the first test instead.)"""
    g = golden("camera")
    for name in ("n4099_c70_random", "n4099_c3_runs", "n257_c70_random"):
        t = _case(g, name)
        cam = _module(t)
        a, b = _run(cam, t), _run(cam, t)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        C = t["rvec"].shape[0]
        for c in sorted(set(t["ids"].cpu().tolist()))[:3]:
            mine = t["ids"] == c
            u = dict(t)
            gen = torch.Generator(device=DEV).manual_seed(c)
            for k in ("rays_o", "rays_d", "G_o", "G_d"):               # every other ray: other values ...
                u[k] = torch.where(mine[:, None], t[k], 100.0 * torch.randn(t[k].shape, device=DEV, generator=gen))
            other = torch.randint(0, C + 2, mine.shape, device=DEV, generator=gen, dtype=torch.int32) - 1   # ... another camera or none
            u["ids"] = torch.where(mine, t["ids"], torch.where(other == c, other + 1, other))
            assert int((u["ids"] == c).sum()) == int(mine.sum())
            _, _, g_rvec, g_tvec = _run(cam, u)
            assert torch.equal(g_rvec[c], a[2][c]) and torch.equal(g_tvec[c], a[3][c]), (name, c)


def test_reference_format_and_package_layout_agree_bit_for_bit(golden):
    """forward(rays_o[...,4], rays_d[...,4]) (camera.py:120-143: the id as a float in the fourth column) and transform(rays, ids)
    are one autograd.Function over the same two kernels; batch dimensions of any rank."""
    g = golden("camera")
    t = _case(g, "n257_c70_random")
    n = 256
    cam = _module(t)
    ids = t["ids"][:n].reshape(4, 64)
    rays = torch.stack([t["rays_o"][:n], t["rays_d"][:n]], 0).reshape(2, 4, 64, 3).requires_grad_(True)
    G = torch.stack([t["G_o"][:n], t["G_d"][:n]], 0).reshape(2, 4, 64, 3)
    out = cam.transform(rays, ids)
    ga = torch.autograd.grad(out, [rays, cam.rvec, cam.tvec], grad_outputs=G)
    col = ids.float()[..., None]
    o4 = torch.cat([rays[0].detach(), col], -1).requires_grad_(True)
    d4 = torch.cat([rays[1].detach(), col], -1).requires_grad_(True)
    o, d = cam(o4, d4)
    assert o.shape == (4, 64, 3) and torch.equal(o, out[0]) and torch.equal(d, out[1])
    gb = torch.autograd.grad([o, d], [o4, d4, cam.rvec, cam.tvec], grad_outputs=[G[0], G[1]])
    assert torch.equal(gb[0][..., :3], ga[0][0]) and torch.equal(gb[1][..., :3], ga[0][1])
    assert not gb[0][..., 3].any() and not gb[1][..., 3].any()          # no gradient to the id column
    assert torch.equal(gb[2], ga[1]) and torch.equal(gb[3], ga[2])
    # host ids: range-checked and uploaded
    out2 = cam.transform(rays.detach(), ids.cpu().tolist())
    assert torch.equal(out2.detach(), out.detach())
    with pytest.raises(IndexError):
        cam.transform(rays.detach(), torch.full((4, 64), 70))
    bad = d4.detach().clone()
    bad[0, 0, 3] += 1
    with pytest.raises(ValueError):
        cam(o4.detach(), bad)


def test_an_out_of_range_id_gives_nan_on_its_ray_and_enters_no_gradient(golden):
    g = golden("camera")
    t = _case(g, "n257_c3_farnorm")
    cam = _module(t)
    C, victim = 3, 100
    c = int(t["ids"][victim])
    base = _run(cam, t)
    for bad_id in (C, -1, 2 ** 31 - 1):
        u = dict(t)
        u["ids"] = t["ids"].clone()
        u["ids"][victim] = bad_id
        out, g_rays, g_rvec, g_tvec = _run(cam, u)
        keep = torch.arange(out.shape[1], device=DEV) != victim
        assert torch.isnan(out[:, victim]).all()
        assert torch.equal(out[:, keep], base[0][:, keep]) and torch.equal(g_rays[:, keep], base[1][:, keep])
        assert not g_rays[:, victim].any()
        # the other cameras' sums never saw the ray; its own camera's are those of the batch without it
        for k in range(C):
            if k != c:
                assert torch.equal(g_rvec[k], base[2][k]) and torch.equal(g_tvec[k], base[3][k])
        sel = keep.cpu()
        want = cp.grads(*[u[k].cpu().double()[sel] for k in ("rays_o", "rays_d")], u["ids"].cpu()[sel], u["rvec"].cpu().double(),
                        u["tvec"].cpu().double(), u["G_o"].cpu().double()[sel], u["G_d"].cpu().double()[sel])
        for got, k in ((g_rvec, "g_rvec"), (g_tvec, "g_tvec")):
            scale = float(want[k].abs().max())
            assert float((got.cpu().double() - want[k]).abs().max()) <= 1e-6 * scale, k
        assert float((g_rvec[c] - base[2][c]).abs().max()) > 0          # it did count before


def test_capture_replays_equal_eager_and_nothing_but_outputs_is_allocated(golden):
    """Forward + backward inside torch.cuda.graph, replayed three times with new inputs copied into the static tensors, against
    eager bit for bit; and the calls allocate their outputs only (the module's workspace is reused)."""
    g = golden("camera")
    t = _case(g, "n4099_c70_random")
    cam = _module(t)
    N, C = t["ids"].numel(), 70
    s_rays = torch.stack([t["rays_o"], t["rays_d"]], 0).requires_grad_(True)
    s_ids, s_G = t["ids"].clone(), torch.stack([t["G_o"], t["G_d"]], 0)

    def step():   # detached: no autograd graph (and no leaf's accumulator node, which remembers its stream) outlives the call
        out = cam.transform(s_rays, s_ids)
        return tuple(x.detach() for x in (out,) + torch.autograd.grad(out, [s_rays, cam.rvec, cam.tvec], grad_outputs=s_G))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step()
    gen = torch.Generator(device=DEV).manual_seed(12)
    for it in range(3):
        with torch.no_grad():
            s_rays.copy_(torch.randn(s_rays.shape, device=DEV, generator=gen))
            s_G.copy_(torch.randn(s_G.shape, device=DEV, generator=gen))
            s_ids.copy_(torch.randint(0, C, (N,), device=DEV, generator=gen, dtype=torch.int32))
            cam.rvec.add_(0.01 * torch.randn(C, 4, device=DEV, generator=gen))
            cam.tvec.add_(0.01 * torch.randn(C, 3, device=DEV, generator=gen))
        graph.replay()
        got = [x.clone() for x in static]
        want = step()
        for x, y in zip(got, want):
            assert torch.equal(x, y), it
    del graph, static
    # allocations: ops level with a caller-owned workspace, then the module with only the parameters asking for a gradient
    ws = ops.camera_workspace(N, C, DEV)
    ids = t["ids"]
    rvec, tvec = cam.rvec.detach(), cam.tvec.detach()
    torch.cuda.synchronize()

    def rounded(*shapes):   # the caching allocator hands out multiples of 512 bytes
        return sum(-(-int(np.prod(s)) * 4 // 512) * 512 for s in shapes)

    m0 = torch.cuda.memory_allocated()
    out = ops.camera_transform(t["rays_o"], t["rays_d"], ids, rvec, tvec, planar=True)
    m1 = torch.cuda.memory_allocated()
    grads = ops.camera_transform_backward(t["G_o"], t["G_d"], t["rays_d"], ids, rvec, workspace=ws, params=True, rays=True)
    m2 = torch.cuda.memory_allocated()
    assert m1 - m0 == rounded((2, N, 3)) and m2 - m1 == rounded((C, 4), (C, 3), (N, 3), (N, 3))
    rays = torch.stack([t["rays_o"], t["rays_d"]], 0)
    G = torch.stack([t["G_o"], t["G_d"]], 0)
    _run(cam, t, ray_grads=False)                                       # the module's workspace exists from here on
    torch.cuda.synchronize()
    m0 = torch.cuda.memory_allocated()
    out2 = cam.transform(rays, ids)
    g2 = torch.autograd.grad(out2, [cam.rvec, cam.tvec], grad_outputs=G)
    m1 = torch.cuda.memory_allocated()
    assert m1 - m0 == rounded((2, N, 3), (C, 4), (C, 3))
    assert torch.equal(out2.detach(), out) and torch.equal(g2[0], grads[0]) and torch.equal(g2[1], grads[1])


def test_a_captured_training_step_survives_a_later_larger_batch(golden):
    """The training pattern -- loss.backward() into rvec.grad / tvec.grad, warmed up on a side stream and captured as
    GraphedPatchStep captures its step -- and the module's workspace: a graph captured at 257 rays keeps pointing into the
    workspace of that size, so an eager call with 4099 rays (three chunks: a larger workspace) must retire it, not free it.  Tensors
    allocated afterwards stay untouched by the replay, and the replay still equals eager."""
    g = golden("camera")
    big = _case(g, "n4099_c70_random")
    cam = _module(big)
    n, C = 257, 70
    assert ops.camera_workspace_bytes(4099, C) > ops.camera_workspace_bytes(n, C)
    s_rays = torch.stack([big["rays_o"][:n], big["rays_d"][:n]], 0).clone()
    s_ids, s_G = big["ids"][:n].clone(), torch.stack([big["G_o"][:n], big["G_d"][:n]], 0).clone()

    def step(rays, ids, G):   # nothing of the autograd graph outlives the call
        cam.rvec.grad = cam.tvec.grad = None
        cam.transform(rays, ids).backward(G)
        return cam.rvec.grad, cam.tvec.grad

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step(s_rays, s_ids, s_G)
    torch.cuda.current_stream().wait_stream(side)
    cam.rvec.grad = cam.tvec.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step(s_rays, s_ids, s_G)
    want = [x.clone() for x in step(s_rays, s_ids, s_G)]
    big_grads = [x.clone() for x in step(torch.stack([big["rays_o"], big["rays_d"]], 0), big["ids"], torch.stack([big["G_o"], big["G_d"]], 0))]
    assert all(torch.isfinite(x).all() for x in big_grads)
    words = ops.camera_workspace_bytes(n, C) // 8
    junk = [torch.full((words,), -7.0, device=DEV, dtype=torch.float64) for _ in range(8)]   # what a freed workspace would be handed to
    for x in static:
        x.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(bool((j == -7.0).all()) for j in junk)
    assert torch.equal(static[0], want[0]) and torch.equal(static[1], want[1])
    # one workspace per device, the outgrown one kept
    assert len(cam._ws) == 1 and len(cam._retired) == 1 and cam._retired[0].numel() == words


def test_second_derivatives_raise_and_wide_ids_are_compared_before_narrowing(golden):
    g = golden("camera")
    t = _case(g, "n257_c3_farnorm")
    cam = _module(t)
    rays = torch.stack([t["rays_o"], t["rays_d"]], 0)
    out = cam.transform(rays, t["ids"])
    G = torch.stack([t["G_o"], t["G_d"]], 0)
    (g_rvec,) = torch.autograd.grad(out, [cam.rvec], grad_outputs=G.clone().requires_grad_(True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g_rvec.sum().backward()
    (g_rvec,) = torch.autograd.grad(cam.transform(rays, t["ids"]), [cam.rvec], grad_outputs=G, create_graph=True)
    assert not g_rvec.requires_grad                    # nothing to differentiate again: a second backward has no graph to follow
    base = cam.transform(rays, t["ids"]).detach()
    # int64 ids on the device: 2^32 and 2^32 + 1 do not wrap to cameras 0 and 1
    wide = t["ids"].long()
    wide[5], wide[6], wide[7] = 2 ** 32, 2 ** 32 + 1, -(2 ** 32)
    out = cam.transform(rays, wide).detach()
    keep = torch.ones(257, dtype=torch.bool, device=DEV)
    keep[5:8] = False
    assert torch.isnan(out[:, 5:8]).all() and torch.equal(out[:, keep], base[:, keep])
    # the reference format's float column: NaN, infinities and huge values name no camera; -0.5 and 1.7 truncate toward zero
    col = t["ids"].float()
    col[5], col[6], col[7], col[8], col[9], col[10] = float("nan"), float("inf"), -float("inf"), 3e38, -0.5, 1.7
    o4, d4 = torch.cat([rays[0], col[:, None]], -1), torch.cat([rays[1], col[:, None]], -1)
    d4[5, 3] = col[5]
    with pytest.raises(ValueError):
        cam(o4, d4)                                    # NaN != NaN: the two id columns do not agree
    o4[5, 3] = d4[5, 3] = 3.0                          # == C: out of range
    o, d = cam(o4, d4)
    assert torch.isnan(o[5:9]).all() and torch.isnan(d[5:9]).all()
    ids = t["ids"].clone()
    ids[9], ids[10] = 0, 1
    keep = torch.ones(257, dtype=torch.bool, device=DEV)
    keep[5:9] = False
    want = cam.transform(rays, ids).detach()
    assert torch.equal(o.detach()[keep], want[0][keep]) and torch.equal(d.detach()[keep], want[1][keep])


def _build(tag, golden, manifest):
    if tag in GENERIC_CASES:
        cfg, sd = generic_state(tag, golden)
        net = nerf_sos_amd.NeRFNet(**GENERIC_CASES[tag][0])
    else:
        cfg = tp.PortConfig(n_importance=128, **CFGS[tag])
        sd = ref_state(tag, manifest, peaky=True)
        net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, **CFGS[tag])
    net = net.to(DEV).eval()
    net.load_state_dict(sd)
    return cfg, net


@pytest.mark.parametrize("tag", ["semcoord", "d6w96_m6"])
def test_camera_gradients_through_the_renderer_vs_the_reference(golden, manifest, tag):
    """The real CameraTransformer feeding the real NeRFNet (make_goldens_camera.py) against net(cam.transform(rays, ids), bounds):
    rvec.grad / tvec.grad of a random linear functional of the rendered maps within 2e-4 of each gradient's scale -- the bar the
    ray gradients carry (test_gpu_raygrad.py), of which these are fixed linear maps; fine positions pinned to the reference's
    through its coarse weights; the network's gradients come out of the same backward."""
    g = golden("camera")
    cfg, net = _build(tag, golden, manifest)
    key = f"render_{tag}"
    rays = torch.from_numpy(g[f"{key}__rays"]).to(DEV)
    ids = torch.from_numpy(g[f"{key}__ids"]).to(DEV)
    R = rays.shape[1]
    near, far = torch.full((R, 1), tp.NEAR), torch.full((R, 1), tp.FAR)
    z = tp.stratified_z(near, far, cfg.n_samples, None)
    z_fine = tp.importance_z(z, torch.from_numpy(g[f"{key}__weights0"]), cfg.n_importance, None)[0].to(DEV)
    cam = nerf_sos_amd.CameraTransformer(3, trainable=True).to(DEV)
    cam.load_state_dict({"rvec": torch.from_numpy(g[f"{key}__rvec"]), "tvec": torch.from_numpy(g[f"{key}__tvec"])})
    ret = net(cam.transform(rays, ids), (tp.NEAR, tp.FAR), z_fine_override=z_fine)
    assert np.abs(ret["rgb"].detach().cpu().numpy() - g[f"{key}__rgb"]).max() <= 1e-4
    loss, used = 0.0, 0
    for k in ret:
        gk = f"{key}__G__{k}"
        if gk in g:
            assert ret[k].requires_grad, k
            loss = loss + (ret[k] * torch.from_numpy(g[gk]).to(DEV)).sum()
            used += 1
    assert used == sum(1 for k in g if k.startswith(f"{key}__G__"))
    loss.backward()
    for p, what in ((cam.rvec, "g_rvec"), (cam.tvec, "g_tvec")):
        want = g[f"{key}__{what}"]
        scale = np.abs(want).max()
        err = np.abs(p.grad.cpu().numpy() - want).max() / scale
        print(f"{tag} {what}: err {err:.3e} of scale {scale:.4g}")
        assert err <= 2e-4, f"{tag}: {what} off by {err:.2e} of its scale {scale:.3g}"
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())


def test_device_scene_batches_carry_camera_ids(golden):
    """cam_id=True on all four batch kinds: int32, one per ray, the image's index within the split (data/datasets.py:100,166,236,
    312) -- checked against the ray origins, which are that image's pose; the flag off leaves today's keys."""
    scene = os.path.join(HERE, "golden", "io_scene")
    ds = nio.PreparedScene(scene, split="train", bin_thres=0.3, load_rays=False).to_device(DEV)
    H, W, N = ds.height, ds.width, ds.image_count
    t_of = ds.poses[:, :3, 3]

    def check(b, want, lead):
        ids = b["cam_ids"]
        assert ids.dtype == torch.int32 and ids.is_cuda and tuple(ids.shape) == lead
        assert torch.equal(ids.cpu(), want.reshape(lead).to(torch.int32))
        return ids

    order = [2, 0, 3, 3, 1, 0]
    origins = [(0, 0), (4, 8), (1, 2), (3, 7), (2, 5), (4, 0)]
    plain = ds.patch_batch(order, 8, 2, origins=origins)
    assert set(plain) == {"rays", "rays_planar", "poses", "start_idx", "target_s", "masks"}
    b = ds.patch_batch(order, 8, 2, origins=origins, cam_id=True)
    assert set(b) == set(plain) | {"cam_ids"} and all(torch.equal(b[k], plain[k]) for k in plain)
    ids = check(b, torch.tensor(order)[:, None].expand(6, 16), (6, 16))
    assert torch.equal(b["rays_planar"][0].reshape(6, 16, 3), t_of[ids.long()])
    sel = torch.tensor([[i, h, w] for i, (h, w) in zip(order, origins)], dtype=torch.int32, device=DEV)
    b2 = ds.patch_batch(None, 8, 2, sel_device=sel, cam_id=True)
    assert torch.equal(b2["cam_ids"], ids) and torch.equal(b2["rays"], b["rays"])
    assert "cam_ids" not in ds.patch_batch(None, 8, 2, sel_device=sel)

    gen = torch.Generator().manual_seed(2)
    pix = torch.randint(0, N * H * W, (5, 7), generator=gen)
    plain = ds.pixel_batch(pix.to(DEV))
    assert set(plain) == {"rays", "target_s", "masks"}
    b = ds.pixel_batch(pix.to(DEV), cam_id=True)
    assert set(b) == {"rays", "target_s", "masks", "cam_ids"}
    ids = check(b, pix // (H * W), (5, 7))
    assert torch.equal(b["rays"][0], t_of[ids.long()]) and torch.equal(b["rays"], plain["rays"])
    picks = torch.randperm(N * H * W, generator=gen)[:33]
    for idx in (picks.tolist(), picks.to(DEV)):
        assert set(ds.ray_batch(idx)) == {"rays", "target_s", "masks"}
        check(ds.ray_batch(idx, cam_id=True), picks // (H * W), (33,))
    np.random.seed(11)
    plain = ds.view_batch(2, 32)
    np.random.seed(11)
    b = ds.view_batch(2, 32, precrop_frac=None, cam_id=True)
    assert set(plain) == {"rays", "target_s", "masks"} and torch.equal(b["rays"], plain["rays"])
    check(b, torch.full((32,), 2), (32,))
    # the ids are what CameraTransformer.transform takes
    cam = nerf_sos_amd.CameraTransformer(N).to(DEV)
    assert torch.equal(cam.transform(b["rays"], b["cam_ids"]), b["rays"])


@pytest.mark.parametrize("layer", ["restatement", "kernels"])
def test_refinement_smoke_on_the_trained_scene(layer):
    """Pose refinement end to end: the trained checkpoint (tests/golden/trained_scene.ckpt), frozen, renders 256 fixed pixels of
    one training view of synthetic.ProceduralScene whose rays had the inverse of a known correction applied -- 2 degrees about the
    world's y axis, offset 0.05 along y -- with the targets traced on the true rays.  A fresh trainable CameraTransformer(1) trained
    by Adam for 30 steps on the photometric loss of the fine map must end with a lower loss than it started with, and with both
    |R - R0| and |t - t0| below where they started (conditions, not measurements).
    Choices: the rotation is about y (it moves the image sideways) and the offset along y (it moves it up), so the two do not
    trade against each other in the 30 steps; Adam's step is 1e-3, which lets a quaternion component cover the 0.0175 it has to
    and the offset most of its 0.05.  `restatement` runs tests/camera_port.py's torch layer in place of the kernels under the
    same conditions: it is what these choices were made with."""
    scene = syn.ProceduralScene()
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, **CFGS["semcoord"]).to(DEV).eval()
    nio.load_checkpoint(os.path.join(HERE, "golden", "trained_scene.ckpt"), net)
    for p in net.parameters():
        p.requires_grad_(False)
    i = scene.i_train[0]
    o, d = scene.pixel_rays(i)
    pix = np.random.default_rng(0).choice(o.shape[0], 256, replace=False)
    o, d = o[pix], d[pix]
    target = torch.from_numpy(scene.trace(o, d)[0]).to(DEV)
    a = np.deg2rad(2.0)
    R0 = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t0 = np.array([0.0, 0.05, 0.0])
    rays = torch.from_numpy(np.stack([o - t0, d @ R0], 0).astype(np.float32)).to(DEV)      # d_in = R0^T d: the layer must undo it
    ids = torch.zeros(256, dtype=torch.int32, device=DEV)
    cam = (nerf_sos_amd.CameraTransformer(1, trainable=True) if layer == "kernels" else cp.Layer(1)).to(DEV)
    opt = torch.optim.Adam(cam.parameters(), lr=1e-3)
    R0t, t0t = torch.from_numpy(R0).float().to(DEV), torch.from_numpy(t0).float().to(DEV)

    def dist():
        with torch.no_grad():
            R = cam.rot_mats()[0] if layer == "kernels" else cp.rot_mats(cam.rvec)[0]
            return float((R - R0t).norm()), float((cam.tvec[0] - t0t).norm())

    start, losses = dist(), []
    for _ in range(30):
        opt.zero_grad(set_to_none=True)
        ret = net(cam.transform(rays, ids), (scene.NEAR, scene.FAR))
        loss = ((ret["rgb"] - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        final = float(((net(cam.transform(rays, ids), (scene.NEAR, scene.FAR))["rgb"] - target) ** 2).mean())
    end = dist()
    print(f"{layer}: loss {losses[0]:.3e} -> {final:.3e}; |R - R0| {start[0]:.4f} -> {end[0]:.4f}; |t - t0| {start[1]:.4f} -> {end[1]:.4f}")
    assert final < losses[0]
    assert end[0] < start[0] and end[1] < start[1]

"""GPU (-m gpu): the HIP path, called through the C ABI, against the oracle and the reference goldens.

Bars: integer indices bit-exact; fp32 within 1e-4 of the reference goldens (BASELINE.json north_star);
against the C oracle (same canonical arithmetic) much tighter, bitwise where libm differences cannot enter.
"""
import os

import numpy as np
import pytest
import torch

import nerf_sos_amd
from nerf_sos_amd import _lib, ops
from oracle import c_oracle as co
from oracle import torch_port as tp
from helpers import CFGS, close, ref_state, tag_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RS = (1, 7, 64, 257)


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def test_native_library_is_the_in_tree_one():
    lib = _lib.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.samefile(_lib.LIB_PATH, os.path.join(root, "nerf-sos_amd", "libnerf_sos_hip.so"))
    with open("/proc/self/maps") as f:
        assert "libnerf_sos_hip.so" in f.read(), "HIP library not mapped into this process"
    assert lib.nsos_abi_version() == _lib.ABI_VERSION
    assert "gfx950" in torch.cuda.get_device_properties(0).gcnArchName


# ------------------------------------------------------------------------------------------ K1
@pytest.mark.parametrize("R", RS)
def test_ray_setup(golden, R):
    g = golden("stratified")
    o, d, near, far, t = (g[f"R{R}_{k}"] for k in ("o", "d", "near", "far", "t_rand"))
    z, v = ops.ray_setup(T(d), T(near), T(far), 64, T(t))
    zo, vo = co.ray_setup(o, d, near, far, t, 64)
    assert np.array_equal(N(z), zo), "jittered z must equal the oracle bit for bit"
    assert np.array_equal(N(v), vo), "viewdirs must equal the oracle bit for bit"
    close(N(z), g[f"R{R}_z"], atol=2e-6, rtol=1e-6, what="z vs reference")
    zd, _ = ops.ray_setup(T(d), T(near), T(far), 64, None)
    assert np.array_equal(N(zd), g[f"R{R}_z_det"]), "deterministic z must equal the REFERENCE bit for bit"
    pts = ops.ray_points(T(o), T(d), T(g[f"R{R}_z"]))
    assert np.array_equal(N(pts), g[f"R{R}_pts"]), "o + d*z must equal the REFERENCE bit for bit"


# ------------------------------------------------------------------------------------------ K3
@pytest.mark.parametrize("C", [4, 6])
@pytest.mark.parametrize("S", [64, 192])
@pytest.mark.parametrize("white", [False, True])
@pytest.mark.parametrize("noisy", [False, True])
def test_composite(golden, C, S, white, noisy):
    g = golden("composite")
    base = f"C{C}_S{S}_{'white' if white else 'black'}"
    tag = base + ("_noise" if noisy else "_clean")
    raw, z, d, nz = g[base + "_raw"], g[base + "_z"], g[base + "_d"], g[base + "_noise"]
    out = ops.composite(T(raw), T(z), T(d), T(nz) if noisy else None, 0.7 if noisy else 0.0, white)
    ref = co.composite(raw, z, d, nz if noisy else None, 0.7 if noisy else 0.0, white)
    for k in ref:
        got = N(out[k])
        # same arithmetic; expf/sqrt of the device libm vs glibc may differ in the last ulp
        close(got, ref[k], atol=1e-6, rtol=2e-6, what=f"{tag} {k} vs oracle")
        close(got, g[f"{tag}_{k}"], atol=2e-6, rtol=2e-5, what=f"{tag} {k} vs reference")
    if not noisy:
        for r in (0, 1):  # empty rays
            assert N(out["acc"])[r, 0] == 0.0 and N(out["depth"])[r, 0] == np.float32(1e10) and N(out["disp"])[r, 0] == 0.0


def test_composite_ragged_sample_counts():
    rng = np.random.default_rng(5)
    for S in (1, 2, 63, 65, 100, 191, 193, 256, 300, 512):
        R = 9
        raw = rng.standard_normal((R, S, 6), dtype=np.float32) * 2
        z = np.sort(1.2 + 13 * rng.random((R, S), dtype=np.float32), -1)
        d = rng.standard_normal((R, 3), dtype=np.float32)
        out = ops.composite(T(raw), T(z), T(d))
        ref = co.composite(raw, z, d)
        for k in ref:
            close(N(out[k]), ref[k], atol=1e-6, rtol=2e-6, what=f"S={S} {k}")


# ------------------------------------------------------------------------------------------ K4
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("det", [False, True])
def test_importance(golden, R, det):
    g = golden("importance")
    tag = f"R{R}_{'det' if det else 'rand'}"
    z, w, u, cdf = g[f"R{R}_z"], g[f"R{R}_w"], g[f"R{R}_u"], g[f"R{R}_cdf"]
    uu = None if det else T(u)
    # stage-wise index pin: reference cdf + u in -> integer indices out, BIT-EXACT
    zf, zs, zstd, cdf_o, inds = ops.importance_sample(T(z), T(w), 128, uu, cdf_in=T(cdf), debug=True)
    assert np.array_equal(N(inds), g[f"{tag}_inds"]), "searchsorted indices must equal the reference bit for bit"
    assert np.array_equal(N(cdf_o), cdf)
    close(N(zs), g[f"{tag}_z_samples"], atol=2e-6, rtol=1e-6, what="z_samples")
    close(N(zf), g[f"{tag}_z_fine"], atol=2e-6, rtol=1e-6, what="z_fine")
    close(N(zstd), g[f"{tag}_z_std"], atol=2e-6, rtol=1e-6, what="z_std")
    ref = co.importance(z, w, None if det else u, 128, cdf_in=cdf)
    for k, got in (("z_samples", zs), ("z_fine", zf), ("z_std", zstd)):
        assert np.array_equal(N(got), ref[k]), f"{k} must equal the oracle bit for bit (same cdf in)"
    # own cdf: equals the oracle's (fp64 accumulation), indices consistent with that cdf
    zf2, zs2, zstd2, cdf2, inds2 = ops.importance_sample(T(z), T(w), 128, uu, debug=True)
    own = co.importance(z, w, None if det else u, 128)
    assert np.array_equal(N(cdf2), own["cdf"]), "cdf must equal the oracle bit for bit"
    assert np.array_equal(N(inds2), own["inds"])
    assert np.array_equal(N(zf2), own["z_fine"])
    close(N(cdf2), cdf, atol=3e-7, rtol=0, what="cdf vs reference")
    assert (np.diff(N(zf2), axis=-1) >= 0).all()


def test_importance_unsorted_depths_follow_torch_sort():
    """The reference sorts cat([z, samples]) and assumes nothing about either list (models/sampler.py:161): caller-supplied
    depths out of order, near > far (descending z), NaNs.  The merge falls back to a general sort per ray; every slot of
    z_fine is written exactly once and equals torch.sort of the kernel's own (z, samples) -- NaNs last, like torch."""
    rng = np.random.default_rng(23)
    for S, n_imp in ((64, 128), (17, 40), (200, 64)):
        R = 37
        z = (1.2 + 13 * rng.random((R, S), dtype=np.float32))
        z[: R // 3] = np.sort(z[: R // 3], -1)[:, ::-1]            # descending (near > far)
        z[R // 3: 2 * R // 3] = np.sort(z[R // 3: 2 * R // 3], -1)  # in order: the fast path, same launch
        z[5, 3] = np.nan                                            # a poisoned ray
        w = rng.random((R, S), dtype=np.float32) ** 4
        for uu in (None, rng.random((R, n_imp), dtype=np.float32)):
            zf = torch.full((R, S + n_imp), -7.0, device=DEV)
            zf_, zs, _ = ops.importance_sample(T(z), T(w), n_imp, None if uu is None else T(uu))
            want = torch.sort(torch.cat([T(z), zs], -1), -1).values
            assert torch.equal(torch.nan_to_num(zf_, nan=-1.0), torch.nan_to_num(want, nan=-1.0)), (S, n_imp, uu is None)
    # through the fused coarse-compositing + importance launch as well
    R, S, n_imp = 9, 64, 128
    z = torch.from_numpy(np.sort(1.2 + 13 * rng.random((R, S), dtype=np.float32), -1)[:, ::-1].copy()).to(DEV)
    raw = torch.randn(R, S, 4, device=DEV)
    d = torch.randn(R, 3, device=DEV)
    ret, zf, zs, _ = ops.composite_importance(raw, z, d, n_imp, None, 0.0, False, None)
    assert torch.equal(zf, torch.sort(torch.cat([z, zs], -1), -1).values)


def test_importance_other_counts():
    rng = np.random.default_rng(11)
    R = 33
    z = np.sort(1.2 + 13 * rng.random((R, 64), dtype=np.float32), -1)
    w = rng.random((R, 64), dtype=np.float32) ** 6
    for n_imp in (1, 64, 100, 128, 200, 448):
        u = rng.random((R, n_imp), dtype=np.float32)
        for uu in (None, u):
            zf, zs, zstd, cdf, inds = ops.importance_sample(T(z), T(w), n_imp, None if uu is None else T(uu), debug=True)
            ref = co.importance(z, w, uu, n_imp)
            assert np.array_equal(N(inds), ref["inds"]) and np.array_equal(N(zf), ref["z_fine"])
            assert np.array_equal(N(zs), ref["z_samples"])
            close(N(zstd), ref["z_std"], atol=1e-6, rtol=1e-6, what="z_std")
    for S in (2, 3, 17, 32, 63):   # fewer coarse samples (the per-call N_samples kwarg, models/sampler.py:41)
        u = rng.random((R, 128), dtype=np.float32)
        for uu in (None, u):
            zf, zs, zstd, cdf, inds = ops.importance_sample(T(z[:, :S]), T(w[:, :S]), 128, None if uu is None else T(uu), debug=True)
            ref = co.importance(z[:, :S], w[:, :S], uu, 128)
            assert np.array_equal(N(cdf), ref["cdf"]) and np.array_equal(N(inds), ref["inds"]), S
            assert np.array_equal(N(zf), ref["z_fine"]) and np.array_equal(N(zs), ref["z_samples"]), S
    # more than 64 coarse samples (per-call N_samples > 64): the general kernel, several entries per lane
    for S in (65, 96, 128, 200, 512):
        zz = np.sort(1.2 + 13 * rng.random((R, S), dtype=np.float32), -1)
        ww = rng.random((R, S), dtype=np.float32) ** 6
        for n_imp in (64, 128, 448):
            u = rng.random((R, n_imp), dtype=np.float32)
            for uu in (None, u):
                zf, zs, zstd, cdf, inds = ops.importance_sample(T(zz), T(ww), n_imp, None if uu is None else T(uu), debug=True)
                ref = co.importance(zz, ww, uu, n_imp)
                close(N(cdf), ref["cdf"], atol=2e-7, rtol=0, what=f"cdf S={S}")
                # the same cdf handed in (stage-wise pin): indices and samples are then exact
                zf, zs, zstd, _, inds = ops.importance_sample(T(zz), T(ww), n_imp, None if uu is None else T(uu), cdf_in=T(ref["cdf"]), debug=True)
                assert np.array_equal(N(inds), ref["inds"]) and np.array_equal(N(zf), ref["z_fine"]), (S, n_imp)
                assert np.array_equal(N(zs), ref["z_samples"]), (S, n_imp)
                close(N(zstd), ref["z_std"], atol=1e-6, rtol=1e-6, what="z_std")
    with pytest.raises(RuntimeError, match="nsos_importance_sample"):
        ops.importance_sample(T(np.zeros((2, 513), np.float32)), T(np.zeros((2, 513), np.float32)), 128)


# ------------------------------------------------------------------------------------------ K2
def _packed(sd, prefix, name):
    params = {k[len(prefix) + 5:]: v.to(DEV) for k, v in sd.items() if k.startswith(prefix + ".mlp.")}
    return ops.pack_mlp(params, ops.sem_mode_of(**CFGS[name]))


@pytest.mark.parametrize("name", list(CFGS))
@pytest.mark.parametrize("peaky", [False, True])
def test_mlp_points_golden(golden, manifest, name, peaky):
    g = golden("mlp")
    sd = ref_state(name, manifest, peaky)
    tag = tag_of(name, peaky)
    mode = ops.sem_mode_of(**CFGS[name])
    for prefix in ("nerf", "nerf_fine"):
        raw = N(ops.mlp_forward_points(_packed(sd, prefix, name), mode, T(g["pts"]), T(g["dirs"])))
        ref = co.mlp(co.Weights(sd, prefix, **CFGS[name]), g["pts"], g["dirs"])
        close(raw, ref, atol=5e-6, rtol=5e-6, what=f"{tag} {prefix} vs oracle")
        close(raw, g[f"{tag}_{prefix}_raw"], atol=2e-5, rtol=2e-5, what=f"{tag} {prefix} vs reference")


@pytest.mark.parametrize("name", list(CFGS))
def test_mlp_exact_fp32_chain(manifest, name):
    """At x = 0, dir = 0 every sin/cos is exactly 0/1 on any libm, so the only arithmetic left is the
    fmaf chains: the exact-fp32 MFMA path must then equal the oracle BIT FOR BIT (k order, bias, ReLU,
    vector-ALU heads, packing)."""
    sd = ref_state(name, manifest, peaky=True)
    mode = ops.sem_mode_of(**CFGS[name])
    pts = np.zeros((130, 3), np.float32)
    raw = N(ops.mlp_forward_points(_packed(sd, "nerf_fine", name), mode, T(pts), T(pts)))
    ref = co.mlp(co.Weights(sd, "nerf_fine", **CFGS[name]), pts, pts)
    assert np.array_equal(raw, ref), f"max abs diff {np.abs(raw - ref).max():.3e}"


@pytest.mark.parametrize("n_pts", [1, 31, 32, 127, 128, 129, 1000, 128 * 300 + 5])
def test_mlp_ragged_point_counts(manifest, n_pts):
    sd = ref_state("semcoord", manifest, peaky=True)
    rng = np.random.default_rng(n_pts)
    pts = (rng.random((n_pts, 3), dtype=np.float32) * 8 - 4)
    dirs = rng.standard_normal((n_pts, 3), dtype=np.float32)
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    guard = torch.full((n_pts + 64, 6), 777.0, device=DEV)
    raw = ops.mlp_forward_points(_packed(sd, "nerf_fine", "semcoord"), 2, T(pts), T(dirs))
    assert raw.shape == (n_pts, 6)
    sel = np.unique(np.concatenate([np.arange(min(n_pts, 40)), np.arange(max(0, n_pts - 40), n_pts),
                                    rng.integers(0, n_pts, 40)]))
    ref = co.mlp(co.Weights(sd, "nerf_fine", True, True), pts[sel], dirs[sel])
    close(N(raw)[sel], ref, atol=2e-5, rtol=2e-5, what=f"n_pts={n_pts}")
    assert (guard == 777.0).all()


def test_mlp_rays_equals_points(manifest):
    sd = ref_state("semcoord", manifest)
    rays = tp.synthetic_rays(77, seed=1)
    o, d = T(rays[0]), T(rays[1])
    near = torch.full((77,), tp.NEAR, device=DEV)
    far = torch.full((77,), tp.FAR, device=DEV)
    packed = _packed(sd, "nerf", "semcoord")
    for S in (64, 192, 50):
        z, v = ops.ray_setup(d, near, far, S, torch.rand(77, S, device=DEV))
        raw_r = ops.mlp_forward_rays(packed, 2, o, d, v, z)
        pts = ops.ray_points(o, d, z)
        raw_p = ops.mlp_forward_points(packed, 2, pts.reshape(-1, 3), v[:, None, :].expand(77, S, 3).reshape(-1, 3))
        assert torch.equal(raw_r.reshape(-1, 6), raw_p), "ray-mode and point-mode kernels must agree bit for bit"


def test_repack_on_parameter_change(manifest):
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, use_semantics=True, sem_with_coord=True).to(DEV).eval()
    net.load_state_dict(ref_state("semcoord", manifest))
    pts = torch.rand(64, 3, device=DEV)
    with torch.no_grad():
        a = net.nerf_fine(pts, viewdirs=pts)
        b = net.nerf_fine(pts, viewdirs=pts)
        assert torch.equal(a, b)
        net.nerf_fine.mlp.semantic_linear[2].bias.add_(1.0)  # what an optimizer step does
        c = net.nerf_fine(pts, viewdirs=pts)
    assert torch.allclose(c[:, 4:], a[:, 4:] + 1.0, atol=1e-6) and torch.equal(c[:, :4], a[:, :4])


# ------------------------------------------------------------------------------------------ end to end
CASES = [("nosem", False, False, 128), ("semcoord", False, False, 128), ("semcoord", True, False, 128),
         ("sem", True, True, 128), ("nosem", True, False, 0)]


class _Draws:
    def __init__(self, tensors):
        self.q = list(tensors)

    def __call__(self, shape, device=None, **kw):
        t = self.q.pop(0)
        assert tuple(t.shape) == tuple(shape), (t.shape, shape)
        return t.to(device)


@pytest.mark.parametrize("name,peaky,white,n_imp", CASES)
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_end_to_end_vs_reference(golden, manifest, monkeypatch, name, peaky, white, n_imp, mode):
    g = golden("end_to_end")
    tag = tag_of(name, peaky, white, n_imp == 0) + "_" + mode
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=n_imp, perturb=1.0, raw_noise_std=1.0, white_bkgd=white,
                               **CFGS[name]).to(DEV)
    net.load_state_dict(ref_state(name, manifest, peaky, n_imp))
    net.train(mode == "train")
    if mode == "train":
        dr = [torch.as_tensor(g[f"{tag}_draw{i}"]) for i in range(4 if n_imp else 2)]
        rand = _Draws([dr[0]] + ([dr[2]] if n_imp else []))
        randn = _Draws([dr[1]] + ([dr[3]] if n_imp else []))
        monkeypatch.setattr(torch, "rand", rand)
        monkeypatch.setattr(torch, "randn", randn)
    with torch.no_grad():
        out = net(T(g["rays"]), (tp.NEAR, tp.FAR), radii=None)
    keys = sorted(k[len(tag) + 1:] for k in g if k.startswith(tag + "_") and "draw" not in k)
    assert sorted(out.keys()) == keys, "output dict keys must match the reference's"
    for k in keys:
        want = g[f"{tag}_{k}"]
        got = N(out[k])
        assert got.shape == want.shape, f"{k}: {got.shape} vs {want.shape}"
        if k in ("weights", "raw", "z_std") and n_imp:
            # the fine pass's per-sample tensors follow the importance samples: where a last-ulp difference of the coarse weights
            # flips a bisect index, a sample moves.  Counted per RAY (measured, round 4, 16 rays per case: weights at most 1 ray,
            # z_std none); `raw` is per SAMPLE POSITION -- any moved sample puts its ray outside -- so it keeps an element share
            # (measured <= 3.1e-3).  With the reference's z_fine pinned every key is strictly inside (tests/test_gpu_pins.py).
            err = np.abs(got.astype(np.float64) - want)
            tol = 1e-4 + 1e-4 * np.abs(want)
            rays_out = int((err > tol).reshape(err.shape[0], -1).any(-1).sum())
            if k == "raw":
                assert (err > tol).mean() < 4e-3, f"{tag} {k}: {(err > tol).mean():.4f} of elements outside tol"
            else:
                assert rays_out <= 1, f"{tag} {k}: {rays_out} of {err.shape[0]} rays outside tol"
        else:
            close(got, want, what=f"{tag} {k}")


def test_flower_full_batch_properties(manifest):
    """BASELINE config C2 size (4096 rays x (64+192), fp32): size-independent properties + a sampled
    oracle check, since the C oracle needs minutes for the full batch."""
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, use_semantics=True, sem_with_coord=True).to(DEV).eval()
    net.load_state_dict(ref_state("semcoord", manifest, peaky=True))
    rays = tp.synthetic_rays(4096, seed=0).to(DEV)
    with torch.no_grad():
        a = net(rays, (tp.NEAR, tp.FAR))
        b = net(rays, (tp.NEAR, tp.FAR))
        net.chunk = 1000  # ragged ray chunks: 4 x 1000 + 96
        c = net(rays, (tp.NEAR, tp.FAR))
        net.chunk = 32768
    for k in a:
        assert torch.equal(a[k], b[k]), f"{k}: not deterministic"
        assert torch.equal(a[k], c[k]), f"{k}: result depends on the ray chunking"
        assert torch.isfinite(a[k]).all() or k in ("depth", "depth0")
    assert a["raw"].shape == (4096, 192, 6) and a["weights"].shape == (4096, 192) and a["z_std"].shape == (4096,)
    assert (a["acc"] <= 1 + 1e-5).all() and (a["weights"] >= 0).all()
    assert torch.allclose(a["weights"].sum(-1, keepdim=True), a["acc"], atol=1e-5)
    sel = torch.arange(0, 4096, 171)
    sd = {k: v.cpu() for k, v in net.state_dict().items()}
    ref = co.render(sd, rays[0][sel].cpu(), rays[1][sel].cpu(), tp.NEAR, tp.FAR, use_semantics=True, sem_with_coord=True)
    for k in ("rgb", "depth", "acc", "disp", "semantics", "rgb0", "depth0", "semantics0", "weights0", "raw0"):
        close(N(a[k][sel]).reshape(ref[k].shape), ref[k], what=f"C2-size {k}")


def test_empty_batch():
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128).to(DEV).eval()
    with torch.no_grad():
        out = net.render_rays(torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, device=DEV),
                              torch.zeros(0, device=DEV), torch.zeros(0, device=DEV))
    assert out["rgb"].shape == (0, 3) and out["weights"].shape == (0, 192)


# ------------------------------------------------------------------------------------------ K5 (training)
GRAD_CASES = [("semcoord", True, False, 128), ("sem", True, True, 128), ("semcoord", False, False, 0)]


def _frozen(net):
    for n, p in net.named_parameters():  # run_nerf.py:307-318 (--fix_backbone)
        p.requires_grad = 'semantic_linear' in n
    return net


@pytest.mark.parametrize("name,peaky,white,n_imp", GRAD_CASES)
def test_frozen_backbone_gradients(golden, manifest, name, peaky, white, n_imp):
    """loss.backward() through NeRFNet with the shipped frozen-backbone recipe: semantic-head gradients equal
    the reference's (captured from the real reference by the golden generator)."""
    g = golden("sem_grads")
    tag = tag_of(name, peaky, white, n_imp == 0)
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=n_imp, white_bkgd=white, **CFGS[name]).to(DEV)
    net.load_state_dict(ref_state(name, manifest, peaky, n_imp))
    _frozen(net).eval()
    ret = net(T(g["rays"]), (tp.NEAR, tp.FAR), radii=None)
    assert ret["semantics"].requires_grad and not ret["rgb"].requires_grad and not ret["weights"].requires_grad
    close(N(ret["semantics"]), g[f"{tag}_semantics"], what="semantics (training-mode kernel variant)")
    loss = (ret["semantics"] * T(g[f"{tag}_G"])).sum()
    if n_imp:
        loss = loss + (ret["semantics0"] * T(g[f"{tag}_G0"])).sum()
    loss.backward()
    sd = dict(net.named_parameters())
    keys = [k[len(tag) + 6:] for k in g if k.startswith(tag + "_grad_")]
    assert len(keys) == (8 if n_imp else 4)
    for k in keys:
        want = g[f"{tag}_grad_{k}"]
        got = N(sd[k].grad)
        scale = np.abs(want).max() + 1e-12
        assert np.abs(got - want).max() <= 1e-4 * scale + 1e-6, f"grad {k}: max err {np.abs(got - want).max():.3e} (scale {scale:.3e})"
    for n, p in net.named_parameters():
        assert (p.grad is None) == ('semantic_linear' not in n)


def test_training_variant_matches_inference_and_optimizer_step(manifest):
    """The SAVE kernel variant produces bit-identical outputs; an Adam step on the heads changes only semantics."""
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, use_semantics=True, sem_with_coord=True,
                               perturb=0., raw_noise_std=0.).to(DEV)
    net.load_state_dict(ref_state("semcoord", manifest, peaky=True))
    _frozen(net).train()
    rays = tp.synthetic_rays(300, seed=5).to(DEV)
    with torch.no_grad():
        a = net(rays, (tp.NEAR, tp.FAR))
    b = net(rays, (tp.NEAR, tp.FAR))
    for k in a:
        assert torch.equal(a[k], b[k].detach()), k
    opt = torch.optim.Adam([p for p in net.parameters() if p.requires_grad], lr=2e-5)  # tiny step along -sign(grad)
    (b["semantics"].square().mean() + b["semantics0"].square().mean()).backward()
    opt.step()
    with torch.no_grad():
        c = net(rays, (tp.NEAR, tp.FAR))
    assert torch.equal(c["rgb"], a["rgb"]) and torch.equal(c["weights"], a["weights"])
    assert not torch.equal(c["semantics"], a["semantics"])
    assert c["semantics"].square().mean() < a["semantics"].square().mean()


def test_unfrozen_backbone_trains_in_fp32_and_on_the_split_kernels_at_16_bit():
    """Everything trainable (configs/*_full.txt): the full backward runs on the fp32 path; there is no 16-bit full backward, so a
    16-bit mlp_precision with a trainable backbone trains on the split-fp16 kernels (a warning says so; the gradients are the
    "fp16x3" ones bit for bit).  Backward twice through one render raises."""
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, use_semantics=True).to(DEV)
    rays = tp.synthetic_rays(8).to(DEV)
    ret = net(rays, (tp.NEAR, tp.FAR))
    assert ret["rgb"].requires_grad and ret["rgb0"].requires_grad and not ret["z_std"].requires_grad
    loss = ret["rgb"].sum() + ret["rgb0"].sum()
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.parameters())
    with pytest.raises(RuntimeError):
        loss.backward()
    grads = {}
    for prec in ("fp16x3", "bf16"):
        net.mlp_precision = prec
        net.zero_grad(set_to_none=True)
        nerf_sos_amd.NeRFNet._warned_full_16bit = False
        torch.manual_seed(3)
        if prec == "bf16":
            with pytest.warns(UserWarning, match="split-fp16"):
                ret = net(rays, (tp.NEAR, tp.FAR))
        else:
            ret = net(rays, (tp.NEAR, tp.FAR))
        (ret["rgb"].sum() + ret["rgb0"].sum()).backward()
        grads[prec] = {n: p.grad.clone() for n, p in net.named_parameters()}
    assert all(torch.equal(grads["bf16"][n], grads["fp16x3"][n]) for n in grads["bf16"])
    with torch.no_grad():                                    # inference under "bf16" stays on the 16-bit kernel
        net.mlp_precision = "bf16"
        a = net(rays, (tp.NEAR, tp.FAR))["raw"]
        net.mlp_precision = "fp16x3"
        assert not torch.equal(a, net(rays, (tp.NEAR, tp.FAR))["raw"])


# ------------------------------------------------------------------------------------------ K0 (section 8f)
@pytest.mark.parametrize("case", [0, 1, 2])
def test_generate_rays(golden, case):
    g = golden("rays")
    H, W, _ = (int(v) for v in g[f"case{case}_HWf"])
    K, c2w, want = g[f"case{case}_K"], g[f"case{case}_c2w"], g[f"case{case}_rays"]
    rays = ops.generate_rays(H, W, K, c2w, DEV)
    assert rays.shape == (2, H, W, 3) and np.array_equal(N(rays), want), "rays must equal the REFERENCE bit for bit"
    b, e = W + 3, H * W - 2   # a ragged flat pixel range, as a ray-sharded rank would request
    part = ops.generate_rays(H, W, K, c2w, DEV, pix_range=(b, e))
    assert np.array_equal(N(part), want.reshape(2, -1, 3)[:, b:e])
    assert ops.generate_rays(H, W, K, c2w, DEV, pix_range=(5, 5)).shape == (2, 0, 3)


def test_full_image_chunked_eval_flow():
    """BASELINE config C5 shape on one GPU: pose -> on-device rays -> chunked eval render without `raw`; the last
    ray chunk is ragged (762048 = 11 x 65536 + 41152) and a rank's pixel block renders the same as the full image."""
    from nerf_sos_amd import sharding
    H, W, f = 756, 1008, 850.0
    K = [[f, 0, W / 2], [0, f, H / 2], [0, 0, 1]]
    c2w = [[1, 0, 0, 0.1], [0, 1, 0, -0.2], [0, 0, 1, 0.3]]
    torch.manual_seed(0)
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, ray_chunk=65536).to(DEV).eval()
    net.load_state_dict(tp.make_peaky({k: v.cpu() for k, v in net.state_dict().items()}, gain=40.0, shift=1.0))
    rays = ops.generate_rays(H, W, K, c2w, DEV)
    with torch.no_grad():
        full = net(rays, (tp.NEAR, tp.FAR), retraw=False)
    assert full["rgb"].shape == (H, W, 3) and full["weights"].shape == (H, W, 192) and "raw" not in full
    assert torch.isfinite(full["rgb"]).all() and full["acc"].max() <= 1 + 1e-5 and full["acc"].max() > 0.5
    b, e = sharding.shard_bounds(H * W, 3, 8)        # what rank 3 of 8 would render
    part = ops.generate_rays(H, W, K, c2w, DEV, pix_range=(b, e))
    with torch.no_grad():
        mine = net(part, (tp.NEAR, tp.FAR), retraw=False)
    for k in ("rgb", "depth", "acc", "weights"):
        assert torch.equal(mine[k], full[k].reshape(H * W, -1)[b:e].reshape(mine[k].shape)), k


# ------------------------------------------------------------------------------------------ K2-LP (reduced precision)
@pytest.fixture
def lp_kernel():
    """Select one of the two 16-bit MLP kernels for a test (1 = mlp_lp_kernel, 3 = mlp_lp16_kernel, the default) and restore the
    default afterwards."""
    lib = _lib.lib()

    def select(which):
        _lib.check(lib.nsos_mlp_lp_select_kernel(which), "select")
    yield select
    _lib.check(lib.nsos_mlp_lp_select_kernel(3), "select")


@pytest.mark.parametrize("kernel", [1, 3])
@pytest.mark.parametrize("precision,tol", [("fp16", 3e-3), ("bf16", 3e-2)])
@pytest.mark.parametrize("name", list(CFGS))
def test_mlp_lp_vs_emulation(manifest, name, precision, tol, kernel, lp_kernel):
    """16-bit-input MFMA kernels vs their torch emulation (same roundings, fp64 accumulation): agreement is limited
    by rare 1-ulp rounding flips of 16-bit activations, far below the format's own error against fp32.  kernel 1 = the
    round-1 kernel, 3 = mlp_lp16_kernel (16x16x32 tiles: fp32 hidden
    biases, 16-bit output heads -- its own emulation variant)."""
    lp_kernel(kernel)
    sd = ref_state(name, manifest, peaky=False)
    cfg = tp.PortConfig(**CFGS[name])
    mode = ops.sem_mode_of(**CFGS[name])
    rays = tp.synthetic_rays(70, seed=2)
    o, d = T(rays[0]), T(rays[1])
    near, far = torch.full((70,), tp.NEAR, device=DEV), torch.full((70,), tp.FAR, device=DEV)
    for S in (64, 192, 50):  # 50: ragged tail inside a 256-point tile
        z, v = ops.ray_setup(d, near, far, S, torch.rand(70, S, device=DEV))
        params = {k[len("nerf_fine") + 5:]: t.to(DEV) for k, t in sd.items() if k.startswith("nerf_fine.mlp.")}
        packed = ops.pack_mlp(params, mode, precision=precision)
        raw = ops.mlp_forward_rays_lp(packed, mode, precision, o, d, v, z)
        again = ops.mlp_forward_rays_lp(packed, mode, precision, o, d, v, z)
        assert torch.equal(raw, again), "reduced-precision kernel is not deterministic"
        pts = tp.ray_points(rays[0], rays[1], z.cpu())
        dirs = v.cpu()[:, None, :].expand(70, S, 3)
        dt = torch.float16 if precision == "fp16" else torch.bfloat16
        ref = tp.point_query_lp(sd, "nerf_fine", pts, dirs, cfg, dt, lp16=(kernel == 3))
        err = (raw.cpu() - ref).abs()
        scale = 1.0 + ref.abs()
        assert (err / scale).max() < tol, f"{precision} {name} S={S}: max rel err {(err / scale).max():.3e}"
        assert (err / scale).mean() < tol / 4, f"{precision} {name} S={S}: mean rel err {(err / scale).mean():.3e}"
        # and against the exact fp32 kernel: the format's own error
        raw32 = ops.mlp_forward_rays(ops.pack_mlp(params, mode), mode, o, d, v, z)
        fmt = ((raw - raw32).abs() / (1.0 + raw32.abs())).max().item()
        assert fmt < (2e-2 if precision == "fp16" else 1.5e-1), f"{precision} vs fp32 kernel: {fmt:.3e}"


# ------------------------------------------------------------------------------------------ K2-X3 (split fp16, fp32-grade)
@pytest.mark.parametrize("name", list(CFGS))
@pytest.mark.parametrize("peaky", [False, True])
def test_mlp_x3_is_fp32_grade(golden, manifest, name, peaky):
    """Split-fp16 kernel (hi.hi + hi.lo + lo.hi on the 16-bit matrix pipe): against the reference's own fp32 outputs it
    must meet the SAME bar as the exact-fp32 kernel (2e-5 here; the north star asks for 1e-4), and against the fp64
    oracle its error must stay within a small multiple of what fp32 arithmetic itself commits."""
    g = golden("mlp")
    sd = ref_state(name, manifest, peaky)
    tag = tag_of(name, peaky)
    mode = ops.sem_mode_of(**CFGS[name])
    P = g["pts"].shape[0]
    o, z = T(g["pts"]), torch.zeros((P, 1), device=DEV)      # one-sample rays: x = o + d * 0
    dirs = T(g["dirs"])
    for prefix in ("nerf", "nerf_fine"):
        params = {k[len(prefix) + 5:]: v.to(DEV) for k, v in sd.items() if k.startswith(prefix + ".mlp.")}
        packed = ops.pack_mlp(params, mode, precision="fp16x3")
        raw = ops.mlp_forward_rays_lp(packed, mode, "fp16x3", o, dirs, dirs, z).reshape(P, -1)
        again = ops.mlp_forward_rays_lp(packed, mode, "fp16x3", o, dirs, dirs, z).reshape(P, -1)
        assert torch.equal(raw, again), "split-fp16 kernel is not deterministic"
        close(N(raw), g[f"{tag}_{prefix}_raw"], atol=2e-5, rtol=2e-5, what=f"x3 {tag} {prefix} vs reference")
        raw32 = ops.mlp_forward_points(ops.pack_mlp(params, mode), mode, o, dirs)
        close(N(raw), N(raw32), atol=1e-5, rtol=1e-5, what=f"x3 {tag} {prefix} vs exact-fp32 kernel")


@pytest.mark.parametrize("S", [64, 192, 50, 1])
def test_mlp_x3_ragged_tiles(manifest, S):
    """tile = 128 points: ragged tails, several tiles per workgroup, guard band untouched"""
    sd = ref_state("semcoord", manifest, peaky=True)
    R = 77 if S > 1 else 128 * 300 + 5
    rays = tp.synthetic_rays(R, seed=3)
    o, d = T(rays[0]), T(rays[1])
    near, far = torch.full((R,), tp.NEAR, device=DEV), torch.full((R,), tp.FAR, device=DEV)
    z, v = ops.ray_setup(d, near, far, max(S, 2), torch.rand(R, max(S, 2), device=DEV))
    z = z[:, :S].contiguous()
    params = {k[len("nerf_fine") + 5:]: t.to(DEV) for k, t in sd.items() if k.startswith("nerf_fine.mlp.")}
    guard = torch.full((R * S + 64, 6), 777.0, device=DEV)
    raw = ops.mlp_forward_rays_lp(ops.pack_mlp(params, 2, precision="fp16x3"), 2, "fp16x3", o, d, v, z)
    raw32 = ops.mlp_forward_rays(ops.pack_mlp(params, 2), 2, o, d, v, z)
    close(N(raw), N(raw32), atol=1e-5, rtol=1e-5, what=f"x3 S={S}")
    assert (guard == 777.0).all()


@pytest.mark.parametrize("sem", [0, 1, 2])
def test_both_split_fp16_forward_kernels_agree(manifest, sem):
    """nsos_mlp_x3_select_kernel: 2 = mlp_x316_kernel (16x16x32, the default since round 6), 1 = mlp_x3_kernel (32x32x16, rounds 2-5; still
    the training variants' kernel).  Same packed buffer (two streams), same inputs, every semantic mode, a ragged point count: both
    within 1e-5 of the exact kernel and within 2e-6 of each other (other contraction order inside the MFMAs; measured 3e-7)."""
    from nerf_sos_amd import _lib
    name = {0: "nosem", 1: "sem", 2: "semcoord"}[sem]
    sd = ref_state(name, manifest, peaky=True)
    R, S = 93, 37                                   # 3441 points: a ragged last tile for both kernels (128-point tiles)
    rays = tp.synthetic_rays(R, seed=8)
    o, d = T(rays[0]), T(rays[1])
    near, far = torch.full((R,), tp.NEAR, device=DEV), torch.full((R,), tp.FAR, device=DEV)
    z, v = ops.ray_setup(d, near, far, S, torch.rand(R, S, device=DEV))
    params = {k[len("nerf_fine") + 5:]: t.to(DEV) for k, t in sd.items() if k.startswith("nerf_fine.mlp.")}
    packed = ops.pack_mlp(params, sem, precision="fp16x3")
    exact = ops.mlp_forward_rays(ops.pack_mlp(params, sem), sem, o, d, v, z)
    outs = {}
    assert _lib.lib().nsos_mlp_x3_selected_kernel() == 2
    try:
        for k in (1, 2):
            _lib.check(_lib.lib().nsos_mlp_x3_select_kernel(k), "select")
            outs[k] = ops.mlp_forward_rays_lp(packed, sem, "fp16x3", o, d, v, z).clone()
            close(N(outs[k]), N(exact), atol=1e-5, rtol=1e-5, what=f"split-fp16 kernel {k}, sem_mode {sem}, vs the exact kernel")
    finally:
        _lib.check(_lib.lib().nsos_mlp_x3_select_kernel(2), "select")
    close(N(outs[2]), N(outs[1]), atol=2e-6, rtol=2e-6, what=f"mlp_x316_kernel vs mlp_x3_kernel, sem_mode {sem}")


def test_render_x3_end_to_end(manifest):
    """whole pipeline with mlp_precision = "fp16x3": same keys, and everything that is not an index-flip casualty
     within the fp32 parity tolerance of the exact path"""
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, use_semantics=True, sem_with_coord=True).to(DEV).eval()
    net.load_state_dict(ref_state("semcoord", manifest, peaky=True))
    rays = tp.synthetic_rays(1024, seed=4).to(DEV)
    with torch.no_grad():
        a = net(rays, (tp.NEAR, tp.FAR))
        net.mlp_precision = "fp16x3"
        b = net(rays, (tp.NEAR, tp.FAR))
    assert set(a) == set(b)
    for k in ("rgb0", "depth0", "acc0", "weights0", "semantics0"):   # coarse pass: no resampling in front of it
        close(N(b[k]), N(a[k]), atol=1e-5, rtol=1e-4, what=k)
    for k in ("rgb", "depth", "acc", "semantics"):
        bad = ((a[k] - b[k]).abs() > 1e-4 + 1e-4 * a[k].abs()).reshape(1024, -1).any(-1).float().mean().item()
        assert bad < 0.01, f"{k}: {bad:.4f} of the rays differ from the exact path by more than 1e-4"


@pytest.mark.parametrize("name", ["semcoord", "sem"])
def test_x3_frozen_backbone_training(manifest, name):
    """--fix_backbone training on the split-fp16 kernel: its SAVE variant returns the inference outputs (bit-identical within a kernel
    family; to fp32 rounding across the two forward kernels), and the
    semantic-head gradients equal the exact-fp32 path's to fp32-rounding accuracy (coarse-only net: no resampling
    between the two arithmetics, so the comparison is not blurred by index flips)."""
    cfg = CFGS[name]
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=0, perturb=0., raw_noise_std=0., **cfg).to(DEV)
    net.load_state_dict(tp.make_peaky(tp.init_state_dict(tp.PortConfig(n_importance=0, **cfg), seed=0)))
    _frozen(net).train()
    rays = tp.synthetic_rays(300, seed=5).to(DEV)
    grads = {}
    for prec in ("fp32", "fp16x3"):
        net.mlp_precision = prec
        net.zero_grad()
        with torch.no_grad():
            a = net(rays, (tp.NEAR, tp.FAR))
        b = net(rays, (tp.NEAR, tp.FAR))
        for k in a:
            if prec == "fp32":
                assert torch.equal(a[k], b[k].detach()), (prec, k)
            else:
                # round 6: inference runs mlp_x316_kernel (16x16x32), the SAVE variant stays on mlp_x3_kernel (32x32x16): the same split
                # arithmetic in another contraction order -- equal to fp32 rounding (measured 3e-7 on raw), no longer bit for bit
                close(N(b[k].detach()), N(a[k]), atol=2e-5, rtol=1e-5, what=f"{prec} {k}: SAVE forward vs inference forward")   # (measured <= 7.5e-6 on depth ~ 2)
        (b["semantics"].square().mean() + 0.3 * b["semantics"][:, 0].mean()).backward()
        grads[prec] = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    # ... and with the 32x32x16 kernel selected for inference the two are the same kernel family again: bit-identical
    from nerf_sos_amd import _lib
    _lib.check(_lib.lib().nsos_mlp_x3_select_kernel(1), "select")
    try:
        with torch.no_grad():
            a = net(rays, (tp.NEAR, tp.FAR))
        b = net(rays, (tp.NEAR, tp.FAR))
        for k in a:
            assert torch.equal(a[k], b[k].detach()), ("fp16x3 on mlp_x3_kernel", k)
    finally:
        _lib.check(_lib.lib().nsos_mlp_x3_select_kernel(2), "select")
    assert set(grads["fp32"]) == set(grads["fp16x3"]) and len(grads["fp32"]) == 4
    for n, g in grads["fp32"].items():
        close(N(grads["fp16x3"][n]), N(g), atol=1e-6 + 1e-5 * float(g.abs().max()), rtol=1e-4, what=n)


@pytest.mark.parametrize("precision,min_psnr", [("fp16", 55.0), ("bf16", 38.0)])
def test_render_lp_end_to_end(manifest, precision, min_psnr):
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, use_semantics=True, sem_with_coord=True).to(DEV).eval()
    net.load_state_dict(tp.make_peaky(ref_state("semcoord", manifest), gain=40.0, shift=1.0))
    rays = tp.synthetic_rays(2048, seed=4).to(DEV)
    with torch.no_grad():
        a = net(rays, (tp.NEAR, tp.FAR))
        net.mlp_precision = precision
        b = net(rays, (tp.NEAR, tp.FAR))
    assert set(a) == set(b) and b["rgb"].dtype == torch.float32
    for k in ("rgb", "rgb0"):
        mse = (a[k] - b[k]).square().mean().item()
        psnr = -10 * np.log10(max(mse, 1e-30))
        assert psnr > min_psnr, f"{precision} {k}: PSNR vs the fp32 path {psnr:.1f} dB"
    assert a["acc"].max() > 0.5


def test_coarse_precision_in_inference_and_frozen_backbone_training(manifest):
    """NeRFNet.coarse_precision (round 6): the coarse pass in one arithmetic, the fine pass in another.  (a) coarse 'fp16x3' + fine
    'bf16': the coarse outputs are the all-fp16x3 render's, the fine pass runs on the bf16 kernel at the coarse pass's sample
    positions (so it equals neither pure render: checked against a staged render with ops); (b) the frozen-backbone step saves each
    pass's head operands in that pass's format (fp32 rows for the split kernel, tile-major bf16 for the 16-bit one) and both heads get
    finite, non-zero gradients that agree with the all-fp16x3 step's to the 16-bit format's accuracy; (c) a wrong value raises."""
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, **CFGS["semcoord"]).to(DEV)
    net.load_state_dict(ref_state("semcoord", manifest, True, 128))
    _frozen(net).eval()
    rays = tp.synthetic_rays(512, seed=11).to(DEV)
    with pytest.raises(ValueError):
        net.coarse_precision = "fp8"
    with torch.no_grad():
        net.mlp_precision, net.coarse_precision = "fp16x3", None
        x3 = net(rays, (tp.NEAR, tp.FAR))
        net.mlp_precision, net.coarse_precision = "bf16", "fp16x3"
        assert net.pass_precision("coarse") == "fp16x3" and net.pass_precision("fine") == "bf16"
        mix = net(rays, (tp.NEAR, tp.FAR))
    assert set(mix) == set(x3)
    for k in ("rgb0", "depth0", "acc0", "weights0", "semantics0", "raw0", "z_std"):       # the coarse pass and its sampler: the split kernel's
        assert torch.equal(mix[k], x3[k]), k
    # the fine pass: the bf16 kernel on the positions the fp16x3 coarse pass produced
    R = rays.shape[1]
    near, far = torch.full((R,), tp.NEAR, device=DEV), torch.full((R,), tp.FAR, device=DEV)
    z, v = ops.ray_setup(rays[1].contiguous(), near, far, 64, None)
    raw0 = ops.mlp_forward_rays_lp(net.nerf.packed_weights("fp16x3"), net.nerf.sem_mode, "fp16x3", rays[0].contiguous(), rays[1].contiguous(), v, z)
    _, zf, _, _ = ops.composite_importance(raw0, z, rays[1].contiguous(), 128)
    raw = ops.mlp_forward_rays_lp(net.nerf_fine.packed_weights("bf16"), net.nerf_fine.sem_mode, "bf16", rays[0].contiguous(), rays[1].contiguous(), v, zf)
    assert torch.equal(raw.reshape(mix["raw"].shape), mix["raw"])
    # ... independent of the ray chunking, like every other mode
    net.chunk = 100
    with torch.no_grad():
        again = net(rays, (tp.NEAR, tp.FAR))
    net.chunk = 1024 * 32
    assert all(torch.equal(again[k], mix[k]) for k in mix)
    # (b) training: gradients of both heads
    grads = {}
    for name, (prec, coarse) in {"x3": ("fp16x3", None), "mixed": ("bf16", "fp16x3")}.items():
        net.mlp_precision, net.coarse_precision = prec, coarse
        net.zero_grad()
        out = net(rays, (tp.NEAR, tp.FAR))
        (out["semantics"].square().sum() + out["semantics0"].square().sum()).backward()
        grads[name] = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
        assert len(grads[name]) == 8 and all(torch.isfinite(g_).all() and g_.abs().max() > 0 for g_ in grads[name].values())
    for n_, g_ in grads["x3"].items():
        scale = float(g_.abs().max()) + 1e-12
        err = float((grads["mixed"][n_] - g_).abs().max()) / scale
        if n_.startswith("nerf."):          # the coarse head: the same kernels in both steps
            assert err <= 1e-6, (n_, err)
        else:                               # the fine head: bf16 operands (8 bits) and a spiky field -- a sanity bound, as in test_lp_training_variant
            assert err <= 0.5, (n_, err)
    net.coarse_precision = None


@pytest.mark.parametrize("precision,tol", [("fp16", 2e-2), ("bf16", 1.5e-1)])
def test_lp_training_variant(golden, manifest, precision, tol, lp_kernel):
    """Config C3: frozen-backbone training at reduced precision.  The SAVE variant of the 16-bit kernel (a) renders
    bit-identically to the inference variant, (b) stores exactly the operands the head consumed -- a torch head with
    the 16-bit-rounded first-layer weights on `sem_in` reproduces `sem_hid` and the logits -- and (c) yields
    semantic-head gradients within the format's error of the reference's fp32 gradients (default-init network; with
    the spiky test field a 16-bit sigma moves the compositing weights themselves, so there only sanity is checked)."""
    g = golden("sem_grads")
    rays = T(g["rays"])
    # (a) two-pass spiky field: identical to inference, finite gradients on the heads only
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, **CFGS["semcoord"]).to(DEV)
    net.load_state_dict(ref_state("semcoord", manifest, True, 128))
    _frozen(net).eval()
    net.mlp_precision = precision
    with torch.no_grad():
        a = net(rays, (tp.NEAR, tp.FAR))
    b = net(rays, (tp.NEAR, tp.FAR))
    for k in a:
        assert torch.equal(a[k], b[k].detach()), k
    (b["semantics"].square().sum() + b["semantics0"].square().sum()).backward()
    for n, p in net.named_parameters():
        assert (p.grad is None) == ('semantic_linear' not in n)
        assert p.grad is None or (torch.isfinite(p.grad).all() and p.grad.abs().max() > 0)
    # (c) coarse-only default-init network against the reference's fp32 gradients
    tag = tag_of("semcoord", False, False, True)
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=0, **CFGS["semcoord"]).to(DEV)
    net.load_state_dict(ref_state("semcoord", manifest, False, 0))
    _frozen(net).eval()
    net.mlp_precision = precision
    ret = net(rays, (tp.NEAR, tp.FAR))
    (ret["semantics"] * T(g[f"{tag}_G"])).sum().backward()
    sd = dict(net.named_parameters())
    keys = [k[len(tag) + 6:] for k in g if k.startswith(tag + "_grad_")]
    assert len(keys) == 4
    for k in keys:
        want = g[f"{tag}_grad_{k}"]
        got = N(sd[k].grad)
        scale = np.abs(want).max() + 1e-12
        assert np.abs(got - want).max() <= tol * scale, f"{precision} grad {k}: {np.abs(got - want).max() / scale:.3e} of scale"
    # (b) the saved operands, straight from the kernel -- of the round-1 kernel first (fp32 and compact), then of mlp_lp16_kernel
    # (the default)
    lp_kernel(1)
    mode = ops.sem_mode_of(**CFGS["semcoord"])
    R = rays.shape[1]
    near, far = torch.full((R,), tp.NEAR, device=DEV), torch.full((R,), tp.FAR, device=DEV)
    z, v = ops.ray_setup(rays[1], near, far, 64, None)
    mlp = net.nerf.mlp
    raw, sem_in, sem_hid = ops.mlp_forward_rays_save(net.nerf.packed_weights(precision), mode, rays[0].contiguous(),
                                                     rays[1].contiguous(), v, z, precision)
    raw_inf = ops.mlp_forward_rays_lp(net.nerf.packed_weights(precision), mode, precision, rays[0].contiguous(),
                                      rays[1].contiguous(), v, z)
    assert torch.equal(raw, raw_inf)
    dt = torch.float16 if precision == "fp16" else torch.bfloat16
    assert torch.equal(sem_in, sem_in.to(dt).float()) and (sem_in[:, 319] == 1).all() and (sem_in[:, :256] >= 0).all()
    raw_c, sem_in_c, sem_hid_c = ops.mlp_forward_rays_save(net.nerf.packed_weights(precision), mode, rays[0].contiguous(),
                                                            rays[1].contiguous(), v, z, precision, compact=True)
    # compact: BOTH saved matrices in the 16-bit format -- sem_in's values are 16-bit anyway (identical), sem_hid is the fp32
    # accumulator's relu rounded to nearest even (what torch's own conversion gives)
    # (the round-1 kernel hands both back row-major; the default kernel's are tile-major -- [groups of 32 points, 20, 64, 8],
    #  include/nerf_sos_hip.h -- and ops.sem_in_rows is the [P,320] view of either)
    assert sem_in_c.dtype == dt and sem_in_c.dim() == 2 and torch.equal(ops.sem_in_rows(sem_in_c, R * 64).float(), sem_in) and torch.equal(raw_c, raw)
    assert torch.equal(ops.sem_in_rows(ops.sem_in_tiled(sem_in.to(dt)), R * 64), sem_in.to(dt))
    assert sem_hid_c.dtype == dt and torch.equal(sem_hid_c, sem_hid.to(dt)) and torch.equal(sem_hid_c > 0, sem_hid.to(dt) > 0)
    W1 = mlp.semantic_linear[0].weight.detach().to(dt).double()
    b1 = mlp.semantic_linear[0].bias.detach().to(dt).double()
    hid = torch.relu(sem_in[:, :W1.shape[1]].double() @ W1.T + b1).float()
    assert (hid - sem_hid).abs().max() < 1e-4 * (1 + sem_hid.abs().max())
    # mlp_lp16_kernel: renders like its own inference variant bit for bit; its operands are self-consistent the same way (the
    # head's hidden activations are stored as the 16-bit values the logit MFMAs consumed) and agree with the round-1 kernel's operands to the
    # format's rounding (another contraction order upstream)
    lp_kernel(3)
    raw16, sem_in16, sem_hid16 = ops.mlp_forward_rays_save(net.nerf.packed_weights(precision), mode, rays[0].contiguous(),
                                                           rays[1].contiguous(), v, z, precision, compact=True)
    raw16_inf = ops.mlp_forward_rays_lp(net.nerf.packed_weights(precision), mode, precision, rays[0].contiguous(), rays[1].contiguous(), v, z)
    assert torch.equal(raw16, raw16_inf)
    rows16 = ops.sem_in_rows(sem_in16, R * 64).float()
    assert sem_in16.dtype == dt and (rows16[:, 319] == 1).all() and (rows16[:, :256] >= 0).all()
    fmt = 2.0 ** -10 if precision == "fp16" else 2.0 ** -7
    # the encoding columns: the same features rounded to the same format; the lp16 encoder forms cos as sin(2 pi (frac + 1/4)),
    # which can land on the neighbouring 16-bit value
    enc_diff = (rows16[:, 256:] - sem_in[:, 256:]).abs()
    assert float(enc_diff.max()) <= fmt * (1 + float(sem_in[:, 256:].abs().max())) and float((enc_diff > 0).float().mean()) < 0.02
    assert (rows16[:, :256] - sem_in[:, :256]).abs().max() <= 8 * fmt * (1 + sem_in[:, :256].abs().max())
    hid16 = torch.relu(rows16[:, :W1.shape[1]].double() @ W1.T + b1).float()
    assert sem_hid16.dim() == 4, "the default kernel stores the hidden activations tile-major"
    sem_hid16 = ops.sem_hid_rows(sem_hid16, R * 64)
    assert (hid16.to(dt).float() - sem_hid16.float()).abs().max() <= 2 * fmt * (1 + hid16.abs().max())
    W2 = mlp.semantic_linear[2].weight.detach().to(dt).double()
    logits = sem_hid16.double() @ W2.T + mlp.semantic_linear[2].bias.detach().double()
    assert (logits.float() - raw16.reshape(-1, 6)[:, 4:]).abs().max() < 1e-4 * (1 + logits.abs().max())
    logits = sem_hid @ mlp.semantic_linear[2].weight.detach().T + mlp.semantic_linear[2].bias.detach()
    assert (logits - raw[..., 4:6].reshape(-1, 2)).abs().max() < 1e-4 * (1 + logits.abs().max())


@pytest.mark.parametrize("precision", ["fp32", "fp16", "fp16x3", "fp16+coarse_fp16x3"])
def test_graphed_render_equals_eager(manifest, precision):
    """hipGraph capture of the eval-mode step: replay is bit-identical to the eager launches, for new inputs too (round 6: also on the
    16x16x32 split kernel and with the coarse pass in another precision than the fine one)."""
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, use_semantics=True, sem_with_coord=True).to(DEV).eval()
    net.load_state_dict(ref_state("semcoord", manifest, peaky=True))
    net.validate_precision = False              # (the range guard renders twice outside any capture; not what is tested here)
    if "+" in precision:
        net.mlp_precision, net.coarse_precision = "fp16", "fp16x3"
    else:
        net.mlp_precision = precision
    g = nerf_sos_amd.GraphedRender(net, 300, (tp.NEAR, tp.FAR), retraw=False)
    for seed in (1, 2):
        rays = tp.synthetic_rays(300, seed=seed).to(DEV)
        with torch.no_grad():
            want = net(rays, (tp.NEAR, tp.FAR), retraw=False)
        got = g(rays)
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k
    with torch.no_grad():                       # trainable net: the pack launches are in the graph, a replay follows
        net.nerf_fine.mlp.rgb_linear.bias.add_(0.1)   # in-place parameter updates (optimizer steps, fused or not)
        want = net(rays, (tp.NEAR, tp.FAR), retraw=False)
    got = g(rays)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    for p in net.parameters():
        p.requires_grad_(False)
    g = nerf_sos_amd.GraphedRender(net, 300, (tp.NEAR, tp.FAR), retraw=False)
    with torch.no_grad():                       # frozen net: packed once outside the graph -> a change must be refused
        net.nerf.mlp.rgb_linear.bias.add_(0.1)
    with pytest.raises(RuntimeError, match="re-capture"):
        g(rays)


@pytest.mark.parametrize("precision", ["fp32", "fp16", "fp16x3"])
def test_nan_and_inf_inputs_stay_in_their_ray(manifest, precision):
    """The reference raises nothing on bad numbers: NaN/Inf propagate silently (SURVEY 8b "Errors").  Here too (the
    kernels poison the outputs of a point whose inputs are not finite: their ReLUs alone would launder a NaN to 0) -- and
    a bad ray must not disturb its neighbours in the same tile (rays are independent end to end)."""
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, use_semantics=True, sem_with_coord=True).to(DEV).eval()
    net.load_state_dict(ref_state("semcoord", manifest, peaky=True))
    net.mlp_precision = precision
    rays = tp.synthetic_rays(70, seed=6).to(DEV)
    with torch.no_grad():
        good = net(rays, (tp.NEAR, tp.FAR))
        bad_rays = rays.clone()
        bad_rays[1, 5, 0] = float("nan")       # direction of ray 5
        bad_rays[0, 9, 2] = float("inf")       # origin of ray 9
        bad = net(bad_rays, (tp.NEAR, tp.FAR))
    torch.cuda.synchronize()
    for r in (5, 9):
        assert torch.isnan(bad["rgb"][r]).all() and torch.isnan(bad["raw"][r]).all() and torch.isnan(bad["semantics0"][r]).all(), r
    keep = [i for i in range(70) if i not in (5, 9)]
    for k in ("rgb", "depth", "acc", "weights", "semantics", "rgb0", "weights0"):
        assert torch.equal(bad[k][keep], good[k][keep]), k


@pytest.mark.parametrize("n_coarse", [32, 96, 130])
def test_per_call_sample_count_override(manifest, n_coarse):
    """`N_samples` is a per-call kwarg in the reference (models/sampler.py:41); the fine pass still draws the
    constructor's N_importance samples (models/sampler.py:100,103).  32 coarse + 128 new = 160 fine samples; more than 64
    coarse samples take the general importance kernel (several coarse samples per lane) and the unfused compositing."""
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, **CFGS["semcoord"]).to(DEV).eval()
    sd = ref_state("semcoord", manifest)
    net.load_state_dict(sd)
    rays = tp.synthetic_rays(40, seed=12)
    with torch.no_grad():
        out = net(rays.to(DEV), (tp.NEAR, tp.FAR), N_samples=n_coarse)
    cfg = tp.PortConfig(n_samples=n_coarse, n_importance=128, **CFGS["semcoord"])
    ref = tp.render(sd, cfg, rays, (tp.NEAR, tp.FAR))
    M = n_coarse + 128
    assert out["weights"].shape == (40, M) and out["weights0"].shape == (40, n_coarse) and out["raw"].shape == (40, M, 6)
    for k in ("rgb0", "depth0", "weights0", "semantics0"):
        close(N(out[k]), ref[k].numpy(), atol=1e-4, rtol=1e-4, what=k)
    for k in ("rgb", "acc", "semantics"):   # fine pass: bulk agreement (index flips)
        bad = (np.abs(N(out[k]) - ref[k].numpy()) > 1e-4 * (1 + np.abs(ref[k].numpy()))).any(-1).mean()
        assert bad * 40 <= 1.5, (k, bad)       # measured (round 4): at most 1 of the 40 rays (an index flip)
    net.train()                              # train mode: jitter + noise draws at the overridden count
    tr = net(rays.to(DEV), (tp.NEAR, tp.FAR), N_samples=n_coarse, raw_noise_std=1.0)
    assert tr["weights"].shape == (40, M) and bool(torch.isfinite(tr["rgb"]).all())
    assert bool((tr["weights"] >= 0).all())


def test_per_call_kwargs_follow_the_reference(manifest):
    """Per-call kwargs: N_importance=0 disables the fine pass for that call; a different positive value does
    NOT change the sample count (models/sampler.py:100,103); retpts adds pts / pts0; perturb / raw_noise_std override the
    mode defaults; unknown kwargs are ignored."""
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, **CFGS["semcoord"]).to(DEV).eval()
    net.load_state_dict(ref_state("semcoord", manifest))
    rays = tp.synthetic_rays(20, seed=14).to(DEV)
    with torch.no_grad():
        full = net(rays, (tp.NEAR, tp.FAR), radii=0.01, some_unknown_flag=True)
        coarse = net(rays, (tp.NEAR, tp.FAR), N_importance=0)
        other = net(rays, (tp.NEAR, tp.FAR), N_importance=17)
        pts = net(rays, (tp.NEAR, tp.FAR), retpts=True, retraw=False)
        noisy = net(rays, (tp.NEAR, tp.FAR), perturb=1.0, raw_noise_std=1.0)
    assert "rgb0" in full and "z_std" in full and full["weights"].shape == (20, 192)
    assert "rgb0" not in coarse and "z_std" not in coarse and coarse["weights"].shape == (20, 64)
    assert torch.equal(coarse["rgb"], full["rgb0"]) and torch.equal(coarse["raw"], full["raw0"])
    assert other["weights"].shape == (20, 192) and torch.equal(other["rgb"], full["rgb"])
    assert pts["pts"].shape == (20, 192, 3) and pts["pts0"].shape == (20, 64, 3) and "raw" not in pts
    assert torch.equal(pts["rgb"], full["rgb"])
    assert not torch.equal(noisy["rgb"], full["rgb"]) and noisy["weights"].shape == (20, 192)
    with pytest.raises(AssertionError):
        net((rays[0], rays[1][:10]), (tp.NEAR, tp.FAR))


@pytest.mark.parametrize("which", ["fp32", "fp16", "fp16x3"])
def test_phase_profile_entries_stamp_monotonically_and_leave_results_alone(manifest, which):
    """The diagnostics entry points (nsos_mlp_profile_rays[_lp|_x3]: shader-clock stamps per kernel phase, the source of the
    phase tables under profiles/) must not change the kernel's output, and their stamps must increase along a tile."""
    import ctypes as C
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128).to(DEV).eval()
    R, S = 700, 192                                  # > 2 tiles per workgroup on 256 CUs: the stamped (second) tile exists
    rays = tp.synthetic_rays(R, seed=0).to(DEV)
    near, far = torch.full((R,), tp.NEAR, device=DEV), torch.full((R,), tp.FAR, device=DEV)
    z, v = ops.ray_setup(rays[1], near, far, S, None)
    o, d = rays[0].contiguous(), rays[1].contiguous()
    P_ = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    packed = net.nerf_fine.packed_weights(which)
    raw = torch.empty(R, S, 4, device=DEV)
    stamps = torch.zeros(16 * 64, dtype=torch.int64, device=DEV)
    lib = _lib.lib()
    if which == "fp32":
        rc = lib.nsos_mlp_profile_rays(P_(packed), 0, P_(o), P_(d), P_(v), P_(z), R, S, P_(raw), P_(stamps), None)
        want = ops.mlp_forward_rays(packed, 0, o, d, v, z)
    elif which == "fp16":
        rc = lib.nsos_mlp_profile_rays_lp(P_(packed), 0, 1, P_(o), P_(d), P_(v), P_(z), R, S, P_(raw), P_(stamps), None)
        want = ops.mlp_forward_rays_lp(packed, 0, "fp16", o, d, v, z)
    else:
        rc = lib.nsos_mlp_profile_rays_x3(P_(packed), 0, P_(o), P_(d), P_(v), P_(z), R, S, P_(raw), P_(stamps), None)
        want = ops.mlp_forward_rays_lp(packed, 0, "fp16x3", o, d, v, z)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(raw, want)
    st = stamps.cpu().view(16, 64)[:, :60]            # (the 16-bit kernel keeps a wave's first / last cycle in slots 62, 63)
    used = st[0] > 0
    assert int(used.sum()) >= 8, "no stamps were taken"
    seq = st[0][used]
    assert (seq[1:] >= seq[:-1]).all()


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["sem", "semcoord"])
def test_heads_only_repack_equals_a_full_pack(manifest, name, precision):
    """nsos_mlp_pack_lp_heads (what a frozen-backbone training step re-packs: the semantic head's chunks of the selected kernel's
    stream, with the vector-ALU heads' block where that kernel reads it) into a buffer holding a full pack of OLD head weights == a fresh full pack of the new ones, byte for
    byte -- and NeRFMLP.packed_weights takes that path exactly when only semantic_linear.* is trainable."""
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, **CFGS[name]).to(DEV)
    net.load_state_dict(ref_state(name, manifest, peaky=True))
    mlp = net.nerf_fine
    params = dict(mlp.mlp.named_parameters())
    plan = ops.PackPlan({k: v for k, v in params.items()}, mlp.sem_mode)
    old = plan.run(None, precision).clone()
    with torch.no_grad():
        for k, v in params.items():
            if "semantic_linear" in k:
                v.add_(torch.randn_like(v) * 0.05)
    fresh = plan.run(None, precision)
    # the re-pack touches the stream of the SELECTED kernel only: per kernel, a render from the partly re-packed buffer equals the
    # render from a fresh full pack, and after both selections the buffer is the fresh pack byte for byte
    rays = tp.synthetic_rays(64, seed=3).to(DEV)
    o, d = rays[0].contiguous(), rays[1].contiguous()
    z, v = ops.ray_setup(d, torch.full((64,), tp.NEAR, device=DEV), torch.full((64,), tp.FAR, device=DEV), 48, None)
    part = old
    try:
        for k in (1, 3):
            _lib.check(_lib.lib().nsos_mlp_lp_select_kernel(k), "select")
            assert ops.lp_selected_kernel() == k
            part = plan.run(part, precision, heads_only=True)
            assert part.data_ptr() == old.data_ptr()
            assert torch.equal(ops.mlp_forward_rays_lp(part, mlp.sem_mode, precision, o, d, v, z),
                               ops.mlp_forward_rays_lp(fresh, mlp.sem_mode, precision, o, d, v, z)), f"kernel {k}: heads-only re-pack != full pack"
            if k == 1:
                assert not torch.equal(part.view(torch.int32), fresh.view(torch.int32))     # the other stream still holds the old heads
    finally:
        _lib.check(_lib.lib().nsos_mlp_lp_select_kernel(3), "select")
    assert torch.equal(part.view(torch.int32), fresh.view(torch.int32)), "heads-only re-packs of both streams != full pack"
    # the module: frozen trunk, trainable heads -> first call full, later calls heads-only; results follow in-place updates
    for n_, p_ in net.named_parameters():
        p_.requires_grad = "semantic_linear" in n_
    a = mlp.packed_weights(precision).clone()
    with torch.no_grad():
        params["semantic_linear.2.bias"].add_(1.0)
        params["semantic_linear.0.weight"].mul_(1.25)
    b = mlp.packed_weights(precision)
    assert not torch.equal(a.view(torch.int32), b.view(torch.int32))
    full = plan.run(None, precision)
    # only the stream of the selected kernel is current; the other keeps the old heads until the next full pack
    assert not torch.equal(b.view(torch.int32), full.view(torch.int32))
    r_sel = ops.mlp_forward_rays_lp(b, mlp.sem_mode, precision, o, d, v, z)
    assert torch.equal(r_sel, ops.mlp_forward_rays_lp(full, mlp.sem_mode, precision, o, d, v, z))
    # ... and a launch that would take another stream REFUSES instead of rendering stale heads: the fp32-sem_in save
    # always runs the round-1 kernel on stream 0; so does any launch once another kernel is selected
    with pytest.raises(RuntimeError, match="heads-only"):
        ops.mlp_forward_rays_save(b, mlp.sem_mode, o, d, v, z, precision, compact=False)
    try:
        _lib.check(_lib.lib().nsos_mlp_lp_select_kernel(1), "select")
        with pytest.raises(RuntimeError, match="heads-only"):
            ops.mlp_forward_rays_lp(b, mlp.sem_mode, precision, o, d, v, z)
    finally:
        _lib.check(_lib.lib().nsos_mlp_lp_select_kernel(3), "select")
    ops.mlp_forward_rays_save(full, mlp.sem_mode, o, d, v, z, precision, compact=False)      # (a full pack serves every stream)
    assert torch.equal(ops.mlp_forward_rays_lp(b, mlp.sem_mode, precision, o, d, v, z), ops.mlp_forward_rays_lp(full, mlp.sem_mode, precision, o, d, v, z))
    # a change of the kernel selection forces a full pack (the other stream's heads would be stale)
    try:
        _lib.check(_lib.lib().nsos_mlp_lp_select_kernel(1), "select")
        with torch.no_grad():
            params["semantic_linear.2.bias"].add_(1.0)
        c = mlp.packed_weights(precision)
        assert torch.equal(c.view(torch.int32), plan.run(None, precision).view(torch.int32))
    finally:
        _lib.check(_lib.lib().nsos_mlp_lp_select_kernel(3), "select")


# ------------------------------------------------------------------------------------------ K2-LP16 (16x16x32 tiles; the default)
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["nosem", "sem", "semcoord"])
def test_lp16_ragged_counts_and_agreement_with_lp4(manifest, name, precision, lp_kernel):
    """mlp_lp16_kernel (round 4, the default 16-bit kernel) on ragged point counts (single points, partial waves, partial
    16-point column blocks, sample counts that straddle tiles): deterministic, finite, rows past the end untouched, the training
    variant renders bit-identically to inference -- and it agrees with mlp_lp_kernel to the 16-bit format's rounding (the two
    contract in different orders and round the output heads differently; each is held to its own emulation in
    test_mlp_lp_vs_emulation)."""
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, **CFGS[name]).to(DEV).eval()
    net.load_state_dict(ref_state(name, manifest, peaky=True))
    mlp = net.nerf_fine
    pk = mlp.packed_weights(precision)
    fmt = 2.0 ** -10 if precision == "fp16" else 2.0 ** -7
    for R, S in ((1, 1), (3, 7), (1, 17), (5, 64), (37, 192), (257, 33), (1024, 192)):
        rays = tp.synthetic_rays(R, seed=R).to(DEV)
        o, d = rays[0].contiguous(), rays[1].contiguous()
        near = torch.full((R,), tp.NEAR, device=DEV)
        far = torch.full((R,), tp.FAR, device=DEV)
        v = ops.ray_setup(d, near, far, 2, None)[1]
        z = (tp.NEAR + (tp.FAR - tp.NEAR) * torch.rand(R, S, generator=torch.Generator().manual_seed(S))).sort(-1).values.to(DEV)
        lp_kernel(1)
        ref = ops.mlp_forward_rays_lp(pk, mlp.sem_mode, precision, o, d, v, z)
        lp_kernel(3)
        out = ops.mlp_forward_rays_lp(pk, mlp.sem_mode, precision, o, d, v, z)
        again = ops.mlp_forward_rays_lp(pk, mlp.sem_mode, precision, o, d, v, z)
        assert torch.equal(out, again), f"not deterministic at R={R}, S={S}"
        assert torch.isfinite(out).all()
        err = ((out - ref).abs() / (1 + ref.abs()))
        assert float(err.max()) <= 40 * fmt and float(err.mean()) <= 2 * fmt, (R, S, float(err.max()), float(err.mean()))
        if name != "nosem":
            sv = ops.mlp_forward_rays_save(pk, mlp.sem_mode, o, d, v, z, precision, compact=True)
            assert torch.equal(sv[0], out), "the training variant renders bit-identically to inference"
            rows = ops.sem_in_rows(sv[1], R * S).float()
            hid_rows = ops.sem_hid_rows(sv[2], R * S).float()        # (rows past the last point of the last group are never written)
            assert bool((rows[:, 319] == 1).all()) and bool((rows[:, :256] >= 0).all()) and bool(torch.isfinite(hid_rows).all()) and bool((hid_rows >= 0).all())


# ------------------------------------------------------------------------------------------ K2-LP (round 1; the fall-back)
@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("name", ["nosem", "sem", "semcoord"])
def test_lp4_ragged_counts_and_saved_operands(manifest, name, precision):
    """mlp_lp_kernel (round 1: 4 waves x 64 points; the kernel behind the fp32 saved operands and launches of >= 2^31 points, and
    the one that carries the accuracy tests against the emulation) on ragged point counts (partial tiles, single points) and
    ray-mode sample counts that straddle tiles: deterministic and finite; the training (SAVE) variants render bit-identically to
    inference; the compact operands come back row-major and are the fp32 ones in the 16-bit format (sem_in exactly -- its values
    are 16-bit anyway --, sem_hid rounded to nearest even).  The selector refuses everything but its two kernels."""
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, **CFGS[name]).to(DEV).eval()
    net.load_state_dict(ref_state(name, manifest, peaky=True))
    mlp = net.nerf_fine
    pk = mlp.packed_weights(precision)
    lib = _lib.lib()
    dt = torch.float16 if precision == "fp16" else torch.bfloat16
    try:
        _lib.check(lib.nsos_mlp_lp_select_kernel(1), "select")
        for R, S in ((1, 1), (3, 7), (5, 64), (37, 192), (257, 33), (1024, 192)):
            rays = tp.synthetic_rays(R, seed=R).to(DEV)
            o, d = rays[0].contiguous(), rays[1].contiguous()
            near = torch.full((R,), tp.NEAR, device=DEV)
            far = torch.full((R,), tp.FAR, device=DEV)
            v = ops.ray_setup(d, near, far, 2, None)[1]
            z = (tp.NEAR + (tp.FAR - tp.NEAR) * torch.rand(R, S, generator=torch.Generator().manual_seed(S))).sort(-1).values.to(DEV)
            out = ops.mlp_forward_rays_lp(pk, mlp.sem_mode, precision, o, d, v, z)
            again = ops.mlp_forward_rays_lp(pk, mlp.sem_mode, precision, o, d, v, z)
            assert torch.equal(out, again), f"not deterministic at R={R}, S={S}"
            assert torch.isfinite(out).all()
            if name != "nosem":
                raw, sem_in, sem_hid = ops.mlp_forward_rays_save(pk, mlp.sem_mode, o, d, v, z, precision, compact=False)
                raw_c, sem_in_c, sem_hid_c = ops.mlp_forward_rays_save(pk, mlp.sem_mode, o, d, v, z, precision, compact=True)
                assert torch.equal(raw, out) and torch.equal(raw_c, out), "the training variants render bit-identically to inference"
                assert sem_in.dtype == torch.float32 and sem_hid.dtype == torch.float32
                assert sem_in_c.dtype == dt and sem_hid_c.dtype == dt and sem_in_c.dim() == 2 and sem_hid_c.dim() == 2      # row-major
                assert torch.equal(sem_in_c.float(), sem_in), f"SAVE R={R} S={S}: compact sem_in differs from the fp32 one"
                assert torch.equal(sem_hid_c, sem_hid.to(dt)), f"SAVE R={R} S={S}: compact sem_hid is not the fp32 one rounded to nearest even"
    finally:
        _lib.check(lib.nsos_mlp_lp_select_kernel(3), "select")     # the default: mlp_lp16_kernel
    for refused in (0, 2, 4):
        assert lib.nsos_mlp_lp_select_kernel(refused) == -3
    assert lib.nsos_mlp_lp_selected_kernel() == 3


# ------------------------------------------------------------------------------------------ train-mode draws in one launch
def test_philox_render_draws():
    """nsos_render_draws: the four train-mode random tensors of a ray chunk from one counter-based launch.  Checked:
    ranges, moments (23-bit uniforms in (0,1); Box-Muller normals), independence of the four tensors and of consecutive
    calls, reproducibility by (seed, call), odd sizes (tail blocks of 4), and the module option NeRFNet.rng = 'philox'."""
    R, S, N = 4099, 64, 128
    t, n0, u, n1 = ops.render_draws(1234, 1, R, S, N, DEV)
    assert t.shape == (R, S) and n0.shape == (R, S) and u.shape == (R, N) and n1.shape == (R, S + N)
    for x in (t, u):
        assert float(x.min()) > 0.0 and float(x.max()) < 1.0
        assert abs(float(x.mean()) - 0.5) < 2e-3 and abs(float(x.var()) - 1 / 12) < 1e-3
    for x in (n0, n1):
        assert torch.isfinite(x).all()
        assert abs(float(x.mean())) < 5e-3 and abs(float(x.var()) - 1.0) < 1e-2
        assert abs(float((x ** 4).mean()) - 3.0) < 0.1                       # kurtosis of a normal
    assert abs(float(torch.corrcoef(torch.stack([t.flatten(), n0.flatten()]))[0, 1])) < 5e-3
    assert abs(float(torch.corrcoef(torch.stack([n0.flatten()[:-1], n0.flatten()[1:]]))[0, 1])) < 5e-3   # Box-Muller pair halves
    again = ops.render_draws(1234, 1, R, S, N, DEV)
    assert all(torch.equal(a, b) for a, b in zip((t, n0, u, n1), again))
    other = ops.render_draws(1234, 2, R, S, N, DEV)
    assert not torch.equal(other[0], t) and abs(float(torch.corrcoef(torch.stack([other[0].flatten(), t.flatten()]))[0, 1])) < 5e-3
    assert not torch.equal(ops.render_draws(1235, 1, R, S, N, DEV)[0], t)
    only = ops.render_draws(7, 3, 5, 64, 0, DEV, jitter=True, noise=False)
    assert only[1] is None and only[2] is None and only[3] is None and only[0].shape == (5, 64)
    # module option: train-mode renders draw from the package's stream; reproducible by (seed, call counter)
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, perturb=1.0, raw_noise_std=1.0).to(DEV).train()
    rays = tp.synthetic_rays(300, seed=2).to(DEV)
    net.rng, net.rng_seed = "philox", 99
    with torch.no_grad():
        a = net(rays, (tp.NEAR, tp.FAR))
        b = net(rays, (tp.NEAR, tp.FAR))
        net._rng_calls = 0
        c = net(rays, (tp.NEAR, tp.FAR))
    assert torch.isfinite(a["rgb"]).all() and not torch.equal(a["rgb"], b["rgb"]) and torch.equal(a["rgb"], c["rgb"])
    state = torch.cuda.get_rng_state()
    with torch.no_grad():
        net(rays, (tp.NEAR, tp.FAR))
    assert torch.equal(state, torch.cuda.get_rng_state()), "philox mode must not touch torch's generator"


def test_fused_composite_importance_equals_the_two_kernels(golden):
    """nsos_composite_importance (coarse compositing + hierarchical resampling in one launch) is the same device code as
    nsos_composite followed by nsos_importance_sample: every output bit-identical, deterministic and random u, noise,
    semantics channels, white background, ragged coarse sample counts."""
    g = torch.Generator().manual_seed(3)
    for R, S, N, C, white, noisy, rand_u in ((257, 64, 128, 6, False, True, True), (5, 64, 128, 4, True, False, False),
                                             (33, 17, 40, 6, False, False, True), (1, 2, 448, 4, False, True, False)):
        raw = (torch.randn(R, S, C, generator=g) * 2).to(DEV)
        z = (tp.NEAR + (tp.FAR - tp.NEAR) * torch.rand(R, S, generator=g)).sort(-1).values.to(DEV)
        d = torch.randn(R, 3, generator=g).to(DEV)
        noise = torch.randn(R, S, generator=g).to(DEV) if noisy else None
        u = torch.rand(R, N, generator=g).to(DEV) if rand_u else None
        a = ops.composite(raw, z, d, noise, 0.7 if noisy else 0.0, white)
        zf, zs, zstd = ops.importance_sample(z, a["weights"], N, u)
        b, zf2, zs2, zstd2 = ops.composite_importance(raw, z, d, N, noise, 0.7 if noisy else 0.0, white, u)
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (k, R, S)
        assert torch.equal(zf, zf2) and torch.equal(zs, zs2) and torch.equal(zstd, zstd2)


@pytest.mark.parametrize("case", range(16))
def test_fuzz_shapes_module_vs_port(case):
    """Seeded random shapes through the whole module against the torch port of the reference (eval mode): ray counts that
    are not multiples of anything, coarse sample counts on both sides of 64 (tuned / general importance kernel, fused /
    unfused compositing), importance counts from 0 up, every head configuration, white background, tensor bounds, an image-
    shaped ray batch.  Coarse outputs within 1e-4; the fine pass in bulk (index flips of the sampler); shapes and
    keys exactly."""
    rng = np.random.default_rng(1000 + case)
    R = int(rng.choice([1, 2, 3, 31, 33, 64, 65, 127, 200, 257]))
    S = int(rng.choice([2, 3, 8, 17, 40, 63, 64, 65, 70, 100, 129]))
    N_ = int(rng.choice([0, 1, 5, 64, 128, 200]))
    if S == 2 and N_ > 0:
        S = 3          # the reference itself cannot importance-sample 2 coarse samples (empty inner-weight cdf, models/sampler.py:93-97)
    name = str(rng.choice(["nosem", "sem", "semcoord"]))
    white = bool(rng.integers(0, 2))
    peaky = bool(rng.integers(0, 2))
    torch.manual_seed(2000 + case)
    kw = dict(CFGS[name])
    net = nerf_sos_amd.NeRFNet(N_samples=S, N_importance=N_, white_bkgd=white, **kw).to(DEV).eval()
    if peaky:
        nerf_sos_amd.synthetic.spiky_density_(net, 6.0, 0.3)
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    rays = tp.synthetic_rays(R, seed=3000 + case)
    if case % 4 == 3 and R % 2 == 0:                       # image-shaped batch [2, R/2, 2, 3]
        rays = rays.reshape(2, R // 2, 2, 3)
    bounds = (tp.NEAR, tp.FAR)
    if case % 3 == 2:                                       # tensor bounds: [R,1] whatever the ray batch's shape (models/nerf_net.py:161-165)
        bounds = (torch.full((R, 1), tp.NEAR), torch.full((R, 1), tp.FAR))
    with torch.no_grad():
        out = net(rays.to(DEV), tuple(b.to(DEV) if torch.is_tensor(b) else b for b in bounds))
    cfg = tp.PortConfig(n_samples=S, n_importance=N_, white_bkgd=white, **kw)
    ref = tp.render(sd, cfg, rays, bounds)
    assert set(out) == set(ref), (sorted(out), sorted(ref))
    for k in ref:
        assert tuple(out[k].shape) == tuple(ref[k].shape), (k, out[k].shape, ref[k].shape)
    coarse = [k for k in ref if k.endswith("0")] if N_ > 0 else [k for k in ref if k != "raw"]
    for k in coarse:
        close(N(out[k]), ref[k].numpy(), atol=1e-4, rtol=1e-4, what=f"case {case}: {k}")
    if N_ > 0:
        for k in ("rgb", "acc"):
            a, b = N(out[k]).reshape(R, -1), ref[k].numpy().reshape(R, -1)
            n_bad = int((np.abs(a - b) > 1e-4 * (1 + np.abs(b))).any(-1).sum())
            # measured (round 4): no ray of any of the 16 cases outside 1e-4; one index flip may move one ray
            assert n_bad <= 1, (case, k, n_bad, dict(R=R, S=S, N=N_, name=name, white=white, peaky=peaky))


@pytest.mark.parametrize("case", range(12))
def test_fuzz_frozen_backbone_gradients_vs_port_autograd(case):
    """Seeded random shapes through the frozen-backbone training path (the shipped recipe): gradients of the semantic heads
    from the one-pass HIP backward against torch autograd through the port of the reference, at ray / sample counts that hit
    the weight-gradient kernels' ragged steps, ray crossings inside a lane's 8 points, the < 8-samples fallback and the
    general importance kernel; then the same step at bf16 (the C3 / C4 kernels, 16-bit sem_in) against the fp32 gradients."""
    rng = np.random.default_rng(7000 + case)
    R = int(rng.choice([1, 3, 17, 33, 100, 130]))
    S = int(rng.choice([4, 8, 9, 24, 64, 65, 96]))
    N_ = int(rng.choice([0, 7, 64, 128]))
    name = str(rng.choice(["sem", "semcoord"]))
    torch.manual_seed(8000 + case)
    net = nerf_sos_amd.NeRFNet(N_samples=S, N_importance=N_, **CFGS[name]).to(DEV).eval()
    nerf_sos_amd.synthetic.spiky_density_(net, 2.0, 0.5)
    for n, p in net.named_parameters():
        p.requires_grad_("semantic_linear" in n)
    sd = {k: v.detach().cpu().clone().requires_grad_("semantic_linear" in k) for k, v in net.state_dict().items()}
    rays = tp.synthetic_rays(R, seed=9000 + case)
    tgt = torch.randn(R, 2, generator=torch.Generator().manual_seed(case))

    def loss_of(out, t):
        l = ((out["semantics"] - t) ** 2).mean()
        return l + ((out["semantics0"] - t) ** 2).mean() if "semantics0" in out else l

    ref = tp.render(sd, tp.PortConfig(n_samples=S, n_importance=N_, **CFGS[name]), rays, (tp.NEAR, tp.FAR))
    loss_of(ref, tgt).backward()
    grads = {}
    for prec in ("fp32", "bf16"):
        net.mlp_precision = prec
        net.zero_grad(set_to_none=True)
        out = net(rays.to(DEV), (tp.NEAR, tp.FAR))
        loss_of(out, tgt.to(DEV)).backward()
        grads[prec] = {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters() if p.requires_grad}
    # The coarse net's gradient does not depend on the sampler; the fine net's does (index flips move a few samples): bulk bar.
    for n, g in grads["fp32"].items():
        want = sd[n].grad
        if want is None:
            assert float(g.abs().max()) == 0.0, n
            continue
        scale = float(want.abs().max()) + 1e-30
        err = float((g - want).abs().max()) / scale
        assert err < (1e-4 if n.startswith("nerf.") or N_ == 0 else 2e-2), (case, n, err, dict(R=R, S=S, N=N_, name=name))
        # 16 bit: 8-bit mantissas through 9 layers and a handful of rays (ReLU masks of near-zero units flip): a direction check,
        # test_lp_training_variant holds the format's error bar
        a, b = grads["bf16"][n].double().flatten(), g.double().flatten()
        cos = float((a @ b) / (a.norm() * b.norm() + 1e-300))
        assert cos > 0.97, (case, n, cos)

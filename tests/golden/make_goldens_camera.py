#!/usr/bin/env python3
"""Goldens of the camera layer (learnable poses: models/camera.py::CameraTransformer, corrupt_cameras) from the REAL reference
(build container only; /root/reference mounted read-only):

    python tests/golden/make_goldens_camera.py

Layer cases: the real module (fp32, CPU) transforms the first N rays of one shared pool, a linear functional sum(o' G_o) +
sum(d' G_d) is back-propagated, and per case go to tests/golden/camera.npz: ids, rvec, tvec, the module's outputs and autograd
gradients, the same from tests/camera_port.py in fp64, and e32 = max |fp32 reference - fp64| per output.  The port's fp32 run must
equal the real module bit for bit, else nothing is written.  To keep the file small the per-ray fp64 arrays are stored as the fp32
residual X64 - X32 (X64 = X32 + residual to 1e-13 of scale, asserted), and g_rays_o is not stored at all: it IS the upstream G_o
(asserted, both precisions).
Render cases: the real CameraTransformer feeds the real NeRFNet (eval mode; one generic architecture and the shipped one), a random
linear functional of the rendered maps is back-propagated; rays, ids, upstream gradients, the coarse weights (from which the tests
rebuild the reference's fine sample positions) and rvec.grad / tvec.grad are recorded.
Also: a real module's state dict, and corrupt_cameras after np.random.seed(0).
Single-threaded and with deterministic algorithms, and written with fixed zip timestamps: a second run gives the same bytes.
Only data is written.
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_goldens as mg  # noqa: E402  (puts the reference and the repository on sys.path, stubs its optional imports)
import make_goldens_generic as mgg  # noqa: E402
from models import camera as ref_camera  # noqa: E402  (reference)
from oracle import torch_port as tp  # noqa: E402
import camera_port as cp  # noqa: E402

torch.autograd.set_detect_anomaly(False)      # models/camera.py:2 turns it on at import
torch.set_num_threads(1)
torch.use_deterministic_algorithms(True)

POOL = 4099
# name -> (N, C, id pattern, quaternions)
LAYER_CASES = {
    "n1_c1": (1, 1, "random", "near"),
    "n63_c3_runs": (63, 3, "runs", "near"),
    "n64_c3_empty": (64, 3, "empty1", "near"),
    "n64_c70_random": (64, 70, "random", "near"),
    "n257_c3_one": (257, 3, "one", "near"),
    "n257_c70_random": (257, 70, "random", "near"),
    "n257_c3_farnorm": (257, 3, "random", "far"),
    "n4099_c3_runs": (4099, 3, "runs", "near"),
    "n4099_c70_random": (4099, 70, "random", "near"),
}
RENDER_KEYS = ("rgb", "semantics", "depth", "acc")
OUTS = ("out_o", "out_d", "g_rays_o", "g_rays_d", "g_rvec", "g_tvec")


def make_ids(n, c, pattern, g):
    if pattern == "random":
        return torch.randint(0, c, (n,), generator=g)
    if pattern == "runs":                        # contiguous runs of unequal length, cameras in a shuffled order (a patch batch)
        cuts = torch.sort(torch.randperm(n - 1, generator=g)[:c - 1] + 1).values.tolist() if c > 1 else []
        order = torch.randperm(c, generator=g)
        ids = torch.empty(n, dtype=torch.int64)
        for k, (b, e) in enumerate(zip([0] + cuts, cuts + [n])):
            ids[b:e] = order[k]
        return ids
    if pattern == "empty1":                      # camera 1 of the three has no ray
        return torch.randint(0, 2, (n,), generator=g) * 2
    if pattern == "one":                         # every ray on camera 1
        return torch.ones(n, dtype=torch.int64)
    raise ValueError(pattern)


def make_params(c, kind, g):
    rvec = torch.tensor([0., 0., 0., 1.]).repeat(c, 1) + 0.05 * torch.randn(c, 4, generator=g)
    tvec = 0.1 * torch.randn(c, 3, generator=g)
    if kind == "far":                            # far from unit norm: the theta terms of the backward matter
        norm = rvec.norm(dim=1, keepdim=True)
        rvec = rvec / norm * torch.tensor([[0.3], [4.0], [1.0]])[:c]
    return rvec, tvec


def run_real(rays_o, rays_d, ids, rvec, tvec, G_o, G_d):
    cam = ref_camera.CameraTransformer(rvec.shape[0], trainable=True)
    cam.load_state_dict({"rvec": rvec, "tvec": tvec})
    col = ids.float()[:, None]
    o4 = torch.cat([rays_o, col], -1).requires_grad_(True)
    d4 = torch.cat([rays_d, col], -1).requires_grad_(True)
    with torch.enable_grad():
        o, d = cam(o4, d4)
        ((o * G_o).sum() + (d * G_d).sum()).backward()
    return {"out_o": o.detach(), "out_d": d.detach(), "g_rays_o": o4.grad[:, :3], "g_rays_d": d4.grad[:, :3],
            "g_rvec": cam.rvec.grad, "g_tvec": cam.tvec.grad}


def layer_cases(out):
    g = torch.Generator().manual_seed(4242)
    pool = {"rays_o": 2.0 * torch.randn(POOL, 3, generator=g),
            "rays_d": torch.cat([1.2 * torch.rand(POOL, 2, generator=g) - 0.6, -torch.ones(POOL, 1)], -1),
            "G_o": torch.randn(POOL, 3, generator=g), "G_d": torch.randn(POOL, 3, generator=g)}
    for k, v in pool.items():
        out[f"pool__{k}"] = v.numpy()
    for name, (n, c, pattern, kind) in LAYER_CASES.items():
        ids = make_ids(n, c, pattern, g)
        rvec, tvec = make_params(c, kind, g)
        args = [pool[k][:n] for k in ("rays_o", "rays_d")] + [ids, rvec, tvec] + [pool[k][:n] for k in ("G_o", "G_d")]
        real = run_real(*args)
        p32 = cp.grads(*args)
        p64 = cp.grads(*[a.double() if a.is_floating_point() else a for a in args])
        for k in OUTS:
            assert real[k].dtype == torch.float32 and torch.equal(real[k], p32[k]), f"{name}: the port's fp32 {k} != the real module's"
        assert torch.equal(real["g_rays_o"], args[5]) and torch.equal(p64["g_rays_o"], args[5].double())
        out[f"{name}__ids"] = ids.numpy().astype(np.int32)
        out[f"{name}__rvec"], out[f"{name}__tvec"] = rvec.numpy(), tvec.numpy()
        e32 = []
        for k in OUTS:
            e32.append(float((real[k].double() - p64[k]).abs().max()))
            if k == "g_rays_o":
                continue
            out[f"{name}__ref32__{k}"] = real[k].numpy()
            if k in ("g_rvec", "g_tvec"):
                out[f"{name}__ref64__{k}"] = p64[k].numpy()
            elif k != "out_o":                   # out_o is held to bit-equality with the fp32 reference: no fp64 needed
                res = (p64[k] - real[k].double()).float()
                assert float((real[k].double() + res.double() - p64[k]).abs().max()) <= 1e-13 * float(p64[k].abs().max())
                out[f"{name}__res64__{k}"] = res.numpy()
        out[f"{name}__e32"] = np.array(e32, np.float64)
        rel = [e / max(float(p64[k].abs().max()), 1e-30) for e, k in zip(e32, OUTS)]
        print(f"{name}: e32 / scale  " + "  ".join(f"{k} {r:.1e}" for k, r in zip(OUTS, rel)))


def render_case(out, tag, model, rays, n_cams, g):
    R = rays.shape[1]
    ids = torch.randint(0, n_cams, (R,), generator=g)
    rvec, tvec = make_params(n_cams, "near", g)
    cam = ref_camera.CameraTransformer(n_cams, trainable=True)
    cam.load_state_dict({"rvec": rvec, "tvec": tvec})
    col = ids.float()[:, None]
    torch.set_grad_enabled(True)
    o, d = cam(torch.cat([rays[0], col], -1), torch.cat([rays[1], col], -1))
    ret = model(torch.stack([o, d], 0), (tp.NEAR, tp.FAR))
    loss = 0.0
    for k in list(ret.keys()):
        if k.rstrip("0") not in RENDER_KEYS or ret[k].numel() == 0:
            continue
        G = torch.randn(ret[k].shape, generator=g)
        if k.rstrip("0") == "depth":
            G = G * (ret[k].detach().abs() < 1e9)       # empty rays carry depth 1e10 (no gradient): keep the loss finite-sized
        out[f"{tag}__G__{k}"] = G.numpy()
        loss = loss + (ret[k] * G).sum()
    loss.backward()
    torch.set_grad_enabled(False)
    assert all(p.grad is not None for p in model.parameters() if p.requires_grad)
    out[f"{tag}__rays"], out[f"{tag}__ids"] = rays.numpy().copy(), ids.numpy().astype(np.int32)
    out[f"{tag}__rvec"], out[f"{tag}__tvec"] = rvec.numpy(), tvec.numpy()
    out[f"{tag}__g_rvec"], out[f"{tag}__g_tvec"] = cam.rvec.grad.numpy().copy(), cam.tvec.grad.numpy().copy()
    out[f"{tag}__weights0"] = ret["weights0"].detach().numpy().copy()
    out[f"{tag}__rgb"] = ret["rgb"].detach().numpy().copy()
    print(f"{tag}: loss {float(loss):.6f}, |g_rvec| max {float(cam.rvec.grad.abs().max()):.4g}, |g_tvec| max {float(cam.tvec.grad.abs().max()):.4g}")


def render_cases(out):
    g = torch.Generator().manual_seed(515)
    torch.set_grad_enabled(False)
    net, pc, sd = mg.build_ref("semcoord", n_importance=128, peaky=True)
    render_case(out, "render_semcoord", net.eval(), tp.synthetic_rays(64, seed=41), 3, g)
    fwd = dict(np.load(os.path.join(HERE, "generic.npz")))
    name = "d6w96_m6"
    ref_kw, port_kw = mgg.CASES[name]
    seed = int(fwd[f"{name}__seed"][0])
    torch.manual_seed(seed)
    model = mgg.NeRFNet(**ref_kw).eval()
    model.load_state_dict(mgg.generic_state(tp.PortConfig(**port_kw), seed))
    render_case(out, f"render_{name}", model, tp.synthetic_rays(96, seed=seed + 2), 3, g)


def extras(out):
    cam = ref_camera.CameraTransformer(5, trainable=True)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        cam.rvec.add_(0.05 * torch.randn(5, 4, generator=g))
        cam.tvec.add_(0.1 * torch.randn(5, 3, generator=g))
    for k, v in cam.state_dict().items():
        out[f"state__{k}"] = v.numpy().copy()
    out["state__keys"] = np.array(list(cam.state_dict().keys()))
    frozen = ref_camera.CameraTransformer(2, trainable=False)
    assert list(frozen.state_dict().keys()) == ["rvec", "tvec"] and not list(frozen.parameters())
    rng = np.random.default_rng(3)
    poses = np.zeros((6, 3, 5))
    for i in range(6):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        poses[i, :, :3], poses[i, :, 3], poses[i, :, 4] = q, rng.normal(size=3), (120, 160, 150)
    out["corrupt__poses"] = poses
    np.random.seed(0)
    out["corrupt__default"] = ref_camera.corrupt_cameras(poses)
    out["corrupt__wide"] = ref_camera.corrupt_cameras(poses, offset=(-0.3, 0.2), rotation=(-10, 20))


def save(path, arrays):
    """np.savez_compressed with fixed member timestamps and sorted names: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    out = {}
    layer_cases(out)
    render_cases(out)
    extras(out)
    path = os.path.join(HERE, "camera.npz")
    save(path, out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()

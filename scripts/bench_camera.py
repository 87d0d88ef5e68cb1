"""The camera layer (nerf_sos_amd.CameraTransformer, csrc/camera.hip) against the reference module's own torch ops on the same GPU.

Two shapes of forward + backward to rvec.grad / tvec.grad: 4096 rays over 8 cameras in contiguous runs (a patch batch) and 65 536 rays
over 200 cameras with random ids (a ray batch), each eager and captured in a graph.  The torch side is tests/camera_port.py, the
restatement that is bit-identical to models/camera.py on the CPU.  Then one whole pose step on the shipped architecture (4096 rays,
frozen net, loss on the fine map: the shape of bench.py's pose_step), once with the rays as the leaf and once with the camera
parameters as the leaf.  Device events around `--iters` calls; the two sides of every comparison take turns window by window
(`--repeats` windows each), the median and the spread are reported.  Prints one JSON line.  No time here is a pass / fail gate.
Every timed function returns detached tensors, and nothing of an eager call's autograd graph is kept while a graph is captured: a
leaf's gradient-accumulator node remembers the stream it was made on, and one made on the default stream and still alive makes
autograd wait on the default stream in the middle of the capture.  The result file is rewritten after every phase; progress goes to
stderr.

    python scripts/bench_camera.py [--iters 50] [--warmup 10] [--repeats 5] [--out profiles/camera/bench_camera.json]
"""
import argparse
import functools
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nerf_sos_amd  # noqa: E402
from nerf_sos_amd import synthetic as syn  # noqa: E402
import camera_port as cp  # noqa: E402


def note(msg):
    print(f"[bench_camera] {msg}", file=sys.stderr, flush=True)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(fns, iters, warmup, repeats):
    """{name: {ms, min, max}}: the functions take turns, one window each per round."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    w = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            w[k].append(window(fn, iters))
    return {k: {"ms": statistics.median(v), "min": min(v), "max": max(v)} for k, v in w.items()}


def captured(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    return g.replay, out


def make_step(rays, ids, G):
    def step(cam):   # forward + backward to the parameters; detached: no autograd graph outlives the call
        out = cam.transform(rays, ids)
        return tuple(x.detach() for x in (out,) + torch.autograd.grad(out, [cam.rvec, cam.tvec], grad_outputs=G))
    return step


def perturbed(cam, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        cam.rvec.add_((0.05 * torch.randn(cam.rvec.shape, generator=gen)).to(cam.rvec.device))
        cam.tvec.add_((0.1 * torch.randn(cam.tvec.shape, generator=gen)).to(cam.tvec.device))
    return cam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_camera: needs a GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "iters": args.iters, "repeats": args.repeats, "layer": {}}
    torch_steps = {}

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(result) + "\n")
    gen = torch.Generator().manual_seed(0)
    for name, n, c, ids in (("4096_rays_8_cams_runs", 4096, 8, torch.arange(4096) // 512),
                            ("65536_rays_200_cams_random", 65536, 200, torch.randint(0, 200, (65536,), generator=gen))):
        rays = syn.synthetic_rays(n, seed=1, device=dev)
        G = torch.randn(2, n, 3, generator=gen).to(dev)
        ids = ids.to(dev, torch.int32)
        ours = perturbed(nerf_sos_amd.CameraTransformer(c, trainable=True).to(dev), 3)
        theirs = perturbed(cp.Layer(c).to(dev), 3)

        step = make_step(rays, ids, G)

        note(f"{name}: first calls")
        a, b = step(ours), step(theirs)
        case = {"rel_diff_vs_torch": {k: float((x - y).abs().max() / y.abs().max()) for k, x, y in zip(("out", "g_rvec", "g_tvec"), a, b)}}
        del a, b
        case.update(alternate({"hip_eager": functools.partial(step, ours), "torch_eager": functools.partial(step, theirs)},
                              args.iters, args.warmup, args.repeats))
        note(f"{name}: eager done, capturing the HIP layer")
        replay, keep = captured(functools.partial(step, ours))
        case.update(alternate({"hip_graph": replay}, args.iters, args.warmup, args.repeats))
        case["speedup_eager"] = case["torch_eager"]["ms"] / case["hip_eager"]["ms"]
        case["torch_eager_over_hip_graph"] = case["torch_eager"]["ms"] / case["hip_graph"]["ms"]
        torch_steps[name] = (functools.partial(step, theirs), replay)
        note(f"{name}: done")
        result["layer"][name] = case
        write()

    # one whole pose step (bench.py's pose_step_shipped_architecture: 4096 rays, frozen shipped net, MSE on the fine map)
    n, c = 4096, 8
    rays = syn.synthetic_rays(n, seed=0, device=dev)
    ids = (torch.arange(n) // (n // c)).to(dev, torch.int32)
    gt = torch.rand(n, 3, device=dev)
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, use_semantics=True, sem_with_coord=True).to(dev).eval()
    for p_ in net.parameters():
        p_.requires_grad_(False)
    cam = perturbed(nerf_sos_amd.CameraTransformer(c, trainable=True).to(dev), 5)
    cam_t = perturbed(cp.Layer(c).to(dev), 5)

    def rays_leaf():
        r = rays.clone().requires_grad_(True)
        ret = net(r, (syn.NEAR, syn.FAR), retraw=False)
        ((ret["rgb"] - gt) ** 2).mean().backward()
        return r.grad

    def camera_leaf(layer):
        for p_ in layer.parameters():
            p_.grad = None
        ret = net(layer.transform(rays, ids), (syn.NEAR, syn.FAR), retraw=False)
        ((ret["rgb"] - gt) ** 2).mean().backward()
        return layer.rvec.grad

    note("pose step")
    it = max(3, args.iters // 5)
    pose = alternate({"rays_leaf": rays_leaf, "camera_leaf_hip": lambda: camera_leaf(cam), "camera_leaf_torch": lambda: camera_leaf(cam_t)},
                     it, 2, args.repeats)
    layer_ms = result["layer"]["4096_rays_8_cams_runs"]
    pose["layer_share_of_camera_leaf_step"] = {"graph": layer_ms["hip_graph"]["ms"] / pose["camera_leaf_hip"]["ms"],
                                               "eager": layer_ms["hip_eager"]["ms"] / pose["camera_leaf_hip"]["ms"]}
    pose["g_rvec_finite"] = bool(torch.isfinite(camera_leaf(cam)).all())
    result["pose_step_4096_rays"] = pose
    write()
    # last, so that everything above is on disk first: the torch module captured (its backward is ATen's sort-based index_put)
    for name, (torch_step, replay) in torch_steps.items():
        note(f"{name}: capturing the torch module")
        case = result["layer"][name]
        try:
            replay_t, keep_t = captured(torch_step)
        except RuntimeError as e:
            case["torch_graph"] = {"ms": None, "not_captured": str(e).splitlines()[0][:200]}
            write()
            break                                  # a failed capture leaves the stream state in doubt: stop here
        case.update(alternate({"hip_graph_again": replay, "torch_graph": replay_t}, args.iters, args.warmup, args.repeats))
        case["speedup_graph"] = case["torch_graph"]["ms"] / case["hip_graph_again"]["ms"]
        write()
    print(json.dumps(result))


if __name__ == "__main__":
    main()

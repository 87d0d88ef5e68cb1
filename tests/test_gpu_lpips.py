"""GPU: LPIPS (AlexNet) on the HIP kernels against the fp64 port (tests/lpips_port.py) on the cases of tests/lpips_weights.CASES.

The bar is the project's (tests/test_gpu_dino.py, tests/test_gpu_losses_edges.py): max|gpu - fp64| <= max(4 * e32, 1e-6 * scale),
capped at 1e-4 * scale, with e32 the port's own fp32 distance from fp64 on that output and scale = max|fp64|; every case, the value,
the per-layer values and all ten feature maps, every element.  The port runs on the CPU at test time, once per case, shared."""
import functools

import numpy as np
import pytest
import torch

import nerf_sos_amd
from nerf_sos_amd import metrics, ops

import lpips_port as port
import lpips_weights as lw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_IDS = [(ci, kind) for ci, c in enumerate(lw.CASES) for kind in c[5]]


@functools.lru_cache(maxsize=None)
def _state(kind):
    return lw.make_state(kind, lw.STATE_SEEDS[kind])


@functools.lru_cache(maxsize=None)
def _model(kind):
    m = nerf_sos_amd.LPIPS()
    m.load_state_dict(_state(kind))
    return m.to(DEV)


@functools.lru_cache(maxsize=None)
def _reference(ci, kind):
    """The port in fp64 and fp32 on the CPU: computed once, shared, never modified."""
    a, b = (torch.from_numpy(x) for x in lw.make_images(ci))
    r64 = port.lpips(_state(kind), a, b, torch.float64)
    r32 = port.lpips(_state(kind), a, b, torch.float32)
    return a, b, r64, r32


def _bar(e32, scale):
    return min(max(4 * e32, 1e-6 * scale), 1e-4 * scale)


@pytest.mark.parametrize("ci,kind", CASE_IDS, ids=[f"{lw.CASES[ci][0]}-{k}" for ci, k in CASE_IDS])
def test_value_layers_and_features_against_fp64(ci, kind, golden):
    name, n = lw.CASES[ci][0], lw.CASES[ci][1]
    a, b, (v64, l64, f0_64, f1_64), (v32, l32, f0_32, f1_32) = _reference(ci, kind)
    g = golden("lpips")
    np.testing.assert_allclose(v64.numpy(), g[f"{name}_{kind}_value"], rtol=1e-11, atol=0)       # the fixture pins the port
    m = _model(kind)
    out = ops.lpips_forward(a.to(DEV), b.to(DEV), m.packed_weights(), 0, None, want_layers=True, want_feats=True)
    torch.cuda.synchronize()
    fails = []

    def check(what, got, ref64, ref32):
        got, ref64 = got.double().cpu(), ref64.double()
        assert tuple(got.shape) == tuple(ref64.shape), (what, tuple(got.shape), tuple(ref64.shape))
        err = float((got - ref64).abs().max())
        e32 = float((ref32.double() - ref64).abs().max())
        scale = float(ref64.abs().max())
        bar = _bar(e32, scale)
        print(f"{name} {kind} {what}: |gpu-fp64| {err:.3e}, e32 {e32:.3e}, scale {scale:.3e}, bar {bar:.3e}, "
              f"ratio to e32 {err / max(e32, 1e-300):.2f}")
        if not err <= bar:
            fails.append((what, err, bar))

    check("value", out["lpips"], v64, v32)
    check("layers", out["layers"], l64, l32)
    for l in range(5):
        f = out["feats"][l]                                  # [2N,H,W,C], image 2b = img0[b], 2b+1 = img1[b]
        f = f.reshape(n, 2, *f.shape[1:]).permute(1, 0, 4, 2, 3)
        check(f"feat{l}/img0", f[0], f0_64[l], f0_32[l])
        check(f"feat{l}/img1", f[1], f1_64[l], f1_32[l])
    assert not fails, fails
    assert tuple(m(a.to(DEV), b.to(DEV)).shape) == (n, 1, 1, 1)
    assert torch.equal(m(a.to(DEV), b.to(DEV)), out["lpips"]) and torch.equal(m.layers(a.to(DEV), b.to(DEV)), out["layers"])


def test_identical_images_give_exactly_zero():
    for ci, kind in ((0, "he"), (1, "wide"), (3, "sparse")):
        a = _reference(ci, kind)[0].to(DEV)
        v = _model(kind)(a, a.clone())
        assert torch.equal(v, torch.zeros_like(v)), (ci, kind, v.flatten().tolist())


def test_symmetric_bit_for_bit():
    for ci, kind in ((1, "wide"), (2, "sparse"), (3, "he")):
        a, b = (x.to(DEV) for x in _reference(ci, kind)[:2])
        m = _model(kind)
        assert torch.equal(m(a, b), m(b, a)) and torch.equal(m.layers(a, b), m.layers(b, a)), (ci, kind)


def test_a_pair_alone_and_inside_a_batch_of_three():
    m = _model("wide")
    a, b = (x.to(DEV) for x in _reference(1, "wide")[:2])                     # N = 2 at 33x47
    rng = np.random.default_rng(5)
    xa = torch.from_numpy(rng.uniform(0, 1, (1, 3, 33, 47)).astype(np.float32)).to(DEV)
    xb = torch.from_numpy(rng.uniform(0, 1, (1, 3, 33, 47)).astype(np.float32)).to(DEV)
    a3, b3 = torch.cat([a[:1], xa, a[1:]]), torch.cat([b[:1], xb, b[1:]])
    v3, l3 = m(a3, b3), m.layers(a3, b3)
    for pos, (pa, pb) in enumerate(((a[:1], b[:1]), (xa, xb), (a[1:], b[1:]))):
        assert torch.equal(m(pa, pb), v3[pos:pos + 1]) and torch.equal(m.layers(pa, pb), l3[pos:pos + 1]), pos


def test_layouts_give_identical_bits():
    m = _model("he")
    a, b = (x.to(DEV) for x in _reference(3, "he")[:2])                       # [1,3,97,130]
    v = metrics.lpips(a, b, format="NCHW", model=m)
    an, bn = a.permute(0, 2, 3, 1).contiguous(), b.permute(0, 2, 3, 1).contiguous()
    assert torch.equal(metrics.lpips(an, bn, format="NHWC", model=m), v)
    assert torch.equal(metrics.lpips(an[0], bn[0], format="HWC", model=m), v)
    assert torch.equal(metrics.lpips(a.permute(0, 2, 3, 1), b.permute(0, 2, 3, 1), format="NHWC", model=m), v)   # a strided view
    assert tuple(v.shape) == (1, 1, 1, 1)


def test_normalize_equals_feeding_2x_minus_1():
    m = _model("wide")
    a, b = (x.to(DEV) for x in _reference(2, "wide")[:2])
    assert torch.equal(m(a, b, normalize=True), m(2 * a - 1, 2 * b - 1))
    assert not torch.equal(m(a, b, normalize=True), m(a, b))


def test_captured_in_a_graph_and_replayed():
    m = _model("wide")
    a, b = (x.to(DEV) for x in _reference(1, "wide")[:2])
    eager = m(a, b).clone()
    sa, sb = a.clone(), b.clone()
    m.prepare(2, 33, 47)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        m(sa, sb)                                            # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = m(sa, sb)
    for _ in range(3):
        got.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got, eager)
    sa.copy_(b), sb.copy_(b)                                 # the graph reads the static inputs: identical images now
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, torch.zeros_like(got))


def test_view_metrics_adds_lpips_only_on_request():
    m = _model("he")
    a, b = (x.to(DEV) for x in _reference(2, "he")[:2])                       # 64x64
    rgb, target = a[0].permute(1, 2, 0).contiguous(), b[0].permute(1, 2, 0).contiguous()
    with_model = metrics.view_metrics({"rgb": rgb}, target, lpips=m)
    assert tuple(with_model["lpips"].shape) == (1, 1, 1, 1)
    assert torch.equal(with_model["lpips"], metrics.lpips(rgb, target, format="HWC", model=m))
    assert torch.equal(with_model["lpips"], m(a, b))
    without = metrics.view_metrics({"rgb": rgb}, target)
    assert "lpips" not in without and set(without) == set(with_model) - {"lpips"}
    for k in without:
        assert torch.equal(without[k], with_model[k]), k


def test_sizes_below_31_are_refused():
    m = _model("he")
    x = torch.rand(1, 3, 30, 64, device=DEV)
    with pytest.raises(ValueError):
        m(x, x)

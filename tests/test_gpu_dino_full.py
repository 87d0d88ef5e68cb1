"""GPU: DINO's full-image path (DinoViT.get_vit_attn_feat_noresize) and find_fg against the fixture written from the real
reference (tests/golden/make_goldens_dino_full.py).

The bar is tests/test_gpu_dino.py's: max|gpu - fp64| <= max(4 * e32, 1e-6 * scale), capped at 1e-4 * scale (e32 = the reference's
own fp32 distance from fp64 on that case, scale = max |fp64|); every case, every output, every stored element.  feat of images
other than image 0 (fp32 reference only) may be twice that from fp32.  Each comparison prints its figures before it asserts."""
import numpy as np
import pytest
import torch

import dino_full_fixture as fx
import dino_full_port as port
import dino_weights as dw
from helpers import state_sha

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_models = {}


def state(kind):
    sd = dw.make_state(kind, fx.meta()["seeds"][kind])
    assert state_sha(sd) == fx.meta()["state_sha256"][kind], f"make_state({kind!r}) differs from the generator's"
    return sd


def model(kind):
    import nerf_sos_amd
    if kind not in _models:
        m = nerf_sos_amd.DinoViT()
        m.load_state_dict(state(kind))
        _models[kind] = m.to(DEV)
    return _models[kind]


def dino_in(c):
    """engines/eval.py:134-136 on the GPU: normalize_batch of the channels-first rgb."""
    return port.eval_dino_in(torch.from_numpy(c["input"]).to(DEV)).contiguous()


def worst(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())


@pytest.mark.parametrize("ci", range(9))
def test_every_element_against_fp64(ci):
    c = fx.case(ci)
    out = model(c["kind"]).get_vit_attn_feat_noresize(dino_in(c))
    out = {k: out[k].cpu().numpy() for k in fx.OUTPUTS}
    n = c["rows"] * c["cols"]
    assert out["attn"].shape == (c["B"], 1, n) and out["feat"].shape == (c["B"], n, 384) and out["cls_"].shape == (c["B"], 384)
    out["feat"] = out["feat"][:, ::c["feat_stride"]]
    fails = []
    for k in fx.OUTPUTS:
        bar = fx.bar(c, k)
        assert np.isfinite(out[k]).all()
        if k == "feat":
            e64 = worst(out[k][0], c["ref64"]["feat0"])
            e32rest = worst(out[k][1:], c["ref32"][k][1:]) if c["B"] > 1 else 0.0
            print(f"case {ci} {c['h']}x{c['w']} {c['kind']} feat: |gpu-fp64| {e64:.3e} (image 0), |gpu-fp32| {e32rest:.3e} (others), "
                  f"e32 {c['e32'][k]:.3e}, scale {c['scale'][k]:.3e}, bar {bar:.3e}, ratio to e32 {e64 / max(c['e32'][k], 1e-30):.2f}")
            if not (e64 <= bar and e32rest <= 2 * bar):
                fails.append((k, e64, e32rest, bar))
        else:
            e64 = worst(out[k], c["ref64"][k])
            print(f"case {ci} {c['h']}x{c['w']} {c['kind']} {k}: |gpu-fp64| {e64:.3e}, e32 {c['e32'][k]:.3e}, scale {c['scale'][k]:.3e}, "
                  f"bar {bar:.3e}, ratio to e32 {e64 / max(c['e32'][k], 1e-30):.2f}")
            if not e64 <= bar:
                fails.append((k, e64, bar))
    assert not fails, fails
    for k in fx.OUTPUTS:
        assert fx.bar(c, k) <= 1e-4 * c["scale"][k]


@pytest.mark.parametrize("ci", range(9))
def test_position_table_against_fp64(ci):
    """The interpolated table the tokens get, against models/vision_transformer.py:174-194 run in fp64 on F.interpolate: within
    one fp32 rounding of the fp64 value (bar 2^-23 of the table's max |value|); the short cut exactly."""
    from nerf_sos_amd import ops
    c = fx.case(ci)
    m = model(c["kind"])
    pos = ops.dino_forward_full(dino_in(c), m.packed_weights(), want_pos=True)["pos"].cpu()
    pe = state(c["kind"])["pos_embed"]
    want = port.interpolate_pos(pe.double(), c["h"], c["w"])[0]
    want[0] = (state(c["kind"])["cls_token"][0, 0] + pe[0, 0]).double()      # row 0 carries cls_token + pos_embed[0]
    err = float((pos.double() - want).abs().max())
    print(f"case {ci} {c['h']}x{c['w']}: |table - fp64| {err:.3e}, scale {float(want.abs().max()):.3e}")
    assert pos.shape == want.shape and err <= 2.0 ** -23 * float(want.abs().max())
    if c["rows"] * c["cols"] == 196 and c["h"] == c["w"]:
        assert torch.equal(pos[1:], pe[0, 1:])


def test_determinism_batch_invariance_and_fused_normalisation():
    from nerf_sos_amd import ops
    c = fx.case(8)
    m = model(c["kind"])
    x = dino_in(c)
    a = {k: v.clone() for k, v in m.get_vit_attn_feat_noresize(x).items()}
    b = m.get_vit_attn_feat_noresize(x)
    for k in fx.OUTPUTS:
        assert torch.equal(a[k], b[k]), k
    for i in range(c["B"]):
        one = m.get_vit_attn_feat_noresize(x[i:i + 1].contiguous())
        for k in fx.OUTPUTS:
            assert torch.equal(one[k][0], a[k][i]), (k, i)
    rgb = torch.from_numpy(c["input"]).to(DEV)                 # normalize_batch fused into the prepare kernel: the same bits
    f = ops.dino_forward_full(rgb, m.packed_weights(), ops.DINO_FULL_NHWC | ops.DINO_FULL_NORMALIZE)
    for k in fx.OUTPUTS:
        assert torch.equal(f[k], a[k]), k


def test_captured_graph_replays_bit_equal():
    import nerf_sos_amd
    c = fx.case(6)
    m = nerf_sos_amd.DinoViT()
    m.load_state_dict(state(c["kind"]))
    m = m.to(DEV)
    x = dino_in(c)
    static = torch.zeros_like(x)
    m.get_vit_attn_feat_noresize(static)                       # packs and allocates outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = m.get_vit_attn_feat_noresize(static)
    torch.cuda.current_stream().wait_stream(s)
    static.copy_(x)
    g.replay()
    torch.cuda.synchronize()
    replayed = {k: out[k].clone() for k in fx.OUTPUTS}
    eager = m.get_vit_attn_feat_noresize(x)
    for k in fx.OUTPUTS:
        assert torch.equal(replayed[k], eager[k]), k


def test_224_agrees_with_the_resized_path():
    """At 224 x 224 the full path and get_vit_attn_feat(prepared=True) see the same network input: equal within the bar."""
    c = fx.case(3)
    m = model(c["kind"])
    x = dino_in(c)
    img = port.normalize(x)                                    # get_vit_attn_feat_noresize's own normalisation
    a = m.get_vit_attn_feat_noresize(x)
    b = m.get_vit_attn_feat(img.contiguous(), prepared=True)
    for k in fx.OUTPUTS:
        err = worst(a[k].cpu().numpy(), b[k].cpu().numpy())
        print(f"224x224 {k}: |full - resized path| {err:.3e}, bar {fx.bar(c, k):.3e}")
        assert a[k].shape == b[k].shape and err <= fx.bar(c, k), (k, err)


def _label_maps(up64):
    """Hand-built label maps over the upsampled fp64 attention [H,W]: a threshold map in both orientations, a disc around the
    most attended pixel, the same with a band of label 2 (three clusters)."""
    h, w = up64.shape
    hi = (up64 > np.median(up64)).astype(np.int32)
    y, x = np.mgrid[0:h, 0:w]
    cy, cx = np.unravel_index(np.argmax(up64), up64.shape)
    disc = (((y - cy) ** 2 + (x - cx) ** 2) <= (min(h, w) // 4) ** 2).astype(np.int32)
    three = (1 - disc).copy()
    three[: h // 8] = 2
    return {"bright_is_1": hi, "bright_is_0": 1 - hi, "disc_is_0": 1 - disc, "three_clusters": three}


@pytest.mark.parametrize("ci", [0, 2, 7])
def test_find_fg_labels_bit_equal(ci):
    """metrics.find_fg against engines/eval.py:138-144 restated in numpy on the reference's fp32 attn, for label maps whose fp64
    gap |mean1 - mean0| is at least 100 x the attn bar (asserted on the inputs: no tie can pass by luck)."""
    from nerf_sos_amd import metrics
    c = fx.case(ci)
    h, w = c["h"], c["w"]
    bar = fx.bar(c, "attn")
    up64 = port.upsample_attn(torch.from_numpy(c["ref64"]["attn"][0:1]), h, w)[..., 0].numpy()
    up32 = port.upsample_attn(torch.from_numpy(c["ref32"]["attn"][0:1]), h, w).numpy()
    rgb = torch.from_numpy(c["input"][0]).to(DEV)
    m = model(c["kind"])
    for name, lab in _label_maps(up64).items():
        gap = abs(up64[lab == 1].mean() - up64[lab == 0].mean())
        print(f"case {ci} {name}: fp64 gap {gap:.3e}, 100 x attn bar {100 * bar:.3e}")
        assert gap >= 100 * bar, (name, gap, bar)
        want, flip = port.find_fg_numpy(up32, lab[..., None])
        got = metrics.find_fg(torch.from_numpy(lab[..., None]).to(DEV), rgb, m)
        assert got["clustering"].dtype == torch.int32 and got["attn"].shape == (h, w, 1)
        assert np.array_equal(got["clustering"].cpu().numpy(), want), name
        assert int(got["flipped"]) == int(flip), name
    # an empty cluster: NaN mean, no flip
    lab = np.zeros((h, w, 1), np.int32)
    got = metrics.find_fg(torch.from_numpy(lab).to(DEV), rgb, m)
    assert int(got["flipped"]) == 0 and torch.equal(got["clustering"].cpu(), torch.from_numpy(lab))
    assert np.isnan(float(got["means"][1])) and np.isfinite(float(got["means"][0]))


def test_find_fg_attn_is_the_nearest_upsample():
    from nerf_sos_amd import metrics
    c = fx.case(6)
    m = model(c["kind"])
    rgb = torch.from_numpy(c["input"][0]).to(DEV)
    attn = m.get_vit_attn_feat_noresize(dino_in(c))["attn"][0:1]
    got = metrics.find_fg(torch.zeros(c["h"], c["w"], 1, dtype=torch.int32, device=DEV), rgb, m)
    assert torch.equal(got["attn"], port.upsample_attn(attn, c["h"], c["w"]))


def test_end_to_end_view_metrics_then_find_fg():
    """A full-size (flower, 756 x 1008) view: device view_metrics clusters the render's semantics, find_fg orients the labels.
    The semantics put a disc around the most attended region; its fp64 gap is asserted as above."""
    from nerf_sos_amd import metrics
    c = fx.case(0)
    h, w = c["h"], c["w"]
    up64 = port.upsample_attn(torch.from_numpy(c["ref64"]["attn"][0:1]), h, w)[..., 0].numpy()
    up32 = port.upsample_attn(torch.from_numpy(c["ref32"]["attn"][0:1]), h, w).numpy()
    disc = _label_maps(up64)["disc_is_0"] == 0
    logits = np.stack([np.where(disc, 2.0, -2.0), np.where(disc, -2.0, 2.0)], -1).astype(np.float32)
    ret = {"rgb": torch.from_numpy(c["input"][0]).to(DEV), "semantics": torch.from_numpy(logits).to(DEV)}
    vm = metrics.view_metrics(ret, N_cluster=2)
    clus = vm["clustering"]
    assert clus.shape == (h, w, 1) and clus.dtype == torch.int32
    lab = clus.cpu().numpy()
    gap = abs(up64[lab[..., 0] == 1].mean() - up64[lab[..., 0] == 0].mean())
    assert gap >= 100 * fx.bar(c, "attn"), gap
    got = metrics.find_fg(clus, ret["rgb"], model(c["kind"]))
    want, flip = port.find_fg_numpy(up32, lab)
    assert np.array_equal(got["clustering"].cpu().numpy(), want) and int(got["flipped"]) == int(flip)
    assert (got["clustering"].cpu().numpy()[disc] == 1).all()            # the attended disc ends up as cluster 1


def test_ops_validate():
    from nerf_sos_amd import metrics, ops
    m = model("init")
    packed = m.packed_weights()
    x = torch.zeros(1, 3, 64, 80, device=DEV)
    with pytest.raises(TypeError, match="float32"):
        ops.dino_forward_full(x.double(), packed)
    with pytest.raises(ValueError, match="channels"):
        ops.dino_forward_full(torch.zeros(1, 4, 64, 80, device=DEV), packed)
    with pytest.raises(ValueError, match="outside"):
        ops.dino_forward_full(torch.zeros(1, 3, 8, 80, device=DEV), packed)
    with pytest.raises(ValueError, match="bytes"):
        ops.dino_forward_full(x, packed, workspace=torch.zeros(16, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dino_forward_full(x, packed.cpu())
    lab = torch.zeros(64, 80, 1, dtype=torch.int32, device=DEV)
    attn = torch.zeros(20, device=DEV)
    with pytest.raises(TypeError, match="int32"):
        ops.dino_find_fg(lab.long(), attn, 64, 80)
    with pytest.raises(TypeError, match="float32"):
        ops.dino_find_fg(lab, attn.double(), 64, 80)
    with pytest.raises(ValueError, match="fit"):
        ops.dino_find_fg(lab, attn[:19], 64, 80)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dino_find_fg(lab, attn.cpu(), 64, 80)
    with pytest.raises(ValueError, match="rgb"):
        metrics.find_fg(lab, torch.zeros(64, 80, 4, device=DEV), m)
    with pytest.raises(ValueError, match="clustering"):
        metrics.find_fg(lab[:32], torch.zeros(64, 80, 3, device=DEV), m)

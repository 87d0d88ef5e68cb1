"""GPU: the HIP DINO ViT-S/16 extractor against the fixture written from the real reference (tests/golden/make_goldens_dino.py).

The bar is the one tests/test_gpu_losses_edges.py uses: max|gpu - fp64| <= max(4 * e32, 1e-6 * scale), e32 = the reference's own
fp32 distance from fp64 on that case, scale = max |fp64|, capped at 1e-4 * scale; every case, every output, every element.  Where the fixture holds only
the fp32 reference of an image (feat of images 1.. of a case) the distance to fp32 may be twice that.  Each comparison prints its
figures before it asserts."""
import os

import numpy as np
import pytest
import torch

import dino_fixture as fx
import dino_port as port
import dino_weights as dw
from helpers import state_sha

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_models = {}


def model(kind):
    import nerf_sos_amd
    if kind not in _models:
        m = nerf_sos_amd.DinoViT()
        m.load_state_dict(state(kind))
        _models[kind] = m.to(DEV)
    return _models[kind]


def state(kind):
    """The generated state dict, its sha256 checked against the fixture's before anything is compared."""
    sd = dw.make_state(kind, fx.meta()["seeds"][kind])
    assert state_sha(sd) == fx.meta()["state_sha256"][kind], f"make_state({kind!r}) differs from the generator's"
    return sd


def run(c, m=None, **want):
    m = m or model(c["kind"])
    x = torch.from_numpy(c["input"]).to(DEV)
    return m.patch_features(x, c["stride"], **want) if c["mode"] == "patch" else m.get_vit_attn_feat(x, **want)


def worst(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())


@pytest.mark.parametrize("ci", range(6))
def test_every_element_against_fp64(ci):
    c = fx.case(ci)
    out = {k: v.cpu().numpy() for k, v in run(c).items() if k in fx.OUTPUTS}
    torch.cuda.synchronize()
    fails = []
    for k in fx.OUTPUTS:
        bar = fx.bar(c, k)
        assert out[k].shape == c["ref32"][k].shape and np.isfinite(out[k]).all()
        if k == "feat":
            e64 = worst(out[k][0], c["ref64"]["feat0"])
            e32rest = worst(out[k][1:], c["ref32"][k][1:]) if c["B"] > 1 else 0.0
            print(f"case {ci} {c['kind']} feat: |gpu-fp64| {e64:.3e} (image 0), |gpu-fp32| {e32rest:.3e} (others), e32 {c['e32'][k]:.3e}, "
                  f"scale {c['scale'][k]:.3e}, bar {bar:.3e}, ratio to e32 {e64 / max(c['e32'][k], 1e-30):.2f}")
            if not (e64 <= bar and e32rest <= 2 * bar):
                fails.append((k, e64, e32rest, bar))
        else:
            e64 = worst(out[k], c["ref64"][k])
            print(f"case {ci} {c['kind']} {k}: |gpu-fp64| {e64:.3e}, e32 {c['e32'][k]:.3e}, scale {c['scale'][k]:.3e}, bar {bar:.3e}, "
                  f"ratio to e32 {e64 / max(c['e32'][k], 1e-30):.2f}")
            if not e64 <= bar:
                fails.append((k, e64, bar))
    assert not fails, fails
    for k in fx.OUTPUTS:                     # the end-to-end ceiling, whatever e32 says
        assert fx.bar(c, k) <= 1e-4 * c["scale"][k]
        assert worst(out[k][:1], c["ref64"]["feat0"][None] if k == "feat" else c["ref64"][k][:1]) <= 1e-4 * c["scale"][k], k


def test_block_checkpoints_localise():
    """Blocks 0 and 5 of image 0 of case 0 against the reference's fp64 run, same bar."""
    c = fx.case(0)
    blocks = run(c, want_blocks=True)["blocks"].cpu().numpy()
    for k in (0, 5):
        d = dict(np.load(os.path.join(fx.GOLDEN, f"dino_vit_block{k}.npz")))
        err, e32, scale = worst(blocks[k][0][:d["out64"].shape[0]], d["out64"]), float(d["e32"]), float(np.abs(d["out64"]).max())
        print(f"block {k}: |gpu-fp64| {err:.3e}, e32 {e32:.3e}, scale {scale:.3e}, ratio {err / e32:.2f}")
        assert err <= min(max(4 * e32, 1e-6 * scale), 1e-4 * scale)
        assert d["out64"].shape[0] <= blocks[k][0].shape[0]


def test_prepared_image_is_bit_equal():
    p = dict(np.load(os.path.join(fx.GOLDEN, "dino_vit_prepared.npz")))
    c = fx.case(int(p["case"]))
    got = run(c, want_prepared=True)["prepared"][int(p["index"])].cpu().numpy()
    assert np.array_equal(got, p["image"])
    for ci in range(fx.n_cases()):          # and equal to torch's own resize + normalise on this GPU, for every case
        c = fx.case(ci)
        x = torch.from_numpy(c["input"]).to(DEV)
        want = port.prepare(x, c["stride"]) if c["mode"] == "patch" else port.extractor_step2(x)
        assert torch.equal(run(c, want_prepared=True)["prepared"], want), ci


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_negatives_match(ci):
    from nerf_sos_amd import losses
    c = fx.case(ci)
    assert c["gap"] > fx.meta()["gap_bar"]
    neg = losses.similarity_negatives(run(c)["cls_"])
    assert neg.cpu().tolist() == c["argmin"].tolist()


def test_batch_invariance_and_determinism():
    c = fx.case(0)
    m = model(c["kind"])
    x = torch.from_numpy(c["input"]).to(DEV)
    a = {k: v.clone() for k, v in m.patch_features(x, c["stride"]).items()}
    b = m.patch_features(x, c["stride"])
    for k in fx.OUTPUTS:
        assert torch.equal(a[k], b[k]), k
    for i in (0, 3, 7):
        one = m.patch_features(x[i:i + 1].contiguous(), c["stride"])
        for k in fx.OUTPUTS:
            assert torch.equal(one[k][0], a[k][i]), (k, i)


@pytest.mark.parametrize("ci", [0, 2, 4])
def test_interfaces_agree_with_each_other_and_the_port(ci):
    c = fx.case(ci)
    m = model(c["kind"])
    sd = {k: v.to(DEV) for k, v in state(c["kind"]).items()}
    x = torch.from_numpy(c["input"]).to(DEV)
    if c["mode"] == "patch":
        a = m.patch_features(x, c["stride"])
        b = m.get_vit_attn_feat(port.trainer_step1(x, c["stride"]).contiguous())       # the trainer's own call sequence
        d = m.patch_features(x.permute(0, 3, 1, 2).contiguous(), c["stride"])          # channels first
        ref = port.patch_features(sd, x, c["stride"])
        img = port.prepare(x, c["stride"])
    else:
        a = m.get_vit_attn_feat(x)
        b = d = m(x)
        ref = port.get_vit_attn_feat(sd, x)
        img = port.extractor_step2(x)
    e = m.get_vit_attn_feat(img.contiguous(), prepared=True)
    for k in fx.OUTPUTS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], d[k]) and torch.equal(a[k], e[k]), k
        err = worst(a[k].cpu().numpy(), ref[k].cpu().numpy())
        print(f"case {ci} {k}: |hip - port on the GPU| {err:.3e}, bar {fx.bar(c, k):.3e}")
        assert err <= fx.bar(c, k), (k, err)
    if c["mode"] == "patch":
        assert a["feats"].shape == (c["B"], 384, 14, 14) and a["feats"].data_ptr() == a["feat"].data_ptr() and a["cls_tokens"] is a["cls_"]
        assert torch.equal(a["feats"][:, :, 3, 5], a["feat"][:, 3 * 14 + 5, :])


def test_capture_and_repack():
    import nerf_sos_amd
    c = fx.case(1)
    m = nerf_sos_amd.DinoViT()
    m.load_state_dict(state("init"))
    m = m.to(DEV)
    x = torch.from_numpy(c["input"]).to(DEV)
    static = torch.zeros_like(x)
    m.patch_features(static, c["stride"])                        # packs and allocates outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            out = m.patch_features(static, c["stride"])
    torch.cuda.current_stream().wait_stream(s)
    static.copy_(x)
    g.replay()
    torch.cuda.synchronize()
    replayed = {k: out[k].clone() for k in fx.OUTPUTS}
    eager = m.patch_features(x, c["stride"])
    for k in fx.OUTPUTS:
        assert torch.equal(replayed[k], eager[k]), k
    before = eager["cls_"].clone()
    with torch.no_grad():
        m.blocks[3].mlp.fc1.bias.add_(0.25)                      # bumps _version: the next call packs again
    after = m.patch_features(x, c["stride"])["cls_"]
    assert not torch.equal(before, after)
    with torch.no_grad():
        m.blocks[3].mlp.fc1.bias.sub_(0.25)
    assert torch.equal(m.patch_features(x, c["stride"])["cls_"], before)


def test_losses_take_the_features():
    """feat / cls_ through similarity_negatives and CorrelationLoss give what the same losses give on the port's features."""
    from nerf_sos_amd import losses
    c = fx.case(0)
    sd = {k: v.to(DEV) for k, v in state(c["kind"]).items()}
    x = torch.from_numpy(c["input"]).to(DEV)
    mine = model(c["kind"]).patch_features(x, c["stride"])
    ref = port.patch_features(sd, x, c["stride"])
    B = c["B"]
    neg_a, sim_a = losses.similarity_negatives(mine["cls_tokens"], want_similarity=True)
    neg_b, sim_b = losses.similarity_negatives(ref["cls_"].contiguous(), want_similarity=True)
    assert torch.equal(neg_a, neg_b)
    assert float((sim_a - sim_b).abs().max()) <= 1e-5
    code = torch.rand(B, 2, 64, 64, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    feats_b = ref["feat"].reshape(B, 14, 14, 384).permute(0, 3, 1, 2)
    vals = []
    for feats, sim in ((mine["feats"], sim_a), (feats_b, sim_b)):
        torch.manual_seed(7)
        loss = losses.CorrelationLoss()
        vals.append(float(loss(feats, code, sim)))
    print("correlation loss on hip / port features:", vals)
    assert abs(vals[0] - vals[1]) <= 1e-4 * (1.0 + abs(vals[1]))


def test_ops_wrappers_validate():
    """A wrong-shaped tensor under a right name, a host-side or short `packed` / `workspace`: refused in Python, nothing launched."""
    from nerf_sos_amd import ops
    sd = {k: v.to(DEV) for k, v in state("init").items()}
    packed = ops.dino_pack(sd)
    bad = dict(sd)
    bad["blocks.4.mlp.fc1.weight"] = sd["blocks.4.mlp.fc1.weight"][:, :100].contiguous()
    with pytest.raises(ValueError, match="shape"):
        ops.dino_pack(bad)
    with pytest.raises(ValueError, match="bytes"):
        ops.dino_pack(sd, packed[:1000])
    x = torch.zeros(1, 3, 32, 32, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dino_forward(x, packed.cpu(), 0)
    with pytest.raises(ValueError, match="bytes"):
        ops.dino_forward(x, packed[:1000], 0)
    with pytest.raises(ValueError, match="bytes"):
        ops.dino_forward(x, packed, 0, workspace=torch.zeros(16, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dino_forward(x, packed, 0, workspace=torch.zeros(1 << 20))

"""GPU: the 16-bit (fp16 / bf16 operand) DINO ViT-S/16 path against the fp64 fixture of the real reference.

The yardstick is tests/golden/dino_vit16.npz: e16 = max |model - fp64| of tests/dino16_model.py (the torch port with the operands
of every matrix product rounded to 16 bits) in two legitimate placements of the roundings, written on a CPU by
tests/golden/make_goldens_dino16.py -- never the kernels under test.  The bar, every case x precision x output, every element:

    max |gpu - fp64| <= 2 * max(e16_A, e16_B)

(the two placements differ by up to 1.5x in these maxima and the kernels' fp32 summation orders resample the same error population;
a wrong operand layout, a missed K tile or a swapped head is 100x to 1000x further out).  Where the fixture holds only the fp32
reference of an image (feat of images 1.. of a case) the distance to fp32 may be that bar plus the fp32 bar.  Each comparison
prints its figures before it asserts.

Measured on the MI355X: max |gpu - fp64| / max(e16_A, e16_B) is 0.63 .. 1.26 over the 36 (case, precision, output) triples (the table
is in DESIGN.md 4.10.2), 0.94 .. 1.00 on the block checkpoints.
"""
import json
import os

import numpy as np
import pytest
import torch

import dino16_model as m16
import dino_fixture as fx
import dino_port as port
import dino_weights as dw
from helpers import state_sha

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRECISIONS = ("fp16", "bf16")
_models = {}
G = dict(np.load(os.path.join(fx.GOLDEN, "dino_vit16.npz")))
META = json.loads(str(G["meta"]))
assert tuple(META["precisions"]) == PRECISIONS and META["placements"] == ["A", "B"] and tuple(META["outputs"]) == fx.OUTPUTS
# the negatives cases: a condition on the inputs (the committed gap against the model's own similarity error), both placements
NEGATIVES = [(ci, p) for ci in (0, 1, 2) for pi, p in enumerate(PRECISIONS) if fx.case(ci)["gap"] > 4.0 * float(G["dsim"][ci, pi].max())]


def state(kind):
    """The generated state dict, its sha256 checked against the fixture's before anything is compared."""
    sd = dw.make_state(kind, fx.meta()["seeds"][kind])
    assert state_sha(sd) == fx.meta()["state_sha256"][kind], f"make_state({kind!r}) differs from the generator's"
    return sd


def model(kind, precision):
    """One module per weight kind; the precision is switched on it, as a user would."""
    import nerf_sos_amd
    if kind not in _models:
        m = nerf_sos_amd.DinoViT()
        m.load_state_dict(state(kind))
        _models[kind] = m.to(DEV)
    _models[kind].precision = precision
    return _models[kind]


def fresh(kind, precision):
    import nerf_sos_amd
    m = nerf_sos_amd.DinoViT(precision=precision)
    m.load_state_dict(state(kind))
    return m.to(DEV)


def run(c, m, **want):
    x = torch.from_numpy(c["input"]).to(DEV)
    return m.patch_features(x, c["stride"], **want) if c["mode"] == "patch" else m.get_vit_attn_feat(x, **want)


def worst(got, want):
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)).max())


def bar16(ci, precision, k):
    pi, oi = PRECISIONS.index(precision), fx.OUTPUTS.index(k)
    e = float(G["e16"][ci, pi, :, oi].max())
    return 2.0 * e, e


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("ci", range(6))
def test_every_element_against_fp64(ci, precision):
    c = fx.case(ci)
    got = run(c, model(c["kind"], precision))
    assert all(v.dtype == torch.float32 for v in got.values())
    out = {k: got[k].cpu().numpy() for k in fx.OUTPUTS}
    fails = []
    for k in fx.OUTPUTS:
        bar, e16 = bar16(ci, precision, k)
        assert out[k].shape == c["ref32"][k].shape and np.isfinite(out[k]).all(), k
        if k == "feat":
            e64 = worst(out[k][0], c["ref64"]["feat0"])
            e32rest = worst(out[k][1:], c["ref32"][k][1:]) if c["B"] > 1 else 0.0
            print(f"case {ci} {c['kind']} {precision} feat: |gpu-fp64| {e64:.3e} (image 0), |gpu-fp32| {e32rest:.3e} (others), "
                  f"e16 A/B {G['e16'][ci, PRECISIONS.index(precision), 0, 2]:.3e}/{G['e16'][ci, PRECISIONS.index(precision), 1, 2]:.3e}, "
                  f"scale {c['scale'][k]:.3e}, bar {bar:.3e}, ratio to e16 {e64 / e16:.2f}, others {e32rest / e16:.2f}")
            if not (e64 <= bar and e32rest <= bar + fx.bar(c, k)):
                fails.append((k, e64, e32rest, bar))
        else:
            e64 = worst(out[k], c["ref64"][k])
            oi = fx.OUTPUTS.index(k)
            print(f"case {ci} {c['kind']} {precision} {k}: |gpu-fp64| {e64:.3e}, "
                  f"e16 A/B {G['e16'][ci, PRECISIONS.index(precision), 0, oi]:.3e}/{G['e16'][ci, PRECISIONS.index(precision), 1, oi]:.3e}, "
                  f"scale {c['scale'][k]:.3e}, bar {bar:.3e}, ratio to e16 {e64 / e16:.2f}")
            if not e64 <= bar:
                fails.append((k, e64, bar))
    assert not fails, fails


@pytest.mark.parametrize("precision", PRECISIONS)
def test_block_checkpoints_localise(precision):
    """Blocks 0 and 5 of image 0 of case 0 against the reference's fp64 run: the same rule on the model's blocks."""
    c = fx.case(0)
    blocks = run(c, model(c["kind"], precision), want_blocks=True)["blocks"]
    assert blocks.dtype == torch.float32 and tuple(blocks.shape) == (12, c["B"], 197, 384)
    blocks = blocks.cpu().numpy()
    pi = PRECISIONS.index(precision)
    fails = []
    for bi, k in enumerate(META["blocks"]):
        d = dict(np.load(os.path.join(fx.GOLDEN, f"dino_vit_block{k}.npz")))
        err, e16 = worst(blocks[k][0][:d["out64"].shape[0]], d["out64"]), float(G["block_e16"][bi, pi].max())
        print(f"block {k} {precision}: |gpu-fp64| {err:.3e}, e16 {e16:.3e}, ratio {err / e16:.2f}")
        if not err <= 2.0 * e16:
            fails.append((k, err, e16))
    assert not fails, fails


@pytest.mark.parametrize("precision", PRECISIONS)
def test_prepared_image_is_bit_equal_to_the_fp32_path(precision):
    for ci in range(fx.n_cases()):
        c = fx.case(ci)
        a = run(c, model(c["kind"], precision), want_prepared=True)["prepared"].clone()
        b = run(c, model(c["kind"], "fp32"), want_prepared=True)["prepared"]
        assert a.dtype == torch.float32 and torch.equal(a, b), ci


@pytest.mark.parametrize("ci,precision", NEGATIVES)
def test_negatives_match(ci, precision):
    from nerf_sos_amd import losses
    c = fx.case(ci)
    pi = PRECISIONS.index(precision)
    print(f"case {ci} {precision}: gap {c['gap']:.3e}, dsim A/B {G['dsim'][ci, pi, 0]:.3e}/{G['dsim'][ci, pi, 1]:.3e}")
    neg = losses.similarity_negatives(run(c, model(c["kind"], precision))["cls_"])
    assert neg.cpu().tolist() == c["argmin"].tolist()


def test_negatives_cases_kept():
    assert sum(p == "fp16" for _, p in NEGATIVES) >= 2 and sum(p == "bf16" for _, p in NEGATIVES) >= 1, NEGATIVES


@pytest.mark.parametrize("precision", PRECISIONS)
def test_batch_invariance_and_determinism(precision):
    c = fx.case(0)
    m = model(c["kind"], precision)
    x = torch.from_numpy(c["input"]).to(DEV)
    a = {k: v.clone() for k, v in m.patch_features(x, c["stride"]).items()}
    b = m.patch_features(x, c["stride"])
    for k in fx.OUTPUTS:
        assert torch.equal(a[k], b[k]), k
    for i in range(c["B"]):
        one = m.patch_features(x[i:i + 1].contiguous(), c["stride"])
        for k in fx.OUTPUTS:
            assert torch.equal(one[k][0], a[k][i]), (k, i)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("ci", [0, 2, 4])
def test_interfaces_agree_with_each_other(ci, precision):
    c = fx.case(ci)
    m = model(c["kind"], precision)
    x = torch.from_numpy(c["input"]).to(DEV)
    if c["mode"] == "patch":
        a = {k: v.clone() for k, v in m.patch_features(x, c["stride"]).items()}
        b = m.get_vit_attn_feat(port.trainer_step1(x, c["stride"]).contiguous())       # the trainer's own call sequence
        d = m.patch_features(x.permute(0, 3, 1, 2).contiguous(), c["stride"])          # channels first
        img = port.prepare(x, c["stride"])
    else:
        a = {k: v.clone() for k, v in m.get_vit_attn_feat(x).items()}
        b = d = m(x)
        img = port.extractor_step2(x)
    e = m.get_vit_attn_feat(img.contiguous(), prepared=True)
    for k in fx.OUTPUTS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], d[k]) and torch.equal(a[k], e[k]), k
    if c["mode"] == "patch":
        assert a["feats"].shape == (c["B"], 384, 14, 14) and torch.equal(a["feats"][:, :, 3, 5], a["feat"][:, 3 * 14 + 5, :])
        assert torch.equal(a["cls_tokens"], a["cls_"])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_capture_and_repack(precision):
    c = fx.case(1)
    m = fresh("init", precision)
    x = torch.from_numpy(c["input"]).to(DEV)
    static = torch.zeros_like(x)
    m.patch_features(static, c["stride"])                        # packs and allocates outside the capture
    torch.cuda.synchronize()
    assert m._packed is None and list(m._packed16) == [precision] and m._workspace == {}     # the 16-bit stream and workspace only
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
        m.blocks[3].mlp.fc1.bias.add_(0.25)                      # bumps _version: the next call packs the 16-bit stream again
    after = m.patch_features(x, c["stride"])["cls_"]
    assert not torch.equal(before, after)
    with torch.no_grad():
        m.blocks[3].mlp.fc1.bias.sub_(0.25)
    assert torch.equal(m.patch_features(x, c["stride"])["cls_"], before)
    with torch.no_grad():
        m.blocks[7].attn.qkv.weight.mul_(1.5)                    # a matrix: the rounded stream, not only the fp32 section
    assert not torch.equal(m.patch_features(x, c["stride"])["cls_"], before)


def test_fp32_after_16_bit_is_untouched():
    """precision = "fp32" after fp16 and bf16 calls on the same module gives exactly what a fresh fp32 module gives, and the other
    way round: the packed streams and workspaces do not disturb each other."""
    c = fx.case(0)
    want32 = {k: v.clone() for k, v in run(c, fresh(c["kind"], "fp32")).items() if k in fx.OUTPUTS}
    want16 = {p: {k: v.clone() for k, v in run(c, fresh(c["kind"], p)).items() if k in fx.OUTPUTS} for p in PRECISIONS}
    m = fresh(c["kind"], "fp16")
    for p in ("fp16", "fp32", "bf16", "fp32", "fp16", "bf16"):
        m.precision = p
        got = run(c, m)
        for k in fx.OUTPUTS:
            assert torch.equal(got[k], want32[k] if p == "fp32" else want16[p][k]), (p, k)
    assert not torch.equal(want16["fp16"]["cls_"], want16["bf16"]["cls_"]) and not torch.equal(want16["fp16"]["cls_"], want32["cls_"])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_full_image_path_refuses(precision):
    m = model("init", precision)
    with pytest.raises(ValueError, match="full-image"):
        m.get_vit_attn_feat_noresize(torch.zeros(1, 3, 64, 64, device=DEV))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_losses_take_the_features(precision):
    """CorrelationLoss on the 16-bit feats against the same loss on the fp32 HIP feats:
    |delta| <= 2 * |delta_model| + 1e-4 * (1 + |loss|), delta_model = the same difference with dino16_model's features (on the GPU)."""
    from nerf_sos_amd import losses
    c = fx.case(0)
    sd = {k: v.to(DEV) for k, v in state(c["kind"]).items()}
    x = torch.from_numpy(c["input"]).to(DEV)
    B = c["B"]
    f32 = {k: v.clone() for k, v in model(c["kind"], "fp32").patch_features(x, c["stride"]).items()}
    f16 = {k: v.clone() for k, v in model(c["kind"], precision).patch_features(x, c["stride"]).items()}
    ref = m16.run_case(sd, c, x, precision, "A")
    code = torch.rand(B, 2, 64, 64, device=DEV, generator=torch.Generator(DEV).manual_seed(5))
    vals = []
    for feats, cls_ in ((f32["feats"], f32["cls_tokens"]), (f16["feats"], f16["cls_tokens"]),
                        (ref["feat"].reshape(B, 14, 14, 384).permute(0, 3, 1, 2), ref["cls_"].contiguous())):
        _, sim = losses.similarity_negatives(cls_, want_similarity=True)
        torch.manual_seed(7)
        loss = losses.CorrelationLoss()
        vals.append(float(loss(feats, code, sim)))
    l32, l16, lm = vals
    print(f"correlation loss {precision}: fp32 hip {l32:.8f}, 16-bit hip {l16:.8f}, 16-bit model {lm:.8f}; "
          f"delta {l16 - l32:.3e}, delta_model {lm - l32:.3e}")
    assert np.isfinite(vals).all()
    assert abs(l16 - l32) <= 2.0 * abs(lm - l32) + 1e-4 * (1.0 + abs(l32))


def test_ops16_wrappers_validate():
    """A wrong-shaped tensor under a right name, a host-side or short `packed` / `workspace`, an fp32 stream handed to the 16-bit
    call: refused in Python, nothing launched."""
    from nerf_sos_amd import ops
    sd = {k: v.to(DEV) for k, v in state("init").items()}
    packed = ops.dino_pack16(sd, "bf16")
    assert packed.numel() * 4 == ops._lib.lib().nsos_dino_packed16_bytes()
    bad = dict(sd)
    bad["blocks.4.mlp.fc1.weight"] = sd["blocks.4.mlp.fc1.weight"][:, :100].contiguous()
    with pytest.raises(ValueError, match="shape"):
        ops.dino_pack16(bad, "fp16")
    with pytest.raises(ValueError, match="bytes"):
        ops.dino_pack16(sd, "fp16", packed[:1000])
    with pytest.raises(ValueError, match="fp16"):
        ops.dino_pack16(sd, "fp32")
    x = torch.zeros(1, 3, 32, 32, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dino_forward16(x, packed.cpu(), 0, "bf16")
    with pytest.raises(ValueError, match="bytes"):
        ops.dino_forward16(x, packed[:1000], 0, "bf16")
    with pytest.raises(ValueError, match="bytes"):
        ops.dino_forward16(x, packed, 0, "bf16", workspace=torch.zeros(16, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.dino_forward16(x, packed, 0, "bf16", workspace=torch.zeros(1 << 20))
    with pytest.raises(ValueError, match="fp16"):
        ops.dino_forward16(x, packed, 0, "fp32")
    out = ops.dino_forward16(x, packed, 0, "bf16")
    assert all(v.dtype == torch.float32 and bool(torch.isfinite(v).all()) for v in out.values())

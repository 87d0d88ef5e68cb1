"""Host-side contract of the training step's `dino=` option (no GPU): where a step's DINO features come from is decided -- and
refused -- before any tensor's device is looked at, so every rule here is exercised on CPU tensors.

  * sharding.sharded_patch_step(..., dino=, patch_stride=): the four argument errors;
  * graphs.GraphedPatchStep(..., dino=, patch_stride=): the same rule at construction, and load()'s two forms;
  * ops._dino_forward(out=...): the shape / dtype / contiguity / key checks, which precede the device check.
"""
import pytest
import torch

import nerf_sos_amd
from nerf_sos_amd import ops, sharding


@pytest.fixture(scope="module")
def dino():
    return nerf_sos_amd.DinoViT()


def _step(feat, cls_tokens, **kw):
    rays = torch.zeros(2, 2, 4, 4, 3)
    return sharding.sharded_patch_step(None, rays, (2.0, 6.0), 2, feat, cls_tokens, **kw)


FEAT, CLS = torch.zeros(2, 384, 14, 14), torch.zeros(2, 384)


# ---- sharded_patch_step
@pytest.mark.parametrize("feat,cls_tokens", [(FEAT, CLS), (FEAT, None), (None, CLS)])
def test_step_refuses_dino_together_with_features(dino, feat, cls_tokens):
    with pytest.raises(ValueError, match="must be None"):
        _step(feat, cls_tokens, dino=dino, patch_stride=2)


@pytest.mark.parametrize("stride", [None, 0, -1, 2.0, "2", True])
def test_step_refuses_dino_without_an_integer_patch_stride(dino, stride):
    with pytest.raises(ValueError, match="patch_stride"):
        _step(None, None, dino=dino, patch_stride=stride)


@pytest.mark.parametrize("feat,cls_tokens", [(None, None), (FEAT, None), (None, CLS)])
def test_step_without_any_features_names_both_ways(feat, cls_tokens):
    with pytest.raises(ValueError) as e:
        _step(feat, cls_tokens)
    msg = str(e.value)
    assert "feat" in msg and "cls_tokens" in msg and "dino=" in msg and "patch_stride" in msg


@pytest.mark.parametrize("other", [object(), torch.nn.Linear(3, 3), "dino", 1])
def test_step_refuses_an_extractor_that_is_no_dinovit(other):
    with pytest.raises(TypeError, match="DinoViT"):
        _step(None, None, dino=other, patch_stride=2)


def test_step_refuses_patch_stride_and_dino_out_without_dino():
    with pytest.raises(ValueError, match="patch_stride"):
        _step(FEAT, CLS, patch_stride=2)
    with pytest.raises(ValueError, match="dino_out"):
        _step(FEAT, CLS, dino_out={"feat": torch.zeros(2, 196, 384), "cls_": CLS})


def test_new_step_parameters_are_keyword_only():
    import inspect
    for fn in (sharding.sharded_patch_step, nerf_sos_amd.GraphedPatchStep.__init__):
        ps = inspect.signature(fn).parameters
        for name in ("dino", "patch_stride"):
            assert ps[name].kind is inspect.Parameter.KEYWORD_ONLY and ps[name].default is None, (fn, name)


# ---- GraphedPatchStep
def _graphed(feat, cls_tokens, **kw):
    return nerf_sos_amd.GraphedPatchStep(None, None, torch.zeros(2, 2, 4, 4, 3), (2.0, 6.0), feat, cls_tokens, **kw)


def test_graphed_step_applies_the_same_rule_first(dino):
    with pytest.raises(ValueError, match="must be None"):
        _graphed(FEAT, CLS, dino=dino, patch_stride=2)
    with pytest.raises(ValueError, match="patch_stride"):
        _graphed(None, None, dino=dino)
    with pytest.raises(ValueError, match="dino="):
        _graphed(None, None)
    with pytest.raises(TypeError, match="DinoViT"):
        _graphed(None, None, dino=object(), patch_stride=2)


def test_graphed_step_load_takes_rays_alone_with_dino(dino):
    g = object.__new__(nerf_sos_amd.GraphedPatchStep)       # load() reads only these attributes
    g.dino, g.rays = dino, torch.zeros(2, 2, 4, 4, 3)
    with pytest.raises(ValueError, match="rays alone"):
        g.load(torch.ones(2, 2, 4, 4, 3), FEAT, CLS)
    with pytest.raises(ValueError, match="rays alone"):
        g.load(torch.ones(2, 2, 4, 4, 3), cls_tokens=CLS)
    assert float(g.rays.sum()) == 0.0                       # refused before anything was copied
    g.load(torch.ones(2, 2, 4, 4, 3))
    assert float(g.rays.min()) == 1.0


def test_graphed_step_load_keeps_its_three_argument_form_without_dino():
    g = object.__new__(nerf_sos_amd.GraphedPatchStep)
    g.dino, g.rays, g.feat, g.cls = None, torch.zeros(2, 2, 4, 4, 3), torch.zeros_like(FEAT), torch.zeros_like(CLS)
    with pytest.raises(TypeError):
        g.load(torch.ones(2, 2, 4, 4, 3))
    g.load(torch.ones(2, 2, 4, 4, 3), FEAT + 2, CLS + 3)
    assert float(g.rays.min()) == 1.0 and float(g.feat.min()) == 2.0 and float(g.cls.min()) == 3.0


# ---- ops._dino_forward(out=...)
def _forward(out, x=None, precision="fp32"):
    x = torch.zeros(2, 8, 8, 3) if x is None else x
    return ops._dino_forward(x, None, ops.DINO_NHWC | ops.DINO_STEP1, 2, None, False, False, False, precision, out)


def _good():
    return {"feat": torch.zeros(2, 196, 384), "cls_": torch.zeros(2, 384)}


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
@pytest.mark.parametrize("name,bad", [
    ("feat", torch.zeros(1, 196, 384)), ("feat", torch.zeros(2, 384, 196)), ("feat", torch.zeros(2, 384, 14, 14)),
    ("feat", torch.zeros(2, 196, 384, dtype=torch.float16)), ("feat", torch.zeros(2, 196, 768)[:, :, ::2]),
    ("cls_", torch.zeros(2, 1, 384)), ("cls_", torch.zeros(3, 384)), ("cls_", torch.zeros(2, 384, dtype=torch.float64)),
    ("cls_", torch.zeros(384, 2).t()), ("cls_", None)])
def test_out_buffers_are_checked_before_the_device(name, bad, precision):
    out = _good()
    out[name] = bad
    with pytest.raises(ValueError, match=name):
        _forward(out, precision=precision)


def test_out_must_hold_exactly_feat_and_cls():
    for out in ({"feat": _good()["feat"]}, dict(_good(), attn=torch.zeros(2, 1, 196)), (_good()["feat"], _good()["cls_"])):
        with pytest.raises(ValueError, match="'feat' and 'cls_'"):
            _forward(out)
    with pytest.raises(ValueError, match="4-d"):
        _forward(_good(), x=torch.zeros(8, 8, 3))


def test_valid_out_buffers_reach_the_device_check():
    """Nothing above is an artefact of the CPU: buffers that satisfy the contract get as far as `no CPU path`."""
    with pytest.raises(RuntimeError, match="no CPU path"):
        _forward(_good())

"""CPU: the torch restatement of the loss / post-processing rows (oracle/losses_port.py) against the goldens captured
from the real reference classes.  The O(P^4) full-size geometric case is left to the GPU test (the port needs
several GB and ~20 s for it); the small case exercises the same code."""
import os

import numpy as np
import pytest
import torch

from oracle import losses_port as lp

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "losses.npz"))
APP, GEO = (0.18, 1, 0.46, 1), (0.5, 1, 3, 1)
t = lambda k: torch.from_numpy(GOLD[k])  # noqa: E731


def test_eval_postprocess_port():
    out = lp.eval_postprocess(t("post_sem"), t("post_rgb"), t("post_tgt"))
    assert np.array_equal(out["sem"].numpy(), GOLD["post_pred"]) and out["sem"].dtype == torch.int32
    assert np.array_equal(out["sem_prob"].numpy(), GOLD["post_prob"])
    assert np.array_equal(out["mse"].numpy(), GOLD["post_mse"]) and np.array_equal(out["psnr"].numpy(), GOLD["post_psnr"])
    assert out["sem"][0, 0, 0] == 0   # tie -> first index


@pytest.mark.parametrize("tag", ["app_small", "app_full"])
def test_correlation_loss_port(tag):
    code = t(f"{tag}_code").clone().requires_grad_(True)
    loss = lp.correlation_loss(t(f"{tag}_feats"), code, lp.neg_index(t(f"{tag}_sim")), t(f"{tag}_rand1") * 2 - 1,
                               t(f"{tag}_rand2") * 2 - 1, lp.CorrParams(*APP))
    loss.backward()
    assert abs(loss.item() - GOLD[f"{tag}_loss"][0]) <= 1e-6 * abs(GOLD[f"{tag}_loss"][0])
    g = GOLD[f"{tag}_grad"]
    assert np.abs(code.grad.numpy() - g).max() <= 1e-6 * np.abs(g).max()


def test_geo_correlation_loss_port():
    tag = "geo_small"
    depth = t(f"{tag}_depth").clone()
    B, _, P, _ = depth.shape
    code = t(f"{tag}_code").clone().requires_grad_(True)
    ray_o = t(f"{tag}_ray_o")[:, :, None, None].expand(B, 3, P, P)
    loss = lp.geo_correlation_loss(depth, code, ray_o, t(f"{tag}_ray_d"), lp.neg_index(t(f"{tag}_sim")), lp.CorrParams(*GEO))
    loss.backward()
    assert abs(loss.item() - GOLD[f"{tag}_loss"][0]) <= 1e-6 * abs(GOLD[f"{tag}_loss"][0])
    assert np.array_equal(depth.numpy(), GOLD[f"{tag}_depth_after"])
    g = GOLD[f"{tag}_grad"]
    assert np.abs(code.grad.numpy() - g).max() <= 1e-6 * np.abs(g).max()


EDGE = np.load(os.path.join(os.path.dirname(__file__), "golden", "losses_edges.npz"))
EDGE_APP = sorted(k[:-6] for k in EDGE.files if k.endswith("_feats"))
EDGE_GEO = sorted(k[:-6] for k in EDGE.files if k.endswith("_depth"))
e = lambda k: torch.from_numpy(EDGE[k])  # noqa: E731


def _edge_neg(tag):
    """The negatives the reference used: the column arg-min of sim_matrix, or super_perm of the recorded randperm draw."""
    B = EDGE[f"{tag}_code"].shape[0]
    neg = lp.neg_index(e(f"{tag}_sim")) if f"{tag}_sim" in EDGE.files else lp.super_perm(e(f"{tag}_perm"))
    assert np.array_equal(neg.numpy(), EDGE[f"{tag}_neg"]) and neg.shape == (B,)
    if f"{tag}_sim" not in EDGE.files:
        assert sorted(EDGE[f"{tag}_perm"].tolist()) == list(range(B))
        assert B == 1 or (neg != torch.arange(B)).all()          # super_perm never pairs a patch with itself
    return neg


def test_edge_goldens_cover_the_issue_axes():
    """losses_edges.npz reaches what losses.npz does not: code widths 1, 3, 4; S != 11 up to 32; Cf below 2 * kMaxC and odd;
    non-square and one-pixel maps; ragged N; B in {1, 2, 5}; super_perm negatives; a whole patch beyond max_depth."""
    widths = {EDGE[f"{t}_code"].shape[1] for t in EDGE_APP} & {EDGE[f"{t}_code"].shape[1] for t in EDGE_GEO}
    assert {1, 3, 4} <= widths
    S = {EDGE[f"{t}_rand1"].shape[1] for t in EDGE_APP}
    assert 32 in S and len(S - {11}) >= 3
    Cf = {EDGE[f"{t}_feats"].shape[1] for t in EDGE_APP}
    assert {3, 7} <= Cf and any(c > 8 and c % 2 for c in Cf)
    assert any(1 in EDGE[f"{t}_code"].shape[2:] for t in EDGE_APP) and any(1 in EDGE[f"{t}_code"].shape[2:] for t in EDGE_GEO)
    assert any(EDGE[f"{t}_code"].shape[2] != EDGE[f"{t}_code"].shape[3] for t in EDGE_GEO)
    Ns = [EDGE[f"{t}_depth"].shape[2] * EDGE[f"{t}_depth"].shape[3] for t in EDGE_GEO]
    assert sum(n % 64 != 0 for n in Ns) >= 3
    assert {1, 2, 5} <= {EDGE[f"{t}_code"].shape[0] for t in EDGE_GEO}
    assert all(any(f"{t}_sim" not in EDGE.files for t in ts) for ts in (EDGE_APP, EDGE_GEO))
    assert any((EDGE[f"{t}_depth"] > 15).reshape(EDGE[f"{t}_depth"].shape[0], -1).all(1).any()
               or (EDGE[f"{t}_depth"] >= 15).reshape(EDGE[f"{t}_depth"].shape[0], -1).all(1).any() for t in EDGE_GEO)


@pytest.mark.parametrize("tag", EDGE_APP)
def test_correlation_loss_port_at_edge_shapes(tag):
    S = EDGE[f"{tag}_rand1"].shape[1]
    code = e(f"{tag}_code").clone().requires_grad_(True)
    loss = lp.correlation_loss(e(f"{tag}_feats"), code, _edge_neg(tag), e(f"{tag}_rand1") * 2 - 1, e(f"{tag}_rand2") * 2 - 1,
                               lp.CorrParams(*APP, feature_samples=S))
    loss.backward()
    want = EDGE[f"{tag}_loss"][0]
    assert abs(loss.item() - want) <= 1e-6 * abs(want)
    g = EDGE[f"{tag}_grad"]
    assert np.abs(code.grad.numpy() - g).max() <= 1e-6 * np.abs(g).max()


@pytest.mark.parametrize("tag", EDGE_GEO)
def test_geo_correlation_loss_port_at_edge_shapes(tag):
    depth = e(f"{tag}_depth").clone()
    B, _, H, W = depth.shape
    code = e(f"{tag}_code").clone().requires_grad_(True)
    ray_o = e(f"{tag}_ray_o")[:, :, None, None].expand(B, 3, H, W)
    loss = lp.geo_correlation_loss(depth, code, ray_o, e(f"{tag}_ray_d"), _edge_neg(tag), lp.CorrParams(*GEO))
    loss.backward()
    want = EDGE[f"{tag}_loss"][0]
    assert abs(loss.item() - want) <= 1e-6 * abs(want)
    assert np.array_equal(depth.numpy(), EDGE[f"{tag}_depth_after"])
    d0 = EDGE[f"{tag}_depth"]                     # the filter: everything above 15 -> the batch-wide max below 15; 15 itself stays
    assert np.array_equal(EDGE[f"{tag}_depth_after"][d0 > 15], np.full(int((d0 > 15).sum()), d0[d0 < 15].max(), np.float32))
    assert (EDGE[f"{tag}_depth_after"][d0 == 15] == 15).all() and (d0 == 15).any()
    g = EDGE[f"{tag}_grad"]
    assert np.abs(code.grad.numpy() - g).max() <= 1e-6 * np.abs(g).max()


CON = np.load(os.path.join(os.path.dirname(__file__), "golden", "contrastive.npz"))
CON_CASES = sorted(k[:-4] for k in CON.files if k.endswith("_emb"))


@pytest.mark.parametrize("tag", CON_CASES)
def test_contrastive_loss_port(tag):
    """oracle/losses_port.nerf_contrastive vs the real NeRFContrastive (utils/image.py:192-218): bit-identical on CPU
    (goldens from tests/golden/make_goldens_contrastive.py); the b5_d7 case is the reference's own NaN (max + min < 0)."""
    e = torch.from_numpy(CON[f"{tag}_emb"]).clone().requires_grad_(True)
    loss = lp.nerf_contrastive(e)
    loss.backward()
    assert np.array_equal(loss.detach().reshape(1).numpy(), CON[f"{tag}_loss"], equal_nan=True)
    assert np.array_equal(e.grad.numpy(), CON[f"{tag}_grad"], equal_nan=True)

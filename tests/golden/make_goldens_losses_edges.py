#!/usr/bin/env python3
"""Golden vectors for the two correlation losses at the edge shapes losses.npz does not reach: code widths 1, 3 and 4,
non-square and one-pixel-wide maps, feature widths below 2 * kMaxC and odd, feature_samples != 11 up to the S = 32
limit, ragged N = H * W for the geometric loss, batch sizes 1..5, the depth filter with a whole patch beyond max_depth
and values exactly at it, and the negatives drawn by super_perm (sim_matrix = None).  Run in the BUILD CONTAINER only
(needs the reference tree):

    python tests/golden/make_goldens_losses_edges.py

Imports the real reference `utils/image.py` (imageio / lpips stubbed, as in make_goldens_losses.py), injects the same
coordinate draws into the reference class and into oracle/losses_port.py, seeds torch's global generator before each
reference call so that super_perm's randperm is recorded (`{tag}_perm`, and `{tag}_neg` the index it becomes), asserts
the port reproduces loss, gradient and filtered depth, and writes tests/golden/losses_edges.npz.  Only data is written.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("NERF_SOS_REFERENCE", "/root/reference")

sys.modules["imageio"] = types.ModuleType("imageio")
_lp = types.ModuleType("lpips")
_lp.LPIPS = lambda *a, **k: None
sys.modules["lpips"] = _lp
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

import utils.image as ref_image  # noqa: E402  (reference)
from oracle import losses_port as lp  # noqa: E402

APP, GEO = (0.18, 1, 0.46, 1), (0.5, 1, 3, 1)       # the recipe's parameters, as losses.npz

# tag: (B, C, code H, code W, Cf, feature H, feature W, S, with sim_matrix)
APP_CASES = {
    "app_c1_13x20": (3, 1, 13, 20, 7, 7, 3, 11, True),
    "app_c3_h1": (2, 3, 1, 16, 3, 5, 4, 7, True),
    "app_c4_w1": (4, 4, 20, 1, 97, 6, 5, 32, False),
    "app_c3_perm": (5, 3, 9, 14, 16, 4, 7, 5, False),
    "app_c2_cf7": (1, 2, 11, 6, 7, 1, 9, 3, False),
}
# tag: (B, C, H, W, with sim_matrix)
GEO_CASES = {
    "geo_c1_9x11": (2, 1, 9, 11, True),
    "geo_c3_13x17": (5, 3, 13, 17, False),
    "geo_c4_20x20": (1, 4, 20, 20, False),
    "geo_c3_1x70": (2, 3, 1, 70, True),
    "geo_c2_33x5": (3, 2, 33, 5, False),
}


def np32(t):
    return t.detach().cpu().numpy()


def ref_args():
    a = types.SimpleNamespace()
    a.rand_neg, a.self_corr_w, a.use_sim_matrix, a.patch_stride = False, 0, True, 6
    a.app_corr_params = [str(x) for x in APP]
    a.geo_corr_params = [str(x) for x in GEO]
    return a


class InjectRand:
    """Replace torch.rand by a queue of prepared tensors (the reference draws coords1 then coords2)."""

    def __init__(self, *tensors):
        self.q = list(tensors)

    def __enter__(self):
        self._rand = torch.rand
        torch.rand = lambda *a, **k: self.q.pop(0)
        return self

    def __exit__(self, *exc):
        torch.rand = self._rand


def negatives(seed, B, sim):
    """(perm, neg): with sim the column arg-min; without, the randperm super_perm draws after manual_seed(seed)."""
    if sim is not None:
        return np.zeros(0, np.int64), lp.neg_index(sim)
    torch.manual_seed(seed)
    perm = torch.randperm(B, dtype=torch.long)
    return np32(perm), lp.super_perm(perm)


def main():
    out = {}
    g = torch.Generator().manual_seed(4242)
    args = ref_args()

    for k, (tag, (B, C, Hc, Wc, Cf, Hf, Wf, S, with_sim)) in enumerate(APP_CASES.items()):
        feats = torch.randn(B, Cf, Hf, Wf, generator=g)
        code = (torch.randn(B, C, Hc, Wc, generator=g) * 2).requires_grad_(True)
        sim = torch.rand(B, B, generator=g) if with_sim else None
        c1 = torch.rand(B, S, S, 2, generator=g)
        c2 = torch.rand(B, S, S, 2, generator=g)
        c1[0, 0, 0] = torch.tensor([0.0, 1.0 - 2 ** -24])   # the lowest and the highest draw torch.rand can make
        seed = 100 + k
        perm, neg = negatives(seed, B, sim)
        mod = ref_image.CorrelationLoss(args)
        mod.feature_samples = S
        torch.manual_seed(seed)
        with InjectRand(c1.clone(), c2.clone()):
            loss = mod(feats, code, sim)
        loss.backward()
        gref = code.grad.clone()
        code2 = code.detach().clone().requires_grad_(True)
        mine = lp.correlation_loss(feats, code2, neg, c1 * 2 - 1, c2 * 2 - 1, lp.CorrParams(*APP, feature_samples=S))
        mine.backward()
        assert torch.equal(mine, loss), (tag, float(mine), float(loss))
        gerr = float((code2.grad - gref).abs().max() / gref.abs().max().clamp_min(1e-30))
        assert gerr < 1e-6, (tag, gerr)
        out.update({f"{tag}_feats": np32(feats), f"{tag}_code": np32(code), f"{tag}_rand1": np32(c1), f"{tag}_rand2": np32(c2),
                    f"{tag}_perm": perm, f"{tag}_neg": np32(neg), f"{tag}_loss": np32(loss.reshape(1)), f"{tag}_grad": np32(gref)})
        if sim is not None:
            out[f"{tag}_sim"] = np32(sim)
        print(tag, float(loss.detach()), float(gref.abs().max()), "grad port-vs-ref rel err", gerr)

    for k, (tag, (B, C, H, W, with_sim)) in enumerate(GEO_CASES.items()):
        depth = 2.0 + 9.0 * torch.rand(B, 1, H, W, generator=g)
        depth[0, 0, 0, :2] = 15.0                                  # exactly max_depth: untouched, and not the replacement
        depth[B - 1, 0, H - 1, W - 1] = 1e10                       # an empty ray (models/renderer.py:72)
        if B >= 3:
            depth[1] = 15.0 + 40.0 * torch.rand(1, H, W, generator=g)   # a whole patch beyond max_depth ...
            depth[1, 0, 0, 0] = 15.0                               # ... but for one value exactly at it
        code = (torch.randn(B, C, H, W, generator=g) * 2).requires_grad_(True)
        if W >= 3:
            code.data[0, :, 0, 2] = code.data[0, :, 0, 1]          # two equal codes: |dc| = 0 off the diagonal
        ray_o = torch.randn(B, 3, 1, 1, generator=g).expand(B, 3, H, W).contiguous() * 0.3
        ray_d = torch.randn(B, 3, H, W, generator=g) * 0.2
        ray_d[:, 2] -= 1.0
        sim = torch.rand(B, B, generator=g) if with_sim else None
        seed = 200 + k
        perm, neg = negatives(seed, B, sim)
        mod = ref_image.GeoCorrelationLoss(args)
        d_ref = depth.clone()
        torch.manual_seed(seed)
        loss = mod(d_ref, code, [ray_o, ray_d, None], sim)
        loss.backward()
        gref = code.grad.clone()
        code2 = code.detach().clone().requires_grad_(True)
        d_mine = depth.clone()
        mine = lp.geo_correlation_loss(d_mine, code2, ray_o, ray_d, neg, lp.CorrParams(*GEO))
        mine.backward()
        assert torch.equal(mine, loss), (tag, float(mine), float(loss))
        scale = float(gref.abs().max())
        gerr = float((code2.grad - gref).abs().max()) / scale if scale > 0 else float((code2.grad - gref).abs().max())
        assert gerr < 1e-6 and torch.equal(d_mine, d_ref), (tag, gerr)
        below = depth[depth < 15.0].max()
        assert torch.equal(d_ref[depth > 15.0], below.expand(int((depth > 15.0).sum()))) and (d_ref[depth == 15.0] == 15.0).all()
        out.update({f"{tag}_depth": np32(depth), f"{tag}_code": np32(code), f"{tag}_ray_o": np32(ray_o[:, :, 0, 0]),
                    f"{tag}_ray_d": np32(ray_d), f"{tag}_perm": perm, f"{tag}_neg": np32(neg), f"{tag}_loss": np32(loss.reshape(1)),
                    f"{tag}_grad": np32(gref), f"{tag}_depth_after": np32(d_ref)})
        if sim is not None:
            out[f"{tag}_sim"] = np32(sim)
        print(tag, float(loss.detach()), scale, "grad port-vs-ref err", gerr)

    path = os.path.join(HERE, "losses_edges.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1e3:.1f} kB")


if __name__ == "__main__":
    main()

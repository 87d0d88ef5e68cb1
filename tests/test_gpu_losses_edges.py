"""GPU: the correlation-loss kernels (csrc/losses.hip) at the shapes tests/test_gpu_losses.py does not reach -- code widths
1, 3 and 4, ragged N = H W, non-square and one-pixel maps, feature widths below 2 * kMaxC, feature_samples up to the S = 32
limit, super_perm negatives, both workgroup shapes of the geometric loss -- against

  (a) goldens captured from the real reference classes (tests/golden/make_goldens_losses_edges.py), at the existing bar;
  (b) a seeded sweep against oracle/losses_port.py run in float64 on the same inputs and the module's exact draws.  The bar
      comes from the port: e32 = the float32 port's error against the float64 port; the kernel's error must be at most
      max(4 e32, 1e-6 scale).  An indexing or tail bug is far above that; the summation-order noise of a kernel that
      accumulates in fp64 is far below it.

Kinks.  The appearance loss clamps cd = <c_p, c_q> at 0; the geometric loss caps 1/(L1 + 0.05) at max_depth for fd and for
cd, and differentiates |c_p - c_q| per channel (sign kink at 0).  A pair within rounding of a kink may land on either side
in fp32, so the sweep moves its inputs off them: sample coordinates (appearance) or per-pixel codes / depths (geometric)
of the row point of every pair closer than MARGIN (KINK_SIGN for the per-channel sign kink, see there) are re-drawn until
none is left, and the test asserts the final distances.  Exact zeros stay: self pairs and equal codes (|dc| = 0, always
capped; a 1 x 1 map has nothing else), C = 1 (the normalised code is +-1, the gradient through the normalisation is zero) and
code pixels no sample reads must come out exactly zero.
"""
import json
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nerf_sos_amd
from oracle import losses_port as lp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EDGE = np.load(os.path.join(os.path.dirname(__file__), "golden", "losses_edges.npz"))
EDGE_APP = sorted(k[:-6] for k in EDGE.files if k.endswith("_feats"))
EDGE_GEO = sorted(k[:-6] for k in EDGE.files if k.endswith("_depth"))
APP, GEO = (0.18, 1, 0.46, 1), (0.5, 1, 3, 1)
MAX_DEPTH = 15.0
CAP = 1.0 / MAX_DEPTH - 0.05          # L1 below which 1 / (L1 + 0.05) is capped at max_depth
MARGIN = 1e-4                          # distance kept from the clamp at 0 and from the two caps
KINK_SIGN = 2e-6                       # from |dc_k| = 0: 4x the largest fp32 discrepancy of a difference of two normalised components
                                       # (2 x 4 ulp of 1); at 1e-4 a 4096-point patch has ~20 such pairs per pixel: no re-draw converges
REDRAWS = 100


def T(a):
    return torch.from_numpy(np.asarray(a)).to(DEV)


def ref_args(rand_neg=False):
    a = types.SimpleNamespace()
    a.rand_neg, a.self_corr_w, a.use_sim_matrix, a.patch_stride = rand_neg, 0, True, 6
    a.app_corr_params = [str(x) for x in APP]
    a.geo_corr_params = [str(x) for x in GEO]
    return a


class Inject:
    """torch.rand / torch.randperm replaced by queues of prepared tensors (the module's draws: rand1, rand2, permutation)."""

    def __init__(self, rand=(), perm=()):
        self.rand, self.perm = [T(a) for a in rand], [T(a) for a in perm]

    def __enter__(self):
        self._rand, self._perm = torch.rand, torch.randperm
        torch.rand = lambda *a, **k: self.rand.pop(0)
        torch.randperm = lambda *a, **k: self.perm.pop(0)

    def __exit__(self, *exc):
        torch.rand, torch.randperm = self._rand, self._perm
        assert exc[0] is not None or (not self.rand and not self.perm), "a prepared draw was not consumed"


def log(record):
    """One JSON line per checked case to $NSOS_LOSS_SWEEP_LOG (if set): the measured error ratios."""
    path = os.environ.get("NSOS_LOSS_SWEEP_LOG")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps(record) + "\n")


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def geo_shape(B, N):
    """The launcher's pick (run_pair_passes): 32-row workgroups while ceil(N/64) * B * 2 < CUs."""
    return "narrow" if math.ceil(N / 64) * B * 2 < cus() else "wide"


# ---------------------------------------------------------------------------------------------------------------- (a) goldens
def _edge_sim_perm(tag):
    sim = T(EDGE[f"{tag}_sim"]) if f"{tag}_sim" in EDGE.files else None
    return sim, ([] if sim is not None else [EDGE[f"{tag}_perm"]])


def _check_grad_at_the_existing_bar(got, want, C):
    got = got.detach().cpu().numpy()
    if C == 1:       # exact zero in the kernel; the reference's fp32 rounding of it is all the golden holds
        assert (got == 0).all() and np.abs(want).max() < 1e-7
        return
    assert np.abs(got - want).max() < 1e-4 * np.abs(want).max()


@pytest.mark.parametrize("tag", EDGE_APP)
def test_correlation_loss_edge_golden(tag):
    mod = nerf_sos_amd.CorrelationLoss(ref_args())
    mod.feature_samples = EDGE[f"{tag}_rand1"].shape[1]
    feats, code0 = T(EDGE[f"{tag}_feats"]), T(EDGE[f"{tag}_code"])
    sim, perm = _edge_sim_perm(tag)
    runs = []
    for _ in range(2):
        code = code0.clone().requires_grad_(True)
        with Inject([EDGE[f"{tag}_rand1"], EDGE[f"{tag}_rand2"]], perm):
            loss = mod(feats, code, sim)
        loss.backward()
        runs.append((loss.detach(), code.grad))
    want = EDGE[f"{tag}_loss"][0]
    assert abs(runs[0][0].item() - want) < 1e-4 * (1 + abs(want)), (runs[0][0].item(), want)
    _check_grad_at_the_existing_bar(runs[0][1], EDGE[f"{tag}_grad"], code0.shape[1])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("tag", EDGE_GEO)
def test_geo_correlation_loss_edge_golden(tag):
    mod = nerf_sos_amd.GeoCorrelationLoss(ref_args())
    d0 = T(EDGE[f"{tag}_depth"])
    B, _, H, W = d0.shape
    ray_o = T(EDGE[f"{tag}_ray_o"])[:, :, None, None].expand(B, 3, H, W)
    ray_d = T(EDGE[f"{tag}_ray_d"])
    sim, perm = _edge_sim_perm(tag)
    runs = []
    for _ in range(2):
        depth = d0.clone()
        code = T(EDGE[f"{tag}_code"]).requires_grad_(True)
        with Inject(perm=perm):
            loss = mod(depth, code, [ray_o, ray_d, None], sim)
        loss.backward()
        assert np.array_equal(depth.cpu().numpy(), EDGE[f"{tag}_depth_after"])      # the in-place filter, exact
        runs.append((loss.detach(), code.grad))
    want = EDGE[f"{tag}_loss"][0]
    assert abs(runs[0][0].item() - want) < 1e-4 * (1 + abs(want)), (runs[0][0].item(), want)
    _check_grad_at_the_existing_bar(runs[0][1], EDGE[f"{tag}_grad"], code.shape[1])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---------------------------------------------------------------------------------------------------------------- (b)-(d) sweep
def _app_cases():
    rng = np.random.default_rng(2026)
    edges = [dict(S=32, B=6), dict(S=1), dict(Cf=1), dict(Hc=1), dict(Wc=1), dict(Cf=3, S=32), dict(Cf=7), dict(Cf=400),
             dict(Hf=1, Wf=1), dict(Hc=1, Wc=1), dict(Cf=97, Hc=13, Wc=20, Hf=7, Wf=3), dict(S=2, B=1)]
    cases = []
    for i in range(20):
        c = dict(C=1 + i % 4, B=int(rng.integers(1, 7)), Hc=int(rng.integers(1, 65)), Wc=int(rng.integers(1, 65)),
                 Cf=int(rng.integers(1, 401)), Hf=int(rng.integers(1, 25)), Wf=int(rng.integers(1, 25)), S=int(rng.integers(1, 33)),
                 sim=bool(i % 3), seed=i)
        c.update(edges[i] if i < len(edges) else {})
        cases.append(c)
    return cases


APP_SWEEP = _app_cases()


def _app_inputs(c):
    g = torch.Generator(DEV).manual_seed(5000 + c["seed"])
    B, C, S = c["B"], c["C"], c["S"]
    feats = torch.randn(B, c["Cf"], c["Hf"], c["Wf"], device=DEV, generator=g)
    code = 2 * torch.randn(B, C, c["Hc"], c["Wc"], device=DEV, generator=g)
    sim = torch.rand(B, B, device=DEV, generator=g) if c["sim"] else None
    neg = lp.neg_index(sim) if sim is not None else lp.super_perm(torch.randperm(B, device=DEV, generator=g))
    r1 = torch.rand(B, S, S, 2, device=DEV, generator=g)
    r2 = torch.rand(B, S, S, 2, device=DEV, generator=g)
    # off the clamp of cd at 0: re-draw the sample coordinates of every pair closer to it than MARGIN (in fp64)
    c64 = code.double()
    for it in range(REDRAWS + 1):
        a = lp._norm(lp._sample(c64, (r1 * 2 - 1).double()))                       # [B,C,S,S]: output (h,w) <- rand[:, w, h]
        b = lp._norm(lp._sample(c64[neg], (r2 * 2 - 1).double()))
        cd_neg, cd_self = lp._dot_correlation(a, b).abs(), lp._dot_correlation(a, a).abs()     # [B,S,S,S,S]
        bad = ((cd_neg < MARGIN) | (cd_self < MARGIN)).flatten(3).any(-1)          # row samples (h,w) with a pair near the clamp
        if not bad.any() or it == REDRAWS:
            break
        m = bad.transpose(1, 2)
        r1[m] = torch.rand(int(m.sum()), 2, device=DEV, generator=g)
    dist = min(float(cd_neg.min()), float(cd_self.min()))
    assert dist >= MARGIN, ("pairs left within MARGIN of the clamp", dist)
    return feats, code, sim, neg, r1, r2, dist


def _footprint_zero(code, neg, r1, r2):
    """Code pixels that no sample of either side reads with a nonzero bilinear weight (fp64: a weight that is zero in fp64 is
    zero in the kernel's fp32 as well -- the pixel coordinate r (W - 1) is then an exact integer)."""
    ones = torch.ones_like(code, dtype=torch.float64).requires_grad_(True)
    (lp._sample(ones, (r1 * 2 - 1).double()).sum() + lp._sample(ones[neg], (r2 * 2 - 1).double()).sum()).backward()
    return ones.grad == 0


def _port_app(feats, code, neg, r1, r2, dtype):
    c = code.to(dtype).clone().requires_grad_(True)
    loss = lp.correlation_loss(feats.to(dtype), c, neg, (r1 * 2 - 1).to(dtype), (r2 * 2 - 1).to(dtype), lp.CorrParams(*APP))
    loss.backward()
    return loss.detach(), c.grad


def _bar(name, hip_l, hip_g, p64, p32, C, record, structural_zero=None):
    """HIP within max(4 e32, 1e-6 scale) of the fp64 port for the loss and the gradient; exact zeros where the gradient is zero
    by structure (`structural_zero`: code pixels no sample reads; C = 1: everywhere)."""
    (l64, g64), (l32, g32) = p64, p32
    hip_l, hip_g = hip_l.double(), hip_g.double()
    for q, hip, v64, v32 in (("loss", hip_l, l64, l32), ("grad", hip_g, g64, g32)):
        e32 = float((v32.double() - v64).abs().max())
        err = float((hip - v64).abs().max())
        scale = float(v64.abs().max())
        bar = max(4 * e32, 1e-6 * scale)
        record[f"{name}_{q}_e32"], record[f"{name}_{q}_ratio"] = e32, (err / e32 if e32 > 0 else (0.0 if err == 0 else math.inf))
        assert err <= bar, (name, q, "hip err", err, "e32", e32, "scale", scale)
    if structural_zero is not None and bool(structural_zero.any()):
        assert float(g64[structural_zero].abs().max()) == 0.0
        assert float(hip_g[structural_zero].abs().max()) == 0.0, (name, "gradient on a pixel no sample reads")
    if C == 1:                                   # normalised code +-1: the gradient is zero (the port's to rounding, the kernel's exactly)
        assert float(g64.abs().max()) < 1e-12 and float(hip_g.abs().max()) == 0.0


@pytest.mark.parametrize("case", APP_SWEEP, ids=lambda c: "C{C}_B{B}_{Hc}x{Wc}_Cf{Cf}_{Hf}x{Wf}_S{S}_{s}".format(
    s="sim" if c["sim"] else "perm", **c))
def test_correlation_loss_sweep_vs_fp64_port(case):
    feats, code, sim, neg, r1, r2, dist = _app_inputs(case)
    mod = nerf_sos_amd.CorrelationLoss(ref_args())
    mod.feature_samples = case["S"]
    # the module draws super_perm's randperm itself: hand it `neg` (super_perm(neg) == neg: no fixed point, or B = 1)
    perm = [] if sim is not None else [neg.cpu().numpy()]
    c = code.clone().requires_grad_(True)
    with Inject([r1.cpu().numpy(), r2.cpu().numpy()], perm):
        loss = mod(feats, c, sim)
    loss.backward()
    p64 = _port_app(feats, code, neg, r1, r2, torch.float64)
    p32 = _port_app(feats, code, neg, r1, r2, torch.float32)
    rec = dict(kind="app", **case, clamp_margin=dist)
    off = _footprint_zero(code, neg, r1, r2)
    rec["pixels_off_footprint"] = int(off.sum())
    _bar("hip", loss.detach(), c.grad, p64, p32, case["C"], rec, off)
    log(rec)


# geometric sweep: (C, B, H, W, with sim_matrix, the shape the launcher must pick unforced on a 256-CU MI355X; None: not asserted)
GEO_SWEEP = [
    (1, 2, 8, 8, True, "narrow"), (1, 3, 9, 11, False, "narrow"), (1, 3, 60, 50, True, "wide"), (1, 1, 1, 1, False, "narrow"),
    (2, 1, 16, 12, True, "narrow"), (2, 5, 13, 17, False, "narrow"), (2, 6, 32, 44, True, "wide"),
    (3, 2, 4, 32, False, "narrow"), (3, 4, 20, 20, True, "narrow"), (3, 3, 50, 60, False, "wide"),
    (4, 1, 32, 128, True, "narrow"), (4, 6, 1, 37, False, "narrow"), (4, 2, 64, 64, False, "wide"), (4, 3, 47, 60, True, "wide"),
]


def _geo_random_cases():
    rng = np.random.default_rng(77)
    out = []
    while len(out) < 5:
        C, B, H, W = int(rng.integers(1, 5)), int(rng.integers(1, 7)), int(rng.integers(1, 65)), int(rng.integers(1, 65))
        if B * (H * W) ** 2 <= 3e7 and H * W <= 1024:
            out.append((C, B, H, W, bool(rng.integers(0, 2)), None))
    return out


GEO_SWEEP += _geo_random_cases()


def _geo_port(depth, code, ray_o, ray_d, neg, dtype):
    c = code.to(dtype).clone().requires_grad_(True)
    d = depth.to(dtype).clone()
    loss = lp.geo_correlation_loss(d, c, ray_o.to(dtype), ray_d.to(dtype), neg, lp.CorrParams(*GEO))
    loss.backward()
    return loss.detach(), c.grad


def _geo_kinks(depth, code, ray_o, ray_d, neg):
    """Per pixel [B,N]: is any of its pairs (as row or column, negative or self set) near a kink -- (fd cap, cd cap or sign) --
    and the smallest distances, all in fp64 on the filtered depth."""
    B, C, H, W = code.shape
    N = H * W
    d = lp.depth_filter_(depth.double().clone(), MAX_DEPTH)
    xyz = (ray_o.double() + ray_d.double() * d).reshape(B, 3, N)
    cn = F.normalize(code.double(), dim=1, eps=1e-10).reshape(B, C, N)
    bad_fd = torch.zeros(B, N, dtype=torch.bool, device=DEV)
    bad_cd = torch.zeros(B, N, dtype=torch.bool, device=DEV)
    dmin = dict(fd_cap=math.inf, cd_cap=math.inf, sign=math.inf)
    for n in range(B):
        for m in (int(neg[n]), n):
            l1x = (xyz[n][:, :, None] - xyz[m][:, None, :]).abs().sum(0)            # [N,N]
            kx = (l1x - CAP).abs()
            fx = kx < MARGIN
            diff = (cn[n][:, :, None] - cn[m][:, None, :]).abs()                      # [C,N,N]
            kc = (diff.sum(0) - CAP).abs()
            live = diff[diff > 0]
            fc = (kc < MARGIN) | ((diff > 0) & (diff < KINK_SIGN)).any(0)
            dmin["fd_cap"] = min(dmin["fd_cap"], float(kx.min()))
            dmin["cd_cap"] = min(dmin["cd_cap"], float(kc.min()))
            if live.numel():
                dmin["sign"] = min(dmin["sign"], float(live.min()))
            bad_fd[n] |= fx.any(1)                           # the row point of each pair is re-drawn
            bad_cd[n] |= fc.any(1)
    return bad_fd, bad_cd, dmin


def _geo_inputs(C, B, H, W, with_sim, seed):
    g = torch.Generator(DEV).manual_seed(9000 + seed)
    N = H * W
    depth = 0.5 + 4.0 * torch.rand(B, 1, H, W, device=DEV, generator=g)
    if N >= 4:
        depth.view(B, -1)[0, 1] = 1e10                      # an empty ray: filtered to the batch-wide max below max_depth
        depth.view(B, -1)[-1, 2] = MAX_DEPTH                # exactly max_depth: kept
    code = 2 * torch.randn(B, C, H, W, device=DEV, generator=g)
    if N >= 2:
        code.view(B, C, -1)[0, :, 1] = code.view(B, C, -1)[0, :, 0]      # equal codes off the diagonal: |dc| = 0, capped
    ray_o = torch.randn(B, 3, device=DEV, generator=g)[:, :, None, None].expand(B, 3, H, W).contiguous()
    ray_d = F.normalize(torch.randn(B, 3, H, W, device=DEV, generator=g), dim=1)
    sim = torch.rand(B, B, device=DEV, generator=g) if with_sim else None
    neg = lp.neg_index(sim) if sim is not None else lp.super_perm(torch.randperm(B, device=DEV, generator=g))
    for it in range(REDRAWS + 1):
        bad_fd, bad_cd, dmin = _geo_kinks(depth, code, ray_o, ray_d, neg)
        if not (bad_fd.any() or bad_cd.any()) or it == REDRAWS:
            break
        dv, cv = depth.view(B, N), code.view(B, C, N)
        dv[bad_fd] = 0.5 + 4.0 * torch.rand(int(bad_fd.sum()), device=DEV, generator=g)
        cv.permute(0, 2, 1)[bad_cd] = 2 * torch.randn(int(bad_cd.sum()), C, device=DEV, generator=g)
    assert dmin["fd_cap"] >= MARGIN and dmin["cd_cap"] >= MARGIN and dmin["sign"] >= KINK_SIGN, dmin
    return depth, code, ray_o, ray_d, sim, neg, dmin


def _geo_run(mod, depth, code, ray_o, ray_d, sim, perm):
    c = code.clone().requires_grad_(True)
    d = depth.clone()
    with Inject(perm=perm):
        loss = mod(d, c, [ray_o, ray_d, None], sim)
    loss.backward()
    return loss.detach(), c.grad, d


@pytest.mark.parametrize("case", GEO_SWEEP, ids=lambda c: "C{}_B{}_{}x{}_{}_{}".format(c[0], c[1], c[2], c[3], "sim" if c[4] else "perm",
                                                                                    c[5] or "any"))
def test_geo_correlation_loss_sweep_vs_fp64_port_in_every_shape(case, monkeypatch):
    C, B, H, W, with_sim, want_shape = case
    N = H * W
    shape = geo_shape(B, N)
    if want_shape is not None:
        assert shape == want_shape, (case, "the launcher's pick on this device", shape, cus())
    depth, code, ray_o, ray_d, sim, neg, dmin = _geo_inputs(C, B, H, W, with_sim, GEO_SWEEP.index(case))
    p64 = _geo_port(depth, code, ray_o, ray_d, neg, torch.float64)
    p32 = _geo_port(depth, code, ray_o, ray_d, neg, torch.float32)
    want_depth = lp.depth_filter_(depth.clone(), MAX_DEPTH)
    mod = nerf_sos_amd.GeoCorrelationLoss(ref_args())
    perm = [] if sim is not None else [neg.cpu().numpy()]       # super_perm(neg) == neg: neg has no fixed point (or B = 1)
    rec = dict(kind="geo", C=C, B=B, H=H, W=W, N=N, sim=with_sim, shape=shape, ragged=N % 64 != 0, **dmin)
    runs = {}
    for mode, env in (("auto_" + shape, {}), ("wide", {"NSOS_GEO_FORCE_WIDE": "1"}),
                      ("wide_separate", {"NSOS_GEO_FORCE_WIDE": "1", "NSOS_GEO_SEPARATE_COLS": "1"})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        loss, grad, d = _geo_run(mod, depth, code, ray_o, ray_d, sim, list(perm))
        assert torch.equal(d, want_depth), mode                       # the filter: batch-wide max below max_depth, exact
        _bar(mode, loss, grad, p64, p32, C, rec)
        runs[mode] = (loss, grad)
    # the fused and the separate column pass share passes 1-2: the same loss bit for bit
    assert torch.equal(runs["wide"][0], runs["wide_separate"][0])
    log(rec)


def test_geo_sweep_covers_both_shapes_at_every_code_width():
    """Every cell of C 1-4 x {narrow, wide, wide-separate} x {N % 64 = 0, ragged}: every case runs forced wide and
    wide-separate; the unforced runs must take the 32-row shape for an aligned and a ragged N at every width, and the
    64-row shape on its own for some."""
    cells = set()
    for C, B, H, W, _, _ in GEO_SWEEP:
        N = H * W
        ragged = N % 64 != 0
        cells |= {(C, "wide", ragged), (C, "wide_separate", ragged), (C, geo_shape(B, N), ragged)}
    assert cells >= {(C, s, r) for C in range(1, 5) for s in ("narrow", "wide", "wide_separate") for r in (False, True)}
    assert {geo_shape(B, H * W) for _, B, H, W, _, _ in GEO_SWEEP} == {"narrow", "wide"}
    assert any(H * W == 4096 and H != W for _, _, H, W, _, _ in GEO_SWEEP) and any(c["S"] == 32 for c in APP_SWEEP)
    assert all(B * (H * W) ** 2 <= 3.5e7 and H * W <= 4096 for _, B, H, W, _, _ in GEO_SWEEP)


# ---------------------------------------------------------------------------------------------------------------- (e) layouts, entries
@pytest.mark.parametrize("C", [3, 1])
def test_appearance_channel_last_and_row_entries_at_a_ragged_non_square_map(C):
    """The renderer's `semantics.permute(0,3,1,2)` view takes the channel-last kernel path: bit-equal to the contiguous one;
    rows_phased over every patch (phases 0, 1, 2 with the exchange buffers) equals the whole-batch entry bit for bit."""
    from nerf_sos_amd.losses import exchange_floats
    B, Hc, Wc, Cf, S = 3, 13, 20, 97, 9
    g = torch.Generator(DEV).manual_seed(31 + C)
    feats = torch.randn(B, Cf, 7, 3, device=DEV, generator=g)
    code = 2 * torch.randn(B, C, Hc, Wc, device=DEV, generator=g)
    sim = torch.rand(B, B, device=DEV, generator=g)
    mod = nerf_sos_amd.CorrelationLoss(ref_args())
    mod.feature_samples = S
    coords = mod.draw_coords(1, B, DEV)[0]
    la, ga = mod.value_and_grad(feats, code, sim, coords=coords)
    nhwc = code.permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    view = nhwc.permute(0, 3, 1, 2)
    assert view.is_contiguous() == (C == 1)     # one channel: [B,P,P,1] is already [B,1,P,P] (the contiguous path)
    mod.queue_coords([coords])
    lb = mod(feats, view, sim)
    lb.backward()
    assert torch.equal(la, lb.detach()) and torch.equal(nhwc.grad.permute(0, 3, 1, 2), ga)
    nx = exchange_floats(B, S * S)
    for x in (code, view.detach()):
        xm, xs = torch.zeros(8, device=DEV, dtype=torch.float64), torch.zeros(nx, device=DEV)
        run, (lo, gr) = mod.rows_phased(feats, x, sim, list(range(B)), (xm, xs), coords=coords)
        for phase in range(3):          # one rank: the reductions between the phases are the identity
            run(phase)
        assert torch.equal(lo, la)
        if x is code:
            assert torch.equal(gr, ga)
        else:                           # (channel-last rows entry: its own scatter order, as in test_gpu_losses.py)
            assert float((gr - ga).abs().max()) <= 1e-6 * max(float(ga.abs().max()), 1e-30)
    if C == 1:
        assert float(ga.abs().max()) == 0.0


@pytest.mark.parametrize("C", [3, 1])
def test_geo_pair_and_row_entries_at_a_ragged_non_square_map(C):
    """forward_pair on the renderer's channel-last tensors equals the stacked row-partitioned evaluation bit for bit (as the
    C = 2 test does), and the row-partitioned entry over every patch meets the whole-batch entry's value and gradient."""
    from nerf_sos_amd import sharding
    B, H, W = 3, 13, 17
    g = torch.Generator(DEV).manual_seed(41 + C)
    depth = 0.5 + 4.0 * torch.rand(B, 1, H, W, device=DEV, generator=g)
    code = 2 * torch.randn(B, C, H, W, device=DEV, generator=g)
    code1 = 2 * torch.randn(B, C, H, W, device=DEV, generator=g)
    ray_o = torch.randn(B, 3, device=DEV, generator=g)[:, :, None, None].expand(B, 3, H, W).contiguous()
    ray_d = F.normalize(torch.randn(B, 3, H, W, device=DEV, generator=g), dim=1)
    sim = torch.rand(B, B, device=DEV, generator=g)
    mod = nerf_sos_amd.GeoCorrelationLoss(ref_args())
    whole = _geo_run(mod, depth, code, ray_o, ray_d, sim, [])
    c = code.clone().requires_grad_(True)
    rows = mod(depth.clone(), c, [ray_o, ray_d, None], sim, rows=list(range(B)))
    rows.backward()
    assert abs(float(rows.detach()) - float(whole[0])) <= 1e-6 * abs(float(whole[0]))
    assert float((c.grad - whole[1]).abs().max()) <= 1e-6 * max(float(whole[1].abs().max()), 1e-30)
    for sub in (list(range(B)), [1]):
        c0, c1 = code.clone().requires_grad_(True), code1.clone().requires_grad_(True)
        want = sharding.geo_loss_both(mod, depth.clone(), c0, c1, ray_o, ray_d, sim, sub)
        want.backward()
        n0 = code.permute(0, 2, 3, 1).contiguous().requires_grad_(True)
        n1 = code1.permute(0, 2, 3, 1).contiguous().requires_grad_(True)
        got = mod.forward_pair(depth.permute(0, 2, 3, 1).contiguous(), n0, n1, ray_o.permute(0, 2, 3, 1).contiguous(),
                               ray_d.permute(0, 2, 3, 1).contiguous(), sim, rows=sub)
        got.backward()
        assert torch.equal(got.detach(), want.detach())
        assert torch.equal(n0.grad.permute(0, 3, 1, 2), c0.grad) and torch.equal(n1.grad.permute(0, 3, 1, 2), c1.grad)
    if C == 1:
        assert float(whole[1].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- (f) limits
def test_out_of_range_shapes_raise_through_the_modules():
    """N > 4096, C outside 1..4 and S > 32 are refused by the entry points (NSOS_ERR_UNSUPPORTED, tests/test_abi.py) and surface
    as a RuntimeError from _lib.check naming the entry; the accepted boundary (N = 4096 on 32 x 128, S = 32) runs in the sweep."""
    geo = nerf_sos_amd.GeoCorrelationLoss(ref_args())
    for B, C, H, W in ((1, 2, 1, 4097), (1, 2, 17, 241), (2, 5, 8, 8)):
        depth = 1.0 + torch.rand(B, 1, H, W, device=DEV)
        rays = [torch.zeros(B, 3, H, W, device=DEV), torch.ones(B, 3, H, W, device=DEV), None]
        with pytest.raises(RuntimeError, match=r"nsos_geo_correlation_loss failed: \[-3\]"):
            geo(depth, torch.randn(B, C, H, W, device=DEV, requires_grad=True), rays, torch.rand(B, B, device=DEV))
    with pytest.raises(RuntimeError, match=r"nsos_geo_correlation_loss failed: \[-"):
        geo(1.0 + torch.rand(2, 1, 8, 8, device=DEV), torch.randn(2, 0, 8, 8, device=DEV), rays, torch.rand(2, 2, device=DEV))
    app = nerf_sos_amd.CorrelationLoss(ref_args())
    feats = torch.randn(2, 7, 5, 3, device=DEV)
    app.feature_samples = 33
    with pytest.raises(RuntimeError, match=r"nsos_app_correlation_loss failed: \[-3\]"):
        app(feats, torch.randn(2, 2, 13, 20, device=DEV), torch.rand(2, 2, device=DEV))
    app.feature_samples = 11
    with pytest.raises(RuntimeError, match=r"nsos_app_correlation_loss failed: \[-3\]"):
        app(feats, torch.randn(2, 5, 13, 20, device=DEV), torch.rand(2, 2, device=DEV))
    with pytest.raises(RuntimeError, match=r"nsos_app_correlation_loss failed: \[-"):
        app(feats, torch.randn(2, 0, 13, 20, device=DEV), torch.rand(2, 2, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- (g) RNG contract
def _expected_draws(make_gen, B, S, app, rand_neg):
    """The reference's order from one generator state: rand1, rand2 (appearance only), then the permutation."""
    gen = make_gen()
    out = {}
    if app:
        out["r1"] = torch.rand([B, S, S, 2], device=DEV, generator=gen)
        out["r2"] = torch.rand([B, S, S, 2], device=DEV, generator=gen)
    perm = torch.randperm(B, device=DEV, dtype=torch.long, generator=gen)
    out["neg"] = perm if rand_neg else lp.super_perm(perm)
    return out


@pytest.mark.parametrize("rand_neg", [False, True], ids=["super_perm", "rand_neg"])
@pytest.mark.parametrize("source", ["global", "module_generator"])
def test_random_draws_follow_the_reference_order(rand_neg, source):
    """sim_matrix=None draws rand1, rand2, then super_perm's randperm; rand_neg=True (with a sim_matrix) rand1, rand2, then
    randperm -- from torch's global generator, or from `module.generator` when set.  The module's loss equals the module fed
    those draws explicitly (bit for bit) and the fp64 port fed them (to fp32 rounding)."""
    B, S, C = 5, 7, 3
    g = torch.Generator(DEV).manual_seed(123)
    feats = torch.randn(B, 9, 6, 5, device=DEV, generator=g)
    code = 2 * torch.randn(B, C, 11, 14, device=DEV, generator=g)
    depth = 0.5 + 4.0 * torch.rand(B, 1, 11, 14, device=DEV, generator=g)
    ray_o = torch.randn(B, 3, device=DEV, generator=g)[:, :, None, None].expand(B, 3, 11, 14).contiguous()
    ray_d = F.normalize(torch.randn(B, 3, 11, 14, device=DEV, generator=g), dim=1)
    sim = torch.rand(B, B, device=DEV, generator=g) if rand_neg else None
    for app in (True, False):
        mod = (nerf_sos_amd.CorrelationLoss if app else nerf_sos_amd.GeoCorrelationLoss)(ref_args(rand_neg))
        mod.feature_samples = S
        if source == "global":
            torch.manual_seed(2024)
            make_gen = lambda: torch.Generator(DEV).manual_seed(2024)   # noqa: E731  (torch.manual_seed seeds cuda:0 alike)
        else:
            mod.generator = torch.Generator(DEV).manual_seed(99)
            make_gen = lambda: torch.Generator(DEV).manual_seed(99)     # noqa: E731
        with torch.no_grad():
            got = mod(feats, code, sim) if app else mod(depth.clone(), code, [ray_o, ray_d, None], sim)
        want = _expected_draws(make_gen, B, S, app, rand_neg)
        if app:
            explicit, _ = mod.value_and_grad(feats, code, sim, neg=want["neg"], coords=(want["r1"], want["r2"]), want_grad=False)
            port = lp.correlation_loss(feats.double(), code.double(), want["neg"], (want["r1"] * 2 - 1).double(),
                                       (want["r2"] * 2 - 1).double(), lp.CorrParams(*APP))
            assert torch.equal(got, explicit), (source, rand_neg)
        else:
            with Inject(perm=[want["neg"].cpu().numpy()]):          # super_perm(neg) == neg; rand_neg uses the draw as it is
                mod.generator = None
                explicit = mod(depth.clone(), code, [ray_o, ray_d, None], sim)
            port = lp.geo_correlation_loss(depth.double().clone(), code.double(), ray_o.double(), ray_d.double(), want["neg"],
                                           lp.CorrParams(*GEO))
            assert torch.equal(got, explicit), (source, rand_neg)
        assert abs(float(got) - float(port)) <= 1e-5 * abs(float(port)), (app, source, rand_neg, float(got), float(port))

"""GPU: SSIM, adjusted Rand index and k-means (nerf_sos_amd.metrics / ops) against the reference's values recorded in
tests/golden/eval_metrics.npz (make_goldens_eval.py: the reference's utils/ssim.py, sklearn 1.x), and the eval_one_view /
i_print metric blocks end to end on the trained field."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import nerf_sos_amd
from nerf_sos_amd import metrics, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def ari_np(t, p):
    """sklearn's pair-confusion ARI in exact integers (test-side port for labels the fixture does not hold)."""
    t, p = np.asarray(t).astype(np.int64), np.asarray(p).astype(np.int64)
    n = t.size
    if n == 0:
        return 1.0
    ct = np.zeros((t.max() + 1, p.max() + 1), np.int64)
    np.add.at(ct, (t, p), 1)
    ss = int((ct.astype(object) ** 2).sum())
    nc, nk = ct.sum(1).astype(object), ct.sum(0).astype(object)
    fp = int((ct.astype(object) * nk[None, :]).sum()) - ss
    fn = int((ct.astype(object) * nc[:, None]).sum()) - ss
    tp, tn = ss - n, n * n - fp - fn - ss
    if fn == 0 and fp == 0:
        return 1.0
    return 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))


# ------------------------------------------------------------------------------------------------------------------ SSIM
def _ssim_case(g, i):
    ws, sa, fmt = (int(v) for v in g[f"ssim{i}_meta"])
    return T(g[f"ssim{i}_img1"]), T(g[f"ssim{i}_img2"]), ws, bool(sa), ["HWC", "NHWC", "NCHW"][fmt]


def test_ssim_matches_fp64_and_the_reference(golden):
    g = golden("eval_metrics")
    for i in range(int(g["ssim_n"][0])):
        a, b, ws, sa, fmt = _ssim_case(g, i)
        got = N(metrics.ssim(a, b, ws, sa, fmt)).astype(np.float64)
        f64, ref = g[f"ssim{i}_fp64"], g[f"ssim{i}_ref"].astype(np.float64)
        assert got.shape == f64.shape, (i, got.shape, f64.shape)
        assert np.abs(got - f64).max() <= 1e-6, (i, got, f64)
        # the reference's own fp32 error (its |ref - fp64|, up to 1.5e-6 on the noisy cases) on top of the 1e-6
        assert np.abs(got - ref).max() <= 1e-6 + np.abs(ref - f64).max(), (i, got, ref)


def test_ssim_map_matches_fp64_conv2d(golden):
    g = golden("eval_metrics")
    for i in range(int(g["ssim_n"][0])):
        a, b, ws, sa, fmt = _ssim_case(g, i)
        if fmt == "HWC":
            a, b = a.permute(2, 0, 1)[None], b.permute(2, 0, 1)[None]
        elif fmt == "NHWC":
            a, b = a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2)
        _, smap = ops.ssim(a.contiguous(), b.contiguous(), ws, sa, return_map=True)
        x, y = a.double().cpu(), b.double().cpu()
        w1 = torch.tensor(list(ops.ssim_window(ws)), dtype=torch.float64)
        C = x.shape[1]
        w = torch.outer(w1, w1)[None, None].expand(C, 1, ws, ws)
        conv = lambda t: F.conv2d(t, w, padding=ws // 2, groups=C)
        m1, m2 = conv(x), conv(y)
        s1, s2, s12 = conv(x * x) - m1 ** 2, conv(y * y) - m2 ** 2, conv(x * y) - m1 * m2
        want = ((2 * m1 * m2 + 1e-4) * (2 * s12 + 9e-4)) / ((m1 ** 2 + m2 ** 2 + 1e-4) * (s1 + s2 + 9e-4))
        assert np.abs(N(smap).astype(np.float64) - want.numpy()).max() <= 1e-4, i


def test_ssim_identity_symmetry_repeatability_and_odd_windows():
    torch.manual_seed(0)
    a = torch.rand(2, 3, 45, 70, device=DEV)
    b = (a + 0.1 * torch.randn_like(a)).clamp(0, 1)
    for ws in (1, 3, 11, 15, 17, 31):
        assert abs(float(ops.ssim(a, a, ws)) - 1.0) <= 1e-6, ws
        ab, ba = ops.ssim(a, b, ws, False), ops.ssim(b, a, ws, False)
        assert torch.equal(ab, ba), ws
    first = ops.ssim(a, b, 11, True, return_map=True)
    for _ in range(3):
        again = ops.ssim(a, b, 11, True, return_map=True)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    big = torch.rand(1, 3, 756, 1008, device=DEV)
    v1, v2 = ops.ssim(big, big * 0.9, 11), ops.ssim(big, big * 0.9, 11)
    assert torch.equal(v1, v2) and 0 < float(v1) < 1


# ------------------------------------------------------------------------------------------------------------------- ARI
def test_ari_matches_sklearn_full_and_fg_from_one_call(golden):
    g = golden("eval_metrics")
    for i in range(int(g["ari_n"][0])):
        t, p, want = g[f"ari{i}_true"], g[f"ari{i}_pred"], g[f"ari{i}_want"]
        got = N(ops.adjusted_rand_score(T(t), T(p)))
        assert np.abs(got - want).max() <= 1e-12, (i, got, want)
        assert np.array_equal(got == 1.0, want == 1.0), (i, got, want)   # sklearn's special case: exactly 1.0
        assert float(metrics.adjusted_rand_score(T(t), T(p))) == got[0]


def test_ari_input_types_and_special_cases():
    rng = np.random.default_rng(1)
    t, p = rng.integers(0, 6, 20000), rng.integers(0, 6, 20000)
    p[:9000] = t[:9000]
    want = ari_np(t, p)
    for dt in (torch.int32, torch.int64, torch.uint8, torch.float32):
        got = ops.adjusted_rand_score(torch.as_tensor(t).to(DEV, dt), torch.as_tensor(p).to(DEV, dt))
        assert abs(float(got[0]) - want) <= 1e-12, dt
    bt, bp = t < 3, p < 3
    assert abs(float(ops.adjusted_rand_score(T(bt), T(bp))[0]) - ari_np(bt, bp)) <= 1e-12
    for n in (0, 1):
        z = torch.zeros(n, dtype=torch.int32, device=DEV)
        assert N(ops.adjusted_rand_score(z, z)).tolist() == [1.0, 1.0]
    one = torch.zeros(50, dtype=torch.int32, device=DEV)
    assert float(ops.adjusted_rand_score(one, one + 3)[0]) == 1.0
    # labels beyond 4 take the LDS-atomic path; 63 is the largest accepted
    t2, p2 = rng.integers(0, 64, 30000), rng.integers(0, 64, 30000)
    assert abs(float(ops.adjusted_rand_score(T(t2.astype(np.int32)), T(p2.astype(np.int32)))[0]) - ari_np(t2, p2)) <= 1e-12


def test_ari_invalid_labels_give_nan():
    ok = torch.tensor([0, 1, 1, 0], dtype=torch.float32, device=DEV)
    for bad in (0.5, -1.0, 64.0, float("nan")):
        lab = ok.clone()
        lab[2] = bad
        assert torch.isnan(ops.adjusted_rand_score(lab, ok)).all(), bad
        assert torch.isnan(ops.adjusted_rand_score(ok, lab)).all(), bad
    big = torch.tensor([0, 1, 70, 0], dtype=torch.int64, device=DEV)
    assert torch.isnan(ops.adjusted_rand_score(big, big)).all()


def test_ari_full_image_size_exact():
    rng = np.random.default_rng(2)
    n = 1008 * 756
    t = (rng.random(n) < 0.3).astype(np.int32)
    p = np.where(rng.random(n) < 0.9, t, 1 - t).astype(np.int32)
    got = N(ops.adjusted_rand_score(T(t), T(p)))
    assert abs(got[0] - ari_np(t, p)) <= 1e-12
    fg = t == 1
    assert abs(got[1] - ari_np(t[fg], p[fg])) <= 1e-12


# ------------------------------------------------------------------------------------------------------------------ k-means
def _trained_sem(golden):
    g = golden("trained_img64k")
    return torch.from_numpy(g["eval_semantics"]).float().softmax(-1), g["gt_label"].astype(np.int32)


def _same_partition_except_ties(got, want, x, centers):
    """labels equal up to a permutation, except where the two nearest centers are within 1e-6 relative"""
    x, c = x.astype(np.float64), centers.astype(np.float64)
    d = ((x[:, None, :] - c[None]) ** 2).sum(-1)
    ds = np.sort(d, 1)
    tie = (ds[:, 1] - ds[:, 0]) <= 1e-6 * np.maximum(ds[:, 1], 1e-30)
    K = c.shape[0]
    m = np.zeros((K, K), np.int64)
    np.add.at(m, (want[~tie], got[~tie]), 1)
    perm = m.argmax(1)
    return len(set(perm.tolist())) == len(perm) and np.array_equal(perm[want[~tie]], got[~tie])


def test_kmeans_pinned_init_follows_sklearn(golden):
    g = golden("eval_metrics")
    sem, _ = _trained_sem(golden)
    for i in range(int(g["km_n"][0])):
        x = g[f"km{i}_x"] if f"km{i}_x" in g else sem.numpy()
        init = g[f"km{i}_init"]
        for mode in ("workgroup", "grid"):
            r = ops.kmeans(T(x), init.shape[0], init=T(init), mode=mode)
            assert int(r["n_iter"]) == int(g[f"km{i}_n_iter"][0]), (i, mode, int(r["n_iter"]), g[f"km{i}_n_iter"])
            assert abs(float(r["inertia"]) / float(g[f"km{i}_inertia"][0]) - 1) <= 1e-5, (i, mode)
            assert _same_partition_except_ties(N(r["labels"]), g[f"km{i}_labels"].astype(np.int64), x, N(r["centers"])), (i, mode)


def test_kmeans_seeded_on_trained_semantics_is_inside_sklearn_seed_range(golden):
    g = golden("eval_metrics")
    sem, gt = _trained_sem(golden)
    spread = g["seed_spread"]
    for j, feats in enumerate((sem, torch.from_numpy(golden("trained_img64k")["eval_semantics"]).float())):
        r = ops.kmeans(feats.to(DEV), 2, seed=0)
        assert float(r["inertia"]) <= spread[j, :, 0].max() * (1 + 1e-6), (j, float(r["inertia"]), spread[j, :, 0])
        a = ari_np(gt, N(r["labels"]))
        assert spread[j, :, 1].min() - 0.005 <= a <= spread[j, :, 1].max() + 0.005, (j, a, spread[j, :, 1])


def test_kmeans_recovers_separated_mixtures():
    rng = np.random.default_rng(3)
    for K, C in ((3, 2), (4, 5), (5, 8), (3, 8)):
        cent = rng.normal(0, 1, (K, C)) * 20
        lab = rng.integers(0, K, 3000)
        x = (cent[lab] + rng.normal(0, 0.5, (3000, C))).astype(np.float32)
        r = ops.kmeans(T(x), K, seed=5, n_init=2)
        assert ari_np(lab, N(r["labels"])) == 1.0, (K, C)


def test_kmeans_batching_regimes_determinism_and_canonical_order(golden):
    sem, _ = _trained_sem(golden)
    x = sem[: 8 * 4096].reshape(8, 4096, 2).to(DEV).contiguous()
    batch = ops.kmeans(x, 2, seed=7)
    for b in range(8):
        single = ops.kmeans(x[b], 2, seed=7, problem_offset=b)
        for k in ("labels", "centers", "inertia", "n_iter"):
            assert torch.equal(batch[k][b], single[k]), (b, k)
    again = ops.kmeans(x, 2, seed=7)
    for k in batch:
        assert torch.equal(batch[k], again[k]), k
    c = N(batch["centers"])
    for b in range(8):
        assert [tuple(v) for v in c[b]] == sorted(tuple(v) for v in c[b]), b
    # the grid regime and the workgroup regime: bitwise-equal results
    for xx, K in ((x, 2), (torch.randn(3, 5000, 4, device=DEV), 5)):
        wg, gr = ops.kmeans(xx, K, seed=1, mode="workgroup"), ops.kmeans(xx, K, seed=1, mode="grid")
        for k in wg:
            assert torch.equal(wg[k], gr[k]), k
    full = sem.to(DEV)
    f1, f2 = ops.kmeans(full, 2, seed=0), ops.kmeans(full, 2, seed=0, mode="grid")
    for k in f1:
        assert torch.equal(f1[k], f2[k]), k


def test_kmeans_empty_cluster_relocation():
    # 13 points: 10 at the origin, 3 far away; every initial center sits among the origin points -> two clusters come out empty
    x = torch.zeros(13, 2, device=DEV)
    x[10:] = torch.tensor([[10.0, 0.0], [0.0, 12.0], [9.0, 9.0]], device=DEV)
    init = torch.tensor([[0.0, 0.0], [-0.5, 0.0], [0.0, -0.5]], device=DEV)
    for mode in ("workgroup", "grid"):
        r = ops.kmeans(x, 3, init=init, mode=mode)
        assert len(set(N(r["labels"]).tolist())) == 3, mode
        assert float(r["inertia"]) < 100.0, mode


def _chi2_p(obs, p):
    """upper tail of Pearson's chi^2 (Wilson-Hilferty normal approximation)"""
    from math import erfc, sqrt
    exp = p * obs.sum()
    keep = exp > 0
    stat = float(((obs[keep] - exp[keep]) ** 2 / exp[keep]).sum())
    dof = int(keep.sum()) - 1
    z = ((stat / dof) ** (1 / 3) - (1 - 2 / (9 * dof))) / np.sqrt(2 / (9 * dof))
    return 0.5 * erfc(z / sqrt(2))


def test_kmeans_seeding_frequencies_pass_chi2():
    """2 000 copies of one 16-point problem in one launch (problem ids 0..1999: per-problem streams), seeding only (max_iter=0,
    seeds in draw order) with one local trial: the first center is uniform, the second is drawn with probability D^2 / sum D^2."""
    rng = np.random.default_rng(4)
    pts = rng.normal(0, 1, (16, 2)).astype(np.float32)
    B = 2000
    r = ops.kmeans(T(np.broadcast_to(pts, (B, 16, 2))), 2, seed=11, n_local_trials=1, max_iter=0)
    c = N(r["centers"])
    idx = np.array([[int(np.flatnonzero((pts == v).all(1))[0]) for v in cs] for cs in c])
    assert (N(r["n_iter"]) == 0).all()
    obs0 = np.bincount(idx[:, 0], minlength=16).astype(np.float64)
    assert _chi2_p(obs0, np.full(16, 1 / 16)) > 1e-3, obs0
    exp = np.zeros(16)
    for a in range(16):
        d2 = ((pts.astype(np.float64) - pts[a]) ** 2).sum(1)
        exp += obs0[a] * d2 / d2.sum()
    obs1 = np.bincount(idx[:, 1], minlength=16).astype(np.float64)
    assert _chi2_p(obs1, exp / exp.sum()) > 1e-3, (obs1, exp)
    assert (idx[:, 0] != idx[:, 1]).all()


# ------------------------------------------------------------------------------------------------------------- end to end
def _render_trained_img64k(golden):
    import hashlib
    from nerf_sos_amd import synthetic as syn
    g = golden("trained_img64k")
    net = nerf_sos_amd.NeRFNet(N_samples=64, N_importance=128, perturb=1.0, raw_noise_std=1.0, use_semantics=True,
                               sem_with_coord=True).to(DEV)
    nerf_sos_amd.io.load_checkpoint(os.path.join(HERE, "golden", "trained_scene.ckpt"), net)
    net.eval()
    net.chunk = 65536
    scene = syn.ProceduralScene()
    H, W, focal = int(g["image_hwf"][0]), int(g["image_hwf"][1]), float(g["image_hwf"][2])
    full = ops.generate_rays(H, W, syn.intrinsics(H, W, focal), scene.poses[int(g["pose_index"][0]), :3, :4], DEV).reshape(2, -1, 3)
    rays = full[:, T(g["pixel_index"]).long()].contiguous()
    assert hashlib.sha256(N(rays).tobytes()).digest() == bytes(g["rays_sha256"])
    near, far = (float(v) for v in g["near_far"])
    with torch.no_grad():
        out = net(rays, (near, far), radii=None, retraw=False)
    return g, out


def test_view_metrics_on_the_trained_field(golden):
    g, out = _render_trained_img64k(golden)
    em = golden("eval_metrics")
    gt = T(g["gt_label"].astype(np.float32))
    ret = {"rgb": out["rgb"].reshape(256, 256, 3), "semantics": out["semantics"].reshape(256, 256, -1)}
    target = T(g["gt_rgb"]).reshape(256, 256, 3)
    m = metrics.view_metrics(ret, target, gt.reshape(256, 256, 1), N_cluster=2)
    for k in ("mse", "psnr", "ssim", "clus_ari", "clus_ari_fg", "sem_ari", "sem_ari_fg", "sem", "clustering"):
        assert k in m and m[k].is_cuda, k
    want = em["view_sem_ari"]
    assert abs(float(m["sem_ari"]) - want[0]) <= 1e-3 and abs(float(m["sem_ari_fg"]) - want[1]) <= 1e-3, (m["sem_ari"], want)
    spread = em["seed_spread"]
    assert spread[0, :, 1].min() - 0.005 <= float(m["clus_ari"]) <= spread[0, :, 1].max() + 0.005, (float(m["clus_ari"]), spread[0, :, 1])
    # the MSE / PSNR / SSIM of the same render against the ground truth, as the reference defines them
    rgb = N(ret["rgb"]).astype(np.float64)
    assert abs(float(m["mse"]) - np.mean(np.mean((rgb - N(target)) ** 2, -1))) <= 1e-6
    assert abs(float(m["ssim"]) - float(ops.ssim(ret["rgb"].permute(2, 0, 1)[None].contiguous(),
                                                 target.permute(2, 0, 1)[None].contiguous()))) == 0.0
    mr = metrics.view_metrics(ret, target, gt.reshape(256, 256, 1), clus_no_sfm=True)
    assert spread[1, :, 1].min() - 0.005 <= float(mr["clus_ari"]) <= spread[1, :, 1].max() + 0.005


def test_patch_metrics_equal_segmap_cluster_then_pooled_ari(golden):
    g, out = _render_trained_img64k(golden)
    sem = out["semantics"][: 4 * 4096].reshape(4, 64, 64, -1)
    masks = T(g["gt_label"][: 4 * 4096].astype(np.float32)).reshape(4, 64, 64, 1)
    pm = metrics.patch_metrics(sem, masks, N_cluster=2)
    prob = ops.eval_postprocess(sem)["sem_prob"]
    clus = torch.stack([metrics.segmap_cluster(prob[b], 2) for b in range(4)])
    assert torch.equal(clus, pm["clustering"])
    c = ops.adjusted_rand_score(masks.reshape(-1), clus.reshape(-1).float())
    s = ops.adjusted_rand_score(masks.reshape(-1), prob.argmax(-1).reshape(-1).float())
    assert float(pm["clus_ari"]) == float(c[0]) and float(pm["clus_ari_fg"]) == float(c[1])
    assert float(pm["sem_ari"]) == float(s[0]) and float(pm["sem_ari_fg"]) == float(s[1])

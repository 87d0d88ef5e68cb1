"""Writes tests/golden/eval_metrics.npz: SSIM, adjusted Rand index and k-means cases with the reference's own values.
Runs on the build machine only (imports the reference's utils/ssim.py and utils/misc.py, and sklearn); data only.

    python tests/golden/make_goldens_eval.py /path/to/NeRF-SOS
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))


def fp64_ssim(img1, img2, window_size, size_average, g32):
    """_ssim in fp64 with the separable window: the outer product (in fp64) of the fp32-normalised 1-D gaussian."""
    a, b = torch.from_numpy(img1).double(), torch.from_numpy(img2).double()
    g = torch.from_numpy(g32.astype(np.float64))
    C = a.shape[1]
    w = torch.outer(g, g)[None, None].expand(C, 1, window_size, window_size).contiguous()
    pad = window_size // 2
    conv = lambda t: F.conv2d(t, w, padding=pad, groups=C)
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1 ** 2, conv(b * b) - mu2 ** 2, conv(a * b) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 ** 2 + mu2 ** 2 + C1) * (s1 + s2 + C2))
    return (m.mean().reshape(1) if size_average else m.mean((1, 2, 3))).numpy()


def main(ref_root):
    sys.path.insert(0, ref_root)
    from utils import ssim as ref_ssim
    from utils.misc import segmap_cluster  # noqa: F401  (the reference's clustering: KMeans(n_clusters, random_state=0))
    from sklearn.cluster import KMeans, kmeans_plusplus
    from sklearn.metrics import adjusted_rand_score

    rng = np.random.default_rng(20261016)
    out = {}

    # ---- SSIM
    def smooth(shape_nchw):
        N, C, H, W = shape_nchw
        yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
        base = 0.5 + 0.3 * np.sin(5 * xx + 3 * yy)[None, None] * np.linspace(0.6, 1.0, C)[None, :, None, None]
        return np.broadcast_to(base, shape_nchw).astype(np.float32)

    cases = []
    for (N, H, W, C, fmt) in [(1, 37, 53, 3, "HWC"), (1, 5, 7, 3, "HWC"), (1, 11, 11, 1, "NCHW"), (2, 24, 31, 3, "NHWC")]:
        for ws in (11, 7):
            for sa in (True, False):
                for kind in ("noise", "flat"):
                    a = smooth((N, C, H, W))
                    b = (a + rng.normal(0, 0.05, a.shape)).astype(np.float32)
                    if kind == "flat":
                        a = a.copy()
                        b = b.copy()
                        a[..., : H // 2, : W // 2] = 0.25
                        b[..., : H // 2, : W // 2] = 0.25 if H > 6 else 0.75
                    cases.append((a, b, ws, sa, fmt, kind))
    for i, (a, b, ws, sa, fmt, kind) in enumerate(cases):
        g32 = ref_ssim.gaussian(ws, 1.5).numpy()
        ref = ref_ssim.ssim(torch.from_numpy(a), torch.from_numpy(b), ws, sa).reshape(-1).numpy()
        f64 = fp64_ssim(a, b, ws, sa, g32)
        if fmt == "HWC":
            sa_in, sb_in = a[0].transpose(1, 2, 0), b[0].transpose(1, 2, 0)
        elif fmt == "NHWC":
            sa_in, sb_in = a.transpose(0, 2, 3, 1), b.transpose(0, 2, 3, 1)
        else:
            sa_in, sb_in = a, b
        out[f"ssim{i}_img1"], out[f"ssim{i}_img2"] = np.ascontiguousarray(sa_in), np.ascontiguousarray(sb_in)
        out[f"ssim{i}_meta"] = np.array([ws, int(sa), ["HWC", "NHWC", "NCHW"].index(fmt)], np.int32)
        out[f"ssim{i}_ref"], out[f"ssim{i}_fp64"] = ref.astype(np.float32), f64
        print(f"ssim case {i}: {a.shape} ws {ws} avg {sa} {kind}: ref-fp64 {np.abs(ref - f64).max():.2e}")
    out["ssim_n"] = np.array([len(cases)], np.int32)

    # ---- ARI
    ari = []
    for k in range(2, 9):
        n = int(rng.integers(50, 3000))
        t, p = rng.integers(0, k, n), rng.integers(0, k, n)
        p[: n // 2] = t[: n // 2]
        ari.append((t, p))
    t = rng.integers(0, 5, 400)
    perm = rng.permutation(5)
    ari += [(t, perm[t]), (np.zeros(100, np.int64), np.zeros(100, np.int64)), (np.zeros(0, np.int64), np.zeros(0, np.int64)),
            (np.array([1]), np.array([0])), (np.array([0, 1]), np.array([1, 1])),
            (np.zeros(300, np.int64), rng.integers(0, 3, 300))]        # empty fg subset (no true label 1)
    t = (rng.random(5000) < 0.3).astype(np.float32)
    ari.append((t, (rng.random(5000) < 0.35).astype(np.float32)))          # float masks, as the trainer's sem_gt
    for i, (t, p) in enumerate(ari):
        fg = t == 1
        out[f"ari{i}_true"], out[f"ari{i}_pred"] = t.astype(np.float32 if t.dtype == np.float32 else np.int32), p.astype(
            np.float32 if p.dtype == np.float32 else np.int32)
        out[f"ari{i}_want"] = np.array([adjusted_rand_score(t, p), adjusted_rand_score(t[fg], p[fg])], np.float64)
    out["ari_n"] = np.array([len(ari)], np.int32)

    # ---- k-means with pinned init
    g = np.load(os.path.join(HERE, "trained_img64k.npz"))
    sem = torch.from_numpy(g["eval_semantics"]).float().softmax(-1).numpy()
    kcases = []
    for K, C, n in [(3, 2, 600), (4, 3, 900), (5, 8, 1500), (2, 2, 4096), (3, 5, 2000), (16, 16, 3000)]:
        cent = rng.normal(0, 1, (K, C)) * 2
        x = (cent[rng.integers(0, K, n)] + rng.normal(0, 1.2, (n, C))).astype(np.float32)
        kcases.append((x, K, True))
    kcases.append((sem, 2, False))
    kept = 0
    for x, K, store_x in kcases:
        init = kmeans_plusplus(x, K, random_state=int(rng.integers(0, 1 << 30)))[0].astype(np.float32)
        a = KMeans(K, init=init, n_init=1, algorithm="lloyd").fit(x)
        b = KMeans(K, init=init.astype(np.float64), n_init=1, algorithm="lloyd").fit(x.astype(np.float64))
        if a.n_iter_ != b.n_iter_ or not np.array_equal(a.labels_, b.labels_):
            print(f"k-means case K={K} C={x.shape[1]} dropped: fp32 and fp64 disagree")
            continue
        pre = f"km{kept}"
        if store_x:
            out[pre + "_x"] = x
        out[pre + "_init"], out[pre + "_labels"] = init, a.labels_.astype(np.int8)
        out[pre + "_n_iter"], out[pre + "_inertia"] = np.array([a.n_iter_], np.int32), np.array([b.inertia_], np.float64)
        print(f"k-means case {kept}: K={K} C={x.shape[1]} N={x.shape[0]}: n_iter {a.n_iter_} inertia {b.inertia_:.6f}")
        kept += 1
    out["km_n"] = np.array([kept], np.int32)

    # ---- seed spread of the reference's clustering on the trained semantics (utils/misc.py:49, random_state 0..7)
    gt = g["gt_label"].astype(np.int32)
    raw = g["eval_semantics"].astype(np.float32)
    spread = np.zeros((2, 8, 2), np.float64)   # [softmax?][seed][inertia, clus_ari]
    for j, feats in enumerate((sem, raw)):
        for s in range(8):
            km = KMeans(2, random_state=s).fit(feats)
            spread[j, s] = km.inertia_, adjusted_rand_score(gt, km.labels_)
    out["seed_spread"] = spread
    print("seed spread (softmax):", spread[0, :, 0].min(), spread[0, :, 0].max(), spread[0, :, 1].min(), spread[0, :, 1].max())
    # eval_one_view numbers on the reference render: sem_ari / sem_ari_fg (argmax of the softmax vs gt_label)
    pred = sem.argmax(-1)
    fg = gt == 1
    out["view_sem_ari"] = np.array([adjusted_rand_score(gt, pred), adjusted_rand_score(gt[fg], pred[fg])], np.float64)
    np.savez_compressed(os.path.join(HERE, "eval_metrics.npz"), **out)
    print("wrote", os.path.join(HERE, "eval_metrics.npz"), os.path.getsize(os.path.join(HERE, "eval_metrics.npz")), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("NERF_SOS_REF", "../NeRF-SOS"))

"""GPU: eval_post_kernel / eval_post_finish_kernel (csrc/eval_post.hip) against fp64 at the ray counts around one workgroup (255 /
256 / 257), around the grid cap of 256 x 256 threads where the grid-stride loop starts its second pass (65 535 / 65 536 / 65 537)
and well past it (200 003), at C = 1, 2, 3 and the limit 64: softmax within a derived bound, labels exact against the kernel's own
probabilities and against fp64 wherever fp64 decides, exact ties, +-inf / NaN logits, the squared error term by term as the kernel
writes it, leading shapes, a non-contiguous rgb, and the refusals."""
import functools

import numpy as np
import pytest
import torch

from nerf_sos_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24 = 2.0 ** -24
PROB_BOUND = 4 * U24      # one expf per term (its argument rounded once), the denominator's sum, one divide; all values <= 1
SMALL, LARGE = (1, 255, 256, 257), (65535, 65536, 65537, 200003)
SHAPES = [(n, C) for C in (1, 2, 3, 64) for n in SMALL] + [(n, C) for C in (3, 64) for n in LARGE]


def ulps(a, b):
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


@functools.lru_cache(maxsize=None)
def inputs(n, C):
    """(logits = randn * 4 [n,C], rgb, target [n,3]) on the host, and their fp64 references, computed once."""
    g = torch.Generator().manual_seed(1000 + n + C)
    sem = torch.randn(n, C, generator=g) * 4
    rgb, tgt = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
    prob64 = torch.softmax(sem.double(), -1).numpy()
    return sem, rgb, tgt, prob64, mse_reference(rgb, tgt)


def mse_reference(rgb, tgt):
    """The per-ray term in fp32 exactly as the kernel writes it -- ((d0 d0 + d1 d1) + d2 d2) / 3, nothing contracted -- summed in
    fp64 and divided by n."""
    d = rgb.numpy() - tgt.numpy()
    term = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) / np.float32(3.0)
    assert term.dtype == np.float32
    return float(term.astype(np.float64).sum() / d.shape[0])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("n,C", SHAPES)
def test_softmax_labels_and_mse_vs_fp64(n, C):
    """sem_prob within 4 x 2^-24 of the fp64 softmax and rows summing to 1 within C x 2^-24; sem the first arg-max of the kernel's
    own sem_prob on every ray and the fp64 arg-max wherever the fp64 top two are > 1e-6 apart (>= 99 % of rays, checked on the
    reference); mse within 1 ulp and psnr within 2e-6 of the fp32 term summed in fp64; repeated, rgb-only and semantics-only calls
    return the same bits.

    Measured on the MI355X: |sem_prob - fp64| <= 1.53 x 2^-24 and |row sum - 1| <= 1.50 x 2^-24 at every shape.  This test found the
    denominator summed by C sequential fp32 adds: 6.7 ... 15.2 x 2^-24 at C = 64 (ATen's fp32 softmax on the CPU: 5.5 on the same
    logits, so neither 4 x 2^-24 nor twice the CPU's error held); it is summed in fp64 now and the CPU yardstick is not needed."""
    sem, rgb, tgt, prob64, mse64 = inputs(n, C)
    s, r, t = sem.to(DEV), rgb.to(DEV), tgt.to(DEV)
    out = ops.eval_postprocess(s, r, t)
    assert set(out) == {"sem_prob", "sem", "mse", "psnr"}
    assert out["sem_prob"].shape == (n, C) and out["sem"].shape == (n, 1) and out["sem"].dtype == torch.int32
    prob, lab = out["sem_prob"].cpu().numpy(), out["sem"].cpu().numpy()[:, 0]
    err = np.abs(prob.astype(np.float64) - prob64).max()
    dev = np.abs(prob.astype(np.float64).sum(-1) - 1.0).max()
    print(f"n={n} C={C}: |sem_prob - fp64| = {err / U24:.2f} x 2^-24, |row sum - 1| = {dev / U24:.2f} x 2^-24")
    assert err <= PROB_BOUND
    assert dev <= C * U24
    assert np.array_equal(lab, np.argmax(prob, -1))                       # first occurrence
    if C > 1:
        top = np.sort(prob64, -1)
        clear = top[:, -1] - top[:, -2] > 1e-6
        assert clear.mean() >= 0.99
        assert np.array_equal(lab[clear], np.argmax(prob64, -1)[clear])
    else:
        assert (prob == 1.0).all() and (lab == 0).all()
    mse, psnr = out["mse"].cpu().numpy(), out["psnr"].cpu().numpy()
    want_psnr = -10.0 * np.log10(mse64)
    print(f"n={n}: mse {mse[0]:.9g} vs {mse64:.12g}, psnr {psnr[0]:.7g} vs {want_psnr:.10g}")
    assert mse.shape == (1,) and int(ulps(mse, np.float32(mse64))[0]) <= 1
    assert abs(float(psnr[0]) - want_psnr) <= 2e-6 * max(1.0, abs(want_psnr))
    again = ops.eval_postprocess(s, r, t)
    assert all(same_bits(out[k], again[k]) for k in out)
    only_sem, only_rgb = ops.eval_postprocess(semantics=s), ops.eval_postprocess(rgb=r, target=t)
    assert set(only_sem) == {"sem_prob", "sem"} and set(only_rgb) == {"mse", "psnr"}
    assert all(same_bits(out[k], v) for k, v in {**only_sem, **only_rgb}.items())


@pytest.mark.parametrize("n", [257, 65537])
def test_identical_images(n):
    """rgb == target: mse is exactly 0 and psnr is +inf."""
    rgb = inputs(n, 3)[1].to(DEV)
    out = ops.eval_postprocess(rgb=rgb, target=rgb.clone())
    assert out["mse"].item() == 0.0 and out["psnr"].item() == float("inf")


@pytest.mark.parametrize("C", [1, 2, 3, 64])
def test_exact_ties_go_to_the_smaller_index(C):
    """Rows of equal logits (sem_prob exactly fl(1 / C), label 0) and rows whose two largest logits are equal at (0, C-1) and at
    (C-2, C-1), spread among ordinary rows over more than one workgroup."""
    n = 300
    sem = inputs(257, C)[0].repeat(2, 1)[:n].clone()
    flat, first, last = range(0, n, 7), range(1, n, 7), range(2, n, 7)
    for k, r_ in enumerate(flat):
        sem[r_] = (0.0, 3.5, -7.25, 30.0)[k % 4]
    if C > 1:
        for rows, lo in ((first, 0), (last, C - 2)):
            for r_ in rows:
                sem[r_] = -1.0 - sem[r_].abs()
                sem[r_, lo] = sem[r_, C - 1] = 2.0
    out = ops.eval_postprocess(semantics=sem.to(DEV))
    prob, lab = out["sem_prob"].cpu().numpy(), out["sem"].cpu().numpy()[:, 0]
    assert (prob[list(flat)] == np.float32(1.0) / np.float32(C)).all() and (lab[list(flat)] == 0).all()
    if C > 1:
        for rows, lo in ((first, 0), (last, C - 2)):
            rows = list(rows)
            assert np.array_equal(prob[rows, lo], prob[rows, C - 1]) and (prob[rows, lo] == prob[rows].max(-1)).all()
            assert (lab[rows] == lo).all()
    assert np.array_equal(lab, np.argmax(prob, -1))


def test_special_logits():
    """A row with one +inf, a row with a NaN and a row of all -inf give what torch.softmax / argmax give on the same fp32 row on the
    CPU (NaN compared as NaN); every other row has the bits it has without them."""
    sem = inputs(257, 3)[0].repeat(1, 2)[:, :5].clone()                    # [257, 5]
    plain = ops.eval_postprocess(semantics=sem.to(DEV))
    odd = sem.clone()
    rows = (0, 100, 255, 256)
    odd[0, 1] = float("inf")
    odd[100, 2] = float("nan")
    odd[255] = float("-inf")
    odd[256, 0] = odd[256, 4] = float("inf")
    out = ops.eval_postprocess(semantics=odd.to(DEV))
    torch.cuda.synchronize()
    want_p = torch.softmax(odd, -1)
    want_l = torch.argmax(want_p, -1)
    prob, lab = out["sem_prob"].cpu(), out["sem"].cpu()[:, 0]
    for r_ in rows:
        assert np.array_equal(prob[r_].numpy(), want_p[r_].numpy(), equal_nan=True) and int(lab[r_]) == int(want_l[r_]), r_
        assert torch.isnan(want_p[r_]).all()                               # what the reference computes for such a row
    keep = torch.ones(257, dtype=torch.bool)
    keep[list(rows)] = False
    assert same_bits(prob[keep], plain["sem_prob"].cpu()[keep]) and torch.equal(lab[keep], plain["sem"].cpu()[:, 0][keep])


def test_leading_shapes_and_strided_rgb():
    """[H, W, C] with H W = 65 537 keeps its leading dimensions; rgb given as a non-contiguous slice of a wider tensor gives the
    bits of its contiguous copy."""
    n, C = 65537, 3
    sem, rgb, tgt, _, _ = inputs(n, C)
    flat = ops.eval_postprocess(sem.to(DEV), rgb.to(DEV), tgt.to(DEV))
    img = ops.eval_postprocess(sem.to(DEV).reshape(n, 1, C), rgb.to(DEV).reshape(n, 1, 3), tgt.to(DEV).reshape(n, 1, 3))
    assert img["sem_prob"].shape == (n, 1, C) and img["sem"].shape == (n, 1, 1) and img["mse"].shape == (1,)
    assert same_bits(img["sem_prob"].reshape(n, C), flat["sem_prob"]) and same_bits(img["sem"].reshape(n, 1), flat["sem"])
    assert same_bits(img["mse"], flat["mse"]) and same_bits(img["psnr"], flat["psnr"])
    wide = torch.full((n, 5), 7.0, device=DEV)
    wide[:, 1:4] = rgb.to(DEV)
    view = wide[:, 1:4]
    assert not view.is_contiguous()
    got = ops.eval_postprocess(rgb=view, target=tgt.to(DEV))
    assert same_bits(got["mse"], flat["mse"]) and same_bits(got["psnr"], flat["psnr"])
    assert (wide[:, 0] == 7.0).all() and (wide[:, 4] == 7.0).all()


def test_refusals():
    for C in (0, 65):
        with pytest.raises(RuntimeError, match="nsos_eval_postprocess"):
            ops.eval_postprocess(semantics=torch.zeros(4, C, device=DEV))
    assert ops.eval_postprocess(semantics=torch.zeros(4, 64, device=DEV))["sem"].shape == (4, 1)
    torch.cuda.synchronize()

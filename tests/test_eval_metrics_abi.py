"""CPU: the evaluation-metric entry points (nsos_ssim, nsos_adjusted_rand, nsos_kmeans) validate before any launch, and their
workspace queries return stable sizes."""
import ctypes as C

from nerf_sos_amd import _lib

one = C.c_void_p(256)
null = None
big = 1 << 40


def test_ssim_rejects_before_launch():
    lib = _lib.lib()
    ok = dict(b=1, c=3, h=16, w=16)
    call = lambda a=one, b=one, n=1, ch=3, h=16, w=16, ws=11, out=one, wsp=one, nb=big: lib.nsos_ssim(
        a, b, n, ch, h, w, ws, None, 1, out, null, wsp, nb, null)
    assert call(a=null) == -1 and call(b=null) == -1 and call(out=null) == -1 and call(wsp=null) == -1
    assert call(n=-1) == -2 and call(ch=0) == -2 and call(h=-3) == -2 and call(w=0) == -2
    for bad in (10, 0, -1, 33, 35):
        assert call(ws=bad) == -3, bad
    assert call(wsp=C.c_void_p(260)) == -5
    assert call(nb=8) == -4
    assert lib.nsos_ssim_workspace_bytes(1, 3, 756, 1008) == 8 * 3 * 48 * 32 == lib.nsos_ssim_workspace_bytes(1, 3, 756, 1008)
    assert lib.nsos_ssim_workspace_bytes(1, 3, 0, 8) == 0 and ok


def test_adjusted_rand_rejects_before_launch():
    lib = _lib.lib()
    out = C.c_void_p(512)
    assert lib.nsos_adjusted_rand(one, one, 4, 0, 1, null, one, null) == -1
    assert lib.nsos_adjusted_rand(one, one, 4, 0, 1, out, null, null) == -1
    assert lib.nsos_adjusted_rand(null, one, 4, 0, 1, out, one, null) == -1
    assert lib.nsos_adjusted_rand(one, one, -1, 0, 1, out, one, null) == -2
    assert lib.nsos_adjusted_rand(one, one, 4, 7, 1, out, one, null) == -3
    assert lib.nsos_adjusted_rand(one, one, 4, -1, 1, out, one, null) == -3
    assert lib.nsos_adjusted_rand(one, one, 4, 0, 1, out, C.c_void_p(260), null) == -5
    assert lib.nsos_adjusted_rand_workspace_bytes() == (64 * 64 + 1) * 8 == lib.nsos_adjusted_rand_workspace_bytes()


def _km(x=one, B=2, N=100, Cf=2, K=2, trials=0, max_iter=300, tol=1e-4, mode=0, labels=one, ws=one, nb=big):
    return _lib.lib().nsos_kmeans(x, B, N, Cf, K, null, 0, 0, 1, trials, max_iter, tol, mode, labels, null, null, null, ws, nb, null)


def test_kmeans_rejects_before_launch():
    assert _km(x=null) == -1 and _km(labels=null) == -1 and _km(ws=null) == -1
    assert _lib.lib().nsos_kmeans(one, 1, 10, 2, 2, null, 0, 0, 0, 0, 300, 1e-4, 0, one, null, null, null, one, big, null) == -2
    assert _km(B=-1) == -2 and _km(N=-5) == -2 and _km(Cf=0) == -2 and _km(K=0) == -2 and _km(max_iter=-1) == -2
    assert _km(K=17) == -3 and _km(Cf=17) == -3
    assert _km(N=3, K=4) == -2                      # N < K
    assert _km(mode=3) == -3 and _km(trials=-1) == -3 and _km(tol=-1.0) == -3
    assert _km(ws=C.c_void_p(264)) == -5
    assert _km(nb=64) == -4
    lib = _lib.lib()
    a = lib.nsos_kmeans_workspace_bytes(8, 4096, 2, 2)
    assert a > 0 and a == lib.nsos_kmeans_workspace_bytes(8, 4096, 2, 2)
    assert lib.nsos_kmeans_workspace_bytes(16, 4096, 2, 2) > a
    assert lib.nsos_kmeans_workspace_bytes(1, 10, 2, 17) == 0 and lib.nsos_kmeans_workspace_bytes(1, 10, 17, 2) == 0
    assert lib.nsos_kmeans_workspace_bytes(-1, 10, 2, 2) == 0

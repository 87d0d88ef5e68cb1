"""CPU: nsos_lpips_* validate before any launch, and the size queries match the documented layouts (include/nerf_sos_hip.h "LPIPS")."""
import ctypes as C

from nerf_sos_amd import _lib

KP, COUT = (384, 1600, 1728, 3456, 2304), (64, 192, 384, 256, 256)


def _sizes(h, w):
    a = ((h + 4 - 11) // 4 + 1, (w + 4 - 11) // 4 + 1)
    b = ((a[0] - 3) // 2 + 1, (a[1] - 3) // 2 + 1)
    c = ((b[0] - 3) // 2 + 1, (b[1] - 3) // 2 + 1)
    return [a, b, c, c, c], [b, c]


def test_packed_bytes_is_the_documented_layout():
    lib = _lib.lib()
    assert lib.nsos_lpips_packed_bytes() == 4 * (8 + sum((kp + 2) * co for kp, co in zip(KP, COUT)))
    assert KP[0] == (3 * 11 * 11 + 31) // 32 * 32 and KP[1:] == (64 * 25, 192 * 9, 384 * 9, 256 * 9)


def test_workspace_bytes():
    lib = _lib.lib()
    f = lib.nsos_lpips_workspace_bytes
    for n, h, w in ((1, 31, 31), (2, 33, 47), (1, 64, 64), (1, 97, 130), (1, 756, 1008)):
        feats, pools = _sizes(h, w)
        floats = 2 * n * (sum(a * b * c for (a, b), c in zip(feats, COUT)) + sum(a * b * c for (a, b), c in zip(pools, COUT))) + 2 * n * 5 * 64
        assert f(n, h, w) == 4 * floats, (n, h, w)
        assert f(n, h, w) == f(n, h, w)                                      # stable
        assert f(n + 1, h, w) > f(n, h, w) and f(n, h + 8, w) > f(n, h, w) and f(n, h, w + 8) > f(n, h, w)
        assert f(n, h, w) % 16 == 0
    for n, h, w in ((0, 64, 64), (-1, 64, 64), (1, 30, 64), (1, 64, 30), (1, 0, 64), (1, 64, -5), (1025, 64, 64), (1, 16385, 64),
                    (1024, 16384, 16384)):
        assert f(n, h, w) == 0, (n, h, w)


def test_return_codes_before_any_launch():
    lib = _lib.lib()
    fwd = lib.nsos_lpips_forward
    p = C.c_void_p(4096)
    big = 1 << 40
    ok = dict(img0=p, img1=p, batch=1, h=64, w=64, flags=0, packed=p, out=p, layers=None, feats=None, workspace=p, nbytes=big)

    def call(**change):
        a = {**ok, **change}
        return fwd(a["img0"], a["img1"], a["batch"], a["h"], a["w"], a["flags"], a["packed"], a["out"], a["layers"], a["feats"],
                   a["workspace"], a["nbytes"], None)

    for name in ("img0", "img1", "packed", "out", "workspace"):
        assert call(**{name: None}) == -1, name
    assert call(batch=-1) == -2 and call(h=0) == -2 and call(w=-3) == -2
    assert call(batch=0) == 0                                               # empty batch: no launch
    assert call(h=30) == -3 and call(w=30) == -3 and call(h=30, w=30) == -3
    assert call(flags=4) == -3 and call(flags=-1) == -3
    assert call(batch=1025) == -3 and call(h=16385) == -3
    need = lib.nsos_lpips_workspace_bytes(1, 64, 64)
    assert call(nbytes=need - 1) == -4 and call(nbytes=0) == -4
    for name, addr in (("img0", 4098), ("img1", 4097), ("out", 4099), ("layers", 4098), ("packed", 4100), ("feats", 4104),
                       ("workspace", 4104)):
        assert call(**{name: C.c_void_p(addr)}) == -5, name
    # precedence: NULL before shape before unsupported before alignment before size
    assert call(img0=None, batch=-1) == -1 and call(batch=-1, h=30) == -2 and call(h=30, nbytes=0) == -3
    assert call(workspace=C.c_void_p(4104), nbytes=0) == -5


def test_pack_return_codes():
    lib = _lib.lib()
    p = 4096
    ts = _lib.LpipsTensors()
    ts.shift = ts.scale = p
    for i in range(5):
        ts.conv_w[i] = ts.conv_b[i] = ts.lin_w[i] = p
    nbytes = lib.nsos_lpips_packed_bytes()
    assert lib.nsos_lpips_pack(None, C.c_void_p(p), nbytes, None) == -1
    assert lib.nsos_lpips_pack(C.byref(ts), None, nbytes, None) == -1
    assert lib.nsos_lpips_pack(C.byref(ts), C.c_void_p(p + 8), nbytes, None) == -5
    assert lib.nsos_lpips_pack(C.byref(ts), C.c_void_p(p), nbytes - 1, None) == -4
    ts.lin_w[3] = None
    assert lib.nsos_lpips_pack(C.byref(ts), C.c_void_p(p), nbytes, None) == -1

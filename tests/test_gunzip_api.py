"""The C ABI of the device's plain-gzip reader as far as it needs no device: the exports, the workspace formula of
include/sickle_amd.h (capacity 0 and SK_GZIP_CHUNK included), and the bad arguments that are refused before anything
touches a device.  CPU only."""
import ctypes as C

from sickle_amd import capi


def test_exports_and_constants():
    L = capi.lib()
    for name in ("sk_gzip_inflate_workspace_bytes", "sk_gzip_inflate_device_async", "sk_gzip_inflate_device_finish"):
        assert name in capi.EXPORTS and hasattr(L, name), name
    assert L.sk_abi_version() == 2
    assert C.sizeof(capi.GzipInflateCounts) == 64
    for name in ("gzip_inflate_device_async", "gzip_inflate_device_finish", "gunzip", "trim_gz"):
        assert callable(getattr(capi.Context, name))


def formula(n, capacity, chunk=None):
    a16 = lambda x: 16 * ((x + 15) // 16)
    if chunk is None:
        chunk = 32768
        while chunk * 4096 < n:
            chunk *= 2
    s = -(-n // chunk)
    return 256 + 128 * (s + 1) + a16(8 * (s + 1)) + a16(4 * (s + 1)) + 32 * (n // 18 + 1) + a16(2 * capacity)


SIZES = sorted(set([0, 1, 17, 18, 19, 255, 256, 257, 32767, 32768, 32769] + [k * 32768 * 4096 + d for k in (1, 2) for d in (-1, 0, 1)] +
                   [1 << 32, (1 << 32) + 1, 1 << 33]))


def test_workspace_formula(monkeypatch):
    monkeypatch.delenv("SK_GZIP_CHUNK", raising=False)
    L = capi.lib()
    for capacity in (0, 1, 16, 17, 1 << 20, 1 << 34):
        for n in SIZES:
            w = L.sk_gzip_inflate_workspace_bytes(n, capacity)
            assert w == formula(n, capacity) and w % 16 == 0, (n, capacity)
    assert L.sk_gzip_inflate_workspace_bytes(1 << 20, 4 << 20) - L.sk_gzip_inflate_workspace_bytes(1 << 20, 0) == 8 << 20


def test_the_chunk_override(monkeypatch):
    L = capi.lib()
    monkeypatch.delenv("SK_GZIP_CHUNK", raising=False)
    plain = L.sk_gzip_inflate_workspace_bytes(1 << 20, 0)
    last = plain
    for chunk in (16384, 4096, 1024, 256):
        monkeypatch.setenv("SK_GZIP_CHUNK", str(chunk))
        w = L.sk_gzip_inflate_workspace_bytes(1 << 20, 0)
        assert w == formula(1 << 20, 0, chunk) and w > last
        last = w
    for ignored in ("128", "300", "0", "-4", "x", "256x", ""):
        monkeypatch.setenv("SK_GZIP_CHUNK", ignored)
        assert L.sk_gzip_inflate_workspace_bytes(1 << 20, 0) == plain, ignored


def test_bad_arguments_need_no_device():
    L = capi.lib()
    c = capi.GzipInflateCounts()
    assert L.sk_gzip_inflate_device_async(None, None, 0, None, 0, None, 0, None) == capi.SK_EINVAL
    assert L.sk_gzip_inflate_device_finish(None, None, None, C.byref(c)) == capi.SK_EINVAL
    assert L.sk_gzip_inflate_device_finish(None, C.c_void_p(16), None, None) == capi.SK_EINVAL

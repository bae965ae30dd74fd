"""The C ABI of the device's BGZF reader as far as it needs no device: the exports, the workspace formula of
include/sickle_amd.h, and the bad arguments that are refused before anything touches a device.  CPU only."""
import ctypes as C

from sickle_amd import capi


def test_exports_and_constants():
    L = capi.lib()
    for name in ("sk_bgzf_inflate_workspace_bytes", "sk_bgzf_inflate_device_async", "sk_bgzf_inflate_device_finish"):
        assert name in capi.EXPORTS and hasattr(L, name), name
    assert capi.SK_EDATA == -7 and L.sk_abi_version() == 2
    assert (capi.SK_GZ_OK, capi.SK_GZ_HEADER, capi.SK_GZ_TRUNCATED, capi.SK_GZ_DEFLATE, capi.SK_GZ_LENGTH,
            capi.SK_GZ_CRC) == (0, 1, 2, 3, 4, 5)
    assert C.sizeof(capi.BgzfInflateCounts) == 48
    assert issubclass(capi.GzDataError, capi.SickleError)
    e = capi.GzDataError(capi.SK_GZ_CRC, 7, 1234)
    assert (e.reason, e.member, e.offset) == (capi.SK_GZ_CRC, 7, 1234)
    for name in ("bgzf_inflate_device_async", "bgzf_inflate_device_finish", "bgunzip", "trim_gz"):
        assert callable(getattr(capi.Context, name))


def formula(n):
    a16 = lambda x: 16 * ((x + 15) // 16)
    c = n // 4 + 1
    return 128 + a16(4 * (n // 4096 + 1)) + a16(8 * c) + 3 * a16(4 * c) + a16(40 * (n // 26 + 1))


def test_workspace_formula():
    L = capi.lib()
    sizes = sorted(set([0, 1, 3, 4, 25, 26, 27, 28, 100, 4095, 4096, 4097] +
                       [k * 65536 + d for k in (1, 2, 1000) for d in (-1, 0, 1)] + [1 << 32, (1 << 32) + 1, 1 << 33]))
    works = [L.sk_bgzf_inflate_workspace_bytes(n) for n in sizes]
    assert works == sorted(works)
    for n, w in zip(sizes, works):
        assert w == formula(n) and w % 16 == 0 and w >= 128, n
    assert works[-1] < 6.7 * (1 << 33)


def test_bad_arguments_need_no_device():
    L = capi.lib()
    c = capi.BgzfInflateCounts()
    assert L.sk_bgzf_inflate_device_async(None, None, 0, None, 0, None, 0, None) == capi.SK_EINVAL
    assert L.sk_bgzf_inflate_device_finish(None, None, None, C.byref(c)) == capi.SK_EINVAL
    assert L.sk_bgzf_inflate_device_finish(None, C.c_void_p(16), None, None) == capi.SK_EINVAL

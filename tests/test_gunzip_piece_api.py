"""CPU: plain gzip read on the device in pieces (sk_gzip_inflate_piece_workspace_bytes, sk_gzip_inflate_piece_device_async,
sk_gzip_inflate_piece_device_finish, include/sickle_amd.h): the symbols, the structs, the workspace formula and the
argument checks that need no device."""
import ctypes as C
import inspect

import pytest

from sickle_amd import capi

NEW = ("sk_gzip_inflate_piece_workspace_bytes", "sk_gzip_inflate_piece_device_async", "sk_gzip_inflate_piece_device_finish")


def offsets(struct):
    return [(f[0], getattr(struct, f[0]).offset) for f in struct._fields_]


def test_symbols_and_structs():
    L = capi.lib()
    for name in NEW:
        assert hasattr(L, name), name
        assert name in capi.EXPORTS
    assert L.sk_abi_version() == 2
    assert C.sizeof(capi.GzipPieceState) == capi.SK_GZIP_PIECE_STATE_BYTES == 128 + 32768
    assert offsets(capi.GzipPieceState) == [("pos_bit", 0), ("in_member", 8), ("member_text", 16), ("member_crc", 24), ("members", 32),
                                            ("text_bytes", 40), ("status", 48), ("error", 56), ("error_member", 64),
                                            ("error_offset", 72), ("done", 80), ("reserved", 88), ("history", 128)]
    assert C.sizeof(capi.GzipPiece) == 24
    assert offsets(capi.GzipPiece) == [("image_offset", 0), ("window_bytes", 8), ("last", 16), ("reserved", 20)]
    assert C.sizeof(capi.GzipPieceCounts) == 40
    assert offsets(capi.GzipPieceCounts) == [("pos_bit", 0), ("in_member", 8), ("image_bytes_consumed", 16), ("window_limited", 24),
                                             ("inherited", 28), ("done", 32), ("reserved", 36)]
    for name in ("gzip_inflate_piece_device_async", "gzip_inflate_piece_device_finish", "gunzip_stream", "trim_gzip_stream"):
        assert hasattr(capi.Context, name), name
    sig = inspect.signature(capi.Context.trim_gzip_stream).parameters
    assert sig["window_bytes"].default is None and sig["gz"].default is True and sig["mode"].default == "se"


def formula(w, capacity, chunk=None):
    a16 = lambda x: (x + 15) // 16 * 16
    if chunk is None:
        chunk = 32768
        while chunk * 4096 < w:
            chunk *= 2
    s = -(-w // chunk)
    return 256 + 128 * (s + 1) + a16(8 * (s + 1)) + a16(4 * (s + 1)) + 32 * (w // 18 + 2) + 32 * (s + 1) + a16(2 * (32768 + capacity))


@pytest.mark.parametrize("chunk", [None, 256, 4096])
def test_workspace_formula(chunk, monkeypatch):
    if chunk is None:
        monkeypatch.delenv("SK_GZIP_CHUNK", raising=False)
    else:
        monkeypatch.setenv("SK_GZIP_CHUNK", str(chunk))
    L = capi.lib()
    for w in (1, 600, 32768, 32769, 1 << 20, (1 << 27) + 5, 1 << 30, 1 << 33):
        for capacity in (0, 1, 4096, 100001, 1 << 32):
            assert L.sk_gzip_inflate_piece_workspace_bytes(w, capacity) == formula(w, capacity, chunk), (w, capacity)
    # the pieces' workspace is the whole call's and a constant more per stretch and for the history
    assert formula(1 << 20, 1 << 22, chunk) - L.sk_gzip_inflate_workspace_bytes(1 << 20, 1 << 22) == \
        32 + 32 * (-(-(1 << 20) // (chunk or 32768)) + 1) + 65536


def _piece(ctx=0x10, image=0x1000, image_bytes=4096, piece=True, window=4096, last=1, reserved=0, image_offset=0, state_in=0x20000,
           state_out=0x30000, out=0x40000, capacity=1 << 16, ws=0x100000, ws_bytes=1 << 30):
    pc = capi.GzipPiece(image_offset, window, last, reserved)
    return capi.lib().sk_gzip_inflate_piece_device_async(ctx, image, image_bytes, C.byref(pc) if piece else None, state_in, state_out,
                                                         out, capacity, ws, ws_bytes, None)


def test_argument_checks_without_device():
    """Every one of these returns SK_EINVAL before anything touches a device: the context is a zeroed block that only
    takes the error text, the other pointers are made up and never dereferenced."""
    E = capi.SK_EINVAL
    assert _piece(ctx=None) == E
    fake = C.create_string_buffer(1 << 16)
    ctx = C.addressof(fake)
    assert _piece(ctx, piece=False) == E
    assert _piece(ctx, state_in=None) == E and _piece(ctx, state_out=None) == E
    assert _piece(ctx, state_out=0x20000) == E  # state_out == state_in
    assert _piece(ctx, state_in=0x20008) == E and _piece(ctx, state_out=0x30004) == E
    assert _piece(ctx, reserved=1) == E
    assert _piece(ctx, window=0) == E and _piece(ctx, window=(1 << 33) + 1) == E
    assert _piece(ctx, out=None) == E and _piece(ctx, out=0x40008) == E
    assert _piece(ctx, image=None) == E
    assert _piece(ctx, ws=None) == E and _piece(ctx, ws=0x100008) == E
    need = capi.lib().sk_gzip_inflate_piece_workspace_bytes(4096, 1 << 16)
    assert _piece(ctx, ws_bytes=need - 1) == E
    c, pc = capi.GzipInflateCounts(), capi.GzipPieceCounts()
    F = capi.lib().sk_gzip_inflate_piece_device_finish
    assert F(None, 0x100000, None, C.byref(c), C.byref(pc)) == E
    assert F(ctx, None, None, C.byref(c), C.byref(pc)) == E
    assert F(ctx, 0x100000, None, None, C.byref(pc)) == E and F(ctx, 0x100000, None, C.byref(c), None) == E

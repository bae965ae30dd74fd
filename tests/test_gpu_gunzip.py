"""GPU: plain gzip read on the device (sk_gzip_inflate_device_async / finish, Context.gunzip, Context.trim_gz) against zlib,
tests/gunzip_model.py and the host run of the same stages (tests/test_gunzip_host.py): every kind of member and header,
images cut into one, a few and hundreds of stretches, the placeholder cases, many members, capacity, every reason code at
member 0 and in a later stretch, bad arguments, and plain .gz in -> .gz out against the BGZF path.  Beyond the fixtures'
sizes: images of more than 16 MiB read by one stretch, a guessed block beyond the text cap, 6 000 members, one member of
more than 4 GiB of text, a slice of tests/soak_gunzip.py, and the legal streams zlib never writes
(tests/foreign_images.py) at the default chunk and at 256, 1 024 and 4 096."""
import ctypes as C
import gzip
import struct

import pytest

import bgunzip_model as bm
import cli_util as cu
import foreign_images as fi
import gunzip_model as gm
import trim_model as tm
from bgzf_raw import SENTINEL, to_device, torch_mod, upload
from sickle_amd import capi
from test_fastq_api import golden_texts
from test_gunzip_host import host_chunk, long_runs, run_host, tool  # noqa: F401 (the fixtures that build and run the host harness)

pytestmark = pytest.mark.gpu
GUARD = 64
KEYS = ("error", "error_member", "error_offset")


def inflate(ctx, image, shift=0, capacity=None, count_only=False, chunk=0, monkeypatch=None, ws=None, surround=None):
    """One async + finish on raw pointers; `out` is capacity + GUARD bytes of SENTINEL, and the guard is checked here, in
    every test.  capacity None: the model's bytes_out.  chunk: SK_GZIP_CHUNK for the call.  ws: the workspace tensor, used
    as it is (the byte count handed to the library stays the formula's).  surround: what lies around the image on the
    device (bgzf_raw.upload).  -> (rc, counts, out[:capacity])"""
    torch = torch_mod()
    L = capi.lib()
    if monkeypatch is not None:
        if chunk:
            monkeypatch.setenv("SK_GZIP_CHUNK", str(chunk))
        else:
            monkeypatch.delenv("SK_GZIP_CHUNK", raising=False)
    keep, ptr = upload(image, shift, surround=surround)
    cap = gm.gunzip(image)["bytes_out"] if capacity is None else capacity
    need = L.sk_gzip_inflate_workspace_bytes(len(image), 0 if count_only else cap)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    out = torch.full((cap + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc = L.sk_gzip_inflate_device_async(ctx._h, ptr if len(image) else None, len(image), None if count_only else out.data_ptr(),
                                        0 if count_only else cap, ws.data_ptr(), need, None)
    assert rc == capi.SK_OK, L.sk_last_error(ctx._h)
    c = capi.GzipInflateCounts()
    rc = L.sk_gzip_inflate_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c))
    del keep
    assert bool((out[cap:] == SENTINEL).all()), "bytes of out at or beyond the capacity were written"
    return rc, c.as_dict(), out[:cap]


def text_of(out, counts):
    return out[:counts["bytes_out"]].cpu().numpy().tobytes()


# ---- 1 every kind of member and header -----------------------------------------------------------------------------
def test_every_kind_of_member(sk_ctx, monkeypatch):
    for k, (name, (image, text)) in enumerate(gm.images().items()):
        for shift in ((k % 16, (k + 7) % 16) if name not in ("level6", "fname") else range(16)):
            rc, c, out = inflate(sk_ctx, image, shift=shift, capacity=len(text), monkeypatch=monkeypatch)
            assert rc == capi.SK_OK, (name, shift, c)
            assert (c["bytes_in"], c["members"], c["bytes_out"], c["error"]) == (len(image), gm.gunzip(image)["members"], len(text), 0)
            assert text_of(out, c) == text, (name, shift)
    for level in (1, 6, 9):
        text = gm.texts()["fq"]
        for image in (gzip.compress(text, level), gm.member(text, level, head=gm.header(name=b"reads.fq"))):
            rc, c, out = inflate(sk_ctx, image, capacity=len(text), monkeypatch=monkeypatch)
            assert rc == capi.SK_OK and text_of(out, c) == text, level


def test_empty_image(sk_ctx, monkeypatch):
    rc, c, out = inflate(sk_ctx, b"", monkeypatch=monkeypatch)
    assert rc == capi.SK_OK and (c["members"], c["bytes_out"], c["error"], c["stretches"]) == (0, 0, 0, 0)
    assert sk_ctx.gunzip(to_device(b"x")[:0]).numel() == 0


# ---- 2 stretches, placeholders, members ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def expected(tool, tmp_path_factory):  # noqa: F811
    """name -> the host run's counts: the algorithm is deterministic, so the device's are the same"""
    d = tmp_path_factory.mktemp("gunzip_expected")
    s = dict(gm.stretch_images())
    s.update({k: v for k, v in gm.big_images().items() if v[2]})
    got = run_host(tool, [(v[0], v[2]) for v in s.values()], d)
    for (name, v), g in zip(s.items(), got):
        assert g["error"] == 0 and g["text"] == v[1], name
    return {name: {k: g[k] for k in ("stretches", "stretches_used", "members", "bytes_out")} for name, g in zip(s, got)}


@pytest.mark.parametrize("name", list(gm.stretch_images()) + ["fq1m_c4096", "fq1m_c1024", "fq1m_c256"])
def test_stretches(sk_ctx, monkeypatch, expected, name):
    """48 KiB, 200 KiB and 1 MiB in chunks of 256, 1024 and 4096 bytes; matches to the far end of the unknown window; a
    run across stretch starts; stretches shorter than the window; member ends inside a stretch and on a chunk boundary;
    65 and 300 members"""
    image, text, chunk = gm.stretch_images()[name] if name in gm.stretch_images() else gm.big_images()[name]
    rc, c, out = inflate(sk_ctx, image, shift=len(name) % 16, capacity=len(text), chunk=chunk, monkeypatch=monkeypatch)
    assert rc == capi.SK_OK, (name, c)
    assert {k: c[k] for k in expected[name]} == expected[name], name
    assert text_of(out, c) == text, name
    assert c["stretches_used"] > 1 and c["stretches"] == -(-len(image) // chunk)


def test_bgzf_image_and_long_member(sk_ctx, monkeypatch):
    monkeypatch.delenv("SK_GZIP_CHUNK", raising=False)
    text = gm.texts()["fq"] * 3
    image = sk_ctx.bgzf(to_device(text), eof=True).cpu().numpy().tobytes()
    rc, c, out = inflate(sk_ctx, image, capacity=len(text), monkeypatch=monkeypatch)
    assert rc == capi.SK_OK and c["members"] == (len(text) + 65279) // 65280 + 1 and text_of(out, c) == text
    image, text, _ = gm.big_images()["fq5m_gzip1"]
    got = sk_ctx.gunzip(to_device(image))
    assert got.cpu().numpy().tobytes() == text


# ---- 2b what zlib never writes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 256, 1024, 4096])
def test_foreign_images(sk_ctx, monkeypatch, tool, tmp_path, chunk):  # noqa: F811
    """Text and counts are the model's; stretches and stretches_used are the host run's of the same stages"""
    images = fi.valid("gzip")
    host = run_host(tool, [(v[0], host_chunk(chunk)) for v in images.values()], tmp_path)
    for (name, (image, text)), h in zip(images.items(), host):
        want = fi.expected("gzip")[name]
        rc, c, out = inflate(sk_ctx, image, shift=len(name) % 16, capacity=len(text), chunk=chunk, monkeypatch=monkeypatch)
        assert rc == capi.SK_OK, (name, chunk, c)
        assert (c["error"], c["members"], c["bytes_out"]) == (0, want["members"], len(text)), (name, chunk, c)
        assert text_of(out, c) == text == h["text"], (name, chunk)
        assert (c["stretches"], c["stretches_used"]) == (h["stretches"], h["stretches_used"]), (name, chunk, c)


def test_foreign_bad_and_shifted(sk_ctx, monkeypatch):
    for k, (name, (image, chunk)) in enumerate(fi.bad_images("gzip").items()):
        want = fi.bad_expected("gzip")[name]
        rc, c, out = inflate(sk_ctx, image, shift=k % 16, capacity=want["bytes_out"], chunk=chunk, monkeypatch=monkeypatch)
        assert rc == capi.SK_EDATA and c["error"] == capi.SK_GZ_DEFLATE, (name, c)
        assert tuple(c[x] for x in KEYS) == tuple(want[x] for x in KEYS), (name, c)
    image, text = fi.valid("gzip")["foreign_members"]
    rc, c, out = inflate(sk_ctx, image, shift=9, capacity=len(text), chunk=1024, monkeypatch=monkeypatch)
    assert rc == capi.SK_OK and c["members"] == fi.expected("gzip")["foreign_members"]["members"] and text_of(out, c) == text


# ---- 3 capacity ----------------------------------------------------------------------------------------------------
def test_capacity(sk_ctx, monkeypatch):
    for name, chunk in (("level6", 0), ("two", 1024), ("one_byte", 0)):
        image, text = gm.images()[name]
        need = len(text)
        rc, c, out = inflate(sk_ctx, image, capacity=need - 1, chunk=chunk, monkeypatch=monkeypatch)
        assert rc == capi.SK_ESPACE and c["bytes_out"] == need and c["error"] == 0
        assert bool((out == SENTINEL).all()), "out was written although the text does not fit"
        rc, c, out = inflate(sk_ctx, image, capacity=need, chunk=chunk, monkeypatch=monkeypatch)
        assert rc == capi.SK_OK and text_of(out, c) == text
        rc, c, out = inflate(sk_ctx, image, count_only=True, chunk=chunk, monkeypatch=monkeypatch)
        assert rc == capi.SK_OK and c["bytes_out"] == need and bool((out == SENTINEL).all())


# ---- 4 errors ------------------------------------------------------------------------------------------------------
def test_every_reason_at_member_0_and_in_a_later_stretch(sk_ctx, monkeypatch):
    seen = set()
    good, good_text = gm.images()["fname"]
    for k, (name, (image, chunk)) in enumerate(gm.bad_images().items()):
        want = gm.gunzip(image)
        rc, c, out = inflate(sk_ctx, image, shift=k % 16, chunk=chunk, monkeypatch=monkeypatch)
        assert rc == capi.SK_EDATA, name
        assert tuple(c[x] for x in KEYS) == tuple(want[x] for x in KEYS), (name, c)
        seen.add(c["error"])
    assert seen == {capi.SK_GZ_HEADER, capi.SK_GZ_TRUNCATED, capi.SK_GZ_DEFLATE, capi.SK_GZ_LENGTH, capi.SK_GZ_CRC}
    rc, c, out = inflate(sk_ctx, good, monkeypatch=monkeypatch)  # the context goes on
    assert rc == capi.SK_OK and text_of(out, c) == good_text
    bad = gm.bad_images()
    # counting sees headers and Huffman-level damage, not CRCs
    rc, c, out = inflate(sk_ctx, bad["crc@1"][0], count_only=True, chunk=1024, monkeypatch=monkeypatch)
    assert rc == capi.SK_OK and c["error"] == 0
    rc, c, out = inflate(sk_ctx, bad["dynamic_header@1"][0], count_only=True, chunk=1024, monkeypatch=monkeypatch)
    assert rc == capi.SK_EDATA and c["error"] == capi.SK_GZ_DEFLATE and c["error_member"] == 1
    rc, c, out = inflate(sk_ctx, bad["trailing_byte@0"][0], capacity=1, chunk=1024, monkeypatch=monkeypatch)
    assert rc == capi.SK_EDATA and c["error"] == capi.SK_GZ_HEADER and bool((out == SENTINEL).all())
    monkeypatch.delenv("SK_GZIP_CHUNK", raising=False)
    with pytest.raises(capi.GzDataError) as e:
        sk_ctx.gunzip(to_device(bad["crc@1"][0]))
    assert (e.value.reason, e.value.member) == (capi.SK_GZ_CRC, 1)


# ---- 5 bad arguments -----------------------------------------------------------------------------------------------
def test_bad_arguments_enqueue_nothing(sk_ctx, monkeypatch):
    monkeypatch.delenv("SK_GZIP_CHUNK", raising=False)
    torch = torch_mod()
    L = capi.lib()
    data, text = gm.images()["level6"]
    image = to_device(data)
    ws_bytes = L.sk_gzip_inflate_workspace_bytes(len(data), len(text))
    ws = torch.full((ws_bytes + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = torch.full((len(text) + 32,), SENTINEL, dtype=torch.uint8, device="cuda")

    def call(ctx=sk_ctx._h, img=image.data_ptr(), n=len(data), o=out.data_ptr(), capacity=len(text), wsp=ws.data_ptr(),
             wsb=ws_bytes):
        return L.sk_gzip_inflate_device_async(ctx, img, n, o, capacity, wsp, wsb, None)

    assert call(ctx=None) == capi.SK_EINVAL
    assert call(img=None) == capi.SK_EINVAL
    assert call(o=out.data_ptr() + 8) == capi.SK_EINVAL
    assert call(o=None) == capi.SK_EINVAL
    assert call(wsp=ws.data_ptr() + 8) == capi.SK_EINVAL
    assert call(wsp=None) == capi.SK_EINVAL
    assert call(wsb=ws_bytes - 1) == capi.SK_EINVAL
    assert call(n=(1 << 33) + 1, wsb=1 << 62) == capi.SK_EINVAL
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all()), "a refused call enqueued something"
    assert L.sk_gzip_inflate_device_finish(None, ws.data_ptr(), None, C.byref(capi.GzipInflateCounts())) == capi.SK_EINVAL
    assert call() == capi.SK_OK
    c = capi.GzipInflateCounts()
    assert L.sk_gzip_inflate_device_finish(sk_ctx._h, ws.data_ptr(), None, C.byref(c)) == capi.SK_OK
    assert out[:c.bytes_out].cpu().numpy().tobytes() == text and bool((out[c.bytes_out:] == SENTINEL).all())


def test_the_bgzf_entry_still_refuses_plain_gzip(sk_ctx):
    with pytest.raises(capi.GzDataError) as e:
        sk_ctx.bgunzip(to_device(gm.images()["py_gzip"][0]))
    assert (e.value.reason, e.value.member, e.value.offset) == (capi.SK_GZ_HEADER, 0, 0)


# ---- 6 Context.gunzip, plain .gz in -> .gz out ---------------------------------------------------------------------
def test_context_gunzip(sk_ctx, monkeypatch):
    monkeypatch.delenv("SK_GZIP_CHUNK", raising=False)
    image, text = gm.images()["two"]
    assert sk_ctx.gunzip(to_device(image)).cpu().numpy().tobytes() == text


def test_trim_gz_takes_plain_gzip(sk_ctx, tmp_path, monkeypatch):
    """A golden input as plain gzip and as BGZF through trim_gz: the same counts and, decompressed, the same bytes"""
    monkeypatch.setenv("SK_GZIP_CHUNK", "1024")
    cu.prepare_inputs(tmp_path)
    cu.prepare_long_inputs(tmp_path)
    name, rec = next((n, r) for n, r in tm.golden_runs() if n not in tm.UNREPLAYABLE)
    mode, texts, files = golden_texts(rec["argv"], tmp_path)
    params = capi.make_params(*tm.run_params(rec["argv"]))
    plain = [to_device(gzip.compress(t, 6)) for t in texts]
    bgzf = [to_device(bm.bgzip(t)) for t in texts]
    got, counts = sk_ctx.trim_gz(params, plain[0], plain[1] if len(plain) > 1 else None, mode=mode)
    want, counts2 = sk_ctx.trim_gz(params, bgzf[0], bgzf[1] if len(bgzf) > 1 else None, mode=mode)
    assert counts == counts2
    for o in range(3):
        assert (got[o] is None) == (want[o] is None)
        if want[o] is not None:
            assert gzip.decompress(got[o].cpu().numpy().tobytes()) == gzip.decompress(want[o].cpu().numpy().tobytes()), (name, o)
    with pytest.raises(capi.GzDataError):
        sk_ctx.trim_gz(params, to_device(b"not gzip at all, not at all"), mode="se")


# ---- 7 beyond the fixtures' sizes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gm.long_images()) + list(gm.long_bad_images()))
def test_long_images(sk_ctx, monkeypatch, long_runs, name):  # noqa: F811
    """The device against the host run of the same stages and against the model: one wavefront that reads 17 MiB and
    re-bases its bit reader on the way (past16m_*, three walks each: search or count, decode), guesses beyond the cap
    (long_run_*), 6 000 members with runs of empty ones, and the damaged past16m_a"""
    host = long_runs[name]
    if name in gm.long_images():
        image, text, chunk = gm.long_images()[name]
        rc, c, out = inflate(sk_ctx, image, shift=len(name) % 16, capacity=len(text), chunk=chunk, monkeypatch=monkeypatch)
        assert rc == capi.SK_OK, (name, c)
        assert {k: c[k] for k in ("stretches", "stretches_used", "members", "bytes_out")} == \
            {k: host[k] for k in ("stretches", "stretches_used", "members", "bytes_out")}, name
        assert c["members"] == gm.long_want(name)["members"] and text_of(out, c) == text, name
    else:
        image, chunk, want = gm.long_bad_images()[name]
        rc, c, out = inflate(sk_ctx, image, shift=len(name) % 16, capacity=want["bytes_out"] + (1 << 20), chunk=chunk,
                             monkeypatch=monkeypatch)
        assert rc == capi.SK_EDATA, (name, c)
        assert tuple(c[x] for x in KEYS) == tuple(want[x] for x in KEYS) == tuple(host[x] for x in KEYS), (name, c)
        assert (c["stretches"], c["stretches_used"]) == (host["stretches"], host["stretches_used"]), name


def test_text_beyond_4_gib_in_one_member(sk_ctx, monkeypatch, tool, tmp_path):  # noqa: F811
    """(1 << 32) + 70 000 bytes of text in one member: 64-bit text offsets in the chain, the symbols, the resolve granules and
    the CRC pieces; a shift of more than 2^32 bytes in the member's CRC-32; ISIZE modulo 2^32.  The text stays on the device."""
    torch = torch_mod()
    image3, seg, tail = gm.repeated_member(3)
    host = run_host(tool, [(image3, 32768)], tmp_path)[0]  # the guesses hold: not one wavefront for the whole text
    assert host["error"] == 0 and host["text"] == seg * 3 + tail and host["stretches_used"] > 3
    image, seg, tail = gm.repeated_member(1024)
    total = 1024 * gm.SEGMENT + len(tail)
    assert total == (1 << 32) + 70000 and struct.unpack("<I", image[-4:])[0] == 70000
    rc, c, out = inflate(sk_ctx, image, capacity=total, monkeypatch=monkeypatch)
    assert rc == capi.SK_OK, c
    assert (c["members"], c["bytes_out"], c["error"]) == (1, total, 0) and c["stretches_used"] > 1024
    want = to_device(seg).repeat(64)  # 256 MiB
    for k in range(16):
        assert torch.equal(out[k * want.numel():(k + 1) * want.numel()], want), k
    assert out[1 << 32:].cpu().numpy().tobytes() == tail
    del out, want
    torch.cuda.empty_cache()
    for bad, reason in ((image[:-8] + bytes([image[-8] ^ 1]) + image[-7:], capi.SK_GZ_CRC),
                        (image[:-4] + struct.pack("<I", 70001), capi.SK_GZ_LENGTH)):
        rc, c, out = inflate(sk_ctx, bad, capacity=total, monkeypatch=monkeypatch)
        assert rc == capi.SK_EDATA and (c["error"], c["error_member"], c["error_offset"]) == (reason, 0, 0), c
        del out
        torch.cuda.empty_cache()


def test_gunzip_soak():
    """tests/soak_gunzip.py's slice: what tests/test_gunzip_model.py's dry run of it draws, on the device"""
    import soak_gunzip
    stats = cu.soak_child("soak_gunzip.py", *soak_gunzip.SLICE)
    print("soak_gunzip slice:", stats)
    soak_gunzip.check_slice(stats, soak_gunzip.SLICE[0])
    assert {k: stats[k] for k in soak_gunzip.SLICE_STATS} == soak_gunzip.SLICE_STATS

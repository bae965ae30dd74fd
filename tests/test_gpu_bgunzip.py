"""GPU: BGZF read on the device (sk_bgzf_inflate_device_async / finish, Context.bgunzip, Context.trim_gz) against zlib and
tests/bgunzip_model.py: the project's own writer round trip, every kind of member zlib writes, many members, capacity, bad
arguments, every reason code, .gz in -> .gz out against the plain-text trim, a slice of tests/soak_bgunzip.py, and the legal
streams zlib never writes (tests/foreign_images.py): constructed, drawn and bad, which tests/test_bgunzip_host.py runs
through the same source on the host."""
import ctypes as C
import gzip

import pytest

import bgunzip_model as bm
import cli_util as cu
import foreign_images as fi
import trim_model as tm
from bgzf_raw import SENTINEL, to_device, torch_mod, upload
from sickle_amd import capi
from test_fastq_api import golden_texts
from test_gz_inflater import _encoder_inputs

pytestmark = pytest.mark.gpu
GUARD = 64


def inflate(ctx, image, shift=0, capacity=None, count_only=False, ws=None, surround=None):
    """One async + finish on raw pointers; `out` is capacity + GUARD bytes of SENTINEL, and the guard is checked here, in
    every test.  capacity None: what the model says the text needs.  -> (rc, counts, out tensor narrowed to capacity)"""
    torch = torch_mod()
    L = capi.lib()
    keep, ptr = upload(image, shift, surround=surround)  # surround: what lies around the image (bgzf_raw.upload)
    need = L.sk_bgzf_inflate_workspace_bytes(len(image))
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert ws.numel() >= need
    cap = bm.bgunzip(image)["bytes_out"] if capacity is None else capacity
    out = torch.full((cap + GUARD,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc = L.sk_bgzf_inflate_device_async(ctx._h, ptr if len(image) else None, len(image), None if count_only else out.data_ptr(),
                                        0 if count_only else cap, ws.data_ptr(), ws.numel(), None)
    assert rc == capi.SK_OK, L.sk_last_error(ctx._h)
    c = capi.BgzfInflateCounts()
    rc = L.sk_bgzf_inflate_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c))
    del keep
    assert bool((out[cap:] == SENTINEL).all()), "bytes of out at or beyond the capacity were written"
    return rc, c.as_dict(), out[:cap]


def text_of(out, counts):
    return out[:counts["bytes_out"]].cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def images():
    return bm.images()


# ---- 1 the project's own writer ------------------------------------------------------------------------------------
def test_round_trip_of_the_device_writer(sk_ctx):
    for name, data in _encoder_inputs().items():
        for eof in (False, True):
            image = sk_ctx.bgzf(to_device(data), eof=eof).cpu().numpy().tobytes()
            members = (len(data) + 65279) // 65280 + eof
            for shift in range(16):
                rc, c, out = inflate(sk_ctx, image, shift=shift, capacity=len(data))
                assert rc == capi.SK_OK, (name, eof, shift, c)
                assert (c["bytes_in"], c["members"], c["bytes_out"], c["error"]) == (len(image), members, len(data), 0)
                assert text_of(out, c) == data, (name, eof, shift)


# ---- 2 what zlib writes --------------------------------------------------------------------------------------------
def test_every_kind_of_member(sk_ctx, images):
    for name, (image, text) in images.items():
        rc, c, out = inflate(sk_ctx, image, shift=len(name) % 16)
        assert rc == capi.SK_OK, (name, c)
        assert c["members"] == bm.bgunzip(image)["members"] and c["bytes_out"] == len(text), name
        assert text_of(out, c) == text, name
    assert sk_ctx.bgunzip(to_device(images["all"][0])).cpu().numpy().tobytes() == images["all"][1]


# ---- 2b what zlib never writes -------------------------------------------------------------------------------------
def test_foreign_members(sk_ctx):
    """Every constructed member singly, and all of them in one image with EOF members between some: on the device the
    tables are built by the 64 lanes block after block, thousands of times a member in tiny_blocks_*"""
    for name, (image, text) in fi.foreign_images("bgzf").items():
        want = fi.expected("bgzf")[name]
        rc, c, out = inflate(sk_ctx, image, shift=len(name) % 16, capacity=len(text))
        assert rc == capi.SK_OK, (name, c)
        assert (c["error"], c["members"], c["bytes_out"]) == (0, want["members"], len(text)), (name, c)
        assert text_of(out, c) == text, name
    image, text = fi.foreign_images("bgzf")["foreign_members"]
    assert sk_ctx.bgunzip(to_device(image)).cpu().numpy().tobytes() == text


@pytest.mark.parametrize("count", [64, 65])
def test_foreign_drawn(sk_ctx, count):
    """Drawn members around the wave: drawn texts, token streams, block cuts, code lengths, 16/17/18 spellings, padding"""
    image, text, features = fi.drawn_members("bgzf", fi.WAVE_SEEDS[count])
    rc, c, out = inflate(sk_ctx, image, shift=count % 16, capacity=len(text))
    assert rc == capi.SK_OK, c
    assert (c["error"], c["members"], c["bytes_out"]) == (0, count, len(text)), c
    assert text_of(out, c) == text


def test_foreign_bad(sk_ctx):
    """Every constructed bad member at index 0, in the middle and last: reason, member and offset exactly.  The two of
    fi.PRECEDENCE state ISIZE 0 and are SK_GZ_LENGTH: the literal in front of the failing match is the first token to fail."""
    reasons = {name: reason for name, (m, reason) in fi.foreign_bad("bgzf").items()}
    for k, (name, image) in enumerate(fi.bad_images("bgzf").items()):
        want = fi.bad_expected("bgzf")[name]
        rc, c, out = inflate(sk_ctx, image, shift=k % 16, capacity=want["bytes_out"])
        assert rc == capi.SK_EDATA, name
        assert (c["error"], c["error_member"], c["error_offset"], c["members"], c["bytes_out"]) == \
            (want["error"], want["error_member"], want["error_offset"], want["members"], want["bytes_out"]), (name, c)
        assert c["error"] == reasons[name.rsplit("@", 1)[0]], name


def test_empty_image(sk_ctx):
    rc, c, out = inflate(sk_ctx, b"")
    assert rc == capi.SK_OK and (c["members"], c["bytes_out"], c["error"]) == (0, 0, 0)
    assert sk_ctx.bgunzip(to_device(b"x")[:0]).numel() == 0


# ---- 3 many members ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_many_small_members(sk_ctx, count):
    """Around the wave, around the scan's chunk of 256 members, and one count above the inflate kernel's grid of 4096."""
    image, text = bm.small_members(count)
    assert gzip.decompress(image) == text
    rc, c, out = inflate(sk_ctx, image, shift=count % 16)
    assert rc == capi.SK_OK and c["members"] == count
    assert text_of(out, c) == text


# ---- 4 capacity ----------------------------------------------------------------------------------------------------
def test_capacity(sk_ctx, images):
    for name in ("level6", "all", "one_byte"):
        image, text = images[name]
        need = len(text)
        rc, c, out = inflate(sk_ctx, image, capacity=need - 1)
        assert rc == capi.SK_ESPACE and c["bytes_out"] == need and c["error"] == 0
        assert bool((out == SENTINEL).all()), "out was written although the text does not fit"
        rc, c, out = inflate(sk_ctx, image, capacity=need)
        assert rc == capi.SK_OK and text_of(out, c) == text
        rc, c, out = inflate(sk_ctx, image, count_only=True)
        assert rc == capi.SK_OK and c["bytes_out"] == need and bool((out == SENTINEL).all())
    with pytest.raises(capi.TrimError) as e:
        image = to_device(images["level6"][0])
        ws = torch_mod().empty(capi.lib().sk_bgzf_inflate_workspace_bytes(image.numel()), dtype=torch_mod().uint8, device="cuda")
        o = torch_mod().empty(64, dtype=torch_mod().uint8, device="cuda")
        sk_ctx.bgzf_inflate_device_async(image.data_ptr(), image.numel(), o.data_ptr(), 40, ws.data_ptr(), ws.numel())
        sk_ctx.bgzf_inflate_device_finish(ws.data_ptr())
    assert e.value.rc == capi.SK_ESPACE and e.value.counts["bytes_out"] == len(images["level6"][1])


# ---- 5 bad arguments -----------------------------------------------------------------------------------------------
def test_bad_arguments_enqueue_nothing(sk_ctx, images):
    torch = torch_mod()
    L = capi.lib()
    data, text = images["level6"]
    image = to_device(data)
    ws_bytes = L.sk_bgzf_inflate_workspace_bytes(len(data))
    ws = torch.full((ws_bytes + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = torch.full((len(text) + 32,), SENTINEL, dtype=torch.uint8, device="cuda")

    def call(ctx=sk_ctx._h, img=image.data_ptr(), n=len(data), o=out.data_ptr(), capacity=len(text), wsp=ws.data_ptr(),
             wsb=ws_bytes):
        return L.sk_bgzf_inflate_device_async(ctx, img, n, o, capacity, wsp, wsb, None)

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
    assert L.sk_bgzf_inflate_device_finish(None, ws.data_ptr(), None, C.byref(capi.BgzfInflateCounts())) == capi.SK_EINVAL
    assert call() == capi.SK_OK
    c = capi.BgzfInflateCounts()
    assert L.sk_bgzf_inflate_device_finish(sk_ctx._h, ws.data_ptr(), None, C.byref(c)) == capi.SK_OK
    assert out[:c.bytes_out].cpu().numpy().tobytes() == text and bool((out[c.bytes_out:] == SENTINEL).all())


# ---- 6 errors ------------------------------------------------------------------------------------------------------
def test_every_reason_at_every_place(sk_ctx, images):
    """The images of tests/test_bgunzip_host.py's sanitizer run: each SK_GZ_* reason at member 0, in the middle and last,
    two bad members, plain gzip, garbage, cuts.  The verdict is the model's, and the same context and workspace take a
    valid image right after each."""
    torch = torch_mod()
    bad = bm.bad_images()
    good, good_text = images["fq_head"]
    ws = torch.empty(capi.lib().sk_bgzf_inflate_workspace_bytes(max(len(i) for i in bad.values())), dtype=torch.uint8, device="cuda")
    seen = set()
    for k, (name, image) in enumerate(bad.items()):
        want = bm.bgunzip(image)
        rc, c, out = inflate(sk_ctx, image, shift=k % 16, ws=ws)
        assert rc == capi.SK_EDATA, name
        assert (c["error"], c["error_member"], c["error_offset"], c["members"], c["bytes_out"]) == \
            (want["error"], want["error_member"], want["error_offset"], want["members"], want["bytes_out"]), name
        seen.add(c["error"])
        rc, c, out = inflate(sk_ctx, good, ws=ws)
        assert rc == capi.SK_OK and text_of(out, c) == good_text, name
    assert seen == {capi.SK_GZ_HEADER, capi.SK_GZ_TRUNCATED, capi.SK_GZ_DEFLATE, capi.SK_GZ_LENGTH, capi.SK_GZ_CRC}
    rc, c, out = inflate(sk_ctx, bad["plain_gzip"])
    assert (rc, c["error"], c["error_member"], c["error_offset"]) == (capi.SK_EDATA, capi.SK_GZ_HEADER, 0, 0)
    rc, c, out = inflate(sk_ctx, bad["two_bad"])
    assert (c["error"], c["error_member"]) == (capi.SK_GZ_CRC, 1)
    # counting sees the framing, not the streams; too small an out decodes nothing, and SK_EDATA still comes first
    rc, c, out = inflate(sk_ctx, bad["crc@1"], count_only=True)
    assert rc == capi.SK_OK and c["error"] == 0
    rc, c, out = inflate(sk_ctx, bad["garbage_after"], capacity=1)
    assert rc == capi.SK_EDATA and c["error"] == capi.SK_GZ_HEADER and bool((out == SENTINEL).all())
    with pytest.raises(capi.GzDataError) as e:
        sk_ctx.bgunzip(to_device(bad["crc@1"]))
    assert (e.value.reason, e.value.member) == (capi.SK_GZ_CRC, 1)
    with pytest.raises(capi.GzDataError) as e:
        sk_ctx.bgunzip(to_device(bad["plain_gzip"]))
    assert (e.value.reason, e.value.member, e.value.offset) == (capi.SK_GZ_HEADER, 0, 0)


# ---- 7 .gz in, .gz out ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgunzip_chain")
    cu.prepare_inputs(d)
    cu.prepare_long_inputs(d)
    return d


def _gz_runs():
    out = []
    for name, rec in tm.golden_runs():
        if name in tm.UNREPLAYABLE:
            continue
        out.append(pytest.param(name, rec, id=name))
    return out


@pytest.mark.parametrize("name,rec", _gz_runs())
def test_trim_gz_equals_the_plain_text_trim(sk_ctx, workdir, name, rec):
    """The golden inputs bgzipped by member(): trim_gz's images inflate to what trim_fastq gives on the plain text (which
    tests/test_gpu_fastq.py holds against the reference's recorded files)."""
    mode, texts, files = golden_texts(rec["argv"], workdir)
    params = capi.make_params(*tm.run_params(rec["argv"]))
    tt = [to_device(t) for t in texts]
    want, counts = sk_ctx.trim_fastq(params, tt[0], tt[1] if len(tt) > 1 else None, mode=mode)
    zz = [to_device(bm.bgzip(t, level=1 + k)) for k, t in enumerate(texts)]
    got, counts2 = sk_ctx.trim_gz(params, zz[0], zz[1] if len(zz) > 1 else None, mode=mode)
    assert counts2 == counts
    for o in range(3):
        assert (got[o] is None) == (want[o] is None)
        if want[o] is not None:
            assert gzip.decompress(got[o].cpu().numpy().tobytes()) == want[o].cpu().numpy().tobytes(), (name, o)


def test_trim_gz_single_end(sk_ctx, workdir):
    """The first mates of the golden paired inputs as a single-end file, through trim_gz and through trim_fastq."""
    name, rec = next((n, r) for n, r in tm.golden_runs() if n not in tm.UNREPLAYABLE)
    text = golden_texts(rec["argv"], workdir)[1][0]
    params = capi.make_params(*tm.run_params(rec["argv"]))
    want, counts = sk_ctx.trim_fastq(params, to_device(text), mode="se")
    got, counts2 = sk_ctx.trim_gz(params, to_device(bm.bgzip(text, block=30000)), mode="se")
    assert counts2 == counts and got[1] is None and got[2] is None
    assert gzip.decompress(got[0].cpu().numpy().tobytes()) == want[0].cpu().numpy().tobytes()


def test_bgunzip_soak():
    """tests/soak_bgunzip.py's slice: what tests/test_bgunzip_model.py's dry run of it draws, on the device"""
    import soak_bgunzip
    stats = cu.soak_child("soak_bgunzip.py", *soak_bgunzip.SLICE)
    print("soak_bgunzip slice:", stats)
    soak_bgunzip.check_slice(stats, soak_bgunzip.SLICE[0])
    assert {k: stats[k] for k in soak_bgunzip.SLICE_STATS} == soak_bgunzip.SLICE_STATS

"""GPU: BGZF on the device (sk_bgzf_device_async / finish, Context.bgzf, Context.trim_fastq_gz) against
tests/cpu_shim/gpu_deflate_sim, the committed statement of the member image, against zlib, and, chained behind the FASTQ
trim, against the reference's recorded output files."""
import ctypes as C
import gzip
import hashlib
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import cli_util as cu
import trim_model as tm
from bgzf_raw import BLOCK, EOF, SENTINEL, image_of, raw, to_device, torch_mod, upload, walk, word
from sickle_amd import capi
from test_fastq_api import golden_texts
from test_gz_inflater import SIM, TEXT, _encoder_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    subprocess.run(["make", "-s", "-C", os.path.join(cu.ROOT, "tests", "cpu_shim"), "all"], check=True)
    d = tmp_path_factory.mktemp("bgzf_gpu")
    images = {}
    for name, data in _encoder_inputs().items():
        src = str(d / (name + ".txt"))
        open(src, "wb").write(data)
        images[name] = subprocess.run([SIM, src], capture_output=True, check=True).stdout
    return images


# ---- 1 byte identity ---------------------------------------------------------------------------------------------
def test_image_equals_the_sim_at_every_alignment(sk_ctx, sim):
    for name, data in _encoder_inputs().items():
        assert len(data) >= 1
        blocks = (len(data) + BLOCK - 1) // BLOCK
        for shift in range(16):
            for eof in (False, True):
                rc, c, out = raw(sk_ctx, data, eof, shift=shift)
                assert rc == capi.SK_OK, (name, shift)
                got = image_of(out, c)
                assert got == sim[name] + (EOF if eof else b""), (name, shift, eof)
                assert (c["bytes_in"], c["blocks"]) == (len(data), blocks)
                if shift == 0:
                    assert gzip.decompress(got) == data, name
                    assert walk(got) == blocks + eof


def test_empty_text(sk_ctx):
    rc, c, out = raw(sk_ctx, b"", False)
    assert rc == capi.SK_OK and image_of(out, c) == b"" and c["blocks"] == 0
    rc, c, out = raw(sk_ctx, b"", True)
    assert rc == capi.SK_OK and image_of(out, c) == EOF and c["blocks"] == 0
    assert sk_ctx.bgzf(to_device(b"x")[:0]).cpu().numpy().tobytes() == EOF


# ---- 2 the length on the device ----------------------------------------------------------------------------------
def test_device_side_length_and_validity(sk_ctx, sim):
    for name in ("fastq", "block_plus_one", "one", "random"):
        data = _encoder_inputs()[name]
        for bound in (len(data) + 1, len(data) + 3 * BLOCK + 17):
            rc, c, out = raw(sk_ctx, data, True, shift=5, bound=bound, dev_len=len(data))
            assert rc == capi.SK_OK and image_of(out, c) == sim[name] + EOF, (name, bound)
            assert c["bytes_in"] == len(data)
        rc, c, out = raw(sk_ctx, data, True, bound=len(data) + 100, dev_len=len(data), valid=1)
        assert rc == capi.SK_OK and image_of(out, c) == sim[name] + EOF
        for eof in (False, True):
            rc, c, out = raw(sk_ctx, data, eof, bound=len(data) + 100, dev_len=len(data), valid=0)
            assert rc == capi.SK_OK and image_of(out, c) == (EOF if eof else b"")
            assert (c["bytes_in"], c["blocks"], c["stored_blocks"]) == (0, 0, 0)
    # a zero length on the device, no validity word
    rc, c, out = raw(sk_ctx, _encoder_inputs()["fastq"], True, dev_len=0)
    assert rc == capi.SK_OK and image_of(out, c) == EOF


# ---- 3 capacity and bad arguments --------------------------------------------------------------------------------
def test_capacity_one_byte_short(sk_ctx, sim):
    for name in ("fastq", "random", "one"):
        data = _encoder_inputs()[name]
        for eof in (False, True):
            need = len(sim[name]) + (28 if eof else 0)
            rc, c, out = raw(sk_ctx, data, eof, capacity=need - 1)
            assert rc == capi.SK_ESPACE and c["bytes_out"] == need
            assert bool((out == SENTINEL).all()), "out was written although the image does not fit"
            rc, c, out = raw(sk_ctx, data, eof, capacity=need)  # the exact fit
            assert rc == capi.SK_OK and image_of(out, c) == sim[name] + (EOF if eof else b"")
    with pytest.raises(capi.TrimError) as e:
        n = 1000
        ws = torch_mod().empty(capi.lib().sk_bgzf_workspace_bytes(n), dtype=torch_mod().uint8, device="cuda")
        t, o = to_device(TEXT[:n]), torch_mod().empty(64, dtype=torch_mod().uint8, device="cuda")
        sk_ctx.bgzf_device_async(t.data_ptr(), n, o.data_ptr(), 40, ws.data_ptr(), ws.numel())
        sk_ctx.bgzf_device_finish(ws.data_ptr())
    assert e.value.rc == capi.SK_ESPACE and e.value.counts["bytes_out"] > 40


def test_bad_arguments_enqueue_nothing(sk_ctx):
    torch = torch_mod()
    L = capi.lib()
    n = 3 * BLOCK
    text = to_device(TEXT[:n])
    ws_bytes = L.sk_bgzf_workspace_bytes(n)
    ws = torch.full((ws_bytes + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    cap = L.sk_bgzf_bound(n, 1)
    out = torch.full((cap + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    w = torch.zeros(4, dtype=torch.int64, device="cuda")
    good = capi.BgzfInput(text.data_ptr(), n, None, None)

    def call(ctx=sk_ctx._h, inp=good, o=out.data_ptr(), capacity=cap, flags=1, wsp=ws.data_ptr(), wsb=ws_bytes):
        return L.sk_bgzf_device_async(ctx, C.byref(inp) if inp is not None else None, o, capacity, flags, wsp, wsb, None)

    assert call(ctx=None) == capi.SK_EINVAL
    assert call(inp=None) == capi.SK_EINVAL
    assert call(o=out.data_ptr() + 8) == capi.SK_EINVAL
    assert call(wsp=ws.data_ptr() + 8) == capi.SK_EINVAL
    assert call(wsp=None) == capi.SK_EINVAL
    assert call(wsb=ws_bytes - 1) == capi.SK_EINVAL
    assert call(flags=2) == capi.SK_EINVAL
    assert call(inp=capi.BgzfInput(text.data_ptr(), n, w.data_ptr() + 4, None)) == capi.SK_EINVAL
    assert call(inp=capi.BgzfInput(text.data_ptr(), n, None, w.data_ptr() + 4)) == capi.SK_EINVAL
    assert call(inp=capi.BgzfInput(None, n, None, None)) == capi.SK_EINVAL
    assert call(o=None) == capi.SK_EINVAL
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all()), "a refused call enqueued something"
    assert L.sk_bgzf_device_finish(None, ws.data_ptr(), None, C.byref(capi.BgzfCounts())) == capi.SK_EINVAL
    assert call() == capi.SK_OK
    c = capi.BgzfCounts()
    assert L.sk_bgzf_device_finish(sk_ctx._h, ws.data_ptr(), None, C.byref(c)) == capi.SK_OK
    assert gzip.decompress(out[:c.bytes_out].cpu().numpy().tobytes()) == TEXT[:n]


# ---- 4 stored blocks, many blocks --------------------------------------------------------------------------------
def test_stored_blocks(sk_ctx):
    inputs = _encoder_inputs()
    rc, c, out = raw(sk_ctx, inputs["random"], True, shift=3)
    assert rc == capi.SK_OK and c["stored_blocks"] == c["blocks"] == 4
    assert c["bytes_out"] == len(inputs["random"]) + 31 * 4 + 28
    rc, c, out = raw(sk_ctx, inputs["same"], True)
    assert rc == capi.SK_OK and c["stored_blocks"] == 0 and c["blocks"] == 4


def test_many_blocks(sk_ctx):
    """More blocks than one round of the block kernel's grid (1280), through Context.bgzf."""
    data = TEXT * 130
    assert len(data) > 1280 * BLOCK
    blob = sk_ctx.bgzf(to_device(data)).cpu().numpy().tobytes()
    assert gzip.decompress(blob) == data and len(blob) < 0.5 * len(data)
    assert walk(blob) == (len(data) + BLOCK - 1) // BLOCK + 1


# ---- 5 chained behind the FASTQ trim -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("bgzf_chain")
    cu.prepare_inputs(d)
    cu.prepare_long_inputs(d)
    return d


def chain_raw(ctx, params, texts, mode):
    """The trim and one BGZF call per output of the mode enqueued through the raw-pointer methods on the NULL stream, and
    only then the finishes.  -> (rc of the trim's finish, its counts, [(rc, counts, image bytes) or None])."""
    torch = torch_mod()
    L = capi.lib()
    tt = [to_device(t) for t in texts]
    sizes = [len(t) for t in texts]
    ws_bytes = L.sk_trim_fastq_workspace_bytes(sum(sizes), params.trunc_n)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device="cuda")
    cap = sum(sizes) + 2
    bound, zws_bytes = L.sk_bgzf_bound(cap, 1), L.sk_bgzf_workspace_bytes(cap)
    used = {"se": (0,), "pe_split": (0, 1, 2), "pe_interleaved": (0, 2)}[mode]
    outs, bufs = [capi.FastqOutput() for _ in range(3)], {}
    for o in used:
        t = torch.full((max(cap, 16),), ord("@"), dtype=torch.uint8, device="cuda")  # never compressed unless written
        img = torch.full((bound + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
        zws = torch.empty(zws_bytes, dtype=torch.uint8, device="cuda")
        bufs[o] = (t, img, zws)
        outs[o] = capi.FastqOutput(t.data_ptr(), cap, None, 0)
    ctx.trim_fastq_device_async(params, [t.data_ptr() if t.numel() else None for t in tt], sizes, outs, ws.data_ptr(),
                                ws_bytes, mode=mode)
    for o in used:
        t, img, zws = bufs[o]
        nbytes, written = ctx.trim_fastq_output_words(ws.data_ptr(), o)
        ctx.bgzf_device_async(t.data_ptr(), cap, img.data_ptr(), bound, zws.data_ptr(), zws_bytes, eof=True,
                              bytes_dev_ptr=nbytes, valid_dev_ptr=written)
    res = [None] * 3
    for o in used:
        c = capi.BgzfCounts()
        rc = L.sk_bgzf_device_finish(ctx._h, bufs[o][2].data_ptr(), None, C.byref(c))
        res[o] = (rc, c.as_dict(), image_of(bufs[o][1], c.as_dict()) if rc == capi.SK_OK else None)
    fc = capi.FastqCounts()
    rc = L.sk_trim_fastq_device_finish(ctx._h, ws.data_ptr(), None, C.byref(fc))
    return rc, fc.as_dict(), res


# the runs a trim can replay (tests/test_gpu_fastq.py skips the others by name)
REPLAYABLE = [pytest.param(name, rec, id=name) for name, rec in tm.golden_runs() if name not in tm.UNREPLAYABLE]


@pytest.mark.parametrize("name,rec", REPLAYABLE)
def test_reference_runs_to_gz(sk_ctx, workdir, name, rec):
    """The input files uploaded byte for byte, trimmed and compressed on the device with no wait in between: every image
    inflates to the recorded output file of the reference."""
    mode, texts, files = golden_texts(rec["argv"], workdir)
    params = capi.make_params(*tm.run_params(rec["argv"]))
    rc, counts, res = chain_raw(sk_ctx, params, texts, mode)
    assert rc == capi.SK_OK
    tt = [to_device(t) for t in texts]
    images, counts2 = sk_ctx.trim_fastq_gz(params, tt[0], tt[1] if len(tt) > 1 else None, mode=mode)
    assert counts2 == counts
    for fname, want in rec["outputs"].items():
        o = files[fname]
        assert res[o][0] == capi.SK_OK
        text = gzip.decompress(res[o][2])
        assert (hashlib.md5(text).hexdigest(), len(text)) == (want["md5"], want["size"]), fname
        assert res[o][1]["bytes_in"] == counts["bytes"][o] == want["size"]
        walk(res[o][2])
        assert images[o].cpu().numpy().tobytes() == res[o][2], fname
    for o in range(3):
        assert (images[o] is None) == (res[o] is None)


BAD_FORMAT = b"@a\nACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIII\n@\nA\n+\nI\n"
BAD_RANGE = b"@range\n" + b"ACGT" * 6 + b"\n+\n" + b"I" * 23 + b" \n"


def test_chain_after_an_upstream_error(sk_ctx):
    """A malformed record and an out-of-range quality raise as trim_fastq does; through the raw calls the images behind
    such a trim are empty (the EOF member only), whatever the text buffers held."""
    params = capi.make_params()
    with pytest.raises(capi.FormatError) as e:
        sk_ctx.trim_fastq_gz(params, to_device(BAD_FORMAT))
    assert (e.value.reason, e.value.input, e.value.record) == (capi.SK_FQ_ID_SHORT, 0, 1)
    with pytest.raises(capi.RangeError):
        sk_ctx.trim_fastq_gz(params, to_device(BAD_RANGE))
    for text, want in ((BAD_FORMAT, capi.SK_EFORMAT), (BAD_RANGE, capi.SK_ERANGE)):
        for mode in ("se", "pe_interleaved"):
            rc, counts, res = chain_raw(sk_ctx, params, [text * (1 if mode == "se" else 2)], mode)
            assert rc == want
            for r in res:
                if r is not None:
                    assert r[0] == capi.SK_OK and r[2] == EOF and r[1]["blocks"] == 0
    # and a good text through the same path, for contrast
    good = BAD_FORMAT[:BAD_FORMAT.index(b"@\n")]
    images, counts = sk_ctx.trim_fastq_gz(params, to_device(good))
    assert gzip.decompress(images[0].cpu().numpy().tobytes()) == good and images[1] is None and images[2] is None


# ---- 6 beyond 4 GiB ----------------------------------------------------------------------------------------------
def test_text_beyond_4_gib(sk_ctx):
    """A text just over 2^32 bytes built on the device; the image is inflated on the host member by member and compared
    by hash, so every 64-bit offset (text, slots, image) is exercised once."""
    torch = torch_mod()
    reps = (1 << 32) // len(TEXT) + 1
    total = reps * len(TEXT)
    assert total > 1 << 32
    big = to_device(TEXT).repeat(reps)
    image = sk_ctx.bgzf(big)
    del big
    torch.cuda.empty_cache()
    blob = image.cpu().numpy()
    del image
    assert blob.size < 0.5 * total and blob[-28:].tobytes() == EOF
    want = hashlib.md5()
    for _ in range(reps):
        want.update(TEXT)
    got, size, at, members = hashlib.md5(), 0, 0, 0
    view = memoryview(blob)
    while at < blob.size:
        assert blob[at] == 0x1f and blob[at + 1] == 0x8b and blob[at + 12] == ord("B")
        m = int(blob[at + 16]) + (int(blob[at + 17]) << 8) + 1
        piece = zlib.decompress(view[at + 18:at + m - 8], -15)
        crc, isize = struct.unpack_from("<II", view, at + m - 8)
        assert (zlib.crc32(piece), len(piece)) == (crc, isize), members
        got.update(piece)
        size += len(piece)
        at += m
        members += 1
    assert at == blob.size and size == total and members == (total + BLOCK - 1) // BLOCK + 1
    assert got.hexdigest() == want.hexdigest()


# ---- 7 soak ------------------------------------------------------------------------------------------------------
BGZF_SOAK = 60  # iterations, one comparison each


def test_bgzf_soak(sk_ctx):
    """tests/soak_bgzf.py: drawn texts (stored and deflated blocks side by side, 2 047 .. 5 000 lines a block, copy sources
    32 768 bytes back, skewed alphabets, lengths around multiples of the block) at a drawn shift, EOF flag, bound,
    device-side length, validity word and capacity, against the sim's image."""
    import soak_bgzf
    assert soak_bgzf.run(BGZF_SOAK, 2028, verbose=False) == BGZF_SOAK

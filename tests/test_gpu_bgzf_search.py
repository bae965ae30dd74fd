"""GPU: the searching BGZF encoder (sk_bgzf_device_async with SK_BGZF_SEARCH; search=True in Context.bgzf, trim_fastq_gz
and trim_gz) against tests/bgzf_search/search_host, the same phases run on the host lane after lane: the image is a
function of the text alone, so the two agree byte for byte."""
import ctypes as C
import gzip

import pytest

import bgzf_search_texts as st
from bgzf_raw import BLOCK, EOF, SENTINEL, image_of, to_device, torch_mod, upload, word
from sickle_amd import capi

pytestmark = pytest.mark.gpu

SEARCH = capi.SK_BGZF_SEARCH | capi.SK_BGZF_EOF


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """name -> (text, the host program's image with the EOF member)"""
    st.build()
    d = tmp_path_factory.mktemp("bgzf_search_gpu")
    texts = dict(st.edge_texts())
    texts.update(st.fastq_texts())
    texts["synth"] = st.synth_text(3)
    return {name: (data, st.host_image(data, d, name, "eof")) for name, data in texts.items()}


def raw(ctx, text, flags=SEARCH, shift=0, bound=None, dev_len=None, valid=None, capacity=None, ws=None, surround=None):
    """One async + finish on raw pointers, `out` pre-filled with SENTINEL (bgzf_raw.raw with flags and a workspace that
    can be handed in) -> (rc of the async call or of finish, counts, out tensor)."""
    torch = torch_mod()
    L = capi.lib()
    nbytes = len(text) if bound is None else bound
    keep, ptr = upload(text, shift, room=nbytes - len(text), surround=surround)
    cap = L.sk_bgzf_bound(nbytes, flags) if capacity is None else capacity
    out = torch.full((cap + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    if ws is None:
        ws = torch.empty(max(L.sk_bgzf_workspace_bytes_flags(nbytes, flags), 16), dtype=torch.uint8, device="cuda")
    wl, wv = None if dev_len is None else word(dev_len), None if valid is None else word(valid)
    inp = capi.BgzfInput(ptr, nbytes, None if wl is None else wl.data_ptr(), None if wv is None else wv.data_ptr())
    rc = L.sk_bgzf_device_async(ctx._h, C.byref(inp), out.data_ptr(), cap, flags, ws.data_ptr(), ws.numel(), None)
    if rc != capi.SK_OK:
        torch.cuda.synchronize()
        return rc, None, out
    c = capi.BgzfCounts()
    rc = L.sk_bgzf_device_finish(ctx._h, ws.data_ptr(), None, C.byref(c))
    del keep
    return rc, c.as_dict(), out


# ---- 1 edge texts and fixtures ------------------------------------------------------------------------------------
def test_image_equals_the_host_program(sk_ctx, host):
    for name, (data, want) in host.items():
        rc, c, out = raw(sk_ctx, data)
        assert rc == capi.SK_OK, name
        got = image_of(out, c)
        assert got == want, name
        assert gzip.decompress(got) == data, name
        assert (c["bytes_in"], c["blocks"]) == (len(data), (len(data) + BLOCK - 1) // BLOCK), name
    data, want = host["test.fastq"]
    rc, c, out = raw(sk_ctx, data, flags=capi.SK_BGZF_SEARCH)  # without the EOF member
    assert rc == capi.SK_OK and image_of(out, c) == want[:-len(EOF)]
    assert sk_ctx.bgzf(to_device(data), search=True).cpu().numpy().tobytes() == want
    assert len(sk_ctx.bgzf(to_device(data)).cpu().numpy().tobytes()) > len(want)


@pytest.mark.parametrize("shift", [0, 1, 7, 15])
def test_three_blocks_at_an_alignment(sk_ctx, host, shift):
    data, want = host["synth"]
    rc, c, out = raw(sk_ctx, data, shift=shift)
    assert rc == capi.SK_OK and image_of(out, c) == want


# ---- 2 more blocks than wavefronts: the table of a wavefront's first block must not reach its second ---------------
def test_stale_table_between_blocks(sk_ctx, tmp_path):
    st.build()
    blocks = 1300
    piece = st.synth_text(16, seed=13)[:16 * BLOCK - 4321]  # the period is no multiple of the block: the blocks differ
    data = (piece * (blocks * BLOCK // len(piece) + 1))[:blocks * BLOCK]
    assert len(data) > 1280 * BLOCK
    want = st.host_image(data, tmp_path, "many", "eof")
    got = sk_ctx.bgzf(to_device(data), search=True).cpu().numpy().tobytes()
    assert len(got) == len(want) and got == want


# ---- 3 chained behind the FASTQ trim ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,names", [("se", ("test.fastq",)), ("pe_split", ("test.f.fastq", "test.r.fastq"))])
def test_chain_inflates_to_the_trimmed_text(sk_ctx, mode, names):
    texts = [to_device(st.fastq_texts()[n]) for n in names]
    params = capi.make_params("sanger", 20, 20)
    second = texts[1] if len(texts) > 1 else None
    plain, counts = sk_ctx.trim_fastq(params, texts[0], second, mode=mode)
    images, counts2 = sk_ctx.trim_fastq_gz(params, texts[0], second, mode=mode, search=True)
    noflag, _ = sk_ctx.trim_fastq_gz(params, texts[0], second, mode=mode)
    assert counts2 == counts
    for o in range(3):
        assert (images[o] is None) == (plain[o] is None)
        if plain[o] is not None:
            blob = images[o].cpu().numpy().tobytes()
            assert gzip.decompress(blob) == plain[o].cpu().numpy().tobytes(), o
            assert blob.endswith(EOF) and len(blob) <= noflag[o].numel()
    if mode == "se":  # and from the .gz image, through trim_gz
        again, counts3 = sk_ctx.trim_gz(params, sk_ctx.bgzf(texts[0]), mode=mode, search=True)
        assert counts3 == counts and again[0].cpu().numpy().tobytes() == images[0].cpu().numpy().tobytes()


def test_device_side_length_and_validity(sk_ctx, host):
    data, want = host["test.fastq"]
    for bound in (len(data) + 1, len(data) + 3 * BLOCK + 17):
        rc, c, out = raw(sk_ctx, data, shift=5, bound=bound, dev_len=len(data))
        assert rc == capi.SK_OK and image_of(out, c) == want and c["bytes_in"] == len(data)
    cut = 2 * BLOCK + 123  # bytes_dev shorter than the text that lies there
    rc, c, out = raw(sk_ctx, data, dev_len=cut, valid=1)
    assert rc == capi.SK_OK and c["bytes_in"] == cut and gzip.decompress(image_of(out, c)) == data[:cut]
    rc, c, out = raw(sk_ctx, data, bound=len(data) + 100, dev_len=len(data), valid=0)
    assert rc == capi.SK_OK and image_of(out, c) == EOF and (c["bytes_in"], c["blocks"], c["stored_blocks"]) == (0, 0, 0)


# ---- 4 refusals ---------------------------------------------------------------------------------------------------
def test_capacity_one_byte_short(sk_ctx, host):
    for name in ("test.fastq", "random"):
        data, want = host[name]
        rc, c, out = raw(sk_ctx, data, capacity=len(want) - 1)
        assert rc == capi.SK_ESPACE and c["bytes_out"] == len(want)
        assert bool((out == SENTINEL).all()), "out was written although the image does not fit"
        rc, c, out = raw(sk_ctx, data, capacity=len(want))  # the exact fit
        assert rc == capi.SK_OK and image_of(out, c) == want


def test_the_old_workspace_size_is_refused(sk_ctx, host):
    torch = torch_mod()
    data, _ = host["synth"]
    old = capi.lib().sk_bgzf_workspace_bytes(len(data))
    need = capi.lib().sk_bgzf_workspace_bytes_flags(len(data), SEARCH)
    assert need > old
    for size in (old, need - 1):
        ws = torch.full((size,), SENTINEL, dtype=torch.uint8, device="cuda")
        rc, _, out = raw(sk_ctx, data, ws=ws)
        assert rc == capi.SK_EINVAL
        assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all()), "a refused call enqueued something"
    assert raw(sk_ctx, data, flags=4)[0] == capi.SK_EINVAL and raw(sk_ctx, data, flags=SEARCH | 4)[0] == capi.SK_EINVAL


# ---- 5 the call without the flag is what it was ---------------------------------------------------------------------
def test_no_flag_call_after_a_search_call(sk_ctx, host, tmp_path):
    torch = torch_mod()
    for name in ("test.fastq", "synth", "long_repeat"):
        data, want = host[name]
        today = st.host_image(data, tmp_path, name, "eof", tool=st.PLAIN)
        ws = torch.empty(capi.lib().sk_bgzf_workspace_bytes_flags(len(data), SEARCH), dtype=torch.uint8, device="cuda")
        rc, c, out = raw(sk_ctx, data, ws=ws)
        assert rc == capi.SK_OK and image_of(out, c) == want
        rc, c, out = raw(sk_ctx, data, flags=capi.SK_BGZF_EOF, ws=ws)
        assert rc == capi.SK_OK and image_of(out, c) == today, name
        rc, c, out = raw(sk_ctx, data, ws=ws)
        assert rc == capi.SK_OK and image_of(out, c) == want

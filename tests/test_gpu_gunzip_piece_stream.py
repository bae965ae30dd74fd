"""GPU: Context.trim_gzip_stream, the FASTQ trim in pieces fed by the plain-gzip reader in pieces, against trim_fastq on
the whole text: every golden run with plain gzip in (mate 2 compressed at another level) and FASTQ or BGZF out, a BGZF
image as input, 50 drawn texts of tests/soak_fastq.py's generator at piece sizes from 4 096 to 100 000, and the two
failures that name a parameter, and the golden FASTQ re-encoded by tests/deflate_writer.py's drawn tokenizer and block cutter
through trim_gz and trim_gzip_stream.  The images have small blocks (gunzip_model.small_blocks) and are read with
SK_GZIP_CHUNK = 1024 or 256, so that a piece of a few KB holds several stretches."""
import gzip

import numpy as np
import pytest

import cli_util as cu
import fastq_model as fm
import foreign_images as fi
import gunzip_model as gm
import soak_fastq
import trim_model as tm
from bgzf_raw import EOF, to_device
from sickle_amd import capi
from test_fastq_api import golden_texts

pytestmark = pytest.mark.gpu


def run_stream(stream):
    parts = list(stream)
    return [None if parts[0][o] is None else b"".join(p[o] for p in parts) for o in range(3)], stream


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("gunzip_piece_stream")
    cu.prepare_inputs(d)
    cu.prepare_long_inputs(d)
    return d


@pytest.mark.parametrize("name,rec", [pytest.param(n, r, id=n) for n, r in tm.golden_runs()])
def test_golden_runs(sk_ctx, workdir, monkeypatch, name, rec):
    monkeypatch.setenv("SK_GZIP_CHUNK", "1024")
    mode, texts, _ = golden_texts(rec["argv"], workdir)
    params = capi.make_params(*tm.run_params(rec["argv"]))
    dev = [to_device(t) for t in texts]
    want, counts = sk_ctx.trim_fastq(params, dev[0], dev[1] if len(dev) > 1 else None, mode=mode)
    want = [None if w is None else w.cpu().numpy().tobytes() for w in want]
    longest = max(len(line) for t in texts for line in t.split(b"\n"))
    room = 4 * longest + 65536
    images = [gm.small_blocks(t, level) for t, level in zip(texts, (6, 9))]
    for gz in (False, True):
        got, st = run_stream(sk_ctx.trim_gzip_stream(params, images[0], images[1] if len(images) > 1 else None, mode=mode,
                                                     piece_bytes=100_000, room=room, gz=gz))
        for o in fm.USED[mode]:
            if gz:
                assert gzip.decompress(got[o]) == want[o] and got[o].endswith(EOF) and got[o].count(EOF) == 1, (gz, o)
            else:
                assert got[o] == want[o], (gz, o)
        for key in ("records_in", "records", "bytes", "tail_lines", "dropped_unpaired"):
            assert st.counts[key] == counts[key], key
        assert st.pieces >= max(len(t) for t in texts) // 100_000 + 1  # and the empty closing piece
        assert st.device_bytes > sum(len(i) for i in images)  # the compressed images are resident


def test_bgzf_image_and_failures(sk_ctx, monkeypatch):
    monkeypatch.delenv("SK_GZIP_CHUNK", raising=False)
    pt = ("sanger", 20, 20, False, False)
    params = capi.make_params(*pt)
    text = gm.fastq_text(300_000, 91)
    text = text[:text.rindex(b"\n@") + 1]
    want = fm.expected(pt, [text], "se")["texts"][0]
    bgzf = sk_ctx.bgzf(to_device(text)).cpu().numpy().tobytes()
    got, st = run_stream(sk_ctx.trim_gzip_stream(params, bgzf, piece_bytes=150_000, window_bytes=60_000, gz=False))
    assert got[0] == want and st.pieces >= 3
    plain = gzip.compress(text, 6)
    got, st = run_stream(sk_ctx.trim_gzip_stream(params, plain, piece_bytes=1 << 20, gz=False))
    assert got[0] == want
    with pytest.raises(ValueError, match="trim_gz"):  # the BGZF driver still refuses plain gzip
        sk_ctx.trim_gz_stream(params, plain)
    stored = gm.member(text, 0)  # stored blocks of 65 535 bytes: none ends inside a window of 20 000
    with pytest.raises(capi.GzDataError, match="window_bytes=20000") as e:
        run_stream(sk_ctx.trim_gzip_stream(params, stored, piece_bytes=150_000, window_bytes=20_000, gz=False))
    assert e.value.counts["window_limited"] == 1
    with pytest.raises(capi.TrimError, match="piece_bytes") as e:  # a stretch of ordinary gzip holds far more than 4 096 bytes
        run_stream(sk_ctx.trim_gzip_stream(params, plain, piece_bytes=4096, window_bytes=1 << 20, gz=False))
    assert e.value.rc == capi.SK_ESPACE


def test_foreign_encoding_of_the_golden_fastq(sk_ctx, monkeypatch):
    """tests/golden/inputs/test.fastq as BGZF members and as one plain gzip member of drawn blocks, code lengths, repeats and
    padding: .gz in -> .gz out and the stream in pieces give what trim_fastq gives on the text"""
    monkeypatch.setenv("SK_GZIP_CHUNK", "1024")
    text, bgzf, plain = fi.reencoded_fastq()
    params = capi.make_params("illumina", 20, 20, False, False)
    want, counts = sk_ctx.trim_fastq(params, to_device(text), mode="se")
    want = want[0].cpu().numpy().tobytes()
    assert 0 < len(want) < len(text)
    for image in (bgzf, plain):
        got, counts2 = sk_ctx.trim_gz(params, to_device(image), mode="se")
        assert counts2 == counts and gzip.decompress(got[0].cpu().numpy().tobytes()) == want
        got, st = run_stream(sk_ctx.trim_gzip_stream(params, image, piece_bytes=200_000, gz=False))
        assert got[0] == want and st.pieces >= 4
        for key in ("records_in", "records", "bytes", "tail_lines"):
            assert st.counts[key] == counts[key], key


@pytest.mark.parametrize("group", range(2))
def test_drawn_texts(sk_ctx, monkeypatch, group):
    """25 texts a group, each at a drawn piece size from 4 096 to 100 000 (raised to a fortieth of the text): trim_fastq's
    outputs and counts, or one of its errors.  Where a stretch of the image holds more text than the drawn piece may take,
    the driver's TrimError is checked and the text repeated at a piece size with room for it."""
    monkeypatch.setenv("SK_GZIP_CHUNK", "256")
    rng, grown = np.random.default_rng(2000 + group), 0
    for it in range(25):
        c = soak_fastq.draw(rng)
        texts, mode, pt = c["texts"], c["mode"], tuple(c["params"])
        size = max(int(np.exp(rng.uniform(np.log(4096), np.log(100_000)))), max(len(t) for t in texts) // 40)
        longest = max(len(r) for t in texts for r in t.split(b"\n")) if texts else 0
        want = fm.expected(pt, texts, mode)
        images = [gm.small_blocks(t, 1 + (it + i) % 9) for i, t in enumerate(texts)]
        for attempt in range(4):
            room = 8 * longest + 4096 + 2 * size
            stream = sk_ctx.trim_gzip_stream(capi.make_params(*pt), images[0], images[1] if len(images) > 1 else None, mode=mode,
                                             piece_bytes=size, room=room, gz=False)
            tag = (group, it, mode, size)
            try:
                if want["verdict"] is None and want["range"] is None:
                    got, st = run_stream(stream)
                    for o in fm.USED[mode]:
                        assert got[o] == want["texts"][o], tag
                    assert st.counts["records_in"] == want["records_in"] and st.counts["tail_lines"] == want["tail_lines"], tag
                    assert st.counts["dropped_unpaired"] == want["dropped_unpaired"], tag
                else:
                    with pytest.raises((capi.FormatError, capi.RangeError)):
                        run_stream(stream)
                break
            except capi.TrimError as e:
                # long records and runs: a stretch of this image holds more text than the drawn piece.  The driver does
                # not retry; the error names piece_bytes and tells the need, and the test repeats with room for it
                need = e.counts["bytes_out"]
                assert e.rc == capi.SK_ESPACE and "piece_bytes" in str(e) and need > 0 and attempt < 3, tag
                size = 2 * need + size
                grown += 1
    assert grown < 25  # most of the drawn sizes hold their images' stretches

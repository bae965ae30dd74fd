"""GPU: mode "pe_combo_all" (SK_TRIM_PE_COMBO_ALL, sickle's -M) of the FASTQ text calls, byte for byte against
tests/combo_all_model.py: the whole-text call on raw pointers with sentinels around every output, the chained call, the
pieces, the -a T order, the .gz drivers and 100 drawn texts."""
import ctypes as C
import gzip
import os
import random
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

import cli_util as cu
import combo_all_model as cm
import fastq_model as fm
import trim_model as tm
from bgzf_raw import EOF, to_device
from fastq_raw import SENTINEL, raw, texts_of, torch_mod, untouched
from sickle_amd import capi
from test_fastq_api import golden_texts
from test_fastq_combo_model import COMBO_RUNS, DRAWS, SEED, TRUTH_IN, TRUTH_OUT, drawn_case

pytestmark = pytest.mark.gpu
MODE = cm.MODE
PT = cm.TRUTH_PARAMS
# the reads of test_gpu_fastq.py's planted errors
BAD = {capi.SK_FQ_ID_SHORT: b"@\nACGT\n+\nIIII\n", capi.SK_FQ_ID_NO_AT: b"Xbad\nACGT\n+\nIIII\n",
       capi.SK_FQ_SEQ_EMPTY: b"@bad\n\n+\nIIII\n", capi.SK_FQ_QUAL_EMPTY: b"@bad\nACGT\n+\n\n",
       capi.SK_FQ_LENGTHS: b"@bad\nACGT\n+\nIII\n"}
RANGE_BAD = b"@range\n" + b"ACGT" * 6 + b"\n+\n" + b"I" * 23 + b" \n"


def call(ctx, ptuple, text, cap=None, shift=0):
    """one raw call of the mode, all three outputs given and filled with sentinels -> (rc, counts, keep)"""
    cap = cm.bound(len(text), len(text) // 7 + 1) + 16 if cap is None else cap
    return raw(ctx, capi.make_params(*ptuple), [text], MODE, caps=[cap, 64, 64], rec_caps=[len(text) // 4 + 4, 8, 8], shift=shift)


def check(ctx, ptuple, text, want=None, shift=0):
    """the raw call against the model: counts, every byte of output 0, the index, and outputs 1 and 2 untouched"""
    want = cm.expected(ptuple, text) if want is None else want
    assert want["texts"] is not None
    rc, counts, keep = call(ctx, ptuple, text, shift=shift)
    assert rc == capi.SK_OK, capi.lib().sk_last_error(ctx._h)
    assert counts["records_in"] == want["records_in"] and counts["tail_lines"] == want["tail_lines"]
    assert counts["dropped_unpaired"] == want["dropped_unpaired"]
    n, b = len(want["records"]), len(want["texts"][0])
    assert counts["records"] == [n, 0, 0] and counts["bytes"] == [b, 0, 0]
    got = texts_of(keep, counts)[0]
    assert got == want["texts"][0]
    assert bool((keep[0][0][b:] == SENTINEL).all()) and bool((keep[0][1][n:] == -7).all())
    assert np.array_equal(keep[0][1][:n].cpu().numpy(), np.arange(n))
    untouched(keep[1:])
    return counts, got


# ---- 1 the truth table at every offset of the constant bytes within a granule -----------------------------------------
def test_truth_table_by_hand(sk_ctx):
    _, got = check(sk_ctx, PT, TRUTH_IN)
    assert got == b"".join(TRUTH_OUT)


@pytest.mark.parametrize("qualtype", sorted(cm.Q_BYTE))
def test_truth_table_name_lengths(sk_ctx, qualtype):
    """names of 2..34 bytes: the six constant bytes start at every offset of a 16-byte output granule and straddle its
    end; 1, 3 and 4 pairs give exactly 2, 6 and 8 records: the ranks between NREAL and a lane's 8 reads emit nothing"""
    ptuple = (qualtype,) + PT[1:]
    q = bytes([cm.Q_BYTE[qualtype]])
    starts = set()
    for name_len in range(2, 35):
        for pairs in (1, 3, 4):
            text = cm.truth_text(pairs, name_len, qualtype, crlf_names=name_len % 5 == 0)
            want = cm.expected(ptuple, text)
            counts, got = check(sk_ctx, ptuple, text, want, shift=name_len % 16)
            assert counts["records"][0] == 2 * pairs
            assert got.count(b"\nN\n+\n" + q + b"\n") == sum((0, 1, 1, 2)[c] for c in want["classes"])
            at = 0
            for r, c in zip(want["records"], want["cuts"]):
                if c[1] < 0:
                    starts.add((at + len(r) - 6) % 16)
                at += len(r)
    assert starts == set(range(16))


# ---- 2 three emit blocks of N records, a gather chunk of about 900 records ---------------------------------------------
FAILED_PAIR = b"@a\nA\n+\n#\n" * 2
KEPT_PAIR = b"@a\nACGTACGTAC\n+\nIIIIIIIIII\n" * 2


@pytest.mark.parametrize("kept_at", [None, 0, 1024, 2048])
def test_three_blocks_of_n_records(sk_ctx, kept_at):
    pairs = [FAILED_PAIR] * 2049
    if kept_at is not None:
        pairs[kept_at] = KEPT_PAIR
    text = b"".join(pairs)
    want = cm.expected(PT, text)
    assert len(want["records"]) == 4098 and sorted(set(want["classes"].tolist())) == ([3] if kept_at is None else [0, 3])
    counts, got = check(sk_ctx, PT, text, want)
    assert counts["records"][0] == 4098 and got.count(b"@a\nN\n+\n!\n") == 4098 - (0 if kept_at is None else 2)


# ---- 3 every read kept: the interleaved mode's output 0 -----------------------------------------------------------------
def test_all_kept_is_pe_interleaved(sk_ctx):
    text = b"".join(b"@r%d x\nACGTACGTACGT\n+%s\nIIIIIIIIII##\n" % (k, b"c" * (k % 3)) for k in range(700))
    params = capi.make_params(*PT)
    dev = to_device(text)
    ref, ref_counts = sk_ctx.trim_fastq(params, dev, mode="pe_interleaved", record_index=True)
    got, counts = sk_ctx.trim_fastq(params, dev, mode=MODE, record_index=True)
    assert ref_counts["records"] == [700, 0, 0] and counts["records"] == [700, 0, 0] and counts["bytes"] == ref_counts["bytes"]
    assert got[1] is None and got[2] is None
    assert bytes(got[0][0].cpu().numpy()) == bytes(ref[0][0].cpu().numpy()) == cm.expected(PT, text)["texts"][0]
    assert np.array_equal(got[0][1].cpu().numpy(), ref[0][1].cpu().numpy())


# ---- 4 the reference's -c runs ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastq_combo")
    cu.prepare_inputs(d)
    cu.prepare_long_inputs(d)
    return d


@pytest.mark.parametrize("name,rec", COMBO_RUNS)
def test_reference_runs(sk_ctx, workdir, name, rec):
    """the device text is the model's, which tests/test_fastq_combo_model.py ties to the reference's recorded files"""
    _, texts, _ = golden_texts(rec["argv"], workdir)
    ptuple = tm.run_params(rec["argv"])
    want = cm.expected(ptuple, texts[0])
    outs, counts = sk_ctx.trim_fastq(capi.make_params(*ptuple), to_device(texts[0]), mode=MODE, record_index=True)
    text, index = outs[0]
    assert bytes(text.cpu().numpy()) == want["texts"][0] and outs[1] is None and outs[2] is None
    assert counts["records"] == [len(want["records"]), 0, 0] and counts["bytes"] == [len(want["texts"][0]), 0, 0]
    assert np.array_equal(index.cpu().numpy(), np.arange(counts["records"][0]))


# ---- 5 the output is longer than the input -------------------------------------------------------------------------------
def test_output_longer_than_the_text(sk_ctx):
    text = b"".join(b"@%s\nA\n\n#\n" % (b"n" * (1 + k % 20)) for k in range(600))
    want = cm.expected(PT, text)
    counts, _ = check(sk_ctx, PT, text, want)
    assert counts["bytes"][0] == len(text) + counts["records"][0] == len(text) + 600
    assert counts["bytes"][0] <= capi.fastq_output_bound(len(text), MODE)
    # one byte short: nothing is written
    rc, short, keep = call(sk_ctx, PT, text, cap=counts["bytes"][0] - 1)
    assert rc == capi.SK_ESPACE and short["bytes"] == counts["bytes"] and short["records"] == counts["records"]
    untouched(keep)
    rc, _, keep = call(sk_ctx, PT, text, cap=len(text))  # "capacity = input bytes" is not enough
    assert rc == capi.SK_ESPACE
    untouched(keep)
    rc, exact, keep = call(sk_ctx, PT, text, cap=counts["bytes"][0])
    assert rc == capi.SK_OK and texts_of(keep, exact)[0] == want["texts"][0]
    # the one-pass driver sizes by the bound
    images, _ = sk_ctx.trim_fastq_gz(capi.make_params(*PT), to_device(text), mode=MODE)
    assert gzip.decompress(bytes(images[0].cpu().numpy())) == want["texts"][0]


# ---- 6 errors, the odd record, the unused outputs ------------------------------------------------------------------------
def test_errors_and_the_odd_record(sk_ctx):
    good = cm.truth_text(40, 11)
    lines = good.split(b"\n")[:-1]
    recs = [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines), 4)]
    assert len(recs) == 80 and b"".join(recs) == good
    params = capi.make_params(*PT)
    for why, bad in BAD.items():
        for k in (0, 37, 80):
            text = b"".join(recs[:k] + [bad] + recs[k:])
            ref = fm.expected(PT, [text], "pe_interleaved")
            assert ref["verdict"] == (why, 0, k)
            rc, counts, keep = call(sk_ctx, PT, text)
            rc_i, counts_i, _ = raw(sk_ctx, params, [text], "pe_interleaved")
            assert rc == rc_i == capi.SK_EFORMAT and counts == counts_i
            assert (counts["format_error"], counts["format_input"], counts["format_record"]) == (why, 0, k)
            assert counts["records"] == [0, 0, 0] and counts["bytes"] == [0, 0, 0] and counts["dropped_unpaired"] == 1
            untouched(keep)
    for k in (0, 37, 79):  # (behind an even number of records at 80 it would be the dropped one's: checked, not scanned)
        text = b"".join(recs[:k] + [RANGE_BAD] + recs[k:])
        ref = fm.expected(PT, [text], "pe_interleaved")
        assert ref["range"] is not None and int(ref["range"][0]) == k
        rc, counts, keep = call(sk_ctx, PT, text)
        rc_i, counts_i, _ = raw(sk_ctx, params, [text], "pe_interleaved")
        assert rc == rc_i == capi.SK_ERANGE and counts["range"] == counts_i["range"] == tuple(ref["range"])
        assert counts["records_in"] == counts_i["records_in"] and counts["dropped_unpaired"] == 1
        untouched(keep)
    # a format error beats a range error
    rc, counts, keep = call(sk_ctx, PT, b"".join(recs[:3] + [RANGE_BAD] + recs[3:30] + [BAD[capi.SK_FQ_SEQ_EMPTY]]))
    assert rc == capi.SK_EFORMAT and counts["format_record"] == 31
    untouched(keep)
    # an odd record count: the last record is checked, then dropped
    counts, _ = check(sk_ctx, PT, b"".join(recs[:7]))
    assert counts["dropped_unpaired"] == 1 and counts["records"][0] == 6 and counts["records_in"] == [7, 0]
    rc, counts, keep = call(sk_ctx, PT, b"".join(recs[:6]) + BAD[capi.SK_FQ_LENGTHS])
    assert rc == capi.SK_EFORMAT and counts["format_record"] == 6
    untouched(keep)
    # a second text is SK_EINVAL on a device too, and nothing is enqueued
    with pytest.raises(capi.SickleError):
        d = to_device(good)
        sk_ctx.trim_fastq(params, d, d, mode=MODE)


# ---- 7 the chained call -----------------------------------------------------------------------------------------------
def chained(ctx, ptuple, text, bound, n=None, valid=None):
    torch = torch_mod()
    params = capi.make_params(*ptuple)
    dev = to_device(text + b"\n" * (bound - len(text)))
    ws_bytes = capi.lib().sk_trim_fastq_workspace_bytes(bound, params.trunc_n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    cap = capi.fastq_output_bound(bound, MODE)
    out = torch.full((cap + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    words = [None if v is None else torch.tensor([v], dtype=torch.int64, device="cuda") for v in (n, valid)]
    ctx.trim_fastq_chained_device_async(params, [dev.data_ptr()], [bound], [capi.FastqOutput(out.data_ptr(), cap, None, 0)],
                                        ws.data_ptr(), ws_bytes, bytes_dev_ptrs=[None if words[0] is None else words[0].data_ptr()],
                                        valid_dev_ptrs=[None if words[1] is None else words[1].data_ptr()], mode=MODE)
    counts = ctx.trim_fastq_device_finish(ws.data_ptr())
    assert bool((out[counts["bytes"][0]:] == SENTINEL).all())
    return counts, bytes(out[:counts["bytes"][0]].cpu().numpy())


CHILD = """
import sys, hashlib
sys.path[:0] = [%r, %r]
import torch
torch.cuda.is_available()
from sickle_amd import capi
import combo_all_model as cm
from bgzf_raw import to_device
ctx = capi.Context(device=0, slots=2)
text = cm.truth_text(300, 13) + b"@odd\\nACGT\\n+\\nIIII\\n"
outs, counts = ctx.trim_fastq(capi.make_params(*cm.TRUTH_PARAMS), to_device(text), mode=cm.MODE)
print("RESULT", hashlib.md5(bytes(outs[0].cpu().numpy())).hexdigest(), counts["records"], counts["bytes"])
ctx.close()
"""


def test_chained(sk_ctx):
    text = cm.truth_text(300, 13) + b"@odd\nACGT\n+\nIIII\n"
    B = len(text)
    whole = cm.expected(PT, text)
    counts, got = chained(sk_ctx, PT, text, B + 4096, n=B)
    assert got == whole["texts"][0] and counts["records"] == [600, 0, 0] and counts["dropped_unpaired"] == 1
    cut = text.index(b"@", B // 2)  # the shorter text ends with a record; one byte more, and inside its name line
    for n in (cut, cut + 1, 0):
        counts, got = chained(sk_ctx, PT, text, B, n=n)
        want = cm.expected(PT, text[:n])
        assert got == want["texts"][0] and counts["records"] == [len(want["records"]), 0, 0]
        assert counts["records_in"] == want["records_in"] and counts["tail_lines"] == want["tail_lines"]
    counts, got = chained(sk_ctx, PT, text, B, n=B, valid=0)
    assert got == b"" and counts["records"] == [0, 0, 0] and counts["records_in"] == [0, 0]
    counts, got = chained(sk_ctx, PT, text, B, n=B, valid=1)
    assert got == whole["texts"][0]


def test_uncounted_walk_in_a_child_process(sk_ctx):
    """SK_FQ_COUNTED=0: the per-read steps walk the bound, so every rank from NREAL to the bound is looked at: same bytes"""
    import hashlib
    text = cm.truth_text(300, 13) + b"@odd\nACGT\n+\nIIII\n"
    want = cm.expected(PT, text)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SK_FQ_COUNTED="0")
    pr = subprocess.run([sys.executable, "-c", CHILD % (root, os.path.join(root, "tests"))], env=env, capture_output=True,
                        timeout=300)
    assert pr.returncode == 0, pr.stderr.decode()[-2000:]
    line = [ln for ln in pr.stdout.decode().splitlines() if ln.startswith("RESULT")][0]
    assert line == "RESULT %s %s %s" % (hashlib.md5(want["texts"][0]).hexdigest(), [600, 0, 0], [len(want["texts"][0]), 0, 0])


# ---- 8 pieces, 9 the -a T order ----------------------------------------------------------------------------------------
def run_stream(stream):
    parts = list(stream)
    return [None if parts[0][o] is None else b"".join(p[o] for p in parts) for o in range(3)], stream


@pytest.fixture(scope="module")
def mixed():
    """about 300 pairs with failures in every class, names and reads of several lengths, an odd last record"""
    rng = random.Random(77)
    parts = [cm.truth_text(rng.randrange(1, 9), rng.randrange(2, 35), crlf_names=rng.random() < 0.2) for _ in range(68)]
    text = b"".join(parts) + b"@odd\nACGT\n+\nIIII\n"
    want = cm.expected(PT, text)
    assert 500 <= len(want["records"]) <= 700 and all(n > 30 for n in Counter(want["classes"].tolist()).values())
    return text, want


@pytest.mark.parametrize("size", [256, 1000, 8192])
def test_pieces(sk_ctx, mixed, size):
    text, want = mixed
    params = capi.make_params(*PT)
    whole, counts = sk_ctx.trim_fastq(params, to_device(text), mode=MODE)
    assert bytes(whole[0].cpu().numpy()) == want["texts"][0]
    got, st = run_stream(sk_ctx.trim_fastq_stream(params, [text[a:a + 7919] for a in range(0, len(text), 7919)], mode=MODE,
                                                  piece_bytes=size, room=4096))
    assert got == [want["texts"][0], None, None]
    for key in ("records_in", "records", "bytes", "tail_lines", "dropped_unpaired"):
        assert st.counts[key] == counts[key], key
    assert st.pieces >= len(text) // size and st.counts["dropped_unpaired"] == 1


def test_ordered(sk_ctx, mixed):
    text, want = mixed
    text = text[:text.index(b"@", 2 * len(text) // 3)]  # about 200 pairs
    want = cm.expected(PT, text)
    params, dev = capi.make_params(*PT), to_device(text)
    batch_len = 5000
    for threads in (1, 2, 3, 5, 16):
        model, order, oc = cm.ordered(PT, text, threads, batch_len)
        assert oc["batches"] >= 3
        outs, counts = sk_ctx.trim_fastq(params, dev, mode=MODE, record_index=True, order=(threads, batch_len))
        assert bytes(outs[0][0].cpu().numpy()) == model, threads
        assert np.array_equal(outs[0][1].cpu().numpy(), order) and outs[1] is None and outs[2] is None
        assert counts["records"] == [len(order), 0, 0] and counts["bytes"] == [len(model), 0, 0]
        assert {k: counts["order"][k] for k in oc} == oc
        if threads in (3, 16):
            for kw in (dict(piece_bytes=20_000, room=16384), dict(piece_bytes=6000, room=16384)):
                got, st = run_stream(sk_ctx.trim_fastq_stream(params, text, mode=MODE, order=(threads, batch_len), **kw))
                assert got == [model, None, None], (threads, kw)
                assert st.counts["order"]["batches"] == oc["batches"] and st.counts["records"] == counts["records"]
    assert cm.ordered(PT, text, 3, batch_len)[0] != cm.ordered(PT, text, 1, batch_len)[0]
    # one batch holds the text: the read order
    outs, counts = sk_ctx.trim_fastq(params, dev, mode=MODE, order=(1, 10 * len(text)))
    assert bytes(outs[0].cpu().numpy()) == want["texts"][0] and counts["order"]["batches"] == 1


# ---- 10 .gz -----------------------------------------------------------------------------------------------------------
def test_gz_drivers(sk_ctx, mixed, workdir):
    text, want = mixed
    params = capi.make_params(*PT)
    images, counts = sk_ctx.trim_fastq_gz(params, to_device(text), mode=MODE)
    assert images[1] is None and images[2] is None and counts["records"] == [len(want["records"]), 0, 0]
    assert gzip.decompress(bytes(images[0].cpu().numpy())) == want["texts"][0]
    bgzf = sk_ctx.bgzf(to_device(text))
    plain = to_device(gzip.compress(text, 6))
    for image in (bgzf, plain):
        for kw in ({}, dict(text_capacity=len(text) + 100)):
            out, c = sk_ctx.trim_gz(params, image, mode=MODE, **kw)
            assert gzip.decompress(bytes(out[0].cpu().numpy())) == want["texts"][0] and out[2] is None
            assert c["records"] == counts["records"] and c["bytes"] == counts["bytes"]
    got, st = run_stream(sk_ctx.trim_gz_stream(params, bytes(bgzf.cpu().numpy()), mode=MODE, piece_bytes=65536, room=16384))
    assert gzip.decompress(got[0]) == want["texts"][0] and got[0].endswith(EOF)
    # the golden interleaved input as ordinary gzip, in pieces
    name, rec = COMBO_RUNS[0].values
    _, texts, _ = golden_texts(rec["argv"], workdir)
    ptuple = tm.run_params(rec["argv"])
    gold = cm.expected(ptuple, texts[0])
    longest = max(len(line) for line in texts[0].split(b"\n"))
    got, st = run_stream(sk_ctx.trim_gzip_stream(capi.make_params(*ptuple), gzip.compress(texts[0], 6), mode=MODE,
                                                 piece_bytes=262144, room=4 * longest + 65536))
    assert gzip.decompress(got[0]) == gold["texts"][0] and got[1] is None and got[2] is None
    assert st.counts["records"] == [len(gold["records"]), 0, 0]


# ---- 11 drawn texts ------------------------------------------------------------------------------------------------------
def test_drawn_texts(sk_ctx):
    """100 drawn interleaved texts, plain and ordered (tests/test_fastq_combo_model.py checks on the CPU that the seed
    draws every class)"""
    rng = random.Random(SEED)
    hit = Counter()
    for it in range(DRAWS):
        ptuple, text, threads, batch_len = drawn_case(rng)
        want = cm.expected(ptuple, text)
        hit.update(cm.CLASSES[c] for c in want["classes"].tolist())
        check(sk_ctx, ptuple, text, want, shift=it % 16)
        model, order, oc = cm.ordered(ptuple, text, threads, batch_len)
        outs, counts = sk_ctx.trim_fastq(capi.make_params(*ptuple), to_device(text), mode=MODE, record_index=True,
                                         order=(threads, batch_len))
        assert bytes(outs[0][0].cpu().numpy()) == model, (it, threads, batch_len)
        assert np.array_equal(outs[0][1].cpu().numpy(), order) and counts["order"]["batches"] == oc["batches"]
    print("pair classes drawn:", dict(hit))
    assert all(hit[c] > 0 for c in cm.CLASSES)


# ---- 12 a bad option raises in front of everything ----------------------------------------------------------------------
FOUR = b"".join(b"@r%d\n%s\n+\n%s\n" % (i, b"ACGT" * (6 + i), b"I" * (20 + 4 * i) + b"#" * 4) for i in range(4))


def test_a_bad_option_raises_with_nothing_in_flight(sk_ctx, monkeypatch):
    """A bad behind-call option of the .gz drivers and of a stream raises its ValueError before the library is called once,
    and the next good call on the same context and stream gives what a fresh context gives: nothing was left unfinished"""
    params = capi.make_params("sanger", 20, 20)
    host = lambda res: ([None if im is None else bytes(im.cpu().numpy()) for im in res[0]], res[1])

    def good(ctx):
        parts = list(ctx.trim_fastq_stream(params, FOUR, mode="se", piece_bytes=40, room=128, gz=True))
        return host(ctx.trim_fastq_gz(params, to_device(FOUR), mode="se")), parts
    fresh = capi.Context(device=0, slots=2)
    want, want_parts = good(fresh)
    fresh.close()
    assert want[1]["records_in"] == [4, 0] and gzip.decompress(want[0][0]) == fm.expected(("sanger", 20, 20), [FOUR], "se")["texts"][0]
    assert len(want_parts) > 1 and gzip.decompress(b"".join(p[0] for p in want_parts)) == gzip.decompress(want[0][0])
    image = sk_ctx.bgzf(to_device(FOUR))
    calls, check = [], capi.Context._check
    monkeypatch.setattr(capi.Context, "_check", lambda self, rc, err=None: (calls.append(rc), check(self, rc, err))[1])
    bad = dict(bases={"len_bins": 4})
    for run in (lambda: sk_ctx.trim_fastq_gz(params, to_device(FOUR), mode="se", **bad),
                lambda: sk_ctx.trim_gz(params, image, mode="se", text_capacity=len(FOUR) + 64, **bad),
                lambda: sk_ctx.trim_gz(params, image, mode="se", order=(2, 64), text_capacity=len(FOUR) + 64, **bad),
                lambda: sk_ctx.trim_gz(params, image, mode="se", **bad),
                lambda: sk_ctx.trim_fastq_stream(params, FOUR, mode="se", piece_bytes=40, room=128, rejects="pairs"),
                lambda: sk_ctx.trim_gz_stream(params, bytes(image.cpu().numpy()), mode="se", piece_bytes=65536, **bad)):
        del calls[:]
        with pytest.raises(ValueError) as e:
            run()
        assert calls == [] and str(e.value) in ("bases: unknown keys ['len_bins']", "rejects=\"pairs\" needs a pair mode")
        got, got_parts = good(sk_ctx)
        assert got == want and got_parts == want_parts and len(calls) > 4

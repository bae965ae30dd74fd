"""CPU: every case of tests/workspace_cases.py is what its label says, by the models and the pure sizing functions alone,
so that tests/test_gpu_workspace.py is not vacuous if a generator drifts."""
import gzip
import zlib

import numpy as np
import pytest

import bgunzip_model as bm
import fastq_model as fm
import gunzip_model as gm
import trim_model as tm
import workspace_cases as wc
from sickle_amd import capi

TEXTS = wc.fastq_texts()


@pytest.mark.parametrize("name", sorted(TEXTS))
def test_fastq_text_is_what_its_label_says(name):
    text, verdict, slots_label = TEXTS[name]  # the label: within or over the packed batch
    f = fm.frame(text)
    lines = 4 * f["records"] + f["tail_lines"]
    slots, reads = wc.fq_slots(len(text)), wc.fq_pack_reads(len(text))
    within = f["records"] <= reads
    print(name, "bytes", len(text), "lines", lines, "records", f["records"], "slots", slots, "packed reads", reads,
          "over" if not within else "within")
    assert ("within" if within else "over") == slots_label
    assert (lines + 3) // 4 <= slots  # every line of any text has a descriptor slot
    for trunc_n in (0, 1):
        lay = wc.fq_layout(len(text), trunc_n)
        assert lay["total"] == capi.lib().sk_trim_fastq_workspace_bytes(len(text), trunc_n)
        assert slots <= lay["S"]
        want = fm.expected(wc.fq_params(trunc_n), [text], "se")
        assert want["verdict"] == verdict and want["range"] is None
        if verdict is None:
            assert f["records"] <= lay["N"]  # every valid record has a place in the packed batch
            assert want["records_in"][0] == f["records"]
            if name == "control_600":  # the ordinary control: reads are cut, some are dropped
                assert 0 < len(want["index"][0]) < 600 and len(want["texts"][0]) < len(text)
            else:  # -l 1 and quality 'I': every record is kept whole, the most bytes the sections can see
                assert len(want["index"][0]) == f["records"]
    for mode in wc.FASTQ_MODES[1:]:
        want = fm.expected(wc.fq_params(0), wc.texts_of_mode(text, mode), mode)
        assert (want["verdict"] is None) == (verdict is None)
        T = len(text) * (2 if mode == "pe_split" else 1)
        assert 2 * slots <= wc.fq_layout(T, 0)["S"] or mode != "pe_split"


def test_fastq_facts_of_the_table():
    for k in (1, 2, 2047, 2048, 2049, 4099):
        assert fm.frame(TEXTS["dense_%d" % k][0])["records"] == k
    text = TEXTS["dense_2049_unterminated"][0]
    want = fm.expected(wc.fq_params(0), [text], "se")
    assert want["verdict"] is None and len(want["texts"][0]) == len(text) + 1
    assert fm.expected(wc.fq_params(0), [b"\n" * 4096], "se")["records_in"][0] == 1024 and wc.fq_pack_reads(4096) == 512
    assert fm.expected(wc.fq_params(1), [wc.one_record(30000)], "se")["verdict"] is None
    assert len(wc.one_record(30000)) < wc.FQ_CHUNK < len(wc.one_record(70000)) // 2 + 40000
    assert wc.FQ_BLOCK_READS == 2048 and len(wc.REC) == 9 and len(wc.BAD7) == 7


@pytest.mark.parametrize("n", wc.TRIM_N)
def test_trim_cases(n):
    assert capi.lib().sk_trim_workspace_bytes(n) == wc.trim_workspace_bytes(n)
    for mode in tm.MODES:
        if mode != "se" and n % 2:
            continue
        for kept in wc.TRIM_KEPT:
            qual, seq, off, starts, cuts = wc.trim_case(n, kept, "ragged", mode)
            c = tm.counts_of(tm.expected(qual, seq, starts, cuts, mode))
            print(n, mode, kept, c)
            if kept == "all":
                assert sum(c["records"]) == n and c["records"][2] == 0
            elif kept == "none":
                assert sum(c["records"]) == 0
            elif mode != "se":
                assert c["records"] == [0, 0, n // 2]  # one mate of every pair: the most singles


@pytest.mark.parametrize("n", wc.BGZF_LENGTHS)
def test_bgzf_cases(n):
    blocks = wc.bgzf_blocks(n)
    print(n, "blocks", blocks)
    assert blocks == {0: 0, 1: 1, 65279: 1, 65280: 1, 65281: 2, 130560: 2, 195841: 4}[n]
    for kind in wc.BGZF_KINDS:
        text = wc.bgzf_text(kind, n)
        assert len(text) == n
        if n >= 65279:
            ratio = len(zlib.compress(text[:65280], 6)) / min(n, 65280)
            assert {"random": ratio > 1.0, "repeat": ratio < 0.01, "fastq": 0.1 < ratio < 0.9}[kind], (kind, ratio)


@pytest.mark.parametrize("k", wc.EMPTY_MEMBERS)
def test_empty_members(k):
    image = wc.empty_members(k)
    want = bm.bgunzip(image)
    assert len(image) == 28 * k and (want["members"], want["bytes_out"], want["error"]) == (k, 0, 0)


def test_gzip_cases():
    for name, (image, text, lo, hi) in wc.gzip_images().items():
        ratio = len(text) / len(image)
        print(name, len(image), len(text), "ratio %.2f" % ratio)
        assert lo <= ratio <= hi, name
        assert gzip.decompress(image) == text
        want = gm.gunzip(image)
        assert (want["bytes_out"], want["error"]) == (len(text), 0)
        assert want["members"] == (3 if name == "three_members" else 1)

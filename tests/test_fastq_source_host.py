"""The source view of a finished FASTQ text call without a device: sickle_amd/csrc/sk_fastq_source.h, what the report,
audit, bases, adapters and rejects calls and the clip commit take of the call they run behind, run on the host
(tests/fastq_source/source_host, and source_host_san: the same stand-alone program under the address and
undefined-behaviour sanitizers, over buffers of exactly the sizes the view is told) against tests/fastq_source_model.py,
which restates DESIGN.md and the layout comment of sk_device.h.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import cli_util as cu
import fastq_source_model as sm

DIR = os.path.join(cu.ROOT, "tests", "fastq_source")


@pytest.fixture(scope="module", params=["source_host", "source_host_san"])
def tool(request):
    subprocess.run(["make", "-s", "-C", DIR, "all"], check=True)
    return os.path.join(DIR, request.param)


def run(tool, case_words, d):
    """a case goes in behind the count of its words; a result comes back behind the count of its words"""
    src, dst = str(d / "cases.bin"), str(d / "results.bin")
    np.array([x for c in case_words for x in [len(c)] + c], dtype="<u8").tofile(src)
    pr = subprocess.run([tool, src, dst], capture_output=True)
    assert pr.returncode == 0 and not pr.stderr, pr.stderr.decode()[-3000:]
    words, out, at = np.fromfile(dst, dtype="<u8"), [], 0
    while at < len(words):
        n = int(words[at])
        out.append([int(x) for x in words[at + 1:at + 1 + n]])
        at += 1 + n
    assert len(out) == len(case_words)
    return out


def test_layout_every_pointer_and_bound(tool, tmp_path):
    cases = sm.layout_cases()
    got = run(tool, [sm.layout_words(c) for c in cases], tmp_path)
    for c, g in zip(cases, got):
        want = sm.layout_expect(c)
        assert g == want, (c, g, want)
        T = c["T"]
        bytes0 = c["texts"][0][1] if c["texts"] else 0
        assert g[10:14] == [bytes0 // 4 + 1, 2 * ((T + 7) // 8) + 2, 2 * ((T + 2) // 16) + 2, 16 * ((T + 31) // 32)]
    assert len(cases) == 15 * 4 * 2 * 4 * 4 * 5  # no case skipped or filtered


def test_validity_every_subset_of_every_kind(tool, tmp_path):
    cases = sm.validity_cases()
    got = run(tool, [sm.validity_words(c) for c in cases], tmp_path)
    seen = set()
    for c, g in zip(cases, got):
        want = sm.validity_expect(c)
        assert g == [want], (c, g, want)
        seen.add((c["kind"], want))
    assert seen == {(k, v) for k in sm.KINDS for v in (0, 1)}
    # every single condition alone makes its kind's call void, but for the mode under the view without one
    for kind in sm.KINDS:
        for cond in sm.conditions_of(kind):
            for mode in sm.MODES + (sm.NO_MODE,):
                c = dict(kind=kind, mode=mode, met={cond}, foreign=1)
                assert sm.validity_expect(c) == int(cond == "mode_differs" and mode is sm.NO_MODE)
    assert len(cases) == (8 + 16 + 32 + 128) * 5 * 2


def test_lookups_stay_inside_the_table_and_the_texts(tool, tmp_path):
    tables = sm.lookup_tables()
    got = run(tool, [sm.lookup_words(t) for t in tables], tmp_path)
    hit = {"slot": 0, "no_slot": 0, "clamped": 0}
    for t, g in zip(tables, got):
        assert len(g) == 8 * len(sm.LOOKUP_READS)
        for q, r in enumerate(sm.LOOKUP_READS):
            have, want = g[8 * q:8 * q + 8], sm.lookup_expect(t, r)
            assert have == want, (t, r, have, want)
            i, ok, name_at, name_len, seq_at, j, rec_at, rec_len = have
            b = t["bytes"][i]
            assert i == j and i in ((0, 1) if t["mode"] == sm.PE_SPLIT else (0,))
            assert 0 <= seq_at <= b and 0 <= rec_at <= b and rec_at + rec_len <= b
            if ok:
                assert 0 <= name_at <= b and name_at + name_len <= b
            else:
                assert (seq_at, rec_at, rec_len) == (b, b, 0)
            _, slot = sm.slot_of(t["mode"], t["slots0"], r)
            assert ok == int(slot < t["slot_bound"])
            hit["slot" if ok else "no_slot"] += 1
            if ok and (rec_at, rec_len) != (t["desc"][slot][0], t["desc"][slot][4] - t["desc"][slot][0]):
                hit["clamped"] += 1
    assert all(hit.values()), hit


def test_the_model_reads_the_slot_bound_as_the_table_end():
    """reads at, below and beyond the bound, in split and unsplit framing, on the model alone"""
    t = dict(mode=sm.SE, bytes=[40, 24], slots0=3, slot_bound=6, desc=[[0, 3, 8, 10, 15]] * 6)
    assert sm.lookup_expect(t, 5)[1] == 1 and sm.lookup_expect(t, 6)[1] == 0
    t["mode"] = sm.PE_SPLIT  # text 1's slots 3, 4, 5 are reads 1, 3, 5; text 0's slots are reads 0, 2, .. 10
    assert [sm.lookup_expect(t, r)[1] for r in (1, 3, 5, 7)] == [1, 1, 1, 0]
    assert [sm.lookup_expect(t, r)[1] for r in (8, 10, 12)] == [1, 1, 0]
    assert sm.lookup_expect(t, 7) == [1, 0, sm.NONE, sm.NONE, 24, 1, 24, 0]

"""tests/fastq_audit_model.py against a truth table written by hand and against the golden inputs (the numbers of
DESIGN 4.18's table, which were worked out on the host with the rule of include/sickle_amd.h)."""
import os

import numpy as np
import pytest

import fastq_audit_model as am
import fastq_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = os.path.join(ROOT, "tests", "golden", "inputs")

# name line -> (key, tag), by hand
KEYS = [
    (b"@read7", (b"read7", 0)),                                   # the key ends at the line's end
    (b"@read7 1:N:0:ACGT", (b"read7", 0)),                        # at a space
    (b"@read7\tcomment", (b"read7", 0)),                          # at a tab
    (b"@read7\r", (b"read7", 0)),                                 # at a '\r'
    (b"@read7/1\r", (b"read7", 1)),
    (b"@read7/1", (b"read7", 1)),
    (b"@read7/2", (b"read7", 2)),
    (b"@read7/3", (b"read7/3", 0)),                               # not a tag
    (b"@read7/1/1", (b"read7/1", 1)),                             # stripped once
    (b"@read7/1/2", (b"read7/1", 2)),
    (b"@/1", (b"", 1)),                                           # a key of exactly /1
    (b"@/2 x", (b"", 2)),
    (b"@ x", (b"", 0)),                                           # '@' and a space: the empty key
    (b"@1", (b"1", 0)),                                           # one byte: no tag
    (b"@a/", (b"a/", 0)),
    (b"@a/1x", (b"a/1x", 0)),
    (b"@a /1", (b"a", 0)),                                        # the tag rule looks at the key only
    (b"@M:1:FC:1:1101:1:1 1:N:0:ACGT", (b"M:1:FC:1:1101:1:1", 0)),
    (b"@@", (b"@", 0)),
    (b"@a\x0bb", (b"a\x0bb", 0)),                                 # a vertical tab ends nothing
]

# (name 1, name 2) -> (mismatch, swapped), by hand
PAIRS = [
    ((b"@r/1", b"@r/2"), (False, False)),
    ((b"@r/2", b"@r/1"), (False, True)),                          # swapped tags on equal keys
    ((b"@r/2", b"@s/1"), (True, False)),                          # swapped tags on unequal keys: a mismatch only
    ((b"@r/1", b"@r/1"), (False, False)),
    ((b"@r/2", b"@r/2"), (False, False)),
    ((b"@r", b"@r"), (False, False)),
    ((b"@r", b"@r/2"), (False, False)),                           # the tag is no part of the key
    ((b"@abcdefgh", b"@abcdefgi"), (True, False)),                # the last byte only
    ((b"@abcdefgh", b"@abcdefg"), (True, False)),                 # the length only
    ((b"@abcdefg", b"@abcdefgh"), (True, False)),
    ((b"@M:1:FC:1:1101:1:1 1:N:0:ACGT", b"@M:1:FC:1:1101:1:1 2:N:0:ACGT"), (False, False)),  # CASAVA 1.8
    ((b"@M:1:FC:1:1101:1:1 1:N:0:ACGT", b"@M:1:FC:1:1101:1:2 2:N:0:ACGT"), (True, False)),
    ((b"@ a", b"@ b"), (False, False)),                           # two empty keys
    ((b"@/1", b"@/2"), (False, False)),
    ((b"@/2", b"@/1"), (False, True)),
    ((b"@x/1/1", b"@x/1/2"), (False, False)),
    ((b"@x/1/1", b"@x/2"), (True, False)),                        # "x/1" against "x"
    ((b"@x\r", b"@x"), (False, False)),
    ((b"@x/3", b"@x/3"), (False, False)),
    ((b"@x/3", b"@x/1"), (True, False)),
]


@pytest.mark.parametrize("line,want", KEYS)
def test_key(line, want):
    assert am.key(line) == want


@pytest.mark.parametrize("names,want", PAIRS)
def test_pair(names, want):
    assert am.pair(*names) == want


def _rec(name, qual=b"IIII"):
    return name + b"\n" + b"A" * len(qual) + b"\n+\n" + qual + b"\n"


def test_text_of_the_table():
    """the pair table as one interleaved text and as two split ones; an odd interleaved record is in no count"""
    inter = b"".join(_rec(a) + _rec(b) for (a, b), _ in PAIRS)
    want_m = [k for k, (_, (m, _)) in enumerate(PAIRS) if m]
    want_s = sum(s for _, (_, s) in PAIRS)
    for texts, mode in (([inter], "pe_interleaved"), ([inter + _rec(b"@odd", b"!~")], "pe_combo_all"),
                        ([b"".join(_rec(a) for (a, _), _ in PAIRS), b"".join(_rec(b) for (_, b), _ in PAIRS)], "pe_split")):
        r = am.audit(None, texts, mode)
        assert (r["calls"], r["calls_failed"], r["pairs"]) == (1, 0, len(PAIRS))
        assert (r["name_mismatch"], r["first_mismatch"], r["tags_swapped"]) == (len(want_m), want_m[0], want_s)
        assert (r["qual_bytes"], r["qual_min"], r["qual_max"]) == (8 * len(PAIRS), 73, 73)  # the odd record's '!' and '~' are not there
        assert r["qual_hist"][73] == 8 * len(PAIRS) and r["qual_hist"].sum() == 8 * len(PAIRS)
    r = am.audit(None, [inter], "se")
    assert (r["pairs"], r["name_mismatch"], r["first_mismatch"], r["tags_swapped"]) == (0, 0, am.NONE, 0)
    assert r["qual_bytes"] == 8 * len(PAIRS)
    r = am.audit(None, [inter], "pe_interleaved", names=False)
    assert (r["pairs"], r["first_mismatch"], r["qual_bytes"]) == (0, am.NONE, 8 * len(PAIRS))


def test_unsigned_bytes_and_empty():
    r = am.audit(None, [_rec(b"@a", b"\x80\xff") + _rec(b"@a", b"\x21")], "pe_interleaved")
    assert (r["qual_bytes"], r["qual_min"], r["qual_max"]) == (3, 0x21, 0xff)
    r = am.audit(None, [b""], "pe_interleaved")
    assert (r["calls"], r["qual_bytes"], r["qual_min"], r["qual_max"], r["first_mismatch"]) == (1, 0, am.NONE, 0, am.NONE)
    r = am.audit(None, [b"@a\nAC\n+\nI\n"], "se")  # a format verdict
    assert am.equal(r, am.failed()) == []


def test_add_numbers_pairs_over_adding_calls():
    a = am.audit(None, [_rec(b"@p/1") + _rec(b"@p/2")] , "pe_interleaved")
    b = am.audit(None, [_rec(b"@p/1") + _rec(b"@p/2") + _rec(b"@q/1") + _rec(b"@x/2")], "pe_interleaved")
    r = am.add(am.add(am.add(am.zero(), a), am.failed()), b)
    assert (r["calls"], r["calls_failed"], r["pairs"], r["name_mismatch"], r["first_mismatch"]) == (2, 1, 3, 1, 2)


def _read(name):
    return open(os.path.join(INPUTS, name), "rb").read()


def _drop(text, first=False, last=False):
    f = fm.frame(text)
    a = int(f["e3"][0]) + 1 if first else 0
    b = int(f["s0"][-1]) if last else len(text)
    return text[a:b]


def test_golden_inputs():
    f, r, inter, problem = _read("test.f.fastq"), _read("test.r.fastq"), _read("test.fastq"), _read("problem1.fastq")
    names = lambda a: (a["pairs"], a["name_mismatch"], a["tags_swapped"])
    a = am.audit(None, [f, r], "pe_split")
    assert names(a) == (1250, 0, 0) and a["first_mismatch"] == am.NONE
    assert names(am.audit(None, [r, f], "pe_split")) == (1250, 0, 1250)
    a = am.audit(None, [_drop(f, last=True), _drop(r, first=True)], "pe_split")
    assert names(a)[:2] == (1249, 1249) and a["first_mismatch"] == 0
    a = am.audit(None, [inter], "pe_interleaved")
    assert names(a) == (1250, 0, 0)
    assert (a["qual_bytes"], a["qual_min"], a["qual_max"]) == (375000, 66, 105)
    a = am.audit(None, [_drop(inter, first=True, last=True)], "pe_interleaved")
    assert names(a)[:2] == (1249, 1249)
    a = am.audit(None, [problem], "pe_interleaved")
    assert names(a)[:2] == (2, 0)

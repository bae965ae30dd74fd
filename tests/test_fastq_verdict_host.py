"""The verdict of a FASTQ text call's finish without a device: fqv_verdict of sickle_amd/csrc/sk_fastq_verdict.h, the
function sk_capi.hip's fastq_finish calls on the words it copied back, run on the host (tests/fastq_verdict/verdict_host,
and verdict_host_san: the same stand-alone program under the address and undefined-behaviour sanitizers) against
tests/fastq_verdict_model.py, which restates include/sickle_amd.h: every kind of call, every framing mode, every subset of
the conditions a kind can meet.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

import cli_util as cu
import fastq_verdict_model as vm

DIR = os.path.join(cu.ROOT, "tests", "fastq_verdict")
POISON32, POISON64 = 0x5a5a5a5a, 0x5a5a5a5a5a5a5a5a
COUNT_WORDS, ORDER_WORDS, PIECE_WORDS, ORDER_PIECE_WORDS = 17, 9, 6, 11


@pytest.fixture(scope="module", params=["verdict_host", "verdict_host_san"])
def tool(request):
    subprocess.run(["make", "-s", "-C", DIR, "all"], check=True)
    return os.path.join(DIR, request.param)


def run(tool, case_words, d):
    src, dst = str(d / "cases.bin"), str(d / "results.bin")
    np.array([x for c in case_words for x in c], dtype="<u8").tofile(src)
    pr = subprocess.run([tool, src, dst], capture_output=True)
    assert pr.returncode == 0 and not pr.stderr, pr.stderr.decode()[-3000:]
    words, out, at = np.fromfile(dst, dtype="<u8"), [], 0
    while at < len(words):
        n = int(words[at])
        out.append([int(x) for x in words[at + 1:at + 1 + n]])
        at += 1 + n
    return out


def signed(x):
    return x - (1 << 64) if x >> 63 else x


def want_words(c):
    """the model's answer in the program's words (without the message), and the numbers the message carries"""
    rc, counts, order, piece, order_piece, numbers = vm.expect(c)
    w = [rc] + counts["records_in"] + counts["tail_lines"] + [counts["dropped_unpaired"]] + counts["records"] + counts["bytes"]
    w += [counts["format_error"], counts["format_input"], counts["format_record"], counts["range"]["read"],
          counts["range"]["pos"], counts["range"]["ch"]]
    assert len(w) == 1 + COUNT_WORDS
    if order is None:  # a struct the kind does not have is not touched
        w += [POISON64] * 5 + [POISON32] * 2 + [POISON64] * 2
    else:
        w += [order["batches"], order["units"], order["last_batch_units"]] + order["records_unbatched"] + \
            [order["stopped_on_mismatch"], order["long_line_input"], order["long_line"], order["error_batch"]]
    if piece is None:
        w += [POISON64] * 4 + [POISON32] * 2
    else:
        w += piece["consumed"] + piece["carried_bytes"] + [piece["ok"], piece["inherited_range"]]
    if order_piece is None:
        w += [POISON32] * 3 + [POISON64] * 8
    else:
        w += [order_piece["table_full"], order_piece["undetermined"], order_piece["inherited_failure"]] + order_piece["state"]
    assert len(w) == 1 + COUNT_WORDS + ORDER_WORDS + PIECE_WORDS + ORDER_PIECE_WORDS
    return w, numbers


def test_every_case_of_every_kind(tool, tmp_path):
    cases = vm.cases()
    got = run(tool, [vm.words(c) for c in cases], tmp_path)
    assert len(got) == len(cases)
    compared, seen = 0, set()
    for c, g in zip(cases, got):
        want, numbers = want_words(c)
        n = len(want)
        have = [signed(g[0])] + g[1:n]
        for at in (12, 17):  # format_error and range.ch are signed
            have[at] = signed(have[at])
        assert have == want, (c, have, want)
        message = bytes(g[n:]).decode()
        if numbers is None:
            assert message == "untouched", (c, message)
        else:
            # a number of the message stands between characters that are no digits
            fields = "".join(ch if ch.isdigit() or ch == "-" else " " for ch in message.replace(" - ", " ")).split()
            for x in numbers:
                assert str(x) in fields, (c, message, x)
        seen.add((c["kind"], want[0]))
        compared += 1
    assert compared == len(cases) and compared > 10000  # no case skipped or filtered
    # every return code the header states for a kind came up
    codes = {vm.PLAIN: {vm.SK_OK, vm.SK_EFORMAT, vm.SK_ERANGE, vm.SK_ESPACE}}
    codes[vm.PIECE] = codes[vm.PLAIN]
    codes[vm.ORDERED] = codes[vm.ORDERED_PIECE] = codes[vm.PLAIN] | {vm.SK_ELONGLINE}
    assert seen == {(k, rc) for k, rcs in codes.items() for rc in rcs}


def test_the_model_keeps_each_finish_its_own_precedence():
    """the sentences of include/sickle_amd.h, case by case, on the model alone"""
    base = dict(mode=vm.SE, inherited_range=0, failed=0, long_input=None, overflow=0, fmt=None, range=0, short=0, odd=0, more=0,
                tail=0)
    every = dict(base, fmt="odd", range=1, short=1)
    assert vm.verdict(dict(every, kind=vm.PLAIN))[1] == vm.SK_EFORMAT
    assert vm.verdict(dict(every, kind=vm.PLAIN, fmt=None))[1] == vm.SK_ERANGE
    assert vm.verdict(dict(every, kind=vm.PLAIN, fmt=None, range=0))[1] == vm.SK_ESPACE
    assert vm.verdict(dict(every, kind=vm.ORDERED, long_input=1, overflow=1))[1] == vm.SK_ELONGLINE
    assert vm.verdict(dict(every, kind=vm.ORDERED, overflow=1)) == ("overflow", vm.SK_ESPACE)
    assert vm.verdict(dict(every, kind=vm.ORDERED))[1] == vm.SK_EFORMAT
    assert vm.verdict(dict(every, kind=vm.PIECE, inherited_range=1)) == ("inherited_range", vm.SK_ERANGE)
    assert vm.verdict(dict(every, kind=vm.PIECE))[1] == vm.SK_EFORMAT
    assert vm.verdict(dict(every, kind=vm.ORDERED_PIECE, inherited_range=1, failed=1, long_input=0))[0] == "inherited_range"
    assert vm.verdict(dict(every, kind=vm.ORDERED_PIECE, failed=1, long_input=0)) == ("failed", vm.SK_OK)
    assert vm.verdict(dict(every, kind=vm.ORDERED_PIECE, long_input=0))[1] == vm.SK_ELONGLINE
    assert vm.verdict(dict(every, kind=vm.ORDERED_PIECE))[1] == vm.SK_EFORMAT
    assert vm.verdict(dict(base, kind=vm.ORDERED_PIECE)) == (None, vm.SK_OK)

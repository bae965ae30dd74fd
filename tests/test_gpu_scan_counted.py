"""sk_scan_counted_device_async on the GPU: an `offsets` batch of B reads whose read count n is a device word, on every
kernel such a batch can reach, against the oracle on the first n reads.  tests/scan_counted_util.py says how a case is
prepared (a sentinel in out, 0x01 in every byte at or beyond offsets[n], descending offsets behind offsets[n]) and holds the
shapes; every shape also runs at two words above the bound."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import scan_counted_util as scu

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [(enc, tn) for enc in scu.ENCODINGS for tn in (False, True)]
IDS = ["%s%s" % (enc, "-n" if tn else "") for enc, tn in CASES]
_drawn = {}


def batch(shape, enc):
    if (shape, enc) not in _drawn:
        _drawn[(shape, enc)] = scu.draw(shape, enc)
    return _drawn[(shape, enc)]


@pytest.fixture(scope="module")
def run(sk_ctx):
    return scu.Runner(sk_ctx)


@pytest.mark.parametrize("enc,tn", CASES, ids=IDS)
def test_uniform_150_on_the_tile_kernel(run, enc, tn):
    """20 000 reads of 150 bases: counts around a tile (64) and a regrouping window (8 192), none, one, all but one, all."""
    run.sweep(batch("uniform", enc), tn, scu.BIG_COUNTS)


@pytest.mark.parametrize("enc,tn", CASES, ids=IDS)
def test_ragged_600_to_3000_on_the_teams(run, enc, tn):
    """300 reads no tile takes, four to a wave: counts around a wave's four reads and a run of eight."""
    run.sweep(batch("ragged", enc), tn, (0, 1, 3, 4, 5, 16, 17, 299, 300))


@pytest.mark.parametrize("enc,tn", CASES, ids=IDS)
def test_long_reads_on_the_streaming_kernel(run, enc, tn):
    """40 reads of 5-40 kb behind a hint: spans of equal cost over n reads, more waves than reads."""
    run.sweep(batch("long", enc), tn, (0, 1, 7, 8, 9, 39, 40))


@pytest.mark.parametrize("enc,tn", CASES, ids=IDS)
def test_hand_over_of_one_tile(run, enc, tn):
    """200 reads, no hint, read 70 is 6 kb: the tile kernel leaves tile 1 to the streaming kernel -- unless the count
    ends before read 70 (n = 64, 70), then nothing is handed over and the kernel behind returns."""
    b = batch("handover", enc)
    assert b["lens"][70] == 6000 and b["lens"][:64].max() <= 300 and b["lens"][128:].max() <= 300
    run.sweep(b, tn, (64, 70, 71, 128, 129, 200))


@pytest.mark.parametrize("enc,tn", CASES, ids=IDS)
def test_every_tile_left(run, enc, tn):
    """130 reads of 5 kb, no hint: the tile kernel leaves every tile and counts them in word 6; the streaming kernel
    compares that count with the tiles of n reads and takes the batch in spans."""
    run.sweep(batch("all_left", enc), tn, (1, 64, 65, 130))


@pytest.mark.parametrize("kernel", ["band", "team", "stream"])
def test_forced_general_kernels(run, kernel):
    """SK_GENERAL (read at every launch) forces one general kernel: alone on the whole batch behind a hint beyond 4 096,
    and behind the tile kernel for the tile it leaves."""
    assert "SK_GENERAL" not in os.environ
    os.environ["SK_GENERAL"] = kernel
    try:
        run.sweep(batch("long", "sanger"), True, (0, 1, 9, 39))
        run.sweep(batch("handover", "illumina"), False, (64, 70, 71, 129))
        run.sweep(batch("ragged", "sanger"), True, (0, 1, 5, 17, 299))
    finally:
        del os.environ["SK_GENERAL"]


def test_regrouped_in_a_child_process():
    """SK_SORT_MIN=1 (read once per process): the mixed 30-504 shape at every count behind the regrouping, and uniform
    150 bp with n = 10 000 of 20 000 -- one run, under a time limit."""
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(HERE, "scan_counted_util.py"), "regrouped"],
                       capture_output=True, text=True, env=dict(os.environ, SK_SORT_MIN="1"))
    assert r.returncode == 0, "exit status %d\n%s%s" % (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    assert "regrouped ok" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("shape", ["uniform", "handover"])
def test_back_to_back_on_one_stream(run, shape):
    """a counted scan of 5 reads behind a full scan and the reverse, no finish in between: the hand-over words of the first
    must not reach the second."""
    b = batch(shape, "sanger")
    for first, second in ((b["B"], 5), (5, b["B"])):
        bufs1, bufs2 = run.prepared(b, first), run.prepared(b, second)
        w1, w2 = run.word(first), run.word(second)
        run.enqueue(b, True, bufs1, w1 if first != b["B"] else None)
        run.enqueue(b, True, bufs2, w2 if second != b["B"] else None)
        run.ctx.scan_device_finish()
        run.check(b, True, first, bufs1[3], "back to back, first")
        run.check(b, True, second, bufs2[3], "back to back, second")


def test_range_error_below_the_count_only(run):
    """a char out of range in read n - 1 is reported, with read n - 1; the same char in read n is not"""
    b = batch("uniform", "sanger")
    n = 8193
    dq, ds, do, out = run.prepared(b, b["B"])  # (the batch as it is: the only bad char is the planted one)
    w = run.word(n)
    dq[int(b["offs"][n - 1]) + 3] = 127
    run.enqueue(b, False, (dq, ds, do, out), w)
    with pytest.raises(run.capi.RangeError) as e:
        run.ctx.scan_device_finish()
    assert (e.value.read, e.value.pos, e.value.ch) == (n - 1, 3, 127)
    dq, ds, do, out = run.prepared(b, b["B"])
    dq[int(b["offs"][n]) + 3] = 127
    run.enqueue(b, False, (dq, ds, do, out), w)
    run.ctx.scan_device_finish()
    run.check(b, False, n, out, "a bad char in read n")


def test_null_word_is_the_plain_scan(run):
    b = batch("handover", "sanger")
    p = run.capi.make_params("sanger", 20, 20, False, True)
    bufs = run.prepared(b, b["B"])
    run.enqueue(b, True, bufs, None)
    run.ctx.scan_device_finish()
    dq, ds, do, out = run.prepared(b, b["B"])
    run.ctx.scan_device_async(p, dq.data_ptr(), out.data_ptr(), b["B"], stride=b["hint"], seq_ptr=ds.data_ptr(), offsets_ptr=do.data_ptr())
    run.ctx.scan_device_finish()
    assert (bufs[3].cpu().numpy() == out.cpu().numpy()).all()
    run.check(b, True, b["B"], out, "NULL word")


def test_argument_checks(run):
    """SK_EINVAL before anything is enqueued: a misaligned word, and a word with a fixed-stride batch, a batch with
    lengths, a segmented batch.  out keeps the sentinel."""
    t, capi = run.t, run.capi
    b = batch("uniform", "sanger")
    dq, ds, do, out = run.prepared(b, b["B"])
    word = run.word(5)
    lens = t.full((b["B"],), 150, dtype=t.int32, device="cuda")
    tiles = t.zeros(8, dtype=t.int32, device="cuda")  # (never read: the call fails on the host)
    p = capi.make_params("sanger")
    q, o, w = dq.data_ptr(), do.data_ptr(), word.data_ptr()
    cases = {
        "misaligned word": (capi.Batch(q, None, o, 150, 0, None, b["B"]), w + 4),
        "fixed stride": (capi.Batch(q, None, None, 150, 150, None, b["B"]), w),
        "lengths": (capi.Batch(q, None, None, 150, 0, lens.data_ptr(), b["B"]), w),
        "offsets and lengths": (capi.Batch(q, None, o, 150, 0, lens.data_ptr(), b["B"]), w),
        "segmented": (capi.Batch(q, None, None, 152, 0, None, 64, tiles.data_ptr(), 1, tiles.data_ptr()), w),
    }
    for name, (bt, wp) in cases.items():
        rc = capi.lib().sk_scan_counted_device_async(run.ctx._h, C.byref(p), C.byref(bt), wp, out.data_ptr(), None)
        assert rc == capi.SK_EINVAL, (name, rc)
        assert b"sk_scan_counted_device_async" in capi.lib().sk_last_error(run.ctx._h), (name, capi.lib().sk_last_error(run.ctx._h))
    run.ctx.scan_device_finish()
    assert (out.cpu().numpy() == scu.SENTINEL).all()

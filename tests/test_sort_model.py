"""The numpy model of the device-side regrouping (tests/sort_model.py) on hand-made windows, its checker against a second
writer of the same format, and the generator of tests/soak_sorted.py against the oracle alone (--dry).  No device."""
import numpy as np
import pytest

import soak_sorted
import sort_model as sm


def test_class_is_the_window_width_or_the_long_class():
    lens = [0, 1, 9, 10, 19, 20, 99, 100, 159, 160, 161, 629, 70_000]
    assert sm.class_of(lens, 160).tolist() == [0, 1, 9, 1, 1, 2, 9, 10, 15, 16, 63, 63, 63]
    assert sm.class_of(lens, 624).tolist() == [0, 1, 9, 1, 1, 2, 9, 10, 15, 16, 16, 63, 63]
    assert sm.class_of([620, 624], 624).max() == 62  # the widest window of a tile read stays below the long class


def test_sample_rule_by_hand():
    W, S = sm.WINDOW, sm.SAMPLE
    assert not sm.mixed([7]) and not sm.mixed([5, 5]) and sm.mixed([5, 6])
    lens = np.full(W + 10, 100)
    assert not sm.mixed(lens)
    lens[S] = 99  # just behind the first eighth: not looked at
    assert not sm.mixed(lens)
    lens[S - 1] = 99  # its last read
    assert sm.mixed(lens)
    lens = np.full(W + 10, 100)
    lens[W:] = 50  # another length in the second window, one length per window: each is compared with its own first read
    assert not sm.mixed(lens)
    lens[W + 9] = 51  # the partial window's sample is all of its 10 reads
    assert sm.mixed(lens)
    lens = np.full(2 * W + S + 5, 100)
    lens[2 * W + S + 4] = 1  # read 1 028 of the last window
    assert not sm.mixed(lens)


def test_counts_by_hand():
    W = sm.WINDOW
    # one window: 65 reads of 150..159 (class 15: two tiles), 3 empty reads (class 0), one of 7 (class 7), 2 beyond max_len
    lens = np.array([150] * 30 + [159] * 35 + [0] * 3 + [7] + [161, 70_000])
    c = sm.counts_of(sm.offsets_of(lens), 160)
    assert c.tolist() == [5, 0, 0, 0, 0, 0, 0, 0, 1, 2] + [0] * 6
    # one length as far as the sample sees: the verdict, and nothing else
    assert sm.counts_of(sm.offsets_of(np.full(500, 150)), 160).tolist() == [0] * 16
    # 9 windows + 5 reads: windows 0 and 8 share list 0, the partial window 9 goes to list 1
    lens = np.tile(np.array([100, 20]), (9 * W + 5 + 1) // 2)[:9 * W + 5]
    c = sm.counts_of(sm.offsets_of(lens), 304)
    assert c[:8].tolist() == [256, 128 + 2, 128, 128, 128, 128, 128, 128] and c[8] == 1 and c[9] == 0
    # k % 624: 63 classes in a window, 8192 = 13 * 624 + 80 reads: every class count is 130 or 140 but class 0..7's
    lens = sm.mix("k % 624", W, 624, None)
    per = sm.window_class_counts(lens, 624)[0]
    assert per[63] == 0 and (per[:63] > 0).all() and per.sum() == W
    tiles = int(((per + 63) // 64).sum())
    assert sm.counts_of(sm.offsets_of(lens), 624)[0] == tiles <= W // 64 + 63 <= sm.list_cap(W)


def test_fit_and_verdict():
    assert sm.fit_of(0) == 304 and sm.fit_of(640) == 624 and sm.fit_of(301) == 301 and sm.fit_of(100) == 100
    assert sm.fit_of(4096) == 624 and sm.fit_of(623) == 623
    offs = sm.offsets_of([100, 50, 300])
    assert sm.verdict(offs, 0) == "sorted" and sm.verdict(offs, 300) == "sorted"
    assert sm.verdict(offs, 299) == "long" and sm.verdict(offs, 5000) == "long"  # a stale hint, a long-read hint
    assert sm.verdict(sm.offsets_of([100] * 3), 0) == "plain"
    assert sm.verdict(sm.offsets_of([100, 50, 305]), 0) == "long" and sm.verdict(sm.offsets_of([100, 50, 305]), 305) == "sorted"


CHECKED = [(name, n, 160 if name != "k % 624" else 624) for name in sm.MIXES for n in (1, 65, 1025, 8193)] + [("0..40", 9 * 8192 + 5, 48)]


@pytest.mark.parametrize("name,n,max_len", CHECKED)
def test_check_accepts_a_second_writer(name, n, max_len):
    rng = np.random.default_rng(n)
    offs = sm.offsets_of(sm.mix(name, n, max_len, rng))
    sm.check(offs, max_len, *sm.emulate(offs, max_len, rng))


def test_check_sees_what_is_wrong():
    rng = np.random.default_rng(3)
    offs = sm.offsets_of(sm.mix("0..40", 8192 + 700, 48, rng))
    good = sm.emulate(offs, 48, rng)
    sm.check(offs, 48, *good)
    u = np.uint64

    def spoiled(fn):
        counts, lists, perm = (a.copy() for a in good)
        fn(counts, lists, perm)
        with pytest.raises(AssertionError):
            sm.check(offs, 48, counts, lists, perm)

    def swap_entries(c, l, p):  # two reads of different tiles trade places: a read in a tile of another class
        p[0, 0, 0], p[0, int(c[0]) - 1, 0] = p[0, int(c[0]) - 1, 0], p[0, 0, 0]

    def twice(c, l, p):
        p[0, 0, 1] = p[0, 0, 0]

    def one_more_tile(c, l, p):
        l[1, int(c[1])] = l[1, int(c[1]) - 1]

    def stray_entry(c, l, p):
        p[1, int(c[1]), 5] = 0

    def wrong_offset(c, l, p):
        p[1, 0, 0] += u(1)

    def wrong_number(c, l, p):
        p[0, 0, 0] ^= u(1) << u(48)

    def wrong_lmax(c, l, p):
        l[0, 0, 3] += u(1)

    def wrong_lmin(c, l, p):
        l[0, 0, 3] += u(1) << u(16)

    def wrong_span(c, l, p):
        l[0, 0, 2] += u(1)

    def wrong_window(c, l, p):
        l[0, 0, 0] += u(8)

    def count_low(c, l, p):
        c[0] -= 1

    def long_count(c, l, p):
        c[9] += 1

    def split_window(c, l, p):  # list 0 holds one window only here; pretend a tile of it sits behind another window's
        l[0, 0, 0], l[0, 0, 1] = l[0, 0, 0] + u(8), l[0, 0, 1]

    for fn in (swap_entries, twice, one_more_tile, stray_entry, wrong_offset, wrong_number, wrong_lmax, wrong_lmin, wrong_span,
               wrong_window, count_low, long_count, split_window):
        spoiled(fn)
    # a partial tile that is not its class's last
    offs2 = sm.offsets_of(np.array([30] * 100 + [50] * 10))
    counts, lists, perm = sm.emulate(offs2, 48, rng)
    sm.check(offs2, 48, counts, lists, perm)
    lists[0, [0, 1]], perm[0, [0, 1]] = lists[0, [1, 0]], perm[0, [1, 0]]
    with pytest.raises(AssertionError, match="not full"):
        sm.check(offs2, 48, counts, lists, perm)
    # one length: nothing may be written
    offs3 = sm.offsets_of(np.full(100, 150))
    counts, lists, perm = sm.emulate(offs3, 160, rng)
    perm[3, 0, 0] = 0
    with pytest.raises(AssertionError, match="something was written"):
        sm.check(offs3, 160, counts, lists, perm)


def test_soak_generator_dry():
    """Every generator of tests/soak_sorted.py with the oracle alone: the planted chars are seen (or, behind the 3' break,
    not seen) by the reference as the soak assumes, and a default run's batches are of all three kinds -- at least half
    of them regrouped, at least a tenth each left to the plain kernel and to the long-read kernels."""
    stats = {}
    assert soak_sorted.run(verbose=False, dry_run=True, stats=stats) == 224
    total = sum(stats.values())
    assert total == 44
    assert 2 * stats["sorted"] >= total and 10 * stats["plain"] >= total and 10 * stats["long"] >= total, stats


def test_soak_refuses_without_the_switch(monkeypatch):
    monkeypatch.delenv("SK_SORT_MIN", raising=False)
    with pytest.raises(SystemExit):
        soak_sorted.run(1, 1, verbose=False)
    monkeypatch.setenv("SK_SORT_MIN", "1")
    monkeypatch.setenv("SK_SORT", "0")
    with pytest.raises(SystemExit):
        soak_sorted.run(1, 1, verbose=False)

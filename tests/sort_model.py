"""TEST INFRASTRUCTURE.  The device-side regrouping of ragged batches (sickle_amd/csrc/sk_sort.hip) as a plain function
of the offsets, in numpy -- written from that file's comments, not from its kernels:

  the batch is cut into windows of 8 192 consecutive reads; window k's tiles go to list k mod 8;
  counts[8] = 1 iff in some window the first min(1 024, reads in the window) reads do not all have the first one's
              length; if it is 0 nothing else is written;
  counts[9] = the reads longer than max_len;
  counts[x], x < 8 = the tiles of list x: per window and class ceil(reads of the class / 64), the class of a read of
              L bases being L // 10 or L (its window width), or 63 when L > max_len;
  a tile:     a descriptor {window, rows, class; where the window starts; its bytes; longest | shortest << 16} and 64
              entries, the first `rows` of them {offset inside the window, min(L, 65 535), number inside the window}.

Which window of a list comes first, and which read of a class comes first, is decided by atomics: check() compares
those order-free.  emulate() is a second, deliberately different writer of the same format (a host-side stand-in for
the device, in a drawn order), so that check() itself is tested without a device (tests/test_sort_model.py).

Also here: the offsets of the cases both the probe test and the soak run (mixes(), NS, MAX_LENS), and what the library
does with a batch by its offsets and the caller's hint (verdict())."""
import numpy as np

WINDOW = 8192
SAMPLE = WINDOW // 8
ROWS = 64
LISTS = 8
LONG_CLASS = 63
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)
NS = (1, 2, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 9 * 8192 + 5, 70_000)
MAX_LENS = (48, 160, 304, 624)
# the tile buffers' bounds (sk_device.h): what a wave's LDS takes without a hint / at most, the longest tile read with them
FIT_DEFAULT, FIT_MAX, LONG_HINT = 304, 624, 4096


def lengths_of(offsets):
    return np.diff(np.asarray(offsets, dtype=np.uint64).astype(np.int64))


def offsets_of(lens):
    offs = np.zeros(len(lens) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(np.asarray(lens, dtype=np.int64))
    return offs


def class_of(lens, max_len):
    lens = np.asarray(lens, dtype=np.int64)
    w = np.where(lens // 10 > 0, lens // 10, lens)
    return np.where(lens > max_len, LONG_CLASS, w)


def list_cap(n):
    """tiles per list, as the library sizes its scratch for n reads"""
    windows = (n + WINDOW - 1) // WINDOW
    per_list = ((windows + 7) // 8) * (WINDOW // ROWS + 64) + 8
    return per_list + (per_list >> 3)


def mixed(lens):
    """the sample rule: counts[8]"""
    lens = np.asarray(lens, dtype=np.int64)
    for r0 in range(0, len(lens), WINDOW):
        head = lens[r0:min(r0 + SAMPLE, len(lens))]
        if (head != head[0]).any():
            return True
    return False


def window_class_counts(lens, max_len):
    """reads per (window, class): [windows, 64]"""
    lens = np.asarray(lens, dtype=np.int64)
    windows = (len(lens) + WINDOW - 1) // WINDOW
    key = (np.arange(len(lens)) // WINDOW) * 64 + class_of(lens, max_len)
    return np.bincount(key, minlength=windows * 64).reshape(windows, 64)


def counts_of(offsets, max_len):
    """the 16 counter words after one regrouping"""
    lens = lengths_of(offsets)
    c = np.zeros(16, dtype=np.uint32)
    if not mixed(lens):
        return c
    c[8] = 1
    c[9] = int((lens > max_len).sum())
    tiles = ((window_class_counts(lens, max_len) + ROWS - 1) // ROWS).sum(axis=1)
    for w, t in enumerate(tiles):
        c[w % LISTS] += int(t)
    return c


def fit_of(hint):
    """the longest read the tiles take, by the caller's longest-read hint (0 = none): enqueue_scan's `fit`"""
    if hint == 0:
        return FIT_DEFAULT
    pitch = 16 * (((hint + 15) >> 4) | 1)
    buf = min(max((64 * pitch + 128 + 15) & ~15, 4096), 40 * 1024)
    best = 0
    for L in range(16, 2041, 16):
        if 64 * 16 * ((L >> 4) | 1) + 128 <= buf:
            best = L
    return min(best, hint)


def verdict(offsets, hint):
    """'sorted': the regrouped scan takes the batch; 'plain': one length as far as the sample sees, the plain tile kernel
    keeps it; 'long': reads beyond the tiles (or a hint that says so), the tile + general pair or the general kernels."""
    lens = lengths_of(offsets)
    if hint > LONG_HINT:
        return "long"
    if not mixed(lens):
        return "plain"
    return "long" if (lens > fit_of(hint)).any() else "sorted"


# ---------------------------------------------------------------------------------------------------------- the cases
MIXES = ("0..9", "0..40", "one class", "two lengths", "75..301", "k % 624", "around max_len", "empty tail", "uniform",
         "uniform eighths", "last window only")


def mix(name, n, max_len, rng):
    """lengths of n reads"""
    k = np.arange(n, dtype=np.int64)
    if name == "0..9":
        return rng.integers(0, 10, size=n)
    if name == "0..40":
        return rng.integers(0, 41, size=n)
    if name == "one class":
        return rng.integers(150, 160, size=n)
    if name == "two lengths":
        return np.where(rng.random(n) < 0.5, 36, 151).astype(np.int64)
    if name == "75..301":
        return rng.integers(75, 302, size=n)
    if name == "k % 624":  # 63 classes in every window, every class with a partial tile
        return (k % WINDOW) % 624
    if name == "around max_len":
        lens = rng.integers(1, 45, size=n)
        at = rng.random(n)
        lens[at < 0.02] = max_len
        lens[(at >= 0.02) & (at < 0.04)] = max_len + 1
        lens[(at >= 0.04) & (at < 0.043)] = 65_535 + rng.integers(0, 3, size=int(((at >= 0.04) & (at < 0.043)).sum()))
        return lens
    if name == "empty tail":  # what the FASTQ front hands over: the last 30 % are empty reads
        lens = rng.integers(75, 152, size=n)
        lens[n - (3 * n) // 10:] = 0
        return lens
    if name == "uniform":
        return np.full(n, 150, dtype=np.int64)
    if name == "uniform eighths":  # one length wherever the sample looks, mixed elsewhere
        lens = rng.integers(30, 200, size=n)
        lens[(k % WINDOW) < SAMPLE] = 100
        return lens
    if name == "last window only":  # one length, but for the first eighth of the last (partial) window
        lens = np.full(n, 100, dtype=np.int64)
        r0 = ((n - 1) // WINDOW) * WINDOW
        head = min(n, r0 + SAMPLE) - r0
        lens[r0:r0 + head] = rng.integers(20, 140, size=head)
        return lens
    raise KeyError(name)


def cases(seed=7):
    """(name, n, max_len, offsets) of every case of the probe test"""
    rng = np.random.default_rng(seed)
    for max_len in MAX_LENS:
        for name in MIXES:
            for n in NS:
                yield name, n, max_len, offsets_of(mix(name, n, max_len, rng))


# ------------------------------------------------------------------------------------------------------------ the check
def check(offsets, max_len, counts, lists, perm):
    """counts[16], lists[8, cap, 4], perm[8, cap, 64] (uint64, pre-filled with SENTINEL) after one regrouping of `offsets`:
    raises AssertionError with what is wrong."""
    offsets = np.asarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    lens = lengths_of(offsets)
    counts = np.asarray(counts, dtype=np.uint32)
    cap = lists.shape[1]
    assert lists.shape == (LISTS, cap, 4) and perm.shape == (LISTS, cap, ROWS), (lists.shape, perm.shape)
    want = counts_of(offsets, max_len)
    assert (counts[:10] == want[:10]).all(), ("counts", counts[:10].tolist(), want[:10].tolist())
    assert (counts[10:] == 0).all(), ("counts[10..15]", counts[10:].tolist())
    if not counts[8]:
        assert (lists == SENTINEL).all() and (perm == SENTINEL).all(), "a batch of one length: something was written"
        return
    windows = (n + WINDOW - 1) // WINDOW
    per_key = window_class_counts(lens, max_len).reshape(-1)  # reads per window * 64 + class
    cls_of_read = class_of(lens, max_len)
    seen = []
    u = np.uint64
    for x in range(LISTS):
        T = int(counts[x])
        assert T <= cap, ("list %d: %d tiles, room for %d" % (x, T, cap))
        assert (lists[x, T:] == SENTINEL).all(), "list %d: a descriptor at or beyond tile %d" % (x, T)
        assert (perm[x, T:] == SENTINEL).all(), "list %d: an entry at or beyond tile %d" % (x, T)
        if T == 0:
            continue
        d, e = lists[x, :T], perm[x, :T]
        widx = (d[:, 0] & u((1 << 48) - 1)).astype(np.int64)
        rows = ((d[:, 0] >> u(48)) & u(0xff)).astype(np.int64)
        cls = (d[:, 0] >> u(56)).astype(np.int64)
        lmax, lmin = (d[:, 3] & u(0xffff)).astype(np.int64), ((d[:, 3] >> u(16)) & u(0xffff)).astype(np.int64)
        assert (d[:, 3] >> u(32) == 0).all(), "list %d: descriptor word 3 beyond its 32 bits" % x
        assert ((widx < windows) & (widx % LISTS == x)).all(), ("list %d holds windows" % x, np.unique(widx).tolist())
        assert ((rows >= 1) & (rows <= ROWS)).all(), ("list %d: rows" % x, rows.min(), rows.max())
        first = widx * WINDOW
        last = np.minimum(first + WINDOW, n)
        assert (d[:, 1] == offsets[first]).all(), "list %d: where a window starts" % x
        assert (d[:, 2] == offsets[last] - offsets[first]).all(), "list %d: a window's bytes" % x
        # a window's tiles are contiguous: as many runs of one window as windows
        runs = 1 + int((widx[1:] != widx[:-1]).sum())
        assert runs == len(np.unique(widx)), "list %d: a window's tiles are not contiguous (%d runs)" % (x, runs)
        # per (window, class): ceil(count / 64) tiles, all full but the last in list order
        key = widx * 64 + cls
        order = np.argsort(key, kind="stable")
        ks, rs = key[order], rows[order]
        starts = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
        ends = np.r_[starts[1:], len(ks)]
        gk, gn = ks[starts], ends - starts
        mine = np.flatnonzero((np.arange(windows * 64) // 64) % LISTS == x)
        mine = mine[per_key[mine] > 0]
        assert np.array_equal(gk, mine), ("list %d: (window, class) pairs with tiles" % x, gk.tolist()[:20], mine.tolist()[:20])
        assert np.array_equal(gn, (per_key[gk] + ROWS - 1) // ROWS), ("list %d: tiles per (window, class)" % x)
        is_last = np.zeros(len(ks), dtype=bool)
        is_last[ends - 1] = True
        assert (rs[~is_last] == ROWS).all(), "list %d: a class's tile before its last is not full" % x
        assert np.array_equal(rs[is_last], per_key[gk] - ROWS * (gn - 1)), "list %d: rows of a class's last tile" % x
        # the entries
        live = np.arange(ROWS)[None, :] < rows[:, None]
        tile_of = np.broadcast_to(np.arange(T)[:, None], (T, ROWS))[live]
        ent = e[live]
        off, ln, k = ent & u(0xffffffff), ((ent >> u(32)) & u(0xffff)).astype(np.int64), (ent >> u(48)).astype(np.int64)
        r = first[tile_of] + k
        assert (r < last[tile_of]).all(), "list %d: an entry names a read beyond its window" % x
        assert (off == offsets[r] - offsets[first[tile_of]]).all(), "list %d: an entry's offset is not its read's" % x
        assert (ln == np.minimum(lens[r], 0xffff)).all(), "list %d: an entry's length is not its read's" % x
        assert (cls_of_read[r] == cls[tile_of]).all(), "list %d: a read in a tile of another class" % x
        t0 = np.flatnonzero(np.r_[True, tile_of[1:] != tile_of[:-1]])
        assert np.array_equal(np.maximum.reduceat(ln, t0), lmax), "list %d: a tile's longest read" % x
        assert np.array_equal(np.minimum.reduceat(ln, t0), lmin), "list %d: a tile's shortest read" % x
        seen.append(r)
    seen = np.sort(np.concatenate(seen)) if seen else np.zeros(0, dtype=np.int64)
    assert len(seen) == n and np.array_equal(seen, np.arange(n)), "the tiles do not hold every read exactly once (%d of %d)" % (len(seen), n)


def emulate(offsets, max_len, rng, cap=None):
    """(counts, lists, perm) as a device might leave them: windows of a list and reads of a class in a drawn order"""
    offsets = np.asarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    lens = lengths_of(offsets)
    cap = list_cap(n) if cap is None else cap
    counts = np.zeros(16, dtype=np.uint32)
    lists = np.full((LISTS, cap, 4), SENTINEL, dtype=np.uint64)
    perm = np.full((LISTS, cap, ROWS), SENTINEL, dtype=np.uint64)
    if not mixed(lens):
        return counts, lists, perm
    counts[8] = 1
    counts[9] = int((lens > max_len).sum())
    cls = class_of(lens, max_len)
    for w in rng.permutation((n + WINDOW - 1) // WINDOW):
        r0, r1 = int(w) * WINDOW, min(n, (int(w) + 1) * WINDOW)
        x = int(w) % LISTS
        for c in range(64):
            members = rng.permutation(np.flatnonzero(cls[r0:r1] == c))
            for j in range(0, len(members), ROWS):
                ks = members[j:j + ROWS]
                t = int(counts[x])
                counts[x] += 1
                L = np.minimum(lens[r0 + ks], 0xffff)
                lists[x, t] = [w | (len(ks) << 48) | (c << 56), int(offsets[r0]), int(offsets[r1] - offsets[r0]),
                               int(L.max()) | (int(L.min()) << 16)]
                perm[x, t, :len(ks)] = (offsets[r0 + ks] - offsets[r0]) | (L.astype(np.uint64) << np.uint64(32)) | (ks.astype(np.uint64) << np.uint64(48))
    return counts, lists, perm

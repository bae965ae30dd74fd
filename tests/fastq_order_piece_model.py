"""Python restatement of sk_trim_fastq_ordered_piece_device_async (include/sickle_amd.h): the reader's rule walked over a
window from a state, the batches a piece commits, what it consumed, the state it hands on, and its outputs in the -a T
order, on top of tests/fastq_order_model.py (the order inside a batch) and tests/fastq_model.py (framing, checks, the
oracle's cuts, the record format).  stream() drives it the way a caller does, with the carry in front of every chunk.  The
tests compare the device, and the whole-text model, against it; it never reads anything the device made."""
import numpy as np

import fastq_model as fm
import fastq_order_model as om

NONE = om.NONE
START = {"carried": [0, 0], "batches": 0, "units": 0, "last_batch_units": 0, "ended": 0, "stopped_on_mismatch": 0, "failed": 0}


def window_lines(window, more):
    """the lines of a window: with more text to come a line exists only if its '\\n' lies in the window"""
    if more:
        return bytes(window).split(b"\n")[:-1]
    return om.lines_of(bytes(window))


def next_stop(lines, a, c, batch_len, more):
    """The reader, which holds lines [a, c), takes line after line until their lengths have used up batch_len (one at
    least).  -> (e, input_ended), or None when the window cannot tell where it stops."""
    left = batch_len - sum(len(l) for l in lines[a:c])
    e = c
    while True:
        if e >= len(lines):  # no line to take
            return None if more else (e, True)
        left -= len(lines[e])
        e += 1
        if left <= 0:
            return e, False


def walk(line_lists, mode, batch_len, capacity, limit, state, more):
    """-> dict(first_unit, a: committed lines per input, carried: the new k_i, batches: per input the committed line
    lists, mismatch, ended, table_full, undetermined)"""
    m = om.LINES_PER_UNIT[mode]
    n_in = len(line_lists)
    a = [0] * n_in
    c = [min(state["carried"][i], len(line_lists[i])) for i in range(n_in)]
    fin = [False] * n_in
    r = {"first_unit": [0], "batches": [[] for _ in range(n_in)], "mismatch": 0, "ended": state["ended"], "table_full": 0,
         "undetermined": 0}
    while not r["ended"]:
        if limit and state["batches"] + len(r["first_unit"]) - 1 >= limit:
            r["ended"] = 1
            break
        stops = [(0, True) if fin[i] else next_stop(line_lists[i], a[i], c[i], batch_len, more) for i in range(n_in)]
        size = [None if s is None else 0 if fin[i] else (s[0] - a[i]) - (s[0] - a[i]) % m for i, s in enumerate(stops)]
        if size[0] == 0:
            r["ended"] = 1
        elif None in size:
            r["undetermined"] = 1
        elif n_in == 2 and size[1] == 0:
            r["ended"] = 1
        elif n_in == 2 and size[0] != size[1]:
            r["ended"] = r["mismatch"] = 1
        elif len(r["first_unit"]) - 1 == capacity:
            r["table_full"] = 1
        else:
            for i in range(n_in):
                r["batches"][i].append(line_lists[i][a[i]:a[i] + size[i]])
                a[i] += size[i]
                c[i], fin[i] = stops[i]
            r["first_unit"].append(r["first_unit"][-1] + size[0] // m)
            continue
        break
    r["a"], r["carried"] = a, [c[i] - a[i] for i in range(n_in)]
    return r


def _pad(xs, fill=0):
    return list(xs) + [fill] * (2 - len(xs))


def piece(ptuple, windows, mode, more, threads, batch_len, capacity, limit=0, state=None, range_set=False, fits=True):
    """One ordered piece on the texts `windows` from `state` (None: the start of a stream).  range_set: the stream's
    range-error word was set when the piece began; fits: its outputs' buffers hold what it emits.  Offsets count from the
    window's start, read numbers from the piece's first record."""
    state = dict(START if state is None else state)
    windows = [bytes(w) for w in windows]
    n_in = len(windows)
    res = {"inherited_range": int(range_set), "inherited_failure": int(bool(state["failed"])), "long_line": None, "verdict": None,
           "range": None, "texts": None, "index": None, "error_batch": NONE, "table_full": 0, "undetermined": 0, "ok": 0,
           "first_unit": [0], "records_in": [0, 0], "tail_lines": [0, 0], "consumed": [0, 0],
           "carried_bytes": _pad([len(w) for w in windows]),
           "order": {"batches": 0, "units": 0, "last_batch_units": 0, "stopped_on_mismatch": 0, "records_unbatched": [0, 0]}}
    if range_set or state["failed"]:  # void
        res["state"] = dict(state, failed=1)
        return res
    lines = [window_lines(w, more) for w in windows]
    w = walk(lines, mode, batch_len, capacity, limit, state, more)
    nb, units = len(w["first_unit"]) - 1, w["first_unit"][-1]
    last = w["first_unit"][-1] - w["first_unit"][-2] if nb else 0
    consumed = [min(sum(len(l) + 1 for l in lines[i][:w["a"][i]]), len(windows[i])) for i in range(n_in)]
    res.update(first_unit=w["first_unit"], table_full=w["table_full"], undetermined=w["undetermined"],
               records_in=_pad([x // 4 for x in w["a"]]), tail_lines=_pad([len(lines[i]) - w["a"][i] for i in range(n_in)]),
               consumed=_pad(consumed), carried_bytes=_pad([len(windows[i]) - consumed[i] for i in range(n_in)]))
    res["order"] = {"batches": nb, "units": units, "last_batch_units": last, "stopped_on_mismatch": w["mismatch"],
                    "records_unbatched": _pad([len(lines[i]) // 4 - w["a"][i] // 4 for i in range(n_in)])}
    advanced = dict(state, carried=_pad(w["carried"]), batches=state["batches"] + nb, units=state["units"] + units,
                    last_batch_units=last if nb else state["last_batch_units"], ended=int(w["ended"]),
                    stopped_on_mismatch=int(state["stopped_on_mismatch"] or w["mismatch"]))
    res["state"] = dict(state, failed=1)  # unless everything below passes
    for i in range(n_in):
        for l, line in enumerate(lines[i]):
            if len(line) >= batch_len - 1 and res["long_line"] is None:
                res["long_line"] = (i, l)
    if res["long_line"] is not None:
        return res
    per_unit = 1 if mode == "se" else 2
    if units == 0:  # nothing committed: empty outputs
        res["texts"] = [b"" if o in fm.USED[mode] else None for o in range(3)]
        res["index"] = [np.zeros(0, np.int64) if o in fm.USED[mode] else None for o in range(3)]
        if fits:
            res["ok"], res["state"] = 1, advanced
        return res
    # the committed records, in read order, as the ordered call treats a text made of them
    buf, recs = fm.reads([w_[:c] for w_, c in zip(windows, consumed)], mode)
    assert len(recs["s0"]) == units * per_unit
    why = fm.reasons(buf, recs)
    bad = np.flatnonzero(why)
    batch_of = lambda read: int(np.searchsorted(w["first_unit"], read // per_unit, side="right") - 1) + state["batches"]
    if len(bad):
        read = int(bad[0])
        i, k = (read & 1, read >> 1) if mode == "pe_split" else (0, read)
        res["verdict"], res["error_batch"] = (int(why[read]), i, k), batch_of(read)
        return res
    cuts, err = fm.oracle_cuts(ptuple, buf, recs)
    if err is not None:
        res["range"], res["error_batch"] = tuple(int(x) for x in err), batch_of(int(err[0]))
        return res
    cuts = np.asarray(cuts, dtype=np.int64).reshape(-1, 2)
    order = om.read_order(w["first_unit"], threads, mode)
    out_texts, index = fm.emit(buf, {k: v[order] for k, v in recs.items()}, cuts[order], mode)
    res["texts"], res["index"] = out_texts, [None if ix is None else order[ix] for ix in index]
    if fits:
        res["ok"], res["state"] = 1, advanced
    return res


def _measure(carry):
    """(bytes of the complete lines without their newlines, bytes behind the last newline) of a carry"""
    n, last = carry.count(b"\n"), carry.rfind(b"\n")
    return last + 1 - n, len(carry) - last - 1


def stream(ptuple, texts, mode, threads, batch_len, piece_bytes, capacity, limit=0, stop_at_end=True, keep_pieces=False):
    """texts cut into chunks of piece_bytes (every input alike), piece by piece with the carry in front and the state
    handed on; closing pieces are repeated on the carry while the table was full.  stop_at_end: no piece behind the one
    that ends the run (they would take nothing).  -> dict: texts and index (stream-wide read numbers) joined, the summed
    counts, first_unit (stream-wide), state, n_pieces, pieces (with keep_pieces: each piece()'s dict with its windows,
    `more` and reads_before), error: None or ("long", input, line) / ("format", why, input, record, batch) / ("range",
    read, pos, ch, batch), stream-wide but for the long line's, which counts within its piece.
    Without keep_pieces a piece that cannot commit anything is not worked out: while input 0's complete lines hold fewer
    than batch_len bytes its batch is undetermined, whatever else the window holds, so the piece takes nothing and hands
    the state on as it is (a line of batch_len - 1 bytes or more that the chunk completed sends it through piece())."""
    texts = [bytes(t) for t in texts]
    n_in = len(texts)
    at, carried = [0] * n_in, [bytearray() for _ in texts]
    content, partial = [0] * n_in, [0] * n_in
    out = {"texts": [b"" if o in fm.USED[mode] else None for o in range(3)], "index": [[] for _ in range(3)],
           "records_in": [0, 0], "records": [0, 0, 0], "bytes": [0, 0, 0], "first_unit": [0], "pieces": [], "n_pieces": 0,
           "error": None, "state": dict(START)}
    parts = [[] for _ in range(3)]
    reads, state, closing = 0, dict(START), False
    while True:
        long_seen = False
        for i in range(n_in):
            chunk = b"" if closing else texts[i][at[i]:at[i] + piece_bytes]
            at[i] += len(chunk)
            carried[i] += chunk
            n = chunk.count(b"\n")
            if n:
                done = chunk[:chunk.rindex(b"\n")].split(b"\n")
                long_seen = long_seen or partial[i] + len(done[0]) >= batch_len - 1 or any(len(l) >= batch_len - 1 for l in done[1:])
                content[i] += partial[i] + sum(len(l) for l in done)
                partial[i] = len(chunk) - chunk.rindex(b"\n") - 1
            else:
                partial[i] += len(chunk)
        more = any(at[i] < len(texts[i]) for i in range(n_in))
        out["n_pieces"] += 1
        if more and not keep_pieces and not long_seen and not state["ended"] and content[0] < batch_len and \
                not (limit and state["batches"] >= limit):
            continue
        windows = [bytes(c) for c in carried]
        p = piece(ptuple, windows, mode, more, threads, batch_len, capacity, limit, state)
        if keep_pieces:
            p["windows"], p["more"], p["reads_before"] = windows, more, reads
            out["pieces"].append(p)
        per_input = reads // 2 if mode == "pe_split" else reads
        if p["long_line"] is not None:
            out["error"] = ("long",) + p["long_line"]
        elif p["verdict"] is not None:
            out["error"] = ("format", p["verdict"][0], p["verdict"][1], p["verdict"][2] + per_input, p["error_batch"])
        elif p["range"] is not None:
            out["error"] = ("range", p["range"][0] + reads, p["range"][1], p["range"][2], p["error_batch"])
        if out["error"] is not None:
            break
        for o in fm.USED[mode]:
            parts[o].append(p["texts"][o])
            out["index"][o] += [int(x) + reads for x in p["index"][o]]
            out["records"][o] += len(p["index"][o])
            out["bytes"][o] += len(p["texts"][o])
        base = out["first_unit"][-1]
        out["first_unit"] += [base + x for x in p["first_unit"][1:]]
        for i in range(n_in):
            out["records_in"][i] += p["records_in"][i]
            del carried[i][:p["consumed"][i]]
            content[i], partial[i] = _measure(carried[i])
        reads += p["order"]["units"] * (1 if mode == "se" else 2)
        state = p["state"]
        if (state["ended"] and stop_at_end) or (not more and not p["table_full"]):
            break
        closing = not more
    out["state"] = state
    for o in fm.USED[mode]:
        out["texts"][o] = b"".join(parts[o])
    return out

"""Python restatement of the piece rule of sk_trim_fastq_piece_device_async and of sk_fastq_carry_device_async
(include/sickle_amd.h): the window, the records a piece takes (u), what it consumed, the carry and its sticky status, and
the outputs via tests/fastq_model.py's expected() on the consumed records.  The tests compare the device against it; it
never reads anything the device made."""
import fastq_model as fm


def take(r, mode):
    """records each input gives a piece with more text to come, from the complete records r[i] of its window"""
    if mode == "pe_split":
        return min(r[0], r[1])
    return r[0] & ~1 if mode == "pe_interleaved" else r[0]


def _nth_newline_end(buf, n):
    """one past the n-th '\\n' (n >= 1) of buf"""
    at = -1
    for _ in range(n):
        at = buf.index(b"\n", at + 1)
    return at + 1


def piece(ptuple, windows, mode, more):
    """One piece on the texts `windows` (each text[i][s_i:n_i], bytes).  -> dict: u, records_in, tail_lines,
    dropped_unpaired, consumed and carried (per input, consumed counted from the window's start) and `res`, what
    fm.expected gives on the records the piece takes (verdict, range, texts, index: numbers count within the piece)."""
    windows = [bytes(w) for w in windows]
    if not more:
        res = fm.expected(ptuple, windows, mode)
        return {"u": None, "records_in": res["records_in"], "tail_lines": res["tail_lines"],
                "dropped_unpaired": res["dropped_unpaired"], "consumed": [len(w) for w in windows] + [0] * (2 - len(windows)),
                "carried": [0, 0], "res": res}
    lines = [w.count(b"\n") for w in windows]  # a line exists only if its '\n' lies in the window
    u = take([n // 4 for n in lines], mode)
    consumed = [_nth_newline_end(w, 4 * u) if u else 0 for w in windows]
    res = fm.expected(ptuple, [w[:c] for w, c in zip(windows, consumed)], mode)
    assert res["records_in"][:len(windows)] == [u] * len(windows) and res["dropped_unpaired"] == 0
    assert res["verdict"] is None or res["verdict"][0] != fm.SK_FQ_PAIR_COUNT
    pad = lambda xs: list(xs) + [0] * (2 - len(xs))
    return {"u": u, "records_in": pad([u] * len(windows)), "tail_lines": pad([n - 4 * u for n in lines]),
            "dropped_unpaired": 0, "consumed": pad(consumed), "carried": pad([len(w) - c for w, c in zip(windows, consumed)]),
            "res": res}


def carry(c, ok, room, chunk_len, chunk_valid=None, prev_status=0, other_status=0):
    """sk_fastq_carry_device_async's words for a carry of c bytes behind a piece whose ok word is `ok`:
    -> (start, end, valid, status)"""
    if prev_status:
        status = prev_status
    elif other_status:
        status = other_status
    elif not ok:
        status = 1
    elif c > room:
        status = 2
    elif chunk_valid is not None and chunk_valid == 0:
        status = 3
    else:
        status = 0
    return (room, room, 0, status) if status else (room - c, room + chunk_len, 1, 0)


def ok_of(p):
    """a piece's ok word, with outputs that fit and a clear range-error word when it began"""
    return int(p["res"]["verdict"] is None and p["res"]["range"] is None)


def stream(ptuple, texts, mode, piece_bytes, room=None):
    """texts cut into chunks of piece_bytes (every input alike), piece by piece with the carry in front.  -> dict: texts
    (each output's concatenation), records_in / records / bytes (sums), tail_lines and dropped_unpaired (the last
    piece's), index (read numbers, stream-wide), pieces, consumed_pieces (pieces with u > 0), and error: None, or
    ("format", reason, input, record), ("range", read, pos, ch) with stream-wide numbers, or ("room", input): the stream
    stops at the first failing piece, as a sticky status makes it."""
    room = piece_bytes if room is None else room
    texts = [bytes(t) for t in texts]
    n_in = len(texts)
    at, carried, lines = [0] * n_in, [bytearray() for _ in texts], [0] * n_in
    out = {"texts": [b"" if o in fm.USED[mode] else None for o in range(3)], "index": [[] for _ in range(3)],
           "records_in": [0, 0], "records": [0, 0, 0], "bytes": [0, 0, 0], "tail_lines": [0, 0], "dropped_unpaired": 0,
           "pieces": 0, "consumed_pieces": 0, "error": None}
    parts = [[] for _ in range(3)]
    reads = 0
    while True:
        for i in range(n_in):
            if len(carried[i]) > room:
                out["error"] = ("room", i)
                return _joined(out, parts)
            chunk = texts[i][at[i]:at[i] + piece_bytes]
            at[i] += len(chunk)
            carried[i] += chunk
            lines[i] += chunk.count(b"\n")
        more = any(at[i] < len(texts[i]) for i in range(n_in))
        out["pieces"] += 1
        if more and take([n // 4 for n in lines], mode) == 0:
            continue  # the piece takes nothing: everything is carried (piece() would say the same, slowly)
        p = piece(ptuple, carried, mode, more)
        res = p["res"]
        per_input = reads // 2 if mode == "pe_split" else reads
        if res["verdict"] is not None:
            why, i, k = res["verdict"]
            out["error"] = ("format", why, i, k + per_input)
            return _joined(out, parts)
        if res["range"] is not None:
            r, pos, ch = res["range"]
            out["error"] = ("range", r + reads, pos, ch)
            return _joined(out, parts)
        out["consumed_pieces"] += 1
        for o in fm.USED[mode]:
            parts[o].append(res["texts"][o])
            out["index"][o] += [int(x) + reads for x in res["index"][o]]
            out["records"][o] += len(res["index"][o])
            out["bytes"][o] += len(res["texts"][o])
        for i in range(n_in):
            out["records_in"][i] += p["records_in"][i]
            carried[i] = carried[i][p["consumed"][i]:]
            lines[i] = carried[i].count(b"\n")
        out["tail_lines"], out["dropped_unpaired"] = p["tail_lines"], p["dropped_unpaired"]
        reads += p["records_in"][0] * (2 if mode == "pe_split" else 1) - p["dropped_unpaired"]
        if not more:
            return _joined(out, parts)


def _joined(out, parts):
    for o in range(3):
        if out["texts"][o] is not None:
            out["texts"][o] = b"".join(parts[o])
    return out

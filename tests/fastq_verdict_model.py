"""What the finish of a FASTQ text call reports, restated from include/sickle_amd.h: the order of precedence each of the
four finishes states (sk_trim_fastq_device_finish, .._ordered_.., .._piece_.., .._ordered_piece_..) and the comments of the
count structs.  A case is a set of conditions a call can meet; words() lays them into the workspace words the kernels
write (sickle_amd/csrc/sk_fastq_words.h, sk_fastq_order.h), expect() says what finish must make of them.  Nothing here is
taken from the C code of the verdict.

Where the header leaves a choice, the model takes these readings:
  * records[] / bytes[] are "0 after an error" for the errors that stop the call before it emits: a format error, and for
    the ordered kinds a long line (and the full batch table of the ordered call).  A range error and a short output keep
    the needs.
  * format_* are filled with SK_EFORMAT and range with SK_ERANGE, not under a verdict that precedes them.
  * the order counts' long_line* are filled whenever the call found such a line.
  * counts are the workspace's own words also in cases a device cannot produce (a void piece with records)."""
SK_OK, SK_ERANGE, SK_ESPACE, SK_EFORMAT, SK_ELONGLINE = 0, 1, -5, -6, -8
SE, PE_SPLIT, PE_INTERLEAVED, PE_COMBO_ALL = 0, 1, 2, 3
PLAIN, ORDERED, PIECE, ORDERED_PIECE = 0, 1, 2, 3
NONE = (1 << 64) - 1
HDR_WORDS, BLOCK_WORDS = 32, 32

# the header's words
H_LINES, H_RECORDS, H_FMT, H_OUT_RECORDS, H_OUT_BYTES, H_FIT, H_PRODUCED, H_RANGE, H_MODE = 0, 2, 4, 7, 10, 13, 16, 19, 20
P_END, P_CONSUMED, P_OK, P_RANGE0, P_MORE = 23, 25, 27, 28, 29
# the order words: in the header for the ordered call, in the block for the ordered piece
O_BATCHES, O_UNITS, O_LAST_UNITS, O_UNBATCHED, O_MISMATCH, O_LONG, O_ERROR_BATCH, O_OVERFLOW = 21, 22, 23, 24, 26, 27, 28, 29
# the block's own words
X_STATE, X_TABLE_FULL, X_UNDETERMINED, X_INHERITED, X_BASE_BATCHES = 0, 8, 9, 10, 13

OWN_RANGE = {"read": 41, "pos": 149, "ch": -3}      # the call's own range error
OTHER_RANGE = {"read": 77, "pos": 5, "ch": 127}     # another call's, which a piece must not take for its own
EARLIER_RANGE = {"read": 1234, "pos": 0, "ch": 10}  # the one a piece finds set when it begins
LONG_LINE, ERROR_BATCH, BASE_BATCHES = 123456, 3, 100
OUT_RECORDS, OUT_BYTES = [5, 6, 7], [500, 600, 700]
ORDER_WORDS = {"batches": 9, "units": 31, "last_batch_units": 4, "records_unbatched": [2, 1], "stopped_on_mismatch": 1}
STATE = [1, 2, 109, 331, 4, 1 | (1 << 32), 0, 0]  # carried_lines[2], batches, units, last_batch_units, ended | mismatch << 32, ..


def is_piece(kind):
    return kind in (PIECE, ORDERED_PIECE)


def is_ordered(kind):
    return kind in (ORDERED, ORDERED_PIECE)


def range_word(e):
    """the range-error word of the scan kernels: read << 32 | pos << 8 | the byte"""
    return e["read"] << 32 | e["pos"] << 8 | (e["ch"] & 0xff)


def framing_mode(mode):
    """SK_TRIM_PE_COMBO_ALL frames as SK_TRIM_PE_INTERLEAVED: that is the header's mode word"""
    return PE_INTERLEAVED if mode == PE_COMBO_ALL else mode


def cases():
    """every subset of the conditions each kind can express; -> dicts"""
    out = []
    for kind in (PLAIN, ORDERED, PIECE, ORDERED_PIECE):
        for mode in (SE, PE_SPLIT, PE_INTERLEAVED, PE_COMBO_ALL):
            for inherited_range in ((0, 1) if is_piece(kind) else (0,)):
                for failed in ((0, 1) if kind == ORDERED_PIECE else (0,)):
                    for long_input in ((None, 0, 1) if is_ordered(kind) else (None,)):
                        for overflow in ((0, 1) if kind == ORDERED else (0,)):
                            for fmt in (None, "even", "odd"):
                                for rng in (0, 1):
                                    for short in (0, 1):
                                        for odd in (0, 1):
                                            for more in ((0, 1) if is_piece(kind) else (0,)):
                                                for tail in range(4):
                                                    out.append(dict(kind=kind, mode=mode, inherited_range=inherited_range,
                                                                    failed=failed, long_input=long_input, overflow=overflow,
                                                                    fmt=fmt, range=rng, short=short, odd=odd, more=more,
                                                                    tail=tail))
    return out


def format_of(c):
    """the malformed record of a case: (input, record, reason); its read number is even or odd as the case says"""
    split = c["mode"] == PE_SPLIT
    read = 18 if c["fmt"] == "even" else 19
    return (read & 1, read >> 1, 5) if split else (0, read, 2)


def own_error(c):
    """the call checked its records and one of them has a format or a range error"""
    void = c["inherited_range"] or c["failed"]
    return not void and (c["fmt"] is not None or c["range"])


def words(c):
    """-> [kind, the stream's live range-error word] + the header + the block"""
    kind, split = c["kind"], c["mode"] == PE_SPLIT
    h, x = [0xdead0000 + i for i in range(HDR_WORDS)], [0xbeef0000 + i for i in range(BLOCK_WORDS)]
    records = [6 + c["odd"], 11 if split else 0]
    # a piece with more to come carries whole records too
    carried = 4 if is_piece(kind) and c["more"] else 0
    lines = [4 * records[0] + c["tail"] + carried, 4 * records[1] + ((c["tail"] + 1) & 3 if split else 0)]
    h[H_LINES:H_LINES + 2], h[H_RECORDS:H_RECORDS + 2] = lines, records
    h[H_FMT] = NONE
    if c["fmt"] is not None:
        inp, record, reason = format_of(c)
        h[H_FMT] = ((2 * record + inp if split else record) << 3) | reason
    h[H_OUT_RECORDS:H_OUT_RECORDS + 3], h[H_OUT_BYTES:H_OUT_BYTES + 3] = OUT_RECORDS, OUT_BYTES
    h[H_PRODUCED:H_PRODUCED + 3], h[H_FIT:H_FIT + 3] = [1, 0, 1], [1, 0, 0 if c["short"] else 1]  # output 1 is not produced
    h[H_MODE] = framing_mode(c["mode"])
    if is_piece(kind):
        # the piece's verdict is the word its emission captured; the live word is a later call's business
        h[H_RANGE] = range_word(OWN_RANGE) if c["range"] else NONE
        live = range_word(OTHER_RANGE)
        h[P_END:P_END + 2], h[P_CONSUMED:P_CONSUMED + 2] = [1000, 2000], [900, 1990]
        h[P_OK] = 0 if c["inherited_range"] or c["failed"] or c["fmt"] or c["range"] or c["short"] or c["long_input"] is not None else 1
        h[P_RANGE0] = range_word(EARLIER_RANGE) if c["inherited_range"] else NONE
        h[P_MORE] = c["more"]
    else:
        # a whole-text call's verdict is the live word as finish finds it, whatever the emission saw
        live = range_word(OWN_RANGE) if c["range"] else NONE
        h[H_RANGE] = range_word(OTHER_RANGE)
    if is_ordered(kind):
        o = h if kind == ORDERED else x
        o[O_BATCHES], o[O_UNITS], o[O_LAST_UNITS] = ORDER_WORDS["batches"], ORDER_WORDS["units"], ORDER_WORDS["last_batch_units"]
        o[O_UNBATCHED:O_UNBATCHED + 2], o[O_MISMATCH] = ORDER_WORDS["records_unbatched"], ORDER_WORDS["stopped_on_mismatch"]
        o[O_LONG] = NONE if c["long_input"] is None else c["long_input"] << 63 | LONG_LINE
        o[O_ERROR_BATCH] = ERROR_BATCH if own_error(c) else NONE
        o[O_OVERFLOW] = c["overflow"] if kind == ORDERED else 0xfeed  # (a piece's table never gives SK_ESPACE)
    if kind == ORDERED_PIECE:
        x[X_STATE:X_STATE + 8] = STATE
        x[X_TABLE_FULL], x[X_UNDETERMINED], x[X_INHERITED], x[X_BASE_BATCHES] = 1, 0, c["failed"], BASE_BATCHES
    return [kind, live] + h + x


def verdict(c):
    """the finish's return code and what it tells in words, by the order of precedence of the case's kind"""
    kind = c["kind"]
    steps = []
    if is_piece(kind):
        steps.append(("inherited_range", SK_ERANGE))
    if kind == ORDERED_PIECE:
        steps.append(("failed", SK_OK))
    if is_ordered(kind):
        steps.append(("long", SK_ELONGLINE))
    if kind == ORDERED:
        steps.append(("overflow", SK_ESPACE))
    steps += [("fmt", SK_EFORMAT), ("range", SK_ERANGE), ("short", SK_ESPACE)]
    met = dict(c, long=c["long_input"] is not None, fmt=c["fmt"] is not None)
    for what, rc in steps:
        if met[what]:
            return what, rc
    return None, SK_OK


def expect(c):
    """-> (rc, counts, order counts, piece counts, order-piece counts, the numbers the message carries); a struct the kind
    does not have is None, as is the message of SK_OK"""
    kind, split = c["kind"], c["mode"] == PE_SPLIT
    w = words(c)
    h, x = w[2:2 + HDR_WORDS], w[2 + HDR_WORDS:]
    why, rc = verdict(c)
    refused = c["long_input"] is not None or bool(c["overflow"])
    stopped = c["fmt"] is not None or refused
    records_in, lines = h[H_RECORDS:H_RECORDS + 2], h[H_LINES:H_LINES + 2]
    pairs_of_one_text = c["mode"] in (PE_INTERLEAVED, PE_COMBO_ALL)
    counts = {
        "records_in": records_in,
        "tail_lines": [l - 4 * r for l, r in zip(lines, records_in)],
        # the ordered kinds count the odd record in records_unbatched; a piece with more to come carries it
        "dropped_unpaired": records_in[0] & 1 if pairs_of_one_text and not is_ordered(kind) and not c["more"] else 0,
        "records": [0, 0, 0] if stopped else OUT_RECORDS,
        "bytes": [0, 0, 0] if stopped else OUT_BYTES,
        "format_error": 0, "format_input": 0, "format_record": 0, "range": {"read": 0, "pos": 0, "ch": 0},
    }
    numbers = None if rc == SK_OK else []
    if why == "fmt":
        counts["format_input"], counts["format_record"], counts["format_error"] = format_of(c)
        numbers = list(format_of(c))
    if why == "inherited_range":
        counts["range"] = EARLIER_RANGE
        numbers = [EARLIER_RANGE["read"]]
    if why == "range":
        counts["range"] = OWN_RANGE
        numbers = [OWN_RANGE["read"], OWN_RANGE["pos"] + 1, OWN_RANGE["ch"]]
    order = piece = order_piece = None
    if is_ordered(kind):
        base = BASE_BATCHES if kind == ORDERED_PIECE else 0
        order = dict(ORDER_WORDS, long_line_input=0, long_line=0,
                     error_batch=base + ERROR_BATCH if own_error(c) and not refused else NONE)
        if c["long_input"] is not None:
            order["long_line_input"], order["long_line"] = c["long_input"], LONG_LINE
        if why == "long":
            numbers = [c["long_input"], LONG_LINE]
    if is_piece(kind):
        piece = {"consumed": [900, 1990], "carried_bytes": [100, 10], "ok": h[P_OK], "inherited_range": c["inherited_range"]}
    if kind == ORDERED_PIECE:
        order_piece = {"table_full": 1, "undetermined": 0, "inherited_failure": c["failed"], "state": STATE}
    return rc, counts, order, piece, order_piece, numbers

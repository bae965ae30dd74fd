"""The source view of a finished FASTQ text call (sickle_amd/csrc/sk_fastq_source.h), restated from DESIGN.md (4.7, 4.7.1,
4.15, 4.17 to 4.23) and the layout comment of sk_device.h, which tests/workspace_cases.py already restates: where the
sections of the call's workspace lie, whether the call adds, and where a read's descriptor sends it in its text.  Nothing
here is taken from the C code of the view.

The workspace: the header (32 words); for an ordered piece its block of 32 words; for the ordered kinds the table of first
units, 8 * (batch_capacity + 1) bytes rounded up to 16; then the sections chunks, desc, offsets, cuts, blocks, emit, qual
(, seq), whose offsets count from the header without the block and the table.
A descriptor slot is 5 words: the name line's start and the ends of the record's four lines, as offsets in the record's
text.  In split framing reads 2k and 2k + 1 are record k of text 0 and of text 1, and text 1's slots lie behind text 0's
bytes[0] / 4 + 1; in the other framings read r is record r of text 0."""
from workspace_cases import FQ_BLOCK_READS, FQ_CHUNK, fq_layout

SE, PE_SPLIT, PE_INTERLEAVED, PE_COMBO_ALL = 0, 1, 2, 3
PLAIN, PIECE, ORDERED, ORDERED_PIECE = 0, 1, 2, 3  # SK_FQ_REPORT_*
KINDS, MODES = (PLAIN, PIECE, ORDERED, ORDERED_PIECE), (SE, PE_SPLIT, PE_INTERLEAVED, PE_COMBO_ALL)
NONE = (1 << 64) - 1
NO_MODE = None  # the report: a view that compares no mode
HDR_WORDS, BLOCK_WORDS = 32, 32

H_FMT, H_NREAL, H_RANGE, H_MODE, P_RANGE0 = 4, 5, 19, 20, 28
O_LONG, O_OVERFLOW, X_INHERITED = 27, 29, 10

TAG_LAYOUT, TAG_VALIDITY, TAG_LOOKUPS = 1, 2, 3


def is_piece(kind):
    return kind in (PIECE, ORDERED_PIECE)


def is_ordered(kind):
    return kind in (ORDERED, ORDERED_PIECE)


def framing_mode(mode):
    """SK_TRIM_PE_COMBO_ALL frames as SK_TRIM_PE_INTERLEAVED: that is the header's mode word"""
    return PE_INTERLEAVED if mode == PE_COMBO_ALL else mode


def u64(x):
    return NONE if x is None else x & NONE


# ---- layout ------------------------------------------------------------------------------------------------------------
def shift(kind, batch_capacity):
    table = (8 * (batch_capacity + 1) + 15) // 16 * 16
    return {PLAIN: 0, PIECE: 0, ORDERED: table, ORDERED_PIECE: 256 + table}[kind]


def sections(T, trunc_n):
    """byte offsets of desc, offsets, cuts and qual from the header, and the four bounds"""
    lay = fq_layout(T, trunc_n)
    S, N = lay["S"], lay["N"]
    Q = 16 * ((T + 31) // 32)
    desc = 8 * HDR_WORDS + 16 * (T // FQ_CHUNK + 3)
    offsets = desc + 40 * S
    cuts = offsets + 8 * (N + 2)
    blocks = cuts + 8 * N
    qual = blocks + 64 * ((N + FQ_BLOCK_READS - 1) // FQ_BLOCK_READS) + 16 * N
    assert qual + Q * (2 if trunc_n else 1) == lay["total"]
    assert S == 2 * ((T + 7) // 8) + 2 and N == 2 * ((T + 2) // 16) + 2
    return {"desc": desc, "offsets": offsets, "cuts": cuts, "qual": qual, "slot_bound": S, "n_bound": N, "q_bound": Q}


def layout_cases():
    """-> dicts; texts: None = in is NULL, else ((text[0] given, bytes[0]), (text[1] given, bytes[1]))"""
    out = []
    for T in (0, 1, 7, 8, 13, 14, 15, 16, 29, 30, 31, 32, 65535, 65536, 65537):
        # a NULL text[0] with bytes[0] = 0; two texts of unequal bytes (text[1] is given in every mode: only split takes it)
        for texts in (None, ((0, 0), (1, T)), ((1, T - T // 3), (1, T // 3)), ((1, T), (0, 0))):
            for trunc_n in (0, 1):
                for kind in KINDS:
                    for cap in (0, 1, 2, 17):
                        for mode in MODES + (NO_MODE,):
                            out.append(dict(T=T, trunc_n=trunc_n, kind=kind, cap=cap, mode=mode, texts=texts))
    return out


def layout_words(c):
    t = c["texts"] or ((0, 0), (0, 0))
    return [TAG_LAYOUT, c["T"], c["trunc_n"], c["kind"], c["cap"], u64(c["mode"]), int(c["texts"] is not None), t[0][0], t[1][0],
            t[0][1], t[1][1]]


def layout_expect(c):
    s, sh = sections(c["T"], c["trunc_n"]), shift(c["kind"], c["cap"])
    mode = NO_MODE if c["mode"] is NO_MODE else framing_mode(c["mode"])
    order_words = {PLAIN: None, PIECE: None, ORDERED: 0, ORDERED_PIECE: 8 * HDR_WORDS}[c["kind"]]
    texts = c["texts"] or ((0, 0), (0, 0))
    taken = 0 if c["texts"] is None else 2 if mode == PE_SPLIT else 1
    text, nbytes = [], []
    for i in range(2):
        given, b = texts[i]
        text.append(0 if i < taken and given else None)
        nbytes.append(b if i < taken and given else 0)
    slots0 = texts[0][1] // 4 + 1  # in->bytes[0] as it stands: where the text call put input 1's slots
    return [0, u64(order_words), sh + s["desc"], sh + s["offsets"], sh + s["cuts"], sh + s["qual"], u64(text[0]), u64(text[1]),
            nbytes[0], nbytes[1], slots0, s["slot_bound"], s["n_bound"], s["q_bound"], c["kind"], u64(-1 if mode is NO_MODE else mode)]


# ---- validity ------------------------------------------------------------------------------------------------------------
CONDITIONS = ("fmt", "range", "range0", "long", "overflow", "inherited", "mode_differs")


def conditions_of(kind):
    """the conditions a kind can meet"""
    c = ["fmt", "range", "mode_differs"]
    if is_piece(kind):
        c.append("range0")
    if is_ordered(kind):
        c += ["long", "overflow"]
    if kind == ORDERED_PIECE:
        c.append("inherited")
    return c


def validity_cases():
    """every subset of the conditions a kind can meet, under every mode and under the view without a mode; and, for every
    kind, the range0 and inherited words set where the kind does not have them (foreign=1): they must not matter"""
    out = []
    for kind in KINDS:
        own = conditions_of(kind)
        for bits in range(1 << len(own)):
            met = {own[i] for i in range(len(own)) if bits >> i & 1}
            for mode in MODES + (NO_MODE,):
                for foreign in (0, 1):
                    out.append(dict(kind=kind, mode=mode, met=met, foreign=foreign))
    return out


def validity_words(c):
    """-> the tag, the kind, the view's mode, the header, the block"""
    kind, met = c["kind"], c["met"]
    h, x = [0xdead0000 + i for i in range(HDR_WORDS)], [0xbeef0000 + i for i in range(BLOCK_WORDS)]
    h[H_FMT] = (19 << 3 | 5) if "fmt" in met else NONE
    h[H_RANGE] = (41 << 32 | 149 << 8 | 0xfd) if "range" in met else NONE
    recorded = framing_mode(SE if c["mode"] is NO_MODE else c["mode"])
    if "mode_differs" in met:
        recorded = {SE: PE_INTERLEAVED, PE_SPLIT: SE, PE_INTERLEAVED: PE_SPLIT}[recorded]
    h[H_MODE] = recorded
    o = h if kind == ORDERED else x
    if is_piece(kind):
        h[P_RANGE0] = (1234 << 32 | 10) if "range0" in met else NONE
    else:  # word 28 is a plain call's to leave as it was and an ordered call's error batch
        h[P_RANGE0] = 77 if c["foreign"] else NONE
    if is_ordered(kind):
        o[O_LONG] = (1 << 63 | 123456) if "long" in met else NONE
        o[O_OVERFLOW] = 1 if "overflow" in met else 0
    if kind == ORDERED_PIECE:
        x[X_INHERITED] = 1 if "inherited" in met else 0
    else:  # only the ordered piece has a block; the ordered call's order words are the header, whose word 10 is an output's bytes
        h[X_INHERITED] = x[X_INHERITED] = 1 if c["foreign"] else 0
    return [TAG_VALIDITY, kind, u64(c["mode"])] + h + x


def validity_expect(c):
    """a call adds iff it has no format verdict, no range verdict, inherited none, was not refused (a long line, a full
    table, a void ordered piece), and framed as the view says, where the view says"""
    met = set(c["met"])
    if c["mode"] is NO_MODE:
        met.discard("mode_differs")
    return int(not met)


# ---- lookups ------------------------------------------------------------------------------------------------------------
def slot_of(mode, slots0, r):
    """-> (input, slot)"""
    if mode == PE_SPLIT:
        return r & 1, (slots0 if r & 1 else 0) + (r >> 1)
    return 0, r


def span(start, end, b):
    """the span of a text of b bytes that a start and an end name, held to the text: (at, len)"""
    at = min(start, b)
    return at, max(min(end, b), at) - at


def lookup_expect(t, r):
    """t: dict(mode, bytes, slots0, slot_bound, desc: slot_bound lists of 5) -> the program's 8 words for read r"""
    i, slot = slot_of(t["mode"], t["slots0"], r)
    b = t["bytes"][i]
    if slot >= t["slot_bound"]:  # no slot: the audit has no name line, the seq line starts at the text's end, the record is empty there
        return [i, 0, NONE, NONE, b, i, b, 0]
    d = t["desc"][slot]
    name_at, name_len = span(d[0], d[1], b)
    rec_at, rec_len = span(d[0], d[4], b)
    return [i, 1, name_at, name_len, min(min(d[1], b) + 1, b), i, rec_at, rec_len]


def lookup_tables():
    """6 slots over texts of 40 and 24 bytes: honest records, entries that start or end beyond the text, entries that end
    before they start; in split framing with input 1's slots behind 3 and behind bytes[0] / 4 + 1 = 11 (beyond the table)"""
    honest0 = [[0, 3, 8, 10, 15], [16, 20, 26, 28, 34]]  # two records of text 0 (40 bytes)
    honest1 = [[0, 2, 9, 11, 18]]                        # one of text 1 (24 bytes)
    beyond = [[30, 45, 50, 52, 60], [41, 44, 50, 52, 60], [NONE, NONE, NONE, NONE, NONE], [24, 25, 30, 31, 40]]
    backwards = [[20, 10, 5, 4, 3], [39, 0, 0, 0, 0], [12, 11, 30, 31, 8]]
    out = []
    for mode in (SE, PE_INTERLEAVED, PE_SPLIT):
        for slots0 in (3, 11):
            for rows in (honest0 + [beyond[0]] + honest1 + backwards[:2], beyond + backwards[1:], backwards + beyond[:3],
                         honest0 + honest1 + beyond[3:] + backwards[2:] + beyond[2:3]):
                assert len(rows) == 6
                out.append(dict(mode=mode, bytes=[40, 24], slots0=slots0, slot_bound=6, desc=rows))
    out.append(dict(mode=PE_SPLIT, bytes=[0, 0], slots0=1, slot_bound=0, desc=[]))  # no slot at all, no text byte
    return out


LOOKUP_READS = list(range(0, 16)) + [21, 22, 23, 1 << 32, (1 << 32) + 1, NONE - 1, NONE]  # below, at and beyond every bound


def lookup_words(t):
    return [TAG_LOOKUPS, t["mode"], t["bytes"][0], t["bytes"][1], t["slots0"], t["slot_bound"]] + [w for d in t["desc"] for w in d] + \
        [len(LOOKUP_READS)] + LOOKUP_READS

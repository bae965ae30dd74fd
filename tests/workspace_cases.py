"""The case tables of tests/test_gpu_workspace.py, which runs them on guarded, poisoned workspaces, and of
tests/test_workspace_cases.py, which holds every case to its label with the models and the sizing formulas alone.  Nothing
here touches the device."""
import zlib

import numpy as np

import bgunzip_model as bm

REC = b"@a\nA\n+\nI\n"      # the densest valid record: 9 bytes
BAD7 = b"@a\n\n+\n\n"        # 7 bytes, malformed (SK_FQ_SEQ_EMPTY): denser than the 8 bytes a valid record needs
FQ_BLOCK_READS = 2048
FQ_CHUNK = 65536
BGZF_BLOCK = 65280


def fq_params(trunc_n):
    """-q 20 -l 1: every record of the texts below (quality 'I') is kept whole"""
    return ("sanger", 20, 1, False, bool(trunc_n))


# ---- sk_device.h's layout comment, restated ------------------------------------------------------------------------------
def fq_slots(nbytes):
    return nbytes // 4 + 1


def fq_pack_reads(nbytes):
    """the most valid records a text holds: what the packed batch is sized by"""
    return (nbytes + 1) // 8


def fq_layout(T, trunc_n):
    """sk_fq_layout_of: H = (T + 2) / 16; header 256; chunks 16 * (T / 65536 + 3); desc 40 * (2 * ((T + 7) / 8) + 2); offsets 8 * (N + 2),
    N = 2H + 2; cuts 8N; blocks 64 * ceil(N / 2048); emit 16N; qual (and seq with trunc_n) 16 * ceil(T / 32)"""
    H = (T + 2) // 16
    S, N = 2 * ((T + 7) // 8) + 2, 2 * H + 2
    Q = 16 * ((T + 31) // 32)
    total = 256 + 16 * (T // FQ_CHUNK + 3) + 40 * S + 8 * (N + 2) + 8 * N + 64 * ((N + FQ_BLOCK_READS - 1) // FQ_BLOCK_READS) \
        + 16 * N + Q * (2 if trunc_n else 1)
    return {"S": S, "N": N, "total": total}


def many_good(n, L=150, seed=0):
    """tests/test_gpu_fastq.py's many_good, joined; restated so that this module imports no GPU test file"""
    rng = np.random.default_rng(seed)
    q = rng.integers(35, 75, size=(n, L), dtype=np.uint8).tobytes()
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (k, b"ACGT" * (L // 4) + b"AC"[:L % 4], q[k * L:(k + 1) * L]) for k in range(n))


def one_record(L):
    return b"@a\n" + b"A" * L + b"\n+\n" + b"I" * L + b"\n"


def fastq_texts():
    """name -> (text, the model's verdict (reason, input, record) or None, "over" / "within": whether the text has more
    records than the packed batch has reads, (b + 1) / 8, which only a malformed text can)"""
    t = {}
    for k in (1, 2, 2047, 2048, 2049, 4099):
        t["dense_%d" % k] = (REC * k, None, "within")
    t["dense_2049_unterminated"] = ((REC * 2049)[:-1], None, "within")
    for L in (1, 15, 16, 17, 30000, 70000):
        t["one_%d" % L] = (one_record(L), None, "within")
    for T in (1, 4096, 65541):
        t["newlines_%d" % T] = (b"\n" * T, (1, 0, 0) if T >= 4 else None, "over" if T > 8 else "within")
    t["bad7_600"] = (BAD7 * 600, (3, 0, 0), "over")
    t["dense_600_bad7_600"] = (REC * 600 + BAD7 * 600, (3, 0, 600), "within")
    t["empty"] = (b"", None, "within")
    t["one_byte"] = (b"@", None, "within")
    t["control_600"] = (many_good(600), None, "within")
    return t


FASTQ_MODES = ("se", "pe_interleaved", "pe_split")  # pe_split: the same text for both inputs
ORDERED = ((1, 20), (3, 64))                        # (threads, batch_len); 20 is the least batch_len the call takes


def texts_of_mode(text, mode):
    return [text, text] if mode == "pe_split" else [text]


# ---- sk_trim_device_async ---------------------------------------------------------------------------------------------
TRIM_N = (0, 1, 2, 2047, 2048, 2049, 4097, 4098)  # 4098: the pair modes' case of several blocks (4097 is odd)
TRIM_KEPT = ("all", "none", "one_mate")
TRIM_LAYOUTS = ("ragged", "fixed")


def trim_case(n, kept, layout, mode):
    """-> (qual, seq, offsets (n + 1, uint64), starts (int64), cuts int32 [n, 2]); layout "fixed": every read 37 bytes"""
    rng = np.random.default_rng(1000 * n + len(kept))
    if layout == "fixed":
        lens = np.full(n, 37, np.int64)
    else:
        lens = rng.integers(1, 60, n).astype(np.int64)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    qual = rng.integers(33, 75, max(total, 1)).astype(np.uint8)
    seq = rng.choice(np.frombuffer(b"ACGTN", np.uint8), max(total, 1))
    five = rng.integers(0, lens) if n else np.zeros(0, np.int64)
    cuts = np.stack([five, lens], axis=1).astype(np.int32).reshape(n, 2)
    if kept == "none":
        cuts[:] = -1
    elif kept == "one_mate" and mode != "se":
        cuts[(np.arange(n) + np.arange(n) // 2) % 2 == 1] = -1  # mate 0 of even pairs, mate 1 of odd pairs
    return qual, seq, off, off[:-1].astype(np.int64), cuts


def trim_workspace_bytes(n):
    """include/sickle_amd.h: 128 + 64 * ceil(n / 2048) + 8 * n (16 header words, 8 per block of 2048 reads, one source
    delta per record of the three outputs, which hold n records at most together)"""
    return 128 + 64 * ((n + 2047) // 2048) + 8 * n


# ---- sk_bgzf_device_async ---------------------------------------------------------------------------------------------
BGZF_LENGTHS = (0, 1, 65279, 65280, 65281, 2 * 65280, 3 * 65280 + 1)
BGZF_KINDS = ("fastq", "random", "repeat")


def bgzf_text(kind, n):
    if kind == "random":
        return np.random.default_rng(n + 5).integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind == "repeat":
        return b"G" * n
    return (many_good(n // 300 + 2, seed=7))[:n]


def bgzf_blocks(n):
    return (n + BGZF_BLOCK - 1) // BGZF_BLOCK


# ---- sk_bgzf_inflate_device_async ------------------------------------------------------------------------------------
EMPTY_MEMBERS = (1, 64, 65, 257, 4097)


# ---- sk_gzip_inflate_device_async --------------------------------------------------------------------------------------
def gzip_images():
    """name -> (image, text, least text-to-image ratio the label promises, most)"""
    zeros = bytes(1 << 20)
    rnd = np.random.default_rng(42).integers(0, 256, 200_000, dtype=np.uint8).tobytes()
    fq = many_good(300, seed=9)
    three = [fq[:20000], b"", fq[20000:]]
    g = {}
    g["zeros_1m_level9"] = (_gz(zeros, 9), zeros, 900.0, 1100.0)
    g["stored_200k"] = (_gz(rnd, 0), rnd, 0.99, 1.0)
    g["three_members"] = (b"".join(_gz(p, 6) for p in three), b"".join(three), 1.5, 10.0)
    return g


def _gz(text, level):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    return c.compress(text) + c.flush()


def empty_members(k):
    return bm.EOF * k

"""numpy restatement of sk_trim_device_async (include/sickle_amd.h): what each output of a trim holds, from the batch and
its cuts.  The tests compare the device against it; it never reads anything the device made."""
import os

import numpy as np

import cli_util as cu
import oracle_bind as ob
from fastq_util import parse_fastq

MODES = ("se", "pe_split", "pe_interleaved")


def dests(cuts, mode):
    """Output of every read (-1: dropped): the pair rule of sk_pair_count_kernel, mates at 2k and 2k+1."""
    kept = np.asarray(cuts)[:, 1] >= 0
    if mode == "se":
        return np.where(kept, 0, -1).astype(np.int8)
    assert len(kept) % 2 == 0
    d = np.full(len(kept), -1, dtype=np.int8)
    k1, k2 = kept[0::2], kept[1::2]
    both = k1 & k2
    d1, d2 = d[0::2], d[1::2]  # views
    d1[both] = 0
    d2[both] = 1 if mode == "pe_split" else 0
    d1[k1 & ~k2] = 2
    d2[k2 & ~k1] = 2
    return d


def expected(qual, seq, starts, cuts, mode, first_read=0):
    """-> [out0, out1, out2], each None (the mode has no such output) or dict(qual, seq, offsets, read_index) for the
    reads whose input bytes start at starts[i] (any layout), cuts int32 [n, 2].  first_read numbers the reads."""
    cuts = np.asarray(cuts, dtype=np.int64)
    starts = np.asarray(starts, dtype=np.int64)
    d = dests(cuts, mode)
    used = {"se": (0,), "pe_split": (0, 1, 2), "pe_interleaved": (0, 2)}[mode]
    res = [None, None, None]
    for o in used:
        idx = np.nonzero(d == o)[0]
        five, three = cuts[idx, 0], cuts[idx, 1]
        lens = three - five
        offsets = np.zeros(len(idx) + 1, dtype=np.int64)
        np.cumsum(lens, out=offsets[1:])
        total = int(offsets[-1])
        src = np.repeat(starts[idx] + five - offsets[:-1], lens) + np.arange(total, dtype=np.int64)
        res[o] = dict(qual=qual[src], seq=None if seq is None else seq[src], offsets=offsets,
                      read_index=idx.astype(np.int64) + first_read)
    return res


def counts_of(res):
    return {"records": [0 if r is None else len(r["read_index"]) for r in res],
            "bytes": [0 if r is None else int(r["offsets"][-1]) for r in res]}


# ---- the reference runs of tests/golden/e2e.json replayed through a trim ------------------------------------------
UNREPLAYABLE = {
    "pe_problem1_inter": "the reference's reader ends this run at its first batch (a byte budget of filesize / 8 holds no "
                         "complete pair), so no record reaches the trim; the library trims the records it is handed",
}


def golden_params():
    """golden_runs() as pytest params, the runs a trim cannot replay skipped by name with the reason."""
    import pytest
    return [pytest.param(name, rec, id=name,
                         marks=[pytest.mark.skip(reason=UNREPLAYABLE[name])] if name in UNREPLAYABLE else [])
            for name, rec in golden_runs()]


def golden_runs():
    """(name, record) of every -a 1 run in e2e.json's runs and long_reads."""
    g = cu.e2e()
    out = []
    for sec in ("runs", "long_reads"):
        for name, rec in g[sec].items():
            argv = rec["argv"]
            if "-a" in argv and argv[argv.index("-a") + 1] == "1":
                out.append((name, rec))
    return out


def run_params(argv):
    """oracle / capi Params fields of a `sickle pe` argv: (qualtype, q, l, no5, trunc_n)."""
    qt, q, l = "sanger", 20, 20
    if "-t" in argv:
        qt = argv[argv.index("-t") + 1]
    if "-q" in argv:
        q = int(argv[argv.index("-q") + 1])
    if "-l" in argv:
        l = int(argv[argv.index("-l") + 1])
    return qt, q, l, "-x" in argv, "-n" in argv


def _plain(path, tmp):
    """The file an argv names; a .gz input -> its plain twin (in tmp, else among the bundled inputs)."""
    path = path.replace("{inputs}", cu.INPUTS).replace("{tmp}", str(tmp))
    if path.endswith(".gz"):
        path = path[:-3]
        if not os.path.exists(path):
            path = os.path.join(cu.INPUTS, os.path.basename(path))
    return path


def run_batch(argv, tmp):
    """-> (mode, records) of a run: the records of the batch in read order (mates at 2k, 2k+1), and the output files
    as {file name: output index}.  An interleaved file with an odd record count loses its last record."""
    if "-c" in argv:
        recs = parse_fastq(open(_plain(argv[argv.index("-c") + 1], tmp), "rb").read())
        recs = recs[:len(recs) // 2 * 2]
        files = {"om.fastq": 0, "os.fastq": 2}
        return "pe_interleaved", recs, files
    r1 = parse_fastq(open(_plain(argv[argv.index("-f") + 1], tmp), "rb").read())
    r2 = parse_fastq(open(_plain(argv[argv.index("-r") + 1], tmp), "rb").read())
    assert len(r1) == len(r2)
    recs = [r for pair in zip(r1, r2) for r in pair]
    return "pe_split", recs, {"o1.fastq": 0, "o2.fastq": 1, "os.fastq": 2}


def pack(recs):
    """records -> (qual, seq, offsets) uint8 / uint8 / uint64, back to back."""
    lens = np.array([len(r[3]) for r in recs], dtype=np.uint64)
    offsets = np.zeros(len(recs) + 1, dtype=np.uint64)
    np.cumsum(lens, out=offsets[1:])
    qual = np.frombuffer(b"".join(r[3] for r in recs), dtype=np.uint8)
    seq = np.frombuffer(b"".join(r[1] for r in recs), dtype=np.uint8)
    return qual, seq, offsets


def fastq_text(recs, out):
    """One output file of the reference (src/trim_single.cpp:393-396 record format) rebuilt from an output of a trim:
    name and '+' lines of the input record read_index[j], seq and qual of record j."""
    if out is None:
        return b""
    q, s, off, idx = (np.asarray(out[k]) for k in ("qual", "seq", "offsets", "read_index"))
    qb, sb = q.tobytes(), s.tobytes()
    parts = []
    for j, r in enumerate(idx.tolist()):
        a, b = int(off[j]), int(off[j + 1])
        parts.append(recs[r][0] + b"\n" + sb[a:b] + b"\n" + recs[r][2] + b"\n" + qb[a:b] + b"\n")
    return b"".join(parts)


def oracle_cuts(params_tuple, qual, seq, offsets):
    cuts, err = ob.oracle_trim_batch(ob.make_params(*params_tuple), qual, seq, offsets=offsets)
    assert err is None
    return cuts

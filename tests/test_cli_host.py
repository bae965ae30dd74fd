"""CPU suite for the host pipeline (ingest, framing, batch-cut emulation, pairing, output
assembly, counters, messages): the CLI built against the oracle-backed shim
(tests/cpu_shim, test infrastructure) replays every reference run recorded in
tests/golden/e2e.json and must produce byte-identical files and the same summary."""
import os
import subprocess

import numpy as np
import pytest

import cli_util as cu
import oracle_bind as ob
from fastq_util import emit_records, pack_records, parse_fastq
from sickle_amd import synth


@pytest.fixture(scope="module")
def hostcheck():
    return cu.build_hostcheck()


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli")
    cu.prepare_inputs(d)
    return d


@pytest.mark.parametrize("name", sorted(cu.e2e()["runs"].keys()))
def test_reference_runs_byte_identical(hostcheck, workdir, name):
    cu.check_run(hostcheck, workdir, name, cu.e2e()["runs"][name])


@pytest.mark.parametrize("piece", [2, 7, 500])
@pytest.mark.parametrize("name", sorted(cu.e2e()["runs"].keys()))
def test_reference_runs_in_pieces(hostcheck, workdir, name, piece):
    """At -a 1 an ingest batch goes through the device and the writers in pieces (host/trim.h: piece_reads);
    forced tiny here: same bytes, same summary (incl. the PE "Total" of the last INGEST batch)."""
    cu.check_run(hostcheck, workdir, name, cu.e2e()["runs"][name], env={"SICKLE_SUBBATCH_READS": str(piece)})


@pytest.mark.parametrize("name", sorted(cu.e2e()["long_reads"].keys()))
def test_long_reads_byte_identical(hostcheck, workdir, name):
    """Reads of 1 .. 40 kb with short ones between them (a ragged batch behind the CLI): the reference's files."""
    cu.prepare_long_inputs(workdir)
    cu.check_run(hostcheck, workdir, name, cu.e2e()["long_reads"][name])


@pytest.mark.parametrize("name", ["pe_fr_illumina", "pe_syn_mixed_inter_illumina_n", "pe_problem1_inter"])
def test_reference_runs_in_one_process(hostcheck, workdir, name):
    """SICKLE_NO_FRONT=1: no front process (host/sickle.h), the run and its teardown in the one process the caller
    started -- the same bytes, summary and exit status as with it (every other test runs with the front process)."""
    cu.check_run(hostcheck, workdir, name, cu.e2e()["runs"][name], env={"SICKLE_NO_FRONT": "1"})


def test_front_process_passes_the_exit_status_and_the_message(hostcheck, workdir):
    """A fatal input error in the worker (exit(1) paths of FQEntry::validate): the front process leaves with status
    1 and the reference's message is on stderr, complete, with and without it."""
    bad = os.path.join(str(workdir), "front_bad.fastq")
    open(bad, "wb").write(b"@r1\nACGT\n+\nIIII\n@r2\nACGTA\n+\nIIII\n")
    outs = []
    for env in (None, {"SICKLE_NO_FRONT": "1"}):
        pr = cu.run_cli(hostcheck, workdir, ["se", "-f", bad, "-t", "sanger", "-o", os.path.join(str(workdir), "front_bad.out")], env=env)
        assert pr.returncode == 1
        assert b"[ERROR]" in pr.stderr
        outs.append(pr.stderr)
    assert outs[0] == outs[1]


def test_front_process_with_closed_standard_descriptors(hostcheck, workdir):
    """A caller that starts sickle with stdin and stdout (or stdin and stderr) CLOSED: the status pipe of the
    front process must not land on descriptor 1 or 2, where the worker's summary / error text would be taken
    for the exit status (`<&- >&-` on a good input exited 10, `<&- 2>&-` on a bad one 91)."""
    import subprocess
    good = os.path.join(str(workdir), "fd_good.fastq")
    bad = os.path.join(str(workdir), "fd_bad.fastq")
    open(good, "wb").write(b"@r1\nACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIII\n" * 50)
    open(bad, "wb").write(b"@r1\nACGT\n+\nIIII\n@r2\nACGTA\n+\nIIII\n")
    out = os.path.join(str(workdir), "fd_out.fastq")
    for env in ({}, {"SICKLE_NO_FRONT": "1"}):
        e = dict(os.environ, **env)
        for redirect in ("<&- >&-", "<&- 2>&-", "<&- >&- 2>&-"):
            pr = subprocess.run("%s se -f %s -t sanger -o %s %s" % (hostcheck, good, out, redirect), shell=True, env=e, timeout=120)
            assert pr.returncode == 0, (env, redirect, pr.returncode)
            assert open(out, "rb").read() == open(good, "rb").read()
            pr = subprocess.run("%s se -f %s -t sanger -o %s %s" % (hostcheck, bad, out, redirect), shell=True, env=e, timeout=120)
            assert pr.returncode == 1, (env, redirect, pr.returncode)


def test_cli_soak_against_reference(hostcheck):
    """tests/soak_cli.py, 80 random paired inputs (two files / interleaved; equal, mixed, long and tiny reads;
    every encoding; -q -l -x -n): this CLI writes the per-batch chunks derived from the oracle in batch order, the
    compiled reference a permutation of exactly those chunks, the summaries agree (the reference's side as
    recorded in tests/golden/ref_soak_cli.json, and run now where oracle/_ref exists)."""
    import soak_cli
    soak_cli.NEW = hostcheck
    assert soak_cli.run(80, 404, verbose=False, golden=cu.ref_soak_record(404)) == 80


def se_expected(path, qt, q=20, l=20, no5=False, trunc_n=False, threads=1, batch_lines=None):
    """SE expectation = the oracle's cuts + the record format (`sickle se` itself crashes in the
    reference).  With threads > 1 the per-batch queue-major order is applied by the test."""
    recs = parse_fastq(open(path, "rb").read())
    seq, qual, offsets = pack_records(recs)
    cuts, err = ob.oracle_trim_batch(ob.make_params(qt, q, l, no5, trunc_n), qual, seq, offsets=offsets)
    assert err is None
    return recs, cuts


def test_se_matches_oracle_plus_format(hostcheck, workdir):
    src = os.path.join(cu.INPUTS, "test.fastq")
    for qt, extra in (("illumina", []), ("illumina", ["-n"]), ("solexa", ["-q", "25", "-x"]), ("sanger", ["-l", "100"])):
        out = os.path.join(str(workdir), "se_out.fastq")
        pr = cu.run_cli(hostcheck, workdir, ["se", "-f", src, "-t", qt, "-o", out, "-a", "1"] + extra)
        assert pr.returncode == 0, pr.stderr
        kw = {"trunc_n": "-n" in extra, "no5": "-x" in extra}
        if "-q" in extra:
            kw["q"] = int(extra[extra.index("-q") + 1])
        if "-l" in extra:
            kw["l"] = int(extra[extra.index("-l") + 1])
        recs, cuts = se_expected(src, qt, **kw)
        assert open(out, "rb").read() == emit_records(recs, cuts)
        kept = int((cuts[:, 1] >= 0).sum())
        text = pr.stdout.decode()
        assert "\nSE input file: %s\n\nTotal FastQ records: %d\nFastQ records kept: %d\nFastQ records discarded: %d\n\n" % (
            src, len(recs), kept, len(recs) - kept) in text


def test_se_equals_selfpaired_pe_golden(hostcheck, workdir):
    """pe -f X -r X' writes in file 1 exactly what se would."""
    rec = cu.e2e()["runs"]["se_equiv_selfpair_illumina"]
    out = os.path.join(str(workdir), "se_self.fastq")
    pr = cu.run_cli(hostcheck, workdir, ["se", "-f", "{inputs}/test.fastq", "-t", "illumina", "-o", out, "-a", "1"])
    assert pr.returncode == 0
    assert cu.md5_file(out) == rec["outputs"]["o1.fastq"]["md5"]


def test_se_thread_count_sets_record_order(hostcheck, workdir):
    """-a T: read k of a batch goes to queue (k+1) mod T, queues are written in turn
    (reference src/trim_single.cpp:263-298,382-405); the kept multiset never changes."""
    src = os.path.join(cu.INPUTS, "test.fastq")
    out1 = os.path.join(str(workdir), "se_a1.fastq")
    out4 = os.path.join(str(workdir), "se_a4.fastq")
    assert cu.run_cli(hostcheck, workdir, ["se", "-f", src, "-t", "illumina", "-o", out1, "-a", "1"]).returncode == 0
    assert cu.run_cli(hostcheck, workdir, ["se", "-f", src, "-t", "illumina", "-o", out4, "-a", "4"]).returncode == 0
    r1 = parse_fastq(open(out1, "rb").read())
    r4 = parse_fastq(open(out4, "rb").read())
    assert r1 != r4 and sorted(r1) == sorted(r4)
    # the first batch's first written record is input record 3 ((k+1) % 4 == 0) unless it was discarded
    recs, cuts = se_expected(src, "illumina")
    first = next(k for k in range(3, len(recs), 4) if cuts[k][1] >= 0)
    assert r4[0][0] == recs[first][0]


@pytest.mark.parametrize("name", sorted(cu.e2e()["thread_order"].keys()))
def test_pe_thread_order_goldens(hostcheck, workdir, name):
    """`sickle pe -a T`, T > 1, byte for byte.  The goldens are the per-batch chunks of the reference in batch
    order: make_golden.py derives them (restated batch-cut rule + queue order) and checks that every run of the
    compiled reference is a permutation of exactly those chunks (its batches race for the files; the order inside
    a batch does not).  No multiset fallback."""
    cu.check_run(hostcheck, workdir, name, dict(cu.e2e()["thread_order"][name], stdout=""), summary=False)


def derived_expectation(paths, qt, threads, interleaved=False, single=False):
    from fastq_util import (expected_pe_outputs, expected_se_output, file_lines, reference_batch_len, reference_batches)
    datas = [open(p, "rb").read() for p in paths]
    blen = reference_batch_len(len(datas[0]), 512, paired=not single)
    cuts = []
    for d in datas:
        recs = parse_fastq(d)
        seq, qual, offsets = pack_records(recs)
        c, err = ob.oracle_trim_batch(ob.make_params(qt), qual, seq, offsets=offsets)
        assert err is None
        cuts.append(c)
    b1 = reference_batches(file_lines(datas[0]), blen, 8 if interleaved else 4)
    if single:
        return b"".join(expected_se_output(b1, lambda f, r: cuts[f][r], threads))
    b2 = None if interleaved else reference_batches(file_lines(datas[1]), blen, 4)
    chunks = expected_pe_outputs(b1, b2, lambda f, r: cuts[f][r], threads, interleaved=interleaved)
    return [b"".join(c[i] for c in chunks) for i in range(3)]


@pytest.mark.parametrize("threads,host_threads", [(2, None), (3, "3"), (4, "5"), (7, "2"), (64, "3"), (5000, None)])
def test_thread_order_derived_for_any_T(hostcheck, workdir, threads, host_threads):
    """Queue-major order for thread counts that do not divide the batch, that exceed the reads of a batch
    (T = 5000 > 312 pairs per batch) and with the host pool cut so that its part boundaries fall inside queues
    (SICKLE_HOST_THREADS): SE (read k -> queue (k+1) mod T) and two-file PE (pair k -> queue k mod T) against
    the expectation derived from the oracle's cuts and the restated batch-cut rule."""
    env = {"SICKLE_HOST_THREADS": host_threads} if host_threads else None
    d = str(workdir)
    src = os.path.join(cu.INPUTS, "test.fastq")
    out = os.path.join(d, "se_T.fastq")
    pr = cu.run_cli(hostcheck, workdir, ["se", "-f", src, "-t", "illumina", "-o", out, "-a", str(threads)], env=env)
    assert pr.returncode == 0, pr.stderr
    assert open(out, "rb").read() == derived_expectation([src], "illumina", threads, single=True)
    f, r = os.path.join(cu.INPUTS, "test.f.fastq"), os.path.join(cu.INPUTS, "test.r.fastq")
    outs = [os.path.join(d, "pe_T_%d" % i) for i in range(3)]
    pr = cu.run_cli(hostcheck, workdir, ["pe", "-f", f, "-r", r, "-t", "illumina", "-o", outs[0], "-p", outs[1], "-s", outs[2],
                                         "-a", str(threads)], env=env)
    assert pr.returncode == 0, pr.stderr
    want = derived_expectation([f, r], "illumina", threads)
    for o, w in zip(outs, want):
        assert open(o, "rb").read() == w, (threads, o)


def test_usage_and_argument_errors(hostcheck, workdir):
    run = lambda *a: cu.run_cli(hostcheck, workdir, list(a))  # noqa: E731
    pr = run()
    assert pr.returncode == 1 and b"Usage: sickle <command> [options]" in pr.stdout
    pr = run("--help")
    assert pr.returncode == 0 and b"pe\tpaired-end sequence trimming" in pr.stdout
    pr = run("--version")
    assert pr.returncode == 0 and pr.stdout.startswith(b"sickle version 1.33\nCopyright (c) 2011")
    pr = run("se", "--version")
    assert pr.returncode == 0 and pr.stdout.startswith(b"sickle version 1.330\n")
    pr = run("se", "-f", "x", "-o", "y")
    assert pr.returncode == 1 and b"****Error: Must have quality type, input file, and output file." in pr.stderr
    pr = run("se", "-f", "{inputs}/test.fastq", "-t", "bogus", "-o", "{tmp}/o")
    assert pr.returncode == 1 and b"Error: Quality type 'bogus' is not a valid type." in pr.stderr
    pr = run("se", "-f", "{inputs}/test.fastq", "-t", "sanger", "-o", "{inputs}/test.fastq")
    assert pr.returncode == 1 and b"****Error: Input file is same as output file." in pr.stderr
    pr = run("se", "-f", "{inputs}/test.fastq", "-t", "sanger", "-o", "{tmp}/o", "-q", "-3")
    assert pr.returncode == 1 and b"Quality threshold must be >= 0" in pr.stderr
    pr = run("pe", "-f", "{inputs}/test.f.fastq", "-t", "sanger")
    assert pr.returncode == 1 and b"you must have the -r, -o, -p, and -s options" in pr.stderr
    pr = run("pe", "-c", "{inputs}/test.fastq", "-t", "sanger", "-M", "{tmp}/x")  # -M: accepted by getopt, unimplemented
    assert pr.returncode == 1 and b"Usage: sickle pe" in pr.stderr
    pr = run("pe", "-t", "sanger")
    assert pr.returncode == 1 and b"****Error: Must have either -f OR -c argument." in pr.stderr


def test_range_error_message_and_exit(hostcheck, workdir):
    """A phred+64 file read as sanger is fine; a sanger-range violation prints the reference's
    six lines and exits 1 (golden text from the reference itself in errors.json)."""
    import json
    cases = [c for c in json.load(open(os.path.join(cu.GOLD, "errors.json"))) if c["rc"] == 1 and len(c["seq"]) == 150]
    for c in cases[:6]:
        seq, qual = synth.make_reads(5, 40, 150, "illumina" if c["params"]["qualtype"] != "sanger" else "sanger")
        if c["params"]["qualtype"] == "solexa":
            pass  # illumina-range chars are legal solexa chars
        body = synth.fastq_bytes(seq[:20], qual[:20])
        bad = c["name"].encode("latin-1") + b"\n" + c["seq"].encode("latin-1") + b"\n+\n" + bytes.fromhex(c["qual_hex"]) + b"\n"
        path = os.path.join(str(workdir), "bad.fastq")
        open(path, "wb").write(body + bad + synth.fastq_bytes(seq[20:], qual[20:], start=20))
        pr = cu.run_cli(hostcheck, workdir, ["se", "-f", path, "-t", c["params"]["qualtype"], "-o", "{tmp}/bad_out.fastq", "-a", "1"])
        assert pr.returncode == 1, c["desc"]
        assert pr.stderr.decode("latin-1") == c["stderr"], c["desc"]


def test_malformed_records_exit_like_reference(hostcheck, workdir):
    good = b"@r1\nACGT\n+\nIIII\n"
    for bad, needle in ((b"@\nACGT\n+\nIIII\n", b"[ERROR] Sequence ID is to short."),
                        (b"r2\nACGT\n+\nIIII\n", b"[ERROR] Invalid char at the beggining of ID."),
                        (b"@r2\nACGT\n+\nIII\n", b"[ERROR] Sequence and quality lines have different lengths:"),
                        (b"@r2\n\n+\n\n", b"[ERROR] Sequence line is empty")):
        path = os.path.join(str(workdir), "mal.fastq")
        open(path, "wb").write(good * 30 + bad + good * 30)
        pr = cu.run_cli(hostcheck, workdir, ["se", "-f", path, "-t", "sanger", "-o", "{tmp}/mal_out.fastq"])
        assert pr.returncode == 1 and needle in pr.stderr, (bad, pr.stderr)


def test_missing_trailing_newline_loses_last_char(hostcheck, workdir):
    """reference src/GZReader.cpp:81-88: the last line of a file without a final newline is stored
    minus its last character, so the record fails the length check."""
    path = os.path.join(str(workdir), "nonl.fastq")
    open(path, "wb").write(b"@r1\nACGT\n+\nIIII\n" * 50 + b"@r2\nACGT\n+\nIIII")
    pr = cu.run_cli(hostcheck, workdir, ["se", "-f", path, "-t", "sanger", "-o", "{tmp}/nonl_out.fastq"])
    assert pr.returncode == 1 and b"Sequence and quality lines have different lengths:" in pr.stderr


def test_gzip_output_roundtrip(hostcheck, workdir):
    import gzip
    out = os.path.join(str(workdir), "o.fastq.gz")
    plain = os.path.join(str(workdir), "o_plain.fastq")
    src = os.path.join(cu.INPUTS, "test.fastq")
    assert cu.run_cli(hostcheck, workdir, ["se", "-f", src, "-t", "illumina", "-o", out, "-g", "-a", "1"]).returncode == 0
    assert cu.run_cli(hostcheck, workdir, ["se", "-f", src, "-t", "illumina", "-o", plain, "-a", "1"]).returncode == 0
    assert gzip.open(out, "rb").read() == open(plain, "rb").read()


def test_empty_and_truncated_inputs(hostcheck, workdir):
    """An empty file, a file that is all one partial record, and a file whose last record is cut
    short: the reference returns no batch / drops the tail (src/GZReader.cpp:29-41,104-129)."""
    d = str(workdir)
    rec = b"@r%d\nACGTACGTACGTACGTACGTACGT\n+\nIIIIIIIIIIIIIIIIIIIIIIII\n"
    cases = {
        "empty.fastq": (b"", 0),
        "partial_only.fastq": (b"@r1\nACGT\n+\n", 0),
        "cut_tail.fastq": (b"".join(rec % i for i in range(40)) + b"@r40\nACGTACGTAC\n", 40),
    }
    for name, (data, kept) in cases.items():
        path = os.path.join(d, name)
        open(path, "wb").write(data)
        out = os.path.join(d, name + ".out")
        pr = cu.run_cli(hostcheck, workdir, ["se", "-f", path, "-t", "sanger", "-o", out, "-a", "1"])
        assert pr.returncode == 0, (name, pr.stderr)
        assert ("FastQ records kept: %d\n" % kept).encode() in pr.stdout, (name, pr.stdout)
        got = parse_fastq(open(out, "rb").read())
        assert len(got) == kept
    if ob.have_ref():  # the same three files through the reference's working driver (self-paired pe)
        for name, (data, kept) in cases.items():
            path = os.path.join(d, name)
            copy = os.path.join(d, "copy_" + name)
            open(copy, "wb").write(data)
            # The reference's per-batch output threads race each other for the file (this 1 kB input is eight
            # batches) and its main thread does not wait for the last of them (src/trim_paired.cpp:445-458): now and
            # then file 1 comes out in another batch order, or short.  Every run must hold records of ours only, one
            # run in six all of them (the order is pinned by the thread-order goldens and the soak, not here).
            ours = sorted(parse_fastq(open(os.path.join(d, name + ".out"), "rb").read()))
            complete = False
            for attempt in range(6):
                pr = subprocess.run([ob.REF_BIN, "pe", "-f", path, "-r", copy, "-t", "sanger", "-o", path + ".r1", "-p",
                                     path + ".r2", "-s", path + ".rs", "-a", "1"], capture_output=True, timeout=60)
                assert pr.returncode == 0
                try:
                    theirs = sorted(parse_fastq(open(path + ".r1", "rb").read()))
                except AssertionError:  # cut inside a record
                    continue
                assert all(r in ours for r in theirs), (name, attempt)
                if theirs == ours:
                    complete = True
                    break
            assert complete, name


def test_output_to_a_pipe(hostcheck, workdir):
    """-o /dev/stdout: not seekable, so no positional writes; the records still arrive in order."""
    src = os.path.join(cu.INPUTS, "test.fastq")
    plain = os.path.join(str(workdir), "pipe_ref.fastq")
    assert cu.run_cli(hostcheck, workdir, ["se", "-f", src, "-t", "illumina", "-o", plain, "-a", "1", "--quiet"]).returncode == 0
    pr = subprocess.run("%s se -f %s -t illumina -o /dev/stdout -a 1 --quiet | cat" % (hostcheck, src), shell=True,
                        capture_output=True, timeout=120)
    assert pr.returncode == 0
    assert pr.stdout == open(plain, "rb").read()


# ---------------------------------------------------------------- BGZF (blocked gzip) in and out
def _bgzf_block(payload, level=6):
    import struct
    import zlib
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(payload) + c.flush()
    total = 18 + len(body) + 8
    return (b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", total - 1) + body +
            struct.pack("<II", zlib.crc32(payload) & 0xffffffff, len(payload)))


def _bgzf_blocks(data, rng, with_empty=True):
    out, at = [], 0
    while at < len(data):
        n = int(rng.integers(1, 0xff00))
        out.append(_bgzf_block(data[at:at + n]))
        at += n
        if with_empty and rng.random() < 0.05:
            out.append(_bgzf_block(b""))
    out.append(_bgzf_block(b""))  # end-of-file marker
    return out


def _walk_bgzf(blob):
    """Block sizes of a BGZF file, asserting every member has the BC field."""
    import struct
    at, sizes = 0, []
    while at < len(blob):
        assert blob[at:at + 4] == b"\x1f\x8b\x08\x04" and blob[at + 12:at + 16] == b"BC\x02\x00", at
        total = struct.unpack_from("<H", blob, at + 16)[0] + 1
        sizes.append(struct.unpack_from("<I", blob, at + total - 4)[0])
        at += total
    assert at == len(blob)
    return sizes


def _synthetic_fastq(n, seed):
    import numpy as np
    from sickle_amd import synth
    rng = np.random.default_rng(seed)
    q, s, lens = synth.make_ragged_reads(n, 30, 120, seed=seed, qualtype="sanger")
    return synth.fastq_bytes(q, s, lens) if hasattr(synth, "fastq_bytes") else None, rng


def test_gzip_output_is_bgzf_and_reads_back(hostcheck, workdir):
    """-g writes BGZF: every member carries its size, the file ends with the empty marker block,
    any gzip reader inflates it to the plain output, and this reader takes it as input again
    (block-parallel path) with the same result as the plain file."""
    import gzip
    d = str(workdir)
    src = os.path.join(cu.INPUTS, "test.fastq")
    big = os.path.join(d, "bgzf_src.fastq")
    open(big, "wb").write(open(src, "rb").read() * 40)  # several blocks per worker
    out, plain = os.path.join(d, "bz.fastq.gz"), os.path.join(d, "bz_plain.fastq")
    fast, gpu = os.path.join(d, "bz_fast.fastq.gz"), os.path.join(d, "bz_gpu.fastq.gz")
    for extra, o, env in ((["-g"], out, None), ([], plain, None), (["-g"], fast, {"SICKLE_GZ_LEVEL": "fast"}),
                          (["-g"], gpu, {"SICKLE_GZ_LEVEL": "gpu"})):  # (the host build runs the GPU encoder's phases on the CPU)
        assert cu.run_cli(hostcheck, workdir, ["se", "-f", big, "-t", "illumina", "-o", o, "-a", "3"] + extra, env=env).returncode == 0
    for alt in (fast, gpu):
        assert gzip.decompress(open(alt, "rb").read()) == open(plain, "rb").read() and _walk_bgzf(open(alt, "rb").read())[-1] == 0
    blob = open(out, "rb").read()
    sizes = _walk_bgzf(blob)
    assert sizes[-1] == 0 and len(sizes) > 20 and max(sizes) <= 0xff00
    assert gzip.decompress(blob) == open(plain, "rb").read()
    # read it back: BGZF path, streaming path and plain input agree (-a 1: with more queues the
    # order depends on the batch cuts, and those on the size of the file on disk)
    outs = []
    for name, path, env in (("a", out, None), ("b", out, {"SICKLE_NO_BGZF": "1"}), ("c", plain, None)):
        o = os.path.join(d, "bz_back_%s.fastq" % name)
        pr = cu.run_cli(hostcheck, workdir, ["se", "-f", path, "-t", "illumina", "-o", o, "-q", "25", "-a", "1"], env=env)
        assert pr.returncode == 0
        outs.append((open(o, "rb").read(), cu.summary_block(pr.stdout.decode())))
    assert outs[0][0] == outs[1][0] == outs[2][0] and len(outs[0][0]) > 0
    assert outs[0][1] == outs[1][1]
    # nothing kept: the file is just the marker block and still a valid (empty) gzip file
    none = os.path.join(d, "bz_none.fastq.gz")
    assert cu.run_cli(hostcheck, workdir, ["se", "-f", src, "-t", "illumina", "-o", none, "-g", "-l", "5000"]).returncode == 0
    assert len(open(none, "rb").read()) == 28 and gzip.decompress(open(none, "rb").read()) == b""


def test_bgzf_input_odd_files(hostcheck, workdir):
    """BGZF input the parallel reader has to hand over to zlib part-way: empty blocks, a plain gzip
    member in the middle, a file cut inside its last block, a block with a wrong CRC, a block whose
    data is damaged.  In every case the result must be what the streaming reader (zlib's gzread,
    i.e. the reference's gzgets on the same bytes) gives."""
    import gzip
    import numpy as np
    d = str(workdir)
    rng = np.random.default_rng(77)
    text = open(os.path.join(cu.INPUTS, "test.fastq"), "rb").read() * 25
    blocks = _bgzf_blocks(text, rng)
    assert len(blocks) > 60
    mid = len(blocks) // 2
    cut = b"".join(blocks[:-1])
    bad_crc = bytearray(b"".join(blocks))
    off = len(b"".join(blocks[:mid]))
    bad_crc[off + len(blocks[mid]) - 8] ^= 0x5a
    bad_data = bytearray(b"".join(blocks))
    bad_data[off + 18 + 20] ^= 0xff
    files = {
        "ok.gz": b"".join(blocks),
        "mixed.gz": b"".join(blocks[:mid]) + gzip.compress(b"".join(gzip.decompress(b) for b in blocks[mid:mid + 5])) +
                    b"".join(blocks[mid + 5:]),
        "cut.gz": cut[:len(cut) - 37],
        "badcrc.gz": bytes(bad_crc),
        "baddata.gz": bytes(bad_data),
    }
    assert gzip.decompress(files["ok.gz"]) == text and gzip.decompress(files["mixed.gz"]) == text
    for name, blob in files.items():
        path = os.path.join(d, "odd_" + name)
        open(path, "wb").write(blob)
        res = []
        for tag, env in (("par", None), ("str", {"SICKLE_NO_BGZF": "1"})):
            o = os.path.join(d, "odd_%s_%s.fastq" % (name, tag))
            pr = cu.run_cli(hostcheck, workdir, ["se", "-f", path, "-t", "illumina", "-o", o, "-b", "1"], env=env)
            res.append((pr.returncode, open(o, "rb").read() if os.path.exists(o) else None,
                        cu.summary_block(pr.stdout.decode()), pr.stderr))
        # (a run that dies on a malformed record leaves however much output its writer had got to)
        if name.startswith("bad"):
            # damaged data: the input ends at (parallel) or within 1 MiB before (streaming) the bad
            # block, with a warning; where exactly the reference's gzgets stops depends on zlib's
            # buffer state, so this is not pinned -- no crash, no hang, and the warning is there
            assert all(r[0] in (0, 1) and b"****Warning:" in r[3] for r in res), name
            continue
        assert res[0][0] == res[1][0] and res[0][3] == res[1][3], name
        if res[0][0] == 0:
            assert res[0] == res[1], name
        if name in ("ok.gz", "mixed.gz"):
            assert res[0][0] == 0 and len(res[0][1]) > 0


def test_gzip_input_own_decoder_matches_zlib(hostcheck, workdir):
    """Plain (single-stream) gzip input: the serial mapped-file decoder, the parallel one (forced
    on this small file with 60 KB stretches) and zlib's gzread give the same run, at several
    compression levels and with a second member appended."""
    import zlib
    d = str(workdir)
    text = open(os.path.join(cu.INPUTS, "test.fastq"), "rb").read() * 20
    for level in (1, 6, 9):
        c = zlib.compressobj(level, zlib.DEFLATED, 31)
        blob = c.compress(text[:len(text) // 2]) + c.flush()
        c = zlib.compressobj(level, zlib.DEFLATED, 31)
        blob += c.compress(text[len(text) // 2:]) + c.flush()
        path = os.path.join(d, "own_l%d.fastq.gz" % level)
        open(path, "wb").write(blob)
        res = []
        for tag, env in (("own", None), ("zlib", {"SICKLE_ZLIB_INFLATE": "1"}), ("par", {"SICKLE_GZ_CHUNK": "60000"})):
            o = os.path.join(d, "own_l%d_%s.fastq" % (level, tag))
            pr = cu.run_cli(hostcheck, workdir, ["se", "-f", path, "-t", "illumina", "-o", o, "-b", "2", "-a", "2"], env=env)
            res.append((pr.returncode, open(o, "rb").read(), cu.summary_block(pr.stdout.decode()), pr.stderr))
        assert res[0] == res[1] == res[2] and res[0][0] == 0 and len(res[0][1]) > 1000000


def test_drivers_embedded_as_a_library(workdir):
    """reference src/sickle.cpp:61-80 as a library caller would write it: several Trim_Paired / Trim_Single runs in one
    process, each trimmer on the stack, sickle_leave_fast false -- close_streams() / close_device() / the destructor
    release everything (host build against the oracle-backed shim; tests/test_cli_gpu.py does the product)."""
    cu.check_embedded(cu.build_embed("embed_host"), workdir, gpu=False)

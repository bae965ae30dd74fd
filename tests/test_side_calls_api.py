"""The one object the Python drivers build from their behind-call keywords (capi._SideCalls) and the clip-word decode,
without a device: what each option builds, what each bad value raises and in which order, and what collect leaves alone."""
import numpy as np
import pytest
import torch

from sickle_amd import capi

SEQS = {"seqs": ["AGATCGGAAGAGC"]}
BUFFERS = ("clp", "rep", "aud", "bas", "adp")


def side(mode="pe_interleaved", clip_ok=False, **options):
    return capi._SideCalls("cpu", clip_ok, mode, **options)


def test_all_off_holds_no_tensor():
    s = side()
    assert all(getattr(s, name) is None for name in BUFFERS) and s.rej_flags is None and s.mode == "pe_interleaved"
    assert not any(isinstance(v, torch.Tensor) for v in vars(s).values())
    # what is off by its falsy value is off; clip_adapters alone is off by None only
    s = side(report=False, audit=False, bases=False, rejects=False, adapters=False, clip_adapters=None)
    assert all(getattr(s, name) is None for name in BUFFERS) and s.rej_flags is None
    s.rewind()  # nothing to put back


def only(s, name):
    assert [n for n in BUFFERS if getattr(s, n) is not None] == [name] and s.rej_flags is None
    return getattr(s, name)


def test_each_option_alone_builds_its_buffers():
    """the fields are the ones the constructor called directly gives"""
    r = only(side(report=True), "rep")
    assert isinstance(r, capi._ReportBuffers) and (r.len_bins, r.pos_bins, r.hists) == (0, 0, None)
    assert r.buf.numel() == capi.REPORT_WORDS and r.ptr == r.buf.data_ptr()
    r = only(side(report=dict(len_bins=5, pos_bins=3)), "rep")
    assert (r.len_bins, r.pos_bins) == (5, 3) and r.buf.numel() == capi.REPORT_WORDS + 2 * 5 + 4 * 3
    assert r.hists.len_bins == 5 and r.hists.pos_bins == 3 and r.hists.len_in == r.ptr + 8 * capi.REPORT_WORDS
    a = only(side(audit=True), "aud")
    assert isinstance(a, capi._AuditBuffers) and a.buf.numel() == capi.AUDIT_WORDS + 256
    assert a.hist_ptr == a.ptr + 8 * capi.AUDIT_WORDS
    b = only(side(bases=True), "bas")
    assert isinstance(b, capi._BasesBuffers) and (b.pos_bins, b.gc, b.hists) == (0, False, None)
    assert b.buf.numel() == capi.BASES_WORDS
    b = only(side(bases=dict(pos_bins=7, gc=True)), "bas")
    assert (b.pos_bins, b.gc) == (7, True) and b.buf.numel() == capi.BASES_WORDS + 12 * 7 + 2 * capi.SK_FQ_BASES_GC_BINS
    assert b.hists.pos_bins == 7 and b.hists.gc_in == b.ptr + 8 * (capi.BASES_WORDS + 12 * 7)
    d = only(side(adapters=dict(SEQS, pos_bins=5, overlap=True)), "adp")
    assert isinstance(d, capi._AdaptersBuffers) and d.buf.numel() == capi.ADAPTERS_WORDS + 40 + 8 * 65
    assert d.out.pos_bins == 5 and d.out.clip is None and d.clip is None and not d.want_clip
    assert d.set.n == 1 and d.set.len[0] == 13 and (d.set.min_overlap, d.set.max_mismatch_permille) == (3, 100)
    d = only(side(adapters=dict(SEQS, clip=True), clip_ok=True), "adp")
    assert d.want_clip and d.clip is None and d.out is None  # the words come with with_clip, once the reads are known
    c = only(side(clip_adapters=dict(SEQS, min_overlap=4)), "clp")
    assert isinstance(c, capi._ClipBuffers) and c.buf.numel() == capi.CLIP_WORDS == 16 and not c.buf.any()
    assert c.reset is True and c.words_ptr is None and not c.want_clip and c.set.min_overlap == 4
    c = only(side(clip_adapters=dict(SEQS, clip=True), clip_ok=True), "clp")
    assert c.want_clip
    for rejects, flags in ((True, 0), ("pairs", capi.SK_FQ_REJECTS_PAIRS), (1, 1)):
        s = side(rejects=rejects)
        assert s.rej_flags == flags and all(getattr(s, name) is None for name in BUFFERS)
    assert side(mode="se", rejects=True).rej_flags == 0


def test_all_on():
    s = side(clip_ok=True, report=True, audit=True, bases=True, rejects="pairs", adapters=SEQS, clip_adapters=SEQS)
    assert all(getattr(s, name) is not None for name in BUFFERS) and s.rej_flags == capi.SK_FQ_REJECTS_PAIRS


@pytest.mark.parametrize("options, message", [
    (dict(report={"gc": True}), "report: unknown keys ['gc']"),
    (dict(bases={"len_bins": 4}), "bases: unknown keys ['len_bins']"),
    (dict(adapters=dict(SEQS, len_bins=4)), "adapters: unknown keys ['len_bins']"),
    (dict(clip_adapters=dict(SEQS, pos_bins=4)), "clip_adapters: unknown keys ['pos_bins']"),
    (dict(adapters=True), "adapters: a dict with seqs=[...]"),
    (dict(clip_adapters={}), "clip_adapters: a dict with seqs=[...]"),
    (dict(clip_adapters=False), "clip_adapters: a dict with seqs=[...]"),
    (dict(rejects="pair"), "rejects: False, True or \"pairs\", not 'pair'"),
    (dict(rejects="pairs", mode="se"), "rejects=\"pairs\" needs a pair mode"),
    (dict(adapters=dict(SEQS, clip=True)), "adapters: clip=True is trim_fastq's alone"),
    (dict(clip_adapters=dict(SEQS, clip=True)), "clip_adapters: clip=True is trim_fastq's alone"),
])
def test_bad_values_and_their_messages(options, message):
    with pytest.raises(ValueError) as e:
        side(**options)
    assert str(e.value) == message


def test_the_earlier_bad_option_wins():
    """the order is clip_adapters, report, audit, bases, adapters, rejects: of two bad options the earlier one raises"""
    bad = [("clip_adapters", {"seq": []}, "clip_adapters:"), ("report", {"gc": 1}, "report:"), ("bases", {"len_bins": 4}, "bases:"),
           ("adapters", True, "adapters:"), ("rejects", "pair", "rejects:")]
    for i, (first, value, word) in enumerate(bad):
        for later, later_value, _ in bad[i + 1:]:
            with pytest.raises(ValueError) as e:
                side(**{later: later_value, first: value})
            assert str(e.value).startswith(word), (first, later)
    with pytest.raises(ValueError) as e:  # the pair-mode check is the rejects' own: behind the adapters'
        side(mode="se", rejects="pairs", adapters=True)
    assert str(e.value).startswith("adapters:")


def test_collect():
    counts = {"records": [1, 2, 3], "bytes": [4, 5, 6]}
    before = {k: list(v) for k, v in counts.items()}
    assert side().collect(counts) is None and counts == before
    assert side(rejects=True).collect(counts) is None and counts == before  # the rejects are the driver's to finish
    s = side(report=dict(len_bins=2), audit=True, bases=True, adapters=SEQS, clip_adapters=SEQS)
    for b in (s.rep, s.aud, s.bas, s.adp):
        b.buf.zero_()
    s.rep.buf[2], s.aud.buf[2], s.bas.buf[2], s.adp.buf[2], s.clp.buf[2] = 11, 12, 13, 14, 15  # reads, pairs, reads, reads, reads
    report = s.collect(counts)
    assert list(counts) == ["records", "bytes", "audit", "bases", "adapters", "clip"]
    assert report["reads"] == 11 and report["len_in"].tolist() == [0, 0] and "qsum_in" not in report
    assert counts["audit"]["pairs"] == 12 and len(counts["audit"]["qual_hist"]) == 256
    assert counts["bases"]["reads"] == 13 and counts["adapters"]["reads"] == 14 and counts["clip"]["reads"] == 15
    assert counts["records"] == [1, 2, 3]
    only_report = side(report=True)
    only_report.rep.buf.zero_()
    got = {}
    assert only_report.collect(got)["calls"] == 0 and got == {}


def test_rewind_puts_back_what_a_run_leaves():
    s = side(clip_ok=True, adapters=dict(SEQS, clip=True), clip_adapters=SEQS)
    s.adp.with_clip(5)
    s.clp.reset, s.clp.words_ptr = False, 0x1000
    assert s.adp.out.clip_capacity == 5
    s.rewind()
    assert s.adp.clip is None and s.adp.out is None and s.clp.reset is True and s.clp.words_ptr is None


def test_decode_clip_words():
    raw = np.array([(2 << 24) | 37,         # a plain hit: adapter 2 at base 37
                    capi.SK_FQ_CLIP_NONE,   # no hit
                    (7 << 24) | 0,          # the last adapter, at the read's start
                    (0 << 24) | 0xFFFFFF,   # the largest clip point a word holds
                    (7 << 24) | 0xFFFFFE], dtype=np.uint32)
    clip, adapter = capi._decode_clip_words(torch.from_numpy(raw.view(np.int32)))
    assert clip.dtype == adapter.dtype == torch.int64
    assert clip.tolist() == [37, -1, 0, 0xFFFFFF, 0xFFFFFE] and adapter.tolist() == [2, -1, 7, 0, 7]
    clip, adapter = capi._decode_clip_words(torch.empty(0, dtype=torch.int32))
    assert clip.numel() == 0 and adapter.numel() == 0

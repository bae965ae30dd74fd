"""What the adapter search (sk_trim_fastq_adapters_device_async, sickle_amd/csrc/sk_fastq_adapters.hip) costs behind a text
call, on the 10 M x 150 bp text of tools/fastq_trim_rates.py on one MI355X.

Four variants are timed with HIP events around what is enqueued, alternated within one job on one device, `--rounds`
rounds of `--iters` calls each:
  trim                  sk_trim_fastq_device_async alone
  trim+adapters_1x13    ... and the search for one 13-base adapter, with pos, overlap and clip
  trim+adapters_1x33    ... for one 33-base adapter
  trim+adapters_8x33    ... for eight 33-base adapters
The text's bases are drawn, so at `--min-overlap` 10 and `--permille` 100 next to no read has a hit and every line is
walked to its last start: the pass's full cost (a hit ends a line's walk at its tile).  One JSON line per variant with the
median and min-max over all rounds, the search's own time (the variant's median less the trim's), its ratio to the trim's
and the base comparisons the rule asks for per read (line length x adapter bases); --out also writes them to a file.
--once: one warm call of the trim with each search behind it, twice, and nothing else (for a run under
`rocprofv3 --kernel-trace --stats`)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

TRUSEQ_13 = "AGATCGGAAGAGC"
TRUSEQ_33 = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"  # the TruSeq read-1 adapter's first 33 bases
EIGHT_33 = [TRUSEQ_33, "AGATCGGAAGAGCGTCGTGTAGGGAAAGAGTGT", "CTGTCTCTTATACACATCTCCGAGCCCACGAGA", "CTGTCTCTTATACACATCTGACGCTGCCGACGA",
            "TGGAATTCTCGGGTGCCAAGGAACTCCAGTCAC", "AATGATACGGCGACCACCGAGATCTACACTCTT", "CAAGCAGAAGACGGCATACGAGATCGTGATGTG",
            "GTTCGTCTTCTGCCGTATGCTCTAGCACTACAC"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bins", type=int, default=512)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--min-overlap", type=int, default=10)
    ap.add_argument("--permille", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()
    from fastq_trim_rates import make_text
    from sickle_amd import capi
    ctx = capi.Context(device=0)
    L = capi.lib()
    mode = "se"
    text = make_text(torch, args.reads, args.length, args.length, 1)
    params = capi.make_params("sanger", 20, 50, False, False)
    T = text.numel()
    nb = L.sk_trim_fastq_workspace_bytes(T, params.trunc_n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ptrs, sizes = [text.data_ptr()], [T]
    ctx.trim_fastq_device_async(params, ptrs, sizes, [capi.FastqOutput() for _ in range(3)], ws.data_ptr(), nb, mode=mode)
    counts = ctx.trim_fastq_device_finish(ws.data_ptr())
    bufs, outs = [], []
    for o in range(3):
        t = torch.empty(counts["bytes"][o] + 16, dtype=torch.uint8, device="cuda")
        bufs.append(t)
        outs.append(capi.FastqOutput(t.data_ptr(), counts["bytes"][o], None, counts["records"][o]))
    B, V = args.bins, capi.SK_FQ_ADAPTERS_OVERLAP_BINS
    res = torch.zeros(capi.ADAPTERS_WORDS + 8 * B + 8 * V, dtype=torch.int64, device="cuda")
    clip = torch.empty(args.reads, dtype=torch.int32, device="cuda")
    at = lambda words: res.data_ptr() + 8 * (capi.ADAPTERS_WORDS + words)
    out = capi.FastqAdaptersOut(at(0), B, at(8 * B), clip.data_ptr(), args.reads)
    sets = {"1x13": [TRUSEQ_13], "1x33": [TRUSEQ_33], "8x33": EIGHT_33}
    structs = {k: capi.adapter_set(v, args.min_overlap, args.permille) for k, v in sets.items()}

    def call(which):
        ctx.trim_fastq_device_async(params, ptrs, sizes, outs, ws.data_ptr(), nb, mode=mode)
        if which:
            ctx.trim_fastq_adapters_device_async(ws.data_ptr(), T, params.trunc_n, res.data_ptr(), ptrs, sizes, structs[which],
                                                 mode=mode, out=out, reset=True)

    variants = [("trim", None)] + [("trim+adapters_" + k, k) for k in sets]
    if args.once:
        for _ in range(2):
            for _, which in variants[1:]:
                call(which)
                ctx.trim_fastq_device_finish(ws.data_ptr())
        ctx.close()
        return
    for _, which in variants:  # warm-up
        call(which)
        ctx.trim_fastq_device_finish(ws.data_ptr())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {v: [] for v, _ in variants}
    got = {}
    for _ in range(args.rounds):
        for v, which in variants:
            for _ in range(args.iters):
                e0.record()
                call(which)
                e1.record()
                ctx.trim_fastq_device_finish(ws.data_ptr())
                ms[v].append(e0.elapsed_time(e1))
            if which:
                got[v] = capi.FastqAdapters.from_buffer_copy(res.cpu().numpy()[:capi.ADAPTERS_WORDS].tobytes()).as_dict()
    median = lambda xs: sorted(xs)[len(xs) // 2]
    trim_ms = median(ms["trim"])
    lines = []
    for v, which in variants:
        x = sorted(ms[v])
        r = {"config": "se_%d" % args.length, "variant": v, "mode": mode, "text_bytes": T, "calls": len(x),
             "median_ms": round(median(x), 3), "min_ms": round(x[0], 3), "max_ms": round(x[-1], 3), "trim_median_ms": round(trim_ms, 3)}
        if which:
            bases = sum(len(s) for s in sets[which])
            own = median(x) - trim_ms
            r.update({"adapters": len(sets[which]), "adapter_bases": bases, "min_overlap": args.min_overlap,
                      "max_mismatch_permille": args.permille, "pos_bins": B, "reads": got[v]["reads"],
                      "reads_hit": got[v]["reads_hit"], "adapters_ms": round(own, 3), "ratio_to_trim": round(own / trim_ms, 3),
                      "comparisons_per_read": args.length * bases,
                      "Gcomparisons_per_s": round(got[v]["reads"] * args.length * bases / own / 1e6, 1)})
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))
    ctx.close()


if __name__ == "__main__":
    main()

"""What the clipped text call (sk_trim_fastq_clipped_device_async, the search of sk_fq_clip_kernel in
sickle_amd/csrc/sk_fastq_adapters.hip in front of the pack) costs, on the 10 M x 150 bp text of tools/fastq_trim_rates.py on
one MI355X, -q 20 -l 50.

The variants are timed with HIP events around what is enqueued, alternated within one job on one device, `--rounds` rounds
of `--iters` calls each, after a warm-up call of each:
  trim                          sk_trim_fastq_device_async alone, on the drawn text
  trim+adapters_1x13            ... and the side search of DESIGN 4.21 for one 13-base adapter, with its clip words
  clipped_1x13_drawn            the clipped call with one 13-base adapter on the drawn text (next to no hit: every line is
  clipped_8x33_drawn            walked to its last start), and with eight 33-base adapters
  trim_planted                  the unclipped call on the text with the adapter planted into half of the reads at drawn starts
  clipped_1x13_planted          the clipped calls on that text: the packed batch is then of mixed lengths, so the scan
  clipped_8x33_planted          regroups it (sk_sort.hip), while a hit ends a line's walk early and less is packed and written
One JSON line per variant with the median and min-max over all rounds and the difference to the unclipped call on the same
text; --out also writes them to a file.  The search's own time and the scan's are told apart by the kernel trace:
--once --input drawn|planted runs the trim, the side search and the two clipped calls once each, warm, and nothing else
(for a run under `rocprofv3 --kernel-trace --stats`)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tools", "probes"))


def plant(torch, text, n, length, adapter, seed):
    """a copy of the text of n records of `length` bases with `adapter` written over half of the seq lines at a drawn start
    1 .. length - 1 (cut at the line's end)"""
    stride = 12 + 2 * length + 4
    out = text.clone().view(n, stride)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    chosen = torch.nonzero(torch.rand(n, generator=g, device="cuda") < 0.5).flatten()
    start = torch.randint(1, length, (chosen.numel(),), generator=g, device="cuda")
    for j, b in enumerate(adapter.encode()):
        ok = start + j < length
        out[chosen[ok], 12 + start[ok] + j] = b
    return out.view(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--min-overlap", type=int, default=10)
    ap.add_argument("--permille", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--input", choices=("drawn", "planted"), default="drawn")
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()
    from fastq_adapters_rate import EIGHT_33, TRUSEQ_13
    from fastq_trim_rates import make_text
    from sickle_amd import capi
    ctx = capi.Context(device=0)
    L = capi.lib()
    mode = "se"
    texts = {"drawn": make_text(torch, args.reads, args.length, args.length, 1)}
    if not args.once or args.input == "planted":
        texts["planted"] = plant(torch, texts["drawn"], args.reads, args.length, TRUSEQ_13, 2)
    params = capi.make_params("sanger", 20, 50, False, False)
    T = texts["drawn"].numel()
    base = L.sk_trim_fastq_workspace_bytes(T, params.trunc_n)
    nb = base + L.sk_trim_fastq_clip_extra_bytes(T)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    # the unclipped call writes the most: its outputs hold every variant's
    ctx.trim_fastq_device_async(params, [texts["drawn"].data_ptr()], [T], [capi.FastqOutput() for _ in range(3)], ws.data_ptr(), base,
                                mode=mode)
    counts = ctx.trim_fastq_device_finish(ws.data_ptr())
    bufs, outs = [], []
    for o in range(3):
        t = torch.empty(counts["bytes"][o] + 16, dtype=torch.uint8, device="cuda")
        bufs.append(t)
        outs.append(capi.FastqOutput(t.data_ptr(), counts["bytes"][o], None, counts["records"][o]))
    side = torch.zeros(capi.ADAPTERS_WORDS, dtype=torch.int64, device="cuda")
    side_clip = torch.empty(args.reads, dtype=torch.int32, device="cuda")
    side_out = capi.FastqAdaptersOut(None, 0, None, side_clip.data_ptr(), args.reads)
    stats = torch.zeros(capi.CLIP_WORDS, dtype=torch.int64, device="cuda")
    sets = {"1x13": [TRUSEQ_13], "8x33": EIGHT_33}
    structs = {k: capi.adapter_set(v, args.min_overlap, args.permille) for k, v in sets.items()}

    def call(kind, which, text):
        ptrs, sizes = [texts[text].data_ptr()], [T]
        if kind == "clipped":
            ctx.trim_fastq_clipped_device_async(params, ptrs, sizes, structs[which], outs, ws.data_ptr(), nb, mode=mode,
                                                stats_ptr=stats.data_ptr(), reset=True)
            return
        ctx.trim_fastq_device_async(params, ptrs, sizes, outs, ws.data_ptr(), base, mode=mode)
        if kind == "side":
            ctx.trim_fastq_adapters_device_async(ws.data_ptr(), T, params.trunc_n, side.data_ptr(), ptrs, sizes, structs[which],
                                                 mode=mode, out=side_out, reset=True)

    variants = [("trim", "trim", None, "drawn"), ("trim+adapters_1x13", "side", "1x13", "drawn"),
                ("clipped_1x13_drawn", "clipped", "1x13", "drawn"), ("clipped_8x33_drawn", "clipped", "8x33", "drawn"),
                ("trim_planted", "trim", None, "planted"), ("clipped_1x13_planted", "clipped", "1x13", "planted"),
                ("clipped_8x33_planted", "clipped", "8x33", "planted")]
    if args.once:
        todo = [("trim", None), ("side", "1x13"), ("side", "8x33"), ("clipped", "1x13"), ("clipped", "8x33")]
        for _ in range(2):  # the first round warms up; both are in the trace
            for kind, which in todo:
                call(kind, which, args.input)
                ctx.trim_fastq_device_finish(ws.data_ptr())
        ctx.close()
        return
    for _, kind, which, text in variants:  # warm-up
        call(kind, which, text)
        ctx.trim_fastq_device_finish(ws.data_ptr())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {v[0]: [] for v in variants}
    got, out_bytes = {}, {}
    for _ in range(args.rounds):
        for v, kind, which, text in variants:
            for _ in range(args.iters):
                e0.record()
                call(kind, which, text)
                e1.record()
                c = ctx.trim_fastq_device_finish(ws.data_ptr())
                ms[v].append(e0.elapsed_time(e1))
            out_bytes[v] = c["bytes"][0]
            if kind == "clipped":
                got[v] = capi.FastqClipStats.from_buffer_copy(stats.cpu().numpy().tobytes()).as_dict()
    median = lambda xs: sorted(xs)[len(xs) // 2]
    lines = []
    for v, kind, which, text in variants:
        x = sorted(ms[v])
        ref = median(ms["trim" if text == "drawn" else "trim_planted"])
        r = {"config": "se_%d" % args.length, "variant": v, "mode": mode, "input": text, "text_bytes": T, "calls": len(x),
             "median_ms": round(median(x), 3), "min_ms": round(x[0], 3), "max_ms": round(x[-1], 3),
             "unclipped_median_ms": round(ref, 3), "over_unclipped_ms": round(median(x) - ref, 3), "bytes_out": out_bytes[v]}
        if which:
            r.update({"adapters": len(sets[which]), "adapter_bases": sum(len(s) for s in sets[which]),
                      "min_overlap": args.min_overlap, "max_mismatch_permille": args.permille})
        if kind == "clipped":
            r.update({k: got[v][k] for k in ("reads", "reads_clipped", "reads_emptied", "bases_clipped")})
        print(json.dumps(r), flush=True)
        lines.append(r)
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))
    ctx.close()


if __name__ == "__main__":
    main()

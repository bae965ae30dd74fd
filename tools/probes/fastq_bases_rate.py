"""What the bases (sk_trim_fastq_bases_device_async, sickle_amd/csrc/sk_fastq_bases.hip) cost behind a text call, on the
four texts of tools/fastq_trim_rates.py on one MI355X.

Three variants are timed with HIP events around what is enqueued, alternated within one job on one device, `--rounds`
rounds of `--iters` calls each:
  trim             sk_trim_fastq_device_async alone
  trim+bases       ... and the bases without arrays (reset, the pass without its position tables)
  trim+bases+pos   ... and the full bases: both position tables at `--bins` bins and both GC histograms
and the read-stream rate sk_probe_read_bandwidth gives on the texts' bytes in the same job: the pass reads the seq lines
out of those bytes, so the time the stream takes for all of them is its floor.  One JSON line per configuration and
variant with the median and min-max over all rounds; --out also writes them to a file.  --once: one warm call of the trim
with the full bases behind it per configuration, twice, and the read probe, and nothing else (for a run under
`rocprofv3 --kernel-trace --stats`)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--bins", type=int, default=512)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated configuration names")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()
    from fastq_trim_rates import make_text
    from sickle_amd import capi
    ctx = capi.Context(device=0)
    L = capi.lib()
    configs = [("se_150", "se", False, [(10_000_000, 150, 150, 1)]),
               ("split_150_n", "pe_split", True, [(5_000_000, 150, 150, 2), (5_000_000, 150, 150, 3)]),
               ("se_mix", "se", False, [(4_000_000, 75, 301, 4)]),
               ("se_10k", "se", False, [(100_000, 10_000, 10_000, 5)])]
    lines = []
    for name, mode, trunc_n, specs in configs:
        if args.only and name not in args.only.split(","):
            continue
        texts = [make_text(torch, n, lo, hi, seed) for n, lo, hi, seed in specs]
        params = capi.make_params("sanger", 20, 50, False, trunc_n)
        T = sum(t.numel() for t in texts)
        nb = L.sk_trim_fastq_workspace_bytes(T, params.trunc_n)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        ptrs, sizes = [t.data_ptr() for t in texts], [t.numel() for t in texts]
        ctx.trim_fastq_device_async(params, ptrs, sizes, [capi.FastqOutput() for _ in range(3)], ws.data_ptr(), nb, mode=mode)
        counts = ctx.trim_fastq_device_finish(ws.data_ptr())
        bufs, outs = [], []
        for o in range(3):
            t = torch.empty(counts["bytes"][o] + 16, dtype=torch.uint8, device="cuda")
            bufs.append(t)
            outs.append(capi.FastqOutput(t.data_ptr(), counts["bytes"][o], None, counts["records"][o]))
        B, G = args.bins, capi.SK_FQ_BASES_GC_BINS
        bas = torch.zeros(capi.BASES_WORDS + 12 * B + 2 * G, dtype=torch.int64, device="cuda")
        at = lambda words: bas.data_ptr() + 8 * (capi.BASES_WORDS + words)
        full = capi.FastqBasesHists(at(0), at(6 * B), B, at(12 * B), at(12 * B + G))

        def call(bases, arrays=False):
            ctx.trim_fastq_device_async(params, ptrs, sizes, outs, ws.data_ptr(), nb, mode=mode)
            if bases:
                ctx.trim_fastq_bases_device_async(ws.data_ptr(), T, params.trunc_n, bas.data_ptr(), ptrs, sizes, mode=mode,
                                                  hists=full if arrays else None, reset=True)

        if args.once:
            for _ in range(2):
                call(True, True)
                ctx.trim_fastq_device_finish(ws.data_ptr())
            for p, n in zip(ptrs, sizes):
                ctx.probe_read_bandwidth(p, n)
            continue
        variants = [("trim", (False, False)), ("trim+bases", (True, False)), ("trim+bases+pos", (True, True))]
        for _, v in variants:  # warm-up
            call(*v)
            ctx.trim_fastq_device_finish(ws.data_ptr())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = {v: [] for v, _ in variants}
        for _ in range(args.rounds):
            for v, how in variants:
                for _ in range(args.iters):
                    e0.record()
                    call(*how)
                    e1.record()
                    ctx.trim_fastq_device_finish(ws.data_ptr())
                    ms[v].append(e0.elapsed_time(e1))
        got = capi.FastqBases.from_buffer_copy(bas.cpu().numpy()[:capi.BASES_WORDS].tobytes()).as_dict()
        # the texts' bytes through the read-stream probe
        stream_ms = sum(n / ctx.probe_read_bandwidth(p, n) / 1e6 for p, n in zip(ptrs, sizes))
        for v, _ in variants:
            x = sorted(ms[v])
            res = {"config": name, "variant": v, "mode": mode, "trunc_n": bool(trunc_n), "pos_bins": B, "reads": got["reads"],
                   "kept": got["kept"], "seq_bytes": sum(got["bases_in"]), "reads_n_in": got["reads_n_in"], "text_bytes": T,
                   "calls": len(x), "median_ms": round(x[len(x) // 2], 3), "min_ms": round(x[0], 3), "max_ms": round(x[-1], 3),
                   "read_stream_GBps": round(T / stream_ms / 1e6, 1), "text_at_stream_ms": round(stream_ms, 3)}
            print(json.dumps(res), flush=True)
            lines.append(res)
        del texts, ws, bufs
        torch.cuda.empty_cache()
    if args.out and lines:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))
    ctx.close()


if __name__ == "__main__":
    main()

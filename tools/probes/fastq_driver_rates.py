"""What the Python drivers of sickle_amd/capi.py cost around their calls, with every behind-call option on: trim_fastq,
trim_fastq_gz, trim_gz(text_capacity=..) and trim_fastq_stream(gz=True) on one interleaved text, mode "pe_interleaved",
order=(3, batch_len) with a batch_len that holds a pair, report, audit, bases, adapters and clip_adapters given (and rejects
where the driver takes it).

Wall time per call, the wait and the read-back included: on the small default text that is the drivers' own host work and
the launches, which is what a change to capi.py alone can move.  --other FILE loads a second capi.py (say the parent
commit's) over the same library, and the two alternate within the one job, `--turns` turns of `--iters` calls each after a
warm-up call; one JSON line per tree, turn and driver, then one per tree and driver with the median of the turns' medians
and their min to max.  --out also writes them to a file.

--once DRIVER runs that driver once and nothing else, on the tree --tree names (for a run under `rocprofv3
--kernel-trace`: the ordered kernel names and grids of two trees are compared line by line)."""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
ADAPTER = "AGATCGGAAGAGC"
DRIVERS = ("trim_fastq", "trim_fastq_gz", "trim_gz", "trim_fastq_stream")


def make_text(records, length, seed):
    """an interleaved text: quality falls off along the read, a third of the reads carry the adapter"""
    import numpy as np
    rng = np.random.default_rng(seed)
    out = []
    for r in range(records):
        seq = "".join("ACGT"[b] for b in rng.integers(0, 4, length))
        if r % 3 == 0:
            at = int(rng.integers(1, length))
            seq = (seq[:at] + ADAPTER + seq)[:length]
        qual = "".join(chr(33 + int(q)) for q in np.clip(38 - rng.integers(0, 30, length) * np.arange(length) // length, 2, 40))
        out.append("@r%d/%d\n%s\n+\n%s\n" % (r // 2, r % 2 + 1, seq, qual))
    return "".join(out).encode()


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from sickle_amd import capi
    mod.LIB_PATH = capi.LIB_PATH  # the same library under both
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=64)
    ap.add_argument("--length", type=int, default=12)
    ap.add_argument("--batch-len", type=int, default=64)
    ap.add_argument("--piece-bytes", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--other", default=None, help="a second capi.py to alternate with")
    ap.add_argument("--other-name", default="parent")
    ap.add_argument("--tree", default="new", help="--once: which tree runs (new, or --other-name)")
    ap.add_argument("--once", choices=DRIVERS, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()
    from sickle_amd import capi
    trees = {"new": capi}
    if args.other:
        trees[args.other_name] = load(args.other, "capi_other")
    text = make_text(args.records, args.length, 1)
    dev = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    order = (3, args.batch_len)
    side = dict(report=dict(len_bins=64, pos_bins=64), audit=True, bases=dict(pos_bins=64, gc=True),
                adapters=dict(seqs=[ADAPTER], pos_bins=64, overlap=True), clip_adapters=dict(seqs=[ADAPTER]))
    if args.once:
        trees = {args.tree: trees[args.tree]}
    ctxs = {name: mod.Context(device=0) for name, mod in trees.items()}
    image = next(iter(ctxs.values())).bgzf(dev)
    torch.cuda.synchronize()

    def run(name, driver):
        ctx, mod = ctxs[name], trees[name]
        params = mod.make_params("sanger", 20, 5)
        if driver == "trim_fastq":
            return ctx.trim_fastq(params, dev, mode="pe_interleaved", order=order, rejects="pairs", record_index=True,
                                  **dict(side, adapters=dict(side["adapters"], clip=True)))
        if driver == "trim_fastq_gz":
            return ctx.trim_fastq_gz(params, dev, mode="pe_interleaved", order=order, **side)
        if driver == "trim_gz":
            return ctx.trim_gz(params, image, mode="pe_interleaved", order=order, text_capacity=len(text) + 64, **side)
        st = ctx.trim_fastq_stream(params, text, mode="pe_interleaved", order=order, piece_bytes=args.piece_bytes, gz=True,
                                   rejects="pairs", **side)
        return list(st), st.counts, st.report

    if args.once:
        got = run(args.tree, args.once)
        torch.cuda.synchronize()
        print(json.dumps({k: got[1][k] for k in ("records_in", "records", "bytes")}))
        for c in ctxs.values():
            c.close()
        return
    for name in trees:
        for d in DRIVERS:
            run(name, d)
    median = lambda xs: sorted(xs)[len(xs) // 2]
    lines, turns = [], {}
    for turn in range(args.turns):
        for name in reversed(list(trees)):  # the other tree first, as parent, new, parent, new, ...
            for d in DRIVERS:
                ms = []
                for _ in range(args.iters):
                    t0 = time.perf_counter()
                    run(name, d)
                    ms.append(1e3 * (time.perf_counter() - t0))
                ms.sort()
                turns.setdefault((name, d), []).append(median(ms))
                lines.append({"probe": "driver_rates", "tree": name, "turn": turn, "driver": d, "text_bytes": len(text),
                              "records": args.records, "calls": len(ms), "median_ms": round(median(ms), 3),
                              "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3)})
                print(json.dumps(lines[-1]), flush=True)
    for (name, d), meds in turns.items():
        lines.append({"probe": "driver_rates", "tree": name, "driver": d, "text_bytes": len(text), "turns": len(meds),
                      "median_of_turns_ms": round(median(meds), 3), "turns_min_ms": round(min(meds), 3),
                      "turns_max_ms": round(max(meds), 3)})
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main()

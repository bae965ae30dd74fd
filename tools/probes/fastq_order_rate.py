"""What the reference's -a T batch order costs the trim of FASTQ text on the device: sk_trim_fastq_ordered_device_async at
T = 16 and batch_len = (bytes of the first text) / 8 against sk_trim_fastq_device_async, alternately, on the same text in
one process, for the four texts of tools/fastq_trim_rates.py.  HIP events around the enqueue of a whole call, median of
10 after 3 warm-ups each.  Prints one JSON line per text; --out also writes them to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

THREADS = 16


def run(ctx, capi, torch, name, texts, mode, trunc_n, iters):
    params = capi.make_params("sanger", 20, 50, False, trunc_n)
    ptrs, sizes = [t.data_ptr() for t in texts], [t.numel() for t in texts]
    T, batch_len = sum(sizes), max(20, sizes[0] // 8)
    order = capi.FastqOrder(THREADS, 0, batch_len, T // batch_len + 16, 0)
    nb = capi.lib().sk_trim_fastq_ordered_workspace_bytes(T, params.trunc_n, order.batch_capacity)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")  # the unordered call needs less: both use it in turn

    def ordered(outs):
        ctx.trim_fastq_ordered_device_async(params, ptrs, sizes, order, outs, ws.data_ptr(), nb, mode=mode)

    def plain(outs):
        ctx.trim_fastq_device_async(params, ptrs, sizes, outs, ws.data_ptr(), nb, mode=mode)

    calls = {"ordered": (ordered, ctx.trim_fastq_ordered_device_finish), "unordered": (plain, ctx.trim_fastq_device_finish)}
    none = [capi.FastqOutput() for _ in range(3)]
    counts, outs, bufs = {}, {}, []
    for k, (start, finish) in calls.items():
        start(none)
        counts[k] = finish(ws.data_ptr())
        outs[k] = []
        for o in range(3):
            t = torch.empty(counts[k]["bytes"][o] + 16, dtype=torch.uint8, device="cuda")
            bufs.append(t)
            outs[k].append(capi.FastqOutput(t.data_ptr(), counts[k]["bytes"][o], None, counts[k]["records"][o]))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = {k: [] for k in calls}
    for it in range(3 + iters):
        for k, (start, finish) in calls.items():
            e0.record()
            start(outs[k])
            e1.record()
            finish(ws.data_ptr())
            if it >= 3:
                ms[k].append(e0.elapsed_time(e1))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    oc = counts["ordered"]["order"]
    return {"config": name, "mode": mode, "trunc_n": bool(trunc_n), "text_bytes": T, "threads": THREADS, "batch_len": batch_len,
            "batches": oc["batches"], "units": oc["units"], "records_unbatched": oc["records_unbatched"],
            "written_bytes": {k: sum(c["bytes"]) for k, c in counts.items()},
            "median_ms": {k: round(v, 3) for k, v in med.items()}, "min_ms": {k: round(min(v), 3) for k, v in ms.items()},
            "ordered_over_unordered": round(med["ordered"] / med["unordered"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated configuration names")
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()
    from fastq_trim_rates import make_text
    from sickle_amd import capi
    ctx = capi.Context(device=0)
    configs = [("se_150", "se", False, [(10_000_000, 150, 150, 1)]),
               ("split_150_n", "pe_split", True, [(5_000_000, 150, 150, 2), (5_000_000, 150, 150, 3)]),
               ("se_mix", "se", False, [(4_000_000, 75, 301, 4)]),
               ("se_10k", "se", False, [(100_000, 10_000, 10_000, 5)])]
    lines = []
    for name, mode, trunc_n, specs in configs:
        if args.only and name not in args.only.split(","):
            continue
        texts = [make_text(torch, n, lo, hi, seed) for n, lo, hi, seed in specs]
        res = run(ctx, capi, torch, name, texts, mode, trunc_n, args.iters)
        print(json.dumps(res), flush=True)
        lines.append(res)
        del texts
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))
    ctx.close()


if __name__ == "__main__":
    main()

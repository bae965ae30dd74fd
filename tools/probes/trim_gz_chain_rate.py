"""What the one-pass Context.trim_gz(text_capacity=...) gains over the two-pass call on one MI355X: .fastq.gz image(s) in
device memory -> trimmed BGZF image(s) in device memory.

Clock: a HOST clock (time.perf_counter) around the whole call, which ends in its last finish, after a device
synchronisation before the start.  What the one-pass call saves is host waits and a count-only pass of each reader, which
device events around one call would hide.  Method: after `--warmup` (3) calls of each kind, `--iters` (10) rounds of
[two-pass, one-pass at the exact capacity, one-pass at 1.5 x it] in turn in one process on the same images; the median of
each.  The outputs of the three are compared once, byte for byte.
Inputs: the texts of tools/fastq_trim_rates.py's first two rows (10 M x 150 bp SK_TRIM_SE; 5 M pairs SK_TRIM_PE_SPLIT with
-n) as BGZF made by Context.bgzf, and 2 M x 150 bp as plain gzip from the host's zlib at level 1 (the same seeded text).
Prints one JSON line per (input, call); --out also writes them to a file."""
import argparse
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated input names")
    ap.add_argument("--scale", type=float, default=1.0, help="scales the read counts (for a quick look)")
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()
    from fastq_trim_rates import make_text
    from sickle_amd import capi
    ctx = capi.Context(device=0)
    n = lambda reads: max(1000, int(reads * args.scale))
    inputs = [("se_150_bgzf", "se", False, "bgzf", [(n(10_000_000), 1)]),
              ("split_150_n_bgzf", "pe_split", True, "bgzf", [(n(5_000_000), 2), (n(5_000_000), 3)]),
              ("se_150_2M_gzip", "se", False, "gzip", [(n(2_000_000), 1)])]
    lines = []
    for name, mode, trunc_n, kind, specs in inputs:
        if args.only and name not in args.only.split(","):
            continue
        params = capi.make_params("sanger", 20, 50, False, trunc_n)
        images, need = [], []
        for reads, seed in specs:
            text = make_text(torch, reads, 150, 150, seed)
            need.append(text.numel())
            if kind == "bgzf":
                images.append(ctx.bgzf(text).clone())
            else:
                z = zlib.compressobj(1, zlib.DEFLATED, 31)
                images.append(torch.frombuffer(bytearray(z.compress(text.cpu().numpy().tobytes()) + z.flush()),
                                               dtype=torch.uint8).cuda())
            del text
        torch.cuda.empty_cache()
        second = images[1] if len(images) > 1 else None
        calls = [("two_pass", {}), ("one_pass_exact", dict(text_capacity=list(need), kind=kind)),
                 ("one_pass_1.5x", dict(text_capacity=[b + b // 2 for b in need], kind=kind))]

        def run(kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got, counts = ctx.trim_gz(params, images[0], second, mode=mode, **kw)
            return (time.perf_counter() - t0) * 1e3, got, counts

        ref = None
        for what, kw in calls:  # the three give the same images
            _, got, counts = run(kw)
            if ref is None:
                ref = (got, counts)
            else:
                assert counts == ref[1], what
                assert all((g is None and r is None) or torch.equal(g, r) for g, r in zip(got, ref[0])), what
        gz_out = sum(g.numel() for g in ref[0] if g is not None)
        del got, ref
        for _ in range(max(args.warmup - 1, 0)):
            for what, kw in calls:
                run(kw)
        ms = {what: [] for what, _ in calls}
        for _ in range(args.iters):
            for what, kw in calls:
                ms[what].append(run(kw)[0])
        for what, kw in calls:
            res = {"input": name, "mode": mode, "trunc_n": bool(trunc_n), "kind": kind, "call": what,
                   "image_bytes": [z.numel() for z in images], "text_bytes": need,
                   "text_capacity": kw.get("text_capacity"), "records_in": counts["records_in"], "gz_bytes_out": gz_out,
                   "clock": "host, whole call", "iters": args.iters, "warmup": args.warmup,
                   "median_ms": round(median(ms[what]), 3), "min_ms": round(min(ms[what]), 3),
                   "vs_two_pass": round(median(ms[what]) / median(ms["two_pass"]), 3)}
            print(json.dumps(res), flush=True)
            lines.append(res)
        del images, second
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))
    ctx.close()


if __name__ == "__main__":
    main()

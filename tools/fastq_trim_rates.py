"""Rates of the trim of FASTQ text on the device (sk_trim_fastq_device_async, sickle_amd/csrc/sk_fastq.hip) on one MI355X.

Times the whole call (frame, check, pack, scan, emit) with HIP events after warm-up, on FASTQ text made on the device:
  se_150      10 M x 150 bp, SK_TRIM_SE
  split_150_n 5 M pairs x 150 bp, SK_TRIM_PE_SPLIT with -n
  se_mix      4 M reads of 75..301 bp, SK_TRIM_SE
  se_10k      100 k x 10 kb, SK_TRIM_SE
and reports bytes/s against the algorithmic bytes: text read + text written + packed qual (and seq with -n), the packed
bytes counted once written and once read.  Per-kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats`.  Prints one JSON line per configuration; --out also writes them to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_text(torch, n, lo, hi, seed, chunk=250_000):
    """n records "@r<9 digits>\\n<seq>\\n+\\n<qual>\\n" built on the device (mostly good qualities, low stretches)."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    parts = []
    for a in range(0, n, chunk):
        m = min(chunk, n - a)
        lens = torch.full((m,), hi, dtype=torch.int64, device="cuda") if lo == hi else \
            torch.randint(lo, hi + 1, (m,), generator=g, device="cuda")
        start = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
        start[1:] = torch.cumsum(12 + 2 * lens + 4, 0)  # name line, seq + '\\n', "+\\n", qual + '\\n'
        total = int(start[-1])
        pos = torch.arange(total, device="cuda")
        r = torch.searchsorted(start[1:], pos, right=True)
        off = pos - start[r]
        L = lens[r]
        rnd = torch.randint(0, 256, (total,), generator=g, device="cuda", dtype=torch.int32)
        qual = torch.where(rnd < 200, 60 + rnd % 15, 33 + rnd % 20)
        base = torch.tensor(list(b"ACGT"), dtype=torch.int32, device="cuda")[rnd % 4]
        digit = 48 + torch.div(r + a, 10 ** torch.clamp(10 - off, 0, 8), rounding_mode="floor") % 10
        out = torch.where(off == 0, 64, torch.where(off == 1, 114, digit))
        out = torch.where(off == 11, 10, out)
        out = torch.where((off >= 12) & (off < 12 + L), base, out)
        out = torch.where(off == 12 + L, 10, out)
        out = torch.where(off == 13 + L, 43, out)
        out = torch.where(off == 14 + L, 10, out)
        out = torch.where((off >= 15 + L) & (off < 15 + 2 * L), qual, out)
        out = torch.where(off == 15 + 2 * L, 10, out)
        parts.append(out.to(torch.uint8))
        del pos, r, off, L, rnd, qual, base, digit, out
    return torch.cat(parts)


def run(ctx, capi, torch, name, texts, mode, trunc_n, iters):
    params = capi.make_params("sanger", 20, 50, False, trunc_n)
    T = sum(t.numel() for t in texts)
    nb = capi.lib().sk_trim_fastq_workspace_bytes(T, params.trunc_n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ptrs, sizes = [t.data_ptr() for t in texts], [t.numel() for t in texts]
    ctx.trim_fastq_device_async(params, ptrs, sizes, [capi.FastqOutput() for _ in range(3)], ws.data_ptr(), nb, mode=mode)
    counts = ctx.trim_fastq_device_finish(ws.data_ptr())
    bufs, outs = [], []
    for o in range(3):
        B, R = counts["bytes"][o], counts["records"][o]
        t = torch.empty(B + 16, dtype=torch.uint8, device="cuda")
        bufs.append(t)
        outs.append(capi.FastqOutput(t.data_ptr(), B, None, R))
    for _ in range(3):
        ctx.trim_fastq_device_async(params, ptrs, sizes, outs, ws.data_ptr(), nb, mode=mode)
        ctx.trim_fastq_device_finish(ws.data_ptr())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(iters):
        e0.record()
        ctx.trim_fastq_device_async(params, ptrs, sizes, outs, ws.data_ptr(), nb, mode=mode)
        e1.record()
        ctx.trim_fastq_device_finish(ws.data_ptr())
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    med = ms[len(ms) // 2]
    written = sum(counts["bytes"])
    recs = counts["records_in"][0] + counts["records_in"][1]
    # packed qual = every framed record's qual line; the text is 12 + 2 L + 4 bytes per record here
    packed = (T - 16 * recs) // 2 * (2 if trunc_n else 1)
    alg = T + written + 2 * packed
    return {"config": name, "mode": mode, "trunc_n": bool(trunc_n), "records": recs, "text_bytes": T,
            "written_bytes": written, "packed_bytes": packed, "workspace_bytes": nb, "median_ms": round(med, 3),
            "min_ms": round(ms[0], 3), "alg_TBps": round(alg / (med * 1e-3) / 1e12, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated configuration names")
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()
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

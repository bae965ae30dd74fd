"""Rates of the device-side trim (sk_trim_device_async, sickle_amd/csrc/sk_trim.hip) on one MI355X.

Times the whole trim (four kernels) with HIP events after warm-up, on batches made and scanned on the device:
  se_150      10 M x 150 bp, SK_TRIM_SE with seq
  pe_150      the same reads as 5 M pairs, SK_TRIM_PE_SPLIT with seq
  se_mix      4 M reads of 75..301 bp (ragged), SK_TRIM_SE with seq
and reports bytes/s against the algorithmic bytes: kept bytes read + written (x 2 with seq), 8 B per output record
for offsets and 8 B for read_index, and 2 x 8 B of cuts per read.  The gather kernel's own time comes from a run
under `rocprofv3 --kernel-trace --stats` (sk_trim_gather_kernel); divide the same bytes minus the cuts and the
offsets/index writes by it.  Prints one JSON line per configuration; --out also writes them to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_batch(torch, n, lo, hi, seed):
    """qual / seq bytes on the device (mostly good qualities, some low stretches), ragged when lo < hi."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    if lo == hi:
        lens = None
        total = n * hi
    else:
        lens = torch.randint(lo, hi + 1, (n,), generator=g, device="cuda")
        total = int(lens.sum())
    r = torch.randint(0, 256, (total,), generator=g, device="cuda", dtype=torch.int32)
    qual = torch.where(r < 200, 60 + r % 15, 33 + r % 20).to(torch.uint8)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    seq = acgt[torch.randint(0, 4, (total,), generator=g, device="cuda")]
    offsets = None
    if lens is not None:
        offsets = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
        offsets[1:] = torch.cumsum(lens, 0)
    return qual, seq, offsets


def run(ctx, capi, torch, name, qual, seq, offsets, n, L, mode, iters):
    params = capi.make_params("sanger", 20, 50, False, False)
    cuts = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    kw = dict(offsets_ptr=offsets.data_ptr()) if offsets is not None else dict(stride=L, read_len=L)
    ctx.scan_device_async(params, qual.data_ptr(), cuts.data_ptr(), n, **kw)
    ctx.scan_device_finish()
    batch = dict(qual_ptr=qual.data_ptr(), seq_ptr=seq.data_ptr(), **kw)
    nb = capi.lib().sk_trim_workspace_bytes(n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    counts = ctx.trim_device(cuts.data_ptr(), n, [capi.TrimOutput() for _ in range(3)], ws.data_ptr(), nb, mode=mode,
                             **batch)
    bufs, outs = [], []
    for o in range(3):
        R, B = counts["records"][o], counts["bytes"][o]
        q = torch.empty(B + 16, dtype=torch.uint8, device="cuda")
        s = torch.empty(B + 16, dtype=torch.uint8, device="cuda")
        off = torch.empty(R + 1, dtype=torch.int64, device="cuda")
        idx = torch.empty(R + 1, dtype=torch.int64, device="cuda")
        bufs.append((q, s, off, idx))
        outs.append(capi.TrimOutput(q.data_ptr(), s.data_ptr(), off.data_ptr(), idx.data_ptr(), B, R))
    for _ in range(3):  # warm-up
        ctx.trim_device(cuts.data_ptr(), n, outs, ws.data_ptr(), nb, mode=mode, **batch)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        ctx.trim_device_async(cuts.data_ptr(), n, outs, ws.data_ptr(), nb, mode=mode, **batch)
    e1.record()
    got = ctx.trim_device_finish(ws.data_ptr())
    assert got == counts
    ms = e0.elapsed_time(e1) / iters
    R, B = sum(counts["records"]), sum(counts["bytes"])
    moved = 2 * B * 2  # kept bytes read + written, qual and seq
    alg = moved + 16 * R + 16 * n
    rec = {"config": name, "mode": mode, "n_reads": n, "records": R, "kept_bytes": B, "trim_ms": round(ms, 4),
           "algorithmic_bytes": alg, "trim_TBps": round(alg / (ms * 1e-3) / 1e12, 3),
           "gather_bytes": moved, "iters": iters}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()
    from sickle_amd import capi
    ctx = capi.Context(device=0, slots=2)
    recs = []
    qual, seq, _ = make_batch(torch, 10_000_000, 150, 150, 1)
    recs.append(run(ctx, capi, torch, "se_150", qual, seq, None, 10_000_000, 150, "se", args.iters))
    recs.append(run(ctx, capi, torch, "pe_150", qual, seq, None, 10_000_000, 150, "pe_split", args.iters))
    del qual, seq
    qual, seq, off = make_batch(torch, 4_000_000, 75, 301, 2)
    recs.append(run(ctx, capi, torch, "se_mix", qual, seq, off, 4_000_000, 0, "se", args.iters))
    for r in recs:
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in recs:
                f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()

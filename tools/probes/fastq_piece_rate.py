"""What trimming FASTQ text in pieces costs against the whole-text call, on the same text in one process, alternately:
  whole   sk_trim_fastq_device_async + finish on the whole text (the baseline: the parent commit's code path)
  pieces  the text cut into pieces of 64 MiB, 256 MiB and 1 GiB, every chunk copied into its piece's buffer beforehand, every
          carry and piece enqueued up front (a workspace and outputs of its own each), then every finish: one wait in effect
  stream  Context.trim_fastq_stream at the same piece sizes from the text in host memory (uploads each chunk, drains each
          piece's outputs to the host: two text buffers, two workspaces, two output sets)
A host clock around everything up to the last finish (the device is idle before and after: every variant ends in a stream
synchronisation), median of --iters after --warmup each.  The stream variant moves the whole text over the host link
twice per run, so it takes seconds: --stream-iters / --stream-warmup size it on their own.  Also records the device bytes
each variant allocates.  Prints one JSON line per text; --out appends them to a file."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROOM = 1 << 20
SIZES = (64 << 20, 256 << 20, 1 << 30)


class Pieces:
    """the buffers of one piece size: allocated once, the chunks copied in once"""

    def __init__(self, ctx, capi, torch, params, texts, mode, size):
        self.ctx, self.capi, self.params, self.mode = ctx, capi, params, mode
        L = capi.lib()
        self.n_in, self.bytes = len(texts), 0
        self.n = max(1, max(-(-t.numel() // size) for t in texts))
        used = {"se": (0,), "pe_split": (0, 1, 2), "pe_interleaved": (0, 2)}[mode]

        def alloc(n):
            self.bytes += n
            return torch.empty(n, dtype=torch.uint8, device="cuda")
        self.text, self.chunk, self.ws, self.out, self.keep = [], [], [], [], []
        for k in range(self.n):
            row, lens = [], []
            for t in texts:
                c = t[k * size:(k + 1) * size]
                b = alloc(ROOM + c.numel() + 16)
                b[ROOM:ROOM + c.numel()] = c
                row.append(b)
                lens.append(c.numel())
            self.text.append(row)
            self.chunk.append(lens)
            T = sum(ROOM + n for n in lens)
            nb = L.sk_trim_fastq_workspace_bytes(T, params.trunc_n)
            self.ws.append((alloc(nb), nb))
            held = [alloc(T + 16) if o in used else None for o in range(3)]
            self.keep.append(held)
            self.out.append([capi.FastqOutput(t.data_ptr(), T + 2, None, 0) if t is not None else capi.FastqOutput() for t in held])
        self.words = torch.zeros((self.n, self.n_in, 4), dtype=torch.int64, device="cuda")

    def run(self):
        ctx, n_in = self.ctx, self.n_in
        w = lambda k, i: self.words.data_ptr() + 32 * (k * n_in + i)
        for k in range(self.n):
            for i in range(n_in):
                ctx.fastq_carry_device_async(self.ws[k - 1][0].data_ptr() if k else None, i,
                                             self.text[k - 1][i].data_ptr() if k else None,
                                             ROOM + self.chunk[k - 1][i] if k else 0, self.text[k][i].data_ptr(), ROOM, w(k, i),
                                             chunk_bytes=self.chunk[k][i], prev_words_ptr=w(k - 1, i) if k else None,
                                             other_prev_words_ptr=w(k - 1, 1 - i) if k and n_in == 2 else None)
            ctx.trim_fastq_piece_device_async(self.params, [t.data_ptr() for t in self.text[k]],
                                              [ROOM + n for n in self.chunk[k]], self.out[k], self.ws[k][0].data_ptr(),
                                              self.ws[k][1], bytes_dev_ptrs=[w(k, i) + 8 for i in range(n_in)],
                                              valid_dev_ptrs=[w(k, i) + 16 for i in range(n_in)],
                                              start_dev_ptrs=[w(k, i) for i in range(n_in)], more=k + 1 < self.n, mode=self.mode)
        total = [0, 0, 0]
        for k in range(self.n):
            c = ctx.trim_fastq_piece_device_finish(self.ws[k][0].data_ptr())
            total = [a + b for a, b in zip(total, c["bytes"])]
        return total


def median(v):
    return sorted(v)[len(v) // 2]


def run(ctx, capi, torch, name, texts, mode, trunc_n, args):
    params = capi.make_params("sanger", 20, 50, False, trunc_n)
    ptrs, sizes = [t.data_ptr() for t in texts], [t.numel() for t in texts]
    T = sum(sizes)
    nb = capi.lib().sk_trim_fastq_workspace_bytes(T, params.trunc_n)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ctx.trim_fastq_device_async(params, ptrs, sizes, [capi.FastqOutput() for _ in range(3)], ws.data_ptr(), nb, mode=mode)
    counts = ctx.trim_fastq_device_finish(ws.data_ptr())
    bufs = [torch.empty(counts["bytes"][o] + 16, dtype=torch.uint8, device="cuda") for o in range(3)]
    outs = [capi.FastqOutput(bufs[o].data_ptr(), counts["bytes"][o], None, 0) for o in range(3)]

    def whole():
        ctx.trim_fastq_device_async(params, ptrs, sizes, outs, ws.data_ptr(), nb, mode=mode)
        return ctx.trim_fastq_device_finish(ws.data_ptr())["bytes"]

    variants, p = {"whole": whole}, None
    device_bytes = {"whole": nb + sum(b.numel() for b in bufs)}
    for size in SIZES:
        if size >= 2 * max(sizes):
            continue
        p = Pieces(ctx, capi, torch, params, texts, mode, size)
        variants["pieces_%dMiB" % (size >> 20)] = p.run
        device_bytes["pieces_%dMiB" % (size >> 20)] = p.bytes
    ms = {k: [] for k in variants}
    note = lambda *a: print(*a, file=sys.stderr, flush=True)
    note(name, "variants", list(variants))
    for it in range(args.warmup + args.iters):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = fn()
            dt = 1e3 * (time.perf_counter() - t0)
            assert list(got) == counts["bytes"], (k, got, counts["bytes"])
            if it >= args.warmup:
                ms[k].append(dt)
    res = {"config": name, "mode": mode, "trunc_n": bool(trunc_n), "text_bytes": T, "written_bytes": sum(counts["bytes"]),
           "iters": args.iters, "room": ROOM, "median_ms": {k: round(median(v), 3) for k, v in ms.items()},
           "min_ms": {k: round(min(v), 3) for k, v in ms.items()}, "device_bytes": device_bytes}
    del variants, ws, bufs
    p = None
    torch.cuda.empty_cache()
    if args.stream_iters:
        host = [t.cpu().numpy() for t in texts]
        sm, sb = {}, {}
        for size in SIZES:
            if size >= 2 * max(sizes):
                continue
            key, v = "stream_%dMiB" % (size >> 20), []
            for it in range(args.stream_warmup + args.stream_iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st = ctx.trim_fastq_stream(params, host[0], host[1] if len(host) > 1 else None, mode=mode, piece_bytes=size,
                                           room=ROOM)
                got = [0, 0, 0]
                for part in st:
                    got = [a + (0 if b is None else len(b)) for a, b in zip(got, part)]
                dt = 1e3 * (time.perf_counter() - t0)
                assert got == counts["bytes"], (key, got)
                if it >= args.stream_warmup:
                    v.append(dt)
                sb[key] = st.device_bytes
                note(name, key, "run", it, "%.0f ms" % dt)
                del st
                torch.cuda.empty_cache()
            sm[key] = v
        res["stream_iters"] = args.stream_iters
        res["median_ms"].update({k: round(median(v), 3) for k, v in sm.items()})
        res["min_ms"].update({k: round(min(v), 3) for k, v in sm.items()})
        res["device_bytes"].update(sb)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--stream-iters", type=int, default=10)
    ap.add_argument("--stream-warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated configuration names")
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()
    from fastq_trim_rates import make_text
    from sickle_amd import capi
    ctx = capi.Context(device=0)
    configs = [("se_150", "se", False, [(10_000_000, 150, 150, 1)]),
               ("split_150_n", "pe_split", True, [(5_000_000, 150, 150, 2), (5_000_000, 150, 150, 3)])]
    for name, mode, trunc_n, specs in configs:
        if args.only and name not in args.only.split(","):
            continue
        texts = [make_text(torch, n, lo, hi, seed) for n, lo, hi, seed in specs]
        res = run(ctx, capi, torch, name, texts, mode, trunc_n, args)
        print(json.dumps(res), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(res) + "\n")
        del texts
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()

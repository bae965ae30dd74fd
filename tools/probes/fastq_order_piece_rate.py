"""What the reference's -a T order costs when FASTQ text is trimmed in pieces, on the same text, pieces and buffers in one
process, alternately:
  pieces   sk_trim_fastq_piece_device_async: read order (the baseline: the launches of the unordered piece stream)
  ordered  sk_trim_fastq_ordered_piece_device_async at T = 16: two states alternate, the table sized as the driver sizes it
Every chunk is copied into its piece's buffer beforehand; a run enqueues every carry and piece up front and is timed with
HIP events around that on the stream (the finishes come after the second event), --warmup runs, then the median of
--iters.  Two settings on the 10 M x 150 bp text of DESIGN 4.7: pieces of 256 MiB with batch_len = piece_bytes / 8, and the
reference's own budget for the file (tests/fastq_util.reference_batch_len) with pieces of 1 GiB, which hold a batch.
Prints one JSON line per setting; --out appends them to a file.  The chain kernel's own time comes from a separate run
under rocprofv3 --kernel-trace --stats (--iters 2 --warmup 1 is enough for that)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

THREADS = 16


class Pieces:
    """the buffers of one setting: allocated once, the chunks copied in once, shared by both variants"""

    def __init__(self, ctx, capi, torch, params, text, size, room, batch_len):
        self.ctx, self.capi, self.params, self.room = ctx, capi, params, room
        L = capi.lib()
        self.n = max(1, -(-text.numel() // size))
        self.capacity = (room + size) // batch_len + 16
        self.order = capi.FastqOrder(THREADS, 0, batch_len, self.capacity, 0)
        self.bytes = 0

        def alloc(n):
            self.bytes += n
            return torch.empty(n, dtype=torch.uint8, device="cuda")
        self.text, self.chunk, self.ws, self.out, self.keep = [], [], [], [], []
        for k in range(self.n):
            c = text[k * size:(k + 1) * size]
            b = alloc(room + c.numel() + 16)
            b[room:room + c.numel()] = c
            self.text.append(b)
            self.chunk.append(c.numel())
            T = room + c.numel()
            nb = L.sk_trim_fastq_ordered_piece_workspace_bytes(T, params.trunc_n, self.capacity)  # holds the unordered call's too
            self.ws.append((alloc(nb), nb, L.sk_trim_fastq_workspace_bytes(T, params.trunc_n)))
            held = alloc(T + 16)
            self.keep.append(held)
            self.out.append([capi.FastqOutput(held.data_ptr(), T + 2, None, 0), capi.FastqOutput(), capi.FastqOutput()])
        self.words = torch.zeros((self.n, 4), dtype=torch.int64, device="cuda")
        self.states = torch.zeros((2, 8), dtype=torch.int64, device="cuda")

    def enqueue(self, ordered):
        ctx, room = self.ctx, self.room
        w = lambda k: self.words.data_ptr() + 32 * k
        if ordered:
            self.states.zero_()
        for k in range(self.n):
            ctx.fastq_carry_device_async(self.ws[k - 1][0].data_ptr() if k else None, 0, self.text[k - 1].data_ptr() if k else None,
                                         room + self.chunk[k - 1] if k else 0, self.text[k].data_ptr(), room, w(k),
                                         chunk_bytes=self.chunk[k], prev_words_ptr=w(k - 1) if k else None)
            words = dict(bytes_dev_ptrs=[w(k) + 8], valid_dev_ptrs=[w(k) + 16], start_dev_ptrs=[w(k)], more=k + 1 < self.n,
                         mode="se")
            if ordered:
                ctx.trim_fastq_ordered_piece_device_async(self.params, [self.text[k].data_ptr()], [room + self.chunk[k]],
                                                          self.order, self.states[k & 1].data_ptr(),
                                                          self.states[(k + 1) & 1].data_ptr(), self.out[k],
                                                          self.ws[k][0].data_ptr(), self.ws[k][1], **words)
            else:
                ctx.trim_fastq_piece_device_async(self.params, [self.text[k].data_ptr()], [room + self.chunk[k]], self.out[k],
                                                  self.ws[k][0].data_ptr(), self.ws[k][2], **words)

    def finish(self, ordered):
        """-> (bytes written, batches, pieces whose table was full)"""
        total = batches = full = 0
        for k in range(self.n):
            if ordered:
                c = self.ctx.trim_fastq_ordered_piece_device_finish(self.ws[k][0].data_ptr())
                batches += c["order"]["batches"]
                full += c["order_piece"]["table_full"]
            else:
                c = self.ctx.trim_fastq_piece_device_finish(self.ws[k][0].data_ptr())
            assert c["piece"]["ok"] == 1
            total += c["bytes"][0]
        return total, batches, full


def median(v):
    return sorted(v)[len(v) // 2]


def run(ctx, capi, torch, name, text, size, room, batch_len, args):
    params = capi.make_params("sanger", 20, 50, False, False)
    p = Pieces(ctx, capi, torch, params, text, size, room, batch_len)
    ms, seen = {"pieces": [], "ordered": []}, {}
    for it in range(args.warmup + args.iters):
        for key in ("pieces", "ordered"):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            p.enqueue(key == "ordered")
            b.record()
            seen[key] = p.finish(key == "ordered")
            b.synchronize()
            if it >= args.warmup:
                ms[key].append(a.elapsed_time(b))
    # SE: every complete record lies in a batch, so both variants write the same bytes (in another order)
    assert seen["pieces"][0] == seen["ordered"][0] and seen["ordered"][2] == 0, seen
    med = {k: round(median(v), 3) for k, v in ms.items()}
    return {"config": name, "text_bytes": text.numel(), "piece_bytes": size, "room": room, "pieces": p.n, "threads": THREADS,
            "batch_len": batch_len, "batch_capacity": p.capacity, "batches": seen["ordered"][1], "written_bytes": seen["ordered"][0],
            "iters": args.iters, "warmup": args.warmup, "median_ms": med, "min_ms": {k: round(min(v), 3) for k, v in ms.items()},
            "ordered_over_pieces": round(med["ordered"] / med["pieces"], 4), "device_bytes": p.bytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated setting names")
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()
    import fastq_util as fu
    from fastq_trim_rates import make_text
    from sickle_amd import capi
    ctx = capi.Context(device=0)
    text = make_text(torch, args.reads, 150, 150, 1)
    small = 256 << 20
    settings = [("piece_256MiB_budget_eighth", small, 64 << 20, small // 8),
                ("piece_1GiB_reference_budget", 1 << 30, 1 << 29, fu.reference_batch_len(text.numel()))]
    for name, size, room, batch_len in settings:
        if args.only and name not in args.only.split(","):
            continue
        res = run(ctx, capi, torch, name, text, size, room, batch_len, args)
        print(json.dumps(res), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(res) + "\n")
        torch.cuda.empty_cache()
    ctx.close()


if __name__ == "__main__":
    main()

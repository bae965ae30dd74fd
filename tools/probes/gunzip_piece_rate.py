"""probe: what plain gzip read in pieces (sk_gzip_inflate_piece_device_async, sickle_amd/csrc/sk_gunzip_piece.hip) costs over
the whole-image call (sk_gzip_inflate_device_async) on one MI355X.

On the `gzip -6` image of the 10 M x 150 bp FASTQ text of tools/probes/gunzip_rate.py (--text-mb cuts the text when the
host compression is not to take minutes):
  whole    sk_gzip_inflate_device_async on the image
  pieces   windows of 16, 64 and 256 MiB of the image, from the zero state to the stream's end, every piece with a
           workspace, a text buffer and a state of its own and all of them enqueued before anything is waited for
The variants alternate in one process; HIP events around the enqueue, which a synchronise ends; median of --iters after 3
warm-ups.  Afterwards every piece is finished once: the text lengths add up to the text's, every piece's text is the
text's bytes at its offset, and the last piece is done.  One JSON line per variant; --out writes them to a file
(profiles/gunzip/gunzip_piece_rates.jsonl).

The split of the stages comes from a run of its own under the profiler, never together with the timing above:
  rocprofv3 --kernel-trace --stats -d profiles/gunzip/trace_piece -- python tools/probes/gunzip_piece_rate.py --iters 1
(the sk_gunzip_piece_*_kernel rows of the kernel statistics are the ten stages)."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, HERE)

RATIO = 8  # text capacity of a piece, in windows: FASTQ at level 6 stays well below


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--text-mb", type=int, default=0, help="cut the text to this many MB (0: the whole text)")
    ap.add_argument("--windows-mib", default="16,64,256")
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()
    from fastq_trim_rates import make_text
    from gunzip_rate import gzip6
    from sickle_amd import capi
    ctx = capi.Context(device=0)
    L = capi.lib()
    text = make_text(torch, 10_000_000, 150, 150, 1)
    if args.text_mb:
        text = text[:args.text_mb * 1_000_000].clone()
    t0 = time.perf_counter()
    blob = gzip6(text.cpu().numpy().tobytes())
    base = {"config": "se_150", "text_bytes": text.numel(), "image_bytes": len(blob), "gzip6_seconds": round(time.perf_counter() - t0, 1)}
    image = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    n, T = image.numel(), text.numel()
    variants = []

    wsb = L.sk_gzip_inflate_workspace_bytes(n, T)
    ws, out = torch.empty(wsb, dtype=torch.uint8, device="cuda"), torch.empty(max(T, 16), dtype=torch.uint8, device="cuda")

    def check_whole():
        counts = ctx.gzip_inflate_device_finish(ws.data_ptr())
        assert counts["bytes_out"] == T and bool(torch.equal(out[:T], text))
        return {"pieces": 1, "stretches_used": counts["stretches_used"]}
    variants.append(({"variant": "whole", "device_bytes": wsb + max(T, 16)},
                     lambda: ctx.gzip_inflate_device_async(image.data_ptr(), n, out.data_ptr(), T, ws.data_ptr(), wsb), check_whole))

    for mib in (int(x) for x in args.windows_mib.split(",")):
        window, cap = mib << 20, RATIO * (mib << 20)
        P = -(-n // window)
        P += 2 + P // 20  # a piece ends at its window's last block boundary: a few more than the image's windows
        pwsb = L.sk_gzip_inflate_piece_workspace_bytes(window, cap)
        pws = [torch.empty(pwsb, dtype=torch.uint8, device="cuda") for _ in range(P)]
        pout = [torch.empty(cap, dtype=torch.uint8, device="cuda") for _ in range(P)]
        states = torch.zeros((P + 1, capi.SK_GZIP_PIECE_STATE_BYTES), dtype=torch.uint8, device="cuda")

        def enqueue(window=window, cap=cap, P=P, pwsb=pwsb, pws=pws, pout=pout, states=states):
            for k in range(P):
                ctx.gzip_inflate_piece_device_async(image.data_ptr(), n, states[k].data_ptr(), states[k + 1].data_ptr(),
                                                    pout[k].data_ptr(), cap, pws[k].data_ptr(), pwsb, window)

        def check(P=P, pws=pws, pout=pout):
            at, used, done = 0, 0, 0
            for k in range(P):
                counts = ctx.gzip_inflate_piece_device_finish(pws[k].data_ptr())
                b = counts["bytes_out"]
                assert bool(torch.equal(pout[k][:b], text[at:at + b])), k
                at, used, done = at + b, used + (b > 0), counts["done"]
            assert at == T and done == 1, (at, T, done)
            return {"pieces": used, "pieces_enqueued": P}
        variants.append(({"variant": "pieces", "window_mib": mib, "device_bytes": P * (pwsb + cap) + states.numel()}, enqueue, check))

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = [[] for _ in variants]
    for it in range(3 + args.iters):
        for v, (_, enqueue, _) in enumerate(variants):
            e0.record()
            enqueue()
            e1.record()
            torch.cuda.synchronize()
            if it >= 3:
                ms[v].append(e0.elapsed_time(e1))
    lines = []
    for (res, enqueue, check), m in zip(variants, ms):
        m.sort()
        res = dict(base, **res, **check(), median_ms=round(m[len(m) // 2], 3), min_ms=round(m[0], 3),
                   GBps_text=round(T / m[len(m) // 2] / 1e6, 2))
        res["over_whole"] = round(res["median_ms"] / lines[0]["median_ms"], 3) if lines else 1.0
        print(json.dumps(res), flush=True)
        lines.append(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))
    ctx.close()


if __name__ == "__main__":
    main()

"""probe: rates of BGZF read on the device (sk_bgzf_inflate_device_async, sickle_amd/csrc/sk_inflate.hip) on one MI355X.

On the FASTQ texts of tools/probes/bgzf_device_rate.py (made on the device), each compressed by sk_bgzf_device_async, per
configuration, HIP-event times around the enqueue, median of --iters after 3 warm-ups:
  inflate   sk_bgzf_inflate_device_async on the image: GB/s of text out and of image in
  count     the same call with out = NULL (framing and scan only)
  bgzf      sk_bgzf_device_async on the same text, the writer's rate, in the same process
  host      zlib on the first --baseline-mb MB of the same image, one member per task on 16 threads (zlib releases the
            interpreter lock), wall clock, median of 4 after one warm-up, between the device measurements
Per-kernel times come from a separate run under `rocprofv3 --kernel-trace --stats`.  One JSON line per configuration."""
import argparse
import json
import os
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tools", "probes"))


def run_host(image, mb, threads=16):
    blob = image[:mb * 1_000_000].cpu().numpy().tobytes()
    view, spans, at = memoryview(blob), [], 0
    while at + 18 <= len(blob):
        size = blob[at + 16] + (blob[at + 17] << 8) + 1
        if at + size > len(blob):
            break
        spans.append((at + 18, at + size - 8))
        at += size
    chunks = [spans[k::threads * 8] for k in range(threads * 8)]
    work = lambda part: sum(len(zlib.decompress(view[a:b], -15)) for a, b in part)
    secs, text = [], 0
    with ThreadPoolExecutor(threads) as pool:
        for _ in range(5):
            t0 = time.perf_counter()
            text = sum(pool.map(work, chunks))
            secs.append(time.perf_counter() - t0)
    med = sorted(secs[1:])[2]
    return {"host_image_bytes": at, "host_text_bytes": text, "host_threads": threads, "host_median_ms": round(med * 1e3, 3),
            "host_GBps_text": round(text / med / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated configuration names")
    ap.add_argument("--baseline", action="store_true", help="also time zlib on 16 host threads on the same image")
    ap.add_argument("--baseline-mb", type=int, default=480)
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()
    from bgzf_device_rate import run_bgzf, timed
    from fastq_trim_rates import make_text
    from sickle_amd import capi
    ctx = capi.Context(device=0)
    L = capi.lib()
    configs = [("se_150", [(10_000_000, 150, 150, 1)]),
               ("split_150_n", [(5_000_000, 150, 150, 2), (5_000_000, 150, 150, 3)]),
               ("se_mix", [(4_000_000, 75, 301, 4)]),
               ("se_10k", [(100_000, 10_000, 10_000, 5)])]
    lines = []
    for name, specs in configs:
        if args.only and name not in args.only.split(","):
            continue
        texts = [make_text(torch, n, lo, hi, seed) for n, lo, hi, seed in specs]
        text = texts[0] if len(texts) == 1 else torch.cat(texts)
        del texts
        res = {"config": name, "text_bytes": text.numel()}
        res.update(run_bgzf(ctx, capi, torch, text, args.iters))
        image = ctx.bgzf(text).clone()
        n, T = image.numel(), text.numel()
        wsb = L.sk_bgzf_inflate_workspace_bytes(n)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        out = torch.empty(T, dtype=torch.uint8, device="cuda")
        counts = {}
        fin = lambda: counts.update(ctx.bgzf_inflate_device_finish(ws.data_ptr()))
        med, lo = timed(torch, args.iters, lambda: ctx.bgzf_inflate_device_async(image.data_ptr(), n, out.data_ptr(), T, ws.data_ptr(), wsb), fin)
        assert counts["bytes_out"] == T and bool(torch.equal(out, text))
        res.update({"image_bytes": n, "members": counts["members"], "inflate_median_ms": round(med, 3), "inflate_min_ms": round(lo, 3),
                    "inflate_GBps_text": round(T / med / 1e6, 2), "inflate_GBps_image": round(n / med / 1e6, 2),
                    "inflate_workspace_bytes": wsb})
        if args.baseline:
            res.update(run_host(image, args.baseline_mb))
        med, lo = timed(torch, args.iters, lambda: ctx.bgzf_inflate_device_async(image.data_ptr(), n, None, 0, ws.data_ptr(), wsb), fin)
        res.update({"count_median_ms": round(med, 3), "count_min_ms": round(lo, 3)})
        print(json.dumps(res), flush=True)
        lines.append(res)
        del text, image, ws, out
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))
    ctx.close()


if __name__ == "__main__":
    main()

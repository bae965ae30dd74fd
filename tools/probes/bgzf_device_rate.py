"""probe: rates of BGZF on the device (sk_bgzf_device_async, sickle_amd/csrc/sk_bgzf.hip) on one MI355X.

On the FASTQ texts of tools/fastq_trim_rates.py (made on the device), per configuration, HIP-event times, median of
--iters after 3 warm-ups:
  bgzf      sk_bgzf_device_async on the untrimmed text (all inputs back to back): GB/s of text in
  chain     sk_trim_fastq_device_async + one sk_bgzf_device_async per output, enqueued without a wait in between
            (what Context.trim_fastq_gz does): GB/s of input text
  host      with --baseline: sk_bgzf_deflate (host pointers, pinned; copies both ways and waits) on the first
            --baseline-mb MB of the same text, wall clock, run between the two above on the same box
  --search  instead of all the above: the call without a flag and the call with SK_BGZF_SEARCH in turn on the same text,
            workspace and stream, one of each per iteration, so that both see the same state of the machine: their times,
            the spread of the no-flag call (it is the yardstick: the same kernel as before the search existed), the ratio
            of the medians and the image / text ratio of each
Per-kernel times come from a separate run under `rocprofv3 --kernel-trace --stats`.  One JSON line per configuration."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(torch, iters, enqueue, finish):
    for _ in range(3):
        enqueue()
        finish()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(iters):
        e0.record()
        enqueue()
        e1.record()
        finish()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


def run_bgzf(ctx, capi, torch, text, iters):
    L = capi.lib()
    n = text.numel()
    cap, wsb = L.sk_bgzf_bound(n, capi.SK_BGZF_EOF), L.sk_bgzf_workspace_bytes(n)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    counts = {}
    med, lo = timed(torch, iters, lambda: ctx.bgzf_device_async(text.data_ptr(), n, out.data_ptr(), cap, ws.data_ptr(), wsb),
                    lambda: counts.update(ctx.bgzf_device_finish(ws.data_ptr())))
    return {"bgzf_median_ms": round(med, 3), "bgzf_min_ms": round(lo, 3), "bgzf_GBps": round(n / med / 1e6, 2),
            "bgzf_blocks": counts["blocks"], "bgzf_stored": counts["stored_blocks"], "bgzf_ratio": round(counts["bytes_out"] / n, 4),
            "bgzf_workspace_bytes": wsb}


def run_search(ctx, capi, torch, text, iters):
    L = capi.lib()
    n = text.numel()
    cap, wsb = L.sk_bgzf_bound(n, capi.SK_BGZF_EOF), L.sk_bgzf_workspace_bytes_flags(n, capi.SK_BGZF_SEARCH)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms, counts = {False: [], True: []}, {}

    def once(search, keep):
        e0.record()
        ctx.bgzf_device_async(text.data_ptr(), n, out.data_ptr(), cap, ws.data_ptr(), wsb, search=search)
        e1.record()
        counts[search] = ctx.bgzf_device_finish(ws.data_ptr())
        if keep:
            ms[search].append(e0.elapsed_time(e1))

    for i in range(3 + iters):
        once(False, i >= 3)
        once(True, i >= 3)
    res = {"search_workspace_bytes": wsb}
    for search, key in ((False, "noflag"), (True, "search")):
        t = sorted(ms[search])
        med = t[len(t) // 2]
        res.update({key + "_median_ms": round(med, 3), key + "_min_ms": round(t[0], 3), key + "_max_ms": round(t[-1], 3),
                    key + "_GBps": round(n / med / 1e6, 2), key + "_ratio": round(counts[search]["bytes_out"] / n, 4),
                    key + "_stored": counts[search]["stored_blocks"]})
    res["search_over_noflag"] = round(res["search_median_ms"] / res["noflag_median_ms"], 3)
    return res


def run_chain(ctx, capi, torch, texts, mode, trunc_n, iters):
    L = capi.lib()
    params = capi.make_params("sanger", 20, 50, False, trunc_n)
    ptrs, sizes = [t.data_ptr() for t in texts], [t.numel() for t in texts]
    T = sum(sizes)
    wsb = L.sk_trim_fastq_workspace_bytes(T, params.trunc_n)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    used = {"se": (0,), "pe_split": (0, 1, 2), "pe_interleaved": (0, 2)}[mode]
    cap = T + 2
    bound, zwsb = L.sk_bgzf_bound(cap, capi.SK_BGZF_EOF), L.sk_bgzf_workspace_bytes(cap)
    outs, bufs = [capi.FastqOutput() for _ in range(3)], {}
    for o in used:
        bufs[o] = (torch.empty(cap, dtype=torch.uint8, device="cuda"), torch.empty(bound, dtype=torch.uint8, device="cuda"),
                   torch.empty(zwsb, dtype=torch.uint8, device="cuda"))
        outs[o] = capi.FastqOutput(bufs[o][0].data_ptr(), cap, None, 0)
    sizes_out = {}

    def enqueue():
        ctx.trim_fastq_device_async(params, ptrs, sizes, outs, ws.data_ptr(), wsb, mode=mode)
        for o in used:
            nbytes, written = ctx.trim_fastq_output_words(ws.data_ptr(), o)
            ctx.bgzf_device_async(bufs[o][0].data_ptr(), cap, bufs[o][1].data_ptr(), bound, bufs[o][2].data_ptr(), zwsb,
                                  bytes_dev_ptr=nbytes, valid_dev_ptr=written)

    def finish():
        for o in used:
            sizes_out[o] = ctx.bgzf_device_finish(bufs[o][2].data_ptr())
        ctx.trim_fastq_device_finish(ws.data_ptr())

    med, lo = timed(torch, iters, enqueue, finish)
    return {"chain_median_ms": round(med, 3), "chain_min_ms": round(lo, 3), "chain_GBps_in": round(T / med / 1e6, 2),
            "chain_trimmed_bytes": sum(c["bytes_in"] for c in sizes_out.values()),
            "chain_gz_bytes": sum(c["bytes_out"] for c in sizes_out.values())}


def run_host(capi, torch, text, mb):
    import numpy as np
    n = min(text.numel(), mb * 1_000_000)
    n_blocks = (n + capi.BGZF_INPUT - 1) // capi.BGZF_INPUT
    host = torch.zeros(n_blocks * capi.BGZF_INPUT, dtype=torch.uint8).pin_memory()
    host[:n] = text[:n].cpu()
    sizes = np.array([min(capi.BGZF_INPUT, n - b * capi.BGZF_INPUT) for b in range(n_blocks)], dtype=np.uint32)
    out = torch.zeros(n_blocks * capi.BGZF_SLOT, dtype=torch.uint8).pin_memory()
    out_sizes = np.zeros(n_blocks, dtype=np.uint32)
    L = capi.lib()
    secs = []
    for _ in range(5):
        t0 = time.perf_counter()
        rc = L.sk_bgzf_deflate(0, host.data_ptr(), sizes.ctypes.data, n_blocks, out.data_ptr(), out_sizes.ctypes.data)
        secs.append(time.perf_counter() - t0)
        assert rc == 0, L.sk_bgzf_last_error()
    secs = sorted(secs[1:])
    return {"host_bytes": n, "host_median_ms": round(secs[len(secs) // 2] * 1e3, 3), "host_GBps": round(n / secs[len(secs) // 2] / 1e9, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated configuration names")
    ap.add_argument("--baseline", action="store_true", help="also time the host-pointer sk_bgzf_deflate on the same text")
    ap.add_argument("--baseline-mb", type=int, default=480)
    ap.add_argument("--no-chain", action="store_true")
    ap.add_argument("--search", action="store_true", help="the no-flag call and the SK_BGZF_SEARCH call in turn, nothing else")
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
        whole = texts[0] if len(texts) == 1 else torch.cat(texts)
        res = {"config": name, "mode": mode, "trunc_n": bool(trunc_n), "text_bytes": whole.numel()}
        if args.search:
            res.update(run_search(ctx, capi, torch, whole, args.iters))
            print(json.dumps(res), flush=True)
            lines.append(res)
            del whole, texts
            torch.cuda.empty_cache()
            continue
        res.update(run_bgzf(ctx, capi, torch, whole, args.iters))
        if args.baseline:
            res.update(run_host(capi, torch, whole, args.baseline_mb))
        del whole
        torch.cuda.empty_cache()
        if not args.no_chain:
            res.update(run_chain(ctx, capi, torch, texts, mode, trunc_n, args.iters))
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

"""probe: rates of plain gzip read on the device (sk_gzip_inflate_device_async, sickle_amd/csrc/sk_gunzip.hip) on one MI355X.

On the FASTQ texts of tools/probes/bgzf_device_rate.py (made on the device), each compressed on the host as `gzip -6` does
(one member, zlib level 6; --text-mb cuts the text when the host compression is not to take minutes), per configuration,
HIP-event times around the enqueue, median of --iters after 3 warm-ups:
  inflate   sk_gzip_inflate_device_async on the image: GB/s of text out and of image in, stretches and stretches used
  count     the same call with out = NULL (search, count and chain only)
  host      (--baseline) host/GzParallel.cpp on 16 threads over the same image, in this process (tools/probes/
            gz_parallel_shim.cpp, built here with g++), wall clock, median of 4 after one warm-up, between the device
            measurements; its text is held against the device's
One JSON line per configuration; --out writes them to a file (profiles/gunzip/gunzip_rate.jsonl).

The split of the stages comes from a run of its own under the profiler, never together with the timing above:
  rocprofv3 --kernel-trace --stats -d profiles/gunzip/trace -- python tools/probes/gunzip_rate.py --iters 3 --only se_150
(the sk_gunzip_*_kernel rows of the kernel statistics are the nine stages)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, HERE)
SHIM = os.path.join(HERE, "libgz_parallel_shim.so")


def host_decoder(threads=16):
    """Builds and loads the shim around GzParallel -> the C function"""
    os.environ["SICKLE_HOST_THREADS"] = str(threads)  # read when the pool is first used
    host = os.path.join(ROOT, "sickle_amd", "csrc", "host")
    src = [os.path.join(HERE, "gz_parallel_shim.cpp")] + [os.path.join(host, f) for f in ("GzParallel.cpp", "Deflate.cpp", "WorkerPool.cpp")]
    if not os.path.exists(SHIM) or any(os.path.getmtime(s) > os.path.getmtime(SHIM) for s in src):
        subprocess.run(["g++", "-O3", "-std=c++17", "-shared", "-fPIC", "-I" + host, "-o", SHIM] + src + ["-lz", "-lpthread"], check=True)
    fn = C.CDLL(SHIM).skp_gz_parallel
    fn.restype = C.c_longlong
    fn.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_ulonglong)]
    return fn


def run_host(fn, image, text_bytes, threads=16):
    """-> (result fields, the text as bytes)"""
    out = C.create_string_buffer(text_bytes + 1)
    used = C.c_ulonglong()
    secs, got = [], 0
    for _ in range(5):
        t0 = time.perf_counter()
        got = fn(image, len(image), out, text_bytes + 1, C.byref(used))
        secs.append(time.perf_counter() - t0)
    assert got == text_bytes, got
    med = sorted(secs[1:])[2]
    return ({"host_threads": threads, "host_stretches_used": int(used.value), "host_median_ms": round(med * 1e3, 3),
             "host_GBps_text": round(text_bytes / med / 1e9, 2)}, out.raw[:text_bytes])


def gzip6(text):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(text) + c.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated configuration names")
    ap.add_argument("--baseline", action="store_true", help="also time GzParallel on 16 host threads on the same image")
    ap.add_argument("--text-mb", type=int, default=0, help="cut each text to this many MB (0: the whole text)")
    args = ap.parse_args()
    fn = host_decoder() if args.baseline else None
    import torch
    torch.cuda.is_available()
    from bgzf_device_rate import timed
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
        if args.text_mb:
            text = text[:args.text_mb * 1_000_000].clone()
        host_text = text.cpu().numpy().tobytes()
        t0 = time.perf_counter()
        blob = gzip6(host_text)
        res = {"config": name, "text_bytes": len(host_text), "image_bytes": len(blob), "gzip6_seconds": round(time.perf_counter() - t0, 1)}
        image = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
        n, T = image.numel(), text.numel()
        wsb = L.sk_gzip_inflate_workspace_bytes(n, T)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        out = torch.empty(max(T, 16), dtype=torch.uint8, device="cuda")
        counts = {}
        fin = lambda: counts.update(ctx.gzip_inflate_device_finish(ws.data_ptr()))
        med, lo = timed(torch, args.iters, lambda: ctx.gzip_inflate_device_async(image.data_ptr(), n, out.data_ptr(), T, ws.data_ptr(), wsb), fin)
        assert counts["bytes_out"] == T and bool(torch.equal(out[:T], text))
        res.update({"members": counts["members"], "stretches": counts["stretches"], "stretches_used": counts["stretches_used"],
                    "inflate_median_ms": round(med, 3), "inflate_min_ms": round(lo, 3), "inflate_GBps_text": round(T / med / 1e6, 2),
                    "inflate_GBps_image": round(n / med / 1e6, 2), "inflate_workspace_bytes": wsb})
        if fn is not None:
            host, decoded = run_host(fn, blob, T)
            assert decoded == host_text
            res.update(host)
            res["device_over_host"] = round(host["host_median_ms"] / med, 2)
        med, lo = timed(torch, args.iters, lambda: ctx.gzip_inflate_device_async(image.data_ptr(), n, None, 0, ws.data_ptr(), wsb), fin)
        res.update({"count_median_ms": round(med, 3), "count_min_ms": round(lo, 3)})
        print(json.dumps(res), flush=True)
        lines.append(res)
        del text, image, ws, out, host_text, blob
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))
    ctx.close()


if __name__ == "__main__":
    main()

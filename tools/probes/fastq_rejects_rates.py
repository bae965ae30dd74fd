"""What the rejects (sk_trim_fastq_rejects_device_async, sickle_amd/csrc/sk_fastq_rejects.hip) cost behind a text call, on
10 M x 150 bp SE (the se_150 text of tools/fastq_trim_rates.py) on one MI355X, at -q 20 -l 20 and with every read rejected
(-l 1000).

Per setting three variants are timed with HIP events around what is enqueued, alternated within one job on one device,
`--rounds` rounds of `--iters` calls each, after a warm-up call of each:
  trim           sk_trim_fastq_device_async alone, writing its outputs
  trim+rejects   ... and the writing rejects call behind it
  rejects        the rejects call alone, over the workspace the last text call left: its four kernels
and the read-stream rate sk_probe_read_bandwidth gives on the text's bytes in the same job.  The rejects call reads the
rejected records out of those bytes and writes as many, so `rejects_GBps` = 2 * bytes / the `rejects` median counts both
directions; it is set beside the stream's rate, which only reads.  One JSON line per setting and variant with the median
and min-max over all rounds; --out also writes them to a file."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()
    from fastq_trim_rates import make_text
    from sickle_amd import capi
    ctx = capi.Context(device=0)
    L = capi.lib()
    text = make_text(torch, args.reads, 150, 150, 1)
    T = text.numel()
    ptrs, sizes = [text.data_ptr()], [T]
    nb = L.sk_trim_fastq_workspace_bytes(T, 0)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    jb = L.sk_trim_fastq_rejects_workspace_bytes(T)
    jws = torch.empty(jb, dtype=torch.uint8, device="cuda")
    lines = []
    for setting, min_len in (("q20_l20", 20), ("all_rejected", 1000)):
        params = capi.make_params("sanger", 20, min_len, False, False)
        ctx.trim_fastq_device_async(params, ptrs, sizes, [capi.FastqOutput() for _ in range(3)], ws.data_ptr(), nb, mode="se")
        ctx.trim_fastq_rejects_device_async(ws.data_ptr(), T, 0, ptrs, sizes, None, jws.data_ptr(), jb, mode="se")
        counts = ctx.trim_fastq_device_finish(ws.data_ptr())
        need = ctx.trim_fastq_rejects_device_finish(jws.data_ptr())
        buf = torch.empty(counts["bytes"][0] + 16, dtype=torch.uint8, device="cuda")
        outs = [capi.FastqOutput(buf.data_ptr(), counts["bytes"][0], None, 0), capi.FastqOutput(), capi.FastqOutput()]
        rej = torch.empty(need["bytes"] + 16, dtype=torch.uint8, device="cuda")
        rej_out = capi.FastqOutput(rej.data_ptr(), need["bytes"], None, 0)

        def call(trim, rejects):
            if trim:
                ctx.trim_fastq_device_async(params, ptrs, sizes, outs, ws.data_ptr(), nb, mode="se")
            if rejects:
                ctx.trim_fastq_rejects_device_async(ws.data_ptr(), T, 0, ptrs, sizes, rej_out, jws.data_ptr(), jb, mode="se")

        def finish(trim, rejects):
            if trim:
                ctx.trim_fastq_device_finish(ws.data_ptr())
            if rejects:
                got = ctx.trim_fastq_rejects_device_finish(jws.data_ptr())
                assert got == dict(need), (got, need)
            torch.cuda.synchronize()

        variants = [("trim", (True, False)), ("trim+rejects", (True, True)), ("rejects", (False, True))]
        for _, how in variants:  # warm-up
            call(*how)
            finish(*how)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = {v: [] for v, _ in variants}
        for _ in range(args.rounds):
            for v, how in variants:
                for _ in range(args.iters):
                    e0.record()
                    call(*how)
                    e1.record()
                    finish(*how)
                    ms[v].append(e0.elapsed_time(e1))
        stream_GBps = ctx.probe_read_bandwidth(ptrs[0], T)
        for v, _ in variants:
            x = sorted(ms[v])
            med = x[len(x) // 2]
            res = {"setting": setting, "variant": v, "reads": need["reads"], "rejected": need["records"],
                   "rejects_bytes": need["bytes"], "kept_bytes": counts["bytes"][0], "text_bytes": T, "calls": len(x),
                   "median_ms": round(med, 3), "min_ms": round(x[0], 3), "max_ms": round(x[-1], 3),
                   "read_stream_GBps": round(stream_GBps, 1), "text_at_stream_ms": round(T / stream_GBps / 1e6, 3)}
            if v == "rejects":
                res["rejects_GBps"] = round(2 * need["bytes"] / med / 1e6, 1)
            print(json.dumps(res), flush=True)
            lines.append(res)
        del buf, rej
        torch.cuda.empty_cache()
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))
    ctx.close()


if __name__ == "__main__":
    main()

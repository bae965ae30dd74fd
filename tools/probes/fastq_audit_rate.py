"""What the audit (sk_trim_fastq_audit_device_async, sickle_amd/csrc/sk_fastq_audit.hip) costs behind a text call, on the
four texts of tools/fastq_trim_rates.py on one MI355X.

Three variants are timed with HIP events around what is enqueued, alternated within one job on one device, `--rounds`
rounds of `--iters` calls each:
  trim             sk_trim_fastq_device_async alone
  trim+audit       ... and the audit without a histogram (reset, names pass in the pair modes, quality pass, fold)
  trim+audit+hist  ... and the full audit (the quality pass with its LDS tables)
and the read-stream rate sk_probe_read_bandwidth gives on the packed qual's bytes of the same workspace in the same job:
the yardstick for the quality pass, which reads those bytes once.  One JSON line per configuration and variant with the
median and min-max over all rounds; --out also writes them to a file.  --once: one warm call of the trim with the full
report (its quality kernel reads the same bytes) and the full audit behind it per configuration, and nothing else (for a
run under `rocprofv3 --kernel-trace --stats`)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

NAME_LINE_BYTES = 11  # make_text's "@r<9 digits>"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated configuration names")
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    import torch
    torch.cuda.is_available()
    from fastq_trim_rates import make_text
    from sickle_amd import capi
    ctx = capi.Context(device=0)
    L = capi.lib()
    configs = [("se_150", "se", False, [(10_000_000, 150, 150, 1)]),
               ("split_150_n", "pe_split", True, [(5_000_000, 150, 150, 2), (5_000_000, 150, 150, 3)]),
               ("se_mix", "se", False, [(4_000_000, 75, 301, 4)]),
               ("se_10k", "se", False, [(100_000, 10_000, 10_000, 5)])]
    lines = []
    for name, mode, trunc_n, specs in configs:
        if args.only and name not in args.only.split(","):
            continue
        texts = [make_text(torch, n, lo, hi, seed) for n, lo, hi, seed in specs]
        params = capi.make_params("sanger", 20, 50, False, trunc_n)
        T = sum(t.numel() for t in texts)
        nb = L.sk_trim_fastq_workspace_bytes(T, params.trunc_n)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        ptrs, sizes = [t.data_ptr() for t in texts], [t.numel() for t in texts]
        ctx.trim_fastq_device_async(params, ptrs, sizes, [capi.FastqOutput() for _ in range(3)], ws.data_ptr(), nb, mode=mode)
        counts = ctx.trim_fastq_device_finish(ws.data_ptr())
        bufs, outs = [], []
        for o in range(3):
            t = torch.empty(counts["bytes"][o] + 16, dtype=torch.uint8, device="cuda")
            bufs.append(t)
            outs.append(capi.FastqOutput(t.data_ptr(), counts["bytes"][o], None, counts["records"][o]))
        aud = torch.zeros(capi.AUDIT_WORDS + 256, dtype=torch.int64, device="cuda")
        hist_ptr = aud.data_ptr() + 8 * capi.AUDIT_WORDS

        def call(audit, hist=False):
            ctx.trim_fastq_device_async(params, ptrs, sizes, outs, ws.data_ptr(), nb, mode=mode)
            if audit:
                ctx.trim_fastq_audit_device_async(ws.data_ptr(), T, params.trunc_n, aud.data_ptr(), text_ptrs=ptrs,
                                                  text_bounds=sizes, mode=mode, qual_hist_ptr=hist_ptr if hist else None,
                                                  reset=True)

        if args.once:
            bins = 512
            rep = torch.zeros(capi.REPORT_WORDS + 6 * bins, dtype=torch.int64, device="cuda")
            at = lambda j: rep.data_ptr() + 8 * (capi.REPORT_WORDS + j * bins)
            full = capi.FastqReportHists(at(0), at(1), bins, at(2), at(3), at(4), at(5), bins)
            for _ in range(2):
                ctx.trim_fastq_device_async(params, ptrs, sizes, outs, ws.data_ptr(), nb, mode=mode)
                ctx.trim_fastq_report_device_async(ws.data_ptr(), T, params.trunc_n, rep.data_ptr(), hists=full, reset=True)
                ctx.trim_fastq_audit_device_async(ws.data_ptr(), T, params.trunc_n, aud.data_ptr(), text_ptrs=ptrs,
                                                  text_bounds=sizes, mode=mode, qual_hist_ptr=hist_ptr, reset=True)
                ctx.trim_fastq_device_finish(ws.data_ptr())
            continue
        variants = [("trim", (False, False)), ("trim+audit", (True, False)), ("trim+audit+hist", (True, True))]
        for _, v in variants:  # warm-up
            call(*v)
            ctx.trim_fastq_device_finish(ws.data_ptr())
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = {v: [] for v, _ in variants}
        for _ in range(args.rounds):
            for v, how in variants:
                for _ in range(args.iters):
                    e0.record()
                    call(*how)
                    e1.record()
                    ctx.trim_fastq_device_finish(ws.data_ptr())
                    ms[v].append(e0.elapsed_time(e1))
        audit = capi.FastqAudit.from_buffer_copy(aud.cpu().numpy()[:capi.AUDIT_WORDS].tobytes()).as_dict()
        packed = audit["qual_bytes"]
        # the same bytes, in the same workspace, through the read-stream probe
        # (the packed qual is the workspace's last section, or with -n the last but one: sk_device.h)
        stream = ctx.probe_read_bandwidth(ws.data_ptr() + (nb - (2 if trunc_n else 1) * 16 * ((T + 31) // 32)), packed)
        for v, _ in variants:
            x = sorted(ms[v])
            res = {"config": name, "variant": v, "mode": mode, "trunc_n": bool(trunc_n), "pairs": audit["pairs"],
                   "name_mismatch": audit["name_mismatch"], "name_line_bytes": 2 * audit["pairs"] * NAME_LINE_BYTES,
                   "text_bytes": T, "packed_qual_bytes": packed, "qual_min": audit["qual_min"], "qual_max": audit["qual_max"],
                   "calls": len(x), "median_ms": round(x[len(x) // 2], 3), "min_ms": round(x[0], 3), "max_ms": round(x[-1], 3),
                   "read_stream_GBps": round(stream, 1), "packed_qual_at_stream_ms": round(packed / stream / 1e6, 3)}
            print(json.dumps(res), flush=True)
            lines.append(res)
        del texts, ws, bufs
        torch.cuda.empty_cache()
    if args.out and lines:
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(r) + "\n" for r in lines))
    ctx.close()


if __name__ == "__main__":
    main()

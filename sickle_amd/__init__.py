"""sickle_amd -- MI355X-native drop-in for the sliding-window quality scan of
pentalpha/sickle (reference src/trim.cpp:3-116) behind its `sickle se` / `sickle pe` CLI.

The product is native: sickle_amd/csrc/ holds the HIP kernels, the C-ABI library
(include/sickle_amd.h -> libsickle_amd.so) and the C++ host pipeline (`sickle` binary).
This Python package is the ctypes view of that C ABI: tests and bench.py use it, and
capi.Context.trim_reads_device gives torch users the trimmed reads of a device-resident
batch (scan, sk_trim_device_async, finish) without leaving the device, and capi.Context.trim_fastq the
trimmed FASTQ text of FASTQ text in device memory (sk_trim_fastq_device_async: frame, check, scan, emit)."""

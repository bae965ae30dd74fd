"""The device-side regrouping of ragged batches (sk_sort.hip) and the scan of its tiles (sk_scan_tile_sorted_kernel<true|false>)
on the GPU: the sort kernels' own output against tests/sort_model.py, and the regrouped scan against the oracle.  The library
reads SK_SORT_MIN and SK_SORT once per process, so everything here runs in child processes -- one run each, under a time
limit, never repeated; a child that fails is reported with the end of its output."""
import os
import subprocess
import sys

import numpy as np
import pytest

import sort_model as sm

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PROBE = os.path.join(HERE, "sort_device", "sort_probe")


def child(cmd, timeout, **env):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **env))
    assert r.returncode == 0, "%s: exit status %d\n%s%s" % (" ".join(cmd[-3:]), r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def soak(script, *args, **env):
    out = child([sys.executable, os.path.join(HERE, script)] + [str(a) for a in args], 900, **env)
    assert "soak ok" in out, out[-2000:]
    return out


@pytest.mark.parametrize("max_len", sm.MAX_LENS)
def test_sort_kernels_against_the_model(tmp_path, max_len):
    """tests/sort_device/sort_probe (built by build(), for gfx950) runs sk_launch_sort once per case on pre-filled scratch;
    counts, tile lists and perm are compared with the model, order-free where atomics decide the order: every read in
    exactly one tile of its class and window, offsets, lengths, rows, longest and shortest, nothing beyond the counts."""
    assert os.path.exists(PROBE), "tests/sort_device/sort_probe is missing: build() makes it (make -C tests/embed all)"
    cases = [c for c in sm.cases() if c[2] == max_len]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.uint64(len(cases)).tobytes())
        for name, n, ml, offs in cases:
            f.write(np.array([n, ml], dtype=np.uint64).tobytes())
            f.write(offs.tobytes())
    out = child([PROBE, src, dst], 600)
    assert "sort_probe ok: %d cases" % len(cases) in out, out[-2000:]
    verdicts = [0, 0]
    with open(dst, "rb") as f:
        for name, n, ml, offs in cases:
            cap = int(np.fromfile(f, dtype=np.uint64, count=1)[0])
            assert cap == sm.list_cap(n), (name, n, cap)
            counts = np.fromfile(f, dtype=np.uint32, count=16)
            lists = np.fromfile(f, dtype=np.uint64, count=8 * cap * 4).reshape(8, cap, 4)
            perm = np.fromfile(f, dtype=np.uint64, count=8 * cap * 64).reshape(8, cap, 64)
            try:
                sm.check(offs, ml, counts, lists, perm)
            except AssertionError as e:
                raise AssertionError("lengths %r, %d reads, max_len %d: %s" % (name, n, ml, e)) from None
            verdicts[int(counts[8])] += 1
        assert f.read(1) == b""
    os.remove(dst)
    assert min(verdicts) >= len(cases) // 6, verdicts  # both verdicts among the cases


def test_regrouped_scan_soak():
    """tests/soak_sorted.py with every ragged batch regrouped (SK_SORT_MIN=1): all three kinds of batch occur."""
    out = soak("soak_sorted.py", 48, 2029, SK_SORT_MIN="1")
    kinds = out[out.rindex("soak ok"):].split("them:")[1]
    assert all(int(part.split()[0]) > 0 for part in kinds.split(",")), out[-500:]


def test_tile_soak_regrouped():
    """tests/soak_tiles.py, whose `offsets` runs are regrouped with SK_SORT_MIN=1 (1 .. 5 000 reads of 1 .. 504 bases)."""
    soak("soak_tiles.py", 100, 2030, SK_SORT_MIN="1")


def test_general_soak_regrouped():
    """tests/soak_general.py behind a regrouping: left-overs for the general kernels, hints, SK_GENERAL=band|team|stream."""
    soak("soak_general.py", 60, 2031, SK_SORT_MIN="1")


def test_regrouping_switched_off():
    """SK_SORT=0: the same batches keep the plain tile kernel and the general kernels, and give the oracle's cuts."""
    soak("soak_sorted.py", "--allow-unsorted", 16, 2032, SK_SORT_MIN="1", SK_SORT="0")

"""The device's BGZF writer without a device: the CRC-32 phases and the framing functions of
sickle_amd/csrc/sk_bgzf_block.h run on the host lane after lane (tests/bgzf_device/bgzf_host) against zlib and against
tests/cpu_shim/gpu_deflate_sim, the committed statement of the member image; and the two pure sizing functions of the
C ABI.  CPU only."""
import gzip
import os
import subprocess
import zlib

import pytest

import cli_util as cu
from test_gz_inflater import SIM, TEXT, _encoder_inputs

HOST = os.path.join(cu.ROOT, "tests", "bgzf_device", "bgzf_host")
BLOCK = 65280
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def tools():
    subprocess.run(["make", "-s", "-C", os.path.join(cu.ROOT, "tests", "bgzf_device"), "all"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(cu.ROOT, "tests", "cpu_shim"), "all"], check=True)
    return HOST


def sim_image(data, tmp_path, name="in"):
    src = str(tmp_path / (name + ".txt"))
    open(src, "wb").write(data)
    pr = subprocess.run([SIM, src], capture_output=True)
    assert pr.returncode == 0, pr.stderr
    return pr.stdout


def test_crc_phases_equal_zlib(tools, tmp_path):
    src = str(tmp_path / "text.txt")
    open(src, "wb").write(TEXT)
    lens = list(range(301)) + [65279, 65280]
    pr = subprocess.run([tools, "crclen", src] + [str(n) for n in lens], capture_output=True)
    assert pr.returncode == 0
    got = [int(x, 16) for x in pr.stdout.split()]
    assert got == [zlib.crc32(TEXT[:n]) for n in lens]
    for name, data in _encoder_inputs().items():
        src = str(tmp_path / (name + ".txt"))
        open(src, "wb").write(data)
        pr = subprocess.run([tools, "crc", src], capture_output=True)
        assert pr.returncode == 0, name
        want = [zlib.crc32(data[a:a + BLOCK]) for a in range(0, len(data), BLOCK)]
        assert [int(x, 16) for x in pr.stdout.split()] == want, name


def test_framing_equals_the_sim(tools, tmp_path):
    for name, data in _encoder_inputs().items():
        assert len(data) >= 1
        want = sim_image(data, tmp_path, name)
        src = str(tmp_path / (name + ".txt"))
        pr = subprocess.run([tools, "image", src], capture_output=True)
        assert pr.returncode == 0, name
        assert pr.stdout == want, name
        assert gzip.decompress(pr.stdout) == data, name
        pr = subprocess.run([tools, "image", src, "eof"], capture_output=True)
        assert pr.stdout == want + EOF and gzip.decompress(pr.stdout) == data, name
    assert gzip.decompress(EOF) == b""


def test_bound_and_workspace_need_no_device(tools, tmp_path):
    from sickle_amd import capi
    L = capi.lib()
    assert capi.SK_BGZF_EOF == 1
    assert L.sk_bgzf_bound(0, capi.SK_BGZF_EOF) == 28 and L.sk_bgzf_bound(0, 0) == 0
    for name, data in _encoder_inputs().items():
        image = sim_image(data, tmp_path, name)
        assert L.sk_bgzf_bound(len(data), 0) >= len(image), name
        assert L.sk_bgzf_bound(len(data), capi.SK_BGZF_EOF) >= len(image) + 28, name
    sizes = sorted(set([0, 1, 2, 100] + [k * BLOCK + d for k in (1, 2, 3, 1279, 1280, 1281, 70000) for d in (-1, 0, 1)] +
                       [1 << 32, (1 << 32) + 1, 1 << 40]))
    bounds = [L.sk_bgzf_bound(n, 0) for n in sizes]
    works = [L.sk_bgzf_workspace_bytes(n) for n in sizes]
    assert bounds == sorted(bounds) and works == sorted(works)
    for n, bound, work in zip(sizes, bounds, works):
        nb = (n + BLOCK - 1) // BLOCK
        assert bound == n + 31 * nb  # every block stored: text + 5 + 26
        assert work == 128 + 16 * nb + 261152 * min(nb, 1280) + 65536 * nb  # the formula of include/sickle_amd.h
        assert work % 16 == 0
    # bad arguments are refused before anything touches a device
    assert L.sk_bgzf_device_async(None, None, None, 0, 0, None, 0, None) == capi.SK_EINVAL
    assert L.sk_trim_fastq_output_words(None, 0, None, None) == capi.SK_EINVAL


def test_codes_of_every_dynamic_header(tools, tmp_path):
    """What inflating cannot show (zlib accepts some incomplete codes): in every deflated member of every encoder input no
    literal/length or distance code is longer than 15 bits, no code-length code longer than 7, and all three codes are
    complete (Kraft sum exactly 1).  tests/golden/bgzf_deep_code_length.txt (one block of FASTQ-like text with a third of
    its bytes random, found by a search over the soak's generator) is an input on which skd_huffman's limiter has to
    act on the code-length code: a Huffman tree over the header's own code-length symbol counts is 8 deep, the header
    states 7 bits and a complete code.  And a block whose matches all have one distance: the distance code is the one
    used symbol plus symbol 0."""
    import numpy as np
    import soak_bgzf
    depth = {}
    for name, data in _encoder_inputs().items():
        soak_bgzf.members(sim_image(data, tmp_path, name), data, depth)
    assert depth["literal/length"] == 15  # "fibonacci"
    deep = open(os.path.join(cu.ROOT, "tests", "golden", "bgzf_deep_code_length.txt"), "rb").read()
    assert len(deep) == BLOCK
    one = {}
    assert [m[0] for m in soak_bgzf.members(sim_image(deep, tmp_path, "deep"), deep, one)] == [False]
    assert one["code-length"] == 7 and one["code-length, unlimited"] == 8
    text = soak_bgzf.one_distance_text(np.random.default_rng(3), BLOCK)
    image = sim_image(text, tmp_path, "one_distance")
    assert soak_bgzf.members(image, text, {}) == [(False, len(image), BLOCK)] and len(image) < BLOCK // 20
    assert soak_bgzf.one_far_distance(soak_bgzf.dynamic_header(image[18:-8])[1])


def test_bgzf_host_soak(tools):
    """tests/soak_bgzf.py run_host: drawn texts through the sim, every member against zlib, every dynamic header checked,
    bgzf_host's image and CRC-32 against the sim and zlib.  Both verdicts occur, and some deflated block is within 2 % of
    its text's size (the sweep reaches the threshold from below)."""
    import soak_bgzf
    stats = {}
    assert soak_bgzf.run_host(15, 2028, verbose=False, stats=stats) == 45
    assert stats["stored"] > 0 and stats["deflated"] > 0 and stats["closest"] > 0.98
    assert stats["depth"]["literal/length"] <= 15 and stats["depth"]["code-length"] <= 7

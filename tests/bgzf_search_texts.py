"""Shared by tests/test_bgzf_search_host.py and tests/test_gpu_bgzf_search.py: the texts the searching BGZF encoder
(SK_BGZF_SEARCH) is tested on, and tests/bgzf_search/search_host, the program that runs its phases on the host."""
import os
import subprocess

import numpy as np

import cli_util as cu

BLOCK = 65280
DIR = os.path.join(cu.ROOT, "tests", "bgzf_search")
HOST = os.path.join(DIR, "search_host")
HOST_SAN = os.path.join(DIR, "search_host_san")
PLAIN = os.path.join(cu.ROOT, "tests", "bgzf_device", "bgzf_host")  # the encoder without the search
FASTQ_FILES = ("test.fastq", "test.f.fastq", "test.r.fastq", "problem1.fastq")
KEY = bytes(range(0x30, 0x30 + 40))  # 40 different bytes, none of them 'a', 'b' or a newline


def build():
    subprocess.run(["make", "-s", "-C", DIR, "all"], check=True)
    subprocess.run(["make", "-s", "-C", os.path.dirname(PLAIN), "all"], check=True)


def synth_text(blocks=3, seed=11):
    from sickle_amd import synth
    seq, qual = synth.make_reads(seed, blocks * BLOCK // 200, 100)
    text = bytes(synth.fastq_bytes_fast(seq, qual))
    assert len(text) >= blocks * BLOCK
    return text[:blocks * BLOCK]


def apart(distance):
    """KEY twice, `distance` bytes apart, in one line of one block, with nothing between them that could take KEY's place
    in the table"""
    return KEY + b"a" * (distance - len(KEY)) + KEY + b"b" * 100 + b"\n"


def edge_texts():
    rng = np.random.default_rng(5)
    long_repeat = rng.integers(65, 91, 700, dtype=np.uint8).tobytes()
    return {
        "empty": b"",
        "one_byte": b"x",
        "no_newline": rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 100000).tobytes(),
        "one_line": rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), BLOCK - 1).tobytes() + b"\n",
        "newlines_only": b"\n" * 70000,
        "one_repeated_byte": b"a" * 150000,
        "random": rng.integers(0, 256, BLOCK, dtype=np.uint8).tobytes(),
        "apart_32768": apart(32768),
        "apart_32769": apart(32769),
        "long_repeat": (long_repeat + b"\n") * 3 + b"tail\n",
        "second_block_one_byte": synth_text(2, seed=12)[:BLOCK + 1],
    }


def fastq_texts():
    return {name: open(os.path.join(cu.ROOT, "tests", "golden", "inputs", name), "rb").read() for name in FASTQ_FILES}


def run(tool, mode, path, *flags):
    pr = subprocess.run([tool, mode, path] + list(flags), capture_output=True)
    assert pr.returncode == 0, (tool, mode, path, flags, pr.returncode, pr.stderr[-2000:])
    return pr.stdout


def host_image(data, directory, name, *flags, tool=HOST):
    path = os.path.join(str(directory), name + ".txt")
    if not os.path.exists(path):
        with open(path, "wb") as f:
            f.write(data)
    return run(tool, "image", path, *flags)

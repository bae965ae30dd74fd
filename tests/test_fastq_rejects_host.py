"""The rule of sickle_amd/csrc/sk_fastq_rejects.h on the host (tests/fastq_rejects/rejects_host.cpp): a stand-alone program
that walks drawn batches and the GPU test's shapes in the four kernels' shape and compares with a naive copy, built plain
and under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

import fastq_rejects_model as jm

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fastq_rejects")


@pytest.fixture(scope="module", params=["rejects_host", "rejects_host_san"])
def tool(request):
    subprocess.run(["make", "-s", "-C", DIR, "all"], check=True)
    return os.path.join(DIR, request.param)


def test_rule_on_the_host(tool):
    pr = subprocess.run([tool], capture_output=True)
    assert pr.returncode == 0, pr.stderr.decode()[-2000:]
    word, cases, _, chunk, _, window, _, block = pr.stdout.split()[:8]
    assert word == b"ok" and int(cases) > 500
    # the kernels' sizes as the program walks them: the GPU test plants its edges at these
    assert (int(chunk), int(window), int(block)) == (jm.GCHUNK, jm.WIN, jm.BLOCK_READS)


def test_the_program_sees_a_forgotten_mate(tool):
    """with the mate no longer looked at in the selection on the walk's side the comparison fails"""
    pr = subprocess.run([tool, "--corrupt"], capture_output=True)
    assert pr.returncode == 1 and b"differ" in pr.stderr

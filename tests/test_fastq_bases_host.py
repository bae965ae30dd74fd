"""The rule of sickle_amd/csrc/sk_fastq_bases.h on the host (tests/fastq_bases/bases_host.cpp): a stand-alone program
that walks drawn batches and the GPU test's shapes in the kernel's shape and compares with a naive computation, built
plain and under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

import fastq_bases_model as bm

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fastq_bases")


@pytest.fixture(scope="module", params=["bases_host", "bases_host_san"])
def tool(request):
    subprocess.run(["make", "-s", "-C", DIR, "all"], check=True)
    return os.path.join(DIR, request.param)


def test_rule_on_the_host(tool):
    pr = subprocess.run([tool], capture_output=True)
    assert pr.returncode == 0, pr.stderr.decode()[-2000:]
    word, cases, _, chunk = pr.stdout.split()[:4]
    assert word == b"ok" and int(cases) > 100
    # the header's chunk as the compiler sees it: the GPU test plants its edges at either side of this boundary
    assert int(chunk) == bm.CHUNK_BYTES


def test_the_program_sees_unfolded_lower_case(tool):
    """with lower case no longer folded into the classes on the walk's side the comparison fails"""
    pr = subprocess.run([tool, "--corrupt"], capture_output=True)
    assert pr.returncode == 1 and b"differ" in pr.stderr

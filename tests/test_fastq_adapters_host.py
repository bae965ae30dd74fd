"""The rule of sickle_amd/csrc/sk_fastq_adapters.h on the host (tests/fastq_adapters/adapters_host.cpp): a stand-alone
program that walks drawn lines in the kernel's shape (encode, window, compare, reduce) and compares with a naive byte
loop, built plain and under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fastq_adapters")


@pytest.fixture(scope="module", params=["adapters_host", "adapters_host_san"])
def tool(request):
    subprocess.run(["make", "-s", "-C", DIR, "all"], check=True)
    return os.path.join(DIR, request.param)


def test_rule_on_the_host(tool):
    pr = subprocess.run([tool], capture_output=True)
    assert pr.returncode == 0, pr.stderr.decode()[-2000:]
    word, cases = pr.stdout.split()[:2]
    assert word == b"ok" and int(cases) > 100000


def test_the_program_sees_a_dropped_valid_plane(tool):
    """with the VALID plane dropped on the walk's side an N reads as an A, and the comparison fails"""
    pr = subprocess.run([tool, "--corrupt"], capture_output=True)
    assert pr.returncode == 1 and b"differ" in pr.stderr

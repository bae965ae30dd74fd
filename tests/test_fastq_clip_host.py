"""The rule of sickle_amd/csrc/sk_fastq_clip.h on the host (tests/fastq_clip/clip_host.cpp): a stand-alone program that
walks drawn lines in the kernel's shape (the line from its descriptor, the search, the clip word, the pack's min, the
stats) and compares with a naive byte loop, built plain and under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fastq_clip")


@pytest.fixture(scope="module", params=["clip_host", "clip_host_san"])
def tool(request):
    subprocess.run(["make", "-s", "-C", DIR, "all"], check=True)
    return os.path.join(DIR, request.param)


def test_rule_on_the_host(tool):
    pr = subprocess.run([tool], capture_output=True)
    assert pr.returncode == 0, pr.stderr.decode()[-2000:]
    word, cases = pr.stdout.split()[:2]
    assert word == b"ok" and int(cases) > 50000


def test_the_program_sees_a_pack_that_ignores_the_clip(tool):
    """with the pack taking every line whole the packed lengths differ, and the comparison fails"""
    pr = subprocess.run([tool, "--corrupt"], capture_output=True)
    assert pr.returncode == 1 and b"differ" in pr.stderr

"""The report rule of sickle_amd/csrc/sk_fastq_report.h on the host (tests/fastq_report/report_host.cpp): a stand-alone
program that walks drawn batches and the GPU test's shapes in the two kernels' shape and compares with a naive
computation, built plain and under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fastq_report")


@pytest.fixture(scope="module", params=["report_host", "report_host_san"])
def tool(request):
    subprocess.run(["make", "-s", "-C", DIR, "all"], check=True)
    return os.path.join(DIR, request.param)


def test_rule_on_the_host(tool):
    pr = subprocess.run([tool], capture_output=True)
    assert pr.returncode == 0, pr.stderr.decode()[-2000:]
    word, cases = pr.stdout.split()[:2]
    assert word == b"ok" and int(cases) > 100


def test_the_program_sees_a_wrong_sum(tool):
    """with the last bin's register sums left out of the walk the comparison fails"""
    pr = subprocess.run([tool, "--corrupt"], capture_output=True)
    assert pr.returncode == 1 and b"differ" in pr.stderr

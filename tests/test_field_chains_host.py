"""The chained field products (csrc/fields.cuh: Fs<P, true>, what the bucket accumulation runs) against the plain ones on the host, limb
for limb, on both moduli: tests/native/fs_chain_check.cpp, a stand-alone program, built here with -fsanitize=undefined so that a signed
overflow of a column in either form ends it.  The plain products are the ones tests/test_fieldu.py holds against big integers at the
extremes of their preconditions; equality with them on the same extremes carries that over to the chained form.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "fs_chain_check.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not found")
def test_chained_products_equal_the_plain_ones(tmp_path):
    exe = str(tmp_path / "fs_chain_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-x", "c++", SRC, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "comparisons equal" in r.stdout and "runtime error" not in r.stderr

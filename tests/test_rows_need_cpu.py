"""CPU tier: the sparse base fetch of the rows kernels (fxg_rows_need_mask, fastx_toolkit_amd/csrc/fxg_rows.h).

tests/emu/rows_need.cpp runs the kernels' own __host__ __device__ predicate on the host (ds_bpermute becomes an index into the lanes'
klen words) against brute-force overlap, for every form the kernels are instantiated in and every stride from 28 up to the longest row
the form holds: whole and partial tiles, every read dropped / kept whole, kept lengths 0..4 and row - 1, prefix ends at every residue
mod 128, random cases.  Every byte of a kept prefix must lie in a fetched chunk, and no chunk that holds none may be fetched.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "rows_need.cpp")


@pytest.fixture(scope="module")
def rows_need(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rows_need") / "rows_need")
    subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-DFXG_HOST_EMULATION",
                           SRC, "-o", exe])
    return exe


@pytest.mark.parametrize("form", ["div", "h1_26", "h1_38", "h2_26", "h2_38", "r4_10", "r3_14", "r2_20"])
@pytest.mark.parametrize("seed", [1, 2])
def test_sparse_base_fetch_predicate(rows_need, form, seed):
    p = subprocess.run([rows_need, form, str(seed)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-2000:]

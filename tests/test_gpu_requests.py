"""The refused requests of tests/request_cases.py through the real libfxg.so: code and fxg_last_error text of each, as the CPU tier's stub gives them
(tests/test_barcode_cpu.py).  Nothing is launched: every case is refused on the host."""
import pytest

import request_cases as rq
from fastx_toolkit_amd import build

pytestmark = pytest.mark.gpu


def test_refused_requests_on_the_engine():
    s = rq.Session(build.LIBFXG)
    try:
        for case in rq.CASES:
            rq.refuse(s, case)
    finally:
        s.close()

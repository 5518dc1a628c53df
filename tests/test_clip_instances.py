"""CPU tier: the engine's one table of clip instances (csrc/fxg_clip_instances.h, as the emulator was compiled with it) against the tests' own
statement of the bucket set (helpers.CLIP_BUCKETS), the builds' unit counts, and the plan."""
import numpy as np

import emu_py as emu
from fastx_toolkit_amd import build
from helpers import CLIP_BUCKETS, CLIP_MAX_ADAPTER, clip_bucket, oracle_params


def test_clip_table_is_the_bucket_set_in_whole_units():
    """The table holds exactly helpers.CLIP_BUCKETS, every bucket in one unit, every unit holds some, and both split builds compile one translation
    unit per unit of the table (fastx_toolkit_amd/build.py: CLIP_UNITS; tests/emu_py.py: EMU_UNITS, which counts the unit without clip instances too)."""
    table, units = emu.clip_table()
    assert sorted(b for b, _ in table) == CLIP_BUCKETS, table          # (sorted: the table's order is the units', and nothing relies on it)
    assert len({b for b, _ in table}) == len(table), "a bucket in two units: %s" % table
    assert {u for _, u in table} == set(range(1, units + 1)), (table, units)
    assert units == build.CLIP_UNITS == emu.EMU_UNITS - 1


def test_plan_picks_the_bucket_of_every_adapter_length():
    """Every adapter length the C-ABI accepts, four letters, 100-byte rows: the planned instance is the packed one of the smallest bucket that holds it."""
    assert CLIP_MAX_ADAPTER == 99
    b = np.ascontiguousarray(np.random.default_rng(5).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(3, 100)))
    q = np.full((3, 100), 70, dtype=np.uint8)
    for alen in range(1, CLIP_MAX_ADAPTER + 1):
        emu.run_pipeline(b, q, None, oracle_params(dict(stages=1, adapter=(b"ACGT" * 25)[:alen], clip_min_len=5, clip_flags=4)))
        assert emu.last_plan()[0] == -clip_bucket(alen), (alen, emu.last_plan())

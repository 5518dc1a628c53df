"""CPU tier: what the generated code of the rows kernels must not contain (fastx_toolkit_amd/csrc/fxg_rows.h, profiles/rows_pack/isa_waits.md).

The unpredicated pack once went through volatile generic pointers; the compiler made every store of it a flat store followed by
s_waitcnt vmcnt(0) -- 84 round trips through the vector-memory path per tile where LDS stores issue back to back.  The pack now names its
LDS store instructions, and the next-ticket atomic a global address.  The built library is disassembled the way scripts/check_exec_zero.py
does it: no fxg_kernel_rows* symbol may hold a flat_ instruction, and none may use scratch (__launch_bounds__(64, 3): 168 VGPRs).
"""
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest

from conftest import ROOT

ROWS = re.compile(r"^_Z\d+fxg_kernel_rows")       # fxg_kernel_rows<NW, H> and fxg_kernel_rows_multi<NW, R>
INSTANCES = 7


@pytest.fixture(scope="module")
def rows_code():
    """{kernel symbol: [mnemonics]} and {kernel symbol: {metadata field: value}} of the built library's rows kernels"""
    from fastx_toolkit_amd import build as b
    b.build_engine()
    spec = importlib.util.spec_from_file_location("check_exec_zero", os.path.join(ROOT, "scripts", "check_exec_zero.py"))
    cez = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cez)
    ins, meta = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in cez.code_objects(b.LIBFXG, tmp):
            text = subprocess.run([os.path.join(cez.LLVM, "llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
            name = None
            for line in text.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
                if m:
                    name = m.group(1) if ROWS.match(m.group(1)) else None
                    if name:
                        ins[name] = []
                    continue
                m = re.match(r"^\s+(\S+)\s*(.*?)\s*// ([0-9A-F]+):", line)
                if m and name:
                    ins[name].append(m.group(1))
            notes = subprocess.run([os.path.join(cez.LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
            name = None
            for line in notes.splitlines():
                m = re.match(r"^\s*(?:- )?\.(\w+):\s*(\S+)\s*$", line)
                if not m:
                    continue
                if m.group(1) == "name" and line.startswith("    .name:"):       # a kernel's own name (its arguments' names are nested deeper)
                    name = m.group(2) if ROWS.match(m.group(2)) else None
                    if name:
                        meta[name] = {}
                elif name and m.group(1) in ("private_segment_fixed_size", "uses_dynamic_stack", "vgpr_count", "vgpr_spill_count", "sgpr_spill_count"):
                    meta[name][m.group(1)] = m.group(2)
    return ins, meta


def test_every_rows_instance_was_read(rows_code):
    ins, meta = rows_code
    assert len(ins) == INSTANCES and set(ins) == set(meta), (sorted(ins), sorted(meta))
    for name, mn in ins.items():
        assert len(mn) > 1000 and "s_endpgm" in mn and any(x.startswith("ds_write_b32") for x in mn), name
        assert "private_segment_fixed_size" in meta[name] and "vgpr_count" in meta[name], (name, meta[name])


def test_rows_kernels_have_no_flat_instruction(rows_code):
    ins, _ = rows_code
    for name, mn in ins.items():
        flat = sorted({x for x in mn if x.startswith("flat_")})
        assert not flat, "%s: %s" % (name, flat)


def test_rows_kernels_use_no_scratch(rows_code):
    ins, meta = rows_code
    for name, mn in ins.items():
        assert not [x for x in mn if x.startswith("scratch_")], name
        md = meta[name]
        assert int(md["private_segment_fixed_size"]) == 0 and md.get("uses_dynamic_stack", "false") == "false", (name, md)
        assert int(md.get("vgpr_spill_count", "0")) == 0, (name, md)
        assert int(md["vgpr_count"]) <= 168, (name, md)             # three waves per SIMD

"""fasta_nucleotide_changer on the MI355X: the C-ABI (fxg_bases_change, then fxg_fastq_format with out_fasta = 1) against the block model of
nucchange_model.py on the cases of nucchange_cases.py -- read lengths each side of the 16-byte pieces, bases lines at every offset modulo 16,
records whose bases share one aligned piece, record counts each side of a workgroup's records, where the `from` and `to` bytes are, what must
stay untouched, irregular blocks, the refusals -- with the whole text downloaded after every call; a block just past 2^31 bytes; the entry as
the first call a context sees; and the tool on the GPU build.  Reads the model and tests/golden/nuc_changer only."""
import ctypes as C

import numpy as np
import pytest

import nucchange_model as M
from fastx_toolkit_amd.engine import NO_RECORD, FxgBasesChangeInfo
from nucchange_cases import assert_tool_case, block_cases, galaxy_pairs, golden_cases, message_of, regular_text, run_tool

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
BLOCKS = block_cases()
ONE_MB = {"FXH_READ_BUFFER_MB": "1"}


class Indexed:
    """a block of records uploaded (16 sentinel bytes behind it) and indexed by fxg_fastq_index"""

    def __init__(self, eng, records):
        text = M.block_text(records)
        self.lpr = 4 if len(records[0]) == 4 else 2
        self.n, self.text_len = len(records), len(text)
        self.d_text = eng.torch.full((len(text) + 16,), SENTINEL, dtype=eng.torch.uint8, device=eng.device)
        self.d_text[:len(text)] = eng.torch.frombuffer(bytearray(text), dtype=eng.torch.uint8).to(eng.device)
        self.ix, self.lens, self.info = eng.fastq_index(self.d_text, len(text), True, cap_records=len(records), fasta=self.lpr == 2)
        assert self.info.records == len(records) and self.info.consumed == len(text) and not self.info.irregular

    def host(self):
        h = self.d_text.cpu().numpy()
        return h[:self.text_len].tobytes(), h[self.text_len:]


def call(eng, ix, mode, records=None, lpr=None, frm=None, to=None, text=True, line=True, ctx_of=None):
    """the C-ABI itself: (rc, info, message)"""
    e = ctx_of or eng
    f, t, _ = M.MODES[mode]
    info = FxgBasesChangeInfo()
    eng._after_torch()
    eng.torch.cuda.synchronize()
    rc = e.lib.fxg_bases_change(e.ctx, ix.d_text.data_ptr() if text else None, ix.text_len, ix.lpr if lpr is None else lpr, ix.ix.line.data_ptr() if line else None,
                                ix.ix.cap_lines, ix.n if records is None else records, f if frm is None else frm, t if to is None else to, C.byref(info))
    eng._before_torch()
    return rc, info, e.lib.fxg_last_error(e.ctx).decode(errors="replace")


def res_of(eng, ix, n):
    """every record kept whole: the res[] the formatter takes, from the indexed lengths"""
    return ((ix.lens[:n].to(eng.torch.int32) & 0xFFFF) | 0x10000).contiguous()


# ---- 1. the shared cases through index, change, format ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,records,mode", BLOCKS, ids=[b[0] for b in BLOCKS])
def test_abi_blocks(engine, name, records, mode):
    blk = M.Block(records, mode)
    ix = Indexed(engine, records)
    stride = max(ix.info.max_len, 1)
    rows_qual = None
    if blk.lpr == 4 and mode == "r" and not blk.irregular:          # -r: the pack comes first, and a U is what its base check refuses
        _, rows_qual, irr = engine.fastq_pack(ix.d_text, ix.text_len, ix.ix, ix.n, stride)
        assert irr == (0 if blk.first_to == M.NONE else M.IRR_BASE), name
    rc, info, msg = call(engine, ix, mode)
    assert rc == 0, (name, msg)
    text, guard = ix.host()
    assert text == blk.rewritten, name
    assert (guard == SENTINEL).all(), name
    assert (info.first_to_record, info.irregular) == (blk.first_to, blk.irregular), name
    if blk.first_to == M.NONE:
        assert info.changed == blk.changed, name
    if blk.lpr == 4 and mode == "d" and not blk.irregular:          # -d: the pack sees what the change left, A C G T N
        _, rows_qual, irr = engine.fastq_pack(ix.d_text, ix.text_len, ix.ix, ix.n, stride)
        assert irr == 0, name
    n = blk.records_out
    if n:
        out = engine.fastq_format(ix.d_text, ix.text_len, ix.ix, n, res=res_of(engine, ix, n), rows_qual=rows_qual, out_fasta=True)
        assert out.cpu().numpy().tobytes() == blk.out, name
    assert ix.host()[0] == blk.rewritten, name                      # (the formatter reads the text, it does not write it)


def test_abi_shared_pieces_many_times(engine):
    """the lost-update case once more, larger: 60 000 one-character records of 1 to 4 bases, all of them `from`, so that every aligned piece holds bases of
    two or three records that different lanes, waves and workgroups rewrite"""
    records = [(b"%d" % (i % 10), bytes([M.MODES["d"][0]]) * (1 + (i * 7) % 4)) for i in range(60000)]
    blk = M.Block(records, "d")
    ix = Indexed(engine, records)
    rc, info, msg = call(engine, ix, "d")
    assert rc == 0 and (info.changed, info.first_to_record, info.irregular) == (blk.total_bases, NO_RECORD, 0), msg
    text, guard = ix.host()
    assert text == blk.rewritten and (guard == SENTINEL).all()


# ---- 2. refusals, the empty call, the first call of a context ---------------------------------------------------------------------------------
def test_abi_refusals_and_the_empty_call(engine):
    name, records, mode = next(b for b in BLOCKS if b[0] == "len_33_fasta_r")
    ix = Indexed(engine, records)
    before = ix.host()[0]
    for kw, frag in ((dict(frm=ord("T"), to=ord("T")), "'T' to 'U'"), (dict(frm=ord("A"), to=ord("U")), "'T' to 'U'"), (dict(frm=ord("u"), to=ord("t")), "'T' to 'U'"),
                     (dict(lpr=3), "lines_per_record 3"), (dict(lpr=0), "lines_per_record 0"), (dict(text=False), "null pointer"), (dict(line=False), "null pointer"),
                     (dict(records=ix.n + 1), "need more than"), (dict(records=ix.text_len), "more than")):
        rc, info, msg = call(engine, ix, mode, **kw)
        assert rc == -1 and frag in msg, (kw, msg)
        assert (info.changed, info.first_to_record, info.irregular) == (0, NO_RECORD, 0) and ix.host()[0] == before, kw
    for kw in (dict(records=0), dict(records=0, text=False, line=False)):
        rc, info, msg = call(engine, ix, mode, **kw)
        assert rc == 0 and (info.changed, info.first_to_record, info.irregular) == (0, NO_RECORD, 0) and ix.host()[0] == before, kw


def test_abi_first_call_of_a_new_context(engine):
    """the entry needs no call before it: a context that has seen nothing changes a block another context indexed; a refused call comes first"""
    from fastx_toolkit_amd import Engine
    name, records, mode = next(b for b in BLOCKS if b[0] == "shared_mixed_d")
    blk = M.Block(records, mode)
    ix = Indexed(engine, records)
    fresh = Engine(0)
    try:
        rc, info, msg = call(engine, ix, mode, lpr=3, ctx_of=fresh)
        assert rc == -1 and "lines_per_record 3" in msg
        rc, info, msg = call(engine, ix, mode, ctx_of=fresh)
        assert rc == 0 and (info.changed, info.first_to_record, info.irregular) == (blk.changed, blk.first_to, 0), msg
        assert ix.host()[0] == blk.rewritten
    finally:
        fresh.close()


def test_engine_binding(engine):
    name, records, mode = next(b for b in BLOCKS if b[0] == "len_150_fastq_d")
    blk = M.Block(records, mode)
    ix = Indexed(engine, records)
    info = engine.bases_change(ix.d_text, ix.text_len, ix.ix, ix.n, rna_to_dna=True)
    assert (info.changed, info.first_to_record, info.irregular) == (blk.changed, NO_RECORD, 0)
    assert ix.host()[0] == blk.rewritten


# ---- 3. offsets past 2^31 -----------------------------------------------------------------------------------------------------------------
def test_abi_block_past_2_31_bytes(engine):
    """8 388 680 records of 256 bytes: the text ends 18 KiB past 2^31, so the last 72 records' lines lie at offsets a signed 32-bit integer does not
    hold.  The block is one record repeated on the device (the generators of tests/large_text.py make distinct records, at several times the
    cost, and a repeated record shows a wrong offset just as well: every position of the whole text is compared), with the last three records
    made different by hand."""
    tc = engine.torch
    free, _ = tc.cuda.mem_get_info()
    if free < 12 << 30:
        pytest.skip("needs 12 GB of free device memory, %d MB are free" % (free >> 20))
    n = (1 << 23) + 72
    rec = b">r\n" + (b"ACGTTGCANT" * 26)[:252] + b"\n"
    assert len(rec) == 256
    tails = [b">r\n" + b"T" * 252 + b"\n", b">r\n" + b"T" + b"G" * 250 + b"T" + b"\n", b">r\n" + b"C" * 251 + b"T" + b"\n"]
    one = tc.frombuffer(bytearray(rec), dtype=tc.uint8).to(engine.device)
    d_text = tc.empty(n * 256 + 16, dtype=tc.uint8, device=engine.device)
    d_text[:n * 256].view(n, 256)[:] = one
    d_text[n * 256:] = SENTINEL
    tail = tc.frombuffer(bytearray(b"".join(tails)), dtype=tc.uint8).to(engine.device)
    d_text[(n - 3) * 256:n * 256] = tail
    text_len = n * 256
    assert text_len > (1 << 31) + 256 * 3
    ix, lens, info = engine.fastq_index(d_text, text_len, True, cap_records=n, fasta=True)
    assert info.records == n and not info.irregular

    class V:
        pass
    v = V()
    v.d_text, v.text_len, v.lpr, v.ix, v.n = d_text, text_len, 2, ix, n
    rc, ci, msg = call(engine, v, "r")
    assert rc == 0, msg
    per = rec.count(b"T")
    assert (ci.changed, ci.first_to_record, ci.irregular) == ((n - 3) * per + 252 + 2 + 1, NO_RECORD, 0)
    want_one = tc.frombuffer(bytearray(rec[:3] + rec[3:].replace(b"T", b"U")), dtype=tc.uint8).to(engine.device)
    assert bool((d_text[:(n - 3) * 256].view(n - 3, 256) == want_one).all())
    got = d_text[(n - 3) * 256:].cpu().numpy()
    assert got[:768].tobytes() == b"".join(t[:3] + t[3:].replace(b"T", b"U") for t in tails)
    assert (got[768:] == SENTINEL).all()


# ---- 4. the tool on the GPU build ---------------------------------------------------------------------------------------------------------
def test_tool_has_its_device_path(engine):
    """the product library exports the entry and the tool refers to it, so the tool tests below run the device path (run_tool takes
    FXH_HOST_PARSE out of the environment); without the symbol the record path would give the same bytes"""
    import subprocess
    from nucchange_cases import TOOL
    assert hasattr(engine.lib, "fxg_bases_change")
    syms = subprocess.run(["nm", "-D", TOOL], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert any(l.split()[-1] == "fxg_bases_change" and l.split()[-2] in ("w", "W", "U") for l in syms.splitlines() if l.strip())
    text = regular_text(1 << 16, "r")
    code, out, err, _ = run_tool(None, ["-r"], text, {"FXH_TIMING": "1"})
    assert code == 0 and out == M.change_whole(text, "r")[0]


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_tool_recorded_case(case):
    assert_tool_case(None, case, ONE_MB)


def test_tool_galaxy_pairs():
    for mode, src, want in galaxy_pairs():
        assert run_tool(None, ["-" + mode], src)[:2] == (0, want)
        code, out, err, outfile = run_tool(None, ["-v", "-" + mode], src, files=True)
        assert (code, outfile, err, out) == (0, want, "", M.report(mode, *M.change_whole(src, mode)[3:]))


@pytest.mark.parametrize("mode,fmt", [("r", "fasta"), ("d", "fasta"), ("r", "fastq"), ("d", "fastq")])
def test_tool_many_blocks(mode, fmt):
    """2 MB in 1 MB blocks against the model, report included; then with an offender in the second block: the records before it are written, the
    message carries the line number of the whole input; then with a read one base too long for the device in the second block, which hands the
    rest of the input to the record API"""
    text = regular_text(2 << 20, mode, fmt)
    want, status, _, rin, rout, changed = M.change_whole(text, mode)
    code, out, err, _ = run_tool(None, ["-v", "-" + mode], text, ONE_MB)
    assert code == 0, err
    assert out == want and err.encode() == M.report(mode, rin, rout, changed)
    frm, to = bytes([M.MODES[mode][0]]), bytes([M.MODES[mode][1]])
    cut = text.rfind(b"\n>" if fmt == "fasta" else b"\n@", 0, len(text) * 3 // 4) + 1
    tail = (b">bad\nAC" + to + b"G\n>after\nAC\n") if fmt == "fasta" else (b"@bad\nAC" + to + b"G\n+\nIIII\n@after\nAC\n+\nII\n")
    bad = text[:cut] + tail + text[cut:]
    code, out, err, _ = run_tool(None, ["-v", "-" + mode], bad, ONE_MB)
    assert (code, out) == (1, M.change_whole(text[:cut], mode)[0])
    assert message_of(err) == M.offender_message(mode, text[:cut].count(b"\n") + (2 if fmt == "fasta" else 4)) and err.count("\n") == 1
    bases = (b"ACG" + frm + frm) * 5000
    long_read = (b">long-5\n" + bases[:24998] + b"\n") if fmt == "fasta" else (b"@long\n" + bases[:24998] + b"\n+\n" + b"I" * 24998 + b"\n")
    whole = text[:cut] + long_read + text[cut:]
    want, status, _, rin, rout, changed = M.change_whole(whole, mode)
    code, out, err, _ = run_tool(None, ["-v", "-" + mode], whole, ONE_MB)
    assert (status, code, out) == (0, 0, want), err
    assert err.encode() == M.report(mode, rin, rout, changed)

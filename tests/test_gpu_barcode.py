"""fastx_barcode_splitter on the MI355X: the C-ABI (fxg_barcode_prepare / fxg_barcode_split) against the Python model on random blocks, inside
poison and canaries; the tool on the recorded goldens, across lanes, devices and block sizes, on its error paths and limits; and one large run
against the vectorised model.  Reads tests/golden only."""
import os
import random

import numpy as np
import pytest

import bcsplit_model as M
from bcsplit_cases import assert_tool_case, golden_cases, make_block, make_table, model_run, run_tool

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "fastx_toolkit_amd")
POISON, CANARY = 0x5A, 0xA5


def upload(eng, data, off=0):
    """the block in device memory at byte offset `off` of its allocation, followed by 16 bytes of poison (read-only slack of the contract)"""
    t = eng.torch.full((off + len(data) + 16,), POISON, dtype=eng.torch.uint8, device=eng.device)
    if data:
        t[off:off + len(data)] = eng.torch.frombuffer(bytearray(data), dtype=eng.torch.uint8).to(eng.device)
    return t[off:]


def device_split(eng, data, lpr, ents, BL, mm, eol, bins, out_off=0):
    n_lines = data.count(b"\n")
    n = n_lines // lpr
    d = upload(eng, data, off=4 * random.Random(len(data)).randint(0, 3))
    ix, _, info = eng.fastq_index(d, len(data), cap_records=n + 2, fasta=(lpr == 2))
    assert info.records == n
    eng.barcode_prepare(ents, BL, bins, mismatches=mm, eol=eol)
    total = int(ix.starts[lpr * n].item()) if n else 0
    guard = 64
    buf = eng.torch.full((guard + out_off + total + guard,), CANARY, dtype=eng.torch.uint8, device=eng.device)
    out = buf[guard + out_off:]
    rbuf = eng.torch.full((n + 64,), -0x5A5B, dtype=eng.torch.int16, device=eng.device)
    eng._after_torch()
    import ctypes as C
    bb, br = (C.c_uint64 * (bins + 8))(*([0xC0FFEE] * (bins + 8))), (C.c_uint64 * (bins + 8))(*([0xC0FFEE] * (bins + 8)))
    eng._check(eng.lib.fxg_barcode_split(eng.ctx, d.data_ptr(), len(data), lpr, ix.line.data_ptr(), ix.cap_lines, n, rbuf.data_ptr(),
                                         out.data_ptr(), bb, br))
    host = buf.cpu().numpy()
    assert (host[:guard + out_off] == CANARY).all() and (host[guard + out_off + total:] == CANARY).all(), "write outside d_out"
    rb = rbuf.cpu().numpy()
    assert (rb[n:] == -0x5A5B).all(), "write outside d_rec_bin"
    assert list(bb)[bins:] == [0xC0FFEE] * 8 and list(br)[bins:] == [0xC0FFEE] * 8, "write outside the totals"
    return rb[:n].astype(np.int64), np.array(list(bb)[:bins], dtype=np.uint64), np.array(list(br)[:bins], dtype=np.uint64), host[guard + out_off:guard + out_off + total].tobytes()


def check_block(eng, rng, n, BL, bins, partial, lpr, eol, special=None):
    mm = min(rng.randint(0, 3), BL - 1) if BL > 0 else 0
    partial = min(partial, mm)
    if bins == 4096:
        ents = []
        for j in range(4095):
            b = bytes(rng.choice(b"ACGT") for _ in range(BL))
            ents.append((b, j))
        ents.append((ents[0][0], 4095))
    else:
        ents = make_table(rng, BL, bins, partial, eol)
    if special == "one_bin" and ents:
        ents = [(ents[0][0], ents[0][1])]
        mm = BL - 1 if BL > 1 else 0
    data = make_block(rng, n, lpr, BL, ents, long_every=(n // 2 or 1) if special == "long" else 0)
    if special == "empty":
        data = b"".join((b"@e\n\n+\n\n" if lpr == 4 else b">e\n\n") for _ in range(n))
    want = M.split_block(data, lpr, [b for b, _ in ents], [j for _, j in ents], BL, mm, eol, bins)
    got = device_split(eng, data, lpr, ents, BL, mm, eol, bins, out_off=rng.randint(0, 17))
    ctx = (n, BL, bins, partial, lpr, eol, special)
    assert np.array_equal(got[0], want[0]), ctx
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), ctx
    assert got[3] == want[3], ctx


def test_abi_random_blocks(engine):
    """2 000+ random blocks: 1 / 2 / 97 / 4 096 bins, barcodes of 1..64 bases, partial 0..3, 1 / tile - 1 / tile / tile + 1 / many tiles of
    records, CR / NUL / lower case in the reads"""
    rng = random.Random(2026)
    count = 0
    for k in range(2000):
        bins = rng.choice([1, 2, 2, 97, 97, 5])
        BL = rng.randint(1, 64)
        n = rng.choice([1, 255, 256, 257, 3, 40, 1000, 2600])
        check_block(engine, rng, n, BL, bins, rng.randint(0, 3), rng.choice([2, 4]), rng.random() < 0.5)
        count += 1
    for bins in (1, 2, 97, 4096):
        for BL in (1, 8, 33, 64):
            check_block(engine, rng, 700, BL, bins, 0, 4, bins % 2 == 0)
            count += 1
    assert count >= 2000


@pytest.mark.parametrize("special", ["one_bin", "empty", "long"])
def test_abi_special_blocks(engine, special):
    rng = random.Random(hash(special) & 0xFFFF)
    for n in (1, 255, 256, 257, 3000):
        for lpr in (2, 4):
            check_block(engine, rng, n if special != "long" else min(n, 300), rng.choice([4, 8, 64]), rng.choice([2, 97]), 1, lpr, n % 2 == 0, special)


def test_abi_no_records_and_no_table(engine):
    rng = random.Random(3)
    check_block(engine, rng, 0, 8, 3, 0, 4, False)
    data = make_block(rng, 300, 2, 8, [])
    want = M.split_block(data, 2, [], [], 0, 0, False, 1)
    got = device_split(engine, data, 2, [], 0, 0, False, 1)
    assert np.array_equal(got[0], want[0]) and got[3] == want[3] and list(got[2]) == [300]


def test_abi_rejects_bad_tables(engine):
    from fastx_toolkit_amd.engine import FxgError
    for ents, BL, bins in [([(b"ACGN", 0)], 4, 2), ([(b"ACGT", 2)], 4, 2), ([(b"ACGTA", 0)], 4, 2), ([(b"A" * 65, 0)], 65, 2), ([], 1, 4097), ([], 1, 0)]:
        with pytest.raises(FxgError):
            engine.barcode_prepare(ents, BL, bins)


def test_large_block_96_barcodes(engine):
    """4 M reads of 150 bases, 96 barcodes of eight bases at the read's start (--mismatches 1): equal to the vectorised model"""
    torch = engine.torch
    rs = np.random.default_rng(11)
    n, L, BL = 4_000_000, 150, 8
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    codes = acgt[rs.integers(0, 4, size=(96, BL))]
    seq = acgt[rs.integers(0, 4, size=(n, L))]
    pick = rs.integers(0, 96, size=n)
    has = rs.random(n) < 0.85
    seq[has, :BL] = codes[pick[has]]
    mut = rs.random(n) < 0.3
    pos = rs.integers(0, BL, size=n)
    seq[mut, pos[mut]] = acgt[rs.integers(0, 4, size=int(mut.sum()))]
    rec = np.empty((n, 3 + L + 3 + L + 1), dtype=np.uint8)
    rec[:, 0:3] = np.frombuffer(b"@r\n", dtype=np.uint8)
    rec[:, 3:3 + L] = seq
    rec[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    rec[:, 6 + L:6 + 2 * L] = ord("I")
    rec[:, -1] = 10
    data_np = rec.reshape(-1)
    d = torch.empty(len(data_np) + 16, dtype=torch.uint8, device=engine.device)
    d[:len(data_np)] = torch.from_numpy(data_np).to(engine.device)
    ix, _, info = engine.fastq_index(d, len(data_np), cap_records=n + 2)
    assert info.records == n
    ents = [(bytes(c), j) for j, c in enumerate(codes)]
    engine.barcode_prepare(ents, BL, 97, mismatches=1, eol=False)
    out, bb, br, rb = engine.barcode_split(d, len(data_np), ix, n)
    want = M.classify(seq[:, :BL], np.full(n, BL), codes, np.full(96, BL), np.arange(96), BL, 1, 96)
    got = rb.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, want)
    assert np.array_equal(br, np.bincount(want, minlength=97).astype(np.uint64))
    assert np.array_equal(bb, (np.bincount(want, minlength=97) * rec.shape[1]).astype(np.uint64))
    order = np.argsort(want, kind="stable")
    assert np.array_equal(out.cpu().numpy(), rec[order].reshape(-1))


# ---- the tool on the real engine -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_cli_goldens(case):
    assert_tool_case(run_tool(None, case["argv"], case["barcodes"], case["stdin"]), case)


def test_cli_galaxy_counts():
    c = next(c for c in golden_cases() if c["name"] == "galaxy")
    code, out, err, files = run_tool(None, c["argv"], c["barcodes"], c["stdin"])
    assert code == 0, err
    assert out.splitlines()[1:] == ["BC1\t11\t{P}BC1", "BC2\t12\t{P}BC2", "BC3\t9\t{P}BC3", "BC4\t1\t{P}BC4", "unmatched\t9\t{P}unmatched", "total\t42"]
    assert files == c["files"]


def test_cli_script_name():
    c = next(c for c in golden_cases() if c["name"] == "galaxy")
    tool = os.path.join(ROOT, "fastx_toolkit_amd", "host", "bin", "fastx_barcode_splitter.pl")
    assert_tool_case(run_tool(None, c["argv"], c["barcodes"], c["stdin"], tool=tool), c)


def test_cli_lanes_devices_blocks_invariance():
    rng = random.Random(9)
    ents = make_table(rng, 8, 12, 1, True)
    bc = "".join("id%d %s\n" % (j, b.decode()) for b, j in ents[::2])
    data = make_block(rng, 40000, 4, 8, ents, long_every=13001).decode("latin-1")
    argv = ["--bcfile", "{B}", "--prefix", "{P}", "--suffix", ".fq", "--eol", "--partial", "1", "--mismatches", "2"]
    o = model_run(argv, bc, data)
    want_files = {k[3:].decode(): v.decode("latin-1") for k, v in o.files.items()}
    for env in ({}, {"FXH_LANES": "1"}, {"FXH_LANES": "3", "FXH_READ_BUFFER_MB": "1"}, {"FXG_DEVICES": "0,0", "FXH_READ_BUFFER_MB": "2"},
                {"FXH_LANES": "2", "FXH_READ_BUFFER_MB": "16"}):
        code, out, err, files = run_tool(None, argv, bc, data, env)
        assert code == 0, (env, err)
        assert out == o.stdout.decode().replace("/o/", "{P}"), env
        assert files == want_files, env


def test_cli_limits_and_errors():
    code, _, err, files = run_tool(None, ["--bcfile", "{B}", "--prefix", "{P}", "--bol"], "A %s\n" % ("ACGT" * 17), ">a\nACGT\n")
    assert code != 0 and "longer than 64" in err[-1] and files == {}
    code, _, err, files = run_tool(None, ["--bcfile", "{B}", "--prefix", "{P}", "--bol"], "".join("i%d ACGTACGT\n" % k for k in range(4096)), ">a\nA\n")
    assert code != 0 and "at most 4095" in err[-1] and files == {}
    code, out, err, files = run_tool(None, ["--bcfile", "{B}", "--prefix", "{P}", "--bol"], "".join("i%d ACGTACGT\n" % k for k in range(4095)),
                                     ">a\nACGTACGT\n>b\nTTTTTTTT\n")
    assert code == 0 and len(files) == 4096 and files["i0"] == ">a\nACGTACGT\n" and files["unmatched"] == ">b\nTTTTTTTT\n"
    code, _, err, files = run_tool(None, ["--bcfile", "{B}", "--prefix", "{P}nodir/", "--bol"], "A ACGT\n", ">a\nACGT\n")
    assert code != 0 and err[-1].startswith("Error: failed to create output file ({P}nodir/")

"""fastx_collapser, CPU tier: the Python model (collapse_model.py) against the recorded answers of the reference and, where the reference tree
is present, against the reference itself on seeded random inputs; the hash against std::hash<std::string> and the host replay against the
recorded order; the engine's host half and the kernels' bodies through the CPU emulator (tests/emu/collapse_emu.cpp) on every shared case, with
the caller's arrays against guard pages; the tool over a stub variant that has the entries; and the emulator as a stand-alone program under
ASan + UBSan."""
import ctypes as C
import hashlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import collapse_cases as K
import collapse_model as M
import emu_py

ROOT = K.ROOT
REF = os.environ.get("FXG_REFERENCE", "/root/reference")
REF_SRC = os.path.join(REF, "src", "fastx_collapser", "fastx_collapser.cpp")
EMU_DIR = os.path.join(ROOT, "tests", "emu")
CSRC = os.path.join(ROOT, "fastx_toolkit_amd", "csrc")
HOST = os.path.join(ROOT, "fastx_toolkit_amd", "host")
NONE = (1 << 64) - 1
IRR_BASE = 0x10             # FXG_TEXT_IRR_BASE


# ---- the model -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.golden_cli(), ids=lambda c: c["name"])
def test_model_matches_recorded(case):
    argv = [a for a in case["argv"] if a not in ("-o", "OUT")]
    ans = M.run_argv(argv, case["stdin"].encode("latin-1"))
    if ans == M.USAGE:
        assert case["stdout"] == M.USAGE and case["exit"] == 1
        return
    status, seqs, reads, sums = ans
    assert status == case["exit"]
    to_file = "-o" in case["argv"]
    out = (case["outfile"] if to_file else case["stdout"])
    if status != 0:
        assert not out or case["name"] == "unknown_option"          # nothing is written before the last read: an empty -o file, or none
        return
    assert M.check_against(case["stdin"].encode("latin-1"), out.encode("latin-1")) == sums
    assert (case["stdout"] if to_file else case["stderr"]).encode("latin-1") == (M.report(seqs, reads, sums) if "-v" in argv else b"")


def test_recorded_cases_hold_the_contract_corners():
    by = {c["name"]: c for c in K.golden_cli()}
    assert len(by) >= 30
    assert by["count_passes_int"]["stdout"].startswith(">1--294967296\nAC\n")
    assert by["count_passes_int"]["stderr"].endswith("Output: 3 sequences (representing 18446744073414584322 reads)\n")
    assert by["count_equals_2_32"]["stdout"].startswith(">1-0\nAC\n")
    assert by["z_is_ignored"]["stdout"] == by["plain"]["stdout"] and by["fastq"]["stdout"].startswith(">1-2\nACGT\n")
    assert by["error_lower_case_o"]["outfile"] == "" and by["error_empty_input_o"]["outfile"] is None
    assert by["error_empty_input"]["stderr"].startswith("fastx_collapser: Premature End-Of-File")
    assert all(by[n]["exit"] == 1 and by[n]["stdout"] == "" for n in by if n.startswith("error_"))
    assert sum(len(c["stdin"]) + len(c["stdout"]) for c in by.values()) < 100000


def test_model_galaxy_pair():
    """the reference's own Galaxy pair: reproduced by no build in the order of its equal counts, so it is compared without that order; the
    HAVE_CXX11 build's own bytes are recorded beside it"""
    src, want = K.galaxy_pair()
    M.check_against(src, want)
    assert K.expected("galaxy")["len"] == len(want)
    assert M.same_up_to_ties(K.expected("galaxy")["stdout"].encode("latin-1"), want)
    assert not M.same_up_to_ties(want.replace(b">1-", b">9-", 1), want)


def test_model_against_recorded_abi_cases():
    for name, records, fastq, _, _ in K.abi_cases():
        want = K.expected(name)
        sums = M.collapse(records_of_block(records), fastq)
        assert want["len"] == M.out_bytes(sums), name
        if "stdout" in want:
            M.check_against(K.case_text(records, fastq), want["stdout"].encode("latin-1"))


def records_of_block(records):
    return [(M.chomp(n), M.chomp(b)) for n, b in records]


@pytest.fixture(scope="module")
def reference_exe(tmp_path_factory):
    if not os.path.exists(REF_SRC):
        pytest.skip("the reference sources exist in the build container only")
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden", "collapser"))
    import make_collapser_golden as G
    return G.build(REF, str(tmp_path_factory.mktemp("ref_collapser")))


def _random_input(rng, k):
    pool = [bytes(rng.choice(b"ACGTN") for _ in range(rng.choice([1, 2, 8, 16, 30, rng.randint(1, 80)]))) for _ in range(rng.randint(1, 12))]
    recs = []
    for i in range(rng.randint(1, 40)):
        shape = rng.random()
        if shape < 0.5:
            name = b"%d-%d" % (i, rng.choice([1, 1, 2, 3, 17, rng.randint(1, 300), 2000000000]))
        elif shape < 0.7:
            name = bytes(rng.choice(b"ab1 -+\t_9") for _ in range(rng.randint(0, 12)))
        else:
            name = bytes(rng.choice(b"xyz-") for _ in range(rng.randint(0, 4))) + b"-" + bytes(rng.choice(b"0123456789 +-x") for _ in range(rng.randint(0, 3)))
        recs.append((name, rng.choice(pool)))
    eol = b"\r\n" if k % 11 == 3 else b"\n"
    if k % 5 == 1:
        text = b"".join(b"@" + n + eol + b + eol + b"+" + eol + b"I" * len(b) + eol for n, b in recs)
    else:
        text = b"".join(b">" + n + eol + b + eol for n, b in recs)
    if k % 7 == 2:
        text = text[:-len(eol)]                              # no final newline
    if k % 13 == 5:                                          # something the reader refuses, somewhere
        lines = text.split(b"\n")
        at = rng.randrange(len(lines))
        lines[at] = rng.choice([b"", b"acgt", lines[at] + b"x", b"@" + lines[at]])
        text = b"\n".join(lines)
    return text


def test_model_matches_reference_on_random_inputs(reference_exe):
    rng = random.Random(2026)
    for k in range(300):
        text = _random_input(rng, k)
        p = subprocess.run([reference_exe, "-v"], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        status, seqs, reads, sums = M.run_argv(["-v"], text)
        assert p.returncode == status, (k, text[:200], p.stderr)
        if status == 0:
            assert M.check_against(text, p.stdout) == sums, k
            assert p.stderr == M.report(seqs, reads, sums), k
        else:
            assert p.stdout == b"", k


# ---- the emulator ----------------------------------------------------------------------------------------------------------------------
class Opts(C.Structure):
    _fields_ = [("initial_slots", C.c_uint64), ("hash_bits", C.c_uint32)]


class Info(C.Structure):
    _fields_ = [("records", C.c_uint64), ("reads", C.c_uint64), ("uniques", C.c_uint64), ("slots", C.c_uint64), ("rebuilds", C.c_uint64),
                ("first_bad", C.c_uint64), ("out_reads", C.c_uint64), ("out_bytes", C.c_uint64), ("irregular", C.c_uint32)]


class Window(C.Structure):
    _fields_ = [("rank_end", C.c_uint64), ("out_bytes", C.c_uint64)]


def _obj(src, out, flags=()):
    deps = [src, os.path.join(ROOT, "include", "fxg.h"), os.path.join(EMU_DIR, "fxg_stub_ctx.h"), os.path.join(EMU_DIR, "collapse_emu.cpp")] + \
           [os.path.join(CSRC, f) for f in ("fxg_collapse.h", "fxg_text.h", "fxg_barcode.h", "fxg_device.h", "fxg_kernels.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(emu_py._CXX + list(flags) + ["-c", src, "-o", out + ".tmp"])
        os.replace(out + ".tmp", out)
    return out


@pytest.fixture(scope="module")
def cldir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("collapse"))
    emu = _obj(os.path.join(EMU_DIR, "collapse_emu.cpp"), os.path.join(d, "collapse_emu.o"))
    subprocess.check_call(emu_py._LINK + [emu, "-o", os.path.join(d, "libcollapse_emu.so")])
    return d


def _load(cldir):
    L = C.CDLL(os.path.join(cldir, "libcollapse_emu.so"))
    vp, u64 = C.c_void_p, C.c_uint64
    L.fxg_emu_collapse_new.restype = vp
    L.fxg_emu_collapse_free.argtypes = [vp]
    L.fxg_emu_collapse_begin.argtypes = [vp, C.POINTER(Opts), C.c_char_p, C.c_size_t]
    L.fxg_emu_collapse_add.argtypes = [vp, vp, u64, C.c_int, vp, u64, u64, vp, C.POINTER(Info), C.c_char_p, C.c_size_t]
    L.fxg_emu_collapse_order.argtypes = [vp, C.POINTER(Info), C.c_char_p, C.c_size_t]
    L.fxg_emu_collapse_write.argtypes = [vp, u64, u64, vp, C.POINTER(Window), C.c_char_p, C.c_size_t]
    L.fxg_emu_collapse_hash.argtypes, L.fxg_emu_collapse_hash.restype = [vp, C.c_uint32], u64
    L.fxg_emu_collapse_replay.argtypes = [vp, vp, u64, vp, C.POINTER(u64)]
    return L


@pytest.fixture(scope="module")
def clemu(cldir):
    return _load(cldir)


class Indexed:
    """a block of records as fxg_fastq_index leaves it, every array at its contracted size (include/fxg.h): the text plus its 16 bytes of slack,
    lpr * records + 1 line starts and as many chomped ends, records lengths"""

    def __init__(self, records, fastq=False, guard=None):
        text = M.block_text(records, fastq)
        self.lpr = 4 if fastq else 2
        self.n, self.text_len, self.cap_lines = len(records), len(text), self.lpr * len(records) + 1
        self.d_text = emu_py._alloc(len(text) + 16, np.uint8, guard)
        raw = np.frombuffer(text, dtype=np.uint8)
        self.d_text[:len(text)] = raw
        self.d_text[len(text):len(text) + 16] = 0x5A
        starts = np.zeros(self.cap_lines, dtype=np.int64)
        nl = np.flatnonzero(raw == 10)
        starts[1:] = nl + 1
        ends = nl.copy()
        for j in np.flatnonzero(raw == 13):              # chomp: a line ends at its first CR
            i = int(np.searchsorted(nl, j))
            ends[i] = min(ends[i], j)
        self.d_line = emu_py._alloc(2 * self.cap_lines, np.uint32, guard)
        self.d_line[:self.cap_lines] = starts
        self.d_line[self.cap_lines:2 * self.cap_lines - 1] = ends
        self.d_len = emu_py._alloc(max(self.n, 1), np.uint16, guard)
        self.d_len[:self.n] = np.minimum(ends[1::self.lpr] - starts[1:-1:self.lpr], 65535)


class EmuSet:
    """one set of the emulator, with the messages"""

    def __init__(self, L):
        self.L, self.h, self.err = L, L.fxg_emu_collapse_new(), C.create_string_buffer(300)

    def close(self):
        self.L.fxg_emu_collapse_free(self.h)

    @property
    def message(self):
        return self.err.value.decode()

    def begin(self, initial_slots=0, hash_bits=0):
        return self.L.fxg_emu_collapse_begin(self.h, C.byref(Opts(initial_slots, hash_bits)), self.err, 300)

    def add(self, ix, lpr=None, text=True, text_len=None, cap_lines=None, n=None):
        info = Info()
        rc = self.L.fxg_emu_collapse_add(self.h, ix.d_text.ctypes.data if text else None, ix.text_len if text_len is None else text_len, ix.lpr if lpr is None else lpr,
                                         ix.d_line.ctypes.data, ix.cap_lines if cap_lines is None else cap_lines, ix.n if n is None else n, ix.d_len.ctypes.data, C.byref(info),
                                         self.err, 300)
        return rc, info

    def order(self):
        info = Info()
        return self.L.fxg_emu_collapse_order(self.h, C.byref(info), self.err, 300), info

    def write(self, rank_begin, out_cap, guard=None):
        """one window into d_out of exactly out_cap bytes.  Returns (rc, bytes written, window)."""
        d_out = emu_py._tight(np.full(out_cap, 0xEE, dtype=np.uint8), guard) if guard else np.full(out_cap, 0xEE, dtype=np.uint8)
        w = Window()
        rc = self.L.fxg_emu_collapse_write(self.h, rank_begin, out_cap, d_out.ctypes.data if out_cap else None, C.byref(w), self.err, 300)
        assert rc != 0 or (d_out[w.out_bytes:] == 0xEE).all()
        assert rc == 0 or (d_out == 0xEE).all(), "a refused call wrote to d_out"
        return rc, bytes(d_out[:w.out_bytes]), w


def expected_info(blocks, fastq, initial):
    """what the set's info says after the blocks, by the model and the documented growth rule"""
    seen, steps, recs = {}, [], []
    for blk in blocks:
        steps.append((len(seen), len(blk)))
        recs += records_of_block(blk)
        for _, b in records_of_block(blk):
            seen[b] = 1
    sums = M.collapse(recs, fastq)
    slots, rebuilds = K.slots_after(initial, steps)
    reads = sum(M.get_reads_count(n, fastq) for n, _ in recs) & M.M64
    return dict(records=len(recs), reads=reads, uniques=len(sums), slots=slots, rebuilds=rebuilds, out_reads=M.out_reads(sums), out_bytes=M.out_bytes(sums))


def run_blocks(S, blocks, fastq=False, initial=0, hash_bits=0, guard=None, windows=None):
    """begin, the blocks, order, and the whole output in one window of exactly its bytes (or in windows of `windows` bytes).  Returns (out, info)."""
    assert S.begin(initial, hash_bits) == 0, S.message
    for blk in blocks:
        rc, info = S.add(Indexed(blk, fastq, guard))
        assert rc == 0 and info.irregular == 0 and info.first_bad == NONE, S.message
    rc, info = S.order()
    assert rc == 0, S.message
    want = expected_info(blocks, fastq, initial)
    assert {k: getattr(info, k) for k in want} == want
    out, rank = b"", 0
    while rank < info.uniques:
        rc, got, w = S.write(rank, windows or info.out_bytes, guard)
        assert rc == 0 and w.rank_end > rank, S.message
        out, rank = out + got, w.rank_end
    assert len(out) == info.out_bytes
    rc, got, w = S.write(info.uniques, 0)                  # the empty call
    assert (rc, got, w.rank_end, w.out_bytes) == (0, b"", info.uniques, 0)
    return out, info


def _variants():
    for name, records, fastq, ways, opts in K.abi_cases():
        for w in ways:
            for initial, bits in opts:
                yield pytest.param(name, records, fastq, w, initial, bits, id="%s-%dblocks-slots%d-bits%d" % (name, w, initial, bits))


def test_hash_is_std_hash_of_this_libstdcxx(tmp_path, clemu):
    """the pin of the order contract: fxg_cl_hash against std::hash<std::string> in a stand-alone program, at every length 0 .. 64, long ones,
    every alignment; and the emulator's export gives the same numbers.  A failure here on some machine is a finding about that machine's
    libstdc++, to be reported, not worked round."""
    exe = str(tmp_path / "collapse_hash")
    subprocess.check_call(["hipcc", "--cuda-host-only", "-O1", "-std=c++17", "-Wno-pass-failed", "-DFXG_HOST_EMULATION", os.path.join(EMU_DIR, "collapse_san_main.cpp"), "-o", exe])
    p = subprocess.run([exe, "hash"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert p.returncode == 0, p.stderr.decode()
    rows = [ln.split() for ln in p.stdout.decode().splitlines()]
    assert [int(n) for n, _ in rows][:65] == list(range(65)) and len(rows) >= 70
    for n, h in rows:
        n = int(n)
        s = bytes(b"ACGTN"[(i * 7 + n + i // 5) % 5] for i in range(n))
        buf = np.frombuffer(s + b"\0" * 8, dtype=np.uint8).copy()
        assert clemu.fxg_emu_collapse_hash(buf.ctypes.data, n) == int(h, 16), n


def test_host_replay_gives_the_recorded_order(clemu):
    """the replay alone, without the kernels: hash and count per distinct sequence in first-occurrence order in, the permutation out, and the
    output in that order is the reference's recorded one -- every case, the rehash sizes of libstdc++ among them"""
    u64 = np.uint64
    cases = [(n, records_of_block(r), f) for n, r, f, _, _ in K.abi_cases()] + [("growth", records_of_block(K.growth_case()[0]), False)]
    for name, recs, fastq in cases:
        sums = M.collapse(recs, fastq)
        keys = list(sums)
        hashes = np.array([clemu.fxg_emu_collapse_hash(np.frombuffer(k + b"\0" * 8, dtype=np.uint8).copy().ctypes.data, len(k)) for k in keys], dtype=u64)
        counts = np.array([sums[k] for k in keys], dtype=u64)
        perm, total = np.zeros(len(keys), dtype=u64), C.c_uint64()
        clemu.fxg_emu_collapse_replay(hashes.ctypes.data, counts.ctypes.data, len(keys), perm.ctypes.data, C.byref(total))
        assert sorted(perm.tolist()) == list(range(len(keys))), name
        K.assert_output(name, M.output_in_order(sums, [keys[int(u)] for u in perm]))
        assert total.value == M.out_reads(sums), name


@pytest.mark.parametrize("name,records,fastq,ways,initial,bits", _variants())
def test_emulated_cases(clemu, name, records, fastq, ways, initial, bits):
    S = EmuSet(clemu)
    try:
        out, _ = run_blocks(S, K.split(records, ways), fastq, initial, bits)
        K.assert_output(name, out)
        out2, _ = run_blocks(S, K.split(records, ways), fastq, initial, bits, windows=max(len(out) // 3, max(len(b) for _, b in records) + 40))      # begin resets everything
        assert out2 == out
    finally:
        S.close()


def test_emulated_growth_from_four_slots(clemu):
    """4 slots growing to 4 096: ten doublings, one rebuild per block from the third block on"""
    records, sizes = K.growth_case()
    S = EmuSet(clemu)
    out, info = run_blocks(S, K.split_sizes(records, sizes), initial=4)
    K.assert_output("growth", out)
    assert (info.slots, info.rebuilds, info.uniques) == (4096, 10, 2048)
    S.close()


@pytest.mark.parametrize("name,records,sizes", K.threshold_cases(), ids=[c[0] for c in K.threshold_cases()])
def test_emulated_growth_threshold(clemu, name, records, sizes):
    S = EmuSet(clemu)
    out, info = run_blocks(S, K.split_sizes(records, sizes), initial=64)
    K.assert_output(name, out)
    assert (info.slots, info.rebuilds) == {31: (128, 1), 32: (128, 1), 33: (128, 1)}[sizes[0]]      # 2 x 31, 2 x 32 fit 64 slots, 2 x 33 do not; the second block of 3 then needs 2 x (n + 3)
    S.close()


def test_emulated_growth_threshold_first_block_alone(clemu):
    for n, want in ((31, (64, 0)), (32, (64, 0)), (33, (128, 1))):
        S = EmuSet(clemu)
        _, info = run_blocks(S, [[(K.ident(i), K.seq(i, 24)) for i in range(n)]], initial=64)
        assert (info.slots, info.rebuilds) == want
        S.close()


def test_emulated_windows_after_every_record(clemu):
    """an out_cap that ends a window after every record of a small case in turn, and one byte less, which ends it a record earlier"""
    name = "ties"
    records = [c for c in K.abi_cases() if c[0] == name][0][1]
    S = EmuSet(clemu)
    whole, info = run_blocks(S, [records])
    recs = M.parse_output(whole)
    sizes = [len(M.record_text(r, c, b)) for r, c, b in recs]
    assert sum(sizes) == len(whole)
    for k in range(1, len(sizes) + 1):
        rc, got, w = S.write(0, sum(sizes[:k]))
        assert (rc, w.rank_end, got) == (0, k, whole[:sum(sizes[:k])]), k
        rc, got, w = S.write(0, sum(sizes[:k]) - 1)
        if k == 1:
            assert rc == -1 and "rank 0 needs %d bytes, d_out takes %d" % (sizes[0], sizes[0] - 1) in S.message
        else:
            assert (rc, w.rank_end, got) == (0, k - 1, whole[:sum(sizes[:k - 1])]), k
        rc, got, w = S.write(k - 1, sizes[k - 1])          # one record, from its own rank
        assert (rc, w.rank_end, got) == (0, k, whole[sum(sizes[:k - 1]):sum(sizes[:k])]), k
    S.close()


@pytest.mark.parametrize("name,records", K.irregular_blocks(), ids=[b[0] for b in K.irregular_blocks()])
def test_emulated_irregular_block_leaves_the_set_as_it_was(clemu, name, records):
    good = [(K.ident(i), K.seq(i % 5, 33)) for i in range(300)]
    bad_at = M.block_irregular(records)
    S = EmuSet(clemu)
    want, want_info = run_blocks(S, [good[:100], good[100:]])
    assert S.begin() == 0
    rc, info = S.add(Indexed(records))                     # the first call on an empty set
    assert (rc, info.irregular, info.first_bad, info.records, info.uniques) == (0, IRR_BASE, bad_at, 0, 0), S.message
    rc, info = S.add(Indexed(good[:100]))
    assert rc == 0 and info.irregular == 0 and info.records == 100
    rc, info = S.add(Indexed(records))
    assert (rc, info.irregular, info.first_bad, info.records, info.reads) == (0, IRR_BASE, bad_at, 100, 100), S.message
    rc, info = S.add(Indexed(good[100:]))
    assert rc == 0 and info.irregular == 0
    rc, info = S.order()
    assert rc == 0 and all(getattr(info, k) == getattr(want_info, k) for k in ("records", "reads", "uniques", "out_reads", "out_bytes"))
    rc, got, _ = S.write(0, info.out_bytes)
    assert rc == 0 and got == want
    S.close()


def test_emulated_refusals(clemu):
    """the refusal table: the code and the text, the set and d_out untouched"""
    recs = [(K.ident(i), K.seq(i, 20)) for i in range(10)]
    ix = Indexed(recs)
    said = {}
    S = EmuSet(clemu)
    said["add_before_begin"] = (S.add(ix)[0], S.message)
    said["order_before_begin"] = (S.order()[0], S.message)
    said["write_before_begin"] = (S.write(0, 100)[0], S.message)
    said["hash_bits_65"] = (S.begin(0, 65), S.message)
    assert S.begin() == 0
    said["write_before_order"] = (S.write(0, 100)[0], S.message)
    said["lines_per_record_3"] = (S.add(ix, lpr=3)[0], S.message)
    said["null_text"] = (S.add(ix, text=False)[0], S.message)
    said["too_many_lines"] = (S.add(ix, cap_lines=20)[0], S.message)
    said["text_too_long"] = (S.add(ix, text_len=0xFFFFFFF1)[0], S.message)
    said["records_do_not_fit"] = (S.add(ix, text_len=39)[0], S.message)
    rc, info = S.add(ix)
    assert rc == 0 and info.records == 10                  # the refused calls left nothing behind
    rc, info = S.order()
    assert rc == 0 and info.uniques == 10
    said["add_after_order"] = (S.add(ix)[0], S.message)
    said["order_after_order"] = (S.order()[0], S.message)
    said["rank_begin_past_end"] = (S.write(11, 100)[0], S.message)
    first = len(M.parse_output(S.write(0, info.out_bytes)[1])[0][2]) + 6
    said["out_cap_too_small"] = (S.write(0, first - 1)[0], S.message)
    for name, text in K.REFUSALS:
        rc, msg = said[name]
        assert rc == -1 and (text % (first, first - 1) if "%d" in text else text) in msg, (name, rc, msg)
    assert set(said) == {n for n, _ in K.REFUSALS}
    rc, got, w = S.write(0, info.out_bytes)                # the set is still there
    assert rc == 0 and len(got) == info.out_bytes
    S.close()


def test_emulated_seeded_case_in_1mb_blocks(clemu):
    text = K.seeded_text()
    lines = text.split(b"\n")[:-1]
    records = [(lines[i][1:], lines[i + 1]) for i in range(0, len(lines), 2)]
    blocks, at, size = [], 0, 0
    for i, (n, b) in enumerate(records):
        size += len(n) + len(b) + 3
        if size >= 1 << 20:
            blocks.append(records[at:i + 1])
            at, size = i + 1, 0
    blocks.append(records[at:])
    S = EmuSet(clemu)
    assert S.begin() == 0
    for blk in blocks:
        rc, info = S.add(Indexed(blk))
        assert rc == 0 and not info.irregular
    rc, info = S.order()
    assert rc == 0 and info.records == 300000 and info.reads == 300000 and info.out_reads == 300000
    out, rank = [], 0
    while rank < info.uniques:
        rc, got, w = S.write(rank, 1 << 20)
        assert rc == 0
        out.append(got)
        rank = w.rank_end
    K.assert_output("seeded", b"".join(out))
    S.close()


def _guard_child(where, cldir):
    try:
        L = _load(cldir)
        for name, records, fastq, ways, opts in K.abi_cases():
            if len(records) > 2000:
                continue
            S = EmuSet(L)
            out, _ = run_blocks(S, K.split(records, ways[-1]), fastq, opts[-1][0], opts[-1][1], guard=where)
            K.assert_output(name, out)
            S.close()
        for _, records in K.irregular_blocks():
            S = EmuSet(L)
            assert S.begin() == 0
            rc, info = S.add(Indexed(records, guard=where))
            assert rc == 0 and info.irregular
            S.close()
        os._exit(0)
    except AssertionError:
        os._exit(3)
    except BaseException:
        os._exit(4)


@pytest.mark.parametrize("where", ["after", "before"])
def test_emulated_kernels_within_bounds(cldir, where):
    """every array of a call at exactly its contracted size against a PROT_NONE page: a byte touched outside it is a SIGSEGV of the child"""
    import multiprocessing as mp
    p = mp.get_context("fork").Process(target=_guard_child, args=(where, cldir))
    p.start()
    p.join(600)
    assert p.exitcode == 0, "child exit %s (-11: an access outside an array's contract, 3: a wrong result)" % p.exitcode


# ---- the tool over the stubs ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stock_stub():
    from fastx_toolkit_amd import build as b
    d = emu_py.build_stub()
    b.build_engine()
    b.build_host()
    return d


@pytest.fixture(scope="module")
def collapse_stub(cldir, stock_stub):
    """a libfxg.so of the stub's own objects plus the four entries (collapse_stub.cpp over collapse_emu.cpp)"""
    so = _obj(os.path.join(EMU_DIR, "collapse_stub.cpp"), os.path.join(cldir, "collapse_stub.o"))
    d = os.path.join(cldir, "stub")
    os.makedirs(d, exist_ok=True)
    subprocess.check_call(emu_py._LINK + [os.path.join(stock_stub, "fxg_stub.o"), so, os.path.join(cldir, "collapse_emu.o")] + emu_py._emu_objects([]) +
                          ["-o", os.path.join(d, "libfxg.so"), "-ldl"])
    return d


def test_tool_on_recorded_cases(collapse_stub):
    """bytes, reports, messages and statuses of the goldens: an empty -o file on a bad record, none on an empty input, stdin and stdout, -z ignored"""
    for case in K.golden_cli():
        K.assert_tool_case(collapse_stub, case)
    for case in K.golden_cli():                             # and in blocks of 1 MB through files
        if case["exit"] == 0 and "-o" not in case["argv"]:
            code, out, err, outfile = K.run_tool(collapse_stub, case["argv"], case["stdin"].encode("latin-1"), {"FXH_READ_BUFFER_MB": "1"}, files=True)
            assert (code, outfile, err) == (0, case["stdout"].encode("latin-1"), ""), case["name"]
            assert out == case["stderr"].encode("latin-1"), case["name"]          # the report goes to stdout once -o is given


def test_tool_galaxy_pair_and_abi_cases(collapse_stub):
    src, want = K.galaxy_pair()
    code, out, err, _ = K.run_tool(collapse_stub, [], src)
    assert code == 0 and M.same_up_to_ties(out, want), err
    K.assert_output("galaxy", out)
    for name in ("dups", "counts", "fastq", "ties", "uniq_1109", "crlf", "len_24997"):
        _, records, fastq, _, _ = [c for c in K.abi_cases() if c[0] == name][0]
        code, out, err, _ = K.run_tool(collapse_stub, [], K.case_text(records, fastq))
        assert code == 0, (name, err)
        K.assert_output(name, out)


def test_tool_seeded_case_in_1mb_blocks(collapse_stub):
    code, out, err, outfile = K.run_tool(collapse_stub, ["-v"], K.seeded_text(), {"FXH_READ_BUFFER_MB": "1"}, files=True)
    assert code == 0 and err == "", err
    K.assert_output("seeded", outfile)
    assert out.decode().startswith("Input: 300000 sequences (representing 300000 reads)\nOutput: %d sequences (representing 300000 reads)\n" % outfile.count(b">"))


def test_tool_takes_irregular_blocks_through_the_record_api(collapse_stub):
    """a block the device calls irregular and the record API accepts -- NUL bytes, where the reference's C strings end -- is rewritten and added,
    and the blocks after it take the device path again; a block the record API refuses ends the run with its message, the line number in the
    whole input, and nothing written"""
    rng = random.Random(4)
    pool = [bytes(rng.choice(b"ACGT") for _ in range(30)) for _ in range(50)]
    recs = [(b"r%d" % i, rng.choice(pool)) for i in range(60000)]
    fa = lambda rs: b"".join(b">" + n + b"\n" + b + b"\n" for n, b in rs)
    text = fa(recs[:30000]) + b">odd\0-7\n" + pool[0] + b"\0acgt\n" + fa(recs[30000:])
    for env in ({"FXH_READ_BUFFER_MB": "1"}, {}):
        code, out, err, _ = K.run_tool(collapse_stub, ["-v"], text, env)
        assert code == 0, err
        sums = M.check_against(text, out)
        assert err == M.report(60001, 60001, sums).decode()
    bad = fa(recs) + b">bad\nACGTacgt\n" + fa(recs[:10])
    code, out, err, outfile = K.run_tool(collapse_stub, ["-o", "OUT"], bad, {"FXH_READ_BUFFER_MB": "1"})
    assert (code, out, outfile) == (1, b"", b"")
    assert "found invalid nucleotide sequence (ACGTacgt) on line %d" % (2 * 60000 + 2) in err


def test_tool_without_the_entries_says_so(stock_stub):
    code, out, err, _ = K.run_tool(stock_stub, [], b">a\nAC\n")
    assert code == 1 and out == b"" and "no CPU fallback" in err and "fxg_collapse_begin" in err


# ---- a stand-alone program under the sanitizers --------------------------------------------------------------------------------------------
REPORT = (b"ERROR: AddressSanitizer", b"runtime error:", b"ERROR: LeakSanitizer", b"SUMMARY: UndefinedBehaviorSanitizer")


@pytest.mark.sanitizers
def test_emulator_under_sanitizers(tmp_path):
    """collapse_san_main.cpp built with -fsanitize=address,undefined and run directly, nothing preloaded: the hash pin, and every case but the
    largest in every blocking and table option, in windows of three sizes, every array in a heap allocation of exactly its size"""
    exe = str(tmp_path / "collapse_san_main")
    subprocess.check_call(["hipcc", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-Wno-pass-failed", "-DFXG_HOST_EMULATION",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(EMU_DIR, "collapse_san_main.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe, "hash"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    assert p.returncode == 0 and not any(m in p.stderr for m in REPORT), p.stderr[-1500:]
    src = tmp_path / "case.txt"
    checked = 0
    cases = [(n, r, f, w, o) for n, r, f, w, o in K.abi_cases() if len(r) <= 2000] + [("growth", K.growth_case()[0], False, (12,), ((4, 0),))]
    for name, records, fastq, ways, opts in cases:
        src.write_bytes(K.case_text(records, fastq))
        want = K.expected(name)
        for w in ways:
            for initial, bits in opts:
                one = max(len(b) for _, b in records) + 40          # room for the largest record
                for cap in (one, max(one, want["len"] // 2), want["len"] + 5):
                    p = subprocess.run([exe, str(src), "4" if fastq else "2", str(w), str(cap), str(initial), str(bits)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                       timeout=120, env=env)
                    assert not any(m in p.stderr for m in REPORT) and p.returncode != 99, (name, p.stderr[-1500:])
                    assert p.returncode == 0 and hashlib.md5(p.stdout).hexdigest() == want["md5"], (name, w, initial, bits, cap, p.stderr[-300:])
                    checked += 1
    assert checked > 100

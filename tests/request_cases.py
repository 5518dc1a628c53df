"""Requests that the C-ABI refuses before anything is launched or dereferenced, with the code and the fxg_last_error text of each.

One table for both tiers: tests/test_barcode_cpu.py runs it through the emulation stub, tests/test_gpu_requests.py through the real libfxg.so.  The
two run the same checks (the host-only functions of csrc/fxg_plan.h, fxg_stats.h, fxg_text.h and fxg_barcode.h), and this table is what holds them to
that: the texts are literals, so a reworded message, a check that one side lacks or a different code fails here.

Every pointer of a case only has to be non-null and aligned: `s.p` is a zeroed 64-byte buffer in host memory, 64-byte aligned.
"""
import ctypes as C

from fastx_toolkit_amd.engine import FxgBarcodeSet, FxgBatch, FxgOut, FxgTextInfo, make_params

E_INVALID = -1
TOO_LARGE = 0xFFFFFFF1                 # one byte past the largest block of text
MAX_READ_LEN, MAX_BARCODE_BINS = 65535, 4096
vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int

ARGTYPES = {
    "fxg_run_pipeline": [vp, C.POINTER(FxgBatch), vp, C.POINTER(FxgOut)],
    "fxg_run_quality_stats": [vp, C.POINTER(FxgBatch), vp, u32],
    "fxg_fastq_index": [vp, vp, u64, i32, i32, vp, u64, vp, vp, C.POINTER(FxgTextInfo)],
    "fxg_fastq_pack": [vp, vp, u64, i32, vp, u64, vp, u64, u32, i32, vp, vp, C.POINTER(u32)],
    "fxg_fastq_format": [vp, vp, i32, vp, u64, vp, u64, vp, u32, i32, vp, vp, vp, vp, u32, i32, i32, vp, C.POINTER(u64)],
    "fxg_barcode_prepare": [vp, C.POINTER(FxgBarcodeSet)],
    "fxg_barcode_split": [vp, vp, u64, i32, vp, u64, u64, vp, vp, vp, vp],
}


class Session:
    """One context of the library at `path` (a CDLL of its own: the argument types set here are nobody else's) and the few host arrays the cases point at."""

    def __init__(self, path):
        self.lib = L = C.CDLL(path)
        for name, types in ARGTYPES.items():
            getattr(L, name).argtypes = types
        L.fxg_ctx_create.argtypes = [i32, C.POINTER(vp)]
        L.fxg_ctx_destroy.argtypes, L.fxg_ctx_destroy.restype = [vp], None
        L.fxg_last_error.argtypes, L.fxg_last_error.restype = [vp], C.c_char_p
        self.ctx = vp()
        assert L.fxg_ctx_create(0, C.byref(self.ctx)) == 0
        self._raw = (C.c_uint8 * 128)()
        self.p = (C.addressof(self._raw) + 63) & ~63
        self.info, self.word, self.bytes_out = FxgTextInfo(), u32(), u64()
        self.bin_bytes, self.bin_records = (u64 * 2)(), (u64 * 2)()
        self._keep = []

    def close(self):
        self.lib.fxg_ctx_destroy(self.ctx)

    def last_error(self):
        return self.lib.fxg_last_error(self.ctx).decode()

    def batch(self, stride=16, fixed_len=16, n=1):
        return C.byref(FxgBatch(self.p, self.p, None, fixed_len, stride, n))

    def barcodes(self, entries=(), barcode_len=4, bins=2):
        """a fxg_barcode_set of (bases, bin) entries"""
        E = len(entries)
        bases, lens, bins_of = (C.c_uint8 * (64 * max(E, 1)))(), (u32 * max(E, 1))(), (u32 * max(E, 1))()
        for k, (b, j) in enumerate(entries):
            bases[64 * k:64 * k + len(b)] = b
            lens[k], bins_of[k] = len(b), j
        self._keep += [bases, lens, bins_of]
        return C.byref(FxgBarcodeSet(C.addressof(bases), C.addressof(lens), C.addressof(bins_of), E, barcode_len, 0, 0, bins))

    def params(self, stages):
        self._keep.append(make_params(stages=stages))
        return self._keep[-1]

    def table(self, on):
        """leave the context with a (trivial) barcode table, or without one: a refused fxg_barcode_prepare drops what was there"""
        rc = self.lib.fxg_barcode_prepare(self.ctx, self.barcodes(bins=2 if on else 0))
        assert rc == (0 if on else E_INVALID), (rc, self.last_error())

    def split(self, text=None, text_len=64, cap_lines=9, n=2):
        return (text or self.p, text_len, 4, self.p, cap_lines, n, self.p, self.p, self.bin_bytes, self.bin_records)


def _format(s, pk_bases=None, pk_qual=None, pk_off=None, rows_qual=None):
    return (s.p, 4, s.p, 5, s.p, 1, s.p, 0, 0, pk_bases, pk_qual, pk_off, rows_qual, 16, 33, 0, s.p, C.byref(s.bytes_out))


# (name, entry point, arguments after the context as a function of the session, code, fxg_last_error afterwards -- None: the call leaves it as it was)
CASES = [
    ("index_text_too_large", "fxg_fastq_index", lambda s: (s.p, TOO_LARGE, 1, 4, s.p, 9, s.p, s.p, C.byref(s.info)),
     E_INVALID, "text block too large (4294967281 bytes)"),
    ("index_three_lines_per_record", "fxg_fastq_index", lambda s: (s.p, 64, 1, 3, s.p, 9, s.p, s.p, C.byref(s.info)), E_INVALID, None),
    ("pack_fasta_with_qualities", "fxg_fastq_pack", lambda s: (s.p, 64, 2, s.p, 3, s.p, 1, 16, 33, s.p, s.p + 16, C.byref(s.word)),
     E_INVALID, "FASTA records have no qualities"),
    ("pack_misaligned_rows", "fxg_fastq_pack", lambda s: (s.p, 64, 4, s.p, 5, s.p, 1, 16, 33, s.p + 1, s.p + 16, C.byref(s.word)),
     E_INVALID, "row arrays must be 16-byte aligned"),
    ("format_packed_without_out_off", "fxg_fastq_format", lambda s: _format(s, pk_bases=s.p, pk_qual=s.p, rows_qual=s.p),
     E_INVALID, "packed output needs bases, out_off and (FASTQ) qual"),
    ("format_fastq_without_quality_rows", "fxg_fastq_format", lambda s: _format(s),
     E_INVALID, "FASTQ output needs the batch's quality rows (numeric records are printed from them)"),
    ("stats_histogram_too_narrow", "fxg_run_quality_stats", lambda s: (s.batch(), s.p, 15),
     E_INVALID, "quality_stats: histogram has 15 columns, batch stride is 16"),
    ("stats_stride_too_long", "fxg_run_quality_stats", lambda s: (s.batch(stride=MAX_READ_LEN + 1), s.p, MAX_READ_LEN + 1),
     E_INVALID, "quality_stats: bad batch (stride 65536, fixed_len 16)"),
    ("stats_fixed_len_over_stride", "fxg_run_quality_stats", lambda s: (s.batch(fixed_len=17), s.p, 16),
     E_INVALID, "quality_stats: bad batch (stride 16, fixed_len 17)"),
    ("barcodes_no_bins", "fxg_barcode_prepare", lambda s: (s.barcodes(bins=0),), E_INVALID, "barcode split: 0 bins (1 .. 4096)"),
    ("barcodes_too_many_bins", "fxg_barcode_prepare", lambda s: (s.barcodes(bins=MAX_BARCODE_BINS + 1),), E_INVALID, "barcode split: 4097 bins (1 .. 4096)"),
    ("barcodes_entry_too_long", "fxg_barcode_prepare", lambda s: (s.barcodes([(b"ACGTA", 0)]),), E_INVALID, "barcode entry 0: length 5, bin 0"),
    ("barcodes_entry_bin_out_of_range", "fxg_barcode_prepare", lambda s: (s.barcodes([(b"ACGT", 0), (b"ACG", 2)]),), E_INVALID, "barcode entry 1: length 3, bin 2"),
    ("barcodes_entry_with_n", "fxg_barcode_prepare", lambda s: (s.barcodes([(b"ACNT", 0)]),), E_INVALID, "barcode entry 0: a base that is not A, C, G or T"),
    ("split_without_table", "fxg_barcode_split", lambda s: (s.table(False), s.split())[1], E_INVALID, "fxg_barcode_split: no table (fxg_barcode_prepare)"),
    ("split_line_array_one_short", "fxg_barcode_split", lambda s: (s.table(True), s.split(cap_lines=8))[1],
     E_INVALID, "fxg_barcode_split: 2 records need more than 8 lines"),
    ("split_text_at_odd_address", "fxg_barcode_split", lambda s: (s.table(True), s.split(text=s.p + 1))[1],
     E_INVALID, "fxg_barcode_split: the text must be 4-byte aligned"),
    ("split_text_too_large", "fxg_barcode_split", lambda s: (s.table(True), s.split(text_len=TOO_LARGE))[1],
     E_INVALID, "text block too large (4294967281 bytes)"),
    ("pipeline_two_stage_groups", "fxg_run_pipeline", lambda s: (s.batch(), C.addressof(s.params(0x02 | 0x08)), C.byref(FxgOut(res=s.p))),
     E_INVALID, "unsupported stage chain 0xa: use [CLIP][QTRIM][QFILTER], [REVCOMP][FTRIM|FTRIM_END], [MASK], [ARTIFACTS] or [NFILTER]"),
]


def refuse(s, case):
    """runs one case on the session; asserts the code and the text"""
    name, entry, args, code, text = case
    argv = args(s)                                   # (may prepare or drop the barcode table first)
    before = s.last_error()
    rc = getattr(s.lib, entry)(s.ctx, *argv)
    assert rc == code, (name, rc, s.last_error())
    assert s.last_error() == (before if text is None else text), name

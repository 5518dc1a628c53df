"""GPU tier (-m gpu): the state a context carries from one call to the next (struct fxg_ctx, csrc/fxg_host.h) -- the workspaces that only grow, the text
state, the uncollapser's kept scans, the barcode table, the clip history, the remembered last launch, the kernels' LDS attributes -- across call orders,
sizes and contexts.  Every comparison is exact, against the oracle, reflow_model, uncollapse_model, bcsplit_model and the text of the blocks themselves;
outputs sit between canaries, text inputs before poison; every compacting run asserts scan_recoveries() unchanged.

  a  the first call a new context sees, for every entry point that takes a context (context_state_cases.FIRST_CALLS): 0 and the reference's answer, or the
     documented refusal with its code, its text and untouched outputs (the collapser's four entries and fxg_bases_change among them; the set among the
     other families is tests/test_gpu_context_state_collapse.py)
  b  one context, about 150 calls of all families interleaved (context_state_sequence.py), every workspace reallocated at least twice while another
     family's kept data must survive; fb_blk on a context whose launches are all done again without the scanner
  c  one context through all 43 tile kernels, then kernels alternating between two LDS sizes, two contexts alternating, two threads with a context each
"""
import contextlib
import ctypes as C
import threading
import zlib

import numpy as np
import pytest

import bcsplit_model as BM
import context_state_cases as K
import context_state_sequence as S
import reflow_model as RM
import uncollapse_model as UM
from fastx_toolkit_amd.engine import (NCOUNTERS, FxgBatch, FxgError, FxgFormatOpts, FxgOut, FxgReflowInfo, FxgReflowOpts, FxgTextInfo, FxgUncollapseInfo, FxgUncollapseOpts, TextIndex,
                                      format_bound, make_params, reflow_bound)
from helpers import assert_same, oracle_params
from oracle import fxoracle_py as fo
from uncollapse_cases import rec

pytestmark = pytest.mark.gpu

POISON, CANARY, GUARD = 0x5A, 0xA5, 64
E_INVALID = -1


# ---- host data and references (no GPU needed) -------------------------------------------------------------------------------------------------------
_host = {}


def cached(key, make):
    if key not in _host:
        _host[key] = make()
    return _host[key]


def fastq_block(n):
    """n records of S.READ_LEN bases from the oracle's generator, its own parse of them, and the FASTA text of the whole records"""
    def make():
        text = fo.synth_fastq(11 + n % 5, 3 * n, n, S.READ_LEN, False)
        p = fo.parse_fastq(text)
        lines = text.split(b"\n")
        assert p["n"] == n and len(lines) == 4 * n + 1
        fasta = b"".join(b">" + a[1:] + b"\n" + s + b"\n" for a, s in zip(lines[0::4], lines[1::4]))
        return dict(kind="fastq", lpr=4, text=text, n=n, bases=p["bases"], qual=p["qual"], lens=p["lens"], fasta=fasta)
    return cached(("fastq", n), make)


def collapsed_block(n, salt):
    def make():
        records = [rec(i + 100000 * salt, 1 + (i + salt) % 3, 12 + (i * 7 + salt) % 9) for i in range(n)]
        lens = np.array([len(b) for _, b in records], np.uint16)
        bases = np.zeros((n, int(lens.max())), np.uint8)
        for i, (_, b) in enumerate(records):
            bases[i, :len(b)] = np.frombuffer(b, np.uint8)
        return dict(kind="collapsed", lpr=2, text=UM.block_text(records), n=n, records=records, bases=bases, qual=None, lens=lens)
    return cached(("collapsed", n, salt), make)


def fasta_block(n):
    """n two-line records of 20 to 28 bases of collapse_cases.seq (every letter of ACGTN), ids of every width modulo 16"""
    def make():
        import collapse_cases as CK
        records = [(CK.ident(i), CK.seq(i, 20 + i % 9)) for i in range(n)]
        return dict(kind="fasta", lpr=2, text=b"".join(b">" + a + b"\n" + b + b"\n" for a, b in records), n=n, records=records, qual=None,
                    lens=np.array([len(b) for _, b in records], np.uint16))
    return cached(("fasta", n), make)


def block_of(key):
    if key[0] == "wide":                                      # (the unrelated blocks of collapse_state_sequence.py)
        import collapse_state_sequence as Q
        return Q.wide_block(key[1], key[2])
    return fastq_block(key[1]) if key[0] == "fastq" else fasta_block(key[1]) if key[0] == "fasta" else collapsed_block(key[1], key[2])


def line_marks(text, lines):
    """(starts of lines 0 .. lines, ends of lines 0 .. lines - 1) of a block whose lines all end in a newline"""
    nl = np.flatnonzero(np.frombuffer(text, np.uint8) == 10)[:lines]
    return np.concatenate([[0], nl + 1]).astype(np.uint32), nl.astype(np.uint32)


def reflow_text(lines):
    """a multi-line FASTA block of exactly `lines` lines: a header and three sequence lines per record, the third one ragged"""
    def make():
        rng = np.random.default_rng(lines)
        acgt = np.frombuffer(b"ACGTN", np.uint8)
        out = []
        for r in range(lines // S.RF_LINES_PER_RECORD):
            seq = rng.choice(acgt, size=2 * S.RF_LINE + 1 + r % S.RF_LINE).tobytes()
            out.append(b">s%d x\n%s\n%s\n%s\n" % (r, seq[:S.RF_LINE], seq[S.RF_LINE:2 * S.RF_LINE], seq[2 * S.RF_LINE:]))
        return b"".join(out)
    return cached(("reflow", lines), make)


def barcode_table(name):
    def make():
        rng = np.random.default_rng(97)
        n = 96 if name == "t97" else 2
        ents = [(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=S.BC_LEN)), j) for j in range(n)]
        return dict(ents=ents, bins=n + 1, BL=S.BC_LEN, mm=1)
    return cached(("table", name), make)


def split_reference(blk, tab):
    return cached(("split", blk["n"], tab["bins"]),
                  lambda: BM.split_block(blk["text"], 4, [b for b, _ in tab["ents"]], [j for _, j in tab["ents"]], tab["BL"], tab["mm"], False, tab["bins"]))


def pipeline_batch(st):
    """(bases, qual, lens) of a run step: the oracle's generator (adapters planted for the clip families), seeded ragged lengths"""
    f = S.FAM[st["fam"]]

    def make():
        n, stride = st["n"], f["stride"]
        b, q = fo.synth_batch(5 + n % 11, 1000 * n, n, stride, bool(f.get("clip")), stride)
        lens = None
        if st["ragged"]:
            lens = np.random.default_rng(zlib.crc32(st["label"].encode())).integers(1, stride + 1, size=n).astype(np.uint16)
        return b, q, lens
    return cached(("batch", st["fam"], st["n"], st["ragged"], st["label"] if st["ragged"] else ""), make)


def stats_reference(n, stride=100):
    def make():
        b, q = fo.synth_batch(23, 7 * n, n, stride, False, stride)
        qs = fo.QStats()
        qs.add(b, q, None, qoffset=33)
        want = qs.device_layout(stride, 33)
        qs.close()
        return b, q, want
    return cached(("stats", n, stride), make)


# ---- device side ------------------------------------------------------------------------------------------------------------------------------------
class Guards:
    """device arrays of exactly their contracted bytes (rounded up to the 16-byte granule) between two canaries"""

    def __init__(self, eng):
        self.eng, self.held = eng, []

    def alloc(self, nbytes, dtype=None, fill=POISON):
        T = self.eng.torch
        span = (int(nbytes) + 15) // 16 * 16
        buf = T.full((GUARD + span + GUARD,), CANARY, dtype=T.uint8, device=self.eng.device)
        buf[GUARD:GUARD + span] = fill
        self.held.append((buf, span))
        v = buf[GUARD:GUARD + span]
        return v if dtype is None else v.view(dtype)

    def check(self, what):
        for buf, span in self.held:
            assert bool((buf[:GUARD] == CANARY).all()) and bool((buf[GUARD + span:] == CANARY).all()), "%s: a write outside an output array" % (what,)
        self.held = []


def upload_text(eng, text):
    t = eng.torch.full((len(text) + 16,), POISON, dtype=eng.torch.uint8, device=eng.device)
    if text:
        t[:len(text)] = eng.torch.frombuffer(bytearray(text), dtype=eng.torch.uint8).to(eng.device)
    return t


@contextlib.contextmanager
def knobs(monkeypatch, env):
    for k in K.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    try:
        yield
    finally:
        for k in (env or {}):
            monkeypatch.delenv(k, raising=False)


@contextlib.contextmanager
def fresh_engine(monkeypatch, **env):
    """a new Engine(0) under the context knobs `env`; closed afterwards"""
    from fastx_toolkit_amd import Engine
    with knobs(monkeypatch, env):
        eng = Engine(0)
    try:
        yield eng
    finally:
        eng.close()


def last_error(eng):
    return eng.lib.fxg_last_error(eng.ctx).decode(errors="replace")


class Runner:
    """the steps of context_state_sequence.py on one context, each against its reference"""

    def __init__(self, eng, monkeypatch, recoveries_per_run=0):
        self.eng, self.mp, self.g = eng, monkeypatch, Guards(eng)
        self.idx, self.ucs, self.results = {}, {}, {}
        self.table, self.al, self.host_base = None, None, 0
        self.per_run = recoveries_per_run
        self.cus = eng.torch.cuda.get_device_properties(eng.device).multi_processor_count          # (not through the context: its first call is the test's)

    def close(self):
        if self.al is not None:
            fo.aligner_free(self.al)
            self.al = None

    def step(self, st):
        getattr(self, "do_" + st["kind"])(st)
        self.g.check(st["label"])

    # -- the pipeline --
    def do_run(self, st, defer=None):
        eng, T = self.eng, self.eng.torch
        f = S.FAM[st["fam"]]
        b, q, lens = pipeline_batch(st)
        n, stride = b.shape
        fl = None if lens is not None else stride
        o = None if st.get("refused") else fo.run_pipeline(b, q, lens, oracle_params(f["pd"]), fixed_len=fl, aligner=self.al if (f.get("clip") and self.al is not None) else None)
        db, dq = T.from_numpy(b).to(eng.device), T.from_numpy(q).to(eng.device)
        dl = T.from_numpy(lens.astype(np.int16)).to(eng.device) if lens is not None else None
        meta = st["meta"]
        out = dict(res=self.g.alloc(4 * n, T.int32), counters=T.zeros(NCOUNTERS, dtype=T.int64, device=eng.device),
                   out_bases=self.g.alloc(n * stride), out_qual=self.g.alloc(n * stride),
                   out_len=self.g.alloc(2 * n, T.int16)[:n] if meta else None, kept_index=self.g.alloc(4 * n, T.int32)[:n] if meta else None,
                   out_off=self.g.alloc(8 * n, T.int64)[:n] if meta else None)
        out["res"] = out["res"][:n]
        before = eng.scan_recoveries()
        if st.get("refused"):                                 # the documented refusal: code and text, every output as it was, the launch record too
            ll = eng.last_launch()
            with knobs(self.mp, f.get("env")), pytest.raises(FxgError) as err:
                eng.run(db, dq, make_params(**f["pd"]), lens=dl, fixed_len=fl, compact=True, meta=meta, outputs=out)
            assert str(err.value) == "fxg error -1: " + st["refused"], st["label"]
            assert all(bool((out[k] == POISON).all()) for k in ("out_bases", "out_qual")) and bool((out["res"].view(T.uint8) == POISON).all()), st["label"]
            assert not bool(out["counters"].any()) and eng.last_launch() == ll and eng.scan_recoveries() == before, st["label"]
            return ll
        with knobs(self.mp, f.get("env")):
            r = eng.run(db, dq, make_params(**f["pd"]), lens=dl, fixed_len=fl, compact=True, meta=meta, outputs=out)
        ll = eng.last_launch()
        assert ll["kernel"].startswith(f["kernel"]) and ll["tile_reads"] == f["T"], (st["label"], ll)
        self.results[st["label"]] = (r, o, meta, before, (db, dq, dl))
        if st["label"].split(".")[-1] == "run" and st["label"].startswith(("fb.", "fb_blk.")):
            return ll                                         # its counters are read by a later step
        self.finish(st["label"])
        return ll

    def finish(self, label):
        r, o, meta, before, _ = self.results.pop(label)
        h = r.to_host()
        assert self.eng.scan_recoveries() == before + self.per_run, "%s: scan_recoveries moved by %d" % (label, self.eng.scan_recoveries() - before)
        if meta:
            assert_same(o, h, label)
        else:
            assert np.array_equal(o["res"], h["res"]) and np.array_equal(o["counters"][:13], h["counters"][:13]), label
            assert np.array_equal(o["out_bases"], h["out_bases"]) and np.array_equal(o["out_qual"], h["out_qual"]), label + ": packed stream"

    def do_read_counters(self, st):
        self.finish(st["of"])

    def do_history(self, st):
        self.eng.set_clip_history(st["on"])
        self.close()
        if st["on"]:
            self.al = fo.aligner_new()

    def do_stats(self, st, stride=100):
        eng, T = self.eng, self.eng.torch
        b, q, want = stats_reference(st["n"], stride)
        hist = self.g.alloc(stride * 5 * 128 * 8, T.int64, fill=0).view(stride, 5, 128)
        got = eng.quality_stats(T.from_numpy(b).to(eng.device), T.from_numpy(q).to(eng.device), hist=hist)
        assert np.array_equal(got.cpu().numpy().astype(np.uint64), want), st["label"]
        assert eng.last_launch()["grid"] == min(-(-st["n"] // 256), self.cus), st["label"]

    # -- text --
    def do_index(self, st, key=None):
        eng, T = self.eng, self.eng.torch
        key = key or st["block"]
        blk = block_of(key)
        text, n, lpr = blk["text"], blk["n"], blk["lpr"]
        d_text = upload_text(eng, text)
        cap_lines = lpr * n + 1
        line = self.g.alloc(8 * cap_lines, T.int32, fill=0)[:2 * cap_lines]
        lens = self.g.alloc(2 * n, T.int16)[:n]
        flags = self.g.alloc(n, T.uint8, fill=0)[:n]
        info = FxgTextInfo()
        eng._after_torch()
        rc = eng.lib.fxg_fastq_index(eng.ctx, d_text.data_ptr(), len(text), 1, lpr, line.data_ptr(), cap_lines, lens.data_ptr(), flags.data_ptr(), C.byref(info))
        assert rc == 0, (st["label"], last_error(eng))
        assert (info.records, info.consumed, info.irregular) == (n, len(text), 0), st["label"]
        assert (info.max_len, info.min_len) == (int(blk["lens"].max()), int(blk["lens"].min())), st["label"]
        starts, ends = line_marks(text, lpr * n)
        got = line.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:lpr * n + 1], starts) and np.array_equal(got[cap_lines:cap_lines + lpr * n], ends), st["label"] + ": line arrays"
        assert np.array_equal(lens.cpu().numpy().view(np.uint16), blk["lens"]) and not bool(flags.any()), st["label"]
        ix = dict(d_text=d_text, text_len=len(text), ix=TextIndex(line, cap_lines, flags, lpr), lens=lens, blk=blk, n=n, keep=self.g.held)
        self.g.check(st["label"])                            # (the arrays live on: a later step of the block reads them)
        self.idx[key] = ix
        return ix

    def do_pack(self, st):
        eng, T = self.eng, self.eng.torch
        x = self.idx[st["block"]]
        blk, n = x["blk"], x["n"]
        stride = blk["bases"].shape[1]
        bases = self.g.alloc(n * stride)
        qual = self.g.alloc(n * stride) if blk["qual"] is not None else None
        irr = C.c_uint32(77)
        eng._after_torch()
        rc = eng.lib.fxg_fastq_pack(eng.ctx, x["d_text"].data_ptr(), x["text_len"], blk["lpr"], x["ix"].line.data_ptr(), x["ix"].cap_lines, x["ix"].flags.data_ptr(), n, stride, 33,
                                    bases.data_ptr(), qual.data_ptr() if qual is not None else None, C.byref(irr))
        assert (rc, irr.value) == (0, 0), (st["label"], rc, irr.value, last_error(eng))
        inside = np.arange(stride)[None, :] < blk["lens"][:, None].astype(np.int64)
        got = bases[:n * stride].cpu().numpy().reshape(n, stride)
        assert np.array_equal(got[inside], blk["bases"][inside]), st["label"] + ": bases"
        if qual is not None:
            got = qual[:n * stride].cpu().numpy().reshape(n, stride)
            assert np.array_equal(got[inside], blk["qual"][inside]), st["label"] + ": qualities"

    def do_format(self, st):
        """every record whole, as FASTA, from the block's line arrays and lengths (fxg_fastq_format_opts with d_len and no res)"""
        eng = self.eng
        x = self.idx[st["block"]]
        blk, n = x["blk"], x["n"]
        cap = format_bound(x["text_len"], n)
        out = self.g.alloc(cap)
        nb = C.c_uint64(12345)
        o = FxgFormatOpts(0, 0, 0, 0, cap, x["lens"].data_ptr())
        eng._after_torch()
        rc = eng.lib.fxg_fastq_format_opts(eng.ctx, x["d_text"].data_ptr(), 4, x["ix"].line.data_ptr(), x["ix"].cap_lines, x["ix"].flags.data_ptr(), n, None, 0, 0, None, None, None, None,
                                           0, 33, 1, out.data_ptr(), C.byref(nb), C.byref(o))
        assert rc == 0 and nb.value == len(blk["fasta"]), (st["label"], rc, nb.value, last_error(eng))
        host = out.cpu().numpy()
        assert host[:nb.value].tobytes() == blk["fasta"], st["label"]
        assert (host[nb.value:] == POISON).all(), st["label"] + ": a byte behind out_bytes changed"

    def do_reflow(self, st, text=None, at_eof=True, open_in=0):
        eng, T = self.eng, self.eng.torch
        text = reflow_text(st["lines"]) if text is None else text
        want, consumed, open_out = RM.reflow_block(text, at_eof, open_in, width=st["width"])
        d_text = upload_text(eng, text)
        cap_lines = text.count(b"\n") + 2
        line = self.g.alloc(8 * cap_lines, T.int32)[:2 * cap_lines]
        cap = max(reflow_bound(len(text)), 16)
        out = self.g.alloc(cap)
        o, info = FxgReflowOpts(st["width"], 0, 0, cap), FxgReflowInfo()
        eng._after_torch()
        rc = eng.lib.fxg_fasta_reflow(eng.ctx, d_text.data_ptr(), len(text), int(at_eof), open_in, C.byref(o), line.data_ptr(), cap_lines, out.data_ptr(), C.byref(info))
        assert rc == 0, (st["label"], last_error(eng))
        assert (info.out_bytes, info.consumed, info.open_bases) == (len(want), consumed, open_out), st["label"]
        host = out.cpu().numpy()
        assert host[:len(want)].tobytes() == want and (host[len(want):] == POISON).all(), st["label"]

    # -- the uncollapser --
    def uc_call(self, x, base, begin, out, cap):
        eng = self.eng
        o, info = FxgUncollapseOpts(base, begin, cap), FxgUncollapseInfo()
        eng._after_torch()
        rc = eng.lib.fxg_fasta_uncollapse(eng.ctx, x["d_text"].data_ptr(), x["text_len"], x["ix"].line.data_ptr(), x["ix"].cap_lines, x["n"], x["lens"].data_ptr(), C.byref(o),
                                          out.data_ptr() if out is not None else None, C.byref(info))
        return rc, info

    def do_uc(self, st):
        key = st["block"]
        x = self.idx[key]
        if st.get("first"):
            base = self.host_base if st.get("chain") else 1000 * key[2]
            blk = UM.Block(x["blk"]["records"], base)
            whole = blk.whole()
            self.ucs[key] = dict(blk=blk, whole=whole, base=base, g=0, got=[], cap=len(whole) // st["parts"] + 64)
        u = self.ucs[key]
        blk = u["blk"]
        while True:
            want_end, want = blk.window(u["g"], u["cap"])
            out = self.g.alloc(u["cap"])
            rc, info = self.uc_call(x, u["base"], u["g"], out, u["cap"])
            assert rc == 0, (st["label"], last_error(self.eng))
            assert (info.copies, info.copy_end, info.out_bytes) == (blk.copies, want_end, len(want)), (st["label"], u["g"])
            host = out.cpu().numpy()
            assert host[:len(want)].tobytes() == want and (host[len(want):] == POISON).all(), (st["label"], u["g"])
            self.g.check(st["label"])
            u["got"].append(want)
            u["g"] = want_end
            if not st.get("rest") or u["g"] == blk.copies:
                break
        if st.get("rest"):
            assert b"".join(u["got"]) == u["whole"] and u["g"] == blk.copies, st["label"]          # the windows, concatenated, are Block.whole()
            if st.get("chain"):
                self.host_base += blk.copies
        else:
            assert u["g"] < blk.copies, st["label"] + ": the walk ended before its last step"

    # -- the barcode splitter --
    def do_bc_prepare(self, st):
        self.table = barcode_table(st["table"])
        t = self.table
        self.eng.barcode_prepare(t["ents"], t["BL"], t["bins"], mismatches=t["mm"], eol=False)

    def do_bc_split(self, st):
        eng, T = self.eng, self.eng.torch
        x, t = self.idx[st["block"]], self.table
        assert st.get("bins", t["bins"]) == t["bins"]
        blk, n, bins = x["blk"], x["n"], t["bins"]
        rb_want, bb_want, br_want, out_want = split_reference(blk, t)
        out = self.g.alloc(x["text_len"])
        rbin = self.g.alloc(2 * n, T.int16)
        bb, br = (C.c_uint64 * (bins + 8))(*([0xC0FFEE] * (bins + 8))), (C.c_uint64 * (bins + 8))(*([0xC0FFEE] * (bins + 8)))
        eng._after_torch()
        rc = eng.lib.fxg_barcode_split(eng.ctx, x["d_text"].data_ptr(), x["text_len"], 4, x["ix"].line.data_ptr(), x["ix"].cap_lines, n, rbin.data_ptr(), out.data_ptr(), bb, br)
        assert rc == 0, (st["label"], last_error(eng))
        assert list(bb)[bins:] == [0xC0FFEE] * 8 and list(br)[bins:] == [0xC0FFEE] * 8, st["label"] + ": write outside the totals"
        assert np.array_equal(np.array(list(bb)[:bins], np.uint64), bb_want) and np.array_equal(np.array(list(br)[:bins], np.uint64), br_want), st["label"]
        assert np.array_equal(rbin[:n].cpu().numpy().astype(np.int64), rb_want), st["label"] + ": record bins"
        assert out[:x["text_len"]].cpu().numpy().tobytes() == out_want, st["label"] + ": the partition"


# ---- a. the first call on a fresh context -------------------------------------------------------------------------------------------------------------
def expect_refusal(eng, row, rc, untouched=True):
    _, code, text, _ = row
    assert rc == code and last_error(eng) == text and untouched, (rc, last_error(eng))


def _st(kind, label="first", **kw):
    return dict(kind=kind, label=label, **kw)


SMALL_FASTQ, SMALL_COLLAPSED, SMALL_FASTA = ("fastq", 3000), ("collapsed", 3000, 1), ("fasta", 3000)


def first_call(cid, outcome, fresh, other, mp):
    """`fresh`: a Runner on a context that has seen no call; `other`: one on the session's context (whatever the call needs from somebody else)"""
    eng, lib, T = fresh.eng, fresh.eng.lib, fresh.eng.torch
    vp = C.c_void_p
    if cid == "destroy_untouched":
        return                                                # (fresh_engine closes it: fxg_ctx_destroy is its first and only call but the stream's adoption)
    if cid == "last_error_empty":
        assert last_error(eng) == ""
    elif cid == "set_stream":
        assert lib.fxg_set_stream(eng.ctx, None) == 0
        eng.use_torch_stream()
        fresh.do_stats(_st("stats", n=600))
    elif cid == "sync":
        assert lib.fxg_sync(eng.ctx) == 0
    elif cid == "device_info":
        assert eng.device_info() == other.eng.device_info() and eng.device_info()["compute_units"] > 0
    elif cid in ("malloc_device", "free_device", "memcpy_h2d", "memcpy_d2h", "memset_device", "malloc_host", "free_host", "host_register", "host_unregister"):
        src = (C.c_uint8 * 4096)(*[(7 * i) % 251 for i in range(4096)])
        back = (C.c_uint8 * 4096)()
        d, h = vp(), vp()
        first = eng if cid == "malloc_device" else other.eng
        assert lib.fxg_malloc_device(first.ctx, 4096, C.byref(d)) == 0 and d.value
        first = eng if cid == "malloc_host" else other.eng
        assert lib.fxg_malloc_host(first.ctx, 4096, C.byref(h)) == 0 and h.value
        first = eng if cid == "host_register" else other.eng
        assert lib.fxg_host_register(first.ctx, C.addressof(src), 4096) == 0
        first = eng if cid == "memset_device" else other.eng
        assert lib.fxg_memset_device(first.ctx, d, 0x3C, 4096) == 0 and lib.fxg_sync(first.ctx) == 0
        first = eng if cid == "memcpy_h2d" else other.eng
        assert lib.fxg_memcpy_h2d(first.ctx, d, C.addressof(src), 2048) == 0 and lib.fxg_sync(first.ctx) == 0
        first = eng if cid == "memcpy_d2h" else other.eng
        assert lib.fxg_memcpy_d2h(first.ctx, C.addressof(back), d, 4096) == 0 and lib.fxg_sync(first.ctx) == 0
        assert bytes(back) == bytes(src)[:2048] + b"\x3c" * 2048
        first = eng if cid == "host_unregister" else other.eng
        assert lib.fxg_host_unregister(first.ctx, C.addressof(src)) == 0
        assert lib.fxg_free_device((eng if cid == "free_device" else other.eng).ctx, d) == 0
        assert lib.fxg_free_host((eng if cid == "free_host" else other.eng).ctx, h) == 0
    elif cid in ("timer_start", "timer_stop"):                # (the pair: a stop with no start is the caller's error)
        eng.timer_start()
        assert eng.timer_stop() >= 0.0
    elif cid == "concat_peer":
        a = T.arange(0, 200, dtype=T.uint8, device=eng.device)
        dst = fresh.g.alloc(256)
        T.cuda.synchronize()
        assert lib.fxg_concat_peer(eng.ctx, vp(dst.data_ptr()), 16, eng.ctx, vp(a.data_ptr()), 200) == 0 and lib.fxg_sync(eng.ctx) == 0
        host = dst.cpu().numpy()
        assert (host[:16] == POISON).all() and np.array_equal(host[16:216], np.arange(200, dtype=np.uint8)) and (host[216:] == POISON).all()
    elif cid == "set_profiling":
        eng.set_profiling(True)
        fresh.do_run(S._run("rows38", 3000, "first.run"))
        assert eng.last_kernel_ms() > 0.0 and len(eng.profiled_kernel_ms()) == 1
    elif cid == "last_kernel_ms_nothing_profiled":
        ms = C.c_float(-5.0)
        expect_refusal(eng, outcome, lib.fxg_last_kernel_ms(eng.ctx, C.byref(ms)), ms.value == -5.0)
    elif cid == "profiled_kernel_ms_none":
        assert eng.profiled_kernel_ms() == []
    elif cid == "last_launch_info_none":
        assert eng.last_launch() == dict(kernel="", grid=0, block=0, lds=0, tile_reads=0)
    elif cid == "scan_recoveries_zero":
        assert eng.scan_recoveries() == 0
    elif cid == "synth":
        b, q = eng.synth(3, 12345, 2000, 100, True, 112)
        ob, oq = fo.synth_batch(3, 12345, 2000, 100, True, 112)
        assert np.array_equal(b.cpu().numpy(), ob) and np.array_equal(q.cpu().numpy(), oq)
    elif cid in ("run_rows", "run_tiles", "run_clip"):
        fresh.do_run(S._run(dict(run_rows="rows38", run_tiles="rev2", run_clip="clip40k")[cid], 3000, "first.run"))
    elif cid in ("run_qtrim_qfilter", "run_clip_entry", "run_revcomp_trim"):
        n, stride = 3000, 100
        b, q = fo.synth_batch(9, 0, n, stride, True, stride)
        pd = dict(run_qtrim_qfilter=dict(stages=6, **K.QTF), run_clip_entry=dict(stages=1, adapter=S.AD13, clip_min_len=7, clip_keep_delta=0, clip_min_adapter_len=0, clip_flags=4),
                  run_revcomp_trim=dict(stages=24, ft_first=3, ft_last=90))[cid]
        o = fo.run_pipeline(b, q, None, oracle_params(pd), fixed_len=stride)
        db, dq = T.from_numpy(b).to(eng.device), T.from_numpy(q).to(eng.device)
        out = eng.alloc_outputs(n, stride)
        out["out_bases"], out["out_qual"] = fresh.g.alloc(n * stride), fresh.g.alloc(n * stride)
        bt = FxgBatch(db.data_ptr(), dq.data_ptr(), None, stride, stride, n)
        fo_ = FxgOut(*[out[k].data_ptr() for k in ("res", "out_bases", "out_qual", "out_len", "kept_index", "out_off", "counters")])
        eng._after_torch()
        if cid == "run_qtrim_qfilter":
            rc = lib.fxg_run_qtrim_qfilter(eng.ctx, C.byref(bt), 33, 1, 20, 30, 1, 20, 80, C.byref(fo_))
        elif cid == "run_clip_entry":
            rc = lib.fxg_run_clip(eng.ctx, C.byref(bt), S.AD13, 7, 0, 0, 4, C.byref(fo_))
        else:
            rc = lib.fxg_run_revcomp_trim(eng.ctx, C.byref(bt), 1, 3, 90, C.byref(fo_))
        assert rc == 0, last_error(eng)
        eng._before_torch()
        from fastx_toolkit_amd.engine import Result
        h = Result(eng, out["res"], out["out_bases"], out["out_qual"], out["out_len"], out["kept_index"], out["out_off"], out["counters"]).to_host()
        assert eng.scan_recoveries() == 0
        assert_same(o, h, cid)
    elif cid == "quality_stats":
        fresh.do_stats(_st("stats", n=3000))
    elif cid == "read_counters_zeroed":
        z = T.zeros(NCOUNTERS, dtype=T.int64, device=eng.device)
        T.cuda.synchronize()
        assert not eng.read_counters(z).any() and eng.scan_recoveries() == 0
    elif cid == "fastq_index":
        fresh.do_index(_st("index", block=SMALL_FASTQ))
    elif cid == "fastq_pack_other_contexts_lines":
        fresh.idx[SMALL_FASTQ] = other.do_index(_st("index", block=SMALL_FASTQ))
        other.eng.sync()
        fresh.do_pack(_st("pack", block=SMALL_FASTQ))
    elif cid in ("fastq_format_opts_len_no_res", "fastq_format_plain", "fasta_weights_unindexed"):
        x = fresh.idx[SMALL_FASTQ] = other.do_index(_st("index", block=SMALL_FASTQ))
        other.eng.sync()
        if cid == "fastq_format_opts_len_no_res":
            return fresh.do_format(_st("format", block=SMALL_FASTQ))
        n = x["n"]
        res = T.from_numpy(((1 << 16) | x["blk"]["lens"].astype(np.int64)).astype(np.int32)).to(eng.device)          # every record kept whole (keep bit 16, length below)
        if cid == "fasta_weights_unindexed":
            w = (C.c_uint64 * 8)(*([5] * 8))
            eng._after_torch()
            rc = lib.fxg_fasta_weights(eng.ctx, x["d_text"].data_ptr(), x["ix"].line.data_ptr(), x["ix"].cap_lines, n, res.data_ptr(), C.byref(w))
            return expect_refusal(eng, outcome, rc, list(w) == [0] * 8)
        out = fresh.g.alloc(format_bound(x["text_len"], n))
        nb = C.c_uint64(1)
        eng._after_torch()
        rc = lib.fxg_fastq_format(eng.ctx, x["d_text"].data_ptr(), 4, x["ix"].line.data_ptr(), x["ix"].cap_lines, x["ix"].flags.data_ptr(), n, res.data_ptr(), 0, 0, None, None, None, None,
                                  0, 33, 1, out.data_ptr(), C.byref(nb))
        assert rc == 0 and out[:nb.value].cpu().numpy().tobytes() == x["blk"]["fasta"], last_error(eng)
    elif cid == "barcode_prepare":
        fresh.do_bc_prepare(_st("bc_prepare", table="t97"))
        fresh.idx[SMALL_FASTQ] = other.do_index(_st("index", block=SMALL_FASTQ))
        other.eng.sync()
        fresh.do_bc_split(_st("bc_split", block=SMALL_FASTQ))
    elif cid == "barcode_split_without_prepare":
        x = other.do_index(_st("index", block=SMALL_FASTQ))
        other.eng.sync()
        out = fresh.g.alloc(x["text_len"], fill=CANARY)
        bb, br = (C.c_uint64 * 4)(9, 9, 9, 9), (C.c_uint64 * 4)(9, 9, 9, 9)
        rc = lib.fxg_barcode_split(eng.ctx, x["d_text"].data_ptr(), x["text_len"], 4, x["ix"].line.data_ptr(), x["ix"].cap_lines, x["n"], None, out.data_ptr(), bb, br)
        expect_refusal(eng, outcome, rc, bool((out == CANARY).all()) and list(bb) == [9] * 4 and list(br) == [9] * 4)
    elif cid == "fasta_reflow":
        fresh.do_reflow(_st("reflow", lines=2000, width=17))
    elif cid == "fasta_reflow_empty_closes_record":
        fresh.do_reflow(_st("reflow", lines=0, width=10), text=b"", at_eof=True, open_in=7)          # 7 bases of an open record: the end of input writes its newline
        fresh.do_reflow(_st("reflow", lines=0, width=7), text=b"", at_eof=True, open_in=7)           # ... and none after a full line
    elif cid in ("fasta_uncollapse_from_zero", "fasta_uncollapse_continue_nothing"):
        key = SMALL_COLLAPSED if cid == "fasta_uncollapse_from_zero" else ("collapsed", 5, 2)
        x = fresh.idx[key] = other.do_index(_st("index", block=key))
        other.eng.sync()
        if cid == "fasta_uncollapse_from_zero":
            fresh.do_uc(_st("uc", block=key, first=True, parts=2))
            return fresh.do_uc(_st("uc", block=key, parts=2, rest=True))
        out = fresh.g.alloc(256, fill=CANARY)
        rc, info = fresh.uc_call(x, 7, 1, out, 256)
        expect_refusal(eng, outcome, rc, bool((out == CANARY).all()))
    elif cid == "clip_history_then_batch":
        fresh.do_history(_st("history", on=True))
        fresh.do_run(S._run("clip13", 3000, "first.batch1", ragged=True))
        fresh.do_run(S._run("clip13", 2000, "first.batch2", ragged=True))
        fresh.do_history(_st("history", on=False))
    elif cid in ("bases_change_other_contexts_lines", "bases_change_no_records"):
        import nucchange_model as NM
        from fastx_toolkit_amd.engine import NO_RECORD, FxgBasesChangeInfo
        x = other.do_index(_st("index", block=SMALL_FASTA))
        other.eng.sync()
        blk = NM.Block(x["blk"]["records"], "r")
        none = cid == "bases_change_no_records"
        info = FxgBasesChangeInfo(5, 5, 5)
        eng._after_torch()
        rc = lib.fxg_bases_change(eng.ctx, x["d_text"].data_ptr(), x["text_len"], 2, x["ix"].line.data_ptr(), x["ix"].cap_lines, 0 if none else x["n"], ord("T"), ord("U"), C.byref(info))
        assert rc == 0, last_error(eng)
        assert (info.changed, info.first_to_record, info.irregular) == ((0, NO_RECORD, 0) if none else (blk.changed, blk.first_to, blk.irregular))
        host = x["d_text"].cpu().numpy()
        assert host[:x["text_len"]].tobytes() == (blk.text if none else blk.rewritten) and (host[x["text_len"]:] == POISON).all()
        assert blk.changed > 0 and blk.first_to == NO_RECORD and eng.last_launch()["kernel"] == ("" if none else "fxg_kernel_bases_change")
    elif cid in ("collapse_begin", "collapse_add_other_contexts_lines"):
        import collapse_cases as CK
        import test_gpu_collapse as GC
        records = [c for c in CK.abi_cases() if c[0] == "ties"][0][1]
        assert GC.begin(eng) == 0, last_error(eng)
        if cid == "collapse_begin":
            out, _ = GC.run_blocks(eng, CK.split(records, 2))          # (begin once more, then the case: the first begin left a set that takes it)
        else:
            ix = GC.Indexed(other.eng, records)
            other.eng.sync()
            rc, info = GC.add(eng, ix)
            want = GC.expected_info([records], False, 0)
            assert rc == 0 and (info.records, info.reads, info.uniques, info.irregular) == (want["records"], want["reads"], want["uniques"], 0), last_error(eng)
            rc, info = GC.order(eng)
            assert rc == 0 and {k: getattr(info, k) for k in want} == want, last_error(eng)
            _, out, w = GC.write(eng, 0, info.out_bytes)
            assert w.rank_end == info.uniques
        CK.assert_output("ties", out)
    elif cid in ("collapse_add_no_set", "collapse_order_no_set", "collapse_write_no_set"):
        import collapse_cases as CK
        import test_gpu_collapse as GC
        from fastx_toolkit_amd.engine import FxgCollapseInfo, FxgCollapseWindow
        ix = GC.Indexed(other.eng, [(CK.ident(i), CK.seq(i, 20)) for i in range(10)])
        other.eng.sync()
        info, win = FxgCollapseInfo(), FxgCollapseWindow(77, 77)
        C.memset(C.byref(info), 0xEE, C.sizeof(info))
        out = fresh.g.alloc(256, fill=CANARY)
        eng._after_torch()
        if cid == "collapse_add_no_set":
            rc = lib.fxg_collapse_add(eng.ctx, ix.d_text.data_ptr(), ix.text_len, 2, ix.ix.line.data_ptr(), ix.ix.cap_lines, ix.n, ix.lens.data_ptr(), C.byref(info))
        elif cid == "collapse_order_no_set":
            rc = lib.fxg_collapse_order(eng.ctx, C.byref(info))
        else:
            rc = lib.fxg_collapse_write(eng.ctx, 3, 256, out.data_ptr(), C.byref(win))
        if cid == "collapse_write_no_set":                   # what include/fxg.h says a refused call leaves: the window zeroed with rank_end = rank_begin,
            quiet = (win.rank_end, win.out_bytes) == (3, 0)
        else:                                                 # info zeroed with first_bad = ~0
            quiet = tuple(getattr(info, k) for k in K.COLLAPSE_INFO_FIELDS) == K.COLLAPSE_INFO_REFUSED
        expect_refusal(eng, outcome, rc, bool((out == CANARY).all()) and quiet)
        assert eng.last_launch()["kernel"] == ""                 # nothing launched
    else:
        raise AssertionError("no first call for " + cid)
    if outcome == K.OK:
        assert last_error(eng) == "", (cid, last_error(eng))


@pytest.mark.parametrize("cid,entry,outcome", K.FIRST_CALLS, ids=["context_state_first_%s" % c[0] for c in K.FIRST_CALLS])
def test_first_call_on_a_fresh_context(engine, monkeypatch, cid, entry, outcome):
    other = Runner(engine, monkeypatch)
    with fresh_engine(monkeypatch) as eng:
        fresh = Runner(eng, monkeypatch)
        try:
            first_call(cid, outcome, fresh, other, monkeypatch)
            fresh.g.check(cid)
            eng.sync()
        finally:
            fresh.close()
            other.close()


# ---- b. one context, interleaved families -----------------------------------------------------------------------------------------------------------
def test_context_state_interleaved_families_growing_and_shrinking(monkeypatch):
    with fresh_engine(monkeypatch) as eng:
        run = Runner(eng, monkeypatch)
        steps = S.build(run.cus)
        model, recov = K.GrowModel(), eng.scan_recoveries()
        try:
            for i, st in enumerate(steps):
                if st["kind"] == "run":
                    ll = run.do_run(st)
                    run.g.check(st["label"])
                    f = S.FAM[st["fam"]]
                    if f.get("bucket") and not st.get("refused"):          # the grid the grow rule of the checkpoint scratch was worked out for
                        assert ll["grid"] == -(-st["n"] // f["T"]) + 1, (i, st["label"], ll)
                else:
                    run.step(st)
                for name, need_cap in S.workspace_use(st, run.cus):
                    model.use(i, name, need_cap)
            assert eng.scan_recoveries() == recov
            assert not run.results, "a run whose counters were never read: %r" % list(run.results)
        finally:
            run.close()
        regrown = model.regrown()
        assert all(len(regrown.get(ws, [])) >= 2 for ws in S.WORKSPACES), regrown


def test_context_state_fallback_workspace_growing_and_shrinking(monkeypatch):
    """fb_blk: every compacting launch of this context gives up waiting and is done again without the scanner by the read_counters that comes two calls
    later; scan_recoveries() goes up by exactly one per run"""
    with fresh_engine(monkeypatch, FXG_TEST_SCAN_TIMEOUT=1) as eng:
        run = Runner(eng, monkeypatch, recoveries_per_run=1)
        try:
            for st in S.fallback_steps():
                if st["kind"] == "run":
                    run.do_run(st)
                else:
                    run.step(st)
            assert eng.scan_recoveries() == 4 and not run.results
        finally:
            run.close()


# ---- c. kernel attributes -----------------------------------------------------------------------------------------------------------------------------
_c_cache = {}


def attr_case(eng, req, n=700):
    """(device bases, device qual, oracle result) of a request of context_state_cases, once per (kernel, stride)"""
    key = (req["kernel"], req["stride"], n)
    if key not in _c_cache:
        b, q = K.batch_of(req, n)
        _c_cache[key] = (b, q, fo.run_pipeline(b, q, None, oracle_params(req["pd"]), fixed_len=req["stride"]))
    b, q, o = _c_cache[key]
    T = eng.torch
    return T.from_numpy(b).to(eng.device), T.from_numpy(q).to(eng.device), o


def attr_run(eng, mp, req, db, dq, o, what="", set_knobs=True):
    """one run of a request: 0, the kernel by its whole name, every array the oracle's, no recovery.  Returns the launch's LDS size."""
    before = eng.scan_recoveries()
    with (knobs(mp, req["env"]) if set_knobs else contextlib.nullcontext()):
        h = eng.run(db, dq, make_params(**req["pd"]), fixed_len=req["stride"]).to_host()
    assert eng.scan_recoveries() == before, (req["kernel"], what)
    ll = eng.last_launch()
    assert ll["kernel"] == req["kernel"], (ll, what)
    assert_same(o, h, "%s stride %d %s" % (req["kernel"], req["stride"], what))
    return ll["lds"]


def alternate(engines, mp, req, order, what):
    """`order`: [(engine index, "large" | "small")] over the request at its two read lengths (the longer reads stage the larger tile); every run is checked,
    each size's LDS is the same every time and the two differ"""
    size = dict(large=max(K.ALT_STRIDES), small=min(K.ALT_STRIDES))
    cases = {s: attr_case(engines[0], K.with_stride(req, s)) for s in K.ALT_STRIDES}
    lds = {}
    for e, which in order:
        s = size[which]
        got = attr_run(engines[e], mp, K.with_stride(req, s), *cases[s], what="%s %s on context %d" % (what, which, e))
        assert got == lds.setdefault(which, got), (req["kernel"], which, got, lds)
    assert lds["large"] > lds["small"], (req["kernel"], lds)


def test_context_state_all_tile_kernels_then_alternating_lds(monkeypatch):
    reqs = K.tile_kernel_requests()
    with fresh_engine(monkeypatch) as eng:
        seen = []
        for req in reqs:
            attr_run(eng, monkeypatch, req, *attr_case(eng, req), what="first pass")
            seen.append(eng.last_launch()["kernel"])
        assert len(set(seen)) == K.N_TILE_KERNELS == 43
        for k in K.ALTERNATING:
            assert reqs[k]["kernel"] in seen[-11:]
            alternate([eng], monkeypatch, reqs[k], [(0, w) for w in ("large", "small", "large", "small", "large")], "one context")


def test_context_state_two_contexts_alternating_lds(monkeypatch):
    reqs = K.tile_kernel_requests()
    with fresh_engine(monkeypatch) as a, fresh_engine(monkeypatch) as b:
        for k in K.ALTERNATING + [20]:                        # (the last one: a kernel any table had room for -- the contexts still disagree)
            alternate([a, b], monkeypatch, reqs[k], [(0, "large"), (1, "small"), (0, "large"), (1, "large"), (0, "small")], "two contexts")


def test_context_state_two_threads_one_context_each(monkeypatch):
    """40 runs each of different requests of one instance (four LDS sizes between them), inputs and oracle answers made before the threads start"""
    with fresh_engine(monkeypatch) as a, fresh_engine(monkeypatch) as b:
        engines = (a, b)
        work = [[(K.thread_request(s), attr_case(engines[t], K.thread_request(s), n=900 + 100 * t)) for s in K.THREAD_STRIDES[t]] for t in (0, 1)]
        failures, lds = [], [set(), set()]
        a.torch.cuda.synchronize()

        def loop(t):
            try:
                for i in range(K.THREAD_RUNS):
                    req, case = work[t][i % 2]
                    lds[t].add(attr_run(engines[t], monkeypatch, req, *case, what="thread %d run %d" % (t, i), set_knobs=False))
            except BaseException as e:       # reported after the join
                failures.append((t, repr(e)))
        for k in K.KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in K.thread_request(100)["env"].items():         # (the request knobs are the process's: set once, for both threads, and left alone while they run)
            monkeypatch.setenv(k, v)
        threads = [threading.Thread(target=loop, args=(t,), daemon=True) for t in (0, 1)]
        for th in threads:
            th.start()
        for th in threads:
            th.join(120)
        assert not any(th.is_alive() for th in threads), "a thread did not finish"
        assert not failures, failures
        assert len(lds[0]) == 2 and len(lds[1]) == 2 and len(lds[0] | lds[1]) == 4, lds


def test_context_state_first_call_table_is_run_whole():
    """every row of the table has its call above (the CPU tier holds the table against the entry points)"""
    import inspect
    src = inspect.getsource(first_call)
    assert all('"%s"' % cid in src for cid, _, _ in K.FIRST_CALLS)

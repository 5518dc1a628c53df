"""ctypes view of tests/emu/libfxgemu.so (serial CPU emulation of the tile kernels, test-only)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_LIB = None
NCOUNTERS = 24


class Batch(C.Structure):
    _fields_ = [("bases", C.c_void_p), ("qual", C.c_void_p), ("len", C.c_void_p),
                ("fixed_len", C.c_uint32), ("stride", C.c_uint32), ("n", C.c_uint64)]


class Out(C.Structure):
    _fields_ = [("res", C.c_void_p), ("out_bases", C.c_void_p), ("out_qual", C.c_void_p), ("out_len", C.c_void_p),
                ("kept_index", C.c_void_p), ("out_off", C.c_void_p), ("counters", C.c_void_p)]


_CXX = ["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-Wno-pass-failed", "-DFXG_HOST_EMULATION"]
_LINK = ["hipcc", "-shared", "-fPIC"]         # (objects only: with --cuda-host-only the driver would read them as sources)
_CSRC = os.path.join(_HERE, "..", "fastx_toolkit_amd", "csrc")
_EMU_DEPS = [os.path.join(_EMU, "fxg_stub_ctx.h")] + [os.path.join(_CSRC, f) for f in ("fxg_device.h", "fxg_clip_instances.h", "fxg_instances.h", "fxg_knobs.h", "fxg_kernels.h", "fxg_plan.h", "fxg_text.h", "fxg_rows.h", "fxg_history.h", "fxg_stats.h")]
EMU_UNITS = 8               # fxg_emu.cpp: -DFXG_EMU_TU=0 (everything but the clipper's instances) and one per unit of clip instances (csrc/fxg_clip_instances.h; tests/test_clip_instances.py)


def _emu_objects(defs):
    """fxg_emu.cpp as EMU_UNITS objects compiled side by side (one unit took over three minutes); both libraries below link the same objects."""
    src = os.path.join(_EMU, "fxg_emu.cpp")
    d = os.path.join(_EMU, "obj%s" % "".join(x.replace("-D", "_").replace("=", "") for x in defs))
    os.makedirs(d, exist_ok=True)
    newest = max(os.path.getmtime(x) for x in [src] + _EMU_DEPS)
    objs = [os.path.join(d, "fxg_emu_%d.o" % k) for k in range(EMU_UNITS)]
    stale = [k for k, o in enumerate(objs) if not os.path.exists(o) or os.path.getmtime(o) < newest]
    procs = [(k, subprocess.Popen(_CXX + defs + ["-DFXG_EMU_TU=%d" % k, "-c", src, "-o", objs[k] + ".tmp"])) for k in stale]
    bad = [k for k, pr in procs if pr.wait() != 0]
    if bad:
        raise RuntimeError("emulator units %s did not compile" % bad)
    for k in stale:
        os.replace(objs[k] + ".tmp", objs[k])
    return objs


def build():
    defs = os.environ.get("FXG_EMU_DEFS", "").split()           # e.g. "-DFXG_ROWS_SPARSE_BASES=0": check a kernel variant on the CPU tier
    so = os.path.join(_EMU, "libfxgemu%s.so" % "".join(d.replace("-D", "_") for d in defs))
    objs = _emu_objects(defs)
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(o) for o in objs):
        subprocess.check_call(_LINK + objs + ["-o", so + ".tmp"])
        os.replace(so + ".tmp", so)
    return so


def build_stub():
    """tests/emu/stub/libfxg.so: the test-only look-alike of the engine library (fxg_stub.cpp over the emulator, plus the product's own
    multi-GPU host code, csrc/fxg_comm.h).  Returns the directory to put first on LD_LIBRARY_PATH."""
    build()
    d = os.path.join(_EMU, "stub")
    os.makedirs(d, exist_ok=True)
    so = os.path.join(d, "libfxg.so")
    src = os.path.join(_EMU, "fxg_stub.cpp")
    objs = _emu_objects([])
    deps = [src, os.path.join(_CSRC, "fxg_comm.h"), os.path.join(_HERE, "..", "include", "fxg.h")] + _EMU_DEPS + objs
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(x) for x in deps):
        subprocess.check_call(_CXX + ["-c", src, "-o", os.path.join(d, "fxg_stub.o")])
        subprocess.check_call(_LINK + [os.path.join(d, "fxg_stub.o")] + objs + ["-o", so + ".tmp", "-ldl"])
        os.replace(so + ".tmp", so)
    return d


def build_fmtopts():
    """tests/emu/fmtopts/libfxg.so: the stub's own objects plus fxg_fastq_format_opts (fmtopts_stub.cpp) and the splitter's two entry points,
    which engine.load_library declares (bcsplit_stub.cpp over bcsplit_emu.cpp, as tests/test_barcode_cpu.py links them).  Returns the directory."""
    stub = build_stub()
    d = os.path.join(_EMU, "fmtopts")
    os.makedirs(d, exist_ok=True)
    so = os.path.join(d, "libfxg.so")
    srcs = [os.path.join(_EMU, f) for f in ("fmtopts_stub.cpp", "bcsplit_stub.cpp", "bcsplit_emu.cpp")]
    base = [os.path.join(stub, "fxg_stub.o")] + _emu_objects([])
    deps = srcs + base + _EMU_DEPS + [os.path.join(_CSRC, "fxg_barcode.h"), os.path.join(_HERE, "..", "include", "fxg.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(x) for x in deps):
        objs = [os.path.join(d, os.path.basename(x)[:-4] + ".o") for x in srcs]
        for x, o in zip(srcs, objs):
            subprocess.check_call(_CXX + ["-c", x, "-o", o])
        subprocess.check_call(_LINK + base + objs + ["-o", so + ".tmp", "-ldl"])
        os.replace(so + ".tmp", so)
    return d


def build_fake_rccl():
    """tests/emu/fakerccl/librccl.so.1: the five NCCL entry points the transport binds, over a shared-memory file (fake_rccl.c)."""
    d = os.path.join(_EMU, "fakerccl")
    os.makedirs(d, exist_ok=True)
    so, src = os.path.join(d, "librccl.so.1"), os.path.join(_EMU, "fake_rccl.c")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-Wall", "-Wextra", "-fPIC", "-shared", src, "-o", so, "-ldl"])
    return d


def lib():
    global _LIB
    if _LIB is None:
        _LIB = C.CDLL(build())
        _LIB.fxg_emu_run_pipeline.argtypes = [C.POINTER(Batch), C.c_void_p, C.POINTER(Out), C.c_char_p, C.c_size_t]
        _LIB.fxg_emu_plan.argtypes = [C.POINTER(Batch), C.c_void_p, C.POINTER(Out), C.c_int, C.c_uint32, C.POINTER(PlanInfo), C.c_char_p, C.c_size_t]
        _LIB.fxg_emu_tile_reads.restype = C.c_uint
        _LIB.fxg_emu_inst_name.argtypes, _LIB.fxg_emu_inst_name.restype = [C.c_int, C.c_int], C.c_char_p
        _LIB.fxg_emu_knobs.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_longlong), C.c_int]
        _LIB.fxg_emu_run_pipeline_hist.argtypes = [C.POINTER(Batch), C.c_void_p, C.POINTER(Out), C.c_char_p, C.c_size_t, C.c_void_p]
        _LIB.fxg_emu_hist_new.restype = C.c_void_p
        _LIB.fxg_emu_hist_free.argtypes = [C.c_void_p]
        _LIB.fxg_emu_run_quality_stats.argtypes = [C.POINTER(Batch), C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t]
        _LIB.fxg_emu_quality_stats_piece_trips.restype = C.c_uint64
        _LIB.fxg_emu_quality_stats_piece_moved.restype = C.c_uint64
    return _LIB


def _aligned(n, dtype=np.uint8):
    """16-byte aligned zeroed array of n items."""
    item = np.dtype(dtype).itemsize
    raw = np.zeros(n * item + 32, dtype=np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw[off:off + n * item].view(dtype)


PAGE = os.sysconf("SC_PAGE_SIZE")
_GUARDED = []                    # mappings handed out by _guarded(): they live as long as the process (the bounds tier runs one case per child)


def _guarded(n, dtype=np.uint8, where="after"):
    """n items between guard pages: the array's contracted range (include/fxg.h: its bytes rounded up to the 16-byte granule) ends exactly at a
    PROT_NONE page (where="after"), or starts exactly behind one (where="before"), the start 16-byte aligned either way.  Zeroed.  An emulated kernel
    that touches a byte outside the contract on that side takes a SIGSEGV."""
    item = np.dtype(dtype).itemsize
    span = (n * item + 15) // 16 * 16
    libc = C.CDLL(None, use_errno=True)
    libc.mmap.restype, libc.mmap.argtypes = C.c_void_p, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_long]
    libc.mprotect.argtypes = [C.c_void_p, C.c_size_t, C.c_int]
    body = (span + PAGE - 1) // PAGE * PAGE
    size = body + 2 * PAGE
    base = libc.mmap(None, size, 3, 0x22, -1, 0)            # PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS
    if base in (None, C.c_void_p(-1).value):
        raise OSError(C.get_errno(), "mmap")
    if libc.mprotect(base, PAGE, 0) != 0 or libc.mprotect(base + PAGE + body, PAGE, 0) != 0:
        raise OSError(C.get_errno(), "mprotect")
    start = base + PAGE + (body - span if where == "after" else 0)
    _GUARDED.append((base, size))
    if n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array((C.c_uint8 * (n * item)).from_address(start)).view(dtype)


def _alloc(n, dtype=np.uint8, guard=None):
    """_aligned() by default; guard="after" / "before": _guarded()"""
    return _aligned(n, dtype) if guard is None else _guarded(n, dtype, guard)


def _tight(a, where):
    """the bytes of `a` at EXACTLY their size against a guard page: the last byte is the one before the PROT_NONE page (where="after": the start is
    then as aligned as the array's size) or the first byte the one behind it (where="before").  An empty array is an address at the guard page."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    pad = (-raw.size) % 16 if where == "after" else 0
    g = _guarded(max(raw.size + pad, 16), np.uint8, where)
    if raw.size == 0:
        return g[16:] if where == "after" else g[:0]
    g[pad:pad + raw.size] = raw
    return g[pad:pad + raw.size]


class FormatOpts(C.Structure):
    _fields_ = [("id_mode", C.c_uint32), ("id_both", C.c_uint32), ("ordinal_base", C.c_uint64), ("qual_mode", C.c_uint32), ("out_cap", C.c_uint64), ("d_len", C.c_void_p)]


_FMTOPTS = None


def format_opts(q, guard, out_cap, id_mode=0, id_both=False, base=0, qual_mode=0, out_fasta=False):
    """fxg_fastq_format_opts of the emulation stub (fmtopts_stub.cpp: build_fmtopts) over the arrays of a format_opts_cases.bounds_request, each at
    exactly its size against a guard page (_tight), d_out of exactly out_cap bytes too.  guard None: plain arrays.  Returns (rc, bytes, out_bytes)."""
    global _FMTOPTS
    if _FMTOPTS is None:
        L = C.CDLL(os.path.join(build_fmtopts(), "libfxg.so"))
        vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
        L.fxg_ctx_create.argtypes = [i32, C.POINTER(vp)]
        L.fxg_fastq_format_opts.argtypes = [vp, vp, i32, vp, u64, vp, u64, vp, u32, i32, vp, vp, vp, vp, u32, i32, i32, vp, C.POINTER(u64), C.POINTER(FormatOpts)]
        ctx = vp()
        assert L.fxg_ctx_create(0, C.byref(ctx)) == 0
        _FMTOPTS = (L, ctx)
    L, ctx = _FMTOPTS
    put = (lambda a: None if a is None else _tight(a, guard)) if guard else (lambda a: None if a is None else np.ascontiguousarray(a).copy())
    arr = {k: put(q[k]) for k in ("text", "line", "flags", "lens", "rows_qual", "res", "pk_bases", "pk_qual", "pk_off")}
    out = _tight(np.zeros(out_cap, np.uint8), guard) if guard else np.zeros(out_cap, np.uint8)
    ptr = lambda a: None if a is None else a.__array_interface__["data"][0]      # (an empty array too: its address is the guard page's edge)
    nb = C.c_uint64()
    o = FormatOpts(id_mode, int(bool(id_both)), base, qual_mode, out_cap, ptr(arr["lens"]))
    rc = L.fxg_fastq_format_opts(ctx, ptr(arr["text"]), 4, ptr(arr["line"]), q["cap_lines"], ptr(arr["flags"]), q["n"], ptr(arr["res"]), q["fwd_start"], q["reverse"],
                                 ptr(arr["pk_bases"]), ptr(arr["pk_qual"]), ptr(arr["pk_off"]), ptr(arr["rows_qual"]), q["stride"], 33, int(out_fasta), ptr(out), C.byref(nb), C.byref(o))
    for k in ("text", "line", "flags", "lens", "rows_qual", "res", "pk_bases", "pk_qual", "pk_off"):
        assert arr[k] is None or np.array_equal(np.asarray(arr[k]).view(np.uint8).reshape(-1), np.ascontiguousarray(q[k]).view(np.uint8).reshape(-1)), "input %s changed" % k
    return rc, out[:nb.value].tobytes(), nb.value


def hist_new():
    return lib().fxg_emu_hist_new()


def hist_free(h):
    lib().fxg_emu_hist_free(h)


def run_pipeline(bases, qual, lens, params, fixed_len=None, compact=True, hist=None, guard=None):
    """guard="after" / "before": every input and output array at exactly its contracted size (include/fxg.h) against a guard page (_guarded)."""
    n, stride = bases.shape
    b = _alloc(n * stride, guard=guard); b[:] = bases.reshape(-1)
    q = None
    if qual is not None:
        q = _alloc(n * stride, guard=guard); q[:] = qual.reshape(-1)
    if lens is not None:
        lv = _alloc(n, np.uint16, guard); lv[:] = lens
        lens = lv
    res = _alloc(n, np.uint32, guard)
    cap = n * stride if guard else n * stride + 16
    ob, oq = _alloc(cap, guard=guard), _alloc(cap, guard=guard)
    ol, ki, oo = _alloc(n, np.uint16, guard), _alloc(n, np.uint32, guard), _alloc(n, np.uint64, guard)
    ctr = _alloc(NCOUNTERS, np.uint64, guard)
    bt = Batch(b.ctypes.data, q.ctypes.data if q is not None else None, lens.ctypes.data if lens is not None else None,
               int(fixed_len or stride), stride, n)
    o = Out(res.ctypes.data, ob.ctypes.data if compact else None, oq.ctypes.data if (compact and q is not None) else None,
            ol.ctypes.data, ki.ctypes.data, oo.ctypes.data, ctr.ctypes.data)
    err = C.create_string_buffer(512)
    rc = lib().fxg_emu_run_pipeline_hist(C.byref(bt), C.addressof(params), C.byref(o), err, 512, hist)
    if rc != 0:
        raise ValueError("emu rc=%d: %s" % (rc, err.value.decode()))
    kept, nbytes = int(ctr[1]), int(ctr[2])
    return dict(res=res.copy(), out_bases=ob[:nbytes].copy(), out_qual=oq[:nbytes].copy() if q is not None else None,
                out_len=ol[:kept].copy(), kept_index=ki[:kept].copy(), out_off=oo[:kept].copy(), counters=ctr.copy())


def run_quality_stats(bases, qual, lens, fixed_len=None, hist=None, cols=None, guard=None):
    """Adds the batch to hist[cols][5][128] (uint64) and returns it.  guard: as in run_pipeline (the histogram too)."""
    n, stride = bases.shape
    cols = cols or stride
    if hist is None:
        hist = np.zeros((cols, 5, 128), dtype=np.uint64)
    h = hist
    if guard:
        h = _guarded(hist.size, np.uint64, guard).reshape(hist.shape); h[:] = hist
    b = _alloc(n * stride, guard=guard); b[:] = bases.reshape(-1)
    q = None
    if qual is not None:
        q = _alloc(n * stride, guard=guard); q[:] = qual.reshape(-1)
    if lens is not None:
        lv = _alloc(n, np.uint16, guard); lv[:] = lens
        lens = lv
    bt = Batch(b.ctypes.data, q.ctypes.data if q is not None else None, lens.ctypes.data if lens is not None else None,
               int(fixed_len or stride), stride, n)
    err = C.create_string_buffer(512)
    rc = lib().fxg_emu_run_quality_stats(C.byref(bt), h.ctypes.data, h.shape[0], err, 512)
    if rc != 0:
        raise ValueError("emu quality_stats rc=%d: %s" % (rc, err.value.decode()))
    if h is not hist:
        hist[:] = h
    return hist


class PlanInfo(C.Structure):
    """fxg_emu_plan_info (fxg_emu.cpp): what fxg_make_plan chose, as the engine would launch and report it"""
    _fields_ = [("name", C.c_char * 96), ("amax", C.c_int), ("two_pass", C.c_int), ("clip_global", C.c_int),
                ("tile", C.c_uint32), ("block", C.c_uint32), ("lds", C.c_uint32)]

    def dict(self):
        return dict(kernel=self.name.decode(), amax=self.amax, two_pass=bool(self.two_pass), clip_global=bool(self.clip_global),
                    tile=self.tile, block=self.block, lds=self.lds)


def plan(stride, params, n=1, fixed_len=None, ragged=False, qual=True, compact=True, hist=None):
    """The plan of a request without running it, under the environment as it is now: dict(kernel, amax, two_pass, clip_global, tile, block, lds).
    The plan never dereferences the batch: every array is one fake aligned address, so n may be anything.  hist: the widest row a context with clip
    history has seen so far (None: no history).  A refused request raises ValueError with the engine's message."""
    A = 1 << 20
    bt = Batch(A, A if qual else None, A if ragged else None, int(fixed_len or stride), stride, n)
    o = Out(A, A if compact else None, A if (compact and qual) else None, A, A, A, A)
    info, err = PlanInfo(), C.create_string_buffer(512)
    rc = lib().fxg_emu_plan(C.byref(bt), C.addressof(params), C.byref(o), int(hist is not None), int(hist or 0), C.byref(info), err, 512)
    if rc != 0:
        raise ValueError("plan rc=%d: %s" % (rc, err.value.decode()))
    return info.dict()


class AttrSet(C.Structure):
    _fields_ = [("step", C.c_uint64), ("device", C.c_int32), ("kernel", C.c_int32), ("lds", C.c_uint32)]


_ATTR = None


def attr_replay(launches, nctx=None):
    """Replays launches [(context, device, kernel, lds), ...] through the engine's own decision about the kernels' dynamic-LDS attribute (csrc/fxg_attr.h,
    compiled into tests/emu/libfxgattr.so from attr_emu.cpp): one process, one occupancy cache per context.  Returns (the log of attribute sets
    [(step, device, kernel, lds), ...] in order, the number of occupancy questions asked)."""
    global _ATTR
    if _ATTR is None:
        so, src = os.path.join(_EMU, "libfxgattr.so"), os.path.join(_EMU, "attr_emu.cpp")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(x) for x in (src, os.path.join(_CSRC, "fxg_attr.h"))):
            subprocess.check_call(["hipcc", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", "-x", "c++", src, "-o", so + ".tmp", "-lpthread"])
            os.replace(so + ".tmp", so)
        _ATTR = C.CDLL(so)
        _ATTR.fxg_emu_attr_replay.restype = C.c_longlong
        _ATTR.fxg_emu_attr_replay.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.POINTER(AttrSet), C.c_uint64, C.POINTER(C.c_uint64)]
    a = np.array(launches, dtype=np.int64).reshape(-1, 4)
    cols = [np.ascontiguousarray(a[:, 0], dtype=np.int32), np.ascontiguousarray(a[:, 1], dtype=np.int32), np.ascontiguousarray(a[:, 2], dtype=np.int32),
            np.ascontiguousarray(a[:, 3], dtype=np.uint32)]
    nctx = nctx or (int(a[:, 0].max()) + 1 if len(a) else 1)
    log, asked = (AttrSet * max(len(a), 1))(), C.c_uint64()
    n = _ATTR.fxg_emu_attr_replay(*[c.ctypes.data for c in cols], len(a), nctx, log, len(a), C.byref(asked))
    if n < 0:
        raise ValueError("attr_replay: bad sequence")
    return [(int(log[i].step), int(log[i].device), int(log[i].kernel), int(log[i].lds)) for i in range(n)], int(asked.value)


def last_plan_clip_global():
    """(clip_global, tile_reads) of the plan the last emulated run was made with (fxg_plan.h: the DP over the batch instead of a staged tile)"""
    a, t = C.c_int(), C.c_int()
    lib().fxg_emu_last_plan_clip_global(C.byref(a), C.byref(t))
    return bool(a.value), t.value


def last_plan():
    """(clip instance, runs its scratch-checkpoint two-pass form) of the last run_pipeline call -- what fxg_make_plan chose."""
    a, t = C.c_int(), C.c_int()
    lib().fxg_emu_last_plan(C.byref(a), C.byref(t))
    return a.value, bool(t.value)


def instance_names():
    """the names of csrc/fxg_instances.h in the table's order, as the emulator was compiled with it"""
    return [lib().fxg_emu_inst_name(i, 0).decode() for i in range(lib().fxg_emu_inst_count())]


def clip_instance_name(amax):
    """the name of the clip instance of `amax` (negative: packed), None where the clip table has none"""
    s = lib().fxg_emu_inst_name(lib().fxg_emu_inst_count(), amax)
    return None if s is None else s.decode()


def knobs(scope):
    """{variable: value} of every knob of one scope ("request" / "context") of csrc/fxg_knobs.h, as fxg_knobs_read parses the environment now"""
    k = ("request", "context").index(scope)
    n = lib().fxg_emu_knobs(k, None, None, 0)
    names, values = (C.c_char_p * n)(), (C.c_longlong * n)()
    assert lib().fxg_emu_knobs(k, names, values, n) == n
    return {a.decode(): int(v) for a, v in zip(names, values)}


# ---- the device text path (fxg_text.h) through fxg_emu_fastq_index / _pack / _format / fxg_emu_fasta_weights ----
class TextInfo(C.Structure):
    _fields_ = [("lines", C.c_uint64), ("records", C.c_uint64), ("consumed", C.c_uint64), ("max_len", C.c_uint32),
                ("min_len", C.c_uint32), ("irregular", C.c_uint32), ("first_bad", C.c_uint32), ("numeric_records", C.c_uint32),
                ("has_cr", C.c_uint32)]


def fastq_index(text, at_eof=True, lpr=4, cap_records=None, guard=None):
    """fxg_fastq_index over `text` (the caller appends the final newline, as the engine does at end of input).  The text array is the contracted
    text_len + 16 bytes, the line / length / flag arrays the contracted cap_lines and cap_records entries (include/fxg.h)."""
    cap_records = cap_records or (len(text) // (4 if lpr == 2 else 7) + 2)
    cap_lines = lpr * cap_records + 1
    t = _alloc(len(text) + 16, guard=guard)
    t[:len(text)] = np.frombuffer(text, dtype=np.uint8)
    line, lens, flags = _alloc(2 * cap_lines, np.uint32, guard), _alloc(cap_records, np.uint16, guard), _alloc(cap_records, np.uint8, guard)
    state, info = C.create_string_buffer(256), TextInfo()
    rc = lib().fxg_emu_fastq_index(state, C.c_void_p(t.ctypes.data), C.c_uint64(len(text)), C.c_int(int(at_eof)), C.c_int(lpr),
                                   C.c_void_p(line.ctypes.data), C.c_uint64(cap_lines), C.c_void_p(lens.ctypes.data), C.c_void_p(flags.ctypes.data), C.byref(info), None, C.c_size_t(0))
    if rc != 0:
        raise ValueError("emu fastq_index rc=%d" % rc)
    return dict(text=t, text_len=len(text), lpr=lpr, line=line, cap_lines=cap_lines, lens=lens, flags=flags, info=info)


def fastq_pack(ix, n, stride, qoffset=33, want_qual=True, guard=None):
    """fxg_fastq_pack into rows of the contracted n * stride bytes (rounded up to 16)."""
    want_qual = want_qual and ix["lpr"] == 4
    b = _alloc(n * stride, guard=guard)
    q = _alloc(n * stride, guard=guard) if want_qual else None
    irr = C.c_uint32()
    rc = lib().fxg_emu_fastq_pack(C.c_void_p(ix["text"].ctypes.data), C.c_uint64(ix["text_len"]), C.c_int(ix["lpr"]), C.c_void_p(ix["line"].ctypes.data),
                                  C.c_uint64(ix["cap_lines"]), C.c_void_p(ix["flags"].ctypes.data), C.c_uint64(n), C.c_uint32(stride), C.c_int(qoffset),
                                  C.c_void_p(b.ctypes.data), C.c_void_p(q.ctypes.data if q is not None else None), C.byref(irr), None, C.c_size_t(0))
    if rc != 0:
        raise ValueError("emu fastq_pack rc=%d" % rc)
    return b.reshape(n, stride).copy(), (q.reshape(n, stride).copy() if q is not None else None), irr.value


def fastq_format(ix, n, res, rows_qual=None, stride=0, qoffset=33, out_fasta=False, guard=None):
    """fxg_fastq_format of the forward slices (no packed arrays) into the contracted text_len + records + 16 bytes; returns the bytes written."""
    r = _alloc(n, np.uint32, guard); r[:] = res
    rq = None
    if rows_qual is not None:
        rq = _alloc(rows_qual.size, guard=guard); rq[:] = rows_qual.reshape(-1)
    out = _alloc(ix["text_len"] + n + 16, guard=guard)
    nb = C.c_uint64()
    rc = lib().fxg_emu_fastq_format(C.c_void_p(ix["text"].ctypes.data), C.c_int(ix["lpr"]), C.c_void_p(ix["line"].ctypes.data), C.c_uint64(ix["cap_lines"]),
                                    C.c_void_p(ix["flags"].ctypes.data), C.c_uint64(n), C.c_void_p(r.ctypes.data), C.c_uint32(0), C.c_int(0),
                                    None, None, None, C.c_void_p(rq.ctypes.data if rq is not None else None), C.c_uint32(stride), C.c_int(qoffset),
                                    C.c_int(int(out_fasta)), C.c_void_p(out.ctypes.data), C.byref(nb), None, C.c_size_t(0))
    if rc != 0:
        raise ValueError("emu fastq_format rc=%d" % rc)
    return out[:nb.value].tobytes()


def fasta_weights(ix, n, res, guard=None):
    r = _alloc(n, np.uint32, guard); r[:] = res
    w = (C.c_uint64 * 8)()
    rc = lib().fxg_emu_fasta_weights(C.c_void_p(ix["text"].ctypes.data), C.c_void_p(ix["line"].ctypes.data), C.c_uint64(ix["cap_lines"]), C.c_uint64(n),
                                     C.c_void_p(r.ctypes.data), w)
    if rc != 0:
        raise ValueError("emu fasta_weights rc=%d" % rc)
    return list(w)


def clip_table():
    """([(bucket, unit), ...] in the order of csrc/fxg_clip_instances.h, number of units): the engine's table of packed clip instances as the emulator was compiled with it."""
    n = lib().fxg_emu_clip_buckets(None, None, 0)
    b, u = (C.c_int * n)(), (C.c_int * n)()
    assert lib().fxg_emu_clip_buckets(b, u, n) == n
    return list(zip(b, u)), lib().fxg_emu_clip_units()

"""Blocks for the collapser's launch shapes that no recorded case reaches (tests/test_gpu_geometry_collapse.py) and for its arena past 2^31 and 2^32 bytes
(tests/test_gpu_large_offsets_collapse.py), in the style of tests/large_text.py: every byte a pure function of (seed, record index), made by torch on whatever
device it is given, and a closed form for the {sequence: count} multiset.  tests/test_collapse_shapes_cpu.py pins generators and closed forms against
collapse_model.collapse on the same text at sizes Python can parse.  Nothing here needs a GPU at import.

A template t (an integer below 2^24) has bases of any length L: the first twelve spell t in base 4, the rest come from a hash of (seed, t, position), fifteen
bases to a 30-bit word.  Two templates differ in their first twelve bases.  A record is ">" + nine digits of its number [+ "-" + its count] + LF + bases + LF,
so a block of records of one length is a matrix of bytes."""
import collapse_cases as CK
import collapse_model as M

STAGE_BYTES = 49152                      # FXG_CL_STAGE_BYTES
WG = 256                                 # records a workgroup of the insert launch takes
SLOT_TRIP = 65536 * 256                  # slots one trip of a slot launch covers: FXG_CL_SLOT_GRID_MAX * FXG_BLOCK = 2^24
ID_W = 9
M64 = (1 << 64) - 1


# ---- std::hash<std::string> of libstdc++ in Python (pinned against the emulator's export, which test_collapse_cpu.py pins against the library itself) ----
def std_hash(b):
    mul = 0xc6a4a7935bd1e995
    h = 0xc70f6907 ^ (len(b) * mul & M64)
    n8 = len(b) // 8 * 8
    for i in range(0, n8, 8):
        d = int.from_bytes(b[i:i + 8], "little") * mul & M64
        d = (d ^ (d >> 47)) * mul & M64
        h = (h ^ d) * mul & M64
    if len(b) & 7:
        h = (h ^ int.from_bytes(b[n8:], "little")) * mul & M64
    h = (h ^ (h >> 47)) * mul & M64
    return h ^ (h >> 47)


# ---- templates and rows -----------------------------------------------------------------------------------------------------------------------------
def _mix(x):
    """31 bits of hash from a non-negative int64 tensor below 2^32 (every product stays below 2^63)"""
    x = (x * 1103515245 + 12345) & 0x7FFFFFFF
    x = x ^ (x >> 13)
    x = (x * 1664525 + 1013904223) & 0x7FFFFFFF
    return x ^ (x >> 16)


def bases_of(torch, t, L, seed, device="cpu"):
    """(len(t), L) uint8: the bases of templates t (int64 tensor, values below 2^24)"""
    t = t.to(device=device, dtype=torch.int64).reshape(-1, 1)
    k = torch.arange(L, dtype=torch.int64, device=device)
    words = _mix(_mix(t + seed * 7919) + torch.arange((L + 14) // 15, dtype=torch.int64, device=device).reshape(1, -1) * 40503)
    b = (words[:, k // 15] >> (2 * (k % 15))) & 3
    head = min(L, 12)
    b[:, :head] = (t >> (2 * k[:head]).reshape(1, -1)) & 3
    return torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=device)[b]


def template_bytes(torch, t, L, seed):
    """the bases of ONE template as bytes (CPU)"""
    return bytes(bases_of(torch, torch.tensor([t]), L, seed)[0].tolist())


def row_width(L, cw=0):
    return 1 + ID_W + ((1 + cw) if cw else 0) + 1 + L + 1


def rows(torch, g, bases, counts=None, cw=0):
    """(n, row_width) uint8: the records numbered g (int64 tensor) with the given bases rows; counts (int64 tensor) are written as cw zero-padded digits"""
    n, L = bases.shape
    dev = bases.device
    out = torch.empty((n, row_width(L, cw)), dtype=torch.uint8, device=dev)
    out[:, 0] = ord(">")
    g = g.to(dev)
    for d in range(ID_W):
        out[:, ID_W - d] = (48 + (g // 10 ** d) % 10).to(torch.uint8)
    at = 1 + ID_W
    if cw:
        out[:, at] = ord("-")
        c = counts.to(dev)
        for d in range(cw):
            out[:, at + cw - d] = (48 + (c // 10 ** d) % 10).to(torch.uint8)
        at += 1 + cw
    out[:, at] = 10
    out[:, at + 1:at + 1 + L] = bases
    out[:, -1] = 10
    return out


def sums_of(torch, t, L, seed, counts=None):
    """{bases: count} of records with templates t (CPU int64 tensor) in first-occurrence order, by the closed form: a bincount, no parsing"""
    w = counts if counts is not None else torch.ones_like(t)
    top = int(t.max()) + 1
    tot = torch.zeros(top, dtype=torch.int64).index_add_(0, t, w)
    first = torch.full((top,), len(t), dtype=torch.int64).scatter_reduce_(0, t, torch.arange(len(t)), "amin")
    order = torch.argsort(first[tot > 0])
    ts = torch.nonzero(tot > 0).reshape(-1)[order]
    b = bases_of(torch, ts, L, seed)
    return {bytes(b[i].tolist()): int(tot[ts[i]]) & M64 for i in range(len(ts))}


def check_sums(sums, out, exact_order=False):
    """collapse_model.check_against from sums instead of text: ranks 1 .. U, every sequence once with its printed count, descending by the untruncated sums,
    M.out_bytes; exact_order: no two counts are equal, so the bytes are determined"""
    recs = M.parse_output(out)
    assert [r for r, _, _ in recs] == list(range(1, len(sums) + 1))
    assert sorted(b for _, _, b in recs) == sorted(sums)
    assert all(c == M.printed(sums[b]) for _, c, b in recs)
    full = [sums[b] for _, _, b in recs]
    assert full == sorted(full, reverse=True)
    assert len(out) == M.out_bytes(sums)
    if exact_order:
        assert len(set(sums.values())) == len(sums)
        assert out == M.output_in_order(sums, sorted(sums, key=lambda b: -sums[b]))


# ---- 1. slot launches in several trips --------------------------------------------------------------------------------------------------------------
TRIPS_NT, TRIPS_A, TRIPS_L, TRIPS_SEED = 5003, 1237, 36, 5
TRIPS_SLOTS = 1 << 25
TRIPS_N = (1 << 24) + 1


def trips_templates(torch, r0, r1, device="cpu"):
    """templates of records r0 .. r1 of the large block: (r * A) mod 5 003 -- every template n div 5 003 times, and once more where its turn comes early"""
    return (torch.arange(r0, r1, dtype=torch.int64, device=device) * TRIPS_A) % TRIPS_NT


def trips_counts(n):
    """the closed form of the large block's counts per template, as a list: r * A = t (mod NT) has n div NT solutions below n, and one more if the
    smallest solution lies below n mod NT"""
    inv = pow(TRIPS_A, -1, TRIPS_NT)
    return [n // TRIPS_NT + (1 if (t * inv) % TRIPS_NT < n % TRIPS_NT else 0) for t in range(TRIPS_NT)]


def trips_block(torch, r0, r1, table, device):
    """(r1 - r0, 48) uint8 rows of the large block from the table of the 5 003 templates' bases"""
    return rows(torch, torch.arange(r0, r1, dtype=torch.int64, device=device), table[trips_templates(torch, r0, r1, device)])


# ---- 2. the staging boundary ----------------------------------------------------------------------------------------------------------------------------
def staged_spans(block_lens, arena_used=0):
    """per block (a list of record lengths), per workgroup of its insert launch: (b1 - b0, staged) as fxg_kernel_cl_insert works them out from the arena
    offsets -- the 16-byte pieces that hold the workgroup's records"""
    out = []
    for lens in block_lens:
        offs, at = [], arena_used
        for n in lens:
            offs.append(at)
            at += n
        spans = []
        for r0 in range(0, len(lens), WG):
            last = min(r0 + WG, len(lens)) - 1
            b0, b1 = offs[r0] & ~15, (offs[last] + lens[last] + 15) & ~15
            spans.append((b1 - b0, b1 - b0 <= STAGE_BYTES))
        out.append(spans)
        arena_used = at
    return out


def boundary_case(lead):
    """[blocks of (name, bases)]: a lead record of `lead` bases, 256 records of 192 bases (the workgroup's first arena offset is `lead`), a pad record that
    moves the offset to the other side of the boundary, and the 256 again in another order with 40 new ones among them: every duplicate's first occurrence
    lies in a workgroup of the other kind"""
    pad = 1 if lead % 16 in (0, 15) else 15
    first = [(CK.ident(i), CK.seq(1000 + i % 200, 192)) for i in range(256)]                      # (56 duplicates inside the workgroup too)
    again = [(CK.ident(300 + i), CK.seq(1000 + (i * 7) % 200 if i % 6 else 5000 + i, 192)) for i in range(256)]
    return [[(b"lead", CK.seq(7, lead))], first, [(b"pad-3", CK.seq(9, pad))], again]


def alternating_case(groups=6):
    """one block of `groups` workgroups, 150-base and 250-base groups of 256 in turn; six records of each group have the other length and repeat a sequence
    first seen in the group before (of the other kind), and every group repeats sequences of the group two before it"""
    recs = []
    for g in range(groups):
        own, other = (150, 250) if g % 2 == 0 else (250, 150)
        for i in range(WG):
            r = g * WG + i
            if i % 43 == 7:                                  # six of them: i = 7, 50, 93, 136, 179, 222
                recs.append((CK.ident(r), CK.seq(10000 * (g - 1) + i + 1 if g else 90000 + i, other)))
            elif i % 5 == 0 and g >= 2:
                recs.append((CK.ident(r), CK.seq(10000 * (g - 2) + i + 1, own)))
            else:
                recs.append((CK.ident(r), CK.seq(10000 * g + i, own)))
    return [recs]


# ---- 3. contention ----------------------------------------------------------------------------------------------------------------------------------------
CONT_L, CONT_CW, CONT_SINGLES = 36, 10, 1000


def contention_block(np, n, count):
    """(text, sums): n records of which CONT_SINGLES (fewer when n is small), spread evenly, are singletons with the distinct counts 1, 2, ... and the rest one
    36-base read with `count` in its id; sums by the closed form, in first-occurrence order.  No two counts are equal, so the output is determined."""
    singles = min(CONT_SINGLES, n // 4)
    W = row_width(CONT_L, CONT_CW)
    X = np.frombuffer(CK.seq(0, CONT_L), np.uint8)
    rows_ = np.empty((n, W), np.uint8)
    rows_[:, 0] = ord(">")
    g = np.arange(n)
    for d in range(ID_W):
        rows_[:, ID_W - d] = 48 + g // 10 ** d % 10
    rows_[:, 1 + ID_W] = ord("-")
    rows_[:, 2 + ID_W:2 + ID_W + CONT_CW] = np.frombuffer(b"%0*d" % (CONT_CW, count), np.uint8)
    at = 2 + ID_W + CONT_CW
    rows_[:, at] = 10
    rows_[:, at + 1:at + 1 + CONT_L] = X
    rows_[:, -1] = 10
    step = n // singles
    where = {}
    for j in range(singles):
        p = j * step + (j * 7) % (step - 1) + 1              # never record 0: the common read comes first
        where[p] = j
        rows_[p, 2 + ID_W:2 + ID_W + CONT_CW] = np.frombuffer(b"%0*d" % (CONT_CW, j + 1), np.uint8)
        rows_[p, at + 1:at + 1 + CONT_L] = np.frombuffer(CK.seq(j + 1, CONT_L), np.uint8)
    sums = {CK.seq(0, CONT_L): (n - singles) * count & M64}
    for p in sorted(where):
        sums[CK.seq(where[p] + 1, CONT_L)] = where[p] + 1
    return rows_.tobytes(), sums


# ---- 4. the arena past 2^31 and 2^32 ------------------------------------------------------------------------------------------------------------------
class Arena:
    """R records of L bases whose arena offsets g * L pass m31 and m32 + m32 / 16, with templates placed by record number:
         lo   (a record that begins below m31)   itself; one in sixteen repeats the record eleven before it
         mid  (begins below m32)                 itself; one in eight repeats a record of lo
         hi   (begins above m32)                 in turn: itself (a sequence that occurs only up here), a repeat of a record of lo, a repeat of a record of
                                                 mid, a repeat of the hi record three before it
    A template's number is the number of its first record.  The real case: L = 24 997 (the longest line the index takes, so the fewest records), m31 = 2^31,
    m32 = 2^32; the CPU tier parses the same construction at L = 97 with the marks at 2^14 and 2^15."""

    def __init__(self, L=CK.LONGEST, m31=1 << 31, m32=1 << 32, seed=9):
        self.L, self.m31, self.m32, self.seed = L, m31, m32, seed
        self.mark = m32 + m32 // 16                          # 2^32 + 2^28
        self.R = self.mark // L + 1                          # the smallest count whose bases end above the mark
        self.G31, self.G32 = m31 // L + 1, m32 // L + 1
        self.Z = self.G31 // 16 * 16
        self.M0 = self.G31 - self.G31 % 8 + 8                # the first multiple of 8 inside mid
        self.Zm = (self.G32 - self.M0) // 8 * 8
        assert self.R * L > self.mark >= (self.R - 1) * L and self.Z >= 32 and self.Zm >= 16 and self.R < 1 << 24

    def templates(self, torch, g0, g1, device="cpu"):
        g = torch.arange(g0, g1, dtype=torch.int64, device=device)
        j = g - self.G32
        lo = torch.where((g % 16 == 5) & (g >= 16), g - 11, g)
        mid = torch.where(g % 8 == 3, ((g - self.G31) // 16 * 16 + 32) % self.Z, g)
        hi = torch.where(j % 4 == 0, g, torch.where(j % 4 == 1, (j * 16 + 48) % self.Z, torch.where(j % 4 == 2, self.M0 + (j * 8) % self.Zm, g - 3)))
        return torch.where(g < self.G31, lo, torch.where(g < self.G32, mid, hi))

    def blocks(self):
        """record ranges of the blocks, each block's text within the text path's 0xFFFFFFF0 bytes: as few as that allows, of nearly equal size"""
        per = 0xFFFFFFF0 // row_width(self.L)
        ways = -(-self.R // per)
        return [(self.R * k // ways, self.R * (k + 1) // ways) for k in range(ways)]

    def text_rows(self, torch, g0, g1, device):
        return rows(torch, torch.arange(g0, g1, dtype=torch.int64, device=device), bases_of(torch, self.templates(torch, g0, g1, device), self.L, self.seed, device))

    def counts(self, torch):
        """(the templates that occur, their counts) by bincount over all R records"""
        t = self.templates(torch, 0, self.R)
        tot = torch.bincount(t, minlength=self.R)
        ts = torch.nonzero(tot).reshape(-1)
        return ts, tot[ts]

    def aliases(self, torch):
        """for every record above m32: the templates of the one or two records whose bytes lie at its offset taken modulo m32"""
        g = torch.arange(self.G32, self.R, dtype=torch.int64)
        at = g * self.L - self.m32
        a, b = at // self.L, (at + self.L - 1) // self.L
        t = self.templates(torch, 0, self.R)
        return t[g], t[a], t[b]


class Seq:
    """stands in for a sequence of L bases where only its length and identity matter (collapse_model.out_bytes over 180 000 sequences of 25 KB)"""

    def __init__(self, t, L):
        self.t, self.L = t, L

    def __len__(self):
        return self.L

    def __hash__(self):
        return hash(self.t)

    def __eq__(self, o):
        return self.t == o.t

"""CPU tier: the reference code of tests/test_gpu_large_offsets.py (tests/large_offsets.py) against the oracle, so that the GPU test does not
trust it on its own word: the closed forms of the whole-stream checks, the read lengths of the ragged shape from torch and from numpy, the
history-free oracle of the ragged clip windows, the window placement, and the case table's N literals against the size rule."""
import numpy as np
import pytest

import large_offsets as lo
from helpers import oracle_params
from oracle import fxoracle_py as fo

FAMS = lo.families()


def test_case_table_covers_every_family():
    from test_gpu_geometry import FAM
    assert set(lo.CASES) == set(FAM) | set(lo.EXTRA) and len(lo.CASES) == 19
    for fam, c in lo.CASES.items():
        f = FAMS[fam]
        assert set(c) - {"N"} == set(lo.shapes(fam)), fam
        assert c["N"] <= 0xFFFFFFFF and c["N"] % lo.ROUND == 0
        assert c["fixed"] == (lo.MARKS, lo.MARKS), fam
        assert lo.crossed(c["N"] * f["stride"]) == lo.MARKS, fam
        for shape in lo.shapes(fam)[1:]:
            assert c[shape][0] == lo.MARKS and set(c[shape][1]) >= {31, 32}, (fam, shape)
    assert lo.crossed(lo.STATS["N"] * lo.STATS["stride"]) == lo.MARKS
    # the two long clip forms: checkpoints in scratch (clip40k), one pass without (clip72)
    assert not lo.clip_one_pass(len(FAMS["clip40k"]["pd"]["adapter"]), FAMS["clip40k"]["stride"])
    assert lo.clip_one_pass(len(lo.AD72), FAMS["clip72"]["stride"]) and lo.clip_one_pass(72, 97)
    assert lo.crossed(1 << 32) == (31,) and lo.crossed((1 << 32) + 1) == (31, 32) and lo.crossed(lo.TARGET) == lo.MARKS


@pytest.mark.parametrize("fam", sorted(lo.CASES))
def test_n_literals_follow_from_the_oracle_prefix(fam):
    """(iv) N = the smallest multiple of ROUND at which the oracle's kept bytes per read (first PREFIX reads, fixed shape) reach TARGET; the
    ragged and padded outputs the oracle predicts at that N cross the declared marks with margin (>= 1.5 GiB over 2^32, >= 0.4 % off 2^33)."""
    f, c = FAMS[fam], lo.CASES[fam]
    kept, kb = lo.prefix_kept_bytes(f)
    assert lo.size_rule(kb) == c["N"], (fam, kb, lo.size_rule(kb))
    assert kb <= f["stride"] * lo.PREFIX                    # the input array is never the smaller one
    import torch
    row = torch.zeros((1, f["stride"]), dtype=torch.uint8)
    if lo.closed_form(torch, fam, f, row, row) is not None:
        assert kept == lo.PREFIX, fam                       # the whole-stream checks need every read kept
    for shape in lo.shapes(fam)[1:]:
        _, kb2 = lo.prefix_kept_bytes(f, shape)
        pred = c["N"] * kb2 / lo.PREFIX
        assert lo.crossed(int(pred)) == c[shape][1], (fam, shape, pred / 2**30)
        assert pred > (1 << 32) + 1.5 * 2**30 and abs(pred - (1 << 33)) > 0.004 * (1 << 33), (fam, shape, pred / 2**30)


@pytest.mark.parametrize("stride", [100, 150, 158])
def test_closed_forms_equal_the_oracle(stride):
    """(i) fixed shape, every stage that has a closed form, at strides 100, 150, 158."""
    import torch
    n = 3001
    b, q = fo.synth_batch(lo.SEED, 12345, n, stride, False, stride)
    tb, tq = torch.from_numpy(b), torch.from_numpy(q)
    seen = 0
    for fam, f in FAMS.items():
        if f["pd"]["stages"] not in (8, 16, 24, 64, 128):
            assert lo.closed_form(torch, fam, f, tb, tq) is None, fam
            continue
        pd = dict(f["pd"])
        if "ft_last" in pd:
            pd["ft_last"] = min(pd["ft_last"], stride - 5)
        f2 = dict(f, stride=stride, pd=pd)
        eb, eq = lo.closed_form(torch, fam, f2, tb, tq)
        o = fo.run_pipeline(b, q, None, oracle_params(pd))
        assert int(o["counters"][fo.C_KEPT]) == n, fam
        assert np.array_equal(eb.reshape(-1).numpy(), o["out_bases"]) and np.array_equal(eq.reshape(-1).numpy(), o["out_qual"]), (fam, stride)
        assert len(set(o["res"].tolist())) == 1 and set(o["out_len"].tolist()) == {eb.shape[1]}, fam
        seen += 1
    assert seen == 5
    assert int((tq.to(torch.int16) - 33 < 20).sum()) > n and int((tb == ord("N")).sum()) > 0      # the masker and the complement of N have work


def test_ragged_lengths_torch_equals_numpy():
    """(ii) the lens hash from torch and from numpy, also for read indices above 2^31 and 2^32; its distribution."""
    import torch
    for r0 in (0, 1, (1 << 31) - 1500, (1 << 32) - 1500, 506_999_000, (1 << 40) + 7):
        for stride, pd in ((36, None), (100, dict(stages=4)), (150, dict(stages=6)), (304, None)):
            a = lo.lens_numpy(r0, 3000, stride, pd)
            t = lo.lens_torch(torch, r0, 3000, stride, pd)
            assert t.dtype == torch.int16 and np.array_equal(t.numpy().view(np.uint16), a), (r0, stride)
            assert a.max() <= stride and a.min() >= (1 if pd and lo.needs_one(pd) else 0)
    a = lo.lens_numpy(0, 1_000_000, 150).astype(np.int64)
    assert (a == 0).sum() > 200 and (a < 75).sum() > 20000 and (a == 150).sum() > 10000          # empty and tiny reads stay present
    assert abs(a.mean() - (15 / 16 * 112.5 + 75 / 16)) < 0.5
    assert lo.lens_numpy(0, 100000, 150, dict(stages=4)).min() == 1
    big = lo.lens_torch(torch, 5, lo.SLAB + 77, 50)                                             # more than one slab
    assert np.array_equal(big.numpy().view(np.uint16), lo.lens_numpy(5, lo.SLAB + 77, 50))


def test_ragged_clip_windows_go_through_the_oracle_read_by_read():
    """The engine without clip history aligns every read on its own; oracle_window() must give the oracle's answer for each read alone, in read order,
    and must be the plain oracle wherever lengths are equal or no clipper runs."""
    for fam in ("clip13", "cfg5", "clip72"):
        f = FAMS[fam]
        st, n = f["stride"], 400
        b, q = fo.synth_batch(lo.SEED, 999, n, st, True, st)
        lens = lo.lens_numpy(999, n, st, f["pd"])
        o = lo.oracle_window(f, b, q, 999, "ragged")
        ob, oq, ol, ki = [], [], [], []
        for i in range(n):
            one = fo.run_pipeline(b[i:i + 1], q[i:i + 1], lens[i:i + 1], oracle_params(f["pd"]))
            assert one["res"][0] == o["res"][i], (fam, i)
            if len(one["kept_index"]):
                ob.append(one["out_bases"]); oq.append(one["out_qual"]); ol.append(int(one["out_len"][0])); ki.append(i)
        assert np.array_equal(np.concatenate(ob), o["out_bases"]) and np.array_equal(np.concatenate(oq), o["out_qual"]), fam
        assert o["out_len"].tolist() == ol and o["kept_index"].tolist() == ki and o["out_len"].dtype == np.uint16 and o["kept_index"].dtype == np.uint32
        assert int(o["counters"][fo.C_KEPT]) == len(ki) and int(o["counters"][fo.C_KEPT_BASES]) == sum(ol)
        for shape in ("fixed", "padded"):
            fl = st - lo.PAD if shape == "padded" else st
            a, p = lo.oracle_window(f, b, q, 999, shape), fo.run_pipeline(b, q, None, oracle_params(f["pd"]), fixed_len=fl)
            assert all(np.array_equal(a[k], p[k]) for k in ("res", "out_bases", "out_qual", "out_len", "kept_index")), (fam, shape)
    f = FAMS["rows38"]
    b, q = fo.synth_batch(lo.SEED, 5, 300, 150, False, 150)
    a, p = lo.oracle_window(f, b, q, 5, "ragged"), fo.run_pipeline(b, q, lo.lens_numpy(5, 300, 150, f["pd"]), oracle_params(f["pd"]))
    assert all(np.array_equal(a[k], p[k]) for k in ("res", "out_bases", "out_qual", "out_len", "kept_index"))


def test_windows_hold_their_marks():
    """(iii) given a synthetic out_off, the windows contain the mark: on a read boundary, one byte either side, in a run of dropped reads, behind
    reads kept with no bytes, near both ends of the batch; input windows hold the row of the mark; torch and numpy agree."""
    import torch
    rng = np.random.default_rng(4)
    n, stride = 50_000, 100
    keep = rng.random(n) < 0.6
    keep[20_000:27_000] = False                              # a run of dropped reads (longer than a window)
    ln = np.where(keep, rng.integers(0, stride + 1, size=n), 0).astype(np.int64)
    ln[30_000:30_050] = 0                                    # kept with no bytes
    kept_index = np.nonzero(keep)[0].astype(np.int32)
    ol = ln[keep]
    out_off = np.cumsum(ol) - ol
    total = int(ol.sum())
    rank_of = np.concatenate([[0], np.cumsum(keep)])
    k20 = int(rank_of[20_000])
    marks = [int(out_off[k20]), int(out_off[k20]) - 1, int(out_off[k20]) + 1, int(out_off[k20 - 1]), int(out_off[rank_of[30_020]]),
             0, 1, total - 1, int(out_off[5]), int(out_off[len(out_off) - 3]) + 1] + [int(x) for x in rng.integers(0, total, size=200)]
    for m in marks:
        rd = lo.output_mark_read(out_off, kept_index, m)
        assert rd == lo.output_mark_read(torch.from_numpy(out_off), torch.from_numpy(kept_index), m)
        k = int(rank_of[rd])
        assert keep[rd] and out_off[k] <= m < out_off[k] + ol[k], m        # the read whose kept bytes hold byte m
        r0 = lo.window_start(rd, n)
        assert 0 <= r0 <= rd < r0 + lo.KI <= n
        o0 = int(out_off[rank_of[r0]]) if rank_of[r0] < len(out_off) else total
        nw = int(ln[r0:r0 + lo.KI].sum())
        assert o0 <= m < o0 + nw, (m, o0, nw)                # the window's packed bytes hold byte m
        if lo.KI // 2 <= rd <= n - lo.KI:
            assert rd - r0 == lo.KI // 2                     # centred: five whole tiles of 256 reads on each side
    for m in (0, 99, 100, 149_999, 150_000, 150_001, n * stride - 1):
        rd = lo.input_mark_read(m, stride)
        r0 = lo.window_start(rd, n)
        assert r0 * stride <= m < (r0 + lo.KI) * stride and 0 <= r0 <= n - lo.KI
    w = lo.windows(n, stride, (31,), (), out_off, kept_index, 7)
    assert w[0] == ("prefix", 0, None, None) and sorted(x[0] for x in w[-2:]) == ["input 2^31", "suffix"] and sum(x[0] == "random" for x in w) == lo.RANDOM_WINDOWS
    assert ("input 2^31", n - lo.KI, "in", 1 << 31) in w
    assert [x[1] for x in w] == sorted(x[1] for x in w)      # in read order
    assert all(0 <= x[1] <= n - lo.KI for x in w) and w == lo.windows(n, stride, (31,), (), out_off, kept_index, 7)
    assert total > 1 << 20
    (label, r0, side, mark), = [x for x in lo.windows(n, stride, (), (20,), out_off, kept_index, 7) if x[2] == "out"]
    o0 = int(out_off[rank_of[r0]])
    assert label == "output 2^20" and mark == 1 << 20 and o0 <= mark < o0 + int(ln[r0:r0 + lo.KI].sum())
    assert lo.KI // 2 >= 5 * 256 + 128

"""The matrix-core Hamming matcher against a numpy popcount model, on the inputs where an inexact key would show.

The kernel keeps (distance, train index) as one number, 8192 d + j plus a constant, in an f32 accumulator of the FP4
matrix instruction.  That is exact only while every distance 0..256, every index 0..8191 and every rebasing step of the
running keys stay inside the 24-bit significand, so the cases below put each distance in the best and in the second
slot, equal distances at the first and the last possible train index, train sets around the 32-row tile and at the
8192-row limit, query counts around a wavefront's share (128 or 256 queries), and empty and unequal sets inside a batch.
"""
import numpy as np
import pytest

from weiner_slamit_v2_amd import api

pytestmark = pytest.mark.gpu

_POP = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(1).astype(np.uint8)


def _model(q, t):
    """best = smallest distance with the FIRST index on ties, second = second smallest value of the multiset;
    (-1, 256, 256) without train rows, second = 256 with one."""
    nq, nt = len(q), len(t)
    idx, best, second = np.full(nq, -1, np.int32), np.full(nq, 256, np.int32), np.full(nq, 256, np.int32)
    if nt == 0:
        return idx, best, second
    for i0 in range(0, nq, 64):
        d = _POP[q[i0:i0 + 64, None, :] ^ t[None, :, :]].sum(-1, dtype=np.int32)
        rows = np.arange(len(d))
        b = d.argmin(1)
        idx[i0:i0 + 64], best[i0:i0 + 64] = b, d[rows, b]
        if nt > 1:
            d[rows, b] = 1 << 20
            second[i0:i0 + 64] = d.min(1)
    return idx, best, second


def _flip(row, k, rs):
    """row with exactly k of its 256 bits flipped"""
    bits = np.unpackbits(row)
    bits[rs.choice(256, k, replace=False)] ^= 1
    return np.packbits(bits)


def _check(q, t, tag):
    gi, gb, gs = api.ORBmatcher.best2(q, t)
    mi, mb, ms = _model(q, t)
    assert np.array_equal(gi, mi), "%s: best index differs at queries %s" % (tag, np.flatnonzero(gi != mi)[:8])
    assert np.array_equal(gb, mb), "%s: best distance differs at queries %s" % (tag, np.flatnonzero(gb != mb)[:8])
    assert np.array_equal(gs, ms), "%s: second distance differs at queries %s" % (tag, np.flatnonzero(gs != ms)[:8])
    return gi, gb, gs


def _batch(qs, ts):
    """slamit_hamming_best2_batch_dev on pairs of unequal sizes; returns the three (P, cap) outputs, prefilled with -7"""
    import torch

    p = len(qs)
    cap = max(max(len(x) for x in qs), max(len(x) for x in ts), 1)
    hq, ht = np.zeros((p, cap, 32), np.uint8), np.zeros((p, cap, 32), np.uint8)
    for i in range(p):
        hq[i, :len(qs[i])], ht[i, :len(ts[i])] = qs[i], ts[i]
    d_q, d_t = torch.from_numpy(hq).cuda(), torch.from_numpy(ht).cuda()
    d_nq = torch.tensor([len(x) for x in qs], dtype=torch.int32, device="cuda")
    d_nt = torch.tensor([len(x) for x in ts], dtype=torch.int32, device="cuda")
    outs = [torch.full((p, cap), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    api.ORBmatcher.best2_batch_dev(d_q, d_nq, d_t, d_nt, outs[0], outs[1], outs[2], cap, device=0,
                                   stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _check_batch(qs, ts, tag):
    gi, gb, gs = _batch(qs, ts)
    for p, (q, t) in enumerate(zip(qs, ts)):
        mi, mb, ms = _model(q, t)
        n = len(q)
        assert np.array_equal(gi[p, :n], mi), "%s pair %d: best index" % (tag, p)
        assert np.array_equal(gb[p, :n], mb), "%s pair %d: best distance" % (tag, p)
        assert np.array_equal(gs[p, :n], ms), "%s pair %d: second distance" % (tag, p)
        for o in (gi, gb, gs):
            assert (o[p, n:] == -7).all(), "%s pair %d: wrote past its %d queries" % (tag, p, n)
    return gi, gb, gs


def _designed_pair(best, second, rs, nt=40):
    """3 queries and nt train rows; query 0 has exactly `best` as its smallest and `second` as its second smallest
    distance (best <= second), at random rows, every other row at `second` or farther"""
    q = rs.randint(0, 256, (3, 32)).astype(np.uint8)
    far = [int(rs.randint(second, 257)) for _ in range(nt)]
    ib, isec = rs.choice(nt, 2, replace=False)
    far[ib], far[isec] = best, second
    t = np.stack([_flip(q[0], k, rs) for k in far])
    return q, t


def test_every_distance_as_best():
    rs = np.random.RandomState(11)
    want = [(d, d + (5 * d) % (257 - d)) for d in range(257)]
    pairs = [_designed_pair(b, s, rs) for b, s in want]
    gi, gb, gs = _check_batch([p[0] for p in pairs], [p[1] for p in pairs], "best 0..256")
    assert [int(x) for x in gb[:, 0]] == [b for b, _ in want]
    assert [int(x) for x in gs[:, 0]] == [s for _, s in want]


def test_every_distance_as_second():
    rs = np.random.RandomState(12)
    want = [(s - (3 * s) % (s + 1), s) for s in range(257)]
    pairs = [_designed_pair(b, s, rs) for b, s in want]
    gi, gb, gs = _check_batch([p[0] for p in pairs], [p[1] for p in pairs], "second 0..256")
    assert [int(x) for x in gb[:, 0]] == [b for b, _ in want]
    assert [int(x) for x in gs[:, 0]] == [s for _, s in want]


def test_equal_distances_first_index_wins_up_to_the_last_row():
    rs = np.random.RandomState(13)
    nt = 8192
    q = rs.randint(0, 256, (6, 32)).astype(np.uint8)
    t = rs.randint(0, 256, (nt, 32)).astype(np.uint8)       # ~128 away from everything
    t[0], t[4000], t[8191] = _flip(q[0], 9, rs), _flip(q[0], 9, rs), _flip(q[0], 9, rs)       # 0 beats 4000 and 8191
    t[5000], t[8190] = _flip(q[1], 30, rs), _flip(q[1], 30, rs)                             # 5000 beats 8190
    t[31], t[32] = _flip(q[2], 0, rs), _flip(q[2], 0, rs)                                   # distance 0 twice, across a tile edge
    t[8189] = _flip(q[3], 17, rs)                                                           # a lone best near the end
    t[1] = _flip(q[4], 256, rs)
    t[8188] = _flip(q[4], 2, rs)
    gi, gb, gs = _check(q, t, "ties at nt = 8192")
    assert (gi[0], gb[0], gs[0]) == (0, 9, 9)
    assert (gi[1], gb[1], gs[1]) == (5000, 30, 30)
    assert (gi[2], gb[2], gs[2]) == (31, 0, 0)
    assert (gi[3], gb[3]) == (8189, 17)
    assert (gi[4], gb[4]) == (8188, 2)
    # the last row alone holds the minimum, then shares it with row 0
    t2 = t.copy()
    t2[8191] = _flip(q[5], 3, rs)
    gi, gb, gs = _check(q, t2, "best at row 8191")
    assert (gi[5], gb[5]) == (8191, 3)
    t2[0] = _flip(q[5], 3, rs)
    gi, gb, gs = _check(q, t2, "rows 0 and 8191 tie")
    assert (gi[5], gb[5], gs[5]) == (0, 3, 3)
    # identical rows everywhere: every distance equal, index 0 wins, second equals best
    same = np.repeat(rs.randint(0, 256, (1, 32)).astype(np.uint8), nt, axis=0)
    gi, gb, gs = _check(q, same, "8192 identical rows")
    assert (gi == 0).all() and np.array_equal(gb, gs)


@pytest.mark.parametrize("nt", [1, 31, 32, 33, 127, 128, 129, 8191, 8192])
def test_train_set_sizes_and_query_counts(nt):
    rs = np.random.RandomState(100 + nt)
    hi = 4 if nt < 1000 else 256          # few distinct byte values: many equal distances
    t = rs.randint(0, hi, (nt, 32)).astype(np.uint8)
    for nq in (1, 31, 33, 127, 128, 129, 255, 256, 257, 300):
        q = rs.randint(0, hi, (nq, 32)).astype(np.uint8)
        q[nq - 1] = t[nt - 1]             # the last query meets the last train row
        gi, gb, gs = _check(q, t, "nq %d nt %d" % (nq, nt))
        assert gb[nq - 1] == 0
    if nt >= 8191:                        # low-entropy rows at the limit: equal keys differ in the index alone
        t4 = rs.randint(0, 2, (nt, 32)).astype(np.uint8)
        _check(rs.randint(0, 2, (130, 32)).astype(np.uint8), t4, "low entropy nt %d" % nt)


def test_empty_sets_in_the_middle_of_a_batch():
    rs = np.random.RandomState(14)
    nq = [130, 0, 257, 5, 300, 64, 0, 129]
    nt = [33, 50, 0, 129, 1, 300, 0, 257]
    qs = [rs.randint(0, 4, (n, 32)).astype(np.uint8) for n in nq]
    ts = [rs.randint(0, 4, (n, 32)).astype(np.uint8) for n in nt]
    gi, gb, gs = _check_batch(qs, ts, "empty sets")
    assert (gi[2, :257] == -1).all() and (gb[2, :257] == 256).all() and (gs[2, :257] == 256).all()
    assert (gi[4, :300] == 0).all() and (gs[4, :300] == 256).all()       # one train row: no second


def test_batch_of_unequal_pairs():
    rs = np.random.RandomState(15)
    nq = [1000, 1, 255, 513, 128, 31, 777, 256]
    nt = [997, 1000, 1, 64, 1000, 33, 95, 513]
    qs = [rs.randint(0, 256, (n, 32)).astype(np.uint8) for n in nq]
    ts = [rs.randint(0, 256, (n, 32)).astype(np.uint8) for n in nt]
    ts[0][500] = qs[0][3]
    ts[3][63] = qs[3][512]
    gi, gb, gs = _check_batch(qs, ts, "unequal pairs")
    assert (gi[0, 3], gb[0, 3]) == (500, 0) and (gi[3, 512], gb[3, 512]) == (63, 0)

"""Conditions on the sparse-sender edge inputs (tests/_sparse_edges.py) and on the oracle they
are checked against, so that tests/test_gpu_sparse_senders.py cannot silently lose the coverage
it is written for.  No GPU.

  * every family meets its claim at every flat size and ratio: the class of the k-th key T,
    the special-value counts against k, the sampled / hidden placements against sample_runs;
  * O.topk / O.topk_segmented equal an independent restatement -- the k first entries of
    np.lexsort((index, -key)), re-sorted by index -- indices equal, values bit for bit;
  * where the answer is unambiguous (top_few, huge: no tie at T) the index set is that of
    torch.topk(d.abs(), k) on the CPU;
  * the read-only forms reach the oracle with their stored bits (NaN payloads included).
"""
import numpy as np
import pytest
import torch

import _sparse_edges as E
from conftest import same_bits
from oracle import choco_oracle as O

F32 = np.float32
U32 = np.uint32


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


def restated_topk(d, k):
    """The k first entries by (key descending, index ascending), re-sorted by index."""
    key = E.keys_of(d).astype(np.int64)
    order = np.lexsort((np.arange(d.size), -key))
    idx = np.sort(order[:k]).astype(np.int64)
    return d[idx], idx


def deltas(case):
    """The deltas a case is compressed as: read-only / xhat form, and the gossip form."""
    out = [("d", case.delta())]
    if case.xhat is not None:
        out.append(("gossip", case.gossip()[1]))
    return out


def test_sample_runs_geometry():
    for n in (65537, 163877, 3_000_011):
        runs = E.sample_runs(n)
        assert len(runs) == 64 and runs[0][0] == 0 and runs[-1][1] <= n
        assert all(b - a == 256 and a % 4 == 0 for a, b in runs)
        assert all(runs[j][1] <= runs[j + 1][0] for j in range(63))     # disjoint, ascending
        assert int(E.in_sample(n).sum()) == 16384
    assert E.sample_runs(163877)[1][0] == 4 * ((163877 - 256) // 63 >> 2) == 2596


def test_placed_positions():
    assert E.placed(163877, E.FLAT_TILE).tolist() == [0, 32767, 32768, 65535, 65536, 98303, 98304, 131071, 131072,
                                                       163839, 163840, 163876]
    assert E.placed(65537, E.FLAT_TILE).tolist() == [0, 32767, 32768, 65535, 65536]
    assert E.placed(16385, E.SEG_TILE).tolist() == [0, 16383, 16384]
    assert E.placed(1, E.SEG_TILE).tolist() == [0]


@pytest.mark.parametrize("ratio", E.RATIOS)
@pytest.mark.parametrize("n", E.FLAT_SIZES)
def test_family_claims(n, ratio):
    k = E.topk_k(n, ratio)
    assert k == O.topk_k(n, ratio) and k >= 40
    tile_pos = E.placed(n, E.FLAT_TILE)
    for computed in (False, True):
        for tag in E.tags(n, ratio, computed):
            case = E.build(tag, n, k, computed)
            assert (case.xhat is None) == (not computed), tag
            d = case.delta()
            key = O.keys(d).astype(np.int64)
            T = E.kth_key(d, k)
            isn, isi = np.isnan(d), np.isinf(d)
            name = tag.split("-")[0]
            what = (tag, n, ratio, computed)
            if name == "top_few":
                nsp = int((key >= E.KEY_FLT_MAX).sum())
                assert nsp == E.N_SPECIAL < k and T < E.KEY_FLT_MAX, what
                assert (key[tile_pos] >= E.KEY_FLT_MAX).all(), what                  # placed
                assert isn.sum() == 8 and isi.sum() == 8, what
                assert np.all(key[O.topk(d, k)[1]] >= T) and set(np.nonzero(key >= E.KEY_FLT_MAX)[0]) <= set(
                    O.topk(d, k)[1].tolist()), what
            elif name == "nan_flood":
                m = E.flood_count(n, k)
                assert int(isn.sum()) == m > k and T > E.KEY_INF, what
                if computed:
                    assert np.all(key[isn] == E.KEY_QNAN) and np.isfinite(case.xhat[isn]).all(), what
                    assert np.all(case.xhat[isn] != 0), what
                else:
                    assert set(np.unique(key[isn]).tolist()) == {E.KEY_QNAN | p for p in E.NAN_PAYLOADS}, what
                    assert len(np.unique(bits(d)[isn])) == 16, what                  # both signs
                    assert int((key == T).sum()) > 1 and int((key > T).sum()) < k, what   # ties at a payload
            elif name == "inf_flood":
                m = E.flood_count(n, k)
                assert int(isi.sum()) == m and int(isn.sum()) == 5 and T == E.KEY_INF, what
                assert (d[isi] > 0).any() and (d[isi] < 0).any(), what
            elif name == "huge":
                fin = ~isi
                assert not isn.any() and key[fin].min() >= E.KEY_2P126, what
                assert int((key == E.KEY_FLT_MAX).sum()) == k // 2 + 1, what
                assert T < E.KEY_FLT_MAX and int((key == T).sum()) == 1, what
                if computed:
                    assert 0 < int(isi.sum()) <= 16 < k, what
                    assert np.all(np.signbit(case.x) != np.signbit(case.xhat)), what
            elif name == "subnormal":
                assert key.max() < E.KEY_MIN_NORMAL, what
                assert np.all(bits(d)[::7] == 0x80000000), what
                assert 0.45 * n < int((key == 0).sum()) < 0.55 * n, what
                assert (T == 0) if ratio == 0.5 else (0 < T < E.KEY_MIN_NORMAL), what
                if computed:
                    nzd = key != 0
                    assert O.keys(case.x)[nzd].min() >= E.KEY_MIN_NORMAL, what
                    assert O.keys(case.xhat)[nzd].min() >= E.KEY_MIN_NORMAL, what
            elif name == "zeros_few":
                assert int((key != 0).sum()) == k // 2 < k and T == 0, what
                sel = O.topk(d, k)[1]
                assert (bits(d)[sel] == 0x80000000).any() and (bits(d)[sel] == 0).any(), what
            elif name == "digit_edges":
                B = E.digit_B(tag)
                assert set(np.unique(key).tolist()) <= {B - 1, B, B + 1} and T == B, what
                ties = np.nonzero(key == B)[0]
                r = k - int((key > B).sum())
                assert 0 < r < ties.size, what
                if n > E.FLAT_TILE:     # the selected ties lie on both sides of the first tile edge
                    assert ties[0] < E.FLAT_TILE <= ties[r - 1], what
                if tag.endswith("span"):
                    assert (B - 1) >> 9 == (B + 1) >> 9, what
                else:
                    assert (B - 1) >> 9 != B >> 9, what
            elif name == "inf_minus_inf":
                both = np.isinf(case.x) & np.isinf(case.xhat)
                assert 0 < int(both.sum()) <= 32 and isn[both].all(), what           # arithmetic NaNs
                assert (np.isinf(case.x) & np.isfinite(case.xhat)).any(), what
                assert (np.isfinite(case.x) & np.isinf(case.xhat)).any(), what
                assert (np.isnan(case.x) & np.isfinite(case.xhat)).any(), what
            else:
                raise AssertionError(tag)
            if tag.endswith(("sampled", "hidden")):
                ins = E.in_sample(n)
                sp = isn if name == "nan_flood" else isi
                if tag.endswith("hidden"):
                    assert not (sp & ins).any(), what
                else:
                    assert int((sp & ins).sum()) == min(E.flood_count(n, k), 16384), what


@pytest.mark.parametrize("n", E.FLAT_SIZES)
def test_oracle_topk_equals_restatement(n):
    """O.topk against the lexsort restatement on every family, ratio and form."""
    for ratio in E.RATIOS:
        k = E.topk_k(n, ratio)
        for computed in (False, True):
            for tag in E.tags(n, ratio, computed):
                case = E.build(tag, n, k, computed)
                for form, d in deltas(case):
                    ov, oi = O.topk(d, k)
                    rv, ri = restated_topk(d, k)
                    assert np.array_equal(oi, ri), (tag, n, ratio, form)
                    assert np.array_equal(bits(ov), bits(rv)), (tag, n, ratio, form)


@pytest.mark.parametrize("ratio", E.RATIOS + [0.0])
def test_oracle_topk_segmented_equals_restatement(ratio):
    lens = E.SEG_LAYOUT
    for computed in (False, True):
        for tag in E.seg_tags(computed):
            case = E.segmented(tag, ratio, computed)
            assert case.x.size == E.SEG_N
            for form, d in deltas(case):
                ov, oi, ks = O.topk_segmented(d, lens, ratio)
                assert ks == [E.topk_k(m, ratio) for m in lens]
                rv, ri = [], []
                for (a, b), k in zip(E.bounds(lens), ks):
                    v, i = restated_topk(d[a:b], k)
                    rv.append(v)
                    ri.append(i + a)
                assert np.array_equal(oi, np.concatenate(ri)), (tag, ratio, form)
                assert np.array_equal(bits(ov), bits(np.concatenate(rv))), (tag, ratio, form)


def test_mixed_layout_holds_whole_special_tensors():
    for computed in (False, True):
        d = E.segmented("mixed", 0.9, computed).delta()
        seg = [d[a:b] for a, b in E.bounds(E.SEG_LAYOUT)]
        assert np.isnan(seg[0]).all() and seg[0].size == 1
        assert np.all(O.keys(seg[2]) == 0) and np.signbit(seg[2]).any() and not np.signbit(seg[2]).all()
        assert np.isnan(seg[3]).all() and np.isinf(seg[4]).all()
        assert (seg[4] > 0).any() and (seg[4] < 0).any()


@pytest.mark.parametrize("n", E.FLAT_SIZES)
def test_unambiguous_sets_match_torch_topk(n):
    """top_few and huge have no tie at T, so the selected set is torch.topk's."""
    for ratio in E.RATIOS:
        k = E.topk_k(n, ratio)
        for tag in ("top_few", "huge"):
            for computed in (False, True):
                d = E.build(tag, n, k, computed).delta()
                T = E.kth_key(d, k)
                assert int((O.keys(d) == T).sum()) == 1, (tag, n, ratio)
                want = torch.topk(torch.from_numpy(np.array(d)).abs(), k).indices.numpy()
                assert np.array_equal(np.sort(want), O.topk(d, k)[1]), (tag, n, ratio, computed)


def test_read_only_forms_keep_their_bits():
    """No arithmetic touches a read-only input: the delta is the stored array, and the oracle
    returns the stored NaN payloads and signs bit for bit.  The order among NaNs is by payload
    (the key is |d| bits: this codec's rule, csrc/choco_common.h -- the reference's torch.topk
    does not distinguish NaNs): every NaN above T's payload is sent, and at T's payload the
    lowest indices."""
    n, k = 163877, E.topk_k(163877, 0.99)
    case = E.build("nan_flood", n, k, False)
    d = case.delta()
    assert d is case.x
    ov, oi = O.topk(d, k)
    assert np.array_equal(bits(ov), bits(case.x)[oi])
    key = O.keys(d).astype(np.int64)
    T = E.kth_key(d, k)
    sel = np.zeros(n, dtype=bool)
    sel[oi] = True
    assert sel[key > T].all() and not sel[key < T].any()
    tie = np.nonzero(key == T)[0]
    r = int(sel[tie].sum())
    assert 0 < r < tie.size and sel[tie[:r]].all()
    assert len(np.unique(bits(ov))) > 2        # several payloads and both signs reach the wire


def test_why_same_bits_lets_nan_match_nan():
    # inf - inf has no operand NaN to propagate, so the sign of the default NaN is the
    # implementation's: x86 SSE returns 0xFFC00000, other targets (the GPU among them) may return
    # 0x7FC00000.  conftest.same_bits therefore lets a NaN match any NaN -- the only relaxation
    # these tests use; everything else (the sign of zero, subnormals, inf's sign) is compared by bits.
    with np.errstate(invalid="ignore"):
        host_nan = np.array([np.inf], dtype=F32) - np.array([np.inf], dtype=F32)
    assert np.isnan(host_nan[0]) and int(bits(host_nan)[0]) & 0x7FFFFFFF == E.KEY_QNAN
    other = (bits(host_nan) ^ U32(0x80000000)).view(F32)
    assert same_bits(host_nan, other)
    assert same_bits(E.from_keys([E.KEY_QNAN | 5], [0]), host_nan)
    assert not same_bits(np.array([0.0], dtype=F32), np.array([-0.0], dtype=F32))
    assert not same_bits(E.from_keys([1], [0]), E.from_keys([2], [0]))
    assert not same_bits(E.from_keys([1], [0]), np.array([0.0], dtype=F32))
    assert not same_bits(np.array([np.inf], dtype=F32), np.array([-np.inf], dtype=F32))
    assert not same_bits(host_nan, np.array([np.inf], dtype=F32))
    # and the key of either NaN is the same, so the selection does not depend on that sign
    assert int(O.keys(host_nan)[0]) == int(O.keys(other)[0])

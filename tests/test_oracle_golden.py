"""Pin the numpy oracle against golden vectors produced by the REFERENCE itself
(tests/golden/gen_golden.py imports dl_code/pcode).  CPU only."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT, golden, golden_json, same_bits
from oracle import choco_oracle as O

TOPK_CASES = ["topk_n1000_r09", "topk_n65536_r099", "topk_n262144_r099", "topk_n30011_r09", "topk_n50_k1",
              "topk_k1_tie"]


def _delta(g):
    return g["x"] - g["xhat"] if "xhat" in g else g["x"]


def test_k_rule_table():
    for n, ratio, k in golden_json("k_table.json"):
        assert O.topk_k(n, ratio) == k, (n, ratio)


@pytest.mark.parametrize("name", TOPK_CASES)
def test_topk_set_matches_reference(name):
    g = golden(name)
    d = _delta(g).astype(np.float32)
    k = int(g["k"])
    assert O.topk_k(d.size, float(g["ratio"])) == k
    vals, idx = O.topk(d, k)
    ref_idx = np.sort(g["indices"])
    assert np.array_equal(idx, ref_idx)
    order = np.argsort(g["indices"])
    assert same_bits(vals, g["values"][order])


def test_topk_k1_tie_first_index():
    g = golden("topk_k1_tie")
    _, idx = O.topk(g["x"], 1)
    assert idx.tolist() == g["indices"].tolist() == [1]


def test_topk_ties_multiset():
    g = golden("topk_ties_n4096_r09")
    d = g["x"]
    k = int(g["k"])
    vals, idx = O.topk(d, k)
    assert np.array_equal(np.sort(np.abs(vals)), np.sort(np.abs(g["values"])))
    thr = np.abs(vals).min()
    assert np.all(np.abs(np.delete(d, idx)) <= thr)
    # canonical tie rule: the lowest indices among |d| == thr are taken
    eq = np.nonzero(np.abs(d) == thr)[0]
    taken = np.intersect1d(idx, eq)
    assert np.array_equal(taken, eq[:taken.size])


def test_randk_gather_matches_reference():
    g = golden("randk_n20000_r095")
    x = g["x"]
    n, k = x.size, O.topk_k(x.size, float(g["ratio"]))
    assert same_bits(O.gather(x, g["idx_biased"]), g["vals_biased"])
    assert same_bits(O.gather(x, g["idx_unbiased"], n, k, is_biased=False), g["vals_unbiased"])
    assert len(np.unique(g["idx_biased"])) == k


@pytest.mark.parametrize("name,q,biased", [("qsgd_n32771_q4", 4, False), ("qsgd_n32771_q4_biased", 4, True),
                                           ("qsgd_n4099_q2", 2, False), ("qsgd_n4099_q8", 8, False),
                                           ("qsgd_n257_q4_small", 4, False)])
def test_qsgd_dense_matches_reference_with_pinned_norm(name, q, biased):
    g = golden(name)
    s = 2 ** q - 1
    out = O.qsgd_dense(g["x"], s, g["u"], g["norm_ref"], is_biased=biased)
    assert same_bits(out, g["out"])
    # fp64-accumulated norm vs fp64 truth
    nrm = O.l2_norms(g["x"], [g["x"].size])[0]
    assert abs(float(nrm) - float(g["norm_f64"])) <= 1e-6 * float(g["norm_f64"])
    # wire round trip decodes to the same floats
    lvl = O.qsgd_levels(g["x"], s, g["u"], g["norm_ref"])
    packed = O.qsgd_pack(lvl, g["x"], q)
    levels, neg = O.qsgd_unpack(packed, g["x"].size, q)
    dec = O.qsgd_decode(levels, neg, g["norm_ref"], s, g["x"].size, is_biased=biased)
    assert same_bits(dec, g["out"])


def test_qsgd_zero_tensor_is_nan_like_reference():
    g = golden("qsgd_zeros")
    out = O.qsgd_dense(g["x"], 15, g["u"], np.float32(0.0))
    assert np.all(np.isnan(g["out"])) and np.all(np.isnan(out))
    levels, neg = O.qsgd_unpack(O.qsgd_pack(O.qsgd_levels(g["x"], 15, g["u"], 0.0), g["x"], 4), 64, 4)
    assert np.all(np.isnan(O.qsgd_decode(levels, neg, 0.0, 15, 64)))


def test_qsgd_q32_passthrough():
    g = golden("qsgd_q32_passthrough")
    assert same_bits(g["x"], g["out"])


@pytest.mark.parametrize("name", ["sign_n4096", "sign_n40003_pad", "sign_n31"])
def test_sign_pack_unpack_matches_reference_wrapper(name):
    g = golden(name)
    packed = O.sign_pack(g["x"])
    assert np.array_equal(packed, g["packed"])
    assert same_bits(O.sign_unpack(packed, g["x"].size), g["decoded"])


def _workers(g):
    return [(g["x"][r] - g["xhat"][r]).astype(np.float32) for r in range(g["x"].shape[0])]


@pytest.mark.parametrize("name,ratio", [("choco_topk_mini_r09", 0.9), ("choco_topk_mini_r099", 0.99)])
def test_choco_topk_round_trip(name, ratio):
    g = golden(name)
    lens = g["layout"].tolist()
    hat, mem = g["hat0"].copy(), g["mem0"].copy()
    self_rank = int(g["self_rank"])
    for r, d in enumerate(_workers(g)):
        vals, idx, ks = O.topk_segmented(d, lens, ratio)
        assert ks == g["selected_shapes"].tolist()
        # the reference message: [values | local indices as fp32], per segment in topk order
        msg = g[f"msg{r}"]
        K = msg.size // 2
        ref_local = msg[K:].astype(np.int64)
        offs = np.repeat(np.cumsum([0] + lens[:-1]), ks)
        ref_global = ref_local + offs
        order = np.argsort(ref_global)
        assert np.array_equal(idx, ref_global[order])
        assert same_bits(vals, msg[:K][order])
        O.sparse_accumulate(hat if r == self_rank else None, mem, vals, idx, g["weights"][r])
    assert same_bits(hat, g["hat1"])
    assert same_bits(mem, g["mem1"])
    assert float(g["n_bits"]) == 64 * sum(ks)


def test_choco_qsgd_round_trip():
    g = golden("choco_qsgd_mini_q4")
    lens = g["layout"].tolist()
    s = 15
    decoded = []
    for r, d in enumerate(_workers(g)):
        off, outs = 0, []
        for si, m in enumerate(lens):
            outs.append(O.qsgd_dense(d[off:off + m], s, g["u"][r][off:off + m], g["norms_ref"][r][si]))
            off += m
        dense = np.concatenate(outs)
        assert same_bits(dense, g[f"msg{r}"])
        decoded.append(dense)
    hat, mem = g["hat0"].copy(), g["mem0"].copy()
    O.qsgd_accumulate(hat, mem, decoded, g["weights"], int(g["self_rank"]))
    assert same_bits(hat, g["hat1"])
    assert same_bits(mem, g["mem1"])
    assert float(g["n_bits"]) == 4 * sum(lens)


def test_choco_sign_round_trip():
    g = golden("choco_sign_mini")
    lens = g["layout"].tolist()
    msgs = []
    for r, d in enumerate(_workers(g)):
        ref_norms = g[f"norms{r}"]
        ours = O.l1_norms(d, lens)
        # the reference's fp32 CPU norm carries its own rounding drift (~6e-7 rel at 2304
        # elements); the oracle is the fp64 sum rounded once
        assert np.allclose(ours, ref_norms, rtol=1e-5, atol=0)
        off = 0
        for si, m in enumerate(lens):
            exact = np.sum(np.abs(d[off:off + m].astype(np.float64)))
            assert ours[si] == np.float32(exact)
            off += m
        assert np.array_equal(O.sign_pack(d), g[f"signs{r}"])
        msgs.append((g[f"signs{r}"], ref_norms))
    hat, mem = g["hat0"].copy(), g["mem0"].copy()
    O.sign_accumulate(hat, mem, msgs, g["weights"], int(g["self_rank"]), lens)
    assert same_bits(hat, g["hat1"])
    assert same_bits(mem, g["mem1"])
    assert float(g["n_bits"]) == 32 * len(lens) + 32 * O.sign_words(sum(lens))


def test_gossip_step():
    g = golden("gossip_n10007")
    assert same_bits(O.gossip_step(g["x"], g["mem"], g["hat"], g["gamma"]), g["out"])
    g2 = golden("choco_topk_mini_r09")
    x = g2["x"][int(g2["self_rank"])]
    assert same_bits(O.gossip_step(x, g2["mem1"], g2["hat1"], g2["gamma"]), g2["x_after_gossip"])


@pytest.mark.parametrize("name", ["choco_step_topk_r099", "choco_step_sign"])
def test_choco_step_fixture(name):
    """ParallelCHOCO_V.step (consensus step, then compress, ring of 3, receiver 1) as the
    reference ran it: the oracle's gossip step is bit-exact for every worker, and the
    oracle's codec on d = x_after - x_hat reproduces the receiver's x_hat / memory."""
    g = golden(name)
    lens = g["layout"].tolist()
    s = int(g["self_rank"])
    ds = []
    for r in range(3):
        xa = O.gossip_step(g["x"][r], g["mem"][r], g["xhat"][r], g["gamma"])
        assert same_bits(xa, g["x_after_gossip"][r])
        ds.append((xa - g["xhat"][r]).astype(np.float32))
    hat, mem = g["xhat"][s].copy(), g["mem"][s].copy()
    if "topk" in name:
        for r in range(3):
            ov, oi, _ = O.topk_segmented(ds[r], lens, 0.99)
            O.sparse_accumulate(hat if r == s else None, mem, ov, oi, g["weights"][r])
        assert same_bits(hat, g["hat1"])
        assert same_bits(mem, g["mem1"])
    else:
        msgs = [(O.sign_pack(d), O.l1_norms(d, lens)) for d in ds]
        O.sign_accumulate(hat, mem, msgs, g["weights"], s, lens)
        assert np.allclose(hat, g["hat1"], rtol=1e-5, atol=1e-6)
        assert np.allclose(mem, g["mem1"], rtol=1e-5, atol=1e-6)


def test_dcd_topk_fixture():
    """DCD (dcd_psgd.py:175-275): every replica hat_r[idx_r] += v_r, v_r = top-k of
    half_r - x_r per tensor."""
    g = golden("dcd_topk_mini_r09")
    lens = g["layout"].tolist()
    for r in range(3):
        d = (g["half"][r] - g["x"][r]).astype(np.float32)
        ov, oi, _ = O.topk_segmented(d, lens, 0.9)
        hat = g["hats0"][r].copy()
        hat[oi] = hat[oi] + ov
        assert same_bits(hat, g["hats1"][r])


def test_dcd_qsgd_fixture():
    import torch
    g = golden("dcd_qsgd_mini_q4")
    lens = g["layout"].tolist()
    for r in range(3):
        d = (g["half"][r] - g["x"][r]).astype(np.float32)
        # the message is the reference's dense floats: the oracle rebuilds it from the captured
        # uniforms and the reference's own fp32 norm (torch CPU, as dcd_psgd.py:310 computes it)
        dense = g[f"msg{r}"]
        assert same_bits((g["hats0"][r] + dense).astype(np.float32), g["hats1"][r])
        off, outs = 0, []
        for m in lens:
            nrm = np.float32(torch.from_numpy(d[off:off + m].copy()).norm(p=2).item())
            outs.append(O.qsgd_dense(d[off:off + m], 15, g["u"][r][off:off + m], nrm))
            off += m
        assert same_bits(np.concatenate(outs), dense)


def test_dcd_sign_fixture():
    g = golden("dcd_sign_mini")
    lens = g["layout"].tolist()
    for r in range(3):
        d = (g["half"][r] - g["x"][r]).astype(np.float32)
        hat = g["hats0"][r].copy()
        O.sign_axpy(hat, O.sign_pack(d), O.l1_norms(d, lens), lens, 1.0, two_roundings=False)
        assert np.allclose(hat, g["hats1"][r], rtol=1e-5, atol=1e-6)


def test_deepsqueeze_topk_fixture():
    """DeepSqueeze (deep_squeeze.py:187-279): local copy = message scattered into zeros;
    aggregate = sum_r c_r * v_r at idx_r, c_r = gamma (w_r - [r == self]), two roundings."""
    g = golden("deepsqueeze_topk_mini_r09")
    lens = g["layout"].tolist()
    s = int(g["self_rank"])
    agg = np.zeros_like(g["agg"])
    for r in range(3):
        ov, oi, _ = O.topk_segmented(g["mem"][r], lens, 0.9)
        local = np.zeros_like(g["mem"][r])
        local[oi] = ov
        assert same_bits(local, g["local"][r])
        c = O.deepsqueeze_weight(float(g["gamma"]), float(g["weights"][r]), r == s)
        agg[oi] = agg[oi] + (c * ov).astype(np.float32)
    assert same_bits(agg, g["agg"])


def test_deepsqueeze_qsgd_fixture():
    g = golden("deepsqueeze_qsgd_mini_q4")
    s = int(g["self_rank"])
    agg = np.zeros_like(g["agg"])
    for r in range(3):
        assert same_bits(g["local"][r], g[f"msg{r}"])  # the local copy IS the dense message
        c = O.deepsqueeze_weight(float(g["gamma"]), float(g["weights"][r]), r == s)
        agg = (agg + (c * g[f"msg{r}"]).astype(np.float32)).astype(np.float32)
    assert same_bits(agg, g["agg"])


def test_deepsqueeze_sign_fixture():
    """With the reference's own fp32 norms (its message) the local copy and the aggregate
    are bit-exact; the oracle's fp64 norms agree with them to 1e-5."""
    g = golden("deepsqueeze_sign_mini")
    lens = g["layout"].tolist()
    s = int(g["self_rank"])
    agg = np.zeros_like(g["agg"])
    for r in range(3):
        x = g["mem"][r]
        norms = g[f"norms{r}"]
        assert np.allclose(O.l1_norms(x, lens), norms, rtol=1e-5, atol=0)
        assert same_bits(O.sign_local(x, norms, lens), g["local"][r])
        c = O.deepsqueeze_weight(float(g["gamma"]), float(g["weights"][r]), r == s)
        O.sign_axpy(agg, O.sign_pack(x), norms, lens, c, two_roundings=True)
    assert same_bits(agg, g["agg"])


def test_ecd_topk_fixture():
    """ECD (ecd_psgd.py:211-303): replica r extrapolated with the top-k of z_r."""
    g = golden("ecd_topk_mini_r09")
    lens = g["layout"].tolist()
    t = int(g["local_index"])
    for r in range(3):
        ov, oi, _ = O.topk_segmented(g["z"][r], lens, 0.9)
        hat = g["hats0"][r].copy()
        hat[oi] = O.ecd_extrapolate(hat[oi], ov, t)
        assert same_bits(hat, g["hats1"][r])


def test_ecd_qsgd_fixture():
    g = golden("ecd_qsgd_mini_q4")
    t = int(g["local_index"])
    for r in range(3):
        assert same_bits(O.ecd_extrapolate(g["hats0"][r], g[f"msg{r}"], t), g["hats1"][r])


def test_ecd_sign_fixture():
    g = golden("ecd_sign_mini")
    lens = g["layout"].tolist()
    t = int(g["local_index"])
    for r in range(3):
        norms = g[f"norms{r}"]
        assert np.allclose(O.l1_norms(g["z"][r], lens), norms, rtol=1e-5, atol=0)
        got = O.ecd_sign_extrapolate(g["hats0"][r], O.sign_pack(g["z"][r]), norms, lens, t)
        assert same_bits(got, g["hats1"][r])


def test_ef_sign_fixture():
    """EFSignCompressor (ef_sign_sgd.py:140-219): the local copy norm * sign(g) / numel
    (sign(0) = 0) plus every other rank's decoded signs, divided by the world size."""
    g = golden("efsign_mini")
    lens = g["layout"].tolist()
    me = int(g["rank"])
    local = O.sign_local(g["grads"][me], g["norms"][me], lens)
    assert same_bits(local, g["local"])
    out = local.copy()
    for r in range(3):
        if r != me:
            O.sign_axpy(out, O.sign_pack(g["grads"][r]), g["norms"][r], lens, 1.0, two_roundings=False)
    assert same_bits((out / np.float32(3.0)).astype(np.float32), g["out"])


def test_dgc_fixture():
    """DGC._compress / _recover_info (dgc.py:153-252): error-feedback top-k and the averaged
    sparse update of all ranks' messages, bit-exact.

    The memory update is NOT reproduced: the reference's get_mask returns
    (~mask.byte()).float() (sparsification.py:33-38), a BITWISE not of uint8 under the
    PyTorch it pins (>= 1.2), i.e. 255 / 254 instead of 1 / 0, so its memory becomes
    255 * _grad (254 * at the selected entries).  The drop-in keeps the intended
    `_grad * nmask` (selected entries zeroed); this test pins what the
    fixture holds so the deviation is explicit."""
    g = golden("dgc_topk_mini_r09")
    lens = g["layout"].tolist()
    grads = np.zeros_like(g["params"])
    for r in range(3):
        x = (g["grads"][r] + g["mems"][r]).astype(np.float32)
        ov, oi, _ = O.topk_segmented(x, lens, float(g["ratio"]))
        factor = np.full(x.size, np.float32(255.0), dtype=np.float32)
        factor[oi] = np.float32(254.0)
        assert same_bits((x * factor).astype(np.float32), g["mems_after"][r])
        grads[oi] = grads[oi] + ov
    upd = (grads / np.float32(3)).astype(np.float32)
    want = O.fma32(np.float32(-float(g["lr"])), upd, g["params"])
    assert same_bits(want, g["params_after"])


def test_splitmix64_known_answer():
    # the first outputs of the splitmix64 generator from state 0 (Vigna's reference
    # implementation: state += gamma; return mix(state))
    z = O.splitmix64_mix(np.array([O.GAMMA, 2 * O.GAMMA % 2 ** 64], dtype=np.uint64))
    assert z.tolist() == [16294208416658607535, 7960286522194355700]
    u = O.qsgd_uniforms(6, 7, 3)
    assert u.dtype == np.float32 and np.all((u >= 0) & (u < 1))


def _xoro_scalar_stream(key, sid, count):
    """xoroshiro128+ written out sequentially in Python ints (Blackman & Vigna 2018,
    a=24 b=16 c=37), seeded by two SplitMix64 outputs: an independent restatement of the
    vectorised oracle form."""
    M = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    def rotl(x, k):
        return ((x << k) | (x >> (64 - k))) & M
    z = (key + (2 * sid + 1) * O.GAMMA) & M
    s0, s1 = mix(z), mix((z + O.GAMMA) & M)
    out = []
    for _ in range(count):
        out.append((s0 + s1) & M)
        t = s1 ^ s0
        s0 = rotl(s0, 24) ^ t ^ ((t << 16) & M)
        s1 = rotl(t, 37)
    return out


def test_qsgd_uniform_stream_mapping():
    """The device stream layout (qsgd.hip qstream_id): with g = (e & 8191) >> 11, element e
    is position (g & 1) * 8 + (e & 7) of stream ((e >> 13) << 9) | ((g >> 1) << 8) |
    ((e & 8191) >> 3 & 255): 16 uniforms per stream, two streams per thread slot."""
    seed, offset = 0xABCDEF, 2
    key = O.qrng_key(seed, offset)
    for tile, t in ((0, 0), (0, 255), (3, 17)):
        for h in range(2):
            r = _xoro_scalar_stream(key, (tile << 9) | (h << 8) | t, 8)
            idx = np.array([tile * 8192 + g * 2048 + 8 * t + c for g in (2 * h, 2 * h + 1) for c in range(8)])
            want = []
            for p in range(16):
                v = r[p // 2]
                want.append(((v >> 40) if p % 2 == 0 else (v >> 16) & 0xFFFFFF) * 2.0 ** -24)
            assert np.array_equal(O.qsgd_uniforms_at(idx, seed, offset), np.array(want, dtype=np.float32))
    # distribution: 2^20 uniforms, 64 bins within 5 sigma, mean 1/2
    u = O.qsgd_uniforms(1 << 20, 11, 0)
    h = np.bincount((u * 64).astype(np.int64), minlength=64)
    assert abs(u.mean() - 0.5) < 2e-3 and np.all(np.abs(h - 16384) < 5 * 128)


def test_randk_indices_distinct_and_streams():
    n, k = 10000, 1000
    for seed in range(40):
        idx = O.randk_indices(n, k, seed)
        assert idx.size == k and np.unique(idx).size == k and np.all(np.diff(idx) > 0)
        assert idx[0] >= 0 and idx[-1] < n
    # (seed, offset) streams are distinct
    assert not np.array_equal(O.randk_indices(n, k, 7, 0), O.randk_indices(n, k, 7, 1))


# Uniformity of the device sampler (randk.hip, restated in the oracle) against the law of
# the reference's np.random.choice(n, k, replace=False) (sparsification.py:48): a uniform
# k-subset.  Chi-square tests over fixed seeds (deterministic), rejected at p < 1e-4.
_RK_P_MIN = 1e-4


def _chi2_p(obs, exp, fpc=1.0):
    from scipy import stats
    obs, exp = np.asarray(obs, np.float64), np.asarray(exp, np.float64)
    x = float(((obs - exp) ** 2 / exp).sum()) / fpc
    return stats.chi2.sf(x, obs.size - 1)


@pytest.mark.parametrize("N", [1 << 18, 1_000_000])
def test_randk_position_residues_uniform(N):
    """In-tile positions modulo 2^s, s = 1..8 (tiles are 2^18-aligned, so idx mod 2^s is the
    in-tile position's residue): each residue class holds its share of the draws.  A uniform
    k-subset's class counts are multivariate hypergeometric: chi-square with the finite
    population correction (N - k) / (N - 1)."""
    k, seeds = N // 64, 128
    draws = [O.randk_indices(N, k, seed) for seed in range(seeds)]
    for s in range(1, 9):
        M = 1 << s
        cnt = sum(np.bincount(i % M, minlength=M) for i in draws)
        exp = np.array([len(range(r, N, M)) for r in range(M)]) * (k / N) * seeds
        p = _chi2_p(cnt, exp, (N - k) / (N - 1))
        assert p > _RK_P_MIN, (N, M, p)


@pytest.mark.parametrize("N", [1 << 18, 1_000_000])
def test_randk_gaps_geometric(N):
    """Gaps between consecutive selected indices follow the geometric law of a uniform
    k-subset for k << N: P(gap = g) = (1 - k/N)^(g-1) k/N (bins g = 1..128, tail pooled)."""
    k, seeds = N // 64, 64
    g = np.concatenate([np.diff(O.randk_indices(N, k, seed)) for seed in range(seeds)])
    q = k / N
    edges = np.array(list(range(1, 129)) + [1 << 40], dtype=np.float64)
    obs = np.histogram(g, bins=edges)[0]
    probs = (1 - q) ** (edges[:-1] - 1) - (1 - q) ** (edges[1:] - 1)
    assert _chi2_p(obs, probs * g.size) > _RK_P_MIN


@pytest.mark.parametrize("N", [1 << 18, 1_000_000])
def test_randk_consecutive_draws_uncorrelated(N):
    """Consecutive draws pi(j), pi(j + 1) of the sampler's bijections -- pi_N (the tile
    counts) and the in-tile pi_L (the positions) -- are independent: correlation within
    5 standard errors, and uniform joint cells on a 16 x 16 grid of the high bits and of
    the low 4 bits (chi-square over 8 keys pooled)."""
    k = N // 64
    T = 1 << O.RK_TILE_BITS
    grids_hi, grids_lo = np.zeros(256), np.zeros(256)
    for seed in range(8):
        K = O.rk_derive(O.randk_key(seed, 0), 0)
        for L, key in ((N, K), (min(T, N), O.rk_derive(K, 8))):
            y = O.rk_perm(np.arange(k), L, key)
            a, b = y[:-1], y[1:]
            assert abs(np.corrcoef(a, b)[0, 1]) < 5.0 / np.sqrt(a.size), (N, L, seed)
            grids_hi += np.bincount((a * 16 // L) * 16 + b * 16 // L, minlength=256)
            grids_lo += np.bincount((a % 16) * 16 + b % 16, minlength=256)
    for grid in (grids_hi, grids_lo):
        assert _chi2_p(grid, np.full(256, grid.sum() / 256)) > _RK_P_MIN


@pytest.mark.parametrize("N", [1, 2, 3, 5, 17, 1000, 65537, 262144, 300001])
def test_randk_permutation_is_a_bijection(N):
    """pi_N (csrc/randk.hip RkPerm) maps [0, N) onto [0, N) for every key."""
    for K in (0, 1, 0xDEADBEEF12345678):
        y = O.rk_perm(np.arange(N), N, K)
        assert np.array_equal(np.sort(y), np.arange(N))


def test_randk_multi_tile_counts_hypergeometric():
    """Over tiles of 2^18, the per-tile counts of a multi-tile draw follow the
    multivariate hypergeometric law of a uniform k-subset (mean k L_t / N, variance
    k p (1 - p) (N - k) / (N - 1)); every index distinct, ascending, in range."""
    N, k = 1_000_003, 30_000
    T = 1 << O.RK_TILE_BITS
    nt = (N + T - 1) // T
    lens = np.array([min(T, N - t * T) for t in range(nt)], dtype=np.float64)
    cs = []
    for seed in range(60):
        idx = O.randk_indices(N, k, seed)
        assert idx.size == k and np.unique(idx).size == k and idx[0] >= 0 and idx[-1] < N
        cs.append(np.bincount(idx // T, minlength=nt))
    cs = np.array(cs, dtype=np.float64)
    p = lens / N
    mean, var = k * p, k * p * (1 - p) * (N - k) / (N - 1)
    assert np.all(np.abs(cs.mean(0) - mean) < 5 * np.sqrt(var / len(cs)))
    assert np.all(np.abs(cs.var(0) / var - 1) < 0.6)


def test_randk_all_and_tiny():
    assert np.array_equal(O.randk_indices(5, 5, 3), np.arange(5))
    assert np.array_equal(O.randk_indices(600_000, 600_000, 3), np.arange(600_000))
    i = O.randk_indices(1, 1, 9)
    assert i.tolist() == [0]
    i = O.randk_indices(700_001, 1, 9)
    assert i.size == 1 and 0 <= i[0] < 700_001


def test_oracle_sampled_helpers_agree_with_full_forms():
    """qsgd_uniforms_at / qsgd_wire_at (the sampled checks at BASELINE sizes) restate the
    full-array forms exactly."""
    n, seed, offset = 10_007, 0x1234_5678_9ABC, 5
    u = O.qsgd_uniforms(n, seed, offset)
    idx = np.array([0, 1, 2, 3, 4, 777, 4096, n - 2, n - 1])
    assert np.array_equal(O.qsgd_uniforms_at(idx, seed, offset), u[idx])
    rng = np.random.default_rng(0)
    d = rng.standard_normal(n).astype(np.float32)
    for q in (1, 2, 4, 8, 16):
        s = 2 ** q - 1
        lvl = O.qsgd_levels(d, s, u, np.float32(np.sqrt(np.sum(d.astype(np.float64) ** 2))) / 40)
        packed = O.qsgd_pack(lvl, d, q)
        levels, neg = O.qsgd_unpack(packed, n, q)
        gl, gn = O.qsgd_wire_at(packed, n, q, idx)
        assert np.array_equal(gl, levels[idx].astype(np.int64)) and np.array_equal(gn, neg[idx])


@pytest.mark.parametrize("q", [1, 2, 3, 4, 5, 8, 9, 16])
@pytest.mark.parametrize("n", [5, 8, 2049, 18_445])
def test_oracle_qsgd_wire_round_trips_at_every_width(q, n):
    """qsgd_pack -> qsgd_unpack gives back the levels and signs, and qsgd_wire_at reads the
    same, at every q the receiver tests use -- the widths that do not fill their container
    (3, 5, 9) included -- with levels 0 and 2^q - 1 present and a partial last group."""
    s = 2 ** q - 1
    rng = np.random.default_rng(1000 * q + n)
    lvl = rng.integers(0, s + 1, size=n)
    lvl[[0, n - 2]] = 0
    lvl[[1, n - 1]] = s
    d = rng.standard_normal(n).astype(np.float32)
    packed = O.qsgd_pack(lvl.astype(np.float32), d, q)
    cw = O.container_bits(q)
    assert cw in (1, 2, 4, 8, 16) and q <= cw < 2 * q
    assert packed.size == O.plane_bytes(n, cw) + O.plane_bytes(n, 1)
    levels, neg = O.qsgd_unpack(packed, n, q)
    assert np.array_equal(levels.astype(np.int64), lvl) and np.array_equal(neg, d < 0)
    idx = np.unique(np.array([0, 1, 2, 3, 4, n // 2, n - 2, n - 1]))
    gl, gn = O.qsgd_wire_at(packed, n, q, idx)
    assert np.array_equal(gl, lvl[idx]) and np.array_equal(gn, neg[idx])


def test_oracle_torch_sign_is_torch_sign():
    """The oracle's torch_sign against the installed torch.sign on the values where sign
    conventions differ: NaN and both zeros give +0 (so the reference's (norm * sign(x)) / numel
    is 0 at a NaN), infinities and subnormals give +-1."""
    import torch
    x = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-41, -1e-41, 1.0, -1.0], dtype=np.float32)
    want = np.array([0, 0, 0, 1, -1, 1, -1, 1, -1], dtype=np.float32)
    got = torch.sign(torch.from_numpy(x)).numpy()
    assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert O.torch_sign(x).view(np.uint32).tolist() == got.view(np.uint32).tolist()
    # torch's vectorised path (whole SIMD lanes) and its scalar tail give the same
    big = np.tile(x, 37)
    assert O.torch_sign(big).view(np.uint32).tolist() == torch.sign(torch.from_numpy(big)).numpy().view(np.uint32).tolist()


def test_oracle_segmented_randk():
    lens = [3, 70, 5, 1000, 17]
    d = np.random.default_rng(1).standard_normal(sum(lens)).astype(np.float32)
    v, i = O.randk_segmented(d, lens, 0.9, 42)
    ks = [O.topk_k(m, 0.9) for m in lens]
    assert v.size == i.size == sum(ks)
    off = 0
    for s, (m, k) in enumerate(zip(lens, ks)):
        part = i[sum(ks[:s]):sum(ks[:s + 1])]
        assert np.all(np.diff(part) > 0) and part[0] >= off and part[-1] < off + m
        assert np.array_equal(part - off, O.randk_segment_indices(m, k, O.rk_derive(O.randk_key(42), s)))
        off += m
    assert same_bits(v, d[i])
    # the flat draw is segment 0 of the same key
    assert np.array_equal(O.randk_indices(1000, 100, 42), O.randk_segment_indices(1000, 100, O.rk_derive(O.randk_key(42), 0)))


# ---------------------------------------------------------------------------- ring > 3
def test_ring_neighborhoods_match_reference_graphs():
    """communication.neighborhood against the reference's own RingGraph (world > 2) /
    CompleteGraph (world 2) rows, generated from topology.py:122-299: same ranks, same
    ascending order, same float64 weights -- including worlds 4..8, where a rank's
    neighbourhood is a strict subset of the world."""
    from chocosgd_amd.communication import neighborhood
    tab = golden_json("ring_neighborhoods.json")
    for w, rows in tab.items():
        for rank, row in enumerate(rows):
            got = neighborhood(rank, int(w))
            assert list(got.items()) == [(int(r), float(x)) for r, x in row], (w, rank)


def _ring_replay(kind, g):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _ring as R
    lens = g["layout"].tolist()
    W = R.RING_WORLD
    nbs = golden_json("ring_neighborhoods.json")[str(W)]
    ins = [R.ring_inputs(r) for r in range(W)]
    msgs = []
    for r in range(W):
        d = (ins[r][0] - ins[r][1]).astype(np.float32)
        if kind == "topk":
            vals, idx, _ = O.topk_segmented(d, lens, R.RING_RATIO)
            msgs.append((vals, idx))
        else:
            assert np.allclose(O.l1_norms(d, lens), g["norms"][r], rtol=1e-5, atol=0)
            msgs.append((O.sign_pack(d), g["norms"][r]))  # the reference's fp32 norms pinned
    for r in range(W):
        hat, mem = ins[r][2].copy(), ins[r][3].copy()
        ranks = [int(q) for q, _ in nbs[r]]
        weights = [float(x) for _, x in nbs[r]]
        if kind == "topk":
            for q, wq in zip(ranks, weights):
                O.sparse_accumulate(hat if q == r else None, mem, msgs[q][0], msgs[q][1], wq)
        else:
            O.sign_accumulate(hat, mem, [msgs[q] for q in ranks], weights, ranks.index(r), lens)
        assert same_bits(hat, g["hat1"][r]), (kind, r)
        assert same_bits(mem, g["mem1"][r]), (kind, r)


@pytest.mark.parametrize("kind,name", [("topk", "choco_ring8_topk_r09"), ("sign", "choco_ring8_sign")])
def test_choco_ring8_round(kind, name):
    """A ring of 8 through the reference (every worker's x_hat / memory after uncompress of
    its own neighbourhood's messages, parallel_choco_v.py:291-310 / :549-558): the oracle,
    replaying each rank's neighbourhood from the reference's RingGraph, is bit-exact."""
    _ring_replay(kind, golden(name))

"""GPU parity of the MX (block-scaled FP4 / FP8) kernels (csrc/mx.hip) with the numpy restatement of
the contract (tests/_mx_oracle.py): every byte and every float bit for bit; the stochastic mode's
properties besides."""
import functools

import numpy as np
import pytest
import torch

import _mx_oracle as R
import _streams as ST
from test_gpu_qsgd_bucket import DEV, GAMMA, N, OFFSET, SEED, Loopback, dev, host  # the sibling family's input sizes
from conftest import golden_json, same_bits
from oracle import choco_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32
W = [1 / 3, 1 / 7] * 4


@functools.lru_cache(maxsize=None)
def delta(n, seed=0):
    """N(0, 1) times a per-block factor spread over 1e-3 .. 1e3, so that the scales matter."""
    rng = np.random.default_rng(1000 * seed + n)
    nb = -(-n // 32)
    f = rng.permutation(10.0 ** np.linspace(-3, 3, nb))
    return (rng.standard_normal(n) * np.repeat(f, 32)[:n]).astype(F32)


@pytest.mark.parametrize("n", [N, 1, 7, 31, 33, 8192, 8193])
@pytest.mark.parametrize("with_xhat", [False, True])
@pytest.mark.parametrize("q", [4, 8])
def test_nearest_bit_for_bit(q, with_xhat, n):
    from chocosgd_amd import codec
    d = delta(n)
    xh = delta(n, seed=1) if with_xhat else None
    x = (d + xh).astype(F32) if with_xhat else d
    d = (x - xh).astype(F32) if with_xhat else d
    msg, dense = codec.mx_compress(dev(x), q, is_biased=True, xhat=dev(xh) if with_xhat else None, want_dense=True)
    sb, codes, v, want = R.quantize(d, q)
    gsb, gcodes = R.split(host(msg), n, q)
    assert np.array_equal(gsb, sb) and np.array_equal(gcodes, codes)
    assert msg.numel() == R.packed_bytes(n, q) and np.array_equal(host(msg), want)  # the padding too
    assert same_bits(host(dense), v) and same_bits(host(codec.mx_decode(msg, n, q)), v)


@pytest.mark.parametrize("q", [4, 8])
def test_stochastic(q):
    """Scales, padding, bracketing codes, determinism, the message of the restated stream, and
    unbiasedness over T seeds per block, even and odd elements apart, in units of the block scale:
    |sum(mean_T(decode) - d)| <= 6 sqrt(sum gap^2 / 4T) (a Bernoulli draw's variance is <= gap^2 / 4)."""
    from chocosgd_amd import codec
    T, d, G = 64, delta(N), R.GRID[q]
    x = dev(d)
    msg = host(codec.mx_compress(x, q, seed=SEED, offset=OFFSET)[0])
    sb, _, _, want = R.quantize(d, q, sr=True, seed=SEED, offset=OFFSET)
    a, lo, hi = R.brackets(d, sb, q)
    gsb, codes = R.split(msg, N, q)
    hb = R.align16(sb.size)
    assert np.array_equal(msg[:hb], want[:hb]) and not msg[hb + (N * q + 7) // 8:].any()  # scales, both paddings
    mag = (codes & (R.SIGN[q] - 1)).astype(np.int64)
    assert np.all((mag == lo) | (mag == hi)) and np.all(mag[G[lo] == a] == lo[G[lo] == a])
    assert np.array_equal((codes & R.SIGN[q]) != 0, np.signbit(d))
    assert np.array_equal(msg, host(codec.mx_compress(x, q, seed=SEED, offset=OFFSET)[0]))
    assert not np.array_equal(msg, host(codec.mx_compress(x, q, seed=SEED + 1, offset=OFFSET)[0]))
    assert np.array_equal(msg, want)  # the hardware's rule as include/choco_codec.h states it
    scale = np.repeat(2.0 ** (sb.astype(np.float64) - 127), 32)[:N]
    mean = sum(host(codec.mx_compress(x, q, seed=s, want_dense=True)[1]).astype(np.float64) for s in range(T)) / T
    err, gap2 = (mean - d) / scale, (G[hi] - G[lo]) ** 2
    worst = 0.0
    for half in (0, 1):
        sel = np.arange(N) % 2 == half
        e = np.add.reduceat(np.where(sel, err, 0), np.arange(0, N, 32))
        bound = 6 * np.sqrt(np.add.reduceat(np.where(sel, gap2, 0), np.arange(0, N, 32)) / (4 * T))
        worst = max(worst, float(np.max(np.abs(e) / np.maximum(bound / 6, 1e-300))))
        print(f"q={q} half={half}: worst block |sum err| / sigma = {worst:.2f}")
        assert np.all(np.abs(e) <= bound)


@pytest.mark.parametrize("sr", [False, True])
@pytest.mark.parametrize("q", [4, 8])
def test_special_blocks(q, sr):
    """One buffer: an all-zero block, a block with an inf, one with a NaN, a block whose maximum sits
    exactly on vmax 2^e, a block whose maximum's mantissa is just above the threshold."""
    from chocosgd_amd import codec
    vmax, n = float(R.GRID[q][-1]), 7 * 32 + 5
    d = (delta(n) * F32(0.01) / np.abs(delta(n)).max()).astype(F32)  # |d| <= 0.01: the planted maxima rule
    d[0:32] = 0.0
    d[32 + 17] = np.inf
    d[64 + 5] = np.nan
    d[96 + 3] = -vmax * 2.0 ** -3
    d[128 + 9] = np.nextafter(F32(vmax), F32(np.inf)) * F32(2.0 ** 4)
    msg, dense = codec.mx_compress(dev(d), q, is_biased=not sr, seed=SEED, want_dense=True)
    sb, codes = R.split(host(msg), n, q)
    v = host(dense)
    assert np.array_equal(sb, R.scale_bytes(d, q)) and same_bits(v, host(codec.mx_decode(msg, n, q)))
    assert sb[0] == 0 and sb[1] == 0xFF and sb[2] == 0xFF and sb[3] == 127 - 3 and sb[4] == 127 + 4 + 1
    assert not codes[:96].any() and not v[:32].any()
    assert np.isnan(v[32:96]).all() and not np.isnan(v[96:]).any()
    # nothing saturates: |d| / 2^e reaches vmax at the planted maximum alone, and the top code is only ever
    # the upper neighbour of a quotient above the grid value below it
    (a, _, hi), mag, top = R.brackets(d, sb, q), codes & (R.SIGN[q] - 1), len(R.GRID[q]) - 1
    assert np.flatnonzero(a >= vmax).tolist() == [96 + 3] and mag[96 + 3] == top and v[96 + 3] == d[96 + 3]
    assert np.all(hi[mag == top] == top) and vmax / 2 < a[128 + 9] < vmax / 2 * (1 + 2.0 ** -22)
    if not sr:
        assert np.array_equal(host(msg), R.quantize(d, q)[3])


@functools.lru_cache(maxsize=None)
def messages(q, nmsg=8):
    """nmsg messages of the restatement (bytes) and their decodes."""
    out = [R.quantize(delta(N, seed=10 + i), q) for i in range(nmsg)]
    return [o[3] for o in out], [o[2] for o in out]


def state():
    return delta(N, seed=3), delta(N, seed=4), delta(N, seed=5)  # x, x_hat, memory


@pytest.mark.parametrize("slot", [lambda k: 0, lambda k: k // 2, lambda k: -1], ids=["first", "middle", "absent"])
@pytest.mark.parametrize("nmsg", [1, 3, 8])
@pytest.mark.parametrize("q", [4, 8])
def test_receive(q, nmsg, slot):
    from chocosgd_amd import codec
    slot = slot(nmsg)
    msgs, vs = messages(q)
    _, hat0, mem0 = state()
    hat, mem = dev(hat0), dev(mem0)
    codec.mx_accumulate([dev(m) for m in msgs[:nmsg]], W[:nmsg], slot, N, q, mem, xhat_self=hat if slot >= 0 else None)
    h, m_ = hat0.copy(), mem0.copy()
    O.qsgd_accumulate(h, m_, vs[:nmsg], W[:nmsg], slot)  # hat += v (self); mem += (float)w * v, two roundings
    assert same_bits(host(hat), h) and same_bits(host(mem), m_)


@pytest.mark.parametrize("sr", [False, True])
@pytest.mark.parametrize("nmsg", [1, 3, 8])
@pytest.mark.parametrize("q", [4, 8])
def test_fused_step_is_the_three_calls(q, nmsg, sr):
    """Kernel 3 against accumulate, gossip_step, compress on copies of the same buffers; the
    gossip-fused compress against gossip_step, compress."""
    from chocosgd_amd import codec
    slot = nmsg // 2
    msgs = [dev(m) for m in messages(q)[0][:nmsg]]
    kw = dict(is_biased=not sr, seed=SEED, offset=OFFSET)
    a, b, c = ([dev(t) for t in state()] for _ in range(3))
    out = codec.mx_recv_gossip_compress(msgs, W[:nmsg], slot, a[0], a[2], a[1], GAMMA, q, **kw)
    codec.mx_accumulate(msgs, W[:nmsg], slot, N, q, b[2], xhat_self=b[1])
    c[1].copy_(b[1])
    c[2].copy_(b[2])
    codec.gossip_step(b[0], b[2], b[1], GAMMA)
    want, _ = codec.mx_compress(b[0], q, xhat=b[1], **kw)
    for got, ref in zip(a, b):
        assert same_bits(host(got), host(ref))
    assert torch.equal(out, want)
    fused, _ = codec.mx_compress(c[0], q, xhat=c[1], gossip=(c[2], GAMMA), **kw)
    assert torch.equal(fused, want) and same_bits(host(c[0]), host(b[0]))


@pytest.mark.parametrize("q", [4, 8])
def test_drop_in_deferred_receive(q):
    """Three utils.fused_step steps on the resnet20 layout with comm_op quantize_mx, deferred (one codec
    launch per step) and not: the same x, x_hat and memory after flush_receive; in nearest mode step
    one's message is the restatement's."""
    from chocosgd_amd import utils
    from chocosgd_amd.parallel_choco import CHOCOCompressor
    from chocosgd_amd.tensor_buffer import TensorBuffer
    lens = golden_json("layouts.json")["resnet20_cifar10"]
    n = sum(lens)
    shapes = [(torch.Size([m]), m) for m in lens]
    x0, hat0, mem0 = delta(n, seed=3), delta(n, seed=4), delta(n, seed=5)

    def run(defer):
        params = list(dev(x0).split(lens))
        groups = [{"params": [p], "name": f"p{i}"} for i, p in enumerate(params)]
        names = list(enumerate(g["name"] for g in groups))
        hat, mem = dev(hat0), dev(mem0)
        nhp = {0: TensorBuffer.from_flat(hat, [(m,) for m in lens]),
               "memory": TensorBuffer.from_flat(mem, [(m,) for m in lens])}
        agg = Loopback()
        comp = CHOCOCompressor(aggregator=agg, comm_op="quantize_mx", comm_device="gpu", compress_ratio=0.9,
                               quantize_level=q, is_biased=True, backend="nccl", use_ipc=False)
        for _ in range(3):
            sb = utils.fused_step(comp, groups, names, shapes, nhp, {0: 0.5, 1: 0.5}, GAMMA, 0, defer_receive=defer)
            assert sb["n_bits"] == q * n and sb["n_bits_wire"] == 8 * agg.first.numel() == 8 * R.packed_bytes(n, q)
        comp.flush_receive()
        return host(torch.cat([p.detach() for p in params])), host(hat), host(mem), host(agg.first)

    plain, deferred = run(False), run(True)
    for a, b in zip(plain, deferred):
        assert same_bits(a, b) if a.dtype == F32 else np.array_equal(a, b)
    x1 = O.gossip_step(x0, mem0, hat0, GAMMA)
    assert np.array_equal(plain[3], R.quantize((x1 - hat0).astype(F32), q)[3])


def test_fused_step_on_a_delayed_side_stream():
    """choco_mx_recv_gossip_compress between the harness's two delays (tests/_streams.py): a launch off
    the caller's stream reads the poison or is held back past the clones."""
    from chocosgd_amd import codec
    q, w = 4, W[:2]
    msgs = messages(q)[0]
    true = dict(zip("xhm", state()), m0=msgs[0], m1=msgs[1])
    poison = dict(x=true["m"], h=true["x"], m=true["h"], m0=msgs[2], m1=msgs[3])
    work = {k: dev(v) for k, v in true.items()}
    out = codec.mx_wire(N, q, DEV)
    _, Wk, (got,) = ST.run(lambda: codec.mx_recv_gossip_compress(
        [work["m0"], work["m1"]], w, 0, work["x"], work["m"], work["h"], GAMMA, q, seed=SEED, out=out),
        work, {k: dev(v) for k, v in true.items()}, {k: dev(v) for k, v in poison.items()}, outs=[out],
        family="mx", case="recv_gossip_compress")
    x, h, m = (dev(t) for t in state())
    want = codec.mx_recv_gossip_compress([dev(msgs[0]), dev(msgs[1])], w, 0, x, m, h, GAMMA, q, seed=SEED)
    assert torch.equal(got, want)
    for k, t in (("x", x), ("h", h), ("m", m)):
        assert same_bits(host(Wk[k]), host(t))

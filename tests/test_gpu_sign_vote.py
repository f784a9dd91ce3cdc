"""Majority-vote signSGD on the device, bit for bit: codec.sign_vote against np.unpackbits counts,
codec.params_sign_step against torch's p.add_(v, alpha=-lr) on CPU tensors of the same dtype (v
decoded by the oracle's sign_unpack), sign_sgd.fused_step against sign_sgd.step_loop on CPU copies,
and both entry points on a delayed side stream.  Every comparison is bit-exact."""
import collections

import numpy as np
import pytest
import torch

import _streams as ST
from conftest import golden_json, same_bits
from oracle import choco_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.0  # exact in every dtype
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# a zero-length tensor, one-element tensors, a tensor over more than one column block; n is no
# multiple of 32 and N' no multiple of 4
LIST4 = [5, 0, 1, 32768 + 160 + 7, 1, 3000]
SPECIALS = [0.0, -0.0, 1e-40, 1e8, -3e7, np.inf, -np.inf, np.nan]  # 1e8, -3e7: an ulp above every lr


def words_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(DEV)


def vote_ref(words):
    """words: (W, nwords) uint32 -> the verdict words, from per-bit counts."""
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=1, bitorder="little")
    verdict = 2 * bits.sum(axis=0, dtype=np.int64) > words.shape[0]
    return np.packbits(verdict, bitorder="little").view(np.uint32)


def random_words(seed, *shape):
    return np.random.RandomState(seed).randint(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)


SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4 * 256 * 3 + 2]
VOTERS = [1, 2, 3, 4, 7, 8, 9, 33, 64]
SHAPES = sorted({(w, m) for w in VOTERS for m in (5, SIZES[-1])} | {(w, m) for w in (3, 8) for m in SIZES})


@pytest.mark.parametrize("W,nwords", SHAPES)
def test_vote_shapes(W, nwords):
    from chocosgd_amd import codec
    words = random_words(1000 * W + nwords, W, nwords)
    c0 = codec.launch_count("sign_vote_kernel")
    got = codec.sign_vote([words_dev(w) for w in words])
    assert codec.launch_count("sign_vote_kernel") - c0 == 1
    assert torch.equal(got.cpu(), torch.from_numpy(vote_ref(words).view(np.int32)))


@pytest.mark.parametrize("W", [2, 8, 9, 64])
def test_vote_thresholds(W):
    """Bit b of word j is set in exactly count[j][b] voters, a window of voters that starts
    somewhere else for every bit; the counts walk over 0, W/2 - 1, W/2, W/2 + 1 and W."""
    from chocosgd_amd import codec
    levels = [0, max(W // 2 - 1, 0), W // 2, W // 2 + 1, W]
    words = np.zeros((W, 5), dtype=np.uint32)
    want = np.zeros(5, dtype=np.uint32)
    for j in range(5):
        for b in range(32):
            count = levels[(b + j) % 5]
            for k in range(count):
                words[(3 * b + j + k) % W, j] |= np.uint32(1 << b)
            want[j] |= np.uint32((2 * count > W) << b)  # a tie (2 count == W) gives 0
    got = codec.sign_vote([words_dev(w) for w in words]).cpu().numpy().view(np.uint32)
    for j in range(5):
        for b in range(32):
            assert (got[j] >> b) & 1 == (want[j] >> b) & 1, (j, b, levels[(b + j) % 5])


@pytest.mark.parametrize("offset", [0, 1], ids=["16-byte path", "per-word path"])
def test_vote_paths_aliasing_and_the_drop_in(offset):
    """Views one word into their allocations take the per-word path; out is one of the inputs;
    SignCompressor.majority_vote and MajorityVoteCompressor.vote give the same words."""
    from chocosgd_amd import codec, sign_sgd
    from chocosgd_amd.sparsification import SignCompressor
    W, nwords = 5, 1029
    words = random_words(77, W, nwords)
    want = torch.from_numpy(vote_ref(words).view(np.int32))
    msgs = [words_dev(np.concatenate([w[:offset], w]))[offset:] for w in words]
    assert all(m.data_ptr() % 16 == 4 * offset for m in msgs)
    assert torch.equal(SignCompressor().majority_vote(msgs).cpu(), want)
    comp = sign_sgd.MajorityVoteCompressor(0, W, None, "gpu")
    assert torch.equal(comp.vote({"signs": msgs[0], "synced_signs": msgs}).cpu(), want)
    got = codec.sign_vote(msgs, out=msgs[1])
    assert got is msgs[1] and torch.equal(got.cpu(), want)
    assert torch.equal(msgs[0].cpu(), torch.from_numpy(words[0].view(np.int32))), "the other inputs are read only"


class Carved:
    """Parameter tensors as views of ONE sentinel-filled storage per dtype, each view on a 16-byte
    boundary plus `shift` elements; want() is what the storages must hold after the step."""

    def __init__(self, lens, dtypes, shift, seed=3):
        rng = np.random.RandomState(seed)
        self.lens, self.dtypes = list(lens), [dtypes] * len(lens) if isinstance(dtypes, str) else list(dtypes)
        n = self.n = int(sum(lens))
        x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(np.float32)
        for k, v in enumerate(SPECIALS):
            x[(13 * k) % n] = v
        size, self.starts = collections.Counter(), []
        for m, d in zip(self.lens, self.dtypes):
            self.starts.append(size[d] + 64 + shift)
            size[d] = (self.starts[-1] + m + 7) // 8 * 8
        self.cpu = {d: torch.full((size[d] + 64,), SENTINEL, dtype=DTYPES[d]) for d in size}
        o = 0
        for m, d, a in zip(self.lens, self.dtypes, self.starts):
            self.cpu[d][a:a + m] = torch.from_numpy(x[o:o + m]).to(DTYPES[d])
            o += m
        self.stores = {d: t.to(DEV) for d, t in self.cpu.items()}
        self.views = [self.stores[d][a:a + m] for m, d, a in zip(self.lens, self.dtypes, self.starts)]
        self.lrs = [0.01 * (s % 7 + 1) for s in range(len(lens))]
        self.verdict = random_words(seed + 1, O.sign_words(n))  # the padding bits are random too

    def want(self):
        v, o, out = torch.from_numpy(O.sign_unpack(self.verdict, self.n)), 0, {d: t.clone() for d, t in self.cpu.items()}
        for m, d, a, lr in zip(self.lens, self.dtypes, self.starts, self.lrs):
            out[d][a:a + m].add_(v[o:o + m].to(DTYPES[d]), alpha=-lr)
            o += m
        return out

    def check(self, stores):
        for d, t in self.want().items():
            assert same_bits(stores[d].float().cpu().numpy(), t.float().numpy()), d


MIXED = ["fp32", "bf16", "fp16"] * 2
LAYOUTS = {**{f"one tensor of {n} {d}": ([n], d, 0) for n in (1, 31, 32, 33, 40003) for d in ("fp32", "bf16")},
           "list fp32": (LIST4, "fp32", 0),
           "list mixed, one element off": (LIST4, MIXED, 1),
           "three launches": ([1 + (7 * s) % 40 for s in range(2 * 176 + 3)], "fp32", 0)}


@pytest.mark.parametrize("case", sorted(LAYOUTS))
def test_step_layouts(case):
    from chocosgd_amd import codec
    lens, dtypes, shift = LAYOUTS[case]
    cap = next(k for k in range(1, 4096) if codec.params_sign_step_launches(k + 1) == 2)
    if case == "three launches":
        assert len(lens) == 2 * cap + 3 and codec.params_sign_step_launches(len(lens)) == 3
    c = Carved(lens, dtypes, shift)
    c0 = codec.launch_count("param_sign_step_kernel")
    codec.params_sign_step(c.views, words_dev(c.verdict), c.lrs)
    assert codec.launch_count("param_sign_step_kernel") - c0 == codec.params_sign_step_launches(len(lens))
    c.check(c.stores)  # every tensor, and the sentinel everywhere else


class Loopback:
    """rank 0's all_gather: its own message, then the other ranks', made from their prepared d_p
    -- packed words for the fused step, dense +-1 tensors for the loop."""

    def __init__(self, others):
        self.others = others

    def _agg(self, data, communication_scheme=None, async_op=False):
        from chocosgd_amd import codec
        assert communication_scheme == "all_gather"
        if data.dtype == torch.int32:
            return [data] + [codec.sign_compress(torch.from_numpy(d).to(DEV), want_norms=False)[0] for d in self.others]
        return [data] + [torch.where(torch.from_numpy(d) < 0, -1.0, 1.0) for d in self.others]


@pytest.mark.parametrize("world", [3, 4])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_fused_step_vs_loop(dtype, momentum, world):
    from chocosgd_amd import codec, sign_sgd
    lens = golden_json("layouts.json")["resnet20_cifar10"]
    rng = np.random.RandomState(world)
    models = []
    for dev in (DEV, "cpu"):
        g = torch.Generator().manual_seed(5)
        ps = [torch.nn.Parameter(torch.randn(m, generator=g).to(DTYPES[dtype]).to(dev)) for m in lens]
        # weight_decay exact in bf16: torch on the CPU rounds an add's alpha to the tensors' dtype, on the
        # device (the batched d_p's contract) it does not; the step kernel rounds lr as the CPU does
        groups = [{"params": [p], "name": f"p{i}", "lr": 0.01 * (i % 3 + 1), "weight_decay": 2.0 ** -13, "momentum": momentum,
                   "dampening": 0.0, "nesterov": False} for i, p in enumerate(ps)]
        models.append((ps, groups, collections.defaultdict(dict)))
    names = list(enumerate(f"p{i}" for i in range(len(lens))))
    for step in range(2):  # the second step reads the momentum buffers
        agg = Loopback([rng.standard_normal(sum(lens)).astype(np.float32) for _ in range(world - 1)])
        grads = [torch.from_numpy(rng.standard_normal(m).astype(np.float32)).to(DTYPES[dtype]) for m in lens]
        bits = []
        for (ps, groups, state), step_fn in zip(models, (sign_sgd.fused_step, sign_sgd.step_loop)):
            for p, gr in zip(ps, grads):
                p.grad = gr.clone().to(p.device)
            c0 = codec.launch_count("sign_vote_kernel"), codec.launch_count("param_sign_step_kernel")
            bits.append(step_fn(sign_sgd.MajorityVoteCompressor(0, world, agg, "gpu"), groups, names, state))
            ran = codec.launch_count("sign_vote_kernel") - c0[0], codec.launch_count("param_sign_step_kernel") - c0[1]
            assert ran == ((1, 1) if step_fn is sign_sgd.fused_step else (0, 0))
        assert bits[0] == bits[1] == 32 * O.sign_words(sum(lens))
        (pd, _, sd), (pc, _, sc) = models
        for i, (a, b) in enumerate(zip(pd, pc)):
            assert torch.equal(a.data.cpu(), b.data), ("param", step, i)
            assert torch.equal(a.grad.cpu(), b.grad), ("d_p", step, i)
            if momentum:
                assert torch.equal(sd[a]["momentum_buffer"].cpu(), sc[b]["momentum_buffer"]), ("buffer", step, i)


def _finite(t):
    return torch.where(torch.isfinite(t), t, torch.ones_like(t))


def test_streams_vote():
    from chocosgd_amd import codec
    W, nwords = 3, O.sign_words(sum(LIST4))
    true, poison = random_words(1, W, nwords), random_words(2, W, nwords)
    work = {f"m{q}": words_dev(poison[q]) for q in range(W)}
    out = torch.empty(nwords, dtype=torch.int32, device=DEV)
    _, _, outs = ST.run(lambda: codec.sign_vote(list(work.values()), out=out), work,
                        {f"m{q}": words_dev(true[q]) for q in range(W)}, {f"m{q}": words_dev(poison[q]) for q in range(W)},
                        outs=[out], family="sign_vote", case="vote")
    assert torch.equal(outs[0].cpu(), torch.from_numpy(vote_ref(true).view(np.int32)))


def test_streams_step():
    from chocosgd_amd import codec
    c = Carved(LIST4, MIXED, 1)
    work = dict(c.stores, verdict=words_dev(c.verdict))
    true = {k: t.clone() for k, t in work.items()}
    poison = {**{d: _finite(t) * 0.5 + 1.0 for d, t in c.stores.items()}, "verdict": words_dev(~c.verdict)}
    plan = codec.ParamSgdPlan(c.views)
    _, got, _ = ST.run(lambda: codec.params_sign_step(c.views, work["verdict"], c.lrs, plan=plan), work, true, poison,
                       family="sign_vote", case="step")
    c.check(got)

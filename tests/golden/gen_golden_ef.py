"""Golden-vector generator for the two error-feedback optimizers' steps: DeepSqueeze.step
(dl_code/pcode/optim/deep_squeeze.py:94-127) and EF_SignSGD.step (ef_sign_sgd.py:78-123).

Runs ONLY in the authoring container, where the upstream reference is mounted read-only at
/root/reference: it builds the reference's own optimizers with object.__new__ (as
gen_golden_mix.py does), with a no-op timer, the reference's own compressors behind a wrapper
that records what they are handed and what they return, aggregators replaced by stand-ins that
supply the neighbours' messages (made by the reference's compressors from recorded buffers),
and the bit2byte stub of gen_golden.py, and runs the reference's own step on CPU fp32 tensors
for two steps.  Nothing from the reference is copied: the fixtures are data only.

Layout: the first ten tensors of layouts.json's resnet20_cifar10 (no zero-length tensor).
DeepSqueeze: a ring of 3, this rank 1; EF-signSGD: 3 ranks, this rank 1.  Momentum 0.9, weight
decay 1e-4, lr 0.1, a non-zero starting memory (the exact set: lr 0.5, momentum 0.5 and NO
weight decay -- 1e-4 is not a power of two -- and consensus_stepsize 0.75, whose products with
1/3 and -2/3 round to 0.25 and -0.5 in fp32).

    ef_<set>_<run>.npz   run = ds_topk, ds_sign, efsign
      layout, hp = [lr, weight_decay, momentum], gamma, rank, p0, mem0, g [2, n] (the gradient
      set before each step), nbr [2, 2, n] (step, neighbour 0 / 2: the buffer that neighbour's
      compressor is handed), and per step t = 1, 2:
        s<t>_sgd      the params when compress is called (DeepSqueeze: after apply_gradient)
        s<t>_handed   the buffer compress is handed
        s<t>_norms    this rank's norms (sign runs)
        s<t>_local    the local copy compress returns
        s<t>_mem      the memory after the step
        s<t>_msg<r>_<c>   rank r's raw message of exchange call c
        s<t>_agg      DeepSqueeze: the aggregate; EF: the divided synced_grads
        s<t>_summed   EF: synced_grads before the division
        s<t>_params, s<t>_bufs, s<t>_grad    the model, the momentum buffers and p.grad after
        s<t>_n_bits

Sets:  general   every flat input repeats a block of 509 values; planted: a param of -0 under
                 an aggregate of +0 (ds_topk), an inf memory and a NaN gradient, and a tensor
                 of tiny values whose quotient by 3 and product with -lr are subnormal (efsign).
                 Feeds the stage tests, which take the recorded intermediates as inputs.
       distinct  not tiled; every tensor's magnitudes handed to a top-k are distinct and
                 nonzero in both steps (asserted): the selection has no ties.  ds_topk only.
       exact     every value handed to a norm is a multiple of one power of two 2^-E with
                 numel_s * max|v| * 2^E < 2^24, in both steps, for every rank (asserted): the
                 L1 norm is the same bits in any summation order.  ds_sign and efsign.

Usage:  python tests/golden/gen_golden_ef.py
"""
import collections
import contextlib
import copy
import json
import os
import sys
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference

import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
import gen_golden  # noqa: E402,F401  (installs the bit2byte stub and the reference's path)

import pcode.optim.deep_squeeze as ref_ds  # noqa: E402
import pcode.optim.ef_sign_sgd as ref_ef  # noqa: E402
from pcode.utils.tensor_buffer import TensorBuffer  # noqa: E402

with open(os.path.join(OUT, "layouts.json")) as f:
    LAYOUT = json.load(f)["resnet20_cifar10"][:10]
N = sum(LAYOUT)
OFF = np.concatenate([[0], np.cumsum(LAYOUT)]).astype(int)
PERIOD = 509
W, RANK, OTHERS = 3, 1, (0, 2)
HP = (0.1, 1e-4, 0.9)
HP_EXACT = (0.5, 0.0, 0.5)
GAMMA, GAMMA_EXACT = 0.5, 0.75
RATIO = 0.9
TINY = float(np.finfo(np.float32).tiny)
# general set: offsets into tensor 0 / tensor 3; tensor 1 holds the tiny values
NEG_ZERO, INF_MEM, NAN_GRAD, TINY_TENSOR = 7, 30, 41, 1
UNIT = 2.0 ** -6  # exact set: the inputs are integer multiples of it


def split(flat):
    return [torch.from_numpy(np.ascontiguousarray(flat[a:b]).copy()) for a, b in zip(OFF[:-1], OFF[1:])]


def cat(tensors):
    return np.concatenate([t.detach().numpy().reshape(-1) for t in tensors]).astype(np.float32)


def timer(*args, **kargs):
    return contextlib.nullcontext()


# ----------------------------------------------------------------------------- inputs
def tiled(rng, scale):
    block = (rng.standard_normal(PERIOD) * scale * 10.0 ** rng.uniform(-2, 1, PERIOD)).astype(np.float32)
    return np.tile(block, N // PERIOD + 1)[:N].copy()


def general_inputs():
    rng = np.random.RandomState(20241020)
    p0, mem0 = tiled(rng, 1.0), tiled(rng, 0.3)
    g = np.stack([tiled(rng, 0.1) for _ in range(2)])
    nbr = np.stack([[tiled(rng, 1.0) for _ in OTHERS] for _ in range(2)])
    a, b = OFF[TINY_TENSOR], OFF[TINY_TENSOR + 1]
    tiny = lambda: (rng.uniform(1.0, 3.0, b - a) * rng.choice([-1.0, 1.0], b - a) * 1.0e-38).astype(np.float32)  # noqa: E731
    p0[a:b] = 0.0
    mem0[a:b] = tiny()
    for t in range(2):
        g[t, a:b] = tiny()
        for j in range(2):
            nbr[t, j, a:b] = tiny()
    p0[NEG_ZERO], mem0[NEG_ZERO], g[:, NEG_ZERO], nbr[:, :, NEG_ZERO] = -0.0, 0.0, 0.0, 0.0
    mem0[OFF[3] + INF_MEM] = np.inf
    g[0, OFF[3] + NAN_GRAD] = np.nan
    return dict(p0=p0, mem0=mem0, g=g, nbr=nbr)


def distinct_inputs(seed):
    rng = np.random.RandomState(seed)
    r = lambda s: (rng.standard_normal(N) * s).astype(np.float32)  # noqa: E731
    return dict(p0=r(1.0), mem0=r(0.3), g=np.stack([r(0.1), r(0.1)]),
                nbr=np.stack([[r(1.0) for _ in OTHERS] for _ in range(2)]))


def exact_inputs(kind):
    """Integer multiples of UNIT.  The buffers a norm is taken of in step 1 (this rank's and the
    neighbours') have per-tensor sums of magnitudes that are multiples of numel_s * UNIT, so
    norm_s / numel_s is a multiple of UNIT and everything step 2 takes a norm of stays on a
    power-of-two grid."""
    rng = np.random.RandomState(20241022 + (kind == "efsign"))

    def even():
        return (2 * rng.randint(1, 5, N) * rng.choice([-1, 1], N)).astype(np.int64)

    def divisible():
        k = even()
        for a, b in zip(OFF[:-1], OFF[1:]):
            d = int(-np.abs(k[a:b]).sum()) % (b - a)
            k[a:a + d] += np.sign(k[a:a + d])
            assert np.abs(k[a:b]).sum() % (b - a) == 0
        return k

    b1, mem0, g1, g2 = divisible(), even(), even(), even()
    if kind == "efsign":  # handed = d_p + memory, d_p = g1 in the first step
        g1, p0 = b1 - mem0, even()
        scale_p = 1.0
    else:  # handed = memory + params after the step p0 - lr * g1, lr = 0.5
        p0, scale_p = 2 * (b1 - mem0) + g1, 0.5
    f = lambda k, s=1.0: (k * (UNIT * s)).astype(np.float32)  # noqa: E731
    nbr = np.stack([[f(divisible()) for _ in OTHERS], [f(even()) for _ in OTHERS]])
    return dict(p0=f(p0, scale_p), mem0=f(mem0), g=np.stack([f(g1), f(g2)]), nbr=nbr)


# ----------------------------------------------------------------------------- the reference's optimizers
class Neighbours:
    """In the aggregators' place: this rank's own data with the neighbours' recorded messages."""

    def __init__(self):
        self.msgs, self.call, self.own = {}, 0, []

    def start(self, msgs):
        self.msgs, self.call, self.own = msgs, 0, []

    def _agg(self, data, op=None, force_wait=True, communication_scheme=None, async_op=False):
        c = self.call
        self.call += 1
        self.own.append(data.clone())
        if communication_scheme == "all_gather":
            return [data if r == RANK else self.msgs[r][c] for r in range(W)]
        assert op == "get_raw_sync_data" and force_wait is True
        return {r: (data if r == RANK else self.msgs[r][c]) for r in range(W)}


class Capture:
    def __init__(self):
        self.sent = []

    def _agg(self, data, op=None, force_wait=True, communication_scheme=None, async_op=False):
        self.sent.append(data.clone())
        return {RANK: data}


class _World(int):
    """world_size for a probe compressor: range() sees 3, `world_size * 1.0` gives 1.0, so the
    reference's own decompress leaves the sum undivided."""

    def __mul__(self, other):
        return 1.0


class Recorder:
    """Wraps the reference's compressor: records what it is handed and what it returns."""

    def __init__(self, inner, params):
        self.inner, self.params, self.rec = inner, params, {}

    # DeepSqueeze
    def compress(self, arg):
        tb = arg["params_tb"] if isinstance(arg, dict) else arg
        self.rec = {"handed": tb.buffer.clone().numpy(), "sgd": cat(self.params)}
        out = self.inner.compress(arg)
        sb = arg if isinstance(arg, dict) else out
        local = out if isinstance(arg, dict) else out["synced_grads_tb"]
        self.rec["local"] = local.buffer.clone().numpy()
        norms = sb.get("param_norms_tb", sb.get("grad_norms_tb"))
        if norms is not None:
            self.rec["norms"] = norms.buffer.clone().numpy()
        return out

    def sync(self, sb):
        self.inner.sync(sb)

    def uncompress(self, sb, neighbors_info):
        out = self.inner.uncompress(sb, neighbors_info)
        self.rec["agg"] = out.buffer.clone().numpy()
        return out

    # EF-signSGD
    def decompress(self, sb):
        probe = ref_ef.EFSignCompressor(rank=RANK, world_size=_World(W), aggregator=None, comm_op="sign",
                                        comm_device="gpu", use_ipc=False)
        sb2 = dict(sb)
        sb2["synced_grads_tb"] = copy.deepcopy(sb["synced_grads_tb"])
        self.rec["summed"] = probe.decompress(sb2).buffer.clone().numpy()
        out = self.inner.decompress(sb)
        self.rec["agg"] = out.buffer.clone().numpy()
        return out


def model(p0, hp):
    lr, wd, mom = hp
    params = [torch.nn.Parameter(t) for t in split(p0)]
    groups = [{"params": [p], "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": 0.0, "nesterov": False,
               "name": f"p{i}", "param_size": p.size(), "nelement": p.nelement()} for i, p in enumerate(params)]
    return params, groups


def consumer_args(comm_op, gamma):
    return dict(comm_op=comm_op, comm_device="gpu", compress_ratio=RATIO, quantize_level=4, is_biased=False,
                backend="nccl", use_ipc=False, consensus_stepsize=gamma)


def neighbour_messages(run, comm_op, gamma, buf, r):
    """Rank r's raw messages (one per exchange call) for the buffer its compressor is handed."""
    cap = Capture()
    if run == "efsign":
        comp = ref_ef.EFSignCompressor(rank=r, world_size=W, aggregator=cap, comm_op="sign", comm_device="gpu",
                                       use_ipc=False)
        sb = comp.compress(TensorBuffer(split(buf)))
    else:
        comp = ref_ds.DeepSqueezeCompressor(aggregator=cap, rank=r, **consumer_args(comm_op, gamma))
        sb = {"original_shapes": [(torch.Size([m]), m) for m in LAYOUT], "params_tb": TensorBuffer(split(buf))}
        comp.compress(sb)
    comp.sync(sb)
    return cap.sent


def run(run_name, comm_op, inp, hp, gamma):
    params, groups = model(inp["p0"], hp)
    nb = Neighbours()
    if run_name == "efsign":
        opt = object.__new__(ref_ef.EF_SignSGD)
        inner = ref_ef.EFSignCompressor(rank=RANK, world_size=W, aggregator=nb, comm_op="sign", comm_device="gpu",
                                        use_ipc=False)
        opt.memory_tb = TensorBuffer(split(inp["mem0"]))
    else:
        opt = object.__new__(ref_ds.DeepSqueeze)
        inner = ref_ds.DeepSqueezeCompressor(aggregator=nb, rank=RANK, **consumer_args(comm_op, gamma))
        opt.memory = TensorBuffer(split(inp["mem0"]))
        opt.shapes = [(g["param_size"], g["nelement"]) for g in groups]
        opt.neighbors_info = {r: 1.0 / W for r in range(W)}
    opt.param_groups, opt.state = groups, collections.defaultdict(dict)
    opt.param_names = list(enumerate(g["name"] for g in groups))
    opt.rank = RANK
    opt.conf = types.SimpleNamespace(epoch_=0)
    opt.compressor = Recorder(inner, params)
    out = dict(layout=np.array(LAYOUT, dtype=np.int64), hp=np.array(hp, dtype=np.float64), gamma=np.float64(gamma),
               rank=np.int64(RANK), **inp)
    for t in (1, 2):
        for p, gt in zip(params, split(inp["g"][t - 1])):
            p.grad = gt  # a fresh tensor: the reference's rebinding of p.grad never aliases the next gradient
        msgs = {r: neighbour_messages(run_name, comm_op, gamma, inp["nbr"][t - 1, j], r) for j, r in enumerate(OTHERS)}
        nb.start(msgs)
        n_bits = opt.step(timer=timer)
        mem = (opt.memory_tb if run_name == "efsign" else opt.memory).buffer  # rebound by the step
        rec = opt.compressor.rec
        for k, v in rec.items():
            out[f"s{t}_{k}"] = v
        msgs[RANK] = nb.own
        for r in range(W):
            for c, m in enumerate(msgs[r]):
                out[f"s{t}_msg{r}_{c}"] = m.numpy()
        out[f"s{t}_mem"] = mem.clone().numpy()
        out[f"s{t}_params"] = cat(params)
        out[f"s{t}_bufs"] = cat([opt.state[p]["momentum_buffer"] for p in params])
        out[f"s{t}_grad"] = cat([p.grad.data for p in params])
        out[f"s{t}_n_bits"] = np.float64(n_bits)
    return out


# ----------------------------------------------------------------------------- what the tests rely on
def bits(v):
    return int(np.float32(v).view(np.uint32))


def check_general(outs):
    tk = outs["ds_topk"]
    assert bits(tk["s1_sgd"][NEG_ZERO]) == 0x80000000 and bits(tk["s1_agg"][NEG_ZERO]) == 0
    assert bits(tk["s1_params"][NEG_ZERO]) == 0, "(-0) + (+0) must be +0"
    for name, out in outs.items():
        assert np.isnan(out["s1_handed"][OFF[3] + NAN_GRAD]) and np.isinf(out["s1_handed"][OFF[3] + INF_MEM]), name
    ef = outs["efsign"]
    lr = np.float32(-ef["hp"][0])
    found_q = found_p = False
    for t in (1, 2):
        q = ef[f"s{t}_agg"]
        found_q |= bool(np.any((q != 0) & (np.abs(q) < TINY) & (np.abs(ef[f"s{t}_summed"]) >= TINY)))
        with np.errstate(all="ignore"):
            pr = (lr * q).astype(np.float32)
        found_p |= bool(np.any((pr != 0) & (np.abs(pr) < TINY)))
    assert found_q, "no normal sum whose quotient by 3 is subnormal"
    assert found_p, "no product with -lr that is subnormal"


def check_distinct(out):
    bufs = [out["s1_handed"], out["s2_handed"]] + [out["nbr"][t, j] for t in range(2) for j in range(2)]
    for buf in bufs:
        for a, b in zip(OFF[:-1], OFF[1:]):
            mag = np.abs(buf[a:b])
            assert np.all(mag > 0) and np.unique(mag).size == b - a, "a tie in a top-k input"


def check_exact(out, E=12):
    bufs = [out["s1_handed"], out["s2_handed"]] + [out["nbr"][t, j] for t in range(2) for j in range(2)]
    for buf in bufs:
        k = buf.astype(np.float64) * 2.0 ** E
        assert np.all(k == np.round(k)), "a value off the 2^-E grid"
        for a, b in zip(OFF[:-1], OFF[1:]):
            assert (b - a) * np.abs(k[a:b]).max() < 2 ** 24, "the norm could depend on the summation order"


def save(name, out, limit):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size)
    assert size <= limit, "larger than the largest fixture there was"


def main():
    torch.set_num_threads(1)
    limit = max(os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if not f.startswith("ef_"))
    gen = general_inputs()
    outs = {"ds_topk": run("ds_topk", "compress_top_k", gen, HP, GAMMA),
            "ds_sign": run("ds_sign", "sign", gen, HP, GAMMA),
            "efsign": run("efsign", "sign", gen, HP, GAMMA)}
    check_general(outs)
    for name, out in outs.items():
        save(f"ef_general_{name}", out, limit)
    for seed in range(20241021, 20241021 + 64):  # the first seed whose six top-k inputs hold no tie
        out = run("ds_topk", "compress_top_k", distinct_inputs(seed), HP, GAMMA)
        try:
            check_distinct(out)
        except AssertionError:
            continue
        print("distinct set: seed", seed)
        break
    else:
        raise AssertionError("no seed without a tie")
    save("ef_distinct_ds_topk", out, limit)
    for name in ("ds_sign", "efsign"):
        out = run(name, "sign", exact_inputs(name), HP_EXACT, GAMMA_EXACT)
        check_exact(out)
        save(f"ef_exact_{name}", out, limit)


if __name__ == "__main__":
    main()

"""Golden-vector generator for the neighbour-weighted model mix of DCD_PSGD.step, ECD_PSGD.step
and the decentralized branch of SGD.step (dl_code/pcode/optim/dcd_psgd.py:96-144,
ecd_psgd.py:99-157, sgd.py:94-121).

Runs ONLY in the authoring container, where the upstream reference is mounted read-only at
/root/reference: it builds the reference's own optimizers with object.__new__ (as
gen_golden_dgc_sgd.py does), with a no-op timer, a compressor that records the buffers it is
handed and leaves the replicas alone, and dist.isend / dist.irecv replaced by stand-ins that
supply the neighbours' messages, and runs the reference's own step on CPU fp32 tensors.
Nothing from the reference is copied: the fixtures are data only.

    mix_inputs.npz   lens, p0, g (flat, the tensors back to back), hats [5, n] (replica r of a
                     neighbourhood is hats[r]; for D-PSGD hats[r] is what neighbour r sends),
                     hp = [lr, weight_decay, momentum, dampening, nesterov]
    mix_<set>.npz    ranks, weights (the neighbourhood in dict order), rank (this rank), and
                       dcd_half, dcd_packed       what DCD's compressor is handed
                       ecd<t>_params, ecd<t>_extrap   the model after the step and what ECD's
                                                  compressor is handed, local_index t = 1, 5
                       dpsgd_sent, dpsgd_agg      the flat params D-PSGD sends, the model after

Every flat input repeats a block of 509 values (a prime: no tile, group or wavefront boundary
is a multiple of it, so a misplaced element still shows) -- the arrays compress to a few KB
each.  Planted in the 8195-element tensor: a position where every source (and, for D-PSGD, the
own model) is -0.0; +0 and -0 gradients; an inf source under the 5-source set's zero weight; a
NaN gradient; a source whose product with its weight is subnormal.

Usage:  python tests/golden/gen_golden_mix.py
"""
import collections
import contextlib
import os
import sys
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the read-only reference

import numpy as np  # noqa: E402
import torch  # noqa: E402

REF = "/root/reference/dl_code"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
# the reference's sparsification module imports the unvendored bit2byte packing extension, which
# nothing here calls: an empty module lets the import pass (gen_golden.py stubs it the same way)
sys.modules.setdefault("bit2byte", types.ModuleType("bit2byte"))

import pcode.optim.dcd_psgd as ref_dcd  # noqa: E402
import pcode.optim.ecd_psgd as ref_ecd  # noqa: E402
import pcode.optim.sgd as ref_sgd  # noqa: E402
import pcode.utils.communication as ref_comm  # noqa: E402
from pcode.utils.tensor_buffer import TensorBuffer  # noqa: E402

LENS = [5, 1, 0, 8195, 33, 4099, 17000, 40, 40, 1]
PERIOD = 509
HP = (0.1, 1e-4, 0.9, 0.0, False)  # lr, weight_decay, momentum, dampening, nesterov
SETS = {  # this rank, {rank: weight} in the order the reference's dicts hold them
    "ring3": (1, {0: 1.0 / 3, 1: 1.0 / 3, 2: 1.0 / 3}),
    "five": (2, {0: 0.4, 1: 0.0, 2: 0.25, 3: 0.2, 4: 0.15}),
    "one": (0, {0: 1.0}),
}
LOCAL_INDEX = [1, 5]
# offsets into the 8195-element tensor
ALL_NEG_ZERO, G_POS_ZERO, G_NEG_ZERO, INF_SRC, G_NAN, SUBNORMAL = 11, 20, 21, 30, 41, 52


def tiled(rng, n, scale):
    block = (rng.standard_normal(PERIOD) * scale * 10.0 ** rng.uniform(-2, 1, PERIOD)).astype(np.float32)
    return np.tile(block, n // PERIOD + 1)[:n].copy()


def inputs():
    rng = np.random.RandomState(20241019)
    n = sum(LENS)
    o = int(np.cumsum(LENS)[2])  # flat offset of the 8195-element tensor
    p0, g = tiled(rng, n, 1.0), tiled(rng, n, 0.1)
    hats = np.stack([tiled(rng, n, 1.0) for _ in range(5)])
    hats[:, o + ALL_NEG_ZERO] = -0.0
    p0[o + ALL_NEG_ZERO], g[o + ALL_NEG_ZERO] = -0.0, 0.0
    g[o + G_POS_ZERO], g[o + G_NEG_ZERO] = 0.0, -0.0
    hats[1, o + INF_SRC] = np.inf
    g[o + G_NAN] = np.nan
    hats[:, o + SUBNORMAL] = 0.0
    hats[0, o + SUBNORMAL] = 2.0e-38
    return p0, g, hats


def split(flat):
    out, o = [], 0
    for m in LENS:
        out.append(torch.from_numpy(flat[o:o + m].copy()))
        o += m
    return out


def cat(tensors):
    return np.concatenate([t.detach().numpy().reshape(-1) for t in tensors]).astype(np.float32)


def timer(*args, **kargs):
    return contextlib.nullcontext()


class Recorder:
    """The compressor's place: records what compress() is handed, changes no replica."""

    def __init__(self):
        self.seen = {}

    def compress(self, sync_buffer):
        self.seen = {k: v.buffer.clone() for k, v in sync_buffer.items() if hasattr(v, "buffer")}
        sync_buffer["n_bits"] = 0

    def sync(self, sync_buffer):
        pass

    def uncompress(self, *args):
        pass


def optimizer(cls, p0, g, rank, info):
    lr, wd, mom, damp, nest = HP
    params = [torch.nn.Parameter(t) for t in split(p0)]
    for p, gt in zip(params, split(g)):
        p.grad = gt
    opt = object.__new__(cls)
    opt.param_groups = [{"params": [p], "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": damp,
                         "nesterov": nest, "name": f"p{i}", "param_size": p.size(), "nelement": p.nelement()}
                        for i, p in enumerate(params)]
    opt.state = collections.defaultdict(dict)
    opt.param_names = list(enumerate(group["name"] for group in opt.param_groups))
    opt.rank, opt.neighbors_info = rank, info
    opt.conf = types.SimpleNamespace(epoch_=0, local_index=None, is_centralized=False, comm_device="gpu")
    return opt, params


def with_replicas(opt, hats, info):
    opt.shapes = [(g["param_size"], g["nelement"]) for g in opt.param_groups]
    opt.neighbor_hat_params = {r: TensorBuffer(split(hats[r])) for r in info}
    opt.compressor = Recorder()


def run_set(p0, g, hats, rank, info):
    out = {"ranks": np.array(list(info), dtype=np.int64), "weights": np.array(list(info.values()), dtype=np.float64),
           "rank": np.int64(rank)}
    # DCD
    opt, params = optimizer(ref_dcd.DCD_PSGD, p0, g, rank, info)
    with_replicas(opt, hats, info)
    opt.step(timer=timer)
    out["dcd_half"] = opt.compressor.seen["flatten_half_params"].numpy()
    out["dcd_packed"] = opt.compressor.seen["flatten_params"].numpy()
    assert np.array_equal(cat(params).view(np.uint32), hats[rank].view(np.uint32))  # the model is the own replica
    # ECD
    for t in LOCAL_INDEX:
        opt, params = optimizer(ref_ecd.ECD_PSGD, p0, g, rank, info)
        with_replicas(opt, hats, info)
        opt.conf.local_index = t
        opt.step(timer=timer)
        out[f"ecd{t}_params"] = cat(params)
        out[f"ecd{t}_extrap"] = opt.compressor.seen["flatten_updated_params"].numpy()
    # D-PSGD: the reference's own aggregator with the exchange supplied
    opt, params = optimizer(ref_sgd.SGD, p0, g, rank, info)
    opt.decentralized_aggregator = ref_comm.DecentralizedAggregation(rank, info)
    sent = []

    class Done:
        def wait(self):
            pass

    def isend(tensor, dst):
        sent.append(tensor.clone())
        return Done()

    def irecv(tensor, src):
        tensor.copy_(torch.from_numpy(hats[src]))
        return Done()

    real = ref_comm.dist.isend, ref_comm.dist.irecv
    ref_comm.dist.isend, ref_comm.dist.irecv = isend, irecv
    try:
        opt.step(timer=timer)
    finally:
        ref_comm.dist.isend, ref_comm.dist.irecv = real
    assert len(sent) == len(info) - 1
    out["dpsgd_agg"] = cat(params)
    # what this rank sends: the flat params after apply_gradient (its own run for a 1-rank set)
    if sent:
        out["dpsgd_sent"] = sent[0].numpy()
    else:
        opt, params = optimizer(ref_sgd.SGD, p0, g, rank, info)
        ref_sgd.utils.apply_gradient(opt.param_groups, opt.state, apply_grad_to_model=True)
        out["dpsgd_sent"] = cat(params)
    return out


def checks(outs, hats):
    """What the tests rely on."""
    o = int(np.cumsum(LENS)[2])
    bits = lambda v: int(np.float32(v).view(np.uint32))  # noqa: E731
    for name, out in outs.items():
        for key in ("dcd_half", "ecd1_params", "dpsgd_agg"):
            assert bits(out[key][o + ALL_NEG_ZERO]) == 0, (name, key, "0 + (-0 * w) must be +0")
        assert np.isnan(out["dcd_half"][o + G_NAN]) and np.isnan(out["ecd5_extrap"][o + G_NAN])
        for key in ("dcd_half", "dpsgd_agg"):
            assert np.isnan(out[key][o + INF_SRC]) == (name == "five"), (name, key, "inf * 0 must be NaN")
    assert np.isinf(outs["ring3"]["dcd_half"][o + INF_SRC])
    x = np.float32(hats[0, o + SUBNORMAL]) * np.float32(1.0 / 3)
    assert 0 < x < np.finfo(np.float32).tiny, "the planted product is not subnormal"


def main():
    torch.set_num_threads(1)
    p0, g, hats = inputs()
    outs = {name: run_set(p0, g, hats, rank, info) for name, (rank, info) in SETS.items()}
    checks(outs, hats)
    np.savez_compressed(os.path.join(OUT, "mix_inputs.npz"), lens=np.array(LENS, dtype=np.int64), p0=p0, g=g, hats=hats,
                        hp=np.array([float(v) for v in HP], dtype=np.float64))
    total = os.path.getsize(os.path.join(OUT, "mix_inputs.npz"))
    for name, out in outs.items():
        path = os.path.join(OUT, f"mix_{name}.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path))
        total += os.path.getsize(path)
    print("total", total)


if __name__ == "__main__":
    main()

"""The all-reduce SGD step on the device: codec.params_sgd_flatgrad (csrc/sgd.hip,
param_sgd_flatgrad_kernel and its master instantiation) and utils.allreduce_sgd_step.

Everything is compared bit for bit.  The model (tests/_allreduce_oracle.py) is a correctly
rounded fp32 division of the summed gradient followed by the models of tests/_sgd_oracle.py /
tests/_master_oracle.py, all pinned to the reference's fixtures on the host
(tests/test_allreduce_sgd_host.py); the kernels are also held against the reference's recorded
steps on the device, against each other, against the path of four passes they replace and
against the torch loop.  Whole storages are compared, so that every byte a launch does not own
is checked together with the ones it does."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, golden, same_bits
import _allreduce_oracle as AO
import _master_oracle as MA
import _mp_allreduce_worker as W
import _sgd_oracle as SO
import test_gpu_param_sgd as PS  # the guarded layouts and value lists of the SGD kernel's tests

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES, NAMES, SENTINEL = PS.DTYPES, PS.NAMES, PS.SENTINEL
MODES = ["fp32", "bf16", "fp16", "mixed"]
KERNELS = ["plain", "master"]
F32 = torch.float32
STEPS = 3
host = MA.host
NAMES_COUNTED = ("param_sgd_flatgrad_kernel", "param_sgd_master_flatgrad_kernel", "param_sgd_kernel",
                 "param_sgd_master_kernel", "param_pack_kernel", "param_unpack_kernel")


def _counts():
    from chocosgd_amd import codec
    return [codec.launch_count(nm) for nm in NAMES_COUNTED]


def _delta(c0):
    return [b - a for a, b in zip(c0, _counts())]


def _guarded_flat(values, shift):
    """A flat fp32 view at element `shift` of a sentinel-filled allocation."""
    n = int(values.size)
    big = torch.full((n + 2 * shift + 8,), SENTINEL, device=DEV)
    view = big[shift:shift + n]
    if n:
        view.copy_(torch.from_numpy(values).to(DEV))
    return big, view


def _check_flat(big, shift, values, what):
    want = torch.full_like(big, SENTINEL)
    if values.size:
        want[shift:shift + values.size] = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).to(DEV)
    assert same_bits(host(big), host(want)), what


# ----------------------------------------------------------------------------- kernel against the model
def run_case(lens, mode, kernel, lead=(0, 0, 0), gap=8, own=False, gsum_shift=4, master_shift=4, hp=PS._varied_hp,
             first=lambda i: i % 2 == 0, write=True, write_grads=True, divisor=3.0, seed=7000):
    """One codec.params_sgd_flatgrad call on guarded storages against the model; returns the
    launches.  lead: sentinel elements in front of the (params, grads, buffers) storages; gsum
    and the master copy are views at an element shift inside sentinel-filled allocations."""
    from chocosgd_amd import codec
    master = kernel == "master"
    k, n = len(lens), sum(lens)
    dts = PS._dtypes(mode, k)
    P = PS.Guarded(lens, dts, seed, -3, 1, lead[0], gap, own)
    G = PS.Guarded(lens, dts, seed + 5000, -4, 0, lead[1], gap, own)  # outputs: what they hold is overwritten
    B = PS.Guarded(lens, [F32] * k if master else dts, seed + 9000, -4, 0, lead[2], gap, own)
    hps = [hp(i) for i in range(k)]
    firsts = [bool(first(i)) and hps[i][2] != 0 for i in range(k)]
    s = [PS._values(m, seed + 30000 + i, -4, 0) for i, m in enumerate(lens)]
    s_all = np.concatenate(s) if n else np.zeros(0, np.float32)
    bigs, gsum = _guarded_flat(s_all, gsum_shift)
    m0 = [PS._values(m, seed + 20000 + i, -3, 1) for i, m in enumerate(lens)]
    bigm, mview = _guarded_flat(np.concatenate(m0) if n else np.zeros(0, np.float32), master_shift)
    new_p, new_g, new_b, new_m = [], [], [], []
    for i in range(k):
        lr, wd, mom, damp, nest = hps[i]
        if master:
            m_new, b_new, p16, g16 = AO.master_step(m0[i], s[i], host(B.views[i]), divisor, lr, wd, mom, damp, nest,
                                                    firsts[i], dtype=NAMES[dts[i]])
            new_m.append(m_new)
        else:
            p16, b_new, g16 = AO.step(host(P.views[i]), s[i], host(B.views[i]), divisor, lr, wd, mom, damp, nest,
                                      firsts[i], dtype=NAMES[dts[i]])
        new_p.append(p16 if write else None), new_g.append(g16 if write_grads else None), new_b.append(b_new)
    c0 = _counts()
    codec.params_sgd_flatgrad(P.views, G.views, [b if hps[i][2] != 0 else None for i, b in enumerate(B.views)], gsum,
                              divisor, [h[0] for h in hps], [h[1] for h in hps], [h[2] for h in hps],
                              [h[3] for h in hps], [h[4] for h in hps], firsts, master=mview if master else None,
                              write=write, write_grads=write_grads)
    d = _delta(c0)
    P.check(new_p, "params (or their guards)")
    G.check(new_g, "grads (or their guards)")
    B.check(new_b, "momentum buffers (or their guards)")
    _check_flat(bigs, gsum_shift, s_all, "gsum was written")
    _check_flat(bigm, master_shift, np.concatenate(new_m) if master and n else np.concatenate(m0) if n else s_all,
                "master (or its guards)")
    want = [0] * len(NAMES_COUNTED)
    want[1 if master else 0] = codec.params_sgd_flatgrad_launches(k)
    assert d == want, "launches: only the kernel of this call, once per chunk"
    return d[1 if master else 0]


@pytest.mark.parametrize("gap", [1, 2, 3])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_views_at_element_alignment(kernel, mode, gap):
    """Views into one allocation whose element offsets run through every residue (lead 1, gaps
    1 / 2 / 3), special values in gsum, p, master and buf: nothing next to a tensor is touched."""
    run_case(PS.BASE, mode, kernel, lead=(1, 1, 1), gap=gap)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_aligned_layout(kernel, mode):
    """Every side on the group grid where the flat offset allows it: the 16-byte path."""
    run_case(PS.BASE, mode, kernel, own=True)
    run_case([40, 8192 + 24, 8, 304], mode, kernel, own=True, first=lambda i: False)


@pytest.mark.parametrize("off", ["p", "grad", "buf", "gsum", "master"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_one_side_off_the_grid_falls_back(kernel, mode, off):
    """Every length a multiple of 8 and each tensor its own allocation: all sides are on the
    16-byte grid but the one moved by an element (gsum, master: 4-byte aligned, one element on).
    The whole tensor moves element by element and no neighbouring byte changes.  (The plain
    kernel has no master side: there the case moves nothing and takes the 16-byte path.)"""
    lead = {"p": (1, 0, 0), "grad": (0, 1, 0), "buf": (0, 0, 1)}.get(off, (0, 0, 0))
    run_case([40, 8192 + 24, 8, 304], mode, kernel, lead=lead, own=True, first=lambda i: False,
             gsum_shift=5 if off == "gsum" else 4, master_shift=5 if off == "master" else 4)


@pytest.mark.parametrize("lead", [(3, 3, 3), (3, 3, 7), (3, 3, 5), (3, 7, 3), (7, 3, 3)])
@pytest.mark.parametrize("mode", ["bf16", "mixed"])
def test_master_sides_of_different_element_sizes_at_an_odd_offset(mode, lead):
    """The long tensor sits at flat offset 3: its 16-bit p and grad are congruent with the group
    grid when their lead is 3 mod 8, its fp32 buf when its lead is 3 mod 4.  Same bits every way."""
    run_case([3, 8192 + 24, 13, 300], mode, "master", lead=lead, own=True, first=lambda i: False)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_a_tensor_across_several_tiles(kernel, mode):
    run_case([3 * 8192 + 5], mode, kernel, own=True)
    run_case([100, 3 * 8192 + 77, 50], mode, kernel, gap=8)


@pytest.mark.parametrize("count", [71, 72, 73, 145])
@pytest.mark.parametrize("kernel", KERNELS)
def test_chunk_boundaries_inside_a_tile(kernel, count):
    lens = [1 + i % 13 for i in range(count)]
    assert run_case(lens, "mixed", kernel, gap=8) == -(-count // 72)
    assert run_case(lens, "bf16", kernel, gap=1, lead=(1, 1, 1)) == -(-count // 72)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_zero_length_tensors(kernel, mode):
    run_case([0, 5, 0, 0, 4100, 0], mode, kernel)
    run_case([0, 304, 0, 8200, 40], mode, kernel, own=True)


@pytest.mark.parametrize("write,write_grads", [(False, True), (True, False), (False, False)])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_a_write_switched_off_leaves_those_bytes_alone(kernel, mode, write, write_grads):
    run_case(PS.BASE, mode, kernel, write=write, write_grads=write_grads)
    run_case([8192 + 16, 64], mode, kernel, write=write, write_grads=write_grads, own=True)


@pytest.mark.parametrize("divisor", [1.0, 2.0, 3.0, 7.0])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", KERNELS)
def test_divisors(kernel, mode, divisor):
    """1 (x / 1 is x: the single-process step), 2 (exact), 3 and 7 (a reciprocal multiply
    differs from the division on about a third of the values)."""
    run_case([33, 8195, 4099], mode, kernel, divisor=divisor)
    run_case([40, 8192 + 24, 304], mode, kernel, divisor=divisor, own=True)


@pytest.mark.parametrize("mode", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("kernel", KERNELS)
def test_uniform_hyperparameter_sets(kernel, mode):
    for lr, wd, mom, damp, nest in [(0.1, 0, 0, 0, False), (0.05, 1e-4, 0, 0, False), (0.1, 0, 0.9, 0, False),
                                    (0.1, 5e-4, 0.9, 0, True), (0.01, 1e-4, 0.9, 0.1, False)]:
        for fst in (True, False):
            run_case([33, 8195, 4099], mode, kernel, hp=lambda i: (lr, wd, mom, damp, nest), first=lambda i: fst)


def test_grads_may_be_left_out_without_the_grad_write():
    from chocosgd_amd import codec
    lens = [40, 300, 7]
    for master in (False, True):
        p = [torch.from_numpy(PS._values(m, i, -3, 1)).to(DEV).to(torch.bfloat16) for i, m in enumerate(lens)]
        q = [t.clone() for t in p]
        g = [torch.full((m,), SENTINEL, device=DEV, dtype=torch.bfloat16) for m in lens]
        gsum = torch.from_numpy(PS._values(sum(lens), 9, -4, 0)).to(DEV)
        ms = [torch.cat([t.float() for t in p]) for _ in range(2)] if master else [None, None]
        codec.params_sgd_flatgrad(p, None, None, gsum, 3.0, 0.1, master=ms[0], write_grads=False)
        codec.params_sgd_flatgrad(q, g, None, gsum, 3.0, 0.1, master=ms[1], write_grads=True)
        assert all(same_bits(host(a), host(b)) for a, b in zip(p, q))
        with pytest.raises(RuntimeError):  # the grad write needs somewhere to write
            codec.params_sgd_flatgrad(p, None, None, gsum, 3.0, 0.1, master=ms[0])


# ----------------------------------------------------------------------------- the reference's recorded steps
@pytest.mark.parametrize("master", [False, True])
@pytest.mark.parametrize("name", ["plain", "wd", "mom", "nesterov", "damp"])
def test_fixture_replay(name, master):
    """The reference's three steps of world 3 replayed through utils.allreduce_sgd_step on the
    device, the loopback aggregator returning the recorded sums: the averaged gradients, p and
    buf after every step, and the launches the steps took.  With fp32 tensors the master step
    gives the reference's bits too."""
    from chocosgd_amd import codec, utils
    inputs, sums, fx = golden("sgd_inputs"), golden("allreduce_sgd_sums"), golden(f"allreduce_sgd_{name}")
    hp = fx["hp"].tolist()
    params, groups, lens = PS._device_model(inputs, hp)
    for i, g in enumerate(groups):
        g["name"] = f"p{i}"
    names = list(enumerate(g["name"] for g in groups))
    n = sum(lens)
    agg = AO.Loopback(3, sums=[sums[f"sum{k}"] for k in range(STEPS)])
    mw = utils.MasterWeights(groups, names) if master else None
    state = collections.defaultdict(dict)
    c0 = _counts()
    for k in range(STEPS):
        o = 0
        for p, m in zip(params, lens):
            p.grad = torch.from_numpy(inputs[f"g{k}"][o:o + m].copy()).to(DEV)
            o += m
        grads = [p.grad for p in params]
        assert utils.allreduce_sgd_step(groups, names, state, agg, master=mw) == 32 * n
        assert same_bits(agg.seen[k], inputs[f"g{k}"]), "the packed gradients"
        assert all(p.grad is g for p, g in zip(params, grads))
        assert same_bits(PS._cat(grads), sums[f"avg{k}"]), f"the averaged gradient after step {k}"
        assert same_bits(PS._cat(params), fx[f"p{k}"]), f"p after step {k}"
        if master:
            assert same_bits(host(mw.buffer), fx[f"p{k}"]), f"master after step {k}"
        if hp[2] != 0:
            assert same_bits(PS._cat([state[p]["momentum_buffer"] for p in params]), fx[f"buf{k}"]), f"buf, step {k}"
    want = [0] * len(NAMES_COUNTED)
    want[1 if master else 0] = STEPS * codec.params_sgd_flatgrad_launches(len(lens))
    want[4] = STEPS * codec.params_launches(len(lens))
    assert _delta(c0) == want, "one pack and one update launch per chunk and step, nothing else"


# ----------------------------------------------------------------------------- against the existing kernels
def _layout(mode, seed, lens=(40, 8192 + 24, 7, 300, 4097)):
    lens = list(lens)
    k = len(lens)
    dts = PS._dtypes(mode, k)
    hps = [PS._varied_hp(i) for i in range(k)]
    firsts = [i % 2 == 0 and hps[i][2] != 0 for i in range(k)]
    cols = [[h[j] for h in hps] for j in range(5)]
    return lens, k, dts, hps, firsts, cols


def test_fp32_tensors_master_and_plain_kernels_agree():
    from chocosgd_amd import codec
    lens, k, dts, hps, firsts, cols = _layout("fp32", 0)
    p0 = [torch.from_numpy(PS._values(m, 50 + i, -3, 1)).to(DEV) for i, m in enumerate(lens)]
    b0 = [torch.from_numpy(PS._values(m, 250 + i, -4, 0)).to(DEV) for i, m in enumerate(lens)]
    gsum = torch.from_numpy(np.concatenate([PS._values(m, 150 + i, -4, 0) for i, m in enumerate(lens)])).to(DEV)
    out = []
    for master in (False, True):
        p, b = [t.clone() for t in p0], [t.clone() for t in b0]
        g = [torch.full_like(t, SENTINEL) for t in p0]
        m = torch.cat(p0) if master else None
        codec.params_sgd_flatgrad(p, g, [x if hps[i][2] != 0 else None for i, x in enumerate(b)], gsum, 3.0, *cols,
                                  firsts, master=m)
        if master:
            assert same_bits(host(m), PS._cat(p)), "fp32 parameters are the master's values"
        out.append((PS._cat(p), PS._cat(g), PS._cat(b)))
    for a, b in zip(*out):
        assert same_bits(a, b)


@pytest.mark.parametrize("divisor", [2.0, 3.0])
@pytest.mark.parametrize("mode", MODES)
def test_plain_kernel_is_the_four_passes_it_replaces(mode, divisor):
    """params_pack of the gradients, the sum, flat / w, the unpack into the grads and
    apply_gradient, on the same values.  The division is by a 0-dim device tensor: a true
    division (torch multiplies a device tensor by the reciprocal of a Python scalar)."""
    from chocosgd_amd import codec, utils
    lens, k, dts, hps, firsts, cols = _layout(mode, 0)
    n = sum(lens)
    mk = lambda seed, lo, hi: [torch.from_numpy(PS._values(m, seed + i, lo, hi)).to(DEV).to(dt)  # noqa: E731
                               for i, (m, dt) in enumerate(zip(lens, dts))]
    p0, g0, b0 = mk(50, -3, 1), mk(150, -4, 0), mk(250, -4, 0)
    peer = torch.from_numpy(PS._values(n, 350, -4, 0)).to(DEV)
    # the parent path
    params = [torch.nn.Parameter(t.clone()) for t in p0]
    for p, g in zip(params, g0):
        p.grad = g.clone()
    groups, names = AO.groups_of(params, hps)
    state = collections.defaultdict(dict)
    for i, p in enumerate(params):
        if hps[i][2] != 0 and not firsts[i]:
            state[p]["momentum_buffer"] = b0[i].clone()
    flat = torch.empty(n, device=DEV)
    codec.params_pack([p.grad for p in params], flat)
    flat.add_(peer)
    gsum = flat.clone()
    flat = flat / torch.full((), divisor, dtype=F32, device=DEV)
    codec.params_unpack(flat, [p.grad for p in params])
    utils.apply_gradient(groups, state)
    # the kernel
    p, g, b = [t.clone() for t in p0], [torch.full_like(t, SENTINEL) for t in p0], [t.clone() for t in b0]
    codec.params_sgd_flatgrad(p, g, [x if hps[i][2] != 0 else None for i, x in enumerate(b)], gsum, divisor, *cols,
                              firsts)
    assert same_bits(PS._cat(p), PS._cat(params)), "parameters"
    assert same_bits(PS._cat(g), PS._cat([q.grad for q in params])), "the averaged gradients"
    for i, q in enumerate(params):
        if hps[i][2] != 0:
            assert same_bits(host(b[i]), host(state[q]["momentum_buffer"])), f"momentum buffer {i}"


@pytest.mark.parametrize("divisor", [2.0, 3.0])
@pytest.mark.parametrize("mode", MODES)
def test_master_kernel_is_the_master_update_on_the_unrounded_average(mode, divisor):
    """The parent path of the master step: the same pack, sum and true division, then
    apply_gradient(master=...) of an fp32 twin of the model (parameters = the master's slices)
    fed the unrounded average as its fp32 gradients; the 16-bit parameters are
    codec.params_unpack of the master, the 16-bit gradients of the average."""
    from chocosgd_amd import codec, utils
    lens, k, dts, hps, firsts, cols = _layout(mode, 0)
    n = sum(lens)
    m0 = [torch.from_numpy(PS._values(m, 50 + i, -3, 1)).to(DEV) for i, m in enumerate(lens)]
    g0 = [torch.from_numpy(PS._values(m, 150 + i, -4, 0)).to(DEV).to(dt) for i, (m, dt) in enumerate(zip(lens, dts))]
    b0 = [torch.from_numpy(PS._values(m, 250 + i, -4, 0)).to(DEV) for i, m in enumerate(lens)]
    peer = torch.from_numpy(PS._values(n, 350, -4, 0)).to(DEV)
    flat = torch.empty(n, device=DEV)
    codec.params_pack(g0, flat)
    flat.add_(peer)
    gsum = flat.clone()
    avg = flat / torch.full((), divisor, dtype=F32, device=DEV)
    twin = [torch.nn.Parameter(t.clone()) for t in m0]
    for q, a in zip(twin, avg.split(lens)):
        q.grad = a.clone()
    groups, names = AO.groups_of(twin, hps)
    mw = utils.MasterWeights(groups, names)
    state = collections.defaultdict(dict)
    for i, q in enumerate(twin):
        if hps[i][2] != 0 and not firsts[i]:
            state[q]["momentum_buffer"] = b0[i].clone()
    utils.apply_gradient(groups, state, master=mw)
    # the kernel, on a 16-bit (or mixed) model over the same master values
    p = [torch.full((m,), SENTINEL, device=DEV, dtype=dt) for m, dt in zip(lens, dts)]
    g = [torch.full((m,), SENTINEL, device=DEV, dtype=dt) for m, dt in zip(lens, dts)]
    b = [t.clone() for t in b0]
    master = torch.cat(m0)
    codec.params_sgd_flatgrad(p, g, [x if hps[i][2] != 0 else None for i, x in enumerate(b)], gsum, divisor, *cols,
                              firsts, master=master)
    assert same_bits(host(master), host(mw.buffer)), "master"
    for i, q in enumerate(twin):
        if hps[i][2] != 0:
            assert same_bits(host(b[i]), host(state[q]["momentum_buffer"])), f"momentum buffer {i}"
    want_p = [torch.full_like(t, SENTINEL) for t in p]
    want_g = [torch.full_like(t, SENTINEL) for t in g]
    codec.params_unpack(master, want_p)
    codec.params_unpack(avg, want_g)
    assert same_bits(PS._cat(p), PS._cat(want_p)) and same_bits(PS._cat(g), PS._cat(want_g))


# ----------------------------------------------------------------------------- the step against the loop
def _device_model(mode, seed):
    lens = PS.BASE
    dts = PS._dtypes(mode, len(lens))
    params = [torch.nn.Parameter(torch.from_numpy(PS._values(m, seed + i, -3, 1)).to(DEV).to(dt))
              for i, (m, dt) in enumerate(zip(lens, dts))]
    groups, names = AO.groups_of(params, [PS._varied_hp(i) for i in range(len(lens))])
    return lens, dts, params, groups, names


@pytest.mark.parametrize("write_grads", [True, False])
@pytest.mark.parametrize("master", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_step_equals_the_loop(mode, master, write_grads):
    """utils.allreduce_sgd_step (one pack and one update launch per chunk) and
    utils.allreduce_sgd_step_loop (torch ops) from the same state on the same gradients, world 3,
    three steps: parameters, gradients, buffers and the master copy; the launches."""
    from chocosgd_amd import codec, utils
    runs = []
    for fn in (utils.allreduce_sgd_step, utils.allreduce_sgd_step_loop):
        lens, dts, params, groups, names = _device_model(mode, 400)
        n = sum(lens)
        mw = utils.MasterWeights(groups, names) if master else None
        state = collections.defaultdict(dict)
        rec = []
        for step in range(STEPS):
            peers = [PS._values(n, 900 + 10 * step + r, -4, 0) for r in range(2)]
            own = []
            for i, p in enumerate(params):
                p.grad = torch.from_numpy(PS._values(lens[i], 600 + 100 * step + i, -4, 0)).to(DEV).to(p.dtype)
                own.append(host(p.grad))
            agg = AO.Loopback(3, peers=[peers])
            c0 = _counts()
            assert fn(groups, names, state, agg, write_grads=write_grads, master=mw) == 32 * n
            d = _delta(c0)
            if fn is utils.allreduce_sgd_step:
                want = [0] * len(NAMES_COUNTED)
                want[1 if master else 0] = codec.params_sgd_flatgrad_launches(len(lens))
                want[4] = codec.params_launches(len(lens))
                assert d == want
            else:
                assert d[0] == 0 and d[1] == 0, "the loop launched the new kernels"
            if not write_grads:
                assert same_bits(PS._cat([p.grad for p in params]), np.concatenate(own)), "p.grad was written"
            rec.append({"p": PS._cat(params), "g": PS._cat([p.grad for p in params]),
                        "buf": PS._cat([state[p]["momentum_buffer"] for p in params if "momentum_buffer" in state[p]]),
                        "m": host(mw.buffer) if master else np.zeros(0, np.float32)})
        runs.append(rec)
    for step, (a, b) in enumerate(zip(*runs)):
        for key in a:
            assert same_bits(a[key], b[key]), (step, key)
    assert not same_bits(runs[0][0]["p"], runs[0][1]["p"]), "the parameters did not move"


@pytest.mark.parametrize("name", ["bf16", "fp16"])
def test_lost_updates(name):
    """64 steps of lr * avg = 2^-12 (bf16; fp16: 2^-14) on parameters at 1.0, world 2: with
    master weights the master is exactly 1 - j * 2^-12 after step j; the 16-bit step leaves the
    parameter at 1.0."""
    c0 = _counts()
    AO.check_lost_updates(name, DEV, same_bits)
    d = _delta(c0)
    assert d[0] == MA.LOST_STEPS and d[1] == MA.LOST_STEPS and d[2] == 0 and d[3] == 0, "both ran their kernels"


def test_python_refusals_change_nothing():
    from chocosgd_amd import codec, utils
    lens = [40, 300, 7]
    params = [torch.nn.Parameter(torch.from_numpy(PS._values(m, i, -3, 1)).to(DEV).to(torch.bfloat16))
              for i, m in enumerate(lens)]
    for p in params:
        p.grad = torch.ones_like(p)
    groups, names = AO.groups_of(params, (0.1, 0.0, 0.9, 0.0, False))
    mw = utils.MasterWeights(groups, names)
    state = collections.defaultdict(dict)
    foreign, small = utils.MasterWeights(groups, names[::-1]), utils.MasterWeights(groups[:2], names[:2])
    agg = AO.Loopback(3, peers=[[np.zeros(sum(lens), np.float32)]] * 8)
    snap = [mw.buffer.clone()] + [p.detach().clone() for p in params] + [p.grad.clone() for p in params]
    c0 = _counts()
    state[params[1]]["momentum_buffer"] = torch.zeros_like(params[1])  # a 16-bit buffer of the 16-bit step
    with pytest.raises(RuntimeError, match="float32 momentum buffers"):
        utils.allreduce_sgd_step(groups, names, state, agg, master=mw)
    del state[params[1]]["momentum_buffer"]
    with pytest.raises(RuntimeError, match="param_names"):
        utils.allreduce_sgd_step(groups, names, state, agg, master=foreign)
    with pytest.raises(RuntimeError):  # a master of another size
        utils.allreduce_sgd_step(groups, names, state, agg, master=small)
    kept, params[2].grad = params[2].grad, None
    with pytest.raises(RuntimeError, match="no gradient"):
        utils.allreduce_sgd_step(groups, names, state, agg)
    params[2].grad = kept
    # the codec's own entry points
    plan = codec.ParamSgdPlan([p.data for p in params])
    data, grads = [p.data for p in params], [p.grad for p in params]
    gsum = torch.zeros(sum(lens), device=DEV)
    with pytest.raises(RuntimeError):  # a 16-bit momentum buffer in the master call
        codec.params_sgd_flatgrad(data, grads, [torch.zeros_like(p) for p in params], gsum, 3.0, 0.1, momentum=0.9,
                                  master=mw.buffer)
    with pytest.raises(RuntimeError):  # a tensor without a gradient
        codec.params_sgd_flatgrad(data, [grads[0], None, grads[2]], None, gsum, 3.0, 0.1)
    for bad in (0.0, float("inf"), float("nan"), 1e-60):
        with pytest.raises(RuntimeError):
            codec.params_sgd_flatgrad(data, grads, None, gsum, bad, 0.1)
    with pytest.raises(RuntimeError):  # gsum of the wrong size
        plan.run_flatgrad(torch.zeros(sum(lens) + 1, device=DEV), 3.0)
    with pytest.raises(RuntimeError):  # gsum on the host
        plan.run_flatgrad(torch.zeros(sum(lens)), 3.0)
    with pytest.raises(RuntimeError):  # master of the wrong size
        plan.run_flatgrad(gsum, 3.0, master=torch.zeros(sum(lens) + 1, device=DEV))
    with pytest.raises(RuntimeError):  # a flat buffer of the wrong size for the pack
        plan.pack_grads(torch.zeros(sum(lens) + 1, device=DEV))
    assert _delta(c0) == [0] * len(NAMES_COUNTED), "a refused call launched something"
    assert agg.calls == 0
    now = [mw.buffer] + [p.detach() for p in params] + [p.grad for p in params]
    assert all(same_bits(host(a), host(b)) for a, b in zip(snap, now))
    assert all("momentum_buffer" not in state[p] for p in params)


# ----------------------------------------------------------------------------- across processes
@pytest.mark.parametrize("mode,world", [("fp32", 2), ("fp32", 3), ("bf16", 2), ("bf16_master", 2), ("bf16_master", 3),
                                        ("fp16_master", 3)])
def test_allreduce_step_across_processes(mode, world, tmp_path):
    """utils.allreduce_sgd_step on `world` ranks sharing the one GPU, the all-reduce over gloo
    with host staging (tests/_mp_allreduce_worker.py, a fresh interpreter).  World 2: the sum is
    order-free; world 3: the gradients are multiples of 2^-10 in [-4, 4], so every partial sum is
    exact in any order.  Every rank's parameters, buffers, grads and master copy against the
    model, and against each other."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_mp_allreduce_worker.py"), mode, str(world),
                        str(tmp_path)], capture_output=True, text=True, timeout=W.TIMEOUT * (W.STEPS + 3))
    assert r.returncode == 0, r.stderr[-4000:]
    got = [dict(np.load(tmp_path / f"rank{q}.npz")) for q in range(world)]
    dtype, master = mode.split("_")[0], mode.endswith("_master")
    cur = [SO.to_grid(v, dtype) for v in W.params0()]
    bufs = [None] * len(W.LENS)
    for step in range(W.STEPS):
        own = [[SO.to_grid(g, dtype) for g in W.grads_of(q, step)] for q in range(world)]
        want_p, want_g, want_b = [], [], []
        for i in range(len(W.LENS)):
            s = own[0][i]
            for q in range(1, world):
                s = (s + own[q][i]).astype(np.float32)
            assert np.all(np.abs(s) <= 4.0 * world) and np.all(s * 1024 == np.round(s * 1024)), "exact sums"
            hp = W.HP[i % 3]
            if master:
                cur[i], bufs[i], p16, g16 = AO.master_step(cur[i], s, bufs[i], float(world), *hp, first=step == 0,
                                                           dtype=dtype)
            else:
                cur[i], bufs[i], g16 = AO.step(cur[i], s, bufs[i], float(world), *hp, first=step == 0, dtype=dtype)
                p16 = cur[i]
            want_p.append(p16), want_g.append(g16)
            if bufs[i] is not None:
                want_b.append(bufs[i])
        for q in range(world):
            assert same_bits(got[q][f"p{step}"], np.concatenate(want_p)), (q, step)
            assert same_bits(got[q][f"g{step}"], np.concatenate(want_g)), (q, step)
            assert same_bits(got[q][f"buf{step}"], np.concatenate(want_b)), (q, step)
            if master:
                assert same_bits(got[q][f"m{step}"], np.concatenate(cur)), (q, step)
            for key in got[0]:
                assert same_bits(got[q][key], got[0][key]), (q, key)

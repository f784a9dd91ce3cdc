"""The neighbour-weighted model mix, host side (no GPU): the numpy model (tests/_mix_oracle.py)
and the per-op torch paths of dcd.fused_step / ecd.fused_step / utils.dpsgd_step against the
reference's fixtures (tests/golden/mix_*.npz, gen_golden_mix.py), bit for bit; the launch count
rule; the argument checks of choco_params_mix, made before any HIP call."""
import collections
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden, same_bits
import _mix_oracle as MO
import _sgd_oracle as SO

CAP, SRC_CAP = 128, 8  # tensors and sources per launch (mix.hip kMixCap, kMixSrc)
ERR_INVALID = -1  # CHOCO_ERR_INVALID
F32, BF16, F16 = 0, 1, 2
GRAD_SUB, GRAD_FMA, WRITE_PARAMS, EXTRAPOLATE = 1, 2, 4, 8
SETS = ["ring3", "five", "one"]
LOCAL_INDEX = [1, 5]


@pytest.fixture(scope="module")
def lib():
    from chocosgd_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def inputs():
    return golden("mix_inputs")


def _neighbourhood(fx):
    ranks = fx["ranks"].tolist()
    return int(fx["rank"]), dict(zip(ranks, fx["weights"].tolist()))


def _d_p(inputs):
    """d_p of the fixtures' one apply_gradient step, and the params it leaves in apply mode."""
    lr, wd, mom, damp, nest = inputs["hp"].tolist()
    p_new, _, d = SO.sgd_step(inputs["p0"], inputs["g"], None, lr, wd, mom, damp, bool(nest), first=True)
    return lr, d, p_new


# ----------------------------------------------------------------------------- the numpy model
@pytest.mark.parametrize("name", SETS)
def test_oracle_matches_the_reference_fixtures(inputs, name):
    fx = golden(f"mix_{name}")
    rank, info = _neighbourhood(fx)
    lr, d, p_sgd = _d_p(inputs)
    hats = [inputs["hats"][r] for r in info]
    w = list(info.values())
    m, _, out = MO.mix(hats, w, g=d, lr=lr, grad="sub")
    assert same_bits(out, fx["dcd_half"]) and same_bits(m, out)
    assert same_bits(inputs["p0"], fx["dcd_packed"])
    for t in LOCAL_INDEX:
        _, p_new, out = MO.mix(hats, w, g=d, lr=lr, grad="fma", x=inputs["p0"], ext=(1 - 0.5 * t, 0.5 * t))
        assert same_bits(p_new, fx[f"ecd{t}_params"]), t
        assert same_bits(out, fx[f"ecd{t}_extrap"]), t
    assert same_bits(p_sgd, fx["dpsgd_sent"])
    # the reference's local_data holds the neighbours first and this rank's own buffer last
    order = [r for r in info if r != rank] + [rank]
    srcs = [p_sgd if r == rank else inputs["hats"][r] for r in order]
    _, p_new, _ = MO.mix(srcs, [info[r] for r in order])
    assert same_bits(p_new, fx["dpsgd_agg"])


def test_fixtures_hold_the_planted_values(inputs):
    o = int(np.cumsum(inputs["lens"])[2])
    five, ring = golden("mix_five"), golden("mix_ring3")
    span = slice(o, o + 8195)
    for fx in (five, ring):
        for key in ("dcd_half", "ecd1_params", "dpsgd_agg"):
            zeros = fx[key][span][np.all(inputs["hats"][:, span] == 0, axis=0) & (inputs["g"][span] == 0)]
            assert zeros.size >= 1 and np.all(zeros.view(np.uint32) == 0), "0 + (-0 * w) is +0"
    inf_at = int(np.flatnonzero(np.isinf(inputs["hats"][1]))[0])
    assert np.isnan(five["dcd_half"][inf_at]) and np.isinf(ring["dcd_half"][inf_at])
    assert np.isnan(inputs["g"]).sum() == 1
    sub = np.float32(2.0e-38) * np.float32(1.0 / 3)
    assert 0 < sub < np.finfo(np.float32).tiny and (inputs["hats"][0] == np.float32(2.0e-38)).any()


# ----------------------------------------------------------------------------- the torch paths
def _cpu_model(inputs, dtype=torch.float32):
    lr, wd, mom, damp, nest = inputs["hp"].tolist()
    lens = inputs["lens"].tolist()
    params, o = [], 0
    for m in lens:
        p = torch.nn.Parameter(torch.from_numpy(inputs["p0"][o:o + m].copy()).to(dtype))
        p.grad = torch.from_numpy(inputs["g"][o:o + m].copy()).to(dtype)
        params.append(p)
        o += m
    groups = [{"params": [p], "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": damp, "nesterov": bool(nest),
               "name": f"p{i}"} for i, p in enumerate(params)]
    names = list(enumerate(g["name"] for g in groups))
    shapes = [(p.size(), p.nelement()) for p in params]
    return params, groups, names, shapes, lens


def _cpu_replicas(inputs, info, lens):
    from chocosgd_amd.tensor_buffer import TensorBuffer
    sizes = [(m,) for m in lens]
    return {r: TensorBuffer.from_flat(torch.from_numpy(inputs["hats"][r].copy()), sizes) for r in info}


def _cat(tensors):
    return np.concatenate([t.detach().float().numpy().reshape(-1) for t in tensors])


@pytest.mark.parametrize("name", SETS)
def test_cpu_dcd_step_matches_the_reference_fixtures(inputs, name):
    from chocosgd_amd import dcd
    fx = golden(f"mix_{name}")
    rank, info = _neighbourhood(fx)
    params, groups, names, shapes, lens = _cpu_model(inputs)
    hats = _cpu_replicas(inputs, info, lens)
    comp = MO.RecordingCompressor(rank)
    bits = dcd.fused_step(comp, groups, names, collections.defaultdict(dict), shapes, hats, info)
    assert bits == 17
    assert same_bits(comp.seen["flatten_half_params"].numpy(), fx["dcd_half"])
    assert same_bits(comp.seen["flatten_params"].numpy(), fx["dcd_packed"])
    assert same_bits(_cat(params), inputs["hats"][rank]), "the model is this rank's own replica"


@pytest.mark.parametrize("t", LOCAL_INDEX)
@pytest.mark.parametrize("name", SETS)
def test_cpu_ecd_step_matches_the_reference_fixtures(inputs, name, t):
    from chocosgd_amd import ecd
    fx = golden(f"mix_{name}")
    rank, info = _neighbourhood(fx)
    params, groups, names, shapes, lens = _cpu_model(inputs)
    hats = _cpu_replicas(inputs, info, lens)
    comp = MO.RecordingCompressor(rank)
    assert ecd.fused_step(comp, groups, names, collections.defaultdict(dict), shapes, hats, info, t) == 17
    assert same_bits(_cat(params), fx[f"ecd{t}_params"])
    assert same_bits(comp.seen["flatten_updated_params"].numpy(), fx[f"ecd{t}_extrap"])
    for r in info:
        assert same_bits(hats[r].buffer.numpy(), inputs["hats"][r])


@pytest.mark.parametrize("name", SETS)
def test_cpu_dpsgd_step_matches_the_reference_fixtures(inputs, name):
    from chocosgd_amd import utils
    fx = golden(f"mix_{name}")
    rank, info = _neighbourhood(fx)
    params, groups, names, _, lens = _cpu_model(inputs)
    received = {r: torch.from_numpy(inputs["hats"][r].copy()) for r in info if r != rank}
    agg = MO.prepared_aggregator(rank, info, received)
    bits = utils.dpsgd_step(groups, names, collections.defaultdict(dict), agg, info)
    assert bits == 32 * sum(lens)
    assert same_bits(_cat(params), fx["dpsgd_agg"])


def test_steps_refuse_a_parameter_without_a_gradient(inputs):
    from chocosgd_amd import dcd, ecd
    fx = golden("mix_one")
    rank, info = _neighbourhood(fx)
    params, groups, names, shapes, lens = _cpu_model(inputs)
    hats = _cpu_replicas(inputs, info, lens)
    params[4].grad = None
    before = _cat(params)
    comp = MO.RecordingCompressor(rank)
    state = collections.defaultdict(dict)
    with pytest.raises(RuntimeError, match="no gradient"):
        dcd.fused_step(comp, groups, names, state, shapes, hats, info)
    with pytest.raises(RuntimeError, match="no gradient"):
        ecd.fused_step(comp, groups, names, state, shapes, hats, info, 3)
    assert comp.seen is None and not state and same_bits(_cat(params), before)


def test_weighted_aggregate_on_cpu_is_the_expression():
    rng = np.random.RandomState(3)
    info = {0: 0.5, 1: 0.3, 2: 0.2}
    data = {r: torch.from_numpy(rng.standard_normal((7, 3)).astype(np.float32)) for r in info}
    agg = MO.prepared_aggregator(1, info, data)
    got = agg._agg(data[1], op="weighted")
    want = sum(t * info[r] for r, t in [(0, data[0]), (2, data[2]), (1, data[1])])
    assert got.shape == (7, 3) and torch.equal(got, want)


# ----------------------------------------------------------------------------- the C ABI
def test_launches_rule(lib):
    from chocosgd_amd import codec
    for nseg in [1, CAP - 1, CAP, CAP + 1, 300, 3000]:
        for nsrc in [1, 3, SRC_CAP, SRC_CAP + 1, 17, 64]:
            want = -(-nseg // CAP) + (nsrc - 1) // SRC_CAP
            assert lib.choco_params_mix_launches(nseg, nsrc) == want, (nseg, nsrc)
            assert codec.params_mix_launches(nseg, nsrc) == want
    assert lib.choco_params_mix_launches(161, 3) == 2  # ResNet-50 on a ring
    for bad in [(0, 3), (-1, 3), (5, 0), (5, 65), (5, -2)]:
        assert lib.choco_params_mix_launches(*bad) == 0, bad


def _call(lib, srcs=(0x10000, 0x20000, 0x30000), w=None, nsrc=None, p=(0x1000, 0x1100), g=(0x2000, 0x2100),
          lens=(4, 4), dts=(F32, BF16), nseg=None, n=8, lr=0.1, mode=GRAD_SUB, flat=0x40000, x_out=0x50000, null=(),
          msg=None):
    """One call with host tables built from the lists; the made-up device pointers are never
    dereferenced (every case here is rejected before the first launch)."""
    arr = lambda ct, vals: (ct * max(len(vals), 1))(*vals)  # noqa: E731
    tabs = {"srcs": arr(ctypes.c_void_p, srcs), "weights": arr(ctypes.c_double, w or [1.0 / len(srcs)] * len(srcs)),
            "params": arr(ctypes.c_void_p, p), "grads": arr(ctypes.c_void_p, g), "lens": arr(ctypes.c_int64, lens),
            "dtypes": arr(ctypes.c_int32, dts)}
    t = {nm: (None if nm in null else tab) for nm, tab in tabs.items()}
    return lib.choco_params_mix(t["srcs"], t["weights"], len(srcs) if nsrc is None else nsrc, t["params"], t["grads"],
                                t["lens"], t["dtypes"], len(lens) if nseg is None else nseg, lr, 0.5, 0.5, mode,
                                ctypes.c_void_p(flat), ctypes.c_void_p(x_out), n, None)


NINE = tuple(0x10000 * (r + 1) for r in range(9))
BAD = {
    **{f"null {t}": dict(null=(t,), msg="null table") for t in ["srcs", "weights", "lens", "dtypes"]},
    "null grads with GRAD_SUB": dict(null=("grads",), msg="grads table"),
    "null grads with GRAD_FMA": dict(null=("grads",), mode=GRAD_FMA | WRITE_PARAMS, msg="grads table"),
    "null params with x_out": dict(null=("params",), msg="params table"),
    "null params with WRITE_PARAMS": dict(null=("params",), x_out=0, mode=WRITE_PARAMS, msg="params table"),
    "null params with EXTRAPOLATE": dict(null=("params",), x_out=0, mode=EXTRAPOLATE, msg="params table"),
    "nsrc zero": dict(nsrc=0, msg="nsrc"),
    "nsrc negative": dict(nsrc=-1, msg="nsrc"),
    "nsrc 65": dict(srcs=tuple(0x10000 * (r + 1) for r in range(65)), msg="nsrc"),
    "null source": dict(srcs=(0x10000, 0, 0x30000), msg="source 1"),
    "source at 2 mod 4": dict(srcs=(0x10000, 0x20002), msg="source 1"),
    "nseg zero": dict(nseg=0, msg="nseg"),
    "negative length": dict(lens=(-4, 12), msg="negative length"),
    "sum below n": dict(n=9, msg="add up"),
    "sum above n": dict(n=7, msg="add up"),
    "n = 2^31": dict(lens=(2 ** 31,), p=(0x1000,), g=(0x2000,), dts=(F32,), n=2 ** 31, msg="2^31"),
    "dtype 3": dict(dts=(F32, 3), msg="dtype"),
    "dtype -1": dict(dts=(-1, F32), msg="dtype"),
    "unknown mode bit": dict(mode=16 | GRAD_SUB, msg="mode"),
    "both GRAD bits": dict(mode=GRAD_SUB | GRAD_FMA, msg="one of them"),
    "null grad": dict(g=(0x2000, 0), msg="null grad"),
    "null param with EXTRAPOLATE": dict(p=(0, 0x1100), x_out=0, mode=EXTRAPOLATE, msg="null param"),
    "null param with x_out": dict(p=(0x1000, 0), mode=0, msg="null param"),
    "null param with WRITE_PARAMS": dict(p=(0x1000, 0), x_out=0, mode=WRITE_PARAMS, msg="null param"),
    "nothing to write": dict(flat=0, x_out=0, mode=GRAD_SUB, msg="nothing to write"),
    "EXTRAPOLATE without flat_out": dict(flat=0, mode=EXTRAPOLATE | WRITE_PARAMS, msg="EXTRAPOLATE"),
    "nine sources without flat_out": dict(srcs=NINE, flat=0, msg="running sum"),
    "fp32 param at 2 mod 4": dict(p=(0x1002, 0x1100), msg="aligned"),
    "bf16 param at odd byte": dict(p=(0x1000, 0x1101), msg="aligned"),
    "fp32 grad at 2 mod 4": dict(g=(0x2002, 0x2100), msg="aligned"),
    "fp16 grad at odd byte": dict(dts=(F32, F16), g=(0x2000, 0x2101), msg="aligned"),
    "flat_out at 2 mod 4": dict(flat=0x40002, msg="4-byte"),
    "x_out at 2 mod 4": dict(x_out=0x50002, msg="4-byte"),
    "lr inf with GRAD_SUB": dict(lr=float("inf"), msg="finite"),
    "lr nan with GRAD_FMA": dict(lr=float("nan"), mode=GRAD_FMA, msg="finite"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib, codec
    before = codec.launch_count("param_mix_kernel")
    assert _call(lib, **BAD[case]) == ERR_INVALID, case
    err = _lib.last_error()
    assert err != "" and BAD[case]["msg"] in err, (case, err)
    assert codec.launch_count("param_mix_kernel") == before


def test_python_wrapper_refuses_cpu_tensors():
    from chocosgd_amd import codec
    with pytest.raises(RuntimeError, match="ROCm device tensors only"):
        codec.params_mix([torch.zeros(8)], [1.0], flat_out=torch.zeros(8))

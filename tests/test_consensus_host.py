"""Consensus evaluation on the host: the numpy model (tests/_consensus_oracle.py) against the
reference's recorded agg_model / get_model_difference (tests/golden/consensus_*.npz), the
package's torch paths on CPU tensors against both, the argument checks of
choco_params_consensus (every case is rejected before the first launch: no GPU is touched) and
the launch / workspace arithmetic."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden, same_bits
import _allreduce_oracle as AO
import _consensus_oracle as CO
import _sgd_oracle as SO

ERR_INVALID = -1
F32, BF16, F16 = 0, 1, 2
DIST, WRITE_AVG = 1, 2
CAP, TILE = 128, 8192
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
MODES = ["fp32", "bf16", "fp16", "mixed"]
SETS = ["ordinary", "special"]
KERNELS = ("param_consensus_kernel", "param_consensus_total_kernel")


@pytest.fixture(scope="module")
def lib():
    from chocosgd_amd import _lib
    return _lib.load()


def host(t):
    return t.detach().float().cpu().numpy()


def _names(mode, k):
    return [mode if mode != "mixed" else list(DTYPES)[i % 3] for i in range(k)]


def _split(flat, lens, names=None):
    out, o = [], 0
    for i, m in enumerate(lens):
        t = torch.from_numpy(np.ascontiguousarray(flat[o:o + m], dtype=np.float32).copy())
        out.append(t if names is None else t.to(DTYPES[names[i]]))
        o += m
    return out


def _cat(tensors):
    return np.concatenate([host(t).reshape(-1) for t in tensors] + [np.zeros(0, np.float32)])


class Model(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(t) for t in tensors])


def _check_distance(got, fx, model_out0):
    """The issue's three distance checks on the ordinary set; on the special set non-finite
    exactly where the model's is."""
    if "ref_rel_gap" not in fx:
        assert np.isfinite(got) == np.isfinite(model_out0) and not np.isfinite(float(fx["distance"]))
        return
    assert CO.adjacent(got, np.float32(fx["distance64"])), (got, float(fx["distance64"]))
    assert abs(float(fx["distance"]) - float(got)) <= float(fx["ref_rel_gap"]) * float(got) + CO.ulp32(got)
    assert np.float32(got).view(np.uint32) == np.float32(model_out0).view(np.uint32)


# ----------------------------------------------------------------------------- the model against the reference
def test_the_fixtures_hold_what_the_issue_asks_for():
    o, s = golden("consensus_ordinary"), golden("consensus_special")
    assert o["lens"].tolist() == golden("sgd_inputs")["lens"].tolist() == s["lens"].tolist()
    assert float(o["world"]) == 3.0 and np.isfinite(o["avg"]).all() and np.isfinite(float(o["distance"]))
    assert 0 < float(o["ref_rel_gap"]) <= o["x0"].size * 2.0 ** -24
    sm, av = s["sum"], s["avg"]
    with np.errstate(all="ignore"):
        assert np.isnan(sm).sum() >= 4 and np.isinf(sm).sum() >= 4
        sub = np.isfinite(sm) & (sm != 0) & (np.abs(sm) < np.float32(1.17549435e-38))
        assert sub.sum() >= 3
        third_sub = (np.abs(sm) >= np.float32(1.17549435e-38)) & np.isfinite(sm) & (av != 0) & (
            np.abs(av) < np.float32(1.17549435e-38))
        assert third_sub.sum() >= 1
        assert ((sm == 0) & np.signbit(sm)).sum() >= 1 and ((sm == 0) & ~np.signbit(sm)).sum() >= 1
        recip = (sm * np.float32(1.0 / 3.0)).astype(np.float32)
        assert (np.isfinite(av) & (recip.view(np.uint32) != av.view(np.uint32))).sum() > 1000
    assert not np.isfinite(float(s["distance"]))


@pytest.mark.parametrize("name", SETS)
def test_the_model_against_the_fixtures(name):
    fx = golden(f"consensus_{name}")
    lens = fx["lens"].tolist()
    with np.errstate(all="ignore"):
        assert same_bits((fx["x0"] + fx["x1"]) + fx["x2"], fx["sum"]), "peer 1 then peer 2"
    avg, out, dists = CO.consensus(fx["x0"], fx["sum"], float(fx["world"]), lens, ["fp32"] * len(lens))
    assert same_bits(avg, fx["avg"])
    _check_distance(out[0], fx, out[0])
    # per tensor, against the fp64 value from the recorded avg - x
    with np.errstate(all="ignore"):
        d = (fx["avg"] - fx["x0"]).astype(np.float32).astype(np.float64)
        o = 0
        for s, m in enumerate(lens):
            want = np.float32(np.sqrt(np.sum(d[o:o + m] ** 2)))
            assert np.isfinite(want) == np.isfinite(dists[s])
            assert not np.isfinite(want) or CO.adjacent(want, dists[s]), s
            o += m
        assert dists[2] == 0 and lens[2] == 0, "a zero-length tensor contributes 0"
        norm = np.float32(np.sqrt(np.sum(fx["avg"].astype(np.float64) ** 2)))
    assert np.isfinite(norm) == np.isfinite(out[1]) and (not np.isfinite(norm) or CO.adjacent(norm, out[1]))


def test_the_summation_order_of_the_model():
    """Spans of one wave and of the workgroup, and a tensor over three tiles: the ordered sum is
    the plain fp64 sum up to its rounding, and exactly it where every partial sum is exact."""
    lens = [5, 1024, 1025, 0, 3 * TILE + 5, 70]
    n = sum(lens)
    ints = np.arange(n, dtype=np.float32) % 7 - 3  # integer squares: every order gives the exact sum
    got = CO.ordered_sums(ints, lens)
    o = 0
    for s, m in enumerate(lens):
        assert got[s] == np.sum(ints[o:o + m].astype(np.float64) ** 2), s
        o += m
    v = np.random.RandomState(5).standard_normal(n).astype(np.float32)
    got, o = CO.ordered_sums(v, lens), 0
    for s, m in enumerate(lens):
        want = np.sum(v[o:o + m].astype(np.float64) ** 2)
        assert abs(got[s] - want) <= 1e-12 * want, s
        o += m


# ----------------------------------------------------------------------------- the torch paths on CPU tensors
class FakeAgg:
    """world 3; _agg(op="sum") adds the recorded peers in place, peer 1 then peer 2."""

    def __init__(self, fx, world=None):
        self.world_size = float(fx["world"]) if world is None else world
        self.x1, self.x2 = torch.from_numpy(fx["x1"].copy()), torch.from_numpy(fx["x2"].copy())
        self.calls = 0

    def _agg(self, data, op=None, distributed=True):
        assert op == "sum", op
        if not distributed:
            return data
        self.calls += 1
        assert data.dtype == torch.float32 and data.numel() == self.x1.numel()
        return data.add_(self.x1).add_(self.x2)


def _centralized(fx):
    from chocosgd_amd.communication import CentralizedAggregation

    class Recorded(CentralizedAggregation):
        _agg = FakeAgg._agg

    agg = object.__new__(Recorded)
    agg.rank, agg.group, agg.world_size = 0, None, float(fx["world"])
    agg.x1, agg.x2, agg.calls = torch.from_numpy(fx["x1"].copy()), torch.from_numpy(fx["x2"].copy()), 0
    return agg


@pytest.mark.parametrize("how", ["list", "module", "in place"])
@pytest.mark.parametrize("name", SETS)
def test_fixture_replay_on_cpu_tensors(name, how):
    from chocosgd_amd import auxiliary
    fx = golden(f"consensus_{name}")
    lens = fx["lens"].tolist()
    _, mout, mdists = CO.consensus(fx["x0"], fx["sum"], 3.0, lens, ["fp32"] * len(lens))
    model, copy = Model(_split(fx["x0"], lens)), Model(_split(np.zeros_like(fx["x0"]), lens))
    agg = FakeAgg(fx)
    if how == "list":
        stats, dists = auxiliary.consensus_eval([p.data for p in model.parameters()], agg,
                                                avg_out=[p.data for p in copy.parameters()], per_tensor=True)
    elif how == "module":
        stats, dists = auxiliary.consensus_eval(model, agg, avg_out=copy, per_tensor=True)
    else:
        stats, dists = auxiliary.consensus_eval_loop(model, agg, avg_out=model, per_tensor=True)
        copy = model
    assert agg.calls == 1, "ONE collective"
    assert same_bits(_cat(copy.parameters()), fx["avg"])
    if how != "in place":
        assert same_bits(_cat(model.parameters()), fx["x0"]), "the model itself is untouched"
    assert stats.dtype == torch.float32 and stats.shape == (2,) and dists.shape == (len(lens),)
    _check_distance(host(stats)[0], fx, mout[0])
    assert same_bits(host(stats), mout) and same_bits(host(dists), mdists)
    s2, d2 = auxiliary.consensus_eval(Model(_split(fx["x0"], lens)), FakeAgg(fx))
    assert d2 is None and same_bits(host(s2), mout), "no avg_out, no per-tensor distances"


@pytest.mark.parametrize("name", SETS)
def test_get_model_difference_on_cpu_tensors(name):
    from chocosgd_amd import auxiliary
    fx = golden(f"consensus_{name}")
    lens = fx["lens"].tolist()
    model, copy = Model(_split(fx["x0"], lens)), Model(_split(fx["avg"], lens))
    got = auxiliary.get_model_difference(model, copy)
    assert isinstance(got, float)
    _, mout, _ = CO.consensus(fx["x0"], fx["avg"], 1.0, lens, ["fp32"] * len(lens))
    _check_distance(np.float32(got), fx, mout[0])
    assert auxiliary.get_model_difference(model, model) == 0.0 or name == "special"
    with pytest.raises(RuntimeError, match="match in size"):
        auxiliary.get_model_difference(model, Model(_split(fx["avg"][:-1], lens[:-1] + [lens[-1] - 1])))


@pytest.mark.parametrize("what", ["model", "grad"])
@pytest.mark.parametrize("op", ["avg", "sum"])
@pytest.mark.parametrize("name", SETS)
def test_agg_model_and_agg_grad_on_cpu_tensors(name, op, what):
    fx = golden(f"consensus_{name}")
    lens = fx["lens"].tolist()
    agg = _centralized(fx)
    if what == "model":
        model = Model(_split(fx["x0"], lens))
        before = [p.data for p in model.parameters()]
        agg.agg_model(model, op)
        got = list(model.parameters())
    else:
        model = Model(_split(np.ones_like(fx["x0"]), lens))
        for p, g in zip(model.parameters(), _split(fx["x0"], lens)):
            p.grad = g
        before = [p.grad for p in model.parameters()]
        agg.agg_grad(model, op)
        got = [p.grad for p in model.parameters()]
        assert same_bits(_cat(model.parameters()), np.ones_like(fx["x0"]))
    assert agg.calls == 1, "ONE collective"
    assert same_bits(_cat(got), fx["avg"] if op == "avg" else fx["sum"])
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(before, got)), "written in place, not rebound"


def test_agg_model_refuses_other_ops_and_missing_gradients():
    fx = golden("consensus_ordinary")
    lens = fx["lens"].tolist()
    agg, model = _centralized(fx), Model(_split(fx["x0"], lens))
    for op in ("min", "max", None):
        with pytest.raises(NotImplementedError):
            agg.agg_model(model, op)
        with pytest.raises(NotImplementedError):
            agg.agg_grad(model, op)
    with pytest.raises(AttributeError):
        agg.agg_grad(model, "avg")  # no parameter has a gradient
    assert agg.calls == 0 and same_bits(_cat(model.parameters()), fx["x0"])


@pytest.mark.parametrize("use_master", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SETS)
def test_cpu_paths_match_the_model_in_every_dtype(name, mode, use_master):
    """bf16 / fp16 / mixed models: the sum is taken on the widened values, the distance against
    the unrounded fp32 average (or from the master copy), the averaged model narrowed once."""
    from chocosgd_amd import auxiliary
    fx = golden(f"consensus_{name}")
    lens = fx["lens"].tolist()
    names = _names(mode, len(lens))
    params = _split(fx["x0"], lens, names)
    x = _cat(params)
    master = fx["x0"] if use_master else None
    src = master if use_master else x
    with np.errstate(all="ignore"):
        xsum = ((src + fx["x1"]) + fx["x2"]).astype(np.float32)
    avg, mout, mdists = CO.consensus(src, xsum, 3.0, lens, names)
    copy = [torch.zeros_like(p) for p in params]
    mt = None if master is None else torch.from_numpy(master.copy())
    stats, dists = auxiliary.consensus_eval(params, FakeAgg(fx), avg_out=copy, master=mt, per_tensor=True)
    assert same_bits(_cat(copy), avg) and same_bits(_cat(params), x)
    assert same_bits(host(stats), mout) and same_bits(host(dists), mdists)
    if use_master:
        assert same_bits(host(mt), master), "the master copy is read only"
        return
    model = Model([p.clone() for p in params])
    agg = _centralized(fx)
    agg.agg_model(model, "avg")
    assert same_bits(_cat(model.parameters()), avg) and agg.calls == 1
    assert [p.dtype for p in model.parameters()] == [DTYPES[nm] for nm in names]
    # the difference of two 16-bit models is the fp32 difference of the widened values
    got = auxiliary.get_model_difference(params, copy)
    _, dout, _ = CO.consensus(x, avg, 1.0, lens, names)
    assert np.float32(got).view(np.uint32) == dout[0].view(np.uint32) or (np.isnan(got) and np.isnan(dout[0]))


def test_not_distributed_divides_by_one():
    from chocosgd_amd import auxiliary
    fx = golden("consensus_ordinary")
    lens = fx["lens"].tolist()
    params = _split(fx["x0"], lens)
    copy = [torch.zeros_like(p) for p in params]
    stats, _ = auxiliary.consensus_eval(params, FakeAgg(fx), avg_out=copy, distributed=False)
    assert same_bits(_cat(copy), fx["x0"]) and host(stats)[0] == 0.0
    assert CO.adjacent(host(stats)[1], np.float32(np.sqrt(np.sum(fx["x0"].astype(np.float64) ** 2))))


def test_other_dtypes_go_per_tensor_through_agg():
    from chocosgd_amd.communication import CentralizedAggregation

    class Doubling(CentralizedAggregation):
        def _agg(self, data, op=None, distributed=True, **kw):
            if op not in ("avg", "sum"):
                raise NotImplementedError
            return data * 2 / (self.world_size if op == "avg" else 1)

    agg = object.__new__(Doubling)
    agg.rank, agg.group, agg.world_size = 0, None, 2.0
    model = Model([torch.arange(4, dtype=torch.float64), torch.ones(3)])
    agg.agg_model(model, "sum")
    assert [p.tolist() for p in model.parameters()] == [[0.0, 2.0, 4.0, 6.0], [2.0, 2.0, 2.0]]


# ----------------------------------------------------------------------------- argument checks
def _call(lib, p, q, lens, dts, n, xsum=0x20000, master=0, divisor=3.0, mode=DIST | WRITE_AVG, out=0x30000,
          dists=0, ws=0x40000, ws_bytes=1 << 20, nseg=None, null=(), msg=None):
    """One call with host tables built from the lists; the made-up device pointers are never
    dereferenced (every case here is rejected before the first launch)."""
    k = len(lens)
    arr = lambda ct, vals: (ct * max(k, 1))(*vals)  # noqa: E731
    tabs = {"params": arr(ctypes.c_void_p, p), "avg_out": arr(ctypes.c_void_p, q),
            "lens": arr(ctypes.c_int64, lens), "dtypes": arr(ctypes.c_int32, dts)}
    a = [None if nm in null else t for nm, t in tabs.items()]
    vp = ctypes.c_void_p
    return lib.choco_params_consensus(*a, k if nseg is None else nseg, vp(xsum), vp(master), n, divisor, mode, vp(out),
                                      vp(dists), vp(ws), ws_bytes, None)


ONE = dict(p=[0x1000], q=[0x2000], lens=[4], dts=[F32], n=4)
TWO = dict(p=[0x1000, 0x1100], q=[0x2000, 0x2100], lens=[4, 4], dts=[F32, BF16], n=8)
BAD = {
    "no mode bit": dict(ONE, mode=0, msg="mode"),
    "unknown mode bit": dict(ONE, mode=4 | DIST, msg="unknown mode"),
    "unknown mode bits alone": dict(ONE, mode=8, msg="unknown mode"),
    "divisor zero": dict(ONE, divisor=0.0, msg="divisor"),
    "divisor zero as fp32": dict(ONE, divisor=1e-60, msg="divisor"),
    "divisor infinite": dict(ONE, divisor=float("inf"), msg="divisor"),
    "divisor infinite as fp32": dict(ONE, divisor=1e39, msg="divisor"),
    "divisor nan": dict(ONE, divisor=float("nan"), msg="divisor"),
    "sum below n": dict(TWO, n=9, msg="lens"),
    "sum above n": dict(TWO, n=7, msg="lens"),
    "negative length": dict(TWO, lens=[-4, 8], n=4, msg="negative length"),
    "null lens": dict(ONE, null=("lens",), msg="lens"),
    "null dtypes": dict(ONE, null=("dtypes",), msg="dtypes"),
    "nseg zero": dict(ONE, nseg=0, msg="nseg"),
    "dtype 3": dict(ONE, dts=[3], msg="dtype"),
    "null xsum": dict(ONE, xsum=0, msg="xsum"),
    "xsum at 2 mod 4": dict(ONE, xsum=0x20002, msg="xsum"),
    "master at 2 mod 4": dict(ONE, master=0x10002, msg="master"),
    "null out with DIST": dict(ONE, out=0, msg="out"),
    "out at 2 mod 4": dict(ONE, out=0x30002, msg="out"),
    "dists at 2 mod 4": dict(ONE, dists=0x50002, msg="dists"),
    "dists without DIST": dict(ONE, mode=WRITE_AVG, dists=0x50000, msg="dists"),
    "null ws with DIST": dict(ONE, ws=0, msg="ws"),
    "ws at 4 mod 8": dict(ONE, ws=0x40004, msg="ws"),
    "ws too small": dict(ONE, ws_bytes=255, msg="ws"),
    "ws empty": dict(ONE, mode=DIST, ws_bytes=0, msg="ws"),
    "null avg_out table with WRITE_AVG": dict(ONE, null=("avg_out",), msg="avg_out"),
    "null avg_out entry with WRITE_AVG": dict(TWO, q=[0x2000, 0], msg="avg_out"),
    "null params table with DIST": dict(ONE, null=("params",), msg="params"),
    "null params entry with DIST": dict(TWO, p=[0x1000, 0], msg="params"),
    "fp32 param at 2 mod 4": dict(TWO, p=[0x1002, 0x1100], msg="params pointer not aligned"),
    "bf16 param at odd byte": dict(TWO, p=[0x1000, 0x1101], msg="params pointer not aligned"),
    "fp32 avg_out at 2 mod 4": dict(TWO, q=[0x2002, 0x2100], msg="avg_out pointer not aligned"),
    "fp16 avg_out at odd byte": dict(TWO, dts=[F32, F16], q=[0x2000, 0x2101], msg="avg_out pointer not aligned"),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_invalid_arguments_are_rejected(lib, case):
    from chocosgd_amd import _lib
    before = [lib.choco_launch_count(nm.encode()) for nm in KERNELS]
    assert _call(lib, **BAD[case]) == ERR_INVALID, case
    err = _lib.last_error()
    assert err != "" and BAD[case]["msg"] in err, (case, err)
    assert [lib.choco_launch_count(nm.encode()) for nm in KERNELS] == before, "nothing was launched"


def test_what_the_checks_let_through(lib):
    """WRITE_AVG alone needs neither out, ws nor params; DIST alone no avg_out; with a master
    copy DIST needs no params; a zero-length tensor no pointers.  (Each call is still rejected,
    later, for its lengths: nothing is launched.)"""
    from chocosgd_amd import _lib
    for kw in (dict(TWO, mode=WRITE_AVG, out=0, ws=0, ws_bytes=0, null=("params",)),
               dict(TWO, mode=WRITE_AVG, p=[0, 0]),
               dict(TWO, mode=DIST, null=("avg_out",)), dict(TWO, mode=DIST, q=[0, 0]),
               dict(TWO, mode=DIST, master=0x10000, null=("params",)), dict(TWO, master=0x10000, p=[0, 0]),
               dict(TWO, divisor=1.0), dict(TWO, divisor=-2.0), dict(TWO, dists=0x50000),
               dict(p=[0x1000, 0, 0x1100], q=[0x2000, 0, 0x2100], lens=[4, 0, 4], dts=[F32, F16, BF16])):
        assert _call(lib, **dict(kw, n=9)) == ERR_INVALID
        assert "add up" in _lib.last_error(), kw


def test_launches_and_workspace_rules(lib):
    from chocosgd_amd import codec
    launches, size = lib.choco_params_consensus_launches, lib.choco_params_consensus_workspace_size
    cap = max(k for k in range(1, 1024) if launches(k, WRITE_AVG) == 1)
    assert cap == CAP
    for nseg in [1, cap - 1, cap, cap + 1, 2 * cap + 3, 3000]:
        chunks = -(-nseg // cap)
        assert launches(nseg, WRITE_AVG) == chunks and launches(nseg, DIST) == chunks + 1
        assert launches(nseg, DIST | WRITE_AVG) == chunks + 1
        assert codec.params_consensus_launches(nseg) == chunks + 1
        assert codec.params_consensus_launches(nseg, want_dist=False) == chunks
    assert launches(161, DIST) == 3, "ResNet-50: two chunk launches and the total"
    assert launches(0, DIST) == 0 and launches(-4, DIST | WRITE_AVG) == 0
    assert launches(5, 0) == 0 and launches(5, 4) == 0 and launches(5, 4 | DIST) == 0
    assert size(0, 100) == 0 and size(-1, 100) == 0 and size(3, -1) == 0
    for nseg, n in [(1, 0), (1, 1), (6, 12333), (161, 25_557_032), (3000, 300_000)]:
        slots = n // TILE + 1 + nseg  # one per (tile, tensor) pair at most
        need = 8 * (2 * slots + 2 * nseg) + 8 * nseg
        assert need <= size(nseg, n) < need + 256 and size(nseg, n) % 256 == 0, (nseg, n)

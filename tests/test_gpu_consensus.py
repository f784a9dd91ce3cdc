"""Consensus evaluation on the device: codec.params_consensus (csrc/consensus.hip,
param_consensus_kernel and param_consensus_total_kernel), auxiliary.consensus_eval /
get_model_difference and CentralizedAggregation.agg_model / agg_grad.

Everything is compared bit for bit against the model (tests/_consensus_oracle.py, pinned to the
reference's recording on the host by tests/test_consensus_host.py), the summation order included:
it depends on the layout alone, so views at every alignment give the same bits.  Whole storages
are compared, so that every byte a launch does not own is checked together with the ones it does."""
import numpy as np
import pytest
import torch

from conftest import golden, same_bits
import _consensus_oracle as CO
import _sgd_oracle as SO
import test_consensus_host as H
import test_gpu_param_sgd as PS  # the guarded layouts and value lists of the SGD kernel's tests

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES, NAMES, SENTINEL = PS.DTYPES, PS.NAMES, PS.SENTINEL
MODES = ["fp32", "bf16", "fp16", "mixed"]
F32 = torch.float32
CAP, TILE = H.CAP, H.TILE
host = H.host
NAMES_COUNTED = ("param_consensus_kernel", "param_consensus_total_kernel", "param_pack_kernel", "param_unpack_kernel")
ZEROS = [0, 5, 0, 0, 4100, 0, 9000, 0]
MANY = [1 + i % 9 for i in range(CAP + 3)]


def _counts():
    from chocosgd_amd import codec
    return [codec.launch_count(nm) for nm in NAMES_COUNTED]


def _delta(c0):
    return [b - a for a, b in zip(c0, _counts())]


def _tame(v):
    """Finite values whose squares and differences stay finite: a finite distance."""
    with np.errstate(all="ignore"):
        return np.where(np.isfinite(v) & (np.abs(v) < 1e4), v, np.float32(1.5)).astype(np.float32)


def _tame_guarded(G):
    for (s, p, m), view in zip(G.where, G.views):
        if m:
            view.copy_(torch.from_numpy(_tame(host(view))).to(DEV).to(view.dtype))
    G.before = [s.clone() for s in G.stores]


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


def _pieces(flat, lens):
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return [flat[offs[s]:offs[s + 1]] for s in range(len(lens))]


# ----------------------------------------------------------------------------- kernel against the model
def run_case(lens, mode, master=False, lead=(0, 0), gap=8, own=False, xsum_shift=4, master_shift=4, divisor=3.0,
             dist=True, write=True, in_place=False, tame=False, per_tensor=True, seed=9000, plan=None):
    """One codec.params_consensus call on guarded storages against the model; returns (out,
    dists, launches, plan).  lead: sentinel elements in front of the (params, avg_out) storages;
    xsum and the master copy are views at an element shift inside sentinel-filled allocations."""
    from chocosgd_amd import codec
    k, n = len(lens), sum(lens)
    dts = PS._dtypes(mode, k)
    names = [NAMES[d] for d in dts]
    P = PS.Guarded(lens, dts, seed, -3, 1, lead[0], gap, own)
    Q = PS.Guarded(lens, dts, seed + 5000, -4, 0, lead[1], gap, own)  # outputs: what they hold is overwritten
    if tame:
        _tame_guarded(P)
    fix = _tame if tame else (lambda v: v)
    s_all = np.concatenate([fix(PS._values(m, seed + 30000 + i, -3, 1)) for i, m in enumerate(lens)] +
                           [np.zeros(0, np.float32)])
    m_all = np.concatenate([fix(PS._values(m, seed + 20000 + i, -3, 1)) for i, m in enumerate(lens)] +
                           [np.zeros(0, np.float32)])
    bigs, xsum = _guarded_flat(s_all, xsum_shift)
    bigm, mview = _guarded_flat(m_all, master_shift)
    x = m_all if master else np.concatenate([host(v) for v in P.views] + [np.zeros(0, np.float32)])
    avg, mout, mdists = CO.consensus(x, s_all, divisor, lens, names)
    bigd, dview = _guarded_flat(np.full(k, 3.0, dtype=np.float32), 1)
    out_views = None if not write else (P.views if in_place else Q.views)
    c0 = _counts()
    out, plan = codec.params_consensus(P.views, xsum, divisor, avg_out=out_views, master=mview if master else None,
                                       dists=dview if dist and per_tensor else None, want_dist=dist, plan=plan)
    d = _delta(c0)
    new = _pieces(avg, lens)
    P.check(new if write and in_place else [None] * k, "params (or their guards)")
    Q.check(new if write and not in_place else [None] * k, "avg_out (or its guards)")
    _check_flat(bigs, xsum_shift, s_all, "xsum was written")
    _check_flat(bigm, master_shift, m_all, "master was written")
    _check_flat(bigd, 1, mdists if dist and per_tensor else np.full(k, 3.0, dtype=np.float32), "dists (or its guards)")
    chunks = -(-k // CAP)
    assert d == [chunks, 1 if dist else 0, 0, 0], "launches: the chunk launches and, under DIST, the total"
    assert sum(d) == codec.params_consensus_launches(k, want_dist=dist)
    if not dist:
        assert out is None
        return None, None, d, plan
    assert out.dtype == F32 and out.shape == (2,) and same_bits(host(out), mout), (host(out), mout)
    if tame:
        assert np.isfinite(mout).all() and np.isfinite(mdists).all()
    return host(out).copy(), host(dview).copy(), d, plan


def both(lens, mode, **kw):
    """Special values everywhere (NaN / inf reach out and dists as in the model), then tame ones
    (a finite distance, every bit of it)."""
    run_case(lens, mode, **kw)
    run_case(lens, mode, tame=True, **kw)


@pytest.mark.parametrize("gap", [1, 2, 3])
@pytest.mark.parametrize("master", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_views_at_element_alignment(mode, master, gap):
    """Views into one allocation whose element offsets run through every residue (lead 1, gaps
    1 / 2 / 3), xsum and master at odd element shifts: nothing next to a tensor is touched."""
    both(PS.BASE, mode, master=master, lead=(1, 1), gap=gap, xsum_shift=4 + gap, master_shift=7 - gap)


@pytest.mark.parametrize("master", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_aligned_layout(mode, master):
    """Every side on the group grid where the flat offset allows it: the 16-byte path."""
    both(PS.BASE, mode, master=master, own=True)
    both([40, TILE + 24, 8, 304], mode, master=master, own=True)


@pytest.mark.parametrize("off", ["p", "avg_out", "xsum", "master"])
@pytest.mark.parametrize("mode", MODES)
def test_one_side_off_the_grid_gives_the_same_bits(mode, off):
    """All sides on the 16-byte grid but one: the tensors move element by element, no
    neighbouring byte changes, and out and dists keep the bits of the aligned call."""
    lens = [40, TILE + 24, 8, 2 * TILE + 304]
    lead = {"p": (1, 0), "avg_out": (0, 1)}.get(off, (0, 0))
    kw = dict(own=True, tame=True, master=off == "master")
    o0, d0, _, _ = run_case(lens, mode, **kw)
    o1, d1, _, _ = run_case(lens, mode, lead=lead, xsum_shift=5 if off == "xsum" else 4,
                            master_shift=5 if off == "master" else 4, **kw)
    assert same_bits(o0, o1) and same_bits(d0, d1)


@pytest.mark.parametrize("lens", [[TILE], [TILE - 1, 1], [TILE + 1], [1, TILE, 1], [2 * TILE + 5], ZEROS, [0], [0, 0, 7]],
                         ids=str)
@pytest.mark.parametrize("mode", MODES)
def test_tile_ends_and_zero_length_tensors(mode, lens):
    both(lens, mode, own=True)
    both(lens, mode, master=True, lead=(1, 3), gap=1, xsum_shift=5)


@pytest.mark.parametrize("count", [CAP - 1, CAP, CAP + 1, CAP + 3, 2 * CAP + 3])
def test_chunk_boundaries_inside_a_tile(count):
    lens = [1 + i % 9 for i in range(count)]
    assert run_case(lens, "mixed", tame=True)[2][0] == -(-count // CAP)
    assert run_case(lens, "bf16", gap=1, lead=(1, 1), master=True)[2][0] == -(-count // CAP)


def test_a_chunk_boundary_inside_a_long_tensor_run():
    """Two launches whose chunks meet inside a tile and tensors that span tiles on both sides."""
    lens = [70] * (CAP - 2) + [TILE + 3, 2 * TILE + 1, 5, 1500]
    both(lens, "mixed", gap=1, lead=(1, 2))


@pytest.mark.parametrize("master", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_one_mode_bit_alone(mode, master):
    """WRITE_AVG alone launches only param_consensus_kernel, once per chunk, and needs no
    workspace; DIST alone writes no tensor."""
    for lens in (PS.BASE, MANY):
        run_case(lens, mode, master=master, dist=False)
        run_case(lens, mode, master=master, write=False, tame=True)
        run_case(lens, mode, master=master, write=False, per_tensor=False)


@pytest.mark.parametrize("master", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_in_place(mode, master):
    """avg_out is the parameters, both bits set: the distance is that of the old values, the
    parameters are the narrowed average."""
    for kw in (dict(own=True), dict(gap=1, lead=(1, 1))):
        o0, d0, _, _ = run_case(PS.BASE, mode, master=master, tame=True, **kw)
        o1, d1, _, _ = run_case(PS.BASE, mode, master=master, tame=True, in_place=True, **kw)
        assert same_bits(o0, o1) and same_bits(d0, d1)
    run_case([3 * TILE + 5, 77], mode, master=master, in_place=True, own=True)
    run_case(PS.BASE, mode, master=master, in_place=True, dist=False)


@pytest.mark.parametrize("divisor", [1.0, 2.0, 3.0, 7.0, -3.0])
@pytest.mark.parametrize("mode", MODES)
def test_divisors_and_special_values(mode, divisor):
    """The _values specials (NaN, +-inf, +-0, subnormals, values past fp16's range) in xsum and
    the parameters; 3 and 7: a reciprocal multiply differs from the division on about a third
    of the values; divisor 1 returns xsum narrowed exactly."""
    from chocosgd_amd import codec
    lens = [33, 8195, 4099]
    both(lens, mode, divisor=divisor)
    both(lens, mode, divisor=divisor, own=True, master=True)
    if divisor != 1.0:
        return
    dts = PS._dtypes(mode, len(lens))
    s = np.concatenate([PS._values(m, 50 + i, -3, 1) for i, m in enumerate(lens)])
    Q = [torch.zeros(m, dtype=dt, device=DEV) for m, dt in zip(lens, dts)]
    codec.params_consensus(Q, torch.from_numpy(s).to(DEV), 1.0, avg_out=Q, want_dist=False)
    for q, piece, dt in zip(Q, _pieces(s, lens), dts):
        assert same_bits(host(q), SO.to_grid(piece, NAMES[dt]))
    stats, _ = codec.params_consensus(Q, torch.cat([q.float() for q in Q]), 1.0)
    assert host(stats)[0] == 0.0 or np.isnan(host(stats)[0])


def test_nan_and_inf_reach_out_and_dists_as_in_the_model():
    from chocosgd_amd import codec
    lens = [100, 100, 0, 100, TILE + 100]
    x = [torch.ones(m, device=DEV) for m in lens]
    s = torch.full((sum(lens),), 6.0, device=DEV)
    s[150], s[250] = float("nan"), float("inf")
    dists = torch.empty(len(lens), device=DEV)
    out, _ = codec.params_consensus(x, s, 3.0, dists=dists)
    got = host(dists)
    assert got[0] == 10.0 and np.isnan(got[1]) and got[2] == 0.0 and np.isinf(got[3]) and got[4] == np.float32(
        np.sqrt(TILE + 100.0))
    assert np.isnan(host(out)).all()


# ----------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("mode", MODES)
def test_determinism_and_the_plan_against_the_free_function(mode):
    """Two calls on the same inputs give identical bits; so does a plan reused across calls, a
    fresh one, and the same tensors at another alignment."""
    from chocosgd_amd import codec
    lens = MANY + [3 * TILE + 11, 900, 2000]
    o0, d0, _, _ = run_case(lens, mode, tame=True)
    o2, d2, _, _ = run_case(lens, mode, tame=True, gap=1, lead=(1, 2), xsum_shift=7)
    assert same_bits(o0, o2) and same_bits(d0, d2)
    dts = PS._dtypes(mode, len(lens))
    ps = [torch.from_numpy(_tame(host(torch.from_numpy(PS._values(m, 9000 + i, -3, 1)).to(dt)))).to(DEV).to(dt)
          for i, (m, dt) in enumerate(zip(lens, dts))]  # run_case's values: narrowed, then tamed
    xsum = torch.from_numpy(np.concatenate([_tame(PS._values(m, 39000 + i, -3, 1)) for i, m in enumerate(lens)])).to(DEV)
    got = []
    plan = None
    for reuse in (False, True, True, False):
        dists = torch.empty(len(lens), device=DEV)
        out, p = codec.params_consensus(ps, xsum, 3.0, dists=dists, plan=plan if reuse else None)
        assert not reuse or p is plan
        plan = p
        got.append((host(out).copy(), host(dists).copy()))
    dists = torch.empty(len(lens), device=DEV)
    got.append((host(plan.consensus(xsum, 3.0, dists=dists)).copy(), host(dists).copy()))
    for o, d in got:
        assert same_bits(o, o0) and same_bits(d, d0)
    # the same flat values cut into other tensors: the total is the model's for that layout
    run_case([sum(MANY)] + [3 * TILE + 11, 900, 2000], mode, tame=True)


# ----------------------------------------------------------------------------- the reference's recording, on the device
class DeviceAgg(H.FakeAgg):
    def __init__(self, fx):
        super().__init__(fx)
        self.x1, self.x2 = self.x1.to(DEV), self.x2.to(DEV)


def _device_model(flat, lens, names=None):
    return H.Model([t.to(DEV) for t in H._split(flat, lens, names)])


@pytest.mark.parametrize("name", H.SETS)
def test_fixture_replay_on_the_device(name):
    from chocosgd_amd import auxiliary, codec
    fx = golden(f"consensus_{name}")
    lens = fx["lens"].tolist()
    k = len(lens)
    _, mout, mdists = CO.consensus(fx["x0"], fx["sum"], 3.0, lens, ["fp32"] * k)
    model, copy = _device_model(fx["x0"], lens), _device_model(np.zeros_like(fx["x0"]), lens)
    agg = DeviceAgg(fx)
    c0 = _counts()
    stats, dists = auxiliary.consensus_eval(model, agg, avg_out=copy, per_tensor=True)
    assert _delta(c0) == [1, 1, codec.params_launches(k), 0] and agg.calls == 1
    assert same_bits(H._cat(copy.parameters()), fx["avg"]) and same_bits(H._cat(model.parameters()), fx["x0"])
    H._check_distance(host(stats)[0], fx, mout[0])
    assert same_bits(host(stats), mout) and same_bits(host(dists), mdists)
    # get_model_difference: the pack of model2 and the kernel with divisor 1
    c0 = _counts()
    got = auxiliary.get_model_difference(model, copy)
    assert _delta(c0) == [1, 1, codec.params_launches(k), 0] and isinstance(got, float)
    H._check_distance(np.float32(got), fx, CO.consensus(fx["x0"], fx["avg"], 1.0, lens, ["fp32"] * k)[1][0])
    # agg_model and agg_grad in place: one pack, one collective, one WRITE_AVG launch
    from chocosgd_amd.communication import CentralizedAggregation

    class Recorded(CentralizedAggregation):
        _agg = H.FakeAgg._agg

    cagg = object.__new__(Recorded)
    cagg.rank, cagg.group, cagg.world_size, cagg.calls = 0, None, 3.0, 0
    cagg.x1, cagg.x2 = agg.x1, agg.x2
    twin = _device_model(fx["x0"], lens)
    ptrs = [p.data_ptr() for p in twin.parameters()]
    c0 = _counts()
    cagg.agg_model(twin, "avg")
    assert _delta(c0) == [1, 0, codec.params_launches(k), 0] and cagg.calls == 1
    assert same_bits(H._cat(twin.parameters()), fx["avg"]) and ptrs == [p.data_ptr() for p in twin.parameters()]
    for p, g in zip(twin.parameters(), H._split(fx["x0"], lens)):
        p.grad = g.to(DEV)
    cagg.agg_grad(twin, "sum")
    assert same_bits(H._cat([p.grad for p in twin.parameters()]), fx["sum"])
    assert same_bits(H._cat(twin.parameters()), fx["avg"])
    with pytest.raises(NotImplementedError):
        cagg.agg_model(twin, "min")


def test_consensus_eval_without_avg_out_copies_no_model():
    """The launch list is the pack, the chunk launch and the total; beyond the flat fp32 buffer
    nothing of the model's size is allocated."""
    from chocosgd_amd import auxiliary, codec
    fx = golden("consensus_ordinary")
    lens = fx["lens"].tolist()
    model, agg = _device_model(fx["x0"], lens), DeviceAgg(fx)
    auxiliary.consensus_eval(model, agg)  # the plan, its workspace and its output exist from here on
    torch.cuda.synchronize()
    flat_bytes = 4 * sum(lens)
    c0, before = _counts(), torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    stats, dists = auxiliary.consensus_eval(model, agg)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert _delta(c0) == [1, 1, codec.params_launches(len(lens)), 0] and dists is None
    assert flat_bytes <= peak < flat_bytes + flat_bytes // 2, "the flat buffer, and no copy of the model"
    assert same_bits(H._cat(model.parameters()), fx["x0"])


# ----------------------------------------------------------------------------- against the loop
@pytest.mark.parametrize("use_master", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_consensus_eval_against_the_loop(mode, use_master):
    from chocosgd_amd import auxiliary
    lens = PS.BASE
    n = sum(lens)
    names = H._names(mode, len(lens))
    fx = {"world": 3.0, "x1": _tame(PS._values(n, 97, -3, 1)), "x2": _tame(PS._values(n, 98, -3, 1))}
    x0 = _tame(np.concatenate([PS._values(m, 70 + i, -3, 1) for i, m in enumerate(lens)]))
    master = torch.from_numpy(_tame(PS._values(n, 99, -3, 1))).to(DEV) if use_master else None
    res = []
    for fn in (auxiliary.consensus_eval, auxiliary.consensus_eval_loop):
        params = [t.to(DEV) for t in H._split(x0, lens, names)]
        copy = [torch.zeros_like(p) for p in params]
        c0 = _counts()
        stats, dists = fn(params, DeviceAgg(fx), avg_out=copy, master=master, per_tensor=True)
        assert (_delta(c0)[0] == 1) == (fn is auxiliary.consensus_eval)
        res.append((host(stats).copy(), host(dists).copy(), H._cat(copy), H._cat(params)))
    for a, b in zip(*res):
        assert same_bits(a, b)
    assert np.isfinite(res[0][0]).all() and res[0][0][0] > 0
    # a non-contiguous parameter takes the loop, with the same bits
    params = [t.to(DEV) for t in H._split(x0, lens, names)]
    wide = torch.zeros(2 * lens[-1], dtype=params[-1].dtype, device=DEV)
    wide[::2] = params[-1]
    params[-1] = wide[::2]
    c0 = _counts()
    stats, dists = auxiliary.consensus_eval(params, DeviceAgg(fx), master=master, per_tensor=True)
    assert _delta(c0)[0] == 0 and same_bits(host(stats), res[0][0]) and same_bits(host(dists), res[0][1])

"""DGC's optimizer half on the device: codec.params_sqnorm, the clipped update
(ParamSgdPlan.run(norms=, clip_threshold=, add_flat=)), codec.params_mask and the layers above
them (dgc.apply_gradient, DGCCodec.compress(momentum_buffers=, grads_in_memory=),
dgc.fused_step).

The fp32 fixtures are the reference's own results (tests/golden/dgc_sgd_*.npz); every other
case is checked bit for bit against the numpy model (tests/_dgc_oracle.py), whole storages at a
time, so that every byte a launch does not own is checked together with the ones it does.  The
norms alone have a tolerance: equal or adjacent on the dtype's grid to
float32(sqrt(sum(d.astype(float64) ** 2))) -- any-order fp64 summation of n <= 2^31
non-negative terms is within n * 2^-53 relative of the exact sum, far inside half an fp32 ulp,
so the two can only round to the same value or to neighbours."""
import collections

import numpy as np
import pytest
import torch

from conftest import golden, same_bits
from oracle import choco_oracle as O
import _dgc_oracle as DO
import _sgd_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SENTINEL = -7.0  # exact in every dtype
SETS = ["clip", "wd", "mom", "nesterov", "damp"]
STEPS = 3
GAP = 64  # elements between two views of a storage: 64 * esz is a multiple of 16 bytes


def host(t):
    return t.detach().float().cpu().numpy()


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(dtype)


@pytest.fixture(scope="module")
def inputs():
    return golden("dgc_sgd_inputs")


def _offs(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


class Views:
    """Tensors as views into ONE storage: view s starts at element GAP * (s + 1) + off_s + shift,
    so with shift 0 every view is congruent with the 16-byte group grid of the flat layout (the
    vector path) and with shift 1 none is (the scalar path); everything between is sentinel."""

    def __init__(self, flat, lens, dtype, shift=0):
        self.lens, self.dtype = list(lens), dtype
        off = _offs(lens)
        self.starts = [GAP * (s + 1) + int(off[s]) + shift for s in range(len(lens))]
        self.total = GAP * (len(lens) + 2) + int(off[-1])
        self.store = torch.full((self.total,), SENTINEL, device=DEV, dtype=DTYPES[dtype])
        self.views = [self.store[a:a + m] for a, m in zip(self.starts, lens)]
        self.write(flat)

    def write(self, flat):
        o = 0
        for v, m in zip(self.views, self.lens):
            v.copy_(dev(flat[o:o + m], v.dtype))
            o += m

    def expect(self, flat):
        """The whole storage as fp32 with `flat` in the views."""
        out = np.full(self.total, SENTINEL, dtype=np.float32)
        o = 0
        for a, m in zip(self.starts, self.lens):
            out[a:a + m] = flat[o:o + m]
            o += m
        return out

    def all(self):
        return host(self.store)


def _grid_key(v, dtype):
    """Non-negative finite values of the dtype's grid as integers ordered like the values."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    if dtype == "fp16":
        return v.astype(np.float16).view(np.int16).astype(np.int64)
    k = v.view(np.int32).astype(np.int64)
    return k >> 16 if dtype == "bf16" else k


def _check_norms(got, p, g, lens, wd, dtype):
    want = DO.norms_layout(p, g, lens, wd, dtype)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    assert np.array_equal(np.isinf(got), np.isinf(want)), (got, want)
    fin = np.isfinite(want)
    assert np.all(got[fin] >= 0)
    assert same_bits(got, SO.to_grid(got, dtype)), "a norm off its dtype's grid"
    assert np.all(np.abs(_grid_key(got[fin], dtype) - _grid_key(want[fin], dtype)) <= 1), (got, want)


def _run_norms(p, g, lens, wd, dtype, shift):
    from chocosgd_amd import codec
    pv, gv = Views(p, lens, dtype, shift), Views(g, lens, dtype, shift)
    pe, ge = pv.all(), gv.all()
    k0, f0 = codec.launch_count("param_sqnorm_kernel"), codec.launch_count("param_sqnorm_finish_kernel")
    plan = codec.ParamSgdPlan(pv.views)
    a = host(codec.params_sqnorm(pv.views, gv.views, wd, plan=plan).clone())
    b = host(codec.params_sqnorm(pv.views, gv.views, wd, plan=plan).clone())
    k1, f1 = codec.launch_count("param_sqnorm_kernel"), codec.launch_count("param_sqnorm_finish_kernel")
    assert f1 - f0 == 2 and (k1 - k0) + (f1 - f0) == 2 * codec.params_sqnorm_launches(len(lens))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "two calls, two results"
    assert same_bits(pv.all(), pe) and same_bits(gv.all(), ge), "the norm pass wrote something"
    return a


# ----------------------------------------------------------------------------- norms
@pytest.mark.parametrize("name", ["clip", "nesterov"])
def test_norms_fixture_layout(inputs, name):
    fx = golden(f"dgc_sgd_{name}")
    wd = float(fx["hp"][1])
    lens = inputs["lens"].tolist()
    for k in range(STEPS):
        got = _run_norms(inputs["p0"], inputs[f"g{k}"], lens, wd, "fp32", 0)
        _check_norms(got, inputs["p0"], inputs[f"g{k}"], lens, wd, "fp32")
        # and next to what torch's CPU norm gave the reference
        ref = fx[f"norm{k}"]
        fin = np.isfinite(ref)
        assert np.all(np.abs(_grid_key(got[fin], "fp32") - _grid_key(ref[fin], "fp32")) <= 2)
        assert got[-1] == ref[-1], "the one-element tensor's norm is exact"


def _layout_values(lens, seed, dtype, scale=1.0):
    rng = np.random.RandomState(seed)
    n = int(sum(lens))
    p = SO.to_grid((rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 1, n)).astype(np.float32), dtype)
    g = SO.to_grid((rng.standard_normal(n) * scale * 10.0 ** rng.uniform(-3, 0, n)).astype(np.float32), dtype)
    return p, g


def test_norms_many_small_tensors():
    """300 tensors of 1-40 elements: more than one launch's table, ~290 tensors in one tile."""
    rng = np.random.RandomState(5)
    lens = rng.randint(1, 41, 300).tolist()
    p, g = _layout_values(lens, 6, "fp32")
    for wd in (0.0, 5e-4):
        _check_norms(_run_norms(p, g, lens, wd, "fp32", 0), p, g, lens, wd, "fp32")


LAYOUT = [5, 1, 0, 8195, 33, 4099, 17000, 40, 1500, 1]  # 1500: a whole-workgroup span inside a tile


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_norms_views_inside_one_storage(dtype, shift):
    p, g = _layout_values(LAYOUT, 11, dtype)
    off = _offs(LAYOUT)
    g[off[3] + 7] = np.inf      # an inf and a NaN tensor
    g[off[5] + 100] = np.nan
    for wd in (0.0, 1e-2):
        _check_norms(_run_norms(p, g, LAYOUT, wd, dtype, shift), p, g, LAYOUT, wd, dtype)


def test_norms_do_not_overflow_where_fp32_accumulation_does():
    lens = [3000, 7]
    g = np.full(sum(lens), 3e19, dtype=np.float32)  # squares past fp32's range
    got = _run_norms(np.zeros_like(g), g, lens, 0.0, "fp32", 0)
    assert np.all(np.isfinite(got))
    _check_norms(got, np.zeros_like(g), g, lens, 0.0, "fp32")


def test_norms_of_no_grad_tensors_are_zero():
    from chocosgd_amd import codec
    lens = [10, 20, 5]
    p, g = _layout_values(lens, 3, "fp32")
    pv, gv = Views(p, lens, "fp32"), Views(g, lens, "fp32")
    got = host(codec.params_sqnorm(pv.views, [gv.views[0], None, gv.views[2]], 0.0))
    want = DO.norms_layout(p, g, lens, 0.0)
    assert got[1] == 0 and abs(int(got[0].view(np.int32)) - int(want[0].view(np.int32))) <= 1
    assert abs(int(got[2].view(np.int32)) - int(want[2].view(np.int32))) <= 1


# ----------------------------------------------------------------------------- the clipped update
def _device_model(inputs, hp, dtype="fp32"):
    lr, wd, mom, damp, nest = hp
    lens = inputs["lens"].tolist()
    params, o = [], 0
    for m in lens:
        params.append(torch.nn.Parameter(dev(inputs["p0"][o:o + m], DTYPES[dtype])))
        o += m
    groups = [{"params": [p], "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": damp, "nesterov": bool(nest)}
              for p in params]
    return params, groups, lens


def _set_grads(params, flat, lens):
    o = 0
    for p, m in zip(params, lens):
        p.grad = dev(flat[o:o + m], p.dtype)
        o += m


def _cat(tensors):
    return np.concatenate([host(t).reshape(-1) for t in tensors])


def _launches():
    from chocosgd_amd import codec
    return np.array([codec.launch_count(k) for k in ("param_sqnorm_kernel", "param_sqnorm_finish_kernel",
                                                     "param_sgd_kernel", "param_pack_kernel", "param_mask_kernel")])


@pytest.mark.parametrize("name", SETS)
def test_clipped_update_with_the_fixture_norms(inputs, name):
    """The reference's three steps through dgc.apply_gradient on the device with the norms the
    reference saw uploaded: d_p, the buffers and flat, bit for bit."""
    from chocosgd_amd import codec, dgc
    fx = golden(f"dgc_sgd_{name}")
    hp = fx["hp"].tolist()
    params, groups, lens = _device_model(inputs, hp)
    n = sum(lens)
    val, n_nodes = float(inputs["clip_grad_val"]), int(inputs["n_nodes"])
    state = collections.defaultdict(dict)
    big = torch.full((n + 8,), SENTINEL, device=DEV)
    flat = big[4:4 + n]
    c0 = _launches()
    for k in range(STEPS):
        _set_grads(params, inputs[f"g{k}"], lens)
        grads = [p.grad for p in params]
        used = dgc.apply_gradient(groups, state, clip_grad=True, clip_grad_val=val, n_nodes=n_nodes, flat_out=flat,
                                  norms=dev(fx[f"norm{k}"]))
        assert same_bits(host(used), fx[f"norm{k}"])
        assert same_bits(_cat(grads), fx[f"d{k}"]), f"d_p after step {k}"
        assert same_bits(host(flat), fx[f"d{k}"]), f"flat after step {k}"
        assert same_bits(_cat(params), inputs["p0"])
        assert all(p.grad is g for p, g in zip(params, grads))
        if hp[2] != 0:
            assert same_bits(_cat([state[p]["momentum_buffer"] for p in params]), fx[f"buf{k}"]), f"buf, step {k}"
        assert torch.all(big[:4] == SENTINEL) and torch.all(big[4 + n:] == SENTINEL)
    assert (_launches() - c0).tolist() == [0, 0, STEPS * codec.params_sgd_launches(len(lens)), 0, 0]


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("name", ["clip", "nesterov", "damp"])
def test_clipped_update_with_device_norms(inputs, name, dtype):
    """Unpinned: the norm pass and the update, against the model evaluated at the device's norms;
    ADD_FLAT against memory + d."""
    from chocosgd_amd import codec, dgc
    fx = golden(f"dgc_sgd_{name}")
    hp = fx["hp"].tolist()
    params, groups, lens = _device_model(inputs, hp, dtype)
    p0 = SO.to_grid(inputs["p0"], dtype)
    n = sum(lens)
    val, n_nodes, thr = float(inputs["clip_grad_val"]), int(inputs["n_nodes"]), float(inputs["thr"])
    state = collections.defaultdict(dict)
    rng = np.random.RandomState(2)
    mem = rng.standard_normal(n).astype(np.float32)
    big = torch.full((n + 8,), SENTINEL, device=DEV)
    big[4:4 + n] = dev(mem)
    flat = big[4:4 + n]
    buf = None
    nseg = len(lens)
    c0 = _launches()
    for k in range(STEPS):
        g = SO.to_grid(inputs[f"g{k}"], dtype)
        _set_grads(params, g, lens)
        used = host(dgc.apply_gradient(groups, state, clip_grad=True, clip_grad_val=val, n_nodes=n_nodes,
                                       flat_out=flat, add_flat=True))
        _check_norms(used, p0, g, lens, hp[1], dtype)
        _, buf, d = DO.step_layout(p0, g, buf, lens, hp, k == 0, used, thr, dtype)
        assert same_bits(_cat([p.grad for p in params]), d), f"d_p after step {k}"
        if hp[2] != 0:
            assert same_bits(_cat([state[p]["momentum_buffer"] for p in params]), buf), f"buf, step {k}"
        with np.errstate(all="ignore"):
            mem = (mem + d).astype(np.float32)
        assert same_bits(host(flat), mem), f"memory + d after step {k}"
        assert torch.all(big[:4] == SENTINEL) and torch.all(big[4 + n:] == SENTINEL)
    want = [STEPS * (codec.params_sqnorm_launches(nseg) - 1), STEPS, STEPS * codec.params_sgd_launches(nseg), 0, 0]
    assert (_launches() - c0).tolist() == want


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_apply_mode_with_clip(dtype, shift):
    """Apply mode (p -= lr * d) with clipping, views inside one storage, against the model; more
    than one launch's table of tensors."""
    from chocosgd_amd import codec
    rng = np.random.RandomState(9)
    lens = LAYOUT + rng.randint(1, 41, 80).tolist()
    nseg, n = len(lens), sum(lens)
    p, g = _layout_values(lens, 21, dtype, scale=0.05)
    off = _offs(lens)
    g[off[3]:off[4]] *= 40  # one long tensor well over the threshold, as are some short ones
    g = SO.to_grid(g, dtype)
    b = SO.to_grid(rng.standard_normal(n).astype(np.float32), dtype)
    hp = (0.1, 5e-4, 0.9, 0.0, True)
    thr = 0.5
    pv, gv, bv = Views(p, lens, dtype, shift), Views(g, lens, dtype, shift), Views(b, lens, dtype, shift)
    plan = codec.ParamSgdPlan(pv.views)
    norms = codec.params_sqnorm(pv.views, gv.views, hp[1], plan=plan)
    nh = host(norms)
    _check_norms(nh, p, g, lens, hp[1], dtype)
    assert np.sum(nh >= thr) >= 3 and np.sum(nh < thr) >= 3
    for i in range(nseg):
        plan.buf_ptrs[i] = bv.views[i].data_ptr()
        plan.lr[i], plan.momentum[i], plan.dampening[i] = hp[0], hp[2], hp[3]
        plan.flags[i] = codec.SGD_F_NESTEROV
    big = torch.full((n + 8,), SENTINEL, device=DEV)
    flat = big[4:4 + n]
    plan.run(flat, grad_mode=False, write=True, norms=norms, clip_threshold=thr)
    p_new, b_new, _ = DO.step_layout(p, g, b, lens, hp, False, nh, thr, dtype)
    assert same_bits(pv.all(), pv.expect(p_new)) and same_bits(bv.all(), bv.expect(b_new))
    assert same_bits(gv.all(), gv.expect(g)), "apply mode wrote the grads"
    assert same_bits(host(flat), p_new)
    assert torch.all(big[:4] == SENTINEL) and torch.all(big[4 + n:] == SENTINEL)


def test_special_norms(inputs):
    """A NaN norm leaves its tensor alone, an inf norm gives c = 0, norm == (float)thr clips."""
    from chocosgd_amd import codec
    lens = [40, 40, 40, 40]
    p, g = _layout_values(lens, 4, "fp32")
    thr = float(inputs["thr"])
    nh = np.array([np.nan, np.inf, np.float32(thr), np.nextafter(np.float32(thr), np.float32(0))], dtype=np.float32)
    pv, gv = Views(p, lens, "fp32"), Views(g, lens, "fp32")
    plan = codec.ParamSgdPlan(pv.views)
    codec.params_sqnorm(pv.views, gv.views, 0.0, plan=plan)  # fills the tables
    for i in range(4):
        plan.lr[i] = 0.1
    plan.run(None, grad_mode=True, write=True, norms=dev(nh), clip_threshold=thr)
    _, _, d = DO.step_layout(p, g, None, lens, (0.1, 0.0, 0.0, 0.0, False), True, nh, thr)
    assert same_bits(d[:40], g[:40]) and np.all(d[40:80] == 0) and same_bits(d[120:], g[120:])
    assert not same_bits(d[80:120], g[80:120])
    assert same_bits(gv.all(), gv.expect(d))


# ----------------------------------------------------------------------------- mask
def _selection(x, lens, ratio):
    """O.topk_segmented with no slot for a zero-length tensor."""
    vals, idxs, ks, off = [], [], [], 0
    for m in lens:
        if m:
            k = O.topk_k(m, ratio)
            v, i = O.topk(x[off:off + m], k)
            vals.append(v)
            idxs.append(i + off)
            ks.append(k)
        else:
            ks.append(0)
        off += m
    return np.concatenate(vals).astype(np.float32), np.concatenate(idxs).astype(np.int32), ks


@pytest.mark.parametrize("which", ["fixture", "small300"])
def test_mask(inputs, which):
    from chocosgd_amd import codec
    rng = np.random.RandomState(31)
    lens = inputs["lens"].tolist() if which == "fixture" else rng.randint(1, 41, 300).tolist()
    nseg, n = len(lens), sum(lens)
    off = _offs(lens)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 1, n)).astype(np.float32)
    x[rng.choice(n, 5, replace=False)] = [np.inf, -np.inf, np.nan, 3e38, -0.0]
    values, indices, ks = _selection(x, lens, 0.9)
    names = ["fp32", "bf16", "fp16"]
    dts = [names[s % 3] for s in range(nseg)]
    b = rng.standard_normal(n).astype(np.float32)
    sel = indices[rng.choice(len(indices), min(len(indices), 24), replace=False)]
    b[sel[:8]], b[sel[8:16]], b[sel[16:20]], b[sel[20:]] = -3.0, np.inf, np.nan, -np.inf
    none = {1, 4} if which == "fixture" else set(range(7, nseg, 11))
    # one out-of-range index: the first slot of a tensor points into the tensor before it
    koff = _offs(ks)
    t = 3 if which == "fixture" else 150
    indices[koff[t]] = off[t] - 1
    stores, bufs, model = [], [], []
    for s in range(nseg):
        if s in none:
            stores.append(None), bufs.append(None), model.append(None)
            continue
        st = torch.full((lens[s] + 16,), SENTINEL, device=DEV, dtype=DTYPES[dts[s]])
        vals = SO.to_grid(b[off[s]:off[s + 1]], dts[s])
        st[8:8 + lens[s]] = dev(vals, st.dtype)
        stores.append(st), bufs.append(st[8:8 + lens[s]]), model.append(vals.copy())
    big = torch.full((n + 8,), SENTINEL, device=DEV)
    big[4:4 + n] = dev(x)
    memory = big[4:4 + n]
    mem_model = x.copy()
    DO.mask(model, dts, lens, values, indices, ks, mem_model)
    c0 = _launches()
    codec.params_mask(bufs, dev(values), torch.from_numpy(indices).to(DEV), ks, memory=memory, lens=lens,
                      dtypes=[DTYPES[d] for d in dts])
    assert (_launches() - c0).tolist() == [0, 0, 0, 0, codec.params_mask_launches(nseg)]
    for s in range(nseg):
        if stores[s] is None:
            continue
        want = np.full(lens[s] + 16, SENTINEL, dtype=np.float32)
        want[8:8 + lens[s]] = model[s]
        assert same_bits(host(stores[s]), want), f"buffer {s}"
    assert same_bits(host(memory), mem_model)
    assert torch.all(big[:4] == SENTINEL) and torch.all(big[4 + n:] == SENTINEL)
    # buffers alone (memory=None) write the same buffers and nothing else
    big2 = big.clone()
    codec.params_mask(bufs, dev(values), torch.from_numpy(indices).to(DEV), ks, memory=None, lens=lens,
                      dtypes=[DTYPES[d] for d in dts])
    assert torch.equal(big2.view(torch.int32), big.view(torch.int32))


# the fixture layout without its zero-length tensor: the reference's k = max(1, ...) rule has no
# selection for an empty tensor, and the segmented top-k refuses one
E2E_KEEP = [0, 1, 3, 4, 5, 6, 7, 8, 9]


def _e2e_inputs(inputs):
    lens_all = inputs["lens"].tolist()
    off = _offs(lens_all)
    pick = np.concatenate([np.arange(off[s], off[s + 1]) for s in E2E_KEEP])
    lens = [lens_all[s] for s in E2E_KEEP]
    return lens, inputs["p0"][pick], [inputs[f"g{k}"][pick] for k in range(STEPS)]


@pytest.mark.parametrize("which", ["fixture", "small300"])
def test_compress_with_momentum_buffers_leaves_the_same_memory(inputs, which):
    """The fused mask launch against the separate sparse clear: the same selection and the same
    memory bits, with inf and NaN among the selected values (v + (-v) = NaN either way) and, on
    the 300-tensor layout, over more than one mask launch."""
    from chocosgd_amd import codec
    from chocosgd_amd.dgc import DGCCodec
    from chocosgd_amd.tensor_buffer import TensorBuffer
    rng = np.random.RandomState(8)
    if which == "fixture":
        lens, _, gs = _e2e_inputs(inputs)
        g = gs[0].copy()  # holds one inf and one NaN
    else:
        lens = rng.randint(1, 41, 300).tolist()
        g = rng.standard_normal(sum(lens)).astype(np.float32)
        g[[3, 1500, 4000]] = [np.inf, -np.inf, np.nan]
    n, nseg = sum(lens), len(lens)
    assert np.isinf(g).any() and np.isnan(g).any()
    mem0 = (rng.standard_normal(n) * 0.3).astype(np.float32)
    split = lambda a: [dev(a[o:o + m]) for o, m in zip(_offs(lens)[:-1], lens)]  # noqa: E731
    a, b = (DGCCodec(None, "compress_top_k", "gpu", 3, strict_reference=False) for _ in range(2))
    ma, mb = TensorBuffer(split(mem0)), TensorBuffer(split(mem0))
    va, ia, _ = a.compress(split(g), ma, 0.9)
    bufs = split(rng.standard_normal(n).astype(np.float32))
    bufs[2] = None
    c0 = _launches()
    vb, ib, _ = b.compress(split(g), mb, 0.9, momentum_buffers=bufs)
    assert (_launches() - c0)[4] == codec.params_mask_launches(nseg)
    assert codec.params_mask_launches(nseg) > 1 or which == "fixture"
    assert torch.equal(ia, ib) and same_bits(host(va), host(vb))
    sel_v = host(vb)
    assert (~np.isfinite(sel_v)).sum() >= 2, "no non-finite value was selected"
    assert same_bits(host(ma.buffer), host(mb.buffer))
    after = host(mb.buffer)[host(ib).astype(np.int64)]
    assert np.all(after[np.isfinite(sel_v)] == 0) and np.all(np.isnan(after[~np.isfinite(sel_v)]))


def test_run_refuses_a_threshold_without_norms():
    """A clip_threshold with no norms would train without clipping: refused, nothing launched."""
    from chocosgd_amd import codec
    p, g = torch.ones(8, device=DEV), torch.ones(8, device=DEV)
    plan = codec.ParamSgdPlan([p])
    codec.params_sqnorm([p], [g], 0.0, plan=plan)
    c0 = _launches()
    with pytest.raises(RuntimeError, match="norms"):
        plan.run(None, grad_mode=True, write=True, clip_threshold=1.0)
    assert (_launches() - c0).tolist() == [0, 0, 0, 0, 0] and torch.equal(g, torch.ones(8, device=DEV))


class _ThreeRanks:
    """all-gather stand-in: this rank's message between two made from it."""

    def _agg(self, data, op=None, communication_scheme="all_gather", **kw):
        K = data.numel() // 2
        v, idx = data[:K].view(torch.float32), data[K:]
        return [torch.cat([(v * 2).view(torch.int32), idx]), data, torch.cat([(v * -0.5).view(torch.int32), idx])]


@pytest.mark.parametrize("name", ["nesterov", "damp"])
def test_fused_step_end_to_end(inputs, name):
    """dgc.fused_step, 3 steps, against (a) the unfused sequence -- the per-tensor torch loop with
    the same norms, today's compress, a per-tensor torch masking loop, sync, recover_info, unpack
    -- and (b) the numpy model with O.topk_segmented for the selection."""
    from chocosgd_amd import codec, dgc, utils
    from chocosgd_amd.dgc import DGCCodec
    from chocosgd_amd.tensor_buffer import TensorBuffer
    fx = golden(f"dgc_sgd_{name}")
    hp = fx["hp"].tolist()
    lr, wd, mom, damp, nest = hp
    lens, p0, gs = _e2e_inputs(inputs)
    n, nseg = sum(lens), len(lens)
    off = _offs(lens)
    val, thr, ratio = float(inputs["clip_grad_val"]), float(inputs["thr"]), 0.9
    rng = np.random.RandomState(12)
    mem0 = (rng.standard_normal(n) * 0.3).astype(np.float32)

    def model():
        params = [torch.nn.Parameter(dev(p0[o:o + m])) for o, m in zip(off[:-1], lens)]
        groups = [{"params": [p], "lr": lr, "weight_decay": wd, "momentum": mom, "dampening": damp,
                   "nesterov": bool(nest), "name": f"p{i}"} for i, p in enumerate(params)]
        names = list(enumerate(g["name"] for g in groups))
        mem = TensorBuffer([dev(mem0[o:o + m]) for o, m in zip(off[:-1], lens)])
        cdc = DGCCodec(_ThreeRanks(), "compress_top_k", "gpu", 3, strict_reference=False)
        return params, groups, names, mem, cdc, collections.defaultdict(dict)

    pa, ga, na, ma, ca, sa = model()   # fused
    pb, gb, nb, mb, cb, sb = model()   # unfused
    p_m, mem_m, buf_m = p0.copy(), mem0.copy(), None
    for k in range(STEPS):
        _set_grads(pa, gs[k], lens)
        _set_grads(pb, gs[k], lens)
        # the norms the fused step will compute (the same call on the same data: the same bits)
        norms = codec.params_sqnorm([p.data for p in pa], [p.grad for p in pa], wd).clone()
        c0 = _launches()
        bits = dgc.fused_step(ca, ga, na, sa, ma, ratio, clip_grad=True, clip_grad_val=val, mask_momentum=True)
        got = (_launches() - c0).tolist()
        assert got[:3] == [codec.params_sqnorm_launches(nseg) - 1, 1, codec.params_sgd_launches(nseg)]
        assert got[4] == codec.params_mask_launches(nseg)
        # (a) unfused
        dgc.apply_gradient_loop(gb, sb, clip_grad=True, clip_grad_val=val, n_nodes=3, norms=norms)
        values, indices, bits_b = cb.compress([p.grad.data for p in pb], mb, ratio)
        for s, p in enumerate(pb):
            sel = indices[(indices >= int(off[s])) & (indices < int(off[s + 1]))].long() - int(off[s])
            nmask = torch.ones_like(p.data)
            nmask[sel] = 0.0
            sb[p]["momentum_buffer"].mul_(nmask)
        synced, size = cb.sync(values, indices)
        _, fp = utils.recover_params(gb, nb, get_hat_params=False)
        fp.buffer = cb.recover_info(fp.buffer, synced, size, lr)
        fp.unpack([p.data for p in pb])
        assert bits == bits_b
        for what, xa, xb in (("params", _cat(pa), _cat(pb)), ("memory", host(ma.buffer), host(mb.buffer)),
                             ("buffers", _cat([sa[p]["momentum_buffer"] for p in pa]),
                              _cat([sb[p]["momentum_buffer"] for p in pb]))):
            assert same_bits(xa, xb), f"{what} after step {k}: fused against unfused"
        # (b) the model
        _, buf_m, d = DO.step_layout(p_m, gs[k], buf_m, lens, hp, k == 0, host(norms), thr)
        with np.errstate(all="ignore"):
            mem_m = (mem_m + d).astype(np.float32)
            ov, oi, ks = O.topk_segmented(mem_m, lens, ratio)
            bufs = DO.split(buf_m, lens)
            bufs = [np.array(x, dtype=np.float32) for x in bufs]
            DO.mask(bufs, ["fp32"] * nseg, lens, ov, oi, ks, mem_m)
            buf_m = np.concatenate(bufs)
            total = np.zeros(n, dtype=np.float32)
            for f in (2.0, 1.0, -0.5):
                total[oi] = total[oi] + (ov * np.float32(f)).astype(np.float32)
            p_m = SO.fma32(np.float32(-lr), (total / np.float32(3)).astype(np.float32), p_m)
        assert same_bits(_cat(pa), p_m), f"params after step {k}: fused against the model"
        assert same_bits(host(ma.buffer), mem_m), f"memory after step {k}"
        assert same_bits(_cat([sa[p]["momentum_buffer"] for p in pa]), buf_m), f"buffers after step {k}"

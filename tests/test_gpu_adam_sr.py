"""Stochastic rounding for bf16 Adam on the device: codec.params_adam(sr=) (csrc/adam.hip,
param_adam_sr_kernel) and the layers above it (utils.apply_adam(rounding=),
utils.fused_step(state=, update="adam_sr", rounding=)).

The kernel is compared bit for bit against the numpy restatement of the header's lines and lanes
(tests/_adam_sr_oracle.py) on p, exp_avg, exp_avg_sq, flat and g -- whole guarded storages at a
time (test_gpu_param_sgd.py's), so that every byte a launch does not own is checked together with
the ones it does."""
import collections

import numpy as np
import pytest
import torch

from conftest import same_bits
import _adam_sr_oracle as ASO
import test_gpu_param_sgd as PS
from test_gpu_param_sgd import SENTINEL, Guarded, _values, host
from test_adam_sr_host import second_moment_experiment, small_update_experiment

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 54  # tensors per launch (adam.hip kAdamCap)
BF16, F32 = torch.bfloat16, torch.float32
NAMES = {BF16: "bf16", F32: "fp32"}
MODES = ["bf16", "mixed"]
BASE = [1, 2, 3, 7, 8, 9, 31, 33, 4097, 16, 8200, 20]
COEF = float(np.float32(0.37))
SR = (5, 12345)
KERNELS = ["param_adam_sr_kernel", "param_adam_kernel", "param_adam_master_kernel", "param_pack_kernel",
           "param_unpack_sr_kernel", "param_unpack_kernel"]


def _counts():
    from chocosgd_amd import codec
    return [codec.launch_count(k) for k in KERNELS]


def _launched(c0):
    return [b - a for a, b in zip(c0, _counts())]


def _dtypes(mode, k):
    """bf16, or bf16 and fp32 tensors alternating in one model."""
    return [F32 if mode == "fp32" or (mode == "mixed" and i % 2) else BF16 for i in range(k)]


def _varied_hp(i):
    """lr, beta1, beta2, eps, wd, step, decoupled differing inside one launch (test_gpu_adam.py's)."""
    return 1e-3 * (1 + i % 5), 0.4 if i % 3 == 1 else 0.9, 0.999, 1e-8, 0.0 if i % 4 == 2 else 0.01, 1 + i % 7, i % 2 == 0


def _abs(guarded):
    """exp_avg_sq is a sum of squares: the storages' magnitudes (the guards become +7)."""
    for s in guarded.stores:
        s.copy_(s.abs())
    guarded.before = [s.clone() for s in guarded.stores]
    return guarded


def run_case(lens, mode, lead=(0, 0, 0, 0), gap=8, own=False, flat_shift=4, nograd=(), hp=_varied_hp,
             first=lambda i: i % 2 == 0, write=True, coef=None, write_clipped=False, seed=1000, m_range=(-4, 0),
             v_range=(-7, 0), sr=SR):
    """One codec.params_adam(sr=) call on guarded storages against the restatement.  Returns what
    the call left in the tensors: per tensor (p, exp_avg, exp_avg_sq) and flat, on the host."""
    from chocosgd_amd import codec
    k, n = len(lens), sum(lens)
    dts = _dtypes(mode, k)
    P = Guarded(lens, dts, seed, -3, 1, lead[0], gap, own)
    G = Guarded(lens, dts, seed + 5000, -4, 0, lead[1], gap, own)
    M = Guarded(lens, dts, seed + 9000, *m_range, lead[2], gap, own)
    V = _abs(Guarded(lens, dts, seed + 13000, *v_range, lead[3], gap, own))
    hps = [hp(i) for i in range(k)]
    firsts = [bool(first(i)) for i in range(k)]
    big = flat = None
    if flat_shift is not None:
        big = torch.full((n + 2 * flat_shift + 8,), SENTINEL, device=DEV)
        flat = big[flat_shift:flat_shift + n]
    gclip = None if coef is None else torch.tensor([1.0, coef], device=DEV)
    new_p, new_g, new_m, new_v, new_flat = [], [], [], [], []
    o = 0
    for i in range(k):
        pw, gw, mw, vw = host(P.views[i]), host(G.views[i]), host(M.views[i]), host(V.views[i])
        start, o = o, o + lens[i]
        if i in nograd:
            new_p.append(None), new_g.append(None), new_m.append(None), new_v.append(None)
            new_flat.append(pw)
            continue
        lr, b1, b2, eps, wd, step, dec = hps[i]
        p_new, m_new, v_new, g_c, x_new = ASO.adam_sr_step(pw, gw, mw, vw, lr, b1, b2, eps, wd, step, dec, firsts[i], coef,
                                                           dtype=NAMES[dts[i]], seed=sr[0], sr_step=sr[1], start=start)
        new_p.append(p_new if write else None)
        new_g.append(g_c if write_clipped else None)
        new_m.append(m_new)
        new_v.append(v_new)
        new_flat.append(x_new)
    c0 = _counts()
    codec.params_adam(P.views, [None if i in nograd else g for i, g in enumerate(G.views)], M.views, V.views,
                      [h[0] for h in hps], [(h[1], h[2]) for h in hps], [h[3] for h in hps], [h[4] for h in hps],
                      [h[5] for h in hps], [h[6] for h in hps], firsts, flat=flat, write=write, gclip=gclip,
                      write_clipped=write_clipped, sr=sr)
    assert _launched(c0) == [codec.params_adam_launches(k), 0, 0, 0, 0, 0]
    P.check(new_p, "params (or their guards)")
    G.check(new_g, "grads (or their guards)")
    M.check(new_m, "exp_avg (or its guards)")
    V.check(new_v, "exp_avg_sq (or its guards)")
    if flat is not None:
        want = torch.full_like(big, SENTINEL)
        if n:
            want[flat_shift:flat_shift + n] = torch.from_numpy(np.concatenate(new_flat).astype(np.float32)).to(DEV)
        assert same_bits(host(big), host(want)), "flat (or its guards)"
    for i in range(k):  # a second moment never becomes negative
        vi = host(V.views[i])
        assert not np.any(np.signbit(vi) & ~np.isnan(vi)), i
    return ([(host(P.views[i]), host(M.views[i]), host(V.views[i])) for i in range(k)],
            None if flat is None else host(flat))


@pytest.mark.parametrize("mode", MODES)
def test_cut_groups_and_tile_crossings(mode):
    """One storage per dtype, every tensor eight elements further in than its flat offset: the
    16-byte path with cut groups at both ends (bf16), FIRST on every other tensor, then on none
    and on all; a tensor across four tiles, in one storage and alone."""
    run_case(BASE, mode)
    run_case(BASE, mode, first=lambda i: False, coef=COEF)
    run_case(BASE, mode, first=lambda i: True, coef=COEF, write_clipped=True)
    run_case([100, 3 * 8192 + 5, 50], mode, first=lambda i: False)
    run_case([3 * 8192 + 5], "bf16", own=True, first=lambda i: True, coef=COEF)


@pytest.mark.parametrize("which", range(4))
@pytest.mark.parametrize("mode", MODES)
def test_views_at_every_offset_of_a_group(mode, which):
    """p, g, m or v alone 1 to 7 elements into its allocation, the other three aligned (each
    tensor its own allocation, every flat offset a multiple of 8): the shifted layouts take the
    element path, the aligned one the 16-byte path, and both store the same bits for the same
    flat index -- the bit fields are a function of the flat index alone."""
    lens = [40, 8192 + 24, 7]
    kw = dict(own=True, first=lambda i: i == 2)
    aligned = {c: run_case(lens, mode, coef=c, **kw) for c in (None, COEF)}
    for off in range(1, 8):
        lead = [0, 0, 0, 0]
        lead[which] = off
        c = COEF if off % 2 else None
        got = run_case(lens, mode, lead=tuple(lead), coef=c, write_clipped=off == 3, **kw)
        for (a, b) in zip(got[0], aligned[c][0]):
            assert all(same_bits(x, y) for x, y in zip(a, b)), (off, "the element path against the 16-byte path")
        assert same_bits(got[1], aligned[c][1])


@pytest.mark.parametrize("mode", MODES)
def test_views_at_element_alignment(mode):
    for gap in (1, 2, 3):
        run_case(BASE, mode, lead=(1, 1, 1, 1), gap=gap)


@pytest.mark.parametrize("count", [CAP + 1, 2 * CAP + 1])
def test_chunk_boundaries_inside_a_tile(count):
    """55 and 109 tensors of 1 to 13 elements: the chunk boundaries at 54 (and 108) fall inside
    one tile, and the launch count is params_adam_launches (run_case asserts it)."""
    from chocosgd_amd import codec
    assert codec.params_adam_launches(count) == -(-count // CAP)
    lens = [1 + i % 13 for i in range(count)]
    run_case(lens, "mixed")
    run_case(lens, "bf16", first=lambda i: False)


@pytest.mark.parametrize("mode", MODES)
def test_zero_length_and_no_grad_tensors(mode):
    run_case([0, 5, 0, 0, 4100, 0], mode)
    run_case([0, 5, 0, 0, 4100, 0], mode, nograd=(1,))
    # a tensor without a gradient between two updated ones: packed as it is, not written
    run_case([300, 8195, 40, 9000, 7], mode, nograd=(1, 2))
    run_case([300, 8195, 40], mode, nograd=(1,), write=False, coef=COEF)


@pytest.mark.parametrize("mode", MODES)
def test_flat_alignment_and_no_flat(mode):
    run_case(BASE, mode, flat_shift=1)  # flat at 4-byte alignment: elementwise
    run_case(BASE, mode, flat_shift=None)  # no flat side: params only
    run_case([8192 * 2 + 8, 30, 64], mode, flat_shift=None, own=True, nograd=(1,), coef=COEF, write_clipped=True)


@pytest.mark.parametrize("mode", MODES)
def test_write_off_leaves_params_alone_and_updates_the_moments(mode):
    """run_case compares whole storages: with write off the parameters must come back
    bit-identical (the CHOCO form: flat receives the unrounded p_new), while exp_avg and
    exp_avg_sq are rounded and stored."""
    run_case(BASE, mode, write=False)
    run_case([8192 + 16, 64], mode, write=False, own=True, coef=COEF)


@pytest.mark.parametrize("mode", MODES)
def test_uniform_hyperparameter_sets(mode):
    """AdamW's and Adam's decay and none, both branches of the lerp, the first step and a late
    one, with and without the clip coefficient."""
    for wd, dec in [(0.01, True), (1e-4, False), (0.0, False)]:
        for b1 in (0.9, 0.4):
            for fst, step in ((True, 1), (False, 1000)):
                run_case([33, 8195], mode, hp=lambda i: (3e-4, b1, 0.999, 1e-8, wd, step, dec), first=lambda i: fst,
                         coef=COEF if fst else None)


def test_fp32_tensors_are_the_plain_kernel_s():
    """A mixed model through params_adam(sr=) and through params_adam: the fp32 tensors' p,
    exp_avg, exp_avg_sq and flat slices are equal bit for bit (and the bf16 ones are not)."""
    from chocosgd_amd import codec
    lens, dts = [40, 8192 + 24, 7, 4099], [BF16, F32, F32, BF16]
    out = []
    for sr in (SR, None):
        t = [[torch.from_numpy(_values(m, 50 * j + i, -3, 0)).to(DEV).to(dt) for i, (m, dt) in enumerate(zip(lens, dts))]
             for j in range(4)]
        t[3] = [x.abs() for x in t[3]]
        flat = torch.empty(sum(lens), device=DEV)
        gclip = torch.tensor([1.0, COEF], device=DEV)
        codec.params_adam(*t, 1e-3, weight_decay=0.01, step=3, decoupled=True, flat=flat, gclip=gclip, sr=sr)
        out.append((t, host(flat)))
    o = 0
    for i, (m, dt) in enumerate(zip(lens, dts)):
        same = [same_bits(host(out[0][0][j][i]), host(out[1][0][j][i])) for j in (0, 2, 3)]
        same.append(same_bits(out[0][1][o:o + m], out[1][1][o:o + m]))
        assert all(same) if dt == F32 else not any(same), (i, same)
        o += m


def test_fp16_is_refused_with_nothing_launched():
    from chocosgd_amd import codec
    t = [[torch.ones(8, device=DEV, dtype=dt) for dt in (BF16, torch.float16)] for _ in range(4)]
    c0 = _counts()
    with pytest.raises(RuntimeError, match="tensor 1: fp16"):
        codec.params_adam(*t, 1e-3, sr=SR)
    assert _launched(c0) == [0] * len(KERNELS)
    assert all(float(x.float().sum()) == 8.0 for col in t for x in col)


# +-0, +-inf, NaN, bf16 denormals (the smallest and the largest), the largest finite bf16 and its
# negative, and ordinary values; every one is exact in bf16
EDGE = np.array([0x0000, 0x8000, 0x7F80, 0xFF80, 0x7FC0, 0x0001, 0x8001, 0x007F, 0x7F7F, 0xFF7F, 0x3F80, 0xBF81, 0x3C00,
                 0x0080], dtype=np.uint32)


def _edge(m, shift):
    """m bf16 values cycling through EDGE from position `shift`, as fp32 on the host."""
    idx = (np.arange(m) * (2 * shift + 1) + shift) % EDGE.size
    return (EDGE[idx] << 16).view(np.float32)


@pytest.mark.parametrize("first", [False, True])
def test_special_values(first):
    """+-0, +-inf, NaN, denormals and the largest finite bf16 in p, g, m and v, each cycling at
    its own stride so that the combinations meet, on the 16-byte path and on the element path;
    then _values' specials sprinkled over wide exponent ranges.  The expectations are the
    restatement's (sr_narrow_bf16's rules: inf kept, NaN -> the quiet NaN, +-0 and denormals as
    any other value, a finite p_new above the largest finite bf16 may round to inf)."""
    from chocosgd_amd import codec
    m = 8192 + 9
    hp = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, step=2, decoupled=True)
    for lead in (0, 3):
        cols = [_edge(m, s) for s in range(4)]
        cols[3] = np.abs(cols[3])
        store = [torch.zeros(m + 8, device=DEV, dtype=BF16) for _ in range(4)]
        t = [s[lead:lead + m] for s in store]
        for x, c in zip(t, cols):
            x.copy_(torch.from_numpy(c).to(DEV))
        flat = torch.empty(m, device=DEV)
        want = ASO.adam_sr_step(*cols, 1e-3, wd=0.01, step=2, decoupled=True, first=first, seed=SR[0], sr_step=SR[1])
        codec.params_adam([t[0]], [t[1]], [t[2]], [t[3]], first=first, flat=flat, sr=SR, **hp)
        assert same_bits(host(t[0]), want[0]) and same_bits(host(t[2]), want[1]) and same_bits(host(t[3]), want[2])
        assert same_bits(host(flat), want[4]) and same_bits(host(t[1]), cols[1])
        v = host(t[3])
        assert not np.any(np.signbit(v) & ~np.isnan(v)), "a second moment became negative"
        assert np.isnan(want[0]).any() and np.isinf(want[0]).any() and np.isfinite(want[0]).any()
    run_case([4099, 70], "bf16", first=lambda i: first, m_range=(-30, 30), v_range=(-38, 30))
    run_case([4099, 70], "mixed", first=lambda i: first, coef=COEF, write_clipped=True, v_range=(-45, -20),
             hp=lambda i: (1e-3, 0.9 if i else 0.4, 0.999, 0.0, 0.01, 3, i == 0))


# ----------------------------------------------------------------------------- through utils
def _finite(m, seed, lo, hi):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal(m) * 10.0 ** rng.uniform(lo, hi, m)).astype(np.float32)


def _model(lens, dev, seed=5):
    dts = _dtypes("mixed", len(lens))
    params = [torch.nn.Parameter(torch.from_numpy(_finite(m, seed + i, -2, 0)).to(dev).to(dt))
              for i, (m, dt) in enumerate(zip(lens, dts))]
    groups = []
    for i, p in enumerate(params):
        lr, b1, b2, eps, wd, _, dec = _varied_hp(i)
        groups.append({"params": [p], "name": f"p{i}", "lr": lr, "betas": (b1, b2), "eps": eps, "weight_decay": wd,
                       "decoupled_weight_decay": dec, "amsgrad": False, "maximize": False, "capturable": False,
                       "differentiable": False, "foreach": None, "fused": None})
    return params, groups


def _grads(params, step, nograd=()):
    for i, p in enumerate(params):
        g = torch.from_numpy(_finite(p.numel(), 100 * step + i, -3, -1)).to(p.device).to(p.dtype)
        p.grad = None if i in nograd else g


def test_three_steps_through_apply_adam_are_the_cpu_loop():
    """A small mixed model, one tensor without a gradient, three steps of apply_adam(rounding=)
    on the device against apply_adam_sr_loop on a CPU copy: params, moments, step counts and the
    flat output bit for bit; params_adam_launches(k) launches of the sr kernel per step and
    nothing else; the stream advanced once per step."""
    from chocosgd_amd import codec, utils
    lens, nograd = [5, 8200, 33, 4097, 64, 1], (2,)
    pd, gd = _model(lens, DEV)
    pc, gc = _model(lens, "cpu")
    sd, sc = collections.defaultdict(dict), collections.defaultdict(dict)
    fd, fc = torch.full((sum(lens),), SENTINEL, device=DEV), torch.full((sum(lens),), SENTINEL)
    sr = utils.StochasticRounding(SR[0], SR[1])
    for k in range(3):
        _grads(pd, k, nograd)
        _grads(pc, k, nograd)
        c0 = _counts()
        utils.apply_adam(gd, sd, flat_out=fd, rounding=sr)
        assert _launched(c0) == [codec.params_adam_launches(len(lens)), 0, 0, 0, 0, 0]
        assert sr.state_dict() == {"seed": SR[0], "step": SR[1] + k + 1}
        utils.apply_adam_sr_loop(gc, sc, SR[0], SR[1] + k, flat=fc)
        for i, (a, b) in enumerate(zip(pd, pc)):
            assert same_bits(host(a), host(b)), (k, i, "p")
            if i in nograd:
                assert a not in sd
                continue
            for key in ("exp_avg", "exp_avg_sq"):
                assert sd[a][key].dtype == a.dtype and same_bits(host(sd[a][key]), host(sc[b][key])), (k, i, key)
            assert float(sd[a]["step"]) == k + 1 and not sd[a]["step"].is_cuda
        assert same_bits(host(fd), host(fc)), (k, "flat")
    assert float(((host(fd).view(np.uint32) & 0xFFFF) != 0).mean()) > 0.3, "flat is unrounded"


@pytest.mark.parametrize("op", ["compress_top_k", "sign"])
def test_fused_step_is_the_update_then_todays_step_then_the_rounding_unpack(op):
    """One rank looped back on itself, a mixed bf16 / fp32 model.  (a) fused_step(update="adam_sr",
    rounding=sr).  (b) the sr update with the parameters not written and flat receiving p_new,
    today's fused_step on an fp32 model holding exactly that flat x, and unpack(rounding=) of the
    x it ends with, all with (a)'s (seed, step).  Parameters, moments, x, x_hat, memory and the
    message are equal bit for bit; (a) stores each parameter once, in the unpack, and advances the
    stream by exactly one."""
    from chocosgd_amd import utils
    from chocosgd_amd.parallel_choco import CHOCOCompressor
    from chocosgd_amd.tensor_buffer import TensorBuffer
    lens = [37, 4096, 5, 8195, 260]
    n = sum(lens)
    shapes = [(torch.Size([m]), m) for m in lens]
    sizes = [(m,) for m in lens]

    def setup():
        params, groups = _model(lens, DEV)
        _grads(params, 0)
        g = torch.Generator(device=DEV).manual_seed(21)
        hat = torch.cat([p.detach().float() for p in params]) + 0.1 * torch.randn(n, generator=g, device=DEV)
        mem = hat + 0.05 * torch.randn(n, generator=g, device=DEV)
        nhp = {0: TensorBuffer.from_flat(hat, sizes), "memory": TensorBuffer.from_flat(mem, sizes)}
        comp = CHOCOCompressor(aggregator=PS._Loopback(), comm_op=op, comm_device="gpu", compress_ratio=0.9,
                               quantize_level=4, is_biased=False, backend="nccl", use_ipc=False)
        return params, groups, list(enumerate(gr["name"] for gr in groups)), nhp, comp

    # (a)
    pa, ga, names, nhp_a, comp_a = setup()
    before = [p.detach().clone() for p in pa]
    sa = collections.defaultdict(dict)
    sr = utils.StochasticRounding(*SR)
    torch.manual_seed(1234)
    c0 = _counts()
    sb_a = utils.fused_step(comp_a, ga, names, shapes, nhp_a, {0: 1.0}, PS.GAMMA, 0, state=sa, update="adam_sr",
                            rounding=sr)
    assert _launched(c0) == [1, 0, 0, 0, 1, 0], "the sr update, the sr unpack, and no pack"
    assert sr.state_dict() == {"seed": SR[0], "step": SR[1] + 1}
    # (b)
    pb, gb, _, nhp_b, comp_b = setup()
    sb = collections.defaultdict(dict)
    entries = [(g, g["params"][0]) for g in gb]
    hps = [utils._adam_hp("test", g) for g in gb]
    x = torch.empty(n, device=DEV)
    assert utils._adam_batched("test", entries, hps, sb, x, None, False, None, sr=SR)
    assert all(same_bits(host(p), host(q)) for p, q in zip(pb, before)), "the update wrote a parameter"
    p32 = [torch.nn.Parameter(x[sum(lens[:i]):sum(lens[:i + 1])].clone()) for i in range(len(lens))]
    g32 = [{"params": [p], "name": f"p{i}"} for i, p in enumerate(p32)]
    torch.manual_seed(1234)
    sb_b = utils.fused_step(comp_b, g32, names, shapes, nhp_b, {0: 1.0}, PS.GAMMA, 0)
    sb_b["flatten_params"].unpack([p.data for p in pb], rounding=SR)
    xa, xb = host(sb_a["flatten_params"].buffer), host(sb_b["flatten_params"].buffer)
    assert same_bits(xa, xb) and same_bits(xb, np.concatenate([host(p) for p in p32])), "x"
    msg = [PS._MESSAGE[op](s).contiguous().view(torch.uint8).cpu().numpy() for s in (sb_a, sb_b)]
    assert msg[0].size > 0 and np.array_equal(*msg), "the message"
    assert same_bits(host(nhp_a[0].buffer), host(nhp_b[0].buffer)), "x_hat"
    assert same_bits(host(nhp_a["memory"].buffer), host(nhp_b["memory"].buffer)), "memory"
    o = 0
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert same_bits(host(a), host(b)), (i, "p")
        for key in ("exp_avg", "exp_avg_sq"):
            assert same_bits(host(sa[a][key]), host(sb[b][key])), (i, key)
        if a.dtype == BF16:  # the ONE store: lane 0 of the flat index, on the x the step ended with
            want = utils.sr_narrow_bf16(torch.from_numpy(xa[o:o + lens[i]]), utils.sr_bits(*SR, o, lens[i]))
            assert same_bits(host(a), host(want)) and not same_bits(host(a), host(before[i])), i
        o += lens[i]
    assert float(((xa.view(np.uint32) & 0xFFFF) != 0).mean()) > 0.5, "the flat x was never rounded"


# ----------------------------------------------------------------------------- what it is for
def test_the_second_moment_decays_on_the_device():
    """test_adam_sr_host.py's experiment and bound, 200 launches of one workgroup each."""
    plain, rounded = second_moment_experiment(DEV)
    assert torch.equal(plain, torch.ones(4096, dtype=torch.float64)), "the stall this feature is for"
    mean, want = float(rounded.mean()), 0.999 ** 200
    print(f"mean of v after 200 steps: {mean:.5f} (0.999^200 = {want:.5f})")
    assert abs(mean - want) <= 0.01 * want, mean


def test_small_updates_survive_on_the_device():
    """test_adam_sr_host.py's experiment and bound (its docstring derives the 5 %)."""
    plain, rounded, ref = small_update_experiment(DEV)
    assert torch.equal(plain, torch.ones(4096, dtype=torch.float64)), "the stall this feature is for"
    moved, want = 1.0 - float(rounded.mean()), 1.0 - ref
    print(f"mean displacement after 200 steps: {moved:.6f} (fp32: {want:.6f})")
    assert abs(moved - want) <= 0.05 * want, moved

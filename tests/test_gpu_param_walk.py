"""The tile walk, the 16-byte rule, the span walk and the host's chunk loop that every kernel
walking a table of parameter tensors shares (csrc/param_common.h), pinned under each of them on
one small set of layouts -- the smallest at which the walk can go wrong:

    cross<L>  one tensor of L = 8191, 8192, 8193, 16385 elements behind a 3-element one, on the
              16-byte grid: it crosses one or two ends of the 8192-element tiles, with cut groups
              at both of its ends
    chunk     cap + 1 tensors of 0 to 9 elements (the kernel's own cap): two launches whose chunk
              boundary falls inside a tile, zero-length tensors among them
    offgrid   a view one element off the grid between two congruent ones (gap 1: tensor 1 starts
              one element late, six empty tensors bring tensor 8 back onto the grid)
    flat4     every tensor on the grid, the flat buffer(s) only 4-byte aligned

in fp32 and bf16, bit for bit against the oracles of the kernels' own tests (whose helpers are
imported, not copied), guards around every view and flat buffer included."""
import collections

import numpy as np
import pytest
import torch

import _dgc_oracle as DO
import _ef_oracle as EO
import _mix_oracle as MO
import test_gpu_allreduce_scaled as ARS
import test_gpu_consensus as CN
import test_gpu_dgc_sgd as DGC
import test_gpu_param_mix as MIX
import test_gpu_param_sgd as PS
import test_gpu_params_ef as EF

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = PS.SENTINEL
host = PS.host

Layout = collections.namedtuple("Layout", "lens lead gap own flat_shift")
LAYOUTS = ["cross8191", "cross8192", "cross8193", "cross16385", "chunk", "offgrid", "flat4"]
both_dtypes = pytest.mark.parametrize("mode", ["fp32", "bf16"])
every_layout = pytest.mark.parametrize("name", LAYOUTS)


def layout(name, cap):
    """PS.Guarded's arguments for layout `name` under a kernel of `cap` tensors per launch.  Views
    of one storage `gap` = 8 elements apart are congruent with the group grid in both dtypes."""
    if name.startswith("cross"):
        return Layout([3, int(name[5:]), 5], 0, 8, False, 4)
    if name == "chunk":
        return Layout([i % 10 for i in range(cap + 1)], 0, 8, False, 4)
    if name == "offgrid":
        return Layout([40, 8200] + [0] * 6 + [300], 0, 1, False, 4)
    return Layout([40, 8200, 304], 0, 8, True, 1)


def guarded(L, mode, seed, lo=-3, hi=1):
    return PS.Guarded(L.lens, PS._dtypes(mode, len(L.lens)), seed, lo, hi, L.lead, L.gap, L.own)


def flat_values(lens, seed, lo=-2, hi=1):
    return np.concatenate([PS._values(m, seed + i, lo, hi) for i, m in enumerate(lens)])


def cat(views):
    return np.concatenate([host(v) for v in views])


def plan_of(views):
    from chocosgd_amd import codec
    plan = codec.ParamSgdPlan(views)
    for i, v in enumerate(views):
        plan.param_ptrs[i] = v.data_ptr()
    return plan


def launched(kernel, c0=None):
    from chocosgd_amd import codec
    return codec.launch_count(kernel) - (c0 or 0)


@every_layout
@both_dtypes
def test_pack_and_unpack(name, mode):
    from chocosgd_amd import codec
    L = layout(name, 192)
    k, n = len(L.lens), sum(L.lens)
    G = guarded(L, mode, 100)
    want = cat(G.views)
    big, flat = CN._guarded_flat(np.full(n, SENTINEL, np.float32), L.flat_shift)
    c0 = launched("param_pack_kernel")
    codec.params_pack(G.views, flat)
    assert launched("param_pack_kernel", c0) == codec.params_launches(k) == -(-k // 192)
    CN._check_flat(big, L.flat_shift, want, "pack: flat (or its guards)")
    G.check([None] * k, "pack wrote to its sources")
    # values off every 16-bit grid and past fp16's range; Guarded.expected narrows as torch does
    src = flat_values(L.lens, 7000, -7, 5)
    big, flat = CN._guarded_flat(src, L.flat_shift)
    c0 = launched("param_unpack_kernel")
    codec.params_unpack(flat, G.views)
    assert launched("param_unpack_kernel", c0) == codec.params_launches(k)
    CN._check_flat(big, L.flat_shift, src, "unpack wrote to the flat buffer")
    G.check(CN._pieces(src, L.lens), "unpack: the tensors (or their guards)")


@every_layout
@both_dtypes
def test_scaled_pack(name, mode):
    L = layout(name, 192)
    for rnd in (True, False):
        ARS.run_pack(L.lens, mode, found=1.0, round=rnd, lead=L.lead, gap=L.gap, own=L.own, flat_shift=L.flat_shift)


@pytest.mark.parametrize("ef_mode", [EO.ACCUM, EO.APPLY | EO.DIV | EO.SCALE], ids=["accum", "apply_div_scale"])
@every_layout
@both_dtypes
def test_ef(name, mode, ef_mode):
    from chocosgd_amd import codec
    L = layout(name, 128)
    k = len(L.lens)
    P = guarded(L, mode, 200, -2, 1)
    f = flat_values(L.lens, 9000)
    big, flat = CN._guarded_flat(f, L.flat_shift)
    want = [EO.ef(ef_mode, fs, host(v), EF.LR, EF.DIVISOR, mode) for fs, v in zip(CN._pieces(f, L.lens), P.views)]
    c0 = launched("param_ef_kernel")
    plan_of(P.views).ef(flat, ef_mode, lr=EF.LR, divisor=EF.DIVISOR)
    assert launched("param_ef_kernel", c0) == codec.params_ef_launches(k) == -(-k // 128)
    P.check([w[0] for w in want], "params (or their guards)")
    CN._check_flat(big, L.flat_shift, np.concatenate([w[1] for w in want]), "flat (or its guards)")


@every_layout
@both_dtypes
def test_mix_write_params(name, mode):
    from chocosgd_amd import codec
    L = layout(name, 128)
    k = len(L.lens)
    P = guarded(L, mode, 300)
    weights = [0.5, 0.0, 1.0 / 3]
    srcs_np = [flat_values(L.lens, 500 + 1000 * r) for r in range(3)]
    srcs = [CN._guarded_flat(s, L.flat_shift) for s in srcs_np]
    _, p_new, _ = MO.mix(srcs_np, weights, dtype=mode)
    c0 = launched("param_mix_kernel")
    plan_of(P.views).mix([v for _, v in srcs], weights, mode=MIX.WRITE)
    assert launched("param_mix_kernel", c0) == codec.params_mix_launches(k, 3) == -(-k // 128)
    P.check(CN._pieces(p_new, L.lens), "params (or their guards)")
    for r, (big, _) in enumerate(srcs):
        CN._check_flat(big, L.flat_shift, srcs_np[r], f"source {r} was written")


@every_layout
@both_dtypes
def test_consensus_dist_and_write_avg(name, mode):
    L = layout(name, CN.CAP)
    assert CN.CAP == 128
    CN.both(L.lens, mode, lead=(L.lead, L.lead), gap=L.gap, own=L.own, xsum_shift=L.flat_shift)


@every_layout
@both_dtypes
def test_sqnorm(name, mode):
    from chocosgd_amd import codec
    L = layout(name, 112)
    k = len(L.lens)
    P, G = guarded(L, mode, 600, -2, 1), guarded(L, mode, 700, -3, 0)
    CN._tame_guarded(P)  # finite norms: every bit of them is compared
    CN._tame_guarded(G)
    p, g = cat(P.views), cat(G.views)
    plan = codec.ParamSgdPlan(P.views)
    for wd in (0.0, 1e-2):
        c0 = launched("param_sqnorm_kernel")
        got = host(codec.params_sqnorm(P.views, G.views, wd, plan=plan).clone())
        assert launched("param_sqnorm_kernel", c0) + 1 == codec.params_sqnorm_launches(k) == -(-k // 112) + 1
        assert np.isfinite(got).all()
        DGC._check_norms(got, p, g, L.lens, wd, mode)
    P.check([None] * k, "the norm pass wrote to the params")
    G.check([None] * k, "the norm pass wrote to the grads")


@every_layout
@both_dtypes
def test_mask(name, mode):
    """The slot walk: 2048 slots per workgroup, so at ratio 0.75 the crossing tensors hold 2047,
    2048, 2048 and 4096 slots behind the first tensor's one."""
    from chocosgd_amd import codec
    L = layout(name, 128)
    k = len(L.lens)
    x = flat_values(L.lens, 800)
    values, indices, ks = DGC._selection(x, L.lens, 0.75)
    B = guarded(L, mode, 900)
    model = [host(v).copy() for v in B.views]
    big, memory = CN._guarded_flat(x, L.flat_shift)
    mem_model = x.copy()
    DO.mask(model, [mode] * k, L.lens, values, indices, ks, mem_model)
    c0 = launched("param_mask_kernel")
    codec.params_mask(B.views, DGC.dev(values), torch.from_numpy(indices).to(DEV), ks, memory=memory)
    assert launched("param_mask_kernel", c0) == codec.params_mask_launches(k) == -(-k // 128)
    B.check(model, "the buffers (or their guards)")
    CN._check_flat(big, L.flat_shift, mem_model, "memory (or its guards)")

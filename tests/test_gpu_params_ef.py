"""choco_params_ef and choco_sign_local_residual on the device against the numpy model
(tests/_ef_oracle.py), bit for bit.  Everything is compared as bit patterns over whole storages,
so that every byte a launch does not own is checked together with the ones it does."""
import numpy as np
import pytest
import torch

from conftest import same_bits
import _ef_oracle as EO
import _sgd_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
SENTINEL = -7.0  # exact in every dtype
GAP = 64  # elements between two views of a storage: 64 * esz is a multiple of 16 bytes
# tensors across the 8192 tile edge, cut groups of 8, a zero-length tensor
LENS = [5, 1, 0, 8195, 33, 4099, 17000, 40, 40, 1]
LR, DIVISOR = 0.1, 3.0
# offsets into the 8195-element tensor
NEG_ZERO, INF_FLAT, NAN_PARAM, NAN_FLAT, INF_PARAM, SUB_PRODUCT, SUB_QUOTIENT, OPPOSITE_INF = 11, 20, 21, 22, 23, 30, 31, 40


def host(t):
    return t.detach().float().cpu().numpy()


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(dtype)


def _offs(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


class Views:
    """Tensors as views packed one behind the other into ONE storage per dtype: view s starts at
    element GAP * (s + 1) + off_s + shift, so with shift 0 every view is congruent with the
    16-byte group grid of the flat layout (the vector path) and with shift 1 none is (the element
    path); everything between is sentinel.  dtypes: one name, or one per tensor (a mixed table)."""

    def __init__(self, flat, lens, dtypes, shift=0):
        self.lens = list(lens)
        self.dtypes = [dtypes] * len(lens) if isinstance(dtypes, str) else list(dtypes)
        off = _offs(lens)
        self.starts = [GAP * (s + 1) + int(off[s]) + shift for s in range(len(lens))]
        self.total = GAP * (len(lens) + 2) + int(off[-1])
        self.stores = {d: torch.full((self.total,), SENTINEL, device=DEV, dtype=DTYPES[d]) for d in set(self.dtypes)}
        self.views = [self.stores[d][a:a + m] for d, a, m in zip(self.dtypes, self.starts, lens)]
        o = 0
        for v, m in zip(self.views, self.lens):
            v.copy_(dev(flat[o:o + m], v.dtype))
            o += m

    def grid(self, flat):
        """flat with every tensor's span on its dtype's grid."""
        out, o = np.array(flat, dtype=np.float32), 0
        for d, m in zip(self.dtypes, self.lens):
            out[o:o + m] = SO.to_grid(out[o:o + m], d)
            o += m
        return out

    def pairs(self, tag, flat):
        """{name: (the whole storage, what it must hold with `flat` in the views)} per dtype."""
        out = {}
        for d, store in self.stores.items():
            want, o = np.full(self.total, SENTINEL, dtype=np.float32), 0
            for dd, a, m in zip(self.dtypes, self.starts, self.lens):
                if dd == d:
                    want[a:a + m] = flat[o:o + m]
                o += m
            out[f"{tag} {d} storage"] = (host(store), want)
        return out


class Flat:
    """A flat fp32 buffer of n elements inside a sentinel storage: 16-byte aligned with shift 0,
    starting 4 bytes later with shift 1."""

    def __init__(self, n, values=None, shift=0):
        self.n, self.a = n, 4 + shift
        self.store = torch.full((n + 12,), SENTINEL, device=DEV)
        self.t = self.store[self.a:self.a + n]
        if values is not None:
            self.t.copy_(dev(values))

    def expect(self, values):
        out = np.full(self.n + 12, SENTINEL, dtype=np.float32)
        out[self.a:self.a + self.n] = values
        return out

    def all(self):
        return host(self.store)


def _inputs(lens, seed=7):
    """(params, flat) with the special values planted in the 8195-element tensor when there is one."""
    rng = np.random.RandomState(seed)
    n = int(sum(lens))
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 1, n)).astype(np.float32)
    f = (rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 1, n)).astype(np.float32)
    if 8195 in lens:
        o = int(_offs(lens)[lens.index(8195)])
        x[o + NEG_ZERO], f[o + NEG_ZERO] = -0.0, 0.0          # (-0) + (+0) = +0
        f[o + INF_FLAT], x[o + NAN_PARAM], f[o + NAN_FLAT], x[o + INF_PARAM] = np.inf, np.nan, np.nan, -np.inf
        x[o + SUB_PRODUCT], f[o + SUB_PRODUCT] = 0.0, 6.0e-38    # -lr * f and -lr * (f / 3) are subnormal
        x[o + SUB_QUOTIENT], f[o + SUB_QUOTIENT] = 0.0, 2.0e-38  # f / 3 is subnormal
        x[o + OPPOSITE_INF], f[o + OPPOSITE_INF] = np.inf, -np.inf  # inf - inf = NaN in APPLY
    return x, f


def _run_modes(lens, dtypes, view_shift, flat_shift, seed=7):
    """Every mode on one layout against the numpy model: {name: (got, want)} of whole storages."""
    from chocosgd_amd import codec
    x_raw, f = _inputs(lens, seed)
    n, nseg = int(sum(lens)), len(lens)
    out = {}
    for mode in EO.MODES:
        pv = Views(x_raw, lens, dtypes, view_shift)
        x = pv.grid(x_raw)
        fl = Flat(n, f, flat_shift)
        plan = codec.ParamSgdPlan(pv.views)
        for i, p in enumerate(pv.views):
            plan.param_ptrs[i] = p.data_ptr()
        c0 = codec.launch_count("param_ef_kernel")
        plan.ef(fl.t, mode, lr=LR, divisor=DIVISOR)
        assert codec.launch_count("param_ef_kernel") - c0 == codec.params_ef_launches(nseg)
        want_p, want_f, o = np.empty(n, np.float32), np.empty(n, np.float32), 0
        for d, m in zip(pv.dtypes, lens):
            want_p[o:o + m], want_f[o:o + m] = EO.ef(mode, f[o:o + m], x[o:o + m], LR, DIVISOR, d)
            o += m
        out.update(pv.pairs(f"mode {mode} params", want_p))
        out[f"mode {mode} flat"] = (fl.all(), fl.expect(want_f))
    return out


def _assert_all(pairs):
    for what, (got, want) in pairs.items():
        assert same_bits(got, want), what


MIXED = ["fp32", "bf16", "fp16", "bf16", "fp32", "fp16", "bf16", "fp32", "fp16", "bf16"]


@pytest.mark.parametrize("shifts", [(0, 0), (1, 1), (0, 1), (1, 0)], ids=["vector", "element", "flat+4B", "views+1"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16", "mixed"])
def test_every_mode_vs_oracle(dtype, shifts):
    """Every mode at the tile-straddling layout with the special values, fp32 / bf16 / fp16 and a
    mixed table; flat 16-byte aligned and 4 bytes later; views on and off the group grid.  The
    guard elements around every view and around flat must not change."""
    _assert_all(_run_modes(LENS, MIXED if dtype == "mixed" else dtype, shifts[0], shifts[1]))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_second_launch_chunk(dtype):
    """130 tensors of 3 to 70 elements: two launches (the count is asserted in _run_modes)."""
    from chocosgd_amd import codec
    lens = [3 + (s * 37) % 68 for s in range(130)]
    assert min(lens) == 3 and max(lens) == 70 and codec.params_ef_launches(len(lens)) == 2
    _assert_all(_run_modes(lens, dtype, 0, 0, seed=11))


def test_public_wrapper_and_special_values():
    """codec.params_ef on plain tensors, and the planted values by hand."""
    from chocosgd_amd import codec
    x_raw, f = _inputs(LENS)
    o = int(_offs(LENS)[3])
    params, a = [], 0
    for m in LENS:
        params.append(dev(x_raw[a:a + m]))
        a += m
    flat = dev(f)
    plan = codec.params_ef(params, flat, codec.EF_APPLY)
    got = np.concatenate([host(p) for p in params])
    assert got[o + NEG_ZERO].view(np.uint32) == 0
    for at in (INF_FLAT, NAN_PARAM, NAN_FLAT, INF_PARAM, OPPOSITE_INF):
        assert not np.isfinite(got[o + at])
    assert np.isnan(got[o + OPPOSITE_INF]) and got[o + INF_FLAT] == np.inf and got[o + INF_PARAM] == -np.inf
    assert same_bits(host(flat), f), "APPLY alone leaves flat as it was"
    params2 = [p.clone().zero_() for p in params]
    codec.params_ef(params2, flat, codec.EF_APPLY | codec.EF_DIV | codec.EF_SCALE, lr=LR, divisor=DIVISOR)
    got, q = np.concatenate([host(p) for p in params2]), host(flat)
    tiny = np.finfo(np.float32).tiny
    for at in (SUB_PRODUCT, SUB_QUOTIENT):
        assert 0 < abs(got[o + at]) < tiny, "a subnormal product was flushed"
    assert 0 < q[o + SUB_QUOTIENT] < tiny, "a subnormal quotient was flushed"
    assert same_bits(q, EO.div32(f, np.float32(DIVISOR)))
    with pytest.raises(RuntimeError, match="another parameter list"):
        codec.params_ef(params2, flat, codec.EF_ACCUM, plan=plan)


@pytest.mark.parametrize("dtype,half,ulp", [("bf16", 2.0 ** -8, 2.0 ** -7), ("fp16", 2.0 ** -11, 2.0 ** -10)])
def test_one_narrowing_at_a_halfway_sum(dtype, half, ulp):
    """x + a exactly halfway between two 16-bit values goes to the even one, and three sums around
    it tell one narrowing of the fp32 sum from any other order of roundings:
      a = half + 2^-23: the fp32 sum lies above halfway -> up (narrowing a first would tie -> 1)
      a = half + 2^-25: the exact sum lies above halfway but is no fp32 value; the fp32 add rounds
                        it to the halfway point, which then goes to the even 1 (one rounding of
                        the exact sum straight to 16 bits would go up)."""
    from chocosgd_amd import codec
    x = np.float32([1.0, 1.0 + ulp, 1.0, 1.0, -1.0])
    a = np.float32([half, half, half + 2.0 ** -23, half + 2.0 ** -25, -half])
    want = np.float32([1.0, 1.0 + 2 * ulp, 1.0 + ulp, 1.0, -1.0])
    assert same_bits(EO.apply(a, x, dtype=dtype)[0], want)
    for shift in (0, 1):
        pv, fl = Views(x, [5], dtype, shift), Flat(5, a, shift)
        codec.params_ef(pv.views, fl.t, codec.EF_APPLY)
        _assert_all(pv.pairs("params", want))
        # through the scale: -lr * a with lr = -1 is a itself
        pv = Views(x, [5], dtype, shift)
        codec.params_ef(pv.views, fl.t, codec.EF_APPLY | codec.EF_SCALE, lr=-1.0)
        _assert_all(pv.pairs("scaled params", want))


# ----------------------------------------------------------------------------- the residual kernel
SEG_LENS = [5, 1, 8195, 33, 4099, 17000, 40, 40, 1]  # segments across the 1024-element tiles


def _residual_inputs():
    rng = np.random.RandomState(5)
    n = sum(SEG_LENS)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 1, n)).astype(np.float32)
    x[::101] = 0.0
    x[7::997] = -0.0
    x[13::1013] = np.nan
    x[6 + 20], x[6 + 21] = np.inf, -np.inf
    norms = (rng.uniform(0.5, 50.0, len(SEG_LENS)) * np.array(SEG_LENS)).astype(np.float32)
    return x, norms


@pytest.mark.parametrize("with_local", [False, True], ids=["no local_out", "local_out"])
@pytest.mark.parametrize("in_place", [False, True], ids=["out of place", "in place"])
@pytest.mark.parametrize("segmented", [True, False], ids=["segments", "one segment"])
def test_residual_vs_oracle(segmented, in_place, with_local):
    from chocosgd_amd import codec
    x, norms = _residual_inputs()
    lens = SEG_LENS if segmented else [x.size]
    norms = norms[:len(lens)]
    n = x.size
    seg_off = torch.from_numpy(_offs(lens)).to(DEV) if segmented else None
    xs, local = Flat(n, x, shift=1), Flat(n, shift=0) if with_local else None
    resid = xs if in_place else Flat(n, shift=1)
    nd = dev(norms)
    c0 = codec.launch_count("sign_local_residual")
    got = codec.sign_local_residual(xs.t, nd, seg_off=seg_off, nseg=len(lens), local_out=local.t if local else None,
                                    resid_out=resid.t)
    assert got is resid.t and codec.launch_count("sign_local_residual") - c0 == 1
    want_r, want_u = EO.residual(x, norms, lens)
    assert same_bits(resid.all(), resid.expect(want_r))
    if not in_place:
        assert same_bits(xs.all(), xs.expect(x)), "x is read only"
    if with_local:
        assert same_bits(local.all(), local.expect(want_u))
        assert np.all(want_u[x == 0].view(np.uint32) == 0) and np.all(want_u[np.isnan(x)].view(np.uint32) == 0)
        # the same u as choco_sign_local_decode: one device function
        u = codec.sign_local_decode(dev(x), nd, seg_off=seg_off, nseg=len(lens))
        assert same_bits(host(u), host(local.t))
    zero = (x == 0) | np.isnan(x)
    assert same_bits(want_r[x == 0], x[x == 0]) and np.isnan(want_r[np.isnan(x)]).all() and zero.sum() > 300


def test_residual_default_output_is_a_new_tensor():
    from chocosgd_amd import codec
    x, norms = _residual_inputs()
    xd, nd = dev(x), dev(norms)
    seg_off = torch.from_numpy(_offs(SEG_LENS)).to(DEV)
    got = codec.sign_local_residual(xd, nd, seg_off=seg_off, nseg=len(SEG_LENS))
    assert got.data_ptr() != xd.data_ptr() and same_bits(host(xd), x)
    assert same_bits(host(got), EO.residual(x, norms, SEG_LENS)[0])
    with pytest.raises(RuntimeError, match="local_out aliases"):
        codec.sign_local_residual(xd, nd, seg_off=seg_off, nseg=len(SEG_LENS), local_out=xd)

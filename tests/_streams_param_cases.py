"""The parameter-table kernels' cases of test_gpu_streams_codec.py (its table, its harness).

Layout: test_gpu_param_walk.py's `chunk` layout for the kernel's cap -- cap + 1 tensors of 0 to 9
elements -- plus one tensor of 8 200: two launches whose chunk boundary falls inside a tile, and a
tensor that crosses a tile end.  The tensors are views 8 elements apart in ONE storage per role,
which is the working tensor the harness poisons and refills; the whole storage is compared, so
the gaps are checked with the views.  fp32 and bf16, bit for bit against the numpy models of the
kernels' own tests; the device's norm totals within one step of their grid (the bound of
test_gpu_gclip / test_gpu_lscale / test_gpu_dgc_sgd) and everything computed from them with the
device's value."""
from types import SimpleNamespace

import numpy as np
import torch

import _adam_oracle as AO
import _adam_sr_oracle as ASR
import _allreduce_oracle as ARO
import _allreduce_scaled_oracle as ASO
import _consensus_oracle as CO
import _dgc_oracle as DO
import _ef_oracle as EO
import _gclip_oracle as GO
import _lscale_oracle as LO
import _master_oracle as MA
import _mix_oracle as MO
import _sgd_oracle as SO
from chocosgd_amd.rounding import sr_bits
from conftest import same_bits

F32 = np.float32
DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
MODES = ["fp32", "bf16"]
GAP = 8
HP = (0.1, 5e-4, 0.9, 0.1, False)  # lr, weight decay, momentum, dampening, nesterov
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, step=3)
SR = (7, 2)  # (seed, step)
MAX_NORM = 0.5


def lens_for(cap):
    return [i % 10 for i in range(cap + 1)] + [8200]


class Views:
    """k tensors as views GAP elements apart in one storage of `mode`'s dtype: the true storage and its
    poison (other finite values; non-negative with positive=True, for second moments)."""

    def __init__(self, lens, mode, seed, scale=1.0, positive=False):
        self.lens, self.mode, self.dt = list(lens), mode, DT[mode]
        self.starts, p = [], 0
        for m in self.lens:
            self.starts.append(p)
            p += m + GAP
        self.total = p
        rng = np.random.default_rng(seed)
        draw = lambda: (np.abs(rng.standard_normal(p)) if positive else rng.standard_normal(p)) * scale  # noqa: E731
        self.true = torch.from_numpy(draw().astype(F32)).to(self.dt)
        self.poison = torch.from_numpy(draw().astype(F32)).to(self.dt)
        self.offs = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)

    def of(self, t):
        return [t[s:s + m] for s, m in zip(self.starts, self.lens)]

    def pieces(self):
        """The true tensors widened to fp32."""
        return [v.float().numpy().copy() for v in self.of(self.true)]

    def flat(self):
        return np.concatenate(self.pieces())

    def expect(self, new):
        """The whole storage as fp32 with tensor i replaced by new[i] (None: unchanged)."""
        want = self.true.float().numpy().copy()
        for s, m, v in zip(self.starts, self.lens, new):
            if v is not None:
                want[s:s + m] = v
        return want

    def split(self, flat):
        return [np.asarray(flat[a:b], F32) for a, b in zip(self.offs[:-1], self.offs[1:])]


def flat_pair(n, seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * scale).astype(F32), (rng.standard_normal(n) * scale).astype(F32)


def near_on_grid(a, b, cd):
    return GO.ulp_distance(a, b, cd) <= 1


def register(case, go):  # noqa: C901  (one closure per wrapper)
    from chocosgd_amd import codec

    def both(family, name, covers):
        """Register fn(mode, id) once per dtype."""
        def reg(fn):
            for mode in MODES:
                cid = f"{name}-{mode}"
                case(family, cid, covers)(lambda mode=mode, cid=cid: fn(mode, cid))
            return fn
        return reg

    def sgd_plan(P, G, B, W, master=False, nograd=False, hp=HP):
        lr, wd, mom, damp, nest = hp
        return codec._sgd_tables(P.of(W.P), None if nograd else G.of(W.G), B.of(W.B) if mom else None, lr, wd, mom,
                                 damp, nest, False, None, master)

    def sgd_inputs(cap, mode, seed, master=False):
        lens = lens_for(cap)
        P, G = Views(lens, mode, seed), Views(lens, mode, seed + 1, 0.1)
        B = Views(lens, "fp32" if master else mode, seed + 2, 0.1)
        return lens, P, G, B

    def stores(**views):
        """({name: true storage}, {name: poison}) of the views given by name."""
        return {k: v.true for k, v in views.items()}, {k: v.poison for k, v in views.items()}

    # ------------------------------------------------------------------ pack and update
    @both("params_update", "params_pack", ["params_pack"])
    def _pack(mode, cid):
        lens = lens_for(192)
        P = Views(lens, mode, 1)
        n = sum(lens)
        assert codec.params_launches(len(lens)) == 2
        true, poison = stores(P=P)
        _, W, o = go("params_update", cid, lambda W: codec.params_pack(P.of(W.P), W.flat), true, poison=poison,
                     outs={"flat": (n, torch.float32)})
        assert same_bits(o.flat, P.flat()) and same_bits(W.P, P.expect([None] * len(lens)))

    def _unpack(mode, cid, sr):
        lens = lens_for(192)
        n = sum(lens)
        P = Views(lens, mode, 2)
        flat, flat_poison = flat_pair(n, 3)
        true, poison = stores(P=P)
        true["flat"], poison["flat"] = flat, flat_poison
        _, W, _ = go("params_update", cid, lambda W: codec.params_unpack(W.flat, P.of(W.P), sr=sr), true,
                     poison=poison)
        if sr is None or mode == "fp32":
            new = [SO.to_grid(f, mode) for f in P.split(flat)]
        else:
            new = [ASR.sr_narrow(f, sr_bits(sr[0], sr[1], a, f.size).astype(np.uint32))
                   for f, a in zip(P.split(flat), P.offs[:-1])]
        assert same_bits(W.P, P.expect(new)) and same_bits(W.flat, flat)

    both("params_update", "params_unpack", ["params_unpack"])(lambda mode, cid: _unpack(mode, cid, None))
    both("params_update", "params_unpack-sr", ["params_unpack"])(lambda mode, cid: _unpack(mode, cid, SR))

    def _run(mode, cid, variant):
        """ParamSgdPlan.run: plain, behind gradnorm (gclip), behind gradnorm_scaled (scaled), sr."""
        lens, P, G, B = sgd_inputs(72, mode, 10)
        n, k = sum(lens), len(lens)
        assert codec.params_sgd_launches(k) == 2
        hp = (0.1, 0.0, 0.0, 0.0, False) if variant == "sr" else HP
        scale = 1024.0
        if variant == "scaled":  # the gradients still carry the loss scale (a power of two: exact in both dtypes)
            G.true, G.poison = G.true * scale, G.poison * scale
        true, poison = stores(P=P, G=G, B=B)
        if variant == "scaled":
            true.update(scale=np.array([scale], F32), tracker=np.array([0], np.int32))
            poison.update(scale=np.array([512.0], F32), tracker=np.array([7], np.int32))

        def call(W):
            plan = sgd_plan(P, G, B, W, hp=hp)
            if variant == "gclip":
                gn = plan.gradnorm(MAX_NORM)
                plan.run(W.flat, gclip=gn)
                return gn, plan
            if variant == "scaled":
                scaler = SimpleNamespace(_scale=W.scale, _growth_tracker=W.tracker, growth_factor=2.0,
                                         backoff_factor=0.5, growth_interval=2000)
                ls = plan.gradnorm_scaled(scaler, max_norm=MAX_NORM)
                plan.run(W.flat, scaled=ls)
                return ls, plan
            plan.run(W.flat, sr=SR if variant == "sr" else None)
            return None, plan

        (stat, _), W, o = go("params_update", cid, call, true, poison=poison, outs={"flat": (n, torch.float32)})
        grads = G.pieces()
        if variant == "gclip":
            assert near_on_grid(stat[0], GO.total(grads, mode), mode), (stat, GO.total(grads, mode))
            c = GO.coef(stat[0], MAX_NORM, mode)
            assert same_bits(stat[1:], [c]) and c < 1
            grads = [GO.clip(g, c, mode) for g in grads]
        elif variant == "scaled":
            assert near_on_grid(stat[0], LO.total(grads, scale, mode), mode), (stat, LO.total(grads, scale, mode))
            assert same_bits(stat, LO.out(stat[0], MAX_NORM, scale, False, mode))
            grads = [LO.unscale(g, stat[1], mode) for g in grads]
            want_scale, want_tracker = LO.update(scale, 0, False)
            assert same_bits(W.scale, [want_scale]) and W.tracker.tolist() == [want_tracker]
        lr, wd, mom, damp, nest = hp
        new_p, new_b, new_flat = [], [], []
        for p, g, b, a in zip(P.pieces(), grads, B.pieces(), P.offs[:-1]):
            if variant == "sr":
                p32 = SO.sgd_step(p, g, None, lr, dtype="fp32")[0]
                new_flat.append(p32)
                new_p.append(p32 if mode == "fp32" else
                             ASR.sr_narrow(p32, sr_bits(SR[0], SR[1], a, p32.size).astype(np.uint32)))
                new_b.append(None)
                continue
            p_new, b_new, _ = SO.sgd_step(p, g, b, lr, wd, mom, damp, nest, False, dtype=mode)
            new_p.append(p_new), new_b.append(b_new), new_flat.append(p_new)
        assert same_bits(W.P, P.expect(new_p)), "params (or the gaps between them)"
        assert same_bits(W.B, B.expect(new_b)), "momentum buffers"
        assert same_bits(W.G, G.expect([None] * k)), "the grads were written"
        assert same_bits(o.flat, np.concatenate(new_flat))

    both("params_update", "sgd_run", ["ParamSgdPlan.run"])(lambda mode, cid: _run(mode, cid, "plain"))
    both("params_update", "sgd_run-gclip", ["ParamSgdPlan.run", "ParamSgdPlan.gradnorm"])(
        lambda mode, cid: _run(mode, cid, "gclip"))
    both("params_update", "sgd_run-scaled", ["ParamSgdPlan.run", "ParamSgdPlan.gradnorm_scaled"])(
        lambda mode, cid: _run(mode, cid, "scaled"))
    both("params_update", "sgd_run-sr", ["ParamSgdPlan.run"])(lambda mode, cid: _run(mode, cid, "sr"))

    @both("params_update", "sgd_run_master", ["ParamSgdPlan.run_master"])
    def _run_master(mode, cid):
        lens, P, G, B = sgd_inputs(72, mode, 20, master=True)
        n, k = sum(lens), len(lens)
        assert codec.params_sgd_master_launches(k) == 2
        master, master_poison = flat_pair(n, 23)
        true, poison = stores(P=P, G=G, B=B)
        true["master"], poison["master"] = master, master_poison
        _, W, _ = go("params_update", cid, lambda W: sgd_plan(P, G, B, W, master=True).run_master(W.master), true,
                     poison=poison)
        lr, wd, mom, damp, nest = HP
        res = [MA.master_step(m, g, b, lr, wd, mom, damp, nest, False, dtype=mode)
               for m, g, b in zip(P.split(master), G.pieces(), B.pieces())]
        assert same_bits(W.master, np.concatenate([r[0] for r in res]))
        assert same_bits(W.B, B.expect([r[1] for r in res])) and same_bits(W.P, P.expect([r[2] for r in res]))

    def _pack_grads(mode, cid, scaled):
        lens, P, G, B = sgd_inputs(192, mode, 30)
        n, k = sum(lens), len(lens)
        true, poison = stores(P=P, G=G, B=B)

        def call(W):
            plan = sgd_plan(P, G, B, W)
            gn = plan.gradnorm(MAX_NORM) if scaled else None
            plan.pack_grads(W.flat, coef=gn)
            return gn, plan

        (gn, _), W, o = go("params_update", cid, call, true, poison=poison, outs={"flat": (n, torch.float32)})
        grads = G.pieces()
        if scaled:
            assert near_on_grid(gn[0], GO.total(grads, mode), mode)
            assert same_bits(gn[1:], [GO.coef(gn[0], MAX_NORM, mode)])
            grads = [ASO.pack(g, gn[1], mode, round=True) for g in grads]
        assert same_bits(o.flat, np.concatenate(grads)) and same_bits(W.G, G.expect([None] * k))

    both("params_update", "pack_grads", ["ParamSgdPlan.pack_grads"])(lambda mode, cid: _pack_grads(mode, cid, False))
    both("params_update", "pack_grads-coef", ["ParamSgdPlan.pack_grads", "ParamSgdPlan.gradnorm"])(
        lambda mode, cid: _pack_grads(mode, cid, True))

    @both("params_update", "sgd_run_flatgrad", ["ParamSgdPlan.run_flatgrad"])
    def _run_flatgrad(mode, cid):
        lens, P, G, B = sgd_inputs(72, mode, 40)
        n, k = sum(lens), len(lens)
        assert codec.params_sgd_flatgrad_launches(k) == 2
        gsum, gsum_poison = flat_pair(n, 43, 0.3)
        true, poison = stores(P=P, G=G, B=B)
        true["gsum"], poison["gsum"] = gsum, gsum_poison
        _, W, _ = go("params_update", cid, lambda W: sgd_plan(P, G, B, W).run_flatgrad(W.gsum, 3.0), true,
                     poison=poison)
        lr, wd, mom, damp, nest = HP
        res = [ARO.step(p, s, b, 3.0, lr, wd, mom, damp, nest, False, dtype=mode)
               for p, s, b in zip(P.pieces(), P.split(gsum), B.pieces())]
        assert same_bits(W.P, P.expect([r[0] for r in res])) and same_bits(W.B, B.expect([r[1] for r in res]))
        assert same_bits(W.G, G.expect([r[2] for r in res])), "the averaged gradient"
        assert same_bits(W.gsum, gsum)

    # ------------------------------------------------------------------ norms, mix and the rest
    @both("params_rest", "sqnorm", ["ParamSgdPlan.sqnorm"])
    def _sqnorm(mode, cid):
        import test_gpu_dgc_sgd as DGC
        lens = lens_for(112)
        P, G = Views(lens, mode, 50), Views(lens, mode, 51, 0.1)
        assert codec.params_sqnorm_launches(len(lens)) == 3
        true, poison = stores(P=P, G=G)
        ret, W, _ = go("params_rest", cid, lambda W: codec.params_sqnorm(P.of(W.P), G.of(W.G), 1e-2), true,
                       poison=poison)
        DGC._check_norms(ret, P.flat(), G.flat(), lens, 1e-2, mode)
        assert same_bits(W.P, P.expect([None] * len(lens))) and same_bits(W.G, G.expect([None] * len(lens)))

    @both("params_rest", "gradnorm+norms", ["ParamSgdPlan.gradnorm"])
    def _gradnorm(mode, cid):
        """The partial launches, then the total launch that also leaves the per-tensor norms."""
        import test_gpu_dgc_sgd as DGC
        lens, P, G, B = sgd_inputs(112, mode, 60)
        k = len(lens)
        assert codec.params_gradnorm_launches(k) >= 2
        true, poison = stores(P=P, G=G, B=B)

        def call(W):
            plan = sgd_plan(P, G, B, W)
            return plan.gradnorm(MAX_NORM, norms=W.norms), plan

        (gn, _), W, o = go("params_rest", cid, call, true, poison=poison, outs={"norms": (k, torch.float32)})
        assert near_on_grid(gn[0], GO.total(G.pieces(), mode), mode)
        assert same_bits(gn[1:], [GO.coef(gn[0], MAX_NORM, mode)])
        DGC._check_norms(o.norms, P.flat(), G.flat(), lens, 0.0, mode)

    @both("params_rest", "gradnorm_scaled_local+loss_scale_update",
          ["ParamSgdPlan.gradnorm_scaled", "ParamSgdPlan.loss_scale_update"])
    def _loss_scale_update(mode, cid):
        """The all-reduce step's two launches: this rank's norm with the scaler's state left alone, then
        the update from the all-reduced flag (another rank overflowed: the scale backs off)."""
        lens, P, G, B = sgd_inputs(112, mode, 70)
        n = sum(lens)
        scale = 1024.0
        G.true, G.poison = G.true * scale, G.poison * scale
        gsum, gsum_poison = flat_pair(n + 1, 73)
        gsum[n], gsum_poison[n] = 2.0, 0.0
        true, poison = stores(P=P, G=G, B=B)
        true.update(scale=np.array([scale], F32), tracker=np.array([5], np.int32), gsum=gsum)
        poison.update(scale=np.array([64.0], F32), tracker=np.array([7], np.int32), gsum=gsum_poison)

        def call(W):
            plan = sgd_plan(P, G, B, W)
            scaler = SimpleNamespace(_scale=W.scale, _growth_tracker=W.tracker, growth_factor=2.0, backoff_factor=0.5,
                                     growth_interval=2000)
            scaler.last = plan.gradnorm_scaled(scaler, max_norm=MAX_NORM, update_state=False)
            plan.loss_scale_update(scaler, W.gsum)
            return scaler.last, plan

        (ls, _), W, _ = go("params_rest", cid, call, true, poison=poison)
        grads = G.pieces()
        assert near_on_grid(ls[0], LO.total(grads, scale, mode), mode)
        want = LO.out(ls[0], MAX_NORM, scale, False, mode)
        want[2] = 1.0  # the common flag
        assert same_bits(ls, want), (ls, want)
        want_scale, want_tracker = LO.update(scale, 5, True)
        assert same_bits(W.scale, [want_scale]) and W.tracker.tolist() == [want_tracker] and want_scale == 512.0
        assert same_bits(W.gsum, gsum)

    WEIGHTS = [0.5, 0.0, 1.0 / 3]

    def mix_sources(n, seed):
        true, poison, srcs = {}, {}, []
        for r in range(3):
            s, sp = flat_pair(n, seed + r)
            true[f"s{r}"], poison[f"s{r}"] = s, sp
            srcs.append(s)
        return true, poison, srcs

    @both("params_rest", "mix-write_params", ["ParamSgdPlan.mix"])
    def _mix(mode, cid):
        lens = lens_for(128)
        n, k = sum(lens), len(lens)
        P = Views(lens, mode, 80)
        assert codec.params_mix_launches(k, 3) == 2
        true, poison, srcs = mix_sources(n, 81)
        true["P"], poison["P"] = P.true, P.poison

        def call(W):
            plan = codec.ParamSgdPlan(P.of(W.P))
            for i, v in enumerate(P.of(W.P)):
                plan.param_ptrs[i] = v.data_ptr()
            plan.mix([W.s0, W.s1, W.s2], WEIGHTS, mode=codec.MIX_WRITE_PARAMS, flat_out=W.flat)
            return None, plan

        _, W, o = go("params_rest", cid, call, true, poison=poison, outs={"flat": (n, torch.float32)})
        _, p_new, out = MO.mix(srcs, WEIGHTS, dtype=mode)
        assert same_bits(W.P, P.expect(P.split(p_new))) and same_bits(o.flat, out)
        assert all(same_bits(getattr(W, f"s{r}"), srcs[r]) for r in range(3))

    @case("params_rest", "params_mix-flat", ["params_mix"])
    def _mix_flat():
        """Without a parameter list: the sources mixed as one flat tensor."""
        n = 8200 * 2 + 5
        true, poison, srcs = mix_sources(n, 85)
        _, W, o = go("params_rest", "params_mix-flat",
                     lambda W: codec.params_mix([W.s0, W.s1, W.s2], WEIGHTS, flat_out=W.flat), true, poison=poison,
                     outs={"flat": (n, torch.float32)})
        assert same_bits(o.flat, MO.mix(srcs, WEIGHTS)[2])

    @both("params_rest", "ef-apply_div_scale", ["ParamSgdPlan.ef"])
    def _ef(mode, cid):
        lens = lens_for(128)
        n, k = sum(lens), len(lens)
        P = Views(lens, mode, 90)
        assert codec.params_ef_launches(k) == 2
        flat, flat_poison = flat_pair(n, 91)
        true, poison = stores(P=P)
        true["flat"], poison["flat"] = flat, flat_poison
        ef_mode = codec.EF_APPLY | codec.EF_DIV | codec.EF_SCALE
        assert (EO.APPLY | EO.DIV | EO.SCALE) == ef_mode
        _, W, _ = go("params_rest", cid, lambda W: (None, codec.params_ef(P.of(W.P), W.flat, ef_mode, lr=0.1,
                                                                           divisor=3.0)), true, poison=poison)
        res = [EO.ef(ef_mode, f, p, 0.1, 3.0, mode) for f, p in zip(P.split(flat), P.pieces())]
        assert same_bits(W.P, P.expect([r[0] for r in res]))
        assert same_bits(W.flat, np.concatenate([r[1] for r in res]))

    @both("params_rest", "consensus-dist+avg", ["ParamSgdPlan.consensus"])
    def _consensus(mode, cid):
        """The distance (partials, then the total launch) and the written average in one call."""
        lens = lens_for(128)
        n, k = sum(lens), len(lens)
        P, Q = Views(lens, mode, 100), Views(lens, mode, 101)
        assert codec.params_consensus_launches(k) == 3
        xsum, xsum_poison = flat_pair(n, 102, 3.0)
        true, poison = stores(P=P, Q=Q)
        true["xsum"], poison["xsum"] = xsum, xsum_poison

        def call(W):
            return codec.params_consensus(P.of(W.P), W.xsum, 3.0, avg_out=Q.of(W.Q), dists=W.dists)

        (out, _), W, o = go("params_rest", cid, call, true, poison=poison, outs={"dists": (k, torch.float32)})
        avg, mout, mdists = CO.consensus(P.flat(), xsum, 3.0, lens, [mode] * k)
        assert np.isfinite(mout).all() and same_bits(out, mout), (out, mout)
        assert same_bits(o.dists, mdists)
        assert same_bits(W.Q, Q.expect(P.split(avg))) and same_bits(W.P, P.expect([None] * k))
        assert same_bits(W.xsum, xsum)

    @both("params_rest", "params_mask", ["params_mask"])
    def _mask(mode, cid):
        import test_gpu_dgc_sgd as DGC
        lens = lens_for(128)
        n, k = sum(lens), len(lens)
        assert codec.params_mask_launches(k) == 2
        B = Views(lens, mode, 110)
        x, x_poison = flat_pair(n, 111)
        values, indices, ks = DGC._selection(x, lens, 0.75)
        pvalues, pindices, pks = DGC._selection(x_poison, lens, 0.75)
        assert pks == ks and not np.array_equal(indices, pindices)
        true, poison = stores(B=B)
        true.update(values=values, indices=indices, memory=x)
        poison.update(values=pvalues, indices=pindices, memory=x_poison)
        _, W, _ = go("params_rest", cid,
                     lambda W: codec.params_mask(B.of(W.B), W.values, W.indices, ks, memory=W.memory), true,
                     poison=poison)
        model, mem = B.pieces(), x.copy()
        DO.mask(model, [mode] * k, lens, values, indices, ks, mem)
        assert same_bits(W.B, B.expect(model)) and same_bits(W.memory, mem)

    def _adam(mode, cid, variant):
        """ParamAdamPlan.run, run_master and run(sr=)."""
        master = variant == "master"
        lens = lens_for(54)
        n, k = sum(lens), len(lens)
        assert codec.params_adam_launches(k) == 2
        P, G = Views(lens, mode, 120), Views(lens, mode, 121, 0.1)
        mdt = "fp32" if master else mode
        M, V = Views(lens, mdt, 122, 0.1), Views(lens, mdt, 123, 0.01, positive=True)
        true, poison = stores(P=P, G=G, M=M, V=V)
        if master:
            true["master"], poison["master"] = flat_pair(n, 124)
        a = ADAM

        def call(W):
            plan = codec._adam_tables(P.of(W.P), G.of(W.G), M.of(W.M), V.of(W.V), a["lr"], (a["beta1"], a["beta2"]),
                                      a["eps"], a["wd"], a["step"], True, False, None, master)
            if master:
                plan.run_master(W.master)
            else:
                plan.run(W.flat, sr=SR if variant == "sr" else None)
            return None, plan

        _, W, o = go("params_rest", cid, call, true, poison=poison, outs={} if master else {"flat": (n, torch.float32)})
        kw = dict(lr=a["lr"], beta1=a["beta1"], beta2=a["beta2"], eps=a["eps"], wd=a["wd"], step=a["step"],
                  decoupled=True, first=False)
        pieces = zip(P.split(true["master"]) if master else P.pieces(), G.pieces(), M.pieces(), V.pieces(),
                     P.offs[:-1])
        if master:
            res = [AO.adam_master_step(p, g, m, v, dtype=mode, **kw) for p, g, m, v, _ in pieces]
            assert same_bits(W.master, np.concatenate([r[0] for r in res]))
            new_p = [r[3] for r in res]
        elif variant == "sr":
            res = [ASR.adam_sr_step(p, g, m, v, dtype=mode, seed=SR[0], sr_step=SR[1], start=int(s), **kw)
                   for p, g, m, v, s in pieces]
            assert same_bits(o.flat, np.concatenate([r[4] for r in res]))
            new_p = [r[0] for r in res]
        else:
            res = [AO.adam_step(p, g, m, v, dtype=mode, **kw) for p, g, m, v, _ in pieces]
            assert same_bits(o.flat, np.concatenate([r[0] for r in res]))
            new_p = [r[0] for r in res]
        assert same_bits(W.P, P.expect(new_p)), "params"
        assert same_bits(W.M, M.expect([r[1] for r in res])), "exp_avg"
        assert same_bits(W.V, V.expect([r[2] for r in res])), "exp_avg_sq"
        assert same_bits(W.G, G.expect([None] * k))

    both("params_rest", "adam_run", ["ParamAdamPlan.run"])(lambda mode, cid: _adam(mode, cid, "plain"))
    both("params_rest", "adam_run_master", ["ParamAdamPlan.run_master"])(lambda mode, cid: _adam(mode, cid, "master"))
    both("params_rest", "adam_run-sr", ["ParamAdamPlan.run"])(lambda mode, cid: _adam(mode, cid, "sr"))

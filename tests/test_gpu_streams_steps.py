"""The CHOCO step across two streams, and every other step function on a delayed side stream
(tests/_streams.py).

The reference binds the compressor's gossip stream at construction (parallel_choco_v.py:214-218); a
training loop that builds the optimizer first and enters its `torch.cuda.stream(...)` scope later steps
on another one.  The contract: pipeline() and flush_receive() make the gossip
stream wait for the caller's current stream on entry and the caller's stream wait for the gossip stream
on exit, and do nothing at all when the two are one stream.

Here the compressor is built under stream G and stepped under stream C, and every case runs once per
hand-over (DIRECTIONS):

    entry   C alone is delayed, in front of the true inputs; G is free.  A pipeline or flush that does not
            wait for C runs at once and packs, compresses or receives into the poison.
    exit    G is delayed as well, by twice C's delay, so that it is the last to finish.  A caller that does
            not wait for G unpacks, or reads x_hat / memory, before the gossip ran.  (With G the later
            stream this run alone could not see a missing entry wait: G's own delay would stand in for it.)

Taking either `wait_stream` line out of `_on_gossip_stream` fails the numerical cases of its direction.
Expectations are the oracle's (oracle/choco_oracle.py) for the
same sequence with the self-echo aggregator of test_fused_step_helper_updates_model: parameters, x_hat and
memory bit for bit, at the norms the device measured (those within rtol 1e-6 of the fp64 norms, the bound
of test_gossip_sign / test_gossip_qsgd)."""
import numpy as np
import pytest
import torch

import _streams as ST
from conftest import same_bits
from oracle import choco_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = np.float32
GAMMA = 0.9
LENS = [37, 4096, 5]
N = sum(LENS)
Q, S_LEVELS = 4, 15
DIRECTIONS = ["entry", "exit"]
both_directions = pytest.mark.parametrize("direction", DIRECTIONS)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def randn(n, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(F32)


def state(seed):
    x = randn(N, seed)
    hat = (x + randn(N, seed + 1, 0.1)).astype(F32)
    mem = (hat + randn(N, seed + 2, 0.05)).astype(F32)
    return {"x": x, "hat": hat, "mem": mem}


def bounds():
    off = np.concatenate([[0], np.cumsum(LENS)])
    return list(zip(off[:-1].tolist(), off[1:].tolist()))


class Echo:
    """Every exchange gives this worker's own message back (rank 0, weight 1)."""

    def _agg(self, data, op, force_wait=False):
        return [], {0: data}

    def complete_wait(self, reqs):
        pass


class World:
    """One worker: a compressor built under stream G, the model, x_hat and memory as views of three flat
    working tensors, stepped under stream C."""

    def __init__(self, comm_op, aggregator=None):
        from chocosgd_amd.parallel_choco import CHOCOCompressor
        from chocosgd_amd.tensor_buffer import TensorBuffer
        self.comm_op = comm_op
        self.G, self.C = ST.side_stream("G"), ST.side_stream("C")
        with torch.cuda.stream(self.G):
            self.comp = CHOCOCompressor(aggregator=aggregator or Echo(), comm_op=comm_op, comm_device="gpu",
                                        compress_ratio=0.9, quantize_level=Q, is_biased=False, backend="nccl",
                                        use_ipc=False)
        assert self.comp.compressor_fn.gossip_stream == self.G
        self.work = {k: torch.empty(N, device=DEV) for k in ("x", "hat", "mem")}
        sizes = [(m,) for m in LENS]
        self.params = list(self.work["x"].split(LENS))
        self.groups = [{"params": [p], "name": f"p{i}"} for i, p in enumerate(self.params)]
        self.names = list(enumerate(g["name"] for g in self.groups))
        self.shapes = [(torch.Size([m]), m) for m in LENS]
        self.nhp = {0: TensorBuffer.from_flat(self.work["hat"], sizes),
                    "memory": TensorBuffer.from_flat(self.work["mem"], sizes)}

    def step(self, defer=False):
        """One utils.fused_step; returns the norms this step's message carries (None for top-k)."""
        from chocosgd_amd import codec, utils
        sb = utils.fused_step(self.comp, self.groups, self.names, self.shapes, self.nhp, {0: 1.0}, GAMMA, 0,
                              defer_receive=defer)
        if self.comm_op == "sign":
            return sb["flatten_norms"].buffer
        if self.comm_op == "quantize_qsgd":
            return codec.qsgd_split(sb["flatten_updates"].buffer, len(LENS))[1]
        return None

    def run(self, sequence, true, case, direction="exit", **kw):
        """`sequence` (a callable of this world returning the steps' norms) under the harness on C, with G
        as the other stream; direction "entry": no delay on G.  Returns (norms per step, x, x_hat, memory)
        as C read them right behind it."""
        kw.setdefault("write_late", direction == "exit")
        case = f"{case}-{direction}"

        def call():
            torch.manual_seed(5)  # the QSGD seeds: one draw per compress, the same in the warm-up and the run
            return sequence(self)

        t_true = {k: dev(v) for k, v in true.items()}
        t_poison = {k: dev(v) for k, v in state(900).items()}
        ret, w, _ = ST.run(call, self.work, t_true, t_poison, family="steps", case=case, stream=self.C, other=self.G,
                           **kw)
        ST.print_report("steps")
        return [None if r is None else host(r) for r in ret], host(w["x"]), host(w["hat"]), host(w["mem"])


def seeds(count):
    torch.manual_seed(5)
    return [int(torch.randint(0, 2**62, (1,)).item()) for _ in range(count)]


def model(comm_op, true, norms):
    """The oracle's sequence of len(norms) CHOCO steps with the self-echo: the consensus step, the message
    of x_new - x_hat, and its receive into x_hat and memory (weight 1).  `norms`: what each step's message
    carried (checked against the fp64 norms here; None entries for top-k).  Returns x, x_hat, memory."""
    x, hat, mem = (true[k].copy() for k in ("x", "hat", "mem"))
    for step, (nm, seed) in enumerate(zip(norms, seeds(len(norms)))):
        x = O.gossip_step(x, mem, hat, GAMMA)
        d = (x - hat).astype(F32)
        if comm_op == "compress_top_k":
            ov, oi = O.topk_segmented(d, LENS, 0.9)[:2]
            O.sparse_accumulate(hat, mem, ov, oi, 1.0)
        elif comm_op == "sign":
            assert np.allclose(nm, O.l1_norms(d, LENS), rtol=1e-6, atol=0), step
            O.sign_accumulate(hat, mem, [(O.sign_pack(d), nm)], [1.0], 0, LENS)
        else:
            assert np.allclose(nm, O.l2_norms(d, LENS), rtol=1e-6, atol=0), step
            u = O.qsgd_uniforms(N, seed, 0)
            dec = []
            for i, (a, b) in enumerate(bounds()):
                lvl = O.qsgd_levels(d[a:b], S_LEVELS, u[a:b], nm[i])
                dec.append(O.qsgd_decode(lvl, d[a:b] < 0, nm[i], S_LEVELS, b - a))
            O.qsgd_accumulate(hat, mem, [np.concatenate(dec)], [1.0], 0)
    return x, hat, mem


def check(comm_op, true, got):
    norms, x, hat, mem = got
    wx, wh, wm = model(comm_op, true, norms)
    assert same_bits(x, wx), "the parameters"
    assert same_bits(hat, wh), "x_hat"
    assert same_bits(mem, wm), "memory"


@both_directions
@pytest.mark.parametrize("comm_op", ["compress_top_k", "sign", "quantize_qsgd"])
def test_fused_step_under_another_stream_than_the_compressors(comm_op, direction):
    """The non-deferred step: pack and x_hat copy on C, the pipeline on G, the unpack on C."""
    true = state(100)
    w = World(comm_op)
    check(comm_op, true, w.run(lambda w: [w.step()], true, f"fused_step-{comm_op}", direction))


@both_directions
@pytest.mark.parametrize("comm_op", ["sign", "quantize_qsgd"])
def test_deferred_steps_then_flush_under_another_stream(comm_op, direction):
    """Two deferred steps, then flush_receive() and a read of x_hat / memory on C right behind it."""
    true = state(200)
    w = World(comm_op)

    def sequence(w):
        norms = [w.step(defer=True), w.step(defer=True)]
        w.comp.flush_receive()
        return norms

    check(comm_op, true, w.run(sequence, true, f"defer-defer-flush-{comm_op}", direction))
    assert w.comp.compressor_fn._pending is None


@both_directions
@pytest.mark.parametrize("comm_op", ["sign", "quantize_qsgd"])
def test_flush_alone_under_another_stream(comm_op, direction):
    """flush_receive() on its own: the deferred step ran beforehand (synchronised); the harness surrounds
    only the flush and C's read of x_hat / memory, so nothing but flush_receive's own exit wait orders
    that read."""
    true = state(300)
    w = World(comm_op)
    # the state the flush finds: one deferred step from `true`, run on the compressor's own stream and
    # synchronised
    for k, t in w.work.items():
        t.copy_(dev(true[k]))
    torch.cuda.synchronize()
    with torch.cuda.stream(w.G):
        torch.manual_seed(5)
        nm = host(w.step(defer=True).clone())
    torch.cuda.synchronize()
    before = {k: host(t) for k, t in w.work.items()}
    pend = w.comp.compressor_fn._pending
    assert pend is not None

    def flush():
        w.comp.compressor_fn._pending = pend  # (the warm-up consumed it)
        w.comp.flush_receive()
        return []

    _, x, hat, mem = w.run(lambda w: flush(), before, f"flush-{comm_op}", direction)
    wx, wh, wm = model(comm_op, true, [nm])
    assert same_bits(x, wx) and same_bits(hat, wh) and same_bits(mem, wm)
    assert not same_bits(hat, before["hat"]), "the flush applied nothing"


@both_directions
@pytest.mark.parametrize("comm_op", ["sign", "quantize_qsgd"])
def test_plain_step_after_a_deferred_one_under_another_stream(comm_op, direction):
    """The non-deferred step flushes first (on G), then copies x_hat on C."""
    true = state(400)
    w = World(comm_op)
    check(comm_op, true, w.run(lambda w: [w.step(defer=True), w.step()], true, f"defer-plain-{comm_op}", direction))
    assert w.comp.compressor_fn._pending is None


class Broken(Echo):
    """The exchange fails after the compress has been queued."""

    def _agg(self, data, op, force_wait=False):
        raise RuntimeError("the exchange is down")


@both_directions
@pytest.mark.parametrize("comm_op", ["compress_top_k", "sign", "quantize_qsgd"])
def test_caller_waits_for_the_gossip_stream_when_pipeline_has_caught_an_error(comm_op, direction, capsys):
    """sync raises; pipeline() prints the error as the reference does, and the caller's stream still waits
    for what the gossip stream has queued: the unpack on C right behind it stores the x of the fused
    consensus step that the compress wrote on G.  Nothing was received: x_hat and memory are untouched."""
    true = state(700)
    w = World(comm_op, aggregator=Broken())

    def sequence(w):
        w.step()
        return []

    _, x, hat, mem = w.run(sequence, true, f"caught-error-{comm_op}", direction)
    assert "the exchange is down" in capsys.readouterr().out
    assert same_bits(x, O.gossip_step(true["x"], true["mem"], true["hat"], GAMMA))
    assert same_bits(hat, true["hat"]) and same_bits(mem, true["mem"])


def test_same_stream_queues_no_waits():
    """Compressor and step on one stream: pipeline() and flush_receive() touch no stream API at all
    (the launch sequence of every existing caller stays what it was)."""
    w = World("sign")
    base = w.comp.compressor_fn
    with torch.cuda.stream(w.G):
        for k, v in state(500).items():
            w.work[k].copy_(dev(v))
        seen = []
        orig_wait = torch.cuda.Stream.wait_stream
        torch.cuda.Stream.wait_stream = lambda self, other: seen.append((self, other))
        try:
            w.step(defer=True)
            w.comp.flush_receive()
            w.step()
        finally:
            torch.cuda.Stream.wait_stream = orig_wait
        assert seen == [] and base._pending is None
    with torch.cuda.stream(w.C):
        orig_wait = torch.cuda.Stream.wait_stream
        torch.cuda.Stream.wait_stream = lambda self, other: (seen.append((self, other)), orig_wait(self, other))[1]
        try:
            w.step()
        finally:
            torch.cuda.Stream.wait_stream = orig_wait
    torch.cuda.synchronize()
    assert seen == [(w.G, w.C), (w.C, w.G)], "entry: G waits for C; exit: C waits for G"


@pytest.mark.parametrize("comm_op", ["sign", "quantize_qsgd"])
def test_reference_style_step_with_a_receive_pending_raises_and_recovers(comm_op):
    """A step without the `gossip` key (the reference's ParallelCHOCO_V.step: recover_params and
    update_params_from_neighbor outside the compressor) after a deferred one: pipeline() raises to the
    caller before anything is launched, the pending receive is kept, x_hat / memory are untouched; after
    flush_receive() the same step runs and gives the bits of the sequence that flushed first."""
    from chocosgd_amd import codec, utils
    from chocosgd_amd.tensor_buffer import TensorBuffer
    kernels = ["sign_pack", "sign_accumulate", "sign_recv_pack", "sign_planes", "qsgd_norm", "qsgd_quantize",
               "qsgd_recv_norm", "gossip_step", "param_pack_kernel", "param_unpack_kernel"]

    def reference_step(w):
        params, fp, fh = utils.recover_params(w.groups, w.names, 0, w.nhp, get_hat_params=True)
        codec.gossip_step(fp.buffer, w.nhp["memory"].buffer, fh.buffer, GAMMA)
        sb = {"original_shapes": w.shapes, "flatten_params": fp, "flatten_hat_params": fh}
        w.comp.pipeline(sb, w.nhp, {0: 1.0})
        fp.unpack(params)

    def start(flush_first):
        w = World(comm_op)
        for k, v in state(600).items():
            w.work[k].copy_(dev(v))
        torch.manual_seed(5)
        w.step(defer=True)
        if flush_first:
            w.comp.flush_receive()
        return w

    a = start(flush_first=True)
    reference_step(a)
    torch.cuda.synchronize()
    want = {k: host(t) for k, t in a.work.items()}

    b = start(flush_first=False)
    torch.cuda.synchronize()
    base = b.comp.compressor_fn
    pend = base._pending
    assert pend is not None
    before = {k: host(t) for k, t in b.work.items()}
    fp = TensorBuffer(b.params, dtype=torch.float32)
    sb = {"original_shapes": b.shapes, "flatten_params": fp,
          "flatten_hat_params": TensorBuffer.from_flat(b.work["hat"].clone(), [(m,) for m in LENS])}
    counts = [codec.launch_count(k) for k in kernels]
    with pytest.raises(RuntimeError, match="flush_receive"):
        b.comp.pipeline(sb, b.nhp, {0: 1.0})
    torch.cuda.synchronize()
    assert [codec.launch_count(k) for k in kernels] == counts, "pipeline() launched before it raised"
    assert base._pending is pend
    assert all(same_bits(host(t), before[k]) for k, t in b.work.items())
    assert "sign_message" not in sb and "flatten_updates" not in sb
    b.comp.flush_receive()
    assert base._pending is None
    reference_step(b)
    torch.cuda.synchronize()
    for k, t in b.work.items():
        assert same_bits(host(t), want[k]), k
    assert not same_bits(want["hat"], before["hat"])


# ------------------------------------------------------------------------------ every other step
def _runners():
    """One smallest case of every other step function: its module's own GPU runner, which builds the
    inputs, steps and compares with the module's oracle."""
    from conftest import golden
    import test_gpu_adam as AD
    import test_gpu_adam_sr as ADSR
    import test_gpu_allreduce_sgd as AR
    import test_gpu_consensus as CN
    import test_gpu_dgc_sgd as DGC
    import test_gpu_ef_steps as EFS
    import test_gpu_lscale as LS
    import test_gpu_param_mix as MIX
    import test_gpu_param_sgd as PS
    import test_gpu_params_sgd_master as PM
    import test_gpu_sr as SR
    return {
        "apply_gradient": lambda: PS.test_fixture_replay("mom", "apply", True),
        "apply_gradient-master": PM.test_apply_gradient_with_master_on_the_device,
        "apply_gradient-rounding": SR.test_small_updates_survive_on_the_device,
        "apply_gradient-loss_scale":
            lambda: LS.test_fp32_step_equals_torchs_unscale_clip_and_update_on_the_device(golden("gclip_inputs")),
        "apply_adam": lambda: AD.test_three_steps_through_apply_adam("plain", None),
        "apply_adam-master": lambda: AD.test_three_steps_through_apply_adam("master", None),
        "apply_adam-rounding": ADSR.test_three_steps_through_apply_adam_are_the_cpu_loop,
        "dpsgd_step": MIX.test_dpsgd_step_against_its_torch_path,
        "allreduce_sgd_step": lambda: AR.test_step_equals_the_loop("fp32", False, True),
        "dcd-fused_step": lambda: MIX.test_fused_steps_against_their_torch_paths("dcd", "sign"),
        "ecd-fused_step": lambda: MIX.test_fused_steps_against_their_torch_paths("ecd", "sign"),
        "deep_squeeze-fused_step":
            lambda: EFS.test_deepsqueeze_fused_step_matches_the_reference("exact_ds_sign", "sign"),
        "ef_sign-fused_step": EFS.test_ef_sign_fused_step_matches_the_reference,
        "dgc-fused_step": lambda: DGC.test_fused_step_end_to_end(golden("dgc_sgd_inputs"), "nesterov"),
        "consensus_eval": lambda: CN.test_consensus_eval_against_the_loop("fp32", False),
    }


RUNNER_NAMES = ["apply_gradient", "apply_gradient-master", "apply_gradient-rounding", "apply_gradient-loss_scale",
                "apply_adam", "apply_adam-master", "apply_adam-rounding", "dpsgd_step", "allreduce_sgd_step",
                "dcd-fused_step", "ecd-fused_step", "deep_squeeze-fused_step", "ef_sign-fused_step", "dgc-fused_step",
                "consensus_eval"]


@pytest.mark.parametrize("name", RUNNER_NAMES)
def test_step_wholly_on_a_side_stream_with_the_null_stream_delayed(name):
    """The write-late direction ONLY: a launch of the step that lands on the null stream is caught; a launch
    that reads early on a third or a stale stream is NOT tested for these steps.  The reused runners upload
    their inputs and read their results back themselves, and both wait for the stream (_streams.run_whole),
    so a delay in front of them would only be waited out: that is a property of the runners, not of the
    steps, which queue no wait of their own that these tests know of.  The read-early direction needs each
    runner split into build, call and check; the steps' kernels are held to it one by one through the
    codec.py wrappers they call (test_gpu_streams_codec.py)."""
    runners = _runners()
    assert sorted(runners) == sorted(RUNNER_NAMES)
    ST.run_whole(runners[name], family="whole steps", case=name)
    ST.print_report("whole steps")

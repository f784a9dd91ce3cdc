"""Multi-process all-reduce SGD steps with dynamic loss scaling for
tests/test_gpu_allreduce_scaled.py (not a test module).

    python tests/_mp_allreduce_scaled_worker.py <fp32|fp16|fp16_master> <world> <scale|both> <outdir>

This launcher process never touches the GPU: it starts `world` rank processes (spawn).  Each
builds the same model on the one GPU with its own gradients, the centralized aggregator as the
reference builds it (get_aggregators(..., "centralized")) over gloo behind a host staging
wrapper, runs STEPS utils.allreduce_sgd_step(loss_scale=) calls (`both`: with clip_norm too) and
saves its parameters, momentum buffers, gradients, master copy, scale, tracker and
LossScaler.last after every step to <outdir>.  At step 1 rank 1 alone holds one inf.  Every
collective has TIMEOUT seconds.
"""
import datetime
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [3, 8195, 5, 20003, 0, 17, 300]
STEPS = 3
TIMEOUT = 60  # seconds, per collective and for the rendezvous
HP = [(0.1, 5e-4, 0.9, 0.0, True), (0.05, 0.0, 0.9, 0.1, False), (0.1, 1e-4, 0.0, 0.0, False)]  # tensor i: HP[i % 3]
SCALE = 2.0 ** 10      # backed off to 2^9 by the skipped step; 2^4 .. 2^10 keep the scaled values exact
INTERVAL = 2000
CLIP = 0.4
BAD = (3, 12345)       # tensor and element of rank 1's inf at step 1


def params0():
    """Every rank's initial parameters (fp32 values; the model narrows them)."""
    rng = np.random.default_rng(78)
    return [rng.standard_normal(m).astype(np.float32) for m in LENS]


def grads_of(rank, step, scale):
    """Rank `rank`'s gradients of one step, multiplied by the loss scale: the unscaled values are
    multiples of 2^-4 in [-2, 2], so with a power-of-two scale of 2^4 .. 2^10 the scaled ones are
    exact in bf16 and fp16, the pack's 1 / scale gives the unscaled ones back exactly and every
    partial sum of three ranks is exact in fp32 whatever the order."""
    rng = np.random.default_rng(1000 * step + rank)
    out = [(rng.integers(-32, 33, m) * 2.0 ** -4 * scale).astype(np.float32) for m in LENS]
    if step == 1 and rank == 1:
        out[BAD[0]][BAD[1]] = np.inf
    return out


def _rank_main(rank, world, port, mode, kind, outdir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import collections
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=TIMEOUT))
    try:
        torch.cuda.set_device(0)
        from chocosgd_amd import codec, utils
        from chocosgd_amd.communication import get_aggregators

        class HostStaged:
            """gloo reduces host tensors: the flat buffer is staged through host memory."""

            def __init__(self, inner):
                self.inner, self.world_size = inner, inner.world_size

            def _agg(self, data, op=None, distributed=True):
                return self.inner._agg(data.cpu(), op=op, distributed=distributed).to(data.device)

        ranks = list(range(world))
        agg = HostStaged(get_aggregators(cur_rank=rank, world=ranks, neighbors_info={r: 1.0 / world for r in ranks},
                                         aggregator_type="centralized"))
        dtype = {"fp32": torch.float32, "fp16": torch.float16}[mode.split("_")[0]]
        params = [torch.nn.Parameter(torch.from_numpy(v).cuda().to(dtype)) for v in params0()]
        groups = [{"params": [p], "name": f"p{i}", "lr": HP[i % 3][0], "weight_decay": HP[i % 3][1],
                   "momentum": HP[i % 3][2], "dampening": HP[i % 3][3], "nesterov": HP[i % 3][4]}
                  for i, p in enumerate(params)]
        names = list(enumerate(g["name"] for g in groups))
        mw = utils.MasterWeights(groups, names) if mode.endswith("_master") else None
        scaler = utils.LossScaler("cuda", init_scale=SCALE, growth_interval=INTERVAL)
        state = collections.defaultdict(dict)
        out = {}
        cat = lambda ts: np.concatenate([t.detach().float().cpu().numpy().reshape(-1) for t in ts])  # noqa: E731
        upd = "param_sgd_master_flatgrad_scaled_kernel" if mw is not None else "param_sgd_flatgrad_scaled_kernel"
        for step in range(STEPS):
            for p, g in zip(params, grads_of(rank, step, scaler.get_scale())):
                p.grad = torch.from_numpy(g).cuda().to(dtype)
            before = codec.launch_count(upd), codec.launch_count("loss_scale_update_kernel")
            bits = utils.allreduce_sgd_step(groups, names, state, agg, master=mw, loss_scale=scaler,
                                            clip_norm=CLIP if kind == "both" else None)
            torch.cuda.synchronize()
            after = codec.launch_count(upd), codec.launch_count("loss_scale_update_kernel")
            assert bits == 32 * (sum(LENS) + 1) and after[1] - before[1] == 1
            assert after[0] - before[0] == codec.params_sgd_flatgrad_launches(len(LENS))
            assert scaler.skipped() == (step == 1), "every rank skips the step one of them overflowed in"
            out[f"p{step}"], out[f"g{step}"] = cat(params), cat([p.grad for p in params])
            out[f"buf{step}"] = cat([state[p]["momentum_buffer"] for p in params if "momentum_buffer" in state[p]])
            out[f"scale{step}"] = scaler._scale.cpu().numpy().copy()
            out[f"tracker{step}"] = scaler._growth_tracker.cpu().numpy().copy()
            out[f"last{step}"] = scaler.last.cpu().numpy().copy()
            if mw is not None:
                out[f"m{step}"] = mw.buffer.cpu().numpy().copy()
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), **out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def main():
    mode, world, kind, outdir = sys.argv[1], int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank_main, args=(rank, world, port, mode, kind, outdir)) for rank in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=TIMEOUT * (STEPS + 2))
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.is_alive():
            p.terminate()
    if any(c != 0 for c in codes):
        print(f"rank exit codes {codes}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()

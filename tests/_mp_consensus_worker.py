"""Multi-process consensus evaluation for tests/test_gpu_consensus_multiproc.py (not a test module).

    python tests/_mp_consensus_worker.py <fp32|bf16> <world> <outdir>

This launcher process never touches the GPU: it starts `world` rank processes (spawn).  Each
builds its own model on the one GPU, the centralized aggregator as the reference builds it
(get_aggregators(..., "centralized")) over gloo behind a host staging wrapper, runs
auxiliary.consensus_eval(avg_out=copy) and then agg_model in place, and saves the sum it
received, its averaged copy, its stats and its model after agg_model to <outdir>.  Every
collective has TIMEOUT seconds.
"""
import datetime
import os
import socket
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = [1, 2, 3, 7, 8, 9, 31, 33, 4097, 16, 8200, 20]  # test_gpu_param_sgd.BASE
TIMEOUT = 60  # seconds, per collective and for the rendezvous


def params_of(rank):
    """Rank `rank`'s model (fp32 values; the model narrows them): a common part and a drift."""
    common = np.random.default_rng(77).standard_normal(sum(LENS)).astype(np.float32)
    drift = np.random.default_rng(500 + rank).standard_normal(sum(LENS)).astype(np.float32)
    flat = (common + np.float32(0.05) * drift).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum(LENS)])
    return [flat[offs[i]:offs[i + 1]] for i in range(len(LENS))]


def _rank_main(rank, world, port, mode, outdir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=TIMEOUT))
    try:
        torch.cuda.set_device(0)
        from chocosgd_amd import auxiliary, codec
        from chocosgd_amd.communication import CentralizedAggregation

        seen = []

        class HostStaged(CentralizedAggregation):
            """gloo reduces host tensors: the flat buffer is staged through host memory."""

            def _agg(self, data, op=None, distributed=True, **kw):
                out = super()._agg(data.cpu(), op=op, distributed=distributed, **kw).to(data.device)
                seen.append(out.detach().float().cpu().numpy().copy())
                return out

        ranks = list(range(world))
        agg = HostStaged(rank, ranks, {r: 1.0 / world for r in ranks})
        dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[mode]

        class Model(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.ps = torch.nn.ParameterList(
                    [torch.nn.Parameter(torch.from_numpy(v.copy()).cuda().to(dtype)) for v in params_of(rank)])

        model, copy = Model(), Model()
        for p in copy.parameters():
            p.data.zero_()
        cat = lambda ts: np.concatenate([t.detach().float().cpu().numpy().reshape(-1) for t in ts])  # noqa: E731
        names = ("param_consensus_kernel", "param_consensus_total_kernel")
        before = [codec.launch_count(nm) for nm in names]
        stats, dists = auxiliary.consensus_eval(model, agg, avg_out=copy, per_tensor=True)
        torch.cuda.synchronize()
        assert [codec.launch_count(nm) - b for nm, b in zip(names, before)] == [1, 1] and len(seen) == 1
        out = {"x": cat(model.parameters()), "sum": seen[0], "avg": cat(copy.parameters()),
               "stats": stats.cpu().numpy().copy(), "dists": dists.cpu().numpy().copy()}
        agg.agg_model(model, "avg")
        torch.cuda.synchronize()
        assert [codec.launch_count(nm) - b for nm, b in zip(names, before)] == [2, 1] and len(seen) == 2
        out["agg_model"] = cat(model.parameters())
        np.savez(os.path.join(outdir, f"rank{rank}.npz"), **out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def main():
    mode, world, outdir = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    import multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank_main, args=(r, world, port, mode, outdir)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=TIMEOUT * 3)
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.is_alive():
            p.terminate()
    if any(c != 0 for c in codes):
        print(f"rank exit codes {codes}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()

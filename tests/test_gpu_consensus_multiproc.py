"""Consensus evaluation across processes: a world of 3 over gloo on the one GPU
(tests/_mp_consensus_worker.py, fresh interpreters)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, same_bits
import _consensus_oracle as CO
import _mp_consensus_worker as W
import _sgd_oracle as SO

pytestmark = pytest.mark.gpu
WORLD = 3


@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_consensus_eval_across_processes(mode, tmp_path):
    """Every rank runs consensus_eval(avg_out=copy), then agg_model in place.  The ranks'
    averaged copies are bit-identical to each other and to the model applied to the sum each
    rank received; each rank's distance is the model's for its own parameters; agg_model
    leaves all three models bit-identical."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_mp_consensus_worker.py"), mode, str(WORLD),
                        str(tmp_path)], capture_output=True, text=True, timeout=W.TIMEOUT * 4)
    assert r.returncode == 0, r.stderr[-4000:]
    got = [dict(np.load(tmp_path / f"rank{q}.npz")) for q in range(WORLD)]
    names = [mode] * len(W.LENS)
    xs = [SO.to_grid(np.concatenate(W.params_of(q)), mode) for q in range(WORLD)]
    exact = np.sum([x.astype(np.float64) for x in xs], axis=0)
    for q in range(WORLD):
        assert same_bits(got[q]["x"], xs[q])
        # whatever order gloo added in, the sum is the exact one up to two fp32 roundings
        assert np.all(np.abs(got[q]["sum"] - exact) <= 2.0 ** -22 * np.maximum(np.abs(exact), 1.0))
        avg, out, dists = CO.consensus(xs[q], got[q]["sum"], float(WORLD), W.LENS, names)
        assert same_bits(got[q]["avg"], avg), q
        assert same_bits(got[q]["stats"], out) and same_bits(got[q]["dists"], dists), q
        assert out[0] > 0 and np.isfinite(out).all()
        assert same_bits(got[q]["agg_model"], got[0]["agg_model"]) and same_bits(got[q]["avg"], got[0]["avg"])
        assert same_bits(got[q]["agg_model"], got[q]["avg"]), "agg_model in place is the averaged copy"

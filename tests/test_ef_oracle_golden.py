"""The numpy model of choco_params_ef and choco_sign_local_residual (tests/_ef_oracle.py) against
the stages the reference's own DeepSqueeze.step and EF_SignSGD.step recorded on the general
input set (tests/golden/ef_general_*.npz, gen_golden_ef.py), bit for bit (a NaN matches any
NaN): the accumulate, the residual with the recorded norms, and both tails.  No GPU."""
import numpy as np
import pytest

from conftest import golden, same_bits
import _ef_oracle as EO

STEPS = (1, 2)
TINY = np.finfo(np.float32).tiny


def _before(fx, t, key, first):
    return fx[first] if t == 1 else fx[f"s{t - 1}_{key}"]


@pytest.mark.parametrize("t", STEPS)
@pytest.mark.parametrize("run", ["ds_topk", "ds_sign"])
def test_accumulate_stage(run, t):
    """deep_squeeze.py:101-108: memory += the packed params."""
    fx = golden(f"ef_general_{run}")
    assert same_bits(EO.accum(_before(fx, t, "mem", "mem0"), fx[f"s{t}_sgd"]), fx[f"s{t}_handed"])


@pytest.mark.parametrize("t", STEPS)
@pytest.mark.parametrize("run", ["ds_sign", "efsign"])
def test_residual_stage_with_the_recorded_norms(run, t):
    """deep_squeeze.py:416-422 with :115, ef_sign_sgd.py:153 with :104-106."""
    fx = golden(f"ef_general_{run}")
    resid, u = EO.residual(fx[f"s{t}_handed"], fx[f"s{t}_norms"], fx["layout"].tolist())
    assert same_bits(u, fx[f"s{t}_local"])
    assert same_bits(resid, fx[f"s{t}_mem"])


@pytest.mark.parametrize("t", STEPS)
def test_topk_residual_is_a_subtraction_at_the_selected_positions(t):
    """memory - local with local zero off the selection: m - 0 = m bit for bit (-0 included), and
    m + (-v) = m - v at the selected positions."""
    fx = golden("ef_general_ds_topk")
    handed, local, mem = fx[f"s{t}_handed"], fx[f"s{t}_local"], fx[f"s{t}_mem"]
    assert same_bits(EO.sub32(handed, local), mem)
    sel = local != 0
    off = ~sel & ~np.isnan(local)
    assert same_bits(mem[off], handed[off])
    assert same_bits(EO.add32(handed[sel], -local[sel]), mem[sel])


@pytest.mark.parametrize("t", STEPS)
@pytest.mark.parametrize("run", ["ds_topk", "ds_sign"])
def test_deepsqueeze_tail(run, t):
    """deep_squeeze.py:125-126: params_tb.buffer += agg, unpack."""
    fx = golden(f"ef_general_{run}")
    p_new, flat = EO.apply(fx[f"s{t}_agg"], fx[f"s{t}_sgd"])
    assert same_bits(p_new, fx[f"s{t}_params"])
    assert same_bits(flat, fx[f"s{t}_agg"])


@pytest.mark.parametrize("t", STEPS)
def test_ef_sign_tail(t):
    """ef_sign_sgd.py:218, :113-122: a true division by the world size, -lr *, the add."""
    fx = golden("ef_general_efsign")
    lr = float(fx["hp"][0])
    p_new, flat = EO.apply(fx[f"s{t}_summed"], fx[f"s{t}_sgd"], divisor=3 * 1.0, lr=lr)
    assert same_bits(flat, fx[f"s{t}_agg"])
    assert same_bits(p_new, fx[f"s{t}_params"])
    assert same_bits(fx[f"s{t}_sgd"], _before(fx, t, "params", "p0")), "the params wait for the tail"


def test_fixtures_hold_the_planted_values():
    tk, ef = golden("ef_general_ds_topk"), golden("ef_general_efsign")
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)  # noqa: E731
    at = np.flatnonzero((bits(tk["s1_sgd"]) == 0x80000000) & (bits(tk["s1_agg"]) == 0))
    assert at.size >= 1 and np.all(bits(tk["s1_params"][at]) == 0), "(-0) + (+0) is +0"
    for fx in (tk, ef):
        assert np.isinf(fx["s1_handed"]).any() and np.isnan(fx["s1_handed"]).any()
    nlr = np.float32(-ef["hp"][0])
    quotient = product = False
    for t in STEPS:
        q, s = ef[f"s{t}_agg"], ef[f"s{t}_summed"]
        quotient |= bool(np.any((q != 0) & (np.abs(q) < TINY) & (np.abs(s) >= TINY)))
        with np.errstate(all="ignore"):
            pr = (nlr * q).astype(np.float32)
        product |= bool(np.any((pr != 0) & (np.abs(pr) < TINY)))
    assert quotient and product


def test_every_mode_of_the_model_on_one_element():
    """The mode table of EO.ef on values worked by hand: 6 / 3 = 2, -0.5 * 2 = -1."""
    flat, x = np.float32([6.0]), np.float32([10.0])
    want = {EO.ACCUM: (10.0, 16.0), EO.APPLY: (16.0, 6.0), EO.APPLY | EO.DIV: (12.0, 2.0),
            EO.APPLY | EO.SCALE: (7.0, 6.0), EO.APPLY | EO.DIV | EO.SCALE: (9.0, 2.0)}
    assert sorted(want) == sorted(EO.MODES)
    for mode, (p, f) in want.items():
        got_p, got_f = EO.ef(mode, flat, x, lr=0.5, divisor=3.0)
        assert (float(got_p[0]), float(got_f[0])) == (p, f), mode
    # one narrowing: 1 + 2^-9 lies halfway between two bf16 values and goes to the even one
    p, _ = EO.apply(np.float32([2.0 ** -9]), np.float32([1.0]), dtype="bf16")
    assert float(p[0]) == 1.0

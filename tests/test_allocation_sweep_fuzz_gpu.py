"""Seeded random allocation sweeps on the GPU (tests/allocation_sweep_fuzz.py draws them, its docstring says from what)
against the restatement: per scenario final, holdings, paid and ruin_period on their bits, depleted_at exactly, of the
record the integer fields, min, max and bucket counts with ==, the two double sums to the relative 1e-12 of
tests/test_gpu_parity.py against oracle.values_stats."""
import numpy as np
import pytest

import allocation_sweep_fuzz as F

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_seeded_random_sweeps(oracle):
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    eng = S.Engine(0)
    try:
        for c in F.cases(oracle):
            want = F.reference(oracle, c)
            n_bins, lo, hi, below = c["hist"]
            sim = S.Engine.make_sim(c["n"], c["P"], S.MODE_TABLE if c["mode"] == "table" else S.MODE_GAUSSIAN, c["seed"], first_path=c["first"],
                                    initial_capital=c["capital"], n_bins=n_bins, hist_lo=lo, hist_hi=hi, below_threshold=below, exact_div=c["exact"])
            law = {}
            if c["mode"] == "table":
                eng.set_asset_table(c["assets"])
            else:
                law = dict(means=c["law"][0], factor=c["law"][1])
            sc = c["scenarios"]
            raw = eng.simulate_allocation_sweep_raw(sim, [s[0] for s in sc], [s[1] for s in sc], [s[2] for s in sc], [s[3] for s in sc],
                                                    [s[4] for s in sc], want_final=True, want_holdings=True, want_paid=True,
                                                    want_ruin_period=True, want_stats=True, want_depleted_at=True, **law)
            eng.sync()
            out = {k: t.cpu().numpy() for k, t in raw.items() if k != "n_assets"}
            rec = int(eng._L.smmc_stats_bytes(n_bins))
            for s, w in enumerate(want):
                tag = (c["id"], s)
                for key in ("final", "holdings", "paid"):
                    assert np.array_equal(_bits(out[key][s]), _bits(w[key])), (tag, key)
                assert np.array_equal(out["ruin_period"][s].view(np.uint32), w["ruin_period"]), tag
                assert np.array_equal(out["depleted_at"][s].view(np.uint64), w["depleted_at"]), tag
                st = stats_from_bytes(out["stats_raw"][s].tobytes()[:rec])
                ost, ohist = oracle.values_stats(w["final"], below, n_bins, lo, hi)
                assert (st.count, st.below, st.underflow, st.overflow, st.min, st.max) == \
                       (ost.count, ost.below, ost.underflow, ost.overflow, ost.min, ost.max), tag
                assert np.array_equal(st.hist, ohist), tag
                assert st.sum == pytest.approx(ost.sum, rel=1e-12) and st.sumsq == pytest.approx(ost.sumsq, rel=1e-12), tag
    finally:
        eng.close()

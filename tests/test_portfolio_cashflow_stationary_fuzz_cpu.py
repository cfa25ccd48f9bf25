"""The cases of tests/portfolio_cashflow_stationary_fuzz.py on the restatement alone: they are requests the header accepts,
the draw is reproducible, the restatement keeps its invariants on every one, the cases spread over what the row rule
depends on (the renewal probability's edges, tables smaller than a segment and on both sides of the dense limit, tails),
and the fuzz is not vacuous."""
import time

import numpy as np

import portfolio_cashflow_stationary_fuzz as F
import portfolio_reference as pref
from stock_market_monte_carlo_amd import _lib

f32 = np.float32


def test_the_cases_are_valid_reproducible_and_keep_the_invariants(oracle):
    assert any(s[0] == "smmc_engine_simulate_portfolio_cashflow_stationary" for s in _lib.SYMBOLS)  # the feature's own entry
    t0 = time.time()
    cases = list(F.cases(oracle))
    again = list(F.cases(oracle))
    assert len(cases) == F.COUNT and 24 <= F.COUNT <= 48
    taking = depleted_part = 0
    for c, d in zip(cases, again):
        assert F.brief(c) == F.brief(d) and all(np.array_equal(c["schedule"][k], d["schedule"][k]) for k in c["schedule"])
        n, P, K, T, q = c["n"], c["P"], c["K"], c["T"], c["q"]
        assert 1 <= K <= _lib.MAX_ASSETS and len(c["weights"]) == K and abs(sum(np.float64(w) for w in c["weights"]) - 1.0) <= 1e-6
        assert all(w >= 0 for w in c["weights"])
        assert 0 <= c["seed"] < 1 << 64 and c["first"] + n < 1 << 63 and 1 <= P <= 64 and 1 <= n <= 1502 and 0 <= q <= _lib.RENEW_Q16_ONE
        assert c["assets"].shape == (T, K) and c["assets"].dtype == np.float32 and T * K <= 16384
        kw = c["schedule"]
        assert np.isfinite(f32(kw.get("floor", 0.0))) and kw.get("floor", 0.0) >= 0
        for key in ("amount", "fraction"):
            assert np.isfinite(f32(kw.get(key, 0.0)))
        for key in ("amounts", "fractions"):
            assert key not in kw or (kw[key].shape == (P,) and kw[key].dtype == np.float32 and np.isfinite(kw[key]).all())
        # the rows: every period reads the parent's row of that period or the row behind the one before
        rows = F.Q.rows(oracle, T, n, P, q, c["seed"], c["first"])
        cand = pref.row_indices(oracle, T, c["seed"], c["first"], n, P)
        assert rows.shape == (n, P) and rows.min() >= 0 and rows.max() < T and np.array_equal(rows[:, 0], cand[:, 0])
        on = (rows[:, :-1] + 1) % T
        assert ((rows[:, 1:] == cand[:, 1:]) | (rows[:, 1:] == on)).all()
        if q == 0:
            assert np.array_equal(rows[:, 1:], on)
        if q == _lib.RENEW_Q16_ONE:
            assert np.array_equal(rows, cand)
        out = F.reference(oracle, c)
        # the restatement's invariants
        assert int(out["depleted_at"].sum()) == n and np.array_equal(out["depleted_at"], np.bincount(out["ruin_period"], minlength=P + 1))
        dead = out["ruin_period"] > 0
        assert not out["final"][dead].any() and not out["holdings"][:, dead].any() and out["holdings"].shape == (K, n)
        assert (out["final"][~dead] > f32(kw.get("floor", 0.0))).all()
        if c["form"] == "contributions":
            assert not dead.any() and (out["paid"] < 0).all()
        else:
            taking += 1
            depleted_part += 0 < int(dead.sum()) < n
    assert {c["K"] for c in cases} == {1, 2, 3, 4} and {c["form"] for c in cases} == {"amount", "fraction", "varying", "contributions"}
    assert any(c["first"] >= 1 << 61 for c in cases) and any(c["seed"] >= 1 << 63 for c in cases) and any(c["exact"] for c in cases)
    assert any(c["T"] > 2048 for c in cases) and any(c["T"] < 8 for c in cases) and any(c["T"] == 1 for c in cases)
    assert any(c["q"] < 8192 for c in cases) and any(c["q"] > 32768 for c in cases) and any(c["q"] in (0, 1, 65535, 65536) for c in cases)
    assert len({c["P"] % 8 for c in cases}) >= 5  # tails
    assert any("amounts" in c["schedule"] and c["P"] % 8 for c in cases)  # a varying schedule whose last segment is a tail
    assert any(0.0 in c["weights"] for c in cases)
    print(f"of {len(cases)} cases {taking} take money out, {depleted_part} of them deplete part of their paths; "
          f"references and sizing {time.time() - t0:.1f} s")
    # the rest have a single path or period, a single row (one path many times), or too short a run for the drawn scale
    assert depleted_part >= taking // 2

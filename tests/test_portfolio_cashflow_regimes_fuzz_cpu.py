"""The cases of tests/portfolio_cashflow_regimes_fuzz.py on the restatement alone: they are requests the header accepts, the
draw is reproducible, the restatement keeps its invariants on every one, the generator reaches every K and schedule form
with and without the IEEE-divide flag (every instantiation the flag and the forms can name) and both regimes, and the fuzz
is not vacuous."""
import time

import numpy as np

import portfolio_cashflow_regimes_fuzz as F
from stock_market_monte_carlo_amd import _lib

f32 = np.float32


def test_the_cases_are_valid_reproducible_and_keep_the_invariants(oracle):
    assert any(s[0] == "smmc_engine_simulate_portfolio_cashflow_regimes" for s in _lib.SYMBOLS)  # the feature's own entry
    t0 = time.time()
    cases = list(F.cases(oracle))
    again = list(F.cases(oracle))
    assert len(cases) == F.COUNT == 40
    taking = depleted_part = both_regimes = 0
    for c, d in zip(cases, again):
        assert F.brief(c) == F.brief(d) and all(np.array_equal(c["schedule"][k], d["schedule"][k]) for k in c["schedule"])
        n, P, K = c["n"], c["P"], c["K"]
        assert 1 <= K <= _lib.MAX_ASSETS and len(c["weights"]) == K and abs(sum(np.float64(w) for w in c["weights"]) - 1.0) <= 1e-6
        assert all(w >= 0 for w in c["weights"])
        assert 0 <= c["seed"] < 1 << 64 and c["first"] + n < 1 << 63 and 1 <= P <= 64 and 1 <= n <= 1502
        assert all(0 <= q <= _lib.REGIME_Q16_ONE for q in c["prob"][0] + (c["prob"][1],))
        for m, f in zip(c["means"], c["factors"]):
            assert len(m) == K and f.shape == (K, K) and f.dtype == np.float32 and np.isfinite(f).all()
            assert not np.triu(f, 1).any() and (np.diag(f) >= 0).all()
            assert all(100.0 + m[k] - 7.0 * float(np.abs(f[k]).sum()) > 1.0 for k in range(K))  # the divide rule has its bounds
        kw = c["schedule"]
        assert np.isfinite(f32(kw.get("floor", 0.0))) and kw.get("floor", 0.0) >= 0
        for key in ("amount", "fraction"):
            assert np.isfinite(f32(kw.get(key, 0.0)))
        for key in ("amounts", "fractions"):
            assert key not in kw or (kw[key].shape == (P,) and kw[key].dtype == np.float32 and np.isfinite(kw[key]).all())
        s = F.Q.states(oracle, n, P, c["prob"], c["seed"], c["first"])
        assert s.shape == (n, P) and set(np.unique(s)) <= {0, 1}
        both_regimes += len(np.unique(s)) == 2
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
    # every instantiation: K x (constant | varying schedule), each with the flag (the IEEE divide) and without it
    assert {F.instantiation(c) for c in cases} == {(K, v) for K in (1, 2, 3, 4) for v in (False, True)}
    assert {F.instantiation(c) for c in cases if c["exact"]} | {F.instantiation(c) for c in cases if c["form"] != "contributions"} \
        == {(K, v) for K in (1, 2, 3, 4) for v in (False, True)}
    assert {c["form"] for c in cases} == {"amount", "fraction", "varying", "contributions"}
    assert any(c["first"] >= 1 << 61 for c in cases) and any(c["seed"] >= 1 << 63 for c in cases) and any(c["exact"] for c in cases)
    assert both_regimes >= len(cases) // 2
    assert len({c["P"] % 8 for c in cases}) >= 5 and len({c["P"] % 4 for c in cases}) == 4  # tails
    assert any(0.0 in c["weights"] for c in cases)
    print(f"of {len(cases)} cases {taking} take money out, {depleted_part} of them deplete part of their paths, {both_regimes} visit both "
          f"regimes; references and sizing {time.time() - t0:.1f} s")
    assert depleted_part >= taking // 2

"""The seeded random cases of tests/glide_reference.py (fuzz_cases) without a GPU: every case is within the contract, and
none is vacuous by the two conditions of tests/test_glide_cpu.py -- its schedule depletes between 10 % and 90 % of the paths
(a schedule of contributions only depletes none, as the FAST per-period rows of the ledger), and where a change can act on
the value (K >= 2, a change before the last period) at least half of the final values differ in bits from the same case
without its changes; where none can, the outputs are the parent's."""
import numpy as np

import glide_reference as G

f32 = np.float32


def test_the_cases_cover_what_the_module_says_and_none_is_vacuous(oracle):
    cases = list(G.fuzz_cases(oracle))
    assert len(cases) == G.FUZZ_COUNT == 36
    acting = 0
    for c in cases:
        K, P = c["K"], c["P"]
        assert 1 <= K <= 4 and P <= 24 and c["n"] <= 3000 and 0 <= len(c["changes"]) <= 6 and c["first"] + c["n"] < 1 << 63, G.brief(c)
        after = [a for a, _ in c["changes"]]
        assert after == sorted(set(after)) and all(a >= 1 for a in after), G.brief(c)
        for row in [c["weights"]] + [r for _, r in c["changes"]]:
            r32 = np.asarray(row, f32)
            assert r32.size == K and (r32 >= 0).all() and abs(float(r32.astype(np.float64).sum()) - 1.0) <= 1e-6, G.brief(c)
        a = G.multipliers(oracle, c)
        out = G.simulate(a, c["weights"], c["changes"], c["R"], capital=c["capital"], **c["schedule"])
        plain = G.simulate(a, c["weights"], (), c["R"], capital=c["capital"], **c["schedule"])
        if c["depletes"]:
            assert 0.1 <= G.depleted_share(out) <= 0.9, (G.brief(c), G.depleted_share(out))
        else:
            assert not out["ruin_period"].any() and (np.asarray(c["schedule"]["amounts"]) < 0).all(), G.brief(c)
        if K >= 2 and any(t < P for t in after):
            acting += 1
            assert G.differing_share(out, plain) >= 0.5, (G.brief(c), G.differing_share(out, plain))
        elif not any(t <= P for t in after) or K == 1:
            for key in G.KEYS:
                assert out[key].tobytes() == plain[key].tobytes(), (G.brief(c), key)
        else:  # a change at P alone: the last settlement
            assert out["final"].tobytes() == plain["final"].tobytes() and out["holdings"].tobytes() != plain["holdings"].tobytes(), G.brief(c)
    assert acting >= 20
    assert {c["mode"] for c in cases} == {"table", "gauss"} and {c["K"] for c in cases} == {1, 2, 3, 4}
    assert any(c["first"] >= 1 << 61 for c in cases) and any(c["T"] > 2048 for c in cases if c["mode"] == "table")
    assert any(not c["changes"] for c in cases) and any(min(min(r) for _, r in c["changes"]) == 0.0 for c in cases if c["changes"])

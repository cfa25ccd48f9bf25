"""smmc_engine_simulate_guardrails on the device against the numpy restatement of its contract
(tests/guardrails_reference.py): final values, holdings, totals paid, periods of depletion, the amounts in force (last and
lowest), the per-path counts of cuts and raises and the three count arrays on their bits; of the record the integer
counters, buckets, min and max on their bits, the two double sums to the relative 1e-12 of tests/test_gpu_parity.py.

Shapes: those of tests/feature_matrix.py -- 64 kW 2 + 37 paths with kW = 4 (table) or 8 (Gaussian), path ids from
2^32 - 100 on, 9 periods on a dense table (E = 2, R = 4), 5 on a four-draw table and in Gaussian mode (E = 2, R = 3) -- for
every instantiation (three modes x K = 1 .. 4), and the edges P = 1, E = 1, E = P, E > P, amount_min == A0 == amount_max and
a review with a rebalance in the partial block.  tests/test_guardrails_cpu.py shows on the restatement alone that every
case cuts, raises, clamps and depletes part of its paths.

The three identities of include/smmc.h are checked against smmc_engine_simulate_portfolio_cashflow and
smmc_engine_simulate_cashflow ON THE DEVICE, whatever divide those take.  The later walk trips run in a fresh child
process with SMMC_BLOCKS_PER_CU=1, as in tests/test_real_cashflow_gpu.py.

On the commit before this feature every test here fails: the symbols do not exist."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import guardrails_reference as G

pytestmark = pytest.mark.gpu


def test_raw_and_to_host_give_the_same_bytes_on_an_engine_with_its_own_stream():
    """300 paths, 8 periods, every want on: the device tensors, read through torch's stream, against the host entry's."""
    import raw_to_host_check
    raw_to_host_check.check("guardrails")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANTS = ("final", "holdings", "paid", "ruin_period", "stats", "depleted_at", "amount_last", "amount_lowest", "cuts", "raises",
         "cuts_at", "raises_at")
ALL = {"want_" + k: True for k in WANTS}
KEYS = tuple("stats_raw" if k == "stats" else k for k in WANTS)
PARENT_ALL = dict(want_holdings=True, want_paid=True, want_ruin_period=True, want_stats=True, want_depleted_at=True)
f32 = np.float32


def _same_floats(got, want, tag):
    """On the bits, NaN matching NaN (the payload of an invalid operation is the machine's own)."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, tag
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), tag
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), tag


def _check_record(oracle, st, values, tag, stats_range):
    bins, lo, hi, below = stats_range
    values = np.ascontiguousarray(values, dtype=np.float32)
    ost, ohist = oracle.values_stats(values, below, bins, lo, hi)
    assert st.count == ost.count == values.size, tag
    assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), tag
    _same_floats([st.min, st.max], [ost.min, ost.max], tag)
    assert np.array_equal(st.hist, ohist) and (not bins or int(st.hist.sum()) + st.underflow + st.overflow == values.size), tag
    d = values.astype(np.float64)
    if np.isfinite(d).all():
        assert st.sum == pytest.approx(math.fsum(d.tolist()), rel=1e-12), tag
        assert st.sumsq == pytest.approx(math.fsum((d * d).tolist()), rel=1e-12), tag


def _check_outputs(out, want, tag):
    """out: numpy arrays by key (the integer outputs as the engine's signed tensors or as unsigned arrays)."""
    n = want["final"].size
    for key in ("final", "paid", "amount_last", "amount_lowest", "holdings"):
        _same_floats(out[key], want[key], (tag, key))
    for key in ("ruin_period", "cuts", "raises"):
        assert np.array_equal(out[key].view(np.uint32), want[key]), (tag, key)
    for key in ("depleted_at", "cuts_at", "raises_at"):
        assert np.array_equal(out[key].view(np.uint64), want[key]), (tag, key)
    assert int(out["depleted_at"].view(np.uint64).sum()) == n, tag
    assert int(out["cuts_at"].view(np.uint64).sum()) == int(out["cuts"].view(np.uint32).sum(dtype=np.uint64)), tag
    assert int(out["raises_at"].view(np.uint64).sum()) == int(out["raises"].view(np.uint32).sum(dtype=np.uint64)), tag
    assert out["cuts_at"][0] == 0 and out["raises_at"][0] == 0, tag


def _numpy(raw):
    return {k: t.cpu().numpy() for k, t in raw.items() if k != "n_assets" and t is not None}


def _engine(made, c):
    import stock_market_monte_carlo_amd as S
    key = ("gauss",) if c["mode"] == "gauss" else ("table", c["K"], id(G.M.assets(c)))
    if key not in made:
        made[key] = S.Engine(0)
        if c["mode"] == "table":
            made[key].set_asset_table(G.M.assets(c))
    return made[key]


@pytest.fixture(scope="module")
def engines():
    made = {}
    yield lambda c: _engine(made, c)
    for e in made.values():
        e.close()


def _sim(c, n=None, first=0, stats=True, **kw):
    import stock_market_monte_carlo_amd as S
    bins, lo, hi, below = G.hist_range(c)
    if stats:
        kw = dict(n_bins=bins, hist_lo=lo, hist_hi=hi, below_threshold=below, **kw)
    kw.setdefault("exact_div", bool(c.get("exact", False)))  # a fuzz case may ask for the flag, which changes nothing
    return S.Engine.make_sim(c["n"] if n is None else n, c["P"], S.MODE_GAUSSIAN if c["mode"] == "gauss" else S.MODE_TABLE,
                             c.get("seed", G.SEED), first_path=c.get("first", G.FIRST_PATH) + first, initial_capital=c["capital"], **kw)


def _law(c):
    return dict(zip(("means", "factor"), G.M.gauss_portfolio(c))) if c["mode"] == "gauss" else {}


def _args(c, rule):
    """The keyword arguments of Engine.simulate_guardrails* for a case and a rule."""
    return dict(rule, rebalance_every=c["R"], **_law(c))


def check_case(oracle, eng, c):
    """A case of tests/guardrails_reference.py (or of tests/guardrails_fuzz.py) against its restatement."""
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    want = G.reference(oracle, c)
    out = _numpy(eng.simulate_guardrails_raw(_sim(c), G.weights(c), **_args(c, G.rule(oracle, c)), **ALL))
    _check_outputs(out, want, c["id"])
    _check_record(oracle, stats_from_bytes(out["stats_raw"].tobytes()), want["final"], c["id"], G.hist_range(c))
    return out


# 1
@pytest.mark.parametrize("c", G.CASES + G.EDGES, ids=[c["id"] for c in G.CASES + G.EDGES])
def test_outputs_bit_for_bit(oracle, engines, c):
    """Every instantiation and every edge: all twelve outputs, the counts exact."""
    check_case(oracle, engines(c), c)


def test_the_result_object(oracle, engines):
    c = G.CASES[5]
    want, n = G.reference(oracle, c), c["n"]
    r = engines(c).simulate_guardrails(_sim(c), G.weights(c), **_args(c, G.rule(oracle, c)), want_final=False, want_stats=True)
    assert r.final is None and r.holdings is None and r.paid is None and r.n_assets == c["K"]
    _check_record(oracle, r.stats, want["final"], c["id"], G.hist_range(c))
    for key in ("depleted_at", "cuts_at", "raises_at"):
        assert np.array_equal(getattr(r, key), want[key]), key
    assert r.ever_cut() == pytest.approx(float((want["cuts"] > 0).mean()))
    assert r.survival()[-1] == pytest.approx(want["depleted_at"][0] / n)
    assert np.array_equal(r.cut_by(), np.cumsum(want["cuts_at"].astype(np.float64)) / n) and r.cut_by()[-1] >= r.ever_cut()


def _parent_equal(got, parent, tag, record=True):
    for key in G.SHARED:
        assert got[key].tobytes() == parent[key].tobytes(), (tag, key)
    if record:
        assert got["stats_raw"].tobytes() == parent["stats_raw"].tobytes(), (tag, "stats_raw")


def _untouched(got, amount):
    a0 = f32(amount)
    assert (got["amount_last"] == a0).all() and (got["amount_lowest"] == a0).all()
    assert not got["cuts"].any() and not got["raises"].any() and not got["cuts_at"].any() and not got["raises_at"].any()


# 2
@pytest.mark.parametrize("c", [G.CASES[i] for i in (0, 3, 5, 7, 8, 10)], ids=[G.CASES[i]["id"] for i in (0, 3, 5, 7, 8, 10)])
def test_identity_1_no_review_or_a_neutral_rule_is_the_parent_with_the_constant_amount(oracle, engines, c):
    """Against smmc_engine_simulate_portfolio_cashflow in the divide the host chooses for IT and forced to the IEEE one."""
    from stock_market_monte_carlo_amd import _lib
    eng, w, r = engines(c), G.weights(c), G.rule(oracle, c)
    kinds = set()
    for exact in (False, True):
        sim = _sim(c, exact_div=exact)
        kinds.add(eng.portfolio_cashflow_divide_kind(sim, w, c["R"], amount=r["amount"], floor=r["floor"], **_law(c)))
        parent = _numpy(eng.simulate_portfolio_cashflow_raw(sim, w, c["R"], amount=r["amount"], floor=r["floor"], **_law(c), **PARENT_ALL))
        assert 0 < int(parent["depleted_at"][0]) < c["n"]
        never = dict(r, review_every=0)
        neutral = G.make_rule(r["amount"], c["E"], cut=1.0, raise_=1.0, index=1.0, floor=r["floor"])
        for rule in (never, neutral):
            got = _numpy(eng.simulate_guardrails_raw(sim, w, **_args(c, rule), **ALL))
            _parent_equal(got, parent, (c["id"], exact))
            _untouched(got, r["amount"])
    assert _lib.DIV_EXACT in kinds  # (whether the parent's own choice is the fast form is the parent's rule)


# 3
@pytest.mark.parametrize("c", [G.CASES[i] for i in (1, 2, 4, 6, 9, 11)], ids=[G.CASES[i]["id"] for i in (1, 2, 4, 6, 9, 11)])
def test_identity_2_open_bands_are_the_parent_with_the_indexed_amounts_array(oracle, engines, c):
    eng, w, r = engines(c), G.weights(c), G.rule(oracle, c)
    for E in (c["E"], 1, 3):
        rule = G.make_rule(r["amount"], E, index=1.02, cut=r["cut"], raise_=r["raise_"], floor=r["floor"])
        amounts = G.indexed_amounts(rule, c["P"])
        parent = _numpy(eng.simulate_portfolio_cashflow_raw(_sim(c), w, c["R"], amounts=amounts, floor=r["floor"], **_law(c), **PARENT_ALL))
        got = _numpy(eng.simulate_guardrails_raw(_sim(c), w, **_args(c, rule), **ALL))
        assert 0 < int(parent["depleted_at"][0]) < c["n"]
        _parent_equal(got, parent, (c["id"], E))
        assert not got["cuts"].any() and not got["raises"].any() and (got["amount_lowest"] == f32(r["amount"])).all()
        assert (got["amount_last"][got["ruin_period"] == 0] == amounts[-1]).all()


# 4
@pytest.mark.parametrize("c", [c for c in G.CASES if c["K"] == 1 and c["mode"] == "table"],
                         ids=[c["id"] for c in G.CASES if c["K"] == 1 and c["mode"] == "table"])
def test_identity_3_one_asset_with_weight_one_is_the_single_series_cash_flow(oracle, engines, c):
    import stock_market_monte_carlo_amd as S
    r = G.rule(oracle, c)
    rule = G.make_rule(r["amount"], c["E"], index=1.02, floor=r["floor"])
    amounts = G.indexed_amounts(rule, c["P"])
    single = S.Engine(0)
    try:
        single.set_table(np.ascontiguousarray(G.M.assets(c)[:, 0]))
        for exact in (False, True):
            sim = _sim(c, exact_div=exact)
            one = single.simulate_cashflow(sim, amounts=amounts, floor=r["floor"], want_paid=True, want_ruin_period=True, want_stats=True)
            for R in (0, c["R"]):
                got = _numpy(engines(c).simulate_guardrails_raw(sim, (1.0,), **_args(dict(c, R=R), rule), **ALL))
                assert got["final"].tobytes() == one.final.cpu().numpy().tobytes() and got["paid"].tobytes() == one.paid.cpu().numpy().tobytes()
                assert got["ruin_period"].tobytes() == one.ruin_period.cpu().numpy().tobytes()
                assert np.array_equal(got["depleted_at"].view(np.uint64), one.depleted_at) and 0 < int(one.depleted_at[0]) < c["n"]
                assert got["holdings"][0].tobytes() == got["final"].tobytes()
    finally:
        single.close()


# 5
@pytest.mark.parametrize("c", [G.CASES[2], G.CASES[6], G.EDGES[5]], ids=[G.CASES[2]["id"], G.CASES[6]["id"], G.EDGES[5]["id"]])
def test_determinism_shards_and_the_host_form(oracle, engines, c):
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd.engine import merge_stats_bytes
    eng, n, cut, w = engines(c), c["n"], 333, G.weights(c)
    kw = _args(c, G.rule(oracle, c))

    def run(first, count):
        raw = eng.simulate_guardrails_raw(_sim(c, n=count, first=first), w, **kw, **ALL)
        eng.sync()
        return {k: raw[k].cpu().numpy() for k in KEYS}

    whole, again, lo, hi = run(0, n), run(0, n), run(0, cut), run(cut, n - cut)
    for key in KEYS:  # two identical calls give the same bytes
        assert whole[key].tobytes() == again[key].tobytes(), key
    for key in ("final", "paid", "ruin_period", "amount_last", "amount_lowest", "cuts", "raises"):
        assert np.concatenate([lo[key], hi[key]]).tobytes() == whole[key].tobytes(), key
    assert np.concatenate([lo["holdings"], hi["holdings"]], axis=1).tobytes() == whole["holdings"].tobytes()
    for key in ("depleted_at", "cuts_at", "raises_at"):
        assert np.array_equal(lo[key] + hi[key], whole[key]), key
    merged = S.engine.stats_from_bytes(merge_stats_bytes([lo["stats_raw"].tobytes(), hi["stats_raw"].tobytes()]))
    want = S.engine.stats_from_bytes(whole["stats_raw"].tobytes())
    assert (merged.count, merged.below, merged.underflow, merged.overflow) == (want.count, want.below, want.underflow, want.overflow)
    assert merged.min == want.min and merged.max == want.max and np.array_equal(merged.hist, want.hist)
    assert merged.sum == pytest.approx(want.sum, rel=1e-12) and merged.sumsq == pytest.approx(want.sumsq, rel=1e-12)
    # a path does not depend on first_path: the second shard alone is the reference's tail
    ref = G.reference(oracle, c)
    assert hi["amount_last"].tobytes() == ref["amount_last"][cut:].tobytes() and np.array_equal(hi["cuts"].view(np.uint32), ref["cuts"][cut:])
    # the host form
    host = eng.simulate_guardrails_to_host(_sim(c), w, **kw, **ALL)
    for key in KEYS:
        h = host[key] if isinstance(host[key], bytes) else host[key].tobytes()
        assert h == whole[key].tobytes(), key
    empty = eng.simulate_guardrails_to_host(_sim(c, n=0), w, **kw, **ALL)
    assert not empty["depleted_at"].any() and not empty["cuts_at"].any() and empty["cuts"].size == 0 and empty["holdings"].shape == (c["K"], 0)
    assert not np.frombuffer(empty["stats_raw"], dtype=np.uint64)[:4].any()  # count, below, underflow, overflow
    # the accumulator is left zero: a plain simulate with buckets straight afterwards has its own record
    plain = S.Engine.make_sim(1000, 36, S.MODE_GAUSSIAN, 99, n_bins=G.BINS, hist_lo=G.LO, hist_hi=G.HI, below_threshold=G.BELOW)
    st = eng.read_stats(eng.simulate(plain, want_final=False, want_stats=True).stats_raw)
    o = oracle.counter_mc(oracle.make_params(oracle.MODE_GAUSSIAN, 36, 1000, 99, n_bins=G.BINS, hist_lo=G.LO, hist_hi=G.HI, below_threshold=G.BELOW))
    assert np.array_equal(st.hist, o["hist"]) and st.below == o["stats"].below and st.count == 1000


# 6
@pytest.mark.parametrize("c", [G.CASES[1], G.CASES[7]], ids=[G.CASES[1]["id"], G.CASES[7]["id"]])
def test_null_outputs_leave_the_others_unchanged(oracle, engines, c):
    """Every single output alone, and every output left out alone: what is written is what the full call writes."""
    eng, w = engines(c), G.weights(c)
    kw = _args(c, G.rule(oracle, c))
    full = _numpy(eng.simulate_guardrails_raw(_sim(c), w, **kw, **ALL))
    none = {k: False for k in ALL}
    for want in WANTS:
        key = "stats_raw" if want == "stats" else want
        only = _numpy(eng.simulate_guardrails_raw(_sim(c), w, **kw, **dict(none, **{"want_" + want: True})))
        assert set(only) == {key} and only[key].tobytes() == full[key].tobytes(), want
        rest = _numpy(eng.simulate_guardrails_raw(_sim(c), w, **kw, **dict(ALL, **{"want_" + want: False})))
        assert set(rest) == set(KEYS) - {key}, want
        for k in rest:
            assert rest[k].tobytes() == full[k].tobytes(), (want, k)


def test_the_exact_divide_flag_changes_nothing(oracle, engines):
    c = G.CASES[9]
    eng, w = engines(c), G.weights(c)
    kw = _args(c, G.rule(oracle, c))
    a = _numpy(eng.simulate_guardrails_raw(_sim(c), w, **kw, **ALL))
    b = _numpy(eng.simulate_guardrails_raw(_sim(c, exact_div=True), w, **kw, **ALL))
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_bad_arguments_are_refused_on_the_device_build_too(oracle, engines):
    from stock_market_monte_carlo_amd import SmmcError
    c = G.CASES[4]
    eng, w, r = engines(c), G.weights(c), G.rule(oracle, c)
    for bad in (dict(amount=0.0, amount_min=0.0), dict(cut=1.5), dict(raise_=0.5), dict(lower=1.0, upper=0.5), dict(amount_min=2 * r["amount"]),
                dict(index=float("nan")), dict(floor=-1.0)):
        with pytest.raises(SmmcError):
            eng.simulate_guardrails_raw(_sim(c), w, **_args(c, dict(r, **bad)))
    with pytest.raises(SmmcError):
        eng.simulate_guardrails_raw(_sim(c, stream=2), w, **_args(c, r))


# 7
_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
from oracle import oracle as O
O.build()
import guardrails_reference as G
import stock_market_monte_carlo_amd as S
out = sys.argv[3]
eng = S.Engine(0)
grid, _, cus = eng.geometry()
assert grid == cus, (grid, cus)
res = {"grid": grid}
for i, kW in ((1, 8), (5, 4)):
    c = G.CASES[i]
    if c["mode"] == "table":
        eng.set_asset_table(G.M.assets(c))
    law = dict(zip(("means", "factor"), G.M.gauss_portfolio(c))) if c["mode"] == "gauss" else {}
    rule = G.rule(O, c)
    for n in (2 * 64 * kW * grid + 37, 3 * 64 * kW * grid - 1):
        sim = S.Engine.make_sim(n, c["P"], S.MODE_GAUSSIAN if c["mode"] == "gauss" else S.MODE_TABLE, G.SEED, first_path=G.FIRST_PATH,
                                initial_capital=c["capital"], n_bins=G.BINS, hist_lo=G.LO, hist_hi=G.HI, below_threshold=G.BELOW)
        raw = eng.simulate_guardrails_raw(sim, G.weights(c), rebalance_every=c["R"], want_holdings=True, want_paid=True,
                                          want_ruin_period=True, want_stats=True, **rule, **law)
        eng.sync()
        for key, t in raw.items():
            if key != "n_assets":
                res[f"{i}:{n}:{key}"] = t.cpu().numpy()
eng.close()
np.savez(out, **res)
"""


def test_later_walk_trips_in_a_child_with_one_workgroup_per_cu(oracle, tmp_path):
    """K = 2, both modes: every wave makes a second and a third trip; the amount in force, its lowest value, the counts
    and both countdowns start again for every path."""
    import stock_market_monte_carlo_amd as S
    out = str(tmp_path / "trips.npz")
    env = dict(os.environ, SMMC_BLOCKS_PER_CU="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(ROOT, "tests"), out], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    got = np.load(out)
    grid = int(got["grid"])
    for i, kW in ((1, 8), (5, 4)):
        c = G.CASES[i]
        sizes = (2 * 64 * kW * grid + 37, 3 * 64 * kW * grid - 1)
        big = dict(c, n=max(sizes), id=c["id"] + "-trips", rule=G.rule(oracle, c))
        want = G.reference(oracle, big)
        for n in sizes:
            tag = (c["id"], n)
            cutn = {k: (v[:, :n] if k == "holdings" else v[:n]) for k, v in want.items() if not k.endswith("_at")}
            part = G.simulate(G.multipliers(oracle, big)[:n], G.weights(c), c["R"], big["rule"], capital=c["capital"]) if n != max(sizes) else want
            for k in ("depleted_at", "cuts_at", "raises_at"):
                cutn[k] = part[k]
            _check_outputs({k: got[f"{i}:{n}:{k}"] for k in KEYS if k != "stats_raw"}, cutn, tag)
            _check_record(oracle, S.engine.stats_from_bytes(got[f"{i}:{n}:stats_raw"].tobytes()), want["final"][:n], tag, G.hist_range(c))

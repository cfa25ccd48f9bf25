"""Every instantiation of stationary_kernel on the device against the numpy restatement over the CPU oracle: the six rows
of the ledger (tests/stationary_matrix.py: ROWS), the WILD inputs that tell the fast divide from the IEEE one, the WINDOW
cases that leave SMMC_DIV_CHECKED's window at the kernel's tests and in the remainder, the EDGES, and the checks the
older families have: shards, identical calls, raw against _to_host on an engine with a stream of its own.

Before a run is trusted the host's choice is asked for (stationary_divide_kind) and must be the kind the case claims.
Compared as in tests/test_stationary_gpu.py: final values, chunk means and variances (against
stationary_reference.chunk_mean_var_device_order), minimum and maximum on their bits; counters and every bucket exactly;
the record's two binary64 sums to the relative 1e-12 where both are finite.  What that file's _check cannot say is said
here: a float that is NaN on one side must be NaN on the other (payloads are no part of any contract, as in
tests/test_feature_matrix_gpu.py), and sums that are not finite must both be NaN or the same infinity.

Evidence that these tests bite.  Four builds of the library, each wrong on purpose in stationary_kernel (built by
tools/variant_build.py from a patched scratch copy of csrc/, never the product sources; loaded through SMMC_LIB), each
run once on the device with this file (40 tests) and tests/test_stationary_gpu.py (66 tests):
- simulate_stationary_path<kDivExact, false> compiled with the fast divide: 5 failed here (the two wild-2049 cases, the
  three mirror-2049 window cases, whose redo it is); tests/test_stationary_gpu.py passed.
- the window test removed for the four-draw layout: 3 failed here (the mirror-2049 window cases; the redo-2049 cases pass,
  as they must: their leavers leave at the top, where the divides agree); tests/test_stationary_gpu.py passed.
- the second candidate block drawn only for n > 5: 10 failed here (the three four-draw rows, wild-2049 at 13 periods,
  three of the largest-layout cases, the id wrap on 2049 entries, both subset cases); 3 of tests/test_stationary_gpu.py
  failed (2500-5, 2500-13, one fuzz case).
- stationary_index wrapping at next > T: 31 failed here, 46 there.
On the device the two files take 35 s together; of this one's tests the first takes 2.3 s (the library's load), every
other under 0.8 s."""
import math

import numpy as np
import pytest

import stationary_matrix as M
import stationary_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    """One engine per table, made on first use."""
    import stock_market_monte_carlo_amd as S
    made = {}

    def get(key):
        if key not in made:
            made[key] = S.Engine(0)
            made[key].set_table(M.table_of(key))
        return made[key]
    yield get
    for e in made.values():
        e.close()


def _sim(c, n=None, first=None, n_bins=None):
    import stock_market_monte_carlo_amd as S
    bins, lo, hi, below = c["hist"]
    return S.Engine.make_sim(c["n"] if n is None else n, c["P"], S.MODE_TABLE, c["seed"], first_path=c["first"] if first is None else first,
                             initial_capital=c["capital"], n_bins=bins if n_bins is None else n_bins, hist_lo=lo, hist_hi=hi,
                             below_threshold=below, exact_div=c["flag"])


def _host(raw):
    out = {k: (None if t is None else t.cpu().numpy()) for k, t in raw.items()}
    if out["stats_raw"] is not None:
        out["stats_raw"] = out["stats_raw"].tobytes()
    return out


def _run(eng, sim, q, final=True, chunks=True, stats=True):
    import stock_market_monte_carlo_amd as S
    raw = S.simulate_stationary_raw(eng, sim, renew_q16=q, want_final=final, want_chunk_stats=chunks, want_stats=stats)
    eng.sync()
    return _host(raw)


def _kind(eng, c):
    import stock_market_monte_carlo_amd as S
    got = S.stationary_divide_kind(eng, _sim(c), renew_q16=c["q"])
    assert got == c["kind"], f"{c['id']}: the host chose divide kind {got}, the case claims {c['kind']}"


def _same_floats(got, want, tag):
    """Bits, and NaN where the restatement has NaN."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, tag
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), tag
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), tag


def _same_sum(got, want, tag):
    if math.isfinite(got) and math.isfinite(want):
        assert got == pytest.approx(want, rel=1e-12), tag
    else:
        assert (math.isnan(got) and math.isnan(want)) or got == want, (tag, got, want)


def _check(got, want, n, tag):
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    with np.errstate(all="ignore"):
        if got["final"] is not None:
            assert got["final"].size == n
            _same_floats(got["final"], want["final"], tag)
        if got["stats_raw"] is not None:
            st, ost = stats_from_bytes(got["stats_raw"]), want["stats"]
            assert st.count == ost.count == n, tag
            assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), tag
            assert st.hist.size == want["hist"].size and np.array_equal(st.hist, want["hist"]), tag
            assert st.hist.size == 0 or int(st.hist.sum()) + st.underflow + st.overflow == n, tag
            _same_floats([st.min, st.max], [ost.min, ost.max], tag)
            _same_sum(st.sum, ost.sum, tag)
            _same_sum(st.sumsq, ost.sumsq, tag)
        if got["chunk_mean"] is not None:
            assert got["chunk_mean"].size == got["chunk_var"].size == -(-n // 256), tag
            cm, cv = ref.chunk_mean_var_device_order(want["final"])
            _same_floats(got["chunk_mean"], cm, tag)
            _same_floats(got["chunk_var"], cv, tag)
            if np.isfinite(cv).all() and np.isfinite(want["chunk_var"]).all():  # the one-pass restatement held to the oracle's two passes
                assert np.allclose(cm, want["chunk_mean"], rtol=1e-6, atol=0.0), tag
                assert np.allclose(cv, want["chunk_var"], rtol=1e-5, atol=1e-6 * float(np.max(want["chunk_var"]) + 1)), tag


def _same_bytes(a, b, tag, keys=("final", "chunk_mean", "chunk_var", "stats_raw")):
    """Two device results: every output asked for, every byte."""
    for k in keys:
        x, y = a[k], b[k]
        assert x is not None and y is not None, (tag, k)
        assert (x if isinstance(x, bytes) else x.tobytes()) == (y if isinstance(y, bytes) else y.tobytes()), (tag, k)


def _case_on_the_device(engines, oracle, c):
    eng = engines(c["table"])
    _kind(eng, c)
    _check(_run(eng, _sim(c), c["q"]), M.reference(oracle, c), c["n"], c["id"])


# ---- the ledger ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", M.ROWS, ids=[r["id"] for r in M.ROWS])
def test_every_instantiation(engines, oracle, row):
    """The row's request at q = 1/12 and 1/2 and 9, 13 and 16 periods, ids from 2^32 - 100."""
    for c in M.row_cases(row):
        _case_on_the_device(engines, oracle, c)


# ---- the divides -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", M.WILD, ids=[c["id"] for c in M.WILD])
def test_inputs_that_tell_the_divides_apart(engines, oracle, c):
    """EXACT without the flag; paths that end at 0, at inf and at NaN, and hundreds whose products the fast divide gets
    wrong (tests/test_stationary_matrix_cpu.py asserts that on the restatement)."""
    _case_on_the_device(engines, oracle, c)


@pytest.mark.parametrize("c", M.WINDOW, ids=[c["id"] for c in M.WINDOW])
def test_the_checked_window_and_its_remainder(engines, oracle, c):
    """CHECKED, and EXACT by the flag: the restatement's bits either way."""
    _case_on_the_device(engines, oracle, c)
    _case_on_the_device(engines, oracle, M.with_flag(c))


# ---- edges -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", M.EDGES, ids=[c["id"] for c in M.EDGES])
def test_edges(engines, oracle, c):
    """16384 entries with 4096 buckets; runs that wrap to entry 0; ids that wrap at 2^64."""
    eng = engines(c["table"])
    _check(_run(eng, _sim(c), c["q"]), M.reference(oracle, c), c["n"], c["id"])


@pytest.mark.parametrize("c", [M.row_cases(M.ROWS[3])[1], M.LARGEST[2]], ids=["four-draw", "largest"])
def test_every_subset_of_the_outputs(engines, oracle, c):
    """Each output alone, and the record without buckets: the bytes of the call that asks for everything."""
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    eng, q, n = engines(c["table"]), c["q"], c["n"]
    full = _run(eng, _sim(c), q)
    _check(full, M.reference(oracle, c), n, c["id"])
    for name, want, keys in (("final", dict(final=True, chunks=False, stats=False), ("final",)),
                             ("chunks", dict(final=False, chunks=True, stats=False), ("chunk_mean", "chunk_var")),
                             ("record", dict(final=False, chunks=False, stats=True), ("stats_raw",))):
        got = _run(eng, _sim(c), q, **want)
        assert {k for k, v in got.items() if v is not None} == set(keys), name
        _same_bytes(got, full, (c["id"], name), keys)
    bare = _run(eng, _sim(c, n_bins=0), q)  # n_bins = 0 together with statistics
    _check(bare, M.reference(oracle, c, n_bins=0), n, (c["id"], "no buckets"))
    _same_bytes(bare, full, (c["id"], "no buckets"), ("final", "chunk_mean", "chunk_var"))
    alone = _run(eng, _sim(c, n_bins=0), q, final=False, chunks=False)
    _same_bytes(alone, bare, (c["id"], "record alone, no buckets"), ("stats_raw",))
    a, b = stats_from_bytes(bare["stats_raw"]), stats_from_bytes(full["stats_raw"])
    assert (a.count, a.below, a.sum, a.sumsq, a.min, a.max) == (b.count, b.below, b.sum, b.sumsq, b.min, b.max)
    assert a.hist.size == 0 and (a.underflow, a.overflow) == (0, 0)


# ---- the siblings' checks --------------------------------------------------------------------------------------------

SHARDED = M._case("shards", "2049", 41, 5461, n=1000)


@pytest.mark.parametrize("cut", [1, 256, 300, 999])
def test_shards_of_one_request_merge(engines, oracle, cut):
    """A request of 1000 paths cut by first_path: the final values concatenate, the records merge by smmc_stats_merge to
    the whole's counters, buckets, minimum and maximum (tests/test_sweep_gpu.py's comparison)."""
    from stock_market_monte_carlo_amd.engine import merge_stats_bytes, stats_from_bytes
    c, eng = SHARDED, engines(SHARDED["table"])
    n, q = c["n"], c["q"]
    whole = _run(eng, _sim(c), q)
    _check(whole, M.reference(oracle, c), n, "whole")
    a = _run(eng, _sim(c, n=cut), q)
    b = _run(eng, _sim(c, n=n - cut, first=c["first"] + cut), q)
    assert np.concatenate([a["final"], b["final"]]).tobytes() == whole["final"].tobytes()
    m, w = stats_from_bytes(merge_stats_bytes([a["stats_raw"], b["stats_raw"]])), stats_from_bytes(whole["stats_raw"])
    assert (m.count, m.below, m.underflow, m.overflow, m.min, m.max) == (w.count, w.below, w.underflow, w.overflow, w.min, w.max)
    assert np.array_equal(m.hist, w.hist) and int(m.hist.sum()) + m.underflow + m.overflow == n
    assert m.sum == pytest.approx(w.sum, rel=1e-12) and m.sumsq == pytest.approx(w.sumsq, rel=1e-12)


@pytest.mark.parametrize("c", [M.WINDOW[11], M.LARGEST[2]], ids=["checked-four-draw", "largest"])
def test_identical_calls_give_identical_bytes(engines, c):
    """... double sums included, also with other users of the engine's accumulator in between: it is left zero."""
    eng, q = engines(c["table"]), c["q"]
    first = _run(eng, _sim(c), q)
    _same_bytes(first, _run(eng, _sim(c), q), "again")
    plain = M._case("plain", c["table"], 41, q, n=1000)
    eng.simulate(_sim(plain), want_stats=True)  # buckets: another user of the engine's bucket accumulator
    eng.simulate_blocks(_sim(plain), 3, want_stats=True)
    r = eng.simulate(_sim(plain), want_final=True)
    eng.order_statistics(r.final, [0, 500, 999])
    _same_bytes(first, _run(eng, _sim(c), q), "after other calls")


def test_raw_against_to_host_on_a_stream_of_its_own():
    """tests/raw_to_host_check.py's engine (Engine(stream="new")) and request: the raw entry's device tensors, read through
    torch's stream without waiting for the engine, against simulate_stationary_to_host -- every output, byte for byte."""
    import raw_to_host_check as R
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    eng = R._engine(S, "table", M.table_of("2049"))
    try:
        sim = R._sim(S, "table")
        raw = S.simulate_stationary_raw(eng, sim, renew_q16=5461, want_final=True, want_chunk_stats=True, want_stats=True)
        device = {k: v.cpu().numpy() for k, v in raw.items()}  # no engine sync
        final, stats, (means, variances) = S.simulate_stationary_to_host(eng, sim, renew_q16=5461, want_stats=True, want_chunk_stats=True)
    finally:
        eng.close()
    assert device["final"].tobytes() == final.tobytes() and final.any() and final.size == R.N_PATHS
    assert device["chunk_mean"].tobytes() == means.tobytes() and device["chunk_var"].tobytes() == variances.tobytes() and means.size == 2
    got = stats_from_bytes(device["stats_raw"].tobytes())
    for name in ("count", "below", "underflow", "overflow", "sum", "sumsq", "min", "max"):
        assert getattr(got, name) == getattr(stats, name), name
    assert got.count == R.N_PATHS and np.array_equal(got.hist, stats.hist) and got.hist.size == R.N_BINS

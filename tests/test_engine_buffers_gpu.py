"""The engine's grow-on-demand device buffers, each driven up, down and up again on ONE engine, every result against
the CPU oracle: the reference stream's final values, redo list and generator states (statistics only, no final
pointer), the checkpoint partials, the three staging buffers of the host pipeline (chunk shrunk to 1024 paths), with
order statistics in between (its own zeroed histogram).  A buffer that is freed while a launch still reads it, kept
at a stale size, or handed out short shows here as a wrong record.

Compared exactly: final values (their bits), counts, buckets, extremes, order statistics.  The two double sums of a
record and the per-256-path means / variances are formed in another order than the oracle's and are compared as the
tests of those entries compare them (tests/test_checkpoints_gpu.py, tests/test_host_pipeline_gpu.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 0x0B0FFE45
P, N_BIG, BINS, LO, HI, BELOW = 24, 70000, 100, 0.0, 4000.0, 1050.0


@pytest.fixture(scope="module")
def refs(table, oracle):
    """The oracle's paths, once, at the largest size: path i does not depend on how many paths a request has."""
    ref_final, _ = oracle.ref_mc_simulations(N_BIG, P, 1000.0, table, SEED)
    o = oracle.counter_mc(oracle.make_params(oracle.MODE_TABLE, P, N_BIG, SEED, table=table), want_traj=True)
    return {"ref_final": ref_final, "final": o["final"], "traj": o["traj"]}


def _same_record(oracle, st, values, tag):
    ost, ohist = oracle.values_stats(values, BELOW, BINS, LO, HI)
    assert st.count == ost.count == values.size, tag
    assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), tag
    assert st.min == ost.min and st.max == ost.max, tag
    assert np.array_equal(st.hist, ohist) and int(st.hist.sum()) + st.underflow + st.overflow == st.count, tag
    assert st.sum == pytest.approx(ost.sum, rel=1e-12) and st.sumsq == pytest.approx(ost.sumsq, rel=1e-12), tag


def test_buffers_grow_shrink_and_grow_again_on_one_engine(table, oracle, refs, monkeypatch):
    import stock_market_monte_carlo_amd as S
    monkeypatch.setenv("SMMC_HOST_CHUNK_PATHS", "1024")  # read when the engine is created
    eng = S.Engine(0)
    eng.set_table(table)

    def ref_stream(n):  # d_ref_final, d_ref_redo, d_ref_ws: statistics formed from final values nobody asked for
        sim = S.Engine.make_sim(n, P, S.MODE_TABLE, SEED, n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW, stream="ref")
        r = eng.simulate(sim, want_final=False, want_stats=True)
        _same_record(oracle, eng.read_stats(r.stats_raw), refs["ref_final"][:n], ("ref", n))

    def checkpoints(n, periods):  # d_ck_partials: [checkpoint][workgroup]
        sim = S.Engine.make_sim(n, P, S.MODE_TABLE, SEED, n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW)
        stats, final = eng.simulate_checkpoints(sim, periods, want_final=True)
        assert len(stats) == len(periods)
        for st, p in zip(stats, periods):
            _same_record(oracle, st, np.ascontiguousarray(refs["traj"][:n, p]), ("checkpoints", n, p))
        assert np.array_equal(final.cpu().numpy().view(np.uint32), refs["final"][:n].view(np.uint32)), n
        return final

    def to_host(n):  # d_stage, d_stage_cs, d_stage_stats: a record per chunk of 1024 paths
        sim = S.Engine.make_sim(n, P, S.MODE_TABLE, SEED, n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW)
        host, st, (cm, cv) = eng.simulate_to_host(sim, want_stats=True, want_chunk_stats=True)
        assert np.array_equal(host.view(np.uint32), refs["final"][:n].view(np.uint32)), n
        _same_record(oracle, st, refs["final"][:n], ("to_host", n))
        ocm, ocv = oracle.chunk_mean_var(refs["final"][:n])  # 1024 is a multiple of 256: the chunks line up
        np.testing.assert_allclose(cm, ocm, rtol=1e-6)
        np.testing.assert_allclose(cv, ocv, rtol=1e-5, atol=1e-30)

    def order_statistics(final):  # the radix histogram: zero between calls, as the bucket accumulator
        n = final.numel()
        ranks = sorted({0, n // 4, n // 2, n - 1})
        got = eng.order_statistics(final, ranks)
        assert np.array_equal(got.view(np.uint32), oracle.order_statistics(final.cpu().numpy(), ranks).view(np.uint32)), n

    to_host(300)  # below the sizes asked for: the staging buffers of the next call GROW, not only come to be
    for n, periods, n_host in ((300, [P], 1000), (N_BIG, [1, 7, 12, 23, P], 9000), (300, [P // 2], 1000)):
        ref_stream(n)
        final = checkpoints(n, periods)
        order_statistics(final)
        to_host(n_host)
        order_statistics(final)
    eng.close()

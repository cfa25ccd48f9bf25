"""simulate_X_raw against simulate_X_to_host on an engine with a stream of its own (Engine(stream="new")): the path on
which the wrapper's _leave matters, since the device tensors are read through torch's stream without waiting for the
engine.  Every want on, 300 paths (more than one 256-path chunk and not a multiple of it), 8 periods; every output must
be byte-equal between the two entries.  check(family) is called by one test in each family's GPU test file."""
import numpy as np

import portfolio_reference as pref

N_PATHS, N_PERIODS, N_BINS = 300, 8, 16
W3 = pref.WEIGHTS[3]
FLOW = dict(amount=6.0, fraction=0.001, floor=0.01)


def _law(K):
    means, stds, corr = pref.gauss_setup(K)
    return dict(means=means, factor=pref.factor_of(stds, corr))


def _on(names):
    return {"want_" + n: True for n in names}


CF = ("final", "paid", "ruin_period", "stats", "depleted_at")
PFCF = ("final", "holdings", "paid", "ruin_period", "stats", "depleted_at")


def families():
    """family -> (stem of the entries, mode, arguments after sim, keyword arguments, names of the wants)"""
    from stock_market_monte_carlo_amd import _lib
    return {
        "cashflow": ("simulate_cashflow", "gauss", (), FLOW, CF),
        "cashflow_sweep": ("simulate_cashflow_sweep", "gauss", ([4.0, 6.0, 8.0],), dict(fractions=0.001, floors=0.01), CF),
        "excursions": ("simulate_excursions", "gauss", (990.0, 1030.0), dict(drawdown_threshold=0.05), _lib.EXCURSION_OUTPUTS),
        "portfolio": ("simulate_portfolio", "gauss", (W3,), dict(rebalance_every=3, **_law(3)), ("final", "holdings", "stats")),
        "portfolio_cashflow": ("simulate_portfolio_cashflow", "gauss", (W3,), dict(rebalance_every=3, **FLOW, **_law(3)), PFCF),
        "glide": ("simulate_glide", "gauss", (W3, [(4, (0.2, 0.3, 0.5))]), dict(rebalance_every=2, **FLOW, **_law(3)), PFCF),
        "portfolio_cashflow_blocks": ("simulate_portfolio_cashflow_blocks", "assets", (W3, 3), dict(rebalance_every=3, **FLOW), PFCF),
        "guardrails": ("simulate_guardrails", "gauss", (W3, 6.0), dict(review_every=2, upper=0.0061, lower=0.0059, floor=0.01,
                                                                        rebalance_every=3, **_law(3)), _lib.GUARDRAILS_OUTPUTS),
        "portfolio_cashflow_checkpoints": ("simulate_portfolio_cashflow_checkpoints", "gauss", (W3, [2, 5, 8]),
                                           dict(rebalance_every=3, **FLOW, **_law(3)), PFCF),
        "real_cashflow": ("simulate_real_cashflow", "gauss", (pref.WEIGHTS[2],), dict(rebalance_every=3, **FLOW, **_law(3)),
                          ("final", "final_real", "index", "holdings", "paid", "ruin_period", "stats", "depleted_at")),
        "allocation_sweep": ("simulate_allocation_sweep", "gauss", ([W3, (0.2, 0.3, 0.5)],),
                             dict(rebalance_every=[0, 3], amounts=[4.0, 6.0], fractions=0.001, floors=0.01, **_law(3)), PFCF),
    }


def _host_bytes(v):
    return v if isinstance(v, bytes) else np.ascontiguousarray(v).tobytes()


def _engine(S, mode, table):
    eng = S.Engine(0, stream="new")
    assert eng.own_stream
    if mode == "table":
        eng.set_table(table)
    elif mode == "assets":
        eng.set_asset_table(pref.asset_table(37, 3))
    return eng


def _sim(S, mode):
    return S.Engine.make_sim(N_PATHS, N_PERIODS, S.MODE_GAUSSIAN if mode == "gauss" else S.MODE_TABLE, 20240607, first_path=3,
                             n_bins=N_BINS, hist_lo=0.0, hist_hi=2500.0)


def check(family, table=None):
    import stock_market_monte_carlo_amd as S
    stem, mode, args, kwargs, wants = families()[family]
    eng = _engine(S, mode, table)
    try:
        sim = _sim(S, mode)
        raw = getattr(eng, stem + "_raw")(sim, *args, **kwargs, **_on(wants))
        # read through torch's current stream, which _leave has made wait for the engine's; no engine sync
        device = {k: (v.cpu().numpy().tobytes() if hasattr(v, "cpu") else v) for k, v in raw.items()}
        host = getattr(eng, stem + "_to_host")(sim, *args, **kwargs, **_on(wants))
    finally:
        eng.close()
    assert list(device) == list(host)
    for key, got in device.items():
        want = host[key]
        if isinstance(got, bytes):
            assert want is not None and len(got) > 0 and got == _host_bytes(want), (family, key)
        else:
            assert np.array_equal(got, want), (family, key)  # n_assets, periods
    assert all(device[k] is not None for k in device) and any(np.frombuffer(device["final"], dtype=np.float32))
    return device


def check_blocks(table):
    """simulate_blocks_raw against simulate_blocks_to_host, whose result is simulate_to_host's triple."""
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    eng = _engine(S, "table", table)
    try:
        sim = _sim(S, "table")
        raw = eng.simulate_blocks_raw(sim, 3, want_final=True, want_chunk_stats=True, want_stats=True)
        device = {k: v.cpu().numpy() for k, v in raw.items()}
        final, stats, (means, variances) = eng.simulate_blocks_to_host(sim, 3, want_stats=True, want_chunk_stats=True)
    finally:
        eng.close()
    assert device["final"].tobytes() == final.tobytes() and final.any() and final.size == N_PATHS
    assert device["chunk_mean"].tobytes() == means.tobytes() and device["chunk_var"].tobytes() == variances.tobytes() and means.size == 2
    got = stats_from_bytes(device["stats_raw"].tobytes())
    for name in ("count", "below", "underflow", "overflow", "sum", "sumsq", "min", "max"):
        assert getattr(got, name) == getattr(stats, name), name
    assert got.count == N_PATHS and np.array_equal(got.hist, stats.hist) and got.hist.size == N_BINS

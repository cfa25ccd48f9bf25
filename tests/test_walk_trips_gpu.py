"""Every kernel walks its work with a loop that outruns the grid; here each kernel other than paths_kernel is run at
sizes where a workgroup, a wave or a thread makes a second and a third trip, and compared with an independent
reference (the CPU oracle, tests/cashflow_reference.py, tests/excursions_reference.py, tests/blocks_reference.py).
tests/test_paths_epilogue_gpu.py and tests/test_paths_wide_groups_gpu.py do the same for paths_kernel.

Where the second trip starts (grid, block, cus = Engine.geometry(); grid = cus * SMMC_BLOCKS_PER_CU, 64 by default):

  checkpoints_kernel, cashflow_kernel   a wave takes 64 paths per trip, kW = 4 (table) or 8 (Gaussian) waves per
                                        workgroup, G = min(ceil(n / (64 kW)), grid) workgroups: above 64 kW G paths.
  excursions_kernel                     the same with G capped at grid // 2.
  blocks_kernel                         a workgroup takes 256 paths per trip, min(ceil(n / 256), grid) workgroups:
                                        above 256 grid paths.
  values_stats_kernel, radix_hist_kernel  a thread takes 8 values per trip (stream_float4), 1024 threads per workgroup,
                                        cus * SMMC_STATS_BLOCKS_PER_CU resp. cus * SMMC_RADIX_BLOCKS_PER_CU workgroups
                                        (4 per CU by default): above 8192 cus knob values.

With SMMC_BLOCKS_PER_CU=1 (read when an engine is made) and the two statistics knobs at 1 (read per call) these are
6.6e4 / 1.3e5 paths, 6.6e4 paths and 2.1e6 values on 256 CUs; every size below is computed from the geometry.

Compared on their bits: per-path outputs, integer counters, per-period counts, buckets, min and max.  The two double
sums are compared to the relative 1e-12 of tests/test_gpu_parity.py with an EXACT reference, so that the tolerance is
the kernel's alone (its tree over n values is bounded by about log2(n) units in the last place): math.fsum of the
reference's binary32 values and of their squares (a binary32 value squared is exact in binary64) up to 2^20 values,
above that numpy's pairwise binary64 sum, whose own bound of log2(n) 2^-53 relative to the sum of magnitudes is 3e-15
for the data sets here (none cancels: the signed mixture's sum is that of its positive half).  blocks_kernel goes
through tests/test_blocks_gpu.py's _check, which takes the oracle's running sum.

Left out, with the reason: the Gaussian runs have 38 periods, so their checkpoints are {1, 8, 9, 37, 38} where the
table runs have {1, 8, 9, 40, 41}.  A device with one compute unit would leave excursions a grid of 0 workgroups at
SMMC_BLOCKS_PER_CU=1; the tests assert grid // 2 >= 1.

What the sizes rest on: Engine.geometry() gives the engine's grid, which the tests assert; the grid of a launch is not
exposed.  That checkpoints and cash flows launch min(chunks, grid) workgroups and excursions grid // 2 is read from
host_wave_walk_grid (smmc_capi.cpp) and smmc_excursions.cpp; if those caps change, the sizes here must follow, and
nothing in this file would say so.  The evidence that the sizes reach the later trips is a build with the walk's
stride doubled (wave_chunks, blocks_body) or its loop cut to one trip (stream_float4): every test of the kernel's
group here fails on it, except the statistics tests at sweep + 1 values, which one trip covers.
"""
import contextlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import blocks_reference as bref
import cashflow_reference as cref
import excursions_reference as xref
import test_blocks_gpu as tb
import test_excursions_gpu as tx
import test_stats_gpu as ts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0123456789AB
FIRST = (1 << 32) - 100   # the id crosses 2^32 inside every launch
BINS, LO, HI, BELOW = 100, 600.0, 1800.0, 1000.0
MODES = ["gaussian", "table", "table2500"]
PERIODS = {"gaussian": 38, "table": 41, "table2500": 41}  # table: five Philox blocks of eight draws and one more period
CHECKPOINTS = {"gaussian": [1, 8, 9, 37, 38], "table": [1, 8, 9, 40, 41], "table2500": [1, 8, 9, 40, 41]}
# cash flows: (amount, fraction) per schedule and the floor; chosen on the restatement, which the tests assert on
FLOOR = 0.01
FLOWS = {"gaussian": {"amount": (29.0, 0.0), "both": (26.5, 0.005)},
         "table": {"amount": (27.0, 0.0), "both": (23.0, 0.005)},
         "table2500": {"amount": (27.0, 0.0), "both": (23.0, 0.005)}}
CF_BELOW, CF_LO, CF_HI = 40.0, 5.0, 150.0  # of the final values: depleted paths end at 0, most others below 200
LEVELS = (950.0, 1100.0)  # excursions: (lower, target)


def _table2500():
    """2500 entries: above the 2048 up to which a Philox block yields eight draws, so the four-draw form runs."""
    rng = np.random.default_rng(2500)
    return rng.normal(0.6, 4.0, 2500).clip(-25.0, 25.0).astype(np.float32)


def _mode_table(mode_name, table):
    import stock_market_monte_carlo_amd as S
    if mode_name == "gaussian":
        return S.MODE_GAUSSIAN, None
    return S.MODE_TABLE, (table if mode_name == "table" else _table2500())


@contextlib.contextmanager
def _one_block_per_cu(monkeypatch, tab=None):
    """An engine whose grid is one workgroup per compute unit (the knob is read when the engine is made)."""
    import stock_market_monte_carlo_amd as S
    monkeypatch.setenv("SMMC_BLOCKS_PER_CU", "1")
    e = S.Engine(0)
    try:
        if tab is not None:
            e.set_table(tab)
        grid, _, cus = e.geometry()
        assert grid == cus  # host_wave_walk_grid and enqueue_blocks cap their grids at this
        yield e, cus
    finally:
        e.close()


def _walk_sizes(G, mode_name):
    """n_paths at which, with G workgroups of kW waves: wave 0 of workgroup 0 makes a third trip on a 13-path chunk and
    every other wave two; exactly one wave makes a second trip; every wave makes two and the last chunk has one active
    lane; the last wave is one trip short."""
    W = G * (8 if mode_name == "gaussian" else 4)
    return [64 * (2 * W + 1) - 51, 64 * (W + 1), 64 * (2 * W - 1) + 1, 64 * (2 * W - 1)]


def _runs(G, mode_name):
    """(n_paths, exact_div) of a mode: the four sizes; the first again with the IEEE divide in table mode; the
    2500-entry table once."""
    sizes = _walk_sizes(G, mode_name)
    if mode_name == "table2500":
        return [(sizes[0], False)]
    return [(n, False) for n in sizes] + ([(sizes[0], True)] if mode_name == "table" else [])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _exact_sums(values):
    d = np.ascontiguousarray(values, dtype=np.float64)
    assert np.isfinite(d).all()
    if d.size <= (1 << 20):
        return math.fsum(d.tolist()), math.fsum((d * d).tolist())
    return float(d.sum()), float((d * d).sum())


def _check_record(oracle, st, values, below, n_bins, lo, hi, tag, sums=None, want=None):
    """A record against oracle.values_stats of the values; the double sums against _exact_sums.  sums, want: these two
    where the caller has them already."""
    ost, ohist = want if want is not None else oracle.values_stats(values, below, n_bins, lo, hi)
    n = int(np.asarray(values).size)
    assert st.count == ost.count == n, tag
    assert (st.below, st.underflow, st.overflow) == (ost.below, ost.underflow, ost.overflow), tag
    assert st.min == ost.min and st.max == ost.max, tag
    assert len(st.hist) == n_bins and np.array_equal(st.hist, ohist), tag
    if n_bins:
        assert int(np.asarray(st.hist).sum()) + st.underflow + st.overflow == n, tag
    s1, s2 = sums if sums is not None else _exact_sums(values)
    assert st.sum == pytest.approx(s1, rel=1e-12) and st.sumsq == pytest.approx(s2, rel=1e-12), tag


def _share(hit, n):
    return int(hit[:n].sum()) / n


# ---- the wave walk: checkpoints_kernel, cashflow_kernel, excursions_kernel -------------------------------------------

@pytest.mark.parametrize("mode_name", MODES)
def test_checkpoint_records_when_waves_make_several_trips(oracle, table, monkeypatch, mode_name):
    """The records (lanes add across the trips, LDS buckets, the waves' partials) and the final values against the
    oracle's trajectory columns."""
    from stock_market_monte_carlo_amd import Engine
    mode, tab = _mode_table(mode_name, table)
    P, periods = PERIODS[mode_name], CHECKPOINTS[mode_name]
    with _one_block_per_cu(monkeypatch, tab) as (eng, cus):
        runs = _runs(cus, mode_name)
        n_max = runs[0][0]
        op = oracle.make_params(mode, P, n_max, SEED, first_path=FIRST, table=tab)
        traj = oracle.counter_mc(op, want_final=False, want_traj=True)["traj"]
        for n, exact in runs:
            sim = Engine.make_sim(n, P, mode, SEED, first_path=FIRST, n_bins=BINS, hist_lo=LO, hist_hi=HI, below_threshold=BELOW,
                                  exact_div=exact)
            stats, final = eng.simulate_checkpoints(sim, periods, want_final=True)
            assert len(stats) == len(periods)
            for st, p in zip(stats, periods):
                _check_record(oracle, st, traj[:n, p], BELOW, BINS, LO, HI, (mode_name, n, exact, p))
            assert np.array_equal(_bits(final.cpu().numpy()), _bits(traj[:n, P])), (mode_name, n, exact)


def _run_cashflow(eng, sim, amount, fraction):
    raw = eng.simulate_cashflow_raw(sim, amount, fraction, None, None, FLOOR, want_final=True, want_paid=True, want_ruin_period=True,
                                    want_stats=True, want_depleted_at=True)
    eng.sync()
    out = {k: t.cpu().numpy() for k, t in raw.items()}
    out["ruin_period"] = out["ruin_period"].view(np.uint32)
    out["depleted_at"] = out["depleted_at"].view(np.uint64)
    out["stats_raw"] = out["stats_raw"].tobytes()
    return out


@pytest.mark.parametrize("mode_name", MODES)
def test_cashflow_outputs_when_waves_make_several_trips(oracle, table, monkeypatch, mode_name):
    """final, paid, the depletion period, the record (per-lane accumulators that persist from chunk to chunk) and
    depleted_at (LDS counters) against the restatement."""
    from stock_market_monte_carlo_amd import Engine
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    mode, tab = _mode_table(mode_name, table)
    P = PERIODS[mode_name]
    with _one_block_per_cu(monkeypatch, tab) as (eng, cus):
        runs = _runs(cus, mode_name)
        n_max = runs[0][0]
        R = cref.returns(oracle, mode, tab, n_max, P, first_path=FIRST, seed=SEED)
        for sched in ("amount", "both"):
            amount, fraction = FLOWS[mode_name][sched]
            v, paid, ruin, _ = cref.simulate(R, amount, fraction, FLOOR)
            share = _share(ruin > 0, n_max)
            print(f"{mode_name} {sched}: the restatement depletes {share:.3f} of {n_max} paths")
            assert 0.05 < share < 0.95  # a degenerate input must not hide a kernel bug
            for n, exact in runs:
                tag = (mode_name, sched, n, exact)
                sim = Engine.make_sim(n, P, mode, SEED, first_path=FIRST, initial_capital=cref.CAPITAL, n_bins=BINS, hist_lo=CF_LO,
                                      hist_hi=CF_HI, below_threshold=CF_BELOW, exact_div=exact)
                out = _run_cashflow(eng, sim, amount, fraction)
                assert np.array_equal(_bits(out["final"]), _bits(v[:n])), tag
                assert np.array_equal(_bits(out["paid"]), _bits(paid[:n])), tag
                assert np.array_equal(out["ruin_period"], ruin[:n]), tag
                assert out["depleted_at"].size == P + 1, tag
                assert np.array_equal(out["depleted_at"], np.bincount(ruin[:n], minlength=P + 1).astype(np.uint64)), tag
                _check_record(oracle, stats_from_bytes(out["stats_raw"]), v[:n], CF_BELOW, BINS, CF_LO, CF_HI, tag)


@pytest.mark.parametrize("mode_name", MODES)
def test_excursion_outputs_when_waves_make_several_trips(oracle, table, monkeypatch, mode_name):
    """The eight per-path outputs, both records (the second one's partials lie behind the first's) and the two
    per-period counts against the restatement; the grid is half the engine's."""
    from stock_market_monte_carlo_amd.engine import stats_from_bytes
    mode, tab = _mode_table(mode_name, table)
    P = PERIODS[mode_name]
    with _one_block_per_cu(monkeypatch, tab) as (eng, cus):
        G = cus // 2  # smmc_excursions.cpp: g->half
        assert G >= 1
        runs = _runs(G, mode_name)
        n_max = runs[0][0]
        want = xref.excursions(xref.trajectories(oracle, mode, tab, n_max, P, first_path=FIRST, seed=SEED), *LEVELS)
        below, reach = _share(want["first_below"] > 0, n_max), _share(want["first_reach"] > 0, n_max)
        print(f"{mode_name}: the restatement has {below:.3f} ever below, {reach:.3f} reached, of {n_max} paths")
        assert 0.05 < below < 0.95 and 0.05 < reach < 0.95
        for n, exact in runs:
            tag = (mode_name, n, exact)
            out = tx._run(eng, tx._sim(mode_name, n, P, first=FIRST, exact_div=exact, n_bins=BINS), levels=LEVELS)
            for k in tx.PER_PATH:
                assert np.array_equal(_bits(out[k]), _bits(want[k][:n])), (tag, k)
            for k, per_path in zip(tx.COUNTS, ("first_below", "first_reach")):
                assert out[k].size == P + 1, (tag, k)
                assert np.array_equal(out[k], np.bincount(want[per_path][:n], minlength=P + 1).astype(np.uint64)), (tag, k)
            _check_record(oracle, stats_from_bytes(out["stats"]), want["final"][:n], tx.BELOW, BINS, tx.LO, tx.HI, (tag, "stats"))
            _check_record(oracle, stats_from_bytes(out["drawdown_stats"]), want["drawdown"][:n], xref.DD_THRESHOLD, BINS, 0.0, 1.0,
                          (tag, "drawdown_stats"))


# ---- blocks_kernel ---------------------------------------------------------------------------------------------------

def _blocks_sizes(vgrid):
    """Workgroup b walks the chunks b, b + vgrid, ...  With 3 vgrid + 2 chunks workgroups 0 and 1 make a fourth trip,
    workgroup 0 on a full chunk and workgroup 1 on the last one, of 7 paths; with 2 vgrid - 1 the last workgroup is one
    trip short; with 2 vgrid - 2 + 1 the last is, and the one before it ends on a chunk of one path."""
    return [256 * (3 * vgrid + 1) + 7, 256 * (2 * vgrid - 1), 256 * (2 * vgrid - 2) + 1]


_blocks_final = {}


def _blocks_check(oracle, eng, key, L, P, sizes, tag, exact_div=False):
    n_max = max(sizes)
    at = (key, L, P, n_max)
    if at not in _blocks_final:  # one entry: the two LDS layouts of the bundled table follow each other
        _blocks_final.clear()
        _blocks_final[at] = bref.finals_bulk(oracle, bref.table_of(key), bref.SEED, bref.FIRST_PATH, n_max, P, L)
    final = _blocks_final[at]
    for n in sizes:
        with np.errstate(all="ignore"):
            tb._check(tb._run(eng, tb._sim(n, P, exact_div=exact_div), L), bref.record_of(oracle, final[:n]), n, (tag, key, L, P, n))


@pytest.mark.parametrize("key,L,P,read", [("bundled", 12, 97, "b32"), ("bundled", 12, 97, "b128"), ("2049", 9, 28, None),
                                          ("7", 9, 41, None)])
def test_blocks_when_workgroups_walk_several_chunks(oracle, monkeypatch, key, L, P, read):
    """The chunk walk and its alternating scratch slots: final values, record and chunk statistics."""
    if read:
        monkeypatch.setenv("SMMC_BLOCKS_READ", read)
    with _one_block_per_cu(monkeypatch, bref.table_of(key)) as (eng, cus):
        _blocks_check(oracle, eng, key, L, P, _blocks_sizes(cus), read)


def test_blocks_checked_divide_when_workgroups_walk_several_chunks(oracle, monkeypatch):
    """The bundled months with the S&P 500's best and worst month put in: 360 periods cannot be proven safe for the fast
    divide, so the range-checked one runs, on every trip."""
    from stock_market_monte_carlo_amd import _lib
    with _one_block_per_cu(monkeypatch, bref.table_of("extremes")) as (eng, cus):
        n = _blocks_sizes(cus)[0]
        assert eng.blocks_divide_kind(tb._sim(n, 360), 12) == _lib.DIV_CHECKED
        _blocks_check(oracle, eng, "extremes", 12, 360, [n], "checked")


def test_blocks_many_chunks_per_workgroup_at_the_default_geometry(oracle):
    import stock_market_monte_carlo_amd as S
    eng = S.Engine(0)
    try:
        eng.set_table(bref.table_of("bundled"))
        grid, _, _ = eng.geometry()
        _blocks_check(oracle, eng, "bundled", 9, 9, [256 * (2 * grid + 3) + 63], "default geometry")
    finally:
        eng.close()


# ---- values_stats_kernel and radix_hist_kernel -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def eng():
    import stock_market_monte_carlo_amd as S
    e = S.Engine(0)
    yield e
    e.close()


def _stats_sizes(cus):
    """With one workgroup per CU a trip of the grid covers sweep values: a third trip for the first three workgroups
    and five values more; one value past the first trip (it goes to the tail path: the single-trip loop is exactly
    full, and a loop that ran on would read past the end); seven short of three whole trips."""
    sweep = cus * 1024 * 8
    return [2 * sweep + 8 * 1024 * 3 + 5, sweep + 1, 3 * sweep - 7]


# (below_threshold, hist_lo, hist_hi) per data set: some values under, some over
RANGES = {"lognormal": (5000.0, 1000.0, 20000.0), "mixture": (0.0, -6.0, 55000.0), "twins": (2.0, 1.6, 5.0)}


def _data(kind, size):
    rng = np.random.default_rng(size)
    if kind == "lognormal":  # final-value-like
        return np.exp(rng.normal(8.5, 0.7, size)).astype(np.float32)
    if kind == "mixture":    # signed: half around -5, half around 5e4
        return np.where(rng.random(size) < 0.5, rng.normal(-5.0, 1.0, size), rng.normal(5.0e4, 3.0e3, size)).astype(np.float32)
    assert kind == "twins"   # two clusters an octave apart with equal middle key bits, tiled
    return np.resize(ts._octave_twins(), size)


def _ranks(kind, host):
    """Eight ranks in an order whose first k are worth asking for alone: the median, a quartile, both ends, the other
    quartile, a repeat, two neighbours; for the twins the two ranks at the seam between the clusters come first."""
    n = host.size
    if kind == "twins":
        seam = int((host < np.float32(3.0)).sum())
        assert 0 < seam < n
        return [seam - 1, seam, 0, n - 1, n // 4, n // 2, n // 4 + n // 2, n // 2]
    return [n // 2, n // 4, 0, n - 1, n // 4 + n // 2, n // 2, n // 4 - 1, n // 4 + n // 2 + 1]


def _n_ranks(which, off):
    """How many of them a view asks for: 8, 1, 2 and 5 over the offsets of a size, shifted from size to size (the
    LDS layout of passes 1 and 2 depends on it)."""
    return (8, 1, 2, 5)[(which + off) % 4]


def _quartiles_of(ranks, ranked, n):
    """oracle.quartiles out of the oracle's values at _ranks(), which hold its five ranks: one sort per view."""
    return ranked[[ranks.index(r) for r in (0, n // 4, n // 2, n // 4 + n // 2, n - 1)]]


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("kind", ["lognormal", "mixture", "twins"])
def test_values_stats_when_threads_make_several_trips(eng, oracle, monkeypatch, kind, which):
    """One workgroup per CU; 100, 1 and 4096 buckets, each with the default, 1 and 64 LDS copies; views at float
    offsets 0 .. 3 (head and tail paths); a bucket-less call and a quartiles call in between, so that whatever a call
    leaves in the engine's accumulators shows in the next."""
    import torch
    monkeypatch.setenv("SMMC_STATS_BLOCKS_PER_CU", "1")
    monkeypatch.setenv("SMMC_RADIX_BLOCKS_PER_CU", "1")
    _, _, cus = eng.geometry()
    n = _stats_sizes(cus)[which]
    base = _data(kind, n + 3)
    dev = torch.from_numpy(base).to(eng.tdevice)
    below, lo, hi = RANGES[kind]
    for off in (0, 1, 2, 3):
        host, view = base[off:off + n], dev[off:off + n]
        sums = _exact_sums(host)
        for bins in (100, 1, 4096):
            want = oracle.values_stats(host, below, bins, lo, hi)
            assert 0 < want[0].underflow and 0 < want[0].overflow and want[0].underflow + want[0].overflow < n
            for copies in (None, "1", "64"):
                if copies is None:
                    monkeypatch.delenv("SMMC_STATS_HIST_COPIES", raising=False)
                else:
                    monkeypatch.setenv("SMMC_STATS_HIST_COPIES", copies)
                st = eng.read_stats(eng.values_stats(view, below_threshold=below, n_bins=bins, hist_lo=lo, hist_hi=hi))
                _check_record(oracle, st, host, below, bins, lo, hi, (kind, n, off, bins, copies), sums, want)
        st = eng.read_stats(eng.values_stats(view, below_threshold=below))
        ost = want[0]  # without buckets: the same counters, extremes and sums, nothing under or over
        assert (st.count, st.below, st.min, st.max, st.underflow, st.overflow) == (n, ost.below, ost.min, ost.max, 0, 0), (kind, n, off)
        assert len(st.hist) == 0 and st.sum == pytest.approx(sums[0], rel=1e-12) and st.sumsq == pytest.approx(sums[1], rel=1e-12)
        q = eng.quartiles(view)
        assert q[0] == ost.min and q[4] == ost.max, (kind, n, off)


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("kind", ["lognormal", "mixture"])
def test_order_statistics_when_threads_make_several_trips(eng, oracle, monkeypatch, kind, which, off):
    """Every pass of the radix select streams the values again: the oracle's sort, bit for bit, at every size and
    offset, for 1 to 8 ranks; quartiles too."""
    import torch
    monkeypatch.setenv("SMMC_RADIX_BLOCKS_PER_CU", "1")
    _, _, cus = eng.geometry()
    n = _stats_sizes(cus)[which]
    base = _data(kind, n + 3)
    host, view = base[off:off + n], torch.from_numpy(base).to(eng.tdevice)[off:off + n]
    ranks, k = _ranks(kind, host), _n_ranks(which, off)
    want = oracle.order_statistics(host, ranks)
    assert np.array_equal(_bits(eng.order_statistics(view, ranks[:k])), _bits(want[:k])), (kind, n, off, k)
    assert np.array_equal(_bits(eng.quartiles(view)), _bits(_quartiles_of(ranks, want, n))), (kind, n, off)


_twins_wanted = {}


def _twins_views(oracle, cus, which):
    """[(n, offset, ranks asked for, the oracle's values as bits, its quartiles as bits)] of the tiled octave twins at
    one size and the four offsets: sorted once, for both children."""
    if (cus, which) not in _twins_wanted:
        n = _stats_sizes(cus)[which]
        base = _data("twins", n + 3)
        views = []
        for off in (0, 1, 2, 3):
            host = base[off:off + n]
            ranks, k = _ranks("twins", host), _n_ranks(which, off)
            want = oracle.order_statistics(host, ranks)
            views.append((n, off, ranks[:k], _bits(want[:k]).tolist(), _bits(_quartiles_of(ranks, want, n)).tolist()))
        _twins_wanted[(cus, which)] = views
    return _twins_wanted[(cus, which)]


def _twins_child(views):
    """Run in a child process (SMMC_RADIX_MATCH is read once per process)."""
    import torch
    import stock_market_monte_carlo_amd as S
    e = S.Engine(0)
    bad = []
    dev = torch.from_numpy(_data("twins", views[0][0] + 3)).to(e.tdevice)
    for n, off, ranks, want, want_q in views:
        view = dev[off:off + n]
        if _bits(e.order_statistics(view, ranks)).tolist() != want:
            bad.append([n, off, "ranks"])
        if _bits(e.quartiles(view)).tolist() != want_q:
            bad.append([n, off, "quartiles"])
    e.close()
    print(json.dumps({"bad": bad, "cases": len(views)}))


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("match", ["table", "chain"])
def test_order_statistics_of_the_octave_twins_when_threads_make_several_trips(eng, oracle, match, which):
    """Passes 1 and 2 under both group-match forms, at every size and offset; the ranks begin with the two at the seam
    between the clusters."""
    _, _, cus = eng.geometry()
    views = _twins_views(oracle, cus, which)
    env = dict(os.environ)
    env.pop("SMMC_RADIX_MATCH", None)
    if match == "chain":
        env["SMMC_RADIX_MATCH"] = "chain"
    env["SMMC_RADIX_BLOCKS_PER_CU"] = "1"
    code = ("import json, os, sys; sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), 'tests')); "
            "import test_walk_trips_gpu as T; T._twins_child(json.loads(sys.argv[1]))")
    r = subprocess.run([sys.executable, "-c", code, json.dumps(views)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["bad"] == [] and out["cases"] == 4, out


def test_statistics_at_the_default_geometry(eng, oracle, monkeypatch):
    """No knob: four workgroups per CU, and two whole trips of that grid plus 4099 values."""
    import torch
    for knob in ("SMMC_STATS_BLOCKS_PER_CU", "SMMC_RADIX_BLOCKS_PER_CU", "SMMC_STATS_HIST_COPIES"):
        monkeypatch.delenv(knob, raising=False)
    _, _, cus = eng.geometry()
    n = 2 * (4 * cus * 1024 * 8) + 4099
    host = _data("lognormal", n)
    dev = torch.from_numpy(host).to(eng.tdevice)
    below, lo, hi = RANGES["lognormal"]
    st = eng.read_stats(eng.values_stats(dev, below_threshold=below, n_bins=BINS, hist_lo=lo, hist_hi=hi))
    _check_record(oracle, st, host, below, BINS, lo, hi, "default geometry")
    ordered = np.sort(host)
    ranks = _ranks("lognormal", host)
    assert np.array_equal(_bits(eng.order_statistics(dev, ranks)), _bits(ordered[ranks]))
    assert np.array_equal(_bits(eng.order_statistics(dev, ranks[:1])), _bits(ordered[ranks[:1]]))
    assert np.array_equal(_bits(eng.quartiles(dev)), _bits(ordered[[0, n // 4, n // 2, n // 4 + n // 2, n - 1]]))

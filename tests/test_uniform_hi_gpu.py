"""paths_hi_kernel against the CPU oracle and against paths_kernel, byte for byte.

launch_paths gives a launch whose paths share the id bits 63..32 the kernel that holds them in a scalar register
(Engine.paths_form == 1); SMMC_UNIFORM_HI=0 gives every launch the generic kernel.  Both must write the oracle's final
values and the same chunk means, chunk variances and statistics record.

Divide kinds with short paths.  The three kinds are chosen as tests/test_paths_epilogue_gpu.py chooses them -- by
parameters, confirmed through Engine.divide_kind -- but those need 360 or 1000 periods.  Here the initial capital
decides: the rule (smmc_capi.cpp, divide_kind) proves the fast divide from log2(capital) + periods x log2(largest
multiplier / 100) staying below 2^127, and from the mirrored bound at 2^-89, so a capital near either end fails the
proof; the range-checked kind then needs its window of 7 more periods to hold the capital with two bits to spare.
With g the log2 of the largest (or smallest) relative step, "fast not proven" and "window holds" together need about
(periods - 7) g > 2..4: NO capital yields the checked kind below 8 periods, whatever the draw.  For those lengths
the fast and the IEEE kernels run; from 8 periods on all three do, with a wide draw (Gaussian N(2, 13) percent; a
37-entry table from -90 % to +30 %) so that g is large enough, and the capital is found by asking the engine.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED0123456789AB
SIZES = [1, 37, 64, 65, 256, 256 * 4 + 1, 256 * 5 + 255]
PERIODS = [1, 3, 4, 5, 8, 9, 36]  # remainders of both 4-draw and 8-draw Philox blocks
HIST = dict(n_bins=64, hist_lo=0.0, hist_hi=4000.0)
WIDE_TABLE = np.linspace(-90.0, 30.0, 37).astype(np.float32)  # percent; dense (<= 2048 entries), odd length
WIDE_GAUSS = dict(gauss_mean=2.0, gauss_std=13.0)


def _firsts(n):
    return [0, 5, (1 << 32) - n, (1 << 32) - n + 1, 1 << 32, (1 << 40) + 12345]


@pytest.fixture(scope="module")
def eng():
    import stock_market_monte_carlo_amd as S
    e = S.Engine(0)
    e.set_table(WIDE_TABLE)
    yield e
    e.close()


def _mode(mode_name):
    from stock_market_monte_carlo_amd import MODE_GAUSSIAN, MODE_TABLE
    return {"table": MODE_TABLE, "gaussian": MODE_GAUSSIAN}[mode_name]


_capitals = {}


def _divides(eng, mode_name, periods):
    """[(kind, make_sim arguments)]: fast, range-checked (from 8 periods on) and IEEE divide, short paths."""
    from stock_market_monte_carlo_amd import Engine, _lib
    key = (mode_name, periods)
    if key not in _capitals:
        found = {}
        wide = {} if mode_name == "table" else WIDE_GAUSS
        for k in list(range(10, -80, -1)) + list(range(11, 120)):  # capital 2^k, nearest to 1000 first
            kw = dict(wide, initial_capital=float(2.0 ** k))
            kind = eng.divide_kind(Engine.make_sim(256, periods, _mode(mode_name), SEED, **kw))
            found.setdefault(kind, kw)
        assert _lib.DIV_FAST in found, key
        assert (_lib.DIV_CHECKED in found) == (periods >= 8), (key, sorted(found))  # the docstring's argument
        out = [(_lib.DIV_FAST, found[_lib.DIV_FAST])]
        if _lib.DIV_CHECKED in found:
            out.append((_lib.DIV_CHECKED, found[_lib.DIV_CHECKED]))
        out.append((_lib.DIV_EXACT, dict(found[_lib.DIV_FAST], exact_div=True)))
        _capitals[key] = out
    return _capitals[key]


def _oracle_final(mode_name, sim_kw, n, periods, first):
    from oracle import oracle as O
    kw = {k: v for k, v in sim_kw.items() if k != "exact_div"}
    omode = O.MODE_TABLE if mode_name == "table" else O.MODE_GAUSSIAN
    p = O.make_params(omode, periods, n, SEED, first_path=first, table=WIDE_TABLE if mode_name == "table" else None, **kw)
    return O.counter_mc(p, n_threads=1 if n * periods < (1 << 20) else 8)["final"]  # a thread pool costs 50 ms to start


def _run(eng, sim):
    r = eng.simulate(sim, want_final=True, want_chunk_stats=True, want_stats=True)
    return (r.final.cpu().numpy(), r.chunk_mean.cpu().numpy().tobytes(), r.chunk_var.cpu().numpy().tobytes(),
            r.stats_raw.cpu().numpy().tobytes())


def _check(eng, monkeypatch, mode_name, n, periods, first, kind, kw):
    from stock_market_monte_carlo_amd import Engine
    what = (mode_name, n, periods, first, kind)
    sim = Engine.make_sim(n, periods, _mode(mode_name), SEED, first_path=first, **HIST, **kw)
    assert eng.divide_kind(sim) == kind, what
    monkeypatch.setenv("SMMC_UNIFORM_HI", "1")
    crosses = (first >> 32) != ((first + n - 1) >> 32)
    assert eng.paths_form(sim) == (0 if crosses else 1), what
    hi = _run(eng, sim)
    monkeypatch.setenv("SMMC_UNIFORM_HI", "0")  # read per call
    assert eng.paths_form(sim) == 0, what
    generic = _run(eng, sim)
    want = _oracle_final(mode_name, kw, n, periods, first)
    assert np.array_equal(hi[0].view(np.uint32), want.view(np.uint32)), (what, np.flatnonzero(hi[0] != want)[:8])
    assert hi[0].tobytes() == generic[0].tobytes(), what
    assert hi[1] == generic[1] and hi[2] == generic[2], (what, "chunk statistics")
    assert hi[3] == generic[3], (what, "statistics record")


@pytest.mark.parametrize("mode_name", ["gaussian", "table"])
@pytest.mark.parametrize("n", SIZES)
def test_sibling_equals_oracle_and_generic_kernel(eng, monkeypatch, mode_name, n):
    for periods in PERIODS:
        for kind, kw in _divides(eng, mode_name, periods):
            for first in _firsts(n):
                _check(eng, monkeypatch, mode_name, n, periods, first, kind, kw)


def test_form_follows_the_range_and_the_knob(eng, monkeypatch):
    from stock_market_monte_carlo_amd import Engine, MODE_GAUSSIAN, MODE_TABLE
    monkeypatch.delenv("SMMC_UNIFORM_HI", raising=False)  # default: on
    for mode in (MODE_GAUSSIAN, MODE_TABLE):
        for n in SIZES:
            for first in _firsts(n):
                sim = Engine.make_sim(n, 9, mode, SEED, first_path=first)
                crosses = n > 1 and first == (1 << 32) - n + 1
                assert eng.paths_form(sim) == (0 if crosses else 1), (mode, n, first)
        assert eng.paths_form(Engine.make_sim(256, 9, mode, SEED, stream=2)) == 0  # stream v2 has no sibling
    monkeypatch.setenv("SMMC_UNIFORM_HI", "0")
    assert eng.paths_form(Engine.make_sim(256, 9, MODE_GAUSSIAN, SEED)) == 0
    monkeypatch.setenv("SMMC_UNIFORM_HI", "7")  # outside 0 .. 1: ignored
    assert eng.paths_form(Engine.make_sim(256, 9, MODE_GAUSSIAN, SEED)) == 1


@pytest.mark.parametrize("mode_name", ["gaussian", "table"])
def test_several_chunks_per_virtual_block(eng, monkeypatch, mode_name):
    from stock_market_monte_carlo_amd import _lib
    vgrid, _, _ = eng.geometry()
    kind, kw = _divides(eng, mode_name, 9)[0]
    assert kind == _lib.DIV_FAST
    _check(eng, monkeypatch, mode_name, 256 * (2 * vgrid + 3) + 63, 9, (1 << 40) + 12345, kind, kw)


def test_host_pipeline_decides_per_chunk(monkeypatch):
    """simulate_to_host in chunks of 256 paths, exactly one of which straddles 2^32: that chunk runs the generic
    kernel, the others the sibling, and the whole equals the oracle."""
    import stock_market_monte_carlo_amd as S
    from stock_market_monte_carlo_amd import Engine
    monkeypatch.setenv("SMMC_HOST_CHUNK_PATHS", "256")  # read when the engine is created
    monkeypatch.setenv("SMMC_UNIFORM_HI", "1")
    n, first = 256 * 4 + 37, (1 << 32) - 256 - 100
    straddling = [c for c in range(0, n, 256) if ((first + c) >> 32) != ((first + min(c + 256, n) - 1) >> 32)]
    assert straddling == [256]
    e = S.Engine(0)
    try:
        e.set_table(WIDE_TABLE)
        for mode_name in ("gaussian", "table"):
            sim = Engine.make_sim(n, 9, _mode(mode_name), SEED, first_path=first, **HIST)
            for c in range(0, n, 256):
                part = Engine.make_sim(min(256, n - c), 9, _mode(mode_name), SEED, first_path=first + c, **HIST)
                assert e.paths_form(part) == (0 if c == 256 else 1)
            got, stats, _ = e.simulate_to_host(sim, want_stats=True)
            want = _oracle_final(mode_name, {}, n, 9, first)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), mode_name
            assert stats.count == n
    finally:
        e.close()

"""The ledger of tests/feature_matrix.py against the kernels as they compile now, and the conditions its cases rest on,
asserted on the restatements alone (no GPU).

The kernels' assembly is compiled once (the isa_loop_count.emit_asm fixture of tests/test_measurement_cpu.py; after a
build it is a copy) and only the instantiations' NAMES are read (tools/isa_table.py: instantiations(), the listing rows()
starts from -- rows() itself analyses every kernel's loops, seconds per row, and nothing of that is needed here).  No
instruction is inspected."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import cashflow_reference as cref  # noqa: E402
import feature_matrix as M  # noqa: E402


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    import isa_loop_count as I
    return I.emit_asm(str(tmp_path_factory.mktemp("isa") / "smmc_kernels.s"))


def _compiled(asm, family):
    """The template-argument lists of a family's instantiations in the assembly."""
    import isa_table as T
    prefix, symbols = T.instantiations(asm, family)
    out = []
    for sym in symbols:
        m = re.match(r"(I(?:L[a-z]\d+E)+E)Ev", sym[len(prefix):])
        assert m, sym
        out.append(m.group(1))
    return out


def _ledger(family, rows=None):
    return [M.mangled(family, c["args"]) for c in M.rows_of(family, M.ROWS if rows is None else rows)]


def _difference(compiled, ledger):
    """(instantiations no row names, rows that name no instantiation)."""
    return sorted(set(compiled) - set(ledger)), sorted(set(ledger) - set(compiled))


@pytest.mark.parametrize("family", M.FAMILIES)
def test_the_ledger_names_exactly_the_compiled_instantiations(asm, family):
    compiled, ledger = _compiled(asm, family), _ledger(family)
    assert len(set(compiled)) == len(compiled) and len(set(ledger)) == len(ledger), "a name twice"
    missing, extra = _difference(compiled, ledger)
    assert not missing, f"{family}: compiled but in no row of tests/feature_matrix.py (add rows and cases): {missing}"
    assert not extra, f"{family}: rows that name nothing that is compiled: {extra}"
    # the check notices a row taken out and an instantiation added
    assert _difference(compiled, ledger[1:]) == ([ledger[0]], [])
    assert _difference(compiled + ["ILi7ELb0ELb0EE"], ledger) == (["ILi7ELb0ELb0EE"], [])


def test_the_counts_the_families_are_known_by():
    count = {f: len(M.rows_of(f, M.ROWS)) for f in M.FAMILIES}
    assert count == {"checkpoints_kernel": 6, "cashflow_kernel": 12, "cashflow_sweep_kernel": 18, "excursions_kernel": 6,
                     "blocks_kernel": 12, "portfolio_kernel": 24, "portfolio_cashflow_kernel": 48}
    assert len({c["id"] for c in M.CASES}) == len(M.CASES)


def test_a_rows_case_is_the_one_its_arguments_say():
    """What the host's ladders look at, restated: mode, table_is_dense (length <= 2048), the flag or an unprovable input,
    K, the schedule's form, sweep_width(S), the layout asked for."""
    for c in M.CASES:
        fam, a = c["family"], c["args"]
        dense = c["mode"] == "table" and c["T"] <= 2048
        if fam == "blocks_kernel":
            assert c["mode"] == "table" and a == (c["kind"], dense, c["read"] == "b128"), c["id"]
            assert c["P"] == 9 if (dense or c["kind"] == M.DIV_CHECKED) else c["P"] == 5, c["id"]
            continue
        assert a[0] == (M.MODE_GAUSSIAN if c["mode"] == "gauss" else M.MODE_TABLE) and a[2] == dense, c["id"]
        assert a[1] == (c["kind"] == M.DIV_EXACT) == (c["exact"] is not None), c["id"]
        assert c["P"] == (9 if dense else 5) and c["n"] == 64 * (8 if c["mode"] == "gauss" else 4) * 2 + 37, c["id"]
        if fam == "cashflow_kernel":
            assert a[3] == c["varying"], c["id"]
        if fam == "cashflow_sweep_kernel":
            assert a[3] == (2 if c["S"] <= 2 else 4 if c["S"] <= 4 else 8), c["id"]
        if fam in ("portfolio_kernel", "portfolio_cashflow_kernel"):
            assert a[3] == c["K"], c["id"]
        if fam == "portfolio_cashflow_kernel":
            assert a[4] == c["varying"], c["id"]
    for fam in M.FAMILIES:  # every family and mode has inputs that tell the divides apart
        modes = {c["mode"] for c in M.rows_of(fam, M.EXTREME)}
        assert modes == ({"table"} if fam == "blocks_kernel" else {"table", "gauss"}), fam


@pytest.mark.parametrize("mode_name,key,P,base", [("gauss", "none", 360, 6.0), ("table", "bundled", 360, 6.0), ("table", "big", 41, 30.0)])
def test_the_oracles_multipliers_are_the_old_route_on_the_old_inputs(oracle, mode_name, key, P, base):
    """cashflow_reference.simulate over 100.0f + returns (stated for multipliers in [50, 200]) and
    simulate_multipliers over the oracle's own multipliers: the same multipliers and the same outputs, bit for bit, on the
    default Gaussian, the bundled table and the 3001-entry table."""
    from conftest import load_table
    mode = oracle.MODE_GAUSSIAN if mode_name == "gauss" else oracle.MODE_TABLE
    table = {"none": None, "bundled": load_table(), "big": cref.big_table()}[key]
    n = 700
    R = cref.returns(oracle, mode, table, n, P)
    A = cref.multipliers(oracle, mode, table, n, P)
    assert A.dtype == np.float32 and np.array_equal((np.float32(100.0) + R).view(np.uint32), A.view(np.uint32))
    assert 50.0 <= A.min() and A.max() <= 200.0
    am = (base * 1.002 ** np.arange(P)).astype(np.float32)
    for kw in (dict(amount=base, floor=0.01), dict(amount=am, fraction=0.002, floor=0.01)):
        old, new = cref.simulate(R, **kw), cref.simulate_multipliers(A, **kw)
        assert (old[2] > 0).any() and np.unique(old[2]).size > 10  # paths are depleted, at many different periods
        for a, b in zip(old, new):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_outside_its_stated_domain_the_old_route_is_not_the_engines_arithmetic(oracle):
    """100.0f + (a - 100.0f) is not a for the multipliers of a wide law (-40 +- 20 %): why such inputs take the oracle's."""
    n = 700
    wide = cref.multipliers(oracle, oracle.MODE_GAUSSIAN, None, n, 8, gauss_mean=-40.0, gauss_std=20.0)
    p = oracle.make_params(oracle.MODE_GAUSSIAN, 8, n, cref.SEED, first_path=cref.FIRST_PATH, gauss_mean=-40.0, gauss_std=20.0)
    back = np.float32(100.0) + np.stack([oracle.counter_path_returns(p, cref.FIRST_PATH + i) for i in range(n)])
    assert (back.view(np.uint32) != wide.view(np.uint32)).any()


@pytest.mark.parametrize("c", M.EXTREME, ids=[c["id"] for c in M.EXTREME])
def test_extreme_inputs_tell_the_divides_apart(oracle, c):
    """Part of the paths, not all, form a product outside the fast divide's domain; for some the restated fast divide
    gives other bits than the IEEE quotient; some end at inf, NaN, 0 or a subnormal."""
    left, differs, ends = M.left_window(oracle, c), M.fast_divide_differs(oracle, c), M.ends_degenerate(oracle, c)
    print(f"{c['id']}: {left.mean():.3f} leave the window, {differs.mean():.3f} with a differing quotient, {ends.mean():.3f} end degenerate")
    assert 0 < left.mean() < 1
    assert differs.any() and not (differs & ~left).any()
    assert ends.any()


@pytest.mark.parametrize("family", M.FAMILIES)
def test_tame_rows_stay_where_the_divides_agree(oracle, family):
    """The flag on a tame table checks the rest of the kernel and proves nothing about the divide: no product of such a
    row leaves the domain."""
    for c in M.rows_of(family, M.ROWS):
        if c["exact"] == "flag" and c["K"] in (1, 3):
            assert not M.left_window(oracle, c).any() and not M.fast_divide_differs(oracle, c).any(), c["id"]


def test_cash_flow_rows_deplete_part_of_their_paths(oracle):
    """No cash-flow row is vacuous: its schedule, sized from the case's own capital and growth, depletes part of the paths
    -- except the per-period FAST rows of portfolio cash flows, whose schedule the host's rule confines to contributions."""
    for c in M.ROWS:
        if c["family"] not in ("cashflow_kernel", "cashflow_sweep_kernel", "portfolio_cashflow_kernel"):
            continue
        share = M.depleted_share(M.reference(oracle, c))
        if c["family"] == "portfolio_cashflow_kernel" and c["varying"] and c["kind"] == M.DIV_FAST:
            assert share == 0.0, c["id"]
        elif isinstance(share, list):
            assert any(0.0 < s < 1.0 for s in share) and len(set(share)) > 1, (c["id"], share)
        else:
            assert 0.05 < share < 0.95, (c["id"], share)


def test_excursion_rows_pass_their_levels_on_part_of_their_paths(oracle):
    for c in M.rows_of("excursions_kernel"):
        r = M.reference(oracle, c)
        below, reach = float((r["first_below"] > 0).mean()), float((r["first_reach"] > 0).mean())
        assert 0.0 < below < 1.0 and (c["extreme"] or 0.0 < reach < 1.0), (c["id"], below, reach)


def test_checked_block_rows_leave_the_hosts_window_on_part_of_their_paths(oracle):
    """Capital 2^100, best month +300 %: hi = 2^(127 - 1 - 7 * 2 - log2 400) (divide_kind, smmc_capi.cpp); a path above
    it at a block boundary is redone with the IEEE divide."""
    hi = 2.0 ** (127.0 - 1.0 - 14.0 - np.log2(400.0))
    for c in M.rows_of("blocks_kernel", M.ROWS):
        if c["kind"] != M.DIV_CHECKED:
            continue
        v = M.compound(M.path_multipliers(oracle, c), c["capital"])[0]
        assert np.isfinite(v).all()
        share = float((v[:, 8] > hi).mean())  # the boundary after the first eight periods (four-draw tables: after two blocks)
        assert 0.0 < share < 1.0, (c["id"], share)

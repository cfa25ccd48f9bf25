"""The ledger of tests/stationary_matrix.py against stationary_kernel as it compiles now, and the conditions its cases rest
on, asserted on the restatement alone (no GPU): a case that cannot do what it is there for fails here and never passes
silently on the device.

The kernels' assembly is compiled once (isa_loop_count.emit_asm; after a build it is a copy) and only the
instantiations' NAMES are read (tools/isa_table.py: instantiations()).  No instruction is inspected."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import stationary_matrix as M  # noqa: E402


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    import isa_loop_count as I
    return I.emit_asm(str(tmp_path_factory.mktemp("isa") / "smmc_kernels.s"))


def _compiled(asm):
    """The template-argument lists of stationary_kernel's instantiations in the assembly."""
    import isa_table as T
    prefix, symbols = T.instantiations(asm, "stationary_kernel")
    out = []
    for sym in symbols:
        m = re.match(r"(I(?:L[a-z]\d+E)+E)Ev", sym[len(prefix):])
        assert m, sym
        out.append(m.group(1))
    return out


def _difference(compiled, ledger):
    """(instantiations no row names, rows that name no instantiation)."""
    return sorted(set(compiled) - set(ledger)), sorted(set(ledger) - set(compiled))


def test_the_ledger_names_exactly_the_compiled_instantiations(asm):
    compiled, ledger = _compiled(asm), [M.mangled(r["args"]) for r in M.ROWS]
    assert len(set(compiled)) == len(compiled) == 6 and len(set(ledger)) == len(ledger) == 6, "a name twice, or not six"
    missing, extra = _difference(compiled, ledger)
    assert not missing, f"compiled but in no row of tests/stationary_matrix.py (add rows and cases): {missing}"
    assert not extra, f"rows that name nothing that is compiled: {extra}"
    # the check notices a row taken out and an instantiation added
    assert _difference(compiled, ledger[1:]) == ([ledger[0]], [])
    assert _difference(compiled + ["ILi7ELb0EE"], ledger) == (["ILi7ELb0EE"], [])


def test_a_rows_request_is_the_one_its_arguments_say():
    """What launch_stationary looks at, restated: the divide kind -- host_divide() restates divide_kind of
    csrc/smmc_capi.cpp -- and table_is_dense (length <= 2048); EXACT by the flag, CHECKED without it."""
    assert sorted(r["args"] for r in M.ROWS) == sorted((d, dense) for d in (0, 1, 2) for dense in (False, True))
    for r in M.ROWS:
        cases = M.row_cases(r)
        assert {(c["q"], c["P"]) for c in cases} == {(q, P) for q in (5461, 32768) for P in (9, 13, 16)}, r["id"]
        for c in cases:
            T = int(M.table_of(c["table"]).size)
            assert T in (2048, 2049) and r["args"] == (c["kind"], T <= 2048), c["id"]
            assert M.host_divide(c)[0] == c["kind"], c["id"]
            assert c["flag"] == (c["kind"] == M.DIV_EXACT), c["id"]
            assert c["n"] == 2 * 256 + 37 and c["first"] == 2 ** 32 - 100, c["id"]
    assert len({c["id"] for c in M.CASES}) == len(M.CASES)


def test_checked_rows_leave_the_window_on_part_of_their_paths(oracle):
    """Capital 2^100, every eighth month +300 %: at the test after period 8 part of the paths are above the window's upper
    end (redone with the IEEE divide) and part are not; at 9 and 13 periods some leave it only in the remainder."""
    for r in M.ROWS:
        for c in M.row_cases(r):
            if c["kind"] != M.DIV_CHECKED:
                continue
            at_test, after = M.window_leavers(oracle, c)
            print(f"{c['id']}: {at_test.mean():.3f} outside the window at a test, {int(after.sum())} only after the last period")
            assert 0.0 < at_test.mean() < 1.0, c["id"]
            assert np.isfinite(M.reference(oracle, c)["final"]).all(), c["id"]
            assert (c["P"] % 8 == 0) == (not after.any()), c["id"]


def test_tame_rows_stay_where_the_divides_agree(oracle):
    """The flag on a tame table checks the rest of the kernel and proves nothing about the divide."""
    for r in M.ROWS:
        for c in M.row_cases(r):
            if c["flag"]:
                assert not M.below_the_fast_domain(oracle, c).any() and not M.fast_divide_differs(oracle, c).any(), c["id"]


@pytest.mark.parametrize("c", M.WILD, ids=[c["id"] for c in M.WILD])
def test_wild_inputs_tell_the_divides_apart(oracle, c):
    """For at least 1 % of the paths, and at least 8, the restated fast divide of some product is not the IEEE quotient's
    bits; at least 1 %, and at least 8, never form such a product; one path at least ends at 0, one at inf, one at NaN.
    The host cannot prove the fast divide (a -100 % month: no lower bound on a multiplier): EXACT without the flag."""
    assert M.host_divide(c)[0] == M.DIV_EXACT and not c["flag"] and c["n"] <= 2048
    assert 1e-37 <= c["capital"] <= 1e-35 and int(M.table_of(c["table"]).size) in (2048, 2049) and c["P"] in (9, 13)
    differs, below = M.fast_divide_differs(oracle, c), M.below_the_fast_domain(oracle, c)
    final = M.reference(oracle, c)["final"]
    ends = [int((final == 0).sum()), int(np.isinf(final).sum()), int(np.isnan(final).sum())]
    print(f"{c['id']}: of {c['n']} paths {int(differs.sum())} ({differs.mean():.3f}) form a product with a differing quotient, "
          f"{int((~differs).sum())} never do; {ends[0]} end at 0, {ends[1]} at inf, {ends[2]} at NaN")
    need = max(8, -(-c["n"] // 100))
    assert differs.sum() >= need and (~differs).sum() >= need
    assert not (differs & ~below).any()  # the divides differ only outside the fast divide's stated domain
    assert min(ends) >= 1, ends


@pytest.mark.parametrize("table", ["redo", "redo-2049", "mirror", "mirror-2049"])
def test_the_checked_window_is_left_at_the_tests_and_in_the_remainder(oracle, table):
    """CHECKED by the host's rule; the share of paths outside the window at one of the kernel's tests is strictly between
    0 and 1 at every P; at P = 363 and 367 some path is inside it at every test and outside it after its last period; no
    path that is inside it at every test forms a product on which the divides differ (the margin of seven periods the host
    claims for the remainder); on the downward tables at least 8 of the paths that left at a test do form one."""
    cases = [c for c in M.WINDOW if c["table"] == table]
    assert [c["P"] for c in cases] == [360, 363, 367]
    for c in cases:
        assert M.host_divide(c)[0] == M.DIV_CHECKED and c["n"] == 2048 and c["q"] == 16384, c["id"]
        at_test, after = M.window_leavers(oracle, c)
        differs = M.fast_divide_differs(oracle, c)
        print(f"{c['id']}: {at_test.mean():.3f} of the paths outside the window at a test; {int(after.sum())} inside it at every test "
              f"and outside it after the last period; {int((differs & at_test).sum())} leavers with a differing quotient")
        assert 0.0 < at_test.mean() < 1.0, c["id"]
        assert not (differs & ~at_test).any(), c["id"]
        if c["P"] % 8:
            assert after.sum() >= 1, c["id"]
        else:
            assert not after.any(), c["id"]
        if table.startswith("mirror"):
            assert (differs & at_test).sum() >= 8, c["id"]
    T = int(M.table_of(table).size)
    assert T == (2049 if table.endswith("2049") else 8)
    assert np.array_equal(M.table_of(table), np.resize(M.table_of(table.split("-")[0]), T))  # the pattern, repeated


def test_runs_wrap_from_the_last_entry_to_the_first(oracle):
    """q = 0, one run per path: at least one path starts within P - 1 entries of the table's end and reads on at 0."""
    for c in M.INDEX_WRAP:
        T = int(M.table_of(c["table"]).size)
        wraps = M.first_candidates(oracle, c) + c["P"] > T
        idx = M.indices(oracle, c)
        print(f"{c['id']}: {int(wraps.sum())} of {c['n']} runs pass the table's end")
        assert c["q"] == 0 and wraps.sum() >= 1, c["id"]
        assert np.array_equal(wraps, (np.diff(idx, axis=1) < 0).any(axis=1)) and (idx[wraps].min(axis=1) == 0).all(), c["id"]
    assert sorted(int(M.table_of(c["table"]).size) for c in M.INDEX_WRAP) == [2049, 16384]


def test_path_ids_cross_two_to_the_32_and_wrap_at_two_to_the_64(oracle):
    """The ids of a ledger row pass 2^32 inside the first chunk, those of the id-wrap cases pass 2^64 inside the launch: the
    restatement's paths past the wrap are the paths 0, 1, .. of a request that starts at 0."""
    for c in M.ID_WRAP:
        assert c["first"] == 2 ** 64 - 300 and 300 < c["n"]
        whole = M.reference(oracle, c)["final"]
        low = M.reference(oracle, dict(c, first=0, n=c["n"] - 300))["final"]
        assert np.array_equal(whole[300:].view(np.uint32), low.view(np.uint32)), c["id"]
        assert not np.array_equal(whole[:249].view(np.uint32), low.view(np.uint32)), c["id"]
    assert M.CROSSING < 2 ** 32 < M.CROSSING + 256


def test_the_largest_layout():
    for c in M.LARGEST:
        assert int(M.table_of(c["table"]).size) == 16384 and c["hist"][0] == 4096 and c["P"] == 13
    assert [c["q"] for c in M.LARGEST] == [0, 1, 5461, 65535, 65536]
    hdr = open(os.path.join(ROOT, "include", "smmc.h")).read()
    assert re.search(r"#define SMMC_MAX_TABLE 16384\b", hdr) and re.search(r"#define SMMC_MAX_BINS 4096\b", hdr)

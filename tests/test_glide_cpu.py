"""The glide-path contract (include/smmc.h, smmc_engine_simulate_glide) without a GPU: the two identities that tie the numpy
restatement (tests/glide_reference.py) to restatements of calls that already exist, the helper glide_linear, the proof that
no case run on the device is vacuous, the divide rule against the restated fast divide, the C ABI, the argument checks,
the divide rule's decisions and the flattened change table of csrc/smmc_glide.cpp (tests/cpp/glide_args.cpp, a stand-alone
program under AddressSanitizer and UBSan) and the kernel's instantiations as compiled.

On the commit before this feature every test here fails: neither the module's subject nor the symbols exist."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import glide_matrix as GM
import glide_reference as G
import portfolio_cashflow_reference as pcref
import portfolio_reference as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
NAMES = ("smmc_engine_simulate_glide", "smmc_engine_simulate_glide_to_host", "smmc_engine_glide_divide_kind")
f32 = np.float32
M = G.M
IDS = [c["id"] for c in G.ALL_CASES]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _all_equal(got, want, tag):
    for key in G.KEYS:
        assert _same(got[key], want[key]), (tag, key)


# ---- the identities ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", G.CASES, ids=[c["id"] for c in G.CASES])
def test_identity_1_without_a_change_or_with_equal_rows_it_is_the_parent(oracle, c):
    a, w, sched = G.multipliers(oracle, c), G.weights(c), G.schedule(oracle, c)
    parent = G.parent(oracle, c)
    _all_equal(G.reference(oracle, c, glide=False), parent, (c["id"], "no change"))
    same = tuple((t, w) for t in range(1, c["P"] + 3))
    _all_equal(G.simulate(a, w, same, c["R"], capital=c["capital"], **sched), parent, (c["id"], "equal rows"))
    beyond = tuple((c["P"] + 1 + i, row) for i, (_, row) in enumerate(c["changes"]))
    _all_equal(G.simulate(a, w, beyond, c["R"], capital=c["capital"], **sched), parent, (c["id"], "beyond P"))
    assert not _same(G.reference(oracle, c)["final"], parent["final"])


@pytest.mark.parametrize("c", G.ALL_CASES, ids=IDS)
def test_identity_2_without_flows_and_rebalancing_nothing_trades(oracle, c):
    a, w = G.multipliers(oracle, c), G.weights(c)
    got = G.simulate(a, w, c["changes"], 0, capital=c["capital"])
    values, holdings = pref.simulate(a, w, 0, capital=c["capital"])
    assert _same(got["final"], values[:, -1].copy()) and _same(got["holdings"], holdings)
    assert not got["ruin_period"].any() and not got["paid"].any()
    # and with a rebalance the same changes do trade
    acts = any(t < c["P"] for t, _ in c["changes"])  # a change at P meets no rebalance
    assert not acts or not _same(G.simulate(a, w, c["changes"], 1, capital=c["capital"])["final"],
                                 G.simulate(a, w, (), 1, capital=c["capital"])["final"])


def test_a_change_acts_from_its_own_period_on_and_not_before(oracle):
    """W(t) is the row of the last change with after <= t: the first after - 1 periods are the parent's whatever follows,
    and the trade at the end of period `after` is the first at the new row."""
    c = G.BY_ID[[i for i in IDS if i.endswith("on_rebalance")][0]]
    a, w, sched = G.multipliers(oracle, c), G.weights(c), G.schedule(oracle, c)
    (after, row), = c["changes"]
    assert after % c["R"] == 0 and after < c["P"]
    # a plan that ends one period before the change is the parent's
    _all_equal(G.simulate(a[:, :after - 1], w, c["changes"], c["R"], capital=c["capital"], **sched),
               pcref.simulate(a[:, :after - 1], w, c["R"], capital=c["capital"], **sched), "before")
    # a plan that ends AT the change rebalances nothing (no rebalance at P) and settles its last flow at the new row
    at = G.simulate(a[:, :after], w, c["changes"], c["R"], capital=c["capital"], **sched)
    was = pcref.simulate(a[:, :after], w, c["R"], capital=c["capital"], **sched)
    assert _same(at["final"], was["final"]) and not _same(at["holdings"], was["holdings"])
    Wt = G.weights_at(w, c["changes"], c["P"])
    assert _same(Wt[after - 1], np.asarray(w, f32)) and _same(Wt[after], np.asarray(row, f32))


def test_a_change_at_the_last_period_moves_the_holdings_only(oracle):
    for c in (c for c in G.EDGES if c["edge"] == "at_last"):
        got, parent = G.reference(oracle, c), G.parent(oracle, c)
        for key in ("final", "paid", "ruin_period", "depleted_at"):
            assert _same(got[key], parent[key]), (c["id"], key)
        live = parent["ruin_period"] == 0
        assert (got["holdings"][:, live] != parent["holdings"][:, live]).any(axis=0).mean() > 0.9, c["id"]


# ---- glide_linear ----------------------------------------------------------------------------------------------------

def _row_passes(row, K):
    row = np.asarray(row, f32)
    return bool(np.isfinite(row).all() and (row >= 0).all() and abs(float(row.astype(np.float64).sum()) - 1.0) <= 1e-6 and row.size == K)


@pytest.mark.parametrize("w_from, w_to, first, last, every", [((0.9, 0.1), (0.4, 0.6), 120, 480, 12), ((0.9, 0.1), (0.4, 0.6), 0, 360, 1),
                                                                ((0.5, 0.3, 0.2), (0.1, 0.2, 0.7), 7, 100, 9),
                                                                ((0.4, 0.3, 0.2, 0.1), (0.1, 0.2, 0.3, 0.4), 1, 512, 1),
                                                                ((1 / 3, 1 / 3, 1 / 3), (0.0, 0.0, 1.0), 3, 4, 5)])
def test_glide_linear_rows_pass_the_weight_check_and_end_at_the_inputs(w_from, w_to, first, last, every):
    from stock_market_monte_carlo_amd import glide_linear
    a32, b32 = np.asarray(w_from, f32), np.asarray(w_to, f32)
    if not _row_passes(a32, a32.size):  # thirds as binary32 are off by less than 1e-6 already; keep the inputs legal
        a32[0] += f32(1.0 - float(a32.astype(np.float64).sum()))
    changes = glide_linear(a32, b32, first, last, every)
    after = [t for t, _ in changes]
    want = [t for t in range(first, last, every) if t >= 1] + [last]
    assert after == want and all(x < y for x, y in zip(after, after[1:])) and len(changes) <= 512
    assert all(row.dtype == f32 and _row_passes(row, a32.size) for _, row in changes)
    assert _same(changes[-1][1], b32) and (first == 0 or (changes[0][0] == first and _same(changes[0][1], a32)))
    for t, row in changes[1:-1]:  # on the straight line, to binary32 and the renormalisation
        line = (a32.astype(np.float64) * (last - t) + b32.astype(np.float64) * (t - first)) / (last - first)
        assert np.abs(row - line).max() < 1e-6
    with pytest.raises(ValueError):
        glide_linear(a32, b32, last, first, every)
    with pytest.raises(ValueError):
        glide_linear(a32, b32[:-1], first, last, every)


# ---- no case run on the device is vacuous --------------------------------------------------------------------------

@pytest.mark.parametrize("c", G.ALL_CASES, ids=IDS)
def test_every_case_depletes_part_of_its_paths_and_differs_from_the_run_without_changes(oracle, c):
    out, plain = G.reference(oracle, c), G.reference(oracle, c, glide=False)
    if not G.fast_varying(c):  # contributions only: what the rule proves for a per-period schedule (exempt, as in the parent's ledger)
        assert 0.1 <= G.depleted_share(out) <= 0.9, (c["id"], G.depleted_share(out))
    else:
        assert (np.asarray(G.schedule(oracle, c)["amounts"]) < 0).all() and not out["ruin_period"].any()
    if G.is_identity(c):
        _all_equal(out, plain, c["id"])
    elif c.get("edge") in ("at_last", "past_boundary"):  # a change at P: the last settlement only
        assert c["changes"][0][0] == c["P"] and _same(out["final"], plain["final"]) and not _same(out["holdings"], plain["holdings"])
    else:
        assert G.differing_share(out, plain) >= 0.5, (c["id"], G.differing_share(out, plain))
    assert int(out["depleted_at"].sum()) == c["n"]


def test_the_cases_are_the_36_instantiations_and_the_edges_at_the_feature_matrix_shapes():
    assert [c["glide"] for c in G.CASES] == GM.ROWS and len(GM.ROWS) == 36 == len(set(GM.ROWS))
    for c in G.ALL_CASES:
        dense = c["mode"] == "table" and c["T"] <= 2048
        assert c["P"] == (9 if dense else 5) and c["n"] == 64 * (8 if c["mode"] == "gauss" else 4) * 2 + 37 and c["R"] == 3
        assert c["glide"][0] == (1 if c["mode"] == "gauss" else 0) and c["glide"][2] == dense and c["glide"][3] == c["K"]
        assert (c["exact"] is None) == (c["kind"] == M.DIV_FAST) and c["glide"][1] == (c["kind"] == M.DIV_EXACT)
    assert G.FIRST_PATH == (1 << 32) - 100
    for c in G.CASES:  # one change off a rebalance period, one on it, both inside the plan
        after = [a for a, _ in c["changes"]]
        assert len(after) == 2 and after[0] % 3 and after[1] % 3 == 0 and after[1] < c["P"]
    by_edge = {}
    for c in G.EDGES:
        by_edge.setdefault(c["edge"], []).append(c)
    assert all(len(v) == 2 and {x["P"] for x in v} == {5, 9} for v in by_edge.values())
    for edge, want in (("after1", lambda P: [1]), ("boundary", lambda P: [P - 1]), ("past_boundary", lambda P: [P]), ("on_rebalance", lambda P: [3]),
                       ("off_rebalance", lambda P: [4]), ("before_last", lambda P: [P - 1]), ("at_last", lambda P: [P]),
                       ("beyond", lambda P: [P + 1, P + 7]), ("consecutive", lambda P: [2, 3]), ("zero_and_back", lambda P: [2, 4]),
                       ("most", lambda P: list(range(1, 513)))):
        for c in by_edge[edge]:
            assert [a for a, _ in c["changes"]] == want(c["P"]), c["id"]
    # the Philox-block boundary: 8 draws per block on the dense table, 4 elsewhere
    assert {c["P"]: c["changes"][0][0] for c in by_edge["boundary"]} == {9: 8, 5: 4}
    for c in by_edge["zero_and_back"]:
        first, second = c["changes"][0][1], c["changes"][1][1]
        assert min(first) == 0.0 and min(second) > 0.0 and min(G.weights(c)) > 0.0 and c["exact"] == "unprovable" and c["kind"] == M.DIV_EXACT
    every_row = [row for c in G.ALL_CASES for _, row in c["changes"]] + [G.weights(c) for c in G.ALL_CASES]
    assert all(_row_passes(row, len(row)) for row in every_row)


# ---- the divide rule against the restated fast divide --------------------------------------------------------------------

@pytest.mark.parametrize("c", [c for c in G.ALL_CASES if c["kind"] == M.DIV_FAST], ids=[c["id"] for c in G.ALL_CASES if c["kind"] == M.DIV_FAST])
def test_no_product_of_a_fast_row_leaves_the_proven_window(oracle, c):
    """What the host's rule claims for a FAST row, on the restatement: every product h_k * a_k is exactly 0 or has a
    magnitude inside [2^-89, 2^127) (feature_matrix.left_window's idea), and there the restated fast divide
    (feature_matrix.fast_div100) gives the IEEE quotient's bits."""
    x = G.products(oracle, c)
    mag = np.abs(x.astype(np.float64))
    assert np.isfinite(x).all() and ((x == 0) | ((mag >= 2.0 ** -89) & (mag < 2.0 ** 127))).all(), c["id"]
    assert (x != 0).mean() > 0.5
    with np.errstate(all="ignore"):
        q = x / f32(100.0)
    assert np.array_equal(q.view(np.uint32), M.fast_div100(x).view(np.uint32)), c["id"]


def test_the_products_restated_are_those_of_the_reference(oracle):
    """products() walks the same recurrence as simulate(): its last column divided is what the final holdings came from."""
    c = G.CASES[2]
    x, a = G.products(oracle, c), G.multipliers(oracle, c)
    n, P, K = a.shape
    short = G.simulate(a[:, :P - 1], G.weights(c), c["changes"], c["R"], capital=c["capital"], **{k: (v[:P - 1] if isinstance(v, np.ndarray) else v)
                                                                                               for k, v in G.schedule(oracle, c).items()})
    # (the run of P - 1 periods makes no rebalance at P - 1; compare where the long run makes none either)
    if (P - 1) % c["R"]:
        with np.errstate(all="ignore"):
            assert _same((short["holdings"].T * a[:, P - 1, :]).astype(f32), x.reshape(n, P, K)[:, P - 1, :])


# ---- the C ABI ------------------------------------------------------------------------------------------------------

def test_entry_points_are_declared_exported_and_bound():
    from stock_market_monte_carlo_amd import _lib, build
    import stock_market_monte_carlo_amd as S
    hdr = open(os.path.join(ROOT, "include", "smmc.h")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    build.build()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in bound, name
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
    assert _lib.ABI_VERSION == 4 and re.search(r"#define SMMC_ABI_VERSION 4\b", hdr)  # additive
    m = re.search(r"#define SMMC_MAX_GLIDE_CHANGES (\d+)", hdr)
    assert m and int(m.group(1)) == _lib.MAX_GLIDE_CHANGES == S.MAX_GLIDE_CHANGES == G.MAX_CHANGES == 512
    assert ctypes.sizeof(_lib.Glide) == 24
    assert "smmc_glide.cpp" in build.SOURCES  # part of the build digest
    for name in ("simulate_glide", "simulate_glide_raw", "simulate_glide_to_host", "glide_divide_kind", "make_glide"):
        assert hasattr(S.Engine, name), name
    gl, keep = S.Engine.make_glide([(3, (0.5, 0.5)), (9, [0.25, 0.25, 0.5])])
    assert gl.n_changes == 2 and [gl.after[i] for i in range(2)] == [3, 9] and [gl.weights[i] for i in range(8)] == [0.5, 0.5, 0, 0, 0.25, 0.25, 0.5, 0]
    none, _ = S.Engine.make_glide([])
    assert none.n_changes == 0 and not none.after and not none.weights and none.struct_size == 24
    for doc, word in (("README.md", "smmc_engine_simulate_glide"), ("INTEGRATION.md", "smmc_engine_simulate_glide"), ("DESIGN.md", "Glide paths: target weights that change along a plan"),
                      (os.path.join("tools", "README.md"), "bench_glide.py")):
        assert word in open(os.path.join(ROOT, doc)).read(), doc


def test_only_the_new_unit_refers_to_the_new_launch_symbol(tmp_path):
    """The units that lend their checks gain no undefined symbol of the new kernel; the new unit refers to its own launch,
    to the parent's entry points (one asset) and LDS need, and to no other launch."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    units = [u for u in sorted(os.listdir(CSRC)) if u.endswith(".cpp")]
    assert "smmc_glide.cpp" in units
    for unit in units:
        obj = str(tmp_path / (unit + ".o"))
        subprocess.check_call(["g++", "-O0", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                               "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-c", os.path.join(CSRC, unit), "-o", obj])
        undefined = subprocess.check_output(["nm", "-u", "-C", obj]).decode()
        if unit == "smmc_glide.cpp":
            for own in ("launch_glide", "portfolio_cashflow_lds_bytes", "smmc_engine_simulate_portfolio_cashflow", "cashflow_check_schedule",
                        "cashflow_stage_schedule", "portfolio_check", "portfolio_asset_bounds"):
                assert own in undefined, own
            for other in ("launch_portfolio_cashflow(", "launch_portfolio(", "launch_cashflow(", "launch_guardrails("):
                assert other not in undefined, other
        else:
            assert "glide" not in undefined, (unit, undefined)
    text = open(os.path.join(CSRC, "smmc_glide.cpp")).read()
    assert "orc_" not in text and "smmc_oracle" not in text and "_reference" not in text


@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/glide_args.cpp over the fake HIP runtime, a stand-alone executable under AddressSanitizer and UBSan:
    {case: tuple of ints}, "_text": {case: error text}."""
    exe = str(tmp_path_factory.mktemp("glide") / "glide_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_cashflow.cpp", "smmc_excursions.cpp", "smmc_blocks.cpp", "smmc_portfolio.cpp",
                                           "smmc_portfolio_cashflow.cpp", "smmc_glide.cpp", "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "cashflow_launch_stub.cpp",
                                                            "excursions_launch_stub.cpp", "blocks_launch_stub.cpp", "portfolio_launch_stub.cpp",
                                                            "portfolio_cashflow_launch_stub.cpp", "glide_launch_stub.cpp", "glide_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "glide_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    out, text, last = {}, {}, None
    for line in r.stdout.splitlines():
        if line.startswith("#") and last:
            text[last] = line[1:].strip()
            continue
        parts = line.split()
        if len(parts) >= 2 and all(re.fullmatch(r"-?\d+", x) for x in parts[1:]):
            out[parts[0]] = tuple(int(x) for x in parts[1:])
            last = parts[0]
    out["_text"] = text
    return out


# case -> a word its error text must hold
INVALID = {"engine_null": "engine", "sim_null": "sim", "sim_struct_size_wrong": "struct_size", "portfolio_null": "smmc_portfolio",
           "five_assets": "n_assets", "weight_negative": "weights[0]", "weights_do_not_sum_to_one": "sum",
           "table_mode_without_asset_table": "set_asset_table", "stream_ref": "REF", "stream_v2": "V2",
           "cashflow_null": "cf", "cashflow_struct_size_wrong": "smmc_cashflow.struct_size", "no_periods": "n_periods",
           "too_many_periods": "SMMC_MAX_CASHFLOW_PERIODS", "floor_negative": "floor", "amount_nan": "amount", "fraction_infinite": "fraction",
           "glide_null": "smmc_glide", "glide_struct_size_wrong": "smmc_glide.struct_size", "too_many_changes": "SMMC_MAX_GLIDE_CHANGES",
           "after_null": "after is NULL", "weights_null": "weights is NULL", "after_zero": "after[0] is 0",
           "after_repeated": "strictly increasing", "after_decreasing": "strictly increasing",
           "row_weight_negative": "row 1 of the glide path: weights[0]", "row_weight_nan": "row 2 of the glide path: weights[0]",
           "row_weight_infinite": "row 0 of the glide path: weights[1]", "row_weight_beyond_the_assets": "row 0 of the glide path: weights[2]",
           "row_does_not_sum_to_one": "row 1 of the glide path: the weights sum",
           "row_beyond_the_plan_does_not_sum_to_one": "row 2 of the glide path: the weights sum",
           "one_asset_row_not_one": "row 0 of the glide path"}
OUTPUTS = {"outputs_null": "smmc_portfolio_cashflow_outputs", "outputs_struct_size_wrong": "struct_size", "outputs_reserved_not_zero": "reserved",
           "paths_per_workgroup": "shard"}
DEVICE_ONLY = {"paid_misaligned": "4-byte", "depleted_at_misaligned": "8-byte"}
VALID = ["valid_table", "valid_gaussian", "valid_exact_div_flag", "valid_no_changes", "valid_most_changes", "valid_changes_beyond_the_plan",
         "valid_one_asset"]
VALID_SIMULATE = ["valid_largest_lds", "valid_no_outputs"]


@pytest.mark.parametrize("entry", ["device", "to_host", "divide_kind"])
@pytest.mark.parametrize("case", sorted(INVALID))
def test_argument_errors_are_invalid_with_a_text_and_without_a_launch(args_report, entry, case):
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0, (entry, case, rc)  # SMMC_ERR_INVALID
    assert INVALID[case] in args_report["_text"][f"{entry}:{case}"], args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", sorted(OUTPUTS))
def test_bad_outputs_and_sizes_are_refused(args_report, entry, case):
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0
    assert OUTPUTS[case] in args_report["_text"][f"{entry}:{case}"]


@pytest.mark.parametrize("case", sorted(DEVICE_ONLY))
def test_misaligned_device_pointers_are_refused(args_report, case):
    rc, text_len, launches = args_report[f"device:{case}"]
    assert rc == -1 and text_len > 0 and launches == 0
    assert DEVICE_ONLY[case] in args_report["_text"][f"device:{case}"]


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", VALID + VALID_SIMULATE)
def test_a_valid_request_passes_the_argument_checks_and_launches_once(args_report, entry, case):
    """The host-only build then stops at its missing kernel: SMMC_ERR_HIP, not SMMC_ERR_INVALID and not a result."""
    rc, text_len, launches = args_report[f"{entry}:{case}"]
    assert rc == -2 and text_len > 0 and launches == 1


@pytest.mark.parametrize("case", VALID)
def test_divide_kind_answers_a_valid_request_without_a_launch(args_report, case):
    rc, text_len, launches = args_report[f"divide_kind:{case}"]
    assert rc in (0, 1) and launches == 0
    if case == "valid_exact_div_flag":
        assert rc == 1
    if case == "valid_table":  # three months within +-2 %, positive rows, a constant amount, a positive floor: FAST
        assert rc == 0


@pytest.mark.parametrize("entry", ["device", "to_host"])
def test_no_paths_is_no_launch_and_no_error(args_report, entry):
    assert args_report[f"{entry}:valid_no_paths"] == (0, 0, 0)


def test_every_case_of_the_args_program_is_claimed(args_report):
    want = {f"{e}:{c}" for e in ("device", "to_host", "divide_kind") for c in list(INVALID) + VALID}
    want |= {f"{e}:{c}" for e in ("device", "to_host") for c in list(OUTPUTS) + VALID_SIMULATE + ["valid_no_paths"]}
    want |= {f"device:{c}" for c in DEVICE_ONLY}
    assert {k for k in args_report if k.startswith(("device:", "to_host:", "divide_kind:"))} == want


@pytest.mark.parametrize("what", ["rc", "portfolio", "schedule", "sim", "outputs", "table_changes_beyond_the_plan", "table_without_a_change",
                                  "table_change_at_1_and_at_the_last_period", "table_most_changes_short_plan", "table_most_changes",
                                  "varying_schedule", "nothing_asked", "one_asset_is_the_parents_launch"])
def test_the_launch_is_given_what_the_request_says(args_report, what):
    assert args_report["staged:" + what] == (1,)


# what: (smmc_engine_glide_divide_kind, the parent's answer for the same sim, pf and cf, the launch's exact_div)
DIVIDE = {"no_changes": (0, 0, 0), "positive_rows": (0, 0, 0), "flag": (1, 1, 1), "an_asset_to_zero_and_back": (1, 0, 1),
          "a_zero_beyond_the_plan": (1, 0, 1), "the_same_asset_unweighted_throughout": (0, 0, 0), "a_tiny_positive_weight": (1, 0, 1),
          "rebalanced_without_a_floor": (1, 1, 1), "a_fraction": (1, 1, 1), "contributions": (0, 0, 0)}


@pytest.mark.parametrize("what", sorted(DIVIDE))
def test_the_divide_rule_decides_as_the_header_states(args_report, what):
    assert args_report["divide:" + what] == DIVIDE[what]


def test_a_tiny_weight_makes_contributions_exact_too(args_report):
    """1000 * 1e-30 shrunk by the worst month over 360 periods is below 2^-89: the all-in bound takes the smallest weight of
    every row, not of pf->weights alone (the parent, which sees 60 / 40, says FAST)."""
    assert args_report["divide:contributions_with_a_tiny_weight"] == (1, 0, 1)


def test_a_failed_launch_leaves_the_accumulator_to_be_cleared(args_report):
    assert args_report["lease:after_failed_launch"] == (0, -2, 0, 1, 1)


def test_sizes_of_the_structures(args_report):
    assert args_report["sizes"] == (24, 32, 56)


# ---- the kernels as they compile now --------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    import isa_loop_count as I
    return I.emit_asm(str(tmp_path_factory.mktemp("isa") / "smmc_kernels.s"))


def test_the_ledger_names_the_36_instantiations_none_with_scratch(asm):
    """Names only (tools/isa_table.instantiations), and the private segment size the assembler reports."""
    import isa_table as T
    lines = open(asm).read().splitlines()
    prefix, symbols = T.instantiations(asm, GM.KERNEL)
    got = sorted(re.match(r"(I(?:L[a-z]\d+E)+E)Ev", s[len(prefix):]).group(1) for s in symbols)
    assert got == sorted(GM.mangled(r) for r in GM.ROWS) and len(got) == 36
    for sym in symbols:
        sizes = [int(m.group(1)) for l in lines for m in [re.match(r"\s*\.set " + re.escape(sym) + r"\.private_seg_size, (\d+)", l)] if m]
        assert sizes == [0], (sym, sizes)


def test_the_committed_listing_is_of_the_kernels_as_they_compile(asm):
    """profiles/glide/isa.txt names every instantiation with the fingerprint it has now."""
    import isa_loop_count as I
    import isa_table as T
    listing = open(os.path.join(ROOT, "profiles", "glide", "isa.txt")).read()
    prefix, symbols = T.instantiations(asm, GM.KERNEL)
    for sym in symbols:
        variant = sym[len(prefix):]
        assert f"{GM.KERNEL}{variant}:" in listing and f"fingerprint {I.fingerprint(asm, variant, GM.KERNEL)[:16]}" in listing, variant
        assert re.search(re.escape(f"{GM.KERNEL}{variant}:") + r".* private_segment 0 ", listing), variant

"""The contract of the feature entries' Python marshalling, without a GPU and without the shared library: what every
simulate_X, simulate_X_raw, simulate_X_to_host and X_divide_kind of stock_market_monte_carlo_amd/engine.py hands to the
C library and gives back is what the commit before the binding layer did (tests/golden/engine_binding_parent.json,
written there by tests/golden/make_engine_binding_golden.py, whose observe() this module runs on the working tree):
the trace of _enter, C calls, _leave and sync, every scalar and structure field, which pointer is null and which
buffer of the result it addresses, the key order, types, dtypes and shapes of the result, the refusals of bad inputs
before anything is allocated -- and the text of every public signature of Engine.  The golden keeps a refusal whole
and of every other observation its trace and a sha256 of the rest; where one differs the test prints what the working
tree does, and the generator's --full, run on the parent, writes what the parent did."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_engine_binding_golden as G  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "engine_binding_parent.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def seen():
    return G.observe()["cases"]


@pytest.fixture(scope="module")
def digests(seen):
    # through JSON, as the golden went: tuples become lists
    return {name: json.loads(json.dumps(G.digest(obs))) for name, obs in seen.items()}


def _families():
    return sorted({name.split("|")[0] for name, *_ in G.cases()})


def test_the_golden_holds_exactly_the_generators_cases(golden, seen):
    assert sorted(golden["cases"]) == sorted(seen)
    assert len(golden["cases"]) > 450


@pytest.mark.parametrize("family", _families())
def test_every_entry_marshals_as_on_the_parent(golden, seen, digests, family):
    names = [n for n in sorted(golden["cases"]) if n.split("|")[0] == family]
    assert names
    wrong = [n for n in names if digests.get(n) != golden["cases"][n]]
    for n in wrong[:3]:  # what the first of them do now
        print("%s\n  parent: %s\n  now:    %s" % (n, json.dumps(golden["cases"][n]), json.dumps(seen.get(n), sort_keys=True)))
    assert not wrong, wrong


def test_a_bad_input_is_refused_before_anything_is_allocated_or_called(golden):
    bad = {n: c for n, c in golden["cases"].items() if "raises" in c and "|bad:" in n}
    assert len(bad) > 80
    for n, c in bad.items():
        assert c["raises"] in ("ValueError", "TypeError") and c["message"] and c["trace"] == [], n
        # no output buffer; make_glide's own zeroed rows, part of the request, are the one array counted for its family
        # (make_portfolio refuses five weights before make_glide runs)
        assert c["allocated"] == (1 if n.startswith("glide|") and "|bad:five_weights|" not in n else 0), n


def test_every_public_signature_is_unchanged(golden):
    now = G.signatures()
    assert sorted(now) == sorted(golden["signatures"])
    for name, text in golden["signatures"].items():
        assert now[name] == text, name


def test_no_entry_gained_a_call_or_a_wait(golden, digests):
    """Part of the comparison above (the allocations are inside the digest); stated alone because it is what keeps the
    per-call cost where it was."""
    for n, want in golden["cases"].items():
        assert digests[n]["trace"] == want["trace"], n

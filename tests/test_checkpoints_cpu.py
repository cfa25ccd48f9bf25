"""Checkpoint statistics without a GPU: the two entry points are exported and bound, every argument error the
header lists comes back as SMMC_ERR_INVALID with a text (csrc/smmc_capi.cpp over tests/cpp/fake_hip.cpp, driven by
tests/cpp/checkpoints_args.cpp), and fan() -- quantiles over time from the bucket counts -- against numpy.quantile."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stock_market_monte_carlo_amd", "csrc")
NAMES = ("smmc_engine_simulate_checkpoints", "smmc_engine_simulate_checkpoints_to_host")


def test_entry_points_are_declared_exported_and_bound():
    from stock_market_monte_carlo_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "smmc.h")).read()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    build.build()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB]).decode()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in bound and len(bound[name][2]) == 6, name
        assert re.search(r" T %s$" % name, exported, flags=re.M), name
    m = re.search(r"#define SMMC_MAX_CHECKPOINT_BINS (\d+)", hdr)
    assert m and int(m.group(1)) == _lib.MAX_CHECKPOINT_BINS >= max(64 * 128, 31 * 256)
    assert re.search(r"#define SMMC_MAX_CHECKPOINTS 64\b", hdr) and _lib.MAX_CHECKPOINTS == 64
    assert _lib.ABI_VERSION == 4  # additive: the ABI version and the structures stay


@pytest.fixture(scope="module")
def args_report(tmp_path_factory):
    """tests/cpp/checkpoints_args.cpp over the fake HIP runtime: {case: (return code, length of the error text)}."""
    exe = str(tmp_path_factory.mktemp("ck") / "checkpoints_args")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = [os.path.join(CSRC, f) for f in ("smmc_capi.cpp", "smmc_group.cpp", "smmc_dropin.cpp")]
    src += [os.path.join(ROOT, "tests", "cpp", f) for f in ("fake_hip.cpp", "launch_fake.cpp", "checkpoints_args.cpp")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + rocm + "/include",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe] + src + ["-pthread", "-ldl"])
    env = dict(os.environ, FAKE_HIP_DEVICES="1")
    r = subprocess.run([exe], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "checkpoints_args: done" in r.stdout, (r.stdout + r.stderr)[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        parts = line.split()
        if len(parts) == 3 and not line.startswith("#"):
            out[parts[0]] = (int(parts[1]), int(parts[2]))
    return out


INVALID = ["n_checkpoints_zero", "n_checkpoints_above_max", "period_zero", "period_above_n_periods", "period_repeated",
           "period_decreasing", "periods_null", "records_null", "stream_ref", "stream_v2", "histogram_budget_64x129",
           "histogram_budget_32x257", "engine_null"]


@pytest.mark.parametrize("entry", ["device", "to_host"])
@pytest.mark.parametrize("case", INVALID)
def test_argument_errors_are_invalid_with_a_text(args_report, entry, case):
    rc, text_len = args_report[f"{entry}:{case}"]
    assert rc == -1, (entry, case, rc)  # SMMC_ERR_INVALID
    assert text_len > 0


def test_a_valid_request_passes_the_argument_checks(args_report):
    """64 checkpoints x 128 buckets is inside the budget: the host-only build then stops at its missing kernel
    (an error of its own, not SMMC_ERR_INVALID and not a result)."""
    assert args_report["budget"] == (1, 1)
    rc, text_len = args_report["valid_request_without_kernel"]
    assert rc == -2 and text_len > 0


def _records(values, lo, hi, n_bins):
    from stock_market_monte_carlo_amd.engine import Stats
    v = np.asarray(values, dtype=np.float64)
    inside = v[(v >= lo) & (v < hi)]
    hist = np.histogram(inside, bins=n_bins, range=(lo, hi))[0].astype(np.uint64)
    return Stats(v.size, int((v < 1000.0).sum()), int((v < lo).sum()), int((v >= hi).sum()), float(v.sum()), float((v * v).sum()),
                 float(v.min()), float(v.max()), hist, lo, hi)


def test_fan_agrees_with_numpy_quantile_to_one_bucket():
    from stock_market_monte_carlo_amd import fan
    rng = np.random.default_rng(11)
    lo, hi, n_bins = 0.0, 2500.0, 100
    width = (hi - lo) / n_bins
    cols = [rng.lognormal(np.log(1000.0) + 0.05 * k, 0.1 + 0.05 * k, 200_000) for k in range(6)]
    qs = [0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0]
    out = fan([_records(c, lo, hi, n_bins) for c in cols], qs)
    assert out.values.shape == out.clipped.shape == (6, len(qs))
    for k, c in enumerate(cols):
        want = np.quantile(c, qs)
        for j, q in enumerate(qs):
            if out.clipped[k, j] == 0:
                assert abs(out.values[k, j] - want[j]) <= width, (k, q, out.values[k, j], want[j])
            elif out.clipped[k, j] > 0:
                assert out.values[k, j] == hi and want[j] >= hi - width, (k, q)
            else:
                assert out.values[k, j] == lo and want[j] <= lo + width, (k, q)
    assert (out.clipped[0, 1:-1] == 0).all()       # the narrow early column lies inside the range
    assert out.clipped[5, -2] == 1                  # the wide late one has its 99 % point above it
    assert np.all(np.diff(out.values, axis=1) >= 0)  # quantiles are monotone in q


def test_fan_respects_underflow_and_overflow_mass():
    from stock_market_monte_carlo_amd import fan
    from stock_market_monte_carlo_amd.engine import Stats
    # 100 values: 30 below the range, 40 inside (10 per bucket), 30 above it
    st = Stats(100, 0, 30, 30, 0.0, 0.0, 0.0, 0.0, np.array([10, 10, 10, 10], dtype=np.uint64), 100.0, 500.0)
    out = fan([st], [0.1, 0.3, 0.35, 0.5, 0.7, 0.71, 0.9])
    assert list(out.clipped[0]) == [-1, 0, 0, 0, 0, 1, 1]
    assert out.values[0, 0] == 100.0 and out.values[0, -1] == 500.0
    assert out.values[0, 1] == pytest.approx(100.0) and out.values[0, 2] == pytest.approx(150.0)
    assert out.values[0, 3] == pytest.approx(300.0) and out.values[0, 4] == pytest.approx(500.0)
    empty = Stats(0, 0, 0, 0, 0.0, 0.0, float("inf"), float("-inf"), np.zeros(4, dtype=np.uint64), 100.0, 500.0)
    assert np.isnan(fan([empty], [0.5]).values).all()
    with pytest.raises(ValueError):
        fan([st], [1.5])
    no_hist = Stats(5, 0, 0, 0, 0.0, 0.0, 0.0, 0.0, np.zeros(0, dtype=np.uint64))
    with pytest.raises(ValueError):
        fan([no_hist], [0.5])

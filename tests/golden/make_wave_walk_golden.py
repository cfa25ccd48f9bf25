"""Writes tests/golden/wave_walk_parent.json: the sha256 of every output buffer of the three wave-walk features
(checkpoint statistics, cash flows, excursions) for the cases below, taken on an MI355X with the library of the
commit BEFORE their kernels were given one skeleton.  The records are hashed as raw bytes, so the order in which the
double sums were accumulated is pinned.  tests/test_wave_walk_bytes_gpu.py runs the same cases (digests() below) and
compares; the digests belong to the launch geometry recorded beside them.

Run it on that commit (copy this file into its tree): python tests/golden/make_wave_walk_golden.py [--out FILE]"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "wave_walk_parent.json")
SEED, FIRST_PATH = 20240607, 3
GROUPS_PER_CU = 32  # of the three kernels alike (csrc/smmc_capi.cpp, smmc_cashflow.cpp, smmc_excursions.cpp)
FOUR_DRAW_TABLE = 2500  # above 2048 entries a table path draws four periods per Philox block


def draw_cases():
    """(name, mode, table_len or 0, periods per Philox block)"""
    return [("gaussian", "gaussian", 0, 4), ("table", "table", 1127, 8), ("table4", "table", FOUR_DRAW_TABLE, 4)]


def shapes(block, group_paths, geometry):
    """(n_paths, n_periods, n_bins, every per-path output | only the final values): every period count at 4099 paths,
    every path count at 13 periods, both with and without buckets, and the size at which every wave walks more than
    one chunk and the last chunk is ragged."""
    grid, _, cus = geometry
    cap = min(cus * GROUPS_PER_CU, grid)
    out = [(4099, p, b, True) for p in (1, block, 13) for b in (0, 100)]
    out += [(n, 13, b, True) for n in (1, 63) for b in (0, 100)]
    out.append((2 * cap * group_paths + 77, 5, 100, False))
    return out


def _sha(t):
    import numpy as np
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return hashlib.sha256(a.tobytes()).hexdigest()


def digests(S, eng, table):
    """{case: {buffer: sha256}} on `eng`; `table` is the bundled returns table."""
    import numpy as np
    out = {}
    geometry = eng.geometry()
    for name, mode, table_len, block in draw_cases():
        if table_len:
            eng.set_table(np.resize(table, table_len))  # the bundled table, repeated to the length
        m = S.MODE_TABLE if mode == "table" else S.MODE_GAUSSIAN
        for n, p, bins, per_path in shapes(block, 512 if mode == "gaussian" else 256, geometry):
            for exact in (False, True):
                sim = S.Engine.make_sim(n, p, m, SEED, first_path=FIRST_PATH, n_bins=bins, hist_lo=0.0, hist_hi=2500.0,
                                        exact_div=exact)
                key = f"{name}|{n}|{p}|{bins}|{'exact' if exact else 'default'}"
                if p == 13:  # checkpoints: periods {1, 4, 13}
                    rec, final = eng.simulate_checkpoints_raw(sim, [1, 4, 13], want_final=True)
                    out["checkpoints|" + key] = {"records": hashlib.sha256(rec).hexdigest(), "final": _sha(final)}
                elif not per_path:
                    rec, final = eng.simulate_checkpoints_raw(sim, [2, 5], want_final=True)
                    out["checkpoints|" + key] = {"records": hashlib.sha256(rec).hexdigest(), "final": _sha(final)}
                schedules = {"constant": dict(amount=6.0, fraction=0.001, floor=0.01),
                             "varying": dict(amounts=(6.0 * 1.01 ** np.arange(p)).astype(np.float32),
                                             fractions=np.linspace(0.0, 0.02, p).astype(np.float32), floor=0.01)}
                for sname, sched in schedules.items():
                    r = eng.simulate_cashflow_raw(sim, want_final=True, want_paid=per_path, want_ruin_period=per_path,
                                                  want_stats=True, want_depleted_at=True, **sched)
                    eng.sync()
                    out[f"cashflow_{sname}|" + key] = {k: _sha(v) for k, v in r.items() if v is not None}
                both = dict(want_stats=True, want_drawdown_stats=True)
                one = dict(want_stats=False, want_drawdown_stats=True)
                for rname, recs in (("both", both), ("one", one)):
                    wants = {"want_" + k: per_path or k == "final" for k in ("final", "peak", "low", "drawdown", "drawdown_period", "underwater",
                                                             "first_below", "first_reach")}
                    r = eng.simulate_excursions_raw(sim, 990.0, 1030.0, 0.01, want_first_below_at=True, want_first_reach_at=True,
                                                    **wants, **recs)
                    eng.sync()
                    out[f"excursions_{rname}|" + key] = {k: _sha(v) for k, v in r.items() if v is not None}
    return out


def generate():
    import stock_market_monte_carlo_amd as S
    table = S.read_historical_returns(os.path.join(ROOT, "data", "SP500_monthly_returns.csv"))
    eng = S.Engine(0)
    doc = {"geometry": list(eng.geometry()), "seed": SEED, "first_path": FIRST_PATH, "cases": digests(S, eng, table)}
    eng.close()
    return doc


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    doc = generate()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{out}: {len(doc['cases'])} cases, geometry {doc['geometry']}")

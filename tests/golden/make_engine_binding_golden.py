"""Writes tests/golden/engine_binding_parent.json: what the feature entries of stock_market_monte_carlo_amd/engine.py
hand to the C library and give back, taken on the commit BEFORE their marshalling was moved into one binding layer.
No GPU and no shared library: an Engine subclass on the CPU whose library is a recorder (observe() below).  Per entry
and case it records the trace (_enter, the C calls, _leave, sync), of every C call the scalars, the non-pointer fields
of every structure and, of every pointer, whether it is null and which buffer of the returned value it addresses, and
the returned value itself: key order, type, dtype and shape per key; for a bad input the exception.  Beside the cases,
the text of every public signature of Engine.  The file keeps a refusal whole and of every other observation its trace
and the sha256 of the rest (digest() below), as tests/golden/wave_walk_parent.json keeps digests of buffers;
--full FILE writes the observations themselves, to read a difference.  tests/test_engine_binding_cpu.py derives the same
from the working tree (observe()) and compares.

Run it on that commit (copy this file into its tree): python tests/golden/make_engine_binding_golden.py [--out FILE] [--full FILE]"""
import contextlib
import ctypes as C
import dataclasses
import hashlib
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, "engine_binding_parent.json")
N_PATHS, N_PERIODS = 5, 3  # nothing here depends on magnitude


# ---- the engine without a GPU -------------------------------------------------------------------------------------------

class Recorder:
    """Stands in for the ctypes library: answers smmc_stats_bytes, records every other call and returns 0."""

    def __init__(self):
        self.trace = []

    def smmc_stats_bytes(self, n_bins):
        from stock_market_monte_carlo_amd import _lib
        return C.sizeof(_lib.Stats) + 8 * int(n_bins)

    def __getattr__(self, name):
        def call(*args):
            self.trace.append((name, args))
            return 0
        return call


def _tensor_class():
    import torch

    class Addressed(torch.Tensor):
        """A tensor whose EMPTY block has an address too, as an allocator's may: torch itself answers 0 there, which
        would hide whether the wrapper passes a null pointer for an output without elements."""

        def data_ptr(self):
            return torch.Tensor.data_ptr(self) or id(self)
    return Addressed


class TorchShim:
    """torch with `empty` returning zeros (a read-back wrapper then decodes an all-zero record) and keeping what it
    allocated, in order, so that a pointer can be named after the call."""

    def __init__(self, made):
        import torch
        self._torch, self._made, self._cls = torch, made, _tensor_class()

    def empty(self, *size, dtype=None, device=None):
        t = self._torch.zeros(*size, dtype=dtype, device=device).as_subclass(self._cls)
        self._made.append(t)
        return t

    def __getattr__(self, name):
        return getattr(self._torch, name)


class NumpyShim:
    """numpy with `zeros` keeping what it allocated: a host record is handed back as bytes, its array is gone by then."""

    def __init__(self, made):
        import numpy
        self._numpy, self._made = numpy, made

    def zeros(self, *args, **kwargs):
        a = self._numpy.zeros(*args, **kwargs)
        self._made.append(a)
        return a

    def __getattr__(self, name):
        return getattr(self._numpy, name)


def make_engine(made):
    import torch
    from stock_market_monte_carlo_amd.engine import Engine

    class CpuEngine(Engine):
        def __init__(self):
            self._torch = TorchShim(made)
            self.tdevice = torch.device("cpu")
            self.device, self.table_len = 0, 0
            self._h = None
            self.own_stream = self.follow_torch = False
            self._L = Recorder()

        def _enter(self):
            self._L.trace.append(("_enter", ()))
            return 0

        def _leave(self, cur, *tensors):
            self._L.trace.append(("_leave", ()))

        def sync(self):
            self._L.trace.append(("sync", ()))

        def __del__(self):
            pass

    return CpuEngine()


@contextlib.contextmanager
def numpy_recorded(made):
    from stock_market_monte_carlo_amd import engine
    real = engine.np
    engine.np = NumpyShim(made)
    try:
        yield
    finally:
        engine.np = real


# ---- describing what was seen -------------------------------------------------------------------------------------------

def _is_tensor(v):
    return hasattr(v, "data_ptr") and hasattr(v, "numel")


def _is_array(v):
    import numpy as np
    return isinstance(v, np.ndarray)


def _buffer(v):
    if _is_tensor(v):
        return "tensor %s%s" % (str(v.dtype).replace("torch.", ""), list(v.shape))
    return "ndarray %s%s" % (v.dtype, list(v.shape))


def describe(v, named=None, made=()):
    """A returned value as JSON: type, dtype and shape, never contents."""
    if isinstance(v, C.Structure):
        return _struct(v, named or {}, made)
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if _is_tensor(v) or _is_array(v):
        return _buffer(v)
    if isinstance(v, (bytes, bytearray)):
        return "bytes[%d]" % len(v)
    if hasattr(v, "item") and not hasattr(v, "__len__"):
        return v.item()  # a numpy scalar
    if isinstance(v, dict):
        return {"type": "dict", "keys": list(v), "values": {k: describe(x) for k, x in v.items()}}
    if dataclasses.is_dataclass(v):
        return {"type": type(v).__name__, "fields": {f.name: describe(getattr(v, f.name)) for f in dataclasses.fields(v)}}
    if isinstance(v, (list, tuple)):
        return {"type": type(v).__name__, "items": [describe(x, named, made) for x in v]}
    return "<%s>" % type(v).__name__


def _named_buffers(value):
    """{name: buffer} of the tensors and arrays a returned value holds."""
    if isinstance(value, dict):
        items = value.items()
    elif dataclasses.is_dataclass(value):
        items = [(f.name, getattr(value, f.name)) for f in dataclasses.fields(value)]
    elif isinstance(value, (list, tuple)):
        items = [(str(i), x) for i, x in enumerate(value)]
        items += [("%d.%d" % (i, j), y) for i, x in enumerate(value) if isinstance(x, (list, tuple)) for j, y in enumerate(x)]
        items += [kv for x in value if isinstance(x, dict) for kv in x.items()]
    else:
        items = []
    return {k: x for k, x in items if _is_tensor(x) or _is_array(x)}


def _address(v):
    return int(v.data_ptr()) if _is_tensor(v) else int(v.ctypes.data)


def _pointer(addr, named, made):
    """null, or the returned value's key whose buffer starts there and what the wrapper allocated there."""
    if not addr:
        return "null"
    key = next((k for k, x in named.items() if _address(x) == addr), None)
    what = next((_buffer(x) for x in made if _address(x) == addr), None)
    return "-> %s (%s)" % (key if key is not None else "?", what if what is not None else "not allocated by the entry")


def _struct(s, named, made):
    out = {}
    for name, ctype in s._fields_:
        v = getattr(s, name)
        if ctype is C.c_void_p:
            out[name] = _pointer(v, named, made)
        elif isinstance(v, C._Pointer):
            out[name] = _pointer(C.cast(v, C.c_void_p).value, named, made)
        elif isinstance(v, C.Array):
            out[name] = list(v)
        else:
            out[name] = v
    return out


def _argument(a, named, made):
    if a is None:
        return "null"
    if isinstance(a, (bool, int, float)):
        return a
    if isinstance(a, C.c_void_p):
        return _pointer(a.value, named, made)
    if isinstance(a, C.Structure):
        return _struct(a, named, made)
    if isinstance(a, C.Array):
        return [_argument(x, named, made) for x in a]
    if hasattr(a, "_obj"):  # byref(...)
        return _argument(a._obj, named, made)
    if hasattr(a, "value"):
        return a.value
    return "<%s>" % type(a).__name__


def run(entry, sim_args, args, kwargs):
    """One call of Engine.<entry> on a fresh CPU engine -> what it did and gave back, or how it refused."""
    from stock_market_monte_carlo_amd.engine import Engine
    made = []
    eng = make_engine(made)
    sim = Engine.make_sim(*sim_args[0], **sim_args[1])
    method = getattr(eng, entry)
    accepted = inspect.signature(method).parameters
    if not any(p.kind is p.VAR_KEYWORD for p in accepted.values()):
        kwargs = {k: v for k, v in kwargs.items() if k in accepted}
    with numpy_recorded(made):
        try:
            value = method(sim, *args, **kwargs)
        except (ValueError, TypeError, AssertionError) as err:
            return {"raises": type(err).__name__, "message": str(err), "trace": [name for name, _ in eng._L.trace],
                    "allocated": len(made)}
    named = _named_buffers(value)
    calls = [{"call": name, "args": [_argument(a, named, made) for a in a_]} for name, a_ in eng._L.trace if a_]
    return {"trace": [name for name, _ in eng._L.trace], "calls": calls, "returns": describe(value, named, made),
            "allocated": [_buffer(x) for x in made]}


# ---- the cases ----------------------------------------------------------------------------------------------------------

def _sim(n_paths=N_PATHS, n_bins=0):
    return ((n_paths, N_PERIODS, 1, 20240607), dict(n_bins=n_bins, hist_lo=0.0, hist_hi=2500.0))


def _wants(names, value):
    return {"want_" + n: value for n in names}


def _want_cases(names):
    """(tag, n_paths, n_bins, want arguments): the defaults, every want on with and without buckets, every want off, and
    every want on without a path."""
    return [("defaults", N_PATHS, 0, {}), ("on_bins4", N_PATHS, 4, _wants(names, True)), ("on_bins0", N_PATHS, 0, _wants(names, True)),
            ("off", N_PATHS, 4, _wants(names, False)), ("on_no_paths", 0, 4, _wants(names, True))]


W1, W3 = (1.0,), (0.5, 0.3, 0.2)
PFCF_WANTS = ("final", "holdings", "paid", "ruin_period", "stats", "depleted_at")
CF_WANTS = ("final", "paid", "ruin_period", "stats", "depleted_at")


def families():
    """name -> (entries, wants, {variant: (args, kwargs)}, {bad input: (args, kwargs)})"""
    import numpy as np
    from stock_market_monte_carlo_amd import _lib
    arrays = dict(amounts=np.array([6.0, 6.5, 7.0], dtype=np.float32), fractions=[0.0, 0.01, 0.02], floor=0.01)
    const = dict(amount=6.0, fraction=0.001, floor=0.01)
    four = lambda f: [f, f + "_raw", f + "_to_host", f[len("simulate_"):] + "_divide_kind"]  # noqa: E731
    three = lambda f: [f, f + "_raw", f + "_to_host"]  # noqa: E731
    law3 = dict(means=(0.5, 0.2, 0.25), factor=np.tril(np.ones((3, 3), dtype=np.float32)))
    out = {}
    out["cashflow"] = (four("simulate_cashflow"), CF_WANTS, {"constant": ((), const), "arrays": ((), arrays)},
                       {"amounts_of_wrong_length": ((), dict(amounts=[1.0, 2.0])), "fractions_two_dimensional": ((), dict(fractions=np.zeros((3, 1))))})
    out["cashflow_sweep"] = (four("simulate_cashflow_sweep"), CF_WANTS,
                             {"S1": (([40.0],), dict(fractions=0.001)), "S3": (([40.0, 50.0, 60.0],), dict(floors=[0.0, 1.0, 2.0]))},
                             {"lengths_differ": (([1.0, 2.0],), dict(fractions=[0.1, 0.2, 0.3])), "amounts_two_dimensional": (([[1.0, 2.0]],), {})})
    out["excursions"] = (three("simulate_excursions"), _lib.EXCURSION_OUTPUTS, {"levels": ((990.0, 1030.0), dict(drawdown_threshold=0.1))},
                         {"unknown_want": ((990.0, 1030.0), dict(want_nothing=True)), "not_a_want": ((990.0, 1030.0), dict(final=True))})
    out["blocks"] = (four("simulate_blocks"), ("final", "chunk_stats", "stats"), {"len2": ((2,), {})}, {})
    out["portfolio"] = (four("simulate_portfolio"), ("final", "holdings", "stats"),
                        {"K1": ((W1,), {}), "K3": ((W3,), dict(rebalance_every=2, **law3))},
                        {"five_weights": (((0.2,) * 5,), {}), "no_weights": (((),), {}), "means_of_wrong_length": ((W3,), dict(means=(0.5, 0.2)))})
    out["portfolio_cashflow"] = (four("simulate_portfolio_cashflow"), PFCF_WANTS,
                                 {"K1": ((W1,), const), "K3": ((W3,), dict(rebalance_every=2, **arrays, **law3))},
                                 {"five_weights": (((0.2,) * 5,), const), "amounts_of_wrong_length": ((W3,), dict(amounts=[1.0]))})
    change = [(2, (0.2, 0.3, 0.5))]
    out["glide"] = (four("simulate_glide"), PFCF_WANTS,
                    {"K1_no_change": ((W1, None), const), "K3_no_change": ((W3, []), const),
                     "K3_one_change": ((W3, change), dict(rebalance_every=1, **arrays, **law3))},
                    {"five_weights": (((0.2,) * 5, change), const), "row_of_five_weights": ((W3, [(1, (0.2,) * 5)]), const),
                     "amounts_of_wrong_length": ((W3, change), dict(amounts=[1.0]))})
    out["portfolio_cashflow_blocks"] = (four("simulate_portfolio_cashflow_blocks"), PFCF_WANTS,
                                        {"K1": ((W1, 2), const), "K3": ((W3, 3), dict(rebalance_every=2, **arrays))},
                                        {"five_weights": (((0.2,) * 5, 2), const), "amounts_of_wrong_length": ((W3, 2), dict(amounts=[1.0]))})
    out["guardrails"] = (three("simulate_guardrails"), _lib.GUARDRAILS_OUTPUTS,
                         {"K1": ((W1, 40.0), {}), "K3": ((W3, 40.0), dict(review_every=2, upper=0.06, lower=0.03, index=1.002, amount_min=10.0,
                                                                         amount_max=90.0, floor=0.5, rebalance_every=2, **law3))},
                         {"five_weights": (((0.2,) * 5, 40.0), {}), "factor_of_wrong_shape": ((W3, 40.0), dict(factor=np.ones((2, 2))))})
    out["portfolio_cashflow_checkpoints"] = (three("simulate_portfolio_cashflow_checkpoints"), PFCF_WANTS,
                                             {"K1_no_period": ((W1, []), const), "K3_two_periods": ((W3, [1, 3]), dict(rebalance_every=2, **arrays, **law3))},
                                             {"negative_period": ((W3, [1, -2]), const), "period_beyond_32_bits": ((W3, [2 ** 32]), const),
                                              "five_weights": (((0.2,) * 5, [1]), const), "amounts_of_wrong_length": ((W3, [1]), dict(amounts=[1.0]))})
    law4 = dict(means=(0.5, 0.2, 0.1, 0.25), factor=np.tril(np.ones((4, 4), dtype=np.float32)))
    out["real_cashflow"] = (four("simulate_real_cashflow"), ("final", "final_real", "index", "holdings", "paid", "ruin_period", "stats", "depleted_at"),
                            {"K1": ((W1,), const), "K3": ((W3,), dict(rebalance_every=2, **arrays, **law4))},
                            {"four_weights": (((0.25,) * 4,), const), "amounts_of_wrong_length": ((W3,), dict(amounts=[1.0])),
                             "means_without_inflation": ((W3,), dict(means=(0.5, 0.2, 0.1)))})
    out["allocation_sweep"] = (four("simulate_allocation_sweep"), PFCF_WANTS,
                               {"S1_K1": (([W1],), dict(amounts=40.0)), "S1_K3": (([W3],), dict(rebalance_every=2, amounts=40.0, **law3)),
                                "S3_K1": (([W1, W1, W1],), dict(amounts=[40.0, 50.0, 60.0], floors=1.0)),
                                "S3_K3": (([W3, (0.2, 0.3, 0.5), (1.0, 0.0, 0.0)],), dict(rebalance_every=[0, 1, 12], amounts=40.0, fractions=[0.0, 0.001, 0.002]))},
                               {"one_weight_vector": ((W3,), {}), "five_weights": (([(0.2,) * 5],), {}), "amounts_of_other_length": (([W3, W3],), dict(amounts=[1.0, 2.0, 3.0]))})
    return out


def extra_cases():
    """(case, entry, sim, args, kwargs): what the families' grid does not reach."""
    import numpy as np
    import torch
    out = []
    for entry in ("simulate_portfolio", "simulate_portfolio_raw"):
        out.append(("portfolio|out_given|" + entry, entry, _sim(n_bins=4), (W3,), dict(out=torch.zeros(8), want_holdings=True, want_stats=True)))
        out.append(("portfolio|out_given_not_wanted|" + entry, entry, _sim(), (W3,), dict(out=torch.zeros(8), want_final=False)))
        out.append(("portfolio|out_too_short|" + entry, entry, _sim(), (W3,), dict(out=torch.zeros(4))))
    for entry in ("simulate_blocks", "simulate_blocks_raw"):
        out.append(("blocks|out_given|" + entry, entry, _sim(n_bins=4), (2,), dict(out=torch.zeros(8), want_chunk_stats=True, want_stats=True)))
        out.append(("blocks|out_of_other_type|" + entry, entry, _sim(), (2,), dict(out=torch.zeros(8, dtype=torch.float64))))
    out.append(("blocks|host_out_given|simulate_blocks_to_host", "simulate_blocks_to_host", _sim(n_bins=4), (2,),
                dict(out=np.zeros(8, dtype=np.float32), want_stats=True, want_chunk_stats=True)))
    for tag, periods in (("no_period", []), ("two_periods", [1, 3])):
        for want_final in (False, True):
            for n in (N_PATHS, 0):
                name = "checkpoints|%s|final_%d|n%d|" % (tag, want_final, n)
                out.append((name + "simulate_checkpoints", "simulate_checkpoints", _sim(n, 4), (periods,), dict(want_final=want_final)))
                for to_host in (False, True):
                    out.append((name + "simulate_checkpoints_raw|to_host_%d" % to_host, "simulate_checkpoints_raw", _sim(n, 4), (periods,),
                                dict(want_final=want_final, to_host=to_host)))
    out.append(("checkpoints|negative_period|simulate_checkpoints", "simulate_checkpoints", _sim(), ([1, -2],), {}))
    for wants in ({}, _wants(("final", "final_real", "index", "holdings", "paid", "ruin_period", "stats", "depleted_at"), True)):
        for n in (N_PATHS, 0):
            out.append(("real_cashflow|outputs|%s|n%d|make_real_cashflow_outputs" % ("on" if wants else "defaults", n),
                        "make_real_cashflow_outputs", _sim(n, 4), (2,), wants))
    out.append(("divide_kind|simulate|divide_kind", "divide_kind", _sim(), (), {}))
    out.append(("divide_kind|keepdata|divide_kind", "divide_kind", _sim(), (), dict(keepdata=True)))
    out.append(("paths_form|simulate|paths_form", "paths_form", _sim(), (), {}))
    return out


def cases():
    """[(case name, entry, sim arguments, args, kwargs)]"""
    out = []
    for family, (entries, wants, variants, bad) in families().items():
        for variant, (args, kwargs) in variants.items():
            for tag, n, bins, want in _want_cases(wants):
                if variant != next(iter(variants)) and tag not in ("on_bins4", "on_no_paths"):
                    continue  # the grid of wants on the family's first variant; every other variant with all of them
                for entry in entries:
                    out.append(("%s|%s|%s|%s" % (family, variant, tag, entry), entry, _sim(n, bins), args, dict(kwargs, **want)))
        for name, (args, kwargs) in bad.items():
            for entry in entries:
                out.append(("%s|bad:%s|%s" % (family, name, entry), entry, _sim(), args, kwargs))
    return out + extra_cases()


def signatures():
    from stock_market_monte_carlo_amd.engine import Engine
    return {name: str(inspect.signature(getattr(Engine, name))) for name in sorted(vars(Engine))
            if not name.startswith("_") and callable(getattr(Engine, name))}


def observe():
    """{"signatures": {...}, "cases": {case: observation}} of the package in the tree this file lies in."""
    seen = {}
    for name, entry, sim, args, kwargs in cases():
        assert name not in seen, name
        seen[name] = run(entry, sim, args, kwargs)
    return {"signatures": signatures(), "cases": seen}


def digest(seen):
    """What the golden keeps of an observation: a refusal as it is, else the trace and the sha256 of the whole."""
    if "raises" in seen:
        return seen
    return {"trace": " ".join(seen["trace"]), "sha256": hashlib.sha256(json.dumps(seen, sort_keys=True).encode()).hexdigest()[:32]}


def dump(doc, fh):
    """One case per line, so that a change shows as the lines of the cases it touches."""
    fh.write('{\n"signatures": {\n')
    fh.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sorted(doc["signatures"].items())))
    fh.write('\n},\n"cases": {\n')
    fh.write(",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(doc["cases"].items())))
    fh.write("\n}\n}\n")


if __name__ == "__main__":
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    doc = observe()
    if "--full" in sys.argv:
        with open(sys.argv[sys.argv.index("--full") + 1], "w") as fh:
            dump(doc, fh)
    doc["cases"] = {name: digest(seen) for name, seen in doc["cases"].items()}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        dump(doc, fh)
    print(f"{out}: {len(doc['cases'])} cases, {len(doc['signatures'])} signatures")

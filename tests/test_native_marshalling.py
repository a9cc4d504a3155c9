"""
CPU-only check of the marshalling layer of _native.py: what every gadget wrapper and Context method hands to its entry point.

_native.lib is replaced by a recorder, so neither the built library nor a GPU is needed.  Every argument of a call is a sentinel or
an array of its own -- no two scalars of the sentinels below are equal, the two syndrome tables have different lengths -- and the
recorded arguments are compared with them by the parameter names of include/gf2hip.h: a swapped, missing or surplus argument, a
pointer to another array or a call of another entry point fails here, before anything runs on a device.
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from quantum_css_codes_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_parameters():
    """name -> parameter names of every declaration of include/gf2hip.h (test_abi.header_functions parses the same text)."""
    text = open(os.path.join(ROOT, "include", "gf2hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = re.findall(r"\b(?:int64_t|int|const char\*)\s+(gf2_\w+)\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    return {name: [re.split(r"[\s*]+", a.strip())[-1] for a in args.split(",")] if args.strip() != "void" else [] for name, args in decls}


PARAMETERS = header_parameters()


class Recorder(object):
    """Stands in for the loaded library: every attribute is a function that appends (name, args, peeked) to `calls` and returns 0.
    `peek` maps a parameter name to (dtype, length): what that pointer addresses is copied while the wrapper's arrays are alive."""

    def __init__(self):
        self.calls, self.peek = [], {}

    def __getattr__(self, name):
        def entry_point(*args):
            peeked = {}
            for param, (dtype, length) in self.peek.items():
                buf = (ctypes.c_char * (np.dtype(dtype).itemsize * length)).from_address(address(args[PARAMETERS[name].index(param)]))
                peeked[param] = np.frombuffer(buf, dtype=dtype).copy()
            self.calls.append((name, args, peeked))
            return 0
        return entry_point


def address(arg):
    """The address a recorded pointer argument holds (0: null)."""
    if arg is None:
        return 0
    if isinstance(arg, int):
        return arg
    if hasattr(arg, "_obj"):                                 # ctypes.byref(...)
        return ctypes.addressof(arg._obj)
    return arg.value or 0                                    # c_void_p


def scalar(arg):
    return arg.value if hasattr(arg, "value") else arg       # (ctypes wraps some scalars: c_int64, ...)


# ---- the sentinels: all different ---------------------------------------------------------------------------------------------
S = dict(rounds=3, nsteps=5, measure_mask=(1 << 63) | 45, r1=11, r2=13, seed=17, first_sample=19, count=23, p_x=0.01, p_y=0.02, p_z=0.03,
         k_x=1.5, k_y=2.5, k_z=3.5, w=4, b=2, first_rank=29, n1=7, n2=9, select=6, capacity=31, p1=0.04, p2=0.05, max_attempts=37,
         flag_words=41)
LDR_ARGUMENT, CTX_HANDLE, OBJECT_HANDLE = 43, 101, 202
EC_F, FT_F = _native.EC_FIELDS_COUNT, _native.FT_FIELDS_COUNT


def arrays():
    """Fresh arrays of the final dtype, contiguous, every length its own: name -> array."""
    rng = np.random.default_rng(7)
    u64 = lambda *shape: rng.integers(0, 1 << 62, shape).astype("<u8")
    return dict(words=u64(15, 16), eff=u64(8, 2, 10), keys1=u64(12, 1), flips1=rng.integers(0, 2, 12).astype(np.uint8), keys2=u64(14, 1),
                flips2=rng.integers(0, 2, 14).astype(np.uint8), site_loc=np.arange(S["n1"] + S["n2"], dtype=np.int32),
                weights=np.arange(20, dtype=np.int32) % 5, counts=np.arange(20, dtype=np.int64) + 100,
                strata=rng.integers(0, 8, (20, 2)).astype(np.int32), block_kind=np.arange(18, dtype=np.int32) % 4)


def sentinels_distinct():
    a = arrays()
    values = list(S.values()) + [LDR_ARGUMENT, CTX_HANDLE, OBJECT_HANDLE, len(a["keys1"]), len(a["keys2"]), len(a["weights"]),
                                 len(a["block_kind"])] + list(a["words"].shape) + [a["eff"].shape[0], a["eff"].shape[2]]
    return len(set(values)) == len(values)


def cases():
    """name of the case -> (entry point, call(ctx, obj, arrays), what the header's parameters must receive beyond S and the arrays,
    the result's shape).  `derived` lists pointers to arrays the wrapper makes itself: parameter -> the contents they must have."""
    ec, ft = ("rounds",), ("nsteps", "measure_mask")
    head = lambda rule: tuple(S[k] for k in rule)
    tables = lambda a: (S["r1"], a["keys1"], a["flips1"], S["r2"], a["keys2"], a["flips2"])
    sites = lambda a: (a["site_loc"], S["n1"], S["n2"])
    mc = (S["seed"], S["first_sample"], S["count"], S["p_x"], S["p_y"], S["p_z"])
    kinds = (S["k_x"], S["k_y"], S["k_z"])
    ranks = (S["w"], S["first_rank"], S["count"])
    gate_ranks = (S["w"], S["b"], S["first_rank"], S["count"])
    listed = ranks + (S["select"], S["capacity"])
    tally = dict(count=15, ldw=16, ldr=LDR_ARGUMENT)
    host = dict(locations=8, ldr=10)
    out = {}
    for name, rule, fields in (("ec", ec, EC_F), ("ft", ft, FT_F)):
        h = head(rule)
        out["%s_tally_host" % name] = ("gf2_%s_tally_host" % name, lambda c, o, a, f=getattr(_native, "%s_tally_host" % name), h=h:
                                       f(a["words"], *h, *tables(a), ldr=LDR_ARGUMENT, classes=True), tally, ((fields,), (15,)))
        out["%s_enumerate_host" % name] = ("gf2_%s_enumerate_host" % name, lambda c, o, a, f=getattr(_native, "%s_enumerate_host" % name), h=h:
                                           f(a["eff"], *h, *tables(a), *ranks), host, (5, 5, fields))
        out["%s_gate_enumerate_host" % name] = ("gf2_%s_gate_enumerate_host" % name,
                                                lambda c, o, a, f=getattr(_native, "%s_gate_enumerate_host" % name), h=h:
                                                f(a["eff"], *h, *tables(a), *sites(a), *gate_ranks), host, (3, fields))
        out["%s_enumerate_list_host" % name] = ("gf2_%s_enumerate_list_host" % name,
                                                lambda c, o, a, f=getattr(_native, "%s_enumerate_list_host" % name), h=h:
                                                f(a["eff"], *h, *tables(a), *listed), host, "list")
        out["mc_%s_decode" % name] = ("gf2_mc_%s_decode" % name, lambda c, o, a, m="mc_%s_decode" % name, h=h:
                                      getattr(c, m)(o, *h, *tables(a), *mc), {}, (fields,))
        out["mc_%s_decode_strata" % name] = ("gf2_mc_%s_decode_strata" % name, lambda c, o, a, m="mc_%s_decode_strata" % name, h=h:
                                             getattr(c, m)(o, *h, *tables(a), S["seed"], S["first_sample"], a["weights"], a["counts"], *kinds),
                                             {}, (20, fields))
        out["%s_enumerate" % name] = ("gf2_%s_enumerate" % name, lambda c, o, a, m="%s_enumerate" % name, h=h:
                                      getattr(c, m)(o, *h, *tables(a), *ranks), {}, (5, 5, fields))
        out["%s_gate_enumerate" % name] = ("gf2_%s_gate_enumerate" % name, lambda c, o, a, m="%s_gate_enumerate" % name, h=h:
                                           getattr(c, m)(o, *h, *tables(a), *sites(a), *gate_ranks), {}, (3, fields))
        out["mc_%s_decode_gate_strata" % name] = ("gf2_mc_%s_decode_gate_strata" % name,
                                                  lambda c, o, a, m="mc_%s_decode_gate_strata" % name, h=h:
                                                  getattr(c, m)(o, *h, *tables(a), *sites(a), S["seed"], S["first_sample"], a["strata"], a["counts"]),
                                                  dict(derived=("a", "b")), (20, 17, fields))
        out["mc_%s_decode_gate" % name] = ("gf2_mc_%s_decode_gate" % name, lambda c, o, a, m="mc_%s_decode_gate" % name, h=h:
                                           getattr(c, m)(o, *h, *tables(a), *sites(a), S["seed"], S["first_sample"], S["count"], S["p1"], S["p2"]),
                                           {}, (fields,))
        out["%s_enumerate_list" % name] = ("gf2_%s_enumerate_list" % name, lambda c, o, a, m="%s_enumerate_list" % name, h=h:
                                           getattr(c, m)(o, *h, *tables(a), *listed), {}, "list")
    out["mc_circuit_decode"] = ("gf2_mc_circuit_decode", lambda c, o, a: c.mc_circuit_decode(o, *tables(a), *mc), {}, (5,))
    out["mc_circuit_decode_strata"] = ("gf2_mc_circuit_decode_strata", lambda c, o, a: c.mc_circuit_decode_strata(
        o, *tables(a), S["seed"], S["first_sample"], a["weights"], a["counts"], *kinds), {}, (20, 5))
    out["circuit_enumerate"] = ("gf2_circuit_enumerate", lambda c, o, a: c.circuit_enumerate(o, *tables(a), *ranks), {}, (5, 5, 5))
    out["circuit_enumerate_host"] = ("gf2_circuit_enumerate_host", lambda c, o, a: _native.circuit_enumerate_host(a["eff"], *tables(a), *ranks),
                                     host, (5, 5, 5))
    out["stream_tally_host"] = ("gf2_stream_tally_host", lambda c, o, a: _native.stream_tally_host(
        a["words"], a["block_kind"], S["flag_words"], *tables(a), classes=True), dict(count=15, ldw=16, nblocks=18),
        ((_native.STREAM_FIELDS_COUNT,), (15,)))
    out["mc_stream_decode"] = ("gf2_mc_stream_decode", lambda c, o, a: c.mc_stream_decode(o, *tables(a), *mc), {}, (_native.STREAM_FIELDS_COUNT,))
    out["mc_retry_decode"] = ("gf2_mc_retry_decode", lambda c, o, a: c.mc_retry_decode(o, *tables(a), *mc, S["max_attempts"]), {},
                              (_native.RETRY_FIELDS_COUNT,))
    return out


CASES = cases()
OBJECT_PARAMETERS = ("circuit", "stream", "retry")


def run_case(monkeypatch, case, change=None):
    """Runs one case against a recorder and checks the one recorded call parameter by parameter.  change(arrays, want) alters the
    arrays passed and what is expected of them."""
    entry, call, extra, shape = CASES[case]
    extra = dict(extra)
    derived = extra.pop("derived", ())
    rec = Recorder()
    monkeypatch.setattr(_native, "lib", lambda: rec)
    ctx = _native.Context.__new__(_native.Context)
    ctx.handle = CTX_HANDLE
    obj = types.SimpleNamespace(handle=OBJECT_HANDLE)
    a = arrays()
    want = dict(S, ctx=CTX_HANDLE, entries1=len(a["keys1"]), entries2=len(a["keys2"]), nstrata=len(a["counts"]), **extra)
    want.update({name: a[name] for name in ("words", "eff", "keys1", "flips1", "keys2", "flips2", "site_loc", "weights", "counts", "block_kind")})
    want.update({name: OBJECT_HANDLE for name in OBJECT_PARAMETERS})
    if change is not None:
        change(a, want)
    contents = {"a": a["strata"][:, 0], "b": a["strata"][:, 1]}
    rec.peek = {param: (np.int32, len(a["strata"])) for param in derived}
    result = call(ctx, obj, a)

    assert len(rec.calls) == 1
    name, args, peeked = rec.calls[0]
    assert name == entry                                                      # the entry point of the wrapper's own name
    params = PARAMETERS[entry]
    assert len(args) == len(params) == len(_native.SIGNATURES[entry])
    for param, arg in zip(params, args):
        if param in derived:
            assert np.array_equal(peeked[param], contents[param]), param
        elif param.endswith("_out"):
            assert address(arg) != 0, param
        elif want[param] is None:
            assert address(arg) == 0, param
        elif isinstance(want[param], np.ndarray):
            assert address(arg) == want[param].ctypes.data, param
        else:
            assert not isinstance(scalar(arg), bool) and scalar(arg) == want[param], param
    outs = [address(arg) for param, arg in zip(params, args) if param.endswith("_out")]
    assert len(set(outs)) == len(outs)

    if shape == "list":                                                       # nothing found: no records, which a capacity of 31 holds
        assert result[0] == 0 and result[1].shape == (0, _native.FAULT_RECORD_WORDS)
    elif isinstance(shape[0], tuple):
        assert tuple(r.shape for r in result) == shape
    else:
        assert result.shape == shape and result.dtype == np.uint64 and not result.any()


def test_the_sentinels_are_all_different():
    assert sentinels_distinct()
    assert len(CASES) == 22 + 7
    assert all(entry in PARAMETERS and entry in _native.SIGNATURES for entry, _, _, _ in CASES.values())


@pytest.mark.parametrize("case", sorted(CASES))
def test_every_argument_reaches_its_parameter(monkeypatch, case):
    run_case(monkeypatch, case)


def empty_first_table(a, want):
    a["keys1"], a["flips1"] = np.zeros((0, 1), dtype="<u8"), np.zeros(0, dtype=np.uint8)
    want.update(keys1=None, flips1=None, entries1=0)


def empty_second_table(a, want):
    a["keys2"], a["flips2"] = np.zeros((0, 1), dtype="<u8"), np.zeros(0, dtype=np.uint8)
    want.update(keys2=None, flips2=None, entries2=0)


@pytest.mark.parametrize("change", [empty_first_table, empty_second_table])
@pytest.mark.parametrize("case", sorted(CASES))
def test_an_empty_table_is_a_null_table(monkeypatch, case, change):
    run_case(monkeypatch, case, change)


def test_circuit_decode_takes_tables_without_flips(monkeypatch):
    def no_flips(a, want):
        a["flips1"] = None
        want.update(flips1=None)
    run_case(monkeypatch, "mc_circuit_decode", no_flips)

    def neither_flips(a, want):
        a["flips1"] = a["flips2"] = None
        want.update(flips1=None, flips2=None)
    run_case(monkeypatch, "mc_circuit_decode", neither_flips)


def test_default_ldr_of_the_tally_is_ldw(monkeypatch):
    for name, head in (("ec", (S["rounds"],)), ("ft", (S["nsteps"], S["measure_mask"]))):
        rec = Recorder()
        monkeypatch.setattr(_native, "lib", lambda: rec)
        a = arrays()
        counts = getattr(_native, "%s_tally_host" % name)(a["words"], *head, S["r1"], a["keys1"], a["flips1"], S["r2"], a["keys2"], a["flips2"])
        (entry, args, _), = rec.calls
        got = dict(zip(PARAMETERS[entry], args))
        assert entry == "gf2_%s_tally_host" % name and got["ldw"] == got["ldr"] == 16 and got["class_out"] is None
        assert counts.shape == (getattr(_native, "%s_FIELDS_COUNT" % name.upper()),)

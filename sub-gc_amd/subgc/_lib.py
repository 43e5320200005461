"""ctypes binding of libsubgc_hip.so, generated from include/subgc_hip.h.

The header is the single source of truth: every `int subgc_*(...)` declaration in it is parsed
into a ctypes prototype, so a symbol that the header declares and the library does not export
fails at import time (tests/test_abi.py checks exactly that without a GPU).

There is NO CPU fallback: if the library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes
import os
import re

# torch bundles its own libamdhip64; it must be the HIP runtime of the process BEFORE
# libsubgc_hip.so is dlopen'ed, so that streams and device pointers are shared with torch.
import torch  # noqa: F401  (import order matters)

_HERE = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include")
# One surface per header: same library, same contract, an invoker that knows only its own declarations.  A new header is a row at the
# end of this table, a `call_x = _invoker("x")` line below, a path constant, and a pin of its exact name set in the feature's own CPU
# test; the table test (tests/test_headers_cpu.py) then covers it without an edit.
HEADERS = {"core": "subgc_hip.h", "metrics": "subgc_metrics_hip.h", "grounding": "subgc_grounding_hip.h",
           "controllability": "subgc_controllability_hip.h", "criterion": "subgc_criterion_hip.h", "selfcritical": "subgc_selfcritical_hip.h",
           "consensus": "subgc_consensus_hip.h", "forced": "subgc_forced_hip.h", "control_input": "subgc_control_input_hip.h",
           "beam_att": "subgc_beam_att_hip.h", "decode_b16": "subgc_decode_b16_hip.h", "gcn_agg": "subgc_gcn_agg_hip.h",
           "neighbours": "subgc_neighbours_hip.h", "decode_rules": "subgc_decode_rules_hip.h"}
HEADER = os.path.join(_INCLUDE, HEADERS["core"])
METRICS_HEADER = os.path.join(_INCLUDE, HEADERS["metrics"])
GROUNDING_HEADER = os.path.join(_INCLUDE, HEADERS["grounding"])
CONTROLLABILITY_HEADER = os.path.join(_INCLUDE, HEADERS["controllability"])
CRITERION_HEADER = os.path.join(_INCLUDE, HEADERS["criterion"])
SELFCRITICAL_HEADER = os.path.join(_INCLUDE, HEADERS["selfcritical"])
CONSENSUS_HEADER = os.path.join(_INCLUDE, HEADERS["consensus"])
FORCED_HEADER = os.path.join(_INCLUDE, HEADERS["forced"])
CONTROL_INPUT_HEADER = os.path.join(_INCLUDE, HEADERS["control_input"])
BEAM_ATT_HEADER = os.path.join(_INCLUDE, HEADERS["beam_att"])
DECODE_B16_HEADER = os.path.join(_INCLUDE, HEADERS["decode_b16"])
GCN_AGG_HEADER = os.path.join(_INCLUDE, HEADERS["gcn_agg"])
NEIGHBOURS_HEADER = os.path.join(_INCLUDE, HEADERS["neighbours"])
DECODE_RULES_HEADER = os.path.join(_INCLUDE, HEADERS["decode_rules"])
LIB_PATH = os.path.join(_HERE, "libsubgc_hip.so")

_SCALARS = {
    "int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "uint8_t": ctypes.c_uint8,
    "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
}


class SubgcError(RuntimeError):
    pass


def _code(path):
    """The header's text without its comments."""
    src = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


def _declared(decl):
    """-> (ctype, name) of one declaration, `type name` or `type* name`; pointers of any type become c_void_p."""
    decl = " ".join(decl.split())
    if "*" in decl:
        return ctypes.c_void_p, decl.split("*")[-1].strip()
    ty, nm = decl.rsplit(" ", 1)
    return _SCALARS[ty.replace("const ", "").strip()], nm


def parse_header(path=HEADER):
    """-> {name: (restype, [(ctype, argname), ...])} for every function the header declares."""
    out = {}
    for m in re.finditer(r"\b(int|const\s+char\s*\*)\s+(subgc_\w+)\s*\(([^;{}]*?)\)\s*;", _code(path), flags=re.S):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        protos = [_declared(a) for a in args.split(",")] if args and args != "void" else []
        out[name] = (ctypes.c_char_p if "char" in ret else ctypes.c_int, protos)
    return out


def parse_struct(name, path=HEADER):
    """ctypes.Structure mirror of `typedef struct <name> { ... } <name>;` in the header (one field per declaration): the header stays
    the single source of truth for the layout, like the prototypes."""
    m = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", _code(path), flags=re.S)
    if m is None:
        raise SubgcError(f"{name} is not declared in {os.path.basename(path)}")
    fields = [(nm, ty) for ty, nm in (_declared(decl) for decl in m.group(1).split(";") if decl.strip())]
    return type(name, (ctypes.Structure,), {"_fields_": fields})


_lib = None
PROTOS = {}         # key of HEADERS -> its parsed prototypes; filled once by lib()


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SubgcError(f"{LIB_PATH} is missing: run `python sub-gc_amd/build.py` (hipcc, gfx950). "
                             "There is no CPU fallback for the Sub-GC hot path.")
        L = ctypes.CDLL(LIB_PATH)
        for key, hdr in HEADERS.items():
            PROTOS[key] = parse_header(os.path.join(_INCLUDE, hdr))
            for name, (ret, args) in PROTOS[key].items():
                try:
                    fn = getattr(L, name)
                except AttributeError as e:
                    raise SubgcError(f"libsubgc_hip.so does not export {name} declared in {hdr}") from e
                fn.restype = ret
                fn.argtypes = [a for a, _ in args]
        if L.subgc_version() != 1:
            raise SubgcError("libsubgc_hip.so ABI version mismatch")
        _lib = L
    return _lib


def _invoker(key):
    """-> the invoker of one header of HEADERS: it calls an int-returning entry point by name and raises on a non-zero code.  A cache of
    bound entry points of its own (one attribute lookup on the CDLL per name instead of one per call), so that no invoker reaches
    another's declarations."""
    cache, hdr = {}, HEADERS[key]

    def invoke(name, *args):
        fn = cache.get(name)
        if fn is None:
            L = lib()
            if name not in PROTOS[key]:
                raise SubgcError(f"{name} is not declared in {hdr}")
            fn = cache[name] = getattr(L, name)
        rc = fn(*args)
        if rc != 0:
            raise SubgcError(f"{name} failed with code {rc}: {lib().subgc_last_error().decode()}")

    return invoke


call = _invoker("core")
call_metrics = _invoker("metrics")
call_grounding = _invoker("grounding")
call_controllability = _invoker("controllability")
call_criterion = _invoker("criterion")
call_selfcritical = _invoker("selfcritical")
call_consensus = _invoker("consensus")
call_forced = _invoker("forced")
call_control_input = _invoker("control_input")
call_beam_att = _invoker("beam_att")
call_decode_b16 = _invoker("decode_b16")
call_gcn_agg = _invoker("gcn_agg")
call_neighbours = _invoker("neighbours")
call_decode_rules = _invoker("decode_rules")

FAM = {"gemm": 1, "attn": 2, "lstm": 3, "gcn": 4, "pool": 5, "softmax": 6}


def prof_enable(family, on=True):
    call("subgc_prof_enable", FAM[family], int(on))


def prof_collect(family):
    n = ctypes.c_int64(0); ms = ctypes.c_double(0); work = ctypes.c_double(0)
    call("subgc_prof_collect", FAM[family], ctypes.byref(n), ctypes.byref(ms), ctypes.byref(work))
    return n.value, ms.value, work.value


def prof_last_moved(family):
    """Bytes the family's launches at the last prof_collect actually moved (LSTM cells: split-K planes, gate terms, saved gates included)."""
    b = ctypes.c_double(0)
    call("subgc_prof_last_moved", FAM[family], ctypes.byref(b))
    return b.value

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
HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "subgc_hip.h")
# the evaluation metrics are a surface of their own (subgc_accuracy_*): same library, same contract, their own header and invoker
METRICS_HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "subgc_metrics_hip.h")
# the grounding scores (subgc_grounding_*): the third header, again with an invoker that knows only its own declarations
GROUNDING_HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "subgc_grounding_hip.h")
# the set-controllability score (subgc_control_*): the fourth header, same arrangement
CONTROLLABILITY_HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "subgc_controllability_hip.h")
# the label-smoothed language loss (subgc_row_lse_sum_f32, subgc_smoothed_*): the fifth header, same arrangement
CRITERION_HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "subgc_criterion_hip.h")
# self-critical training (subgc_sc_*, subgc_reward_*): the sixth header, same arrangement
SELFCRITICAL_HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "subgc_selfcritical_hip.h")
# consensus re-ranking, method 'bleu' (subgc_consensus_bleu_*): the seventh header, same arrangement
CONSENSUS_HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "subgc_consensus_hip.h")
# forced decode and grounding on ground-truth sentences (subgc_forced_*, subgc_gt_grounding_*): the eighth header, same arrangement
FORCED_HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "subgc_forced_hip.h")
# the controllability experiment's input side (subgc_sct_*): the ninth header, same arrangement
CONTROL_INPUT_HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "subgc_control_input_hip.h")
# attention of the winning beams (subgc_beam_step_anc, subgc_beam_att_gather): the tenth header, same arrangement
BEAM_ATT_HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "subgc_beam_att_hip.h")
LIB_PATH = os.path.join(_HERE, "libsubgc_hip.so")

_SCALARS = {
    "int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "uint8_t": ctypes.c_uint8,
    "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
}


class SubgcError(RuntimeError):
    pass


def parse_header(path=HEADER):
    """-> {name: (restype, [(ctype, argname), ...])} for every function the header declares."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    out = {}
    for m in re.finditer(r"\b(int|const\s+char\s*\*)\s+(subgc_\w+)\s*\(([^;{}]*?)\)\s*;", src, flags=re.S):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        protos = []
        if args and args != "void":
            for a in args.split(","):
                a = " ".join(a.split())
                if "*" in a:
                    protos.append((ctypes.c_void_p, a.split("*")[-1].strip()))
                else:
                    ty, nm = a.rsplit(" ", 1)
                    protos.append((_SCALARS[ty.replace("const ", "").strip()], nm))
        out[name] = (ctypes.c_char_p if "char" in ret else ctypes.c_int, protos)
    return out


def parse_struct(name, path=HEADER):
    """ctypes.Structure mirror of `typedef struct <name> { ... } <name>;` in the header (one field per declaration; pointers of any
    type become c_void_p): the header stays the single source of truth for the layout, like the prototypes."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    m = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", src, flags=re.S)
    if m is None:
        raise SubgcError(f"{name} is not declared in subgc_hip.h")
    fields = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        if "*" in decl:
            fields.append((decl.split("*")[-1].strip(), ctypes.c_void_p))
        else:
            ty, nm = decl.rsplit(" ", 1)
            fields.append((nm, _SCALARS[ty.replace("const ", "").strip()]))
    return type(name, (ctypes.Structure,), {"_fields_": fields})


_lib = None
_protos = None


def lib():
    global _lib, _protos
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SubgcError(f"{LIB_PATH} is missing: run `python sub-gc_amd/build.py` (hipcc, gfx950). "
                             "There is no CPU fallback for the Sub-GC hot path.")
        L = ctypes.CDLL(LIB_PATH)
        _protos = parse_header()
        for hdr, protos in (("subgc_hip.h", _protos), ("subgc_metrics_hip.h", parse_header(METRICS_HEADER)),
                            ("subgc_grounding_hip.h", parse_header(GROUNDING_HEADER)),
                            ("subgc_controllability_hip.h", parse_header(CONTROLLABILITY_HEADER)),
                            ("subgc_criterion_hip.h", parse_header(CRITERION_HEADER)),
                            ("subgc_selfcritical_hip.h", parse_header(SELFCRITICAL_HEADER)),
                            ("subgc_consensus_hip.h", parse_header(CONSENSUS_HEADER)),
                            ("subgc_forced_hip.h", parse_header(FORCED_HEADER)),
                            ("subgc_control_input_hip.h", parse_header(CONTROL_INPUT_HEADER)),
                            ("subgc_beam_att_hip.h", parse_header(BEAM_ATT_HEADER))):
            for name, (ret, args) in protos.items():
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


_FN = {}          # bound entry points (one attribute lookup on the CDLL per name instead of one per call)


def call(name, *args):
    """Invoke an int-returning entry point and raise on a non-zero code."""
    fn = _FN.get(name)
    if fn is None:
        L = lib()
        if name not in _protos:
            raise SubgcError(f"{name} is not declared in subgc_hip.h")
        fn = _FN[name] = getattr(L, name)
    rc = fn(*args)
    if rc != 0:
        raise SubgcError(f"{name} failed with code {rc}: {lib().subgc_last_error().decode()}")


def _call_in(header, cache, name, args):
    """`call` for the entry points of one of the other headers: a cache per header, so that no invoker reaches another's declarations."""
    fn = cache.get(name)
    if fn is None:
        if name not in parse_header(header):
            raise SubgcError(f"{name} is not declared in {os.path.basename(header)}")
        fn = cache[name] = getattr(lib(), name)
    rc = fn(*args)
    if rc != 0:
        raise SubgcError(f"{name} failed with code {rc}: {lib().subgc_last_error().decode()}")


_FN_METRICS, _FN_GROUNDING, _FN_CONTROLLABILITY, _FN_CRITERION, _FN_SELFCRITICAL, _FN_CONSENSUS = {}, {}, {}, {}, {}, {}
_FN_FORCED, _FN_CONTROL_INPUT, _FN_BEAM_ATT = {}, {}, {}


def call_metrics(name, *args):
    """`call` for the entry points of subgc_metrics_hip.h."""
    _call_in(METRICS_HEADER, _FN_METRICS, name, args)


def call_grounding(name, *args):
    """`call` for the entry points of subgc_grounding_hip.h."""
    _call_in(GROUNDING_HEADER, _FN_GROUNDING, name, args)


def call_controllability(name, *args):
    """`call` for the entry points of subgc_controllability_hip.h."""
    _call_in(CONTROLLABILITY_HEADER, _FN_CONTROLLABILITY, name, args)


def call_criterion(name, *args):
    """`call` for the entry points of subgc_criterion_hip.h."""
    _call_in(CRITERION_HEADER, _FN_CRITERION, name, args)


def call_selfcritical(name, *args):
    """`call` for the entry points of subgc_selfcritical_hip.h."""
    _call_in(SELFCRITICAL_HEADER, _FN_SELFCRITICAL, name, args)


def call_consensus(name, *args):
    """`call` for the entry points of subgc_consensus_hip.h."""
    _call_in(CONSENSUS_HEADER, _FN_CONSENSUS, name, args)


def call_forced(name, *args):
    """`call` for the entry points of subgc_forced_hip.h."""
    _call_in(FORCED_HEADER, _FN_FORCED, name, args)


def call_control_input(name, *args):
    """`call` for the entry points of subgc_control_input_hip.h."""
    _call_in(CONTROL_INPUT_HEADER, _FN_CONTROL_INPUT, name, args)


def call_beam_att(name, *args):
    """`call` for the entry points of subgc_beam_att_hip.h."""
    _call_in(BEAM_ATT_HEADER, _FN_BEAM_ATT, name, args)


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

"""CPU checks that the Python side of the package and the C ABI still agree: every attribute the package reads from its own modules
exists, every entry point it calls by name is declared in include/subgc_hip.h, the profiling families match the header's, and the
host-side rejects of the decode-step entry points return SUBGC_EINVAL before any launch.  No GPU needed."""
import ast
import importlib
import os
import re

import pytest

from subgc import _lib

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sub-gc_amd", "subgc")
CHECKED = ("subgc.ops", "subgc.functions", "subgc._lib", "subgc.models.sampling")


def _sources():
    """-> (path, package of the module) for every module of the package."""
    for root, _, files in os.walk(PKG):
        for f in sorted(files):
            if f.endswith(".py"):
                pkg = os.path.relpath(root, os.path.dirname(PKG)).replace(os.sep, ".")
                yield os.path.join(root, f), pkg


def _resolve(modname, level, pkg):
    """Absolute name of `from <level dots><modname> import ...` in a module of package `pkg`."""
    if level == 0:
        return modname
    parts = pkg.split(".")
    base = parts[:len(parts) - (level - 1)]
    return ".".join(base + ([modname] if modname else []))


def _reads(path, pkg):
    """-> [(line, module, attribute)] for every attribute READ on a name bound to one of CHECKED, and for every name imported
    from one of them (`from .ops import _ptr`)."""
    tree = ast.parse(open(path).read(), path)
    alias = {}
    out = []
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            src = _resolve(node.module, node.level, pkg)
            for a in node.names:
                full = src + "." + a.name
                if full in CHECKED:
                    alias[a.asname or a.name] = full
                elif src in CHECKED:
                    out.append((node.lineno, src, a.name))
        elif isinstance(node, ast.Import):
            for a in node.names:
                if a.name in CHECKED and a.asname:
                    alias[a.asname] = a.name
    for node in ast.walk(tree):
        if isinstance(node, ast.Attribute) and isinstance(node.ctx, ast.Load) and isinstance(node.value, ast.Name) and node.value.id in alias:
            out.append((node.lineno, alias[node.value.id], node.attr))
    return out


def test_every_attribute_read_on_a_package_module_exists():
    """A wrapper removed from ops.py while a caller still uses it (functions.DecodeState once called a missing
    ops.gemm_skinny_wb16 on every bf16 decode step of <= 16 rows) fails here, not on the first decode that reaches it."""
    mods = {m: importlib.import_module(m) for m in CHECKED}
    seen, missing = 0, []
    for path, pkg in _sources():
        for line, mod, attr in _reads(path, pkg):
            seen += 1
            if not hasattr(mods[mod], attr):
                missing.append(f"{os.path.relpath(path, PKG)}:{line}: {mod}.{attr}")
    assert seen > 500
    assert not missing, "attributes read but not defined:\n" + "\n".join(missing)


def test_every_entry_point_called_by_name_is_declared():
    protos = _lib.parse_header()
    keyed = {"call_" + key: (hdr, _lib.parse_header(os.path.join(os.path.dirname(_lib.HEADER), hdr))) for key, hdr in _lib.HEADERS.items() if key != "core"}
    seen, missing, seen_keyed = 0, [], set()
    for path, _ in _sources():
        for node in ast.walk(ast.parse(open(path).read(), path)):
            if not isinstance(node, ast.Call) or not node.args:
                continue
            f = node.func
            name = f.id if isinstance(f, ast.Name) else (f.attr if isinstance(f, ast.Attribute) else None)
            a0 = node.args[0]
            if name == "call" and isinstance(a0, ast.Constant) and isinstance(a0.value, str):
                seen += 1
                if a0.value not in protos:
                    missing.append(f"{os.path.relpath(path, PKG)}:{node.lineno}: {a0.value}")
            # call_metrics("subgc_xxx", ...) ... call_neighbours("subgc_xxx", ...): the name must be declared in THAT invoker's header
            if name in keyed and isinstance(a0, ast.Constant) and isinstance(a0.value, str):
                seen_keyed.add((name, a0.value))
                if a0.value not in keyed[name][1]:
                    missing.append(f"{os.path.relpath(path, PKG)}:{node.lineno}: {a0.value} (not in {keyed[name][0]})")
            # lib().subgc_xxx(...) / _lib.lib().subgc_xxx(...): direct calls through the CDLL
            if isinstance(f, ast.Attribute) and f.attr.startswith("subgc_") and isinstance(f.value, ast.Call):
                seen += 1
                if f.attr not in protos:
                    missing.append(f"{os.path.relpath(path, PKG)}:{node.lineno}: {f.attr}")
    assert seen > 100
    assert {n for n, _ in seen_keyed} == set(keyed) and len(keyed) == len(_lib.HEADERS) - 1 >= 12      # every invoker is in use
    declared = {(inv, name) for inv, (_, p) in keyed.items() for name in p}
    # every other header's entry point is called by name through its invoker, but the host-side size query that Python never makes
    assert declared - seen_keyed == {("call_gcn_agg", "subgc_colsum_rows_workspace_bytes")}
    first = {"call_" + key for key in list(_lib.HEADERS)[1:13]}                    # the twelve pinned by test_headers_cpu.py: 37 of their 38
    assert len(first) == 12 and sum(inv in first for inv, _ in declared) == 38 and sum(inv in first for inv, _ in seen_keyed) == 37
    assert not missing, "entry points called but not declared in their invoker's header:\n" + "\n".join(missing)


def test_profiling_families_match_the_header():
    src = open(_lib.HEADER).read()
    fams = {int(v) for v in re.findall(r"#define\s+SUBGC_FAM_\w+\s+(\d+)", src)}
    assert fams == set(range(1, 7))
    bad = {k: v for k, v in _lib.FAM.items() if v not in fams}
    assert not bad, f"_lib.FAM names families the header does not define: {bad}"
    assert sorted(_lib.FAM.values()) == sorted(fams)


@pytest.mark.parametrize("M,K,what", [(0, 64, b"1 <= M <= 16"), (17, 64, b"1 <= M <= 16"), (4, 66, b"K % 4 == 0")])
def test_gemm_skinny_wb16_rejects_on_the_host(M, K, what):
    L = _lib.lib()
    fake = 1 << 20                                                 # never dereferenced: the shape check comes first
    rc = L.subgc_gemm_skinny_wb16(fake, 128, fake, 128, fake, 64, None, M, 64, K, 0, None)
    assert rc == -1
    err = L.subgc_last_error()
    assert b"gemm_skinny_wb16" in err and what in err, err


@pytest.mark.parametrize("S,R,what", [(33, 48, b"S <= 32"), (4, 50, b"R % 4 == 0")])
def test_lstm_step_skinny_rejects_on_the_host(S, R, what):
    L = _lib.lib()
    fake = 1 << 20
    rc = L.subgc_lstm_step_skinny(fake, 2 * R, fake, 2 * R, 2 * R, S, R, None, 0, None, 0, None, 0, None, None, None, fake, fake, R,
                                  None, 0, None, 0, 1, None)
    assert rc == -1
    err = L.subgc_last_error()
    assert b"lstm_step_skinny" in err and what in err, err

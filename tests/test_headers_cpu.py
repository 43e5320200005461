"""The public headers as one table (`_lib.HEADERS`), without a GPU: how many entry points each declares, that no name is declared twice,
that the built library exports every one, and that each invoker -- `call` for the core header, `call_<key>` for the others -- refuses the
names of every other header before anything reaches the library.  The first thirteen rows and their counts are pinned; every structural
check runs over whatever the table holds, so a header appended later is covered without an edit here.  What is specific to one header
(its exact names, argument names and ctypes, the citations in its text) stays in that feature's own test file."""
import os

import pytest

from subgc import _lib
from subgc._lib import SubgcError

COUNTS = {"core": 133, "metrics": 2, "grounding": 2, "controllability": 1, "criterion": 4, "selfcritical": 7, "consensus": 2, "forced": 4,
          "control_input": 3, "beam_att": 2, "decode_b16": 2, "gcn_agg": 7, "neighbours": 2}
KEYS = list(_lib.HEADERS)


@pytest.fixture(scope="module")
def protos():
    return {key: _lib.parse_header(os.path.join(os.path.dirname(_lib.HEADER), hdr)) for key, hdr in _lib.HEADERS.items()}


def _invoker(key):
    return _lib.call if key == "core" else getattr(_lib, "call_" + key)


def test_the_table_starts_with_the_thirteen_headers_in_order():
    assert KEYS[:13] == list(COUNTS) and len(COUNTS) == 13 and sum(COUNTS.values()) == 171
    assert _lib.HEADERS["core"] == "subgc_hip.h" and all(_lib.HEADERS[k] == f"subgc_{k}_hip.h" for k in KEYS[1:])
    for key in KEYS:                                                     # the path constants the per-feature tests read
        const = "HEADER" if key == "core" else key.upper() + "_HEADER"
        assert os.path.basename(getattr(_lib, const)) == _lib.HEADERS[key] and os.path.isfile(getattr(_lib, const))
        assert callable(_invoker(key))
    for gone in ("EXTRA_HEADERS", "LATER_HEADERS", "NEWER_HEADERS"):      # one table: the side tables are not coming back
        assert not hasattr(_lib, gone), gone


@pytest.mark.parametrize("key", KEYS)
def test_declared_entry_points_are_counted_and_exported(protos, key):
    assert protos[key]
    if key in COUNTS:                                                     # a header appended later pins its names in its own test
        assert len(protos[key]) == COUNTS[key]
    L = _lib.lib()
    for name in protos[key]:
        assert hasattr(L, name), name
    assert L.subgc_version() == 1 and _lib.PROTOS[key] == protos[key]     # lib() parsed this header once and kept it


def test_no_name_is_declared_in_two_headers(protos):
    every = [set(p) for p in protos.values()]
    assert sum(len(p) for p in every) == len(set().union(*every))
    assert sum(len(protos[k]) for k in COUNTS) == 171
    assert set(_lib.PROTOS) == set(KEYS)


def test_every_invoker_refuses_the_names_of_every_other_header(protos, monkeypatch):
    """All n (n - 1) ordered pairs, 156 for the thirteen headers: each invoker against one name of each of the other headers; the message
    names the invoker's own header file, and the library is not reached (once loaded, the handle is swapped for one that fails on any
    attribute read)."""
    _lib.lib()

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"the refusal of a foreign name reached the library ({name})")

    monkeypatch.setattr(_lib, "_lib", Untouchable())
    pairs = [(key, other) for key in KEYS for other in KEYS if other != key]
    assert len(pairs) == len(KEYS) * (len(KEYS) - 1) and (len(KEYS) != 13 or len(pairs) == 156)
    for key, other in pairs:
        inv, hdr, name = _invoker(key), _lib.HEADERS[key], sorted(protos[other])[0]
        with pytest.raises(SubgcError, match=f"^{name} is not declared in {hdr}$"):
            inv(name)
        with pytest.raises(SubgcError, match=f"^{name} is not declared in {hdr}$"):
            inv(name, 0, None)

"""The aggregation-first entry points without a GPU: their header (include/subgc_gcn_agg_hip.h, a row of `_lib.HEADERS`; what holds for
every row, the invokers' refusals included, is in test_headers_cpu.py), the exported symbols, the host-side refusals and the host-side
choice."""
import ctypes
import os

from subgc import _lib, ops
import subgc.functions as F_

NAMES = {"subgc_gcn_agg_fwd", "subgc_gcn_agg_bwd", "subgc_gcn_agg_relu_bwd", "subgc_gemm_f32_rowbias", "subgc_gemm_f32_pair_rowbias",
         "subgc_colsum_rows_f32", "subgc_colsum_rows_workspace_bytes"}


def test_the_header_declares_exactly_the_seven_entry_points():
    assert os.path.basename(_lib.GCN_AGG_HEADER) == "subgc_gcn_agg_hip.h" and os.path.isfile(_lib.GCN_AGG_HEADER)
    protos = _lib.parse_header(_lib.GCN_AGG_HEADER)
    assert set(protos) == NAMES
    L = _lib.lib()
    assert _lib.PROTOS["gcn_agg"] == protos and all(hasattr(L, n) for n in NAMES)
    every = [set(_lib.parse_header(os.path.join(os.path.dirname(_lib.HEADER), h))) for k, h in _lib.HEADERS.items() if k != "gcn_agg"]
    assert len(every) == len(_lib.HEADERS) - 1 >= 12 and not NAMES & set().union(*every)      # declared nowhere else


def test_host_side_refusals_need_no_gpu():
    L = _lib.lib()
    assert L.subgc_gcn_agg_fwd(16, 16, 16, 16, 16, 16, 16, 1, 4, 8, 6, None) == -1 and b"multiple of 4" in L.subgc_last_error()
    assert L.subgc_gcn_agg_fwd(16, 16, 16, 16, 16, None, 16, 1, 4, 8, 8, None) == -1 and b"null pointer" in L.subgc_last_error()
    assert L.subgc_gcn_agg_fwd(20, 16, 16, 16, 16, 16, 16, 1, 4, 8, 8, None) == -1 and b"16-byte aligned" in L.subgc_last_error()
    assert L.subgc_gcn_agg_bwd(16, 16, 16, 16, 16, 0, 1, 4, 8, 10, None) == -1 and b"multiple of 4" in L.subgc_last_error()
    assert L.subgc_gcn_agg_bwd(16, 16, 16, 16, 24, 0, 1, 4, 8, 8, None) == -1 and b"16-byte aligned" in L.subgc_last_error()
    assert L.subgc_gcn_agg_fwd(None, None, None, None, None, None, None, 0, 4, 8, 8, None) == 0            # no image: nothing to do
    assert L.subgc_gcn_agg_relu_bwd(16, 16, None, 16, 16, 4, None) == -1 and b"null pointer" in L.subgc_last_error()
    assert L.subgc_gemm_f32_rowbias(0, 1, 4, 4, 4, 16, 4, 16, 4, 16, 4, None, 16, 0, None, 0, None) == -1 and b"without a bias" in L.subgc_last_error()
    assert L.subgc_gemm_f32_rowbias(1, 1, 4, 4, 4, 16, 4, 16, 4, 16, 4, None, None, 0, None, 0, None) == -1 and b"transA && transB" in L.subgc_last_error()
    rc = L.subgc_gemm_f32_pair_rowbias(0, 1, 4, 4, 4, 16, 16, 4, 16, 16, 4, 16, 16, 4, 16, 16, 16, None, 0, None, 0, None)
    assert rc == -1 and b"both biases or for none" in L.subgc_last_error()
    need = ctypes.c_size_t(0)
    assert L.subgc_colsum_rows_workspace_bytes(4736, 1024, 2, ctypes.byref(need)) == 0 and need.value == 2 * 64 * 1024 * 4    # 74 rows per slab
    assert L.subgc_colsum_rows_workspace_bytes(0, 64, 1, ctypes.byref(need)) == 0 and need.value == 64 * 4
    assert L.subgc_colsum_rows_f32(1, 16, None, 64, 70, 64, None, None, 16, None, 0, 16, 64, None) == -1 and b"bytes of workspace" in L.subgc_last_error()
    assert L.subgc_colsum_rows_f32(3, 16, None, 64, 70, 64, None, None, 16, None, 0, None, 0, None) == -1 and b"bad sizes" in L.subgc_last_error()


def test_the_choice_is_made_from_the_row_counts_the_layer_and_the_switch():
    ok = F_.gcn_aggregate_first_ok
    assert ops.GCN_AGGREGATE_FIRST is True
    assert ok(False, False, 128, 37, 65, 1024) and ok(False, False, 10, 101, 301, 1024)
    assert not ok(True, False, 128, 37, 65, 1024)                            # BatchNorm between fc_rgt and the aggregation: Full_GC_Kar
    assert not ok(False, True, 128, 37, 65, 1024)                            # bf16 storage keeps the old order
    assert not ok(False, False, 128, 65, 65, 1024) and not ok(False, False, 128, 37, 65, 1022)
    ops.GCN_AGGREGATE_FIRST = False
    try:
        assert not ok(False, False, 128, 37, 65, 1024)
    finally:
        ops.GCN_AGGREGATE_FIRST = True

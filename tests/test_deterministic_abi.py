"""CPU checks of the deterministic-mode switch (subgc_deterministic) and of the `_ws` siblings of the entry points that add with float
atomics: declared, bound, off by default, process-wide, restored by the context manager.  No GPU needed."""
import argparse

from subgc import _lib, ops
import subgc.models as models

SIBLINGS = ("subgc_embed_bwd_ws", "subgc_scatter_add_rows_ws", "subgc_sumsq_f32_ws", "subgc_subgraph_pool_bwd_ws", "subgc_gpn_score_bwd_ws")


def test_header_declares_and_lib_binds_the_mode_and_siblings():
    protos = _lib.parse_header()
    L = _lib.lib()
    for name in ("subgc_deterministic",) + SIBLINGS:
        assert name in protos, name
        assert hasattr(L, name), name
    for name in SIBLINGS:                      # each sibling = its original's arguments, then workspace, ws_bytes, stream
        args = [a for _, a in protos[name][1]]
        assert args[-3:] == ["workspace", "ws_bytes", "stream"], (name, args)
        orig = [a for _, a in protos[name[:-3]][1]]
        assert args[:len(orig) - 1] == orig[:-1], (name, args, orig)


def test_mode_off_by_default_and_returns_previous():
    L = _lib.lib()
    assert L.subgc_deterministic(0) == 0                 # off by default (no test before this one leaves it on)
    assert L.subgc_deterministic(1) == 0
    assert L.subgc_deterministic(7) == 1                 # any non-zero value is "on"
    assert L.subgc_deterministic(0) == 1
    assert L.subgc_deterministic(0) == 0


def test_context_manager_restores_previous():
    L = _lib.lib()
    with ops.deterministic():
        assert L.subgc_deterministic(1) == 1
        with ops.deterministic(False):
            assert L.subgc_deterministic(0) == 0
        assert L.subgc_deterministic(1) == 1
    assert L.subgc_deterministic(0) == 0
    L.subgc_deterministic(1)
    try:
        with ops.deterministic(False):
            assert L.subgc_deterministic(0) == 0
        assert L.subgc_deterministic(1) == 1             # restored to ON
    finally:
        L.subgc_deterministic(0)
    assert ops.set_deterministic(True) is False
    assert ops.set_deterministic(False) is True


def test_originals_refuse_in_mode_and_name_their_sibling():
    L = _lib.lib()
    with ops.deterministic():
        assert L.subgc_sumsq_f32(None, 16, None, None) == -1
        assert b"subgc_sumsq_f32_ws" in L.subgc_last_error()
        assert L.subgc_embed_bwd(None, None, 1, None, 1.0, None, None, 4, 8, 10, None) == -1
        assert b"subgc_embed_bwd_ws" in L.subgc_last_error()
        assert L.subgc_scatter_add_rows(None, 8, None, None, 8, 4, 8, None, None) == -1
        assert b"subgc_scatter_add_rows_ws" in L.subgc_last_error()
    # mode off: the sibling is the original (same host-side checks, the workspace is not looked at)
    assert L.subgc_sumsq_f32_ws(None, 16, None, None, 0, None) == -1
    assert b"null pointer" in L.subgc_last_error()


def test_workspace_too_small_reports_bytes_needed():
    L = _lib.lib()
    with ops.deterministic():
        # host-side plan check before any launch: non-null fake pointers are never dereferenced on this path
        fake = 1 << 20
        assert L.subgc_sumsq_f32_ws(fake, 1 << 20, fake, None, 0, None) == -1
        assert b"needs 2048 bytes" in L.subgc_last_error()
        assert L.subgc_embed_bwd_ws(fake, fake, 1, None, 1.0, fake, fake, 100, 64, 50, fake, 16, None) == -1
        assert b"needs" in L.subgc_last_error() and b"bytes" in L.subgc_last_error()


def test_setup_option_switches_the_mode_on():
    L = _lib.lib()
    opt = dict(caption_model="topdown", vocab_size=50, input_encoding_size=32, rnn_size=32, num_layers=1, drop_prob_lm=0.0, max_length=16,
               seq_length=16, fc_feat_size=16, att_feat_size=16, att_hid_size=16, use_bn=0, sampling_prob=0.0, use_gpn=0)
    try:
        models.setup(argparse.Namespace(**opt))
        assert L.subgc_deterministic(0) == 0             # missing option: off, as before
        models.setup(argparse.Namespace(**opt, deterministic=0))
        assert L.subgc_deterministic(0) == 0
        models.setup(argparse.Namespace(**opt, deterministic=1))
        assert L.subgc_deterministic(0) == 1
    finally:
        L.subgc_deterministic(0)

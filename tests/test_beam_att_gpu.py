"""Attention of the winning beams on the device (include/subgc_beam_att_hip.h): the ancestry step against `subgc_beam_step` (common
outputs bit for bit) and the host bookkeeping (`beam._beam_step`), the gather against numpy, the closed-form hash-chain property through
`DeviceSearch` (beam_att_fake), the model against the fixture the reference wrote (tests/golden/make_golden_beam_att.py) and against a
forced decode along the winners, and `caption_images` with beam search, grounding and consensus in one pass.

Tolerances: attention rows 1e-4 (the project's tolerance for tapped alpha); arg-max nodes are compared on every word whose reference
top-2 gap is at least 1e-3 (ten times that), and at most 5 % of a configuration's words may fall below it."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

import beam_att_fake as FK
from subgc import beam, forced, ops, synthetic
from subgc.beam import _F32
from test_parity_gpu import DEV, build

pytestmark = pytest.mark.gpu

ATOL, GAP, CAP = 1e-4, 1e-3, 0.05
N_SUB, T, N, LENS = 3, 6, 5, (5, 2, 4)
CONFIGS = [(1, 1), (3, 1), (2, 2), (4, 2)]                                       # (beam, groups)
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(HERE, "golden", "beam_att_meta.json")) as f:
        meta = json.load(f)
    with np.load(os.path.join(HERE, "golden", "beam_att_case.npz")) as z:
        return meta, {k: z[k] for k in z.files}


# ------------------------------------------------------------------------------------------------ 1. kernels
@pytest.mark.parametrize("constraint", [0, 1])
@pytest.mark.parametrize("beam_size,G", CONFIGS)
def test_ancestry_step_and_gather_against_the_plain_step_and_the_host(beam_size, G, constraint):
    bd, V1, lam = beam_size // G, FK.V1, float(_F32(0.5))
    kk, rows, unk = min(V1, beam_size + 2), N_SUB * beam_size, V1 - 1
    rng = np.random.default_rng(100 * beam_size + 10 * G + constraint)
    plain, anc = beam.DeviceTables(N_SUB, G, T, bd, DEV), beam.DeviceTables(N_SUB, G, T, bd, DEV, return_att=True)
    z = lambda dt: ops.zero_(torch.empty(rows, device=DEV, dtype=dt))
    tok_p, src_p, tok_a, src_a = z(torch.long), z(torch.int32), z(torch.long), z(torch.int32)
    groups = [[beam._Group(T, bd) for _ in range(G)] for _ in range(N_SUB)]
    done = [[[] for _ in range(G)] for _ in range(N_SUB)]
    for t in range(T + G - 1):
        # leading log-probs with TIES (multiples of 1/2, descending) over distinct word ids; the end token is among them half the time
        tv = -np.sort(rng.integers(0, 5, (rows, kk)), 1).astype(np.float32) / 2
        ti = np.stack([rng.permutation(V1)[:kk] for _ in range(rows)]).astype(np.int32)
        d_tv, d_ti = torch.from_numpy(tv).to(DEV), torch.from_numpy(ti).to(DEV)
        ops.beam_step(d_tv, d_ti, plain, tok_p, src_p, t, T, G, bd, kk, unk, constraint, lam)
        ops.beam_step_anc(d_tv, d_ti, anc, tok_a, src_a, t, T, G, bd, kk, unk, constraint, lam)
        for a, b in ((plain.seq, anc.seq), (plain.lps, anc.lps), (plain.sums, anc.sums), (plain.done_all, anc.done_all), (tok_p, tok_a), (src_p, src_a)):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), t
        h_anc = anc.anc.cpu().numpy()
        tv4, ti4 = tv.reshape(N_SUB, G, bd, kk), ti.reshape(N_SUB, G, bd, kk)
        for g in range(G):
            if not g <= t <= T + g - 1:
                continue
            tau = t - g
            for s in range(N_SUB):
                grp = groups[s][g]
                beam._beam_step(grp, tv4[s, g], ti4[s, g], tau, bd, unk, constraint, groups[s][:g], _F32(lam))
                np.testing.assert_array_equal(h_anc[s, g, :tau + 1], grp.anc[:tau + 1], err_msg=f"t {t} group {g} sub-graph {s}")
                for vix in range(bd):
                    if grp.seq[tau, vix] == 0 or t == T + g - 1:
                        done[s][g].append((grp.anc[:tau + 1, vix].copy(), tau + 1))
                        grp.sums[vix] = -1000
    cnt = anc.done_cnt.cpu().numpy()
    h_done, h_len = anc.done_anc.cpu().numpy(), anc.done_len.cpu().numpy()
    for s in range(N_SUB):
        for g in range(G):
            assert cnt[s, g] == len(done[s][g]) >= bd
            for j, (col, L) in enumerate(done[s][g]):
                assert h_len[s, g, j] == L
                np.testing.assert_array_equal(h_done[s, g, j, :L], col)
                assert not h_done[s, g, j, L:].any()
    # the gather: random step rows, several valid picks per sub-graph, against the numpy restatement
    al = rng.random((T + G - 1, rows, N)).astype(np.float32)
    d_al = torch.from_numpy(al).to(DEV)
    for trial in range(4):
        pick = np.array([[g_, rng.integers(0, cnt[s, g_])] for s in range(N_SUB) for g_ in [int(rng.integers(0, G))]], np.int32)
        pick = beam.check_picks(pick, cnt)
        want = np.zeros((T + 1, N_SUB, N), np.float32)
        for s, (g_, j) in enumerate(pick):
            col, L = done[s][g_][j]
            base = (s * G + g_) * bd
            want[0, s] = al[0, base]
            for w in range(1, L):
                want[w, s] = al[w + g_, base + col[w - 1]]
        out = torch.full((T + 1, N_SUB, N), float("nan"), device=DEV)
        ops.beam_att_gather(d_al, anc, torch.from_numpy(pick.ravel().copy()).to(DEV), N_SUB, G, bd, T, out)
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32), err_msg=f"trial {trial}")


# ------------------------------------------------------------------------------------------------ 2. the hash chain through DeviceSearch
@pytest.mark.parametrize("constraint", [0, 1])
@pytest.mark.parametrize("beam_size,G", CONFIGS)
def test_device_search_attention_is_the_code_of_the_beams_own_token_chain(beam_size, G, constraint):
    salt, bd = 3, beam_size // G
    opt = dict(beam_size=beam_size, group_size=G, diversity_lambda=0.5, decoding_constraint=constraint)
    eng = FK.DeviceEngine(N_SUB, beam_size, LENS, N, salt, DEV)
    ds = beam.DeviceSearch(eng, T, opt, return_att=True)
    ds.loop(fresh_tables=True)
    lengths = set()
    for rnd in range(2):                                                         # the second search re-uses tables, ancestry and step buffers
        if rnd:
            eng.st.reset()
            ds.loop()
        for g in range(G):
            for r in range(bd):                                                  # every kept beam, not only the winner
                seq, seqlp, done, att = ds.collect((g, r))
                AL = att["AL"].cpu().numpy()
                assert AL.shape == (T + 1, N_SUB, N)
                for s in range(N_SUB):
                    words = done[s][g * bd + r]["seq"].tolist()
                    L = words.index(0) + 1 if 0 in words else T
                    assert att["len"][s] == L
                    FK.check_beam(words, AL[:L, s], L, s, salt, LENS[s], N)
                    assert not AL[L:, s].any()
                    lengths.add(L)
                    if (g, r) == (0, 0):
                        assert words == seq[s].tolist()
    assert len(lengths) > 1
    off = beam.DeviceSearch(FK.DeviceEngine(N_SUB, beam_size, LENS, N, salt, DEV), T, opt)
    off.loop(fresh_tables=True)
    plain = off.collect()
    assert len(plain) == 3 and plain[0].equal(seq) and plain[1].equal(seqlp)
    with pytest.raises(ops.SubgcError, match="kept beam"):
        ds.collect((G, 0))


# ------------------------------------------------------------------------------------------------ 3. - 5. the model
def _case(golden, fixture, name):
    meta, arr = fixture
    c = meta["cases"][name]
    g = golden(c["inputs"])
    m = build(g, golden(c["weights"]).group("weights"), False)
    b = {k: v.to(DEV) for k, v in g.tensors("inputs").items()}
    return m, b, dict(c["sample_opt"]), {k[len(name) + 1:]: v for k, v in arr.items() if k.startswith(name + "_")}, c


def _sample(m, b, opt):
    ret = m(*synthetic.sample_args({k: v.clone() for k, v in b.items()}), opt=opt, mode="sample")
    return ret, m.done_beams


def _same_search(a, da, b, db):
    assert torch.equal(a[0].cpu(), b[0].cpu()) and torch.equal(a[1].cpu().view(torch.int32), b[1].cpu().view(torch.int32))
    assert torch.equal(a[3].cpu(), b[3].cpu()) and len(da) == len(db)
    for x, y in zip(da, db):
        assert len(x) == len(y)
        for p, q in zip(x, y):
            assert torch.equal(p["seq"], q["seq"]) and torch.equal(p["logps"].view(torch.int32), q["logps"].view(torch.int32))
            assert p["p"] == q["p"] and p["unaug_p"] == q["unaug_p"]


def _check_against(att, want, lens, gap, n_max, tag):
    """att [rows, steps, n_max] of the device against the reference rows [rows, T, N]: 1e-4 on every row, zero behind the length, the
    arg-max on every word the gap rule keeps."""
    steps = int(lens.max())
    assert att.shape == (len(lens), steps, n_max), (tag, att.shape)
    assert not want[:, :, n_max:].any()
    live = np.arange(steps)[None, :] < lens[:, None]
    err = np.abs(att - want[:, :steps, :n_max])
    print(tag, "max attention error", float(err.max()), "words", int(live.sum()))
    assert float(err.max()) <= ATOL
    assert not att[~live].any()                                                  # zero from the length on
    keep = live & (gap[:, :steps] >= GAP)
    skipped = 1.0 - keep.sum() / live.sum()
    print(tag, "share of words below the gap", skipped)
    assert skipped <= CAP
    np.testing.assert_array_equal(att.argmax(2)[keep], want[:, :steps, :n_max].argmax(2)[keep], err_msg=tag)


@pytest.mark.parametrize("name", ["sgpn_beam2", "fullgc_beam3", "div_beam4"])
def test_model_against_the_reference_fixture_forced_decode_and_the_eager_path(golden, fixture, name):
    m, b, opt, ref, c = _case(golden, fixture, name)
    on = dict(opt, return_att=1)
    plain, d_plain = _sample(m, b, opt)
    got, d_got = _sample(m, b, on)                                               # one image: the hipGraph path (capture)
    again, d_again = _sample(m, b, on)                                           # ... and a replay
    assert len(plain) == 4 and len(got) == 5 and any(k[0] == "beam" for k in m._graph_cache)
    _same_search(plain, d_plain, got, d_got)                                     # 5. the search does not change
    _same_search(got, d_got, again, d_again)
    assert torch.equal(got[4].view(torch.int32), again[4].view(torch.int32))     # the replay gives the same bits
    np.testing.assert_array_equal(got[0].cpu().numpy(), ref["tokens"])           # 3. tokens identical
    lens, att = ref["len"], got[4].cpu().numpy()
    n_max = att.shape[2]
    _check_against(att, ref["att"], lens, ref["gap"], n_max, name + " graph")
    # the eager batched path (two images: no graph): same search, attention at the fast-path tolerance
    b2 = {k: v.clone() for k, v in b.items()}
    hold = {}
    rs = m.sample_images([b, b2], opt=on, batch_out=hold)
    rs_off = m.sample_images([b, b2], opt=opt)
    for r, r_off in zip(rs, rs_off):
        assert len(r) == 5 and len(r_off) == 4
        assert torch.equal(r[0], r_off[0]) and torch.equal(r[1].view(torch.int32), r_off[1].view(torch.int32))
        torch.testing.assert_close(r[4].cpu(), got[4].cpu(), atol=1e-4, rtol=1e-4)
        _check_against(r[4].cpu().numpy(), ref["att"], lens, ref["gap"], n_max, name + " eager")
    rows = len(lens)
    assert hold["AL"].shape == (m.seq_length + 1, 2 * rows, hold["idx"].size(1)) and hold["seq"].is_cuda and hold["bounds"] == [0, rows, 2 * rows]
    assert not hold["AL"][m.seq_length].any()                                    # beam search has no T + 1-th entry
    # 4. a forced decode along the winners: candidate keep[j] of the image follows row j's tokens
    keep = got[3].cpu().numpy().astype(np.int64)
    C = int(b["gpn_obj_ind"].size(1) * b["gpn_obj_ind"].size(2)) if m.gpn else 1
    tok = np.zeros((C if m.gpn else rows, m.seq_length), np.int64)
    where = keep if m.gpn else np.arange(rows)
    tok[where] = got[0].cpu().numpy()
    f = forced.forced_decode(m, [b], [tok], return_att=True)
    fa = f["AL"].cpu().numpy()[:, where].transpose(1, 0, 2)                      # [rows, Tf, N]
    steps = int(lens.max())
    live = np.arange(steps)[None, :] < lens[:, None]
    err = np.abs(fa[:, :steps, :n_max] - att)[live]
    print(name, "beam attention against forced decode", float(err.max()))
    assert float(err.max()) <= ATOL


def test_eager_one_image_search_and_the_graph_cache_key(golden, fixture):
    m, b, opt, ref, c = _case(golden, fixture, "sgpn_beam2")
    on = dict(opt, return_att=1)
    _sample(m, b, opt)
    g_ret, _ = _sample(m, b, on)
    keys = [k for k in m._graph_cache if k[0] == "beam"]
    assert len(keys) == 2 and {dict(k[3])["return_att"] for k in keys} == {False, True}
    m.decode_hipgraph = False
    m.__dict__.pop("_graph_cache")
    e_ret, _ = _sample(m, b, on)
    assert torch.equal(g_ret[0].cpu(), e_ret[0].cpu())
    torch.testing.assert_close(g_ret[4].cpu(), e_ret[4].cpu(), atol=1e-4, rtol=1e-4)


def test_host_search_backtracks_the_same_rows_as_the_device_gather(golden, fixture):
    """`beam.search(return_att=True)` (host bookkeeping, every kept beam) against the device path on the same engine kind: the winners'
    buffer within the fast-path tolerance, and every kept beam's rows = the device gather of that beam."""
    from subgc import functions as F_
    from test_beam_device_gpu import prepared
    m, b, opt, ref, c = _case(golden, fixture, "div_beam4")
    pr, P, N = prepared(m, [b])
    T = m.seq_length
    with torch.no_grad():
        host = beam.beam_decode(pr, P, N, T, dict(opt), xt_table=m.xt_gates_table(), on_device=False, return_att=True)
        eng = beam._BatchEngine(pr, P, N, opt["beam_size"], m.xt_gates_table(), return_att=True)
        ds = beam.DeviceSearch(eng, T, opt, return_att=True)
        ds.loop(fresh_tables=True)
        dev = ds.collect()
        assert torch.equal(dev[0], host[0]) and np.array_equal(dev[3]["len"], host[3]["len"])
        np.testing.assert_allclose(dev[3]["AL"].cpu().numpy(), host[3]["AL"], atol=1e-4, rtol=1e-4)
        G, bd = opt["group_size"], opt["beam_size"] // opt["group_size"]
        for g in range(G):
            for r in range(bd):
                AL = ds.collect((g, r))[3]["AL"].cpu().numpy()
                for s in range(pr.S):
                    hb = host[2][s][g * bd + r]
                    assert torch.equal(hb["seq"], dev[2][s][g * bd + r]["seq"])
                    np.testing.assert_allclose(AL[:hb["len"], s], hb["att"], atol=1e-4, rtol=1e-4)
                    assert not AL[hb["len"]:, s].any()


# ------------------------------------------------------------------------------------------------ 6. the glue
@pytest.mark.parametrize("name", ["subgc", "fullgc"])
def test_caption_images_grounds_the_beam_caption_in_the_decode_pass(golden, name):
    import grounding_golden as G
    import subgc.models as models
    from subgc import consensus, eval_glue, grounding
    from test_grounding_score_gpu import _grd_case
    fmeta, arr = G.load()
    out, meta, opt, w, det_wd = _grd_case(golden, name)
    opt.caption_model = "topdown"
    m = models.setup(opt)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    m = m.to(DEV).eval()
    imgs = meta["cases"][name]
    dev = [{k: v.to(DEV) for k, v in synthetic.make_test_batch(i["M"], D=opt.att_feat_size, seed=i["seed"], fc_size=opt.att_feat_size,
                                                                node_pool=i["pool"]).items()} for i in imgs]
    infos = [{"id": i["id"]} for i in imgs]
    vocab = meta["vocab"]
    refs = G.references(fmeta, arr, f"grd_{name}_0", device=DEV)
    sc = grounding.GroundingScorer(refs)
    arg = {"scorer": sc, "index": {i["id"]: refs.index[str(i["id"])] for i in imgs}, "boxes": {i["id"]: out[f"{name}_{i['id']}_boxes"] for i in imgs},
           "img_wh": {i["id"]: i["wh"] for i in imgs}}
    rng = np.random.default_rng(5)
    words = sorted(vocab.values())
    sents = [[[words[int(x)] for x in rng.integers(0, len(words), int(rng.integers(1, 12)))] for _ in range(3)] for _ in range(30)]
    rr = consensus.ConsensusReranker(consensus.ConsensusCorpus(sents, vocab, device=DEV), k=6, m=10)
    cons = {"reranker": rr, "nn": {info["id"]: [int(x) for x in rng.choice(30, 8, replace=False)] for info in infos}, "top_k": None}
    kw = dict(sample_max=1, beam_size=2, return_att=1)
    preds = eval_glue.caption_images(m, dev, infos, vocab, kw, grounding=arg, consensus=cons)
    off = eval_glue.caption_images(m, dev, infos, vocab, dict(kw, return_att=0), consensus=cons)
    one = eval_glue.caption_images(m, dev, infos, vocab, kw, group=1, grounding=arg, consensus=cons)      # one image per batch: the graphed path
    two = eval_glue.caption_images(m, dev, infos, vocab, kw, group=1, grounding=arg, consensus=cons)      # ... replayed
    assert any(k[0] == "beam" for k in m._graph_cache)
    for p, p_off, p1, p2, img, b in zip(preds, off, one, two, imgs, dev):
        assert "grounding" in p and "grounding_score" in p and "grounding" not in p_off
        assert p["caption"] == p_off["caption"] == p1["caption"] and np.array_equal(p["consensus_rerank_ind"], p_off["consensus_rerank_ind"])
        g = p["grounding"]
        assert g["subg_index"] == int(p["consensus_rerank_ind"][0])              # the grounded sentence is the re-ranker's first choice
        for key in ("att2_ind", "node_ind", "sort_ind"):                         # the replay gives the same bits
            np.testing.assert_array_equal(p1["grounding"][key], p2["grounding"][key])
        for key in ("clss", "idx_in_sent", "bbox"):
            np.testing.assert_array_equal(p1["grounding_score"][key], p2["grounding_score"][key])
        # the same caption driven by a forced decode: its attention arg-max, fed to the host restatement of the material
        row = int(g["sort_ind"][g["subg_index"]])                                # the caption's row among the image's kept sub-graphs
        cand = int(p["sorted_subgraph_ind"][g["subg_index"]])                    # ... and its candidate index in the image
        ret = m(*synthetic.sample_args({k: v.clone() for k, v in b.items()}), opt=dict(kw, return_att=0), mode="sample")
        toks = ret[0].cpu().numpy()[row]
        assert int(ret[3][row]) == cand or not m.gpn
        C = int(b["gpn_obj_ind"].size(1) * b["gpn_obj_ind"].size(2)) if m.gpn else 1
        tok = np.zeros((C, m.seq_length), np.int64)
        tok[cand if m.gpn else 0] = toks
        f = forced.forced_decode(m, [b], [tok], return_att=True)
        fa = f["AL"].cpu().numpy()[:, cand if m.gpn else 0]                      # [Tf, N]
        idx = f["idx"].cpu().numpy()[cand if m.gpn else 0]
        n_words = len(g["node_ind"])
        assert n_words == int((np.cumprod(toks > 0)).sum())
        top2 = np.sort(fa[:n_words], 1)[:, -2:]
        safe = (top2[:, 1] - top2[:, 0]) >= GAP
        assert safe.any()
        f_node = idx[fa[:n_words].argmax(1)]
        np.testing.assert_array_equal(g["node_ind"][safe], f_node[safe])
        np.testing.assert_array_equal(p1["grounding"]["node_ind"][safe], f_node[safe])
        entry = dict(p, grounding=dict(g, node_ind=np.where(safe, f_node, g["node_ind"])))
        host = eval_glue.grounding_material(entry, out[f"{name}_{img['id']}_boxes"], meta["wd_to_lemma"], meta["lemma_det_id_dict"], det_wd, img_wh=img["wh"])
        gs = p["grounding_score"]
        assert [refs.class_names[c] for c in gs["clss"]] == list(host["clss"]) and gs["idx_in_sent"].tolist() == list(host["idx_in_sent"])
        np.testing.assert_array_equal(gs["bbox"], np.asarray(host["bbox"], np.float64).reshape(-1, 4).astype(np.float32))

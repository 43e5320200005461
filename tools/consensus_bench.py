#!/usr/bin/env python3
"""Consensus re-ranking of one decode batch (cook + score + rank, subgc.consensus) next to the decode that produces the batch and
to the reference scorer's per-pair CPU time.

    python tools/consensus_bench.py [--out profiles/r09_consensus_bench.txt] [--reps 40] [--scorer-only]
    python tools/consensus_bench.py --method bleu [--out profiles/r16_consensus_bleu_bench.txt]

--method bleu times the launches of method 'bleu' (subgc_consensus_bleu_cook / _bleu_score / subgc_consensus_rank, the defaults k = 60,
m = 175, n = 4, fpr = 1.0) beside the 'cider' launches and the decode of the same batch, and the m-RNN sentence BLEU
(calculate_bleu_sentence) as the CPU scorer.

Shapes: 256 images x top-4 of 10 captions (test.sh Karpathy + cr_mRNN_demo.py --top_k 4), 8 images x ~100 and 8 x ~1000 captions (the
MRNN settings, --rand_k 100 / up to 1000 kept sub-graphs); 60 neighbours x 5 captions = 300 neighbour captions, m = 125; a synthetic
corpus of 100 500 captions (Zipf ids over the 9487-word vocabulary plus corpus-only words) so the binary searches and gathers see a
realistic table.  The candidates that are re-ranked have the decode batch's row layout but are cut from neighbour captions, so n-grams
do match (a randomly initialised decoder emits words no caption holds).
Method: every shape is warmed up, then timed `reps` times; device time = HIP events around the three launches (with the upload of
the neighbour lists), wall = host clock around rerank() incl. its device -> host copy; median, min and max are reported.  The
decode is timed in the same process, same box: host clock around sample_images + synchronise.
The reference's scorer (its CiderScorer, read from where the reference lies; absent there: the restatement of tests/consensus_golden.py
with its vector cache off) is timed on a sample of pairs of the same inputs: CPU time per pair, and x pairs per batch."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "sub-gc_amd"), ROOT, os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

REF_SCORER = "/root/reference/misc/consensus_reranking/external/coco_caption_patch_mRNN_cr"
REF_BLEU = "/root/reference/misc/consensus_reranking/concensus_reranking_utils"
M_BLEU, N_BLEU, FPR_BLEU = 175, 4, 1.0
V, N_IMG, CAPS, K, M = 9487, 20100, 5, 60, 125


def make_corpus(rng):
    ids = np.minimum(rng.zipf(1.2, size=N_IMG * CAPS * 18), V + 500)
    lens = rng.integers(6, 19, size=N_IMG * CAPS)
    off = np.concatenate([[0], np.cumsum(lens)])
    return [[[int(x) for x in ids[off[i * CAPS + c]:off[i * CAPS + c + 1]]] for c in range(CAPS)] for i in range(N_IMG)]


def bleu_scorer():
    """-> (the sentence BLEU of two id lists, what it is): the reference's calculate_bleu_sentence where the reference lies (with a
    sliding-window stand-in for nltk.util.ngrams where nltk is missing), else the restatement of subgc.consensus."""
    if os.path.isdir(REF_BLEU):
        try:
            import nltk.util  # noqa: F401
            how = ""
        except ImportError:
            import types
            nltk, util = types.ModuleType("nltk"), types.ModuleType("nltk.util")
            util.ngrams = lambda seq, n: [tuple(seq[i:i + n]) for i in range(len(seq) - n + 1)]
            nltk.util = util
            sys.modules["nltk"], sys.modules["nltk.util"] = nltk, util
            how = " (nltk.util.ngrams: a sliding-window stand-in)"
        sys.path.insert(0, REF_BLEU)
        from bleu_score_util import calculate_bleu_sentence
        return (lambda a, b: calculate_bleu_sentence([f"w{x}" for x in a], [f"w{x}" for x in b], N_BLEU, fpr=FPR_BLEU),
                "the reference's calculate_bleu_sentence" + how)
    from subgc.consensus import bleu_pair_restatement
    return (lambda a, b: bleu_pair_restatement(a, b, N_BLEU, FPR_BLEU),
            "the Python restatement of the reference's sentence BLEU (subgc.consensus.bleu_pair_restatement; the reference is not on this box)")


def scorer_time(corpus_ids, cands, nn, pairs=1500, method="cider"):
    """CPU seconds per pair of the reference scorer on (candidate, neighbour caption) pairs of these inputs."""
    rng = np.random.default_rng(3)
    if method == "bleu":
        fn, what = bleu_scorer()
    elif os.path.isdir(REF_SCORER):
        sys.path.insert(0, REF_SCORER)
        from cider_scorer_compute_sentence import CiderScorer
        sc = CiderScorer(n=4, sigma=6.0)
        for caps in corpus_ids:
            refs = [" ".join(f"w{x}" for x in c) for c in caps]
            sc += (refs[0], refs)
        sc.compute_doc_freq()
        what = "the reference's CiderScorer.compute_cider_sen_pair"
        fn = lambda a, b: sc.compute_cider_sen_pair(" ".join(f"w{x}" for x in a), " ".join(f"w{x}" for x in b))  # noqa: E731
    else:
        import consensus_golden as G
        sc = G.Scorer(corpus_ids)
        what = "the numpy restatement of the reference scorer (tests/consensus_golden.py, cache off; the reference is not on this box)"

        def fn(a, b):
            sc._cache.clear()
            return sc.pair(a, b)
    sample = [(cands[int(rng.integers(len(cands)))], corpus_ids[int(nn[int(rng.integers(len(nn)))])][int(rng.integers(CAPS))]) for _ in range(pairs)]
    t0 = time.process_time()
    for a, b in sample:
        fn(a, b)
    return (time.process_time() - t0) / pairs, what


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/r09_consensus_bench.txt, with --method bleu profiles/r16_consensus_bleu_bench.txt")
    ap.add_argument("--method", default="cider", choices=["cider", "bleu"], help="bleu: time method 'bleu' beside method 'cider'")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--scorer-only", action="store_true", help="only time the CPU scorer (needs no GPU)")
    a = ap.parse_args()
    bleu = a.method == "bleu"
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r16_consensus_bleu_bench.txt" if bleu else "r09_consensus_bench.txt")
    rng = np.random.default_rng(9)
    t0 = time.perf_counter()
    corpus_ids = make_corpus(rng)
    lines = [f"consensus re-ranking bench: corpus {N_IMG} images x {CAPS} = {N_IMG * CAPS} captions, k = {K}, m = {M}, {K * CAPS} neighbour captions per image"]
    if bleu:
        lines.append(f"method 'bleu' (m = {M_BLEU}, n = {N_BLEU}, fpr = {FPR_BLEU}) beside method 'cider' (m = {M}) on the same batches")

    def cut_candidates(n, nn_row):
        out = []
        for _ in range(n):
            src = [x for x in corpus_ids[int(nn_row[int(rng.integers(K))])][int(rng.integers(CAPS))] if x <= V]
            s = src[:int(rng.integers(4, 14))] + [int(x) for x in np.minimum(rng.zipf(1.2, size=int(rng.integers(0, 6))), V)]
            out.append(s[:16])
        return out

    if a.scorer_only:
        nn_row = rng.choice(N_IMG, K, replace=False)
        per, what = scorer_time(corpus_ids, cut_candidates(100, nn_row), nn_row, method=a.method)
        lines.append(f"CPU scorer: {what}: {1e3 * per:.3f} ms per pair -> 256x4: {per * 256 * 4 * 300:.1f} s, 8x100: {per * 8 * 100 * 300:.1f} s, "
                     f"8x1000: {per * 8 * 1000 * 300:.1f} s per decode batch")
        print("\n".join(lines))
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return

    import torch
    import bench
    import subgc.models as models
    from subgc import consensus, synthetic
    assert torch.cuda.is_available(), "consensus_bench needs the MI355X (or --scorer-only)"
    dev = torch.device("cuda:0")
    vocab = {str(i): f"w{i}" for i in range(1, V + 1)}
    corpus = consensus.ConsensusCorpus([[[f"w{x}" for x in c] for c in caps] for caps in corpus_ids], vocab, device=dev)
    torch.cuda.synchronize()
    lines.append(f"corpus build (host tables + one cook launch): {time.perf_counter() - t0:.1f} s, {len(corpus.ukeys)} distinct n-grams, {corpus.n_ids} word ids")
    rr = consensus.ConsensusReranker(corpus, k=K, m=M)
    rb = None
    if bleu:
        rb = consensus.BleuConsensusReranker(corpus, k=K, m=M_BLEU, ngram=N_BLEU, fpr=FPR_BLEU)
        t1 = time.perf_counter()
        corpus.bleu_cooked()
        torch.cuda.synchronize()
        lines.append(f"the corpus's BLEU lists (one cook launch over the uploaded words, first use only): {1e3 * (time.perf_counter() - t1):.1f} ms")
    shapes = [("256 images x top-4 of <= 10", 256, 50, dict(gpn_nms_thres=0.75, gpn_max_subg=10), 4),
              ("8 images x <= 100", 8, 100, dict(gpn_nms_thres=0.55, gpn_max_subg=100, use_topk_sampling=1, topk_temp=0.6, the_k=3), None),
              ("8 images x <= 1000", 8, 500, dict(gpn_nms_thres=0.55, gpn_max_subg=1000, use_topk_sampling=1, topk_temp=0.6, the_k=3), None)]
    sopt = dict(sample_max=1, beam_size=1)
    per_pair = None
    for name, I, Mc, over, top_k in shapes:
        torch.manual_seed(0)
        m = models.setup(argparse.Namespace(**dict(bench.KAR, test_LSTM=1, **over))).to(dev).eval()
        images = [{k: v.to(dev) for k, v in synthetic.make_test_batch(Mc, seed=700 + i).items()} for i in range(I)]
        hold = {"skip_att": True}
        for _ in range(2):
            hold = {"skip_att": True}
            m.sample_images(images, opt=sopt, batch_out=hold)
        torch.cuda.synchronize()
        dec = []
        for _ in range(max(5, a.reps // 4)):
            t = time.perf_counter()
            m.sample_images(images, opt=sopt, batch_out={"skip_att": True})
            torch.cuda.synchronize()
            dec.append(1e3 * (time.perf_counter() - t))
        bounds = [int(x) for x in hold["bounds"]]
        rows, T = hold["seq"].shape
        nn = [[int(x) for x in rng.choice(N_IMG, K, replace=False)] for _ in range(I)]
        host_rows = np.zeros((rows, T), np.int64)
        cands = []
        for i in range(I):
            for r, s in enumerate(cut_candidates(bounds[i + 1] - bounds[i], nn[i])):
                host_rows[bounds[i] + r, :len(s)] = s
                cands.append(s)
        seq = torch.from_numpy(host_rows).to(dev)
        seg = torch.tensor(bounds, dtype=torch.int32).to(dev)
        max_rows = max(b - x for x, b in zip(bounds, bounds[1:]))
        scored = sum(min(b - x, top_k or b - x) for x, b in zip(bounds, bounds[1:]))
        sim = torch.empty(rows, dtype=torch.float64, device=dev)
        order = torch.empty(rows, dtype=torch.int32, device=dev)

        def timed(r):
            for _ in range(3):
                r.rerank(seq, bounds, nn, top_k=top_k)
            torch.cuda.synchronize()
            ev, wall = [], []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                r.enqueue(seq, seg, I, max_rows, nn, top_k, 0, sim, order)
                e1.record()
                e1.synchronize()
                ev.append(e0.elapsed_time(e1))
                t = time.perf_counter()
                r.rerank(seq, bounds, nn, top_k=top_k)
                wall.append(1e3 * (time.perf_counter() - t))
            return ev, wall

        ev, wall = timed(rr)
        if per_pair is None:
            per_pair, what = scorer_time(corpus_ids, cands[:200], nn[0], method=a.method)
            lines.append(f"CPU scorer on this box: {what}: {1e3 * per_pair:.3f} ms per pair")
        q = lambda x: f"median {statistics.median(x):.3f} (min {min(x):.3f}, max {max(x):.3f})"  # noqa: E731
        pairs = scored * K * CAPS
        lines.append(f"{name}: decode batch {rows} rows ({scored} re-ranked, {pairs} pairs)")
        lines.append(f"    decode (sample_images, wall ms, {len(dec)} runs):     {q(dec)}")
        if bleu:
            lines.append(f"    cider re-rank device ms (events, {a.reps} runs):           {q(ev)}")
            lines.append(f"    cider re-rank wall ms incl. the host copy ({a.reps} runs): {q(wall)}")
            ev, wall = timed(rb)
            lines.append(f"    bleu  re-rank device ms (events, {a.reps} runs):           {q(ev)}")
            lines.append(f"    bleu  re-rank wall ms incl. the host copy ({a.reps} runs): {q(wall)}")
        else:
            lines.append(f"    re-rank device ms (events, {a.reps} runs):           {q(ev)}")
            lines.append(f"    re-rank wall ms incl. the host copy ({a.reps} runs): {q(wall)}")
        lines.append(f"    {'bleu ' if bleu else ''}re-rank / decode (medians): {statistics.median(wall) / statistics.median(dec):.4f};  CPU scorer for the same pairs: "
                     f"{per_pair * pairs:.1f} s = {1e3 * per_pair * pairs / statistics.median(wall):.0f} x the re-rank wall time")
        del m
    print("\n".join(lines))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

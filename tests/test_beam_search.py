"""Batched, device-resident beam search (csrc/lv_beam.hip, engine.LSTMBeamSearcher, LSTMDecoder.beam_search_decode) and the
file-level entry points of generation.py.

The comparison rule (fixtures tests/golden/beam_*.npz, written by make_golden_beam.py from the reference's unmodified
beam_search_decode).  Beam search is a discrete function of f32 scores and torch.topk leaves ties unspecified, so with
TAU = 1e-4 (the project's parity bar, applied to log-probabilities):
  * a sentence whose recorded reference min_margin is >= TAU is reproduced id for id, its winner's score within 1e-4 relative
    of the recorded logp;
  * a sentence under TAU is left out of the id comparison but must be well-formed (<s> in front, no </s> before the last
    word, at most 101 ids);
  * every sentence is self-consistent: the returned score equals decoder.log_probability(returned ids, its z) (the
    teacher-forced HIP forward) within 1e-4 relative -- this pins parents, gathers and the back-trace without a reference;
  * at most 1/4 of a fixture's sentences are under TAU (a condition on the fixture, asserted by the generator and here).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import ALL_KEYS, build_vae, fixture_params, load

TAU = 1e-4
START, END = 1, 2
NEG = float("-inf")


# ---- kernel level (emulator build of the same sources) -------------------------------------------------------------------------
def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def _ref_step(logits, score, n_done, K, V):
    """float64 statement of dec_lstm.py:214-246 for one sentence: logits [K][V], score [K] (-inf = dead slot).
    -> picks [(score, slot, word)] in rank order, runner-up score (or None), float64 scores of all candidates."""
    live = [k for k in range(K) if score[k] != NEG]
    x = logits[live].astype(np.float64)
    m = x.max(axis=1, keepdims=True)
    logp = x - (m + np.log(np.exp(x - m).sum(axis=1, keepdims=True))) + score[live].astype(np.float64)[:, None]
    flat = (np.array(live)[:, None] * V + np.arange(V)[None, :]).reshape(-1)
    val = logp.reshape(-1)
    order = np.lexsort((flat, -val))                     # score descending, then flat index ascending
    n_pick = K - n_done
    picks = [(val[i], int(flat[i] // V), int(flat[i] % V)) for i in order[:n_pick]]
    nxt = float(val[order[n_pick]]) if len(order) > n_pick else None
    return picks, nxt


def _make_state(rng, B, K, V, H, inactive):
    ld = (V + 31) // 32 * 32
    st = dict(
        logits=(rng.standard_normal((B * K, ld)) * 3).astype(np.float32),
        tok=rng.integers(4, V, size=B * K).astype(np.int64),
        score=np.full(B * K, NEG, dtype=np.float32),
        meta=np.zeros((B, 4), dtype=np.int32),
        done_score=np.full(B * K, NEG, dtype=np.float32),
        done_ref=np.full((B * K, 2), -7, dtype=np.int32),
        h_src=rng.standard_normal((B * K, H)).astype(np.float32), c_src=rng.standard_normal((B * K, H)).astype(np.float32),
        h_dst=rng.standard_normal((B * K, H)).astype(np.float32), c_dst=rng.standard_normal((B * K, H)).astype(np.float32),
        margin=np.full(B, np.inf, dtype=np.float32), ld=ld)
    for b in range(B):
        n_done = 0 if b == 0 else int(rng.integers(0, K))              # sentence 0: nothing completed yet
        n_live = 1 if b == 0 else int(rng.integers(1, K - n_done + 1))
        # running log-probabilities in [-20, -2]: a candidate's score (logit - lse) + running is then never small against the f32
        # spacing of the log-sum-exp itself (1e-6 at lse ~ 12), below which no f32 evaluation can hold a relative 1e-6
        st["score"][b * K:b * K + n_live] = -2.0 - rng.random(n_live).astype(np.float32) * 18
        st["done_score"][b * K:b * K + n_done] = -rng.random(n_done).astype(np.float32) * 20
        st["meta"][b] = (n_done, 0 if b in inactive else 1, 3, 0)
    return st


# (16, 23001): 12 chunks x 16 slots x 17 survivors = 3264 candidates, more than the merge keeps in LDS (its recomputing path)
@pytest.mark.parametrize("K,V", [(1, 2500), (5, 2500), (16, 4099), (4, 61), (16, 23001)])
def test_select_and_advance_against_float64_statement(emu_backend, K, V):
    lib = emu_backend
    rng = np.random.default_rng(100 + K)
    B, H, T, t = 5, 24, 100, 3
    st = _make_state(rng, B, K, V, H, inactive={2})
    st["logits"][::2, END] += 9.0                                      # </s> among the picks of every other row
    if K >= 5:                                                         # a dead slot BELOW a live one: compaction is not assumed
        st["score"][3 * K:3 * K + 3] = (-1.5, NEG, -2.5)
        st["meta"][3] = (1, 1, 3, 0)
    part = np.zeros(lib.lv_beam_ws_floats(B, K, V), dtype=np.float32)
    pick_score = np.full((B, K + 1), 123.0, dtype=np.float32)
    pick_flat = np.full((B, K + 1), 123, dtype=np.int32)
    trace = np.full((T, B * K, 3), 77, dtype=np.int32)
    counter = np.array([B - 1], dtype=np.int32)
    before = {k: v.copy() for k, v in st.items() if isinstance(v, np.ndarray)}
    lib.lv_beam_select_f32(_p(st["logits"]), st["ld"], _p(st["score"]), _p(st["meta"]), _p(part), _p(pick_score), _p(pick_flat),
                           _p(st["margin"]), B, K, V, None)
    lib.lv_beam_advance_f32(_p(pick_score), _p(pick_flat), _p(st["h_src"]), _p(st["c_src"]), _p(st["h_dst"]), _p(st["c_dst"]),
                            _p(st["tok"]), _p(st["score"]), _p(st["meta"]), _p(st["done_score"]), _p(st["done_ref"]), _p(trace),
                            _p(counter), t, T, B, K, H, V, END, None)
    went_inactive = 0
    for b in range(B):
        sl = slice(b * K, (b + 1) * K)
        if b == 2:                                                     # an inactive sentence's state is untouched
            for k in ("tok", "score", "done_score", "done_ref", "h_dst", "c_dst"):
                assert np.array_equal(st[k][sl], before[k][sl]), k
            assert np.array_equal(st["meta"][b], before["meta"][b]) and np.all(trace[t, sl] == 77)
            assert np.all(pick_flat[b] == 123) and st["margin"][b] == np.inf
            continue
        n_done0 = int(before["meta"][b, 0])
        picks, nxt = _ref_step(before["logits"][sl, :V], before["score"][sl], n_done0, K, V)
        n_pick = K - n_done0
        got = [(float(pick_score[b, r]), int(pick_flat[b, r]) // V, int(pick_flat[b, r]) % V) for r in range(n_pick)]
        gaps = [picks[r][0] - picks[r + 1][0] for r in range(n_pick - 1)] + ([picks[-1][0] - nxt] if nxt is not None else [])
        if nxt is None or picks[-1][0] - nxt > 1e-5:                   # the accepted set, where the decision was not marginal
            assert sorted(g[1:] for g in got) == sorted(p[1:] for p in picks)
        if all(g > 1e-5 for g in gaps):                                # ... and the rank order
            assert [g[1:] for g in got] == [p[1:] for p in picks]
            for g, p in zip(got, picks):
                assert abs(g[0] - p[0]) <= 1e-6 * abs(p[0])
            if nxt is not None:
                assert abs(float(st["margin"][b]) - (picks[-1][0] - nxt)) < 1e-4
        # the bookkeeping follows the kernel's own picks, in rank order: completed list, compaction, gathered rows, trace
        n_done, n_live = n_done0, 0
        for r, (sc, parent, word) in enumerate(got):
            if word == END:
                assert st["done_score"][b * K + n_done] == np.float32(sc)
                assert tuple(st["done_ref"][b * K + n_done]) == (t, r)
                assert tuple(trace[t, b * K + r]) == (parent, word, -1)
                n_done += 1
            else:
                row = b * K + n_live
                assert st["tok"][row] == word and st["score"][row] == np.float32(sc)
                assert np.array_equal(st["h_dst"][row], before["h_src"][b * K + parent])       # bit-equal to their sources
                assert np.array_equal(st["c_dst"][row], before["c_src"][b * K + parent])
                assert tuple(trace[t, b * K + r]) == (parent, word, n_live)
                n_live += 1
        assert np.all(st["score"][b * K + n_live:(b + 1) * K] == NEG)
        assert np.all(trace[t, b * K + n_pick:(b + 1) * K] == -1)
        assert np.array_equal(st["h_dst"][b * K + n_live:(b + 1) * K], before["h_dst"][b * K + n_live:(b + 1) * K])
        active = not (n_done == K or n_live == 0)
        assert tuple(st["meta"][b][:3]) == (n_done, int(active), t + 1)
        went_inactive += not active
    assert counter[0] == B - 1 - went_inactive
    assert np.all(trace[:t] == 77) and np.all(trace[t + 1:] == 77)


def test_select_forces_completion_and_resolves_ties_to_the_lower_flat_index(emu_backend):
    lib = emu_backend
    B, K, V, H, T = 1, 3, 2500, 8, 100
    ld = (V + 31) // 32 * 32
    rng = np.random.default_rng(5)
    row = (rng.standard_normal(ld) * 0.1).astype(np.float32)
    row[7] = row[2100] = 9.0                                           # the same best logit in two different chunks
    row[END] = 8.0
    logits = np.stack([row, row, row]).copy()
    score = np.array([-1.0, -1.0, NEG], dtype=np.float32)             # two live slots with the same score, one dead
    meta = np.array([[0, 1, 0, 0]], dtype=np.int32)
    part = np.zeros(lib.lv_beam_ws_floats(B, K, V), dtype=np.float32)
    pick_score = np.zeros((B, K + 1), dtype=np.float32)
    pick_flat = np.zeros((B, K + 1), dtype=np.int32)
    margin = np.full(B, np.inf, dtype=np.float32)
    lib.lv_beam_select_f32(_p(logits), ld, _p(score), _p(meta), _p(part), _p(pick_score), _p(pick_flat), _p(margin), B, K, V, None)
    assert list(pick_flat[0]) == [7, 2100, V + 7, V + 2100]            # four equal scores: lower flat index first
    assert pick_score[0, 0] == pick_score[0, 3] and margin[0] == 0.0
    # next step: every pick is </s> -> K completed, the sentence goes inactive and the counter drops
    row2 = row.copy()
    row2[END] = 30.0
    logits = np.stack([row2, row2 - 1.0, row2]).copy()
    tok = np.full(K, START, dtype=np.int64)
    done_score = np.full(K, NEG, dtype=np.float32)
    done_ref = np.zeros((K, 2), dtype=np.int32)
    h = rng.standard_normal((2, K, H)).astype(np.float32)
    c = rng.standard_normal((2, K, H)).astype(np.float32)
    trace = np.zeros((T, K, 3), dtype=np.int32)
    counter = np.array([1], dtype=np.int32)
    meta[0, 0] = 1                                                     # one already completed: two picks
    lib.lv_beam_select_f32(_p(logits), ld, _p(score), _p(meta), _p(part), _p(pick_score), _p(pick_flat), _p(margin), B, K, V, None)
    assert list(pick_flat[0][:2]) == [END, V + END] and pick_flat[0][3] == -1
    lib.lv_beam_advance_f32(_p(pick_score), _p(pick_flat), _p(h[1]), _p(c[1]), _p(h[0]), _p(c[0]), _p(tok), _p(score), _p(meta),
                            _p(done_score), _p(done_ref), _p(trace), _p(counter), 0, T, B, K, H, V, END, None)
    assert tuple(meta[0][:3]) == (3, 0, 1) and counter[0] == 0 and np.all(score == NEG)
    assert done_ref[1:].tolist() == [[0, 0], [0, 1]]


def test_backtrace_on_a_hand_made_trace(emu_backend):
    lib = emu_backend
    B, K, T = 4, 2, 100
    rng = np.random.default_rng(8)
    trace = np.full((T, B, K, 3), -1, dtype=np.int32)
    score = np.full((B, K), NEG, dtype=np.float32)
    meta = np.zeros((B, 4), dtype=np.int32)
    done_score = np.full((B, K), NEG, dtype=np.float32)
    done_ref = np.zeros((B, K, 2), dtype=np.int32)
    # sentence 0: </s> completed at step 1 with the best score, a live hypothesis went on for three more steps
    trace[0, 0] = [(0, END, -1), (0, 9, 0)]
    for s in (1, 2):
        trace[s, 0, 0] = (0, 10 + s, 0)
    done_score[0, 0], done_ref[0, 0] = -1.0, (0, 0)
    score[0, 0] = -5.0
    meta[0] = (1, 1, 3, 0)
    # sentence 1: two live hypotheses that swap slots at random for 100 steps; the winner is the live one in slot 1
    seqs = [[START], [START]]
    for s in range(T):
        if s == 0:
            parents = [0, 0]
        else:
            parents = [int(v) for v in rng.integers(0, 2, size=2)]
        words = [int(v) for v in rng.integers(4, 50, size=2)]
        new = []
        for r in range(2):
            trace[s, 1, r] = (parents[r], words[r], 1 - r)             # rank 0 lands in slot 1, rank 1 in slot 0
            new.append(seqs[parents[r]] + [words[r]])
        seqs = [new[1], new[0]]
    score[1] = (-30.0, -20.0)
    done_score[1, 0], done_ref[1, 0] = -25.0, (4, 0)                   # a completed one that loses (never walked)
    meta[1] = (1, 1, T, 0)
    # sentence 2: a completed and a live hypothesis with the SAME score: the completed one comes first
    trace[0, 2] = [(0, 5, 0), (0, 6, 1)]
    trace[1, 2] = [(1, END, -1), (0, 8, 0)]
    done_score[2, 0], done_ref[2, 0] = -3.0, (1, 0)
    score[2, 0] = -3.0
    meta[2] = (1, 1, 2, 0)
    # sentence 3: nothing at all (guarded): [<s>]
    ids = np.full((B, T + 1), -5, dtype=np.int64)
    ln = np.zeros(B, dtype=np.int32)
    win = np.zeros(B, dtype=np.float32)
    lib.lv_beam_backtrace(_p(score), _p(meta), _p(done_score), _p(done_ref), _p(trace), _p(ids), _p(ln), _p(win), B, K, T, START, None)
    assert list(ln) == [2, T + 1, 3, 1]
    assert list(ids[0][:2]) == [START, END] and win[0] == -1.0
    assert list(ids[1]) == seqs[1] and win[1] == -20.0
    assert list(ids[2][:3]) == [START, 6, END] and win[2] == -3.0
    assert ids[3][0] == START


def test_beam_entry_points_refuse_bad_arguments_and_shapes(emu_backend):
    raw = emu_backend.cdll
    a = np.zeros(64, dtype=np.float32)
    i = np.zeros(64, dtype=np.int32)
    l = np.zeros(64, dtype=np.int64)
    assert emu_backend.lv_beam_supported(32, 5, 20001) == 1
    assert emu_backend.lv_beam_supported(32, 17, 20001) == 0           # K > 16
    assert emu_backend.lv_beam_supported(1, 16, 1 << 27) == 0          # K * V >= 2^31
    assert emu_backend.lv_beam_supported(2000, 5, 100) == 0            # B * K > 8192 rows
    assert emu_backend.lv_beam_ws_floats(32, 17, 20001) == 0 and emu_backend.lv_beam_ws_floats(2, 3, 2049) == 2 * 3 * 2 * 36
    sel = raw.lv_beam_select_f32
    assert sel(None, 64, _p(a), _p(i), _p(a), _p(a), _p(i), _p(a), 1, 2, 8, None) == -1
    assert sel(_p(a), 4, _p(a), _p(i), _p(a), _p(a), _p(i), _p(a), 1, 2, 8, None) == -2       # ld < V
    assert sel(_p(a), 8, _p(a), _p(i), _p(a), _p(a), _p(i), _p(a), 1, 17, 8, None) == -4
    adv = raw.lv_beam_advance_f32
    args = [_p(a), _p(i), _p(a), _p(a), _p(a[32:]), _p(a[32:]), _p(l), _p(a), _p(i), _p(a), _p(i), _p(i), _p(i)]
    assert adv(*(args + [100, 100, 1, 2, 4, 8, END, None])) == -2       # t >= Tmax
    assert adv(*(args + [0, 100, 1, 2, 4, 8, 8, None])) == -2           # </s> outside the vocabulary
    assert adv(*(args[:4] + [_p(a), _p(a)] + args[6:] + [0, 100, 1, 2, 4, 8, END, None])) == -1   # gather in place
    assert adv(*(args + [0, 100, 1, 17, 4, 8, END, None])) == -4
    assert raw.lv_beam_backtrace(_p(a), _p(i), _p(a), _p(i), _p(i), None, _p(i), _p(a), 1, 2, 100, START, None) == -1
    assert raw.lv_beam_backtrace(_p(a), _p(i), _p(a), _p(i), _p(i), _p(l), _p(i), _p(a), 1, 17, 100, START, None) == -4
    assert raw.lv_beam_init_f32(_p(a), _p(a), _p(a), _p(a), _p(l), _p(a), _p(i), _p(a), _p(a), _p(i), 1, 2, 4, 8, 9, None) == -2


# ---- route level ---------------------------------------------------------------------------------------------------------------
def _ids(sents):
    return [[int(w[1:]) for w in s] for s in sents]


def _mid_vae(device):
    fx = load("beam_mid")
    V, ni, H, nz = (int(fx[k]) for k in ("V", "ni", "H", "nz"))
    vae = build_vae(V, ni, H, nz, device, params=fixture_params(fx))
    vae.eval()
    return vae


def _yahoo_vae(device):
    """Weights regenerated from the seed through the same nn.Module construction order as the fixture script's, + its </s>
    boost; checked against the stored samples."""
    fx = load("beam_yahoo_seeded")
    V, ni, H, nz = (int(fx[k]) for k in ("V", "ni", "H", "nz"))
    vae = build_vae(V, ni, H, nz, "cpu", seed=int(fx["model_seed"]), model_scale=float(fx["model_scale"]),
                    emb_scale=float(fx["emb_scale"]))
    with torch.no_grad():
        vae.decoder.pred_linear.weight[END] *= float(fx["boost"])
    sd = vae.state_dict()
    for k in ALL_KEYS:
        idx = torch.from_numpy(fx["sample_idx/" + k])
        assert torch.equal(sd[k].reshape(-1)[idx], torch.from_numpy(fx["sample_param/" + k])), k
    vae = vae.to(device)
    vae.eval()
    return vae


def _check_self_consistent(vae, z, ids, score):
    """score[i] == log p(ids[i] | z[i]) by the teacher-forced forward, one call per group of equal length."""
    by_len = {}
    for i, s in enumerate(ids):
        by_len.setdefault(len(s), []).append(i)
    for n, rows in by_len.items():
        if n < 2:
            continue
        x = torch.tensor([ids[i] for i in rows], dtype=torch.int64, device=z.device)
        with torch.no_grad():
            lp = vae.decoder.log_probability(x, z[rows].view(len(rows), 1, -1)).view(-1).cpu().numpy()
        for i, v in zip(rows, lp):
            print("  self-consistency sentence %d len %d: score %.6f teacher-forced %.6f" % (i, n, score[i], v))
            assert abs(float(score[i]) - float(v)) <= 1e-4 * abs(float(v)), (i, float(score[i]), float(v))


def _check_comparison_rule(vae, fx, K, device, n=None):
    tag = "K%d/" % K
    margin_ref = fx[tag + "min_margin"]
    assert 4 * int((margin_ref < TAU).sum()) <= len(margin_ref)         # the cap is a condition on the fixture
    n = len(margin_ref) if n is None else n
    z = torch.from_numpy(fx["z"][:n]).to(device)
    sents, info = vae.decode(z, "beam", K=K, return_info=True)
    ids = _ids(sents)
    assert len(ids) == n and all(len(info[k]) == n for k in ("score", "steps", "n_completed", "min_margin"))
    for i, s in enumerate(ids):
        assert s[0] == START and END not in s[1:-1] and 2 <= len(s) <= 101, (i, s[:8])
        print("  sentence %d: margin ref %.3e ours %.3e, logp ref %.6f ours %.6f, len %d" % (
            i, margin_ref[i], info["min_margin"][i], fx[tag + "logp"][i], info["score"][i], len(s)))
        if margin_ref[i] >= TAU:
            want = list(fx[tag + "ids"][i][:int(fx[tag + "len"][i])])
            assert s == want, (i, s[:12], want[:12])
            assert abs(float(info["score"][i]) - float(fx[tag + "logp"][i])) <= 1e-4 * abs(float(fx[tag + "logp"][i])), i
            assert int(info["steps"][i]) == int(fx[tag + "steps"][i]) and int(info["n_completed"][i]) == int(fx[tag + "n_completed"][i])
    _check_self_consistent(vae, z, ids, info["score"])
    return ids, info


def _qualified(fx, K, n):
    return [i for i in range(n) if fx["K%d/min_margin" % K][i] >= TAU]


def _check_route_properties(vae, fx, K, device, n, alone):
    """batched_beam = False gives the same sentences; a sentence decoded alone gives the same ids; the result does not depend
    on poll; both routes report the same min_margin -- all on the TAU-qualified set."""
    dec = vae.decoder
    z = torch.from_numpy(fx["z"][:n]).to(device)
    q = _qualified(fx, K, n)
    sents, info = dec.beam_search_decode(z, K, return_info=True)
    assert all(info[k].shape == (n,) for k in info)
    try:
        dec.batched_beam = False
        sents_old, info_old = dec.beam_search_decode(z, K, return_info=True)
        assert all(info_old[k].shape == (n,) for k in info_old) and sorted(info_old) == sorted(info)
        assert dec.beam_search_decode(z[:2], K) == sents_old[:2]                     # and without the dict, as before
    finally:
        del dec.batched_beam
    for i in q:
        assert sents[i] == sents_old[i], i
        assert abs(float(info["min_margin"][i]) - float(info_old["min_margin"][i])) <= 1e-4, i
        assert abs(float(info["score"][i]) - float(info_old["score"][i])) <= 1e-4 * abs(float(info_old["score"][i])), i
        assert int(info["steps"][i]) == int(info_old["steps"][i]) and int(info["n_completed"][i]) == int(info_old["n_completed"][i])
    for i in [j for j in alone if j in q]:
        assert dec.beam_search_decode(z[i:i + 1], K) == [sents[i]], i
    try:
        outs = []
        for poll in (1, 100):
            dec.beam_poll = poll
            outs.append(dec.beam_search_decode(z, K, return_info=True))
    finally:
        del dec.beam_poll
    for s, inf in outs:
        assert s == sents
        for k in info:
            assert np.array_equal(inf[k], info[k]), k


def test_beam_mid_first_12_sentences_emulated(emu_backend):
    """The first 12 of beam_mid's 48 sentences (emulator time; the GPU test takes all 48)."""
    _check_comparison_rule(_mid_vae("cpu"), load("beam_mid"), 5, "cpu", n=12)


@pytest.mark.parametrize("K", [1, 2, 8])
def test_beam_k_emulated(emu_backend, K):
    """beam_k at K = 1, 2 (all 16 sentences) and K = 8 (the first 8: emulator time)."""
    _check_comparison_rule(_mid_vae("cpu"), load("beam_k"), K, "cpu", n=8 if K == 8 else None)


def test_route_properties_emulated(emu_backend):
    _check_route_properties(_mid_vae("cpu"), load("beam_mid"), 5, "cpu", n=6, alone=(0, 3))


def test_shape_outside_the_envelope_takes_the_per_sentence_route(emu_backend, monkeypatch):
    from vae_lagging_encoder_amd import engine
    fx = load("generate_small")
    V, ni, H, nz = (int(fx[k]) for k in ("V", "ni", "H", "nz"))
    vae = build_vae(V, ni, H, nz, "cpu", params=fixture_params(fx))
    vae.eval()
    z = torch.from_numpy(fx["z"])[:2]
    calls = []
    real = engine.LSTMBeamSearcher.search
    monkeypatch.setattr(engine.LSTMBeamSearcher, "search", lambda self, *a: calls.append(1) or real(self, *a))
    inside = vae.decode(z, "beam", K=4)
    assert calls == [1]
    sents, info = vae.decode(z, "beam", K=17, return_info=True)        # K = 17: outside, the old route
    assert calls == [1] and len(sents) == 2 and info["score"].shape == (2,)
    assert all(s[0] == "w%d" % START for s in sents) and all(s[0] == "w%d" % START for s in inside)


# ---- generation.py ---------------------------------------------------------------------------------------------------------------
def _corpus_model(tmp_path, device):
    from vae_lagging_encoder_amd.data import MonoTextData
    from vae_lagging_encoder_amd.factory import build_text_vae
    fx = load("data_small")
    paths = {}
    for name in ("train", "val"):
        paths[name] = os.path.join(str(tmp_path), name + ".txt")
        with open(paths[name], "w") as fh:
            txt = str(fx[name + "_txt"])
            fh.write(txt if name == "train" else "\n".join(txt.split("\n")[:26]) + "\n")     # 26 lines of val (23 sentences): emulator time
    train = MonoTextData(paths["train"], max_length=12)
    val = MonoTextData(paths["val"], vocab=train.vocab)
    vae = build_text_vae(len(train.vocab), 8, 16, 4, device, seed=3, model_scale=0.6, emb_scale=1.0, vocab=train.vocab)
    with torch.no_grad():
        vae.decoder.pred_linear.weight[train.vocab["</s>"]] *= 4.0
    vae.eval()
    return vae, val


def _inject_z(vae, monkeypatch, nz=4):
    """sample_from_inference replaced by a z that depends on the sentence alone, whatever batch it arrives in."""
    def z_of(x, nsamples=1):
        rows = []
        for r in x.tolist():
            words = tuple(w for w in r if w != 0)
            g = torch.Generator().manual_seed(hash(words) % (1 << 31))
            rows.append(torch.randn(nz, generator=g))
        return torch.stack(rows).unsqueeze(1).to(x.device)
    monkeypatch.setattr(vae, "sample_from_inference", z_of)


def _check_generation_files(tmp_path, monkeypatch, device):
    from vae_lagging_encoder_amd import generation
    vae, val = _corpus_model(tmp_path, device)
    _inject_z(vae, monkeypatch)
    assert len(val) % 7 != 0                                           # there is a trailing partial batch to lose
    for strategy in ("greedy", "beam"):
        files = []
        for bs in (1, 7):
            f = os.path.join(str(tmp_path), "%s_%d.txt" % (strategy, bs))
            generation.reconstruct(vae, val, strategy, f, device, batch_size=bs)
            with open(f) as fh:
                files.append(fh.read().split("\n"))
        assert files[0] == files[1], strategy
        lines = files[0]
        assert lines[-1] == "" and len(lines) == len(val) + 1          # one line per sentence
        # ... in input order: line i is what decoding sentence i alone gives
        for i in (0, 5, len(val) - 1):
            x, _ = val._frame([val.data[i]], True, device)
            with torch.no_grad():
                want = vae.reconstruct(x, strategy)[0]
            assert lines[i] == " ".join(want), (strategy, i)
        if strategy == "beam":
            assert all(ln.split()[0] == "<s>" for ln in lines[:-1])
        z = torch.randn(9, 4, generator=torch.Generator().manual_seed(2)).to(device)
        f = os.path.join(str(tmp_path), "prior_%s.txt" % strategy)
        generation.sample_from_prior(vae, z, strategy, f)
        with open(f) as fh:
            got = fh.read().split("\n")
        with torch.no_grad():
            assert got == [" ".join(s) for s in vae.decode(z, strategy)] + [""]


def test_generation_files_emulated(emu_backend, tmp_path, monkeypatch):
    _check_generation_files(tmp_path, monkeypatch, "cpu")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_beam_mid_gpu(hip_device):
    _check_comparison_rule(_mid_vae(hip_device), load("beam_mid"), 5, hip_device)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 8])
def test_beam_k_gpu(hip_device, K):
    _check_comparison_rule(_mid_vae(hip_device), load("beam_k"), K, hip_device)


@pytest.mark.gpu
def test_route_properties_gpu(hip_device):
    _check_route_properties(_mid_vae(hip_device), load("beam_mid"), 5, hip_device, n=48, alone=(0, 7, 19, 33, 47))


@pytest.mark.gpu
def test_rerun_is_bit_identical_gpu(hip_device):
    vae, fx = _mid_vae(hip_device), load("beam_mid")
    z = torch.from_numpy(fx["z"]).to(hip_device)
    a, ia = vae.decode(z, "beam", K=5, return_info=True)
    b, ib = vae.decode(z, "beam", K=5, return_info=True)
    assert a == b
    for k in ia:
        assert np.array_equal(ia[k], ib[k]), k


@pytest.mark.gpu
def test_generation_files_gpu(hip_device, tmp_path, monkeypatch):
    _check_generation_files(tmp_path, monkeypatch, hip_device)


@pytest.mark.gpu
def test_beam_yahoo_seeded_gpu_fixture_parent_route_and_speed(hip_device):
    """beam_yahoo_seeded (V/ni/H/nz = 20001/512/1024/32, B = 32, K = 5) against the fixture, against the per-sentence route
    (the parent commit's) on the same card, and the floor on speed: with one set of launches per step serving 32 sentences and
    no host read per step, the batched route is not slower than the per-sentence one."""
    import time
    fx = load("beam_yahoo_seeded")
    vae = _yahoo_vae(hip_device)
    dec = vae.decoder
    ids, info = _check_comparison_rule(vae, fx, 5, hip_device)          # warms the batched route
    z = torch.from_numpy(fx["z"]).to(hip_device)
    try:
        dec.batched_beam = False
        old, info_old = dec.beam_search_decode(z, 5, return_info=True)  # warms the per-sentence route
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.beam_search_decode(z, 5)
        torch.cuda.synchronize()
        t_old = time.perf_counter() - t0
    finally:
        del dec.batched_beam
    for i in _qualified(fx, 5, len(ids)):
        assert ids[i] == _ids(old)[i], i
        assert abs(float(info["min_margin"][i]) - float(info_old["min_margin"][i])) <= 1e-4, i
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dec.beam_search_decode(z, 5)
    torch.cuda.synchronize()
    t_new = time.perf_counter() - t0
    print("beam search, Yahoo shape, B = 32, K = 5: per-sentence %.1f ms, batched %.1f ms, ratio %.2f" % (
        1e3 * t_old, 1e3 * t_new, t_old / t_new))
    assert t_new <= t_old

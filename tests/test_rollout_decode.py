"""Device-resident greedy and sample decoding (csrc/lv_rollout.hip, engine.LSTMRollout, LSTMDecoder.greedy_decode /
sample_decode, VAE.decode(..., return_info=True)).

Kernel level (emulator build and MI355X through one fixture): lv_rollout_pick_f32 against a float64 statement of the step and,
bit for bit, against lv_argmax_rows_f32 / lv_sample_rows_f32 on the same rows; the bookkeeping on poisoned buffers.

Route level: tests/golden/rollout_mid.npz (make_golden_rollout.py: the reference's unmodified greedy_decode on beam_mid's model
and its 48 latent codes).  The comparison rule is the beam tests', TAU = 1e-4:
  * a sentence whose recorded reference min_margin is >= TAU is reproduced id for id, its score within 1e-4 relative of the
    recorded logp, steps equal, min_margin within 1e-4 absolute;
  * every sentence is well-formed (1 <= len <= 99, no </s> before the last word, all ids < V) and self-consistent: the returned
    score equals decoder.log_probability([<s>] + words, its z) within 1e-4 relative;
  * at most 1/4 of the fixture's sentences are under TAU (a condition on the fixture, asserted by the generator and here).
"""
import numpy as np
import pytest
import torch

from helpers import build_vae, fixture_params, load
from vae_lagging_encoder_amd import engine as _eng
from vae_lagging_encoder_amd.engine import P

TAU = 1e-4
START, END = 1, 2
TMAX = 99
EPS = float(torch.finfo(torch.float32).eps)
INF = float("inf")
SHAPES = [(1, 61), (5, 2500), (37, 4099), (3, 23001)]
H = 24
PAD = 1e30                         # padding columns V .. ld: wins every argmax and swamps every sum if it is read


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def target(request):
    if request.param == "emu":
        request.getfixturevalue("emu_backend")
        dev = torch.device("cpu")
    else:
        dev = request.getfixturevalue("hip_device")
    return _eng.backend_for(dev), dev


def _s(dev):
    return _eng.stream_ptr(dev)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _scenarios(n, roles):
    """Rows take the roles in turn: one launch when there are enough rows, else as many launches as it takes."""
    return [dict(enumerate(roles[i:i + n])) for i in range(0, len(roles), n)]


class _State(object):
    """Poisoned roll-out buffers on the host (ids 77, len 123 for dead rows, ...), moved to the device by launch()."""

    def __init__(self, n, V, g, dead=(), t=3):
        self.n, self.V, self.t = n, V, t
        self.ld = (V + 31) // 32 * 32
        self.logits = torch.full((n, self.ld), PAD)
        self.logits[:, :V] = 3.0 * torch.randn(n, V, generator=g)
        self.h_src, self.c_src = torch.randn(n, H, generator=g), torch.randn(n, H, generator=g)
        self.h_dst, self.c_dst = torch.full((n, H), 5.0), torch.full((n, H), -5.0)
        self.tok = torch.randint(4, V, (n,), generator=g)
        self.alive = torch.ones(n, dtype=torch.int32)
        self.ids = torch.full((n * TMAX + 8,), 77, dtype=torch.int64)          # 8 guard words behind the last row
        self.len = torch.full((n,), t, dtype=torch.int32)
        self.score = torch.zeros(n)
        self.margin = torch.full((n,), INF)
        for r in dead:
            self.alive[r] = 0
            self.len[r] = 123
            self.score[r] = -123.0
            self.margin[r] = 0.123
        self.counter = torch.tensor([n - len(dead) + 5], dtype=torch.int32)   # never reaches zero here: the drop is what is checked
        self.u = None
        self.names = ("h_dst", "c_dst", "tok", "alive", "ids", "len", "score", "margin", "counter")

    def launch(self, lib, dev, t=None):
        t = self.t if t is None else t
        self.before = {k: getattr(self, k).clone() for k in self.names}
        d = {k: getattr(self, k).to(dev) for k in self.names + ("logits", "h_src", "c_src")}
        u = None if self.u is None else self.u.to(dev)
        lib.lv_rollout_pick_f32(P(d["logits"]), self.ld, P(u), P(d["h_src"]), P(d["c_src"]), P(d["h_dst"]), P(d["c_dst"]), P(d["tok"]),
                                P(d["alive"]), P(d["ids"]), P(d["len"]), P(d["score"]), P(d["margin"]), P(d["counter"]), t, TMAX,
                                self.n, H, self.V, END, _s(dev))
        ref = torch.full((self.n + 1,), -9, dtype=torch.int64, device=dev)     # the stand-alone row kernel on the same rows
        if u is None:
            lib.lv_argmax_rows_f32(P(d["logits"]), self.ld, self.n, self.V, P(ref), _s(dev))
        else:
            lib.lv_sample_rows_f32(P(d["logits"]), self.ld, self.n, self.V, P(u), P(ref), _s(dev))
        for k in self.names:
            setattr(self, k, d[k].cpu())
        assert int(ref[self.n]) == -9
        return ref[:self.n].cpu()

    def check_bookkeeping(self, pick, t=None):
        """What every launch must leave behind, given the picks of the live rows."""
        t = self.t if t is None else t
        b, n, V = self.before, self.n, self.V
        ids, ids0 = self.ids[:n * TMAX].view(n, TMAX), b["ids"][:n * TMAX].view(n, TMAX)
        ended = 0
        for r in range(n):
            if not int(b["alive"][r]):                                   # a dead row keeps its bytes
                for k in ("tok", "alive", "len", "score", "margin"):
                    assert _same(getattr(self, k)[r], b[k][r]), (k, r)
                assert torch.equal(ids[r], ids0[r]), r
                continue
            w = int(pick[r])
            assert int(ids[r, t]) == w and int(self.tok[r]) == w, r
            assert torch.equal(ids[r, :t], ids0[r, :t]) and torch.equal(ids[r, t + 1:], ids0[r, t + 1:]), r
            assert int(self.len[r]) == int(b["len"][r]) + 1
            assert int(self.alive[r]) == int(w != END)
            ended += w == END
        assert bool(((self.tok >= 0) & (self.tok < V)).all())
        assert _same(self.h_dst, self.h_src) and _same(self.c_dst, self.c_src)       # every row's state, bit for bit
        assert int(self.counter[0]) == int(b["counter"][0]) - ended
        assert bool((self.ids[n * TMAX:] == 77).all())
        return ended


def _logp64(row, V, w):
    x = row[:V].double()
    m = x.max()
    return float((x[w] - m) - (x - m).exp().sum().log())


# ---- kernel level ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,V", SHAPES)
def test_greedy_pick_against_float64_statement(target, n, V):
    lib, dev = target
    for k, roles in enumerate(_scenarios(n, ["tie", "end", "dead"])):
        g = torch.Generator().manual_seed(1000 * n + V + k)
        dead = [r for r, role in roles.items() if role == "dead"]
        st = _State(n, V, g, dead=dead)
        a, b2 = V // 3, V - 1                                            # the tie spans the row: the lowest column must win
        for r, role in roles.items():
            top = float(st.logits[r, :V].max())
            if role == "tie":
                st.logits[r, a] = st.logits[r, b2] = top + 1.0
            elif role == "end":
                st.logits[r, END] = top + 2.0                            # </s> wins: the row ends
        ref = st.launch(lib, dev)
        ended = st.check_bookkeeping(ref)
        assert ended == sum(role == "end" for role in roles.values())
        for r in range(n):
            role = roles.get(r, "plain")
            if role == "dead":
                continue
            w = int(ref[r])
            x = st.logits[r, :V]
            assert float(x[w]) == float(x.max()) and not bool((x[:w] == x[w]).any())       # the argmax, lowest column
            if role == "tie":
                assert w == a and float(st.margin[r]) == 0.0
            if role == "end":
                assert w == END
            lp64 = _logp64(st.logits[r], V, w)
            got = float(st.score[r])                                     # score was 0: the increment itself
            top2 = torch.topk(x.double(), 2)[0]
            gap64 = float(top2[0] - top2[1])
            print("  greedy n=%d V=%d row %d (%s): logp %.9g ours %.9g rel %.2e; gap %.9g ours %.9g" % (
                n, V, r, role, lp64, got, abs(got - lp64) / abs(lp64), gap64, float(st.margin[r])))
            if abs(lp64) >= 1e-3:
                assert abs(got - lp64) <= 1e-6 * abs(lp64), (r, got, lp64)
            assert abs(float(st.margin[r]) - gap64) <= 1e-6, (r, float(st.margin[r]), gap64)


@pytest.mark.parametrize("n,V", SHAPES)
def test_sample_pick_is_bit_equal_to_sample_rows(target, n, V):
    """Roles: u = 0 with -inf in front (the first POSITIVE column), u = 1 - 2^-24 with -inf at the end (a running sum that may
    come out short: the last positive column), a row whose weights all underflow but the maximum's, a dead row, ordinary draws."""
    lib, dev = target
    for k, roles in enumerate(_scenarios(n, ["u0", "u1", "underflow", "dead", "plain", "plain"])):
        g = torch.Generator().manual_seed(2000 * n + V + k)
        dead = [r for r, role in roles.items() if role == "dead"]
        st = _State(n, V, g, dead=dead)
        st.u = torch.rand(n, generator=g)
        st.margin[:] = 0.5                                               # sampling leaves margin alone
        for r, role in roles.items():
            st.logits[r, (7 * r + 5) % V] = -INF
            if role == "u0":
                st.u[r] = 0.0
                st.logits[r, :3] = -INF
            elif role == "u1":
                st.u[r] = 1.0 - 2.0 ** -24
                st.logits[r, V - 3:V] = -INF
            elif role == "underflow":
                st.logits[r, :V] = -200.0 + 3.0 * torch.randn(V, generator=g)
                st.logits[r, V // 2] = 0.0
                st.u[r] = 1.0 - 2.0 ** -24
        ref = st.launch(lib, dev)
        st.check_bookkeeping(ref)                                        # ids / tok of live rows == lv_sample_rows_f32's pick
        assert _same(st.margin, st.before["margin"])
        L = (V + 63) // 64 + 8          # the wave's serial chain of log-sum-exp merges (tests/test_eval_txn_kernels.py's rule) + x - M, log
        for r in range(n):
            role = roles.get(r, "plain")
            if role == "dead":
                continue
            w = int(ref[r])
            assert float(st.logits[r, w]) > -INF
            if role == "u0":
                assert w == int((st.logits[r, :V] > -INF).nonzero()[0])
            if role == "underflow":
                assert w == V // 2
            lp64 = _logp64(st.logits[r], V, w)
            got = float(st.score[r])
            print("  sample n=%d V=%d row %d (%s): pick %d logp %.9g ours %.9g" % (n, V, r, role, w, lp64, got))
            assert abs(got - lp64) <= (8 + L) * EPS * max(1.0, abs(lp64)), (r, got, lp64)


def test_bookkeeping_over_steps_last_column_and_the_counter_gate(target):
    lib, dev = target
    n, V = 5, 2500
    g = torch.Generator().manual_seed(77)
    st = _State(n, V, g, dead=[3], t=0)
    st.counter[0] = 4
    st.score[:] = torch.tensor([-1.0, -2.0, -3.0, -123.0, -5.0])
    st.margin[0] = 1e-3                                                  # smaller than any gap of this row: the minimum is kept
    st.logits[1, END] = 99.0
    lp = [_logp64(st.logits[r], V, int(st.logits[r, :V].argmax())) for r in range(n)]
    ref = st.launch(lib, dev, t=TMAX - 1)                                # the last column, nothing behind it
    assert st.check_bookkeeping(ref, t=TMAX - 1) == 1 and int(st.counter[0]) == 3
    assert float(st.margin[0]) == float(np.float32(1e-3)) and float(st.margin[1]) > 50.0
    for r in (0, 2, 4):
        assert abs(float(st.score[r]) - (float(st.before["score"][r]) + lp[r])) <= 4 * EPS * abs(float(st.score[r]))
    # all remaining rows end: the counter reaches zero ...
    st.logits[:, END] = 99.0
    ref = st.launch(lib, dev, t=5)
    assert int(st.counter[0]) == 0 and not bool(st.alive.any())
    assert all(int(ref[r]) == END for r in range(n))
    # ... and a launch that finds it at zero changes nothing at all, in either mode
    for u in (None, torch.rand(n, generator=g)):
        st.u = u
        st.alive[2] = 1                                                  # even a row that claims to be alive
        st.h_dst.fill_(5.0)
        st.launch(lib, dev, t=6)
        for k in st.names:
            assert _same(getattr(st, k), st.before[k]), k


def test_init_sets_the_start_state(target):
    lib, dev = target
    n, V = 7, 61
    g = torch.Generator().manual_seed(5)
    h0, c0 = torch.randn(n, H, generator=g).to(dev), torch.randn(n, H, generator=g).to(dev)
    hs, cs = torch.full((2, n, H), 9.0, device=dev), torch.full((2, n, H), 9.0, device=dev)
    tok = torch.full((n + 1,), 77, dtype=torch.int64, device=dev)
    alive, ln = torch.full((n + 1,), 77, dtype=torch.int32, device=dev), torch.full((n + 1,), 77, dtype=torch.int32, device=dev)
    score, margin = torch.full((n + 1,), 123.0, device=dev), torch.full((n + 1,), 123.0, device=dev)
    counter = torch.tensor([77, 77], dtype=torch.int32, device=dev)
    lib.lv_rollout_init_f32(P(h0), P(c0), P(hs), P(cs), P(tok), P(alive), P(ln), P(score), P(margin), P(counter), n, H, V, START, _s(dev))
    assert _same(hs[0], h0) and _same(cs[0], c0) and bool((hs[1] == 9.0).all()) and bool((cs[1] == 9.0).all())
    assert tok.tolist() == [START] * n + [77] and alive.tolist() == [1] * n + [77] and ln.tolist() == [0] * n + [77]
    assert score.tolist() == [0.0] * n + [123.0] and margin.tolist() == [INF] * n + [123.0] and counter.tolist() == [n, 77]


def test_rollout_entry_points_refuse_bad_arguments(target):
    lib, dev = target
    raw = lib.cdll
    f = torch.zeros(256, device=dev)
    i = torch.zeros(64, dtype=torch.int32, device=dev)
    q = torch.zeros(256, dtype=torch.int64, device=dev)
    s = _s(dev)

    def pick(logits=P(f), ld=32, u=None, hs=P(f), cs=P(f), hd=P(f, 128), cd=P(f, 128), tok=P(q), margin=P(f), t=0, Tmax=TMAX, n=1, V=8,
             end=END):
        return raw.lv_rollout_pick_f32(logits, ld, u, hs, cs, hd, cd, tok, P(i), P(q), P(i), P(f), margin, P(i), t, Tmax, n, 4, V, end, s)
    assert pick(logits=None) == -1 and pick(tok=None) == -1
    assert pick(margin=None) == -1                                       # greedy needs margin ...
    assert pick(ld=4) == -2                                              # ld < V
    assert pick(t=TMAX) == -2 and pick(t=-1) == -2                       # t >= Tmax
    assert pick(end=8) == -2 and pick(end=-1) == -2                      # </s> outside [0, V)
    assert pick(hd=P(f)) == -1 and pick(cd=P(f)) == -1                   # h_src == h_dst
    assert pick(n=0) == -2
    assert pick(ld=10) == -3 and pick(logits=P(f, 1)) == -3              # greedy rows are read in 16-byte pieces

    def init(h0=P(f), h=P(f, 128), tok=P(q), start=START, n=1, V=8):
        return raw.lv_rollout_init_f32(h0, P(f), h, P(f, 128), tok, P(i), P(i), P(f), P(f), P(i), n, 4, V, start, s)
    assert init(h0=None) == -1 and init(tok=None) == -1
    assert init(start=8) == -2 and init(start=-1) == -2                  # <s> outside [0, V)
    assert init(n=0) == -2


# ---- route level -----------------------------------------------------------------------------------------------------------------
def _ids(sents):
    return [[int(w[1:]) for w in s] for s in sents]


def _mid_vae(device):
    fx = load("beam_mid")
    V, ni, Hd, nz = (int(fx[k]) for k in ("V", "ni", "H", "nz"))
    vae = build_vae(V, ni, Hd, nz, device, params=fixture_params(fx))
    vae.eval()
    return vae


def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def _check_well_formed(ids, V):
    for i, s in enumerate(ids):
        assert 1 <= len(s) <= TMAX and END not in s[:-1] and all(0 <= w < V for w in s), (i, s[:8])


def _check_self_consistent(vae, z, ids, score):
    """score[i] == log p([<s>] + ids[i] | z[i]) by the teacher-forced forward, one call per group of equal length."""
    by_len = {}
    for i, s in enumerate(ids):
        by_len.setdefault(len(s), []).append(i)
    for n, rows in by_len.items():
        x = torch.tensor([[START] + ids[i] for i in rows], dtype=torch.int64, device=z.device)
        with torch.no_grad():
            lp = vae.decoder.log_probability(x, z[rows].view(len(rows), 1, -1)).view(-1).cpu().numpy()
        for i, v in zip(rows, lp):
            print("  self-consistency sentence %d len %d: score %.6f teacher-forced %.6f" % (i, n, score[i], v))
            assert abs(float(score[i]) - float(v)) <= 1e-4 * abs(float(v)), (i, float(score[i]), float(v))


def _check_comparison_rule(vae, device, n=None):
    fx = load("rollout_mid")
    mid = load("beam_mid")
    assert np.array_equal(fx["z"], mid["z"])
    margin_ref = fx["min_margin"]
    assert 4 * int((margin_ref < TAU).sum()) <= len(margin_ref)         # the cap is a condition on the fixture
    n = len(margin_ref) if n is None else n
    z = torch.from_numpy(fx["z"][:n]).to(device)
    sents, info = vae.decode(z, "greedy", return_info=True)
    ids = _ids(sents)
    assert isinstance(info, dict) and sorted(info) == ["min_margin", "score", "steps"]
    assert len(ids) == n and all(info[k].shape == (n,) for k in info)
    _check_well_formed(ids, int(fx["V"]))
    for i, s in enumerate(ids):
        print("  sentence %d: margin ref %.3e ours %.3e, logp ref %.6f ours %.6f, len %d" % (
            i, margin_ref[i], info["min_margin"][i], fx["logp"][i], info["score"][i], len(s)))
        assert int(info["steps"][i]) == len(s)
        if margin_ref[i] >= TAU:
            want = list(fx["ids"][i][:int(fx["len"][i])])
            assert s == want, (i, s[:12], want[:12])
            assert abs(float(info["score"][i]) - float(fx["logp"][i])) <= 1e-4 * abs(float(fx["logp"][i])), i
            assert int(info["steps"][i]) == int(fx["len"][i])
            assert abs(float(info["min_margin"][i]) - float(margin_ref[i])) <= 1e-4, i
    _check_self_consistent(vae, z, ids, info["score"])


def _same_info(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def _check_route_properties(vae, device, n, alone):
    dec = vae.decoder
    fx = load("rollout_mid")
    z = torch.from_numpy(fx["z"][:n]).to(device)
    V = int(fx["V"])
    sents, info = dec.greedy_decode(z, return_info=True)
    drawn, dinfo = dec.sample_decode(z, generator=_gen(device, 3), return_info=True)
    assert sorted(dinfo) == ["score", "steps"] and all(dinfo[k].shape == (n,) for k in dinfo)
    # sample validity: valid, score self-consistent (and reproducible from a generator seeded alike: the runs below)
    _check_well_formed(_ids(drawn), V)
    assert [len(s) for s in drawn] == dinfo["steps"].tolist()
    _check_self_consistent(vae, z, _ids(drawn), dinfo["score"])
    # route equality: the per-step route returns the same sentences, every one of them
    try:
        dec.batched_rollout = False
        old, oinfo = dec.greedy_decode(z, return_info=True)
        odrawn, odinfo = dec.sample_decode(z, generator=_gen(device, 3), return_info=True)
        assert dec.greedy_decode(z[:2]) == old[:2]                       # and without the dict, as before
    finally:
        del dec.batched_rollout
    assert sents == old and drawn == odrawn
    for a, b in ((info, oinfo), (dinfo, odinfo)):
        assert sorted(a) == sorted(b) and np.array_equal(a["steps"], b["steps"])
        assert bool((np.abs(a["score"] - b["score"]) <= 1e-4 * np.abs(b["score"])).all())
    assert bool((np.abs(info["min_margin"] - oinfo["min_margin"]) <= 1e-4).all())
    # poll independence: {1, 8, 100}, the runs above being the ones at 8
    assert dec.rollout_poll == 8
    try:
        for poll in (1, 100):
            dec.rollout_poll = poll
            s2, i2 = dec.greedy_decode(z, return_info=True)
            assert s2 == sents
            _same_info(i2, info)
            d2, di2 = dec.sample_decode(z, generator=_gen(device, 3), return_info=True)
            assert d2 == drawn
            _same_info(di2, dinfo)
    finally:
        del dec.rollout_poll
    # decoding alone
    for i in [j for j in alone if fx["min_margin"][j] >= TAU]:
        assert dec.greedy_decode(z[i:i + 1]) == [sents[i]], i


def _check_generate_small(device):
    fx = load("generate_small")
    V, ni, Hd, nz = (int(fx[k]) for k in ("V", "ni", "H", "nz"))
    vae = build_vae(V, ni, Hd, nz, device, params=fixture_params(fx))
    vae.eval()
    z = torch.from_numpy(fx["z"]).to(device)
    want = [list(fx["greedy_ids"][i][:int(fx["greedy_len"][i])]) for i in range(z.shape[0])]
    assert _ids(vae.decode(z, "greedy")) == want
    sents, info = vae.decode(z, "greedy", return_info=True)             # the tuple and the dict
    assert _ids(sents) == want and all(info[k].shape == (z.shape[0],) for k in ("score", "steps", "min_margin"))
    assert isinstance(vae.decode(z, "sample", return_info=True), tuple) and isinstance(vae.decode(z, "sample"), list)
    try:
        vae.decoder.batched_rollout = False
        assert _ids(vae.decode(z, "greedy")) == want
    finally:
        del vae.decoder.batched_rollout
    return vae, z


def test_rollout_mid_first_12_sentences_emulated(emu_backend):
    """The first 12 of rollout_mid's 48 sentences (emulator time; the GPU test takes all 48)."""
    _check_comparison_rule(_mid_vae("cpu"), "cpu", n=12)


def test_route_properties_emulated(emu_backend):
    _check_route_properties(_mid_vae("cpu"), "cpu", n=6, alone=(0, 3))


def test_generate_small_and_the_route_taken_emulated(emu_backend, monkeypatch):
    vae, z = _check_generate_small("cpu")
    calls = []
    real = _eng.LSTMRollout.decode
    monkeypatch.setattr(_eng.LSTMRollout, "decode", lambda self, *a, **kw: calls.append(1) or real(self, *a, **kw))
    vae.decode(z, "greedy")
    assert calls == [1]
    vae.decoder.sample_decode(z)
    assert calls == [1, 1]
    try:
        vae.decoder.batched_rollout = False
        vae.decode(z, "greedy", return_info=True)
        vae.decoder.sample_decode(z)
    finally:
        del vae.decoder.batched_rollout
    assert calls == [1, 1]


@pytest.mark.gpu
def test_rollout_mid_gpu(hip_device):
    _check_comparison_rule(_mid_vae(hip_device), hip_device)


@pytest.mark.gpu
def test_route_properties_gpu(hip_device):
    _check_route_properties(_mid_vae(hip_device), hip_device, n=48, alone=(0, 7, 19, 33, 47))


@pytest.mark.gpu
def test_generate_small_gpu(hip_device):
    _check_generate_small(hip_device)

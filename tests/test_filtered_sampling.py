"""Temperature, top-k and nucleus (top-p) sampling for the LSTM decoder (csrc/lv_pick.h: lv_block_filtered_pick;
lv_sample_filtered_rows_f32, lv_rollout_pick_filtered_f32; LSTMDecodeStepper.sample_filtered, LSTMRollout.decode and
LSTMDecoder.sample_decode with temperature / top_k / top_p; the pass-through of VAE.decode and generation.py).

The reference has no truncated sampling, so there are two oracles: a float64 statement of the contract (include/lvae.h at
lv_sample_filtered_rows_f32), written here, and the greedy route, which tests/test_rollout_decode.py pins to the reference's own
greedy_decode: top_k = 1 and top_p = 1e-6 must reproduce it.

Kernel level (emulator build and MI355X through one fixture).  y = x * inv_temp as ONE f32 multiply; everything behind it in float64.
  exact: K rebuilt from (tau, ntie) has `kept` members and is a prefix of the f32 order of y; the pick is in K and has positive
         weight; top_k = 1 / top_p = 1e-6 give the argmax (lowest column) with lq == 0.0; ties at rank k keep the lower columns.
  band:  delta = (8 + L) EPS, L = LV_FILTERED_L of lv_pick.h (asserted <= (V + 63) // 64 + 8).  With c_j the float64 cumulative
         masses of the renormalised top-k set in contract order, the nucleus length m satisfies c_m >= top_p - delta and
         c_{m-1} < top_p + delta; the pick c satisfies excl(c) - delta <= u <= incl(c) + delta over K in column order.  For at least
         3/4 of the rows the band admits exactly one m (a condition on the inputs, asserted).
  score: lp, lq against float64 under (8 + L) EPS max(1, |value|).
"""
import os
import re

import numpy as np
import pytest
import torch

from helpers import build_vae, load
from test_rollout_decode import END, H, PAD, TMAX, _check_self_consistent, _check_well_formed, _gen, _ids, _mid_vae, _same, _State
from vae_lagging_encoder_amd import engine as _eng
from vae_lagging_encoder_amd import generation
from vae_lagging_encoder_amd.engine import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -23
INF = float("inf")
U_TOP = 1.0 - 2.0 ** -24
SHAPES = [(1, 61), (5, 2500), (37, 4099), (3, 23001)]
INV_TEMPS = [1.0, float(np.float32(1 / 0.7))]
TOP_PS = [1.0, 0.95, 0.9, 0.5, 1e-6]
ROLES = ["plain", "tie40", "neginf", "underflow", "u0", "u1"]


def _top_ks(V):
    return [0, 1, 40, V, V + 7]


def _chain_length():
    with open(os.path.join(ROOT, "vae_lagging_encoder_amd", "csrc", "lv_pick.h")) as fh:
        m = re.search(r"constexpr int LV_FILTERED_L = (\d+);", fh.read())
    assert m, "lv_pick.h states L as LV_FILTERED_L"
    return int(m.group(1))


L = _chain_length()
DELTA = (8 + L) * EPS


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


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
_INPUTS = {}


def _inputs(n, V):
    """The launches of one shape: [(x f32 [n][V], u f32 [n], roles, planted)], rows taking ROLES in turn (as many launches as it
    takes for every role to occur).  Computed once per shape and left unchanged."""
    if (n, V) in _INPUTS:
        return _INPUTS[(n, V)]
    rs, ru = np.random.RandomState(1000 + V), np.random.RandomState(2000 + V)
    out = []
    for k in range(-(-len(ROLES) // n)):
        x = (rs.randn(n, V) * 5).astype(np.float32)
        u = np.minimum(ru.rand(n), U_TOP).astype(np.float32)
        roles, planted = [], {}
        for r in range(n):
            role = ROLES[(k * n + r) % len(ROLES)]
            roles.append(role)
            if role == "tie40":                                          # five equal values on ranks 37 .. 41: rank 39 is the 40th column
                order = np.argsort(-x[r], kind="stable")
                cols = np.sort(order[37:42])
                x[r, cols] = x[r, order[39]]
                assert x[r, order[36]] > x[r, cols[0]] > x[r, order[42]]
                planted[r] = cols
            elif role == "neginf":
                x[r, :3] = -INF
                x[r, (7 * r + 5) % V] = -INF
                x[r, V - 2:] = -INF
                u[r] = [0.0, U_TOP][r % 2]
            elif role == "underflow":
                x[r] = (-200.0 + 3.0 * rs.randn(V)).astype(np.float32)
                x[r, V // 2] = 0.0
                u[r] = U_TOP
            elif role == "u0":
                u[r] = 0.0
            elif role == "u1":
                u[r] = U_TOP
        out.append((x, u, roles, planted))
    _INPUTS[(n, V)] = out
    return out


_ROWS = {}


def _row64(key, x, inv_temp):
    """(y f32, contract order, float64 weights) of one row at one temperature, computed once."""
    if key not in _ROWS:
        y = x * np.float32(inv_temp)                                     # one f32 multiply
        assert y.dtype == np.float32
        order = np.lexsort((np.arange(len(y)), -y.astype(np.float64)))  # larger first, lower column among equals
        y64 = y.astype(np.float64)
        d = y64 - y64.max()
        # a condition on the inputs: no weight near the f32 underflow threshold, where "w > 0" would depend on the exp in use
        assert not bool(((d < -80.0) & (d > -150.0)).any())
        w = np.where(d > -150.0, np.exp(d), 0.0)
        _ROWS[key] = (y, order, w)
    return _ROWS[key]


def _run_rows(lib, dev, x, u, inv_temp, top_k, top_p):
    """lv_sample_filtered_rows_f32 on padded rows; every output has a guard element behind it."""
    n, V = x.shape
    ld = (V + 31) // 32 * 32
    full = np.full((n, ld), PAD, dtype=np.float32)
    full[:, :V] = x
    lg, ud = torch.from_numpy(full).to(dev), torch.from_numpy(u).to(dev)
    idx = torch.full((n + 1,), -9, dtype=torch.int64, device=dev)
    kept, ntie = (torch.full((n + 1,), -9, dtype=torch.int32, device=dev) for _ in range(2))
    lp, lq, tau = (torch.full((n + 1,), 123.0, device=dev) for _ in range(3))
    lib.lv_sample_filtered_rows_f32(P(lg), ld, n, V, P(ud), inv_temp, top_k, top_p, P(idx), P(lp), P(lq), P(kept), P(tau), P(ntie), _s(dev))
    assert int(idx[n]) == -9 and int(kept[n]) == -9 and int(ntie[n]) == -9
    assert float(lp[n]) == 123.0 and float(lq[n]) == 123.0 and float(tau[n]) == 123.0
    return {k: v[:n].cpu().numpy() for k, v in (("idx", idx), ("lp", lp), ("lq", lq), ("kept", kept), ("tau", tau), ("ntie", ntie))}


def _check_row(tag, x, u, role, planted, out, r, inv_temp, top_k, top_p, tally):
    V = len(x)
    y, order, w = _row64(tag, x, inv_temp)
    p32 = float(np.float32(top_p))
    pick, kept, ntie, tau = int(out["idx"][r]), int(out["kept"][r]), int(out["ntie"][r]), out["tau"][r]
    k_eff = V if (top_k <= 0 or top_k >= V) else top_k
    # exact: K from (tau, ntie) has `kept` members and is a prefix of the order
    ties = np.flatnonzero(y == tau)
    assert 1 <= ntie <= len(ties), (tag, ntie, len(ties))
    in_k = y > tau
    in_k[ties[:ntie]] = True
    members = np.flatnonzero(in_k)
    assert len(members) == kept and 1 <= kept <= k_eff, (tag, kept, len(members), k_eff)
    assert np.array_equal(np.sort(order[:kept]), members), tag
    if top_k > 0:
        assert kept <= top_k
    # band: the nucleus length
    ck = np.cumsum(w[order[:k_eff]])
    ck /= ck[-1]
    if p32 >= 1.0:
        assert kept == k_eff
    else:
        m = kept
        assert ck[m - 1] >= p32 - DELTA, (tag, m, ck[m - 1], p32)
        assert m == 1 or ck[m - 2] < p32 + DELTA, (tag, m, ck[m - 2], p32)
        lo = int(np.searchsorted(ck, p32 - DELTA, "left")) + 1          # the m the band admits: lo .. hi
        hi = min(int(np.searchsorted(ck, p32 + DELTA, "left")) + 1, k_eff)
        assert lo <= m <= hi
        tally["rows"] += 1
        tally["single"] += hi == lo
    # the pick: in K, positive weight, finite logit, inside the band of u over K in column order
    i = int(np.searchsorted(members, pick))
    assert i < kept and members[i] == pick, (tag, pick)
    wk = w[members]
    assert wk[i] > 0.0 and np.isfinite(x[pick]), (tag, pick, x[pick])
    S = wk.sum()
    incl = np.cumsum(wk) / S
    excl = incl[i] - wk[i] / S
    assert excl - DELTA <= float(u) <= incl[i] + DELTA, (tag, pick, excl, float(u), incl[i])
    if float(u) == 0.0:
        assert pick == members[np.flatnonzero(wk > 0.0)[0]]             # the first POSITIVE column of K
    if top_k == 1 or top_p == 1e-6:
        assert pick == order[0] and kept == 1 and float(out["lq"][r]) == 0.0, (tag, pick, order[0], kept, out["lq"][r])
    if role == "underflow":
        assert pick == V // 2
    if role == "tie40" and top_k == 40 and p32 >= 1.0:                   # the tie straddles rank 40: the three lower columns are in
        assert ntie == 3 and tau == y[planted[0]] and np.array_equal(ties[:ntie], planted[:3]), (tag, ntie)
    # scores
    x64 = x.astype(np.float64)
    lp64 = (x64[pick] - x64.max()) - np.log(np.exp(x64 - x64.max()).sum())
    lq64 = (float(y[pick]) - float(y.max())) - np.log(S)
    for name, got, want in (("lp", float(out["lp"][r]), lp64), ("lq", float(out["lq"][r]), lq64)):
        assert abs(got - want) <= (8 + L) * EPS * max(1.0, abs(want)), (tag, name, got, want)


# ---- kernel level ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,V", SHAPES)
def test_filtered_rows_against_float64_contract(target, n, V):
    """Every row of every launch under every setting of inv_temp x top_k x top_p; nothing is skipped."""
    lib, dev = target
    assert L <= (V + 63) // 64 + 8
    tally = {"rows": 0, "single": 0}
    seen = set()
    for k, (x, u, roles, planted) in enumerate(_inputs(n, V)):
        seen.update(roles)
        for inv_temp in INV_TEMPS:
            for top_k in _top_ks(V):
                for top_p in TOP_PS:
                    out = _run_rows(lib, dev, x, u, inv_temp, top_k, top_p)
                    for r in range(n):
                        _check_row((n, V, k, r, inv_temp), x[r], u[r], roles[r], planted.get(r), out, r, inv_temp, top_k, top_p, tally)
    assert seen == set(ROLES)
    print("  n=%d V=%d: the band admits a single nucleus length in %d of %d row checks" % (n, V, tally["single"], tally["rows"]))
    assert 4 * tally["single"] >= 3 * tally["rows"] > 0


def test_top_k_distribution_as_a_whole(target):
    """V = 61, top_k = 5, 512 rows of the same logits with u_i = (i + 0.5) / 512: every column's count within +-2 of 512 q64[c],
    columns outside K never drawn."""
    lib, dev = target
    V, R = 61, 512
    x1 = _inputs(1, V)[0][0][0]
    x = np.repeat(x1[None, :], R, axis=0)
    u = ((np.arange(R) + 0.5) / R).astype(np.float32)
    out = _run_rows(lib, dev, x, u, 1.0, 5, 1.0)
    y, order, w = _row64(("dist", V), x1, 1.0)
    q = np.zeros(V)
    q[order[:5]] = w[order[:5]] / w[order[:5]].sum()
    counts = np.bincount(out["idx"], minlength=V)
    print("  top-5 columns %s: counts %s, expected %s" % (order[:5], counts[order[:5]], np.round(R * q[order[:5]], 2)))
    assert counts.sum() == R and bool((counts[q == 0.0] == 0).all())
    assert bool((np.abs(counts - R * q) <= 2.0).all())
    assert bool((out["kept"] == 5).all())


class _FState(_State):
    """_State with qscore; launch() runs lv_rollout_pick_filtered_f32 and, on the same rows, lv_sample_filtered_rows_f32."""

    def __init__(self, n, V, g, dead=(), t=3):
        super(_FState, self).__init__(n, V, g, dead=dead, t=t)
        self.logits[:, :V] = torch.from_numpy((np.random.RandomState(1000 + V).randn(n, V) * 5).astype(np.float32))
        self.qscore = torch.zeros(n)
        for r in dead:
            self.qscore[r] = -77.0
        self.margin[:] = 0.5
        self.u = torch.rand(n, generator=g)
        self.names = self.names + ("qscore",)

    def launch(self, lib, dev, filt, t=None):
        t = self.t if t is None else t
        self.before = {k: getattr(self, k).clone() for k in self.names}
        d = {k: getattr(self, k).to(dev) for k in self.names + ("logits", "h_src", "c_src", "u")}
        lib.lv_rollout_pick_filtered_f32(P(d["logits"]), self.ld, P(d["u"]), filt[0], filt[1], filt[2], P(d["h_src"]), P(d["c_src"]),
                                         P(d["h_dst"]), P(d["c_dst"]), P(d["tok"]), P(d["alive"]), P(d["ids"]), P(d["len"]),
                                         P(d["score"]), P(d["qscore"]), P(d["counter"]), t, TMAX, self.n, H, self.V, END, _s(dev))
        idx = torch.full((self.n + 1,), -9, dtype=torch.int64, device=dev)
        lp, lq = torch.zeros(self.n, device=dev), torch.zeros(self.n, device=dev)
        lib.lv_sample_filtered_rows_f32(P(d["logits"]), self.ld, self.n, self.V, P(d["u"]), filt[0], filt[1], filt[2], P(idx), P(lp), P(lq),
                                        None, None, None, _s(dev))
        for k in self.names:
            setattr(self, k, d[k].cpu())
        assert int(idx[self.n]) == -9
        return idx[:self.n].cpu(), lp.cpu(), lq.cpu()


FILTERS = [(float(np.float32(1 / 0.7)), 40, float(np.float32(0.9))), (1.0, 0, 0.5), (1.0, 7, 1.0), (float(np.float32(1 / 0.7)), 0, 1.0)]


@pytest.mark.parametrize("n,V", SHAPES)
def test_rollout_entry_is_bit_equal_to_the_row_entry_and_keeps_the_books(target, n, V):
    lib, dev = target
    for k, filt in enumerate(FILTERS if V < 20000 else FILTERS[:2]):
        g = torch.Generator().manual_seed(3000 * n + V + k)
        dead = [1] if n > 1 else []
        st = _FState(n, V, g, dead=dead)
        if n > 2:
            st.logits[2, END] = 99.0                                     # </s> holds all the weight: the row ends
        idx, lp, lq = st.launch(lib, dev, filt)
        ended = st.check_bookkeeping(idx)                               # picks == the row entry's; dead rows, state, counter, guards
        assert ended == (1 if n > 2 else 0)
        assert _same(st.margin, st.before["margin"])                    # there is no margin here
        for r in range(n):
            if r in dead:
                assert _same(st.qscore[r], st.before["qscore"][r])
            else:                                                        # score and qscore were 0: the increments themselves
                assert _same(st.score[r], lp[r]) and _same(st.qscore[r], lq[r]), (r, st.score[r], lp[r], st.qscore[r], lq[r])
        # a second launch on the same inputs is bit-identical
        first = {name: getattr(st, name).clone() for name in st.names}
        for name in st.names:
            setattr(st, name, st.before[name].clone())
        idx2, lp2, lq2 = st.launch(lib, dev, filt)
        assert torch.equal(idx, idx2) and _same(lp, lp2) and _same(lq, lq2)
        for name in st.names:
            assert _same(getattr(st, name), first[name]), name


def test_filtered_pick_counter_gate_and_the_last_column(target):
    lib, dev = target
    n, V = 5, 2500
    g = torch.Generator().manual_seed(78)
    st = _FState(n, V, g, dead=[3], t=0)
    st.counter[0] = 4
    st.logits[:, END] = 99.0
    idx, _, _ = st.launch(lib, dev, FILTERS[0], t=TMAX - 1)             # the last column, nothing behind it; every live row ends
    assert st.check_bookkeeping(idx, t=TMAX - 1) == 4 and int(st.counter[0]) == 0 and not bool(st.alive.any())
    st.alive[2] = 1                                                      # even a row that claims to be alive
    st.h_dst.fill_(5.0)
    st.launch(lib, dev, FILTERS[0], t=6)                                 # counter == 0: nothing changes
    for name in st.names:
        assert _same(getattr(st, name), st.before[name]), name


def test_filtered_entry_points_refuse_bad_arguments(target):
    lib, dev = target
    raw = lib.cdll
    f = torch.full((256,), 7.0, device=dev)
    i = torch.full((64,), 7, dtype=torch.int32, device=dev)
    q = torch.full((256,), 7, dtype=torch.int64, device=dev)
    s = _s(dev)
    nan = float("nan")

    def rows(lg=P(f), ld=32, R=1, C=8, u=P(f), it=1.0, k=0, p=1.0, idx=P(q)):
        return raw.lv_sample_filtered_rows_f32(lg, ld, R, C, u, it, k, p, idx, P(f), P(f), P(i), P(f), P(i), s)
    assert rows(lg=None) == -1 and rows(u=None) == -1 and rows(idx=None) == -1
    assert rows(R=0) == -2 and rows(C=0) == -2 and rows(ld=4) == -2
    assert rows(it=0.0) == -2 and rows(it=-1.0) == -2 and rows(it=INF) == -2 and rows(it=nan) == -2
    assert rows(p=0.0) == -2 and rows(p=1.5) == -2 and rows(p=-0.1) == -2 and rows(p=nan) == -2
    assert rows(k=-1) == -2
    assert rows(ld=10) == -3 and rows(lg=P(f, 1)) == -3                  # rows are read in 16-byte pieces

    def pick(logits=P(f), ld=32, u=P(f), it=1.0, k=0, p=1.0, hs=P(f), cs=P(f), hd=P(f, 128), cd=P(f, 128), tok=P(q), qs=P(f), t=0,
             Tmax=TMAX, n=1, V=8, end=END):
        return raw.lv_rollout_pick_filtered_f32(logits, ld, u, it, k, p, hs, cs, hd, cd, tok, P(i), P(q), P(i), P(f), qs, P(i), t, Tmax,
                                                n, 4, V, end, s)
    assert pick(logits=None) == -1 and pick(tok=None) == -1 and pick(qs=None) == -1
    assert pick(u=None) == -1                                            # u is mandatory here
    assert pick(hd=P(f)) == -1 and pick(cd=P(f)) == -1                   # h_src == h_dst
    assert pick(ld=4) == -2 and pick(n=0) == -2
    assert pick(t=TMAX) == -2 and pick(t=-1) == -2
    assert pick(end=8) == -2 and pick(end=-1) == -2
    assert pick(it=0.0) == -2 and pick(it=-2.0) == -2 and pick(it=INF) == -2 and pick(it=nan) == -2
    assert pick(p=0.0) == -2 and pick(p=1.0001) == -2 and pick(p=nan) == -2
    assert pick(k=-3) == -2
    assert pick(ld=10) == -3 and pick(logits=P(f, 1)) == -3
    # nothing was launched: the buffers are as they were
    assert bool((f == 7.0).all()) and bool((i == 7).all()) and bool((q == 7).all())


# ---- decoder level ---------------------------------------------------------------------------------------------------------------
FILT = dict(temperature=0.7, top_k=40, top_p=0.9)


def _score_bound(score, steps):
    """Two routes' sums of `steps` per-step log-probabilities, each within (8 + L) EPS max(1, |lp_t|) of float64 and added in f32
    (half an ulp of the running sum per addition, in either route): sum_t max(1, |lp_t|) <= steps + |score|."""
    return 2.0 * (8 + L) * EPS * (steps + abs(score)) + steps * EPS * abs(score)


def _check_greedy_limit(vae, device, n, settings):
    """top_k = 1 and top_p = 1e-6 leave the argmax alone in K: greedy_decode's sentences, whatever the generator and temperature."""
    dec = vae.decoder
    z = torch.from_numpy(load("rollout_mid")["z"][:n]).to(device)
    want, ginfo = dec.greedy_decode(z, return_info=True)
    for seed, kw in enumerate(settings):
        got, info = dec.sample_decode(z, generator=_gen(device, seed), return_info=True, **kw)
        assert sorted(info) == ["proposal_score", "score", "steps"]
        assert got == want, kw
        assert np.array_equal(info["steps"], ginfo["steps"])
        assert bool((info["proposal_score"] == 0.0).all()), kw
        for j in range(n):
            gap = abs(float(info["score"][j]) - float(ginfo["score"][j]))
            assert gap <= _score_bound(float(ginfo["score"][j]), int(ginfo["steps"][j])), (kw, j, gap)


def _check_filtered_routes(vae, device, n, n_poll):
    dec = vae.decoder
    fx = load("rollout_mid")
    z = torch.from_numpy(fx["z"][:n]).to(device)
    drawn, info = dec.sample_decode(z, generator=_gen(device, 5), return_info=True, **FILT)
    assert sorted(info) == ["proposal_score", "score", "steps"] and all(info[k].shape == (n,) for k in info)
    assert info["score"].dtype == np.float32 and info["proposal_score"].dtype == np.float32
    _check_well_formed(_ids(drawn), int(fx["V"]))
    assert [len(s) for s in drawn] == info["steps"].tolist()
    _check_self_consistent(vae, z, _ids(drawn), info["score"])           # score is the MODEL's log-probability of what was drawn
    assert bool((info["proposal_score"] <= 0.0).all())
    try:                                                                 # the per-step route: the same bits from the same generator state
        dec.batched_rollout = False
        old, oinfo = dec.sample_decode(z, generator=_gen(device, 5), return_info=True, **FILT)
    finally:
        del dec.batched_rollout
    assert drawn == old and sorted(oinfo) == sorted(info)
    for k in info:
        assert np.array_equal(info[k], oinfo[k]) and info[k].dtype == oinfo[k].dtype, k
    # poll independence: {1, 8, 100} on the first n_poll sentences (the emulator takes 80 ms a step, and a sampled sentence can run
    # to 99 words: the first two of the fixture end early)
    assert dec.rollout_poll == 8
    zp = z[:n_poll]
    base, binfo = (drawn, info) if n_poll == n else dec.sample_decode(zp, generator=_gen(device, 5), return_info=True, **FILT)
    try:
        for poll in (1, 100):
            dec.rollout_poll = poll
            d2, i2 = dec.sample_decode(zp, generator=_gen(device, 5), return_info=True, **FILT)
            assert d2 == base
            for k in binfo:
                assert np.array_equal(binfo[k], i2[k]), (poll, k)
    finally:
        del dec.rollout_poll


def _check_route_taken(vae, device, monkeypatch):
    dec = vae.decoder
    lib = _eng.backend_for(torch.device(device))
    z = torch.from_numpy(load("rollout_mid")["z"][8:9]).to(device)     # a sentence the model ends at once: cheap to sample
    calls = []
    for name in ("lv_rollout_pick_f32", "lv_rollout_pick_filtered_f32", "lv_sample_rows_f32", "lv_sample_filtered_rows_f32"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _real=real, _name=name: calls.append(_name) or _real(*a), raising=False)
    dec.sample_decode(z, generator=_gen(device, 1))
    vae.decode(z, "sample", temperature=1.0, top_k=0, top_p=1.0)
    vae.decode(z, "greedy")
    assert calls and set(calls) == {"lv_rollout_pick_f32"}               # neutral arguments: today's launches, never the filtered entry
    del calls[:]
    for kw in (dict(temperature=0.7), dict(top_k=40), dict(top_p=0.9), FILT):
        dec.sample_decode(z, generator=_gen(device, 1), **kw)
    vae.decode(z, "sample", **FILT)
    assert calls and set(calls) == {"lv_rollout_pick_filtered_f32"}
    del calls[:]
    try:
        dec.batched_rollout = False
        dec.sample_decode(z, generator=_gen(device, 1))
        assert calls and set(calls) == {"lv_sample_rows_f32"}
        del calls[:]
        dec.sample_decode(z, generator=_gen(device, 1), **FILT)
        assert calls and set(calls) == {"lv_sample_filtered_rows_f32"}
    finally:
        del dec.batched_rollout


def _check_pass_through(vae, device, tmp_path):
    z = torch.from_numpy(load("rollout_mid")["z"][:2]).to(device)
    dec = vae.decoder
    want, winfo = dec.sample_decode(z, generator=None, return_info=True, top_k=1)
    got, info = vae.decode(z, "sample", return_info=True, top_k=1)
    assert got == want and sorted(info) == ["proposal_score", "score", "steps"] and np.array_equal(info["score"], winfo["score"])
    assert vae.decode(z, "sample", top_p=1e-6, temperature=0.5) == want
    f = str(tmp_path / "prior.txt")
    generation.sample_from_prior(vae, z, "sample", f, top_k=1)
    with open(f) as fh:
        assert [line.split() for line in fh.read().splitlines()] == want
    for strategy in ("greedy", "beam"):                                  # non-neutral values belong to "sample" alone
        for kw in (dict(temperature=0.7), dict(top_k=40), dict(top_p=0.9)):
            with pytest.raises(ValueError):
                vae.decode(z, strategy, **kw)
        with pytest.raises(ValueError):
            generation.sample_from_prior(vae, z, strategy, f, top_k=3)
        with pytest.raises(ValueError):
            vae.reconstruct(None, strategy, top_p=0.5)
        with pytest.raises(ValueError):
            generation.reconstruct(vae, None, strategy, f, device, temperature=2.0)
    assert vae.decode(z[:1], "greedy", temperature=1.0, top_k=0, top_p=1.0) == dec.greedy_decode(z[:1])


def _check_value_errors(vae, device, monkeypatch):
    """Bad values raise ValueError before any launch: every launch asks engine.stream_ptr for its stream."""
    z = torch.from_numpy(load("rollout_mid")["z"][:2]).to(device)
    st = vae.decoder._stepper(torch.device(device))
    ro = vae.decoder._rollout(torch.device(device))
    launches = []
    real = _eng.stream_ptr
    monkeypatch.setattr(_eng, "stream_ptr", lambda d: launches.append(1) or real(d))
    logits, u = torch.zeros(2, 32, device=device), torch.zeros(2, device=device)
    bad = [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=INF), dict(temperature=float("nan")), dict(temperature=1e-60),
           dict(top_k=-1), dict(top_k=2.5), dict(top_k="3"), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=-0.5),
           dict(top_p=float("nan"))]
    for kw in bad:
        for call in (lambda: vae.decoder.sample_decode(z, **kw), lambda: vae.decode(z, "sample", **kw), lambda: vae.decode(z, "greedy", **kw),
                     lambda: st.sample_filtered(logits, u, **kw),
                     lambda: ro.decode(z, 1, 2, sample=True, **kw)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):                                      # the roll-out itself refuses a filter on the greedy pick
        ro.decode(z, 1, 2, sample=False, top_k=5)
    assert not launches


def test_sample_filtered_returns_the_kernels_outputs(target):
    lib, dev = target
    V = 61
    x, u, _, _ = _inputs(1, V)[0]
    out = _run_rows(lib, dev, x, u, INV_TEMPS[1], 40, float(np.float32(0.9)))
    ld = 64
    full = torch.full((1, ld), PAD)
    full[:, :V] = torch.from_numpy(x)
    full = full.to(dev)

    class _Eng(object):
        def ensure(self, device):
            self.lib = lib
    st = _eng.LSTMDecodeStepper(_Eng(), dev)
    idx, lp, lq = st.sample_filtered(full[:, :V], torch.from_numpy(u).to(dev), temperature=0.7, top_k=40, top_p=0.9)
    assert idx.dtype == torch.int64 and int(idx[0]) == int(out["idx"][0])
    assert _same(lp, torch.from_numpy(out["lp"])) and _same(lq, torch.from_numpy(out["lq"]))


def test_greedy_limit_emulated(emu_backend):
    _check_greedy_limit(_mid_vae("cpu"), "cpu", 12, (dict(top_k=1), dict(top_p=1e-6, temperature=0.7)))


def test_filtered_routes_emulated(emu_backend):
    _check_filtered_routes(_mid_vae("cpu"), "cpu", n=12, n_poll=2)


def test_route_taken_pass_through_and_value_errors_emulated(emu_backend, monkeypatch, tmp_path):
    vae = _mid_vae("cpu")
    _check_pass_through(vae, "cpu", tmp_path)
    _check_route_taken(vae, "cpu", monkeypatch)
    _check_value_errors(vae, "cpu", monkeypatch)


@pytest.mark.gpu
def test_greedy_limit_gpu(hip_device):
    _check_greedy_limit(_mid_vae(hip_device), hip_device, 48, (dict(top_k=1), dict(top_p=1e-6), dict(top_k=1, temperature=0.7),
                                                               dict(top_p=1e-6, temperature=1.9), dict(top_k=1, top_p=0.5, temperature=0.3)))


@pytest.mark.gpu
def test_filtered_routes_gpu(hip_device):
    _check_filtered_routes(_mid_vae(hip_device), hip_device, n=48, n_poll=48)


@pytest.mark.gpu
def test_route_taken_pass_through_and_value_errors_gpu(hip_device, monkeypatch, tmp_path):
    vae = _mid_vae(hip_device)
    _check_pass_through(vae, hip_device, tmp_path)
    _check_route_taken(vae, hip_device, monkeypatch)
    _check_value_errors(vae, hip_device, monkeypatch)


@pytest.mark.gpu
def test_large_model_gpu(hip_device):
    """H = 1024, V = 20001 (an odd vocabulary: the last 16-byte piece of a row holds one column), n = 4."""
    V, n = 20001, 4
    vae = build_vae(V, 128, 1024, 32, hip_device, seed=11, model_scale=0.05)
    vae.eval()
    dec = vae.decoder
    z = torch.randn(n, 32, generator=torch.Generator().manual_seed(4)).to(hip_device)
    want, ginfo = dec.greedy_decode(z, return_info=True)
    for kw in (dict(top_k=1), dict(top_p=1e-6, temperature=0.7)):
        got, info = dec.sample_decode(z, generator=_gen(hip_device, 9), return_info=True, **kw)
        assert got == want and np.array_equal(info["steps"], ginfo["steps"]) and bool((info["proposal_score"] == 0.0).all())
        for j in range(n):
            assert abs(float(info["score"][j]) - float(ginfo["score"][j])) <= _score_bound(float(ginfo["score"][j]), int(ginfo["steps"][j]))
    drawn, info = dec.sample_decode(z, generator=_gen(hip_device, 9), return_info=True, **FILT)
    _check_well_formed(_ids(drawn), V)
    _check_self_consistent(vae, z, _ids(drawn), info["score"])
    try:
        dec.batched_rollout = False
        old, oinfo = dec.sample_decode(z, generator=_gen(hip_device, 9), return_info=True, **FILT)
    finally:
        del dec.batched_rollout
    assert drawn == old
    for k in info:
        assert np.array_equal(info[k], oinfo[k]), k

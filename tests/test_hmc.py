"""Hamiltonian transitions for VAE.nll_ais / VAE.sample_from_posterior (csrc/lv_hmc.hip: lv_hmc_leap_f32; engine.hmc_leap,
engine.hmc_chain, engine.LSTMDecoderEngine.hmc_ais).  The contract every layer follows, with the float32
evaluation order of each expression, is at the top of lv_hmc.hip.

Kernel and session tests run on the emulator build and on the MI355X through one fixture.  References: float64 statements of
the contract written here (the kernel launch by launch; the session on the oracle's float64 decoder under torch autograd, with
positions, momenta and step sizes rounded to float32 where the contract stores them).

The comparison rule for sessions is test_ais.py's prefix rule with dH in place of the ratio: an accept decision is
discontinuous, so a chain is compared up to, not including, its first transition whose REFERENCE margin |log u - dH| (dH < 0)
is under TAU = 1e-3; on that prefix the flags are equal and dH, the logw trace and cur agree within the tolerance; at most 1/4 of
a case's chains may hold such a transition (a condition on seeds).
"""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from helpers import build_vae
from oracle import text_vae_oracle as O
from vae_lagging_encoder_amd import _lib
from vae_lagging_encoder_amd import engine as E
from vae_lagging_encoder_amd import evaluation as EV
from vae_lagging_encoder_amd.engine import P

TAU = 1e-3
RATIO_TOL = 2e-4
U24 = 2.0 ** -24
LOG_2PI = math.log(2 * math.pi)
POISON = 7777.0
IPOISON = 7777
INF = float("inf")


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def target(request):
    if request.param == "emu":
        request.getfixturevalue("emu_backend")
        dev = torch.device("cpu")
    else:
        dev = request.getfixturevalue("hip_device")
    return E.backend_for(dev), dev


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _f32(v):
    return float(np.float32(v))


def _drift(p, e, z):
    """The float32 two-rounding drift (CPU tensors): the product e * p is rounded, then the sum with z."""
    t = p.float() * e.float()
    return t + z.float()


def _prior64(z):
    z = z.double()
    return -0.5 * (z * z).sum(-1) - 0.5 * z.shape[-1] * LOG_2PI


def _logq0_64(z, mu0, lv0):
    """log N(z; mu0, diag exp(lv0)) in float64, z [B][C][nz], mu0 / lv0 [B][nz]; None: the prior."""
    if mu0 is None:
        return _prior64(z)
    mu, lv = mu0.double().unsqueeze(1), lv0.double().unsqueeze(1)
    dev = z.double() - mu
    return -0.5 * (dev * dev * torch.exp(-lv)).sum(-1) - 0.5 * (z.shape[-1] * LOG_2PI + lv.sum(-1))


def _g64(z, lq, rec, mu0):
    return -rec.double() if mu0 is None else (_prior64(z) - lq) + (-rec.double())


def _grad_u64(z, d, bf, mu0, lv0, dabs=None):
    """grad U_beta in float64, z / d [B][C][nz]; also the sum of the magnitudes of the terms it combines (dabs: that of d's own
    summands, |d| if it has none)."""
    z, d = z.double(), d.double()
    dabs = d.abs() if dabs is None else dabs.double()
    if mu0 is None:
        return z + bf * d, z.abs() + bf * dabs
    a = (z - mu0.double().unsqueeze(1)) * torch.exp(-lv0.double()).unsqueeze(1)
    return a + bf * ((z - a) + d), a.abs() + bf * (z.abs() + a.abs() + dabs)


def _margin(dh, u):
    """|log u - dH| where dH < 0, inf elsewhere (float64; u = 0 gives inf: such a draw never accepts a dH < 0)."""
    dh, u = dh.double(), u.double()
    m = (torch.log(u) - dh).abs()
    return torch.where(dh < 0, m, torch.full_like(m, INF))


# ---- 1. lv_hmc_leap_f32 against the float64 statement --------------------------------------------------------------------------
ROLES = ("plain", "nan", "u0", "u_max", "inf")
INIT, MID, LAST = E.HMC_INIT, E.HMC_MID, E.HMC_LAST
FIXED = (1.0, 1.0, 0.0, INF)
ADAPT = (_f32(math.exp(0.02 * 0.35)), _f32(math.exp(-0.02 * 0.65)), 0.05, 0.1)      # eps starts in [0.02, 0.2): both clamps hit


def _leap_case(lib, dev, rows, C, nz, parts, enc, mode, more, role, adapt, outs, seed):
    """One launch on poisoned, over-allocated buffers; asserts everything.

    Bounds: counted operations x 2^-24 x the sum of the absolute terms of the quantity.  Counts: a sum over nz terms costs at
    most ceil(nz / 64) lane adds and 6 butterfly adds, its terms up to 4 operations (expf within 2 ulp counted as 2): K_SUM = nz
    + 12 covers it for any nz.  d_j: `parts` adds.  grad_j: 6 operations (subtract, multiply by expf(-lv) (3), subtract, add,
    multiply, add) on top of d_j.  A kick: 2 more (h * grad, the subtraction); the half step 0.5f * eps is exact.  So a momentum
    coordinate carries K_P = parts + 10 roundings of |p_j| + h * A_j, A_j the magnitude sum of grad_j's terms.  K: each p_j^2
    inherits 2 |p_j| dp_j + dp_j^2, plus K_SUM roundings of K.  dH: log q0(z) and g(z) as in test_ais.py (K_SUM roundings of their
    magnitude sums), K1 as above, and 6 more roundings (two multiply-adds, three differences / sums) of the magnitude sum of its
    six terms."""
    gen = torch.Generator().manual_seed(seed)
    B, pad = rows // C, 2
    beta, beta_next = 0.2 + 0.7 * float(torch.rand(1, generator=gen, dtype=torch.float64)), 0.93
    dbeta = beta_next - beta
    bf, bn = _f32(beta), _f32(beta_next)
    up, down, emin, emax = adapt
    mu0 = (0.5 * torch.randn(B, nz, generator=gen)) if enc else None
    lv0 = (0.3 * torch.randn(B, nz, generator=gen) - 0.5) if enc else None
    e_in = 0.02 + 0.18 * torch.rand(rows, generator=gen)
    cur = torch.randn(rows, nz, generator=gen)
    pos = cur + 0.2 * torch.randn(rows, nz, generator=gen)
    mom = torch.randn(rows, nz, generator=gen)
    mom_next = torch.randn(rows, nz, generator=gen)
    k0_in = 0.5 * (torch.randn(rows, nz, generator=gen) ** 2).sum(-1)
    d_cur = 2.0 * torch.randn(rows, nz, generator=gen)
    dz = 2.0 * torch.randn(parts, rows, nz, generator=gen)
    g_cur = torch.randn(rows, generator=gen) * 5 - 30
    rec_cur = torch.rand(rows, generator=gen) * 30
    lq_cur = _logq0_64(cur.view(B, C, nz), mu0, lv0).view(rows).float()
    logw_in = torch.randn(rows, generator=gen, dtype=torch.float64) * 3 - 10
    counts = torch.randint(0, 50, (rows,), generator=gen, dtype=torch.int32)
    target_dh = torch.rand(rows, generator=gen, dtype=torch.float64) * 5 - 3              # in [-3, 2)
    want_accept = torch.rand(rows, generator=gen) < 0.5
    special = seed % rows
    if role == "u_max":
        target_dh[special] = 0.25
    elif role == "u0":
        target_dh[special] = -200.0
    K_SUM, K_P = (nz + 12) * U24, (parts + 10) * U24
    v3 = lambda t: t.view(B, C, nz)
    d_at = dz.double().sum(0)                                                           # d(pos) in float64
    e64 = e_in.double().unsqueeze(1)
    # the closing half kick and K1 (mode last), in float64 from the operands the kernel gets
    gr, A = (t.view(rows, nz) for t in _grad_u64(v3(pos), v3(d_at), bf, mu0, lv0, v3(dz.double().abs().sum(0))))
    h = (0.5 if mode == LAST else 1.0) * e64
    p_kick = mom.double() - h * gr
    dp = K_P * (mom.double().abs() + h * A)
    K1 = 0.5 * (p_kick ** 2).sum(-1)
    b_K1 = (p_kick.abs() * dp + dp ** 2).sum(-1) + K_SUM * K1
    lq_at = _logq0_64(v3(pos), mu0, lv0).view(rows)
    pz_at = _prior64(pos)
    # rec such that dH lands on its target: dH = (lq_at + b g_at) - (lq_cur + b g_cur) + (K0 - K1), g_at = (pz_at - lq_at) - rec
    g_at_want = (target_dh - (k0_in.double() - K1) + lq_cur.double() + bf * g_cur.double() - lq_at) / bf
    rec = (-(g_at_want - ((pz_at - lq_at) if enc else 0.0))).float()
    if role == "nan":
        rec[special] = float("nan")
    elif role == "inf":
        rec[special] = INF
    g_at = _g64(v3(pos), lq_at.view(B, C), rec.view(B, C), mu0).view(rows)
    dh64 = ((lq_at + bf * g_at) - (lq_cur.double() + bf * g_cur.double())) + (k0_in.double() - K1)
    quad = 0.5 * ((v3(pos).double() - (mu0.double().unsqueeze(1) if enc else 0.0)) ** 2
                  * (torch.exp(-lv0.double()).unsqueeze(1) if enc else 1.0)).sum(-1).view(rows)
    const = 0.5 * nz * LOG_2PI + (0.5 * lv0.double().abs().sum(-1).repeat_interleave(C) if enc else 0.0)
    mag_lq = quad + const
    mag_g = rec.double().abs() + ((0.5 * (pos.double() ** 2).sum(-1) + 0.5 * nz * LOG_2PI + mag_lq) if enc else 0.0)
    b_lq, b_g = K_SUM * mag_lq, (K_SUM * mag_g if enc else torch.zeros(rows, dtype=torch.float64))
    bound = (b_lq + bf * b_g + b_K1
             + 6 * U24 * (lq_at.abs() + bf * g_at.abs() + lq_cur.double().abs() + bf * g_cur.double().abs() + k0_in.double() + K1))
    pacc = torch.exp(torch.clamp(dh64, max=0.0))
    can_reject = pacc < 0.9
    accept = torch.where(can_reject, want_accept, torch.ones_like(want_accept))
    u = torch.where(accept, 0.5 * pacc, pacc + 0.5 * (1 - pacc)).float()
    ok = torch.ones(rows, dtype=torch.bool)
    if role == "u_max":
        u[special], accept[special] = 1.0 - U24, True
    elif role in ("u0", "nan", "inf"):
        u[special], accept[special] = 0.0, False
        ok[special] = role == "u0"
    if mode == LAST and bool(ok.any()):                    # every margin is at least twice the bound on dH, by construction
        assert bool((_margin(dh64[ok], u[ok]) >= 2 * bound[ok]).all()) and float(_margin(dh64[ok], u[ok]).min()) > 0.05
        assert float(bound[ok].max()) < 0.025

    def dv(t, fill):
        full = torch.full((t.shape[0] + pad,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
        full[:t.shape[0]] = t
        return full.to(dev)
    d = dict(rec=dv(rec, POISON), dz=dz.contiguous().to(dev), pos=dv(pos, POISON), mom=dv(mom, POISON), k0=dv(k0_in, POISON),
             cur=dv(cur, POISON), g=dv(g_cur, POISON), lq=dv(lq_cur, POISON), rc=dv(rec_cur, POISON), dc=dv(d_cur, POISON),
             lw=dv(logw_in, POISON), cnt=dv(counts, IPOISON), eps=dv(e_in, POISON), u=dv(u, POISON), mn=dv(mom_next, POISON),
             dh=torch.full((rows + pad,), POISON).to(dev), flag=torch.full((rows + pad,), IPOISON, dtype=torch.int32).to(dev),
             lwn=torch.full((rows + pad,), POISON, dtype=torch.float64).to(dev), keep=torch.full((rows + pad, nz), POISON).to(dev))
    d_mu, d_lv = (mu0.to(dev), lv0.to(dev)) if enc else (None, None)
    lib.lv_hmc_leap_f32(P(d["rec"]), P(d["dz"]), parts, P(d["pos"]), P(d["mom"]), P(d["k0"]), P(d["cur"]), P(d["g"]), P(d["lq"]),
                        P(d["rc"]), P(d["dc"]), P(d["lw"]), P(d["cnt"]), P(d["eps"]), P(d["u"]) if mode == LAST else None,
                        P(d["mn"]) if more else None, beta, beta_next, dbeta, P(d_mu), P(d_lv), rows, C, nz, 3, mode, up, down, emin,
                        emax, P(d["dh"]) if outs else None, P(d["flag"]) if outs else None, P(d["lwn"]) if outs else None,
                        P(d["keep"]) if outs else None, E.stream_ptr(dev))
    got = {k_: v.cpu() for k_, v in d.items()}
    for k_ in ("pos", "mom", "k0", "cur", "g", "lq", "rc", "dc", "lw", "eps", "dh", "lwn", "keep"):   # guard rows keep their poison
        assert bool((got[k_][rows:] == POISON).all()), k_
    assert bool((got["cnt"][rows:] == IPOISON).all()) and bool((got["flag"][rows:] == IPOISON).all())
    same_in = lambda k_, t: _same(got[k_][:rows], t)
    if mode == MID:
        for k_, t in (("cur", cur), ("g", g_cur), ("lq", lq_cur), ("rc", rec_cur), ("dc", d_cur), ("lw", logw_in), ("cnt", counts),
                      ("eps", e_in), ("k0", k0_in)):
            assert same_in(k_, t), k_
        assert bool((got["dh"] == POISON).all()) and bool((got["flag"] == IPOISON).all()) and bool((got["keep"] == POISON).all())
        assert bool(((got["mom"][:rows].double() - p_kick).abs() <= dp).all())
        assert same_in("pos", _drift(got["mom"][:rows], e_in.unsqueeze(1), pos))          # the drift, from the kernel's own momentum
        return
    gg, gl = got["g"][:rows], got["lq"][:rows]
    if mode == INIT:
        sel = torch.ones(rows, dtype=torch.bool)
        assert bool((got["cnt"][:rows] == 0).all()) and same_in("eps", e_in)
        assert bool((got["dh"] == POISON).all()) and bool((got["flag"] == IPOISON).all())
        base, e_new = torch.zeros(rows, dtype=torch.float64), e_in
        fin = torch.isfinite(rec)
    else:
        sel = accept
        assert torch.equal(got["flag"][:rows] != 0, accept) if outs else bool((got["flag"] == IPOISON).all()), role   # exact
        assert torch.equal(got["cnt"][:rows], counts + accept.to(torch.int32))
        if outs:
            assert bool(((got["dh"][:rows].double() - dh64).abs()[ok] <= bound[ok]).all())
            if role == "nan":
                assert math.isnan(float(got["dh"][special]))
            if role == "inf":
                assert not float(got["dh"][special]) > -INF
        e_new = torch.minimum(torch.maximum(e_in * torch.where(accept, torch.tensor(up), torch.tensor(down)), torch.tensor(emin)),
                              torch.tensor(emax))
        assert same_in("eps", e_new)                                                     # float32 by value, bit for bit
        if adapt is ADAPT and rows > 3:
            assert bool((e_new == emin).any()) and bool((e_new == emax).any()), "both clamps"
        base = logw_in
        fin = torch.ones(rows, dtype=torch.bool)
    rej = ~sel
    new_cur = torch.where(sel.unsqueeze(1), pos, cur)
    assert same_in("cur", new_cur)                                                       # selected, bit for bit
    assert _same(gg[rej], g_cur[rej]) and _same(gl[rej], lq_cur[rej])                    # a rejected row's state is untouched
    assert _same(got["rc"][:rows][rej], rec_cur[rej]) and _same(got["dc"][:rows][rej], d_cur[rej])
    assert _same(got["rc"][:rows][sel], rec[sel])
    if mode == LAST:
        assert bool(torch.isfinite(gg).all()) and bool(torch.isfinite(gl).all())         # ... a NaN or infinite score included
    if not enc:
        assert _same(gg[sel], -rec[sel])                                                 # g is the conditional log-likelihood, bit for bit
    okf = sel & fin
    assert bool(((gg.double() - g_at).abs()[okf] <= b_g[okf]).all()) and bool(((gl.double() - lq_at).abs()[sel] <= b_lq[sel]).all())
    d_new = got["dc"][:rows]
    if parts == 1:
        assert _same(d_new[sel], dz[0][sel])
    else:
        assert bool(((d_new.double() - d_at).abs()[sel] <= (parts * U24 * dz.double().abs().sum(0))[sel]).all())
    if outs:                                                                             # (init too: z_0 is the selected state)
        assert same_in("keep", new_cur)
    else:
        assert bool((got["keep"] == POISON).all())
    if not more:
        assert same_in("pos", pos) and same_in("mom", mom) and same_in("k0", k0_in) and bool((got["lwn"] == POISON).all())
        assert same_in("lw", base)
        return
    want = base + dbeta * gg.double()                                                    # the next increment, in float64
    wf = torch.isfinite(want)
    assert bool(((got["lw"][:rows] - want).abs()[wf] <= 1e-12 * want.abs().clamp(min=1.0)[wf]).all())
    assert bool((torch.isnan(got["lw"][:rows]) == torch.isnan(want)).all())
    if outs:
        assert _same(got["lwn"][:rows], got["lw"][:rows])
    # the opening of the next transition from the SELECTED state: K0, the half kick at beta_next from the kernel's own d_cur, drift
    K0n = 0.5 * (mom_next.double() ** 2).sum(-1)
    assert bool(((got["k0"][:rows].double() - K0n).abs() <= K_SUM * K0n).all())
    gr2, A2 = _grad_u64(v3(new_cur), v3(d_new), bn, mu0, lv0)
    h2 = 0.5 * e_new.double().unsqueeze(1)
    p2 = mom_next.double() - h2 * gr2.view(rows, nz)
    dp2 = (10 * U24) * (mom_next.double().abs() + h2 * A2.view(rows, nz))
    assert bool(((got["mom"][:rows].double() - p2).abs() <= dp2).all())
    assert same_in("pos", _drift(got["mom"][:rows], e_new.unsqueeze(1), new_cur))


@pytest.mark.parametrize("enc", [False, True], ids=["prior", "encoder"])
@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("nz", [1, 5, 32, 67])
@pytest.mark.parametrize("rows,C", [(1, 1), (3, 3), (70, 10)])
def test_hmc_leap_against_float64_statement(target, rows, C, nz, parts, enc):
    lib, dev = target
    seed = 1000 * rows + 10 * nz + parts + (500 if enc else 0)
    for i, role in enumerate(ROLES):                       # last with a successor: every role, adaptation off and on
        _leap_case(lib, dev, rows, C, nz, parts, enc, LAST, True, role, ADAPT if i % 2 else FIXED, True, seed + i)
    _leap_case(lib, dev, rows, C, nz, parts, enc, LAST, True, "plain", ADAPT, False, seed + 5)       # optional outputs absent
    _leap_case(lib, dev, rows, C, nz, parts, enc, LAST, False, "plain", ADAPT, True, seed + 6)       # last without a successor
    _leap_case(lib, dev, rows, C, nz, parts, enc, LAST, False, "inf", FIXED, False, seed + 7)
    _leap_case(lib, dev, rows, C, nz, parts, enc, MID, False, "plain", FIXED, True, seed + 8)
    _leap_case(lib, dev, rows, C, nz, parts, enc, INIT, True, "plain", FIXED, True, seed + 9)
    _leap_case(lib, dev, rows, C, nz, parts, enc, INIT, True, "nan", FIXED, False, seed + 10)
    _leap_case(lib, dev, rows, C, nz, parts, enc, INIT, False, "plain", FIXED, True, seed + 11)


# ---- 2. argument checks ----------------------------------------------------------------------------------------------------------
def test_hmc_leap_bad_arguments_write_nothing(target):
    lib, dev = target
    raw = lib._raw_lv_hmc_leap_f32
    B, C, nz, parts = 2, 3, 4, 2
    rows = B * C
    shapes = dict(rec=(rows,), dz=(parts, rows, nz), pos=(rows, nz), mom=(rows, nz), k0=(rows,), cur=(rows, nz), g=(rows,), lq=(rows,),
                  rc=(rows,), dc=(rows, nz), eps=(rows,), u=(rows,), mn=(rows, nz), mu=(B, nz), lv=(B, nz), dh=(rows,), keep=(rows, nz))
    t = {k: torch.full(s, POISON, device=dev) for k, s in shapes.items()}
    t["lw"] = torch.full((rows + 1,), POISON, dtype=torch.float64, device=dev)
    t["lwn"] = torch.full((rows + 1,), POISON, dtype=torch.float64, device=dev)
    t["cnt"] = torch.full((rows,), IPOISON, dtype=torch.int32, device=dev)
    t["flag"] = torch.full((rows,), IPOISON, dtype=torch.int32, device=dev)
    odd = lambda k: ctypes.c_void_p(t[k].data_ptr() + 4)

    def call(**kw):
        a = {k: P(v) for k, v in t.items()}
        a.update(parts=parts, rows=rows, C=C, nz=nz, L=3, mode=LAST, up=1.0, down=1.0, emin=0.0, emax=INF)
        a.update(kw)
        return raw(a["rec"], a["dz"], a["parts"], a["pos"], a["mom"], a["k0"], a["cur"], a["g"], a["lq"], a["rc"], a["dc"], a["lw"],
                   a["cnt"], a["eps"], a["u"], a["mn"], 0.5, 0.6, 0.1, a["mu"], a["lv"], a["rows"], a["C"], a["nz"], a["L"], a["mode"],
                   a["up"], a["down"], a["emin"], a["emax"], a["dh"], a["flag"], a["lwn"], a["keep"], E.stream_ptr(dev))
    for k in ("rec", "dz", "pos", "mom", "k0", "cur", "g", "lq", "rc", "dc", "lw", "cnt", "eps", "u", "mu", "lv"):
        assert call(**{k: None}) == -1, k                  # (mu0 without lv0 and the reverse included)
    for bad in (dict(mode=3), dict(mode=-1), dict(up=0.0), dict(down=-1.0), dict(up=float("nan")), dict(emin=-0.1),
                dict(emin=0.2, emax=0.1)):
        assert call(**bad) == -1, bad
    for bad in (dict(rows=0), dict(C=0), dict(rows=rows - 1), dict(nz=0), dict(L=0), dict(parts=0), dict(mode=MID, L=1)):
        assert call(**bad) == -2, bad
    assert call(lw=odd("lw")) == -3 and call(lwn=odd("lwn")) == -3
    for k, v in t.items():
        assert bool((v == (IPOISON if v.dtype == torch.int32 else POISON)).all()), k


# ---- the float64 statement of a session ---------------------------------------------------------------------------------------
def _params(V, ni, H, nz, seed):
    return O.random_params(V, ni, H, nz, seed=seed, scale=0.3, emb_scale=0.5)


def _score64(Pm, x):
    """rec and d rec / d z of the oracle's float64 decoder under torch autograd, at float32 points z [B][C][nz]."""
    P64 = {k: v.double() for k, v in Pm.items()}

    def score(z):
        zz = z.double().requires_grad_(True)
        rec = O.decoder_reconstruct_error(P64, x, zz)
        d, = torch.autograd.grad(rec.sum(), zz)
        return rec.detach(), d
    return score


def _hmc64(score, z0, mom, u, beta, L, step, adapt=None, mu0=None, lv0=None, until=None):
    """The contract with float64 densities and gradients; positions, the momentum after every stored kick and the step sizes are
    rounded to float32 where the contract stores them (the closing half kick is not stored).  adapt: (up, down, min, max)."""
    N = mom.shape[0]
    until = N if until is None else until
    cur = z0.clone().float()
    rec, d = score(cur)
    lq = _logq0_64(cur, mu0, lv0)
    g = _g64(cur, lq, rec, mu0)
    logw = torch.zeros_like(g)
    e = torch.full(g.shape, step, dtype=torch.float32)
    dhs, flags, trace, curs, es = [], [], [], [], []
    for it in range(N):
        bf = _f32(beta[it + 1])
        logw = logw + (beta[it + 1] - beta[it]) * g
        trace.append(logw.clone())
        p = mom[it].float()
        K0 = 0.5 * (p.double() ** 2).sum(-1)
        e64 = e.double().unsqueeze(-1)
        p = (p.double() - 0.5 * e64 * _grad_u64(cur, d, bf, mu0, lv0)[0]).float()
        z = cur
        for l in range(1, L + 1):
            z = _drift(p, e.unsqueeze(-1), z)
            rec_z, d_z = score(z)
            p = p.double() - (1.0 if l < L else 0.5) * e64 * _grad_u64(z, d_z, bf, mu0, lv0)[0]
            if l < L:
                p = p.float()
        lq_z = _logq0_64(z, mu0, lv0)
        g_z = _g64(z, lq_z, rec_z, mu0)
        dh = ((lq_z + bf * g_z) - (lq + bf * g)) + (K0 - 0.5 * (p ** 2).sum(-1))
        acc = (dh >= 0) | (u[it].double() < dh.exp())
        cur = torch.where(acc.unsqueeze(-1), z, cur)
        d = torch.where(acc.unsqueeze(-1), d_z, d)
        g, lq = torch.where(acc, g_z, g), torch.where(acc, lq_z, lq)
        if adapt is not None and it < until:
            e = torch.minimum(torch.maximum(e * torch.where(acc, torch.tensor(adapt[0]), torch.tensor(adapt[1])),
                                            torch.tensor(adapt[2])), torch.tensor(adapt[3]))
        dhs.append(dh)
        flags.append(acc)
        curs.append(cur.clone())
        es.append(e.clone())
    dhs, flags = torch.stack(dhs), torch.stack(flags)
    return {"logw": logw, "cur": cur, "dh": dhs, "flags": flags, "trace": torch.stack(trace), "margin": _margin(dhs, u),
            "curs": torch.stack(curs), "eps": e, "eps_trace": torch.stack(es)}


def _session_tol():
    """The larger of RATIO_TOL and 4 x the largest float32-vs-float64 deviation of the reference's own two runs on the compared
    prefix (tests/golden/hmc_small.npz, `dev`; 4 x: test_svi_refine.py's rule for dependent steps).  Recorded: 5.0e-6 (dH),
    1.1e-6 (logw), 5.3e-7 (cur) at most, so the bound is RATIO_TOL."""
    from helpers import load
    fx = load("hmc_small")
    worst = max(float(fx[c + "/dev"].max()) for c in ("nz1", "enc", "adapt"))
    return max(RATIO_TOL, 4.0 * worst)


def _check_prefix(name, dh, flags, trace, cur, ref_dh, ref_flag, ref_trace, ref_cur, margin, tol, cap=True):
    """The comparison rule on every chain ([n][B][C] arrays, cur [B][C][nz]); returns the chains compared to the end."""
    n, B, C = ref_dh.shape
    dh, flags, trace, cur = dh.cpu().double(), flags.cpu(), trace.cpu().double(), cur.cpu().double()
    worst_r = worst_w = worst_c = 0.0
    full = []
    for b in range(B):
        for c in range(C):
            low = (margin[:, b, c] < TAU).nonzero()
            stop = int(low[0]) if low.numel() else n
            assert torch.equal(flags[:stop, b, c] != 0, ref_flag[:stop, b, c] != 0), (name, b, c)
            if stop:
                worst_r = max(worst_r, float((dh[:stop, b, c] - ref_dh[:stop, b, c].double()).abs().max()))
            upto = min(stop + 1, n)                    # the increment of transition `stop` uses a state the earlier decisions settled
            worst_w = max(worst_w, float((trace[:upto, b, c] - ref_trace[:upto, b, c].double()).abs().max()))
            if stop == n:
                full.append((b, c))
                worst_c = max(worst_c, float((cur[b, c] - ref_cur[b, c].double()).abs().max()))
    print("%s: %d of %d chains compared to the end, largest |dH - dH_ref| %.3e, |logw - logw_ref| %.3e, |cur - cur_ref| %.3e (bound %.1e)"
          % (name, len(full), B * C, worst_r, worst_w, worst_c, tol))
    assert worst_r <= tol and worst_w <= tol and worst_c <= tol, (name, worst_r, worst_w, worst_c)
    if cap:
        assert 4 * (B * C - len(full)) <= B * C, "%s: more than 1/4 of the chains are marginal -- pick another seed, not another TAU" % name
    return full


# V, ni, H, nz, B, T, C, L, N, init, step, adapt (target, rate), step_bounds, seed
SESSION_CASES = {
    "prior": (53, 8, 16, 4, 3, 6, 4, 3, 8, "prior", 1.2, None, (1e-4, 0.5), 300),
    "encoder": (53, 8, 16, 4, 3, 6, 4, 3, 8, "encoder", 1.5, None, (1e-4, 0.5), 310),
    "nz1": (53, 8, 16, 1, 3, 6, 4, 3, 8, "prior", 1.3, None, (1e-4, 0.5), 320),
    "adapt": (53, 8, 16, 4, 3, 6, 4, 3, 8, "prior", 1.3, (0.65, 0.1), (0.4, 1.4), 330),
}
_session_cache = {}


def _factors(adapt, bounds):
    if adapt is None:
        return None
    target, rate = adapt
    return (_f32(math.exp(rate * (1.0 - target))), _f32(math.exp(-rate * target)), _f32(bounds[0]), _f32(bounds[1]))


def _session_case(name):
    """Model, data, noise and the float64 statement of a case -- computed once (q0 of the encoder case: the oracle's encoder in
    float32, which the drop-in's encode_stats is held to 1e-4 of elsewhere; the device run gets ITS mu0 / lv0, the statement too)."""
    if name in _session_cache:
        return _session_cache[name]
    from vae_lagging_encoder_amd.modules import VAE
    V, ni, H, nz, B, T, C, L, N, init, step, adapt, bounds, seed = SESSION_CASES[name]
    Pm = _params(V, ni, H, nz, seed)
    x = O.synthetic_batch(B, T, V, seed=seed + 1)
    gen = torch.Generator().manual_seed(seed + 2)
    z0 = torch.randn(B, C, nz, generator=gen)
    mu0 = lv0 = None
    if init == "encoder":
        with torch.no_grad():
            mu0, lv0 = (t.contiguous() for t in O.encoder_forward(Pm, x))
        z0 = mu0.unsqueeze(1) + torch.exp(0.5 * lv0).unsqueeze(1) * z0
    mom, u = torch.randn(N, B, C, nz, generator=gen), torch.rand(N, B, C, generator=gen)
    beta = VAE.ais_schedule("sigmoid", N)
    c = dict(P=Pm, x=x, z0=z0, mom=mom, u=u, beta=beta, mu0=mu0, lv0=lv0, dims=(V, ni, H, nz), B=B, C=C, L=L, N=N, init=init, step=step,
             adapt=adapt, bounds=bounds)
    c["ref"] = _hmc64(_score64(Pm, x), z0, mom, u, beta, L, step, _factors(adapt, bounds), mu0, lv0)
    _session_cache[name] = c
    return c


@pytest.mark.parametrize("name", sorted(SESSION_CASES))
def test_session_seeds_meet_the_cap(name):
    """The seeds' own check, on the CPU: at most 1/4 of a case's chains hold a transition under TAU in the float64 statement, and
    the case exercises both decisions (and, with adaptation, moves the step size)."""
    c = _session_case(name)
    ref = c["ref"]
    marginal = int((ref["margin"].amin(dim=0) < TAU).sum())
    rate = float(ref["flags"].float().mean())
    print("%s: acceptance %.3f, %d of %d chains marginal, final eps %s" % (name, rate, marginal, c["B"] * c["C"], ref["eps"].unique().tolist()))
    assert 4 * marginal <= c["B"] * c["C"] and 0.3 < rate < 1.0
    if c["adapt"] is not None:
        assert ref["eps"].unique().numel() > 1


def _run_nll_ais(vae, c, dev, fused, **kw):
    vae.fused_hmc = fused
    try:
        noise = (c["z0"].to(dev), c["mom"].to(dev), c["u"].to(dev))
        return vae.nll_ais(c["x"].to(dev), chains=c["C"], temps=c["N"], schedule=c["beta"], init=c["init"], noise=noise, transition="hmc",
                           leapfrog=c["L"], step_size=c["step"], adapt=c["adapt"], step_bounds=c["bounds"], return_info=True, **kw)
    finally:
        del vae.fused_hmc


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
@pytest.mark.parametrize("name", sorted(SESSION_CASES))
def test_session_against_float64_statement(target, name, fused):
    _, dev = target
    c = _session_case(name)
    vae = build_vae(*c["dims"], dev, params=c["P"])
    ref = c["ref"]
    if c["init"] == "encoder":                             # the statement on the q0 the device run uses: its own encode_stats
        vae.eval()
        with torch.no_grad():
            mu0, lv0 = (t.float().cpu() for t in vae.encode_stats(c["x"].to(dev)))
        assert float((mu0 - c["mu0"]).abs().max()) <= 1e-4 and float((lv0 - c["lv0"]).abs().max()) <= 1e-4
        ref = _hmc64(_score64(c["P"], c["x"]), c["z0"], c["mom"], c["u"], c["beta"], c["L"], c["step"], None, mu0, lv0)
        vae.train()
    nll, info = _run_nll_ais(vae, c, dev, fused)
    assert info["route"] == ("hmc-fused" if fused else "hmc-generic") and info["leapfrog"] == c["L"] and info["iterations"] == c["N"]
    full = _check_prefix("%s/%s" % (name, info["route"]), info["ratios"], info["accepts"], info["logw_trace"], info["cur"], ref["dh"],
                         ref["flags"], ref["trace"], ref["cur"], ref["margin"], _session_tol())
    for b, ch in full:
        assert abs(float(info["logw"][b, ch]) - float(ref["logw"][b, ch])) <= _session_tol()
        assert _same(info["step_size"][b, ch], ref["eps"][b, ch])                     # float32 by value: the same factors, the same flags
    assert _same(info["logw"], info["logw_trace"][-1]) and tuple(nll.shape) == (c["B"],) and nll.dtype == torch.float32


# ---- 5. the drop-in against the reference's recorded chains -------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
@pytest.mark.parametrize("case", ["nz1", "enc", "adapt"])
def test_dropin_against_reference_fixture(target, case, fused):
    from helpers import load
    from vae_lagging_encoder_amd.modules import VAE
    _, dev = target
    fx = load("hmc_small")
    V, ni, H, nz = (int(v) for v in fx[case + "/dims"])
    N, L, C = (int(v) for v in fx[case + "/shape"])
    vae = build_vae(V, ni, H, nz, dev, params={k: torch.from_numpy(fx[case + "/param/" + k]) for k in O.ALL_KEYS})
    t = lambda k: torch.from_numpy(fx[case + "/" + k])
    assert float(fx[case + "/tau"]) == TAU
    beta = fx[case + "/beta"].tolist()
    ours = VAE.ais_schedule("sigmoid", N)
    assert max(abs(a - b) for a, b in zip(ours, beta)) <= 1e-15
    margin = _margin(t("f64/dh"), t("u"))
    B = t("x").shape[0]
    assert 4 * int((margin.amin(dim=0) < TAU).sum()) <= B * C
    adapt = tuple(fx[case + "/adapt"].tolist()) or None
    c = dict(z0=t("z0"), mom=t("mom"), u=t("u"), x=t("x"), C=C, N=N, beta=beta, init=str(fx[case + "/init"]), L=L,
             step=float(fx[case + "/step_size"]), adapt=adapt, bounds=tuple(fx[case + "/step_bounds"].tolist()))
    nll, info = _run_nll_ais(vae, c, dev, fused)
    assert info["route"] == ("hmc-fused" if fused else "hmc-generic")
    full = _check_prefix("fixture %s/%s" % (case, info["route"]), info["ratios"], info["accepts"], info["logw_trace"], info["cur"],
                         t("f32/dh"), t("f32/accept"), t("f32/logw_trace"), t("f32/cur"), margin, _session_tol(), cap=False)
    for b, ch in full:
        assert abs(float(info["logw"][b, ch]) - float(t("f32/logw")[b, ch])) <= _session_tol()
        assert _same(info["step_size"][b, ch], t("f32/eps")[b, ch])
    if len(full) == B * C:
        want = torch.logsumexp(t("f32/logw"), dim=1) - math.log(C)
        assert float((nll.double().cpu() + want).abs().max()) <= _session_tol() + 1e-5   # (+ the float32 of the returned value)


# ---- 3. identities that need no tolerance ---------------------------------------------------------------------------------------
def _identity_model(dev, C=5):
    V, ni, H, nz, B, T = 31, 6, 12, 3, 2, 5
    vae = build_vae(V, ni, H, nz, dev, params=_params(V, ni, H, nz, 9))
    vae.eval()
    x = O.synthetic_batch(B, T, V, seed=10).to(dev)
    return vae, x, torch.Generator().manual_seed(11), (B, C, nz)


def _noise(gen, N, B, C, nz, dev):
    return (torch.randn(B, C, nz, generator=gen).to(dev), torch.randn(N, B, C, nz, generator=gen).to(dev),
            torch.rand(N, B, C, generator=gen).to(dev))


HMC_KEYS = ("logw", "ratios", "accepts", "logw_trace", "step_size", "cur", "accept_rate")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
def test_one_temperature_from_the_prior_is_the_conditional_log_likelihood(target, fused):
    """The existing AIS identity: temps = 1 from the prior gives logw == (double) log p(x|z0), bit for bit -- g is -rec itself."""
    _, dev = target
    vae, x, gen, (B, C, nz) = _identity_model(dev)
    noise = _noise(gen, 1, B, C, nz, dev)
    vae.fused_hmc = fused
    nll, info = vae.nll_ais(x, chains=C, temps=1, noise=noise, transition="hmc", leapfrog=2, step_size=0.2, return_info=True)
    assert info["route"] == ("hmc-fused" if fused else "hmc-generic") and info["logw"].dtype == torch.float64
    with torch.no_grad():
        cond = -vae.decoder.reconstruct_error(x, noise[0])
    assert _same(info["logw"], cond.double())
    assert tuple(nll.shape) == (B,) and nll.dtype == torch.float32 and not nll.requires_grad


def test_zero_momentum_at_the_mode_of_q0_with_a_constant_likelihood_stays_put(target):
    """A decoder that ignores z (trans_linear and the z columns of W_ih zeroed) has d = 0 exactly; at the prior's mode grad U_beta
    is 0 for every beta, a zero momentum stays zero and cur never moves: dH = 0, every transition accepts.  (With the encoder as
    q0 the annealed target q0^(1 - beta) p(z)^beta has its mode between mu0 and 0, so mu0 is no fixed point unless it is 0.)"""
    _, dev = target
    vae, x, gen, (B, C, nz) = _identity_model(dev)
    ni = 6
    with torch.no_grad():
        vae.decoder.trans_linear.weight.zero_()
        vae.decoder.lstm.weight_ih_l0[:, ni:].zero_()
    N = 4
    z0 = torch.zeros(B, C, nz, device=dev)
    noise = (z0, torch.zeros(N, B, C, nz, device=dev), torch.rand(N, B, C, generator=gen).to(dev))
    for fused in (True, False):
        vae.fused_hmc = fused
        _, info = vae.nll_ais(x, chains=C, temps=N, noise=noise, transition="hmc", leapfrog=3, step_size=0.7, return_info=True)
        assert _same(info["cur"], z0) and bool((info["ratios"] == 0).all()) and bool((info["accepts"] == 1).all())


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
def test_reruns_neighbours_and_noise_chunks_are_bit_identical(target, fused):
    _, dev = target
    vae, x, gen, (B, C, nz) = _identity_model(dev, C=10)
    N = 5
    noise = _noise(gen, N, B, C, nz, dev)
    vae.fused_hmc = fused
    kw = dict(temps=N, transition="hmc", leapfrog=3, step_size=0.9, adapt=(0.65, 0.1), step_bounds=(0.3, 1.2), return_info=True)
    nll, one = vae.nll_ais(x, chains=C, noise=noise, **kw)
    assert 0.0 < float(one["accept_rate"].mean()) < 1.0, "both decisions"
    for per in (1, 3, N):                                  # reruns, with the noise asked for in chunks of 1 / 3 / all transitions
        nll2, again = vae.nll_ais(x, chains=C, noise=noise, iters_per_launch=per, **kw)
        assert _same(nll2, nll)
        for k in HMC_KEYS:
            assert _same(again[k], one[k]), (per, k)
    for ch in (0, 9):                                      # a chain alone: a row does not depend on its neighbours
        alone = tuple(t.narrow(-2 if t.dim() > 3 or (t.dim() == 3 and t is noise[0]) else -1, ch, 1).contiguous() for t in noise)
        _, a = vae.nll_ais(x, chains=1, noise=alone, **kw)
        for k in ("logw", "step_size", "accept_rate"):
            assert _same(a[k][:, 0], one[k][:, ch]), k
        for k in ("ratios", "accepts", "logw_trace"):
            assert _same(a[k][:, :, 0], one[k][:, :, ch]), k
        assert _same(a["cur"][:, 0], one["cur"][:, ch])


# ---- 6. against the truth at nz = 1 ---------------------------------------------------------------------------------------------
# test_ais.py's model and latent grid, restated; temps, leapfrog and step_size chosen so that the float64 statement meets the rule
TRUTH = dict(V=17, ni=4, H=20, nz=1, B=3, T=7, C=64, temps=40, L=3, step=0.6, noise_seed=41)
_truth_cache = {}


def _estimate(logw):
    logw = logw.double().cpu()
    C = logw.shape[1]
    w = torch.exp(logw - logw.max(dim=1, keepdim=True)[0])
    w = w / w.mean(dim=1, keepdim=True)
    return torch.logsumexp(logw, dim=1) - math.log(C), torch.sqrt(w.var(dim=1, unbiased=True) / C)


def _rule(name, lp, se, truth):
    err = (lp.double().cpu() - truth).abs()
    print("%s: |log p^ - truth| %s, se %s" % (name, err.tolist(), se.tolist()))
    assert bool((se <= 0.1).all()), (name, se)           # a degenerate run cannot pass by inflating its own error bar
    assert bool((err <= 4 * se + 2e-4).all()), (name, err, se)


def _truth():
    if _truth_cache:
        return _truth_cache
    from vae_lagging_encoder_amd.modules import VAE
    t = TRUTH
    Pm = O.random_params(t["V"], t["ni"], t["H"], t["nz"], seed=11, scale=1.0, emb_scale=0.5)
    x = O.synthetic_batch(t["B"], t["T"], t["V"], seed=12)
    P64 = {k: v.double() for k, v in Pm.items()}
    grid = (torch.arange(1601, dtype=torch.float64) * 0.01 - 8.0).view(1, -1, 1).expand(t["B"], -1, -1)
    truth = torch.logsumexp(_prior64(grid) - O.decoder_reconstruct_error(P64, x, grid), dim=1) + math.log(0.01)
    gen = torch.Generator().manual_seed(t["noise_seed"])
    B, C, n = t["B"], t["C"], t["temps"]
    noise = (torch.randn(B, C, 1, generator=gen), torch.randn(n, B, C, 1, generator=gen), torch.rand(n, B, C, generator=gen))
    beta = VAE.ais_schedule("sigmoid", n)
    ref = _hmc64(_score64(Pm, x), noise[0], noise[1], noise[2], beta, t["L"], t["step"])
    lp, se = _estimate(ref["logw"])
    print("float64 statement: log p^ %s, truth %s, acceptance %.3f" % (lp.tolist(), truth.tolist(), float(ref["flags"].float().mean())))
    _rule("float64 statement", lp, se, truth)
    _truth_cache.update(P=Pm, x=x, truth=truth, noise=noise, ref=ref)
    return _truth_cache


def test_float64_statement_meets_the_rule_at_nz1():
    """The seed's own check, on the CPU: a bad seed is thereby told from a bad kernel."""
    _truth()


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
def test_hmc_ais_against_the_grid_truth_at_nz1(hip_device, fused):
    """(GPU only: 121 decoder passes on 192 rows are minutes on the thread-level emulator, a fraction of a second here.)"""
    dev = hip_device
    c, t = _truth(), TRUTH
    vae = build_vae(t["V"], t["ni"], t["H"], t["nz"], dev, params=c["P"])
    vae.fused_hmc = fused
    noise = tuple(v.to(dev) for v in c["noise"])
    nll, info = vae.nll_ais(c["x"].to(dev), chains=t["C"], temps=t["temps"], noise=noise, transition="hmc", leapfrog=t["L"],
                            step_size=t["step"], return_info=True)
    assert info["route"] == ("hmc-fused" if fused else "hmc-generic") and info["iterations"] == t["temps"]
    lp, se = _estimate(info["logw"])
    assert float((nll.double().cpu() + lp).abs().max()) <= 1e-5 and float((info["se"].double().cpu() - se).abs().max()) <= 1e-9
    _rule("nll_ais hmc/" + info["route"], lp, se, c["truth"])


# ---- 7. surface ------------------------------------------------------------------------------------------------------------------
class Spy(object):
    """Records (name, args) of every backend entry that is looked up and called."""

    def __init__(self, lib, calls):
        self.lib, self.calls = lib, calls

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("lv_") or not callable(fn):
            return fn

        def call(*a):
            self.calls.append((name, a))
            return fn(*a)
        return call


class spying(object):
    def __init__(self):
        self.calls = []

    def __enter__(self):
        self.real = E.backend_for
        E.backend_for = lambda d: Spy(self.real(d), self.calls)
        return self.calls

    def __exit__(self, *a):
        E.backend_for = self.real


def _counts(calls):
    c = {}
    for name, _ in calls:
        c[name] = c.get(name, 0) + 1
    return c


ONCE_PER_CALL = ("lv_embed_gather_f32", "lv_embed_gather_b16", "lv_embed_scatter_f32", "lv_embed_scatter_full_f32",
                 "lv_embed_scatter_full_sumsq_f32", "lv_token_sort", "lv_repeat_rows_i64", "lv_cvt_bf16_f32", "lv_cvt_bf16_lo_f32",
                 "lv_cvt_h16_f32", "lv_gate_interleave_f32", "lv_lstm_persist16_pack", "lv_lstm_persist16_pack2")
WGRAD_ENTRIES = ("lv_dec_tail_bwd_f32", "lv_gemm_b16_sumsq", "lv_gemm_b16_dual", "lv_gemm_b16_pair", "lv_conv32_wgrad_f32")
SCATTERS = ("lv_embed_scatter_f32", "lv_embed_scatter_full_f32", "lv_embed_scatter_full_sumsq_f32")
PASS_F32 = ("lv_dec_init_f32", "lv_gx_expand_add_f32", "lv_lstm_fwd_f32", "lv_softmax_nll_fwd_f32", "lv_vae_loss_f32",
            "lv_softmax_nll_bwd_f32", "lv_lstm_bwd_f32", "lv_dec_tail_dz_f32", "lv_hmc_leap_f32")


def test_per_pass_work(target):
    """The fused route's launches per decoder pass, f32: 1 + N L passes, each the list of PASS_F32 once plus two products (logits,
    dO); nothing z-independent is repeated, no weight-gradient product, no dX, no scatter."""
    _, dev = target
    V, ni, H, nz, B, T, C, L = 53, 8, 16, 4, 3, 6, 4, 2
    vae = build_vae(V, ni, H, nz, dev, params=_params(V, ni, H, nz, 71))
    x = O.synthetic_batch(B, T, V, seed=76).to(dev)
    gen = torch.Generator().manual_seed(1)
    kw = dict(chains=C, transition="hmc", leapfrog=L, step_size=0.5, schedule="linear", return_info=True)
    vae.nll_ais(x, temps=1, noise=_noise(gen, 1, B, C, nz, dev), **kw)       # workspaces and weight images exist from here on
    runs = {}
    for N in (1, 3):
        noise = _noise(gen, N, B, C, nz, dev)
        with spying() as calls:
            info = vae.nll_ais(x, temps=N, noise=noise, **kw)[1]
        assert info["route"] == "hmc-fused"
        runs[N] = (_counts(calls), list(calls))
    c1, c3 = runs[1][0], runs[3][0]
    for name in ONCE_PER_CALL:
        assert c3.get(name, 0) == c1.get(name, 0), (name, c1.get(name, 0), c3.get(name, 0))
    assert c1["lv_embed_gather_f32"] >= 1 and c1["lv_repeat_rows_i64"] == 1
    for counts, calls in runs.values():
        for name in WGRAD_ENTRIES + SCATTERS:
            assert counts.get(name, 0) == 0, name
        for name, a in calls:
            if name in ("lv_gemm_f32", "lv_gemm_bf16"):
                assert a[0] == 0, "a transposed-A (weight-gradient) product ran"
                assert not (a[0] == 0 and a[1] == 0 and a[3] == ni), "dX ran"
    for name in PASS_F32:
        assert c1[name] == 1 + L and c3[name] == 1 + 3 * L, (name, c1[name], c3[name])
    assert c3["lv_gemm_f32"] - c1["lv_gemm_f32"] == 2 * 2 * L
    modes = [a[25] for name, a in runs[3][1] if name == "lv_hmc_leap_f32"]
    assert modes == [INIT] + [MID, LAST] * 3


@pytest.mark.gpu
def test_per_pass_work_and_smoke_bf16(hip_device):
    """bf16 at test_svi_refine.py's bf16 shape: forward() as it is and backward_dz() per pass -- no weight-gradient product, no
    scatter; two runs bit-identical and finite, the persistent status clean.  The distance from the f32 run is printed, not
    asserted."""
    dev = hip_device
    V, ni, H, nz, B, T, C, L, N = 2003, 32, 1024, 32, 4, 12, 2, 2, 2
    Pm = O.random_params(V, ni, H, nz, seed=78, scale=0.05, emb_scale=0.5, head_scale=0.5)
    vae = build_vae(V, ni, H, nz, dev, params=Pm)
    x = O.synthetic_batch(B, T, V, seed=79).to(dev)
    noise = _noise(torch.Generator().manual_seed(2), N, B, C, nz, dev)
    kw = dict(chains=C, temps=N, noise=noise, transition="hmc", leapfrog=L, step_size=0.05, return_info=True)
    nll32, i32 = vae.nll_ais(x, **kw)
    vae.set_precision("bf16")
    outs = []
    for _ in range(2):
        with spying() as calls:
            outs.append(vae.nll_ais(x, **kw))
    counts = _counts(calls)
    assert outs[0][1]["route"] == "hmc-fused"
    for name in WGRAD_ENTRIES + SCATTERS:
        assert counts.get(name, 0) == 0, name
    for name, a in calls:
        if name in ("lv_gemm_f32", "lv_gemm_bf16", "lv_gemm_b16"):
            assert a[0] == 0, "a transposed-A (weight-gradient) product ran: %s" % name
    assert counts["lv_hmc_leap_f32"] == counts["lv_dec_tail_dz_f32"] == 1 + N * L
    assert _same(outs[0][0], outs[1][0]) and bool(torch.isfinite(outs[0][0]).all())
    for k in HMC_KEYS:
        assert _same(outs[0][1][k], outs[1][1][k]), k
    E.check_persistent_status(vae.decoder._hip)
    print("bf16 vs f32: largest |nll - nll32| %.3e, largest |dH - dH32| %.3e"
          % (float((outs[0][0] - nll32).abs().max()), float((outs[0][1]["ratios"] - i32["ratios"]).abs().max())))


def _check_routing_and_refusals(dev, other):
    V, ni, H, nz, B, T, C, N = 31, 6, 12, 2, 2, 5, 4, 3
    vae = build_vae(V, ni, H, nz, dev, params=_params(V, ni, H, nz, 9))          # train mode, dropout 0.5 / 0.5
    x = O.synthetic_batch(B, T, V, seed=10).to(dev)
    for eng in (vae.encoder._hip, vae.decoder._hip):
        eng.ensure(dev)
    gen = torch.Generator().manual_seed(3)
    noise = _noise(gen, N, B, C, nz, dev)
    kw = dict(chains=C, temps=N, transition="hmc", leapfrog=2)
    with pytest.raises(ValueError, match="ais_step_size"):
        vae.nll_ais(x, **kw)
    vae.args.ais_step_size = 0.4
    nll, info = vae.nll_ais(x, return_info=True, **kw)         # a training-mode decoder runs in eval arithmetic: still fused
    assert info["route"] == "hmc-fused" and tuple(nll.shape) == (B,) and bool(torch.isfinite(nll).all()) and vae.decoder.training
    assert tuple(info["step_size"].shape) == (B, C) and bool((info["step_size"] == np.float32(0.4)).all()) and info["leapfrog"] == 2
    assert tuple(info["accept_rate"].shape) == (B, C) and tuple(info["ratios"].shape) == (N, B, C) and tuple(info["se"].shape) == (B,)
    vae.fused_hmc = False
    assert vae.nll_ais(x, noise=noise, return_info=True, **kw)[1]["route"] == "hmc-generic"
    del vae.fused_hmc
    # a batch beyond the session's envelope takes the generic route
    wide = 125
    assert not vae.decoder._hip.svi_supported(B, wide)
    big = _noise(gen, 1, B, wide, nz, dev)
    nll_w, info_w = vae.nll_ais(x, chains=wide, temps=1, noise=big, transition="hmc", leapfrog=1, return_info=True)
    assert info_w["route"] == "hmc-generic" and bool(torch.isfinite(nll_w).all())
    # the same seed gives the same tensor twice; the encoder init and `transitions` work without injected noise
    outs = [vae.nll_ais(x, generator=torch.Generator(device=dev).manual_seed(6), **kw) for _ in range(2)]
    assert _same(outs[0], outs[1])
    nll_e = vae.nll_ais(x, chains=3, temps=2, transitions=2, schedule="linear", init="encoder", transition="hmc", leapfrog=1)
    assert tuple(nll_e.shape) == (B,) and bool(torch.isfinite(nll_e).all())
    # refusals by value, and a variable-length pair: all before any launch
    z0, mom, u = noise
    with spying() as calls:
        for bad in (dict(transition="nuts"), dict(leapfrog=0), dict(step_size=0.0), dict(step_size=-1.0), dict(step_size=float("nan")),
                    dict(std=0.3), dict(step_bounds=(0.5, 0.1)), dict(step_bounds=(0.0, 0.1)), dict(adapt=(0.0, 0.1)),
                    dict(adapt=(1.0, 0.1)), dict(adapt=(0.65, 0.0)), dict(noise=(z0[:, :2].contiguous(), mom, u)),
                    dict(noise=(z0, mom[:2], u)), dict(noise=(z0, mom, u[:, :, :1].contiguous())), dict(iters_per_launch=0)):
            args = dict(kw, noise=noise)
            args.update(bad)
            with pytest.raises(ValueError):
                vae.nll_ais(x, **args)
        with pytest.raises(ValueError, match="variable-length"):
            vae.nll_ais((x, [5, 4]), **kw)
        with pytest.raises(ValueError, match="variable-length"):
            vae.sample_from_posterior((x, [5, 4]), 1, burn_in=1, thin=1, transition="hmc", step_size=0.3)
        with pytest.raises(ValueError):
            vae.sample_from_posterior(x, 1, burn_in=1, thin=1, transition="hmc", step_size=0.3, std=0.2)
        with pytest.raises(ValueError, match="mh_step_size"):
            vae.sample_from_posterior(x, 1, burn_in=1, thin=1, transition="hmc")
        # operands on another device never reach a kernel
        for bad in ((z0.to(other), mom, u), (z0, mom.to(other), u), (z0, mom, u.to(other))):
            for fused in (True, False):
                vae.fused_hmc = fused
                with pytest.raises(_lib.LvaeError):
                    vae.nll_ais(x, noise=bad, **kw)
        del vae.fused_hmc
        st = {k: torch.zeros(B, C, nz, device=dev) for k in ("pos", "mom", "cur", "d_cur")}
        st.update({k: torch.zeros(B, C, device=dev) for k in ("k0", "g_cur", "lq_cur", "rec_cur", "eps")})
        st.update(logw=torch.zeros(B, C, dtype=torch.float64, device=dev), accepts=torch.zeros(B, C, dtype=torch.int32, device=dev))
        with pytest.raises(_lib.LvaeError):
            E.hmc_leap(torch.zeros(B * C, device=dev), torch.zeros(1, B * C, nz).to(other), st, INIT, 1)
        with pytest.raises(ValueError):
            E.hmc_leap(torch.zeros(B * C, device=dev), torch.zeros(1, B * C, nz, device=dev), dict(st, logw=st["logw"].float()), INIT, 1)
    assert [n for n, _ in calls] == [], calls


def test_routing_and_refusals_emulated(emu_backend):
    _check_routing_and_refusals(torch.device("cpu"), "meta")


@pytest.mark.gpu
def test_routing_and_refusals(hip_device):
    _check_routing_and_refusals(hip_device, "cpu")


def _state(vae):
    out = {"param/" + k: p.detach().clone() for k, p in vae.named_parameters()}
    out.update({"grad/" + k: (None if p.grad is None else p.grad.detach().clone()) for k, p in vae.named_parameters()})
    out.update({"buf/" + k: b.detach().clone() for k, b in vae.named_buffers()})
    out.update({"train/" + k: m.training for k, m in vae.named_modules()})
    for n, m in (("enc", vae.encoder), ("dec", vae.decoder)):
        for i, slot in enumerate(m._hip.flat._slots):
            out["flat/%s/%d" % (n, i)] = slot[0].detach().clone()
    out["rng/cpu"] = torch.get_rng_state()
    if torch.cuda.is_available():
        out["rng/cuda"] = torch.cuda.get_rng_state()
    return out


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
def test_hmc_leaves_the_model_and_the_generators_alone(target, fused):
    _, dev = target
    V, ni, H, nz, B, T, C, N = 53, 8, 16, 4, 3, 6, 2, 2
    vae = build_vae(V, ni, H, nz, dev, params=_params(V, ni, H, nz, 71))
    vae.train()
    x = O.synthetic_batch(B, T, V, seed=80).to(dev)
    vae.loss(x, 1.0)[0].mean().backward()               # gradients exist (views of the flat buffers) before the call
    noise = _noise(torch.Generator().manual_seed(4), N, B, C, nz, dev)
    before = _state(vae)
    grad_ids = {k: id(p.grad) for k, p in vae.named_parameters()}
    vae.fused_hmc = fused
    try:
        for init in ("prior", "encoder"):
            nll = vae.nll_ais(x, chains=C, temps=N, noise=noise, init=init, transition="hmc", leapfrog=2, step_size=0.4, adapt=(0.65, 0.05))
            assert not nll.requires_grad
        vae.sample_from_posterior(x, 1, chains=C, burn_in=1, thin=1, noise=noise, transition="hmc", leapfrog=2, step_size=0.4)
    finally:
        del vae.fused_hmc
    after = _state(vae)
    assert before.keys() == after.keys()
    for k in before:
        if torch.is_tensor(before[k]):
            assert after[k] is not None and _same(before[k], after[k]), k
        else:
            assert before[k] == after[k], k
    assert grad_ids == {k: id(p.grad) for k, p in vae.named_parameters()}       # the same .grad OBJECTS as before


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "generic"])
def test_posterior_sampling_keeps_the_sessions_states_and_freezes_adaptation(target, fused):
    """sample_from_posterior(transition="hmc"): sample k is cur after transition burn_in + k * thin -- the final state of the same
    chain cut there (adaptation off, so the cut changes nothing else) -- within the statement's tolerance of the float64 statement
    at beta = 1; with adaptation, the factors a launch is given are 1.0 from transition burn_in on."""
    _, dev = target
    c = _session_case("prior")
    V, ni, H, nz = c["dims"]
    B, C = c["B"], c["C"]
    vae = build_vae(V, ni, H, nz, dev, params=c["P"])
    vae.fused_hmc = fused
    x = c["x"].to(dev)
    burn_in, thin, ns, L, step = 2, 2, 3, 2, 0.9
    total = burn_in + ns * thin
    z0, mom, u = c["z0"].to(dev), c["mom"][:total].to(dev), c["u"][:total].to(dev)
    kw = dict(chains=C, transition="hmc", leapfrog=L, step_size=step)
    samples, info = vae.sample_from_posterior(x, ns, burn_in=burn_in, thin=thin, noise=(z0, mom, u), return_info=True, **kw)
    assert tuple(samples.shape) == (B, ns, C, nz) and info["route"] == ("hmc-fused" if fused else "hmc-generic")
    assert sorted(info) == ["accept_rate", "accepts", "iterations", "log_joint", "ratios", "route"] and info["iterations"] == total
    assert 0.0 < float(info["accept_rate"].mean()) < 1.0
    ref = _hmc64(_score64(c["P"], c["x"]), c["z0"], c["mom"][:total], c["u"][:total], [1.0] * (total + 1), L, step)
    for k in range(ns):
        it = burn_in + k * thin
        cut, icut = vae.sample_from_posterior(x, 1, burn_in=it, thin=1, noise=(z0, mom[:it + 1], u[:it + 1]), return_info=True, **kw)
        assert _same(samples[:, k], cut[:, 0]) and _same(info["ratios"][:it + 1], icut["ratios"])
        ok = ref["margin"][:it + 1].amin(dim=0) >= TAU
        assert bool(ok.any()) and float((samples[:, k].cpu().double() - ref["curs"][it].double()).abs()[ok].max()) <= _session_tol()
    vae.eval()                                             # (the sampler ran in eval arithmetic whatever the flag said)
    with torch.no_grad():                                  # (the last cut ends at its kept transition: its final state is the sample)
        joint = vae.eval_complete_ll(x, cut[:, 0].contiguous())
    assert float((icut["log_joint"] - joint).abs().max()) <= 3e-4                 # log p(cur, x) of the final state
    with spying() as calls:
        vae.sample_from_posterior(x, ns, burn_in=burn_in, thin=thin, noise=(z0, mom, u), adapt=(0.65, 0.1), step_bounds=(0.3, 1.2), **kw)
    last = [a for name, a in calls if name == "lv_hmc_leap_f32" and a[25] == LAST]
    assert len(last) == total
    up, down = _f32(math.exp(0.1 * 0.35)), _f32(math.exp(-0.1 * 0.65))
    for it, a in enumerate(last):
        assert (a[26], a[27]) == ((up, down) if it < burn_in else (1.0, 1.0)), it
        assert (a[33] is not None) == (it >= burn_in and (it - burn_in) % thin == 0), it      # keep_out at the kept transitions only
    del vae.fused_hmc


def _check_evaluation(dev):
    V, ni, H, nz, T = 31, 6, 12, 2, 5
    vae = build_vae(V, ni, H, nz, dev, params=_params(V, ni, H, nz, 9))
    vae.eval()
    batches = [O.synthetic_batch(3, T, V, seed=40).to(dev), O.synthetic_batch(2, T + 1, V, seed=41).to(dev)]
    args = types.SimpleNamespace(ais_std=0.3, ais_step_size=0.5)       # ais_std must not leak into a Hamiltonian run
    kw = dict(chains=3, temps=3, transition="hmc", leapfrog=2, adapt=(0.65, 0.05))

    def gen():
        return torch.Generator(device=dev).manual_seed(8)
    nll, ppl = EV.calc_aisnll(vae, batches, args, np_rng=np.random.RandomState(0), generator=gen(), **kw)
    g2, tot = gen(), 0.0
    for i in np.random.RandomState(0).permutation(2):
        tot += float(vae.nll_ais(batches[i], step_size=0.5, generator=g2, **kw).sum())
    sents, words = 5, 3 * (T - 1) + 2 * T
    assert abs(nll - tot / sents) <= 1e-5 * abs(nll) and abs(ppl - math.exp(nll * sents / words)) <= 1e-9 * ppl
    gaps = EV.calc_inference_gaps(vae, batches, steps=2, np_rng=np.random.RandomState(1), ais=dict(kw, step_size=0.5, generator=gen()))
    assert gaps["n"] == sents and math.isfinite(gaps["log_px"]) and gaps["approximation_gap"] == gaps["log_px"] - gaps["elbo_svi"]
    img = EV.image_calc_aisnll(vae, [(b, None) for b in batches], args, generator=gen(), **kw)
    g3 = gen()
    want = sum(float(vae.nll_ais(b, step_size=0.5, generator=g3, **kw).sum()) for b in batches) / sents
    assert abs(img - want) <= 1e-5 * abs(want)


def test_evaluation_passes_the_arguments_through_emulated(emu_backend):
    _check_evaluation(torch.device("cpu"))


@pytest.mark.gpu
def test_evaluation_passes_the_arguments_through(hip_device):
    _check_evaluation(hip_device)


@pytest.mark.gpu
def test_pixelcnn_decoder_takes_the_generic_route(hip_device):
    """One image, L = 2, N = 2 through lv_bn_eval_bwd_f32: finite, deterministic, the model's buffers as before."""
    from vae_lagging_encoder_amd.factory import build_image_vae
    dev = hip_device
    vae = build_image_vae(dev, seed=3)
    vae.train()
    with torch.no_grad():
        x = (torch.rand(1, 1, 28, 28, generator=torch.Generator().manual_seed(4)) < 0.3).float().to(dev)
        vae.loss(x, 1.0)              # MaskedConv2d masks its weight in place on every forward: idempotent from here on
    C, N = 2, 2
    noise = _noise(torch.Generator().manual_seed(5), N, 1, C, vae.nz, dev)
    before = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    outs = [vae.nll_ais(x, chains=C, temps=N, schedule="linear", noise=noise, transition="hmc", leapfrog=2, step_size=0.02,
                        return_info=True) for _ in range(2)]
    (nll, info), (nll2, info2) = outs
    assert info["route"] == "hmc-generic" and tuple(nll.shape) == (1,) and bool(torch.isfinite(nll).all())
    assert bool(torch.isfinite(info["logw_trace"]).all()) and bool(torch.isfinite(info["ratios"]).all())
    assert _same(nll, nll2) and all(_same(info[k], info2[k]) for k in HMC_KEYS)
    for k, v in vae.state_dict().items():
        assert _same(v, before[k]), k
    assert vae.training and vae.decoder.training

"""Annealed importance sampling estimate of log p(x) (csrc/lv_ais.hip, engine.LSTMDecoderEngine.ais_chain / engine.ais_step,
VAE.nll_ais, evaluation.calc_aisnll / calc_inference_gaps).  The contract every layer follows is at the top of lv_ais.hip.

Kernel level (emulator build and MI355X through one fixture): lv_ais_step_f32 and lv_ais_chain_f32 against float64 statements
of the chain with proposals formed in float32; launch cuts, reruns and tile neighbours bit-identical; the argument checks.

The comparison rule is test_mh_posterior.py's, TAU = 1e-3 and RATIO_TOL = 2e-4: an accept decision is discontinuous, so a
chain is compared up to, not including, its first iteration whose REFERENCE margin |log u - ratio| (ratio < 0) is under TAU;
on that prefix the flags are equal, |ratio - ratio_ref| <= 2e-4 and |logw_trace - logw_ref| <= 2e-4 (the increments' weights
beta_i - beta_{i-1} sum to 1 and each g is held to 1e-4 by the grid tests; the largest values seen are printed); a chain
compared to its end also has a bit-equal final state.  At most 1/4 of a case's chains may contain an under-TAU decision: a
condition on seeds.

Against the truth (nz = 1, a latent grid on the float64 oracle): |log p^ - truth| <= 4 se + 2e-4 with se <= 0.1, asserted for
the float64 statement on the same noise first, then for the kernels.  Drop-in level: tests/golden/ais_small.npz
(make_golden_ais.py: the contract's loop over the reference's unmodified density methods).
"""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from helpers import build_vae, load
from oracle import text_vae_oracle as O
from vae_lagging_encoder_amd import _lib
from vae_lagging_encoder_amd import engine as E
from vae_lagging_encoder_amd import evaluation as EV
from vae_lagging_encoder_amd.engine import P
from vae_lagging_encoder_amd.factory import build_image_vae, build_text_vae

TAU = 1e-3
RATIO_TOL = 2e-4
U24 = 2.0 ** -24
LOG_2PI = math.log(2 * math.pi)
POISON = 7777.0
IPOISON = 7777


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


def _propose(eps, std, cur):
    """The float32 two-rounding proposal (CPU tensors): the product is rounded, then the sum."""
    t = eps.float() * torch.tensor(std, dtype=torch.float32)
    return t + cur.float()


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


def _g64(z, lq, cond, mu0):
    return cond.double() if mu0 is None else (_prior64(z) - lq) + cond.double()


def _margin(ratio, u):
    """|log u - ratio| where ratio < 0, inf elsewhere (float64; u = 0 gives inf: such a draw never accepts a ratio < 0)."""
    ratio, u = ratio.double(), u.double()
    m = (torch.log(u) - ratio).abs()
    return torch.where(ratio < 0, m, torch.full_like(m, float("inf")))


def _f32(v):
    return float(np.float32(v))


def _ais64(cond_fn, z0, eps, u, beta, stds, mu0=None, lv0=None):
    """The contract with float64 densities and float32 proposals.  cond_fn(z [B][C][nz] float32) -> log p(x|z) [B][C] float64.
    -> dict(logw, cur, g, ratios, flags, trace, margin, accepts)."""
    cur = z0.clone().float()
    lq = _logq0_64(cur, mu0, lv0)
    g = _g64(cur, lq, cond_fn(cur), mu0)
    logw = torch.zeros_like(g)
    ratios, flags, trace = [], [], []
    for it in range(eps.shape[0]):
        logw = logw + (beta[it + 1] - beta[it]) * g
        trace.append(logw.clone())
        nxt = _propose(eps[it], stds[it], cur)
        lqn = _logq0_64(nxt, mu0, lv0)
        gn = _g64(nxt, lqn, cond_fn(nxt), mu0)
        bf = _f32(beta[it + 1])
        ratio = (lqn + bf * gn) - (lq + bf * g)
        acc = (ratio >= 0) | (u[it].double() < ratio.exp())
        cur = torch.where(acc.unsqueeze(-1), nxt, cur)
        g, lq = torch.where(acc, gn, g), torch.where(acc, lqn, lq)
        ratios.append(ratio)
        flags.append(acc)
    ratios, flags, trace = torch.stack(ratios), torch.stack(flags), torch.stack(trace)
    return {"logw": logw, "cur": cur, "g": g, "ratios": ratios, "flags": flags, "trace": trace, "margin": _margin(ratios, u),
            "accepts": flags.sum(0)}


def _check_prefix(name, ratios, flags, trace, ref_ratio, ref_flag, ref_trace, margin, cap=True):
    """The comparison rule on every chain ([n][B][C] arrays); returns the chains compared to the end."""
    n, B, C = ref_ratio.shape
    ratios, flags, trace = ratios.cpu().double(), flags.cpu(), trace.cpu().double()
    worst_r = worst_w = 0.0
    full = []
    for b in range(B):
        for c in range(C):
            low = (margin[:, b, c] < TAU).nonzero()
            stop = int(low[0]) if low.numel() else n
            if stop == n:
                full.append((b, c))
            assert torch.equal(flags[:stop, b, c] != 0, ref_flag[:stop, b, c] != 0), (name, b, c)
            if stop:
                worst_r = max(worst_r, float((ratios[:stop, b, c] - ref_ratio[:stop, b, c].double()).abs().max()))
            # the increment of iteration `stop` still uses a state the decisions before it settled
            upto = min(stop + 1, n)
            worst_w = max(worst_w, float((trace[:upto, b, c] - ref_trace[:upto, b, c].double()).abs().max()))
    print("%s: %d of %d chains compared to the end, largest |ratio - ratio_ref| %.3e, largest |logw - logw_ref| %.3e"
          % (name, len(full), B * C, worst_r, worst_w))
    assert worst_r <= RATIO_TOL and worst_w <= RATIO_TOL, (name, worst_r, worst_w)
    if cap:
        assert 4 * (B * C - len(full)) <= B * C, "%s: more than 1/4 of the chains are marginal -- pick another seed, not another TAU" % name
    return full


# ---- 1. lv_ais_step_f32 ---------------------------------------------------------------------------------------------------
ROLES = ("plain", "nan", "u0", "u_max")


def _step_case(lib, dev, rows, C, nz, role, enc, init, last, seed):
    """One launch on poisoned, over-allocated buffers; asserts everything.  enc: q0 is a per-sentence Gaussian (else the prior);
    init: the scoring of z_0; last: no next iteration (eps_next NULL)."""
    gen = torch.Generator().manual_seed(seed)
    B, pad = rows // C, 2
    std, std_next = 0.7, 0.45
    beta, dbeta = 0.2 + 0.7 * float(torch.rand(1, generator=gen, dtype=torch.float64)), 0.0371
    bf = _f32(beta)
    mu0 = (0.5 * torch.randn(B, nz, generator=gen)) if enc else None
    lv0 = (0.3 * torch.randn(B, nz, generator=gen) - 0.5) if enc else None
    cur = torch.randn(rows, nz, generator=gen)
    prop = _propose(torch.randn(rows, nz, generator=gen), std, cur)
    eps_next = torch.randn(rows, nz, generator=gen)
    g_cur = torch.randn(rows, generator=gen) * 5 - 30
    lq_cur = _logq0_64(cur.view(B, C, nz), mu0, lv0).view(rows).float()
    logw_in = torch.randn(rows, generator=gen, dtype=torch.float64) * 3 - 10
    counts = torch.randint(0, 50, (rows,), generator=gen, dtype=torch.int32)
    target_ratio = torch.rand(rows, generator=gen, dtype=torch.float64) * 5 - 3          # in [-3, 2)
    want_accept = torch.rand(rows, generator=gen) < 0.5
    special = seed % rows
    if role == "u_max":
        target_ratio[special] = 0.25
    elif role == "u0":
        target_ratio[special] = -200.0
    at = cur if init else prop
    lq_at = _logq0_64(at.view(B, C, nz), mu0, lv0).view(rows)
    pz_at = _prior64(at)
    # cond such that the ratio lands on its target: ratio = (lq_at + b g_at) - (lq_cur + b g_cur), g_at = (pz_at - lq_at) + cond
    g_at_want = (target_ratio + lq_cur.double() + bf * g_cur.double() - lq_at) / bf
    cond = (g_at_want - ((pz_at - lq_at) if enc else 0.0)).float()
    if role == "nan":
        cond[special] = float("nan")
    # the float64 statement from the operands the kernel actually gets
    g_at = _g64(at.view(B, C, nz), lq_at.view(B, C), cond.view(B, C), mu0).view(rows)
    ratio64 = (lq_at + bf * g_at) - (lq_cur.double() + bf * g_cur.double())
    # float32 arithmetic: every operation rounds to within 2^-24 relative, expf(-lv) to within 2 ulp; a sum of nz + O(1) terms
    # is off by at most (terms + 12) * 2^-24 * the sum of the addends' magnitudes
    quad = 0.5 * ((at.view(B, C, nz).double() - (mu0.double().unsqueeze(1) if enc else 0.0)) ** 2
                  * (torch.exp(-lv0.double()).unsqueeze(1) if enc else 1.0)).sum(-1).view(rows)
    const = 0.5 * nz * LOG_2PI + (0.5 * lv0.double().abs().sum(-1).repeat_interleave(C) if enc else 0.0)
    mag_lq = quad + const
    mag_g = cond.double().abs() + ((0.5 * (at.double() ** 2).sum(-1) + 0.5 * nz * LOG_2PI + mag_lq) if enc else 0.0)
    k = (nz + 12) * U24
    b_lq, b_g = k * mag_lq, k * mag_g
    bound = k * (mag_lq + mag_g + lq_cur.double().abs() + g_cur.double().abs()) + 2 * U24 * ratio64.abs()
    p = torch.exp(torch.clamp(ratio64, max=0.0))
    can_reject = p < 0.9
    accept = torch.where(can_reject, want_accept, torch.ones_like(want_accept))
    u = torch.where(accept, 0.5 * p, p + 0.5 * (1 - p)).float()
    if role == "u_max":
        u[special], accept[special] = 1.0 - U24, True
    elif role == "u0":
        u[special], accept[special] = 0.0, False
    elif role == "nan":
        u[special], accept[special] = 0.0, False
    ok = torch.ones(rows, dtype=torch.bool)
    if role == "nan":
        ok[special] = False
    if not init and bool(ok.any()):                          # every margin is large by construction: twice the bound and more
        assert float(_margin(ratio64[ok], u[ok]).min()) > 0.05 and float(bound[ok].max()) < 0.025

    def dv(t, fill):
        full = torch.full((t.shape[0] + pad,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
        full[:t.shape[0]] = t
        return full.to(dev)
    d_cond, d_prop, d_cur, d_g, d_lq = dv(cond, POISON), dv(prop, POISON), dv(cur, POISON), dv(g_cur, POISON), dv(lq_cur, POISON)
    d_lw, d_cnt, d_u, d_eps = dv(logw_in, POISON), dv(counts, IPOISON), dv(u, POISON), dv(eps_next, POISON)
    d_ratio, d_flag = torch.full((rows + pad,), POISON).to(dev), torch.full((rows + pad,), IPOISON, dtype=torch.int32).to(dev)
    d_lwn = torch.full((rows + pad,), POISON, dtype=torch.float64).to(dev)
    d_mu, d_lv = (mu0.to(dev), lv0.to(dev)) if enc else (None, None)
    lib.lv_ais_step_f32(P(d_cond), P(d_prop), P(d_cur), P(d_g), P(d_lq), P(d_lw), P(d_cnt), None if init else P(d_u), beta,
                        None if last else P(d_eps), std_next, dbeta, P(d_mu), P(d_lv), rows, C, nz, 1 if init else 0,
                        P(d_ratio), P(d_flag), P(d_lwn), E.stream_ptr(dev))
    got = {k_: v.cpu() for k_, v in dict(prop=d_prop, cur=d_cur, g=d_g, lq=d_lq, lw=d_lw, cnt=d_cnt, ratio=d_ratio, flag=d_flag,
                                         lwn=d_lwn).items()}
    for k_ in ("prop", "cur", "g", "lq", "lw", "ratio", "lwn"):                        # rows beyond the count keep their poison
        assert bool((got[k_][rows:] == POISON).all()), k_
    assert bool((got["cnt"][rows:] == IPOISON).all()) and bool((got["flag"][rows:] == IPOISON).all())
    gg, gl = got["g"][:rows], got["lq"][:rows]
    if init:
        assert _same(got["cur"][:rows], cur) and bool((got["cnt"][:rows] == 0).all())
        assert bool((got["ratio"] == POISON).all()) and bool((got["flag"] == IPOISON).all())
        if role == "nan":
            assert math.isnan(float(gg[special]))
        if not enc:
            assert _same(gg[ok], cond[ok])                                            # g is the conditional log-likelihood, bit for bit
        assert bool(((gg.double() - g_at).abs()[ok] <= b_g[ok]).all()) and bool(((gl.double() - lq_at).abs() <= b_lq).all())
        new_cur, base = cur, torch.zeros(rows, dtype=torch.float64)
    else:
        assert torch.equal(got["flag"][:rows] != 0, accept), role                     # decisions are exact
        new_cur = torch.where(accept.unsqueeze(1), prop, cur)
        assert _same(got["cur"][:rows], new_cur)                                      # selected, bit for bit
        assert torch.equal(got["cnt"][:rows], counts + accept.to(torch.int32))
        rej = ~accept
        assert _same(gg[rej], g_cur[rej]) and _same(gl[rej], lq_cur[rej])             # a rejected row's state is untouched
        assert bool(torch.isfinite(gg).all()) and bool(torch.isfinite(gl).all())      # ... a NaN score included
        assert bool(((gg.double() - g_at).abs()[accept] <= b_g[accept]).all())
        assert bool(((gl.double() - lq_at).abs()[accept] <= b_lq[accept]).all())
        assert bool(((got["ratio"][:rows].double() - ratio64).abs()[ok] <= bound[ok]).all())
        if role == "nan":
            assert math.isnan(float(got["ratio"][special]))
        base = logw_in
    if last:
        assert _same(got["prop"][:rows], prop) and bool((got["lwn"] == POISON).all())
        assert _same(got["lw"][:rows], base)
    else:
        assert _same(got["prop"][:rows], _propose(eps_next, std_next, new_cur))       # the next proposals
        want = base + dbeta * gg.double()                                             # the next increment, in float64
        fin = torch.isfinite(want)
        assert bool(((got["lw"][:rows] - want).abs()[fin] <= 1e-12 * want.abs().clamp(min=1.0)[fin]).all())
        assert bool((torch.isnan(got["lw"][:rows]) == ~fin).all())
        assert _same(got["lwn"][:rows], got["lw"][:rows])


@pytest.mark.parametrize("enc", [False, True], ids=["prior", "encoder"])
@pytest.mark.parametrize("nz", [1, 5, 32, 67])
@pytest.mark.parametrize("rows,C", [(1, 1), (3, 3), (70, 10)])
def test_ais_step_against_float64_statement(target, rows, C, nz, enc):
    lib, dev = target
    seed = 1000 * rows + nz + (500 if enc else 0)
    for i, role in enumerate(ROLES):
        _step_case(lib, dev, rows, C, nz, role, enc, init=False, last=False, seed=seed + i)
    _step_case(lib, dev, rows, C, nz, "plain", enc, init=False, last=True, seed=seed + 5)
    _step_case(lib, dev, rows, C, nz, "plain", enc, init=True, last=False, seed=seed + 7)
    _step_case(lib, dev, rows, C, nz, "nan", enc, init=True, last=False, seed=seed + 8)


# ---- 2. lv_ais_chain_f32 --------------------------------------------------------------------------------------------------
def _params(V, ni, H, nz, seed):
    return O.random_params(V, ni, H, nz, seed=seed, scale=0.3, emb_scale=0.5)


def _batch(B, T, V, seed):
    x = O.synthetic_batch(B, T, V, seed=seed)
    if T > 2:
        x[0, T - 2:] = 0
    return x


def _cond64(Pm, x):
    P64 = {k: v.double() for k, v in Pm.items()}
    return lambda z: -O.decoder_reconstruct_error(P64, x, z.double())


# V, ni, H, nz, B, T, chains: all four padded sizes, a ragged second tile, nz 1 .. 64 (H = 100 fits the registers without
# scratch -- DESIGN.md 3.1.2 -- so those two are chain-route cases too)
CHAIN_CASES = [
    (17, 4, 5, 1, 1, 2, 1),
    (17, 4, 5, 3, 3, 7, 5),
    (60, 8, 20, 8, 1, 7, 16),
    (60, 8, 20, 1, 3, 2, 17),
    (17, 6, 50, 64, 1, 7, 5),
    (17, 6, 50, 3, 1, 7, 17),
    (60, 8, 100, 8, 1, 7, 1),
    (17, 4, 100, 64, 3, 2, 5),
]
# 12 iterations: non-uniform, one temperature repeated (a further transition there, with a zero increment)
BETA = [0.0, 0.04, 0.15, 0.15, 0.27, 0.4, 0.5, 0.62, 0.7, 0.81, 0.9, 0.96, 1.0]
STDS = [0.5, 0.48, 0.46, 0.44, 0.42, 0.4, 0.38, 0.36, 0.34, 0.32, 0.3, 0.28]
N_IT = 12
KEYS = ("logw", "cur", "g", "accepts", "ratios", "flags", "logw_trace")


def _run_chain(eng, x, z0, eps, u, mu0, lv0, per):
    dev = x.device
    return eng.ais_chain(x, z0, lambda i0, n: (eps[i0:i0 + n], u[i0:i0 + n]), torch.tensor(BETA, dtype=torch.float64, device=dev),
                         torch.tensor(STDS, dtype=torch.float32, device=dev), mu0, lv0, iters_per_launch=per)


def _check_chain(lib, dev, V, ni, H, nz, B, T, C, enc, seed):
    Pm = _params(V, ni, H, nz, seed)
    vae = build_vae(V, ni, H, nz, dev, params=Pm)
    vae.eval()
    x = _batch(B, T, V, seed + 1)
    gen = torch.Generator().manual_seed(seed + 2)
    mu0 = (0.5 * torch.randn(B, nz, generator=gen)) if enc else None
    lv0 = (0.3 * torch.randn(B, nz, generator=gen) - 0.5) if enc else None
    z0 = torch.randn(B, C, nz, generator=gen)
    if enc:
        z0 = mu0.unsqueeze(1) + torch.exp(0.5 * lv0).unsqueeze(1) * z0
    eps = torch.randn(N_IT, B, C, nz, generator=gen)
    u = torch.rand(N_IT, B, C, generator=gen)
    ref = _ais64(_cond64(Pm, x), z0, eps, u, BETA, STDS, mu0, lv0)
    eng = vae.decoder._hip
    eng.ensure(dev)
    assert lib.lv_ais_chain_f32_supported(V, ni, H, nz, T) == 1
    xd, zd, ed, ud = x.to(dev), z0.to(dev), eps.to(dev), u.to(dev)
    md, ld = (mu0.to(dev), lv0.to(dev)) if enc else (None, None)
    one = _run_chain(eng, xd, zd, ed, ud, md, ld, N_IT)
    name = "ais chain V%d H%d nz%d B%d T%d C%d %s" % (V, H, nz, B, T, C, "encoder" if enc else "prior")
    full = _check_prefix(name, one["ratios"], one["flags"], one["logw_trace"], ref["ratios"], ref["flags"], ref["trace"], ref["margin"])
    for b, c in full:                                      # chains compared to the end: the final state too
        assert _same(one["cur"][b, c], ref["cur"][b, c])
        assert abs(float(one["logw"][b, c]) - float(ref["logw"][b, c])) <= RATIO_TOL
        assert abs(float(one["g"][b, c]) - float(ref["g"][b, c])) <= RATIO_TOL
        assert int(one["accepts"][b, c]) == int(ref["accepts"][b, c])
    assert _same(one["logw"], one["logw_trace"][-1])
    for per in (1, 5, 12):                                 # the cut into launches does not matter, a rerun is bit-identical
        again = _run_chain(eng, xd, zd, ed, ud, md, ld, per)
        for k in KEYS:
            assert _same(again[k], one[k]), (name, per, k)
    return vae, xd, zd, ed, ud, md, ld, one


@pytest.mark.parametrize("enc", [False, True], ids=["prior", "encoder"])
@pytest.mark.parametrize("V,ni,H,nz,B,T,C", CHAIN_CASES)
def test_ais_chain_against_float64_statement_cuts_and_reruns(target, V, ni, H, nz, B, T, C, enc):
    lib, dev = target
    _check_chain(lib, dev, V, ni, H, nz, B, T, C, enc, seed=V + 7 * H + nz + C + (3 if enc else 0))


def test_ais_chain_a_chain_does_not_depend_on_its_tile(target):
    lib, dev = target
    vae, xd, zd, ed, ud, md, ld, all16 = _check_chain(lib, dev, 60, 8, 20, 3, 2, 7, 16, True, seed=77)
    eng = vae.decoder._hip
    for c in (0, 9, 15):
        alone = _run_chain(eng, xd, zd[:, c:c + 1].contiguous(), ed[:, :, c:c + 1].contiguous(), ud[:, :, c:c + 1].contiguous(),
                           md, ld, 5)
        for k in ("logw", "cur", "g", "accepts"):
            assert _same(alone[k][:, 0], all16[k][:, c]), k
        for k in ("ratios", "flags", "logw_trace"):
            assert _same(alone[k][:, :, 0], all16[k][:, :, c]), k


@pytest.mark.gpu
def test_ais_chain_toy_vocabulary_against_float64_statement(hip_device):
    _check_chain(_lib.load(), hip_device, 1004, 50, 50, 1, 3, 7, 17, False, seed=5)


def test_ais_argument_checks_negative_without_touching_memory(emu_backend):
    raw = emu_backend.cdll
    p = ctypes.c_void_p(4096)                  # never dereferenced: every call below is refused before a launch
    odd = ctypes.c_void_p(4096 + 4)
    D = ctypes.c_double

    def chain(x=p, B=2, T=5, ws=p, V=30, H=16, nz=2, C=3, cur=p, logw=p, eps=p, beta=p, std=p, mu=None, lv=None, n_iter=4):
        return raw.lv_ais_chain_f32(x, B, T, ws, V, H, nz, C, cur, p, p, logw, p, eps, p, beta, std, mu, lv, n_iter, 1, None, None,
                                    None, None)

    def step(cond=p, rows=6, C=3, nz=2, u=p, logw=p, mu=None, lv=None):
        return raw.lv_ais_step_f32(cond, p, p, p, p, logw, p, u, D(0.5), p, ctypes.c_float(0.5), D(0.1), mu, lv, rows, C, nz, 0, None,
                                   None, None, None)
    for rc in (chain(x=None), chain(ws=None), chain(cur=None), chain(logw=None), chain(eps=None), chain(beta=None), chain(std=None),
               chain(mu=p), chain(lv=p), step(cond=None), step(u=None), step(logw=None), step(mu=p), step(lv=p)):
        assert rc == -1
    for rc in (chain(B=0), chain(B=-3), chain(C=0), chain(n_iter=-1), step(rows=0), step(C=0), step(rows=7), step(nz=0)):
        assert rc == -2
    for rc in (chain(H=129), chain(nz=65), chain(T=1)):
        assert rc == -4
    assert chain(ws=odd) == -3 and chain(logw=odd) == -3 and chain(beta=odd) == -3 and step(logw=odd) == -3
    lib = emu_backend
    for dims in ((1004, 50, 50, 1, 12), (97, 8, 16, 4, 2), (30, 4, 128, 64, 3), (30, 4, 129, 2, 5), (30, 4, 16, 65, 5),
                 (30, 4, 16, 2, 1), (20000, 512, 1024, 32, 40), (0, 4, 16, 2, 5)):
        assert lib.lv_ais_chain_f32_supported(*dims) == lib.lv_mh_chain_f32_supported(*dims), dims


# ---- 3. exact identities ------------------------------------------------------------------------------------------------------
def _identity_model(dev):
    V, ni, H, nz, B, T, C = 31, 6, 12, 3, 2, 5, 5
    vae = build_vae(V, ni, H, nz, dev, params=_params(V, ni, H, nz, 9))
    vae.eval()
    x = _batch(B, T, V, 10).to(dev)
    gen = torch.Generator().manual_seed(11)
    return vae, x, gen, (B, C, nz)


def test_ais_one_temperature_from_the_prior_is_the_conditional_log_likelihood(target):
    lib, dev = target
    vae, x, gen, (B, C, nz) = _identity_model(dev)
    z0 = torch.randn(B, C, nz, generator=gen).to(dev)
    noise = (z0, torch.randn(1, B, C, nz, generator=gen).to(dev), torch.rand(1, B, C, generator=gen).to(dev))
    nll, info = vae.nll_ais(x, chains=C, temps=1, std=0.3, noise=noise, return_info=True)
    assert info["route"] == "chain" and info["logw"].dtype == torch.float64
    assert _same(info["logw"], vae.decoder._hip.cond_ll(x, z0).double())              # bit-equal
    vae.fused_ais = False
    nll_s, info_s = vae.nll_ais(x, chains=C, temps=1, std=0.3, noise=noise, return_info=True)
    assert info_s["route"] == "step" and _same(info_s["logw"], vae.eval_cond_ll(x, z0).double())
    assert tuple(nll.shape) == (B,) and nll.dtype == torch.float32 and not nll.requires_grad


def test_ais_one_temperature_from_the_encoder_is_the_importance_weight(target):
    lib, dev = target
    vae, x, gen, (B, C, nz) = _identity_model(dev)
    with torch.no_grad():
        mu, lv = vae.encode_stats(x)
        z0 = (mu.unsqueeze(1) + torch.exp(0.5 * lv).unsqueeze(1) * torch.randn(B, C, nz, generator=gen).to(dev)).contiguous()
        want = (vae.eval_complete_ll(x, z0) - vae.eval_inference_dist(x, z0, (mu, lv))).double()
    noise = (z0, torch.randn(1, B, C, nz, generator=gen).to(dev), torch.rand(1, B, C, generator=gen).to(dev))
    iw = -(torch.logsumexp(want, dim=1) - math.log(C))                                # nll_iw on the same draws
    for fused in (True, False):
        vae.fused_ais = fused
        nll, info = vae.nll_ais(x, chains=C, temps=1, std=0.3, init="encoder", noise=noise, return_info=True)
        assert info["route"] == ("chain" if fused else "step")
        err = float((info["logw"] - want).abs().max())
        print("encoder init, one temperature, %s: largest |logw - (log p(z, x) - log q(z|x))| %.3e" % (info["route"], err))
        assert err <= 3e-4                     # three log-densities, each held to 1e-4 by the eval / grid tests
        assert float((nll.double() - iw).abs().max()) <= 3e-4


def test_ais_zero_proposal_scale_moves_nothing(target):
    lib, dev = target
    vae, x, gen, (B, C, nz) = _identity_model(dev)
    eng = vae.decoder._hip
    eng.ensure(dev)
    z0 = torch.randn(B, C, nz, generator=gen)
    mu0, lv0 = 0.4 * torch.randn(B, nz, generator=gen), 0.2 * torch.randn(B, nz, generator=gen)
    eps, u = torch.randn(N_IT, B, C, nz, generator=gen).to(dev), torch.rand(N_IT, B, C, generator=gen).to(dev)
    for m, l in ((None, None), (mu0.to(dev), lv0.to(dev))):
        r = eng.ais_chain(x, z0.to(dev), lambda i0, n: (eps[i0:i0 + n], u[i0:i0 + n]), torch.tensor(BETA, dtype=torch.float64, device=dev),
                          torch.zeros(N_IT, device=dev), m, l, iters_per_launch=5)
        assert _same(r["cur"], z0)
        g = r["g"].double().cpu()
        assert bool(((r["logw"].cpu() - g).abs() <= 1e-12 * g.abs().clamp(min=1.0)).all())
        if m is None:
            assert _same(r["g"], eng.cond_ll(x, z0.to(dev)))
    vae.fused_ais = False
    noise = (z0.to(dev), eps, u)
    _, info = vae.nll_ais(x, chains=C, temps=N_IT, schedule=BETA, std=0.0, noise=noise, return_info=True)
    g = vae.eval_cond_ll(x, z0.to(dev)).double().cpu()
    assert info["route"] == "step" and bool(((info["logw"].cpu() - g).abs() <= 1e-12 * g.abs().clamp(min=1.0)).all())


# ---- 4. against the truth at nz = 1 ---------------------------------------------------------------------------------------------
TRUTH = dict(V=17, ni=4, H=20, nz=1, B=3, T=7, C=64, temps=200, std=0.5, noise_seed=31)
_truth_cache = {}


def _truth():
    """Model, data, the grid truth, the injected noise and the float64 statement on it -- computed once."""
    if _truth_cache:
        return _truth_cache
    t = TRUTH
    Pm = O.random_params(t["V"], t["ni"], t["H"], t["nz"], seed=11, scale=1.0, emb_scale=0.5)
    x = O.synthetic_batch(t["B"], t["T"], t["V"], seed=12)
    cond = _cond64(Pm, x)
    grid = (torch.arange(1601, dtype=torch.float64) * 0.01 - 8.0).view(1, -1, 1).expand(t["B"], -1, -1)
    truth = torch.logsumexp(_prior64(grid) + cond(grid), dim=1) + math.log(0.01)
    gen = torch.Generator().manual_seed(t["noise_seed"])
    B, C, n = t["B"], t["C"], t["temps"]
    z0, eps, u = torch.randn(B, C, 1, generator=gen), torch.randn(n, B, C, 1, generator=gen), torch.rand(n, B, C, generator=gen)
    from vae_lagging_encoder_amd.modules import VAE
    beta = VAE.ais_schedule("sigmoid", n)
    ref = _ais64(cond, z0, eps, u, beta, [t["std"]] * n)
    lp, se = _estimate(ref["logw"])
    print("float64 statement: log p^ %s, truth %s, se %s, acceptance %.3f"
          % (lp.tolist(), truth.tolist(), se.tolist(), float(ref["flags"].float().mean())))
    _rule("float64 statement", lp, se, truth)
    _truth_cache.update(P=Pm, x=x, truth=truth, noise=(z0, eps, u), ref=ref)
    return _truth_cache


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


def test_ais_float64_statement_meets_the_rule_at_nz1():
    """The seed's own check, on the CPU: a bad seed is thereby told from a bad kernel."""
    _truth()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["chain", "step"])
def test_ais_against_the_grid_truth_at_nz1(hip_device, route):
    """(GPU only: 200 iterations of 192 chains are minutes on the thread-level emulator, a fraction of a second here.)"""
    dev = hip_device
    c = _truth()
    t = TRUTH
    vae = build_vae(t["V"], t["ni"], t["H"], t["nz"], dev, params=c["P"])
    vae.eval()
    vae.fused_ais = route == "chain"
    noise = tuple(v.to(dev) for v in c["noise"])
    nll, info = vae.nll_ais(c["x"].to(dev), chains=t["C"], temps=t["temps"], std=t["std"], noise=noise, return_info=True)
    assert info["route"] == route and info["iterations"] == t["temps"]
    lp, se = _estimate(info["logw"])
    assert float((nll.double().cpu() + lp).abs().max()) <= 1e-5 and float((info["se"].double().cpu() - se).abs().max()) <= 1e-9
    rate = float(info["accept_rate"].mean())
    assert abs(rate - float(info["accept_rate_iter"].mean())) < 1e-6 and 0.5 < rate < 0.95, rate
    _rule("nll_ais/" + route, lp, se, c["truth"])


# ---- 5. the drop-in against the reference's recorded chains -------------------------------------------------------------------
def _fixture_vae(fx, c, dev):
    V, ni, H, nz = (int(v) for v in fx[c + "/dims"])
    if c == "mid8":
        src, pre = load("beam_mid"), "param/"
    else:
        src, pre = fx, c + "/param/"
    vae = build_vae(V, ni, H, nz, dev, params={k: torch.from_numpy(src[pre + k]) for k in O.ALL_KEYS})
    vae.eval()
    return vae


def _check_fixture(dev, c, init, route, nb=None):
    """nb: the first nb sentences only (the emulator's budget); the rule is the same."""
    from vae_lagging_encoder_amd.modules import VAE
    fx = load("ais_small")
    vae = _fixture_vae(fx, c, dev)
    temps, transitions, C = (int(v) for v in fx[c + "/shape"])
    t = {k: torch.from_numpy(fx["%s/%s/%s" % (c, init, k)]) for k in ("z0", "eps", "u", "ratio", "accept", "logw_trace", "logw", "cur",
                                                                      "log_px")}
    x, std, beta = torch.from_numpy(fx[c + "/x"]), float(fx[c + "/std"]), fx[c + "/beta"].tolist()
    assert float(fx[c + "/tau"]) == TAU
    ours = VAE.ais_schedule("sigmoid", temps, transitions)
    assert len(ours) == len(beta) == temps * transitions + 1 and max(abs(a - b) for a, b in zip(ours, beta)) <= 1e-15
    margin = _margin(t["ratio"], t["u"])
    B_full = x.shape[0]
    assert 4 * int((margin.amin(dim=0) < TAU).sum()) <= B_full * C, "fixture case %s: more than 1/4 of its chains are marginal" % c
    nb = B_full if nb is None else nb
    vae.fused_ais = route == "chain"
    noise = (t["z0"][:nb].to(dev), t["eps"][:, :nb].contiguous().to(dev), t["u"][:, :nb].contiguous().to(dev))
    nll, info = vae.nll_ais(x[:nb].to(dev), chains=C, temps=temps, transitions=transitions, std=std, schedule=fx[c + "/beta_temps"].tolist(),
                            init=init, noise=noise, return_info=True)
    assert info["route"] == route and info["iterations"] == temps * transitions and tuple(nll.shape) == (nb,)
    full = _check_prefix("%s/%s/%s" % (c, init, route), info["ratios"], info["accepts"], info["logw_trace"], t["ratio"][:, :nb],
                         t["accept"][:, :nb], t["logw_trace"][:, :nb], margin[:, :nb], cap=False)
    for b, ch in full:
        assert abs(float(info["logw"][b, ch]) - float(t["logw"][b, ch])) <= RATIO_TOL
    for b in range(nb):                                    # every chain of the sentence compared to its end: the estimate too
        if all((b, ch) in full for ch in range(C)):
            assert abs(float(nll[b]) + float(t["log_px"][b])) <= RATIO_TOL + 1e-5      # (+ the float32 of the returned value)


@pytest.mark.parametrize("route", ["chain", "step"])
@pytest.mark.parametrize("init", ["prior", "encoder"])
@pytest.mark.parametrize("case,nb", [("nz1", 2), ("nz4", 2), ("mid8", 1)])
def test_dropin_against_reference_fixture_emulated(emu_backend, case, nb, init, route):
    _check_fixture("cpu", case, init, route, nb)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["chain", "step"])
@pytest.mark.parametrize("init", ["prior", "encoder"])
@pytest.mark.parametrize("case", ["nz1", "nz4", "mid8"])
def test_dropin_against_reference_fixture(hip_device, case, init, route):
    _check_fixture(hip_device, case, init, route)


# ---- 6. routing and refusals --------------------------------------------------------------------------------------------------
def _restate(vae, x, z0, eps, u, beta, stds, mu0=None, lv0=None):
    """The contract from eval_complete_ll and torch ops (float32 densities, float64 log-weight), on CPU copies of the state."""
    dev = x.device

    def lq0(z):
        if mu0 is None:
            return vae.eval_prior_dist(z.to(dev)).cpu()
        return vae.eval_inference_dist(x, z.to(dev), (mu0, lv0)).cpu()

    def gfn(z, lq):
        joint = vae.eval_complete_ll(x, z.to(dev)).cpu()
        return joint - lq
    with torch.no_grad():
        cur = z0.clone()
        lq = lq0(cur)
        g = gfn(cur, lq)
        logw = torch.zeros_like(g, dtype=torch.float64)
        ratios, flags, trace = [], [], []
        for it in range(eps.shape[0]):
            logw = logw + (beta[it + 1] - beta[it]) * g.double()
            trace.append(logw.clone())
            nxt = _propose(eps[it], stds[it], cur)
            lqn = lq0(nxt)
            gn = gfn(nxt, lqn)
            bf = torch.tensor(beta[it + 1], dtype=torch.float32)
            ratio = (lqn + bf * gn) - (lq + bf * g)
            acc = (ratio >= 0) | (u[it] < ratio.exp())
            cur = torch.where(acc.unsqueeze(-1), nxt, cur)
            g, lq = torch.where(acc, gn, g), torch.where(acc, lqn, lq)
            ratios.append(ratio)
            flags.append(acc)
    ratios = torch.stack(ratios)
    return ratios, torch.stack(flags), torch.stack(trace), _margin(ratios, u)


def _check_wide_decoder_takes_steps(dev):
    """H = 144 is outside the fused kernel's envelope: route "step", checked against the restatement under the margin rule."""
    V, ni, H, nz, B, T, C = 24, 6, 144, 3, 1, 4, 2
    vae = build_vae(V, ni, H, nz, dev, seed=21, model_scale=0.1, emb_scale=0.5)
    vae.eval()
    vae.decoder._hip.ensure(dev)
    assert not vae.decoder._hip.ais_chain_supported(T)
    x = _batch(B, T, V, 22).to(dev)
    gen = torch.Generator().manual_seed(23)
    z0, eps, u = torch.randn(B, C, nz, generator=gen), torch.randn(N_IT, B, C, nz, generator=gen), torch.rand(N_IT, B, C, generator=gen)
    nll, info = vae.nll_ais(x, chains=C, temps=N_IT, schedule=BETA, std=STDS, noise=(z0.to(dev), eps.to(dev), u.to(dev)), return_info=True)
    assert info["route"] == "step" and info["iterations"] == N_IT and tuple(nll.shape) == (B,)
    ratios, flags, trace, margin = _restate(vae, x, z0, eps, u, BETA, STDS)
    _check_prefix("H144/step", info["ratios"], info["accepts"], info["logw_trace"], ratios, flags, trace, margin)


def test_wide_decoder_takes_the_step_route_emulated(emu_backend):
    _check_wide_decoder_takes_steps(torch.device("cpu"))


@pytest.mark.gpu
def test_wide_decoder_takes_the_step_route(hip_device):
    _check_wide_decoder_takes_steps(hip_device)


def _check_routing(dev, other, lib, monkeypatch):
    V, ni, H, nz, B, T, C = 31, 6, 12, 2, 2, 5, 4
    Pm = _params(V, ni, H, nz, 9)
    x = _batch(B, T, V, 10).to(dev)
    chain_calls = []
    orig = E.LSTMDecoderEngine.ais_chain

    def counted(self, *a, **k):
        chain_calls.append(1)
        return orig(self, *a, **k)
    monkeypatch.setattr(E.LSTMDecoderEngine, "ais_chain", counted)
    gen = torch.Generator().manual_seed(3)
    z0, eps, u = torch.randn(B, C, nz, generator=gen), torch.randn(N_IT, B, C, nz, generator=gen), torch.rand(N_IT, B, C, generator=gen)
    noise = (z0.to(dev), eps.to(dev), u.to(dev))
    kw = dict(chains=C, temps=N_IT, schedule=BETA)

    vae = build_vae(V, ni, H, nz, dev, params=Pm)             # train mode, dropout 0.5 / 0.5
    with pytest.raises(ValueError, match="ais_std"):
        vae.nll_ais(x, **kw)
    vae.args.ais_std = 0.3
    nll, info = vae.nll_ais(x, return_info=True, **kw)        # a training-mode decoder with dropout: the step route
    assert info["route"] == "step" and chain_calls == [] and tuple(nll.shape) == (B,) and bool(torch.isfinite(nll).all())
    vae.eval()
    # the eval-mode decoder: the chain route, which agrees with the forced step route and the restatement under the rule
    nll_c, info_c = vae.nll_ais(x, std=STDS, noise=noise, return_info=True, **kw)
    assert info_c["route"] == "chain" and len(chain_calls) == 1 and tuple(info_c["accept_rate"].shape) == (B, C)
    assert tuple(info_c["accept_rate_iter"].shape) == (N_IT,) and tuple(info_c["se"].shape) == (B,) and not nll_c.requires_grad
    vae.fused_ais = False
    nll_s, info_s = vae.nll_ais(x, std=STDS, noise=noise, return_info=True, **kw)
    assert info_s["route"] == "step" and len(chain_calls) == 1
    ratios, flags, trace, margin = _restate(vae, x, z0, eps, u, BETA, STDS)
    for name, info in (("routing/chain", info_c), ("routing/step", info_s)):
        _check_prefix(name, info["ratios"], info["accepts"], info["logw_trace"], ratios, flags, trace, margin)
    vae.fused_ais = True
    # the same seed and iters_per_launch give the same tensor twice
    outs = []
    for _ in range(2):
        g2 = torch.Generator(device=dev).manual_seed(6)
        outs.append(vae.nll_ais(x, chains=2, temps=6, std=0.3, generator=g2, iters_per_launch=4))
    assert _same(outs[0], outs[1])
    with torch.no_grad():
        nll_e = vae.nll_ais(x, chains=3, temps=4, transitions=2, schedule="linear", init="encoder")
    assert tuple(nll_e.shape) == (B,) and bool(torch.isfinite(nll_e).all())
    # train mode without dropout draws no mask: the fused route
    vae0 = build_text_vae(V, ni, H, nz, dev, params=Pm, dropout_in=0.0, dropout_out=0.0)
    assert vae0.nll_ais(x, std=0.3, return_info=True, **kw)[1]["route"] == "chain"
    # refusals by value
    for bad in (dict(chains=0), dict(temps=0), dict(transitions=0), dict(schedule=[0.1] + BETA[1:]), dict(schedule=BETA[:-1] + [0.99]),
                dict(schedule=BETA[:5] + [0.2] + BETA[6:]), dict(schedule=BETA[:-1]), dict(schedule="cosine"), dict(init="posterior"),
                dict(std=-0.1), dict(std=[0.3] * (N_IT - 1)), dict(noise=(z0[:, :2].to(dev), noise[1], noise[2])),
                dict(noise=(noise[0], noise[1][:5], noise[2])), dict(noise=(noise[0], noise[1], noise[2][:, :, :1]))):
        args = dict(kw, std=0.3)
        args.update(bad)
        with pytest.raises(ValueError):
            vae.nll_ais(x, **args)
    # a starting point (or any noise) on another device never reaches a kernel
    reached = []

    def refuse(*a):
        reached.append(1)
        raise AssertionError("a kernel was launched with operands on different devices")
    for name in ("lv_mh_chain_prep_f32", "lv_ais_chain_f32", "lv_ais_step_f32"):
        monkeypatch.setattr(lib, name, refuse, raising=False)
    for bad in ((z0.to(other), noise[1], noise[2]), (noise[0], eps.to(other), noise[2]), (noise[0], noise[1], u.to(other))):
        for fused in (True, False):
            vae.fused_ais = fused
            with pytest.raises(_lib.LvaeError):
                vae.nll_ais(x, std=0.3, noise=bad, **kw)
    eng = vae.decoder._hip
    bt, st = torch.tensor(BETA, dtype=torch.float64, device=dev), torch.tensor(STDS, device=dev)
    with pytest.raises(_lib.LvaeError):
        eng.ais_chain(x, z0.to(other), lambda i0, n: (noise[1][i0:i0 + n], noise[2][i0:i0 + n]), bt, st, None, None)
    with pytest.raises(_lib.LvaeError):
        eng.ais_chain(x, noise[0], lambda i0, n: (eps[i0:i0 + n].to(other), noise[2][i0:i0 + n]), bt, st, None, None)
    with pytest.raises(_lib.LvaeError):
        eng.ais_chain(x, noise[0], lambda i0, n: (noise[1][i0:i0 + n], noise[2][i0:i0 + n]), bt, st, torch.zeros(B, nz).to(other),
                      torch.zeros(B, nz, device=dev))
    zr = torch.zeros(B, C, device=dev)
    with pytest.raises(_lib.LvaeError):
        E.ais_step(zr, z0.to(other), noise[0].clone(), zr.clone(), zr.clone(), zr.double(), zr.int(), None, 0.0, None, 0.0, 0.0, init=True)
    assert reached == []


def test_ais_routing_emulated(emu_backend, monkeypatch):
    _check_routing(torch.device("cpu"), "meta", emu_backend, monkeypatch)


@pytest.mark.gpu
def test_ais_routing(hip_device, monkeypatch):
    _check_routing(hip_device, "cpu", _lib.load(), monkeypatch)


def test_variable_length_pairs_take_the_step_route_or_are_refused_emulated(emu_backend):
    dev = torch.device("cpu")
    V, ni, H, nz, B, T = 31, 6, 12, 2, 3, 6
    Pm = _params(V, ni, H, nz, 9)
    x = _batch(B, T, V, 10)
    pair = (x, [6, 4, 5])
    var = build_text_vae(V, ni, H, nz, dev, params=Pm, varlen=True)
    var.eval()
    nll, info = var.nll_ais(pair, chains=2, temps=3, std=0.3, return_info=True)
    assert info["route"] == "step" and tuple(nll.shape) == (B,) and bool(torch.isfinite(nll).all())
    fixed = build_vae(V, ni, H, nz, dev, params=Pm)
    fixed.eval()
    with pytest.raises(ValueError, match="variable-length"):
        fixed.nll_ais(pair, chains=2, temps=3, std=0.3)


@pytest.mark.gpu
def test_pixelcnn_decoder_takes_the_step_route(hip_device):
    dev = hip_device
    vae = build_image_vae(dev, seed=3)
    vae.eval()
    nz, B, C, n = vae.nz, 2, 2, 4
    gen = torch.Generator().manual_seed(4)
    x = (torch.rand(B, 1, 28, 28, generator=gen) < 0.3).float().to(dev)
    z0, eps, u = torch.randn(B, C, nz, generator=gen), torch.randn(n, B, C, nz, generator=gen), torch.rand(n, B, C, generator=gen)
    nll, info = vae.nll_ais(x, chains=C, temps=n, std=0.05, schedule="linear", noise=(z0.to(dev), eps.to(dev), u.to(dev)),
                            return_info=True)
    assert info["route"] == "step" and tuple(nll.shape) == (B,) and bool(torch.isfinite(nll).all())
    assert bool(torch.isfinite(info["logw"]).all()) and info["iterations"] == n
    # the first increment is beta_1 g(z_0), g = log p(x|z_0) bit for bit under the prior
    first = info["logw_trace"][0].cpu()
    want = 0.25 * vae.eval_cond_ll(x, z0.to(dev)).double().cpu()
    assert bool(((first - want).abs() <= 1e-12 * want.abs().clamp(min=1.0)).all())


# ---- 7. evaluation ------------------------------------------------------------------------------------------------------------
def _check_evaluation(dev):
    V, ni, H, nz, T = 31, 6, 12, 2, 5
    vae = build_vae(V, ni, H, nz, dev, params=_params(V, ni, H, nz, 9))
    vae.eval()
    batches = [_batch(3, T, V, 40).to(dev), _batch(2, T + 1, V, 41).to(dev)]
    args = types.SimpleNamespace(ais_std=0.3)
    kw = dict(chains=4, temps=6)

    def gen():
        return torch.Generator(device=dev).manual_seed(8)
    nll, ppl = EV.calc_aisnll(vae, batches, args, np_rng=np.random.RandomState(0), generator=gen(), **kw)
    g2, tot = gen(), 0.0
    for i in np.random.RandomState(0).permutation(2):
        tot += float(vae.nll_ais(batches[i], std=0.3, generator=g2, **kw).sum())
    sents, words = 5, 3 * (T - 1) + 2 * T
    assert abs(nll - tot / sents) <= 1e-5 * abs(nll) and abs(ppl - math.exp(nll * sents / words)) <= 1e-9 * ppl
    gaps = EV.calc_inference_gaps(vae, batches, steps=3, np_rng=np.random.RandomState(1), ais=dict(kw, std=0.3, generator=gen()))
    assert sorted(gaps) == ["amortization_gap", "approximation_gap", "elbo_enc", "elbo_svi", "log_px", "n"] and gaps["n"] == sents
    total = gaps["log_px"] - gaps["elbo_enc"]
    assert abs(gaps["approximation_gap"] + gaps["amortization_gap"] - total) <= 1e-12 * max(1.0, abs(gaps["log_px"]))
    assert gaps["amortization_gap"] >= 0.0 and gaps["approximation_gap"] == gaps["log_px"] - gaps["elbo_svi"]
    with pytest.raises(ValueError):
        EV.calc_inference_gaps(vae, batches, steps=1, kl_weight=0.5, ais=dict(kw, std=0.3))
    loader = [(b, None) for b in batches]
    img = EV.image_calc_aisnll(vae, loader, args, generator=gen(), **kw)
    g3 = gen()
    want = sum(float(vae.nll_ais(b, std=0.3, generator=g3, **kw).sum()) for b in batches) / sents
    assert abs(img - want) <= 1e-5 * abs(want)


def test_ais_evaluation_emulated(emu_backend):
    _check_evaluation(torch.device("cpu"))


@pytest.mark.gpu
def test_ais_evaluation(hip_device):
    _check_evaluation(hip_device)

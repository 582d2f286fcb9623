"""Metropolis-Hastings sampling from the model posterior (csrc/lv_mh.hip, engine.LSTMDecoderEngine.mh_chain / engine.mh_step,
VAE.sample_from_posterior; reference modules/vae.py:218-254).

Kernel level (emulator build and MI355X through one fixture): lv_mh_step_f32 and lv_mh_chain_f32 against float64 statements
of the chain with proposals formed in float32; the argument checks; lv_mh_chain_f32_supported against
lv_dec_cond_ll_f32_supported.

Drop-in level: tests/golden/mh_small.npz (make_golden_mh.py: the reference's unmodified method on three seeded models, every
random draw recorded).  The comparison rule, TAU = 1e-3: an accept decision is discontinuous, two correct float32 evaluations
can disagree where the margin |log u - ratio| (ratio < 0) is tiny, and from there on the chains legitimately differ.  The grid
tests hold this decoder's log-densities within 1e-4 absolute of the reference, a ratio (a difference of two) within 2e-4; TAU
is five times that.
  * a chain (one sentence) is compared up to, not including, its first iteration whose RECORDED REFERENCE margin is under TAU;
  * on that prefix the accept flags are equal, the kept samples are BIT-equal to the reference's, and
    |ratio_ours - ratio_ref| <= 2e-4 (the largest value seen is printed);
  * at most 1/4 of a case's chains contain an under-TAU decision (a condition on the fixture, asserted by the generator and here).
The float64 statements of the kernel tests apply the same rule to their own float64 margins.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from helpers import build_vae, load
from oracle import text_vae_oracle as O
from vae_lagging_encoder_amd import _lib
from vae_lagging_encoder_amd import engine as E
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
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _propose(eps, std, cur):
    """The float32 two-rounding proposal (CPU tensors): the product is rounded, then the sum."""
    t = eps.float() * torch.tensor(std, dtype=torch.float32)
    return t + cur.float()


def _prior64(z):
    z = z.double()
    return -0.5 * (z * z).sum(-1) - 0.5 * z.shape[-1] * LOG_2PI


def _margin(ratio, u):
    """|log u - ratio| where ratio < 0, inf elsewhere (float64; u = 0 gives inf: such a draw never accepts a ratio < 0)."""
    ratio, u = ratio.double(), u.double()
    m = (torch.log(u) - ratio).abs()
    return torch.where(ratio < 0, m, torch.full_like(m, float("inf")))


# ---- 1. lv_mh_step_f32 ------------------------------------------------------------------------------------------------------
ROLES = ("plain", "pos_u_max", "underflow_u0", "nan")


def _step_case(lib, dev, rows, C, nz, role, keep, init, seed):
    """One launch on poisoned, over-allocated buffers; returns nothing, asserts everything."""
    g = torch.Generator().manual_seed(seed)
    std = 0.7
    B, nsamples, pad = rows // C, 4, 2
    cur = torch.randn(rows, nz, generator=g)
    prop = _propose(torch.randn(rows, nz, generator=g), std, cur)
    eps_next = torch.randn(rows, nz, generator=g)
    cur_ll = torch.randn(rows, generator=g) * 5 - 30
    counts = torch.randint(0, 50, (rows,), generator=g, dtype=torch.int32)
    target_ratio = torch.rand(rows, generator=g, dtype=torch.float64) * 5 - 3          # in [-3, 2)
    want_accept = torch.rand(rows, generator=g) < 0.5
    special = seed % rows
    if role == "pos_u_max":
        target_ratio[special] = 0.25
    elif role == "underflow_u0":
        target_ratio[special] = -200.0
    at = cur if init else prop
    cond = (cur_ll.double() + target_ratio - _prior64(at)).float()
    if role == "nan":
        cond[special] = float("nan")
    # the float64 statement from the operands the kernel actually gets
    terms = (at.double() ** 2).sum(-1) * 0.5 + 0.5 * nz * LOG_2PI + cond.double().abs()
    next_ll64 = _prior64(at) + cond.double()
    ratio64 = next_ll64 - cur_ll.double()
    bound = (nz + 2) * U24 * (terms + cur_ll.double().abs())
    p = torch.exp(torch.clamp(ratio64, max=0.0))
    can_reject = p < 0.9
    accept = torch.where(can_reject, want_accept, torch.ones_like(want_accept))
    u = torch.where(accept, 0.5 * p, p + 0.5 * (1 - p)).float()
    if role == "pos_u_max":
        u[special], accept[special] = 0.99999994, True
    elif role == "underflow_u0":
        u[special], accept[special] = 0.0, False
    elif role == "nan":
        u[special], accept[special] = 0.0, False
        bound[special] = 0.0
    ok = torch.ones(rows, dtype=torch.bool)
    if role == "nan":
        ok[special] = False
    if not init and bool(ok.any()):                          # every margin is large by construction
        mg = _margin(ratio64[ok], u[ok])
        assert float(mg.min()) > 0.05 and float(bound[ok].max()) < 5e-3

    def dv(t, fill):
        full = torch.full((t.shape[0] + pad,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
        full[:t.shape[0]] = t
        return full.to(dev)
    d_cond, d_prop, d_cur, d_ll, d_cnt = dv(cond, POISON), dv(prop, POISON), dv(cur, POISON), dv(cur_ll, POISON), dv(counts, IPOISON)
    d_u, d_eps = dv(u, POISON), dv(eps_next, POISON)
    d_samples = torch.full((B * nsamples * C + pad, nz), POISON).to(dev)
    d_ratio, d_flag = torch.full((rows + pad,), POISON).to(dev), torch.full((rows + pad,), IPOISON, dtype=torch.int32).to(dev)
    lib.lv_mh_step_f32(P(d_cond), P(d_prop), P(d_cur), P(d_ll), P(d_cnt), None if init else P(d_u), P(d_eps), std, P(d_samples),
                       rows, C, nz, nsamples, keep, 1 if init else 0, P(d_ratio), P(d_flag), E.stream_ptr(dev))
    got = {k: v.cpu() for k, v in dict(prop=d_prop, cur=d_cur, ll=d_ll, cnt=d_cnt, samples=d_samples, ratio=d_ratio,
                                       flag=d_flag).items()}
    # rows beyond the count keep their poison
    for k in ("prop", "cur", "ll", "ratio"):
        assert bool((got[k][rows:] == POISON).all()), k
    assert bool((got["cnt"][rows:] == IPOISON).all()) and bool((got["flag"][rows:] == IPOISON).all())
    if init:
        assert _same(got["cur"][:rows], cur)
        assert bool((got["cnt"][:rows] == 0).all())
        if role == "nan":
            assert math.isnan(float(got["ll"][special]))
        err = (got["ll"][:rows].double() - next_ll64).abs()
        assert bool((err[ok] <= (nz + 2) * U24 * terms[ok]).all()), float(err[ok].max())
        assert _same(got["prop"][:rows], _propose(eps_next, std, cur))
        assert bool((got["samples"] == POISON).all()) and bool((got["ratio"] == POISON).all())
        return
    assert torch.equal(got["flag"][:rows] != 0, accept), role                       # decisions are exact
    new_cur = torch.where(accept.unsqueeze(1), prop, cur)
    assert _same(got["cur"][:rows], new_cur)                                        # selected, bit for bit
    assert torch.equal(got["cnt"][:rows], counts + accept.to(torch.int32))
    rej = ~accept
    assert _same(got["ll"][:rows][rej], cur_ll[rej])                                # a rejected row's cur_ll is untouched
    assert bool(torch.isfinite(got["ll"][:rows]).all())                             # ... a NaN score included
    assert bool(((got["ll"][:rows].double() - next_ll64).abs()[accept] <= ((nz + 2) * U24 * terms)[accept]).all())
    assert bool(((got["ratio"][:rows].double() - ratio64).abs()[ok] <= bound[ok]).all())
    if role == "nan":
        assert math.isnan(float(got["ratio"][special]))
    assert _same(got["prop"][:rows], _propose(eps_next, std, new_cur))              # the next proposal
    smp = got["samples"][:B * nsamples * C].view(B, nsamples, C, nz)
    for k in range(nsamples):
        if k == keep:
            assert _same(smp[:, k], new_cur.view(B, C, nz))
        else:
            assert bool((smp[:, k] == POISON).all())                                # slots that are not due keep their poison
    assert bool((got["samples"][B * nsamples * C:] == POISON).all())


@pytest.mark.parametrize("nz", [1, 5, 32, 67])
@pytest.mark.parametrize("rows,C", [(1, 1), (3, 3), (70, 10)])
def test_mh_step_against_float64_statement(target, rows, C, nz):
    lib, dev = target
    seed = 1000 * rows + nz
    for i, role in enumerate(ROLES):
        # keep: none (e.g. one past burn-in with thin 3), the first kept sample, the last
        _step_case(lib, dev, rows, C, nz, role, keep=(-1, 0, 3, -1)[i], init=False, seed=seed + i)
    _step_case(lib, dev, rows, C, nz, "plain", keep=-1, init=True, seed=seed + 7)
    _step_case(lib, dev, rows, C, nz, "nan", keep=-1, init=True, seed=seed + 8)


# ---- 2. lv_mh_chain_f32 -----------------------------------------------------------------------------------------------------
def _params(V, ni, H, nz, seed):
    return O.random_params(V, ni, H, nz, seed=seed, scale=0.3, emb_scale=0.5)


def _batch(B, T, V, seed):
    x = O.synthetic_batch(B, T, V, seed=seed)
    if T > 2:
        x[0, T - 2:] = 0
    return x


def _joint64(P64, x, z):
    return _prior64(z) - O.decoder_reconstruct_error(P64, x, z.double())


def _chain64(Pm, x, z0, eps, u, std, burn_in, thin, nsamples):
    """The chain with float64 log-densities and float32 proposals -> samples [B][ns][C][nz] f32, ratios, flags, margins
    [n][B][C], final cur, cur_ll, counts."""
    P64 = {k: v.double() for k, v in Pm.items()}
    cur = z0.clone().float()
    cur_ll = _joint64(P64, x, cur)
    samples, ratios, flags = [], [], []
    for it in range(eps.shape[0]):
        nxt = _propose(eps[it], std, cur)
        next_ll = _joint64(P64, x, nxt)
        ratio = next_ll - cur_ll
        acc = (ratio >= 0) | (u[it].double() < ratio.exp())
        cur = torch.where(acc.unsqueeze(-1), nxt, cur)
        cur_ll = torch.where(acc, next_ll, cur_ll)
        ratios.append(ratio)
        flags.append(acc)
        if it >= burn_in and (it - burn_in) % thin == 0 and (it - burn_in) // thin < nsamples:
            samples.append(cur.clone())
    ratios, flags = torch.stack(ratios), torch.stack(flags)
    return torch.stack(samples, dim=1), ratios, flags, _margin(ratios, u), cur, cur_ll, flags.sum(0)


def _run_chain(eng, x, z0, eps, u, std, burn_in, thin, nsamples, per):
    def draw(i0, n):
        return eps[i0:i0 + n], u[i0:i0 + n]
    return eng.mh_chain(x, z0, draw, burn_in, thin, nsamples, std, iters_per_launch=per)


def _check_prefix(name, r, ref_samples, ref_ratio, ref_flag, margin, burn_in, thin, cap=True):
    """The comparison rule on every chain of r (mh_chain's / sample_from_posterior's arrays, [n][B][C] and [B][ns][C][nz]);
    returns (number of chains compared to the end, largest ratio difference on the compared prefixes)."""
    n, B, C = ref_ratio.shape
    ratios, flags, samples = r["ratios"].cpu(), r["flags"].cpu(), r["samples"].cpu()
    worst, full = 0.0, []
    for b in range(B):
        for c in range(C):
            low = (margin[:, b, c] < TAU).nonzero()
            stop = int(low[0]) if low.numel() else n
            if stop == n:
                full.append((b, c))
            assert torch.equal(flags[:stop, b, c] != 0, ref_flag[:stop, b, c] != 0), (name, b, c)
            if stop:
                worst = max(worst, float((ratios[:stop, b, c].double() - ref_ratio[:stop, b, c].double()).abs().max()))
            for k in range(samples.shape[1]):
                if burn_in + k * thin < stop:
                    assert _same(samples[b, k, c], ref_samples[b, k, c]), (name, b, c, k)
    print("%s: %d of %d chains compared to the end, largest |ratio - ratio_ref| on the compared prefixes %.3e"
          % (name, len(full), B * C, worst))
    assert worst <= RATIO_TOL, (name, worst)
    if cap:
        assert 4 * (B * C - len(full)) <= B * C, "%s: more than 1/4 of the chains are marginal -- pick another seed, not another TAU" % name
    return full, worst


# V, ni, H, nz, B, T, chains -- every H in {5, 20, 50, 100} (all four padded sizes), nz in {1, 3, 8, 64}, V in {17, 60},
# chains in {1, 5, 16, 17} (a ragged second tile), B in {1, 3}, T in {2, 7}
CHAIN_CASES = [
    (17, 4, 5, 1, 1, 2, 1),
    (17, 4, 5, 3, 3, 7, 5),
    (60, 8, 20, 8, 1, 7, 16),
    (60, 8, 20, 1, 3, 2, 17),
    (17, 6, 50, 64, 1, 7, 5),
    (17, 6, 50, 3, 1, 7, 17),
    (17, 6, 50, 8, 3, 2, 16),
    (60, 8, 100, 8, 1, 7, 1),
    (17, 4, 100, 64, 3, 2, 5),
    (60, 8, 100, 1, 3, 2, 17),
    (60, 6, 5, 64, 3, 7, 1),
    (17, 4, 20, 3, 1, 2, 16),
]
N_IT, BURN, THIN, NS = 12, 4, 2, 4                      # keeps at iterations 4, 6, 8, 10; the last iteration keeps nothing


def _check_chain(lib, dev, V, ni, H, nz, B, T, C, seed):
    Pm = _params(V, ni, H, nz, seed)
    vae = build_vae(V, ni, H, nz, dev, params=Pm)
    vae.eval()
    x = _batch(B, T, V, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    std = 0.4
    z0 = torch.randn(B, C, nz, generator=g)
    eps = torch.randn(N_IT, B, C, nz, generator=g)
    u = torch.rand(N_IT, B, C, generator=g)
    ref = _chain64(Pm, x, z0, eps, u, std, BURN, THIN, NS)
    eng = vae.decoder._hip
    eng.ensure(dev)
    assert lib.lv_mh_chain_f32_supported(V, ni, H, nz, T) == 1
    xd, zd, ed, ud = x.to(dev), z0.to(dev), eps.to(dev), u.to(dev)
    one = _run_chain(eng, xd, zd, ed, ud, std, BURN, THIN, NS, N_IT)
    name = "chain V%d H%d nz%d B%d T%d C%d" % (V, H, nz, B, T, C)
    full, _ = _check_prefix(name, one, ref[0], ref[1], ref[2], ref[3], BURN, THIN)
    for b, c in full:                                      # chains compared to the end: the final state too
        assert _same(one["cur"][b, c], ref[4][b, c])
        assert abs(float(one["log_joint"][b, c]) - float(ref[5][b, c])) <= RATIO_TOL
        assert int(one["accepts"][b, c]) == int(ref[6][b, c])
    keys = ("samples", "cur", "log_joint", "accepts", "ratios", "flags")
    # the cut into launches does not matter, a repeated run is bit-identical
    for per in (1, 5, 12):
        again = _run_chain(eng, xd, zd, ed, ud, std, BURN, THIN, NS, per)
        for k in keys:
            assert _same(again[k], one[k]), (name, per, k)
    return vae, xd, zd, ed, ud, std, one


@pytest.mark.parametrize("V,ni,H,nz,B,T,C", CHAIN_CASES)
def test_mh_chain_against_float64_statement_cuts_and_reruns(target, V, ni, H, nz, B, T, C):
    lib, dev = target
    _check_chain(lib, dev, V, ni, H, nz, B, T, C, seed=V + 7 * H + nz + C)


def test_mh_chain_a_chain_does_not_depend_on_its_tile(target):
    lib, dev = target
    vae, xd, zd, ed, ud, std, all16 = _check_chain(lib, dev, 60, 8, 20, 3, 2, 7, 16, seed=77)
    eng = vae.decoder._hip
    for c in (0, 9, 15):
        alone = _run_chain(eng, xd, zd[:, c:c + 1].contiguous(), ed[:, :, c:c + 1].contiguous(), ud[:, :, c:c + 1].contiguous(),
                           std, BURN, THIN, NS, 5)
        assert _same(alone["samples"][:, :, 0], all16["samples"][:, :, c])
        assert _same(alone["cur"][:, 0], all16["cur"][:, c]) and _same(alone["log_joint"][:, 0], all16["log_joint"][:, c])
        assert _same(alone["accepts"][:, 0], all16["accepts"][:, c]) and _same(alone["ratios"][:, :, 0], all16["ratios"][:, :, c])


@pytest.mark.gpu
def test_mh_chain_toy_vocabulary_against_float64_statement(hip_device):
    _check_chain(_lib.load(), hip_device, 1004, 50, 50, 1, 3, 7, 17, seed=5)
    _check_chain(_lib.load(), hip_device, 1004, 50, 50, 8, 1, 7, 5, seed=6)


# ---- 3. argument checks ---------------------------------------------------------------------------------------------------------
def test_mh_argument_checks_negative_without_touching_memory(emu_backend):
    raw = emu_backend.cdll
    p = ctypes.c_void_p(4096)                  # never dereferenced: every call below is refused before a launch
    odd = ctypes.c_void_p(4096 + 4)

    def prep(x=p, B=2, T=5, w=p, V=30, ni=4, H=16, nz=2, ws=p):
        return raw.lv_mh_chain_prep_f32(x, B, T, w, w, w, w, w, w, w, V, ni, H, nz, ws, None)

    def chain(x=p, B=2, T=5, ws=p, V=30, H=16, nz=2, C=3, cur=p, n_iter=4, samples=p, eps=p):
        return raw.lv_mh_chain_f32(x, B, T, ws, V, H, nz, C, cur, p, p, eps, p, n_iter, 0, 1, 1, 2, 0.5, 1, samples, None, None, None)

    def step(cond=p, rows=6, C=3, nz=2, u=p, keep=0, nsamples=2, samples=p):
        return raw.lv_mh_step_f32(cond, p, p, p, p, u, p, 0.5, samples, rows, C, nz, nsamples, keep, 0, None, None, None)
    for rc in (prep(x=None), prep(w=None), prep(ws=None), chain(x=None), chain(ws=None), chain(cur=None), chain(samples=None),
               chain(eps=None), step(cond=None), step(u=None), step(samples=None)):
        assert rc == -1
    for rc in (prep(B=0), chain(B=0), chain(B=-3), chain(C=0), chain(C=-1), chain(n_iter=-1), step(rows=0), step(C=0), step(rows=7),
               step(nz=0), step(keep=2), step(keep=-2)):
        assert rc == -2
    for rc in (prep(H=129), prep(nz=65), prep(T=1), chain(H=129), chain(nz=65), chain(T=1)):
        assert rc == -4
    assert prep(ws=odd) == -3 and chain(ws=odd) == -3
    lib = emu_backend
    for dims in ((1004, 50, 50, 1, 12), (97, 8, 16, 4, 2), (30, 4, 128, 64, 3), (30, 4, 129, 2, 5), (30, 4, 16, 65, 5),
                 (30, 4, 16, 2, 1), (20000, 512, 1024, 32, 40), (0, 4, 16, 2, 5)):
        assert lib.lv_mh_chain_f32_supported(*dims) == lib.lv_dec_cond_ll_f32_supported(*dims), dims
    V, ni, H, nz, T = 1004, 50, 50, 1, 12
    hp, vp, nzp = 64, 1008, 4                  # the grid kernel's workspace: padded weight images + the input projection [B][T-1][4][Hp]
    assert lib.lv_mh_chain_f32_ws_floats(V, H, nz, 16, T) == 4 * hp * hp + vp * hp + 4 * hp * nzp + hp * nzp + 16 * (T - 1) * 4 * hp
    assert lib.lv_mh_chain_f32_ws_floats(V, H, nz, 16, 1) == 0


# ---- 4. the drop-in against the reference's recorded chains -----------------------------------------------------------------------
def _fixture_case(fx, c, dev):
    V, ni, H, nz = (int(v) for v in fx[c + "/dims"])
    if c == "mid8":
        src, pre = load("beam_mid"), "param/"
    else:
        src, pre = fx, c + "/param/"
    Pm = {k: torch.from_numpy(src[pre + k]) for k in O.ALL_KEYS}
    vae = build_vae(V, ni, H, nz, dev, params=Pm)
    vae.eval()
    t = {k: torch.from_numpy(fx[c + "/" + k]) for k in ("x", "z0", "eps", "u", "samples", "ratio", "accept")}
    burn_in, thin, nsamples = (int(v) for v in fx[c + "/chain"])
    return vae, t, burn_in, thin, nsamples, float(fx[c + "/std"])


def _check_fixture(dev, c, route, nb=None, nsamples=None, short=None):
    """nb / nsamples: the first nb sentences and kept samples only (the emulator's budget); the rule is the same.
    short = (burn_in, thin): a chain that keeps earlier than the recorded one does.  The draws, and with them the proposals,
    ratios and flags, do not depend on when samples are kept; what the reference held at the other iterations is the
    recorded flags replayed on the recorded draws (the replay the generator asserts to reproduce the reference bit for bit)."""
    fx = load("mh_small")
    vae, t, burn_in, thin, ns_full, std = _fixture_case(fx, c, dev)
    if short is not None:
        assert nsamples is not None
        cur, states = t["z0"].clone(), []
        for it in range(t["eps"].shape[0]):
            cur = torch.where((t["accept"][it] != 0).unsqueeze(-1), _propose(t["eps"][it], std, cur), cur)
            states.append(cur.clone())
        k_rec = torch.stack([states[burn_in + k * thin] for k in range(ns_full)], dim=1)
        assert _same(k_rec, t["samples"])
        burn_s, thin_s = short
        t["samples"] = torch.stack([states[burn_s + k * thin_s] for k in range(nsamples)], dim=1)
        full_total = burn_in + ns_full * thin
        burn_in, thin, ns_full = burn_s, thin_s, (full_total - burn_s) // thin_s
    margin = _margin(t["ratio"], t["u"])
    n_full, B_full = margin.shape[0], margin.shape[1]
    assert n_full >= burn_in + ns_full * thin and float(fx[c + "/tau"]) == TAU
    marginal = int((margin.amin(dim=0) < TAU).sum())
    assert 4 * marginal <= B_full, "fixture case %s: more than 1/4 of its chains are marginal" % c
    rate = float(t["accept"].float().mean())
    assert 0.2 <= rate <= 0.9, rate
    nb = B_full if nb is None else nb
    ns = ns_full if nsamples is None else nsamples
    total = burn_in + ns * thin
    vae.args.mh_burn_in, vae.args.mh_thin, vae.args.mh_std = burn_in, thin, std
    vae.fused_mh = route == "chain"
    noise = (t["z0"][:nb].to(dev), t["eps"][:total, :nb].contiguous().to(dev), t["u"][:total, :nb].contiguous().to(dev))
    samples, info = vae.sample_from_posterior(t["x"][:nb].to(dev), ns, noise=noise, return_info=True)
    nz = t["z0"].shape[-1]
    assert tuple(samples.shape) == (nb, ns, 1, nz) and samples.dtype == torch.float32 and samples.device.type == torch.device(dev).type
    assert info["route"] == route and info["iterations"] == total
    r = {"samples": samples, "ratios": info["ratios"], "flags": info["accepts"]}
    full, _ = _check_prefix("%s/%s" % (c, route), r, t["samples"][:nb, :ns], t["ratio"][:total, :nb], t["accept"][:total, :nb],
                            margin[:total, :nb], burn_in, thin, cap=False)
    for b, ch in full:
        want = float(t["accept"][:total, b, ch].float().mean())
        assert abs(float(info["accept_rate"][b, ch]) - want) < 1e-6
    assert tuple(info["accept_rate"].shape) == (nb, 1) and tuple(info["log_joint"].shape) == (nb, 1)


@pytest.mark.parametrize("case,nb,ns", [("nz1", 3, None), ("nz4", 3, None), ("mid8", 1, 2)])
def test_dropin_chain_route_against_reference_fixture_emulated(emu_backend, case, nb, ns):
    _check_fixture("cpu", case, "chain", nb, ns)


@pytest.mark.parametrize("case,nb,ns,short", [("nz1", None, 10, None), ("nz4", None, 10, None), ("mid8", 1, 2, (2, 2))])
def test_dropin_step_route_against_reference_fixture_emulated(emu_backend, case, nb, ns, short):
    _check_fixture("cpu", case, "step", nb, ns, short)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["chain", "step"])
@pytest.mark.parametrize("case", ["nz1", "nz4", "mid8"])
def test_dropin_against_reference_fixture(hip_device, case, route):
    _check_fixture(hip_device, case, route)


# ---- 5. routing ---------------------------------------------------------------------------------------------------------------
def _mh_args(vae, burn_in=4, thin=2, std=0.3):
    vae.args.mh_burn_in, vae.args.mh_thin, vae.args.mh_std = burn_in, thin, std
    return vae


def _check_routing(dev, other, lib, monkeypatch):
    V, ni, H, nz, B, T = 31, 6, 12, 2, 2, 5
    Pm = _params(V, ni, H, nz, 9)
    x = _batch(B, T, V, 10).to(dev)
    chain_calls = []
    orig = E.LSTMDecoderEngine.mh_chain

    def counted(self, *a, **k):
        chain_calls.append(1)
        return orig(self, *a, **k)
    monkeypatch.setattr(E.LSTMDecoderEngine, "mh_chain", counted)

    vae = build_vae(V, ni, H, nz, dev, params=Pm)             # train mode, dropout 0.5 / 0.5
    with pytest.raises(ValueError, match="mh_burn_in.*mh_thin.*mh_std"):
        vae.sample_from_posterior(x, 3)
    vae.args.mh_burn_in, vae.args.mh_thin = 4, 2
    with pytest.raises(ValueError, match="mh_std"):
        vae.sample_from_posterior(x, 3)
    _mh_args(vae)
    s, info = vae.sample_from_posterior(x, 3, return_info=True)
    assert info["route"] == "step" and chain_calls == [] and tuple(s.shape) == (B, 3, 1, nz)
    vae.eval()

    def forbidden(*a, **k):
        raise AssertionError("route 'chain' must not call decoder.log_probability")
    monkeypatch.setattr(vae.decoder, "log_probability", forbidden)
    s, info = vae.sample_from_posterior(x, 3, chains=4, return_info=True)
    assert info["route"] == "chain" and len(chain_calls) == 1
    assert tuple(s.shape) == (B, 3, 4, nz) and tuple(info["accept_rate"].shape) == (B, 4) and info["iterations"] == 10
    assert not s.requires_grad and bool(torch.isfinite(s).all())
    # the same seed and iters_per_launch give the same tensor twice (a different cut consumes the generator differently)
    outs = []
    for _ in range(2):
        torch.manual_seed(5)
        gen = torch.Generator(device=dev).manual_seed(6)
        outs.append(vae.sample_from_posterior(x, 3, chains=2, generator=gen, iters_per_launch=4))
    assert _same(outs[0], outs[1])
    monkeypatch.undo()
    monkeypatch.setattr(E.LSTMDecoderEngine, "mh_chain", counted)
    vae.fused_mh = False
    n_chain = len(chain_calls)
    s, info = vae.sample_from_posterior(x, 3, chains=4, return_info=True)
    assert info["route"] == "step" and len(chain_calls) == n_chain and tuple(s.shape) == (B, 3, 4, nz)
    vae.fused_mh = True
    # train mode without dropout draws no mask: the fused route
    vae0 = _mh_args(build_text_vae(V, ni, H, nz, dev, params=Pm, dropout_in=0.0, dropout_out=0.0))
    assert vae0.sample_from_posterior(x, 2, return_info=True)[1]["route"] == "chain"
    # a starting point (or any noise) on another device never reaches a kernel
    reached = []

    def refuse(*a):
        reached.append(1)
        raise AssertionError("a kernel was launched with operands on different devices")
    for name in ("lv_mh_chain_prep_f32", "lv_mh_chain_f32", "lv_mh_step_f32"):
        monkeypatch.setattr(lib, name, refuse, raising=False)
    total = 4 + 3 * 2
    z0, eps, u = torch.zeros(B, 1, nz), torch.zeros(total, B, 1, nz), torch.zeros(total, B, 1)
    for bad in ((z0.to(other), eps.to(dev), u.to(dev)), (z0.to(dev), eps.to(other), u.to(dev)),
                (z0.to(dev), eps.to(dev), u.to(other))):
        for fused in (True, False):
            vae.fused_mh = fused
            with pytest.raises(_lib.LvaeError):
                vae.sample_from_posterior(x, 3, noise=bad)
    with pytest.raises(_lib.LvaeError):
        vae.decoder._hip.mh_chain(x, z0.to(other), lambda i0, n: (eps[i0:i0 + n].to(dev), u[i0:i0 + n].to(dev)), 4, 2, 3, 0.3)
    with pytest.raises(_lib.LvaeError):
        vae.decoder._hip.mh_chain(x, z0.to(dev), lambda i0, n: (eps[i0:i0 + n].to(other), u[i0:i0 + n].to(dev)), 4, 2, 3, 0.3)
    with pytest.raises(_lib.LvaeError):
        E.mh_step(torch.zeros(B, 1, device=dev), z0.to(other), z0.to(dev), torch.zeros(B, 1, device=dev),
                  torch.zeros(B, 1, dtype=torch.int32, device=dev), None, None, 0.3, torch.zeros(B, 3, 1, nz, device=dev), -1, init=True)
    assert reached == []


def test_dropin_routing_emulated(emu_backend, monkeypatch):
    _check_routing(torch.device("cpu"), "meta", emu_backend, monkeypatch)


@pytest.mark.gpu
def test_dropin_routing(hip_device, monkeypatch):
    _check_routing(hip_device, "cpu", _lib.load(), monkeypatch)


def _check_wide_decoder_takes_steps(dev):
    """H = 144 is outside the fused kernel's envelope: route "step", checked against a per-iteration restatement written here
    from eval_complete_ll and torch ops, under the margin rule on the restatement's own margins."""
    V, ni, H, nz, B, T, C = 24, 6, 144, 3, 1, 4, 2
    vae = _mh_args(build_vae(V, ni, H, nz, dev, seed=21, model_scale=0.1, emb_scale=0.5), burn_in=2, thin=2, std=0.4)
    vae.eval()
    vae.decoder._hip.ensure(dev)
    assert not vae.decoder._hip.cond_ll_supported(T)
    x = _batch(B, T, V, 22).to(dev)
    g = torch.Generator().manual_seed(23)
    n = 10
    z0, eps, u = torch.randn(B, C, nz, generator=g), torch.randn(n, B, C, nz, generator=g), torch.rand(n, B, C, generator=g)
    samples, info = vae.sample_from_posterior(x, 4, chains=C, noise=(z0.to(dev), eps.to(dev), u.to(dev)), return_info=True)
    assert info["route"] == "step" and info["iterations"] == n and tuple(samples.shape) == (B, 4, C, nz)
    with torch.no_grad():
        cur = z0.clone()
        cur_ll = vae.eval_complete_ll(x, cur.to(dev)).cpu()
        kept, ratios, flags = [], [], []
        for it in range(n):
            nxt = _propose(eps[it], 0.4, cur)
            next_ll = vae.eval_complete_ll(x, nxt.to(dev)).cpu()
            ratio = next_ll - cur_ll
            acc = (ratio >= 0) | (u[it] < ratio.exp())
            cur, cur_ll = torch.where(acc.unsqueeze(-1), nxt, cur), torch.where(acc, next_ll, cur_ll)
            ratios.append(ratio)
            flags.append(acc)
            if it >= 2 and (it - 2) % 2 == 0:
                kept.append(cur.clone())
    ratios, flags = torch.stack(ratios), torch.stack(flags)
    r = {"samples": samples, "ratios": info["ratios"], "flags": info["accepts"]}
    _check_prefix("H144/step", r, torch.stack(kept, dim=1), ratios, flags, _margin(ratios, u), 2, 2)


def test_wide_decoder_takes_the_step_route_emulated(emu_backend):
    _check_wide_decoder_takes_steps(torch.device("cpu"))


@pytest.mark.gpu
def test_wide_decoder_takes_the_step_route(hip_device):
    _check_wide_decoder_takes_steps(hip_device)


@pytest.mark.gpu
def test_pixelcnn_decoder_takes_the_step_route(hip_device):
    dev = hip_device
    vae = build_image_vae(dev, seed=3)
    vae.eval()
    nz, B, burn_in, thin, ns, std = vae.nz, 2, 2, 1, 2, 0.05
    g = torch.Generator().manual_seed(4)
    x = (torch.rand(B, 1, 28, 28, generator=g) < 0.3).float().to(dev)
    n = burn_in + ns * thin
    with torch.no_grad():
        z0 = vae.encoder.sample(x, 1)[0].float().cpu()
    eps, u = torch.randn(n, B, 1, nz, generator=g), torch.rand(n, B, 1, generator=g)
    samples, info = vae.sample_from_posterior(x, ns, burn_in=burn_in, thin=thin, std=std,
                                              noise=(z0.to(dev), eps.to(dev), u.to(dev)), return_info=True)
    assert info["route"] == "step" and tuple(samples.shape) == (B, ns, 1, nz) and bool(torch.isfinite(samples).all())
    assert bool(torch.isfinite(info["log_joint"]).all())
    # every kept sample is the starting point or a proposal: replay the selects with the returned flags
    cur, flags, k = z0.clone(), info["accepts"].cpu() != 0, 0
    for it in range(n):
        cur = torch.where(flags[it].unsqueeze(-1), _propose(eps[it], std, cur), cur)
        if it >= burn_in and (it - burn_in) % thin == 0:
            assert _same(samples[:, k], cur)
            k += 1
    assert k == ns

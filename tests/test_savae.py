"""Semi-amortized training (SA-VAE): lv_svi_rec_step_f32, lv_savae_adjoint_f32, lv_savae_hvp_f32 (csrc/lv_savae.hip),
engine.LSTMDecoderEngine.savae_forward / savae_backward, VAE.loss_savae, trainer.SemiAmortizedTextTrainer and
TextTrainingLoop(args.svi_steps).

Kernel and engine tests run on the emulator build and on the MI355X through test_svi_refine.py's `target` fixture.  References:
float64 statements of the definition written here (kernel level); tests/golden/savae_small.npz (make_golden_savae.py: the
reference's unmodified classes under torch autograd -- the exact gradient through the K refinement steps in float64, and the
finite-difference scheme in float64 and float32); the generic route (fused_savae = False) as the second oracle.

Bounds.  loss / rec / kl: parity_common.RTOL.  Iterates lambda_k: test_svi_refine.py's rule (the larger of RTOL * max|lambda_k|
and 4 x the recorded float32-vs-float64 deviation of the reference's own trajectory).  Gradients, per tensor and max-norm, against
the fixture's float64 scheme: the larger of GRAD_RTOL * max|tensor| and 4 x the recorded deviation of the reference's own float32
run of the scheme (DESIGN.md 3.7's rule for compounded rounding); fused against generic: the first term alone.
"""
import argparse
import math

import numpy as np
import pytest
import torch

from helpers import ALL_KEYS, build_vae, load, rel_err
from parity_common import GRAD_RTOL, RTOL
from test_svi_refine import (POISON, U, _assert_same_state, _batch, _guarded, _guards_intact, _s, _same, _small_vae, _state,  # noqa: F401
                             _svi_ref, spying, target)
from vae_lagging_encoder_amd import engine as E
from vae_lagging_encoder_amd.engine import P

SHAPES = [(B, ns, nz) for B in (1, 5, 33) for ns in (1, 3) for nz in (1, 4, 32, 33)]
NAN = float("nan")


def _clip_rows(B, case):
    """Per-sentence gradient scale: rows with (b + case) even far above the clip, the others far below it."""
    return torch.where((torch.arange(B) + case) % 2 == 0, torch.tensor(50.0), torch.tensor(0.01))


# ---- 1. the recording step ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,ns,nz", SHAPES)
def test_rec_step_equals_svi_step_and_records(target, B, ns, nz):
    lib, dev = target
    beta, lr, clip = 0.7, 0.8, 5.0
    for case, (parts, mom) in enumerate([(1, 0.0), (3, 0.5)]):
        g = torch.Generator().manual_seed(2000 * B + 100 * ns + nz + case)
        phi = torch.randn(B, 2 * nz, generator=g) * 0.5
        vel = torch.randn(B, 2 * nz, generator=g) * 0.3
        eps = torch.randn(B, ns, nz, generator=g)
        rec = torch.rand(B * ns, generator=g) * 30 + 5
        kl = torch.rand(B, generator=g) * 2
        dzp = torch.randn(parts, B * ns, nz, generator=g) * _clip_rows(B, case).repeat_interleave(ns).view(1, B * ns, 1)
        _, g64, active, _, _ = _svi_ref(rec, dzp, eps, kl, beta, lr, mom, clip, phi, vel)
        if B > 1:
            assert bool(active.any()) and bool((~active).any()), "both clip branches in one batch"
        d_dz, d_eps, d_rec, d_kl = dzp.to(dev), eps.to(dev), rec.to(dev), kl.to(dev)
        klw = torch.tensor([beta], device=dev)
        # lv_svi_step_f32 on the same inputs
        p1, v1 = phi.clone().to(dev), vel.clone().to(dev)
        best, bl, tr = torch.empty(B, 2 * nz, device=dev), torch.full((B,), float("inf"), device=dev), torch.empty(B, device=dev)
        z1, k1 = torch.empty(B, ns, nz, device=dev), torch.empty(B, device=dev)
        lib.lv_svi_step_f32(P(d_rec), P(d_dz), parts, P(d_eps), P(d_kl), P(klw), lr, mom, clip, P(p1), P(v1), P(best), P(bl), P(tr),
                            P(z1), P(k1), B, ns, nz, _s(dev))
        b_phi, p2 = _guarded(phi, dev)
        b_vel, v2 = _guarded(vel, dev)
        b_g, g_rec = _guarded(torch.full((B, 2 * nz), NAN), dev)
        b_l, l_rec = _guarded(torch.full((B, 2 * nz), NAN), dev)
        b_z, z2 = _guarded(torch.full((B, ns, nz), NAN), dev)
        b_k, k2 = _guarded(torch.full((B,), NAN), dev)
        lib.lv_svi_rec_step_f32(P(d_dz), parts, P(d_eps), P(klw), lr, mom, clip, P(p2), P(v2), P(g_rec), P(l_rec), P(z2), P(k2), B, ns,
                                nz, _s(dev))
        for b in (b_phi, b_vel, b_g, b_l, b_z, b_k):
            assert _guards_intact(b)
        for out in (g_rec, l_rec, z2, k2):
            assert not bool(torch.isnan(out).any()), "an output was not fully overwritten"
        assert _same(p2, p1) and _same(v2, v1) and _same(z2, z1) and _same(k2, k1)
        assert _same(l_rec, phi)
        # g_k: the gradient part of test_svi_step_against_float64's count -- parts * ns adds for dz (+ ns multiply-adds with eps), two
        # expf (<= 2 ulp each), 6 multiplies / adds for the KL term -- each within u of the magnitude sum A of the terms it combines
        ops = parts * ns + ns + 2 * 2 + 6
        mu, lv = phi[:, :nz].double(), phi[:, nz:].double()
        sd = (0.5 * lv).exp()
        adz = dzp.double().abs().sum(dim=0).view(B, ns, nz)
        A = torch.cat((adz.sum(dim=1) + beta * mu.abs(), (adz * eps.double().abs()).sum(dim=1) * 0.5 * sd + beta * 0.5 * (lv.exp() + 1.0)),
                      dim=1)
        err = (g_rec.cpu().double() - g64).abs()
        assert bool((err <= ops * U * A).all()), float((err / (ops * U * A)).max())


def test_rec_step_bad_arguments_write_nothing(target):
    lib, dev = target
    raw = lib._raw_lv_svi_rec_step_f32
    B, ns, nz = 3, 2, 4
    t = {k: torch.full(shape, POISON, device=dev) for k, shape in
         dict(dz=(1, B * ns, nz), eps=(B, ns, nz), klw=(1,), phi=(B, 2 * nz), vel=(B, 2 * nz), g=(B, 2 * nz), l=(B, 2 * nz),
              z=(B, ns, nz), kn=(B,)).items()}

    def call(**kw):
        a = dict(dz=P(t["dz"]), parts=1, eps=P(t["eps"]), klw=P(t["klw"]), lr=1.0, mom=0.5, clip=5.0, phi=P(t["phi"]), vel=P(t["vel"]),
                 g=P(t["g"]), l=P(t["l"]), z=P(t["z"]), kn=P(t["kn"]), B=B, ns=ns, nz=nz)
        a.update(kw)
        return raw(a["dz"], a["parts"], a["eps"], a["klw"], a["lr"], a["mom"], a["clip"], a["phi"], a["vel"], a["g"], a["l"], a["z"],
                   a["kn"], a["B"], a["ns"], a["nz"], _s(dev))
    for bad in (dict(dz=None), dict(eps=None), dict(klw=None), dict(phi=None), dict(vel=None), dict(g=None), dict(l=None), dict(z=None),
                dict(kn=None), dict(B=0), dict(ns=0), dict(nz=-1), dict(parts=0), dict(lr=0.0), dict(lr=NAN), dict(clip=-1.0),
                dict(mom=1.0), dict(mom=-0.1)):
        assert call(**bad) < 0, bad
    for k, v in t.items():
        assert bool((v == POISON).all()), k


# ---- 2. the adjoint step and the Hessian-vector assembly ----------------------------------------------------------------------------
def _adjoint_ref(lbar, vbar, g, lam, eps, lr, mom, clip, fd_eps):
    """The definition in float64 on the float32 inputs (fd_eps as the float32 the entry receives)."""
    B, ns, nz = eps.shape
    lbar, vbar, g, lam, eps = (t.double() for t in (lbar, vbar, g, lam, eps))
    fd = float(np.float32(fd_eps))
    vb = vbar - lr * lbar
    r = g.norm(dim=1, keepdim=True)
    s = clip / (r + 1e-6)
    active = s < 1.0
    gb = torch.where(active, s * vb - clip * (g * vb).sum(dim=1, keepdim=True) / (r * (r + 1e-6) ** 2) * g, vb)
    n = float(gb.pow(2).sum().sqrt())
    e = fd * max(1.0, float(lam.abs().max()))
    c = n / (2 * e)
    u = gb / n if n > 0 else torch.zeros_like(gb)
    lp, lm = lam + e * u, lam - e * u
    z = torch.cat([q[:, :nz].unsqueeze(1) + eps * (0.5 * q[:, nz:]).exp().unsqueeze(1) for q in (lp, lm)], dim=1)
    seeds = torch.cat((torch.full((B, ns), c / ns), torch.full((B, ns), -c / ns)), dim=1).double().reshape(-1)
    return dict(vb=vb, gb=gb, active=active.view(-1), s=s, r=r, vbar=mom * vb, n=n, e=e, c=c, u=u, z=z, seeds=seeds)


def _adjoint_call(lib, dev, lbar, vbar, g, lam, eps, lr, mom, clip, fd_eps):
    B, ns, nz = eps.shape
    b_v, d_v = _guarded(vbar, dev)
    b_u, d_u = _guarded(torch.full((B, 2 * nz), NAN), dev)
    b_s, d_s = _guarded(torch.full((3,), NAN), dev)
    b_z, d_z = _guarded(torch.full((B, 2 * ns, nz), NAN), dev)
    b_sd, d_sd = _guarded(torch.full((B * 2 * ns,), NAN), dev)
    ins = [t.to(dev) for t in (lbar, g, lam, eps)]
    lib.lv_savae_adjoint_f32(P(ins[0]), P(d_v), P(ins[1]), P(ins[2]), P(ins[3]), lr, mom, clip, fd_eps, P(d_u), P(d_s), P(d_z), P(d_sd),
                             B, ns, nz, _s(dev))
    for b in (b_v, b_u, b_s, b_z, b_sd):
        assert _guards_intact(b)
    for out in (d_v, d_u, d_s, d_z, d_sd):
        assert not bool(torch.isnan(out).any()), "an output was not fully overwritten"
    return d_v.cpu(), d_u.cpu(), d_s.cpu(), d_z.cpu(), d_sd.cpu()


@pytest.mark.parametrize("B,ns,nz", SHAPES)
def test_adjoint_against_float64(target, B, ns, nz):
    """Counted operations, each within u of the magnitude sum of the terms it combines (first order; the counts are rounded up):
      vb:   2 (multiply, subtract) on |vbar| + lr |lbar| =: Avb
      r:    nr = 2 * 2 ceil(nz / 64) + 6 + 1 (squares and adds per lane, butterfly, sqrt), relative (a sum of squares)
      dot:  nd = 2 * 2 ceil(nz / 64) + 6 on D = sum_i |g_i| Avb_i, plus the 2 of vb
      s:    nr + 2;   back = clip * dot / (r * (r + 1e-6)^2): 3 (nr + 1) + 5 relative, plus dot's
      gb (clip active):   |s vb| (nr + 2 + 2 + 2) + clip D |g_j| / (r (r + 1e-6)^2) (nd + 2 + 3 nr + 8 + 2)   -> ops_gb = 4 nr + nd + 20
      gb (clip inactive): vb's 2
      vbar' = m * vb: 3.   n: |n - n64| <= |e_gb|_2 + 2 u n (the squares are summed in double).   e: 2 relative.   c: n's + 2.
      u = gb / n: e_gb / n + |u| (e_n / n + 1).
      z+-: arg = lv +- e u_lv: error e_a = e e_u + 3 u (|lv| + e |u|); sigma = expf(arg / 2): relative e_a / 2 + 3 u;
           mp = mu +- e u_mu: e e_u + 3 u (|mu| + e |u|); z = mp + eps * sigma: 2 more on |mp| + |eps| sigma.
      seeds: c's + 1."""
    lib, dev = target
    lr, mom, clip, fd_eps = 0.8, 0.5, 5.0, 1e-2
    nr = 4 * math.ceil(nz / 64) + 7
    nd = 4 * math.ceil(nz / 64) + 6
    ops_gb = 4 * nr + nd + 20
    for case in range(2):
        gen = torch.Generator().manual_seed(3000 * B + 100 * ns + nz + case)
        lbar = torch.randn(B, 2 * nz, generator=gen)
        vbar = torch.randn(B, 2 * nz, generator=gen) * 0.5
        g = torch.randn(B, 2 * nz, generator=gen) * _clip_rows(B, case).view(B, 1) / math.sqrt(2 * nz) * 3
        lam = torch.randn(B, 2 * nz, generator=gen) * (0.5 + case)
        eps = torch.randn(B, ns, nz, generator=gen)
        ref = _adjoint_ref(lbar, vbar, g, lam, eps, lr, mom, clip, fd_eps)
        if B > 1:
            assert bool(ref["active"].any()) and bool((~ref["active"]).any()), "both clip branches in one batch"
        v, u, scal, z, seeds = _adjoint_call(lib, dev, lbar, vbar, g, lam, eps, lr, mom, clip, fd_eps)
        Avb = vbar.double().abs() + lr * lbar.double().abs()
        D = (g.double().abs() * Avb).sum(dim=1, keepdim=True)
        r, s = ref["r"], ref["s"]
        e_gb = torch.where(ref["active"].view(B, 1), ops_gb * U * (s * Avb + clip * D * g.double().abs() / (r * (r + 1e-6) ** 2)), 2 * U * Avb)
        assert bool(((v.double() - ref["vbar"]).abs() <= 3 * U * mom * Avb).all())
        n, e, c = ref["n"], ref["e"], ref["c"]
        e_n = float(e_gb.norm()) + 2 * U * n
        assert abs(float(scal[0]) - n) <= e_n, (float(scal[0]), n, e_n)
        assert abs(float(scal[1]) - e) <= 2 * U * e
        e_c = c * (e_n / n + 4 * U)
        assert abs(float(scal[2]) - c) <= e_c
        e_u = e_gb / n + ref["u"].abs() * (e_n / n + U)
        assert bool(((u.double() - ref["u"]).abs() <= e_u).all()), float(((u.double() - ref["u"]).abs() / e_u).max())
        lam64, u64 = lam.double(), ref["u"]
        mu, lv, um, ul = lam64[:, :nz], lam64[:, nz:], u64[:, :nz], u64[:, nz:]
        e_m = e * e_u[:, :nz] + 3 * U * (mu.abs() + e * um.abs())
        e_a = e * e_u[:, nz:] + 3 * U * (lv.abs() + e * ul.abs())
        for sign, half in ((1.0, z[:, :ns]), (-1.0, z[:, ns:])):
            sd = (0.5 * (lv + sign * e * ul)).exp().unsqueeze(1)
            mp = (mu + sign * e * um).unsqueeze(1)
            want = mp + eps.double() * sd
            bound = e_m.unsqueeze(1) + eps.double().abs() * sd * (0.5 * e_a.unsqueeze(1) + 3 * U) + 2 * U * (mp.abs() + eps.double().abs() * sd)
            err = (half.double() - want).abs()
            assert bool((err <= bound).all()), float((err / bound).max())
        assert bool(((seeds.double() - ref["seeds"]).abs() <= e_c / ns + U * c / ns).all())
        assert bool((seeds.view(B, 2 * ns)[:, :ns] > 0).all()) and bool((seeds.view(B, 2 * ns)[:, ns:] < 0).all())


@pytest.mark.parametrize("B,ns,nz", [(5, 3, 4), (33, 1, 33)])
def test_adjoint_zero_direction(target, B, ns, nz):
    """lbar = vbar = 0: n = 0, so u = 0, c = 0, every seed 0 and both halves of z_pm are the samples at lambda itself."""
    lib, dev = target
    gen = torch.Generator().manual_seed(B + nz)
    g = torch.randn(B, 2 * nz, generator=gen) * _clip_rows(B, 0).view(B, 1)
    lam = torch.randn(B, 2 * nz, generator=gen)
    eps = torch.randn(B, ns, nz, generator=gen)
    zero = torch.zeros(B, 2 * nz)
    v, u, scal, z, seeds = _adjoint_call(lib, dev, zero, zero, g, lam, eps, 1.0, 0.5, 5.0, 1e-2)
    assert float(scal[0]) == 0.0 and float(scal[2]) == 0.0 and float(scal[1]) > 0.0
    assert bool((u == 0).all()) and bool((seeds == 0).all()) and bool((v == 0).all())
    z0 = torch.empty(B, ns, nz, device=dev)
    kl0 = torch.empty(B, device=dev)
    d_lam, d_eps = lam.to(dev), eps.to(dev)
    lib.lv_reparam_kl_fwd_f32(P(d_lam), P(d_eps), P(z0), P(kl0), B, ns, nz, _s(dev))
    assert _same(z[:, :ns], z0) and _same(z[:, ns:], z0)
    # ... and lv_savae_hvp_f32 leaves lbar alone, bit for bit
    lbar = torch.randn(B, 2 * nz, generator=gen)
    b_l, d_l = _guarded(lbar, dev)
    dz = torch.randn(2, B * 2 * ns, nz, generator=gen).to(dev)
    klw = torch.tensor([0.7], device=dev)
    d_u, d_scal = u.to(dev), scal.to(dev)
    lib.lv_savae_hvp_f32(P(dz), 2, P(d_eps), P(d_lam), P(d_u), P(d_scal), P(klw), P(d_l), B, ns, nz, _s(dev))
    assert _guards_intact(b_l) and _same(d_l, lbar)


@pytest.mark.parametrize("B,ns,nz", SHAPES)
def test_hvp_against_float64(target, B, ns, nz):
    """Counted operations per coordinate, each within u of the magnitude sum of the terms it combines (scal, u, lam are inputs):
      mu half:  (parts + 1) ns adds for each of the two dz sums, their sum (1), mp and mm (2 each), their difference (1), c * beta and
                the product (2), two adds (2): ops = 2 (parts + 1) ns + 10 on |lbar| + sum |dz| + c beta (|mp| + |mm|)
      lv half:  (parts + 2) ns per sum, the arguments lp, lm (2 each, error 3 u (|lv| + e |u|) =: e_a), sigma = expf(arg / 2):
                relative e_a / 2 + 3 u, expf(arg): relative e_a + 2 u; 0.5 * sigma, the products, three adds, c beta / 2 (...): 12 more:
                ops = 2 (parts + 2) ns + 12 on |lbar| + sum |dz eps| sigma / 2 + c beta (e^lp + e^lm) / 2, plus the expf-argument terms."""
    lib, dev = target
    beta = 0.7
    for case, parts in enumerate((1, 3)):
        gen = torch.Generator().manual_seed(4000 * B + 100 * ns + nz + case)
        lam = torch.randn(B, 2 * nz, generator=gen) * 0.7
        u = torch.randn(B, 2 * nz, generator=gen)
        u = u / u.norm()
        eps = torch.randn(B, ns, nz, generator=gen)
        lbar = torch.randn(B, 2 * nz, generator=gen)
        n = 3.7
        e = float(np.float32(1e-2 * max(1.0, float(lam.abs().max()))))
        scal = torch.tensor([n, e, n / (2 * e)])
        c = float(scal[2])
        dz = torch.randn(parts, B * 2 * ns, nz, generator=gen) * c / ns
        b_l, d_l = _guarded(lbar, dev)
        ins = [t.to(dev) for t in (dz, eps, lam, u, scal)]
        klw = torch.tensor([beta], device=dev)
        lib.lv_savae_hvp_f32(P(ins[0]), parts, P(ins[1]), P(ins[2]), P(ins[3]), P(ins[4]), P(klw), P(d_l), B, ns, nz, _s(dev))
        assert _guards_intact(b_l)
        kw = float(klw.cpu()[0])
        l64, u64, e64 = lam.double(), u.double(), eps.double()
        mu, lv, um, ul = l64[:, :nz], l64[:, nz:], u64[:, :nz], u64[:, nz:]
        mp, mm, lp, lm = mu + e * um, mu - e * um, lv + e * ul, lv - e * ul
        d = dz.double().sum(dim=0).view(B, 2 * ns, nz)
        ad = dz.double().abs().sum(dim=0).view(B, 2 * ns, nz)
        dp, dm, adp, adm = d[:, :ns], d[:, ns:], ad[:, :ns], ad[:, ns:]
        sp, sm = (0.5 * lp).exp(), (0.5 * lm).exp()
        want_mu = lbar.double()[:, :nz] + dp.sum(dim=1) + dm.sum(dim=1) + c * kw * (mp - mm)
        want_lv = lbar.double()[:, nz:] + (dp * e64).sum(dim=1) * 0.5 * sp + (dm * e64).sum(dim=1) * 0.5 * sm \
            + c * kw * 0.5 * (lp.exp() - lm.exp())
        A_mu = lbar.double()[:, :nz].abs() + adp.sum(dim=1) + adm.sum(dim=1) + c * kw * (mp.abs() + mm.abs())
        tp, tm = (adp * e64.abs()).sum(dim=1) * 0.5 * sp, (adm * e64.abs()).sum(dim=1) * 0.5 * sm
        kp = c * kw * 0.5 * (lp.exp() + lm.exp())
        A_lv = lbar.double()[:, nz:].abs() + tp + tm + kp
        e_a = 3 * U * (lv.abs() + e * ul.abs())
        b_mu = (2 * (parts + 1) * ns + 10) * U * A_mu
        b_lv = (2 * (parts + 2) * ns + 12) * U * A_lv + (tp + tm) * (0.5 * e_a + 3 * U) + kp * (e_a + 2 * U)
        got = d_l.cpu().double()
        err_mu, err_lv = (got[:, :nz] - want_mu).abs(), (got[:, nz:] - want_lv).abs()
        assert bool((err_mu <= b_mu).all()), float((err_mu / b_mu).max())
        assert bool((err_lv <= b_lv).all()), float((err_lv / b_lv).max())


def test_adjoint_and_hvp_bad_arguments_write_nothing(target):
    lib, dev = target
    B, ns, nz = 3, 2, 4
    t = {k: torch.full(shape, POISON, device=dev) for k, shape in
         dict(lbar=(B, 2 * nz), vbar=(B, 2 * nz), g=(B, 2 * nz), lam=(B, 2 * nz), eps=(B, ns, nz), u=(B, 2 * nz), scal=(3,),
              z=(B, 2 * ns, nz), seeds=(B * 2 * ns,), dz=(1, B * 2 * ns, nz), klw=(1,)).items()}

    def adjoint(**kw):
        a = dict(lbar=P(t["lbar"]), vbar=P(t["vbar"]), g=P(t["g"]), lam=P(t["lam"]), eps=P(t["eps"]), lr=1.0, mom=0.5, clip=5.0, fd=1e-2,
                 u=P(t["u"]), scal=P(t["scal"]), z=P(t["z"]), seeds=P(t["seeds"]), B=B, ns=ns, nz=nz)
        a.update(kw)
        return lib._raw_lv_savae_adjoint_f32(a["lbar"], a["vbar"], a["g"], a["lam"], a["eps"], a["lr"], a["mom"], a["clip"], a["fd"],
                                             a["u"], a["scal"], a["z"], a["seeds"], a["B"], a["ns"], a["nz"], _s(dev))

    def hvp(**kw):
        a = dict(dz=P(t["dz"]), parts=1, eps=P(t["eps"]), lam=P(t["lam"]), u=P(t["u"]), scal=P(t["scal"]), klw=P(t["klw"]),
                 lbar=P(t["lbar"]), B=B, ns=ns, nz=nz)
        a.update(kw)
        return lib._raw_lv_savae_hvp_f32(a["dz"], a["parts"], a["eps"], a["lam"], a["u"], a["scal"], a["klw"], a["lbar"], a["B"],
                                         a["ns"], a["nz"], _s(dev))
    for bad in [dict([(k, None)]) for k in ("lbar", "vbar", "g", "lam", "eps", "u", "scal", "z", "seeds")] + [
            dict(B=0), dict(ns=0), dict(nz=-1), dict(lr=0.0), dict(lr=NAN), dict(clip=0.0), dict(mom=1.0), dict(mom=-0.1), dict(fd=0.0),
            dict(fd=NAN)]:
        assert adjoint(**bad) < 0, bad
    for bad in [dict([(k, None)]) for k in ("dz", "eps", "lam", "u", "scal", "klw", "lbar")] + [dict(B=0), dict(ns=-1), dict(nz=0),
                                                                                                dict(parts=0)]:
        assert hvp(**bad) < 0, bad
    for k, v in t.items():
        assert bool((v == POISON).all()), k


# ---- 3..6. the reference fixture -----------------------------------------------------------------------------------------------------
def _fixture_case(fx, name, dev):
    V, ni, H, nz, ns, K = (int(v) for v in fx[name + "/dims"])
    lr, mom, clip, beta, fd_eps = (float(v) for v in fx[name + "/hyper"])
    params = {k: torch.from_numpy(fx[name + "/param/" + k]) for k in ALL_KEYS}
    vae = build_vae(V, ni, H, nz, dev, params=params)
    x = torch.from_numpy(fx[name + "/x"]).to(dev)
    eps = torch.from_numpy(fx[name + "/eps"]).to(dev)
    masks = bool(int(fx[name + "/masks"][0]))
    m_in = torch.from_numpy(fx[name + "/mask_in"]).to(dev) if masks else None
    m_out = torch.from_numpy(fx[name + "/mask_out"]).to(dev) if masks else None
    vae.train(masks)
    kw = dict(kl_weight=beta, svi_steps=K, svi_lr=lr, svi_momentum=mom, svi_clip=clip, fd_eps=fd_eps, nsamples=ns)
    return vae, x, (eps, m_in, m_out), kw


def _grads(vae):
    return {k: p.grad.detach().clone() for k, p in vae.named_parameters()}


def _check_fixture_gradients(fx, name, got):
    worst = 0.0
    for k in ALL_KEYS:
        fd64, fd32, exact = (fx["%s/grad_%s/%s" % (name, kind, k)].astype(np.float64) for kind in ("fd64", "fd32", "exact"))
        g = got[k].detach().cpu().double().numpy()
        bound = max(GRAD_RTOL * float(np.abs(fd64).max()), 4.0 * float(np.abs(fd32 - fd64).max()))
        err = float(np.abs(g - fd64).max())
        to_exact = float(np.abs(g - exact).max() / np.abs(exact).max())
        worst = max(worst, to_exact)
        print("%s %-28s |got - scheme64| %.3e (bound %.3e)   to the exact gradient %.3e of max|tensor|" % (name, k, err, bound, to_exact))
        assert err <= bound, (name, k, err, bound)
    return worst


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_loss_savae_against_reference_fixture(target, name):
    _, dev = target
    fx = load("savae_small")
    vae, x, noise, kw = _fixture_case(fx, name, dev)
    loss, rec, kl = vae.loss_savae(x, noise=noise, **kw)
    assert not rec.requires_grad and not kl.requires_grad and loss.requires_grad
    assert rel_err(loss, fx[name + "/loss32"]) < RTOL and rel_err(rec, fx[name + "/rec32"]) < RTOL and rel_err(kl, fx[name + "/kl32"]) < RTOL
    loss.mean().backward()
    _check_fixture_gradients(fx, name, _grads(vae))
    # and the step is not the ordinary ELBO step: far from the K = 0 gradient the fixture records
    got = _grads(vae)
    num = sum(float((got[k].cpu().double() - torch.from_numpy(fx["%s/grad_k0/%s" % (name, k)])).pow(2).sum()) for k in ALL_KEYS) ** 0.5
    den = sum(float(got[k].double().pow(2).sum()) for k in ALL_KEYS) ** 0.5
    assert num / den >= 100 * GRAD_RTOL


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_trajectory_against_reference_fixture(target, name):
    _, dev = target
    fx = load("savae_small")
    vae, x, (eps, m_in, m_out), kw = _fixture_case(fx, name, dev)
    lam32, lam64 = fx[name + "/lam32"], fx[name + "/lam64"]
    K = lam32.shape[0] - 1
    dev_k = np.abs(lam32.astype(np.float64) - lam64).max(axis=(1, 2))
    eng = vae.decoder._hip
    dec = vae.decoder
    with torch.no_grad():
        mulv = vae.encoder._forward_mulv(x)
        st = eng.savae_forward(x, mulv, eps, m_in, m_out, dec.dropout_in.p, dec.dropout_out.p, K, kw["svi_lr"], kw["svi_momentum"],
                               kw["svi_clip"], kw["kl_weight"])
    got = torch.cat((st.lam_rec, st.lam.unsqueeze(0)), dim=0).cpu().numpy().astype(np.float64)
    for k in range(K + 1):
        bound = max(RTOL * float(np.abs(lam32[k]).max()), 4.0 * float(dev_k[k]))
        err = float(np.abs(got[k] - lam32[k]).max())
        assert err <= bound, (k, err, bound)
    g32, g64 = fx[name + "/g32"], fx[name + "/g64"]
    for k in range(K):
        bound = max(GRAD_RTOL * float(np.abs(g64[k]).max()), 4.0 * float(np.abs(g32[k].astype(np.float64) - g64[k]).max()))
        assert float(np.abs(st.g_rec[k].cpu().numpy().astype(np.float64) - g64[k]).max()) <= bound, k
    if name == "b":                                     # both clip states at k = 0, as the fixture guarantees
        norms = st.g_rec[0].norm(dim=1)
        assert bool((norms > kw["svi_clip"]).any()) and bool((norms < kw["svi_clip"]).any())


# ---- 7. routes ------------------------------------------------------------------------------------------------------------------------
def _both_routes(vae, x, noise, **kw):
    out = {}
    for fused in (True, False):
        vae.fused_savae = fused
        try:
            vae.zero_grad()
            with spying() as calls:
                loss, rec, kl = vae.loss_savae(x, noise=noise, **kw)
                loss.mean().backward()
        finally:
            del vae.fused_savae
        names = {n for n, _ in calls}
        assert {"lv_svi_rec_step_f32", "lv_savae_adjoint_f32", "lv_savae_hvp_f32"} <= names
        assert ("lv_dec_tail_dz_f32" in names) == fused, "route"
        out[fused] = (loss.detach().clone(), rec.clone(), kl.clone(), _grads(vae))
    f, g = out[True], out[False]
    for i in range(3):
        assert rel_err(f[i], g[i]) < RTOL
    for k in f[3]:
        err, scale = float((f[3][k] - g[3][k]).abs().max()), float(g[3][k].abs().max())
        assert err <= GRAD_RTOL * scale, (k, err, scale)
    return out


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_fused_route_equals_generic_route(target, name):
    _, dev = target
    vae, x, noise, kw = _fixture_case(load("savae_small"), name, dev)
    _both_routes(vae, x, noise, **kw)


def test_fused_route_equals_generic_route_mid(target):
    """H 64, nz 32, B 8, T 12, K 2 with masks: full-width lanes and more than 16 decoder rows in the perturbed pair."""
    _, dev = target
    V, ni, H, nz, B, T = 97, 16, 64, 32, 8, 12
    vae = _small_vae(dev, V, ni, H, nz, seed=75, scale=0.2)
    vae.train()
    x = _batch(B, T, V, 76, dev)
    g = torch.Generator().manual_seed(9)
    noise = (torch.randn(B, 1, nz, generator=g).to(dev), (torch.rand(B, T - 1, ni, generator=g) < 0.5).to(torch.uint8).to(dev),
             (torch.rand(B, T - 1, H, generator=g) < 0.5).to(torch.uint8).to(dev))
    _both_routes(vae, x, noise, kl_weight=0.8, svi_steps=2, svi_clip=0.5)


# ---- 8..12. invariants ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 3])
def test_forward_trajectory_equals_refine_posterior(target, ns):
    _, dev = target
    vae = _small_vae(dev)
    vae.eval()
    B, T, K = 5, 7, 3
    x = _batch(B, T, 53, 77, dev)
    eps = torch.randn(B, ns, 4, generator=torch.Generator().manual_seed(2)).to(dev)
    eng = vae.decoder._hip
    with torch.no_grad():
        mulv = vae.encoder._forward_mulv(x)
        st = eng.savae_forward(x, mulv, eps, None, None, 0.5, 0.5, K, 1.0, 0.5, 5.0, 0.8)
    traj = torch.cat((st.lam_rec, st.lam.unsqueeze(0)), dim=0)
    for k in range(K + 1):
        mu, logvar = vae.refine_posterior(x, steps=k, nsamples=ns, noise=eps, keep="last", kl_weight=0.8)
        assert _same(traj[k], torch.cat((mu, logvar), dim=1)), k


def test_two_backward_calls_accumulate(target):
    _, dev = target
    vae, x, noise, kw = _fixture_case(load("savae_small"), "a", dev)
    vae.loss_savae(x, noise=noise, **kw)[0].mean().backward()
    once = _grads(vae)
    vae.loss_savae(x, noise=noise, **kw)[0].mean().backward()
    for k, g in _grads(vae).items():
        assert float((g - 2 * once[k]).abs().max()) <= 8 * U * float(once[k].abs().max()), k
    # seeds other than the mean's: the gradient is linear in them (the differences' rounding is not: the bound between two routes)
    vae.zero_grad()
    (3.0 * vae.loss_savae(x, noise=noise, **kw)[0].mean()).backward()
    for k, g in _grads(vae).items():
        assert float((g - 3 * once[k]).abs().max()) <= GRAD_RTOL * 3 * float(once[k].abs().max()), k


@pytest.mark.parametrize("fused", [True, False])
def test_loss_savae_leaves_the_rest_alone(target, fused):
    _, dev = target
    vae, x, noise, kw = _fixture_case(load("savae_small"), "b", dev)
    for e in (vae.encoder._hip, vae.decoder._hip):
        e.ensure(dev)
    before = _state(vae)
    vae.fused_savae = fused
    try:
        loss = vae.loss_savae(x, noise=noise, **kw)[0]
        loss.mean().backward()
    finally:
        del vae.fused_savae
    after = _state(vae)
    for k in before:
        if k.startswith(("param/", "buf/", "train/", "rng/")):
            if torch.is_tensor(before[k]):
                assert _same(before[k], after[k]), k
            else:
                assert before[k] == after[k], k


def test_refusals_come_before_any_launch(target):
    _, dev = target
    vae = _small_vae(dev)
    B, T, nz = 4, 6, 4
    x = _batch(B, T, 53, 90, dev)
    for eng in (vae.encoder._hip, vae.decoder._hip):
        eng.ensure(dev)
    ok = (torch.zeros(B, 1, nz, device=dev), None, None)
    from vae_lagging_encoder_amd.trainer import SemiAmortizedTextTrainer
    from vae_lagging_encoder_amd.training import TextTrainingLoop
    with spying() as calls:
        for kw in (dict(svi_steps=-1), dict(svi_lr=0.0), dict(svi_lr=-1.0), dict(svi_clip=0.0), dict(fd_eps=0.0), dict(fd_eps=-1e-2),
                   dict(svi_momentum=1.0), dict(svi_momentum=-0.1), dict(nsamples=0),
                   dict(noise=(torch.zeros(B, 2, nz, device=dev), None, None)), dict(noise=(torch.zeros(B + 1, 1, nz, device=dev), None, None)),
                   dict(noise=(ok[0].double(), None, None)), dict(noise=(ok[0].to("meta"), None, None)), dict(noise=ok[0]),
                   dict(noise=(ok[0], torch.ones(B, T, 8, dtype=torch.uint8, device=dev), None)),
                   dict(noise=(ok[0], None, torch.ones(B, T - 1, 8, dtype=torch.uint8, device=dev)))):
            with pytest.raises(ValueError):
                vae.loss_savae(x, **kw)
        with pytest.raises(ValueError, match="variable-length"):
            vae.loss_savae((x, [6, 5, 4, 3]))
        vae.set_precision("bf16")
        try:
            with pytest.raises(ValueError, match="bf16"):
                vae.loss_savae(x, noise=ok)
        finally:
            vae.set_precision("f32")
        for kw in (dict(precision="bf16"), dict(use_graph=True), dict(micro_batches=2), dict(decoder_grads="norm"), dict(fold_norm=True),
                   dict(svi_steps=-1), dict(fd_eps=0.0), dict(svi_momentum=1.0), dict(objective="iw")):
            with pytest.raises(ValueError):
                SemiAmortizedTextTrainer(vae, **kw)
        for extra in (dict(aggressive=1), dict(objective="iw")):
            a = dict(kl_start=0.1, warm_up=1, batch_size=B, epochs=1, aggressive=0, nsamples=1, test_nepoch=5, iw_nsamples=20, momentum=0,
                     svi_steps=2)
            a.update(extra)
            with pytest.raises(ValueError, match="svi_steps"):
                TextTrainingLoop(vae, [x], [x], [x], argparse.Namespace(**a), log=lambda *_: None)
    assert [n for n, _ in calls] == [], calls
    # a decoder that is not the LSTM decoder
    from parity_common import build_image_vae
    img = build_image_vae(dev, 31)
    with pytest.raises(ValueError, match="LSTMDecoder"):
        img.loss_savae(torch.zeros(2, 5, dtype=torch.int64, device=dev))
    assert tuple(vae.loss_savae(x, svi_steps=1, noise=ok)[0].shape) == (B,)       # and the same objects still work


# ---- 9, 13, 14. the fused trainer -----------------------------------------------------------------------------------------------------
def _weights(vae):
    return {k: v.detach().cpu().clone() for k, v in vae.state_dict().items() if k in ALL_KEYS}


def test_trainer_zero_steps_equals_ordinary_step(target):
    from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer, SemiAmortizedTextTrainer
    _, dev = target
    fx = load("savae_small")
    out = []
    for cls, extra in ((SemiAmortizedTextTrainer, dict(svi_steps=0)), (AggressiveTextTrainer, dict())):
        vae, x, noise, kw = _fixture_case(fx, "b", dev)
        tr = cls(vae, lr=0.5, clip=5.0, nsamples=kw["nsamples"], **extra)
        tr.step(x, kw["kl_weight"], noise=noise, update="both")
        out.append((tr.read_stats(), _weights(vae)))
    for key in ("loss_sum", "rec_sum", "kl_sum"):
        assert abs(out[0][0][key] - out[1][0][key]) <= RTOL * abs(out[1][0][key])
    assert abs(out[0][0]["loss0_sum"] - out[0][0]["loss_sum"]) <= 1e-6 * abs(out[0][0]["loss_sum"])
    for k in ALL_KEYS:
        assert rel_err(out[0][1][k], out[1][1][k]) < RTOL, k


@pytest.mark.parametrize("name", ["a", "b"])
def test_trainer_against_generic_route_with_torch_sgd(target, name):
    """Three consecutive steps: the fused trainer against VAE.loss_savae on the generic route with torch's clip_grad_norm_ and SGD."""
    from vae_lagging_encoder_amd.trainer import SemiAmortizedTextTrainer
    _, dev = target
    fx = load("savae_small")
    lr, clip = 0.5, 1.0
    vae, x, noise, kw = _fixture_case(fx, name, dev)
    tr = SemiAmortizedTextTrainer(vae, svi_steps=kw["svi_steps"], svi_lr=kw["svi_lr"], svi_momentum=kw["svi_momentum"],
                                  svi_clip=kw["svi_clip"], fd_eps=kw["fd_eps"], lr=lr, clip=clip, nsamples=kw["nsamples"])
    ref, _, _, _ = _fixture_case(fx, name, dev)
    ref.fused_savae = False
    opt = torch.optim.SGD(ref.parameters(), lr=lr)
    want_loss = 0.0
    for step in range(3):
        tr.step(x, kw["kl_weight"], noise=noise)
        if step == 0:
            # the first step's gradient is coef * the fixture's (clip_grad_norm_ scales every gradient in place)
            coef = tr.read_stats()["coef"]
            got = {"encoder." + n: g for n, g in tr.enc.flat.gviews.items()}
            got.update({"decoder." + n: g for n, g in tr.dec.flat.gviews.items()})
            _check_fixture_gradients(fx, name, {k: got[k] / coef for k in ALL_KEYS})
        opt.zero_grad()
        loss = ref.loss_savae(x, noise=noise, **kw)[0]
        loss.mean().backward()
        torch.nn.utils.clip_grad_norm_(ref.parameters(), clip)
        opt.step()
        want_loss += float(loss.detach().sum())
    st = tr.read_stats()
    assert abs(st["loss_sum"] - want_loss) <= RTOL * abs(want_loss)
    assert st["loss0_sum"] > st["loss_sum"], "the refinement closed no gap"
    a, b = _weights(vae), _weights(ref)
    for k in ALL_KEYS:
        assert rel_err(a[k], b[k]) < RTOL, k


def test_voided_step_leaves_the_weights_untouched(target):
    from vae_lagging_encoder_amd.trainer import SemiAmortizedTextTrainer
    _, dev = target
    vae, x, noise, kw = _fixture_case(load("savae_small"), "a", dev)
    tr = SemiAmortizedTextTrainer(vae, svi_steps=2, lr=0.5, clip=5.0)
    before = _weights(vae)
    tr.dec.status.fill_(101)            # what a timed-out recurrence leaves behind -- set by hand, nothing is provoked
    tr.step(x, 1.0, noise=noise)
    assert float(tr.scal[8]) == 1.0 and float(tr.scal0[0]) == 0.0 and float(tr.scal[5]) == 0.0
    after = _weights(vae)
    for k in ALL_KEYS:
        assert torch.equal(before[k], after[k]), k
    tr.dec.status.zero_()
    tr.scal[8:13] = 0
    tr._journal = []
    tr.step(x, 1.0, noise=noise)
    st = tr.read_stats()
    assert st["loss_sum"] > 0 and st["loss0_sum"] >= st["loss_sum"]
    assert any(not torch.equal(before[k], v) for k, v in _weights(vae).items())


# ---- 15. the training loop ------------------------------------------------------------------------------------------------------------
def test_training_loop_with_and_without_svi_steps(target):
    from vae_lagging_encoder_amd.factory import build_text_vae, synthetic_batch
    from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer, SemiAmortizedTextTrainer
    from vae_lagging_encoder_amd.training import TextTrainingLoop
    _, dev = target
    train = [synthetic_batch(4, T, 53, seed=10 + i).to(dev) for i, T in enumerate((5, 6))]

    def run(**extra):
        vae = build_text_vae(53, 8, 16, 4, dev, seed=2, model_scale=0.1)
        a = dict(kl_start=0.1, warm_up=1, batch_size=4, epochs=1, aggressive=0, nsamples=1, test_nepoch=5, iw_nsamples=20, momentum=0)
        a.update(extra)
        loop = TextTrainingLoop(vae, train, train[:1], train[:1], argparse.Namespace(**a), log=lambda *_: None,
                                np_rng=np.random.RandomState(3), seed=11)
        loop.run()
        return loop, _weights(vae)
    loop, _ = run(svi_steps=2, svi_clip=1.0)
    assert type(loop.trainer) is SemiAmortizedTextTrainer and loop.trainer.svi == (2, 1.0, 0.5, 1.0, 1e-2)
    assert len(loop.iterations) == 2 and all(np.isfinite(r["rec_sum"]) and np.isfinite(r["kl_sum"]) for r in loop.iterations)
    assert all(np.isfinite(h["loss"]) for h in loop.history)
    plain, w_plain = run()
    zero, w_zero = run(svi_steps=0)
    assert type(plain.trainer) is AggressiveTextTrainer and type(zero.trainer) is AggressiveTextTrainer
    assert [r["rec_sum"] for r in plain.iterations] == [r["rec_sum"] for r in zero.iterations]
    for k in ALL_KEYS:
        assert torch.equal(w_plain[k], w_zero[k]), k

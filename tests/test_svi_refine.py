"""Posterior refinement by SVI on the encoder's output: lv_svi_step_f32 (csrc/lv_svi.hip), lv_dec_tail_dz_f32
(csrc/lv_head.hip), engine.LSTMDecoderEngine.backward_dz / svi_refine, VAE.refine_posterior and
evaluation.calc_amortization_gap / image_calc_amortization_gap; lv_bn_eval_bwd_f32 (csrc/lv_conv.hip), the eval-mode BatchNorm
backward the image decoder's route needs.

Kernel and engine tests run on the emulator build and on the MI355X through one fixture.  References: a float64 statement of
the definition written here (kernel level); tests/golden/svi_small.npz (make_golden_svi.py: the reference's unmodified
classes under torch autograd, float32 and float64); the generic route (fused_svi = False) as the second oracle.

Bounds.  trace: parity_common.RTOL, max-norm relative (the bound on rec / loss everywhere else).  Iterates phi_k against the
fixture: the larger of RTOL * max|phi_k| (the bound parity_common holds an updated encoder weight to) and 4 x the recorded
float32-vs-float64 deviation of the reference's own trajectory at step k; against the second oracle (no recorded deviation) the
first term alone.
"""
import math

import numpy as np
import pytest
import torch

from helpers import ALL_KEYS, build_vae, load, rel_err
from parity_common import RTOL
from vae_lagging_encoder_amd import engine as E
from vae_lagging_encoder_amd import evaluation as EV
from vae_lagging_encoder_amd.engine import P

POISON = 7777.0
GUARD = 16
U = 2.0 ** -24          # unit roundoff of f32


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


def _s(dev):
    return E.stream_ptr(dev)


def _guarded(values, dev):
    """values inside a buffer with GUARD poisoned floats on either side -> (whole buffer, the view the kernel is given)."""
    flat = values.reshape(-1).float()
    buf = torch.full((flat.numel() + 2 * GUARD,), POISON)
    buf[GUARD:GUARD + flat.numel()] = flat
    buf = buf.to(dev)
    return buf, buf[GUARD:GUARD + flat.numel()].view(values.shape)


def _guards_intact(buf):
    b = buf.cpu()
    return bool((b[:GUARD] == POISON).all() and (b[-GUARD:] == POISON).all())


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


def _small_vae(dev, V=53, ni=8, H=16, nz=4, seed=71, scale=0.3):
    from oracle import text_vae_oracle as O
    params = O.random_params(V, ni, H, nz, seed=seed, scale=scale, emb_scale=0.5, head_scale=0.5)
    return build_vae(V, ni, H, nz, dev, params=params)


def _batch(B, T, V, seed, dev):
    from oracle import text_vae_oracle as O
    return O.synthetic_batch(B, T, V, seed=seed).to(dev)


# ---- 1. lv_svi_step_f32 against the float64 statement -----------------------------------------------------------------------------
def _svi_ref(rec, dzp, eps, kl, beta, lr, mom, clip, phi, vel):
    """The definition in float64.  -> L [B], g (unclipped) [B][2nz], clip active [B], new vel, new phi."""
    B, ns, nz = eps.shape
    rec, dz, eps, kl, phi, vel = (t.double() for t in (rec, dzp.sum(dim=0), eps, kl, phi, vel))
    L = rec.view(B, ns).sum(dim=1) / ns + beta * kl
    mu, lv = phi[:, :nz], phi[:, nz:]
    sd = (0.5 * lv).exp()
    dz = dz.view(B, ns, nz)
    g = torch.cat((dz.sum(dim=1) + beta * mu, (dz * eps).sum(dim=1) * 0.5 * sd + beta * 0.5 * (lv.exp() - 1.0)), dim=1)
    norm = g.norm(dim=1, keepdim=True)
    coef = torch.clamp(clip / (norm + 1e-6), max=1.0)
    v = mom * vel + g * coef
    return L, g, (coef < 1.0).view(-1), v, phi - lr * v


@pytest.mark.parametrize("nz", [1, 4, 32, 33])
@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("B", [1, 5, 33])
def test_svi_step_against_float64(target, B, ns, nz):
    lib, dev = target
    beta, lr, clip = 0.7, 0.8, 5.0
    seen_active, seen_inactive = False, False
    for case, (parts, mom) in enumerate([(1, 0.0), (3, 0.5), (3, 0.0), (1, 0.5)]):
        g = torch.Generator().manual_seed(1000 * B + 100 * ns + nz + case)
        phi = torch.randn(B, 2 * nz, generator=g) * 0.5
        vel = torch.randn(B, 2 * nz, generator=g) * 0.3
        eps = torch.randn(B, ns, nz, generator=g)
        rec = torch.rand(B * ns, generator=g) * 30 + 5
        kl = torch.rand(B, generator=g) * 2
        # gradients built so that the clip is active on some rows and inactive on others: rows b with (b + case) even carry a dz of
        # norm ~ 50 * sqrt(ns nz) >> clip, the others one of norm ~ 0.01 * sqrt(ns nz) next to beta-terms of norm < clip
        scale = torch.where((torch.arange(B) + case) % 2 == 0, torch.tensor(50.0), torch.tensor(0.01))
        dzp = torch.randn(parts, B * ns, nz, generator=g) * scale.repeat_interleave(ns).view(1, B * ns, 1)
        L64, g64, active, v64, phi64 = _svi_ref(rec, dzp, eps, kl, beta, lr, mom, clip, phi, vel)
        seen_active |= bool(active.any())
        seen_inactive |= bool((~active).any())
        if B > 1:
            assert bool(active.any()) and bool((~active).any()), "both clip branches in one batch"
        # best tracking: even rows start above L (a new minimum), odd rows far below it (no update)
        best_loss0 = torch.where(torch.arange(B) % 2 == 0, torch.tensor(float("inf")), torch.tensor(-1.0e3))
        best0 = torch.full((B, 2 * nz), 3.25)
        b_phi, d_phi = _guarded(phi, dev)
        b_vel, d_vel = _guarded(vel, dev)
        b_best, d_best = _guarded(best0, dev)
        b_bl, d_bl = _guarded(best_loss0, dev)
        nan = float("nan")
        b_tr, d_tr = _guarded(torch.full((B,), nan), dev)
        b_z, d_z = _guarded(torch.full((B, ns, nz), nan), dev)
        b_kn, d_kn = _guarded(torch.full((B,), nan), dev)
        d_rec, d_dz, d_eps, d_kl = rec.to(dev), dzp.to(dev), eps.to(dev), kl.to(dev)
        klw = torch.tensor([beta], device=dev)
        lib.lv_svi_step_f32(P(d_rec), P(d_dz), parts, P(d_eps), P(d_kl), P(klw), lr, mom, clip, P(d_phi), P(d_vel), P(d_best), P(d_bl),
                            P(d_tr), P(d_z), P(d_kn), B, ns, nz, _s(dev))
        for b in (b_phi, b_vel, b_best, b_bl, b_tr, b_z, b_kn):
            assert _guards_intact(b)
        for out in (d_tr, d_z, d_kn, d_phi, d_vel):
            assert not bool(torch.isnan(out).any()), "an output was not fully overwritten"
        # trace: ns adds, one divide, one multiply-add, each within u of magnitudes bounded by sum|rec|/ns + beta |kl|
        mag = rec.view(B, ns).abs().sum(dim=1).double() / ns + beta * kl.double()
        assert bool(((d_tr.cpu().double() - L64).abs() <= (ns + 3) * U * mag).all())
        # best: even rows updated to (L, phi before the update), odd rows untouched -- bit for bit
        even = torch.arange(B) % 2 == 0
        assert _same(d_bl.cpu()[even], d_tr.cpu()[even]) and _same(d_bl.cpu()[~even], best_loss0[~even])
        assert _same(d_best.cpu()[even], phi[even]) and _same(d_best.cpu()[~even], best0[~even])
        # update.  Operation count per coordinate: parts * ns adds for dz (+ ns multiply-adds with eps), two expf (<= 2 ulp each), 6
        # multiplies / adds for the KL term; the clip coefficient: 2 ceil(nz / 64) squares and adds per lane, 6 butterfly adds,
        # sqrt, add, divide, min; then 2 multiply-adds for vel and 1 for phi.  Each operation contributes at most u relative to
        # the magnitude sum A of the terms it combines (no cancellation is assumed away: A sums absolute values).
        ops = parts * ns + ns + 2 * 2 + 6 + (2 * math.ceil(nz / 64) + 6 + 4) + 3
        mu, lv = phi[:, :nz].double(), phi[:, nz:].double()
        sd = (0.5 * lv).exp()
        adz = dzp.double().abs().sum(dim=0).view(B, ns, nz)
        A = torch.cat((adz.sum(dim=1) + beta * mu.abs(), (adz * eps.double().abs()).sum(dim=1) * 0.5 * sd
                       + beta * 0.5 * (lv.exp() + 1.0)), dim=1)
        bound_v = ops * U * (mom * vel.double().abs() + A)
        bound_phi = bound_v * lr + ops * U * phi.double().abs()
        assert bool(((d_vel.cpu().double() - v64).abs() <= bound_v).all()), float(((d_vel.cpu().double() - v64).abs() / bound_v).max())
        assert bool(((d_phi.cpu().double() - phi64).abs() <= bound_phi).all()), float(((d_phi.cpu().double() - phi64).abs() / bound_phi).max())
        # z_next / kl_next: what lv_reparam_kl_fwd_f32 gives for the updated mulv, bit for bit
        z2, kl2 = torch.empty(B, ns, nz, device=dev), torch.empty(B, device=dev)
        lib.lv_reparam_kl_fwd_f32(P(d_phi), P(d_eps), P(z2), P(kl2), B, ns, nz, _s(dev))
        assert _same(d_z, z2) and _same(d_kn, kl2)
    assert seen_active and seen_inactive


@pytest.mark.parametrize("B,ns,nz", [(5, 3, 4), (33, 1, 33)])
def test_svi_step_finish_mode_and_ties(target, B, ns, nz):
    """Finish mode (NULL dz) records and tracks the best iterate only; an equal L keeps the EARLIER iterate, a smaller one wins."""
    lib, dev = target
    g = torch.Generator().manual_seed(B + nz)
    phi_a, phi_b = torch.randn(B, 2 * nz, generator=g).to(dev), torch.randn(B, 2 * nz, generator=g).to(dev)
    rec = (torch.rand(B * ns, generator=g) * 20).to(dev)
    kl = torch.rand(B, generator=g).to(dev)
    klw = torch.tensor([1.0], device=dev)
    best = torch.full((B, 2 * nz), float("nan"), device=dev)
    best_loss = torch.full((B,), float("inf"), device=dev)
    b_tr, tr = _guarded(torch.full((B,), float("nan")), dev)

    def finish(phi):
        before = phi.clone()
        lib.lv_svi_step_f32(P(rec), None, 0, None, P(kl), P(klw), 1.0, 0.5, 5.0, P(phi), None, P(best), P(best_loss), P(tr), None, None,
                            B, ns, nz, _s(dev))
        assert _same(phi, before) and _guards_intact(b_tr)
    finish(phi_a)
    assert _same(best, phi_a) and _same(best_loss, tr) and not bool(torch.isnan(tr).any())
    finish(phi_b)                                       # the same L: a tie keeps the earlier iterate
    assert _same(best, phi_a)
    rec[:ns] -= 1.0                                     # sentence 0 improves, the others tie again
    finish(phi_b)
    assert _same(best[0], phi_b[0]) and _same(best[1:], phi_a[1:])
    assert _same(best_loss, tr)


def test_svi_step_bad_arguments_write_nothing(target):
    lib, dev = target
    raw = lib._raw_lv_svi_step_f32
    B, ns, nz = 3, 2, 4
    t = {k: torch.full(shape, POISON, device=dev) for k, shape in
         dict(rec=(B * ns,), dz=(1, B * ns, nz), eps=(B, ns, nz), kl=(B,), klw=(1,), phi=(B, 2 * nz), vel=(B, 2 * nz), best=(B, 2 * nz),
              bl=(B,), tr=(B,), z=(B, ns, nz), kn=(B,)).items()}

    def call(**kw):
        a = dict(rec=P(t["rec"]), dz=P(t["dz"]), parts=1, eps=P(t["eps"]), kl=P(t["kl"]), klw=P(t["klw"]), lr=1.0, mom=0.5, clip=5.0,
                 phi=P(t["phi"]), vel=P(t["vel"]), best=P(t["best"]), bl=P(t["bl"]), tr=P(t["tr"]), z=P(t["z"]), kn=P(t["kn"]), B=B, ns=ns,
                 nz=nz)
        a.update(kw)
        return raw(a["rec"], a["dz"], a["parts"], a["eps"], a["kl"], a["klw"], a["lr"], a["mom"], a["clip"], a["phi"], a["vel"], a["best"],
                   a["bl"], a["tr"], a["z"], a["kn"], a["B"], a["ns"], a["nz"], _s(dev))
    for bad in (dict(rec=None), dict(kl=None), dict(klw=None), dict(phi=None), dict(best=None), dict(bl=None), dict(tr=None),
                dict(eps=None), dict(vel=None), dict(z=None), dict(kn=None), dict(B=0), dict(ns=0), dict(nz=-1), dict(parts=0),
                dict(lr=0.0), dict(lr=float("nan")), dict(clip=-1.0), dict(mom=1.0), dict(mom=-0.1)):
        assert call(**bad) < 0, bad
    for k, v in t.items():
        assert bool((v == POISON).all()), k


# ---- 2. lv_dec_tail_dz_f32 ----------------------------------------------------------------------------------------------------------
def _tail_case(lib, dev, Bd, H, nz, ni=8):
    g = torch.Generator().manual_seed(Bd * 7 + H + nz)
    dGsum = torch.randn(Bd, 4 * H, generator=g).to(dev)
    dc0 = torch.randn(Bd, H, generator=g).to(dev)
    z = torch.randn(Bd, nz, generator=g).to(dev)
    wih = (torch.randn(4 * H, ni + nz, generator=g) / H ** 0.5).to(dev)
    wtr = (torch.randn(H, nz, generator=g) / nz ** 0.5).to(dev)
    parts = lib.lv_dec_tail_parts(H)
    gwih, gwtr = torch.empty(4 * H, ni + nz, device=dev), torch.empty(H, nz, device=dev)
    gb1, gb2 = torch.empty(4 * H, device=dev), torch.empty(4 * H, device=dev)
    full = torch.empty(parts, Bd, nz, device=dev)
    lib.lv_dec_tail_bwd_f32(P(dGsum), P(dc0), P(z), P(wih), ni + nz, ni, P(wtr), P(gwih), ni + nz, P(gwtr), P(gb1), P(gb2), P(full),
                            Bd, H, nz, _s(dev))
    buf, only = _guarded(torch.full((parts, Bd, nz), float("nan")), dev)
    lib.lv_dec_tail_dz_f32(P(dGsum), P(dc0), P(wih), ni + nz, ni, P(wtr), P(only), Bd, H, nz, _s(dev))
    assert _guards_intact(buf) and not bool(torch.isnan(only).any())
    assert _same(only, full)
    # and the partials are the product they claim to be
    want = dGsum.double().cpu() @ wih.double().cpu()[:, ni:] + dc0.double().cpu() @ wtr.double().cpu()
    assert rel_err(only.sum(dim=0), want) < 1e-5


@pytest.mark.parametrize("Bd,H,nz", [(4, 16, 4), (33, 64, 32)])
def test_dec_tail_dz_equals_full_tail(target, Bd, H, nz):
    """The gradient buffers do not even reach the dz entry (its signature has no such pointer); test 3 checks flat.grad."""
    _tail_case(*target, Bd, H, nz)


@pytest.mark.gpu
def test_dec_tail_dz_equals_full_tail_h1024(hip_device):
    _tail_case(E.backend_for(hip_device), hip_device, 8, 1024, 32)


def test_dec_tail_dz_bad_arguments(target):
    lib, dev = target
    a = torch.zeros(64, device=dev)
    raw = lib._raw_lv_dec_tail_dz_f32
    assert raw(None, P(a), P(a), 8, 4, P(a), P(a), 1, 2, 4, _s(dev)) < 0
    assert raw(P(a), P(a), P(a), 7, 4, P(a), P(a), 1, 2, 4, _s(dev)) < 0          # ld_wih < col0 + nz
    assert raw(P(a), P(a), P(a), 8, 4, P(a), P(a), 0, 2, 4, _s(dev)) < 0


# ---- 3. dz-only backward against the full backward -------------------------------------------------------------------------------
def _dz_only_case(dev, V, ni, H, nz, B, T, ns, precision="f32", scale=0.3):
    vae = _small_vae(dev, V, ni, H, nz, seed=73, scale=scale)
    vae.set_precision(precision)
    vae.eval()
    eng = vae.decoder._hip
    x = _batch(B, T, V, 74, dev)
    g = torch.Generator().manual_seed(75)
    z = (torch.randn(B, ns, nz, generator=g) * 0.7).to(dev)
    drec = (torch.rand(B * ns, generator=g) + 0.5).to(dev)
    eng.forward(x, z, None, None, 0.0, 0.0)
    dz_full = eng.backward(drec).clone()
    eng.join()
    E.check_persistent_status(eng)
    eng.forward(x, z, None, None, 0.0, 0.0)            # (the f32 softmax backward rewrites the logits in place)
    eng.flat.grad_padded.fill_(float("nan"))
    poisoned = eng.flat.grad_padded.clone()
    dz_only = eng.backward_dz(drec).clone()
    E.check_persistent_status(eng)
    assert _same(eng.flat.grad_padded, poisoned), "backward_dz wrote to flat.grad"
    eng.flat.grad_padded.zero_()
    if precision == "bf16" and H == 1024:
        assert E._persistent_ok(eng, eng._lstm_images(B * ns, T - 1, ns), B * ns, H, dev, E._PERSIST_BWD_MAX_B), "not on the persistent route"
    return dz_full, dz_only


@pytest.mark.parametrize("B,T,ns", [(4, 6, 1), (5, 7, 3)])
def test_backward_dz_equals_full_backward(target, B, T, ns):
    _, dev = target
    dz_full, dz_only = _dz_only_case(dev, 53, 8, 16, 4, B, T, ns)
    assert float(dz_full.abs().max()) > 0 and _same(dz_only, dz_full)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_backward_dz_equals_full_backward_h1024(hip_device, precision):
    dz_full, dz_only = _dz_only_case(hip_device, 2003, 32, 1024, 32, 8, 12, 1, precision=precision, scale=0.05)
    if precision == "f32":
        assert _same(dz_only, dz_full)
    else:
        # parity_common.check_bf16_native_operands_equal_on_the_fly's bound on bf16 gradients: 5e-3 max-norm relative
        assert rel_err(dz_only, dz_full) < 5e-3


# ---- 4. per-iteration work ------------------------------------------------------------------------------------------------------------
ONCE_PER_CALL = ("lv_embed_gather_f32", "lv_embed_gather_b16", "lv_embed_scatter_f32", "lv_embed_scatter_full_f32",
                 "lv_embed_scatter_full_sumsq_f32", "lv_token_sort", "lv_repeat_rows_i64",
                 "lv_cvt_bf16_f32", "lv_cvt_bf16_lo_f32", "lv_cvt_h16_f32", "lv_gate_interleave_f32",
                 "lv_lstm_persist16_pack", "lv_lstm_persist16_pack2")
# weight-gradient product entries: none may run at all (the f32 products share lv_gemm_f32 with the forward and are told apart by
# their transposed-A form, tA = 1; dX is the (0, 0) product with N = ni)
WGRAD_ENTRIES = ("lv_dec_tail_bwd_f32", "lv_gemm_b16_sumsq", "lv_gemm_b16_dual", "lv_gemm_b16_pair", "lv_conv32_wgrad_f32")
RECURRENCES = ("lv_lstm_fwd_f32", "lv_lstm_bwd_f32")


def _counts(calls):
    c = {}
    for name, _ in calls:
        c[name] = c.get(name, 0) + 1
    return c


def test_per_iteration_work(target):
    _, dev = target
    V, ni, H, nz, B, T = 53, 8, 16, 4, 4, 6
    vae = _small_vae(dev, V, ni, H, nz)
    x = _batch(B, T, V, 76, dev)
    eps = torch.randn(B, 3, nz, generator=torch.Generator().manual_seed(1)).to(dev)
    vae.refine_posterior(x, steps=1, nsamples=3, noise=eps)          # workspaces and weight images exist from here on
    runs = {}
    for steps in (1, 3):
        with spying() as calls:
            info = vae.refine_posterior(x, steps=steps, nsamples=3, noise=eps, return_info=True)[2]
        assert info["route"] == "fused"
        runs[steps] = (_counts(calls), list(calls))
    c1, c3 = runs[1][0], runs[3][0]
    for name in ONCE_PER_CALL:
        assert c3.get(name, 0) == c1.get(name, 0), (name, c1.get(name, 0), c3.get(name, 0))
    assert c1["lv_embed_gather_f32"] >= 1
    for counts, calls in runs.values():
        for name in WGRAD_ENTRIES:
            assert counts.get(name, 0) == 0, name
        for name, a in calls:
            if name in ("lv_gemm_f32", "lv_gemm_bf16"):
                assert a[0] == 0, "a transposed-A (weight-gradient) product ran"
                assert not (a[0] == 0 and a[1] == 0 and a[3] == ni), "dX ran"
    for name in RECURRENCES + ("lv_svi_step_f32", "lv_dec_tail_dz_f32", "lv_dec_init_f32", "lv_gx_expand_add_f32"):
        assert c3[name] - c1[name] == 2, (name, c1[name], c3[name])
    assert c1["lv_svi_step_f32"] == 2 and c1["lv_lstm_bwd_f32"] == 1
    # the forward products: the input projection once per call (encoder + decoder), logits and dO once per iteration
    assert c3["lv_gemm_f32"] - c1["lv_gemm_f32"] == 4


@pytest.mark.gpu
def test_per_iteration_work_bf16(hip_device):
    """What the bf16 route does per iteration, pinned: like f32 it runs no weight-gradient product, no dX, no scatter and one
    lv_dec_tail_dz_f32 / lv_svi_step_f32 per step -- but it runs the training forward() as it is, so the embedding gather into the
    operand images and the three-image conversion of the hidden states (two of which only the dropped products would read) ARE
    repeated every iteration (not hoisted yet); the token sort is served from the per-batch cache."""
    dev = hip_device
    V, ni, H, nz, B, T = 2003, 32, 1024, 32, 8, 12
    vae = _small_vae(dev, V, ni, H, nz, seed=78, scale=0.05)
    vae.set_precision("bf16")
    x = _batch(B, T, V, 79, dev)
    eps = torch.randn(B, 1, nz, generator=torch.Generator().manual_seed(1)).to(dev)
    vae.refine_posterior(x, steps=1, noise=eps)
    runs = {}
    for steps in (1, 3):
        with spying() as calls:
            info = vae.refine_posterior(x, steps=steps, noise=eps, return_info=True)[2]
        assert info["route"] == "fused"
        runs[steps] = (_counts(calls), list(calls))
    c1, c3 = runs[1][0], runs[3][0]
    for counts, calls in runs.values():
        for name in WGRAD_ENTRIES + ("lv_embed_scatter_f32", "lv_embed_scatter_full_f32", "lv_embed_scatter_full_sumsq_f32"):
            assert counts.get(name, 0) == 0, name
        for name, a in calls:
            if name in ("lv_gemm_f32", "lv_gemm_bf16", "lv_gemm_b16"):
                assert a[0] == 0, "a transposed-A (weight-gradient) product ran: %s" % name
    for name in ("lv_svi_step_f32", "lv_dec_tail_dz_f32", "lv_lstm_fwd_bf16_persist16", "lv_lstm_bwd_bf16_persist16"):
        assert c3[name] - c1[name] == 2, (name, c1.get(name), c3.get(name))
    for name in ("lv_embed_gather_b16", "lv_cvt_bf16_hs3_f32"):            # the repeated z-independent / unused work
        assert c3[name] - c1[name] == 2, (name, c1.get(name), c3.get(name))
    for name in ("lv_token_sort", "lv_lstm_persist16_pack", "lv_lstm_persist16_pack2"):
        assert c3.get(name, 0) == c1.get(name, 0), name


# ---- 5. the reference fixture ----------------------------------------------------------------------------------------------------------
def _fixture_case(fx, name, dev):
    V, ni, H, nz, ns = (int(v) for v in fx[name + "/dims"])
    lr, mom, clip, beta = (float(v) for v in fx[name + "/hyper"])
    params = {k: torch.from_numpy(fx[name + "/param/" + k]) for k in ALL_KEYS}
    vae = build_vae(V, ni, H, nz, dev, params=params)
    x = torch.from_numpy(fx[name + "/x"]).to(dev)
    eps = torch.from_numpy(fx[name + "/eps"]).to(dev)
    return vae, x, eps, dict(lr=lr, momentum=mom, clip=clip, kl_weight=beta, nsamples=ns)


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_refine_against_reference_fixture(target, name):
    _, dev = target
    fx = load("svi_small")
    vae, x, eps, kw = _fixture_case(fx, name, dev)
    phi32, phi64 = fx[name + "/phi32"], fx[name + "/phi64"]
    K = phi32.shape[0] - 1
    dev_k = np.abs(phi32.astype(np.float64) - phi64).max(axis=(1, 2))
    trace = None
    for k in range(K + 1):                              # phi_k = the last iterate of a k-step run
        mu, logvar, info = vae.refine_posterior(x, steps=k, noise=eps, keep="last", return_info=True, **kw)
        assert info["route"] == "fused"
        got = torch.cat((mu, logvar), dim=1).cpu().numpy().astype(np.float64)
        bound = max(RTOL * float(np.abs(phi32[k]).max()), 4.0 * float(dev_k[k]))
        err = float(np.abs(got - phi32[k]).max())
        assert err <= bound, (k, err, bound)
        trace = info["trace"]
    assert rel_err(trace, fx[name + "/trace32"]) < RTOL
    mu, logvar, info = vae.refine_posterior(x, steps=K, noise=eps, return_info=True, **kw)
    best = torch.from_numpy(fx[name + "/best"])
    assert torch.equal(info["trace"].argmin(dim=0).cpu(), best)                       # the kept index, exactly
    got = torch.cat((mu, logvar), dim=1).cpu()
    rows = torch.arange(got.shape[0])
    assert _same(info["loss"], info["trace"][best.to(dev), rows.to(dev)])
    bound = max(RTOL * float(np.abs(fx[name + "/kept"]).max()), 4.0 * float(dev_k.max()))
    assert float((got.double() - torch.from_numpy(fx[name + "/kept"]).double()).abs().max()) <= bound


# ---- 6. route equality -------------------------------------------------------------------------------------------------------------------
def _routes_agree(vae, x, eps, **kw):
    out = {}
    for fused in (True, False):
        vae.fused_svi = fused
        try:
            mu, logvar, info = vae.refine_posterior(x, noise=eps, return_info=True, **kw)
        finally:
            del vae.fused_svi
        assert info["route"] == ("fused" if fused else "generic")
        out[fused] = (mu, logvar, info)
    (mu_f, lv_f, i_f), (mu_g, lv_g, i_g) = out[True], out[False]
    assert rel_err(i_f["trace"], i_g["trace"]) < RTOL
    for a, b in ((mu_f, mu_g), (lv_f, lv_g)):
        assert float((a - b).abs().max()) <= RTOL * float(torch.cat((mu_g, lv_g), dim=1).abs().max())
    return out


@pytest.mark.parametrize("ns,keep", [(1, "best"), (3, "last")])
def test_fused_route_equals_generic_route(target, ns, keep):
    _, dev = target
    vae = _small_vae(dev)
    x = _batch(5, 7, 53, 77, dev)
    eps = torch.randn(5, ns, 4, generator=torch.Generator().manual_seed(2)).to(dev)
    _routes_agree(vae, x, eps, steps=4, nsamples=ns, keep=keep, kl_weight=0.8)


@pytest.mark.gpu
def test_fused_route_equals_generic_route_h1024(hip_device):
    V, ni, H, nz, B, T = 2003, 32, 1024, 32, 8, 12
    vae = _small_vae(hip_device, V, ni, H, nz, seed=78, scale=0.05)
    x = _batch(B, T, V, 79, hip_device)
    eps = torch.randn(B, 1, nz, generator=torch.Generator().manual_seed(3)).to(hip_device)
    _routes_agree(vae, x, eps, steps=3)


# ---- 7. properties -----------------------------------------------------------------------------------------------------------------------
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


def _assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if torch.is_tensor(a[k]):
            assert b[k] is not None and _same(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("fused", [True, False])
def test_refine_leaves_the_model_alone(target, fused):
    _, dev = target
    vae = _small_vae(dev)
    vae.train()
    assert vae.decoder.dropout_in.p == 0.5 and vae.decoder.dropout_out.p == 0.5 and vae.decoder.training
    x = _batch(4, 6, 53, 80, dev)
    vae.loss(x, 1.0)[0].mean().backward()               # gradients exist (views of the flat buffers) before the call
    eps = torch.randn(4, 2, 4, generator=torch.Generator().manual_seed(4)).to(dev)
    before = _state(vae)
    grad_ids = {k: id(p.grad) for k, p in vae.named_parameters()}
    vae.fused_svi = fused
    try:
        mu, logvar, info = vae.refine_posterior(x, steps=3, nsamples=2, noise=eps, return_info=True)
    finally:
        del vae.fused_svi
    assert info["route"] == ("fused" if fused else "generic")
    assert not mu.requires_grad and not logvar.requires_grad
    _assert_same_state(before, _state(vae))
    assert grad_ids == {k: id(p.grad) for k, p in vae.named_parameters()}       # the same .grad OBJECTS as before


def test_refine_properties(target):
    _, dev = target
    vae = _small_vae(dev)
    B, T, ns, beta = 4, 6, 2, 0.9
    x = _batch(B, T, 53, 81, dev)
    eps = torch.randn(B, ns, 4, generator=torch.Generator().manual_seed(5)).to(dev)
    vae.eval()
    with torch.no_grad():
        mu0, lv0 = vae.encode_stats(x)
        loss_ref = vae.loss(x, beta, nsamples=ns, noise=(eps, None, None))[0]
    vae.train()
    mu, logvar, info = vae.refine_posterior(x, steps=6, nsamples=ns, noise=eps, kl_weight=beta, return_info=True)
    assert bool((info["loss"] <= info["loss0"]).all())                              # keep = "best": exactly
    assert _same(info["loss0"], info["trace"][0]) and _same(info["loss"], info["trace"].min(dim=0)[0])
    assert rel_err(info["trace"][0], loss_ref) < RTOL
    assert bool((info["trace"].min(dim=0)[0] < info["trace"][0]).any()), "the refinement improved no sentence"
    # steps = 0: the encoder's output, bit for bit, and no backward
    with spying() as calls:
        m0, l0 = vae.refine_posterior(x, steps=0, nsamples=ns, noise=eps)
        m0i, l0i, i0 = vae.refine_posterior(x, steps=0, nsamples=ns, noise=eps, return_info=True)
    assert _same(m0, mu0) and _same(l0, lv0) and _same(m0i, mu0) and _same(l0i, lv0) and tuple(i0["trace"].shape) == (1, B)
    names = {n for n, _ in calls}
    assert not names & {"lv_lstm_bwd_f32", "lv_softmax_nll_bwd_f32", "lv_dec_tail_dz_f32", "lv_dec_tail_bwd_f32"}, names
    # keep = "last" returns phi_K: bit-equal to the `last` array of the same engine call
    ml, ll, il = vae.refine_posterior(x, steps=6, nsamples=ns, noise=eps, kl_weight=beta, keep="last", return_info=True)
    vae.eval()
    with torch.no_grad():
        r = vae.decoder._hip.svi_refine(x, vae.encoder._forward_mulv(x).contiguous(), eps, 6, 1.0, 0.5, 5.0, beta)
    vae.train()
    assert _same(torch.cat((ml, ll), dim=1), r["last"]) and _same(torch.cat((mu, logvar), dim=1), r["best"])
    assert _same(il["rec"], r["rec_trace"][6]) and _same(il["kl"], r["kl_trace"][6])
    # rec / kl of the report are the two terms of the kept iterate's L_b as the loop computed them
    k = info["trace"].argmin(dim=0, keepdim=True)
    assert _same(info["rec"], r["rec_trace"].gather(0, k)[0]) and _same(info["kl"], r["kl_trace"].gather(0, k)[0])
    assert float((info["rec"] + beta * info["kl"] - info["loss"]).abs().max()) <= 4 * U * float(info["loss"].abs().max())
    with torch.no_grad():
        kl_kept = 0.5 * (mu.double() ** 2 + logvar.double().exp() - logvar.double() - 1).sum(dim=1)
    assert rel_err(info["kl"], kl_kept) < 1e-5
    assert _same(il["loss"], il["trace"][6]) and _same(il["trace"], info["trace"])
    worse = info["trace"][6] > info["trace"].min(dim=0)[0]
    if bool(worse.any()):
        assert not _same(ml[worse], mu[worse])
    # a sentence alone: no cross-sentence term
    for b in (0, B - 1):
        m1, l1, i1 = vae.refine_posterior(x[b:b + 1], steps=6, nsamples=ns, noise=eps[b:b + 1].contiguous(), kl_weight=beta,
                                          return_info=True)
        assert rel_err(i1["trace"][:, 0], info["trace"][:, b]) < RTOL
        scale = float(torch.cat((mu, logvar), dim=1).abs().max())
        assert float((m1[0] - mu[b]).abs().max()) <= RTOL * scale and float((l1[0] - logvar[b]).abs().max()) <= RTOL * scale


# ---- 8. wiring ---------------------------------------------------------------------------------------------------------------------------
def test_amortization_gap_equals_hand_computation(target):
    _, dev = target
    vae = _small_vae(dev)
    batches = [_batch(B, T, 53, 82 + i, dev) for i, (B, T) in enumerate([(4, 6), (3, 5), (5, 7)])]
    gen = torch.Generator(device=dev).manual_seed(11)
    res = EV.calc_amortization_gap(vae, batches, steps=4, nsamples=2, np_rng=np.random.RandomState(3), generator=gen)
    gen = torch.Generator(device=dev).manual_seed(11)
    enc = svi = 0.0
    for i in np.random.RandomState(3).permutation(len(batches)):
        info = vae.refine_posterior(batches[i], steps=4, nsamples=2, generator=gen, return_info=True)[2]
        enc += float(info["loss0"].sum())
        svi += float(info["loss"].sum())
    n = sum(b.size(0) for b in batches)
    assert res["n"] == n and res["gap"] >= 0.0
    assert abs(res["elbo_enc"] + enc / n) <= 1e-6 * abs(enc / n) and abs(res["elbo_svi"] + svi / n) <= 1e-6 * abs(svi / n)
    assert abs(res["gap"] - (res["elbo_svi"] - res["elbo_enc"])) <= 1e-12


@pytest.mark.parametrize("C,nterms,act", [(3, 1, True), (16, 3, True), (64, 4, False), (64, 2, True)])
def test_bn_eval_bwd_against_float64(target, C, nterms, act):
    """lv_bn_eval_bwd_f32: the backward of the eval-mode BatchNorm (+ residual) (+ ELU).  Bounds, relative to the sum G of the
    summands' absolute values: dv = G-sum * elu'(y) -- nterms adds and a multiply, plus the error of elu'(y) = y + 1 read from the f32
    forward: the pre-activation o carries 6 roundings of its own magnitude sum M (sub, three multiplies, two adds), |d elu'/do| <= 1,
    and expm1 / the add contribute 4 more -- so |dv error| <= G * ((nterms + 1) + 6 M + 4) u; dx adds three multiplies; the parameter
    gradients are sums over Pn rows of such terms, held to Pn more roundings of the sum of absolute terms (any summation order)."""
    lib, dev = target
    Pn = 2 * 49 + 1
    g = torch.Generator().manual_seed(C * 10 + nterms)
    x = torch.randn(Pn, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    rmean, rvar = torch.randn(C, generator=g) * 0.3, torch.rand(C, generator=g) + 0.2
    res = torch.randn(Pn, C, generator=g)
    dys = [torch.randn(Pn, C, generator=g) for _ in range(nterms)]
    d = lambda t: t.to(dev)
    y, mean, invstd = (torch.empty(Pn, C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev))
    dx_, dg, db, drm, drv, dres = d(x), d(gamma), d(beta), d(rmean), d(rvar), d(res)      # (kept alive: the launch is asynchronous)
    lib.lv_bn_eval_f32(P(dx_), P(dg), P(db), P(drm), P(drv), 1e-5, P(dres), int(act), P(y), P(mean), P(invstd), Pn, C, _s(dev))
    ddys = [d(t) for t in dys] + [None] * (4 - nterms)
    b_dv, dv = _guarded(torch.full((Pn, C), float("nan")), dev)
    b_dx, dxo = _guarded(torch.full((Pn, C), float("nan")), dev)
    b_gg, gg = _guarded(torch.full((C,), 2.0), dev)
    b_gb, gb = _guarded(torch.full((C,), -3.0), dev)
    for accumulate in (0, 1):
        lib.lv_bn_eval_bwd_f32(P(dx_), P(ddys[0]), P(ddys[1]), P(ddys[2]), P(ddys[3]), P(y), P(mean), P(invstd), P(dg), int(act), P(dv),
                               P(dxo), P(gg), P(gb), accumulate, Pn, C, _s(dev))
    for b in (b_dv, b_dx, b_gg, b_gb):
        assert _guards_intact(b)
    # float64 statement through autograd
    x64 = x.double().requires_grad_(True)
    r64 = res.double().requires_grad_(True)
    g64, be64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    o = (x64 - rmean.double()) / (rvar.double() + 1e-5).sqrt() * g64 + be64 + r64
    if act:
        o = torch.nn.functional.elu(o)
    dy64 = sum(t.double() for t in dys)
    o.backward(dy64)
    G = sum(t.double().abs() for t in dys)
    istd = 1.0 / (rvar.double() + 1e-5).sqrt()
    M = (x.double() - rmean.double()).abs() * istd * gamma.double() + beta.double().abs() + res.double().abs()
    e_dv = G * ((nterms + 1) + (6 * M + 4 if act else 0)) * U
    assert bool(((dv.cpu().double() - r64.grad).abs() <= e_dv + 1e-30).all())
    scale = gamma.double() * istd
    e_dx = (e_dv + 3 * U * G) * scale
    assert bool(((dxo.cpu().double() - x64.grad).abs() <= e_dx + 1e-30).all())
    xhat = (x.double() - rmean.double()).abs() * istd
    # two launches: '=' then '+=' -> twice the gradient
    assert bool(((gb.cpu().double() - 2 * be64.grad).abs() <= 2 * (e_dv + Pn * U * G).sum(dim=0) + 1e-30).all())
    assert bool(((gg.cpu().double() - 2 * g64.grad).abs() <= 2 * ((e_dv + (Pn + 3) * U * G) * xhat).sum(dim=0) + 1e-30).all())
    raw = lib._raw_lv_bn_eval_bwd_f32
    assert raw(None, P(ddys[0]), None, None, None, P(y), P(mean), P(invstd), P(dg), 1, P(dv), P(dxo), P(gg), P(gb), 0, Pn, C, _s(dev)) < 0
    assert raw(P(dx_), P(ddys[0]), None, P(ddys[0]), None, P(y), P(mean), P(invstd), P(dg), 1, P(dv), P(dxo), P(gg), P(gb), 0, Pn, C, _s(dev)) < 0
    assert raw(P(dx_), P(ddys[0]), None, None, None, P(y), P(mean), P(invstd), P(dg), 1, P(dv), P(dxo), P(gg), P(gb), 0, 0, C, _s(dev)) < 0


def _image_case(dev, B):
    from parity_common import build_image_vae
    vae = build_image_vae(dev, 31)
    x = (torch.rand(B, 1, 28, 28, generator=torch.Generator().manual_seed(6)) < 0.4).float().to(dev)
    eps = torch.randn(B, 1, vae.nz, generator=torch.Generator().manual_seed(7)).to(dev)
    return vae, x, eps


def test_image_decoder_eval_backward_to_z_against_oracle(target):
    """The eval-mode PixelCNN decoder differentiated with respect to z (what the generic route of refine_posterior needs), against
    torch autograd on the oracle's eval-mode restatement; parity_common's bounds on rec and on a gradient."""
    from oracle import image_vae_oracle as IO
    from parity_common import GRAD_RTOL
    _, dev = target
    B = 2
    vae, x, eps = _image_case(dev, B)
    vae.eval()
    sd = {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}
    z = (eps * 0.5).clone().requires_grad_(True)
    rec = vae.decoder.reconstruct_error(x, z)
    dz, = torch.autograd.grad(rec, z, torch.ones_like(rec))
    zr = (eps.cpu() * 0.5).clone().requires_grad_(True)
    rec_r = IO.decoder_reconstruct_error(IO.Ctx(sd, train=False), x.cpu(), zr)
    dz_r, = torch.autograd.grad(rec_r.sum(), zr)
    assert rel_err(rec, rec_r) < RTOL
    assert bool(torch.isfinite(dz).all()) and rel_err(dz, dz_r) < GRAD_RTOL, rel_err(dz, dz_r)


@pytest.mark.gpu
def test_pixelcnn_refine_smoke_and_image_gap(hip_device):
    """B = 2, K = 1 on the generic route; image_calc_amortization_gap over a loader equals the hand computation."""
    vae, x, eps = _image_case(hip_device, 2)
    vae.train()
    with torch.no_grad():
        vae.loss(x, 1.0)              # MaskedConv2d masks its weight in place on EVERY forward, as the reference does: idempotent from here on
    before = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    mu, logvar, info = vae.refine_posterior(x, steps=1, noise=eps, return_info=True)
    assert info["route"] == "generic" and tuple(mu.shape) == (2, vae.nz) and tuple(info["trace"].shape) == (2, 2)
    assert bool(torch.isfinite(info["trace"]).all()) and bool((info["loss"] <= info["loss0"]).all())
    assert bool((info["trace"][1] < info["trace"][0]).all()), "one step along the gradient did not lower L_b"
    for k, v in vae.state_dict().items():                  # BatchNorm statistics and weights as before, module still training
        assert _same(v, before[k]), k
    assert vae.training and vae.decoder.training
    loader = [(x, None), (x.flip(0).contiguous(), None)]
    gen = torch.Generator(device=hip_device).manual_seed(5)
    res = EV.image_calc_amortization_gap(vae, loader, steps=1, generator=gen)
    gen = torch.Generator(device=hip_device).manual_seed(5)
    enc = svi = 0.0
    for xb, _ in loader:
        i2 = vae.refine_posterior(xb, steps=1, generator=gen, return_info=True)[2]
        enc += float(i2["loss0"].sum())
        svi += float(i2["loss"].sum())
    assert res["n"] == 4 and res["gap"] >= 0.0
    assert abs(res["elbo_enc"] + enc / 4) <= 1e-6 * abs(enc / 4) and abs(res["elbo_svi"] + svi / 4) <= 1e-6 * abs(svi / 4)


def test_refusals_come_before_any_launch(target):
    _, dev = target
    vae = _small_vae(dev)
    B, T, nz = 4, 6, 4
    x = _batch(B, T, 53, 90, dev)
    for eng in (vae.encoder._hip, vae.decoder._hip):
        eng.ensure(dev)
    ok = torch.zeros(B, 1, nz, device=dev)
    with spying() as calls:
        for kw in (dict(steps=-1), dict(lr=0.0), dict(lr=-1.0), dict(clip=0.0), dict(momentum=1.0), dict(momentum=-0.1),
                   dict(keep="first"), dict(nsamples=0), dict(noise=torch.zeros(B, 2, nz, device=dev)),
                   dict(noise=torch.zeros(B + 1, 1, nz, device=dev)), dict(noise=ok.double()), dict(noise=ok.to("meta")),
                   dict(noise=[0.0])):
            with pytest.raises(ValueError):
                vae.refine_posterior(x, **kw)
        with pytest.raises(ValueError, match="variable-length"):
            vae.refine_posterior((x, [6, 5, 4, 3]))
    assert [n for n, _ in calls] == [], calls
    assert tuple(vae.refine_posterior(x, steps=1, noise=ok)[0].shape) == (B, nz)       # and the same objects still work

"""The model posterior on a latent grid (lv_grid_posterior.hip; VAE.eval_log_model_posterior / calc_model_posterior_mean,
reference modules/vae.py:170-196, 256-273): the shared-sentence conditional log-likelihood kernel and the grid normalisation
against float64 restatements built on oracle.text_vae_oracle, the envelope query, the drop-in routing, and the drop-in
methods against the reference's own numbers (tests/golden/grid_posterior_small.npz).  Unmarked tests run the same kernel
sources on the emulator; the @gpu tests run the toy shape on the MI355X."""
import math

import pytest
import torch

from helpers import build_vae, load, rel_err
from oracle import text_vae_oracle as O
from vae_lagging_encoder_amd import engine as E
from vae_lagging_encoder_amd.factory import build_text_vae


def _params(V, ni, H, nz, seed):
    # weights wide enough that the posterior is far from the prior (U(-0.01, 0.01) leaves log p(x|z) flat in z)
    return O.random_params(V, ni, H, nz, seed=seed, scale=0.3, emb_scale=0.5)


def _batch(B, T, V, seed, pads=True):
    x = O.synthetic_batch(B, T, V, seed=seed)
    if pads and T > 2:
        x[0, T - 2:] = 0                    # <pad> positions count like any other
    return x


def _oracle_cond_ll(P, x, z):
    """float64 log p(x|z): z [K][nz] (shared) or [B][K][nz], expanded here as the reference does."""
    P64 = {k: v.double() for k, v in P.items()}
    B = x.shape[0]
    zz = z.double().unsqueeze(0).expand(B, *z.shape) if z.dim() == 2 else z.double()
    return -O.decoder_reconstruct_error(P64, x, zz.contiguous())


def _oracle_posterior(cond, z):
    """float64 restatement of eval_prior_dist + log_sum_exp normalisation + the posterior mean."""
    cond = cond.double()
    B, K = cond.shape
    zz = z.double().unsqueeze(0).expand(B, *z.shape) if z.dim() == 2 else z.double()
    nz = zz.shape[-1]
    joint = cond + (-0.5 * (zz * zz).sum(-1) - 0.5 * nz * math.log(2 * math.pi))
    log_post = joint - torch.logsumexp(joint, dim=1, keepdim=True)
    mean = (log_post.exp().unsqueeze(2) * zz).sum(1)
    return log_post, mean


def _grid(zmin, zmax, dz, ndim):
    x = torch.arange(zmin, zmax, dz)
    if ndim == 1:
        return x.unsqueeze(1)
    k = x.size(0)
    return torch.cat((x.unsqueeze(1).repeat(1, k).view(-1, 1), x.repeat(k).unsqueeze(1)), dim=-1)


def _model(V, ni, H, nz, dev, seed):
    P = _params(V, ni, H, nz, seed)
    vae = build_vae(V, ni, H, nz, dev, params=P)
    vae.eval()
    return P, vae


def _check_cond_ll(dev, V, ni, H, nz, B, T, K, shared, seed, tol=1e-4):
    P, vae = _model(V, ni, H, nz, dev, seed)
    x = _batch(B, T, V, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    z = torch.randn(K, nz, generator=g) * 2 if shared else torch.randn(B, K, nz, generator=g) * 2
    eng = vae.decoder._hip
    eng.ensure(torch.device(dev))
    assert eng.cond_ll_supported(T)
    got = eng.cond_ll(x.to(dev), z.to(dev))
    ref = _oracle_cond_ll(P, x, z)
    assert got.shape == (B, K)
    e = rel_err(got, ref)
    assert e < tol, e
    return P, vae, x, z, got, ref


# ---- emulator (GPU-less CI) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ni,H,nz,B,T,K,shared", [
    (53, 8, 16, 1, 3, 6, 20, True),        # shared nz = 1 grid, a partial sample tile
    (41, 6, 20, 2, 2, 5, 18, False),       # per-sentence z, nz = 2, H not a multiple of 16
    (37, 8, 16, 4, 3, 2, 16, True),        # T = 2: one decoder step; the small fixtures' ni / H / nz
])
def test_cond_ll_matches_float64_oracle_emulated(emu_backend, V, ni, H, nz, B, T, K, shared):
    _check_cond_ll("cpu", V, ni, H, nz, B, T, K, shared, seed=V)


@pytest.mark.parametrize("shared", [True, False])
def test_grid_normalisation_matches_float64_restatement_emulated(emu_backend, shared):
    g = torch.Generator().manual_seed(5)
    B, K, nz = 3, 300, 2
    cond = torch.randn(B, K, generator=g) * 20 - 40
    z = torch.randn(K, nz, generator=g) if shared else torch.randn(B, K, nz, generator=g)
    log_post, mean = E.grid_posterior(cond, z)
    ref_lp, ref_mean = _oracle_posterior(cond, z)
    mass = ref_lp.exp() > 1e-6
    assert (log_post.double() - ref_lp).abs()[mass].max() < 1e-4
    assert (mean.double() - ref_mean).abs().max() < 1e-5
    lp2, mean2 = E.grid_posterior(cond, z, want_log_post=False)
    assert lp2 is None and torch.equal(mean2, mean)


def test_envelope_query(emu_backend):
    lib = emu_backend
    assert lib.lv_dec_cond_ll_f32_supported(1004, 50, 50, 1, 12)        # toy.py
    assert lib.lv_dec_cond_ll_f32_supported(97, 8, 16, 4, 2)            # small fixtures, T = 2
    assert lib.lv_dec_cond_ll_f32_supported(1004, 50, 50, 2, 100000)    # nz = 2, long sentences
    assert not lib.lv_dec_cond_ll_f32_supported(20000, 512, 1024, 32, 40)
    assert not lib.lv_dec_cond_ll_f32_supported(1004, 50, 50, 1, 1)


def test_argument_checks_negative_without_touching_memory(emu_backend):
    raw = emu_backend.cdll
    assert raw.lv_dec_cond_ll_f32(None, 1, 4, None, 0, 8, None, None, None, None, None, None, None, 10, 4, 8, 1, None, None,
                                  None) < 0
    assert raw.lv_grid_posterior_f32(None, None, 0, 1, 8, 1, None, None, None) < 0


def test_dropin_against_reference_fixture_emulated(emu_backend):
    _check_dropin_fixture("cpu", cases=("nz2",))


def test_dropin_routing_emulated(emu_backend, monkeypatch):
    _check_routing("cpu", monkeypatch)


def test_grid_on_another_device_never_reaches_the_kernels_emulated(emu_backend, monkeypatch):
    _check_device_mismatch("cpu", "meta", emu_backend, monkeypatch)


# ---- shared checks ------------------------------------------------------------------------------------------------------
def _check_dropin_fixture(dev, cases=("nz1", "nz2")):
    fx = load("grid_posterior_small")
    for c in cases:
        V, ni, H, nz = (int(v) for v in fx[c + "/dims"])
        P = {k[len(c) + 7:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith(c + "/param/")}
        vae = build_vae(V, ni, H, nz, dev, params=P)
        vae.eval()
        x = torch.from_numpy(fx[c + "/x"]).to(dev)
        grid = torch.from_numpy(fx[c + "/grid"]).to(dev)
        ref_lp = torch.from_numpy(fx[c + "/log_post"]).double()
        with torch.no_grad():                                   # as toy.py calls them
            lp = vae.eval_log_model_posterior(x, grid).cpu().double()
            mean = vae.calc_model_posterior_mean(x, grid).cpu().double()
        mass = ref_lp.exp() > 1e-6
        assert (lp - ref_lp).abs()[mass].max() < 1e-4, c
        assert (mean - torch.from_numpy(fx[c + "/mean"]).double()).abs().max() < 1e-4, c


def _check_routing(dev, monkeypatch):
    """The fused kernels run exactly where the eval-mode decoder without autograd is what the reference computes: eval mode, or
    train mode with both dropout p = 0, under torch.no_grad(); train mode with live dropout (toy.py's epoch-end dump), grad
    enabled (the result stays differentiable) and fused_grid = False take the generic route."""
    V, ni, H, nz, B, T = 31, 6, 12, 1, 2, 5
    P = _params(V, ni, H, nz, 9)
    x = _batch(B, T, V, 10).to(dev)
    grid = _grid(-2, 2, 0.5, 1).to(dev)
    calls = []
    orig = E.LSTMDecoderEngine.cond_ll

    def counted(self, *a, **k):
        calls.append(1)
        return orig(self, *a, **k)
    monkeypatch.setattr(E.LSTMDecoderEngine, "cond_ll", counted)

    vae = build_vae(V, ni, H, nz, dev, params=P)             # train mode, dropout 0.5 / 0.5
    with torch.no_grad():
        vae.calc_model_posterior_mean(x, grid)
        vae.eval_log_model_posterior(x, grid)
    assert calls == []
    vae.eval()
    with torch.no_grad():
        fused = vae.calc_model_posterior_mean(x, grid)
    assert len(calls) == 1
    with_grad = vae.calc_model_posterior_mean(x, grid)        # autograd on: the generic, differentiable route
    assert len(calls) == 1 and with_grad.requires_grad
    assert (fused - with_grad.detach()).abs().max() < 1e-5
    vae.fused_grid = False
    with torch.no_grad():
        generic = vae.calc_model_posterior_mean(x, grid)
    assert len(calls) == 1
    assert (fused - generic).abs().max() < 1e-5
    vae.fused_grid = True
    vae0 = build_text_vae(V, ni, H, nz, dev, params=P, dropout_in=0.0, dropout_out=0.0)    # train mode without dropout
    with torch.no_grad():
        vae0.eval_log_model_posterior(x, grid)
    assert len(calls) == 2


def _check_device_mismatch(dev, other, lib, monkeypatch):
    """A grid on another device than the sentences never reaches the kernels (they take raw pointers): the drop-in methods keep
    the generic route (and its error), the engine entries refuse before any launch."""
    from vae_lagging_encoder_amd import _lib
    V, ni, H, nz, B, T = 31, 6, 12, 1, 2, 5
    P, vae = _model(V, ni, H, nz, dev, 9)
    x = _batch(B, T, V, 10).to(dev)
    grid = _grid(-2, 2, 0.5, 1)
    reached = []

    def refuse(*a):
        reached.append(1)
        raise AssertionError("a kernel was launched with operands on different devices")
    monkeypatch.setattr(lib, "lv_dec_cond_ll_f32", refuse, raising=False)
    monkeypatch.setattr(lib, "lv_grid_posterior_f32", refuse, raising=False)
    with torch.no_grad():
        assert vae._fused_grid_ok(x, grid.to(dev))
        assert not vae._fused_grid_ok(x, grid.to(other))
        with pytest.raises(_lib.LvaeError):
            vae.decoder._hip.cond_ll(x, grid.to(other))
        with pytest.raises(_lib.LvaeError):
            E.grid_posterior(torch.zeros(B, grid.shape[0], device=dev), grid.to(other))
        with pytest.raises(_lib.LvaeError):
            E.grid_posterior(torch.zeros(B, grid.shape[0], device=other), grid.to(dev))
    assert reached == []


# ---- MI355X ---------------------------------------------------------------------------------------------------------------
TOY = (1004, 50, 50, 1)


@pytest.mark.gpu
def test_toy_shape_default_grid_against_oracle_existing_path_and_reruns(hip_device):
    V, ni, H, nz = TOY
    B, T = 50, 12
    grid = _grid(-20, 20, 0.1, 1)
    assert grid.shape[0] == 400
    P, vae = _model(V, ni, H, nz, hip_device, 3)
    x = _batch(B, T, V, 4)
    xd, gd = x.to(hip_device), grid.to(hip_device)
    eng = vae.decoder._hip
    got = eng.cond_ll(xd, gd)
    ref = _oracle_cond_ll(P, x, grid)
    assert rel_err(got, ref) < 1e-4
    # the existing HIP route (f32 configuration): the grid expanded to [B][K][nz] through reconstruct_error
    generic = vae.decoder.log_probability(xd, gd.unsqueeze(0).expand(B, *gd.shape).contiguous())
    assert rel_err(got, generic) < 1e-5
    # bit-identical reruns (fixed-order sums, no atomics)
    for _ in range(3):
        assert torch.equal(eng.cond_ll(xd, gd), got)
    lp, mean = E.grid_posterior(got, gd)
    ref_lp, ref_mean = _oracle_posterior(ref, grid)
    mass = ref_lp.exp() > 1e-6
    assert (lp.cpu().double() - ref_lp).abs()[mass].max() < 1e-4
    assert (mean.cpu().double() - ref_mean).abs().max() < 1e-4
    lp2, mean2 = E.grid_posterior(got, gd)
    assert torch.equal(lp2, lp) and torch.equal(mean2, mean)
    # the drop-in methods against the forced existing path
    with torch.no_grad():
        a = vae.calc_model_posterior_mean(xd, gd)
        vae.fused_grid = False
        b = vae.calc_model_posterior_mean(xd, gd)
    assert (a - b).abs().max() < 1e-4


@pytest.mark.gpu
def test_nz2_40x40_grid_against_oracle(hip_device):
    V, ni, H, nz = 1004, 50, 50, 2
    B, T = 6, 10
    grid = _grid(-2, 2, 0.1, 2)
    assert grid.shape[0] == 1600
    P, vae = _model(V, ni, H, nz, hip_device, 5)
    x = _batch(B, T, V, 6)
    got = vae.decoder._hip.cond_ll(x.to(hip_device), grid.to(hip_device))
    ref = _oracle_cond_ll(P, x, grid)
    assert rel_err(got, ref) < 1e-4
    with torch.no_grad():
        lp = vae.eval_log_model_posterior(x.to(hip_device), grid.to(hip_device))
        mean = vae.calc_model_posterior_mean(x.to(hip_device), grid.to(hip_device))
    ref_lp, ref_mean = _oracle_posterior(ref, grid)
    mass = ref_lp.exp() > 1e-6
    assert (lp.cpu().double() - ref_lp).abs()[mass].max() < 1e-4
    assert (mean.cpu().double() - ref_mean).abs().max() < 1e-4


@pytest.mark.gpu
def test_per_sentence_z_and_small_shapes(hip_device):
    _check_cond_ll(hip_device, 41, 6, 20, 2, 5, 5, 37, False, seed=41)
    _check_cond_ll(hip_device, 97, 8, 16, 4, 4, 2, 16, True, seed=97)
    _check_cond_ll(hip_device, 300, 32, 128, 3, 3, 9, 50, True, seed=300)      # the top of the envelope (Hp = 128)


@pytest.mark.gpu
def test_dropin_against_reference_fixture(hip_device):
    _check_dropin_fixture(hip_device)


@pytest.mark.gpu
def test_dropin_routing_train_mode_dropout_keeps_existing_path(hip_device, monkeypatch):
    _check_routing(hip_device, monkeypatch)


@pytest.mark.gpu
def test_grid_on_the_host_never_reaches_the_kernels(hip_device, monkeypatch):
    from vae_lagging_encoder_amd import _lib
    _check_device_mismatch(hip_device, "cpu", _lib.load(), monkeypatch)

"""The order in which VAE.nll_ais draws its random numbers, on every route: z0 = randn(B, C, nz) first, then per launch chunk of
iters_per_launch iterations one randn(n, B, C, nz) (eps / momenta) followed by one rand(n, B, C) (u).  A seeded call must
therefore give, bit for bit, what the same call gives with those draws made here and injected as `noise`.

Shapes: H = 12 pads to one 16-column block and 3 chains of a 16-chain tile are in use; 7 iterations in chunks of 3 are a full
chunk, a chunk boundary inside the look-ahead (iteration 2 needs eps[3], the first of the next chunk) and a ragged last chunk
of 1.  There is no tolerance: both calls run the same launches on the same numbers."""
import pytest
import torch

from helpers import build_vae
from oracle import text_vae_oracle as O
from vae_lagging_encoder_amd import engine as E

V, NI, H, NZ, B, T, C = 11, 4, 12, 3, 2, 5, 3
TEMPS, PER, SEED = 7, 3, 1234
CHUNKS = (3, 3, 1)

ROUTES = {
    "chain": (dict(), dict(std=0.3)),
    "step": (dict(fused_ais=False), dict(std=0.3)),
    "hmc-fused": (dict(), dict(transition="hmc", leapfrog=2, step_size=0.3)),
    "hmc-generic": (dict(fused_hmc=False), dict(transition="hmc", leapfrog=2, step_size=0.3)),
}


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


def _injected(dev):
    gen = torch.Generator(device=dev).manual_seed(SEED)
    z0 = torch.randn(B, C, NZ, device=dev, generator=gen)
    step, u = [], []
    for n in CHUNKS:
        step.append(torch.randn(n, B, C, NZ, device=dev, generator=gen))
        u.append(torch.rand(n, B, C, device=dev, generator=gen))
    return z0, torch.cat(step), torch.cat(u)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_seeded_nll_ais_draws_z0_then_per_chunk_randn_then_rand(target, route):
    _, dev = target
    assert sum(CHUNKS) == TEMPS and all(n <= PER for n in CHUNKS)
    switches, kw = ROUTES[route]
    vae = build_vae(V, NI, H, NZ, dev, params=O.random_params(V, NI, H, NZ, seed=5, scale=0.3, emb_scale=0.5))
    vae.eval()
    for k, v in switches.items():
        setattr(vae, k, v)
    x = O.synthetic_batch(B, T, V, seed=6).to(dev)
    kw = dict(kw, chains=C, temps=TEMPS, iters_per_launch=PER, init="prior", return_info=True)
    nll_s, info_s = vae.nll_ais(x, generator=torch.Generator(device=dev).manual_seed(SEED), **kw)
    nll_n, info_n = vae.nll_ais(x, noise=_injected(dev), **kw)
    assert info_s["route"] == route and info_n["route"] == route
    pairs = [("nll", nll_s, nll_n)] + [(k, info_s[k], info_n[k]) for k in ("logw", "ratios", "accepts", "logw_trace")]
    for name, a, b in pairs:
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(_bits(a), _bits(b)), name
    assert tuple(info_s["ratios"].shape) == (TEMPS, B, C) and bool(torch.isfinite(nll_s).all())

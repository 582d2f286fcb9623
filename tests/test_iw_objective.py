"""Training on the importance-weighted bound (AggressiveTextTrainer(objective="iw"), VAE.loss_iw): the kernels of csrc/lv_iw.hip and
lv_enc_head_iw_bwd_f32 against float64 statements, the fused step against fixtures produced by the reference's own
`vae.nll_iw(x, ns, ns).mean().backward()` (tests/golden/make_golden_iw.py), the drop-in route against the fused one and against torch
autograd, device-drawn noise, the fences and the wiring of the loops.  Emulator (`not gpu`) and MI355X (`gpu`)."""
import argparse
import json
import math

import numpy as np
import pytest
import torch

from helpers import ALL_KEYS, DEC_KEYS, ENC_KEYS, build_vae, load, rel_err
from oracle import text_vae_oracle as O
from parity_common import GRAD_RTOL, RTOL
from vae_lagging_encoder_amd import engine as _eng
from vae_lagging_encoder_amd.engine import P

ULP1 = 2.0 ** -23                     # one unit in the last place of 1.0f


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def target(request):
    if request.param == "emu":
        request.getfixturevalue("emu_backend")
        dev = torch.device("cpu")
    else:
        dev = request.getfixturevalue("hip_device")
    return _eng.backend_for(dev), dev


def _trainer(*a, **k):
    from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer
    return AggressiveTextTrainer(*a, **k)


def _dev_noise(noise, dev):
    e, a, b = noise
    return e.to(dev), a.to(torch.uint8).to(dev), b.to(torch.uint8).to(dev)


# ---------------------------------------------------------------------------------------------------------------------
# 1. lv_loss_assemble_iw_f32 / lv_loss_assemble_iw_rng_f32 against the float64 statement
SHAPES = [(1, 1, 1, 1), (6, 5, 2, 4), (70, 3, 3, 32), (11, 17, 4, 2), (130, 2, 5, 32), (3, 2, 70, 8)]        # T, B, ns, nz


def _latents(B, ns, nz, g, scale=0.3):
    mulv = torch.randn(B, 2 * nz, generator=g) * scale
    eps = torch.randn(B, ns, nz, generator=g)
    z = mulv[:, None, :nz] + eps * torch.exp(0.5 * mulv[:, None, nz:])          # f32, as the head forward hands it over
    return mulv, eps, z


def _statement(nll, mulv, eps, z, beta, ns):
    """float64: log w [B][ns], loss [B], wn [B][ns], rec [B] from (mulv, eps, nll); z is the kernel's own f32 input."""
    T = nll.shape[0]
    B, nz = mulv.shape[0], mulv.shape[1] // 2
    rec_s = nll.double().view(T, B, ns).sum(0)
    lv = mulv[:, nz:].double()
    logw = -rec_s - beta * (0.5 * z.double().pow(2).sum(-1) - 0.5 * eps.double().pow(2).sum(-1) - 0.5 * lv.sum(-1, keepdim=True))
    loss = -(torch.logsumexp(logw, dim=1) - math.log(ns))
    return logw, loss, torch.softmax(logw, dim=1), rec_s.mean(1)


def _assemble(lib, dev, nll, mulv, eps, z, kl, klw, gl, acc, T, B, ns, nz, rng_state=None, inc=0, want_logw=True):
    """One launch on NaN-filled outputs -> dict of host tensors."""
    s = _eng.stream_ptr(dev)
    d = {k: v.clone().to(dev) for k, v in dict(nll=nll, mulv=mulv, eps=eps, z=z, kl=kl, klw=klw, gl=gl, acc=acc).items()}
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
    o = dict(loss=nan(B), rec=nan(B), rowscale=nan(B * ns), wz=nan(B, ns), logw=nan(B, ns) if want_logw else None)
    a = (P(d["nll"]), P(d["mulv"]), P(d["eps"]), P(d["z"]), P(d["kl"]), P(d["klw"]), P(d["gl"]), P(o["loss"]), P(o["rec"]),
         P(o["rowscale"]), P(o["wz"]), P(o["logw"]) if want_logw else None, P(d["acc"]), T, B, ns, nz)
    if rng_state is not None:
        lib.lv_loss_assemble_iw_rng_f32(*a, P(rng_state), inc, s)
    else:
        lib.lv_loss_assemble_iw_f32(*a, s)
    out = {k: v.cpu() for k, v in o.items() if v is not None}
    out["acc"] = d["acc"].cpu()
    return out


@pytest.mark.parametrize("beta", [1.0, 0.37, 0.0])
@pytest.mark.parametrize("T,B,ns,nz", SHAPES)
def test_loss_assemble_iw(target, T, B, ns, nz, beta):
    lib, dev = target
    g = torch.Generator().manual_seed(T + 31 * B + ns + 7 * nz)
    nll = torch.rand(T, B * ns, generator=g) * 5
    mulv, eps, z = _latents(B, ns, nz, g)
    kl = torch.rand(B, generator=g)
    klw = torch.tensor([beta])
    acc0 = torch.tensor([1.5, -2.0, 0.25])
    # seeds that are powers of two: g * wn is then exact and wn can be read back from rowscale without a rounding
    gl2 = torch.tensor([2.0 ** -(1 + b % 5) for b in range(B)])
    gl = torch.rand(B, generator=g) / B
    logw64, loss64, wn64, rec64 = _statement(nll, mulv, eps, z, float(klw[0]), ns)
    r = _assemble(lib, dev, nll, mulv, eps, z, kl, klw, gl2, acc0, T, B, ns, nz)
    for k, v in r.items():
        assert torch.isfinite(v).all(), k                                  # every NaN of the pre-fill was overwritten
    print("T %d B %d ns %d nz %d beta %.2f: rec %.1e loss %.1e" % (T, B, ns, nz, beta, rel_err(r["rec"], rec64), rel_err(r["loss"], loss64)))
    assert rel_err(r["rec"], rec64) < 1e-6 and rel_err(r["loss"], loss64) < 1e-6                       # test_loss_assemble_ns's bound
    want_acc = acc0.double() + torch.stack([loss64.sum(), rec64.sum(), kl.double().sum()])
    assert rel_err(r["acc"], want_acc) < 1e-6
    # log w at the same relative bound, as an absolute figure: delta
    delta = 1e-6 * float(logw64.abs().max())
    assert float((r["logw"].double() - logw64).abs().max()) <= delta
    # wn = softmax_s(log w).  If every log w_s is off by at most delta, exp(log w_s) is off by a factor within e^(+-delta), and so
    # is the sum in the denominator (a sum of positive terms each within that factor): the quotient moves by a factor within
    # e^(+-2 delta), |d wn| <= (e^(2 delta) - 1) wn ~ 2 delta wn.  The kernel's own roundings (expf, the f32 sum, one division) are
    # relative to wn <= 1: one ulp of 1.0 covers them.
    wn = r["rowscale"].view(B, ns) / gl2[:, None]                          # exact: a division by a power of two
    assert bool(((wn.double() - wn64).abs() <= 2 * delta * wn64 + ULP1).all()), float((wn.double() - wn64).abs().max())
    assert float((wn.double().sum(1) - 1).abs().max()) <= 2 * ULP1         # the normaliser is summed in double and rounded once
    assert torch.equal(r["wz"], klw * r["rowscale"].view(B, ns))           # c_s = beta * (g * wn_s), one f32 product
    if ns == 1:
        assert bool((wn == 1).all())
    # arbitrary seeds: rowscale == g * wn, bit for bit; ns == 1: rowscale == g_loss
    r2 = _assemble(lib, dev, nll, mulv, eps, z, kl, klw, gl, acc0, T, B, ns, nz, want_logw=False)
    assert torch.equal(r2["rowscale"].view(B, ns), gl[:, None] * wn)
    assert torch.equal(r2["wz"], klw * r2["rowscale"].view(B, ns))
    if ns == 1:
        assert torch.equal(r2["rowscale"], gl)
    for k in ("loss", "rec", "acc"):
        assert torch.equal(r2[k], r[k]), k
    # the rng twin: the same bits, and only the offset word of the Philox state moves
    state = torch.tensor([12345, 7], dtype=torch.int64, device=dev)
    r3 = _assemble(lib, dev, nll, mulv, eps, z, kl, klw, gl, acc0, T, B, ns, nz, rng_state=state, inc=3, want_logw=False)
    assert state.cpu().tolist() == [12345, 10]
    for k in r2:
        assert torch.equal(r3[k], r2[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 2. weights 200 nats apart
def test_loss_assemble_iw_far_apart_weights(target):
    lib, dev = target
    T, B, ns, nz = 4, 3, 3, 4
    g = torch.Generator().manual_seed(5)
    base = torch.rand(T, B, 1, generator=g) * 5
    step = torch.tensor([[0.0, 50.0, 100.0], [50.0, 0.0, 75.0], [0.0, 0.125, 50.0]])       # per timestep: x T = 200 / 300 / 400 nats
    nll = (base + step[None]).reshape(T, B * ns)
    mulv, eps, z = _latents(B, ns, nz, g)
    kl = torch.rand(B, generator=g)
    klw = torch.tensor([1.0])
    gl2 = torch.full((B,), 0.25)
    r = _assemble(lib, dev, nll, mulv, eps, z, kl, klw, gl2, torch.zeros(3), T, B, ns, nz)
    for k, v in r.items():
        assert torch.isfinite(v).all(), k
    logw64, loss64, wn64, _ = _statement(nll, mulv, eps, z, 1.0, ns)
    wn = r["rowscale"].view(B, ns) / 0.25
    far = (logw64.max(1, keepdim=True).values - logw64) > 150              # exp(-150) is below the smallest f32 subnormal
    assert int(far.sum()) == 5 and bool((wn[far] == 0).all()) and bool((r["wz"][far] == 0).all())
    assert abs(float(wn[0, 0]) - 1) <= ULP1 and abs(float(wn[1, 1]) - 1) <= ULP1         # a lone dominant weight is 1
    assert bool(((wn.double() - wn64).abs() <= 2e-6 * float(logw64.abs().max()) * wn64 + ULP1).all())
    assert rel_err(r["loss"], loss64) < 1e-6
    lone = -logw64.max(1).values[:2] + math.log(ns)                        # loss = -log w_max + log ns where one weight is alone
    assert rel_err(r["loss"][:2], lone) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# 3. the two backward kernels against float64
def _head_case(B, ns, nz, H, parts, seed):
    g = torch.Generator().manual_seed(seed)
    mulv, eps, _ = _latents(B, ns, nz, g, scale=0.5)
    dz = torch.randn(B, ns, nz, generator=g)
    frac = torch.rand(parts, generator=g) + 0.1
    frac = frac / frac.sum()
    dzp = (frac[:, None, None, None] * dz[None]).contiguous()              # partial sums of one sign per element: no cancellation
    wz = torch.rand(B, ns, generator=g) / ns
    hT = torch.randn(B, H, generator=g)
    wlin = torch.randn(2 * nz, H, generator=g) * 0.3
    return mulv, eps, dzp, wz, hT, wlin


def _head_statement(mulv, eps, dzp, wz, hT, wlin):
    nz = mulv.shape[1] // 2
    mu, lv = mulv[:, None, :nz].double(), mulv[:, None, nz:].double()
    sd = torch.exp(0.5 * lv)
    e = eps.double()
    t = dzp.double().sum(0) + wz.double()[:, :, None] * (mu + e * sd)
    dmulv = torch.cat((t.sum(1), (t * 0.5 * e * sd).sum(1) - 0.5 * wz.double().sum(1, keepdim=True)), dim=1)
    return dmulv, dmulv @ wlin.double(), dmulv.t() @ hT.double()


def _run_head(lib, dev, name, mulv, eps, dzp, seed4, hT, wlin):
    B, ns, nz = eps.shape
    H = hT.shape[1]
    d = [t.to(dev) for t in (mulv, eps, dzp, seed4, hT, wlin)]
    out = [torch.full(shape, float("nan"), device=dev) for shape in ((B, 2 * nz), (B, H), (2 * nz, H))]
    getattr(lib, name)(P(d[0]), P(d[1]), P(d[2]), dzp.shape[0], P(d[3]), P(d[4]), P(d[5]), P(out[0]), P(out[1]), P(out[2]), B, H, ns, nz,
                       _eng.stream_ptr(dev))
    return [o.cpu() for o in out]


HEAD_SHAPES = [(1, 1, 1), (5, 2, 4), (3, 3, 32), (17, 4, 2), (2, 5, 32), (2, 70, 8)]               # B, ns, nz


@pytest.mark.parametrize("B,ns,nz", HEAD_SHAPES)
def test_iw_backward_kernels(target, B, ns, nz):
    lib, dev = target
    s = _eng.stream_ptr(dev)
    # H = 1024 (64 workgroups, 80 partial sums of dz) on the GPU only: the thread-level emulator would spend its time there
    for H, parts in [(16, 1), (16, lib.lv_dec_tail_parts(16))] + ([(1024, 1), (1024, lib.lv_dec_tail_parts(1024))] if dev.type == "cuda" else []):
        mulv, eps, dzp, wz, hT, wlin = _head_case(B, ns, nz, H, parts, seed=B * 100 + ns * 10 + nz + parts)
        dmulv64, dhT64, gW64 = _head_statement(mulv, eps, dzp, wz, hT, wlin)
        dmulv, dhT, gW = _run_head(lib, dev, "lv_enc_head_iw_bwd_f32", mulv, eps, dzp, wz, hT, wlin)
        # the bounds tests/test_gpu_kernels.py holds lv_reparam_kl_bwd_f32 / lv_enc_head_bwd_f32 to
        assert float((dmulv.double() - dmulv64).abs().max()) < 1e-5 * (1 + float(dmulv64.abs().max())), parts
        assert float((dhT.double() - dhT64).abs().max()) < 2e-5 * float(dhT64.abs().max()), parts
        assert float((gW.double() - gW64).abs().max()) < 2e-5 * float(gW64.abs().max()), parts
        # wz all zeros: the bits of lv_enc_head_bwd_f32 with dkl all zeros
        a = _run_head(lib, dev, "lv_enc_head_iw_bwd_f32", mulv, eps, dzp, torch.zeros(B, ns), hT, wlin)
        b = _run_head(lib, dev, "lv_enc_head_bwd_f32", mulv, eps, dzp, torch.zeros(B), hT, wlin)
        for x, y, k in zip(a, b, ("dmulv", "dhT", "gW_lin")):
            assert torch.equal(x, y), (k, parts)
    # the direct terms alone (autograd route): the same statement with dz = 0
    direct64 = _head_statement(mulv, eps, torch.zeros_like(dzp), wz, hT, wlin)[0]
    d = [t.to(dev) for t in (mulv, eps, wz)]
    out = torch.full((B, 2 * nz), float("nan"), device=dev)
    lib.lv_reparam_iw_bwd_f32(P(d[0]), P(d[1]), P(d[2]), P(out), B, ns, nz, s)
    assert float((out.cpu().double() - direct64).abs().max()) < 1e-5 * (1 + float(direct64.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------
# 4. refusals
def test_iw_kernels_refuse_bad_arguments(target):
    lib, dev = target
    t = torch.full((64,), 7.0, device=dev)
    raw = lambda name: getattr(lib, "_raw_" + name)
    a = [P(t)] * 13
    for name, tail in (("lv_loss_assemble_iw_f32", (None,)), ("lv_loss_assemble_iw_rng_f32", (P(t), 1, None))):
        for i in range(13):
            if i == 11:
                continue                                                   # logw may be NULL
            bad = list(a)
            bad[i] = None
            assert raw(name)(*bad, 1, 1, 1, 1, *tail) < 0, (name, i)
        for sizes in ((-1, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, -3, 1, 1)):
            assert raw(name)(*a, *sizes, *tail) < 0, (name, sizes)
    assert raw("lv_loss_assemble_iw_rng_f32")(*a, 1, 1, 1, 1, None, 1, None) < 0                   # no rng state
    for i in range(4):
        bad = [P(t)] * 4
        bad[i] = None
        assert raw("lv_reparam_iw_bwd_f32")(*bad, 1, 1, 1, None) < 0
    for sizes in ((0, 1, 1), (1, 0, 1), (1, 1, 0)):
        assert raw("lv_reparam_iw_bwd_f32")(*[P(t)] * 4, *sizes, None) < 0
    h = lambda ptrs, parts, sizes: raw("lv_enc_head_iw_bwd_f32")(ptrs[0], ptrs[1], ptrs[2], parts, *ptrs[3:], *sizes, None)
    for i in range(9):
        bad = [P(t)] * 9
        bad[i] = None
        assert h(bad, 1, (1, 1, 1, 1)) < 0, i
    for parts, sizes in ((0, (1, 1, 1, 1)), (1, (0, 1, 1, 1)), (1, (1, 0, 1, 1)), (1, (1, 1, 0, 1)), (1, (1, 1, 1, 0))):
        assert h([P(t)] * 9, parts, sizes) < 0, (parts, sizes)
    assert bool((t.cpu() == 7.0).all())                                    # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# 5. the fused step, exact-f32 configuration, against the reference fixtures
def _case(fx, tag):
    pre = tag + "/"
    return {k[len(pre):]: fx[k] for k in fx.files if k.startswith(pre)}


def _case_params(c, prefix="param/"):
    return {k: torch.from_numpy(c[prefix + k]) for k in ALL_KEYS}


def _pair_delta(got, want):
    """largest error of a within-sentence difference log w_s - log w_s'"""
    d = torch.as_tensor(got).detach().double().cpu() - torch.as_tensor(want).double()
    return float((d.unsqueeze(2) - d.unsqueeze(1)).abs().max())


CASES = ["ns2_wide_clip", "ns3_T2", "ns4_mid", "ns4_refinit", "ns1"]


@pytest.mark.parametrize("tag", CASES)
def test_fused_iw_step_matches_reference_fixture(target, tag):
    """One encoder step of AggressiveTextTrainer(nsamples=ns, objective="iw") against the reference's
    nll_iw(x, ns, ns).mean().backward() + clip_grad_norm_ + SGD: the quantities and bounds of
    test_multisample.py::test_fused_step_matches_reference_fixture, plus log w.  The self-normalised weights turn an absolute error
    in rec into a relative error of the gradient: its bound is GRAD_RTOL + 2 * delta with delta the measured error of a
    within-sentence difference of log w, and delta itself is capped by the rec bound, RTOL * max|rec|."""
    _, dev = target
    c = _case(load("text_iw_small"), tag)
    V, ni, H, nz, B, T, ns = (int(c[k]) for k in ("V", "ni", "H", "nz", "B", "T", "ns"))
    vae = build_vae(V, ni, H, nz, dev, params=_case_params(c))
    tr = _trainer(vae, lr=1.0, clip=float(c["max_norm"]), nsamples=ns, objective="iw")
    x = torch.from_numpy(c["x"]).to(dev)
    noise = tuple(torch.from_numpy(c[k]).to(dev) for k in ("eps", "mask_in", "mask_out"))
    assert tuple(noise[0].shape) == (B, ns, nz) and tuple(noise[1].shape) == (B, T - 1, ni) and tuple(noise[2].shape) == (B * ns, T - 1, H)
    tr.step(x, float(c["kl_weight"]), noise=noise)
    stt = tr.read_stats()
    st = tr.static[(B, T)]
    rec_scale = float(np.abs(c["rec"]).max())
    delta = _pair_delta(st.logw, c["logw"])
    print(tag, "loss %.1e rec %.1e logw %.1e delta %.1e" % (rel_err(st.loss, c["loss"]), rel_err(st.rec, c["rec"]),
                                                          float((st.logw.cpu().double() - torch.from_numpy(c["logw"]).double()).abs().max()), delta))
    assert rel_err(st.loss, c["loss"]) < RTOL and rel_err(st.rec, c["rec"]) < RTOL
    assert rel_err(st.logw, c["logw"]) < RTOL and delta < RTOL * rec_scale
    kl_err = float(np.abs(st.kl.cpu().numpy() - c["kl"]).max())
    assert kl_err < RTOL * float(np.abs(c["kl"]).max()) + 1e-6 * (1 + rec_scale), ("kl", kl_err)
    assert abs(stt["loss_sum"] - float(c["loss"].sum())) < RTOL * abs(float(c["loss"].sum()))
    assert abs(stt["rec_sum"] - float(c["rec"].sum())) < RTOL * abs(float(c["rec"].sum()))
    assert abs(stt["kl_sum"] - float(c["kl"].sum())) < RTOL * abs(float(c["kl"].sum())) + 1e-6 * B * (1 + rec_scale)
    assert abs(stt["norm"] - float(c["total_norm"])) < RTOL * float(c["total_norm"])
    assert abs(stt["coef"] - float(c["coef"])) < RTOL
    if tag == "ns2_wide_clip":
        assert stt["coef"] < 0.99                              # the clip is active in this case
    named = dict(vae.named_parameters())
    worst = 0.0
    for k in ALL_KEYS:                                          # .grad holds the CLIPPED gradient, as clip_grad_norm_ leaves it
        g = c["grad/" + k] * float(c["coef"])
        if np.abs(g).max() > 0:
            worst = max(worst, rel_err(named[k].grad, g))
            assert rel_err(named[k].grad, g) < GRAD_RTOL + 2 * delta, (k, rel_err(named[k].grad, g))
        else:
            assert float(named[k].grad.abs().max()) == 0.0, k
    print(tag, "gradients %.1e" % worst)
    sd = vae.state_dict()
    for k in ENC_KEYS:
        assert rel_err(sd[k], c["new/" + k]) < RTOL, k
    for k in DEC_KEYS:                                          # an encoder step leaves the decoder untouched, bit for bit
        assert torch.equal(sd[k].cpu(), torch.from_numpy(c["param/" + k])), k


def test_fused_iw_trajectory_matches_reference_fixture(target):
    """Three consecutive steps (encoder, encoder, both), each on the weights the previous one left."""
    _, dev = target
    c = _case(load("text_iw_small"), "traj_ns2")
    V, ni, H, nz, B, T, ns = (int(c[k]) for k in ("V", "ni", "H", "nz", "B", "T", "ns"))
    vae = build_vae(V, ni, H, nz, dev, params=_case_params(c))
    tr = _trainer(vae, lr=1.0, clip=float(c["max_norm"]), nsamples=ns, objective="iw")
    assert [str(u) for u in c["updates"]] == ["encoder", "encoder", "both"]
    for it, up in enumerate(c["updates"]):
        noise = tuple(torch.from_numpy(c[k][it]).to(dev) for k in ("eps", "mask_in", "mask_out"))
        tr.reset_stats()
        tr.step(torch.from_numpy(c["x"][it]).to(dev), float(c["kl_weight"]), noise=noise, update=str(up))
        st = tr.read_stats()
        rec_scale = float(np.abs(c["rec"][it]).max())
        assert _pair_delta(tr.static[(B, T)].logw, c["logw"][it]) < RTOL * rec_scale
        assert abs(st["loss_sum"] - float(c["loss"][it].sum())) < RTOL * abs(float(c["loss"][it].sum()))
        assert abs(st["rec_sum"] - float(c["rec"][it].sum())) < RTOL * abs(float(c["rec"][it].sum()))
        assert abs(st["kl_sum"] - float(c["kl"][it].sum())) < RTOL * abs(float(c["kl"][it].sum())) + 1e-6 * (1 + rec_scale)
        assert abs(st["norm"] - float(c["total_norm"][it])) < RTOL * float(c["total_norm"][it])
    sd = vae.state_dict()
    for k in ALL_KEYS:
        assert rel_err(sd[k], c["final/" + k]) < RTOL, k


# ---------------------------------------------------------------------------------------------------------------------
# 6. the wide fixture (H = 1024, V = 20001) on the GPU
WIDE = "text_iw_h1024_b8_t50"


def _wide(dev):
    from test_gpu_parity import _seeded_full_size_vae
    fx = load(WIDE)
    vae = _seeded_full_size_vae(fx, dev)
    x = torch.from_numpy(fx["x"]).to(dev)
    unpack = lambda k: torch.from_numpy(np.unpackbits(fx[k + "_bits"])[:int(np.prod(fx[k + "_shape"]))].reshape(tuple(fx[k + "_shape"])))
    noise = (torch.from_numpy(fx["eps"]).to(dev), unpack("mask_in").to(dev), unpack("mask_out").to(dev))
    return fx, vae, x, noise


@pytest.mark.gpu
def test_wide_iw_fixture_f32(hip_device):
    """test_multisample.py::test_wide_fixture_f32's bounds; delta capped by that test's rec bound."""
    fx, vae, x, noise = _wide(hip_device)
    B, T, ns = int(fx["B"]), int(fx["T"]), int(fx["ns"])
    tr = _trainer(vae, lr=1.0, clip=5.0, nsamples=ns, objective="iw")
    tr.step(x, float(fx["kl_weight"]), noise=noise)
    stt = tr.read_stats()
    st = tr.static[(B, T)]
    delta = _pair_delta(st.logw, fx["logw"])
    print(WIDE, "f32: loss %.2e rec %.2e kl %.2e delta %.2e norm %.2e" % (rel_err(st.loss, fx["loss"]), rel_err(st.rec, fx["rec"]),
          rel_err(st.kl, fx["kl"]), delta, abs(stt["norm"] - float(fx["total_norm64"])) / float(fx["total_norm64"])))
    assert rel_err(st.loss, fx["loss"]) < 1e-4 and rel_err(st.rec, fx["rec"]) < 1e-4 and rel_err(st.kl, fx["kl"]) < 1e-4
    assert delta < 1e-4 * float(np.abs(fx["rec"]).max())
    coef = min(1.0, 5.0 / (float(fx["total_norm64"]) + 1e-6))
    named = dict(vae.named_parameters())
    for k in ALL_KEYS:
        ref_n = float(fx["gradnorm/" + k]) * coef
        assert abs(float(named[k].grad.double().norm()) - ref_n) / ref_n < GRAD_RTOL + 2 * delta, k


@pytest.mark.gpu
def test_wide_iw_fixture_bf16(hip_device):
    """The throughput configuration against the reference run at test_multisample.py::test_wide_fixture_bf16's bounds, the gradient
    ones with + 2 * delta; delta (measured: the error of a within-sentence difference of log w) is capped by that test's own rec
    bound, 1e-4 * max|rec|."""
    fx, vae, x, noise = _wide(hip_device)
    p0 = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    B, T, V, ns = int(fx["B"]), int(fx["T"]), int(fx["V"]), int(fx["ns"])
    tr = _trainer(vae, lr=1.0, clip=5.0, precision="bf16", nsamples=ns, objective="iw")
    tr.step(x, float(fx["kl_weight"]), noise=noise)
    st = tr.read_stats()
    delta = _pair_delta(tr.static[(B, T)].logw, fx["logw"])
    out = {"delta": delta, "delta_cap": 1e-4 * float(np.abs(fx["rec"]).max())}
    base = B * (T - 1) * math.log(V)
    out["loss_rel"] = abs(st["loss_sum"] - float(fx["loss"].sum())) / abs(float(fx["loss"].sum()))
    out["rec_rel"] = abs(st["rec_sum"] - float(fx["rec"].sum())) / abs(float(fx["rec"].sum()))
    out["rec_excess_rel"] = abs(st["rec_sum"] - float(fx["rec"].sum())) / abs(float(fx["rec"].sum()) - base)
    out["kl_rel"] = abs(st["kl_sum"] - float(fx["kl"].sum())) / abs(float(fx["kl"].sum()))
    out["norm_rel"] = abs(st["norm"] - float(fx["total_norm64"])) / float(fx["total_norm64"])
    coef = min(1.0, 5.0 / (float(fx["total_norm64"]) + 1e-6))
    named = dict(vae.named_parameters())
    gn, gs = {}, {}
    for k in ALL_KEYS:
        g = named[k].grad
        ref_n = float(fx["gradnorm/" + k]) * coef
        gn[k] = abs(float(g.double().norm()) - ref_n) / ref_n
        idx = torch.from_numpy(fx["sample_idx/" + k]).to(hip_device)
        rms = ref_n / max(1.0, g.numel() ** 0.5)
        gs[k] = float((g.reshape(-1)[idx].cpu() - torch.from_numpy(fx["sample_grad/" + k]) * coef).abs().max()) / rms
    out["gradnorm_rel_max"], out["grad_sample_err_over_rms_max"] = max(gn.values()), max(gs.values())
    upd = {}
    coef_ref = min(1.0, 5.0 / (float(fx["total_norm"]) + 1e-6))
    for k in ENC_KEYS:
        idx = torch.from_numpy(fx["sample_idx/" + k]).to(hip_device)
        q0 = torch.from_numpy(fx["sample_param/" + k])
        u_ref = (torch.from_numpy(fx["sample_new/" + k]) - q0) / coef_ref
        u_got = (vae.state_dict()[k].reshape(-1)[idx].cpu() - q0) / min(1.0, 5.0 / (st["norm"] + 1e-6))
        upd[k] = float((u_got - u_ref).abs().max()) / (float(u_ref.abs().max()) + 1e-30)
    out["enc_update_rel_max"] = max(upd.values())
    for k in DEC_KEYS:
        assert torch.equal(vae.state_dict()[k], p0[k]), k
    print(WIDE + " bf16:", json.dumps(out))
    assert out["loss_rel"] < 1e-4 and out["rec_rel"] < 1e-4 and out["kl_rel"] < 1e-4, out
    assert out["delta"] < out["delta_cap"], out
    assert out["norm_rel"] < 1e-4 + 2 * delta and out["rec_excess_rel"] < 1e-3, out
    assert out["gradnorm_rel_max"] < 2e-3 + 2 * delta, out
    assert out["grad_sample_err_over_rms_max"] < 0.1 + 2 * delta and out["enc_update_rel_max"] < 2e-2 + 2 * delta, out


# ---------------------------------------------------------------------------------------------------------------------
# 7. the drop-in route: VAE.loss_iw against the fused step and against torch autograd
def _autograd_bound(vae, x, beta, ns, noise):
    """-(logsumexp_s(-rec_s - beta (log q - log p)) - log ns) as a torch graph on the device: rec_s from the package's own
    reconstruct_error; log q and log p as torch expressions of (mulv, eps) -- the package's eval_inference_dist / eval_prior_dist are
    forward-only kernels, so they pin the VALUES of the two expressions here and autograd differentiates the expressions."""
    from vae_lagging_encoder_amd.modules.encoders.encoder import _ReparamKLFn
    eps, m_in, m_out = noise
    mulv = vae.encoder._forward_mulv(x)
    nz = mulv.shape[1] // 2
    mu, lv = mulv[:, None, :nz], mulv[:, None, nz:]
    z, _ = _ReparamKLFn.apply(mulv, eps)
    rec_s = vae.decoder.reconstruct_error(x, z, masks=(m_in, m_out))
    zt = mu + eps * torch.exp(0.5 * lv)
    logq = (-0.5 * (zt - mu).pow(2) / lv.exp() - 0.5 * lv - 0.5 * math.log(2 * math.pi)).sum(-1)
    logp = (-0.5 * zt.pow(2) - 0.5 * math.log(2 * math.pi)).sum(-1)
    with torch.no_grad():
        assert rel_err(logq, vae.eval_inference_dist(x, z, (mulv[:, :nz], mulv[:, nz:]))) < 1e-5
        assert rel_err(logp, vae.eval_prior_dist(z)) < 1e-5
    logw = -rec_s - beta * (logq - logp)
    return -(torch.logsumexp(logw, dim=1) - math.log(ns)), logw.detach()


@pytest.mark.parametrize("tag", ["ns4_mid", "ns2_wide_clip"])
def test_loss_iw_equals_fused_step_and_autograd(target, tag):
    from vae_lagging_encoder_amd import optim as lvo
    _, dev = target
    c = _case(load("text_iw_small"), tag)
    V, ni, H, nz, B, T, ns = (int(c[k]) for k in ("V", "ni", "H", "nz", "B", "T", "ns"))
    clip, klw = float(c["max_norm"]), float(c["kl_weight"])
    x = torch.from_numpy(c["x"]).to(dev)
    noise = tuple(torch.from_numpy(c[k]).to(dev) for k in ("eps", "mask_in", "mask_out"))
    b = build_vae(V, ni, H, nz, dev, params=_case_params(c))
    enc_opt = lvo.SGD(b.encoder.parameters(), lr=1.0, momentum=0)
    b.zero_grad()
    loss, rec, kl = b.loss_iw(x, klw, nsamples=ns, noise=noise)
    assert tuple(loss.shape) == tuple(rec.shape) == tuple(kl.shape) == (B,)
    loss.mean(dim=-1).backward()
    raw = {k: p.grad.detach().clone() for k, p in b.named_parameters()}
    total = float(lvo.clip_grad_norm_(b.parameters(), clip))
    enc_opt.step()
    gb = {k: p.grad.detach().clone() for k, p in b.named_parameters()}
    # (a) the fused step on the same tree and noise: same arithmetic, another order
    a = build_vae(V, ni, H, nz, dev, params=_case_params(c))
    tr = _trainer(a, lr=1.0, clip=clip, nsamples=ns, objective="iw")
    tr.step(x, klw, noise=noise)
    st = tr.read_stats()
    s_ = tr.static[(B, T)]
    assert abs(st["norm"] - total) < 1e-5 * total
    assert rel_err(s_.loss, loss) < 1e-5 and rel_err(s_.rec, rec) < 1e-5 and rel_err(s_.kl, kl) < 1e-5
    for k, p in a.named_parameters():
        if float(gb[k].abs().max()) > 0:
            assert rel_err(p.grad, gb[k]) < 1e-5, (k, rel_err(p.grad, gb[k]))
        else:
            assert float(p.grad.abs().max()) == 0.0, k
    sa, sb = a.state_dict(), b.state_dict()
    for k in ENC_KEYS:
        assert rel_err(sa[k], sb[k]) < 1e-5, k
    # (b) torch autograd through the composed bound
    o = build_vae(V, ni, H, nz, dev, params=_case_params(c))
    o.zero_grad()
    lo, logw = _autograd_bound(o, x, klw, ns, noise)
    lo.mean().backward()
    delta = _pair_delta(s_.logw, logw.cpu())
    assert rel_err(loss, lo) < 1e-5 and delta < 1e-5 * float(rec.abs().max())
    for k, p in o.named_parameters():
        if float(raw[k].abs().max()) > 0:
            assert rel_err(raw[k], p.grad) < 1e-5 + 2 * delta, (k, rel_err(raw[k], p.grad))
        else:
            assert float(p.grad.abs().max()) == 0.0, k


# ---------------------------------------------------------------------------------------------------------------------
# 8. the PixelCNN decoder takes the same drop-in route
@pytest.mark.gpu
def test_loss_iw_pixelcnn_smoke(hip_device):
    from parity_common import build_image_vae
    from vae_lagging_encoder_amd.modules.encoders.encoder import _ReparamKLFn
    dev = hip_device
    B, ns, beta = 2, 3, 0.7
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(B, 1, 28, 28, generator=g) < 0.3).float().to(dev)
    grads = {}
    for route in ("loss_iw", "autograd"):
        vae = build_image_vae(dev, 11)
        vae.train()
        nz = vae.nz
        eps = torch.randn(B, ns, nz, generator=torch.Generator().manual_seed(4)).to(dev)
        vae.zero_grad()
        if route == "loss_iw":
            loss, rec, kl = vae.loss_iw(x, beta, nsamples=ns, noise=(eps, None, None))
            assert tuple(loss.shape) == tuple(rec.shape) == tuple(kl.shape) == (B,)
        else:
            mulv = vae.encoder._forward_mulv(x)
            mu, lv = mulv[:, None, :nz], mulv[:, None, nz:]
            z, _ = _ReparamKLFn.apply(mulv, eps)
            rec_s = vae.decoder.reconstruct_error(x, z)
            zt = mu + eps * torch.exp(0.5 * lv)
            logw = -rec_s - beta * ((-0.5 * eps.pow(2) - 0.5 * lv).sum(-1) + 0.5 * zt.pow(2).sum(-1))
            loss = -(torch.logsumexp(logw, dim=1) - math.log(ns))
        loss.mean().backward()
        grads[route] = ({k: p.grad.detach().clone() for k, p in vae.named_parameters()}, loss.detach())
    (ga, la), (gb, lb) = grads["loss_iw"], grads["autograd"]
    assert torch.isfinite(la).all() and rel_err(la, lb) < 1e-4
    for k in ga:
        assert torch.isfinite(ga[k]).all(), k
    # BatchNorm in train mode: both routes normalise with the statistics of the same batch
    worst = max(rel_err(ga[k], gb[k]) for k in ga if float(gb[k].abs().max()) > 0)
    print("pixelcnn loss_iw vs autograd: loss %.1e gradients %.1e" % (rel_err(la, lb), worst))
    assert worst < 1e-3


# ---------------------------------------------------------------------------------------------------------------------
# 9. device-drawn noise
def test_iw_device_drawn_noise(target):
    _, dev = target
    V, ni, H, nz, B, T, ns = 97, 12, 20, 8, 6, 9, 3
    Pm = O.random_params(V, ni, H, nz, seed=6, scale=0.3, emb_scale=0.5, head_scale=0.5)
    x = O.synthetic_batch(B, T, V, seed=3).to(dev)

    def run(seed, objective):
        vae = build_vae(V, ni, H, nz, dev, params=Pm)
        tr = _trainer(vae, lr=0.1, clip=5.0, nsamples=ns, seed=seed, objective=objective)
        for _ in range(2):
            tr.step(x, 0.5)
        stats = tr.read_stats()
        st = tr.static[(B, T)]
        return stats, {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}, st.eps.cpu().clone(), int(tr.rng_state[1].item())

    a, b, other, elbo = run(5, "iw"), run(5, "iw"), run(6, "iw"), run(5, "elbo")
    assert a[0] == b[0] and torch.equal(a[2], b[2])
    for k in ALL_KEYS:
        assert torch.equal(a[1][k], b[1][k]), k
    assert not torch.equal(a[2], other[2]) and a[0]["loss_sum"] != other[0]["loss_sum"]
    assert a[3] == elbo[3] == 2                                 # one Philox offset per step, as the "elbo" step at the same ns
    assert torch.equal(a[2], elbo[2])                           # ... and the same draws


# ---------------------------------------------------------------------------------------------------------------------
# 10. wiring
def test_objective_elbo_is_bit_identical_to_the_default(target):
    _, dev = target
    V, ni, H, nz, B, ns = 97, 12, 20, 4, 6, 2
    Pm = O.random_params(V, ni, H, nz, seed=5, scale=0.3, emb_scale=0.5, head_scale=0.5)
    xs = [O.synthetic_batch(B, T, V, seed=70 + i).to(dev) for i, T in enumerate((5, 8, 6))]
    out = []
    for kw in ({}, {"objective": "elbo"}):
        vae = build_vae(V, ni, H, nz, dev, params=Pm)
        tr = _trainer(vae, lr=1.0, clip=5.0, seed=11, nsamples=ns, **kw)
        assert tr.objective == "elbo"
        sums = []
        for i in range(4):
            x = xs[i % 3]
            noise = _dev_noise(O.draw_noise(B, x.shape[1], ni, H, nz, ns=ns, seed=90 + i), dev) if i % 2 == 0 else None
            tr.step(x, 0.6, noise=noise, update=("encoder", "decoder", "encoder", "both")[i])
            sums.append(tr.read_stats())
        out.append((sums, {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}))
    assert out[0][0] == out[1][0]
    for k in ALL_KEYS:
        assert torch.equal(out[0][1][k], out[1][1][k]), k


def test_iw_fences_and_single_sample(target):
    _, dev = target
    V, ni, H, nz, B, T = 53, 8, 16, 4, 4, 6
    vae = build_vae(V, ni, H, nz, dev, seed=0)
    with pytest.raises(ValueError, match="objective"):
        _trainer(vae, objective="iwae")
    for ns in (1, 2):                                           # "iw" shares the multi-sample route's fences, also with one sample
        for kw in (dict(grad_sync=object()), dict(use_graph=True), dict(micro_batches=2), dict(decoder_grads="norm")):
            with pytest.raises(ValueError, match="nsamples"):
                _trainer(vae, nsamples=ns, objective="iw", **kw)
    vae = build_vae(V, ni, H, nz, dev, params=O.random_params(V, ni, H, nz, seed=2, scale=0.2, emb_scale=0.5, head_scale=0.5))
    tr = _trainer(vae, nsamples=1, objective="iw")
    x = O.synthetic_batch(B, T, V, seed=1).to(dev)
    eps, mi, mo = _dev_noise(O.draw_noise(B, T, ni, H, nz, ns=1, seed=2), dev)
    with pytest.raises(ValueError, match="nsamples"):
        tr.step(x, 0.5, noise=(eps.reshape(B, nz), mi, mo))
    w0 = {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}
    tr.step(x, 0.5, noise=(eps, mi, mo))
    st = tr.read_stats()
    s_ = tr.static[(B, T)]
    assert any(not torch.equal(w0[k], vae.state_dict()[k].cpu()) for k in ENC_KEYS)
    # one sample: the weight is 1, the bound is rec + beta * (log q - log p) at the sample -- not rec + beta * analytic KL
    assert torch.equal(s_.rowscale.cpu(), torch.full((B,), 1.0 / B))
    assert rel_err(s_.loss, -s_.logw[:, 0]) < 1e-6
    gap = (s_.loss - (s_.rec + 0.5 * s_.kl)).abs().cpu()
    print("sampled against analytic KL term, per sentence:", gap.tolist())
    assert float(gap.max()) > 1e-2 and abs(st["kl_sum"] - float(s_.kl.sum())) < 1e-5 * (1 + abs(st["kl_sum"]))


def test_training_loops_honour_objective(target):
    from vae_lagging_encoder_amd.training import TextTrainingLoop
    _, dev = target
    V, ni, H, nz, B, ns = 53, 8, 16, 4, 4, 2
    Pm = O.random_params(V, ni, H, nz, seed=2, scale=0.2, emb_scale=0.5, head_scale=0.5)
    train = [O.synthetic_batch(B, T, V, seed=10 + i).to(dev) for i, T in enumerate((5, 6, 4))]

    def mk_args(**extra):
        return argparse.Namespace(kl_start=0.1, warm_up=1, batch_size=B, epochs=1, aggressive=0, nsamples=ns, test_nepoch=5,
                                  iw_nsamples=20, momentum=0, **extra)

    def noise_fn():
        cnt = {"n": 0}

        def fn(x):
            cnt["n"] += 1
            return _dev_noise(O.draw_noise(x.shape[0], x.shape[1], ni, H, nz, ns=ns, seed=500 + cnt["n"]), dev)
        return fn

    losses = {}
    for name, extra in (("missing", {}), ("elbo", {"objective": "elbo"}), ("iw", {"objective": "iw"})):
        vae = build_vae(V, ni, H, nz, dev, params=Pm)
        loop = TextTrainingLoop(vae, train, train[:2], train[:1], mk_args(**extra), log=lambda *_: None, np_rng=np.random.RandomState(3),
                                noise_fn=noise_fn())
        assert loop.trainer.objective == ("iw" if name == "iw" else "elbo") == loop.objective
        loop.run()
        losses[name] = [r["rec_sum"] for r in loop.iterations]
        order = [r["batch"] for r in loop.iterations]
        klws = [r["kl_weight"] for r in loop.iterations]
    assert losses["missing"] == losses["elbo"] and losses["iw"] != losses["elbo"]
    # the same "iw" steps driven by hand
    vae = build_vae(V, ni, H, nz, dev, params=Pm)
    tr = _trainer(vae, lr=1.0, clip=5.0, nsamples=ns, objective="iw")
    fn = noise_fn()
    hand = []
    for i, w in zip(order, klws):
        tr.reset_stats()
        tr.step(train[i], w, noise=fn(train[i]), update="both")
        hand.append(tr.read_stats()["rec_sum"])
    assert losses["iw"] == hand
    # a trainer built for the other objective is refused, either way round; so is an unknown objective
    vae = build_vae(V, ni, H, nz, dev, params=Pm)
    with pytest.raises(ValueError, match="objective"):
        TextTrainingLoop(vae, train, train[:2], train[:1], mk_args(objective="iw"), trainer=_trainer(vae, nsamples=ns), log=lambda *_: None)
    with pytest.raises(ValueError, match="objective"):
        TextTrainingLoop(vae, train, train[:2], train[:1], mk_args(), trainer=_trainer(vae, nsamples=ns, objective="iw"), log=lambda *_: None)
    with pytest.raises(ValueError, match="objective"):
        TextTrainingLoop(vae, train, train[:2], train[:1], mk_args(objective="iwae"), log=lambda *_: None)


def test_iw_steady_state_allocates_no_new_workspace(target):
    _, dev = target
    V, ni, H, nz, B, ns = 97, 12, 20, 4, 6, 3
    vae = build_vae(V, ni, H, nz, dev, params=O.random_params(V, ni, H, nz, seed=8, scale=0.3, emb_scale=0.5, head_scale=0.3))
    tr = _trainer(vae, lr=0.1, clip=5.0, nsamples=ns, objective="iw")
    batches = [O.synthetic_batch(B, T, V, seed=20 + i).to(dev) for i, T in enumerate((7, 9))]
    tr.prepare_batches(batches)
    for x in batches:                                           # first step of each shape: workspaces are built
        tr.step(x, 0.5)
    tr.commit()
    misses = (tr.enc.wsc.misses, tr.dec.wsc.misses)
    static = {k: (v.wz.data_ptr(), v.logw.data_ptr(), v.rowscale.data_ptr()) for k, v in tr.static.items()}
    cuda = dev.type == "cuda"
    if cuda:
        torch.cuda.synchronize(dev)
        a0 = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    for i in range(10):
        tr.step(batches[i % 2], 0.5)
    if cuda:
        torch.cuda.synchronize(dev)
        grew = torch.cuda.memory_stats(dev)["allocation.all.allocated"] - a0
    tr.commit()
    assert (tr.enc.wsc.misses, tr.dec.wsc.misses) == misses
    assert {k: (v.wz.data_ptr(), v.logw.data_ptr(), v.rowscale.data_ptr()) for k, v in tr.static.items()} == static
    if cuda:
        # the "elbo" trainer at the same shapes is the yardstick: the objective adds no allocation to a steady-state step
        vae2 = build_vae(V, ni, H, nz, dev, params=O.random_params(V, ni, H, nz, seed=8, scale=0.3, emb_scale=0.5, head_scale=0.3))
        tr2 = _trainer(vae2, lr=0.1, clip=5.0, nsamples=ns)
        tr2.prepare_batches(batches)
        for x in batches:
            tr2.step(x, 0.5)
        tr2.commit()
        torch.cuda.synchronize(dev)
        b0 = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
        for i in range(10):
            tr2.step(batches[i % 2], 0.5)
        torch.cuda.synchronize(dev)
        assert grew <= torch.cuda.memory_stats(dev)["allocation.all.allocated"] - b0

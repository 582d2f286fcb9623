"""The importance-weighted bound in the fused image step (AggressiveImageTrainer(objective="iw")) and the doubly-reparameterised
estimator on both modalities (iw_estimator="dreg", VAE.loss_iw(estimator="dreg")): the new kernels against float64
statements, the fused steps against fixtures produced by the reference's own classes (tests/golden/make_golden_iw_dreg.py), the
drop-in route against the fused one, hipGraph replay, fences and the wiring of the loops.

Kernel, text-step and host-contract tests run on the emulator (`not gpu`) and on the MI355X (`gpu`).  Everything that runs a whole
image step runs on the MI355X only, as in tests/test_image_multisample.py: one ResNet / PixelCNN step takes minutes on the
thread-level emulator."""
import argparse
import math

import numpy as np
import pytest
import torch

import parity_common as pc
from helpers import ALL_KEYS, DEC_KEYS, ENC_KEYS, build_vae, load, rel_err
from parity_common import GRAD_RTOL, RTOL
from vae_lagging_encoder_amd import engine as _eng
from vae_lagging_encoder_amd.engine import P

ULP1 = 2.0 ** -23


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def target(request):
    if request.param == "emu":
        request.getfixturevalue("emu_backend")
        dev = torch.device("cpu")
    else:
        dev = request.getfixturevalue("hip_device")
    return _eng.backend_for(dev), dev


@pytest.fixture
def gpu(request):
    dev = request.getfixturevalue("hip_device")
    return _eng.backend_for(dev), dev


def _text_trainer(*a, **k):
    from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer
    return AggressiveTextTrainer(*a, **k)


def _image_trainer(*a, **k):
    from vae_lagging_encoder_amd.trainer import AggressiveImageTrainer
    return AggressiveImageTrainer(*a, **k)


def _pair_delta(got, want):
    """largest error of a within-row difference log w_s - log w_s'"""
    d = torch.as_tensor(got).detach().double().cpu() - torch.as_tensor(want).double()
    return float((d.unsqueeze(2) - d.unsqueeze(1)).abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# 1. lv_loss_assemble_dreg_f32 / _rng_f32
SHAPES = [(1, 1, 1, 1), (1, 3, 2, 5), (7, 5, 4, 32), (1, 2, 7, 65)]                 # T, B, ns, nz


def _latents(B, ns, nz, g, scale=0.3):
    mulv = torch.randn(B, 2 * nz, generator=g) * scale
    eps = torch.randn(B, ns, nz, generator=g)
    z = mulv[:, None, :nz] + eps * torch.exp(0.5 * mulv[:, None, nz:])
    return mulv, eps, z


def _statement(nll, mulv, eps, z, beta, ns):
    """float64: log w [B][ns] and wn = softmax_s(log w)"""
    T = nll.shape[0]
    B, nz = mulv.shape[0], mulv.shape[1] // 2
    rec_s = nll.double().view(T, B, ns).sum(0)
    lv = mulv[:, nz:].double()
    logw = -rec_s - beta * (0.5 * z.double().pow(2).sum(-1) - 0.5 * eps.double().pow(2).sum(-1) - 0.5 * lv.sum(-1, keepdim=True))
    return logw, torch.softmax(logw, dim=1)


def _assemble(lib, dev, dreg, nll, mulv, eps, z, kl, klw, gl, acc, T, B, ns, nz, rng_state=None, inc=0):
    """One launch on NaN-filled outputs -> dict of host tensors."""
    s = _eng.stream_ptr(dev)
    d = {k: v.clone().to(dev) for k, v in dict(nll=nll, mulv=mulv, eps=eps, z=z, kl=kl, klw=klw, gl=gl, acc=acc).items()}
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
    o = dict(loss=nan(B), rec=nan(B), rowscale=nan(B * ns), wz=nan(B, ns), logw=nan(B, ns))
    if dreg:
        o["rs"] = nan(B, ns)
    a = (P(d["nll"]), P(d["mulv"]), P(d["eps"]), P(d["z"]), P(d["kl"]), P(d["klw"]), P(d["gl"]), P(o["loss"]), P(o["rec"]),
         P(o["rowscale"]), P(o["wz"])) + ((P(o["rs"]),) if dreg else ()) + (P(o["logw"]), P(d["acc"]), T, B, ns, nz)
    name = "lv_loss_assemble_%s%s_f32" % ("dreg" if dreg else "iw", "_rng" if rng_state is not None else "")
    if rng_state is not None:
        getattr(lib, name)(*a, P(rng_state), inc, s)
    else:
        getattr(lib, name)(*a, s)
    out = {k: v.cpu() for k, v in o.items()}
    out["acc"] = d["acc"].cpu()
    return out


@pytest.mark.parametrize("beta", [1.0, 0.37, 0.0])
@pytest.mark.parametrize("T,B,ns,nz", SHAPES)
def test_loss_assemble_dreg(target, T, B, ns, nz, beta):
    lib, dev = target
    g = torch.Generator().manual_seed(T + 31 * B + ns + 7 * nz)
    nll = torch.rand(T, B * ns, generator=g) * 5
    mulv, eps, z = _latents(B, ns, nz, g)
    kl = torch.rand(B, generator=g)
    klw = torch.tensor([beta])
    acc0 = torch.tensor([1.5, -2.0, 0.25])
    gl2 = torch.tensor([2.0 ** -(1 + b % 5) for b in range(B)])            # powers of two: g * wn is exact
    args = (nll, mulv, eps, z, kl, klw, gl2, acc0, T, B, ns, nz)
    iw = _assemble(lib, dev, False, *args)
    r = _assemble(lib, dev, True, *args)
    for k, v in r.items():
        assert torch.isfinite(v).all(), k                                  # every NaN of the pre-fill was overwritten
    for k in ("loss", "rec", "rowscale", "logw", "acc"):                   # the iw entry's bits
        assert torch.equal(r[k], iw[k]), k
    # rs and wz against the float64 statement.  wn is within 2 delta wn + 1 ulp of the statement's (the argument of
    # tests/test_iw_objective.py::test_loss_assemble_iw, delta = 1e-6 max|log w| the bound on log w); r = 1 - beta (1 - wn) adds the
    # rounding of 1 - wn and of the result, both at most half an ulp of 1; c' = (beta g wn) r: three more roundings, relative.
    logw64, wn64 = _statement(nll, mulv, eps, z, beta, ns)
    delta = 1e-6 * float(logw64.abs().max())
    r64 = 1.0 - beta * (1.0 - wn64)
    err_wn = 2 * delta * wn64 + ULP1
    err_r = beta * err_wn + ULP1
    assert bool(((r["rs"].double() - r64).abs() <= err_r).all()), float((r["rs"].double() - r64).abs().max())
    c64 = beta * gl2.double()[:, None] * wn64 * r64
    err_c = beta * gl2.double()[:, None] * (err_wn * r64.abs() + wn64 * err_r) + 3 * ULP1 * c64.abs()
    assert bool(((r["wz"].double() - c64).abs() <= err_c).all()), float((r["wz"].double() - c64).abs().max())
    # ... and as the kernel's own f32 statement, bit for bit: c' = (beta * rowscale) * r
    assert torch.equal(r["wz"], (klw * r["rowscale"].view(B, ns)) * r["rs"])
    if ns == 1:
        assert bool((r["rs"] == 1).all())                                  # exactly 1 at wn = 1, for every beta
    if beta == 0.0:
        assert bool((r["rs"] == 1).all()) and bool((r["wz"] == 0).all())
    # the rng twin: the same bits, and only the offset word of the Philox state moves
    state = torch.tensor([12345, 7], dtype=torch.int64, device=dev)
    r3 = _assemble(lib, dev, True, *args, rng_state=state, inc=3)
    assert state.cpu().tolist() == [12345, 10]
    for k in r:
        assert torch.equal(r3[k], r[k]), k


def test_loss_assemble_dreg_far_apart_weights(target):
    """A weight that underflows to exactly 0: every output finite, r = 1 - beta there, c' = 0."""
    lib, dev = target
    T, B, ns, nz = 4, 3, 3, 4
    g = torch.Generator().manual_seed(5)
    base = torch.rand(T, B, 1, generator=g) * 5
    step = torch.tensor([[0.0, 50.0, 100.0], [50.0, 0.0, 75.0], [0.0, 0.125, 50.0]])
    nll = (base + step[None]).reshape(T, B * ns)
    mulv, eps, z = _latents(B, ns, nz, g)
    kl = torch.rand(B, generator=g)
    for beta in (1.0, 0.4):
        klw = torch.tensor([beta])
        r = _assemble(lib, dev, True, nll, mulv, eps, z, kl, klw, torch.full((B,), 0.25), torch.zeros(3), T, B, ns, nz)
        for k, v in r.items():
            assert torch.isfinite(v).all(), k
        wn = r["rowscale"].view(B, ns) / 0.25
        far = wn == 0
        assert int(far.sum()) == 5
        assert bool((r["wz"][far] == 0).all()) and bool((r["rs"][far] == torch.tensor(1.0) - klw).all())
        lone = wn == 1                                                     # a lone dominant weight: r is exactly 1
        assert bool((r["rs"][lone] == 1).all())


# ---------------------------------------------------------------------------------------------------------------------
# 2. lv_reparam_iwdz_bwd_f32 and lv_enc_head_dreg_bwd_f32 against float64
BWD_SHAPES = [(1, 1, 1), (3, 2, 5), (5, 4, 32), (2, 7, 65)]                # B, ns, nz


def _bwd_case(B, ns, nz, H, parts, seed):
    g = torch.Generator().manual_seed(seed)
    mulv, eps, _ = _latents(B, ns, nz, g, scale=0.5)
    dz = torch.randn(B, ns, nz, generator=g)
    frac = torch.rand(parts, generator=g) + 0.1
    frac = frac / frac.sum()
    dzp = (frac[:, None, None, None] * dz[None]).contiguous()              # partial sums of one sign per element: no cancellation
    wz = torch.rand(B, ns, generator=g) / ns
    rs = 1.0 - 0.7 * torch.rand(B, ns, generator=g)
    hT = torch.randn(B, H, generator=g)
    wlin = torch.randn(2 * nz, H, generator=g) * 0.3
    return mulv, eps, dzp, wz, rs, hT, wlin


def _dmulv_statement(mulv, eps, dz, wz, rs):
    """float64 dmulv of DESIGN.md 3.3b (rs None) / 3.3c"""
    nz = mulv.shape[1] // 2
    mu, lv = mulv[:, None, :nz].double(), mulv[:, None, nz:].double()
    sd, e, c = torch.exp(0.5 * lv), eps.double(), wz.double()[:, :, None]
    zz = mu + e * sd
    if rs is None:
        t = dz.double() + c * zz
        return torch.cat((t.sum(1), (t * 0.5 * e * sd).sum(1) - 0.5 * wz.double().sum(1, keepdim=True)), dim=1)
    t = rs.double()[:, :, None] * dz.double() + c * (zz - e * torch.exp(-0.5 * lv))
    return torch.cat((t.sum(1), (t * 0.5 * e * sd).sum(1)), dim=1)


def _run_iwdz(lib, dev, mulv, eps, dz, wz, rs):
    B, ns, nz = eps.shape
    d = [t.to(dev) for t in (mulv, eps, dz.contiguous(), wz)]
    rs_d = None if rs is None else rs.to(dev)
    out = torch.full((B, 2 * nz), float("nan"), device=dev)
    lib.lv_reparam_iwdz_bwd_f32(P(d[0]), P(d[1]), P(d[2]), P(d[3]), None if rs_d is None else P(rs_d), P(out), B, ns, nz, _eng.stream_ptr(dev))
    return out.cpu()


def _run_head(lib, dev, name, mulv, eps, dzp, seed4, hT, wlin, rs=None):
    B, ns, nz = eps.shape
    H = hT.shape[1]
    d = [t.to(dev) for t in (mulv, eps, dzp, seed4, hT, wlin)]
    rs_d = None if rs is None else rs.to(dev)
    extra = () if rs is None else (P(rs_d),)
    out = [torch.full(shape, float("nan"), device=dev) for shape in ((B, 2 * nz), (B, H), (2 * nz, H))]
    getattr(lib, name)(P(d[0]), P(d[1]), P(d[2]), dzp.shape[0], P(d[3]), *extra, P(d[4]), P(d[5]), P(out[0]), P(out[1]), P(out[2]), B, H, ns,
                       nz, _eng.stream_ptr(dev))
    return [o.cpu() for o in out]


@pytest.mark.parametrize("B,ns,nz", BWD_SHAPES)
def test_iwdz_and_dreg_head_backward(target, B, ns, nz):
    lib, dev = target
    # H = 40: two full blocks of 16 columns and one of 8 (not a multiple of 64, nor of the block); H = 1000 on the GPU only
    for H, parts in [(40, 1), (40, 3)] + ([(1000, 1), (1000, 3)] if dev.type == "cuda" else []):
        mulv, eps, dzp, wz, rs, hT, wlin = _bwd_case(B, ns, nz, H, parts, seed=B * 100 + ns * 10 + nz + parts)
        dz = dzp.sum(0)
        for mode_rs in (None, rs):
            want = _dmulv_statement(mulv, eps, dzp.double().sum(0), wz, mode_rs)
            tol = 1e-5 * (1 + float(want.abs().max()))                     # tests/test_iw_objective.py::test_iw_backward_kernels's bounds
            got = _run_iwdz(lib, dev, mulv, eps, dz, wz, mode_rs)
            assert torch.isfinite(got).all()                               # '=' into a NaN-poisoned buffer
            assert float((got.double() - want).abs().max()) < tol, (H, parts, mode_rs is None)
        want = _dmulv_statement(mulv, eps, dzp.double().sum(0), wz, rs)
        dmulv, dhT, gW = _run_head(lib, dev, "lv_enc_head_dreg_bwd_f32", mulv, eps, dzp, wz, hT, wlin, rs=rs)
        dhT64, gW64 = want @ wlin.double(), want.t() @ hT.double()
        for o in (dmulv, dhT, gW):
            assert torch.isfinite(o).all()
        assert float((dmulv.double() - want).abs().max()) < 1e-5 * (1 + float(want.abs().max())), (H, parts)
        assert float((dhT.double() - dhT64).abs().max()) < 2e-5 * float(dhT64.abs().max()), (H, parts)
        assert float((gW.double() - gW64).abs().max()) < 2e-5 * float(gW64.abs().max()), (H, parts)
        # wz = 0, rs = 1: the plain head's bits at dkl = 0
        a = _run_head(lib, dev, "lv_enc_head_dreg_bwd_f32", mulv, eps, dzp, torch.zeros(B, ns), hT, wlin, rs=torch.ones(B, ns))
        b = _run_head(lib, dev, "lv_enc_head_bwd_f32", mulv, eps, dzp, torch.zeros(B), hT, wlin)
        for x, y, k in zip(a, b, ("dmulv", "dhT", "gW_lin")):
            assert torch.equal(x, y), (k, H, parts)
        # the head's dmulv and lv_reparam_iwdz_bwd_f32's are the same sums in the same order when dz arrives in one part
        if parts == 1:
            assert torch.equal(dmulv, _run_iwdz(lib, dev, mulv, eps, dz, wz, rs))
    # rs = NULL, wz = 0: lv_reparam_kl_bwd_f32 with dkl = 0, bit for bit
    got = _run_iwdz(lib, dev, mulv, eps, dz, torch.zeros(B, ns), None)
    d = [t.to(dev) for t in (mulv, eps, dz.contiguous(), torch.zeros(B))]
    ref = torch.full((B, 2 * nz), float("nan"), device=dev)
    lib.lv_reparam_kl_bwd_f32(P(d[0]), P(d[1]), P(d[2]), P(d[3]), P(ref), B, ns, nz, _eng.stream_ptr(dev))
    assert torch.equal(got, ref.cpu())


def test_new_kernels_refuse_bad_arguments(target):
    lib, dev = target
    t = torch.full((64,), 7.0, device=dev)
    raw = lambda name: getattr(lib, "_raw_" + name)
    a = [P(t)] * 14
    for name, tail in (("lv_loss_assemble_dreg_f32", (None,)), ("lv_loss_assemble_dreg_rng_f32", (P(t), 1, None))):
        for i in range(14):
            if i == 12:
                continue                                                   # logw may be NULL
            bad = list(a)
            bad[i] = None
            assert raw(name)(*bad, 1, 1, 1, 1, *tail) < 0, (name, i)
        for sizes in ((-1, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, -3, 1, 1)):
            assert raw(name)(*a, *sizes, *tail) < 0, (name, sizes)
    assert raw("lv_loss_assemble_dreg_rng_f32")(*a, 1, 1, 1, 1, None, 1, None) < 0                 # no rng state
    for i in (0, 1, 2, 3, 5):                                              # (4: rs may be NULL -- the standard estimator)
        bad = [P(t)] * 6
        bad[i] = None
        assert raw("lv_reparam_iwdz_bwd_f32")(*bad, 1, 1, 1, None) < 0, i
    for sizes in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-2, 1, 1)):
        assert raw("lv_reparam_iwdz_bwd_f32")(*[P(t)] * 6, *sizes, None) < 0
    h = lambda ptrs, parts, sizes: raw("lv_enc_head_dreg_bwd_f32")(ptrs[0], ptrs[1], ptrs[2], parts, *ptrs[3:], *sizes, None)
    for i in range(10):
        bad = [P(t)] * 10
        bad[i] = None
        assert h(bad, 1, (1, 1, 1, 1)) < 0, i
    for parts, sizes in ((0, (1, 1, 1, 1)), (1, (0, 1, 1, 1)), (1, (1, 0, 1, 1)), (1, (1, 1, 0, 1)), (1, (1, 1, 1, 0))):
        assert h([P(t)] * 10, parts, sizes) < 0, (parts, sizes)
    assert bool((t.cpu() == 7.0).all())                                    # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# 3. the fused text step with iw_estimator="dreg" against the reference fixture
def _text_case(tag):
    """The case as tests/test_iw_objective.py reads it: inputs and weights from text_iw_small.npz (or the case's own), the values and
    the encoder's gradients from text_dreg_small.npz; the decoder's gradient is the "iwae" case's."""
    fx = load("text_dreg_small")
    pre = tag + "/"
    d = {k[len(pre):]: fx[k] for k in fx.files if k.startswith(pre)}
    if not bool(d["own_inputs"]):
        base = load("text_iw_small")
        c = {k[len(pre):]: base[k] for k in base.files if k.startswith(pre)}
        c.update(d)
        d = c
    coef = np.float32(d["coef"])
    for k in ENC_KEYS:                                                     # plain SGD, lr = 1, on the clipped gradient
        d["new/" + k] = d["param/" + k] - d["grad/" + k] * coef
    return d


TEXT_CASES = ["ns2_wide_clip", "ns3_T2", "ns4_mid", "ns1"]


@pytest.mark.parametrize("tag", TEXT_CASES)
def test_fused_text_dreg_step_matches_reference_fixture(target, tag):
    """tests/test_iw_objective.py::test_fused_iw_step_matches_reference_fixture's quantities and bounds."""
    _, dev = target
    c = _text_case(tag)
    V, ni, H, nz, B, T, ns = (int(c[k]) for k in ("V", "ni", "H", "nz", "B", "T", "ns"))
    vae = build_vae(V, ni, H, nz, dev, params={k: torch.from_numpy(c["param/" + k]) for k in ALL_KEYS})
    tr = _text_trainer(vae, lr=1.0, clip=float(c["max_norm"]), nsamples=ns, objective="iw", iw_estimator="dreg")
    x = torch.from_numpy(c["x"]).to(dev)
    noise = tuple(torch.from_numpy(c[k]).to(dev) for k in ("eps", "mask_in", "mask_out"))
    tr.step(x, float(c["kl_weight"]), noise=noise)
    stt = tr.read_stats()
    st = tr.static[(B, T)]
    rec_scale = float(np.abs(c["rec"]).max())
    delta = _pair_delta(st.logw, c["logw"])
    print(tag, "loss %.1e rec %.1e delta %.1e" % (rel_err(st.loss, c["loss"]), rel_err(st.rec, c["rec"]), delta))
    assert rel_err(st.loss, c["loss"]) < RTOL and rel_err(st.rec, c["rec"]) < RTOL
    assert rel_err(st.logw, c["logw"]) < RTOL and delta < RTOL * rec_scale
    kl_err = float(np.abs(st.kl.cpu().numpy() - c["kl"]).max())
    assert kl_err < RTOL * float(np.abs(c["kl"]).max()) + 1e-6 * (1 + rec_scale), ("kl", kl_err)
    assert abs(stt["loss_sum"] - float(c["loss"].sum())) < RTOL * abs(float(c["loss"].sum()))
    assert abs(stt["rec_sum"] - float(c["rec"].sum())) < RTOL * abs(float(c["rec"].sum()))
    assert abs(stt["norm"] - float(c["total_norm"])) < RTOL * float(c["total_norm"])
    assert abs(stt["coef"] - float(c["coef"])) < RTOL
    named = dict(vae.named_parameters())
    worst = 0.0
    for k in ALL_KEYS:
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
    for k in DEC_KEYS:
        assert torch.equal(sd[k].cpu(), torch.from_numpy(c["param/" + k])), k
    if ns == 1:
        assert bool((st.rs == 1).all())


# ---------------------------------------------------------------------------------------------------------------------
# 4. VAE.loss_iw(estimator=...) on the text model
def test_loss_iw_dreg_equals_fused_step_and_iwae_keeps_its_bits(target):
    from vae_lagging_encoder_amd import optim as lvo
    _, dev = target
    c = _text_case("ns4_mid")
    V, ni, H, nz, B, T, ns = (int(c[k]) for k in ("V", "ni", "H", "nz", "B", "T", "ns"))
    clip, klw = float(c["max_norm"]), float(c["kl_weight"])
    params = {k: torch.from_numpy(c["param/" + k]) for k in ALL_KEYS}
    x = torch.from_numpy(c["x"]).to(dev)
    noise = tuple(torch.from_numpy(c[k]).to(dev) for k in ("eps", "mask_in", "mask_out"))

    def dropin(**kw):
        b = build_vae(V, ni, H, nz, dev, params=params)
        b.zero_grad()
        loss, rec, kl = b.loss_iw(x, klw, nsamples=ns, noise=noise, **kw)
        loss.mean(dim=-1).backward()
        return b, loss.detach(), rec.detach(), kl.detach(), {k: p.grad.detach().clone() for k, p in b.named_parameters()}
    b, loss, rec, kl, raw = dropin(estimator="dreg")
    total = float(lvo.clip_grad_norm_(b.parameters(), clip))
    a = build_vae(V, ni, H, nz, dev, params=params)
    tr = _text_trainer(a, lr=1.0, clip=clip, nsamples=ns, objective="iw", iw_estimator="dreg")
    tr.step(x, klw, noise=noise)
    s_ = tr.static[(B, T)]
    assert abs(tr.read_stats()["norm"] - total) < 1e-5 * total
    assert rel_err(s_.loss, loss) < 1e-5 and rel_err(s_.rec, rec) < 1e-5 and rel_err(s_.kl, kl) < 1e-5
    for k, p in a.named_parameters():
        gb = dict(b.named_parameters())[k].grad
        if float(gb.abs().max()) > 0:
            assert rel_err(p.grad, gb) < 1e-5, (k, rel_err(p.grad, gb))
        else:
            assert float(p.grad.abs().max()) == 0.0, k
    # the decoder's parameters receive sum_s wn_s grad_theta under both estimators; the encoder's gradient differs
    _, loss_i, _, _, raw_i = dropin(estimator="iwae")
    assert torch.equal(loss_i, loss)
    for k in DEC_KEYS:
        assert rel_err(raw[k], raw_i[k]) < 1e-5 or float(raw_i[k].abs().max()) == 0.0, k
    assert rel_err(raw["encoder.linear.weight"], raw_i["encoder.linear.weight"]) > 1e-2
    # estimator="iwae" is the call without the argument, bit for bit
    _, loss_0, rec_0, kl_0, raw_0 = dropin()
    assert torch.equal(loss_0, loss_i)
    for k in raw_0:
        assert torch.equal(raw_0[k], raw_i[k]), k
    with pytest.raises(ValueError, match="estimator"):
        b.loss_iw(x, klw, nsamples=ns, noise=noise, estimator="score")


# ---------------------------------------------------------------------------------------------------------------------
# 5. fences and wiring (no image step is run: also on the emulator)
def test_fences(target):
    _, dev = target
    vae = pc.build_image_vae(dev, 5)
    with pytest.raises(ValueError, match="free_bits"):
        _image_trainer(vae, objective="iw", free_bits=0.1)
    with pytest.raises(ValueError, match="iw_estimator"):
        _image_trainer(vae, objective="elbo", iw_estimator="dreg")
    with pytest.raises(ValueError, match="iw_estimator"):
        _image_trainer(vae, iw_estimator="dreg")
    with pytest.raises(ValueError, match="objective"):
        _image_trainer(vae, objective="iwae")
    with pytest.raises(ValueError, match="iw_estimator"):
        _image_trainer(vae, objective="iw", iw_estimator="stl")
    tr = _image_trainer(vae, objective="iw", iw_estimator="dreg", nsamples=1)
    assert (tr.objective, tr.iw_estimator, tr.logw) == ("iw", "dreg", None)
    assert (_image_trainer(vae).objective, _image_trainer(vae).iw_estimator) == ("elbo", "iwae")
    tv = build_vae(53, 8, 16, 4, dev, seed=0)
    with pytest.raises(ValueError, match="iw_estimator"):
        _text_trainer(tv, iw_estimator="dreg")
    with pytest.raises(ValueError, match="iw_estimator"):
        _text_trainer(tv, objective="iw", iw_estimator="stl")
    with pytest.raises(ValueError, match="nsamples"):                      # "dreg" keeps the fences of "iw"
        _text_trainer(tv, objective="iw", iw_estimator="dreg", use_graph=True)
    assert _text_trainer(tv, objective="iw", iw_estimator="dreg").iw_estimator == "dreg"


def _loop_args(**kw):
    d = dict(kl_start=0.1, warm_up=2, batch_size=4, epochs=1, aggressive=0, nsamples=2, test_nepoch=5)
    d.update(kw)
    return argparse.Namespace(**d)


def test_training_loops_read_objective_and_estimator(target):
    from vae_lagging_encoder_amd.training import ImageTrainingLoop, TextTrainingLoop
    from oracle import text_vae_oracle as O
    _, dev = target
    vae = pc.build_image_vae(dev, 6)
    xs = torch.rand(8, 1, 28, 28, generator=torch.Generator().manual_seed(1))
    mk = lambda trainer=None, **kw: ImageTrainingLoop(vae, xs, xs[:4], None, _loop_args(**kw), trainer=trainer, log=lambda *a: None)
    loop = mk()
    assert (loop.objective, loop.iw_estimator, loop.trainer.objective, loop.trainer.iw_estimator) == ("elbo", "iwae", "elbo", "iwae")
    loop = mk(objective="iw")
    assert (loop.trainer.objective, loop.trainer.iw_estimator, loop.trainer.nsamples) == ("iw", "iwae", 2)
    loop = mk(objective="iw", iw_estimator="dreg")
    assert (loop.trainer.objective, loop.trainer.iw_estimator) == ("iw", "dreg")
    with pytest.raises(ValueError, match="objective"):
        mk(trainer=_image_trainer(vae, nsamples=2), objective="iw")
    with pytest.raises(ValueError, match="objective"):
        mk(trainer=_image_trainer(vae, nsamples=2, objective="iw"))
    with pytest.raises(ValueError, match="iw_estimator"):
        mk(trainer=_image_trainer(vae, nsamples=2, objective="iw"), objective="iw", iw_estimator="dreg")
    with pytest.raises(ValueError, match="iw_estimator"):
        mk(trainer=_image_trainer(vae, nsamples=2, objective="iw", iw_estimator="dreg"), objective="iw")
    with pytest.raises(ValueError, match="iw_estimator"):
        mk(iw_estimator="dreg")                                            # an estimator of "iw", not of "elbo"
    with pytest.raises(ValueError, match="iw_estimator"):
        mk(objective="iw", iw_estimator="stl")
    with pytest.raises(ValueError, match="free_bits"):
        mk(objective="iw", free_bits=0.1)
    assert mk(trainer=_image_trainer(vae, nsamples=2, objective="iw", iw_estimator="dreg"), objective="iw",
              iw_estimator="dreg").trainer.iw_estimator == "dreg"
    # the text loop
    V, ni, H, nz, B = 53, 8, 16, 4, 4
    tv = build_vae(V, ni, H, nz, dev, params=O.random_params(V, ni, H, nz, seed=2, scale=0.2, emb_scale=0.5, head_scale=0.5))
    train = [O.synthetic_batch(B, T, V, seed=10 + i).to(dev) for i, T in enumerate((5, 6))]
    targs = lambda **kw: argparse.Namespace(kl_start=0.1, warm_up=1, batch_size=B, epochs=1, aggressive=0, nsamples=2, test_nepoch=5,
                                            iw_nsamples=20, momentum=0, **kw)
    tl = TextTrainingLoop(tv, train, train[:1], train[:1], targs(objective="iw", iw_estimator="dreg"), log=lambda *_: None)
    assert (tl.iw_estimator, tl.trainer.iw_estimator) == ("dreg", "dreg")
    assert TextTrainingLoop(tv, train, train[:1], train[:1], targs(objective="iw"), log=lambda *_: None).trainer.iw_estimator == "iwae"
    with pytest.raises(ValueError, match="iw_estimator"):
        TextTrainingLoop(tv, train, train[:1], train[:1], targs(objective="iw", iw_estimator="dreg"),
                         trainer=_text_trainer(tv, nsamples=2, objective="iw"), log=lambda *_: None)
    with pytest.raises(ValueError, match="iw_estimator"):
        TextTrainingLoop(tv, train, train[:1], train[:1], targs(iw_estimator="dreg"), log=lambda *_: None)


def test_toy_loop_reads_iw_estimator(target):
    from vae_lagging_encoder_amd import training
    _, dev = target
    # the helper all three loops read the field through
    ns_ = argparse.Namespace
    assert training._iw_estimator(ns_(), None, "elbo") == "iwae"
    assert training._iw_estimator(ns_(iw_estimator="dreg"), None, "iw") == "dreg"
    with pytest.raises(ValueError, match="iw_estimator"):
        training._iw_estimator(ns_(iw_estimator="dreg"), None, "elbo")
    tv = build_vae(53, 8, 16, 4, dev, seed=0)
    with pytest.raises(ValueError, match="iw_estimator"):
        training._iw_estimator(ns_(iw_estimator="dreg"), _text_trainer(tv, objective="iw"), "iw")
    toy = lambda trainer, **kw: training.ToyTrainingLoop(None, [1, 2], [], [], None, ns_(nsamples=1, optim="sgd", plot_mode="multiple", **kw),
                                                         trainer=trainer)
    with pytest.raises(ValueError, match="iw_estimator"):
        toy(_text_trainer(tv, objective="iw"), objective="iw", iw_estimator="dreg")
    with pytest.raises(ValueError, match="iw_estimator"):
        toy(_text_trainer(tv, objective="iw", iw_estimator="dreg"), objective="iw")
    with pytest.raises(ValueError, match="iw_estimator"):
        toy(None, iw_estimator="dreg")


# ---------------------------------------------------------------------------------------------------------------------
# 6. the fused image step against the reference fixtures (MI355X)
def _image_fixture():
    fx = load("image_iw_small")
    return {k: fx[k] for k in fx.files}


def _image_model(dev, fx):
    """The seeded model with the fixture's encoder head (make_golden_iw_dreg.build_image); the stored entries are checked."""
    vae = pc.build_image_vae(dev, int(fx["model_seed"]))
    g = torch.Generator().manual_seed(int(fx["head_seed"]))
    w = vae.encoder.linear.weight
    with torch.no_grad():
        w.copy_(((torch.rand(tuple(w.shape), generator=g) * 2 - 1) * float(fx["head_scale"])).to(dev))
    sd = vae.state_dict()
    for i, k in enumerate(str(n) for n in fx["names"]):
        idx = torch.from_numpy(fx["sample_idx"][i].astype(np.int64))
        assert torch.equal(sd[k].reshape(-1)[idx].cpu(), torch.from_numpy(fx["sample_p0"][i])), k
    return vae


def _image_case(fx, tag):
    pre = tag + "/"
    c = {k[len(pre):]: fx[k] for k in fx if k.startswith(pre)}
    if "base" in c:                       # a "dreg" case: batch, noise, values, statistics and the decoder's records are the base case's
        b = _image_case(fx, str(c["base"]))
        names, enc = [str(n) for n in fx["names"]], [str(n) for n in fx["enc_names"]]
        gradnorm, sample_grad = b["gradnorm"].copy(), b["sample_grad"].copy()
        for j, k in enumerate(enc):
            gradnorm[names.index(k)], sample_grad[names.index(k)] = c["gradnorm"][j], c["sample_grad"][j]
        b.update(c)
        b["gradnorm"], b["sample_grad"] = gradnorm, sample_grad
        c = b
    return c


def _unclipped_grads(tr):
    coef = tr.read_stats()["coef"]
    out = {}
    for pre, eng in (("encoder.", tr.enc), ("decoder.", tr.dec)):
        for n in eng.flat.names:
            out[pre + n] = eng.flat.gviews[n].detach().clone() / coef
    return out


def _check_image_step(fx, tag, dev, precision="f32", use_graph=False):
    """parity_common's image bounds (_check_image_outputs, test_image_multisample's step check); the gradient bounds widened by
    2 * delta, delta the measured within-row error of log w, itself capped at 1e-4 * max|rec|."""
    c = _image_case(fx, tag)
    B, ns, est = int(c["B"]), int(c["ns"]), str(c["estimator"])
    vae = _image_model(dev, fx)
    tr = _image_trainer(vae, lr=1e-3, clip=5.0, nsamples=ns, objective="iw", iw_estimator=est, precision=precision, use_graph=use_graph)
    x = torch.from_numpy(c["x"]).float().to(dev)
    tr.step(x, float(c["kl_weight"]), eps=torch.from_numpy(c["eps"]).to(dev))
    st = tr.read_stats()
    assert tuple(tr.logw.shape) == (B, ns)
    delta = _pair_delta(tr.logw, c["logw"])
    cap = 1e-4 * float(np.abs(c["rec"]).max())
    errs = dict(loss=abs(st["loss_sum"] - float(c["loss"].sum())) / abs(float(c["loss"].sum())),
                rec=abs(st["rec_sum"] - float(c["rec"].sum())) / abs(float(c["rec"].sum())),
                kl=abs(st["kl_sum"] - float(c["kl"].sum())) / abs(float(c["kl"].sum())), logw=rel_err(tr.logw, c["logw"]),
                norm=abs(st["norm"] - float(c["total_norm64"])) / float(c["total_norm64"]))
    print(tag, precision, "delta %.2e (cap %.2e)" % (delta, cap), errs)
    assert delta < cap, (delta, cap)
    assert errs["loss"] < RTOL and errs["rec"] < RTOL and errs["kl"] < RTOL and errs["logw"] < RTOL, errs
    assert errs["norm"] < 5e-4 + 2 * delta, errs
    grads = _unclipped_grads(tr)
    names = [str(n) for n in fx["names"]]
    worst = 0.0
    for i, k in enumerate(names):
        g = grads[k]
        ref_n = float(c["gradnorm"][i])
        assert abs(float(g.double().norm()) - ref_n) <= (2e-3 + 2 * delta) * ref_n + 1e-7, (k, float(g.double().norm()), ref_n)
        idx = torch.from_numpy(fx["sample_idx"][i].astype(np.int64)).to(dev)
        e = float((g.reshape(-1)[idx].cpu() - torch.from_numpy(c["sample_grad"][i])).abs().max())
        worst = max(worst, e / (ref_n / max(1.0, g.numel() ** 0.5) + 1e-12))
    assert worst < 0.05 + 2 * delta, worst
    sd = vae.state_dict()
    for i, k in enumerate(str(n) for n in fx["stat_names"]):
        assert rel_err(sd[k][:8], c["stat"][i]) < 1e-4, k
    enc = [str(n) for n in fx["enc_names"]]
    upd = 0.0
    for i, k in enumerate(names):
        idx = torch.from_numpy(fx["sample_idx"][i].astype(np.int64))
        got, p0 = sd[k].reshape(-1)[idx].cpu(), torch.from_numpy(fx["sample_p0"][i])
        if k in enc:                      # Adam's first step moves every weight by ~lr: compare the UPDATE
            e = float(((got - p0) - (torch.from_numpy(c["sample_new"][enc.index(k)]) - p0)).abs().max())
            upd = max(upd, e)
            assert e < 2e-5, (k, e)
        else:                             # decoder untouched except MaskedConv2d's in-place weight masking
            assert bool(((got == p0) | (got == 0)).all()), k
    print(tag, "gradient samples %.2e of the RMS, encoder update %.1e" % (worst, upd))
    return delta, tr


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["b6_ns3", "b4_ns2", "b5_ns1", "b6_ns3_dreg", "b4_ns2_dreg"])
def test_fused_image_iw_step_matches_reference_fixture(gpu, tag):
    """Measured on the MI355X, exact-f32 configuration: delta = 1.22e-4 nats in the three ns > 1 "iwae" cases (cap 5.6e-2), sampled
    gradient entries within 6.4e-5 of the tensor's RMS, encoder update 1.3e-5.

    The decoder's BatchNorm (train mode, statistics over all B * ns images) couples the rows, so under "dreg" the step takes dz from a
    decoder backward of its own, seeded with g * u_s ("Decoders that couple the rows"): scaling the dz of the
    g * wn_s pass by r_s misses these cases by 2-3 % of a tensor's gradient norm (1.27665 against the fixture's 1.29132)."""
    _, dev = gpu
    _check_image_step(_image_fixture(), tag, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["bf16x3", "bf16"])
def test_fused_image_iw_step_other_precisions_run(gpu, precision):
    """"bf16x3" holds the f32 fixture (as for "elbo"); "bf16" is out of the fixture's reach: the step runs, its weights are finite
    and normalised."""
    _, dev = gpu
    fx = _image_fixture()
    if precision == "bf16x3":
        _check_image_step(fx, "b4_ns2", dev, precision=precision)
        return
    c = _image_case(fx, "b4_ns2_dreg")
    vae = _image_model(dev, fx)
    tr = _image_trainer(vae, nsamples=2, objective="iw", iw_estimator="dreg", precision=precision)
    tr.step(torch.from_numpy(c["x"]).float().to(dev), float(c["kl_weight"]), eps=torch.from_numpy(c["eps"]).to(dev))
    st = tr.read_stats()
    assert all(math.isfinite(v) for v in st.values()) and bool(torch.isfinite(tr.enc.flat.data).all())
    assert abs(st["loss_sum"] - float(c["loss"].sum())) / abs(float(c["loss"].sum())) < 1e-2
    assert float((torch.softmax(tr.logw, dim=1).sum(1) - 1).abs().max()) < 1e-5


@pytest.mark.gpu
def test_fused_image_iw_trajectory_matches_reference_fixture(gpu):
    """Two encoder-only steps and one update="both" step: test_image_multisample.py::test_trajectory_against_reference's quantities
    and bounds, the norm's widened by 2 * delta."""
    _, dev = gpu
    fx = _image_fixture()
    c = _image_case(fx, "traj_b4_ns2")
    ns = int(c["ns"])
    vae = _image_model(dev, fx)
    tr = _image_trainer(vae, lr=1e-3, clip=5.0, nsamples=ns, objective="iw")
    updates = [str(u) for u in c["updates"]]
    assert updates == ["encoder", "encoder", "both"]
    for i, upd in enumerate(updates):
        tr.reset_stats()
        tr.step(torch.from_numpy(c["x"][i]).float().to(dev), float(c["kl_weight"]), eps=torch.from_numpy(c["eps"][i]).to(dev), update=upd)
        st = tr.read_stats()
        delta = _pair_delta(tr.logw, c["logw"][i])
        assert delta < 1e-4 * float(c["rec_max"][i]), (i, delta)
        for k in ("loss", "rec", "kl"):
            e = abs(st[k + "_sum"] - float(c[k + "_sum"][i])) / abs(float(c[k + "_sum"][i]))
            assert e < RTOL, (i, k, e)
        en = abs(st["norm"] - float(c["total_norm64"][i])) / float(c["total_norm64"][i])
        assert en < 5e-4 + 2 * delta, (i, en)
    sd = vae.state_dict()
    for j, k in enumerate(str(n) for n in fx["names"]):
        steps = sum(1 for u in updates if u == "both" or k.startswith("encoder."))
        idx = torch.from_numpy(fx["sample_idx"][j].astype(np.int64))
        p0 = torch.from_numpy(fx["sample_p0"][j])
        got = sd[k].reshape(-1)[idx].cpu()
        ref = torch.from_numpy(c["sample_new"][j])
        live = got != 0                                                    # (MaskedConv2d re-zeroes its masked taps on the next forward)
        assert float(((got - p0) - (ref - p0))[live].abs().max() if bool(live.any()) else 0.0) < 0.05 * 1e-3 * steps + 1e-7, k


# ---------------------------------------------------------------------------------------------------------------------
# 7. hipGraph, the default objective's bits, the drop-in route, the loop, steady state (MI355X)
def _state(vae, tr):
    return {k: v.detach().clone() for k, v in vae.state_dict().items()}, tr.scal.clone(), tr.logw.clone() if tr.logw is not None else None


@pytest.mark.gpu
@pytest.mark.parametrize("est", ["iwae", "dreg"])
def test_hipgraph_replays_equal_eager_steps(gpu, est):
    """Warm-up plus two replays against three eager steps from the same state, bit for bit."""
    _, dev = gpu
    fx = _image_fixture()
    c = _image_case(fx, "b4_ns2")
    x = torch.from_numpy(c["x"]).float().to(dev)
    g = torch.Generator().manual_seed(8)
    epss = [torch.randn(4, 2, 32, generator=g).to(dev) for _ in range(3)]
    res = []
    for use_graph in (False, True):
        vae = _image_model(dev, fx)
        tr = _image_trainer(vae, use_graph=use_graph, nsamples=2, objective="iw", iw_estimator=est)
        ptrs = None
        for e in epss:
            tr.step(x, 0.5, eps=e)
            if ptrs is None:
                ptrs = tuple(t.data_ptr() for t in tr._iw_state[4])
        assert ptrs == tuple(t.data_ptr() for t in tr._iw_state[4]) and tr.logw.data_ptr() == ptrs[2]
        res.append(_state(vae, tr))
    for k in res[0][0]:
        assert torch.equal(res[0][0][k], res[1][0][k]), k
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [1, 3])
def test_objective_elbo_is_bit_identical_to_the_default(gpu, ns):
    _, dev = gpu
    g = torch.Generator().manual_seed(3)
    xs = [(torch.rand(3, 1, 28, 28, generator=g) < 0.4).float().to(dev) for _ in range(2)]
    out = []
    for kw in ({}, {"objective": "elbo", "iw_estimator": "iwae"}):
        vae = pc.build_image_vae(dev, 11)
        tr = _image_trainer(vae, seed=4242, nsamples=ns, **kw)
        for i, x in enumerate(xs):
            tr.step(x, 0.6, update="both" if i == 1 else "encoder")
        out.append(({k: v.clone() for k, v in vae.state_dict().items()}, tr.scal.clone(), tr.rng_state.clone()))
        assert tr.logw is None and not tr._iw_state
    for k in out[0][0]:
        assert torch.equal(out[0][0][k], out[1][0][k]), k
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])


@pytest.mark.gpu
@pytest.mark.parametrize("est", ["iwae", "dreg"])
def test_fused_image_step_against_dropin_loss_iw(gpu, est):
    """test_image_multisample.py::test_fused_ns3_against_dropin_route's quantities and bounds."""
    _, dev = gpu
    fx = _image_fixture()
    c = _image_case(fx, "b4_ns2")
    B, ns, klw = 4, 2, float(c["kl_weight"])
    x = torch.from_numpy(c["x"]).float().to(dev)
    eps = torch.from_numpy(c["eps"]).to(dev)
    vae = _image_model(dev, fx)
    for p in vae.parameters():
        p.grad = None
    loss, rec, kl = vae.loss_iw(x, klw, nsamples=ns, noise=(eps, None, None), estimator=est)
    loss.mean(dim=-1).backward()
    grads = {k: p.grad.detach().clone() for k, p in vae.named_parameters()}
    total = float(torch.nn.utils.clip_grad_norm_(vae.parameters(), 5.0))
    vae2 = _image_model(dev, fx)
    tr = _image_trainer(vae2, nsamples=ns, objective="iw", iw_estimator=est)
    tr.step(x, klw, eps=eps)
    st = tr.read_stats()
    assert abs(st["loss_sum"] - float(loss.sum())) / abs(float(loss.sum())) < RTOL
    assert abs(st["rec_sum"] - float(rec.sum())) / abs(float(rec.sum())) < RTOL
    assert abs(st["kl_sum"] - float(kl.sum())) / abs(float(kl.sum())) < RTOL
    assert abs(st["norm"] - total) / total < 5e-4
    for k, gv in _unclipped_grads(tr).items():
        ref_n = float(grads[k].double().norm())
        assert abs(float(gv.double().norm()) - ref_n) <= 2e-3 * ref_n + 1e-7, k


@pytest.mark.gpu
def test_image_loop_trains_on_the_bound_and_leaves_evaluation_untouched(gpu, monkeypatch):
    """Two tiny epochs (two batches of 4, nsamples = 2) under args.objective = "iw": the loop's steps are the hand-driven "iw" steps,
    bit for bit, and its validation passes are VAE.loss's -- the evaluation of the "elbo" loop on the same weights."""
    from vae_lagging_encoder_amd import evaluation as E
    from vae_lagging_encoder_amd.training import ImageTrainingLoop
    _, dev = gpu
    g = torch.Generator().manual_seed(2)
    xs = torch.rand(8, 1, 28, 28, generator=g).to(dev)
    epss = [torch.randn(4, 2, 32, generator=g) for _ in range(4)]
    order_fn = lambda n: np.arange(n)
    binarize_fn = lambda probs: (probs.to(dev) > 0.5).float()
    args = _loop_args(epochs=2, test_nepoch=99, objective="iw", iw_estimator="dreg")
    # the evaluation passes draw their eps from torch's generator: seeded per call here (the function itself is E.image_test)
    image_test, calls = E.image_test, []

    def seeded(*a, **k):
        calls.append(a[2])
        torch.manual_seed(77 + len(calls))
        return image_test(*a, **k)
    monkeypatch.setattr(E, "image_test", seeded)
    vae = pc.build_image_vae(dev, 8)
    q = list(epss)
    loop = ImageTrainingLoop(vae, xs, xs[:4], None, args, log=lambda *a: None, order_fn=order_fn, binarize_fn=binarize_fn,
                             eps_fn=lambda x: q.pop(0).to(dev))
    assert (loop.trainer.objective, loop.trainer.iw_estimator) == ("iw", "dreg")
    klw, rate, batches = loop.kl_weight, loop.anneal_rate, [binarize_fn(p) for p, _ in loop.train_loader]
    out = loop.run()
    assert not q and out["epochs"] == 2 and calls == ["VAL", "VAL"]
    vae2 = pc.build_image_vae(dev, 8)
    tr = _image_trainer(vae2, lr=1e-3, clip=5.0, nsamples=2, objective="iw", iw_estimator="dreg")
    vals = []
    for ep in range(2):
        for xb, e in zip(batches, epss[2 * ep:2 * ep + 2]):
            klw = min(1.0, klw + rate)
            tr.step(xb, klw, eps=e.to(dev), update="both")
        vae2.eval()
        with torch.no_grad():                                             # the validation pass of every objective: VAE.loss, by hand
            torch.manual_seed(77 + ep + 1)
            vals.append(image_test(vae2, loop.val_loader, "VAL", _loop_args(), verbose=False))
        vae2.train()
    for h, v in zip(out["history"], vals):                                 # equal weights and the same evaluation: equal figures
        assert (h["loss"], h["nll"], h["kl"]) == tuple(v)


@pytest.mark.gpu
def test_second_step_allocates_no_new_iw_buffer(gpu):
    _, dev = gpu
    vae = pc.build_image_vae(dev, 11)
    tr = _image_trainer(vae, nsamples=2, objective="iw", iw_estimator="dreg")
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(3, 1, 28, 28, generator=g) < 0.4).float().to(dev)
    tr.step(x, 0.6)
    ptrs = tuple(t.data_ptr() for t in tr._iw_state[3])
    first = tr.logw.clone()
    tr.step(x, 0.6)
    assert list(tr._iw_state) == [3] and tuple(t.data_ptr() for t in tr._iw_state[3]) == ptrs and tr.logw is tr._iw_state[3][2]
    assert not torch.equal(first, tr.logw)                                 # the last step's values, in the same buffer


@pytest.mark.gpu
def test_decoder_backward_can_be_repeated_on_retained_activations(gpu):
    """ImageDecoderEngine.backward(seeds, retain=True) leaves the tape usable: a pass with other seeds in between changes nothing of
    what the final pass writes -- dz and every parameter gradient have the bits of a single backward."""
    _, dev = gpu
    B, ns = 3, 2
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(B, 1, 28, 28, generator=g) < 0.4).float().to(dev)
    z = torch.randn(B * ns, 32, generator=g).to(dev)
    seeds, other = torch.rand(B * ns, generator=g).to(dev), torch.rand(B * ns, generator=g).to(dev)
    out = []
    for twice in (False, True):
        vae = pc.build_image_vae(dev, 13)
        vae.train()
        eng = vae.decoder._hip
        eng.ensure(dev)
        eng.flat.attach_grads()
        eng.forward(x, z, ns)
        if twice:
            dz_other = eng.backward(other, retain=True).clone()
            assert eng.tape.back and not eng.tape.grads
        dz = eng.backward(seeds)
        assert not eng.tape.back                                           # the last pass releases the activations
        out.append((dz.clone(), eng.flat.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert not torch.equal(dz_other, out[0][0])

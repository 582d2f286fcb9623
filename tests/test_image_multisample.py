"""Multi-sample training on the Omniglot path (image.py --nsamples N: VAE.loss(x, kl_weight, nsamples=N)) in the fused image trainer:
the ns-aware edge kernels against torch one-liners and their ns = 1 twins, the finish-then-apply BatchNorm (producers' partial rows at
any row count) against float64 torch, AggressiveImageTrainer(nsamples=N) against reference fixtures
(tests/golden/make_golden_image_multisample.py), against itself on the other BatchNorm route, through a captured hipGraph, with
device-drawn noise, against the drop-in route on the same tree, and ImageTrainingLoop with args.nsamples.
Emulator (`not gpu`) and MI355X (`gpu`)."""
import argparse

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity_common as pc
from helpers import load, rel_err
from parity_common import RTOL
from vae_lagging_encoder_amd import engine as _eng
from vae_lagging_encoder_amd.engine import P


@pytest.fixture(scope="module", params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def target(request):
    if request.param == "emu":
        request.getfixturevalue("emu_backend")
        dev = torch.device("cpu")
    else:
        dev = request.getfixturevalue("hip_device")
    return _eng.backend_for(dev), dev


@pytest.fixture
def gpu(request):
    """For the cases that run on the MI355X only (each of them marked gpu)."""
    dev = request.getfixturevalue("hip_device")
    return _eng.backend_for(dev), dev


def _trainer(*a, **k):
    from vae_lagging_encoder_amd.trainer import AggressiveImageTrainer
    return AggressiveImageTrainer(*a, **k)


# ---------------------------------------------------------------------------------------------------------------------
# 1. edge kernels: bit-exact against torch one-liners and against the ns = 1 twins on an explicitly repeated x
EDGE_SIZES = [(1, 1, 784, 4), (3, 2, 784, 4), (2, 5, 784, 1), (4, 3, 17, 4), (7, 2, 1, 2)]          # B, ns, npix, fm


@pytest.mark.parametrize("B,ns,npix,fm", EDGE_SIZES)
def test_dec_input_ns_bit_exact(target, B, ns, npix, fm):
    lib, dev = target
    s = _eng.stream_ptr(dev)
    g = torch.Generator().manual_seed(B * 100 + ns * 10 + fm)
    x = (torch.rand(B, npix, generator=g) < 0.4).float()
    zt = torch.randn(B * ns, fm * npix, generator=g)
    in5 = torch.full((B * ns * npix, 1 + fm), float("nan"), device=dev)
    xd, ztd = x.to(dev), zt.to(dev)
    lib.lv_dec_input_ns_fwd_f32(P(xd), P(ztd), P(in5), B, ns, npix, fm, s)
    want = torch.cat([x.repeat_interleave(ns, dim=0).view(B * ns, 1, npix), zt.view(B * ns, fm, npix)], dim=1)      # NCHW ...
    want = want.permute(0, 2, 1).reshape(B * ns * npix, 1 + fm)                                                      # ... as NHWC
    assert torch.equal(in5.cpu(), want)
    if ns == 1:
        twin = torch.full_like(in5, float("nan"))
        lib.lv_dec_input_fwd_f32(P(xd), P(ztd), P(twin), B, npix, fm, s)
        assert torch.equal(twin.cpu(), in5.cpu())
    # the backward is the twin's with B := B * ns
    dzt = torch.full((B * ns, fm * npix), float("nan"), device=dev)
    lib.lv_dec_input_bwd_f32(P(in5), P(dzt), B * ns, npix, fm, s)
    assert torch.equal(dzt.cpu(), zt)


@pytest.mark.parametrize("B,ns,npix,fm", EDGE_SIZES)
def test_sigmoid_bce_ns_bit_exact(target, B, ns, npix, fm):
    lib, dev = target
    s = _eng.stream_ptr(dev)
    g = torch.Generator().manual_seed(B * 7 + ns * 3 + npix)
    Bd = B * ns
    logit = (torch.randn(Bd, npix, generator=g) * 3).to(dev)
    x = (torch.rand(B, npix, generator=g) < 0.4).float().to(dev)
    xrep = x.repeat_interleave(ns, dim=0).contiguous()
    drec = torch.randn(Bd, generator=g).to(dev)
    rec = torch.full((Bd,), float("nan"), device=dev)
    rec_t = torch.full((Bd,), float("nan"), device=dev)
    lib.lv_sigmoid_bce_ns_fwd_f32(P(logit), P(x), P(rec), B, ns, npix, 1e-12, s)
    lib.lv_sigmoid_bce_fwd_f32(P(logit), P(xrep), P(rec_t), Bd, npix, 1e-12, s)
    assert torch.equal(rec.cpu(), rec_t.cpu())
    p = torch.sigmoid(logit.cpu().double())
    want = -(torch.log(p + 1e-12) * xrep.cpu().double() + torch.log(1 - p + 1e-12) * (1 - xrep.cpu().double())).sum(1)
    assert rel_err(rec, want) < 1e-5
    dl = torch.full((Bd, npix), float("nan"), device=dev)
    dl_t = torch.full((Bd, npix), float("nan"), device=dev)
    lib.lv_sigmoid_bce_ns_bwd_f32(P(logit), P(x), P(drec), P(dl), B, ns, npix, 1e-12, s)
    lib.lv_sigmoid_bce_bwd_f32(P(logit), P(xrep), P(drec), P(dl_t), Bd, npix, 1e-12, s)
    assert torch.equal(dl.cpu(), dl_t.cpu())
    if ns == 1:          # (xrep is x: the twin on the very same buffers)
        lib.lv_sigmoid_bce_fwd_f32(P(logit), P(x), P(rec_t), B, npix, 1e-12, s)
        assert torch.equal(rec.cpu(), rec_t.cpu())


def test_image_multisample_kernels_refuse_bad_arguments(target):
    lib, dev = target
    t = torch.zeros(256, device=dev)
    raw = lambda name: getattr(lib, "_raw_" + name)
    assert raw("lv_dec_input_ns_fwd_f32")(None, P(t), P(t), 1, 1, 4, 1, None) < 0
    assert raw("lv_dec_input_ns_fwd_f32")(P(t), P(t), P(t), 1, 0, 4, 1, None) < 0
    assert raw("lv_dec_input_ns_fwd_f32")(P(t), P(t), P(t), 0, 1, 4, 1, None) < 0
    assert raw("lv_sigmoid_bce_ns_fwd_f32")(P(t), P(t), None, 1, 1, 4, 1e-12, None) < 0
    assert raw("lv_sigmoid_bce_ns_fwd_f32")(P(t), P(t), P(t), 1, 0, 4, 1e-12, None) < 0
    assert raw("lv_sigmoid_bce_ns_bwd_f32")(P(t), None, P(t), P(t), 1, 1, 4, 1e-12, None) < 0
    assert raw("lv_sigmoid_bce_ns_bwd_f32")(P(t), P(t), P(t), P(t), 1, 1, 0, 1e-12, None) < 0
    m = (P(t),) * 2
    assert raw("lv_bn_finish_fwd_f32")(None, 1, 4, 32, 1e-5, 0.1, *m, *m, None) < 0
    assert raw("lv_bn_finish_fwd_f32")(P(t), 0, 4, 32, 1e-5, 0.1, *m, *m, None) < 0                 # no rows
    assert raw("lv_bn_finish_fwd_f32")(P(t), 1, 4, 24, 1e-5, 0.1, *m, *m, None) < 0                 # C not a power of two
    assert raw("lv_bn_finish_fwd_f32")(P(t), 1, 4, 32, 1e-5, 0.1, *m, P(t), None, None) < 0         # one running statistic only
    assert raw("lv_bn_finish_fwd_f32")(P(t, 1), 1, 4, 32, 1e-5, 0.1, *m, *m, None) < 0              # misaligned rows
    assert raw("lv_bn_fwd_stats_f32")(P(t), P(t), P(t), None, 1, None, *m, 4, 32, None) < 0
    assert raw("lv_bn_fwd_stats_f32")(P(t), P(t), P(t), None, 1, P(t), *m, 0, 32, None) < 0
    assert raw("lv_bn_finish_bwd_f32")(P(t), 1, 32, None, *m, 0, None) < 0
    assert raw("lv_bn_finish_bwd_f32")(P(t), -3, 32, P(t), *m, 0, None) < 0
    assert raw("lv_bn_bwd_stats_f32")(P(t), P(t), P(t), *m, P(t), None, 4, 32, None) < 0
    assert raw("lv_bn_bwd_stats_f32")(P(t), P(t), P(t), *m, P(t), P(t), 4, 12, None) < 0
    assert lib.lv_bn_partial_floats(3000, 32) == 3000 * 64 and lib.lv_bn_partial_floats(1025, 64) == 1025 * 128


# ---------------------------------------------------------------------------------------------------------------------
# 2. finish-then-apply BatchNorm at the kernel level: synthetic x [P][C] cut into nblk chunks, partial rows computed on the host,
#    against float64 torch within the bounds of tests/test_gpu_kernels.py::test_batchnorm_train_fwd_bwd
def _chunks(Pn, nblk):
    cuts = np.linspace(0, Pn, nblk + 1).astype(np.int64)
    return [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])]


@pytest.mark.parametrize("use_res,act", [(True, True), (False, False)])
@pytest.mark.parametrize("nblk", [1, 7, 1024, 1025, 3000])
@pytest.mark.parametrize("C", [32, 64])
def test_bn_finish_then_apply(target, C, nblk, use_res, act):
    lib, dev = target
    s = _eng.stream_ptr(dev)
    Pn = nblk + 37                                   # every chunk holds a row; chunk lengths differ (1 or 2 rows at the large counts)
    g = torch.Generator().manual_seed(C * 10000 + nblk)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    rmd, rvd = rm0.clone().to(dev), rv0.clone().to(dev)
    rm, rv = rm0.double().clone(), rv0.double().clone()
    gd, bd = gamma.to(dev), beta.to(dev)
    rows = int(lib.lv_bn_partial_floats(nblk, C))
    ws = torch.empty(rows + 4 * 2 * C, device=dev)                       # four rows past the end: never read
    ch = _chunks(Pn, nblk)
    for rnd in range(2):                                                 # a second launch on changed data: a stale row cannot pass
        x = torch.randn(Pn, C, generator=g) * (2 + rnd) + 0.5 - rnd
        res = torch.randn(Pn, C, generator=g)
        dv = torch.randn(Pn, C, generator=g)
        x64 = x.double().requires_grad_(True)
        g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        xn = F.batch_norm(x64.t().reshape(1, C, Pn), rm, rv, g64, b64, True, 0.1, 1e-5).reshape(C, Pn).t()      # (updates rm, rv)
        y_ref = xn + res.double() if use_res else xn
        if act:
            y_ref = F.elu(y_ref)
        (xn * dv.double()).sum().backward()                              # dv: the gradient at the BatchNorm's own output
        part = torch.stack([torch.stack([x[a:b].double().sum(0), (x[a:b].double() ** 2).sum(0)]) for a, b in ch]).float()      # [nblk][2][C]
        ws.fill_(float("nan"))
        ws[:rows].copy_(part.reshape(-1).to(dev))
        xd, resd, dvd = x.to(dev), res.to(dev), dv.to(dev)
        mean = torch.full((C,), float("nan"), device=dev)
        invstd = torch.full((C,), float("nan"), device=dev)
        y = torch.full((Pn, C), float("nan"), device=dev)
        lib.lv_bn_finish_fwd_f32(P(ws), nblk, Pn, C, 1e-5, 0.1, P(mean), P(invstd), P(rmd), P(rvd), s)
        lib.lv_bn_fwd_stats_f32(P(xd), P(gd), P(bd), P(resd) if use_res else None, int(act), P(y), P(mean), P(invstd), Pn, C, s)
        m64, v64 = x.double().mean(0), x.double().var(0, unbiased=False)
        assert float((mean.cpu().double() - m64).abs().max()) < 1e-5
        assert float((invstd.cpu().double() - (v64 + 1e-5).rsqrt()).abs().max()) < 1e-5 * float((v64 + 1e-5).rsqrt().max())
        assert float((y.cpu().double() - y_ref.detach()).abs().max()) < 2e-5
        assert float((rmd.cpu().double() - rm).abs().max()) < 1e-5 and float((rvd.cpu().double() - rv).abs().max()) < 1e-4
        # backward: rows of (sum dv, sum dv * xhat) with the statistics the forward saved
        xh = (x.double() - mean.cpu().double()) * invstd.cpu().double()
        bpart = torch.stack([torch.stack([dv[a:b].double().sum(0), (dv[a:b].double() * xh[a:b]).sum(0)]) for a, b in ch]).float()
        ws.fill_(float("nan"))
        ws[:rows].copy_(bpart.reshape(-1).to(dev))
        sums = torch.full((2 * C,), float("nan"), device=dev)
        dg = torch.full((C,), 0.25, device=dev)
        db = torch.full((C,), -0.5, device=dev)
        dx = torch.full((Pn, C), float("nan"), device=dev)
        acc = rnd                                                        # first round: =, second round: +=
        lib.lv_bn_finish_bwd_f32(P(ws), nblk, C, P(sums), P(dg), P(db), acc, s)
        lib.lv_bn_bwd_stats_f32(P(xd), P(dvd), P(sums), P(mean), P(invstd), P(gd), P(dx), Pn, C, s)
        assert float((dx.cpu().double() - x64.grad).abs().max()) < 2e-4 * float(x64.grad.abs().max())
        assert float((dg.cpu().double() - 0.25 * acc - g64.grad).abs().max()) < 2e-4 * float(g64.grad.abs().max())
        assert float((db.cpu().double() + 0.5 * acc - b64.grad).abs().max()) < 2e-4 * float(b64.grad.abs().max())
        assert float((sums[:C].cpu().double() - b64.grad).abs().max()) < 2e-4 * float(b64.grad.abs().max())
        # ... and the single-launch entries give the same results on the same rows where they accept them
        if nblk <= 1024:
            y1 = torch.empty_like(y)
            m1, i1 = torch.empty_like(mean), torch.empty_like(invstd)
            ws[:rows].copy_(part.reshape(-1).to(dev))
            lib.lv_bn_fwd_partials_f32(P(xd), P(gd), P(bd), P(resd) if use_res else None, int(act), P(y1), P(m1), P(i1), None, None, 1e-5,
                                       0.1, P(ws), nblk, Pn, C, s)
            assert float((y1 - y).abs().max()) < 1e-5 and rel_err(m1, mean, floor=1e-6) < 1e-5 and rel_err(i1, invstd) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# fixtures
def _fixture(name):
    """The stacked per-tensor records of make_golden_image_multisample.py as the keys parity_common._check_image_outputs reads."""
    fx = load(name)
    d = {k: fx[k] for k in fx.files}
    for i, k in enumerate(str(n) for n in fx["names"]):
        d["gradnorm/" + k] = fx["gradnorm"][i]
        for f in ("sample_idx", "sample_grad", "sample_p0", "sample_new"):
            d[f + "/" + k] = fx[f][i]
    for i, k in enumerate(str(n) for n in fx["stat_names"]):
        d["stat/" + k] = fx["stat"][i]
    return d


def _unclipped_grads(tr):
    """The step wrote every gradient back clipped (g * coef): the raw ones, by name."""
    coef = tr.read_stats()["coef"]
    out = {}
    for pre, eng in (("encoder.", tr.enc), ("decoder.", tr.dec)):
        for n in eng.flat.names:
            out[pre + n] = eng.flat.gviews[n].detach().clone() / coef
    return out


def _fused_step_against_fixture(name, dev, precision="f32", use_graph=False, rtol=RTOL, norm_tol=5e-4, upd_tol=2e-5, full=True, caps=None):
    fx = _fixture(name)
    B, ns = int(fx["B"]), int(fx["ns"])
    vae = pc.build_image_vae(dev, int(fx["model_seed"]))
    tr = _trainer(vae, lr=1e-3, clip=5.0, use_graph=use_graph, precision=precision, nsamples=ns)
    if caps is not None:
        tr.enc.bn_partial_cap = tr.dec.bn_partial_cap = caps
    x = torch.from_numpy(fx["x"]).float().to(dev)
    eps = torch.from_numpy(fx["eps"]).to(dev)
    assert tuple(eps.shape) == (B, ns, 32)
    tr.step(x, float(fx["kl_weight"]), eps=eps)
    st = tr.read_stats()
    errs = dict(loss=abs(st["loss_sum"] - float(fx["loss"].sum())) / abs(float(fx["loss"].sum())),
                rec=abs(st["rec_sum"] - float(fx["rec"].sum())) / abs(float(fx["rec"].sum())),
                kl=abs(st["kl_sum"] - float(fx["kl"].sum())) / abs(float(fx["kl"].sum())),
                norm=abs(st["norm"] - float(fx["total_norm64"])) / float(fx["total_norm64"]), upd=0.0)
    print(name, precision, "graph" if use_graph else "eager", errs)
    assert errs["loss"] < rtol and errs["rec"] < rtol and errs["kl"] < rtol and errs["norm"] < norm_tol, errs
    sd = vae.state_dict()
    for k, _ in vae.named_parameters():
        idx = torch.from_numpy(fx["sample_idx/" + k])
        got = sd[k].reshape(-1)[idx].cpu()
        p0 = torch.from_numpy(fx["sample_p0/" + k])
        if k.startswith("encoder."):          # Adam's first step moves every weight by ~lr: compare the UPDATE
            e = float(((got - p0) - (torch.from_numpy(fx["sample_new/" + k]) - p0)).abs().max())
            errs["upd"] = max(errs["upd"], e)
            assert e < upd_tol, (k, e)
        else:                                 # decoder untouched except MaskedConv2d's in-place weight masking
            assert bool(((got == p0) | (got == 0)).all()), k
    if full:
        # The project's own bounds on the clip norm, the per-tensor gradient norms, the sampled gradient entries and the running
        # statistics.  The fused trainer keeps no per-image loss / rec / KL rows (their sums were checked above), so the fixture's own
        # rows are handed in: the helper's three row comparisons hold trivially here and check nothing.
        rows = [torch.from_numpy(fx[k]) for k in ("loss", "rec", "kl")]
        pc._check_image_outputs(fx, vae, rows[0], rows[1], rows[2], _unclipped_grads(tr), st["norm"])
    return errs, tr


@pytest.fixture(scope="module")
def default_route_b6_ns3(target):
    """The b6_ns3 step on the default BatchNorm route, checked against the reference fixture on the way: run once per target, and
    what it left (report scalars, updated encoder weights, launch counters) is shared by the tests below, which do not modify it."""
    lib, dev = target
    _, tr = _fused_step_against_fixture("image_ms_b6_ns3", dev)
    return dict(stats=tr.read_stats(), enc=tr.enc.flat.data.detach().clone(), dec_launches=dict(tr.dec.launches),
                enc_launches=dict(tr.enc.launches))


def test_fused_step_b6_ns3_against_reference(default_route_b6_ns3):
    r = default_route_b6_ns3                  # (the comparison with the reference is the fixture's own; it fails this test)
    assert r["dec_launches"] == {"bn_finish_fwd": 0, "bn_finish_bwd": 0}          # 18 images: the partial rows fit the one-launch route


LARGE = [("image_ms_b37_ns2", 74, False), ("image_ms_b42_ns5", 210, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("name,N,pointwise_too", LARGE)
def test_fused_step_past_the_partial_row_cap_against_reference(gpu, name, N, pointwise_too, precision):
    lib, dev = gpu
    assert lib.lv_conv32_blocks(N) > 1024                        # the masked convolutions leave more rows than one apply launch totals
    assert (lib.lv_conv1x1_blocks(784 * N) > 1024) == pointwise_too
    _, tr = _fused_step_against_fixture(name, dev, precision=precision)
    assert tr.dec.launches["bn_finish_fwd"] >= (70 if pointwise_too else 23) and tr.dec.launches["bn_finish_bwd"] >= 23, tr.dec.launches


@pytest.mark.gpu
@pytest.mark.parametrize("name,N,pointwise_too", LARGE)
def test_fused_step_past_the_partial_row_cap_bf16_contract(gpu, name, N, pointwise_too):
    """precision="bf16" at the bounds tests/test_gpu_parity.py::test_image_step_bf16_convolutions_contract states."""
    lib, dev = gpu
    assert lib.lv_conv32_blocks(N) > 1024 and (lib.lv_conv1x1_blocks(784 * N) > 1024) == pointwise_too
    e, _ = _fused_step_against_fixture(name, dev, precision="bf16", rtol=1e-2, norm_tol=2e-2, upd_tol=2.1e-3, full=False)
    assert e["loss"] < 1e-3, e


def test_trajectory_against_reference(target):
    """Two encoder-only steps and one update="both" step on three batches: per-step loss / rec / KL sums, clip norms, and the
    accumulated update of sampled weights of both halves (Adam moves every weight by ~lr per step whatever the gradient's size: the
    bound is check_image_inner_loop's, 5 % of lr per step a tensor was stepped)."""
    lib, dev = target
    fx = load("image_ms_traj_b6_ns3")
    B, ns = int(fx["B"]), int(fx["ns"])
    vae = pc.build_image_vae(dev, int(fx["model_seed"]))
    tr = _trainer(vae, lr=1e-3, clip=5.0, nsamples=ns)
    updates = [str(u) for u in fx["updates"]]
    for i, upd in enumerate(updates):
        tr.reset_stats()
        tr.step(torch.from_numpy(fx["x"][i]).float().to(dev), float(fx["kl_weight"]), eps=torch.from_numpy(fx["eps"][i]).to(dev), update=upd)
        st = tr.read_stats()
        for k in ("loss", "rec", "kl"):
            e = abs(st[k + "_sum"] - float(fx[k + "_sum"][i])) / abs(float(fx[k + "_sum"][i]))
            assert e < RTOL, (i, k, e)
        en = abs(st["norm"] - float(fx["total_norm64"][i])) / float(fx["total_norm64"][i])
        assert en < 5e-4, (i, en)
    sd = vae.state_dict()
    for j, k in enumerate(str(n) for n in fx["names"]):
        steps = sum(1 for u in updates if u == "both" or k.startswith("encoder."))
        idx = torch.from_numpy(fx["sample_idx"][j])
        p0 = torch.from_numpy(fx["sample_p0"][j])
        got = sd[k].reshape(-1)[idx].cpu()
        ref = torch.from_numpy(fx["sample_new"][j])
        live = got != 0                                                    # (MaskedConv2d re-zeroes its masked taps on the next forward)
        assert float(((got - p0) - (ref - p0))[live].abs().max() if bool(live.any()) else 0.0) < 0.05 * 1e-3 * steps + 1e-7, k


# ---------------------------------------------------------------------------------------------------------------------
# 3. the same step on both BatchNorm routes
def test_same_step_on_both_batchnorm_routes(target, default_route_b6_ns3):
    lib, dev = target
    r0 = default_route_b6_ns3
    (e1, tr1) = _fused_step_against_fixture("image_ms_b6_ns3", dev, full=True, caps=0)
    assert r0["dec_launches"] == {"bn_finish_fwd": 0, "bn_finish_bwd": 0} and r0["enc_launches"] == r0["dec_launches"]
    # every BatchNorm behind a fused producer finishes its statistics in a launch of its own: 23 blocks x 3 + the head, and the backward
    # of every one whose output has the one reader
    assert tr1.dec.launches["bn_finish_fwd"] == 70 and tr1.dec.launches["bn_finish_bwd"] >= 46, tr1.dec.launches
    s0, s1 = r0["stats"], tr1.read_stats()
    for k in ("loss_sum", "rec_sum", "kl_sum", "norm"):
        assert abs(s0[k] - s1[k]) / abs(s0[k]) < RTOL, (k, s0[k], s1[k])
    assert float((tr1.enc.flat.data - r0["enc"]).abs().max()) < 2e-5
    # bn_partial_cap = inf: past 1024 rows the fusions are dropped, as before this route existed -- nothing finishes, nothing breaks
    vae = pc.build_image_vae(dev, 3)
    tr = _trainer(vae, nsamples=1)
    tr.dec.bn_partial_cap = float("inf")
    assert vae.decoder._hip is tr.dec
    from vae_lagging_encoder_amd.image_engine import Tape
    tp = Tape(dev, bn_partial_cap=float("inf"))
    assert [tp._bn_route(n) for n in (0, 1, 1024, 1025, 5000)] == [None, "totals", "totals", None, None]
    tp = Tape(dev)
    assert [tp._bn_route(n) for n in (0, 1, 1024, 1025, 5000)] == [None, "totals", "totals", "finish", "finish"]
    tp = Tape(dev, bn_partial_cap=0)
    assert [tp._bn_route(n) for n in (0, 1, 1025)] == [None, "finish", "finish"]


# ---------------------------------------------------------------------------------------------------------------------
# 5. hipGraph
@pytest.mark.gpu
def test_hipgraph_replay_equals_eager_ns3(gpu):
    lib, dev = gpu
    fx = load("image_ms_b6_ns3")
    x = torch.from_numpy(fx["x"]).float().to(dev)
    eps = torch.from_numpy(fx["eps"]).to(dev)
    res = []
    for use_graph in (False, True):
        vae = pc.build_image_vae(dev, int(fx["model_seed"]))
        tr = _trainer(vae, use_graph=use_graph, nsamples=3)
        for _ in range(3):
            tr.step(x, 0.5, eps=eps)
        res.append(({k: v.clone() for k, v in vae.state_dict().items()}, tr.read_stats()))
        if use_graph:
            assert [k[:2] for k in tr._static] == [(6, 3)] and tr._static[(6, 3, "encoder", False, True)]["eps"].shape == (6, 3, 32)
    for k in res[0][0]:
        assert rel_err(res[1][0][k].float(), res[0][0][k].float(), floor=1e-12) < 1e-5, k
    assert abs(res[0][1]["loss_sum"] - res[1][1]["loss_sum"]) / abs(res[0][1]["loss_sum"]) < 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# 6. device-drawn noise
def _run_steps(dev, steps, B=4, **kw):
    vae = pc.build_image_vae(dev, 11)
    tr = _trainer(vae, seed=4242, **kw)
    g = torch.Generator().manual_seed(3)
    for i in range(steps):
        x = (torch.rand(B, 1, 28, 28, generator=g) < 0.4).float().to(dev)
        tr.step(x, 0.6, update="both" if i == steps - 1 else "encoder")
    return {k: v.clone() for k, v in vae.state_dict().items()}, tr.scal.clone(), tr.rng_state.clone()


@pytest.mark.gpu
def test_device_drawn_noise_is_reproducible_ns3(gpu):
    lib, dev = gpu
    a, b = _run_steps(dev, 2, nsamples=3), _run_steps(dev, 2, nsamples=3)
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert a[2].cpu().tolist() == [4242, 2]                                 # one lv_rng_advance of 1 per step
    assert float(a[1][7]) > 0 and bool(torch.isfinite(a[1]).all())


@pytest.mark.gpu
def test_nsamples_1_through_the_argument_keeps_the_bits(gpu):
    lib, dev = gpu
    a, b = _run_steps(dev, 3, B=3), _run_steps(dev, 3, B=3, nsamples=1)
    for k in a[0]:
        assert torch.equal(a[0][k], b[0][k]), k
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


# ---------------------------------------------------------------------------------------------------------------------
# 7. against the drop-in route on the same tree
@pytest.mark.gpu
def test_fused_ns3_against_dropin_route(gpu):
    lib, dev = gpu
    B, ns = 6, 3
    g = torch.Generator().manual_seed(12)
    x = (torch.rand(B, 1, 28, 28, generator=g) < 0.4).float().to(dev)
    eps = torch.randn(B, ns, 32, generator=g).to(dev)
    vae = pc.build_image_vae(dev, 21)
    for p in vae.parameters():
        p.grad = None
    loss, rec, kl = vae.loss(x, 0.7, nsamples=ns, noise=(eps, None, None))
    loss.mean(dim=-1).backward()
    grads = {k: p.grad.detach().clone() for k, p in vae.named_parameters()}
    total = float(torch.nn.utils.clip_grad_norm_(vae.parameters(), 5.0))
    vae2 = pc.build_image_vae(dev, 21)
    tr = _trainer(vae2, nsamples=ns)
    tr.step(x, 0.7, eps=eps)
    st = tr.read_stats()
    assert abs(st["loss_sum"] - float(loss.sum())) / abs(float(loss.sum())) < RTOL
    assert abs(st["rec_sum"] - float(rec.sum())) / abs(float(rec.sum())) < RTOL
    assert abs(st["kl_sum"] - float(kl.sum())) / abs(float(kl.sum())) < RTOL
    assert abs(st["norm"] - total) / total < 5e-4
    for k, gv in _unclipped_grads(tr).items():
        ref_n = float(grads[k].double().norm())
        assert abs(float(gv.double().norm()) - ref_n) <= 2e-3 * ref_n + 1e-7, k


# ---------------------------------------------------------------------------------------------------------------------
# 8. host contract
def test_host_contract_refuses_before_a_launch(target):
    lib, dev = target
    vae = pc.build_image_vae(dev, 5)
    for bad in (0, -1, 1.5, "2", True):
        with pytest.raises(ValueError):
            _trainer(vae, nsamples=bad)
    tr = _trainer(vae, nsamples=2)
    x = torch.zeros(3, 1, 28, 28, device=dev)
    before = (tr.scal.clone(), tr.rng_state.clone(), tr.enc.flat.data.clone(), tr.enc.gen, tr.dec.gen)
    for shape in ((3, 1, 32), (3, 32), (3, 2, 31), (6, 32), (2, 2, 32), (3, 2, 32, 1)):
        with pytest.raises(ValueError):
            tr.step(x, 1.0, eps=torch.zeros(*shape, device=dev))
    assert torch.equal(tr.scal, before[0]) and torch.equal(tr.rng_state, before[1]) and torch.equal(tr.enc.flat.data, before[2])
    assert (tr.enc.gen, tr.dec.gen) == before[3:]                           # no forward ran
    with pytest.raises(ValueError):
        tr.dec.forward(x, torch.zeros(3, 32, device=dev), 2)                # 3 rows of z for 3 images x 2 samples


def _loop_args(**kw):
    d = dict(kl_start=0.1, warm_up=2, batch_size=4, epochs=1, aggressive=0, nsamples=2, test_nepoch=5)
    d.update(kw)
    return argparse.Namespace(**d)


def test_image_training_loop_reads_nsamples(target):
    lib, dev = target
    from vae_lagging_encoder_amd.training import ImageTrainingLoop
    vae = pc.build_image_vae(dev, 6)
    g = torch.Generator().manual_seed(1)
    xs = torch.rand(8, 1, 28, 28, generator=g)
    loop = ImageTrainingLoop(vae, xs, xs[:4], None, _loop_args(), log=lambda *a: None)
    assert loop.trainer.nsamples == 2
    with pytest.raises(ValueError, match="args.nsamples = 2, but the trainer was built with nsamples = 3"):
        ImageTrainingLoop(vae, xs, xs[:4], None, _loop_args(), trainer=_trainer(vae, nsamples=3))
    with pytest.raises(ValueError, match="nsamples = 1"):
        ImageTrainingLoop(vae, xs, xs[:4], None, _loop_args(), trainer=_trainer(vae))
    assert ImageTrainingLoop(vae, xs, xs[:4], None, _loop_args(nsamples=1), trainer=_trainer(vae)).trainer.nsamples == 1


@pytest.mark.gpu
def test_one_epoch_of_the_loop_takes_the_hand_driven_steps(gpu):
    """One short non-aggressive epoch (two batches of 4, nsamples = 2) with injected order, binarisation and eps: the loop's weights
    equal those of a trainer stepped by hand on the same batches, bit for bit.  (MI355X only, like the device-drawn-noise and drop-in
    comparisons above: a whole training step takes minutes on the thread-level emulator, which already runs the b6_ns3 fixture, the
    trajectory and the two-route comparison; the loop's wiring of args.nsamples is covered there by
    test_image_training_loop_reads_nsamples.)"""
    lib, dev = gpu
    from vae_lagging_encoder_amd.training import ImageTrainingLoop
    g = torch.Generator().manual_seed(2)
    xs = torch.rand(8, 1, 28, 28, generator=g).to(dev)
    epss = [torch.randn(4, 2, 32, generator=g) for _ in range(2)]
    order_fn = lambda n: np.arange(n)
    binarize_fn = lambda probs: (probs.to(dev) > 0.5).float()
    args = _loop_args(epochs=1, test_nepoch=99)
    vae = pc.build_image_vae(dev, 8)
    q = list(epss)
    seen = []

    def eps_fn(x):
        seen.append(tuple(x.shape))
        return q.pop(0).to(dev)
    loop = ImageTrainingLoop(vae, xs, xs[:4], None, args, log=lambda *a: None, order_fn=order_fn, binarize_fn=binarize_fn, eps_fn=eps_fn)
    klw, rate, batches = loop.kl_weight, loop.anneal_rate, [binarize_fn(p) for p, _ in loop.train_loader]
    loop.run()
    assert seen == [(4, 1, 28, 28)] * 2 and not q
    vae2 = pc.build_image_vae(dev, 8)
    tr = _trainer(vae2, lr=1e-3, clip=5.0, nsamples=2)
    for xb, e in zip(batches, epss):
        klw = min(1.0, klw + rate)
        tr.step(xb, klw, eps=e.to(dev), update="both")
    sd, sd2 = vae.state_dict(), vae2.state_dict()
    for k in sd2:
        if k.endswith("num_batches_tracked") or k.endswith(".mask"):
            continue
        # (the loop's evaluation passes re-applied MaskedConv2d's in-place weight masking after the last update: compare under the mask)
        m = sd2.get(k[:-len("weight")] + "mask", 1.0) if k.endswith(".weight") else 1.0
        assert torch.equal(sd[k] * m, sd2[k] * m), k
    assert [it["n"] for it in loop.iterations] == [4, 4]

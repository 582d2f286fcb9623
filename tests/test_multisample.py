"""Multi-sample training (text.py --nsamples N: VAE.loss(x, kl_weight, nsamples=N)) on the fused path: the kernels of
csrc/lv_multisample.hip against torch one-liners, AggressiveTextTrainer(nsamples=N) against reference fixtures
(tests/golden/make_golden_multisample.py) and against the drop-in route on the same tree, device-drawn noise, transactional
recovery, steady-state behaviour, the fences, and TextTrainingLoop with args.nsamples.  Emulator (`not gpu`) and MI355X (`gpu`)."""
import argparse
import math

import numpy as np
import pytest
import torch

from helpers import ALL_KEYS, DEC_KEYS, ENC_KEYS, build_vae, load, rel_err
from oracle import text_vae_oracle as O
from parity_common import GRAD_RTOL, RTOL
from vae_lagging_encoder_amd import engine as _eng
from vae_lagging_encoder_amd.engine import P


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
# 1. kernel contracts
SIZES = [(1, 1, 1, 5), (3, 2, 2, 12), (4, 3, 3, 7), (2, 5, 4, 64), (5, 1, 5, 1030), (1, 4, 2, 1), (7, 2, 3, 24)]      # Td, B, ns, C


@pytest.mark.parametrize("Td,B,ns,C", SIZES)
def test_gx_expand_add_and_repeat_rows_bit_exact(target, Td, B, ns, C):
    lib, dev = target
    s = _eng.stream_ptr(dev)
    g = torch.Generator().manual_seed(Td * 1000 + C)
    gxw = torch.randn(Td, B, C, generator=g).to(dev)
    zp = torch.randn(B * ns, C, generator=g).to(dev)
    gx = torch.full((Td, B * ns, C), float("nan"), device=dev)
    lib.lv_gx_expand_add_f32(P(gxw), P(zp), P(gx), Td, B, ns, C, s)
    want = (gxw.view(Td, B, 1, C) + zp.view(1, B, ns, C)).reshape(Td, B * ns, C)
    assert torch.equal(gx.cpu(), want.cpu())
    T = Td + 1
    x = torch.randint(0, 1 << 40, (B, T), generator=g, dtype=torch.int64).to(dev)
    xr = torch.full((B * ns, T), -1, dtype=torch.int64, device=dev)
    lib.lv_repeat_rows_i64(P(x), P(xr), B, T, ns, s)
    assert torch.equal(xr.cpu(), x.repeat_interleave(ns, dim=0).cpu())


@pytest.mark.parametrize("Td,B,ns,C", SIZES)
def test_sample_sum_bit_exact(target, Td, B, ns, C):
    lib, dev = target
    s = _eng.stream_ptr(dev)
    g = torch.Generator().manual_seed(Td * 77 + C)
    dg = torch.randn(Td, B * ns, C, generator=g)
    out = torch.full((Td, B, C), float("nan"), device=dev)
    dgd = dg.to(dev)
    lib.lv_sample_sum_f32(P(dgd), P(out), Td, B, ns, C, s)
    v = dg.view(Td, B, ns, C)
    want = v[:, :, 0].clone()
    for i in range(1, ns):
        want = want + v[:, :, i]                              # left to right, f32
    assert torch.equal(out.cpu(), want)
    # 16-bit twin: bf16 in, summed in f32, rounded to nearest even once; padded rows (ld > C) and dense ones
    for pad_in, pad_out in ((0, 0), (8, 16), (3, 5)):
        ld_in, ld_out = C + pad_in, C + pad_out
        src = torch.zeros(Td * B * ns, ld_in, dtype=torch.bfloat16)
        src[:, :C] = (dg * 3).reshape(-1, C).to(torch.bfloat16)
        dst = torch.full((Td * B, ld_out), -1, dtype=torch.int16, device=dev)
        srcd = src.view(torch.int16).to(dev)
        lib.lv_sample_sum_b16(P(srcd), ld_in, P(dst), ld_out, Td, B, ns, C, s)
        v = src[:, :C].float().view(Td * B, ns, C)
        acc = v[:, 0].clone()
        for i in range(1, ns):
            acc = acc + v[:, i]
        want16 = acc.to(torch.bfloat16).view(torch.int16)
        assert torch.equal(dst.cpu()[:, :C], want16), (pad_in, pad_out)
        if pad_out:
            assert bool((dst.cpu()[:, C:] == -1).all())         # the row padding is not written


@pytest.mark.parametrize("T,B,ns", [(1, 1, 1), (6, 5, 2), (70, 3, 3), (11, 17, 4), (130, 2, 5)])
def test_loss_assemble_ns(target, T, B, ns):
    lib, dev = target
    s = _eng.stream_ptr(dev)
    g = torch.Generator().manual_seed(T + 31 * B + ns)
    nll = torch.rand(T, B * ns, generator=g) * 5
    kl = torch.rand(B, generator=g)
    gl = torch.rand(B, generator=g) / B
    klw = torch.tensor([0.37])
    acc0 = torch.tensor([1.5, -2.0, 0.25])
    for rng in (False, True):
        d = {k: v.clone().to(dev) for k, v in dict(nll=nll, kl=kl, gl=gl, klw=klw, acc=acc0).items()}
        loss, rec, dkl = (torch.empty(B, device=dev) for _ in range(3))
        rowscale = torch.empty(B * ns, device=dev)
        state = torch.tensor([12345, 7], dtype=torch.int64, device=dev)
        args = (P(d["nll"]), P(d["kl"]), P(d["klw"]), P(d["gl"]), P(loss), P(rec), P(rowscale), P(dkl), P(d["acc"]), T, B, ns)
        if rng:
            lib.lv_loss_assemble_ns_rng_f32(*args, P(state), 3, s)
            assert state.cpu().tolist() == [12345, 10]
        else:
            lib.lv_loss_assemble_ns_f32(*args, s)
            assert state.cpu().tolist() == [12345, 7]
        want_rec = nll.double().view(T, B, ns).sum(0).mean(1)
        want_loss = want_rec + 0.37 * kl.double()
        assert rel_err(rec, want_rec) < 1e-6 and rel_err(loss, want_loss) < 1e-6
        assert torch.equal(rowscale.cpu(), (gl / ns).repeat_interleave(ns))          # g_loss[b] / ns, one IEEE division
        assert torch.equal(dkl.cpu(), klw * gl)
        want_acc = acc0.double() + torch.stack([want_loss.sum(), want_rec.sum(), kl.double().sum()])
        assert rel_err(d["acc"], want_acc) < 1e-6
        if ns == 1:
            # ... and for ns = 1 the bits of the single-sample kernel
            d1 = {k: v.clone().to(dev) for k, v in dict(acc=acc0).items()}
            l1, r1, k1, rs1 = (torch.empty(B, device=dev) for _ in range(4))
            lib.lv_loss_assemble_f32(P(d["nll"]), P(d["kl"]), P(d["klw"]), P(d["gl"]), P(l1), P(r1), P(rs1), P(k1), P(d1["acc"]), T, B, s)
            for a, b in ((l1, loss), (r1, rec), (rs1, rowscale), (k1, dkl), (d1["acc"], d["acc"])):
                assert torch.equal(a.cpu(), b.cpu())


def test_multisample_kernels_refuse_bad_arguments(target):
    lib, dev = target
    t = torch.zeros(64, device=dev)
    i64 = torch.zeros(64, dtype=torch.int64, device=dev)
    raw = lambda name: getattr(lib, "_raw_" + name)
    assert raw("lv_gx_expand_add_f32")(None, P(t), P(t), 1, 1, 1, 4, None) < 0
    assert raw("lv_gx_expand_add_f32")(P(t), P(t), P(t), 1, 1, 0, 4, None) < 0
    assert raw("lv_gx_expand_add_f32")(P(t), P(t), P(t), 1, 0, 1, 4, None) < 0
    assert raw("lv_sample_sum_f32")(P(t), None, 1, 1, 1, 4, None) < 0
    assert raw("lv_sample_sum_f32")(P(t), P(t), 1, 1, 1, 0, None) < 0
    assert raw("lv_sample_sum_b16")(P(t), 2, P(t), 4, 1, 1, 1, 4, None) < 0            # ld_in < C
    assert raw("lv_sample_sum_b16")(None, 4, P(t), 4, 1, 1, 1, 4, None) < 0
    assert raw("lv_repeat_rows_i64")(P(i64), None, 1, 1, 1, None) < 0
    assert raw("lv_repeat_rows_i64")(P(i64), P(i64), 1, 0, 1, None) < 0
    a = (P(t),) * 9
    assert raw("lv_loss_assemble_ns_f32")(*a, 1, 1, 0, None) < 0
    assert raw("lv_loss_assemble_ns_f32")(*((None,) + a[1:]), 1, 1, 1, None) < 0
    assert raw("lv_loss_assemble_ns_rng_f32")(*a, 1, 1, 1, None, 1, None) < 0           # no rng state


# ---------------------------------------------------------------------------------------------------------------------
# 2. the fused step, f32 configuration, against the reference fixtures
def _case(fx, tag):
    pre = tag + "/"
    return {k[len(pre):]: fx[k] for k in fx.files if k.startswith(pre)}


def _case_params(c, prefix="param/"):
    return {k: torch.from_numpy(c[prefix + k]) for k in ALL_KEYS}


CASES = ["ns2_wide_clip", "ns3_T2", "ns4_mid", "ns4_refinit"]


@pytest.mark.parametrize("tag", CASES)
def test_fused_step_matches_reference_fixture(target, tag):
    """One encoder step of AggressiveTextTrainer(nsamples=ns), exact-f32 configuration, against the reference's
    vae.loss(x, w, nsamples=ns) + backward + clip_grad_norm_ + SGD (bounds: parity_common's small-fixture ones)."""
    _, dev = target
    c = _case(load("text_ms_small"), tag)
    V, ni, H, nz, B, T, ns = (int(c[k]) for k in ("V", "ni", "H", "nz", "B", "T", "ns"))
    vae = build_vae(V, ni, H, nz, dev, params=_case_params(c))
    tr = _trainer(vae, lr=1.0, clip=float(c["max_norm"]), nsamples=ns)
    x = torch.from_numpy(c["x"]).to(dev)
    noise = tuple(torch.from_numpy(c[k]).to(dev) for k in ("eps", "mask_in", "mask_out"))
    assert tuple(noise[0].shape) == (B, ns, nz) and tuple(noise[1].shape) == (B, T - 1, ni) and tuple(noise[2].shape) == (B * ns, T - 1, H)
    tr.step(x, float(c["kl_weight"]), noise=noise)
    stt = tr.read_stats()
    st = tr.static[(B, T)]
    rec_scale = float(np.abs(c["rec"]).max())
    assert rel_err(st.loss, c["loss"]) < RTOL and rel_err(st.rec, c["rec"]) < RTOL
    kl_err = float(np.abs(st.kl.cpu().numpy() - c["kl"]).max())
    assert kl_err < RTOL * float(np.abs(c["kl"]).max()) + 1e-6 * (1 + rec_scale), ("kl", kl_err)
    assert abs(stt["loss_sum"] - float(c["loss"].sum())) < RTOL * abs(float(c["loss"].sum()))        # sums over the B SENTENCES
    assert abs(stt["rec_sum"] - float(c["rec"].sum())) < RTOL * abs(float(c["rec"].sum()))
    assert abs(stt["norm"] - float(c["total_norm"])) < RTOL * float(c["total_norm"])
    assert abs(stt["coef"] - float(c["coef"])) < RTOL
    if tag == "ns2_wide_clip":
        assert stt["coef"] < 0.99                              # the clip is active in this case
    named = dict(vae.named_parameters())
    for k in ALL_KEYS:                                          # .grad holds the CLIPPED gradient, as clip_grad_norm_ leaves it
        g = c["grad/" + k] * float(c["coef"])
        if np.abs(g).max() > 0:
            assert rel_err(named[k].grad, g) < GRAD_RTOL, (k, rel_err(named[k].grad, g))
        else:
            assert float(named[k].grad.abs().max()) == 0.0, k
    sd = vae.state_dict()
    for k in ENC_KEYS:
        assert rel_err(sd[k], c["new/" + k]) < RTOL, k
    for k in DEC_KEYS:                                          # an encoder step leaves the decoder untouched, bit for bit
        assert torch.equal(sd[k].cpu(), torch.from_numpy(c["param/" + k])), k


def test_fused_trajectory_matches_reference_fixture(target):
    """Three consecutive steps (encoder, encoder, both), each on the weights the previous one left."""
    _, dev = target
    c = _case(load("text_ms_small"), "traj_ns2")
    V, ni, H, nz, B, T, ns = (int(c[k]) for k in ("V", "ni", "H", "nz", "B", "T", "ns"))
    vae = build_vae(V, ni, H, nz, dev, params=_case_params(c))
    tr = _trainer(vae, lr=1.0, clip=float(c["max_norm"]), nsamples=ns)
    assert [str(u) for u in c["updates"]] == ["encoder", "encoder", "both"]
    for it, up in enumerate(c["updates"]):
        noise = tuple(torch.from_numpy(c[k][it]).to(dev) for k in ("eps", "mask_in", "mask_out"))
        tr.reset_stats()
        tr.step(torch.from_numpy(c["x"][it]).to(dev), float(c["kl_weight"]), noise=noise, update=str(up))
        st = tr.read_stats()
        assert abs(st["loss_sum"] - float(c["loss"][it].sum())) < RTOL * abs(float(c["loss"][it].sum()))
        assert abs(st["kl_sum"] - float(c["kl"][it].sum())) < RTOL * abs(float(c["kl"][it].sum())) + 1e-6 * (1 + float(np.abs(c["rec"][it]).max()))
        assert abs(st["norm"] - float(c["total_norm"][it])) < RTOL * float(c["total_norm"][it])
    sd = vae.state_dict()
    for k in ALL_KEYS:
        assert rel_err(sd[k], c["final/" + k]) < RTOL, k


# ---------------------------------------------------------------------------------------------------------------------
# 3. shared sentence == expanded: the fused step against the drop-in route on the same tree
@pytest.mark.parametrize("tag", ["ns4_mid", "ns2_wide_clip"])
def test_fused_step_equals_dropin_route(target, tag):
    from vae_lagging_encoder_amd import optim as lvo
    _, dev = target
    c = _case(load("text_ms_small"), tag)
    V, ni, H, nz, B, T, ns = (int(c[k]) for k in ("V", "ni", "H", "nz", "B", "T", "ns"))
    clip, klw = float(c["max_norm"]), float(c["kl_weight"])
    x = torch.from_numpy(c["x"]).to(dev)
    noise = tuple(torch.from_numpy(c[k]).to(dev) for k in ("eps", "mask_in", "mask_out"))
    # the drop-in route: x, the dropout_in mask and z repeated ns times onto the ns = 1 engine (LSTMDecoder.reconstruct_error)
    b = build_vae(V, ni, H, nz, dev, params=_case_params(c))
    enc_opt, dec_opt = lvo.SGD(b.encoder.parameters(), lr=1.0, momentum=0), lvo.SGD(b.decoder.parameters(), lr=1.0, momentum=0)
    enc_opt.zero_grad()
    dec_opt.zero_grad()
    loss, rec, kl = b.loss(x, klw, nsamples=ns, noise=noise)
    loss.mean(dim=-1).backward()
    total = float(lvo.clip_grad_norm_(b.parameters(), clip))
    enc_opt.step()
    gb = {k: p.grad.detach().clone() for k, p in b.named_parameters()}
    norms = {}
    for fold in (True, False):
        a = build_vae(V, ni, H, nz, dev, params=_case_params(c))
        tr = _trainer(a, lr=1.0, clip=clip, nsamples=ns, fold_norm=fold)
        tr.step(x, klw, noise=noise)
        st = tr.read_stats()
        assert (tr._fold is not None) == fold
        norms[fold] = st["norm"]
        assert abs(st["norm"] - total) < 1e-5 * total
        s_ = tr.static[(B, T)]
        assert rel_err(s_.loss, loss) < 1e-5 and rel_err(s_.rec, rec) < 1e-5
        for k, p in a.named_parameters():                       # both hold the clipped gradient: same arithmetic, another order
            if float(gb[k].abs().max()) > 0:
                assert rel_err(p.grad, gb[k]) < 1e-5, (k, rel_err(p.grad, gb[k]))
            else:
                assert float(p.grad.abs().max()) == 0.0, k
        sa, sb = a.state_dict(), b.state_dict()
        for k in ENC_KEYS:
            assert rel_err(sa[k], sb[k]) < 1e-5, k
    assert abs(norms[True] - norms[False]) <= 1e-6 * norms[False], norms


# ---------------------------------------------------------------------------------------------------------------------
# 4. nsamples = 1 is today's trainer, bit for bit
def test_nsamples_one_is_bit_identical_to_the_default(target):
    _, dev = target
    V, ni, H, nz, B = 97, 12, 20, 4, 6
    Pm = O.random_params(V, ni, H, nz, seed=5, scale=0.3, emb_scale=0.5, head_scale=0.5)
    xs = [O.synthetic_batch(B, T, V, seed=70 + i).to(dev) for i, T in enumerate((5, 8, 6))]
    out = []
    for kw in ({}, {"nsamples": 1}):
        vae = build_vae(V, ni, H, nz, dev, params=Pm)
        tr = _trainer(vae, lr=1.0, clip=5.0, seed=11, **kw)
        sums = []
        for i in range(5):
            x = xs[i % 3]
            noise = _dev_noise(O.draw_noise(B, x.shape[1], ni, H, nz, seed=90 + i), dev) if i % 2 == 0 else None      # injected and device-drawn
            tr.step(x, 0.6, noise=noise, update=("encoder", "encoder", "decoder", "encoder", "both")[i])
            sums.append(tr.read_stats())
        out.append((sums, {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}))
    for a, b in zip(out[0][0], out[1][0]):
        assert a == b
    for k in ALL_KEYS:
        assert torch.equal(out[0][1][k], out[1][1][k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 5. the wide fixtures (H = 1024, V = 20001) on the GPU
def _wide(name, dev):
    from test_gpu_parity import _seeded_full_size_vae
    fx = load(name)
    vae = _seeded_full_size_vae(fx, dev)
    x = torch.from_numpy(fx["x"]).to(dev)
    unpack = lambda k: torch.from_numpy(np.unpackbits(fx[k + "_bits"])[:int(np.prod(fx[k + "_shape"]))].reshape(tuple(fx[k + "_shape"])))
    noise = (torch.from_numpy(fx["eps"]).to(dev), unpack("mask_in").to(dev), unpack("mask_out").to(dev))
    return fx, vae, x, noise


WIDE = ["text_ms_h1024_b8", "text_ms_h1024_b32_t50"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", WIDE)
def test_wide_fixture_f32(hip_device, name):
    fx, vae, x, noise = _wide(name, hip_device)
    B, T, ns = int(fx["B"]), int(fx["T"]), int(fx["ns"])
    tr = _trainer(vae, lr=1.0, clip=5.0, nsamples=ns)
    tr.step(x, float(fx["kl_weight"]), noise=noise)
    tr.read_stats()
    st = tr.static[(B, T)]
    print(name, "f32: loss %.2e rec %.2e kl %.2e" % (rel_err(st.loss, fx["loss"]), rel_err(st.rec, fx["rec"]), rel_err(st.kl, fx["kl"])))
    assert rel_err(st.loss, fx["loss"]) < 1e-4 and rel_err(st.rec, fx["rec"]) < 1e-4 and rel_err(st.kl, fx["kl"]) < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("name", WIDE)
def test_wide_fixture_bf16(hip_device, name):
    """The throughput configuration (operand images, persistent recurrences on B * ns = 32 / 128 decoder rows) against the
    reference run, at the bounds tests/test_gpu_parity.py::_check_bf16_against_full_size_fixture holds the ns = 1 step to."""
    import json
    fx, vae, x, noise = _wide(name, hip_device)
    p0 = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    B, T, V, ns = int(fx["B"]), int(fx["T"]), int(fx["V"]), int(fx["ns"])
    tr = _trainer(vae, lr=1.0, clip=5.0, precision="bf16", nsamples=ns)
    tr.step(x, float(fx["kl_weight"]), noise=noise)
    st = tr.read_stats()
    big = torch.cuda.get_device_properties(hip_device).multi_processor_count >= 256
    w = tr.dec._ws(B * ns, T - 1, ns)
    out = {"persistent_used": bool(big and tr.dec.persistent and getattr(w, "saved_layout", ("",))[0] == "persist16"
                                   and _eng.persist_rung(tr.dec) < 2 and _eng.persist_rung(tr.enc) < 2)}
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
    out["gradnorm_rel"], out["gradnorm_rel_max"] = gn, max(gn.values())
    out["grad_sample_err_over_rms"], out["grad_sample_err_over_rms_max"] = gs, max(gs.values())
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
    print(name + ":", json.dumps(out))                       # (profiles/multisample_parity.json holds these lines of one run)
    if big:
        assert out["persistent_used"], out
    assert out["loss_rel"] < 1e-4 and out["rec_rel"] < 1e-4 and out["kl_rel"] < 1e-4 and out["norm_rel"] < 1e-4, out
    assert out["rec_excess_rel"] < 1e-3 and out["gradnorm_rel_max"] < 2e-3, out
    assert out["grad_sample_err_over_rms_max"] < 0.1 and out["enc_update_rel_max"] < 2e-2, out


# ---------------------------------------------------------------------------------------------------------------------
# 6. device-drawn noise
def test_device_drawn_noise(target):
    _, dev = target
    V, ni, H, nz, B, T, ns = 97, 12, 20, 8, 6, 9, 3
    vae = build_vae(V, ni, H, nz, dev, params=O.random_params(V, ni, H, nz, seed=6, scale=0.3, emb_scale=0.5, head_scale=0.5))
    tr = _trainer(vae, lr=0.1, clip=5.0, nsamples=ns, seed=5)
    x = O.synthetic_batch(B, T, V, seed=3).to(dev)
    snaps = []
    for _ in range(2):
        tr.step(x, 0.5)
        tr.commit()
        st = tr.static[(B, T)]
        snaps.append((st.eps.cpu().clone(), st.m_in.cpu().clone(), st.m_out.cpu().clone()))
    assert int(tr.rng_state[1].item()) == 2                     # one Philox offset per step; the element index is a counter word of its own
    (e0, i0, o0), (e1, i1, o1) = snaps
    assert tuple(e0.shape) == (B, ns, nz) and tuple(i0.shape) == (B, T - 1, ni) and tuple(o0.shape) == (B * ns, T - 1, H)
    assert not torch.equal(e0, e1) and not torch.equal(o0, o1) and not torch.equal(i0, i1)
    assert float((e0.reshape(-1)[:, None] == e1.reshape(-1)[None, :]).float().sum()) == 0      # consecutive steps repeat no value
    for e in (e0, e1):
        rows = e.reshape(B * ns, nz)
        assert len({tuple(r.tolist()) for r in rows}) == B * ns                               # no two (b, s) rows are equal
        assert torch.isfinite(e).all() and abs(float(e.mean())) < 4 / math.sqrt(e.numel()) and 0.6 < float(e.std()) < 1.4
    for o in (o0, o1):
        v = o.view(B, ns, -1)
        for b in range(B):
            for s in range(1, ns):
                assert not torch.equal(v[b, 0], v[b, s])                                     # the samples of a sentence get their own dropout_out mask
    for m, p in ((i0, vae.decoder.dropout_in.p), (i1, vae.decoder.dropout_in.p), (o0, vae.decoder.dropout_out.p), (o1, vae.decoder.dropout_out.p)):
        assert set(m.unique().tolist()) <= {0, 1}
        sigma = math.sqrt(p * (1 - p) / m.numel())
        assert abs(float(m.float().mean()) - (1 - p)) < 4 * sigma


# ---------------------------------------------------------------------------------------------------------------------
# 7. transactional recovery
def _recovery(dev, V, ni, H, nz, B, ns, Ts, precision, scale, K=4, fault_at=2):
    Pm = O.random_params(V, ni, H, nz, seed=51, scale=scale, emb_scale=0.5, head_scale=0.5)
    batches = [O.synthetic_batch(B, T, V, seed=60 + i).to(dev) for i, T in enumerate(Ts)]
    picks = [0] + [int(i) for i in np.random.RandomState(9).randint(0, len(batches), size=K)]

    def noise_for(step, x):
        return _dev_noise(O.draw_noise(x.shape[0], x.shape[1], ni, H, nz, ns=ns, seed=700 + step), dev)

    def run(faulty):
        vae = build_vae(V, ni, H, nz, dev, params=Pm)
        tr = _trainer(vae, lr=1.0, clip=5.0, precision=precision, nsamples=ns)
        demotions = []
        tr.on_demote = demotions.append
        sums = []
        tr.reset_stats()
        for step in range(K):
            x = batches[picks[step]]
            if step == fault_at:
                if faulty:
                    tr.dec.status.fill_(100 + step)     # what a timed-out recurrence leaves behind -- set by hand, nothing is provoked
                else:
                    for e in (tr.enc, tr.dec):
                        _eng.demote_persistent(e)       # the clean run moves to the next rung by hand at the same step
            tr.step(x, 0.7, noise=noise_for(step, x))
            if step == K - 2:
                sums.append(tr.read_stats())
        tr.step(batches[1], 0.7, noise=noise_for(K, batches[1]), update="decoder")
        sums.append(tr.read_stats())
        return {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}, sums, tr, demotions

    sd_f, sums_f, tr_f, dem = run(True)
    sd_c, sums_c, tr_c, _ = run(False)
    assert dem == [1] and tr_f.recoveries == 1 and tr_c.recoveries == 0
    assert _eng.persist_rung(tr_f.enc) == _eng.persist_rung(tr_c.enc) == 1
    assert int(tr_f.enc.status.item()) == 0 and int(tr_f.dec.status.item()) == 0
    for k in ALL_KEYS:
        assert torch.equal(sd_f[k], sd_c[k]), k
    for a, b in zip(sums_f, sums_c):
        for key in ("loss_sum", "rec_sum", "kl_sum"):
            assert a[key] == b[key], (key, a[key], b[key])


def test_transactional_recovery_multisample(target):
    _, dev = target
    _recovery(dev, 97, 12, 20, 4, 6, 3, [5, 8, 6], "f32", 0.3)


@pytest.mark.gpu
def test_transactional_recovery_multisample_persistent(hip_device):
    """bf16 configuration at H = 1024: 8 sentences x 4 samples = 32 decoder rows on the persistent launches."""
    _recovery(hip_device, 2003, 64, 1024, 32, 8, 4, [12, 9, 14], "bf16", 0.03)


# ---------------------------------------------------------------------------------------------------------------------
# 8. steady state
def _steady(dev, ns, precision, dims, steps=10):
    V, ni, H, nz, B = dims
    vae = build_vae(V, ni, H, nz, dev, params=O.random_params(V, ni, H, nz, seed=8, scale=0.05 if H >= 512 else 0.3, emb_scale=0.5, head_scale=0.3))
    tr = _trainer(vae, lr=0.1, clip=5.0, precision=precision, nsamples=ns)
    batches = [O.synthetic_batch(B, T, V, seed=20 + i).to(dev) for i, T in enumerate((7, 9))]
    tr.prepare_batches(batches)
    lib = tr.lib
    orig = lib.lv_token_sort
    calls = []
    lib.__dict__["lv_token_sort"] = lambda *a: calls.append(1) or orig(*a)
    try:
        for x in batches:                                       # first step of each shape: workspaces are built
            tr.step(x, 0.5)
        tr.commit()
        assert not calls, "a prepared batch was sorted again"
        misses = (tr.enc.wsc.misses, tr.dec.wsc.misses)
        cuda = torch.device(dev).type == "cuda"
        if cuda:
            torch.cuda.synchronize(dev)
            a0 = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
        for i in range(steps):
            tr.step(batches[i % 2], 0.5)
        grew = None
        if cuda:
            torch.cuda.synchronize(dev)
            grew = torch.cuda.memory_stats(dev)["allocation.all.allocated"] - a0
        tr.commit()
        assert not calls
        assert (tr.enc.wsc.misses, tr.dec.wsc.misses) == misses
    finally:
        lib.__dict__["lv_token_sort"] = orig
    return grew


def test_steady_state_no_sort_no_new_workspace(target):
    _, dev = target
    grew_ms = _steady(dev, 3, "f32", (97, 12, 20, 4, 6))
    grew_1 = _steady(dev, 1, "f32", (97, 12, 20, 4, 6))
    if grew_ms is not None:
        assert grew_ms <= grew_1, (grew_ms, grew_1)


@pytest.mark.gpu
def test_steady_state_bf16_h1024(hip_device):
    grew_ms = _steady(hip_device, 4, "bf16", (2003, 64, 1024, 32, 8))
    grew_1 = _steady(hip_device, 1, "bf16", (2003, 64, 1024, 32, 8))
    assert grew_ms <= grew_1, (grew_ms, grew_1)


def test_workspaces_do_not_alias_single_sample_shapes(target):
    """(B, ns, Td) and (B * ns, 1, Td) are different workspaces of one engine."""
    _, dev = target
    V, ni, H, nz = 53, 8, 16, 4
    vae = build_vae(V, ni, H, nz, dev, seed=0)
    dec = vae.decoder._hip
    dec.ensure(dev)
    a, b = dec._ws(6, 5, 3), dec._ws(6, 5)
    assert a is not b and a.nll.data_ptr() != b.nll.data_ptr() and a is dec._ws(6, 5, 3)
    assert tuple(a.X.shape) == (5 * 2, ni) and tuple(b.X.shape) == (5 * 6, ni) and tuple(a.x_rep.shape) == (6, 6)
    assert dec.wsc.total == sum(dec.wsc.nbytes.values()) and dec.wsc.nbytes[(2, 3, 5)] > 0      # counted by the byte budget


# ---------------------------------------------------------------------------------------------------------------------
# 9. fences
def test_fences(target):
    _, dev = target
    V, ni, H, nz, B, T = 53, 8, 16, 4, 4, 6
    vae = build_vae(V, ni, H, nz, dev, seed=0)
    for kw in (dict(grad_sync=object()), dict(use_graph=True), dict(micro_batches=2), dict(decoder_grads="norm")):
        with pytest.raises(ValueError, match="nsamples"):
            _trainer(vae, nsamples=2, **kw)
    with pytest.raises(ValueError, match="nsamples"):
        _trainer(vae, nsamples=0)
    tr = _trainer(vae, nsamples=2)
    x = O.synthetic_batch(B, T, V, seed=1).to(dev)
    eps, mi, mo = _dev_noise(O.draw_noise(B, T, ni, H, nz, ns=2, seed=2), dev)
    w0 = {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}
    gen = (tr.enc.gen, tr.dec.gen)
    bad = [(eps[:, :1], mi, mo), (eps, mi.repeat_interleave(2, dim=0), mo), (eps, mi, mo[:B]), (eps.reshape(B * 2, 1, nz), mi, mo)]
    for noise in bad:
        with pytest.raises(ValueError, match="nsamples"):
            tr.step(x, 0.5, noise=noise)
    assert (tr.enc.gen, tr.dec.gen) == gen and not tr._journal      # nothing was launched or journalled
    tr.step(x, 0.5, noise=(eps, mi, mo))
    tr.commit()
    assert any(not torch.equal(w0[k], vae.state_dict()[k].cpu()) for k in ENC_KEYS)


# ---------------------------------------------------------------------------------------------------------------------
# 10. TextTrainingLoop
def test_training_loop_honours_nsamples(target):
    from vae_lagging_encoder_amd.training import TextTrainingLoop
    _, dev = target
    V, ni, H, nz, B = 53, 8, 16, 4, 4
    Pm = O.random_params(V, ni, H, nz, seed=2, scale=0.2, emb_scale=0.5, head_scale=0.5)
    train = [O.synthetic_batch(B, T, V, seed=10 + i).to(dev) for i, T in enumerate((5, 6, 4))]

    def mk_args(ns):
        return argparse.Namespace(kl_start=0.1, warm_up=1, batch_size=B, epochs=1, aggressive=0, nsamples=ns, test_nepoch=5,
                                  iw_nsamples=20, momentum=0)

    def noise_fn_for(ns):
        cnt = {"n": 0}

        def fn(x):
            cnt["n"] += 1
            return _dev_noise(O.draw_noise(x.shape[0], x.shape[1], ni, H, nz, ns=ns, seed=500 + cnt["n"]), dev)
        return fn

    recs = {}
    for ns in (2, 1):
        vae = build_vae(V, ni, H, nz, dev, params=Pm)
        loop = TextTrainingLoop(vae, train, train[:2], train[:1], mk_args(ns), log=lambda *_: None, np_rng=np.random.RandomState(3),
                                noise_fn=noise_fn_for(ns))
        assert loop.trainer.nsamples == ns
        loop.run()
        recs[ns] = [r["rec_sum"] for r in loop.iterations]
        order = [r["batch"] for r in loop.iterations]
        klws = [r["kl_weight"] for r in loop.iterations]
    # the same steps driven by hand
    vae = build_vae(V, ni, H, nz, dev, params=Pm)
    tr = _trainer(vae, lr=1.0, clip=5.0, nsamples=2)
    fn = noise_fn_for(2)
    hand = []
    for i, w in zip(order, klws):
        tr.reset_stats()
        tr.step(train[i], w, noise=fn(train[i]), update="both")
        hand.append(tr.read_stats()["rec_sum"])
    assert recs[2] == hand
    assert all(abs(a - b) > 1e-4 * abs(b) for a, b in zip(recs[2], recs[1]))
    # a trainer built for another sample count is refused
    vae = build_vae(V, ni, H, nz, dev, params=Pm)
    with pytest.raises(ValueError, match="nsamples"):
        TextTrainingLoop(vae, train, train[:2], train[:1], mk_args(2), trainer=_trainer(vae, nsamples=1), log=lambda *_: None)
    with pytest.raises(ValueError, match="nsamples"):
        TextTrainingLoop(vae, train, train[:2], train[:1], mk_args(1), trainer=_trainer(vae, nsamples=2), log=lambda *_: None)


@pytest.mark.gpu
def test_grouped_input_side_products_equal_separate(hip_device):
    """bf16 configuration at a shape where dW_ih[:, :ni] and dX (both over Td * B rows) take ONE grouped lv_gemm_b16_pair launch:
    the same step with the grouped launch switched off (engine.PAIR_WGRAD) -- two lv_gemm_b16 products on the same bf16 operands,
    f32 accumulation in another order -- must give the same gradients to summation-order accuracy (1e-5, parity_common's bound for
    two routes doing the same arithmetic in a different order); everything upstream of the two products is the same launches."""
    V, ni, H, nz, B, T, ns = 2003, 512, 1024, 32, 32, 101, 2
    Pm = O.random_params(V, ni, H, nz, seed=77, scale=0.03, emb_scale=0.3, head_scale=0.2)
    x = O.synthetic_batch(B, T, V, seed=3).to(hip_device)
    noise = _dev_noise(O.draw_noise(B, T, ni, H, nz, ns=ns, seed=4), hip_device)
    res = {}
    saved = _eng.PAIR_WGRAD
    try:
        for pair in (True, False):
            _eng.PAIR_WGRAD = pair
            vae = build_vae(V, ni, H, nz, hip_device, params=Pm)
            tr = _trainer(vae, lr=1.0, clip=5.0, precision="bf16", nsamples=ns)
            if pair:
                ws = _eng._gemm_ws(tr.lib, _eng.stream_ptr(hip_device))
                assert tr.lib.lv_gemm_b16_pair_supported(1, 4 * H, ni, (T - 1) * B, 0, (T - 1) * B, ni, 4 * H, ws.numel()) == 1
            tr.step(x, 0.5, noise=noise)
            st = tr.read_stats()
            res[pair] = (st, {k: p.grad.detach().clone() for k, p in vae.named_parameters()})
            pending = torch.zeros(1, dtype=torch.int32, device=hip_device)
            tr.lib.lv_gemm_b16_pair_pending(P(pending), _eng.stream_ptr(hip_device))
            assert int(pending.item()) == 0
    finally:
        _eng.PAIR_WGRAD = saved
    (s1, g1), (s0, g0) = res[True], res[False]
    assert s1["loss_sum"] == s0["loss_sum"] and abs(s1["norm"] - s0["norm"]) <= 1e-5 * s0["norm"]
    for k in g0:
        assert rel_err(g1[k], g0[k]) < 1e-5, (k, rel_err(g1[k], g0[k]))

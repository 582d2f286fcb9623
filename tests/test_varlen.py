"""Variable-length batches (x, lengths): lv_lstm_fwd_len_f32 / lv_lstm_bwd_len_f32 / lv_nll_mask_len_f32 (csrc/lv_lstm.hip),
engine.LSTMEncoderEngine / LSTMDecoderEngine with lengths, VarLSTMEncoder / VarLSTMDecoder (reference enc_lstm.py:77-126,
dec_lstm.py:370-476) and the VAE methods on a pair.

Kernel level (emulator build and MI355X through one fixture): the length-aware recurrences against a float64 statement written
here (a finished row keeps its state; its outputs are zero; nothing flows back through a padded step), inputs drawn as
tests/test_gpu_kernels.py::test_lstm_fwd_bwd draws them and held to the bounds that test applies to the equal-length kernels:
2e-5 on hs / cs, 4e-5 on hdrop, 1e-4 of the largest reference entry on dG / dc0 / dh0, times T for dGsum.

Drop-in level: tests/golden/varlen_small.npz (make_golden_varlen.py: the reference's unmodified classes, every random draw
recorded) at parity_common's RTOL / GRAD_RTOL; the by-length route (class switch masked = False: every group of equal length
through the equal-length classes) as the second oracle where no fixture reaches.
"""
import ctypes

import numpy as np
import pytest
import torch

from helpers import ALL_KEYS, load, rel_err
from parity_common import GRAD_RTOL, RTOL
from vae_lagging_encoder_amd import _lib
from vae_lagging_encoder_amd import engine as E
from vae_lagging_encoder_amd.engine import P
from vae_lagging_encoder_amd.factory import build_text_vae
from vae_lagging_encoder_amd.modules import LSTMDecoder, LSTMEncoder, VarLSTMDecoder, VarLSTMEncoder

PAD, BOS, EOS = 0, 1, 2
POISON = 7777.0


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


# ---- 1. the recurrences ---------------------------------------------------------------------------------------------------------
def _lstm_len_ref(gx, whh, h0, c0, steps, mask, scale):
    """The float64 statement: row b runs while t < steps[b]; afterwards its state stays and its output is zero."""
    T = gx.shape[0]
    h, c = h0, c0
    hs, cs, outs = [h0], [c0], []
    for t in range(T):
        live = (t < steps).view(-1, 1)
        a = gx[t] + h @ whh.t()
        i, f, g, o = a.chunk(4, -1)
        i, f, o, g = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(g)
        cn = f * c + i * g
        hn = o * torch.tanh(cn)
        c = torch.where(live, cn, c)
        h = torch.where(live, hn, h)
        hs.append(h)
        cs.append(c)
        out = hn * mask[:, t].to(hn.dtype) * scale if mask is not None else hn
        outs.append(torch.where(live, out, torch.zeros_like(out)))
    return torch.stack(hs), torch.stack(cs), torch.stack(outs)


def _steps_for(T, B, seed):
    """Unsorted step counts that include 1 and T."""
    g = torch.Generator().manual_seed(seed)
    st = torch.randint(1, T + 1, (B,), generator=g, dtype=torch.int32)
    st[B // 2], st[0], st[B - 1] = 1, T, max(1, T - 1)
    if B > 3:
        st[1] = 1
    return st


def _draw(T, B, H):
    g = torch.Generator().manual_seed(T * 100 + B + H)
    return dict(gx=torch.randn(T, B, 4 * H, generator=g) * 0.5, whh=torch.randn(4 * H, H, generator=g) / H ** 0.5,
                c0=torch.randn(B, H, generator=g) * 0.5, mask=torch.rand(B, T, H, generator=g) < 0.5,
                wext=torch.randn(T, B, H, generator=g), wlast=torch.randn(B, H, generator=g))


def _s(dev):
    return E.stream_ptr(dev)


def _run_fwd(lib, dev, d, steps, T, B, H, use_mask, tanh_init, len_entry=True):
    hs = torch.zeros(T + 1, B, H, device=dev)
    cs = torch.zeros(T + 1, B, H, device=dev)
    hs[0] = (torch.tanh(d["c0"].double()).float() if tanh_init else torch.zeros(B, H)).to(dev)
    cs[0] = d["c0"].to(dev)
    gates = torch.full((T, B, 4 * H), POISON, device=dev)
    hdrop = torch.full((T, B, H), POISON, device=dev)
    ws = torch.full((lib.lv_lstm_ws_floats(B, H),), float("nan"), device=dev)
    gx, whh, m8 = d["gx"].to(dev), d["whh"].to(dev), d["mask"].to(torch.uint8).contiguous().to(dev)
    if len_entry:
        lib.lv_lstm_fwd_len_f32(P(gx), P(whh), P(hs), P(cs), P(gates), P(m8) if use_mask else None, 2.0, P(hdrop), P(ws),
                                P(steps), int(steps.max()), T, B, H, _s(dev))
    else:
        lib.lv_lstm_fwd_f32(P(gx), P(whh), P(hs), P(cs), P(gates), P(m8) if use_mask else None, 2.0, P(hdrop), P(ws), T, B, H, _s(dev))
    return dict(hs=hs, cs=cs, gates=gates, hdrop=hdrop, gx=gx, whh=whh, m8=m8, ws=ws)


def _run_bwd(lib, dev, d, f, steps, T, B, H, use_mask, tanh_init, use_ext, use_last, len_entry=True, wext=None):
    dG = torch.full((T, B, 4 * H), POISON, device=dev)
    dGsum = torch.full((B, 4 * H), 7.0, device=dev)
    dc0 = torch.full((B, H), POISON, device=dev)
    dh0 = torch.full((B, H), POISON, device=dev)
    wext = d["wext"].to(dev) if wext is None else wext
    wlast = d["wlast"].to(dev)
    ws = f["ws"]
    ws.fill_(float("nan"))            # scratch content must not matter
    args = (P(wext) if use_ext else None, P(wlast) if use_last else None, P(f["m8"]) if use_mask else None, 2.0, P(f["whh"]),
            P(f["gates"]), P(f["hs"]), P(f["cs"]), P(dG), P(dGsum), P(ws), P(dh0), P(dc0), int(tanh_init))
    if len_entry:
        lib.lv_lstm_bwd_len_f32(*args, P(steps), int(steps.max()), T, B, H, _s(dev))
    else:
        lib.lv_lstm_bwd_f32(*args, T, B, H, _s(dev))
    return dict(dG=dG, dGsum=dGsum, dc0=dc0, dh0=dh0)


def _check_len_kernels(lib, dev, T, B, H, use_mask, tanh_init, use_ext, use_last):
    d = _draw(T, B, H)
    steps_h = _steps_for(T, B, T * 7 + B)
    assert int(steps_h.min()) == 1 and int(steps_h.max()) == T and not bool((steps_h[:-1] >= steps_h[1:]).all())
    steps = steps_h.to(dev)
    gx64 = d["gx"].double().requires_grad_(True)
    c064 = d["c0"].double().requires_grad_(True)
    h0free = torch.zeros(B, H, dtype=torch.float64, requires_grad=True)
    h064 = torch.tanh(c064) if tanh_init else h0free
    hs_r, cs_r, out_r = _lstm_len_ref(gx64, d["whh"].double(), h064, c064, steps_h, d["mask"] if use_mask else None, 2.0)
    loss = (hs_r[-1] * 0).sum()
    if use_ext:
        loss = loss + (out_r * d["wext"].double()).sum()
    if use_last:
        loss = loss + (hs_r[-1] * d["wlast"].double()).sum()
    loss.backward()
    f = _run_fwd(lib, dev, d, steps, T, B, H, use_mask, tanh_init)
    e_hs = float((f["hs"].cpu().double() - hs_r.detach()).abs().max())
    e_cs = float((f["cs"].cpu().double() - cs_r.detach()).abs().max())
    e_hd = float((f["hdrop"].cpu().double() - out_r.detach()).abs().max())
    print("forward errors: hs %.2e cs %.2e hdrop %.2e" % (e_hs, e_cs, e_hd))
    assert e_hs < 2e-5 and e_cs < 2e-5 and e_hd < 4e-5
    # inactive steps: hdrop exactly 0, the frozen state bit-equal to the row's last active state
    hs_c, cs_c, hd_c = f["hs"].cpu(), f["cs"].cpu(), f["hdrop"].cpu()
    for b in range(B):
        n = int(steps_h[b])
        if n < T:
            assert float(hd_c[n:, b].abs().max()) == 0.0
            assert _same(hs_c[n + 1:, b], hs_c[n, b].expand(T - n, H)) and _same(cs_c[n + 1:, b], cs_c[n, b].expand(T - n, H))
    r = _run_bwd(lib, dev, d, f, steps, T, B, H, use_mask, tanh_init, use_ext, use_last)
    dG = r["dG"].cpu()
    sc = float(gx64.grad.abs().max())
    assert sc > 0
    e_dG = float((dG.double() - gx64.grad).abs().max())
    e_sum = float((r["dGsum"].cpu().double() - gx64.grad.sum(0)).abs().max())
    e_dc0 = float((r["dc0"].cpu().double() - c064.grad).abs().max())
    print("backward errors: dG %.2e (scale %.2e) dGsum %.2e dc0 %.2e" % (e_dG, sc, e_sum, e_dc0))
    assert e_dG < 1e-4 * sc and e_sum < 1e-4 * sc * T and e_dc0 < 1e-4 * float(c064.grad.abs().max())
    if not tanh_init:
        e_dh0 = float((r["dh0"].cpu().double() - h0free.grad).abs().max())
        assert e_dh0 < 1e-4 * float(h0free.grad.abs().max()), e_dh0
    for b in range(B):
        n = int(steps_h[b])
        if n < T:
            assert float(dG[n:, b].abs().max()) == 0.0
    # what the BPTT may not read: the gate records, cs and dh_ext of inactive steps, and the scratch
    gates4 = f["gates"].view(T, B, H, 4)
    wext = d["wext"].to(dev).clone()
    for b in range(B):
        n = int(steps_h[b])
        if n < T:
            gates4[n:, b] = float("nan")
            f["cs"][n + 1:, b] = float("nan")
            wext[n:, b] = float("nan")
    r2 = _run_bwd(lib, dev, d, f, steps, T, B, H, use_mask, tanh_init, use_ext, use_last, wext=wext)
    for k in ("dG", "dGsum", "dc0", "dh0"):
        assert bool(torch.isfinite(r2[k]).all()), k
        assert _same(r2[k], r[k]), k


LEN_CASES = [
    # T, B, H, use_mask, tanh_init, use_ext, use_last
    (7, 5, 20, True, True, True, False),        # unaligned H, decoder-shaped
    (7, 5, 20, False, False, False, True),      # ... encoder-shaped (dh_last enters each row at its own last step)
    (6, 33, 64, True, False, True, True),       # next row-block template
    (5, 70, 64, False, True, True, True),       # largest row-block template
    (3, 130, 64, True, True, True, False),      # two batch chunks: steps follows the chunk
    (3, 130, 64, False, False, False, True),
]


@pytest.mark.parametrize("T,B,H,use_mask,tanh_init,use_ext,use_last", LEN_CASES)
def test_len_recurrences_against_float64(target, T, B, H, use_mask, tanh_init, use_ext, use_last):
    lib, dev = target
    _check_len_kernels(lib, dev, T, B, H, use_mask, tanh_init, use_ext, use_last)


@pytest.mark.gpu
@pytest.mark.parametrize("use_mask,tanh_init,use_ext,use_last", [(True, True, True, False), (False, False, False, True)])
def test_len_recurrences_against_float64_h1024(hip_device, use_mask, tanh_init, use_ext, use_last):
    _check_len_kernels(E.backend_for(hip_device), hip_device, 6, 32, 1024, use_mask, tanh_init, use_ext, use_last)


@pytest.mark.parametrize("T,B,H", [(7, 5, 20), (6, 33, 64), (5, 70, 64), (3, 130, 64)])
def test_all_steps_active_equals_the_equal_length_entries_bit_for_bit(target, T, B, H):
    lib, dev = target
    d = _draw(T, B, H)
    steps = torch.full((B,), T, dtype=torch.int32).to(dev)
    fa = _run_fwd(lib, dev, d, steps, T, B, H, True, True)
    fb = _run_fwd(lib, dev, d, steps, T, B, H, True, True, len_entry=False)
    for k in ("hs", "cs", "hdrop", "gates"):
        assert _same(fa[k], fb[k]), k
    ra = _run_bwd(lib, dev, d, fa, steps, T, B, H, True, True, True, True)
    rb = _run_bwd(lib, dev, d, fb, steps, T, B, H, True, True, True, True, len_entry=False)
    for k in ("dG", "dGsum", "dc0", "dh0"):
        assert _same(ra[k], rb[k]), k


@pytest.mark.parametrize("T,B", [(7, 5), (3, 300)])
def test_nll_mask(target, T, B):
    lib, dev = target
    g = torch.Generator().manual_seed(T + B)
    nll = torch.randn(T + 1, B, generator=g)
    steps_h = _steps_for(T, B, 3)
    d_nll, steps = nll.clone().to(dev), steps_h.to(dev)
    lib.lv_nll_mask_len_f32(P(d_nll), P(steps), int(steps_h.max()), T, B, _s(dev))
    got = d_nll.cpu()
    live = torch.arange(T).view(T, 1) < steps_h.view(1, B)
    assert _same(got[:T][live], nll[:T][live]) and float(got[:T][~live].abs().max()) == 0.0
    assert _bits(got[:T][~live]).abs().max() == 0          # +0.0, not -0.0
    assert _same(got[T], nll[T])                             # the row behind the buffer is not touched


def test_len_entries_check_their_arguments(target):
    lib, dev = target
    T, B, H = 3, 5, 20
    d = _draw(T, B, H)
    steps = torch.full((B,), 2, dtype=torch.int32).to(dev)

    def bufs():
        return dict(hs=torch.full((T + 1, B, H), POISON, device=dev), cs=torch.full((T + 1, B, H), POISON, device=dev),
                    gates=torch.full((T, B, 4 * H), POISON, device=dev), hdrop=torch.full((T, B, H), POISON, device=dev),
                    ws=torch.full((lib.lv_lstm_ws_floats(B, H),), POISON, device=dev), dG=torch.full((T, B, 4 * H), POISON, device=dev),
                    dGsum=torch.full((B, 4 * H), POISON, device=dev), nll=torch.full((T, B), POISON, device=dev))
    gx, whh = d["gx"].to(dev), d["whh"].to(dev)
    fwd, bwd, msk = lib.cdll.lv_lstm_fwd_len_f32, lib.cdll.lv_lstm_bwd_len_f32, lib.cdll.lv_nll_mask_len_f32
    for what, st, mx, b_arg in (("null steps", None, 2, B), ("a step count above T", P(steps), T + 1, B), ("B <= 0", P(steps), 2, 0),
                                ("a negative bound", P(steps), -1, B)):
        w = bufs()
        rc = fwd(P(gx), P(whh), P(w["hs"]), P(w["cs"]), P(w["gates"]), None, 1.0, P(w["hdrop"]), P(w["ws"]), st, mx, T, b_arg, H, _s(dev))
        assert rc < 0, what
        rc = bwd(None, None, None, 1.0, P(whh), P(w["gates"]), P(w["hs"]), P(w["cs"]), P(w["dG"]), P(w["dGsum"]), P(w["ws"]), None, None,
                 0, st, mx, T, b_arg, H, _s(dev))
        assert rc < 0, what
        assert msk(P(w["nll"]), st, mx, T, b_arg, _s(dev)) < 0, what
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)
        for k, t in w.items():
            assert bool((t == POISON).all()), (what, k)
    assert msk(None, P(steps), 2, T, B, _s(dev)) < 0
    with pytest.raises(_lib.LvaeError):
        lib.lv_nll_mask_len_f32(None, P(steps), 2, T, B, _s(dev))


# ---- 2. the drop-in classes -------------------------------------------------------------------------------------------------------
def _var_vae(V, ni, H, nz, dev, params=None, seed=0, model_scale=0.3, emb_scale=0.5):
    return build_text_vae(V, ni, H, nz, dev, seed=seed, model_scale=model_scale, emb_scale=emb_scale, params=params, varlen=True)


def _padded_batch(B, T, V, lens, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(4, V, (B, T), generator=g, dtype=torch.int64)
    x[:, 0] = BOS
    for b, n in enumerate(lens):
        x[b, n - 1] = EOS
        x[b, n:] = PAD
    return x


def _noise(B, T, ni, H, nz, ns, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, ns, nz, generator=g).to(dev), (torch.rand(B, T - 1, ni, generator=g) < 0.5).to(torch.uint8).to(dev),
            (torch.rand(B * ns, T - 1, H, generator=g) < 0.5).to(torch.uint8).to(dev))


def _step(vae, x, klw, ns, noise):
    vae.zero_grad()
    loss, rec, kl = vae.loss(x, klw, nsamples=ns, noise=noise)
    loss.mean().backward()
    return (loss.detach().cpu(), rec.detach().cpu(), kl.detach().cpu(),
            {k: p.grad.detach().cpu().clone() for k, p in vae.named_parameters()})


def _set_masked(vae, flag):
    vae.encoder.masked = vae.decoder.masked = flag


@pytest.mark.parametrize("tag", ["a_ns1", "b_ns3", "c_wide"])
def test_parity_with_the_reference_classes(target, tag):
    _, dev = target
    fx = load("varlen_small")
    g = lambda k: fx[tag + "/" + k]                                       # noqa: E731
    V, ni, H, nz, ns = (int(g(k)) for k in ("V", "ni", "H", "nz", "ns"))
    params = {k: torch.from_numpy(g("param/" + k)) for k in ALL_KEYS}
    vae = _var_vae(V, ni, H, nz, dev, params=params)
    x = (torch.from_numpy(g("x")).to(dev), torch.from_numpy(g("lens")))
    noise = tuple(torch.from_numpy(g(k)).to(dev) for k in ("eps", "mask_in", "mask_out"))
    loss, rec, kl, grads = _step(vae, x, float(g("kl_weight")), ns, noise)
    errs = dict(loss=rel_err(loss, g("loss")), rec=rel_err(rec, g("rec")), kl=rel_err(kl, g("kl")))
    mu, logvar = vae.encode_stats(x)
    errs.update(mu=rel_err(mu, g("mu")), logvar=rel_err(logvar, g("logvar")))
    print(tag, errs)
    assert max(errs.values()) < RTOL, errs
    for k in ALL_KEYS:
        want = g("grad/" + k)
        e = rel_err(grads[k], want)
        assert e < GRAD_RTOL, (k, e)
    assert float(grads["decoder.embed.weight"][PAD].abs().max()) == 0.0
    assert float(grads["decoder.embed.weight"][V - 1].abs().max()) > 0.0 or not bool((g("x") == V - 1).any())
    vae.eval()
    with torch.no_grad():
        z = torch.from_numpy(g("z_eval")).to(dev)
        assert rel_err(vae.decoder.log_probability(x, z), g("log_probability")) < RTOL
        assert rel_err(vae.eval_inference_dist(x, z), g("eval_inference_dist")) < RTOL


def test_a_seed_gives_the_reference_weights(target):
    _, dev = target
    fx = load("varlen_small")
    V, ni, H, nz, seed = (int(fx["init/" + k]) for k in ("V", "ni", "H", "nz", "seed"))
    vae = _var_vae(V, ni, H, nz, dev, seed=seed, model_scale=float(fx["init/model_scale"]), emb_scale=float(fx["init/emb_scale"]))
    assert isinstance(vae.encoder, VarLSTMEncoder) and isinstance(vae.decoder, VarLSTMDecoder)
    assert isinstance(vae.encoder, LSTMEncoder) and isinstance(vae.decoder, LSTMDecoder)
    sd = vae.state_dict()
    plain = build_text_vae(V, ni, H, nz, dev, seed=seed)
    assert sorted(sd.keys()) == sorted(plain.state_dict().keys())
    for k in ALL_KEYS:
        assert _same(sd[k], torch.from_numpy(fx["init/param/" + k])), k
    assert vae.decoder.embed.padding_idx == PAD


def _route_equality(dev, V, ni, H, nz, B, T, lens, ns, seed, model_scale=0.3):
    vae = _var_vae(V, ni, H, nz, dev, seed=seed, model_scale=model_scale)
    x = (_padded_batch(B, T, V, lens, seed + 1).to(dev), list(lens))
    noise = _noise(B, T, ni, H, nz, ns, seed + 2, dev)
    out = {}
    for masked in (True, False):
        _set_masked(vae, masked)
        out[masked] = _step(vae, x, 0.8, ns, noise)
    (l1, r1, k1, g1), (l0, r0, k0, g0) = out[True], out[False]
    errs = dict(loss=rel_err(l1, l0), rec=rel_err(r1, r0), kl=rel_err(k1, k0))
    gerr = {k: rel_err(g1[k], g0[k]) for k in ALL_KEYS}
    print(errs, max(gerr.values()))
    assert max(errs.values()) < RTOL, errs
    for k in ALL_KEYS:
        assert float(g0[k].abs().max()) > 0 and gerr[k] < GRAD_RTOL, (k, gerr[k])
    assert float(g1["decoder.embed.weight"][PAD].abs().max()) == 0.0


def test_masked_route_equals_by_length_route(target):
    """Unsorted lengths, T > max(len), ns = 2, injected noise, B = 6."""
    _, dev = target
    _route_equality(dev, V=97, ni=12, H=20, nz=4, B=6, T=10, lens=[5, 8, 2, 5, 3, 8], ns=2, seed=31)


@pytest.mark.gpu
def test_masked_route_equals_by_length_route_at_h1024(hip_device):
    g = torch.Generator().manual_seed(5)
    lens = torch.randint(2, 25, (32,), generator=g).tolist()
    lens[3], lens[17] = 24, 2
    _route_equality(hip_device, V=2003, ni=512, H=1024, nz=32, B=32, T=24, lens=lens, ns=1, seed=41, model_scale=0.05)


def test_all_lengths_equal_T_is_the_equal_length_path_bit_for_bit(target):
    _, dev = target
    V, ni, H, nz, B, T, ns = 97, 12, 20, 4, 6, 7, 2
    var = _var_vae(V, ni, H, nz, dev, seed=51)
    plain = build_text_vae(V, ni, H, nz, dev, seed=52)
    plain.load_state_dict(var.state_dict(), strict=False)
    x = _padded_batch(B, T, V, [T] * B, 53).to(dev)
    noise = _noise(B, T, ni, H, nz, ns, 54, dev)
    with torch.no_grad():
        lv, rv, kv = var.loss((x, [T] * B), 1.0, nsamples=ns, noise=noise)
        lp, rp, kp = plain.loss(x, 1.0, nsamples=ns, noise=noise)
        mv, lvv = var.encode_stats((x, torch.full((B,), T)))
        mp, lvp = plain.encode_stats(x)
        lt = var.loss(x, 1.0, nsamples=ns, noise=noise)[1]               # a plain tensor is taken as the parent takes it
    assert _same(rv, rp) and _same(mv, mp) and _same(lvv, lvp) and _same(kv, kp) and _same(lt, rp)


def test_vae_methods_on_a_pair_agree_with_the_by_length_route(target):
    _, dev = target
    V, ni, H, nz, B, T = 97, 12, 20, 4, 6, 9
    lens = [4, 9, 2, 6, 9, 3]
    vae = _var_vae(V, ni, H, nz, dev, seed=61)
    vae.eval()
    x = (_padded_batch(B, T, V, lens, 62).to(dev), torch.tensor(lens, dtype=torch.int32).to(dev))
    g = torch.Generator().manual_seed(63)
    draws = [torch.randn(B, 5, nz, generator=g) for _ in range(2)] + [torch.randn(B, 1, nz, generator=g)]
    grid = torch.randn(7, nz, generator=g).to(dev)
    total = 2 + 3
    mh_noise = (torch.randn(B, 2, nz, generator=g).to(dev), torch.randn(total, B, 2, nz, generator=g).to(dev),
                torch.rand(total, B, 2, generator=g).to(dev))
    orig = vae.encoder._draw_eps

    def run():
        state = {"i": 0}

        def draw(batch, nsamples, nzz, device, eps=None):
            e = draws[state["i"]]
            state["i"] += 1
            assert tuple(e.shape) == (batch, nsamples, nzz)
            return e.to(device)
        vae.encoder._draw_eps = draw
        try:
            with torch.no_grad():
                res = dict(nll_iw=vae.nll_iw(x, 10, ns=5).cpu(), mi=vae.calc_mi_q(x))
        finally:
            vae.encoder._draw_eps = orig
        with torch.no_grad():
            res["post"] = vae.eval_log_model_posterior(x, grid).cpu()
            res["post_mean"] = vae.calc_model_posterior_mean(x, grid).cpu()
            res["mean"] = vae.calc_infer_mean(x).cpu()
            res["kl"] = vae.KL(x).cpu()
            res["cond"] = vae.eval_cond_ll(x, grid.unsqueeze(0).expand(B, 7, nz).contiguous()).cpu()
            assert tuple(vae.sample_from_inference(x, 3).shape) == (B, 3, nz)
            assert len(vae.reconstruct(x)) == B
            smp, info = vae.sample_from_posterior(x, 3, chains=2, burn_in=2, thin=1, std=0.5, noise=mh_noise, return_info=True)
        assert info["route"] == "step"
        res["mh"], res["mh_ratio"], res["mh_flag"] = smp.cpu(), info["ratios"].cpu(), info["accepts"].cpu()
        return res
    _set_masked(vae, True)
    a = run()
    _set_masked(vae, False)
    b = run()
    for k in ("nll_iw", "post_mean", "mean", "kl", "cond"):
        assert rel_err(a[k], b[k]) < RTOL, (k, rel_err(a[k], b[k]))
    assert float((a["post"] - b["post"]).abs().max()) < RTOL * float(b["cond"].abs().max())
    assert abs(a["mi"] - b["mi"]) < RTOL * max(1.0, abs(b["mi"]))
    # Metropolis-Hastings: the two routes' chains coincide wherever no accept decision sits on the edge
    margin = (torch.log(mh_noise[2].cpu().double()) - b["mh_ratio"].double()).abs()
    clear = ((b["mh_ratio"] >= 0) | (margin > 1e-3)).all(dim=0)          # [B][chains]
    assert bool(clear.any())
    assert torch.equal(a["mh_flag"][:, clear], b["mh_flag"][:, clear])
    sel = clear.unsqueeze(1).expand(B, 3, 2)
    assert float((a["mh"][sel] - b["mh"][sel]).abs().max()) < 1e-5


def test_refusals_come_before_any_launch(target):
    _, dev = target
    V, ni, H, nz, B, T = 53, 8, 16, 4, 4, 6
    vae = _var_vae(V, ni, H, nz, dev, seed=71)
    x = _padded_batch(B, T, V, [6, 4, 3, 2], 72).to(dev)
    z = torch.zeros(B, 1, nz, device=dev)
    calls = []
    for eng in (vae.encoder._hip, vae.decoder._hip):
        eng.ensure(dev)

    class Spy(object):
        def __init__(self, lib):
            self.lib = lib

        def __getattr__(self, name):
            calls.append(name)
            return getattr(self.lib, name)
    real_backend = E.backend_for
    E.backend_for = lambda d: Spy(real_backend(d))
    try:
        for bad in ([6, 4, 3], [6, 4, 3, 1], [7, 4, 3, 2], [6.0, 4.0, 3.0, 2.0], torch.tensor([6., 4., 3., 2.]), 5):
            with pytest.raises(ValueError):
                vae.encoder((x, bad))
            with pytest.raises(ValueError):
                vae.decoder.reconstruct_error((x, bad), z)
            with pytest.raises(ValueError):
                vae.encoder._hip.forward(x, lengths=bad)
        with pytest.raises(_lib.LvaeError, match="another device|is on"):
            vae.decoder.reconstruct_error((x, [6, 4, 3, 2]), torch.zeros(B, 1, nz, device="meta"))
        with pytest.raises(_lib.LvaeError, match="is on"):
            vae.decoder._hip.forward(x, torch.zeros(B, 1, nz, device="meta"), None, None, 0.5, 0.5, lengths=[6, 4, 3, 2])
        vae.set_precision("bf16")
        for fn in (lambda: vae.encoder((x, [6, 4, 3, 2])), lambda: vae.decoder.reconstruct_error((x, [6, 4, 3, 2]), z),
                   lambda: vae.encoder._hip.forward(x, lengths=[6, 4, 3, 2]),
                   lambda: vae.decoder._hip.forward(x, z, None, None, 0.5, 0.5, lengths=[6, 4, 3, 2])):
            with pytest.raises(_lib.LvaeError, match="exact-f32"):
                fn()
        vae.set_precision("f32")
    finally:
        E.backend_for = real_backend
    assert [c for c in calls if c.startswith("lv_")] == [], calls
    with torch.no_grad():                                         # and the same objects still work
        assert tuple(vae.loss((x, [6, 4, 3, 2]), 1.0)[0].shape) == (B,)

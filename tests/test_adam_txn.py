"""The gated Adam step (lv_adam_step_txn_f32 / lv_adam_step_scale_txn_f32) and AggressiveTextTrainer(optimizer="adam"), on the
emulator (`not gpu`) and on the MI355X: against torch.optim.Adam with a clip coefficient, under the transaction gate's void flag,
and as toy.py --optim adam steps the drop-in modules (zero_grad, loss.mean().backward(), clip_grad_norm_, Adam.step)."""
import pytest
import torch

from helpers import ALL_KEYS, build_vae, rel_err
from oracle import text_vae_oracle as O
from vae_lagging_encoder_amd import engine as _eng
from vae_lagging_encoder_amd.engine import P

N, N2 = 5003, 1301                # odd lengths: the float4 body and the scalar tail


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def target(request):
    if request.param == "emu":
        request.getfixturevalue("emu_backend")
        dev = torch.device("cpu")
    else:
        dev = request.getfixturevalue("hip_device")
    return _eng.backend_for(dev), dev


def _bufs(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(N, generator=g)
    x2 = torch.randn(N2, generator=g)
    grads = [torch.randn(N, generator=g) * (0.5 + i) for i in range(5)]
    coefs = [1.0, 0.37, 1.0, 0.81, 0.05]
    return p, x2, grads, coefs


def _run_kernel(lib, dev, p0, x20, grads, coefs, lr, betas, eps, scale, void_at=None):
    """Five gated steps on device copies; void_at: index of a step queued with the void flag up.  Returns the device state."""
    st = dict(p=p0.clone().to(dev), m=torch.zeros(N, device=dev), v=torch.zeros(N, device=dev), x2=x20.clone().to(dev))
    sc = torch.zeros(4, device=dev)                      # [lr, coef, step, void]
    sc[0] = lr
    s = _eng.stream_ptr(dev)
    st["g"] = []
    for i, (gr, c) in enumerate(zip(grads, coefs)):
        g = gr.clone().to(dev)
        sc[1] = c
        sc[3] = 1.0 if i == void_at else 0.0
        if scale:
            lib.lv_adam_step_scale_txn_f32(P(st["p"]), P(g), P(st["m"]), P(st["v"]), N, P(sc, 0), P(sc, 1), P(sc, 2), betas[0], betas[1],
                                            eps, 1, P(st["x2"]), N2, P(sc, 3), s)
        else:
            lib.lv_adam_step_txn_f32(P(st["p"]), P(g), P(st["m"]), P(st["v"]), N, P(sc, 0), P(sc, 1), P(sc, 2), betas[0], betas[1], eps,
                                      1, P(sc, 3), s)
        st["g"].append(g)
    st["step"] = float(sc[2].item())
    return st


@pytest.mark.parametrize("scale", [False, True])
def test_adam_txn_matches_torch_adam(target, scale):
    lib, dev = target
    p0, x20, grads, coefs = _bufs(dev)
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8
    st = _run_kernel(lib, dev, p0, x20, grads, coefs, lr, betas, eps, scale)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=lr, betas=betas, eps=eps)
    x2 = x20.clone()
    for gr, c in zip(grads, coefs):
        ref.grad = gr * c                                   # clip_grad_norm_ leaves the clipped gradient in .grad
        opt.step()
        x2 = x2 * c
    s = opt.state[ref]
    assert st["step"] == float(s["step"]) == 5.0
    assert rel_err(st["p"], ref.detach()) < 2e-6
    assert rel_err(st["m"], s["exp_avg"]) < 2e-6 and rel_err(st["v"], s["exp_avg_sq"]) < 2e-6
    for g, gr, c in zip(st["g"], grads, coefs):             # the clipped gradient is written back
        assert torch.equal(g.cpu(), gr * c) or (c == 1.0 and torch.equal(g.cpu(), gr))
    if scale:
        assert rel_err(st["x2"], x2) < 1e-6
    else:
        assert torch.equal(st["x2"].cpu(), x20)


@pytest.mark.parametrize("scale", [False, True])
def test_adam_txn_void_flag_leaves_everything(target, scale):
    lib, dev = target
    p0, x20, grads, _ = _bufs(dev, seed=1)
    s = _eng.stream_ptr(dev)
    p, g = p0.clone().to(dev), grads[0].clone().to(dev)
    m, v = torch.randn(N, device=dev), torch.rand(N, device=dev)
    x2 = x20.clone().to(dev)
    sc = torch.tensor([1e-3, 0.5, 7.0, 1.0], device=dev)          # void flag up, step count 7
    before = [t.clone() for t in (p, g, m, v, x2, sc)]
    if scale:
        lib.lv_adam_step_scale_txn_f32(P(p), P(g), P(m), P(v), N, P(sc, 0), P(sc, 1), P(sc, 2), 0.9, 0.999, 1e-8, 1, P(x2), N2, P(sc, 3), s)
    else:
        lib.lv_adam_step_txn_f32(P(p), P(g), P(m), P(v), N, P(sc, 0), P(sc, 1), P(sc, 2), 0.9, 0.999, 1e-8, 1, P(sc, 3), s)
    for a, b in zip((p, g, m, v, x2, sc), before):
        assert torch.equal(a.cpu().view(torch.int32), b.cpu().view(torch.int32))


def test_adam_txn_voided_then_replayed_equals_uninterrupted(target):
    lib, dev = target
    p0, x20, grads, coefs = _bufs(dev, seed=2)
    clean = _run_kernel(lib, dev, p0, x20, grads, coefs, 1e-3, (0.5, 0.999), 1e-8, True)
    # steps 0, 1 committed; step 2 voided (and with it everything behind it); then steps 2.. queued again
    part = _run_kernel(lib, dev, p0, x20, grads[:3], coefs[:3], 1e-3, (0.5, 0.999), 1e-8, True, void_at=2)
    assert part["step"] == 2.0
    sc = torch.zeros(4, device=dev)
    sc[0], sc[2] = 1e-3, part["step"]
    s = _eng.stream_ptr(dev)
    for gr, c in zip(grads[2:], coefs[2:]):
        g = gr.clone().to(dev)
        sc[1] = c
        lib.lv_adam_step_scale_txn_f32(P(part["p"]), P(g), P(part["m"]), P(part["v"]), N, P(sc, 0), P(sc, 1), P(sc, 2), 0.5, 0.999, 1e-8, 1,
                                       P(part["x2"]), N2, P(sc, 3), s)
    assert float(sc[2].item()) == clean["step"] == 5.0
    for k in ("p", "m", "v", "x2"):
        assert torch.equal(part[k].cpu(), clean[k].cpu()), k


def test_adam_refused_with_data_parallel_or_micro_batches(target):
    from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer
    _, dev = target
    vae = build_vae(50, 8, 16, 4, dev, seed=0)
    with pytest.raises(ValueError, match="adam"):
        AggressiveTextTrainer(vae, lr=1e-3, optimizer="adam", micro_batches=2)
    with pytest.raises(ValueError, match="adam"):
        AggressiveTextTrainer(vae, lr=1e-3, optimizer="adam", grad_sync=object())
    with pytest.raises(ValueError, match="optimizer"):
        AggressiveTextTrainer(vae, lr=1e-3, optimizer="rmsprop")


UPDATES = ["encoder", "encoder", "decoder", "encoder", "both", "reset", "encoder", "decoder", "both", "both"]


def _trainer_vs_dropin(dev, use_graph, decoder_grads="full", V=61, ni=8, H=16, nz=4, B=5, T=7):
    from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer
    params = O.random_params(V, ni, H, nz, seed=4, scale=0.3, emb_scale=0.5, head_scale=0.5)
    a = build_vae(V, ni, H, nz, dev, params=params)
    b = build_vae(V, ni, H, nz, dev, params=params)
    tr = AggressiveTextTrainer(a, lr=1e-3, clip=5.0, optimizer="adam", use_graph=use_graph, decoder_grads=decoder_grads)
    mk = lambda b_: (torch.optim.Adam(b.encoder.parameters(), lr=1e-3, betas=b_), torch.optim.Adam(b.decoder.parameters(), lr=1e-3, betas=b_))
    enc_opt, dec_opt = mk((0.9, 0.999))
    xs = [O.synthetic_batch(B, T, V, seed=30 + i).to(dev) for i in range(3)]
    n_enc = n_dec = 0
    for i, up in enumerate(UPDATES):
        if up == "reset":
            tr.reset_optimizer(5e-4, betas=(0.5, 0.999))               # toy.py:510-511
            enc_opt, dec_opt = mk((0.5, 0.999))
            for o in (enc_opt, dec_opt):
                o.param_groups[0]["lr"] = 5e-4
            n_enc = n_dec = 0
            continue
        x = xs[i % 3]
        eps, mi, mo = O.draw_noise(B, T, ni, H, nz, seed=50 + i)
        noise = (eps.to(dev), mi.to(torch.uint8).to(dev), mo.to(torch.uint8).to(dev))
        tr.step(x, 0.7, noise=noise, update=up)
        enc_opt.zero_grad()
        dec_opt.zero_grad()
        b.loss(x, 0.7, noise=noise)[0].mean(dim=-1).backward()
        torch.nn.utils.clip_grad_norm_(b.parameters(), 5.0)
        if up in ("encoder", "both"):
            enc_opt.step()
            n_enc += 1
        if up in ("decoder", "both"):
            dec_opt.step()
            n_dec += 1
    tr.commit()
    assert tr.adam_steps() == (n_enc, n_dec)
    sa, sb = a.state_dict(), b.state_dict()
    worst = max(rel_err(sa[k], sb[k]) for k in ALL_KEYS)
    assert worst < 1e-4, worst
    # the moments too
    ef = tr.enc.flat
    for name, p in b.encoder.named_parameters():
        st = enc_opt.state[p]
        off = ef.offsets[name]
        assert rel_err(tr.adam_m["enc"][off:off + p.numel()], st["exp_avg"].reshape(-1), floor=1e-6) < 1e-3, name
    return tr


def test_trainer_adam_matches_dropin_emulated(emu_backend):
    _trainer_vs_dropin(torch.device("cpu"), use_graph=False)


def test_trainer_sgd_default_unchanged(emu_backend):
    from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer
    vae = build_vae(40, 8, 16, 4, torch.device("cpu"), seed=0)
    tr = AggressiveTextTrainer(vae)
    assert tr.optimizer == "sgd" and tr.adam_m is None


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
def test_trainer_adam_matches_dropin(hip_device, use_graph):
    _trainer_vs_dropin(hip_device, use_graph)


@pytest.mark.gpu
def test_trainer_adam_fold_norm_decoder_grads(hip_device):
    _trainer_vs_dropin(hip_device, use_graph=False, decoder_grads="norm")

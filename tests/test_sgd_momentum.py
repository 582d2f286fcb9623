"""SGD with momentum (text.py --momentum: optim.SGD(lr, momentum), text.py:30,325-326,492-493) through every layer: the gated kernels
(lv_sgd_momentum_step_f32 / lv_sgd_momentum_step_txn_f32 / lv_sgd_momentum_step_scale_txn_f32) bit for bit against torch's CPU SGD,
AggressiveTextTrainer(momentum=mu), the drop-in optim.SGD(momentum=mu), TextTrainingLoop with args.momentum, and the replay of a
recorded reference run (tests/golden/make_golden_policy_momentum.py).  Emulator (`not gpu`) and MI355X (`gpu`)."""
import argparse
import os

import numpy as np
import pytest
import torch

import parity_common as pc
from helpers import ALL_KEYS, build_vae, load, rel_err
from oracle import text_vae_oracle as O
from vae_lagging_encoder_amd import engine as _eng
from vae_lagging_encoder_amd.engine import P

N, N2 = 5003, 1301                # odd lengths: the float4 body and the scalar tail
COEFS = [1.0, 0.37, 1.0, 0.81, 0.05]


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def target(request):
    if request.param == "emu":
        request.getfixturevalue("emu_backend")
        dev = torch.device("cpu")
    else:
        dev = request.getfixturevalue("hip_device")
    return _eng.backend_for(dev), dev


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _host_data(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    x2 = torch.randn(N2, generator=g)
    grads = [torch.randn(n, generator=g) * (0.5 + i) for i in range(5)]
    return p, x2, grads


class _Buf(object):
    """A device copy of host tensor t inside a larger allocation: `shift` floats past a 16-byte boundary (shift = 1: the kernel's
    scalar path) and four guard floats behind it, which no launch may change.  The pointer is valid for n = 0 too."""

    def __init__(self, t, dev, shift=0):
        self.n, self.shift = t.numel(), shift
        self.base = torch.full((shift + self.n + 4,), 7.0, device=dev)
        self.v = self.base[shift:shift + self.n]
        self.v.copy_(t)
        assert self.base.data_ptr() % 16 == 0

    def ptr(self):
        return P(self.base, self.shift)

    def guard_intact(self):
        return bool((self.base[self.shift + self.n:] == 7.0).all()) and bool((self.base[:self.shift] == 7.0).all())


def _launch(lib, dev, form, st, g, sc, mu, n):
    """One step in the given entry point's form.  sc = [lr, coef, void flag]."""
    s = _eng.stream_ptr(dev)
    if form == "plain":
        lib.lv_sgd_momentum_step_f32(st["p"].ptr(), g.ptr(), st["buf"].ptr(), n, P(sc, 0), P(sc, 1), mu, 1, s)
    elif form == "txn":
        lib.lv_sgd_momentum_step_txn_f32(st["p"].ptr(), g.ptr(), st["buf"].ptr(), n, P(sc, 0), P(sc, 1), mu, 1, P(sc, 2), s)
    else:
        lib.lv_sgd_momentum_step_scale_txn_f32(st["p"].ptr(), g.ptr(), st["buf"].ptr(), n, P(sc, 0), P(sc, 1), mu, 1, st["x2"].ptr(), N2,
                                               P(sc, 2), s)


def _five_steps_against_torch(lib, dev, form, mu, lr, n=N, shift=0, seed=0):
    p0, x20, grads = _host_data(n, seed)
    st = dict(p=_Buf(p0, dev, shift), buf=_Buf(torch.zeros(n), dev, shift), x2=_Buf(x20, dev))
    sc = torch.tensor([lr, 1.0, 0.0], device=dev)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([ref], lr=lr, momentum=mu)
    x2 = x20.clone()
    for i, (gr, c) in enumerate(zip(grads, COEFS)):
        g = _Buf(gr, dev, shift)
        sc[1] = c
        _launch(lib, dev, form, st, g, sc, mu, n)
        ref.grad = gr * c                                   # clip_grad_norm_ leaves the clipped gradient in .grad
        opt.step()
        x2 = x2 * c
        # the arithmetic contract: bit-identical to torch after EVERY step
        assert _same_bits(st["p"].v, ref), (i, "p")
        assert _same_bits(st["buf"].v, opt.state[ref]["momentum_buffer"]), (i, "buf")
        assert _same_bits(g.v, gr * c if c != 1.0 else gr), (i, "g")          # written back as g * c; left alone when c == 1
        assert _same_bits(st["x2"].v, x2 if form == "scale" else x20), (i, "x2")
        assert all(t.guard_intact() for t in (st["p"], st["buf"], st["x2"], g)), i
    return st


# ---------------------------------------------------------------------------------------------------------------------
# 1. five steps against torch's CPU SGD
@pytest.mark.parametrize("lr", [1.0, 0.5, 0.3])
@pytest.mark.parametrize("mu", [0.5, 0.9])
@pytest.mark.parametrize("form", ["plain", "txn", "scale"])
def test_momentum_kernel_is_bit_identical_to_torch_sgd(target, form, mu, lr):
    lib, dev = target
    _five_steps_against_torch(lib, dev, form, mu, lr)


@pytest.mark.parametrize("form", ["plain", "scale"])
def test_momentum_kernel_unaligned_buffers(target, form):
    lib, dev = target
    _five_steps_against_torch(lib, dev, form, 0.9, 0.3, shift=1, seed=3)


@pytest.mark.parametrize("n", [0, 3])
@pytest.mark.parametrize("form", ["plain", "txn", "scale"])
def test_momentum_kernel_tiny_lengths(target, form, n):
    lib, dev = target
    _five_steps_against_torch(lib, dev, form, 0.5, 0.3, n=n, seed=4)


# ---------------------------------------------------------------------------------------------------------------------
# 2. void flag up: nothing moves
@pytest.mark.parametrize("form", ["txn", "scale"])
def test_momentum_kernel_void_flag_leaves_everything(target, form):
    lib, dev = target
    p0, x20, grads = _host_data(N, seed=1)
    st = dict(p=_Buf(p0, dev), buf=_Buf(torch.randn(N, generator=torch.Generator().manual_seed(8)), dev), x2=_Buf(x20, dev))
    g = _Buf(grads[0], dev)
    sc = torch.tensor([0.3, 0.5, 1.0], device=dev)              # void flag up, clip active
    now = (st["p"].base, g.base, st["buf"].base, st["x2"].base, sc)
    before = [t.clone() for t in now]
    _launch(lib, dev, form, st, g, sc, 0.9, N)
    for a, b in zip(now, before):
        assert _same_bits(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# 3. voided then replayed == uninterrupted
def test_momentum_kernel_voided_then_replayed_equals_uninterrupted(target):
    lib, dev = target
    p0, x20, grads = _host_data(N, seed=2)
    mu, lr = 0.9, 0.3

    def run(order):
        """order: (gradient index, void flag) per queued step"""
        st = dict(p=_Buf(p0, dev), buf=_Buf(torch.zeros(N), dev), x2=_Buf(x20, dev))
        sc = torch.tensor([lr, 1.0, 0.0], device=dev)
        for i, void in order:
            g = _Buf(grads[i], dev)
            sc[1] = COEFS[i]
            sc[2] = 1.0 if void else 0.0
            _launch(lib, dev, "scale", st, g, sc, mu, N)
        return st
    clean = run([(i, False) for i in range(5)])
    # steps 0, 1 committed; step 2 queued with the flag up; then steps 2.. queued again
    part = run([(0, False), (1, False), (2, True), (2, False), (3, False), (4, False)])
    for k in ("p", "buf", "x2"):
        assert _same_bits(part[k].base, clean[k].base), k


def test_momentum_entry_points_check_their_arguments(target):
    lib, _ = target
    raw = lib.cdll
    assert raw.lv_sgd_momentum_step_f32(None, None, None, 4, None, None, 0.5, 1, None) < 0
    assert raw.lv_sgd_momentum_step_txn_f32(None, None, None, 4, None, None, 0.5, 1, None, None) < 0
    assert raw.lv_sgd_momentum_step_scale_txn_f32(None, None, None, 4, None, None, 0.5, 1, None, 4, None, None) < 0


# ---------------------------------------------------------------------------------------------------------------------
# trainer level
V_, NI, H_, NZ, B_, T_ = 61, 8, 16, 4, 5, 7
UPDATES = ["encoder", "encoder", "decoder", "encoder", "both", "reset", "encoder", "decoder", "both", "both"]


def _params():
    return O.random_params(V_, NI, H_, NZ, seed=4, scale=0.3, emb_scale=0.5, head_scale=0.5)


def _noise(dev, i, B=B_, T=T_):
    eps, mi, mo = O.draw_noise(B, T, NI, H_, NZ, seed=50 + i)
    return eps.to(dev), mi.to(torch.uint8).to(dev), mo.to(torch.uint8).to(dev)


def _trainer(vae, **kw):
    from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer
    return AggressiveTextTrainer(vae, clip=5.0, **kw)


# 4. the trainer against the drop-in modules stepped by torch.optim.SGD(momentum=0.9)
def _trainer_vs_dropin(dev, use_graph=False, decoder_grads="full", mu=0.9):
    params = _params()
    a = build_vae(V_, NI, H_, NZ, dev, params=params)
    b = build_vae(V_, NI, H_, NZ, dev, params=params)
    tr = _trainer(a, lr=1.0, momentum=mu, use_graph=use_graph, decoder_grads=decoder_grads)
    assert tr.sgd_buf is not None and tr.momentum == mu
    mk = lambda lr: (torch.optim.SGD(b.encoder.parameters(), lr=lr, momentum=mu), torch.optim.SGD(b.decoder.parameters(), lr=lr, momentum=mu))
    enc_opt, dec_opt = mk(1.0)
    xs = [O.synthetic_batch(B_, T_, V_, seed=30 + i).to(dev) for i in range(3)]
    for i, up in enumerate(UPDATES):
        if up == "reset":
            tr.reset_optimizer(0.5)                                    # text.py:492-493
            assert all(float(v.abs().max()) == 0.0 for v in tr.sgd_buf.values())
            enc_opt, dec_opt = mk(0.5)
            continue
        x = xs[i % 3]
        noise = _noise(dev, i)
        tr.step(x, 0.7, noise=noise, update=up)
        enc_opt.zero_grad()
        dec_opt.zero_grad()
        b.loss(x, 0.7, noise=noise)[0].mean(dim=-1).backward()
        torch.nn.utils.clip_grad_norm_(b.parameters(), 5.0)
        if up in ("encoder", "both"):
            enc_opt.step()
        if up in ("decoder", "both"):
            dec_opt.step()
    tr.commit()
    sa, sb = a.state_dict(), b.state_dict()
    worst = max(rel_err(sa[k], sb[k]) for k in ALL_KEYS)
    print("trainer vs drop-in: worst weight rel_err %.3g" % worst)
    assert worst < 1e-4, worst
    for key, eng, mod, opt in (("enc", tr.enc, b.encoder, enc_opt), ("dec", tr.dec, b.decoder, dec_opt)):
        for name, p in mod.named_parameters():
            off = eng.flat.offsets[name]
            e = rel_err(tr.sgd_buf[key][off:off + p.numel()], opt.state[p]["momentum_buffer"].reshape(-1), floor=1e-6)
            assert e < 1e-3, (key, name, e)
    return tr


def test_trainer_momentum_matches_dropin_emulated(emu_backend):
    _trainer_vs_dropin(torch.device("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("use_graph", [False, True])
def test_trainer_momentum_matches_dropin(hip_device, use_graph):
    _trainer_vs_dropin(hip_device, use_graph=use_graph)


@pytest.mark.gpu
def test_trainer_momentum_fold_norm_decoder_grads(hip_device):
    _trainer_vs_dropin(hip_device, decoder_grads="norm")


def _run_sequence(dev, B=B_, **kw):
    vae = build_vae(V_, NI, H_, NZ, dev, params=_params())
    tr = _trainer(vae, lr=1.0, **kw)
    xs = [O.synthetic_batch(B, T_, V_, seed=30 + i).to(dev) for i in range(3)]
    for i, up in enumerate(UPDATES):
        if up == "reset":
            tr.reset_optimizer(0.5)
            continue
        tr.step(xs[i % 3], 0.7, noise=_noise(dev, i, B=B), update=up)
    tr.commit()
    return tr, {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}


# 5. momentum off: nothing allocated, and the weights of today's trainer bit for bit
def test_momentum_zero_is_the_plain_trainer(target):
    _, dev = target
    tr0, sd0 = _run_sequence(dev, momentum=0)
    assert tr0.sgd_buf is None and tr0.momentum == 0.0
    tr1, sd1 = _run_sequence(dev)
    assert tr1.sgd_buf is None
    for k in ALL_KEYS:
        assert _same_bits(sd0[k], sd1[k]), k


def test_momentum_argument_checks(target):
    _, dev = target
    vae = build_vae(V_, NI, H_, NZ, dev, seed=0)
    with pytest.raises(ValueError, match="momentum"):
        _trainer(vae, lr=1e-3, optimizer="adam", momentum=0.9)
    with pytest.raises(ValueError, match="momentum"):
        _trainer(vae, momentum=-0.1)


# 6. a voided step in the trainer: neither weights nor velocities move, the replay advances both once
def test_trainer_voided_step_moves_neither_weights_nor_velocity(target):
    _, dev = target
    ups = ["encoder", "encoder", "decoder", "encoder", "both", "encoder"]
    xs = [O.synthetic_batch(B_, T_, V_, seed=30 + i).to(dev) for i in range(3)]

    def run(faulty, at=3):
        vae = build_vae(V_, NI, H_, NZ, dev, params=_params())
        tr = _trainer(vae, lr=1.0, momentum=0.9)
        tr.on_demote = None
        for i, up in enumerate(ups):
            if i == at:
                if faulty:
                    tr.dec.status.fill_(207)            # what a timed-out persistent launch leaves behind
                else:
                    for e in (tr.enc, tr.dec):          # the clean run changes rung by hand where the faulty one is forced to
                        _eng.demote_persistent(e)
            tr.step(xs[i % 3], 0.7, noise=_noise(dev, i), update=up)
        tr.commit()
        return tr, vae.state_dict()
    tr_f, sd_f = run(True)
    tr_c, sd_c = run(False)
    assert tr_f.recoveries == 1 and tr_c.recoveries == 0
    for k in ALL_KEYS:
        assert _same_bits(sd_f[k], sd_c[k]), k
    for k in ("enc", "dec"):
        assert float(tr_c.sgd_buf[k].abs().max()) > 0
        assert _same_bits(tr_f.sgd_buf[k], tr_c.sgd_buf[k]), k


# 7. micro-batches (B = 6: two row slices of three; 5 sentences do not split in two)
def test_trainer_momentum_with_micro_batches_emulated(emu_backend):
    dev = torch.device("cpu")
    tr1, sd1 = _run_sequence(dev, B=6, momentum=0.9, micro_batches=1)
    tr2, sd2 = _run_sequence(dev, B=6, momentum=0.9, micro_batches=2)
    worst = max(rel_err(sd2[k], sd1[k]) for k in ALL_KEYS)
    worst_v = max(rel_err(tr2.sgd_buf[k], tr1.sgd_buf[k], floor=1e-6) for k in ("enc", "dec"))
    print("micro_batches 2 vs 1: weights %.3g, velocities %.3g" % (worst, worst_v))
    assert worst < 1e-5 and worst_v < 1e-5, (worst, worst_v)


# ---------------------------------------------------------------------------------------------------------------------
# 8. the drop-in optim.SGD(momentum=0.9)
def test_dropin_sgd_momentum_matches_torch(target):
    from vae_lagging_encoder_amd import optim as lvo
    _, dev = target
    params = _params()
    a = build_vae(V_, NI, H_, NZ, dev, params=params)
    b = build_vae(V_, NI, H_, NZ, dev, params=params)
    ours = [lvo.SGD(a.encoder.parameters(), lr=0.5, momentum=0.9), lvo.SGD(a.decoder.parameters(), lr=0.5, momentum=0.9)]
    theirs = [torch.optim.SGD(b.encoder.parameters(), lr=0.5, momentum=0.9), torch.optim.SGD(b.decoder.parameters(), lr=0.5, momentum=0.9)]
    xs = [O.synthetic_batch(B_, T_, V_, seed=30 + i).to(dev) for i in range(3)]

    def round_(i, opts_a):
        x, noise = xs[i % 3], _noise(dev, i)
        for m, opts, clip in ((a, opts_a, lvo.clip_grad_norm_), (b, theirs, torch.nn.utils.clip_grad_norm_)):
            for o in opts:
                o.zero_grad()
            m.loss(x, 0.7, noise=noise)[0].mean(dim=-1).backward()
            clip(m.parameters(), 5.0)
            for o in opts:
                o.step()

    def compare():
        sa, sb = a.state_dict(), b.state_dict()
        worst = max(rel_err(sa[k], sb[k]) for k in ALL_KEYS)
        assert worst < 1e-5, worst
    for i in range(5):
        round_(i, ours)
    compare()
    # the fused route was taken: one flat velocity per engine, momentum_buffer = views into it, state_dict() in torch's layout
    for opt, mod, ref in zip(ours, (a.encoder, a.decoder), theirs):
        flat = mod._hip.flat
        buf = opt._flat_buf[id(flat)][1]
        assert buf.shape == flat.data.shape
        for name, p in mod.named_parameters():
            mb = opt.state[p]["momentum_buffer"]
            assert mb.shape == p.shape and mb.data_ptr() == buf.data_ptr() + 4 * flat.offsets[name]
        sd, sd_ref = opt.state_dict(), ref.state_dict()
        assert sorted(sd["state"].keys()) == sorted(sd_ref["state"].keys())
        for i, p in enumerate(mod.parameters()):
            assert tuple(sd["state"][i]["momentum_buffer"].shape) == tuple(p.shape)
            assert rel_err(sd["state"][i]["momentum_buffer"], sd_ref["state"][i]["momentum_buffer"], floor=1e-6) < 1e-4
    # torch's state loaded into fresh drop-in optimizers: the next step still matches
    fresh = [lvo.SGD(a.encoder.parameters(), lr=0.5, momentum=0.9), lvo.SGD(a.decoder.parameters(), lr=0.5, momentum=0.9)]
    for o, ref in zip(fresh, theirs):
        o.load_state_dict(ref.state_dict())
    round_(5, fresh)
    compare()
    for opt, mod in zip(fresh, (a.encoder, a.decoder)):
        assert id(mod._hip.flat) in opt._flat_buf


# ---------------------------------------------------------------------------------------------------------------------
# 9. TextTrainingLoop and args.momentum
def test_training_loop_honours_momentum(target):
    from vae_lagging_encoder_amd.training import TextTrainingLoop
    _, dev = target
    train = [O.synthetic_batch(4, T, V_, seed=10 + i).to(dev) for i, T in enumerate((5, 6, 4))]

    def mk_args(mu):
        return argparse.Namespace(kl_start=0.1, warm_up=1, batch_size=4, epochs=1, aggressive=0, nsamples=1, test_nepoch=5,
                                  iw_nsamples=20, momentum=mu)
    vae = build_vae(V_, NI, H_, NZ, dev, params=_params())
    loop = TextTrainingLoop(vae, train, train[:2], train[:1], mk_args(0.5), log=lambda *_: None, np_rng=np.random.RandomState(3))
    tr = loop.trainer
    assert tr.momentum == 0.5 and tr.sgd_buf is not None
    # a trainer that disagrees with args.momentum is refused, either way round
    with pytest.raises(ValueError, match="momentum"):
        TextTrainingLoop(vae, train, train[:2], train[:1], mk_args(0.5), trainer=_trainer(vae), log=lambda *_: None)
    with pytest.raises(ValueError, match="momentum"):
        TextTrainingLoop(vae, train, train[:2], train[:1], mk_args(0), trainer=_trainer(vae, momentum=0.5), log=lambda *_: None)
    TextTrainingLoop(vae, train, train[:2], train[:1], mk_args(0.5), trainer=_trainer(vae, momentum=0.5), log=lambda *_: None)
    # a learning-rate decay re-creates the optimizers (text.py:492-493): zero velocities, the new learning rate
    tr.step(train[0], 0.5, noise=_noise(dev, 0, B=4, T=5), update="both")
    tr.commit()
    assert all(float(v.abs().max()) > 0 for v in tr.sgd_buf.values())
    loop.opt.update(not_improved=1, best_loss=1.0)
    assert loop.end_of_epoch(15, 2.0, 2.0, 0.1, 3.0) is False
    assert loop.decay_cnt == 1 and loop.opt["lr"] == 0.5
    assert float(tr.scal[1].item()) == 0.5
    assert all(float(v.abs().max()) == 0.0 for v in tr.sgd_buf.values())


# ---------------------------------------------------------------------------------------------------------------------
# 10. policy replay of the recorded --momentum 0.5 run
def check_policy_replay_text_momentum(device, tmp_dir, max_epochs=None, rtol=2e-3):
    """parity_common.check_policy_replay_text for tests/golden/policy_text_momentum.npz: the reference's text.main() with
    momentum = 0.5 (19 epochs, 247 outer iterations, 600 inner encoder steps, one STOP BURNING, one decay to lr 0.5 that re-creates
    both optimizers), replayed through TextTrainingLoop with args.momentum = 0.5.  Same decisions, exactly; statistics within the
    same rtol and derived bounds (the added arithmetic is two f32 operations per element).  The epoch hook re-synchronises the
    weights AND trainer.sgd_buf from the fixture; the drift of the weights, and of every parameter's velocity slice, over one epoch
    stays under the same 5e-3."""
    from vae_lagging_encoder_amd.data import MonoTextData
    from vae_lagging_encoder_amd.factory import build_text_vae
    from vae_lagging_encoder_amd.modules.encoders.encoder import GaussianEncoderBase
    from vae_lagging_encoder_amd.training import TextTrainingLoop
    fx = load("policy_text_momentum")
    mu = float(fx["momentum"])
    assert mu == 0.5
    paths = {}
    for k in ("train", "val", "test"):
        paths[k] = os.path.join(str(tmp_dir), k + ".txt")
        with open(paths[k], "w") as fh:
            fh.write(str(fx[k + "_txt"]))
    train = MonoTextData(paths["train"])
    val = MonoTextData(paths["val"], vocab=train.vocab)
    test = MonoTextData(paths["test"], vocab=train.vocab)
    bs, nz, ni, H = int(fx["batch_size"]), int(fx["nz"]), int(fx["ni"]), int(fx["H"])
    tb = train.create_data_batch(bs, torch.device(device), batch_first=True)
    vb = val.create_data_batch(bs, torch.device(device), batch_first=True)
    sb = test.create_data_batch(bs, torch.device(device), batch_first=True)
    assert [len(tb), len(vb), len(sb)] == [int(v) for v in fx["n_lists"][:3]]
    V = len(train.vocab)
    init = {k[5:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("init/")}
    assert init["encoder.embed.weight"].shape[0] == V
    vae = build_text_vae(V, ni, H, nz, device, seed=int(fx["seed"]), params=init, dropout_in=0.0, dropout_out=0.0, vocab=train.vocab)
    epochs = int(fx["epochs"]) if max_epochs is None else max_epochs
    args = argparse.Namespace(kl_start=float(fx["kl_start"]), warm_up=int(fx["warm_up"]), batch_size=bs, epochs=epochs, aggressive=1,
                              nsamples=1, test_nepoch=int(fx["test_nepoch"]), iw_nsamples=100, momentum=mu)
    queue = pc._EpsQueue(fx, nz, device)
    rng = pc._RecordingRng(int(fx["seed"]))
    saved = GaussianEncoderBase._draw_eps
    GaussianEncoderBase._draw_eps = lambda self, batch, nsamples, nz_, dev, eps=None: queue.pop(batch, nsamples, nz_) if eps is None else saved(self, batch, nsamples, nz_, dev, eps)
    logs, drift, drift_v = [], [], []

    def resync(loop, epoch):
        st = {k[12:]: torch.from_numpy(fx[k][epoch]) for k in fx.files if k.startswith("epoch_start/")}
        tr = loop.trainer
        tr.commit()
        if epoch > 0:
            sd = vae.state_dict()
            drift.append(max(rel_err(sd[k], st[k]) for k in ALL_KEYS))
        vae.load_state_dict(st, strict=False)
        for side, eng in (("enc", tr.enc), ("dec", tr.dec)):
            flat, buf = eng.flat, tr.sgd_buf[side]
            for name, p in zip(flat.names, flat.params):
                ref = torch.from_numpy(fx["epoch_start_buf/%s/%s" % (side, name)][epoch]).reshape(-1).to(buf.device)
                seg = buf[flat.offsets[name]:flat.offsets[name] + p.numel()]
                if epoch > 0:
                    drift_v.append(rel_err(seg, ref, floor=1e-3))
                seg.copy_(ref)
    try:
        loop = TextTrainingLoop(vae, tb, vb, sb, args, n_train_sentences=len(train), log=logs.append, np_rng=rng,
                                seed=int(fx["seed"]), noise_fn=lambda x: (queue.pop(x.shape[0], 1, nz), None, None), epoch_hook=resync)
        assert loop.trainer.momentum == mu and loop.trainer.sgd_buf is not None
        out = loop.run()
    finally:
        GaussianEncoderBase._draw_eps = saved
    it = loop.iterations
    n_it = len(it)
    assert n_it == epochs * len(tb)
    print("momentum replay: weight drift per epoch %s, worst velocity drift %.3g" % (["%.2g" % d for d in drift], max(drift_v + [0.0])))
    # ---- per-iteration decisions: exact
    assert [r["batch"] for r in it] == [int(v) for v in fx["it_batch"][:n_it]]
    assert np.allclose([r["kl_weight"] for r in it], fx["it_klw"][:n_it], rtol=0, atol=1e-12)
    assert [int(r["aggressive"]) for r in it] == [int(v) for v in fx["it_aggr"][:n_it]]
    assert [r["inner_steps"] for r in it] == [int(v) for v in fx["it_inner"][:n_it]], "inner-loop exit decisions differ"
    n_picks = int(sum(fx["it_inner"][:n_it]))
    assert rng.picks[:n_picks] == [int(v) for v in fx["picks"][:n_picks]]
    # ---- per-iteration statistics of the joint step
    rec = np.array([r["rec_sum"] for r in it])
    kl = np.array([r["kl_sum"] for r in it])
    assert np.abs(rec - fx["it_rec"][:n_it]).max() <= rtol * np.abs(fx["it_rec"][:n_it]).max(), np.abs(rec - fx["it_rec"][:n_it]).max()
    assert np.abs(kl - fx["it_kl"][:n_it]).max() <= rtol * max(1.0, np.abs(fx["it_kl"][:n_it]).max()) * 5
    # ---- aggressive stop
    stop_ref = [int(v) for v in fx["stop_burning"]]
    flips = [i for i in range(1, n_it) if it[i - 1]["aggressive"] and not it[i]["aggressive"]]
    assert flips == [s for s in stop_ref if s < n_it], (flips, stop_ref)
    k = len(loop.mi_checks)
    assert k <= len(fx["mi_checks"]) and np.allclose(np.array(loop.mi_checks), fx["mi_checks"][:k], atol=2e-3)
    # ---- per-epoch table
    h = loop.history
    assert len(h) == epochs
    ref_val = fx["val"][:epochs]
    for e in range(epochs):
        assert abs(h[e]["loss"] - ref_val[e][0]) <= rtol * abs(ref_val[e][0]) + 1e-4, (e, h[e]["loss"], ref_val[e][0])
        assert abs(h[e]["kl"] - ref_val[e][1]) <= 5 * rtol * max(1.0, abs(ref_val[e][1])) + 1e-4
        assert abs(h[e]["mi"] - ref_val[e][2]) <= 5 * rtol * max(1.0, abs(ref_val[e][2])) + 1e-4
        assert abs(h[e]["ppl"] - ref_val[e][5]) <= 5 * rtol * abs(ref_val[e][5])
        assert h[e]["au"] == int(fx["au"][e])
    assert [e for e in range(epochs) if h[e]["best_updated"]] == [int(v) for v in fx["best_epochs"] if v < epochs]
    assert np.allclose([h[e]["lr_after"] for e in range(epochs)], fx["lr_by_epoch"][:epochs])
    if max_epochs is None:
        best = {k[5:]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("best/")}
        sd = vae.state_dict()
        worst = max(rel_err(sd[k], best[k]) for k in ALL_KEYS)
        assert worst < 50 * rtol, worst
        # the recorded run ends on a decay (epoch 18): the optimizers were re-created -- zero velocities, lr 0.5
        assert loop.decay_cnt == 1 and float(loop.trainer.scal[1].item()) == 0.5
        assert all(float(v.abs().max()) == 0.0 for v in loop.trainer.sgd_buf.values())
    assert max(drift + [0.0]) < 5e-3, drift
    # ... and the velocities, before the hook overwrites them: a velocity is 1 / (1 - mu) = two steps' worth of the gradients whose
    # lr-weighted sum over the epoch's steps is the weight drift bounded above, so relative to its own size (floor 1e-3: a side that
    # has not stepped yet is all zeros) it is held to the same 5e-3; a layout or offset error in sgd_buf is an error of order 1,
    # which the re-synchronisation would otherwise hide
    assert max(drift_v + [0.0]) < 5e-3, max(drift_v)
    return dict(iterations=n_it, inner_steps=int(sum(r["inner_steps"] for r in it)), eps_used=queue.pos, out=out, drift=drift)


def test_text_policy_replay_momentum_first_epochs_emulated(emu_backend, tmp_path):
    """The aggressive phase (13 inner loops, the MI stop check) and the first plain epoch on the emulator."""
    r = check_policy_replay_text_momentum("cpu", tmp_path, max_epochs=2)
    assert r["iterations"] == 26 and r["inner_steps"] == 600


@pytest.mark.gpu
def test_text_policy_replay_momentum(hip_device, tmp_path):
    r = check_policy_replay_text_momentum(hip_device, tmp_path)
    assert r["iterations"] == 247 and r["inner_steps"] == 600

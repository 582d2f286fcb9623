"""The free-bits (KL thresholding) objective: csrc/lv_freebits.hip, lv_enc_head_gated_bwd_f32 (csrc/lv_head.hip),
engine.kl_freebits_forward / reparam_kl_gated_backward, LSTMEncoderEngine.backward(head=(..., gate)), VAE.loss(free_bits=...),
AggressiveTextTrainer / AggressiveImageTrainer (free_bits=...) and the three training loops.

Kernel and engine tests run on the emulator build and on the MI355X through one fixture, with poisoned guard bands around every
output.  References: a float64 statement of the contract written here; tests/golden/freebits_small.npz (make_golden_freebits.py:
the reference's unmodified LSTMEncoder / LSTMDecoder under torch autograd, float32 and float64); oracle.text_vae_oracle and
oracle.image_vae_oracle composed into the float64 statement of a whole step.

THE DECISION RULE (a condition, not a tolerance).  A gate is a comparison, so every decision is made exact by construction: for
every compared statistic |stat - threshold| in the float64 statement must be at least twice the rounding bound of the f32 statistic
-- counted operations x 2^-24 x the sum of absolute terms; for batch means the B - 1 adds and the divide are counted too --, the
test asserts that margin and then requires the gate BIT-EXACT.  lambda is the midpoint of the widest gap between consecutive sorted
statistics in the middle half of their sorted order (rounded to float32, which is what the kernel is given), which makes the margin
hold and gives both outcomes.  Where a mode has ONE statistic (mode "batch"; "batch_dim" at nz = 1; "dim" at B = nz = 1) there is
no gap to choose: the case runs twice, with the threshold at half and at twice the statistic -- one open and one closed run.

Bounds of the values: kl_obj and stat within their counted bounds (the same count); gradients within counted bounds of their dot
products; whole steps within parity_common.RTOL / GRAD_RTOL or, where larger, 4 x the recorded float32-vs-float64 deviation of the
reference's own two runs (the rule of tests/test_svi_refine.py).
"""
import argparse
import math

import numpy as np
import pytest
import torch

from helpers import ALL_KEYS, DEC_KEYS, ENC_KEYS, build_vae, load, rel_err
from parity_common import GRAD_RTOL, RTOL
from vae_lagging_encoder_amd import engine as E
from vae_lagging_encoder_amd.engine import P

POISON = 7777.0
GUARD = 16
U = 2.0 ** -24          # unit roundoff of f32
MODES = ["dim", "batch_dim", "batch"]
MODE_NO = {"dim": 0, "batch_dim": 1, "batch": 2}


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


def _poisoned(shape, dev):
    return _guarded(torch.full(shape, POISON), dev)


def _guards_intact(buf):
    b = buf.cpu()
    return bool((b[:GUARD] == POISON).all() and (b[-GUARD:] == POISON).all())


def _untouched(buf):
    return bool((buf.cpu() == POISON).all())


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
    def __enter__(self):
        self.calls = []
        self.real = E.backend_for
        E.backend_for = lambda d: Spy(self.real(d), self.calls)
        return self.calls

    def __exit__(self, *a):
        E.backend_for = self.real


# ---- the float64 statement of the contract and the decision rule ---------------------------------------------------------------------
def _kl_terms64(mulv):
    """mulv [B][2nz] (the f32 values the kernel reads) -> KL_bj in float64 and the sum of absolute terms of each."""
    nz = mulv.shape[1] // 2
    m, l = mulv[:, :nz].double(), mulv[:, nz:].double()
    return 0.5 * (m * m + l.exp() - l - 1.0), 0.5 * (m * m + l.exp() + l.abs() + 1.0)


def _stat64(mulv, mode):
    """-> (statistic in float64, rounding bound of the f32 statistic), shaped [B][nz] / [nz] / [1].
    Counted operations of one KL_bj: a square, an exponential (2: the device exponential is good to an ulp), an add, two
    subtractions, and the product with 0.5 (exact) -- 6, taken as 8.  A batch mean adds B - 1 adds and a divide (B, taken as
    B + 1) on top of its terms' own bounds; kl_b adds nz - 1 adds (taken as nz + 1)."""
    kl, mag = _kl_terms64(mulv)
    B, nz = kl.shape
    e = 8 * U * mag
    if mode == "dim":
        return kl, e
    if mode == "batch_dim":
        return kl.sum(0) / B, e.sum(0) / B + (B + 1) * U * kl.sum(0) / B
    klb, eb = kl.sum(1), e.sum(1) + (nz + 1) * U * mag.sum(1)
    return (klb.sum() / B).view(1), (eb.sum() / B + (B + 1) * U * klb.sum() / B).view(1)


def _pick_lambdas(mulv, mode):
    """The thresholds lambda (float32-representable) this case runs with, per the decision rule of the module docstring."""
    stat, _ = _stat64(mulv, mode)
    nz = mulv.shape[1] // 2
    s = np.sort(stat.reshape(-1).numpy())
    div = nz if mode == "batch" else 1                   # mode "batch" compares against tau = nz * lambda
    if s.size == 1:
        return [float(np.float32(0.5 * s[0] / div)), float(np.float32(2.0 * s[0] / div))]
    n = s.size
    lo, hi = (n - 1) // 4, max((n - 1) // 4 + 1, -(-3 * (n - 1) // 4))
    gaps = s[lo + 1:hi + 1] - s[lo:hi]
    i = lo + int(np.argmax(gaps))
    return [float(np.float32(0.5 * (s[i] + s[i + 1]) / div))]


def _tau(lam, nz):
    return float(np.float32(float(nz) * float(lam)))     # (float)(nz * lambda), the product in double


def _fb_ref(mulv, lam, mode, check_margin=True):
    """The contract in float64 -> gate [B][nz] (bool), kl_obj [B], its rounding bound [B], stat, stat bound.
    Asserts the decision margin (every |stat - threshold| >= 2 x the statistic's rounding bound)."""
    kl, mag = _kl_terms64(mulv)
    B, nz = kl.shape
    stat, sb = _stat64(mulv, mode)
    thr = _tau(lam, nz) if mode == "batch" else lam
    if check_margin:
        margin = (stat - thr).abs() - 2 * sb
        assert bool((margin >= 0).all()), "decision margin missed: min(|stat - thr| - 2 bound) = %.3e" % float(margin.min())
    g = stat > thr
    e = 8 * U * mag
    if mode == "batch":
        gate = g.view(1, 1).expand(B, nz)
        klb = kl.sum(1)
        kl_obj = klb if bool(g) else torch.full((B,), thr, dtype=torch.float64)
        bound = e.sum(1) + (nz + 1) * U * mag.sum(1) if bool(g) else torch.zeros(B, dtype=torch.float64)
    else:
        gate = g if mode == "dim" else g.view(1, nz).expand(B, nz)
        terms = torch.where(gate, kl, torch.full_like(kl, lam))
        kl_obj = terms.sum(1)
        bound = torch.where(gate, e, torch.zeros_like(e)).sum(1) + (nz + 1) * U * torch.where(gate, mag, torch.full_like(kl, lam)).sum(1)
    return gate, kl_obj, bound, stat, sb


def _mulv(B, nz, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat((torch.randn(B, nz, generator=g) * 0.7, torch.randn(B, nz, generator=g) * 0.5), dim=1)


def _run_fb(lib, dev, mulv, lam, mode_no, with_stat=True):
    """One raw launch into poisoned, guarded outputs -> rc, kl_obj, gate, stat (views), and the three whole buffers."""
    B, nz = mulv.shape[0], mulv.shape[1] // 2
    d_mulv = mulv.to(dev)
    bk, kl_obj = _poisoned((B,), dev)
    bg, gate = _poisoned((B, nz), dev)
    bs, stat = _poisoned(((B, nz), (nz,), (1,))[min(max(mode_no, 0), 2)], dev)
    rc = getattr(lib, "_raw_lv_kl_freebits_fwd_f32")(P(d_mulv), lam, mode_no, P(kl_obj), P(gate), P(stat) if with_stat else None, B, nz,
                                                     _s(dev))
    if dev.type == "cuda":
        torch.cuda.synchronize(dev)
    return rc, kl_obj, gate, stat, (bk, bg, bs)


# ---- 1. lv_kl_freebits_fwd_f32 against the float64 statement ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nz", [1, 4, 32, 70])
@pytest.mark.parametrize("B", [1, 5, 64, 130])
def test_freebits_fwd_against_float64(target, B, nz, mode):
    lib, dev = target
    mulv = _mulv(B, nz, 1000 * B + 10 * nz + MODE_NO[mode])
    lams = _pick_lambdas(mulv, mode)
    seen = set()
    for lam in lams:
        gate64, obj64, bound, stat64, sb = _fb_ref(mulv, lam, mode)
        rc, kl_obj, gate, stat, bufs = _run_fb(lib, dev, mulv, lam, MODE_NO[mode])
        assert rc == 0 and all(_guards_intact(b) for b in bufs)
        print("B %d nz %d %s lambda %.6g: open %d / %d, min margin %.2e (2 x bound %.2e), kl_obj err %.2e (bound %.2e)" % (
            B, nz, mode, lam, int(gate64.sum()), gate64.numel(), float(((stat64 - (_tau(lam, nz) if mode == "batch" else lam)).abs()).min()),
            float(2 * sb.max()), float((kl_obj.cpu().double() - obj64).abs().max()), float(bound.max())))
        assert torch.equal(gate.cpu(), gate64.float()), "gate is not bit-exact"
        assert bool(((kl_obj.cpu().double() - obj64).abs() <= bound).all())
        assert bool(((stat.cpu().double() - stat64).abs() <= sb).all())
        seen |= set(gate64.reshape(-1).tolist())
        # stat = NULL: the same bits elsewhere
        rc2, kl_obj2, gate2, stat2, bufs2 = _run_fb(lib, dev, mulv, lam, MODE_NO[mode], with_stat=False)
        assert rc2 == 0 and _same(kl_obj2, kl_obj) and _same(gate2, gate) and _untouched(bufs2[2])
    assert seen == {True, False}, "both gate outcomes in every case"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,nz", [(1, 1), (5, 4), (64, 32), (130, 70), (5, 70), (130, 1)])
def test_freebits_fwd_open_closed_and_refusals(target, B, nz, mode):
    lib, dev = target
    mulv = _mulv(B, nz, 77 * B + nz)
    d_mulv = mulv.to(dev)
    eps = torch.zeros(B, 1, nz, device=dev)
    z, kl = torch.empty(B, 1, nz, device=dev), torch.empty(B, device=dev)
    lib.lv_reparam_kl_fwd_f32(P(d_mulv), P(eps), P(z), P(kl), B, 1, nz, _s(dev))
    # lambda = -1 through the raw entry: every gate open, kl_obj is lv_reparam_kl_fwd_f32's kl bit for bit
    rc, kl_obj, gate, stat, bufs = _run_fb(lib, dev, mulv, -1.0, MODE_NO[mode])
    assert rc == 0 and all(_guards_intact(b) for b in bufs)
    assert bool((gate.cpu() == 1.0).all()) and _same(kl_obj, kl)
    # a huge lambda closes every gate
    lam = 1000.0
    rc, kl_obj, gate, stat, bufs = _run_fb(lib, dev, mulv, lam, MODE_NO[mode])
    assert rc == 0 and all(_guards_intact(b) for b in bufs) and bool((gate.cpu() == 0.0).all())
    if mode == "batch":
        assert bool((kl_obj.cpu() == np.float32(_tau(lam, nz))).all())
    else:
        assert bool(((kl_obj.cpu().double() - nz * lam).abs() <= (nz + 1) * U * nz * lam).all())
    # a bad mode or a NULL output: an error, nothing written
    for bad in (-1, 3):
        rc, kl_obj, gate, stat, bufs = _run_fb(lib, dev, mulv, 0.1, bad)
        assert rc < 0 and all(_untouched(b) for b in bufs)
    raw = getattr(lib, "_raw_lv_kl_freebits_fwd_f32")
    bk, ko = _poisoned((B,), dev)
    bg, gt = _poisoned((B, nz), dev)
    assert raw(P(d_mulv), 0.1, MODE_NO[mode], None, P(gt), None, B, nz, _s(dev)) < 0
    assert raw(P(d_mulv), 0.1, MODE_NO[mode], P(ko), None, None, B, nz, _s(dev)) < 0
    assert raw(None, 0.1, MODE_NO[mode], P(ko), P(gt), None, B, nz, _s(dev)) < 0
    assert raw(P(d_mulv), 0.1, MODE_NO[mode], P(ko), P(gt), None, 0, nz, _s(dev)) < 0
    assert _untouched(bk) and _untouched(bg)


@pytest.mark.parametrize("nz", [1, 4, 70])
def test_freebits_batch_dim_is_dim_at_b1(target, nz):
    lib, dev = target
    mulv = _mulv(1, nz, 5 + nz)
    for lam in (0.0, 0.05, 0.3):
        a = _run_fb(lib, dev, mulv, lam, 0)
        b = _run_fb(lib, dev, mulv, lam, 1)
        assert a[0] == 0 and b[0] == 0
        assert _same(a[1], b[1]) and _same(a[2], b[2]) and _same(a[3].reshape(-1), b[3].reshape(-1))


def test_engine_wrappers_check_their_arguments(target):
    lib, dev = target
    mulv = _mulv(5, 4, 3).to(dev)
    with spying() as calls:
        for lam, mode in ((-0.1, "dim"), (float("nan"), "dim"), (float("inf"), "batch"), (0.1, "per_dim"), ("x", "dim")):
            with pytest.raises(ValueError):
                E.kl_freebits_forward(mulv, lam, mode)
        assert calls == []
    kl_obj, gate, stat = E.kl_freebits_forward(mulv, 0.2, "batch_dim", want_stat=True)
    g64, o64, bound, s64, sb = _fb_ref(mulv.cpu(), float(np.float32(0.2)), "batch_dim", check_margin=False)
    assert tuple(stat.shape) == (4,) and bool(((stat.cpu().double() - s64).abs() <= sb).all())
    with pytest.raises(ValueError):
        E.reparam_kl_gated_backward(mulv, torch.zeros(5, 1, 4, device=dev), torch.zeros(5, 1, 4, device=dev), torch.zeros(5, device=dev),
                                    torch.ones(5, 3, device=dev))


# ---- 2. the gated backward kernels against the float64 statement ------------------------------------------------------------------------
def _gates(B, nz, g):
    return [("random", (torch.rand(B, nz, generator=g) < 0.5).float()), ("zeros", torch.zeros(B, nz)), ("ones", torch.ones(B, nz))]


def _dmulv_ref(mulv, eps, dzp, dkl, gate):
    """-> dmulv [B][2nz] in float64 and its counted rounding bound (parts * ns adds, the products, two exponentials)."""
    B, ns, nz = eps.shape
    parts = dzp.shape[0]
    m, l = mulv[:, :nz].double(), mulv[:, nz:].double()
    dz, e = dzp.double().sum(0).view(B, ns, nz), eps.double()
    adz = dzp.double().abs().sum(0).view(B, ns, nz)
    sd = (0.5 * l).exp()
    gk = dkl.double().view(B, 1) * gate.double()
    dm = dz.sum(1) + gk * m
    dl = (dz * e).sum(1) * 0.5 * sd + gk * 0.5 * (l.exp() - 1.0)
    n = parts * ns + 8
    bm = n * U * (adz.sum(1) + (gk * m).abs())
    bl = n * U * ((adz * e.abs()).sum(1) * 0.5 * sd + gk.abs() * 0.5 * (l.exp() + 1.0))
    return torch.cat((dm, dl), 1), torch.cat((bm, bl), 1)


@pytest.mark.parametrize("B,nz", [(5, 4), (130, 70), (1, 1)])
@pytest.mark.parametrize("ns", [1, 3])
def test_reparam_kl_gated_bwd_against_float64(target, B, ns, nz):
    lib, dev = target
    g = torch.Generator().manual_seed(100 * B + 10 * ns + nz)
    mulv, eps = _mulv(B, nz, B + nz), torch.randn(B, ns, nz, generator=g)
    dz, dkl = torch.randn(B, ns, nz, generator=g), torch.rand(B, generator=g) + 0.1
    d = [t.to(dev) for t in (mulv, eps, dz, dkl)]
    for name, gate in _gates(B, nz, g):
        want, bound = _dmulv_ref(mulv, eps, dz.view(1, B, ns, nz), dkl, gate)
        buf, out = _poisoned((B, 2 * nz), dev)
        d_gate = gate.to(dev)
        lib.lv_reparam_kl_gated_bwd_f32(P(d[0]), P(d[1]), P(d[2]), P(d[3]), P(d_gate), P(out), B, ns, nz, _s(dev))
        assert _guards_intact(buf)
        assert bool(((out.cpu().double() - want).abs() <= bound).all()), name
        if name == "ones":
            twin = torch.empty(B, 2 * nz, device=dev)
            lib.lv_reparam_kl_bwd_f32(P(d[0]), P(d[1]), P(d[2]), P(d[3]), P(twin), B, ns, nz, _s(dev))
            assert _same(out, twin)
        if name == "zeros":
            z0 = torch.zeros(B, ns, nz, device=dev)
            lib.lv_reparam_kl_gated_bwd_f32(P(d[0]), P(d[1]), P(z0), P(d[3]), P(d_gate), P(out), B, ns, nz, _s(dev))
            assert bool((out.cpu() == 0).all())
    raw = getattr(lib, "_raw_lv_reparam_kl_gated_bwd_f32")
    buf, out = _poisoned((B, 2 * nz), dev)
    assert raw(P(d[0]), P(d[1]), P(d[2]), P(d[3]), None, P(out), B, ns, nz, _s(dev)) < 0
    assert raw(P(d[0]), P(d[1]), P(d[2]), P(d[3]), P(d[0]), P(out), B, 0, nz, _s(dev)) < 0
    assert _untouched(buf)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("H", [16, 1024])
def test_enc_head_gated_bwd_against_float64(target, H, ns, split):
    lib, dev = target
    B, nz = 5, 4
    parts = lib.lv_dec_tail_parts(H) if split else 1
    g = torch.Generator().manual_seed(H + 10 * ns + parts)
    mulv, eps = _mulv(B, nz, H + ns), torch.randn(B, ns, nz, generator=g)
    dzp = torch.randn(parts, B, ns, nz, generator=g) / math.sqrt(parts)
    dkl = torch.rand(B, generator=g) + 0.1
    hT, wlin = torch.randn(B, H, generator=g) * 0.5, torch.randn(2 * nz, H, generator=g) * 0.3
    d = [t.to(dev) for t in (mulv, eps, dzp, dkl, hT, wlin)]

    def run(entry, gate_dev, dz_dev):
        bufs = [_poisoned(s, dev) for s in ((B, 2 * nz), (B, H), (2 * nz, H))]
        a = (P(d[0]), P(d[1]), P(dz_dev), parts, P(d[3])) + ((P(gate_dev),) if gate_dev is not None else ()) + \
            (P(d[4]), P(d[5]), P(bufs[0][1]), P(bufs[1][1]), P(bufs[2][1]), B, H, ns, nz, _s(dev))
        getattr(lib, entry)(*a)
        assert all(_guards_intact(b[0]) for b in bufs)
        return [b[1] for b in bufs]
    for name, gate in _gates(B, nz, g):
        d_gate = gate.to(dev)
        dmulv, dhT, gW = run("lv_enc_head_gated_bwd_f32", d_gate, d[2])
        want, bound = _dmulv_ref(mulv, eps, dzp.view(parts, B, ns, nz), dkl, gate)
        assert bool(((dmulv.cpu().double() - want).abs() <= bound).all()), name
        # dh_T = dmulv . W_lin (2nz terms), dW_lin = dmulv^T . h_T (B terms): the dot's own count plus the operand's bound carried through
        w64, h64 = wlin.double(), hT.double()
        assert bool(((dhT.cpu().double() - want @ w64).abs() <= (2 * nz + 2) * U * (want.abs() @ w64.abs()) + bound @ w64.abs()).all()), name
        assert bool(((gW.cpu().double() - want.t() @ h64).abs() <= (B + 2) * U * (want.abs().t() @ h64.abs()) + bound.t() @ h64.abs()).all()), name
        if name == "ones":
            twin = run("lv_enc_head_bwd_f32", None, d[2])
            assert all(_same(a, b) for a, b in zip((dmulv, dhT, gW), twin))
        if name == "zeros":
            z0 = torch.zeros_like(d[2])
            assert bool((run("lv_enc_head_gated_bwd_f32", d_gate, z0)[0].cpu() == 0).all())
    raw = getattr(lib, "_raw_lv_enc_head_gated_bwd_f32")
    buf, out = _poisoned((B, 2 * nz), dev)
    assert raw(P(d[0]), P(d[1]), P(d[2]), parts, P(d[3]), None, P(d[4]), P(d[5]), P(out), P(out), P(out), B, H, ns, nz, _s(dev)) < 0
    assert _untouched(buf)


# ---- 3. lv_loss_assemble_fb[_rng]_f32 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,B,ns", [(1, 1, 1), (7, 5, 1), (7, 37, 3), (70, 3, 2)])
def test_loss_assemble_fb(target, T, B, ns):
    lib, dev = target
    s = _s(dev)
    g = torch.Generator().manual_seed(T + 31 * B + ns)
    nll = torch.rand(T, B * ns, generator=g) * 5
    kl, kl_obj = torch.rand(B, generator=g), torch.rand(B, generator=g) + 1.0
    gl = torch.rand(B, generator=g) / B
    klw, acc0 = torch.tensor([0.37]), torch.tensor([1.5, -2.0, 0.25])
    for rng in (False, True):
        def run(entry, obj):
            d = {k: v.clone().to(dev) for k, v in dict(nll=nll, kl=kl, gl=gl, klw=klw).items()}
            bufs = [_poisoned((n,), dev) for n in (B, B, B * ns, B)]              # loss, rec, rowscale, dkl
            ba, acc = _guarded(acc0, dev)
            state = torch.tensor([12345, 7], dtype=torch.int64, device=dev)
            a = (P(d["nll"]), P(d["kl"])) + ((P(obj),) if obj is not None else ()) + (P(d["klw"]), P(d["gl"])) + \
                tuple(P(b[1]) for b in bufs) + (P(acc), T, B, ns)
            getattr(lib, entry + ("_rng_f32" if rng else "_f32"))(*(a + ((P(state), 3, s) if rng else (s,))))
            assert all(_guards_intact(b[0]) for b in bufs) and _guards_intact(ba)
            assert state.cpu().tolist() == [12345, 10 if rng else 7]
            return [b[1] for b in bufs] + [acc]
        # kl_obj = kl: the bits of lv_loss_assemble_ns[_rng]_f32
        d_kl = kl.to(dev)
        for a, b in zip(run("lv_loss_assemble_fb", d_kl), run("lv_loss_assemble_ns", None)):
            assert _same(a, b)
        # another kl_obj: the float64 statement; acc[2] is the TRUE KL sum
        loss, rec, rowscale, dkl, acc = run("lv_loss_assemble_fb", kl_obj.to(dev))
        want_rec = nll.double().view(T, B, ns).sum(0).mean(1)
        want_loss = want_rec + float(klw) * kl_obj.double()
        assert rel_err(rec, want_rec) < 1e-6 and rel_err(loss, want_loss) < 1e-6
        assert torch.equal(rowscale.cpu(), (gl / ns).repeat_interleave(ns)) and torch.equal(dkl.cpu(), klw * gl)
        want_acc = acc0.double() + torch.stack([want_loss.sum(), want_rec.sum(), kl.double().sum()])
        assert rel_err(acc, want_acc) < 1e-6
        assert abs(float(acc[2].cpu()) - float(want_acc[2])) < 1e-6 * float(kl.sum()) + 1e-7
    raw = lambda n: getattr(lib, "_raw_" + n)
    t = torch.zeros(64, device=dev)
    a = (P(t),) * 10
    assert raw("lv_loss_assemble_fb_f32")(*a, 1, 1, 0, None) < 0
    assert raw("lv_loss_assemble_fb_f32")(*(a[:2] + (None,) + a[3:]), 1, 1, 1, None) < 0
    assert raw("lv_loss_assemble_fb_rng_f32")(*a, 1, 1, 1, None, 1, None) < 0


# ---- the float64 statement of a whole text step --------------------------------------------------------------------------------------
SCALES = dict(scale=0.3, emb_scale=0.5, head_scale=0.5)


def _params(V, ni, H, nz, seed):
    from oracle import text_vae_oracle as O
    return O.random_params(V, ni, H, nz, seed=seed, **SCALES)


def _text_step64(P32, x, klw, noise, lam, mode, update="encoder", lr=1.0, clip=5.0):
    """One body of the aggressive loop with the thresholded loss, composed from oracle.text_vae_oracle's functions in float64; the
    gate is formed under no_grad, as gate * KL + (1 - gate) * lambda.  lam = None: the plain step (every gate open)."""
    from oracle import text_vae_oracle as O
    eps, m_in, m_out = noise
    Q = {k: v.detach().clone().double().requires_grad_(True) for k, v in P32.items()}
    mu, lv = O.encoder_forward(Q, x)
    z, _ = O.reparam_kl(mu, lv, eps.double())
    rec = O.decoder_reconstruct_error(Q, x, z, m_in, m_out).mean(dim=1)
    KL = 0.5 * (mu.pow(2) + lv.exp() - lv - 1)
    B, nz = KL.shape
    mulv = torch.cat((mu, lv), dim=1).detach()
    if lam is None:
        gate, kl_obj = torch.ones(B, nz, dtype=torch.bool), KL.sum(1)
    else:
        gate = _fb_ref(mulv, lam, mode, check_margin=False)[0]
        g = gate.double()
        kl_obj = g[:, 0] * KL.sum(1) + (1 - g[:, 0]) * _tau(lam, nz) if mode == "batch" else (g * KL + (1 - g) * lam).sum(1)
    loss = rec + klw * kl_obj
    loss.mean().backward()
    grads = {k: (Q[k].grad if Q[k].grad is not None else torch.zeros_like(Q[k])) for k in ALL_KEYS}
    total = math.sqrt(sum(float(g.pow(2).sum()) for g in grads.values()))
    coef = min(1.0, clip / (total + 1e-6))
    keys = {"encoder": ENC_KEYS, "decoder": DEC_KEYS, "both": ALL_KEYS}[update]
    new = {k: (P32[k].double() - lr * grads[k] * coef) for k in keys}
    return dict(loss=loss.detach(), rec=rec.detach(), kl=KL.sum(1).detach(), kl_obj=kl_obj.detach(), gate=gate, mulv=mulv, grads=grads,
                total=total, coef=coef, new=new)


def _noise(B, T, ni, H, nz, ns, seed, dev):
    from oracle import text_vae_oracle as O
    eps, mi, mo = O.draw_noise(B, T, ni, H, nz, ns=ns, seed=seed)
    return (eps, mi, mo), (eps.to(dev), mi.to(torch.uint8).to(dev), mo.to(torch.uint8).to(dev))


def _text_trainer(*a, **k):
    from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer
    return AggressiveTextTrainer(*a, **k)


def _trainer_grads(tr):
    """The step wrote every gradient back clipped (g * coef): the raw ones, by state_dict name."""
    coef = tr.read_stats()["coef"]
    out = {}
    for pre, eng in (("encoder.", tr.enc), ("decoder.", tr.dec)):
        for n in eng.flat.names:
            out[pre + n] = eng.flat.gviews[n].detach().clone() / coef
    return out


# ---- 4. the reference fixture ------------------------------------------------------------------------------------------------------------
FX_CASES = ["dim_ns1", "dim_ns3", "batch_dim_ns1", "batch_dim_ns3", "batch_ns1_open", "batch_ns3_closed"]
DEV_ORDER = ["loss", "rec", "kl", "total"] + ["grad/" + k for k in ALL_KEYS] + ["new/" + k for k in ALL_KEYS]


def _fx_case(fx, tag):
    pre = tag + "/"
    d = {k[len(pre):]: fx[k] for k in fx.files if k.startswith(pre)}
    if "dev" in d:
        d["devs"] = dict(zip(DEV_ORDER, d["dev"].tolist()))
    return d


def _mode_of(tag):
    return "batch_dim" if tag.startswith("batch_dim") else ("batch" if tag.startswith("batch") else "dim")


def _within(got, ref, rtol, dev, what):
    """|got - ref| <= the larger of rtol x max|ref| and 4 x the recorded float32-vs-float64 deviation of the reference's own two runs."""
    got, ref = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(ref).double()
    err, tol = float((got - ref).abs().max()), max(rtol * float(ref.abs().max()), 4 * dev)
    print("  %-40s err %.3e tol %.3e" % (what, err, tol))
    assert err <= tol, (what, err, tol)


def _check_margin_of_fixture(c, lam, mode, nz):
    thr = _tau(lam, nz) if mode == "batch" else lam
    assert bool((np.abs(c["stat"] - thr) >= 2 * c["stat_bound"]).all()), "the fixture misses the decision margin"


@pytest.mark.parametrize("route", ["dropin", "trainer"])
@pytest.mark.parametrize("tag", FX_CASES)
def test_step_against_reference_fixture(target, tag, route):
    lib, dev = target
    fx = load("freebits_small")
    c = _fx_case(fx, tag)
    V, ni, H, nz, B, T, ns, mseed = (int(v) for v in c["dims"])
    lam, klw = float(c["hyper"][0]), float(c["hyper"][1])
    mode = _mode_of(tag)
    _check_margin_of_fixture(c, lam, mode, nz)
    gate_ref = torch.from_numpy(c["gate"]).float()
    if mode != "batch":
        assert set(gate_ref.reshape(-1).tolist()) == {0.0, 1.0}
    vae = build_vae(V, ni, H, nz, dev, params=_params(V, ni, H, nz, mseed))
    x = torch.from_numpy(c["x"]).to(dev)
    noise = tuple(torch.from_numpy(c[k]).to(dev) for k in ("eps", "mask_in", "mask_out"))
    if route == "dropin":
        enc_opt = torch.optim.SGD(vae.encoder.parameters(), lr=1.0, momentum=0)
        dec_opt = torch.optim.SGD(vae.decoder.parameters(), lr=1.0, momentum=0)
        enc_opt.zero_grad()
        dec_opt.zero_grad()
        loss, rec, kl = vae.loss(x, klw, nsamples=ns, noise=noise, free_bits=lam, free_bits_mode=mode)
        loss.mean(dim=-1).backward()
        grads = {k: p.grad.detach().clone() for k, p in vae.named_parameters()}
        total = float(torch.nn.utils.clip_grad_norm_(vae.parameters(), 5.0))
        enc_opt.step()
        gate = vae.last_free_bits_gate
    else:
        tr = _text_trainer(vae, lr=1.0, clip=5.0, nsamples=ns, free_bits=lam, free_bits_mode=mode)
        tr.step(x, klw, noise=noise)
        st = tr.read_stats()
        s = tr.static[(B, T)]
        loss, rec, kl, gate, total = s.loss, s.rec, s.kl, s.kl_gate, st["norm"]
        grads = _trainer_grads(tr)
        for k, r in (("loss_sum", "loss"), ("rec_sum", "rec"), ("kl_sum", "kl")):
            _within(st[k], float(c[r].astype(np.float64).sum()), RTOL, B * c["devs"][r], k)
        assert float((s.loss - s.rec - klw * s.kl_obj).abs().max()) <= 4 * U * float(s.loss.abs().max())
    assert torch.equal(gate.cpu(), gate_ref), "gate differs from the fixture's"
    _within(loss, c["loss"], RTOL, c["devs"]["loss"], "loss")
    _within(rec, c["rec"], RTOL, c["devs"]["rec"], "rec")
    _within(kl, c["kl"], RTOL, c["devs"]["kl"], "kl (analytic)")
    for k in ALL_KEYS:
        _within(grads[k], c["grad/" + k], GRAD_RTOL, c["devs"]["grad/" + k], "grad " + k)
    _within(total, float(c["total_norm"]), RTOL, c["devs"]["total"], "clip norm")
    sd = vae.state_dict()
    for k in ENC_KEYS:
        _within(sd[k], c["new/" + k], RTOL, c["devs"]["new/" + k], "new " + k)
    P0 = _params(V, ni, H, nz, mseed)
    for k in DEC_KEYS:
        assert torch.equal(sd[k].cpu(), P0[k]), k


def test_trajectory_against_reference_fixture(target):
    lib, dev = target
    fx = load("freebits_small")
    V, ni, H, nz, B, T, ns, mseed = (int(v) for v in fx["traj/dims"])
    lam, klw = float(fx["traj/hyper"][0]), float(fx["traj/hyper"][1])
    updates = [str(u) for u in fx["traj/updates"]]
    vae = build_vae(V, ni, H, nz, dev, params=_params(V, ni, H, nz, mseed))
    tr = _text_trainer(vae, lr=1.0, clip=5.0, free_bits=lam, free_bits_mode="batch_dim")
    for it, up in enumerate(updates):
        c = _fx_case(fx, "traj/%d" % it)
        _check_margin_of_fixture(c, lam, "batch_dim", nz)
        x = torch.from_numpy(fx["traj/x"][it]).to(dev)
        tr.reset_stats()
        tr.step(x, klw, noise=tuple(torch.from_numpy(c[k]).to(dev) for k in ("eps", "mask_in", "mask_out")), update=up)
        st = tr.read_stats()
        s = tr.static[(B, T)]
        assert torch.equal(s.kl_gate.cpu(), torch.from_numpy(c["gate"]).float()), it
        _within(s.loss, c["loss"], RTOL, c["devs"]["loss"], "step %d loss" % it)
        _within(s.rec, c["rec"], RTOL, c["devs"]["rec"], "step %d rec" % it)
        _within(s.kl, c["kl"], RTOL, c["devs"]["kl"], "step %d kl" % it)
        _within(st["norm"], float(c["total_norm"]), RTOL, c["devs"]["total"], "step %d clip norm" % it)
    sd = vae.state_dict()
    for k in ALL_KEYS:
        _within(sd[k], c["new/" + k], RTOL, c["devs"]["new/" + k], "final " + k)


# ---- 5. routes and wiring ------------------------------------------------------------------------------------------------------------------
NEW_ENTRIES = {"lv_kl_freebits_fwd_f32", "lv_reparam_kl_gated_bwd_f32", "lv_loss_assemble_fb_f32", "lv_loss_assemble_fb_rng_f32",
               "lv_enc_head_gated_bwd_f32"}
SMALL = (53, 8, 16, 4)


def _spied_step(dev, B, T, dims=SMALL, draw=False, ns=1, **kw):
    """One trainer step with every backend entry recorded -> (names of the step's launches, trainer)."""
    from oracle import text_vae_oracle as O
    V, ni, H, nz = dims
    with spying() as calls:
        vae = build_vae(V, ni, H, nz, dev, params=_params(V, ni, H, nz, 5))
        tr = _text_trainer(vae, lr=1.0, clip=5.0, nsamples=ns, **kw)
        x = O.synthetic_batch(B, T, V, seed=9).to(dev)
        n0 = len(calls)
        tr.step(x, 0.5, noise=None if draw else _noise(B, T, ni, H, nz, ns, 3, dev)[1])
        tr.commit()
        names = [n for n, _ in calls[n0:]]
    return names, tr


@pytest.mark.parametrize("draw,ns", [(False, 1), (True, 1), (False, 3)])
def test_default_route_calls_no_new_entry_and_free_bits_differs_in_three_places(target, draw, ns):
    lib, dev = target
    off, _ = _spied_step(dev, 6, 7, draw=draw, ns=ns)
    assert not set(off) & NEW_ENTRIES
    on, _ = _spied_step(dev, 6, 7, draw=draw, ns=ns, free_bits=0.05, free_bits_mode="batch_dim")
    # the three places: one launch more behind the encoder's head, the loss assembly's twin, the head backward's twin
    assemble = ("lv_loss_assemble_ns" if ns > 1 else "lv_loss_assemble") + ("_rng_f32" if draw else "_f32")
    want = []
    for n in off:
        if n == "lv_enc_head_fwd_f32":
            want += [n, "lv_kl_freebits_fwd_f32"]
        elif n == assemble:
            want.append("lv_loss_assemble_fb" + ("_rng_f32" if draw else "_f32"))
        elif n == "lv_enc_head_bwd_f32":
            want.append("lv_enc_head_gated_bwd_f32")
        else:
            want.append(n)
    assert off.count("lv_enc_head_fwd_f32") == 1 and off.count(assemble) == 1 and off.count("lv_enc_head_bwd_f32") == 1
    assert on == want and len(on) == len(off) + 1


@pytest.mark.parametrize("mode", MODES)
def test_gemm_fallback_past_the_fused_ends(target, mode):
    """B = 128, nz = 64 is beyond fused_ends_ok: the GEMM sequence with lv_reparam_kl_gated_bwd_f32, against the float64 statement."""
    from oracle import text_vae_oracle as O
    lib, dev = target
    V, ni, H, nz, B, T = 53, 8, 16, 64, 128, 4
    assert not E.fused_ends_ok(B, nz, 1)
    P0 = _params(V, ni, H, nz, 21)
    x = O.synthetic_batch(B, T, V, seed=22)
    noise, noise_d = _noise(B, T, ni, H, nz, 1, 23, dev)
    klw = 0.8
    plain = _text_step64(P0, x, klw, noise, None, mode)
    lam = _pick_lambdas(plain["mulv"].float(), mode)[0]
    r = _text_step64(P0, x, klw, noise, lam, mode)
    with spying() as calls:
        vae = build_vae(V, ni, H, nz, dev, params=P0)
        tr = _text_trainer(vae, lr=1.0, clip=5.0, free_bits=lam, free_bits_mode=mode)
        tr.step(x.to(dev), klw, noise=noise_d)
        st = tr.read_stats()
    names = [n for n, _ in calls]
    assert "lv_reparam_kl_gated_bwd_f32" in names and "lv_enc_head_gated_bwd_f32" not in names and "lv_reparam_kl_bwd_f32" not in names
    s = tr.static[(B, T)]
    # the decision rule on the step's own mulv, then the gate bit-exact -- and equal to the statement's
    own = tr.enc._ws(B, T).mulv.detach().cpu()
    gate64, obj64, bound, _, _ = _fb_ref(own, lam, mode)
    assert torch.equal(s.kl_gate.cpu(), gate64.float()) and torch.equal(gate64, r["gate"])
    assert bool(((s.kl_obj.cpu().double() - obj64).abs() <= bound).all())
    for k, ref in (("loss_sum", r["loss"].sum()), ("rec_sum", r["rec"].sum()), ("kl_sum", r["kl"].sum())):
        assert abs(st[k] - float(ref)) <= RTOL * abs(float(ref)), (k, st[k], float(ref))
    assert abs(st["norm"] - r["total"]) <= RTOL * r["total"]
    grads = _trainer_grads(tr)
    for k in ALL_KEYS:
        assert rel_err(grads[k], r["grads"][k]) < GRAD_RTOL, k
    sd = vae.state_dict()
    for k in ENC_KEYS:
        assert rel_err(sd[k], r["new"][k]) < RTOL, k


@pytest.mark.parametrize("kw", [dict(optimizer="adam", lr=1e-3), dict(momentum=0.5), dict(fold_norm=False), dict()])
@pytest.mark.parametrize("update", ["encoder", "decoder", "both"])
def test_optimizers_and_updates_respect_the_gate(target, kw, update):
    """Two steps from the same weights that differ in kl_weight alone: rec's gradient does not depend on it, so where the gate is
    closed dmulv is the same bits, and where it is open the mu half differs by (w2 - w1) / B * mu."""
    from oracle import text_vae_oracle as O
    lib, dev = target
    V, ni, H, nz = SMALL
    B, T = 6, 7
    x = O.synthetic_batch(B, T, V, seed=9).to(dev)
    noise = _noise(B, T, ni, H, nz, 1, 3, dev)[1]
    P0 = _params(V, ni, H, nz, 5)
    plain = _text_step64(P0, x.cpu(), 0.5, _noise(B, T, ni, H, nz, 1, 3, dev)[0], None, "dim")
    lam = _pick_lambdas(plain["mulv"].float(), "dim")[0]
    runs = []
    for w in (0.5, 2.0):
        vae = build_vae(V, ni, H, nz, dev, params=P0)
        tr = _text_trainer(vae, clip=5.0, free_bits=lam, free_bits_mode="dim", **dict(dict(lr=1.0), **kw))
        tr.step(x, w, noise=noise, update=update)
        st = tr.read_stats()
        assert all(math.isfinite(v) for v in st.values())
        sd = vae.state_dict()
        assert all(bool(torch.isfinite(sd[k]).all()) for k in ALL_KEYS)
        moved = [k for k in ALL_KEYS if not torch.equal(sd[k].cpu(), P0[k])]
        assert set(moved) == set({"encoder": ENC_KEYS, "decoder": DEC_KEYS, "both": ALL_KEYS}[update])
        ws = tr.enc._ws(B, T)
        runs.append((ws.dmulv.detach().cpu().clone(), ws.mulv.detach().cpu().clone(), tr.static[(B, T)].kl_gate.cpu().clone()))
    (d1, m1, g1), (d2, m2, g2) = runs
    assert torch.equal(m1, m2) and torch.equal(g1, g2) and set(g1.reshape(-1).tolist()) == {0.0, 1.0}
    _fb_ref(m1, lam, "dim")                                                  # (the decision margin holds on the step's own mulv)
    closed = g1 == 0
    assert _same(d1[:, :nz][closed], d2[:, :nz][closed]) and _same(d1[:, nz:][closed], d2[:, nz:][closed])
    want = (2.0 - 0.5) / B * m1[:, :nz].double()
    diff = (d2[:, :nz].double() - d1[:, :nz].double())
    assert bool(((diff - want)[~closed].abs() <= 1e-5 * want[~closed].abs() + 1e-7).all())


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_hipgraph_equals_eager_over_three_steps(hip_device, mode):
    from oracle import text_vae_oracle as O
    dev = hip_device
    V, ni, H, nz = SMALL
    B, T = 6, 7
    P0 = _params(V, ni, H, nz, 5)
    xs = [O.synthetic_batch(B, T, V, seed=30 + i).to(dev) for i in range(3)]
    noises = [_noise(B, T, ni, H, nz, 1, 40 + i, dev) for i in range(3)]
    plain = _text_step64(P0, xs[0].cpu(), 0.5, noises[0][0], None, mode)
    lam = _pick_lambdas(plain["mulv"].float(), mode)[0]
    out = []
    for use_graph in (False, True):
        vae = build_vae(V, ni, H, nz, dev, params=P0)
        tr = _text_trainer(vae, lr=1.0, clip=5.0, use_graph=use_graph, free_bits=lam, free_bits_mode=mode)
        rows = []
        for i, up in enumerate(("encoder", "encoder", "both")):
            tr.reset_stats()
            tr.step(xs[i], 0.5, noise=noises[i][1], update=up)
            st = tr.read_stats()
            _fb_ref(tr.enc._ws(B, T).mulv.detach().cpu(), lam, mode)          # the decision margin holds on this step's own mulv
            rows.append((st, tr.static[(B, T)].kl_gate.cpu().clone(), tr.static[(B, T)].kl_obj.cpu().clone()))
        out.append((rows, {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}))
    for (s0, g0, o0), (s1, g1, o1) in zip(out[0][0], out[1][0]):
        assert torch.equal(g0, g1)
        assert rel_err(o1, o0) < RTOL
        for k in ("loss_sum", "rec_sum", "kl_sum", "norm"):
            assert abs(s0[k] - s1[k]) <= RTOL * abs(s0[k]), k
    for k in ALL_KEYS:
        assert rel_err(out[1][1][k], out[0][1][k]) < RTOL, k


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_bf16_h1024_head_route_is_wired(hip_device, mode):
    """bf16, H = 1024, B = 8, T = 12 (the persistent recurrences): the step's own mulv is read back, gates and kl_obj are recomputed in
    float64 from it under the decision rule, and loss_sum - rec_sum = w sum kl_obj.  Not a parity claim for bf16."""
    from oracle import text_vae_oracle as O
    dev = hip_device
    V, ni, H, nz, B, T = 2003, 64, 1024, 32, 8, 12
    P0 = O.random_params(V, ni, H, nz, seed=61, scale=0.05, emb_scale=0.3, head_scale=0.2)
    x = O.synthetic_batch(B, T, V, seed=62).to(dev)
    noise = _noise(B, T, ni, H, nz, 1, 63, dev)[1]
    klw = 0.7
    # the same weights through the same route with a zero learning rate: the mulv lambda is chosen from
    vae = build_vae(V, ni, H, nz, dev, params=P0)
    probe = _text_trainer(vae, lr=0.0, clip=5.0, precision="bf16")
    probe.step(x, klw, noise=noise)
    probe.commit()
    lam = _pick_lambdas(probe.enc._ws(B, T).mulv.detach().cpu().clone(), mode)[0]
    with spying() as calls:
        vae = build_vae(V, ni, H, nz, dev, params=P0)
        tr = _text_trainer(vae, lr=1.0, clip=5.0, precision="bf16", free_bits=lam, free_bits_mode=mode)
        tr.step(x, klw, noise=noise)
        st = tr.read_stats()
    names = [n for n, _ in calls]
    assert "lv_enc_head_gated_bwd_f32" in names and "lv_kl_freebits_fwd_f32" in names
    assert any(n.startswith("lv_lstm_fwd_bf16_persist16") for n in names), "the persistent recurrence was expected at this shape"
    own = tr.enc._ws(B, T).mulv.detach().cpu()
    gate64, obj64, bound, _, _ = _fb_ref(own, lam, mode)
    s = tr.static[(B, T)]
    assert torch.equal(s.kl_gate.cpu(), gate64.float())
    if mode != "batch":
        assert set(gate64.reshape(-1).tolist()) == {True, False}
    assert bool(((s.kl_obj.cpu().double() - obj64).abs() <= bound).all())
    want = klw * float(obj64.sum())
    assert abs((st["loss_sum"] - st["rec_sum"]) - want) <= RTOL * max(abs(want), abs(st["loss_sum"]))
    kl64 = _kl_terms64(own)[0].sum()
    assert abs(st["kl_sum"] - float(kl64)) <= RTOL * float(kl64)              # the reported KL is the analytic one


def test_fences_refuse_before_any_launch(target):
    from vae_lagging_encoder_amd.trainer import AggressiveImageTrainer, SemiAmortizedTextTrainer
    lib, dev = target
    V, ni, H, nz = SMALL
    vae = build_vae(V, ni, H, nz, dev, params=_params(V, ni, H, nz, 5))
    for eng in (vae.encoder._hip, vae.decoder._hip):
        eng.ensure(dev)
    before = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    x = torch.ones(3, 5, dtype=torch.int64, device=dev)
    with spying() as calls:
        for kw in (dict(objective="iw"), dict(grad_sync=object()), dict(micro_batches=2), dict(free_bits=-0.1), dict(free_bits=float("nan")),
                   dict(free_bits=float("inf")), dict(free_bits_mode="per_dim"), dict(free_bits="much")):
            with pytest.raises(ValueError):
                _text_trainer(vae, **dict(dict(free_bits=0.1), **kw))
        with pytest.raises(ValueError, match="free_bits"):
            SemiAmortizedTextTrainer(vae, svi_steps=2, free_bits=0.1)
        for kw in (dict(free_bits=-1.0), dict(free_bits=0.1, free_bits_mode="row"), dict(free_bits=float("nan"))):
            with pytest.raises(ValueError):
                vae.loss(x, 1.0, **kw)
            with pytest.raises(ValueError):
                AggressiveImageTrainer(vae, **kw)
        assert calls == []
    assert all(torch.equal(v, before[k]) for k, v in vae.state_dict().items())
    assert vae.encoder._hip.gen == 0 or getattr(vae.encoder._hip, "last", None) is None


def test_training_loops_hand_the_fields_through(target):
    from oracle import text_vae_oracle as O
    from vae_lagging_encoder_amd.training import TextTrainingLoop, ToyTrainingLoop
    lib, dev = target
    V, ni, H, nz = SMALL
    train = [O.synthetic_batch(4, T, V, seed=10 + i).to(dev) for i, T in enumerate((5, 6, 4))]
    quiet = dict(log=lambda *_: None)

    def text_args(**kw):
        return argparse.Namespace(**dict(dict(kl_start=0.1, warm_up=1, batch_size=4, epochs=1, aggressive=0, nsamples=1, test_nepoch=5,
                                              iw_nsamples=20), **kw))

    def toy_args(**kw):
        return text_args(optim="sgd", plot_mode="multiple", num_plot=4, plot_niter=1, zmin=-2.0, zmax=2.0, dz=0.5, **kw)
    vae = build_vae(V, ni, H, nz, dev, params=_params(V, ni, H, nz, 5))
    for Loop, mk, extra in ((TextTrainingLoop, text_args, ()), (ToyTrainingLoop, toy_args, (train[0],))):
        def build(args, **kw):
            return Loop(vae, train, train[:2], train[:1], *extra, args, **dict(quiet, **kw))
        tr = build(mk(free_bits=0.25, free_bits_mode="batch_dim")).trainer
        assert tr.free_bits == 0.25 and tr.free_bits_mode == "batch_dim"
        assert build(mk()).trainer.free_bits is None                         # a namespace without the two fields: as before
        assert build(mk(free_bits=0.5)).trainer.free_bits_mode == "dim"
        with pytest.raises(ValueError, match="free_bits"):
            build(mk(free_bits=0.25), trainer=_text_trainer(vae))
        with pytest.raises(ValueError, match="free_bits"):
            build(mk(), trainer=_text_trainer(vae, free_bits=0.25))
        with pytest.raises(ValueError):
            build(mk(free_bits=-1.0))
        build(mk(free_bits=0.25, free_bits_mode="batch"), trainer=_text_trainer(vae, free_bits=0.25, free_bits_mode="batch"))
    with pytest.raises(ValueError, match="svi_steps"):
        TextTrainingLoop(vae, train, train[:2], train[:1], text_args(free_bits=0.1, svi_steps=2), **quiet)


def test_text_loop_trains_an_epoch_with_free_bits_and_evaluates_without(target):
    """One epoch of TextTrainingLoop with free bits: the training steps take the new launches, the evaluation passes do not."""
    from oracle import text_vae_oracle as O
    from vae_lagging_encoder_amd.training import TextTrainingLoop
    lib, dev = target
    V, ni, H, nz = SMALL
    train = [O.synthetic_batch(4, T, V, seed=10 + i).to(dev) for i, T in enumerate((5, 6, 4))]
    args = argparse.Namespace(kl_start=0.5, warm_up=1, batch_size=4, epochs=1, aggressive=0, nsamples=1, test_nepoch=5, iw_nsamples=2,
                              free_bits=0.05, free_bits_mode="batch_dim")
    with spying() as calls:
        vae = build_vae(V, ni, H, nz, dev, params=_params(V, ni, H, nz, 5))
        loop = TextTrainingLoop(vae, train, train[:2], train[:1], args, log=lambda *_: None, np_rng=np.random.RandomState(3))
        out = loop.run()
    names = [n for n, _ in calls]
    assert names.count("lv_kl_freebits_fwd_f32") >= len(train) and math.isfinite(out["best_loss"])
    assert names.count("lv_kl_freebits_fwd_f32") == names.count("lv_enc_head_gated_bwd_f32")          # training steps only


def test_varlen_pair_through_vae_loss(target):
    """An (x, lengths) pair through VAE.loss(free_bits=...) on VarLSTMEncoder / VarLSTMDecoder: the by-statement value from the call's
    own mu / logvar and the free_bits=None call's rec."""
    from oracle import text_vae_oracle as O
    from vae_lagging_encoder_amd.factory import build_text_vae
    lib, dev = target
    V, ni, H, nz = SMALL
    B, T = 5, 8
    try:
        vae = build_text_vae(V, ni, H, nz, dev, params=_params(V, ni, H, nz, 5), varlen=True)
    except TypeError:
        pytest.fail("factory.build_text_vae(varlen=True) is how the variable-length modules are built")
    x = O.synthetic_batch(B, T, V, seed=9).to(dev)
    lengths = torch.tensor([8, 6, 8, 5, 7])
    vae.eval()
    eps = torch.randn(B, 1, nz, generator=torch.Generator().manual_seed(4)).to(dev)
    with torch.no_grad():
        mu, lv = vae.encode_stats((x, lengths))
        l0, r0, k0 = vae.loss((x, lengths), 0.7, noise=(eps, None, None))
    mulv = torch.cat((mu, lv), dim=1).cpu()
    for mode in MODES:
        for lam in _pick_lambdas(mulv, mode):
            gate64, obj64, bound, _, _ = _fb_ref(mulv, lam, mode)
            loss, rec, kl = vae.loss((x, lengths), 0.7, noise=(eps, None, None), free_bits=lam, free_bits_mode=mode)
            assert torch.equal(vae.last_free_bits_gate.cpu(), gate64.float())
            assert _same(rec, r0) and _same(kl, k0)
            want = r0.cpu().double() + 0.7 * obj64
            assert bool(((loss.cpu().double() - want).abs() <= 0.7 * bound + 4 * U * want.abs()).all())


# ---- 6. image ---------------------------------------------------------------------------------------------------------------------------
_IMAGE_REF = {}


def _image_inputs(ns, B=6):
    g = torch.Generator().manual_seed(900 + ns)
    return (torch.rand(B, 1, 28, 28, generator=g) < 0.4).float(), torch.randn(B, ns, 32, generator=g)


def _image_step64(P, x, klw, eps, lam, mode, lr=1e-3, clip=5.0, betas=(0.9, 0.999), adam_eps=1e-8):
    """image.py:300-314 with the thresholded loss, composed from oracle.image_vae_oracle's functions in float64 (first Adam step on the
    encoder).  lam = None: the plain step."""
    from oracle import image_vae_oracle as IO
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    c = IO.Ctx(P64, train=True)
    x, eps = x.double(), eps.double()
    mu, lv = IO.encoder_forward(c, x)
    z = mu.unsqueeze(1) + eps * (0.5 * lv).exp().unsqueeze(1)
    KL = 0.5 * (mu.pow(2) + lv.exp() - lv - 1)
    B, nz = KL.shape
    rec = IO.decoder_reconstruct_error(c, x, z).mean(dim=1)
    mulv = torch.cat((mu, lv), dim=1).detach()
    if lam is None:
        gate, kl_obj = torch.ones(B, nz, dtype=torch.bool), KL.sum(1)
    else:
        gate = _fb_ref(mulv, lam, mode, check_margin=False)[0]
        g = gate.double()
        kl_obj = g[:, 0] * KL.sum(1) + (1 - g[:, 0]) * _tau(lam, nz) if mode == "batch" else (g * KL + (1 - g) * lam).sum(1)
    loss = rec + klw * kl_obj
    loss.mean().backward()
    keys = IO.param_keys(P64)
    grads = {k: (c.leaf[k].grad if k in c.leaf and c.leaf[k].grad is not None else torch.zeros_like(P64[k])) for k in keys}
    total = math.sqrt(sum(float(g.pow(2).sum()) for g in grads.values()))
    coef = min(1.0, clip / (total + 1e-6))
    upd, gclip = {}, {}
    for k in keys:
        if k.startswith("encoder."):
            g = gclip[k] = grads[k] * coef
            m, v = g * (1 - betas[0]), (1 - betas[1]) * g * g
            upd[k] = -(lr / (1 - betas[0])) * (m / (v.sqrt() / math.sqrt(1 - betas[1]) + adam_eps))
    return dict(loss=loss.detach(), rec=rec.detach(), kl=KL.sum(1).detach(), kl_obj=kl_obj.detach(), gate=gate, mulv=mulv, total=total,
                upd=upd, gclip=gclip)


def _image_sample_idx(key, numel, n=16):
    """n entries of a tensor (all of a smaller one), drawn from a generator seeded by the tensor's name alone."""
    g = torch.Generator().manual_seed(sum(ord(c) for c in key))
    return torch.randperm(numel, generator=g)[:n]


def _image_case(dev, ns, klw=0.7):
    """The model, the inputs, lambda by the decision rule on the drop-in encoder's own f32 mu / logvar, and the float64 statement
    (computed once per ns and left unchanged)."""
    import parity_common as pc
    vae = pc.build_image_vae(dev, 41)
    x, eps = _image_inputs(ns)
    P0 = {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}
    with torch.no_grad():
        mu, lv = vae.encode_stats(x.to(dev))
    own = torch.cat((mu, lv), dim=1).cpu()
    vae.load_state_dict(P0)                                                  # (the forward moved the BatchNorm running statistics)
    lam = _pick_lambdas(own, "batch_dim")[0]
    gate_own = _fb_ref(own, lam, "batch_dim")[0]                             # asserts the decision margin on the f32 mulv
    if ns not in _IMAGE_REF:
        _IMAGE_REF[ns] = (lam, _image_step64(P0, x, klw, eps, lam, "batch_dim"))
    lam_ref, r = _IMAGE_REF[ns]
    assert lam_ref == lam and torch.equal(gate_own, r["gate"]) and set(gate_own.reshape(-1).tolist()) == {True, False}
    return vae, P0, x.to(dev), eps.to(dev), klw, lam, r


# (the whole-step image tests run on the MI355X only: one such step takes minutes on the emulator; the launches they add to the
#  step are the kernels of sections 1-3, which run on both)
@pytest.mark.gpu
@pytest.mark.parametrize("ns", [1, 3])
def test_image_trainer_against_float64_statement(hip_device, ns):
    """The Adam update is held to parity_common.check_image_step_fused's bound the way that helper holds it: 2e-5 on 16 sampled
    entries of every encoder tensor (indices from a generator seeded here, before any run; _image_sample_idx).
    On top of that, every entry: Adam's first step is u = -lr g / (|g| + eps), and where |g| is within a few orders of eps = 1e-8 the
    update follows the gradient's own rounding (du/dg = -lr eps / (|g| + eps)^2), so the same 2e-5 is required of ALL entries whose
    clipped float64 gradient is at least 1e3 eps = 1e-5 -- there |du/dg| <= lr eps / g^2 = 0.1, and a gradient error of 2e-4 still
    stays inside it -- which must be at least 99 % of the encoder's entries and some of every tensor's; the rest only |u| <= lr."""
    from vae_lagging_encoder_amd.trainer import AggressiveImageTrainer
    dev = hip_device
    vae, P0, x, eps, klw, lam, r = _image_case(dev, ns)
    with spying() as calls:
        tr = AggressiveImageTrainer(vae, lr=1e-3, clip=5.0, nsamples=ns, free_bits=lam, free_bits_mode="batch_dim")
        tr.step(x, klw, eps=eps)
        st = tr.read_stats()
    names = [n for n, _ in calls]
    assert names.count("lv_kl_freebits_fwd_f32") == 1 and names.count("lv_loss_assemble_fb_f32") == 1
    assert names.count("lv_reparam_kl_gated_bwd_f32") == 1 and "lv_reparam_kl_bwd_f32" not in names and "lv_vae_loss_f32" not in names
    assert torch.equal(tr.kl_gate.cpu(), r["gate"].float())
    # the bounds of parity_common.check_image_step_fused
    for k, ref in (("loss_sum", r["loss"].sum()), ("rec_sum", r["rec"].sum()), ("kl_sum", r["kl"].sum())):
        assert abs(st[k] - float(ref)) < RTOL * abs(float(ref)), (k, st[k], float(ref))
    assert abs(st["norm"] - r["total"]) / r["total"] < 5e-4
    assert rel_err(tr.kl_obj, r["kl_obj"]) < RTOL
    sd = vae.state_dict()
    n_live = sum(int((g.abs() >= 1e-5).sum()) for g in r["gclip"].values())
    assert n_live >= 0.99 * sum(g.numel() for g in r["gclip"].values())
    for k, u in r["upd"].items():
        got = sd[k].cpu().double() - P0[k].double()
        idx = _image_sample_idx(k, u.numel())
        e = float((got.reshape(-1)[idx] - u.reshape(-1)[idx]).abs().max())
        assert e < 2e-5, (k, "sampled", e)
        live = r["gclip"][k].abs() >= 1e-5
        assert bool(live.any()), k
        e = float((got - u)[live].abs().max())
        assert e < 2e-5, (k, e)
        # (|u| <= lr; the difference of two stored f32 weights carries the rounding of the new one)
        assert float(got.abs().max()) <= 1e-3 * (1 + 1e-5) + 2 * U * (float(P0[k].abs().max()) + 1e-3), k


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [1, 3])
def test_image_dropin_loss_against_float64_statement(hip_device, ns):
    dev = hip_device
    vae, P0, x, eps, klw, lam, r = _image_case(dev, ns)
    vae.zero_grad()
    loss, rec, kl = vae.loss(x, klw, nsamples=ns, noise=(eps, None, None), free_bits=lam, free_bits_mode="batch_dim")
    loss.mean(dim=-1).backward()
    total = float(torch.nn.utils.clip_grad_norm_(vae.parameters(), 5.0))
    assert torch.equal(vae.last_free_bits_gate.cpu(), r["gate"].float())
    assert rel_err(loss, r["loss"]) < RTOL and rel_err(rec, r["rec"]) < RTOL and rel_err(kl, r["kl"]) < RTOL
    assert abs(total - r["total"]) / r["total"] < 5e-4


@pytest.mark.gpu
def test_image_hipgraph_step(hip_device):
    """Two steps under hipGraph (the eager warm-up that is captured, then a replay) against the same two steps in eager mode.  The
    learning rate is zero, so that the second step decides on the statistics the decision rule was asserted for."""
    from vae_lagging_encoder_amd.trainer import AggressiveImageTrainer
    import parity_common as pc
    dev = hip_device
    out = []
    for use_graph in (False, True):
        vae, P0, x, eps, klw, lam, r = _image_case(dev, 3)
        tr = AggressiveImageTrainer(vae, lr=0.0, clip=5.0, nsamples=3, use_graph=use_graph, free_bits=lam, free_bits_mode="batch_dim")
        rows = []
        for i in range(2):
            tr.reset_stats()
            tr.step(x, klw, eps=eps)
            rows.append((tr.read_stats(), tr.kl_gate.cpu().clone()))
        out.append(rows)
    for (s0, g0), (s1, g1) in zip(*out):
        assert torch.equal(g0, r["gate"].float()) and torch.equal(g1, r["gate"].float())
        for k in ("loss_sum", "rec_sum", "kl_sum", "norm"):
            assert abs(s0[k] - s1[k]) <= RTOL * abs(s0[k]), (k, s0[k], s1[k])


def test_image_training_loop_hands_the_fields_through(target):
    from vae_lagging_encoder_amd.training import ImageTrainingLoop
    from vae_lagging_encoder_amd.trainer import AggressiveImageTrainer
    import parity_common as pc
    lib, dev = target
    vae = pc.build_image_vae(dev, 6)
    xs = torch.rand(8, 1, 28, 28, generator=torch.Generator().manual_seed(1))

    def args(**kw):
        return argparse.Namespace(**dict(dict(kl_start=0.1, warm_up=2, batch_size=4, epochs=1, aggressive=0, nsamples=1, test_nepoch=5), **kw))
    quiet = dict(log=lambda *a: None)
    tr = ImageTrainingLoop(vae, xs, xs[:4], None, args(free_bits=0.02, free_bits_mode="batch"), **quiet).trainer
    assert tr.free_bits == float(np.float64(0.02)) and tr.free_bits_mode == "batch"
    assert ImageTrainingLoop(vae, xs, xs[:4], None, args(), **quiet).trainer.free_bits is None
    with pytest.raises(ValueError, match="free_bits"):
        ImageTrainingLoop(vae, xs, xs[:4], None, args(free_bits=0.02), trainer=AggressiveImageTrainer(vae), **quiet)
    with pytest.raises(ValueError, match="free_bits"):
        ImageTrainingLoop(vae, xs, xs[:4], None, args(), trainer=AggressiveImageTrainer(vae, free_bits=0.02), **quiet)

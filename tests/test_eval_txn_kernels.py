"""Kernel-level tests of the evaluation reductions (lv_eval.hip), the SGD half of the transaction gate (lv_optim.hip) and a few
helpers no other test names, on the emulator build (`not gpu`) and on the MI355X.

Every reference is a float64 torch restatement of the op's definition, written here.  Every 2-D input carries padding columns
(ld > C) filled with a value that wrecks the result if it is read; every output carries one extra sentinel element or column
that must come back untouched.

Tolerance rule (derived from the kernels' arithmetic, not measured): |out - ref64| <= (8 + L) * eps32 * S, with L the longest
serial f32 accumulation chain behind one output, S = max(1, sum |terms|) for plain sums and S = max(1, |ref|) for log-domain
results.  Integer outputs and "left alone" claims are compared as bit patterns.  Each test prints max(err / bound) in a line that
starts with `eval_txn_margin` (profiles/eval_txn_kernel_margins.txt keeps one run of each target)."""
import math

import pytest
import torch

from vae_lagging_encoder_amd import engine as _eng
from vae_lagging_encoder_amd.engine import P

EPS = float(torch.finfo(torch.float32).eps)
NEG_INF = float("-inf")
SENT = 12345.0                    # output sentinel
LOG_2PI = math.log(2.0 * math.pi)


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def target(request):
    if request.param == "emu":
        request.getfixturevalue("emu_backend")
        dev = torch.device("cpu")
    else:
        dev = request.getfixturevalue("hip_device")
    return _eng.backend_for(dev), dev


def _s(dev):
    return _eng.stream_ptr(dev)


def _gen(*key):
    seed = 0
    for k in key:
        seed = seed * 1009 + int(k) + 1
    return torch.Generator().manual_seed(seed % (2 ** 31))


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _padded(x, pad, fill):
    """(R, C) -> contiguous (R, C + pad) buffer whose padding columns hold `fill`."""
    buf = torch.full((x.shape[0], x.shape[1] + pad), fill, dtype=x.dtype)
    buf[:, :x.shape[1]] = x
    return buf


def _check(dev, op, case, out, ref, L, S):
    """|out - ref| <= (8 + L) eps32 S elementwise; non-finite reference entries must be reproduced exactly."""
    out = out.detach().cpu().double().reshape(-1)
    ref = ref.double().reshape(-1)
    bound = ((8.0 + L) * EPS * torch.as_tensor(S, dtype=torch.float64)).reshape(-1).expand_as(ref)
    fin = torch.isfinite(ref)
    assert torch.equal(out[~fin], ref[~fin]), (op, case, "non-finite entries differ")
    ratio = float(((out[fin] - ref[fin]).abs() / bound[fin]).max()) if bool(fin.any()) else 0.0
    _report(dev, op, case, ratio)
    assert ratio <= 1.0, (op, case, ratio)             # a NaN ratio fails too


def _report(dev, op, case, ratio):
    print("eval_txn_margin target=%s op=%s case=%s max_err_over_bound=%.4f" % ("emu" if dev.type == "cpu" else "gpu", op, case, ratio))


def _regime(name, R, C, g):
    x = torch.randn(R, C, generator=g)
    if name == "b":
        x = -900.0 + 40.0 * x
    elif name == "c":
        x = 80.0 + 10.0 * x                               # a naive exp overflows
    return x


def _lse64(x, dim=-1):
    """log sum exp in float64 by its definition (max shifted); an all -inf row gives -inf."""
    m = x.max(dim=dim, keepdim=True).values
    m0 = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    return (m0 + (x - m0).exp().sum(dim=dim, keepdim=True).log()).squeeze(dim)


# ---------------------------------------------------------------------------------------------------------------- lv_eval.hip

@pytest.mark.parametrize("regime", ["a", "b", "c"])
@pytest.mark.parametrize("R,C", [(1, 1), (5, 63), (6, 64), (7, 65), (9, 130), (3, 1000)])
def test_logsumexp_rows(target, R, C, regime):
    lib, dev = target
    x = _regime(regime, R, C, _gen(1, R, C, ord(regime)))
    if C > 1:
        for r in range(R):
            x[r, (7 * r + 1) % C] = NEG_INF                # some -inf entries, never a whole row here
    if R > 1:
        x[R - 1, :] = NEG_INF                             # a row of all -inf: -inf, not NaN
    add = -math.log(10.0)
    xin = _padded(x, 3, float("nan")).to(dev)
    out = torch.full((R + 1,), SENT, device=dev)
    lib.lv_logsumexp_rows_f32(P(xin), C + 3, R, C, add, P(out), _s(dev))
    o = out.cpu()
    assert float(o[R]) == SENT
    ref = _lse64(x.double()) + add
    if R > 1:
        assert float(o[R - 1]) == NEG_INF
    _check(dev, "logsumexp_rows", "%dx%d/%s" % (R, C, regime), o[:R], ref, (C + 63) // 64 + 6, ref.abs().clamp(min=1.0))


@pytest.mark.parametrize("R,C", [(1, 1), (2, 65)])
def test_logsumexp_rows_all_neg_inf(target, R, C):
    lib, dev = target
    xin = _padded(torch.full((R, C), NEG_INF), 2, float("nan")).to(dev)
    out = torch.full((R + 1,), SENT, device=dev)
    lib.lv_logsumexp_rows_f32(P(xin), C + 2, R, C, -math.log(10.0), P(out), _s(dev))
    assert _same_bits(out, torch.tensor([NEG_INF] * R + [SENT]))


@pytest.mark.parametrize("with_addrow", [False, True])
@pytest.mark.parametrize("regime", ["a", "c"])
@pytest.mark.parametrize("R,C", [(1, 1), (2, 255), (2, 257), (3, 300), (5, 1000)])
def test_log_softmax_rows(target, R, C, regime, with_addrow):
    lib, dev = target
    g = _gen(2, R, C, ord(regime))
    x = _regime(regime, R, C, g)
    if C > 1:
        for r in range(R):
            x[r, (11 * r + 2) % C] = NEG_INF
    addrow = -(torch.randn(R, generator=g) * 3.0).abs()        # a hypothesis' running log-probability: <= 0
    ldo = C + 2
    xin = _padded(x, 3, float("nan")).to(dev)
    out = torch.full((R, ldo), SENT, device=dev)
    ad = addrow.to(dev)
    lib.lv_log_softmax_rows_f32(P(xin), C + 3, R, C, P(ad) if with_addrow else None, P(out), ldo, _s(dev))
    o = out.cpu()
    assert _same_bits(o[:, C:], torch.full((R, ldo - C), SENT))
    ref = x.double() - _lse64(x.double()).unsqueeze(1)
    if with_addrow:
        ref = ref + addrow.double().unsqueeze(1)
    _check(dev, "log_softmax_rows", "%dx%d/%s/%s" % (R, C, regime, "addrow" if with_addrow else "plain"), o[:, :C], ref,
           (C + 255) // 256 + 9, ref.abs().clamp(min=1.0))


@pytest.mark.parametrize("prior", [False, True])
@pytest.mark.parametrize("B,ns,nz", [(1, 1, 1), (5, 3, 40), (130, 2, 7)])
def test_gauss_logpdf(target, B, ns, nz, prior):
    lib, dev = target
    g = _gen(3, B, ns, nz)
    mu = torch.randn(B, nz, generator=g)
    logvar = torch.rand(B, nz, generator=g) * 10.0 - 8.0                 # [-8, 2]
    z = mu.unsqueeze(1) + torch.randn(B, ns, nz, generator=g) * (0.5 * logvar).exp().unsqueeze(1)
    if prior:
        z = torch.randn(B, ns, nz, generator=g)
    out = torch.full((B * ns + 1,), SENT, device=dev)
    zd, md, ld = z.contiguous().to(dev), mu.to(dev), logvar.to(dev)
    lib.lv_gauss_logpdf_f32(P(zd), None if prior else P(md), None if prior else P(ld), P(out), B, ns, nz, _s(dev))
    o = out.cpu()
    assert float(o[B * ns]) == SENT
    z64 = z.double()
    if prior:
        q = z64 ** 2
        ref = -0.5 * q.sum(-1) - 0.5 * nz * LOG_2PI
        S = 0.5 * q.sum(-1) + 0.5 * nz * LOG_2PI
    else:
        m64, l64 = mu.double().unsqueeze(1), logvar.double().unsqueeze(1)
        q = (z64 - m64) ** 2 / l64.exp()
        ref = -0.5 * q.sum(-1) - 0.5 * (nz * LOG_2PI + l64.sum(-1))
        S = 0.5 * q.sum(-1) + 0.5 * (nz * LOG_2PI + l64.abs().sum(-1))   # a plain sum: the magnitudes of its terms
    _check(dev, "gauss_logpdf", "%dx%dx%d/%s" % (B, ns, nz, "prior" if prior else "posterior"), o[:B * ns], ref, nz, S.clamp(min=1.0))


@pytest.mark.parametrize("Bx,Bz,nz", [(3, 3, 1), (70, 70, 7), (65, 257, 5), (300, 130, 32)])
def test_calc_mi(target, Bx, Bz, nz):
    """GaussianEncoderBase.calc_mi (modules/encoders/encoder.py:111-145) restated in float64: out[1] = mean_b(-0.5 nz log 2pi -
    0.5 sum_k (1 + logvar)), out[2] = mean_i (logsumexp_j log N(z_i; mu_j, var_j) - log Bx), out[0] = out[1] - out[2].  out[0] is
    formed in double from the two means and rounded once, so its bound is the sum of the other two."""
    lib, dev = target
    g = _gen(4, Bx, Bz, nz)
    mu = torch.randn(Bx, nz, generator=g)
    logvar = 0.5 * torch.randn(Bx, nz, generator=g) - 1.0
    src = torch.arange(Bz) % Bx
    z = (mu[src] + torch.randn(Bz, nz, generator=g) * (0.5 * logvar[src]).exp()).contiguous()
    ws = torch.full((Bz + 1,), SENT, device=dev)
    out = torch.full((4,), SENT, device=dev)
    md, ld, zd = mu.to(dev), logvar.to(dev), z.to(dev)
    lib.lv_calc_mi_f32(P(md), P(ld), P(zd), P(ws), P(out), Bx, Bz, nz, _s(dev))
    o = out.cpu()
    assert float(o[3]) == SENT and float(ws.cpu()[Bz]) == SENT
    m64, l64, z64 = mu.double(), logvar.double(), z.double()
    ne = (-0.5 * nz * LOG_2PI - 0.5 * (1.0 + l64).sum(-1)).mean()
    dens = -0.5 * ((z64.unsqueeze(1) - m64.unsqueeze(0)) ** 2 / l64.exp().unsqueeze(0)).sum(-1) - 0.5 * (nz * LOG_2PI + l64.sum(-1)).unsqueeze(0)
    log_qz = _lse64(dens, dim=1) - math.log(Bx)
    lq = log_qz.mean()
    case = "%dx%dx%d" % (Bx, Bz, nz)
    S1 = max(1.0, float((0.5 * nz * LOG_2PI + 0.5 * (1.0 + l64).abs().sum(-1)).mean()))
    S2 = max(1.0, abs(float(lq)))
    L1, L2 = nz + (Bx + 255) // 256 + 6, nz + (Bx + 63) // 64 + 6
    _check(dev, "calc_mi.neg_entropy", case, o[1:2], ne.reshape(1), L1, S1)
    _check(dev, "calc_mi.log_qz", case, o[2:3], lq.reshape(1), L2, S2)
    b0 = (8.0 + L1) * EPS * S1 + (8.0 + L2) * EPS * S2
    r0 = abs(float(o[0]) - float(ne - lq)) / b0
    _report(dev, "calc_mi.mi", case, r0)
    assert r0 <= 1.0, r0
    # the per-sample log q(z_i) the first stage leaves in ws
    _check(dev, "calc_mi.ws", case, ws.cpu()[:Bz], log_qz, L2, log_qz.abs().clamp(min=1.0))


@pytest.mark.parametrize("B,nz", [(1, 1), (5, 300), (33, 257)])
def test_au_accum(target, B, nz):
    lib, dev = target
    g = _gen(5, B, nz)
    mu = torch.randn(B, nz, generator=g) * 2.0 + 0.5
    acc0 = torch.randn(nz, generator=g) * 3.0                  # the kernel accumulates: start non-zero
    mean = (mu.double().mean(0) + 0.1 * torch.randn(nz, generator=g).double()).float()
    md, mean_d = mu.to(dev), mean.to(dev)
    for name, mp in (("sum", None), ("var", mean_d)):
        acc = torch.cat([acc0, torch.tensor([SENT])]).to(dev)
        lib.lv_au_accum_f32(P(md), P(mp), P(acc), B, nz, _s(dev))
        a = acc.cpu()
        assert float(a[nz]) == SENT
        terms = mu.double() if mp is None else (mu.double() - mean.double()) ** 2
        ref = acc0.double() + terms.sum(0)
        S = (acc0.double().abs() + terms.abs().sum(0)).clamp(min=1.0)
        _check(dev, "au_accum." + name, "%dx%d" % (B, nz), a[:nz], ref, B + 1, S)


@pytest.mark.parametrize("R,C", [(1, 1), (5, 63), (6, 130), (9, 1000)])
def test_argmax_rows(target, R, C):
    """Integer-valued entries from {0..3}: ties fall across lanes and across 64-column strides; the lowest index wins, as
    torch.argmax on CPU.  The padding columns hold a value larger than every entry."""
    lib, dev = target
    x = torch.randint(0, 4, (R, C), generator=_gen(6, R, C)).float()
    want = []
    if R > 1:
        x[1, :] = 2.0
        x[1, C - 1] = 7.0                                   # unique maximum in the last column
        x[2, :] = NEG_INF                                   # all -inf: 0
    if R > 3:
        x[3, :] = 1.0                                       # every column ties
        x[4, :] = 0.0
        x[4, C // 2] = 3.0
        x[4, C - 1] = 3.0                                   # two maxima, possibly on the same lane of different strides
    for r in range(R):
        row = x[r].tolist()
        best = max(row)
        want.append(0 if best == NEG_INF else row.index(best))
    xin = _padded(x, 4, 1e9).to(dev)
    idx = torch.full((R + 1,), -77, dtype=torch.int64, device=dev)
    lib.lv_argmax_rows_f32(P(xin), C + 4, R, C, P(idx), _s(dev))
    assert torch.equal(idx.cpu(), torch.tensor(want + [-77], dtype=torch.int64))


def _sample_logits(C):
    """One row of logits; for C > 6 the first three, the last three and one middle column have probability zero, and the first
    and last columns of positive probability are given a logit of 2 (p >= 4e-3 at C = 1000, far above the f32 running sum's
    worst-case error C * eps32 = 1.2e-4, so that the edge draws below have one right answer)."""
    x = torch.randn(C, generator=_gen(7, C))
    lo, hi = 0, C - 1
    if C > 6:
        x[:3] = NEG_INF
        x[C - 3:] = NEG_INF
        x[C // 2] = NEG_INF
        lo, hi = 3, C - 4
        x[lo] = 2.0
        x[hi] = 2.0
    p = (x.double() - x.double().max()).exp()
    p = p / p.sum()
    return x, p, lo, hi


def _run_sample(lib, dev, x, u):
    R, C = u.numel(), x.numel()
    xin = _padded(x.unsqueeze(0).expand(R, C), 5, float("nan")).to(dev)
    idx = torch.full((R + 1,), -77, dtype=torch.int64, device=dev)
    ud = u.float().to(dev)
    lib.lv_sample_rows_f32(P(xin), C + 5, R, C, P(ud), P(idx), _s(dev))
    out = idx.cpu()
    assert int(out[R]) == -77
    return out[:R]


@pytest.mark.parametrize("C", [1, 6, 64, 65, 130, 1000])
def test_sample_rows_interior_draws(target, C):
    """For every column k with p[k] >= 1e-3, u at 1/4, 1/2 and 3/4 of (cdf[k-1], cdf[k]) must pick exactly k: the margin to the
    interval's ends is >= 2.5e-4, the f32 running sum's worst case C * eps32 <= 1.2e-4."""
    lib, dev = target
    x, p, _, _ = _sample_logits(C)
    cdf = p.cumsum(0)
    us, want = [], []
    for k in range(C):
        if float(p[k]) >= 1e-3:
            left = float(cdf[k - 1]) if k > 0 else 0.0
            for f in (0.25, 0.5, 0.75):
                us.append(left + f * (float(cdf[k]) - left))
                want.append(k)
    assert us
    got = _run_sample(lib, dev, x, torch.tensor(us, dtype=torch.float64))
    assert torch.equal(got, torch.tensor(want, dtype=torch.int64))


@pytest.mark.parametrize("C", [1, 6, 64, 65, 130, 1000])
def test_sample_rows_edge_draws(target, C):
    """A column of probability zero is never drawn (torch.multinomial never returns one): u = 0 and u = 2^-30 give the first
    column with p > 0, u = 1 - 2^-24 (the largest f32 below 1) the last one."""
    lib, dev = target
    x, p, lo, hi = _sample_logits(C)
    assert float(p[lo]) > 2.0 ** -20 and float(p[hi]) > 4 * C * EPS
    got = _run_sample(lib, dev, x, torch.tensor([0.0, 2.0 ** -30, 1.0 - 2.0 ** -24], dtype=torch.float64))
    assert got.tolist() == [lo, lo, hi]


def test_sample_rows_no_positive_weight(target):
    """Only when no column has positive weight (all -inf: the row maximum is -inf, every weight NaN) is C - 1 returned."""
    lib, dev = target
    got = _run_sample(lib, dev, torch.full((70,), NEG_INF), torch.tensor([0.0, 0.5], dtype=torch.float64))
    assert got.tolist() == [69, 69]


# ------------------------------------------------------------------------------------------------- the SGD transaction gate

TXN0 = [4.0, 1.5, 2.5, 3.5]                  # txn[1..4]: steps committed, pending loss / rec / kl sums
ACC0 = [10.0, 20.0, 30.0]
GOOD_ACC = [11.5, 22.5, 33.5]


def _gate_inputs(dev, s1, s2, gd, v, with_acc=True):
    st = torch.tensor([s1 if s1 is not None else 99, s2 if s2 is not None else 99], dtype=torch.int32, device=dev)
    guard = torch.tensor([SENT, gd if gd is not None else 9.0, SENT], device=dev)
    txn = torch.tensor([float(v)] + TXN0 + [SENT], device=dev)
    acc = torch.tensor(ACC0 + [SENT], device=dev) if with_acc else None
    ptrs = (P(st, 0) if s1 is not None else None, P(st, 1) if s2 is not None else None, P(guard, 1) if gd is not None else None,
            P(txn), P(acc))
    return st, guard, txn, acc, ptrs


def _gate_check(s1, s2, gd, v, st, guard, txn, acc):
    good = s1 in (None, 0) and s2 in (None, 0) and gd in (None, 0.0) and v == 0
    want_txn = [0.0, 5.0, 0.0, 0.0, 0.0, SENT] if good else [1.0, 4.0, 0.0, 0.0, 0.0, SENT]
    assert _same_bits(txn, torch.tensor(want_txn)), (s1, s2, gd, v, txn.cpu().tolist())
    if acc is not None:
        assert _same_bits(acc, torch.tensor((GOOD_ACC if good else ACC0) + [SENT])), (s1, s2, gd, v, acc.cpu().tolist())
    # the gate only reads its inputs
    assert st.cpu().tolist() == [s1 if s1 is not None else 99, s2 if s2 is not None else 99]
    assert _same_bits(guard, torch.tensor([SENT, gd if gd is not None else 9.0, SENT]))
    return good


def _coef_norm_check(coef, norm, sumsq64, max_norm):
    """norm = sqrt(sumsq), coef = min(1, max_norm / (norm + 1e-6)) from an EXACT sumsq: a square root, an add and a divide, each
    within an ulp -> 4 eps32 relative."""
    n64 = math.sqrt(sumsq64)
    c64 = min(1.0, max_norm / (n64 + 1e-6))
    assert float(coef.cpu()[1]) == SENT and float(norm.cpu()[1]) == SENT
    ratio = max(abs(float(norm.cpu()[0]) - n64) / (4 * EPS * max(1.0, n64)), abs(float(coef.cpu()[0]) - c64) / (4 * EPS))
    assert ratio <= 1.0, ratio
    return ratio


GATE_ROWS_1_GOOD_3_BAD = [(0, 0, 0.0), (3, 0, 0.0), (0, -1, 0.0), (0, 0, 0.25)]       # one cause each


def test_gate_truth_table_clip_coef(target):
    lib, dev = target
    sumsq = torch.tensor([49.0, SENT], device=dev)
    n_good, worst = 0, 0.0
    for s1 in (None, 0, 3):
        for s2 in (None, 0, -1):
            for gd in (None, 0.0, 0.25):
                for v in (0, 1):
                    st, guard, txn, acc, ptrs = _gate_inputs(dev, s1, s2, gd, v)
                    coef = torch.tensor([SENT, SENT], device=dev)
                    norm = torch.tensor([SENT, SENT], device=dev)
                    lib.lv_clip_coef_txn_f32(P(sumsq), 5.0, P(coef), P(norm), *ptrs, _s(dev))
                    n_good += _gate_check(s1, s2, gd, v, st, guard, txn, acc)
                    worst = max(worst, _coef_norm_check(coef, norm, 49.0, 5.0))           # correct either way
    _report(dev, "clip_coef_txn", "54 gate rows", worst)
    assert n_good == 8
    assert _same_bits(sumsq, torch.tensor([49.0, SENT]))
    for s1, s2, gd in GATE_ROWS_1_GOOD_3_BAD:                        # acc = NULL
        st, guard, txn, acc, ptrs = _gate_inputs(dev, s1, s2, gd, 0, with_acc=False)
        coef = torch.tensor([SENT, SENT], device=dev)
        lib.lv_clip_coef_txn_f32(P(sumsq), 5.0, P(coef), None, *ptrs, _s(dev))
        assert _gate_check(s1, s2, gd, 0, st, guard, txn, None) == ((s1, s2, gd) == (0, 0, 0.0))


@pytest.mark.parametrize("fold", [False, True])
def test_gate_through_clip_norm2(target, fold):
    lib, dev = target
    g = _gen(8, fold)
    g1, g2, extra = torch.randn(300, generator=g), torch.randn(77, generator=g), torch.rand(9, generator=g)
    ss64 = float((g1.double() ** 2).sum() + (g2.double() ** 2).sum() + (extra.double().sum() if fold else 0.0))
    g1d, g2d, ed = g1.to(dev), g2.to(dev), extra.to(dev)
    ws = torch.zeros(lib.lv_sumsq_workspace_floats(), device=dev)
    for s1, s2, gd in GATE_ROWS_1_GOOD_3_BAD:
        st, guard, txn, acc, ptrs = _gate_inputs(dev, s1, s2, gd, 0)
        sumsq, coef, norm = (torch.tensor([SENT, SENT], device=dev) for _ in range(3))
        if fold:
            lib.lv_clip_norm2_fold_txn_f32(P(g1d), 300, P(g2d), 77, P(ws), P(ed), 9, 5.0, P(sumsq), P(coef), P(norm), *ptrs, _s(dev))
        else:
            lib.lv_clip_norm2_txn_f32(P(g1d), 300, P(g2d), 77, P(ws), 5.0, P(sumsq), P(coef), P(norm), *ptrs, _s(dev))
        assert _gate_check(s1, s2, gd, 0, st, guard, txn, acc) == ((s1, s2, gd) == (0, 0, 0.0))
        assert float(sumsq.cpu()[1]) == SENT and float(coef.cpu()[1]) == SENT and float(norm.cpu()[1]) == SENT
        ratio = max(abs(float(sumsq.cpu()[0]) - ss64) / (16 * EPS * ss64), abs(float(coef.cpu()[0]) - 5.0 / (math.sqrt(ss64) + 1e-6)) / (16 * EPS))
        _report(dev, "clip_norm2_fold_txn" if fold else "clip_norm2_txn", "gate row %s,%s,%s" % (s1, s2, gd), ratio)
        assert ratio <= 1.0, ratio


def test_txn_guard(target):
    lib, dev = target
    for s1 in (None, 0, 3):
        for s2 in (None, 0, -1):
            st = torch.tensor([s1 if s1 is not None else 99, s2 if s2 is not None else 99], dtype=torch.int32, device=dev)
            guard = torch.tensor([SENT, 0.5, SENT], device=dev)
            lib.lv_txn_guard_f32(P(st, 0) if s1 is not None else None, P(st, 1) if s2 is not None else None, P(guard, 1), _s(dev))
            want = 1.0 if (s1 == 3 or s2 == -1) else 0.0           # exactly 0.0 or 1.0, neighbours untouched
            assert _same_bits(guard, torch.tensor([SENT, want, SENT])), (s1, s2)


@pytest.mark.parametrize("n1,n2,n_extra,off", [(10, 10, 0, 0), (300, 300, 3, 3), (5, 1, 17, 1), (8193, 4099, 16389, 0),
                                               (1000, 77, 30001, 0), (1000, 77, 30001, 1)])
def test_clip_norm2_fold(target, n1, n2, n_extra, off):
    """sumsq = sum g1^2 + sum g2^2 + sum extra; the offset rows take the scalar paths (extra, and g2, off a 16-byte boundary);
    16389 and 30001 partials take a second trip of the four-deep unrolled loop with its clamped index live."""
    lib, dev = target
    g = _gen(9, n1, n2, n_extra, off)
    small = (n1, n2, n_extra) == (10, 10, 0)                          # this case stays below max_norm: coef exactly 1
    g1 = torch.randn(n1, generator=g) * (0.1 if small else 1.0)
    g2 = torch.randn(n2, generator=g) * (0.1 if small else 1.0)
    extra = torch.rand(max(n_extra, 1), generator=g) * 0.05
    extra[-1] = 40.0                                                   # the scalar tail carries weight
    max_norm = 5.0
    g1d = g1.to(dev)
    g2b = torch.cat([torch.full((off,), 1e18), g2, torch.full((1,), 1e18)]).to(dev)
    eb = torch.cat([torch.full((off,), 1e18), extra, torch.full((1,), 1e18)]).to(dev)
    ws = torch.zeros(lib.lv_sumsq_workspace_floats(), device=dev)
    txn = torch.zeros(5, device=dev)
    sumsq, coef, norm = (torch.tensor([SENT, SENT], device=dev) for _ in range(3))
    lib.lv_clip_norm2_fold_txn_f32(P(g1d), n1, P(g2b, off), n2, P(ws), P(eb, off) if n_extra else None, n_extra, max_norm, P(sumsq),
                                   P(coef), P(norm), None, None, None, P(txn), None, _s(dev))
    ss = float((g1.double() ** 2).sum() + (g2.double() ** 2).sum() + (extra.double().sum() if n_extra else 0.0))
    nr = math.sqrt(ss)
    cf = min(1.0, max_norm / (nr + 1e-6))
    got = [float(t.cpu()[0]) for t in (sumsq, norm, coef)]
    assert all(float(t.cpu()[1]) == SENT for t in (sumsq, norm, coef))
    ratios = [abs(got[0] - ss) / (16 * EPS * max(1.0, ss)), abs(got[1] - nr) / (16 * EPS * max(1.0, nr)), abs(got[2] - cf) / (16 * EPS)]
    _report(dev, "clip_norm2_fold", "%d,%d,%d,+%d" % (n1, n2, n_extra, off), max(ratios))
    assert max(ratios) <= 1.0, ratios
    if small:
        assert nr < max_norm and got[2] == 1.0
    else:
        assert nr > max_norm
    assert txn.cpu().tolist() == [0.0, 1.0, 0.0, 0.0, 0.0]


def test_clip_norm2_fold_all_zero(target):
    lib, dev = target
    z1, z2, ze = torch.zeros(300, device=dev), torch.zeros(300, device=dev), torch.zeros(3, device=dev)
    ws = torch.ones(lib.lv_sumsq_workspace_floats(), device=dev)
    txn = torch.zeros(5, device=dev)
    sumsq, coef, norm = (torch.tensor([SENT, SENT], device=dev) for _ in range(3))
    lib.lv_clip_norm2_fold_txn_f32(P(z1), 300, P(z2), 300, P(ws), P(ze), 3, 5.0, P(sumsq), P(coef), P(norm), None, None, None, P(txn), None,
                                   _s(dev))
    assert _same_bits(sumsq, torch.tensor([0.0, SENT])) and _same_bits(norm, torch.tensor([0.0, SENT]))
    assert _same_bits(coef, torch.tensor([1.0, SENT]))


UPDATE_CASES = [(5003, 1301, 0, 0, 0.37, 1), (5003, 1301, 1, 1, 0.37, 1), (7, 3, 0, 2, 1.0, 1), (4096, 4096, 0, 0, 0.5, 0), (1, 1, 3, 1, 0.25, 1)]
LEAD = 4                                        # floats in front of every window: keeps the base alignment, offsets add to it


def _window(vals, off, dev):
    """vals inside a buffer with LEAD + off sentinel floats in front and 5 behind; returns (device buffer, host copy, start)."""
    start = LEAD + off
    host = torch.cat([torch.full((start,), SENT), vals, torch.full((5,), SENT)])
    return host.clone().to(dev), host, start


@pytest.mark.parametrize("kernel,void", [("sgd_step_txn", False), ("sgd_step_txn", True), ("sgd_step_scale_txn", False),
                                         ("sgd_step_scale_txn", True), ("scale_txn", False), ("scale_txn", True), ("scale", False)])
@pytest.mark.parametrize("n,n2,off,off2,c,wb", UPDATE_CASES)
def test_update_kernels(target, n, n2, off, off2, c, wb, void, kernel):
    lib, dev = target
    g_ = _gen(10, n, n2, off, off2)
    p0, g0, x0 = torch.randn(n, generator=g_), torch.randn(n, generator=g_) * 3.0, torch.randn(n2, generator=g_)
    pd, ph, ps = _window(p0, off, dev)
    gd, gh, gs = _window(g0, off, dev)
    xd, xh, xs = _window(x0, off2, dev)
    sc = torch.tensor([0.7, c, 1.0 if void else 0.0, SENT], device=dev)          # lr, coef, void flag
    c32 = torch.tensor(c, dtype=torch.float32)
    lr64, c64 = float(torch.tensor(0.7, dtype=torch.float32)), float(c32)
    s = _s(dev)
    if kernel == "sgd_step_txn":
        lib.lv_sgd_step_txn_f32(P(pd, ps), P(gd, gs), n, P(sc, 0), P(sc, 1), wb, P(sc, 2), s)
    elif kernel == "sgd_step_scale_txn":
        lib.lv_sgd_step_scale_txn_f32(P(pd, ps), P(gd, gs), n, P(sc, 0), P(sc, 1), wb, P(xd, xs), n2, P(sc, 2), s)
    elif kernel == "scale_txn":
        lib.lv_scale_txn_f32(P(xd, xs), n2, P(sc, 1), P(sc, 2), s)
    else:
        lib.lv_scale_f32(P(xd, xs), n2, P(sc, 1), s)
    po, go, xo = pd.cpu(), gd.cpu(), xd.cpu()
    assert _same_bits(sc, torch.tensor([0.7, c, 1.0 if void else 0.0, SENT]))
    # elements on both sides of each window are untouched, whatever happened inside
    for o, h, st_, m in ((po, ph, ps, n), (go, gh, gs, n), (xo, xh, xs, n2)):
        assert _same_bits(o[:st_], h[:st_]) and _same_bits(o[st_ + m:], h[st_ + m:])
    steps = kernel.startswith("sgd") and not void
    scales_x2 = kernel != "sgd_step_txn" and not void
    # x2: a single f32 multiply (bit-unchanged when c == 1 or the call does not touch it)
    assert _same_bits(xo[xs:xs + n2], x0 * c32 if scales_x2 else x0)
    if c == 1.0:
        assert _same_bits(xo[xs:xs + n2], x0)
    if not steps:
        assert _same_bits(po[ps:ps + n], p0) and _same_bits(go[gs:gs + n], g0)
        return
    # g: written back as the single multiply g * c, bit-unchanged with write_back = 0 or c == 1
    assert _same_bits(go[gs:gs + n], g0 * c32 if wb else g0)
    if c == 1.0:
        assert _same_bits(go[gs:gs + n], g0)
    # p: within 2 eps32 (|p| + |lr c g|) of float64 (multiply, multiply, subtract: half an ulp each, fused or not)
    upd = lr64 * c64 * g0.double()
    bound = 2 * EPS * (p0.double().abs() + upd.abs())
    ratio = float(((po[ps:ps + n].double() - (p0.double() - upd)).abs() / bound).max())
    _report(dev, kernel, "%d,%d,+%d,+%d,c=%g,wb=%d" % (n, n2, off, off2, c, wb), ratio)
    assert ratio <= 1.0, ratio


SEQ_N, SEQ_N2 = 5003, 1301


def _seq_data():
    g = _gen(11)
    p0 = torch.randn(SEQ_N, generator=g)
    x20 = torch.randn(SEQ_N2, generator=g)
    scales = [1.0, 0.01, 2.5, 0.02, 0.5]               # steps 1 and 3 stay below max_norm once x2 has been clipped: coef exactly 1
    grads = [torch.randn(SEQ_N, generator=g) * sc for sc in scales]
    pend = [[1.5 + i, 0.25 * (i + 1), 3.0 - i] for i in range(5)]
    return p0, x20, grads, pend


def _seq_state(dev, p0, x20):
    return dict(p=p0.clone().to(dev), x2=x20.clone().to(dev), txn=torch.zeros(5, device=dev), acc=torch.tensor([10.0, 20.0, 30.0], device=dev),
                status=torch.zeros(1, dtype=torch.int32, device=dev), sc=torch.tensor([0.5, 0.0], device=dev),       # lr, coef
                ws=None, coefs=[])


def _seq_step(lib, dev, st, grad, pend):
    if st["ws"] is None:
        st["ws"] = torch.zeros(lib.lv_sumsq_workspace_floats(), device=dev)
    g = grad.clone().to(dev)
    st["txn"][2:5] = torch.tensor(pend)                 # the step's pending report sums
    s = _s(dev)
    lib.lv_clip_norm2_txn_f32(P(g), SEQ_N, P(st["x2"]), SEQ_N2, P(st["ws"]), 5.0, None, P(st["sc"], 1), None, P(st["status"]), None, None,
                              P(st["txn"]), P(st["acc"]), s)
    lib.lv_sgd_step_scale_txn_f32(P(st["p"]), P(g), SEQ_N, P(st["sc"], 0), P(st["sc"], 1), 1, P(st["x2"]), SEQ_N2, P(st["txn"], 0), s)
    st["coefs"].append(float(st["sc"][1].item()))


def test_sgd_txn_voided_then_replayed_equals_uninterrupted(target):
    lib, dev = target
    p0, x20, grads, pend = _seq_data()
    clean = _seq_state(dev, p0, x20)
    for i in range(5):
        _seq_step(lib, dev, clean, grads[i], pend[i])
    assert clean["txn"].cpu().tolist() == [0.0, 5.0, 0.0, 0.0, 0.0]
    assert 1.0 in clean["coefs"] and min(clean["coefs"]) < 1.0          # both sides of the clip are exercised
    assert not _same_bits(clean["p"], p0)
    acc = torch.tensor([10.0, 20.0, 30.0])
    acc2 = None
    for i in range(5):
        acc = acc + torch.tensor(pend[i])                               # f32, in step order, as the gate adds them
        if i == 1:
            acc2 = acc.clone()
    assert _same_bits(clean["acc"], acc)

    part = _seq_state(dev, p0, x20)
    for i in range(2):
        _seq_step(lib, dev, part, grads[i], pend[i])
    before = [part[k].clone() for k in ("p", "x2", "acc")]
    part["status"][0] = 7                                               # step 2: a persistent launch timed out
    _seq_step(lib, dev, part, grads[2], pend[2])
    part["status"][0] = 0                                               # steps 3, 4 queued with clean status: the flag is sticky
    for i in (3, 4):
        _seq_step(lib, dev, part, grads[i], pend[i])
    assert part["txn"].cpu().tolist() == [1.0, 2.0, 0.0, 0.0, 0.0]
    for k, b in zip(("p", "x2", "acc"), before):
        assert _same_bits(part[k], b), k
    assert _same_bits(part["acc"], acc2)
    part["txn"][0] = 0.0                                                # the host noticed: clears the flag, queues 2.. again
    for i in (2, 3, 4):
        _seq_step(lib, dev, part, grads[i], pend[i])
    assert part["txn"].cpu().tolist() == [0.0, 5.0, 0.0, 0.0, 0.0]
    for k in ("p", "x2", "acc"):
        assert _same_bits(part[k], clean[k]), k


# --------------------------------------------------------------------------------------------------------------------- helpers

@pytest.mark.parametrize("R,C", [(0, 5), (1, 1), (5, 300), (130, 257)])
def test_colsum(target, R, C):
    lib, dev = target
    x = torch.randn(max(R, 1), C, generator=_gen(12, R, C))
    xin = _padded(x, 3, float("nan")).to(dev)
    out = torch.full((C + 1,), SENT, device=dev)
    out2 = torch.full((C + 1,), SENT, device=dev)
    lib.lv_colsum_f32(P(xin), C + 3, R, C, P(out), P(out2), _s(dev))
    o = out.cpu()
    assert float(o[C]) == SENT and _same_bits(out2, out)
    if R == 0:
        assert _same_bits(o[:C], torch.zeros(C))
        return
    x64 = x[:R].double()
    _check(dev, "colsum", "%dx%d" % (R, C), o[:C], x64.sum(0), R, x64.abs().sum(0).clamp(min=1.0))
    only = torch.full((C + 1,), SENT, device=dev)
    lib.lv_colsum_f32(P(xin), C + 3, R, C, P(only), None, _s(dev))
    assert _same_bits(only, out)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000])
def test_sum_accum(target, n):
    """out[0] += sum(x): 256 threads stride the input (a serial chain of ceil(n / 256)), a six-level wave butterfly, two levels
    across the four waves, one add onto the accumulator: L = ceil(n / 256) + 9."""
    lib, dev = target
    x = torch.randn(max(n, 1), generator=_gen(13, n)) * 2.0
    xin = torch.cat([x[:n], torch.full((3,), float("nan"))]).to(dev)
    out = torch.tensor([-3.25, SENT], device=dev)
    lib.lv_sum_accum_f32(P(xin), n, P(out), _s(dev))
    o = out.cpu()
    assert float(o[1]) == SENT
    x64 = x[:n].double()
    if n == 0:
        assert float(o[0]) == -3.25
        return
    _check(dev, "sum_accum", str(n), o[:1], (x64.sum() - 3.25).reshape(1), (n + 255) // 256 + 9, max(1.0, 3.25 + float(x64.abs().sum())))


@pytest.mark.parametrize("n", [1, 257])
def test_tanh(target, n):
    lib, dev = target
    x = torch.linspace(-20.0, 20.0, n) if n > 1 else torch.tensor([0.7])
    if n > 1:
        x[3], x[4], x[n // 2] = 0.0, -0.0, 1e-5
    xin = torch.cat([x, torch.tensor([float("nan")])]).to(dev)
    out = torch.full((n + 1,), SENT, device=dev)
    lib.lv_tanh_f32(P(xin), P(out), n, _s(dev))
    o = out.cpu()
    assert float(o[n]) == SENT
    err = float((o[:n].double() - x.double().tanh()).abs().max())
    _report(dev, "tanh", str(n), err / (4 * EPS))
    assert err <= 4 * EPS
    if n > 1:
        assert _same_bits(o[3:5], torch.tensor([0.0, -0.0]))          # tanh(+-0) = +-0


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1, 7, 4096])
def test_add_and_mul_inplace(target, n, off):
    lib, dev = target
    g = _gen(14, n, off)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ad, _, s0 = _window(a, off, dev)
    bd, _, _ = _window(b, off, dev)
    od, oh, _ = _window(torch.full((n,), SENT), off, dev)
    lib.lv_add_f32(P(ad, s0), P(bd, s0), P(od, s0), n, _s(dev))
    want = oh.clone()
    want[s0:s0 + n] = a + b
    assert _same_bits(od, want)
    lib.lv_add_f32(P(od, s0), P(bd, s0), P(od, s0), n, _s(dev))         # `a` and `out` may alias
    want[s0:s0 + n] = (a + b) + b
    assert _same_bits(od, want)
    wd, wh, _ = _window(a, off, dev)
    lib.lv_mul_inplace_f32(P(wd, s0), P(bd, s0), n, _s(dev))
    wh[s0:s0 + n] = a * b
    assert _same_bits(wd, wh)


@pytest.mark.parametrize("rows,cols,in_ld,out_ld", [(1, 1, 1, 1), (33, 70, 75, 40), (64, 32, 32, 64), (5, 130, 131, 9)])
def test_transpose_ld(target, rows, cols, in_ld, out_ld):
    lib, dev = target
    x = torch.randn(rows, in_ld, generator=_gen(15, rows, cols))
    x[:, cols:] = float("nan")
    out = torch.full((cols * out_ld + 1,), SENT, device=dev)
    xd = x.to(dev)
    lib.lv_transpose_ld_f32(P(xd), in_ld, P(out), out_ld, rows, cols, _s(dev))
    want = torch.full((cols, out_ld), SENT)
    want[:, :rows] = x[:, :cols].t()
    assert _same_bits(out, torch.cat([want.reshape(-1), torch.tensor([SENT])]))


@pytest.mark.parametrize("absent", ["g_loss", "g_rec", "g_kl"])
@pytest.mark.parametrize("B", [1, 257])
def test_loss_bwd_scales(target, B, absent):
    """rowscale = g_loss + g_rec (one add: exact), dkl = klw * g_loss + g_kl (a multiply and an add: 2 eps32 of the terms)."""
    lib, dev = target
    g = _gen(16, B)
    t = {k: torch.randn(B, generator=g) for k in ("g_loss", "g_rec", "g_kl")}
    d = {k: (None if k == absent else v.to(dev)) for k, v in t.items()}
    z = {k: (torch.zeros(B) if k == absent else v) for k, v in t.items()}
    klw = torch.tensor([0.3], device=dev)
    rs = torch.full((B + 1,), SENT, device=dev)
    dkl = torch.full((B + 1,), SENT, device=dev)
    lib.lv_loss_bwd_scales_f32(P(d["g_loss"]), P(d["g_rec"]), P(d["g_kl"]), P(klw), P(rs), P(dkl), B, _s(dev))
    assert _same_bits(rs, torch.cat([z["g_loss"] + z["g_rec"], torch.tensor([SENT])]))
    o = dkl.cpu()
    assert float(o[B]) == SENT
    k64 = float(klw.cpu()[0])
    ref = k64 * z["g_loss"].double() + z["g_kl"].double()
    bound = 2 * EPS * ((k64 * z["g_loss"].double()).abs() + z["g_kl"].double().abs()) + 1e-300
    ratio = float(((o[:B].double() - ref).abs() / bound).max())
    _report(dev, "loss_bwd_scales.dkl", "%d/no_%s" % (B, absent), ratio)
    assert ratio <= 1.0


@pytest.mark.parametrize("T,B", [(7, 5), (70, 33)])
def test_loss_assemble_rng_equals_loss_assemble(target, T, B):
    lib, dev = target
    g = _gen(17, T, B)
    nll, kl, gl = torch.rand(T, B, generator=g).to(dev), torch.rand(B, generator=g).to(dev), torch.randn(B, generator=g).to(dev)
    klw = torch.tensor([0.45], device=dev)
    outs = []
    state = torch.tensor([1234567, (1 << 40) + 5, -77], dtype=torch.int64, device=dev)      # {seed, offset}, sentinel
    inc = (1 << 33) + 12
    for rng in (False, True):
        o = [torch.full((B + 1,), SENT, device=dev) for _ in range(4)] + [torch.tensor([1.0, 2.0, 3.0, SENT], device=dev)]
        args = [P(nll), P(kl), P(klw), P(gl)] + [P(t) for t in o] + [T, B]
        if rng:
            lib.lv_loss_assemble_rng_f32(*args, P(state), inc, _s(dev))
        else:
            lib.lv_loss_assemble_f32(*args, _s(dev))
        outs.append(o)
    for a, b in zip(*outs):
        assert _same_bits(a, b)
        assert float(a.cpu()[-1]) == SENT
    rec64 = nll.cpu().double().sum(0)
    assert float((outs[0][1].cpu()[:B].double() - rec64).abs().max()) <= (8 + (T + 63) // 64 + 6) * EPS * float(rec64.abs().max().clamp(min=1.0))
    assert state.cpu().tolist() == [1234567, (1 << 40) + 5 + inc, -77]                    # advanced by exactly rng_inc


def test_persist16_xch_clear(target):
    """lv_lstm_persist16_xch_clear zeroes the exchange area of the persistent recurrence and nothing behind it: the buffer is
    lv_lstm_persist16_xch_floats() floats, whose last 64 are slack the clear does not own."""
    lib, dev = target
    n = int(lib.lv_lstm_persist16_xch_floats())
    buf = torch.full((n + 1,), SENT, device=dev)
    lib.lv_lstm_persist16_xch_clear(P(buf), _s(dev))
    o = buf.cpu()
    assert _same_bits(o[:n - 64], torch.zeros(n - 64)) and _same_bits(o[n - 64:], torch.full((65,), SENT))

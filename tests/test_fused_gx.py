"""The persistent forward that computes its own input projection (lv_lstm_fwd_bf16_persist16_x, the XIN form of
lstm_fwd_persist_k16_kernel): kernel level against a float64 recurrence and against the existing path (input-projection GEMM
into Gx + lv_lstm_fwd_bf16_persist16), and engine level through one AggressiveTextTrainer.step with LVAE_FUSED_GX on and off.
The kernel-level functions take (lib, device, ...) and also run on the CPU emulator (tests/test_fused_gx_emu.py)."""
import pytest
import torch

from vae_lagging_encoder_amd import _lib
from vae_lagging_encoder_amd import engine as E
from vae_lagging_encoder_amd.engine import P, stream_ptr

H, NI = 1024, 512
SHAPES = [(1, 5, 1), (3, 13, 2), (5, 30, 4), (9, 32, 4), (40, 32, 4)]


@pytest.fixture(scope="module")
def lib(hip_device):
    return _lib.load()


def _rnd(x, f16):
    return x.to(torch.float16 if f16 else torch.bfloat16)


def _saved_unpack(saved, T, B, R):
    """saved[group][member][t]{ gates [R][32][4], c [R][32] } -> (gates [T][B][H][4], c_t [T][B][H])"""
    sv = saved.view(8, 32, T, R * 160)
    g = sv[..., :R * 128].reshape(8, 32, T, R, 32 * 4).permute(2, 0, 3, 1, 4).reshape(T, 8 * R, H, 4)
    c = sv[..., R * 128:].reshape(8, 32, T, R, 32).permute(2, 0, 3, 1, 4).reshape(T, 8 * R, H)
    return g[:, :B].contiguous(), c[:, :B].contiguous()


_INPUTS = {}


def _inputs(T, B, f16, per_row, zero_state=False):
    """Operands (X and W_ih already rounded to the 16-bit format) and the float64 recurrence that sees the same rounded operands:
    computed once per case on the CPU, shared by the flags variants and by both paths, never modified."""
    key = (T, B, f16, per_row, zero_state)
    if key in _INPUTS:
        return _INPUTS[key]
    g = torch.Generator().manual_seed(T * 1000 + B * 10 + 2 * int(f16) + int(per_row))
    X = _rnd(torch.randn(T * B, NI, generator=g), f16)
    wih = _rnd(torch.randn(4 * H, NI, generator=g) / NI ** 0.5, f16)            # gate-major rows g * H + u
    whh = torch.randn(4 * H, H, generator=g) / H ** 0.5
    add = torch.randn(B if per_row else 1, 4 * H, generator=g) * 0.3            # gate-major
    c0 = torch.zeros(B, H) if zero_state else torch.randn(B, H, generator=g) * 0.5
    h0 = torch.tanh(c0)
    perm = torch.arange(4 * H).view(4, H).t().reshape(-1)                       # unit-major row 4u + g <- gate-major g * H + u
    w64 = _rnd(whh, f16).double()
    gx = (X.double() @ wih.double().t()).view(T, B, 4 * H) + add.double()
    h, c = h0.double(), c0.double()
    hs, cs, gates = [h], [c], []
    for t in range(T):
        a = gx[t] + _rnd(h.float(), f16).double() @ w64.t()
        i, f, gg, o = a.chunk(4, -1)
        i, f, o, gg = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(gg)
        c = f * c + i * gg
        h = o * torch.tanh(c)
        hs.append(h), cs.append(c), gates.append(torch.stack([i, f, gg, o], -1))
    d = dict(X=X, wih_um=wih[perm].contiguous(), whh=whh, add_um=add[:, perm].contiguous(), c0=c0, h0=h0,
             hs=torch.stack(hs), cs=torch.stack(cs), gates=torch.stack(gates))
    _INPUTS[key] = d
    return d


def _run(lib, dev, d, T, B, R, f16, flags, fused):
    """One forward on `dev`: the fused entry, or the existing path on the same images (lv_gemm_b16 / lv_gemm_h16 into Gx, then
    lv_lstm_fwd_bf16_persist16).  Returns (hs [T+1][B][H], final cs [B][H], gates [T][B][H][4], c_t [T][B][H]) on the CPU."""
    s = stream_ptr(dev)
    X16 = d["X"].view(torch.int16).to(dev)
    W16 = d["wih_um"].view(torch.int16).to(dev)
    add = d["add_um"].to(dev)
    per_row = add.shape[0] > 1
    whh = d["whh"].to(dev)
    hs = torch.full((T + 1, B, H), float("nan"), device=dev)
    cs = torch.zeros(T + 1, B, H, device=dev)
    hs[0], cs[0] = d["h0"].to(dev), d["c0"].to(dev)
    wpk = torch.full((lib.lv_lstm_persist16_wpk_floats(),), float("nan"), device=dev)
    xch = torch.zeros(lib.lv_lstm_persist16_xch_floats(), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    saved = torch.full((lib.lv_lstm_persist16_saved_floats(T, R),), float("nan"), device=dev)
    lib.lv_lstm_persist16_pack(P(whh), P(wpk), 2 if f16 else 0, H, s)
    fl = flags | (32 if f16 else 0)
    if fused:
        lib.lv_lstm_fwd_bf16_persist16_x(P(X16), NI, P(W16), NI, P(add), 4 * H if per_row else 0, P(wpk), P(hs), P(cs), P(saved),
                                         P(xch), P(status), T, B, R, fl, H, s)
    else:
        Gx = torch.empty(T * B, 4 * H, device=dev)
        ws = E._gemm_ws(lib, s)
        ld1, mod1 = (4 * H, B) if per_row else (0, 1)
        if f16:
            lib.lv_gemm_h16(T * B, 4 * H, NI, 1.0, P(X16), NI, P(W16), NI, P(Gx), 4 * H, 0, P(add), ld1, mod1, None, 0, 1,
                            P(ws), ws.numel(), s)
        else:
            lib.lv_gemm_b16(0, T * B, 4 * H, NI, 1.0, P(X16), NI, P(W16), NI, P(Gx), 4 * H, 0, P(add), ld1, mod1, None, 0, 1,
                            P(ws), ws.numel(), s)
        lib.lv_lstm_fwd_bf16_persist16(P(Gx), P(wpk), P(hs), P(cs), P(saved), P(xch), P(status), T, B, R, fl, H, s)
    assert int(status.item()) == 0                                               # (c)
    gates, c_t = _saved_unpack(saved.cpu(), T, B, R)
    return hs.cpu(), cs[T].cpu(), gates, c_t


def check_fused_forward(lib, dev, T, B, R, f16, flags, per_row):
    """(a) hs, the final cs and the unpacked gates / cell states against the float64 recurrence on the same rounded operands at
    1e-3 (the bound test_lstm_fwd_persistent16 holds its two paths to: f32 summation order, ~1e-6 of hardware exp, and what an h
    element that rounds the other way moves downstream); (b) the same outputs against the existing path on the same images, which
    differs from the fused one only by the f32 summation order of the K = 512 chain -- the same bound by the same reasoning;
    (c) status word 0 (asserted in _run)."""
    d = _inputs(T, B, f16, per_row)
    hs, cT, gates, c_t = _run(lib, dev, d, T, B, R, f16, flags, True)
    cmax = max(1.0, float(d["cs"].abs().max()))
    assert float((hs.double() - d["hs"]).abs().max()) < 1e-3
    assert float((cT.double() - d["cs"][T]).abs().max()) < 1e-3 * cmax
    assert float((gates.double() - d["gates"]).abs().max()) < 1e-3
    assert float((c_t.double() - d["cs"][1:]).abs().max()) < 1e-3 * cmax
    hs2, cT2, gates2, c_t2 = _run(lib, dev, d, T, B, R, f16, flags, False)
    for a, b, what in ((hs, hs2, "h"), (cT, cT2, "cT"), (gates, gates2, "gates"), (c_t, c_t2, "c")):
        assert float((a - b).abs().max()) < 1e-3, what


def check_projection_error(lib, dev, B, R, f16, per_row):
    """T = 1 with h0 = c0 = 0: the saved gates are a pure function of the input projection.  Both paths' errors against float64;
    the fused one must not exceed twice the existing path's + 1e-6 (factor 2: the other chain order; 1e-6: the activations'
    hardware exp noise).  A wrong row, step or slot fails this by orders of magnitude.  Returns (fused, existing)."""
    d = _inputs(1, B, f16, per_row, zero_state=True)
    e = []
    for fused in (True, False):
        _, _, gates, _ = _run(lib, dev, d, 1, B, R, f16, 1, fused)
        e.append(float((gates.double() - d["gates"]).abs().max()))
    print("projection error vs float64: fused %.3e existing %.3e" % (e[0], e[1]))
    assert e[0] <= 2 * e[1] + 1e-6, e
    return e


def check_refusals(lib, dev):
    """(d) shapes the entry does not take return a negative status and launch nothing (hs stays as it was)."""
    s = stream_ptr(dev)
    z = torch.zeros(1 << 16, device=dev)
    hs = torch.full((2 * 40 * H,), float("nan"), device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    raw = lib._raw_lv_lstm_fwd_bf16_persist16_x
    def call(ni, R, B, Hh):
        return raw(P(z), ni, P(z), ni, P(z), 0, P(z), P(hs), P(z), P(z), P(z), P(st), 1, B, R, 0, Hh, s)
    assert call(256, 4, 32, 1024) < 0          # ni != 512
    assert call(512, 4, 32, 512) < 0           # H != 1024
    assert call(512, 5, 40, 1024) < 0          # more than 4 rows per group: instantiation not built
    assert call(512, 2, 32, 1024) < 0          # 8 R < B
    with pytest.raises(_lib.LvaeError):
        lib.lv_lstm_fwd_bf16_persist16_x(P(z), 256, P(z), 256, P(z), 0, P(z), P(hs), P(z), P(z), P(z), P(st), 1, 32, 4, 0, 1024, s)
    assert bool(torch.isnan(hs).all()) and int(st.item()) == 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("per_row", [True, False])
@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("T,B,R", SHAPES)
def test_fused_gx_forward(lib, hip_device, T, B, R, f16, flags, per_row):
    check_fused_forward(lib, hip_device, T, B, R, f16, flags, per_row)


@pytest.mark.gpu
@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("B,R", [(5, 1), (32, 4)])
def test_fused_gx_projection_error(lib, hip_device, B, R, f16):
    """Measured on MI355X, max abs error of the saved gates against float64, fused / existing: bf16 (5, 1) 4.46e-7 / 3.90e-7,
    (32, 4) 5.93e-7 / 3.88e-7; binary16 (5, 1) 5.89e-7 / 6.15e-7, (32, 4) 6.15e-7 / 6.27e-7."""
    check_projection_error(lib, hip_device, B, R, f16, True)


@pytest.mark.gpu
def test_fused_gx_refusals(lib, hip_device):
    check_refusals(lib, hip_device)


# ---- engine level -----------------------------------------------------------------------------------------------------------------
def _engine_step(dev, fused_gx, monkeypatch, second_without_persistent=False):
    """One AggressiveTextTrainer.step of a small text VAE at the kernel's shape class (H = 1024, ni = 512; bf16) with the fused
    forward on or off, on fixed parameters, batch and noise.  lr = 0: the weights stay put, a second step sees the same model."""
    from helpers import build_vae
    from oracle import text_vae_oracle as O
    from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer
    V, ni, Hh, nz, B, T, klw = 300, NI, H, 32, 8, 7, 0.5
    monkeypatch.setattr(E, "FUSED_GX", fused_gx)
    prm = O.random_params(V, ni, Hh, nz, seed=21, scale=0.03, head_scale=0.2)
    x = O.synthetic_batch(B, T, V, seed=22)
    eps, m_in, m_out = O.draw_noise(B, T, ni, Hh, nz, seed=23)
    noise = (eps.to(dev), m_in.to(torch.uint8).to(dev), m_out.to(torch.uint8).to(dev))
    vae = build_vae(V, ni, Hh, nz, dev, params=prm)
    tr = AggressiveTextTrainer(vae, lr=0.0, clip=5.0, precision="bf16")

    def one():
        tr.step(x.to(dev), klw, noise=noise)
        tr.read_stats()
        assert tr.recoveries == 0
        st = next(reversed(tr.static.values()))
        out = {k: getattr(st, k).detach().float().cpu().clone() for k in ("loss", "rec", "kl")}
        out.update({"grad." + n: p.grad.detach().float().cpu().clone() for n, p in vae.named_parameters() if p.grad is not None})
        return out
    res = [one()]
    gx = [tr.enc._ws(B, T).Gx, tr.dec._ws(B, T - 1).Gx]
    persistent_here = E._persistent_ok(tr.enc, object(), B, Hh, dev, 128)
    assert all((g is None) == (fused_gx and persistent_here) for g in gx), "which path ran: %r" % ([g is None for g in gx],)
    if second_without_persistent:
        tr.enc.persistent = tr.dec.persistent = False        # by hand: what a demotion to the launch-per-timestep rung does
        res.append(one())
        assert tr.enc._ws(B, T).Gx is not None and tr.dec._ws(B, T - 1).Gx is not None      # the GEMM path computed Gx
    return res


def _compare_steps(a, b, what):
    worst = {"seq": 0.0, "grad": 0.0}
    for k in a:
        if k.startswith("grad."):
            e = float((a[k] - b[k]).abs().max()) / max(float(b[k].abs().max()), 1e-30)
            worst["grad"] = max(worst["grad"], e)
        else:
            e = float(((a[k] - b[k]).abs() / b[k].abs().clamp_min(1e-30)).max())
            worst["seq"] = max(worst["seq"], e)
    print("%s: per-sequence loss / rec / kl worst relative %.3e, gradients worst %.3e of their max-abs" % (what, worst["seq"], worst["grad"]))
    for k in a:
        if k.startswith("grad."):
            assert float((a[k] - b[k]).abs().max()) <= 1e-3 * float(b[k].abs().max()), (what, k)
        else:
            assert bool(((a[k] - b[k]).abs() <= 1e-5 * b[k].abs()).all()), (what, k)
    return worst


@pytest.mark.gpu
def test_fused_gx_engine_step_matches_gemm_path(hip_device, monkeypatch):
    """LVAE_FUSED_GX = 1 against = 0 (engine.FUSED_GX) on identical parameters, batch and noise: per-sequence loss / rec / kl to
    1e-5 relative, every gradient tensor to 1e-3 of its own max-abs; then each trainer with eng.persistent switched off by hand
    steps again -- the GEMM path computes Gx, the launch-per-timestep kernels read it -- and the two agree inside the same bounds.
    (The second steps are compared with each other, not with the first ones: the launch-per-timestep rung runs the encoder's
    recurrence on bf16 operands where the persistent launch uses binary16, 3.0e-4 on the KL per sequence with or without this
    change.)  Measured on MI355X: first steps 6.0e-6 per sequence, 6.7e-4 of max-abs on the gradients."""
    off, off_demoted = _engine_step(hip_device, False, monkeypatch, second_without_persistent=True)
    on, demoted = _engine_step(hip_device, True, monkeypatch, second_without_persistent=True)
    _compare_steps(on, off, "fused vs GEMM path")
    _compare_steps(demoted, off_demoted, "launch-per-timestep rung, engine with the fused forward vs without")

"""The decoder's three hidden-state images from one pass over hs (lv_cvt_bf16_hs3_f32, lv_gemm_b16.hip) against the two conversions
it replaces -- lv_cvt_bf16_keep_f32 on rows [Bd, (Td + 1) Bd) for O / O^T and lv_cvt_bf16_f32 on rows [0, Td Bd) for h_prev^T --
bit for bit, and a trainer step with the one-pass route on and off.  Emulator (`not gpu`) and MI355X (`gpu`).

Shapes: rows and columns that are no multiple of the 64-tile, a row shift Bd below and at a tile edge, Bd % 4 != 0 (2-byte
stores of the shifted transposed image) and Bd % 4 == 0 (8-byte stores)."""
import pytest
import torch

from helpers import build_vae
from oracle import text_vae_oracle as O
from vae_lagging_encoder_amd import engine as _eng
from vae_lagging_encoder_amd.engine import P

SENT = 0x7B7B                      # destination fill: what the launches do not write must stay


@pytest.fixture(params=["emu", pytest.param("gpu", marks=pytest.mark.gpu)])
def target(request):
    if request.param == "emu":
        request.getfixturevalue("emu_backend")
        dev = torch.device("cpu")
    else:
        dev = request.getfixturevalue("hip_device")
    return _eng.backend_for(dev), dev


def _images(dev, Td, Bd, H):
    ldr = (Td * Bd + 7) // 8 * 8
    mk = lambda r, c: torch.full((r, c), SENT, dtype=torch.int16, device=dev)
    return mk(Td * Bd + 1, H), mk(H + 1, ldr), mk(H + 1, ldr), ldr          # O, OT, hT (+ one guard row each)


@pytest.mark.parametrize("scale", [2.0, 1.0 / 0.7, None])
@pytest.mark.parametrize("Td,Bd,H", [(1, 1, 8), (3, 5, 72), (2, 64, 64), (5, 7, 136), (3, 68, 72)])
def test_three_images_equal_the_two_conversions(target, Td, Bd, H, scale):
    lib, dev = target
    s = _eng.stream_ptr(dev)
    gen = torch.Generator().manual_seed(1000 * Td + 10 * Bd + H)
    hs = torch.randn((Td + 1) * Bd, H, generator=gen)
    hs[0, 0] = -0.25                                                     # a dropped negative element is -0 in the image
    keep = None
    if scale is not None:
        keep = (torch.rand(Bd, Td, H, generator=gen) < 0.7).to(torch.uint8)
        keep[0, 0, 0] = 0
        keep = keep.to(dev)
    hs = hs.to(dev)
    O1, OT1, hT1, ldr = _images(dev, Td, Bd, H)
    O2, OT2, hT2, _ = _images(dev, Td, Bd, H)
    kscale = scale if scale is not None else 1.0
    lib.lv_cvt_bf16_hs3_f32(P(hs), H, Td, Bd, H, P(keep), kscale, P(O1), H, P(OT1), ldr, P(hT1), ldr, s)
    if keep is not None:
        lib.lv_cvt_bf16_keep_f32(P(hs, Bd * H), H, Td, Bd, H, P(keep), kscale, P(O2), H, P(OT2), ldr, s)
    else:
        lib.lv_cvt_bf16_f32(P(hs, Bd * H), H, Td * Bd, H, P(O2), H, P(OT2), ldr, s)
    lib.lv_cvt_bf16_f32(P(hs), H, Td * Bd, H, None, 0, P(hT2), ldr, s)
    for name, a, b in (("O", O1, O2), ("OT", OT1, OT2), ("hT", hT1, hT2)):
        assert torch.equal(a.cpu(), b.cpu()), name
        assert bool((a.cpu()[-1] == SENT).all()), (name, "guard row")
    assert bool((O1.cpu()[:-1] != SENT).all()) and bool((hT1.cpu()[:H, :Td * Bd] != SENT).all())      # (no bf16 of a randn is 0x7B7B)
    if keep is not None and Td * Bd > 1:
        assert not torch.equal(OT1.cpu()[:H, :Td * Bd], hT1.cpu()[:H, :Td * Bd])                         # two different images


def test_three_images_entry_checks_its_arguments(target):
    lib, dev = target
    s = _eng.stream_ptr(dev)
    Td, Bd, H = 3, 5, 72
    hs = torch.zeros((Td + 1) * Bd, H, device=dev)
    O_, OT, hT, ldr = _images(dev, Td, Bd, H)
    good = [P(hs), H, Td, Bd, H, None, 1.0, P(O_), H, P(OT), ldr, P(hT), ldr, s]
    for i, bad in ((0, None), (7, None), (9, None), (11, None), (3, 0), (1, H - 4), (10, Td * Bd - 1), (12, Td * Bd - 1)):
        a = list(good)
        a[i] = bad
        with pytest.raises(_eng._lib.LvaeError):
            lib.lv_cvt_bf16_hs3_f32(*a)
    assert bool((O_.cpu() == SENT).all())


def test_three_images_unaligned_operands_take_the_two_conversions(target):
    """A source off the 16-byte grid cannot take the 16-byte loads: the entry runs the two separate conversions, same images."""
    lib, dev = target
    s = _eng.stream_ptr(dev)
    Td, Bd, H = 3, 5, 72
    gen = torch.Generator().manual_seed(5)
    base = torch.randn((Td + 1) * Bd * H + 1, generator=gen).to(dev)
    keep = (torch.rand(Bd, Td, H, generator=gen) < 0.7).to(torch.uint8).to(dev)
    O1, OT1, hT1, ldr = _images(dev, Td, Bd, H)
    O2, OT2, hT2, _ = _images(dev, Td, Bd, H)
    lib.lv_cvt_bf16_hs3_f32(P(base, 1), H, Td, Bd, H, P(keep), 2.0, P(O1), H, P(OT1), ldr, P(hT1), ldr, s)
    lib.lv_cvt_bf16_keep_f32(P(base, 1 + Bd * H), H, Td, Bd, H, P(keep), 2.0, P(O2), H, P(OT2), ldr, s)
    lib.lv_cvt_bf16_f32(P(base, 1), H, Td * Bd, H, None, 0, P(hT2), ldr, s)
    for a, b in ((O1, O2), (OT1, OT2), (hT1, hT2)):
        assert torch.equal(a.cpu(), b.cpu())


# ---- the trainer: one step sequence with the one-pass route on and off -----------------------------------------------------------
def _trainer_run(dev, monkeypatch, on, H, B, T, precision, ns=1):
    from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer
    V, NI, NZ = 61, 8, 4
    monkeypatch.setattr(_eng, "HS3_CVT", on)
    vae = build_vae(V, NI, H, NZ, dev, params=O.random_params(V, NI, H, NZ, seed=4, scale=0.3 if H < 256 else 0.02, emb_scale=0.5, head_scale=0.5))
    tr = AggressiveTextTrainer(vae, clip=5.0, lr=1.0, precision=precision, nsamples=ns)
    lib = tr.lib
    calls = []
    raw = lib.lv_cvt_bf16_hs3_f32
    monkeypatch.setattr(lib, "lv_cvt_bf16_hs3_f32", lambda *a: (calls.append(1), raw(*a))[1], raising=False)
    xs = [O.synthetic_batch(B, T, V, seed=30 + i).to(dev) for i in range(2)]
    for i, up in enumerate(["encoder", "both", "encoder"]):
        tr.step(xs[i % 2], 0.7, noise=_noise(dev, i, B, T, NI, H, NZ, ns), update=up)
    tr.commit()
    out = {"param." + k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}
    out.update({"grad." + k: p.grad.detach().cpu().clone() for k, p in vae.named_parameters()})
    return out, len(calls)


def _noise(dev, i, B, T, NI, H, NZ, ns):
    eps, mi, mo = O.draw_noise(B, T, NI, H, NZ, ns=ns, seed=50 + i)
    return eps.to(dev), mi.to(torch.uint8).to(dev), mo.to(torch.uint8).to(dev)


def _equal_runs(a, b):
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_trainer_step_h64_route_on_and_off(target, monkeypatch, precision):
    """H = 64: the decoder runs the launch-per-timestep recurrence (dropout inside it), where the one-pass conversion does not
    apply -- the switch must change nothing."""
    _, dev = target
    a, _ = _trainer_run(dev, monkeypatch, True, 64, 5, 7, precision)
    b, nb = _trainer_run(dev, monkeypatch, False, 64, 5, 7, precision)
    assert nb == 0
    _equal_runs(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [1, 2])
def test_trainer_step_h1024_route_on_and_off(hip_device, monkeypatch, ns):
    """H = 1024, bf16: the persistent recurrences, where the decoder's forward does take the one-pass conversion (one call per
    step) and its backward skips the h_prev image: gradients and weights equal the two-conversion route bit for bit."""
    dev = hip_device
    a, na = _trainer_run(dev, monkeypatch, True, 1024, 5, 4, "bf16", ns)
    b, nb = _trainer_run(dev, monkeypatch, False, 1024, 5, 4, "bf16", ns)
    assert nb == 0
    if torch.cuda.get_device_properties(dev).multi_processor_count >= 256:
        assert na == 3, na
    _equal_runs(a, b)

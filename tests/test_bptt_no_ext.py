"""The persistent BPTT (lv_lstm_bwd_bf16_persist16, lv_lstm_persist16.hip) without an external gradient of every h_t -- the
encoder's call: dh_ext = NULL, only h_T has a gradient -- against the same launch with dh_ext = zeros: dG16, dGsum, dh0 and dc0
bit for bit.  The NULL form is an instantiation of its own (HAS_EXT = false: no dh block, no load of it); zeros go through the
decoder's instantiation, so the comparison crosses the two.

B in {3, 32, 40, 128} at R = 1, 4, 6, 16 rows per group: the 4-, 8- and 16-row instantiations, groups left empty (B = 3) and a
ragged one (B = 40: six full groups, one of four rows, one empty); T in {2, 9, 200} -- 200 is the one length at which a missing
MFMA drain has shown up.  The saved activations are drawn, not computed: the BPTT is a function of the
record buffer whatever wrote it.  Emulator (`not gpu`, short shapes) and MI355X (`gpu`)."""
import pytest
import torch

from vae_lagging_encoder_amd import engine as _eng
from vae_lagging_encoder_amd.engine import P

H = 1024


def _run_pair(lib, dev, T, B, R, flags):
    s = _eng.stream_ptr(dev)
    g = torch.Generator().manual_seed(1000 * T + B)
    whh = (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(dev)
    wpk = torch.empty(lib.lv_lstm_persist16_wpk_floats(), device=dev)
    lib.lv_lstm_persist16_pack(P(whh), P(wpk), 1, H, s)
    gates = torch.rand(T, B, H, 4, generator=g) * 0.9 + 0.05                 # (i, f, g, o) per unit, all inside (0, 1)
    cs = torch.randn(T + 1, B, H, generator=g) * 0.5
    dh_last = torch.randn(B, H, generator=g).to(dev)
    gates, cs = gates.to(dev), cs.to(dev)
    saved = torch.zeros(lib.lv_lstm_persist16_saved_floats(T, R), device=dev)
    lib.lv_lstm_persist16_import_saved(P(gates), P(cs), P(saved), T, B, R, H, s)
    hs = torch.zeros(T + 1, B, H, device=dev)
    zeros = torch.zeros(T, B, H, device=dev)
    outs = []
    for ext in (None, zeros):
        dG16 = torch.full((T, B, 4 * H), 0x7FC0, dtype=torch.int16, device=dev)
        dGsum = torch.full((B, 4 * H), 7.0, device=dev)
        dh0, dc0 = torch.full((B, H), 7.0, device=dev), torch.full((B, H), 7.0, device=dev)
        xch = torch.zeros(lib.lv_lstm_persist16_xch_floats(), device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        lib.lv_lstm_bwd_bf16_persist16(P(ext), P(dh_last), P(wpk), P(saved), P(hs), P(cs), P(dG16), P(dGsum), P(xch), P(status), P(dh0),
                                       P(dc0), 0, T, B, R, flags, H, s)
        assert int(status.item()) == 0, "hand-off timeout, status %d" % int(status.item())
        outs.append((dG16.cpu(), dGsum.cpu().view(torch.int32), dh0.cpu().view(torch.int32), dc0.cpu().view(torch.int32)))
    for name, a, b in zip(("dG16", "dGsum", "dh0", "dc0"), *outs):
        assert torch.equal(a, b), name
    dG = outs[0][0].view(torch.bfloat16).float()
    assert bool(torch.isfinite(dG).all()) and float(dG[T - 1].abs().max()) > 0.0 and float(dG[max(T - 3, 0)].abs().max()) > 0.0
    assert not bool((outs[0][1] == torch.tensor(7.0).view(torch.int32)).all())


@pytest.mark.parametrize("T,B,R", [(2, 3, 1), (2, 18, 6), (2, 27, 14)])
def test_bptt_without_dh_ext_equals_zero_dh_ext_emulated(emu_backend, T, B, R):
    _run_pair(emu_backend, torch.device("cpu"), T, B, R, 0)


ROWS = [(3, 1), (32, 4), (40, 6), (128, 16)]
# flags 1 (hand-off granules kept in the XCD's L2: what the trainer runs) at every length; flags 0 (agent-scope write-through: the
# other set of instantiations, which differs in its hand-off stores alone) at one
GPU_CASES = [(B, R, T, 1) for B, R in ROWS for T in (2, 9, 200)] + [(B, R, 9, 0) for B, R in ROWS]


@pytest.mark.gpu
@pytest.mark.parametrize("B,R,T,flags", GPU_CASES)
def test_bptt_without_dh_ext_equals_zero_dh_ext(hip_device, B, R, T, flags):
    _run_pair(_eng.backend_for(hip_device), hip_device, T, B, R, flags)

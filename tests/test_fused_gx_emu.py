"""tests/test_fused_gx.py's kernel-level checks of lv_lstm_fwd_bf16_persist16_x on the CPU emulator build of the same kernel
source (every workgroup of the grid live at once; hand-off polls yield; 16-byte stores tear)."""
import pytest
import torch

import test_fused_gx as F

CPU = torch.device("cpu")


@pytest.mark.parametrize("T,B,R,f16,flags,per_row", [(3, 3, 2, False, 0, True), (9, 1, 1, True, 1, False), (5, 3, 4, False, 1, True)])
def test_fused_gx_forward_emulated(emu_backend, T, B, R, f16, flags, per_row):
    """T shorter than a pass with a ragged last group; three passes (record-buffer and staging reuse) at one row per group; one
    full pass + one step with 3 of the 4 rows.  Few groups carry rows (the others leave at once): a group and timestep cost the
    emulator about a second, (3, 13, 2) and (9, 8, 1) took 40 s and 137 s and passed."""
    F.check_fused_forward(emu_backend, CPU, T, B, R, f16, flags, per_row)


def test_fused_gx_projection_error_emulated(emu_backend):
    F.check_projection_error(emu_backend, CPU, 2, 1, False, True)


def test_fused_gx_refusals_emulated(emu_backend):
    F.check_refusals(emu_backend, CPU)

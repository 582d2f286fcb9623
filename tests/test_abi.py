"""The C-ABI shared library builds for gfx950, loads, and exports every symbol include/lvae.h declares with the
signature table the ctypes binding uses.  No compute calls (no GPU needed)."""
import ctypes
import os
import re
import sys

from vae_lagging_encoder_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    with open(os.path.join(ROOT, "include", "lvae.h")) as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|long)\s+(lv_[a-z0-9_]+)\s*\(", text)))


def test_header_and_binding_agree():
    syms = header_symbols()
    assert syms, "no declarations parsed from include/lvae.h"
    assert sorted(_lib.SIGNATURES.keys()) == syms


def test_hip_library_builds_loads_and_exports_everything():
    path = build.build_hip()
    assert os.path.exists(path)
    cdll = ctypes.CDLL(path)
    for name in header_symbols():
        assert hasattr(cdll, name), name
    lib = _lib.bind(cdll, path)
    # value-returning helpers are host-only and safe to call without a GPU
    assert lib.lv_lstm_bwd_ksplit(1024) == 4
    assert lib.lv_sumsq_workspace_floats() >= 256


def test_argument_checks_return_negative_status_without_touching_the_gpu():
    lib = _lib.bind(ctypes.CDLL(build.build_hip()))
    raw = lib.cdll.lv_gemm_f32
    assert raw(0, 1, -1, 4, 4, 1.0, None, 4, None, 4, None, 4, 0, None, 0, 1, None, 0, 1, None, 0, None) < 0
    assert raw(0, 1, 4, 4, 4, 1.0, None, 4, None, 4, None, 4, 0, None, 0, 1, None, 0, 1, None, 0, None) < 0   # NULL operands
    assert lib.cdll.lv_lstm_fwd_f32(None, None, None, None, None, None, 1.0, None, None, 1, 1, 1, None) < 0
    assert lib.lv_lstm_ws_floats(32, 1024) > 4 * 1024 * 1024


def test_package_has_no_cpu_fallback():
    import torch
    from vae_lagging_encoder_amd import engine
    sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
    import install as emu_install
    saved = emu_install.install(None)       # the session fixture may have installed the emulator
    try:
        try:
            engine.backend_for(torch.device("cpu"))
            raise AssertionError("CPU tensors must be refused")
        except _lib.LvaeError:
            pass
        # and the package itself carries no switch for it
        assert not any("TEST_BACKEND" in n.upper() or "install_test" in n for n in dir(engine))
    finally:
        emu_install.install(saved)


# Entry points no test names, and why that is acceptable.  Nothing of lv_eval.hip / lv_optim.hip may be listed: those are tested
# kernel by kernel (tests/test_eval_txn_kernels.py, tests/test_adam_txn.py, tests/test_gpu_kernels.py).
EXEMPT = {
    "lv_lstm_persist16_pack2_h16": "the encoder's default binary16 forward operands: tests/test_gpu_parity.py::test_bf16_headline_path_at_headline_shape",
    "lv_pixelcnn_pixel_step_f32": "driven by PixelCNNSampler.step: tests/test_emu_engine.py::test_pixelcnn_incremental_sampling_emulated",
    "lv_pixelcnn_net_words": "host-only size helper (asserted against the packed table in PixelCNNSampler.start)",
    "lv_pixelcnn_block_words": "host-only size helper (asserted against the packed table in PixelCNNSampler.start)",
    "lv_conv32_tap_split": "host-only size helper",
    "lv_conv32_wgrad_slabs": "host-only size helper",
    "lv_dec_cond_ll_f32_ws_floats": "host-only size helper",
}


def _defined_in(*hip_files):
    names = set()
    for f in hip_files:
        with open(os.path.join(ROOT, "vae_lagging_encoder_amd", "csrc", f)) as fh:
            names.update(re.findall(r'extern "C" (?:int|long) (lv_[a-z0-9_]+)\s*\(', fh.read()))
    return names


def test_every_entry_point_is_named_by_a_test():
    """Every key of _lib.SIGNATURES occurs as a whole word in tests/test_*.py or tests/parity_common.py (the exemption list itself
    does not count), or is exempt with a stated reason."""
    tdir = os.path.join(ROOT, "tests")
    files = sorted(f for f in os.listdir(tdir) if re.fullmatch(r"test_\w+\.py", f) or f == "parity_common.py")
    text = {}
    for f in files:
        with open(os.path.join(tdir, f)) as fh:
            text[f] = fh.read()
    text["test_abi.py"], n_cut = re.subn(r"^EXEMPT = \{\n.*?^\}\n", "", text["test_abi.py"], flags=re.S | re.M)
    assert n_cut == 1
    words = set(re.findall(r"\blv_[a-z0-9_]+\b", "\n".join(text.values())))
    unnamed = sorted(n for n in _lib.SIGNATURES if n not in words and n not in EXEMPT)
    assert not unnamed, "entry points no test names: %s" % ", ".join(unnamed)
    assert len(EXEMPT) <= 8
    assert not sorted(set(EXEMPT) - set(_lib.SIGNATURES)), "exempt names that are not entry points"
    assert not sorted(n for n in EXEMPT if n in words), "exempt names a test does name: drop the exemption"
    kernel_tested = _defined_in("lv_eval.hip", "lv_optim.hip")
    assert len(kernel_tested) > 20
    assert not sorted(set(EXEMPT) & kernel_tested)
    for name, reason in EXEMPT.items():
        m = re.search(r"tests/(test_\w+\.py)::(test_\w+)", reason)
        if m:
            assert m.group(1) in text and re.search(r"^def %s\(" % m.group(2), text[m.group(1)], flags=re.M), (name, reason)
        else:
            assert "host-only size helper" in reason, (name, reason)

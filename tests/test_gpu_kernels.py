"""MI355X kernel-level parity: every C-ABI entry point against a float64 torch restatement of the same op."""
import ctypes
import math

import numpy as np
import pytest
import torch

from vae_lagging_encoder_amd import _lib
from vae_lagging_encoder_amd.engine import P, stream_ptr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip_device):
    return _lib.load()


def _s(dev):
    return stream_ptr(dev)


@pytest.mark.parametrize("tA,tB,M,N,K", [
    (0, 1, 130, 140, 37), (0, 0, 130, 140, 37), (1, 0, 70, 260, 50), (1, 1, 33, 17, 20),
    (0, 1, 512, 4096, 512), (0, 0, 640, 1024, 2001), (1, 0, 2001, 1024, 640), (0, 1, 32, 64, 1024),
    (0, 1, 1, 1, 1), (0, 1, 257, 129, 16), (1, 0, 4096, 32, 32), (0, 0, 32, 32, 4096), (1, 0, 512, 256, 6368),
    (0, 1, 4000, 4100, 64), (0, 0, 100, 70, 3000), (0, 0, 1300, 1024, 4100), (1, 0, 1100, 1200, 2300),
])
def test_gemm_f32(lib, hip_device, tA, tB, M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    lda = (M if tA else K) + 4
    ldb = (K if tB else N) + 8
    A = torch.randn(K if tA else M, lda, generator=g)
    B = torch.randn(N if tB else K, ldb, generator=g)
    C0 = torch.randn(M, N + 3, generator=g)
    add1 = torch.randn(5, N, generator=g)
    add2 = torch.randn(1, N, generator=g)
    Aop = (A[:, :M].t() if tA else A[:, :K]).double()
    Bop = (B[:, :K].t() if tB else B[:, :N]).double()
    ref = 0.5 * (Aop @ Bop) + add1[torch.arange(M) % 5].double() + add2.double() + C0[:, :N].double()
    Ad, Bd, Cd, a1, a2 = (t.to(hip_device) for t in (A, B, C0.clone(), add1, add2))
    ws = torch.empty(1 << 24, device=hip_device)
    lib.lv_gemm_f32(tA, tB, M, N, K, 0.5, P(Ad), lda, P(Bd), ldb, P(Cd), N + 3, 1, P(a1), N, 5, P(a2), N, 1, P(ws), ws.numel(), _s(hip_device))
    out = Cd.cpu()
    assert torch.equal(out[:, N:], C0[:, N:])          # padding columns untouched
    err = float((out[:, :N].double() - ref).abs().max())
    assert err < 2e-6 * (K ** 0.5 + 1) * 8, err


@pytest.mark.parametrize("tA,tB,M,N,K", [
    (0, 1, 130, 140, 37), (0, 0, 130, 140, 70), (1, 0, 70, 260, 50), (1, 1, 33, 17, 20), (0, 1, 1, 1, 1),
    (0, 1, 3000, 2100, 512), (0, 0, 640, 1024, 2001), (1, 0, 2001, 1024, 640), (0, 0, 32, 32, 4096), (1, 0, 512, 256, 6368),
    (0, 0, 1300, 1024, 4100), (1, 0, 1100, 1200, 2300),
])
def test_gemm_bf16(lib, hip_device, tA, tB, M, N, K):
    """bf16 matrix pipe: exact against a float64 product of the bf16-ROUNDED operands (f32-accumulate class error),
    and within bf16 input precision of the unrounded product."""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + 1)
    lda = (M if tA else K) + 4
    ldb = (K if tB else N) + 8
    A = torch.randn(K if tA else M, lda, generator=g)
    B = torch.randn(N if tB else K, ldb, generator=g)
    C0 = torch.randn(M, N + 3, generator=g)
    add1 = torch.randn(5, N, generator=g)
    rb = lambda x: x.to(torch.bfloat16).double()
    Aop = (A[:, :M].t() if tA else A[:, :K])
    Bop = (B[:, :K].t() if tB else B[:, :N])
    ref = 0.5 * (rb(Aop) @ rb(Bop)) + add1[torch.arange(M) % 5].double() + C0[:, :N].double()
    ref_exact = 0.5 * (Aop.double() @ Bop.double()) + add1[torch.arange(M) % 5].double() + C0[:, :N].double()
    Ad, Bd, Cd, a1 = (t.to(hip_device) for t in (A, B, C0.clone(), add1))
    ws = torch.empty(1 << 24, device=hip_device)
    lib.lv_gemm_bf16(tA, tB, M, N, K, 0.5, P(Ad), lda, P(Bd), ldb, P(Cd), N + 3, 1, P(a1), N, 5, None, 0, 1,
                     P(ws), ws.numel(), _s(hip_device))
    out = Cd.cpu()
    assert torch.equal(out[:, N:], C0[:, N:])
    assert float((out[:, :N].double() - ref).abs().max()) < 2e-6 * (K ** 0.5 + 1) * 8
    assert float((out[:, :N].double() - ref_exact).abs().max()) < 2e-2 * (K ** 0.5 + 1)


def _bf16_bits(x):
    """f32 tensor -> int16 tensor holding the RNE bf16 bit patterns (what lv_cvt_bf16_f32 produces)."""
    return x.to(torch.bfloat16).view(torch.int16)


@pytest.mark.parametrize("R,C", [(1, 1), (64, 64), (70, 130), (200, 33), (641, 1024)])
def test_cvt_bf16(lib, hip_device, R, C):
    g = torch.Generator().manual_seed(R * 5 + C)
    lds, ldd, ldt = C + 3, C + 5, R + 7
    src = torch.randn(R, lds, generator=g)
    src[0, 0] = 1.00390625            # exact tie between two bf16 values: RNE picks the even mantissa (1.0)
    d = torch.full((R, ldd), 0x1234, dtype=torch.int16)
    dT = torch.full((C, ldt), 0x1234, dtype=torch.int16)
    sd, dd, dTd = src.to(hip_device), d.to(hip_device), dT.to(hip_device)
    lib.lv_cvt_bf16_f32(P(sd), lds, R, C, P(dd), ldd, P(dTd), ldt, _s(hip_device))
    want = _bf16_bits(src[:, :C])
    assert torch.equal(dd.cpu()[:, :C], want)
    assert torch.equal(dTd.cpu()[:, :R], want.t())
    assert bool((dd.cpu()[:, C:] == 0x1234).all()) and bool((dTd.cpu()[:, R:] == 0x1234).all())   # padding untouched
    only_t = torch.zeros(C, ldt, dtype=torch.int16, device=hip_device)
    lib.lv_cvt_bf16_f32(P(sd), lds, R, C, None, 0, P(only_t), ldt, _s(hip_device))
    assert torch.equal(only_t.cpu()[:, :R], want.t())


@pytest.mark.parametrize("mode,R,C", [("plain", 70, 52), ("plain", 131, 128), ("gates", 4 * 24, 40), ("lo", 66, 68), ("lo_gates", 4 * 20, 36),
                                      ("h16", 203, 64), ("h16_gates", 4 * 17, 132)])
def test_cvt_16_byte_form(lib, hip_device, mode, R, C):
    """The conversions on operands that allow the 16-byte form of the kernel (C % 4 == 0, strides % 4 == 0: cvt_b16_v4_kernel -- one
    float4 load and one 8-byte store per four elements, transposed image as 8-byte stores of four rows): every variant bit for bit
    against torch, ragged R (tail of the transposed rows), padding untouched.  (Odd strides -- the tests above -- take cvt_b16_kernel.)"""
    dev = hip_device
    g = torch.Generator().manual_seed(R * 7 + C)
    lds, ldd, ldt = C + 4, C + 8, (R + 3) // 4 * 4 + 4
    src = torch.randn(R, lds, generator=g) * 3.0
    src[0, 0] = 1.00390625
    rows = src[:, :C]
    bf = rows.to(torch.bfloat16)
    gates = mode.endswith("gates")
    H = R // 4
    perm = torch.arange(4 * H).view(4, H).t().reshape(-1) if gates else None
    d = torch.full((R, ldd), 0x1234, dtype=torch.int16, device=dev)
    dT = torch.full((C, ldt), 0x1234, dtype=torch.int16, device=dev)
    sd = src.to(dev)
    if mode in ("plain",):
        lib.lv_cvt_bf16_f32(P(sd), lds, R, C, P(d), ldd, P(dT), ldt, _s(dev))
        want_d = want_t = bf.view(torch.int16)
    elif mode == "gates":
        lib.lv_cvt_bf16_gates_f32(P(sd), lds, H, C, P(d), ldd, P(dT), ldt, _s(dev))
        want_t = bf.view(torch.int16); want_d = want_t[perm]
    elif mode.startswith("lo"):
        lib.lv_cvt_bf16_lo_f32(P(sd), lds, R, C, H if gates else 0, None, 0, 1, 0, P(d), ldd, P(dT), ldt, _s(dev))
        want_t = (rows - bf.float()).to(torch.bfloat16).view(torch.int16); want_d = want_t[perm] if gates else want_t
    else:
        lib.lv_cvt_h16_f32(P(sd), lds, R, C, H if gates else 0, None, 0, 1, 0, P(d), ldd, P(dT), ldt, _s(dev))
        want_t = bf.view(torch.int16)
        want_d = rows.clamp(-65504.0, 65504.0).to(torch.float16).view(torch.int16)
        if gates: want_d = want_d[perm]
    assert torch.equal(d.cpu()[:, :C], want_d)
    assert torch.equal(dT.cpu()[:, :R], want_t.t())
    assert bool((d.cpu()[:, C:] == 0x1234).all()) and bool((dT.cpu()[:, R:] == 0x1234).all())


@pytest.mark.parametrize("mode,R,C", [("plain", 70, 50), ("plain", 64, 128), ("gates", 4 * 24, 40), ("gather", 5 * 7, 33)])
def test_cvt_bf16_lo(lib, hip_device, mode, R, C):
    """lv_cvt_bf16_lo_f32: the low half of a split-bf16 operand, bit for bit bf16(x - bf16(x)), in the plain, gate-interleaved and
    gathered layouts of the three high-half conversions; hi + lo reproduces x to 2^-16 |x| (bf16 RNE of a residual <= 2^-9 |x|)."""
    g = torch.Generator().manual_seed(R * 3 + C)
    dev = hip_device
    lds, ldd, ldt = C + 3, C + 8, R + 5
    if mode == "gather":
        T, B, V = 5, 7, 19
        src = torch.randn(V, C, generator=g); lds = C
        ids = torch.randint(0, V, (B, T + 2), generator=g)
        rows = torch.stack([src[ids[b, t]] for t in range(T) for b in range(B)])
    else:
        src = torch.randn(R, lds, generator=g)
        rows = src[:, :C]
    hi = rows.to(torch.bfloat16).float()
    want = _bf16_bits(rows - hi)
    if mode == "gates":
        H = R // 4
        want_d = want[torch.arange(4 * H).view(4, H).t().reshape(-1)]
    else:
        want_d = want
    d = torch.full((R, ldd), 0x1234, dtype=torch.int16, device=dev)
    dT = torch.full((C, ldt), 0x1234, dtype=torch.int16, device=dev)
    sd = src.to(dev)
    if mode == "gather":
        idd = ids.to(dev)
        lib.lv_cvt_bf16_lo_f32(P(sd), lds, R, C, 0, P(idd), T + 2, B, V, P(d), ldd, P(dT), ldt, _s(dev))
    else:
        lib.lv_cvt_bf16_lo_f32(P(sd), lds, R, C, R // 4 if mode == "gates" else 0, None, 0, 1, 0, P(d), ldd, P(dT), ldt, _s(dev))
    assert torch.equal(d.cpu()[:, :C], want_d)
    assert torch.equal(dT.cpu()[:, :R], want.t())
    assert bool((d.cpu()[:, C:] == 0x1234).all()) and bool((dT.cpu()[:, R:] == 0x1234).all())
    lo = want.view(torch.bfloat16).float()
    assert float((hi + lo - rows).abs().max()) <= 2.0 ** -16 * float(rows.abs().max())


@pytest.mark.parametrize("H,C,R", [(8, 16, 3), (50, 33, 1), (256, 128, 5)])
def test_gate_interleave_and_gate_weight_image(lib, hip_device, H, C, R):
    g = torch.Generator().manual_seed(H + C)
    W = torch.randn(4 * H, C + 3, generator=g)
    a = torch.randn(R, 4 * H, generator=g)
    b = torch.randn(R, 4 * H, generator=g)
    perm = torch.arange(4 * H).view(4, H).t().reshape(-1)           # unit-major position 4u+g <- gate-major g*H+u
    Wd, ad, bd = W.to(hip_device), a.to(hip_device), b.to(hip_device)
    img = torch.zeros(4 * H, C + 5, dtype=torch.int16, device=hip_device)
    imgT = torch.zeros(C, 4 * H + 8, dtype=torch.int16, device=hip_device)
    lib.lv_cvt_bf16_gates_f32(P(Wd), C + 3, H, C, P(img), C + 5, P(imgT), 4 * H + 8, _s(hip_device))
    want = _bf16_bits(W[:, :C])
    assert torch.equal(img.cpu()[:, :C], want[perm])
    assert torch.equal(imgT.cpu()[:, :4 * H], want.t())
    out = torch.empty(R, 4 * H, device=hip_device)
    lib.lv_gate_interleave_f32(P(ad), P(bd), R, H, P(out), _s(hip_device))
    assert torch.equal(out.cpu(), (a + b)[:, perm])
    lib.lv_gate_interleave_f32(P(ad), None, R, H, P(out), _s(hip_device))
    assert torch.equal(out.cpu(), a[:, perm])


@pytest.mark.parametrize("T,B,H,use_mask", [(3, 5, 50, True), (2, 33, 20, False), (4, 32, 256, True)])
def test_lstm_fwd_unit_major_gx(lib, hip_device, T, B, H, use_mask):
    """Same recurrence fed the gate pre-activations in unit-major column order: every output bit-identical."""
    dev = hip_device
    g = torch.Generator().manual_seed(T + B + H)
    gx = (torch.randn(T, B, 4 * H, generator=g) * 0.5).to(dev)
    whh = (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(dev)
    mask = (torch.rand(B, T, H, generator=g) < 0.5).to(torch.uint8).to(dev)
    perm = torch.arange(4 * H).view(4, H).t().reshape(-1).to(dev)
    gxu = gx[:, :, perm].contiguous()
    for pair in ((lib.lv_lstm_fwd_bf16, lib.lv_lstm_fwd_bf16_ug), (lib.lv_lstm_fwd_f32, lib.lv_lstm_fwd_f32_ug)):
        outs = []
        for fn, x in zip(pair, (gx, gxu)):
            hs = torch.zeros(T + 1, B, H, device=dev)
            cs = torch.zeros(T + 1, B, H, device=dev)
            hs[0] = 0.1
            cs[0] = -0.2
            gates = torch.empty(T, B, 4 * H, device=dev)
            hdrop = torch.empty(T, B, H, device=dev)
            ws = torch.empty(lib.lv_lstm_ws_floats(B, H), device=dev)
            fn(P(x), P(whh), P(hs), P(cs), P(gates), P(mask) if use_mask else None, 2.0, P(hdrop), P(ws), T, B, H, _s(dev))
            outs.append((hs.cpu(), cs.cpu(), gates.cpu(), hdrop.cpu()))
        for a, b in zip(*outs):
            assert torch.equal(a, b)


@pytest.mark.parametrize("tA,M,N,K,split", [
    (0, 130, 140, 37, False), (1, 70, 130, 50, False), (0, 1, 1, 1, False), (1, 33, 17, 20, False), (1, 129, 64, 200, False),
    (0, 257, 129, 1000, True), (1, 301, 100, 1100, True), (0, 640, 1024, 2001, True), (1, 2001, 1024, 640, False),
    (0, 3000, 2100, 512, False), (1, 1100, 1200, 2300, True),
])
def test_gemm_b16(lib, hip_device, tA, M, N, K, split, exact=None, tile=0):
    """Pre-rounded bf16 operands: bit-identical to lv_gemm_bf16 on the f32 data when neither splits K (same MFMA
    chain), f32-accumulate-class agreement with a float64 product of the rounded operands always."""
    exact = (not split) if exact is None else exact
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + 2)
    lda = ((M + 7) // 8) * 8 + 8 if tA else ((K + 7) // 8) * 8 + 8
    ldb = ((K + 7) // 8) * 8
    A = torch.randn(K if tA else M, lda, generator=g)
    B = torch.randn(N, ldb, generator=g)
    A[:, (M if tA else K):] = float("nan")          # row padding may be read but must never reach the result
    B[:, K:] = float("nan")
    C0 = torch.randn(M, N + 3, generator=g)
    mod = 5 if M % 2 else 37                         # addend rows cycle with the output row (small modulus / >= 32: two index paths)
    add1 = torch.randn(mod, N, generator=g)
    rb = lambda x: x.to(torch.bfloat16).double()
    Aop = (A[:, :M].t() if tA else A[:, :K])
    Bop = B[:, :K].t()
    ref = 0.5 * (rb(Aop) @ rb(Bop)) + add1[torch.arange(M) % mod].double() + C0[:, :N].double()
    A16, B16 = _bf16_bits(A).to(hip_device), _bf16_bits(B).to(hip_device)
    Ad, Bd, a1 = A.to(hip_device), B.to(hip_device), add1.to(hip_device)
    C1, C2 = C0.clone().to(hip_device), C0.clone().to(hip_device)
    ws = torch.empty(1 << 24, device=hip_device) if split else None
    wsp, wsn = (P(ws), ws.numel()) if split else (None, 0)
    lib.lv_gemm_b16_tile(tile, tA, M, N, K, 0.5, P(A16), lda, P(B16), ldb, P(C1), N + 3, 1, P(a1), N, mod, None, 0, 1, wsp, wsn, _s(hip_device))
    out = C1.cpu()
    assert torch.equal(out[:, N:], C0[:, N:])
    assert float((out[:, :N].double() - ref).abs().max()) < 2e-6 * (K ** 0.5 + 1) * 8
    if exact:
        lib.lv_gemm_bf16(tA, 1, M, N, K, 0.5, P(Ad), lda, P(Bd), ldb, P(C2), N + 3, 1, P(a1), N, mod, None, 0, 1, None, 0,
                         _s(hip_device))
        assert torch.equal(out, C2.cpu())


@pytest.mark.parametrize("tA,M,N,K,split", [
    (0, 130, 140, 37, False), (1, 70, 130, 50, False), (0, 1, 1, 1, False), (1, 300, 260, 200, False), (0, 257, 513, 1000, True),
    (1, 301, 100, 1100, True), (0, 640, 1024, 2001, True), (1, 2001, 1024, 640, False), (0, 3000, 2100, 512, False),
    (1, 1100, 1200, 2304, True), (0, 4200, 4100, 320, True),
    (0, 7100, 7000, 130, False), (1, 7000, 7100, 200, True),      # 784 tiles: three whole rounds of 256 + a tail
])
@pytest.mark.parametrize("tile", [256, 257, 258])
def test_gemm_b16_tile256(lib, hip_device, tA, M, N, K, split, tile):
    """The 256 x 256 x 64 kernel (forced; 256 = lockstep K loop, 257 = the two wave groups half a k-step apart): same checks; with a
    workspace the tail tiles (tiles % 256) are cut along K and reduced in piece order.  Bit-identical to the 128 x 128 chain when K
    is a multiple of 64 and nothing is cut (the ragged K tile is accumulated first here, last there)."""
    test_gemm_b16(lib, hip_device, tA, M, N, K, split, exact=(not split) and K % 64 == 0, tile=tile)


@pytest.mark.parametrize("T,B,N,K,big", [(5, 4, 70, 100, False), (9, 32, 64, 1100, False), (40, 32, 1024, 4200, True), (3, 7, 300, 64, False)])
def test_gemm_b16_keep(lib, hip_device, T, B, N, K, big):
    """lv_gemm_b16_keep: C = (A . B^T) * (keep ? kscale : 0), the dropout backward applied in the product's reduction stage (split-K
    reduce of the 128 x 128 kernel, tail reduce of the 256 x 256 one) or, where there is none, by a pass of its own -- bit-identical
    to lv_gemm_b16 followed by lv_keep_scale_f32."""
    dev = hip_device
    g = torch.Generator().manual_seed(T * 31 + N)
    M = T * B
    lda = ldb = ((K + 7) // 8) * 8
    A16 = _bf16_bits(torch.randn(M, lda, generator=g)).to(dev)
    B16 = _bf16_bits(torch.randn(N, ldb, generator=g)).to(dev)
    keep = (torch.rand(B, T, N, generator=g) < 0.5).to(torch.uint8).to(dev)
    ws = torch.empty(1 << 24, device=dev)
    C1 = torch.full((M, N), float("nan"), device=dev)
    C2 = torch.full((M, N), float("nan"), device=dev)
    lib.lv_gemm_b16_keep(M, N, K, P(A16), lda, P(B16), ldb, P(C1), P(keep), 2.0, B, P(ws), ws.numel(), _s(dev))
    lib.lv_gemm_b16(0, M, N, K, 1.0, P(A16), lda, P(B16), ldb, P(C2), N, 0, None, 0, 1, None, 0, 1, P(ws), ws.numel(), _s(dev))
    lib.lv_keep_scale_f32(P(C2), P(keep), 2.0, T, B, N, _s(dev))
    assert torch.equal(C1.cpu(), C2.cpu())
    ref = (A16.cpu().view(torch.bfloat16).double()[:, :K] @ B16.cpu().view(torch.bfloat16).double()[:, :K].t())
    ref = ref.view(T, B, N) * keep.cpu().double().permute(1, 0, 2) * 2.0
    assert float((C1.cpu().double().view(T, B, N) - ref).abs().max()) < 2e-6 * (K ** 0.5 + 1) * 16


@pytest.mark.parametrize("tA,M,N,K", [(1, 20001, 1024, 6368), (0, 2048, 2304, 1536), (1, 4100, 1024, 3100), (0, 1024, 1024, 200)])
def test_gemm_b16_sumsq(lib, hip_device, tA, M, N, K):
    """lv_gemm_b16_sumsq: the product as lv_gemm_b16 writes it (bit for bit) and partial sums of squares that add up to its
    squared Frobenius norm -- tiles that hold whole-K results, tail tiles whose K pieces meet in the reduce kernel, ragged edges
    (rows / columns outside C contribute nothing); sq_only leaves C alone; shapes off the 256 x 256 tile are refused."""
    if hip_device.type != "cuda":
        pytest.skip("GPU only")
    dev = hip_device
    g = torch.Generator().manual_seed(M + N + K)
    ld_a = (M + 7) // 8 * 8 if tA else (K + 7) // 8 * 8
    ld_b = (K + 7) // 8 * 8
    A = (torch.randn((K, ld_a) if tA else (M, ld_a), generator=g) * 0.1).to(torch.bfloat16).view(torch.int16).to(dev)
    Bm = (torch.randn(N, ld_b, generator=g) * 0.1).to(torch.bfloat16).view(torch.int16).to(dev)
    ws = torch.empty(1 << 26, device=dev)
    n = lib.lv_gemm_b16_sumsq_parts(M, N, K, ws.numel())
    C0 = torch.empty(M, N, device=dev)
    lib.lv_gemm_b16(tA, M, N, K, 1.0, P(A), ld_a, P(Bm), ld_b, P(C0), N, 0, None, 0, 1, None, 0, 1, P(ws), ws.numel(), _s(dev))
    if n == 0:
        sq = torch.zeros(8, device=dev)
        with pytest.raises(_lib.LvaeError):
            lib.lv_gemm_b16_sumsq(tA, M, N, K, P(A), ld_a, P(Bm), ld_b, P(C0), N, P(ws), ws.numel(), P(sq), 0, _s(dev))
        return
    sq = torch.full((n,), float("nan"), device=dev)
    C1 = torch.full((M, N), float("nan"), device=dev)
    lib.lv_gemm_b16_sumsq(tA, M, N, K, P(A), ld_a, P(Bm), ld_b, P(C1), N, P(ws), ws.numel(), P(sq), 0, _s(dev))
    assert torch.equal(C1, C0)
    want = float(C0.double().pow(2).sum())
    assert abs(float(sq.double().sum()) - want) <= 1e-5 * want
    sq2 = torch.full((n,), float("nan"), device=dev)
    C2 = torch.full((M, N), 3.0, device=dev)
    lib.lv_gemm_b16_sumsq(tA, M, N, K, P(A), ld_a, P(Bm), ld_b, P(C2), N, P(ws), ws.numel(), P(sq2), 1, _s(dev))
    assert torch.equal(sq2, sq) and float((C2 - 3.0).abs().max()) == 0.0


@pytest.mark.parametrize("world,V,ni,counts,b16", [(2, 53, 8, (5, 9), 0), (3, 200, 64, (40, 1, 17), 1), (8, 1000, 512, (120,) * 8, 0),
                                                    (2, 37, 12, (37, 37), 1)])
def test_rows_merge(lib, hip_device, world, V, ni, counts, b16):
    """lv_rows_merge_f32: the dense mean embedding gradient rebuilt from every rank's (sorted ids, rows) list -- overlapping and
    disjoint token sets, an absent rank list entry (-1 padding), every row of the table written (zeros where nobody has it), rows
    added in rank order."""
    dev = hip_device
    g = torch.Generator().manual_seed(V + world)
    cap = (max(counts) + 7) // 8 * 8
    ids = torch.full((world, cap), -1, dtype=torch.int64)
    rows = torch.zeros(world, cap, ni)
    ref = torch.zeros(V, ni, dtype=torch.float64)
    for r, n in enumerate(counts):
        pick = torch.randperm(V, generator=g)[:n].sort().values
        ids[r, :n] = pick
        vals = torch.randn(n, ni, generator=g)
        if b16:
            vals = vals.to(torch.bfloat16).float()
        rows[r, :n] = vals
        rows[r, n:] = float("nan")                        # padding slots must never be read into the result
    acc = torch.zeros(V, ni)
    for r, n in enumerate(counts):                         # rank order, f32: the kernel's summation order
        acc[ids[r, :n]] += rows[r, :n]
    acc = acc * (1.0 / world)
    wire = rows.to(torch.bfloat16).view(torch.int16) if b16 else rows
    dE = torch.full((V, ni), float("nan"), device=dev)
    ids_d, wire_d = ids.to(dev), wire.to(dev)                 # (held: a temporary's block may be handed out again at once)
    lib.lv_rows_merge_f32(P(ids_d), P(wire_d), b16, world, cap, ni, V, 1.0 / world, P(dE), _s(dev))
    assert torch.equal(dE.cpu(), acc)


def test_gemm_b16_alignment_errors(lib, hip_device):
    z = torch.zeros(64, 64, dtype=torch.int16, device=hip_device)
    c = torch.zeros(8, 8, device=hip_device)
    with pytest.raises(_lib.LvaeError):
        lib.lv_gemm_b16(0, 8, 8, 8, 1.0, P(z), 12, P(z), 8, P(c), 8, 0, None, 0, 1, None, 0, 1, None, 0, _s(hip_device))
    with pytest.raises(_lib.LvaeError):
        lib.lv_gemm_b16(1, 8, 8, 8, 1.0, P(z), 10, P(z), 8, P(c), 8, 0, None, 0, 1, None, 0, 1, None, 0, _s(hip_device))


def test_gemm_unaligned_rows(lib, hip_device):
    # ld % 4 != 0 and odd base offset: scalar load path (toy config has ni + nz = 51)
    g = torch.Generator().manual_seed(5)
    M, N, K = 45, 200, 50
    A = torch.randn(M, 51, generator=g)
    B = torch.randn(N, 51, generator=g)
    ref = A[:, 1:].double() @ B[:, 1:].double().t()
    Ad, Bd = A.to(hip_device), B.to(hip_device)
    C = torch.zeros(M, N, device=hip_device)
    lib.lv_gemm_f32(0, 1, M, N, K, 1.0, P(Ad, 1), 51, P(Bd, 1), 51, P(C), N, 0, None, 0, 1, None, 0, 1, None, 0, _s(hip_device))
    assert float((C.cpu().double() - ref).abs().max()) < 1e-4


def _lstm_ref(gx, whh, h0, c0, mask, scale):
    T, B, _ = gx.shape
    H = whh.shape[1]
    h, c = h0, c0
    hs, cs, outs = [h0], [c0], []
    for t in range(T):
        a = gx[t] + h @ whh.t()
        i, f, g, o = a.chunk(4, -1)
        i, f, o, g = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(g)
        c = f * c + i * g
        h = o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
        outs.append(h * mask[:, t].to(h.dtype) * scale if mask is not None else h)
    return torch.stack(hs), torch.stack(cs), torch.stack(outs)


@pytest.mark.parametrize("T,B,H,use_mask,tanh_init,use_ext,use_last", [
    (6, 32, 1024, True, True, True, False),      # decoder-shaped (Yahoo dims)
    (6, 32, 1024, False, False, False, True),    # encoder-shaped
    (3, 5, 50, True, True, True, True),          # toy dims, unaligned H
    (4, 128, 256, False, True, True, False),     # stress batch
    (2, 130, 64, True, False, True, True),       # batch > 128 -> two batch chunks
])
def test_lstm_fwd_bwd(lib, hip_device, T, B, H, use_mask, tanh_init, use_ext, use_last, prec="f32"):
    dev = hip_device
    fwd = lib.lv_lstm_fwd_f32 if prec == "f32" else lib.lv_lstm_fwd_bf16
    bwd = lib.lv_lstm_bwd_f32 if prec == "f32" else lib.lv_lstm_bwd_bf16
    tol = 1.0 if prec == "f32" else 300.0       # bf16 recurrent operands: ~2^-9 relative per product
    g = torch.Generator().manual_seed(T * 100 + B + H)
    gx = (torch.randn(T, B, 4 * H, generator=g) * 0.5).to(dev)
    whh = (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(dev)
    c0 = (torch.randn(B, H, generator=g) * 0.5).to(dev)
    mask = (torch.rand(B, T, H, generator=g) < 0.5).to(dev)
    wext = torch.randn(T, B, H, generator=g).to(dev)
    wlast = torch.randn(B, H, generator=g).to(dev)
    gx64 = gx.double().requires_grad_(True)
    whh64 = whh.double()
    c064 = c0.double().requires_grad_(True)
    h064 = torch.tanh(c064) if tanh_init else torch.zeros_like(c064)
    hs_r, cs_r, out_r = _lstm_ref(gx64, whh64, h064, c064, mask if use_mask else None, 2.0)
    loss = 0
    if use_ext:
        loss = loss + (out_r * wext.double()).sum()
    if use_last:
        loss = loss + (hs_r[-1] * wlast.double()).sum()
    loss.backward()
    hs = torch.zeros(T + 1, B, H, device=dev)
    cs = torch.zeros(T + 1, B, H, device=dev)
    hs[0] = h064.detach().float()
    cs[0] = c0
    gates = torch.empty(T, B, 4 * H, device=dev)
    hdrop = torch.empty(T, B, H, device=dev)
    m8 = mask.to(torch.uint8).contiguous()
    ws = torch.empty(lib.lv_lstm_ws_floats(B, H), device=dev)
    fwd(P(gx), P(whh), P(hs), P(cs), P(gates), P(m8) if use_mask else None, 2.0, P(hdrop), P(ws), T, B, H, _s(dev))
    assert float((hs.double() - hs_r.detach()).abs().max()) < 2e-5 * tol
    assert float((cs.double() - cs_r.detach()).abs().max()) < 2e-5 * tol
    assert float((hdrop.double() - out_r.detach()).abs().max()) < 4e-5 * tol
    whhT = torch.empty(H, 4 * H, device=dev)
    lib.lv_transpose_f32(P(whh), P(whhT), 4 * H, H, _s(dev))
    assert torch.equal(whhT, whh.t().contiguous())
    dG = torch.empty(T, B, 4 * H, device=dev)
    dGsum = torch.full((B, 4 * H), 7.0, device=dev)
    dc0 = torch.empty(B, H, device=dev)
    ws.fill_(float("nan"))            # scratch content must not matter
    if prec == "bf16_img":          # one launch per step; also emits the bf16 image of dG and dh0
        dG16 = torch.full((T, B, 4 * H), 0x7FC0, dtype=torch.int16, device=dev)
        dh0 = torch.empty(B, H, device=dev)
        lib.lv_lstm_bwd_bf16_img(P(wext) if use_ext else None, P(wlast) if use_last else None, P(m8) if use_mask else None, 2.0,
                                   P(whh), P(gates), P(hs), P(cs), P(dG), P(dG16), P(dGsum), P(ws), P(dh0), P(dc0),
                                   int(tanh_init), T, B, H, _s(dev))
        assert torch.equal(dG16.cpu(), dG.cpu().to(torch.bfloat16).view(torch.int16))
        if not tanh_init:             # then h0 is a free input: dh0 = d loss / d h0 = dG[0] . W_hh
            ref_dh0 = gx64.grad[0] @ whh64
            assert float((dh0.double() - ref_dh0).abs().max()) < 1e-4 * float(ref_dh0.abs().max()) * tol
        only16 = torch.empty_like(dG16)
        dGsum2 = torch.empty_like(dGsum)
        lib.lv_lstm_bwd_bf16_img(P(wext) if use_ext else None, P(wlast) if use_last else None, P(m8) if use_mask else None, 2.0,
                                   P(whh), P(gates), P(hs), P(cs), None, P(only16), P(dGsum2), P(ws), None, None,
                                   int(tanh_init), T, B, H, _s(dev))
        assert torch.equal(only16, dG16) and torch.equal(dGsum2, dGsum)
    else:
        bwd(P(wext) if use_ext else None, P(wlast) if use_last else None, P(m8) if use_mask else None, 2.0,
            P(whh), P(gates), P(hs), P(cs), P(dG), P(dGsum), P(ws), None, P(dc0),
            int(tanh_init), T, B, H, _s(dev))
    sc = float(gx64.grad.abs().max())
    assert float((dG.double() - gx64.grad).abs().max()) < 1e-4 * sc * tol
    assert float((dGsum.double() - gx64.grad.sum(0)).abs().max()) < 1e-4 * sc * T * tol
    assert float((dc0.double() - c064.grad).abs().max()) < 1e-4 * float(c064.grad.abs().max()) * tol


@pytest.mark.parametrize("T,B,H,use_mask,tanh_init,use_ext,use_last", [
    (6, 32, 1024, True, True, True, False), (3, 5, 50, True, True, True, True), (4, 128, 256, False, True, True, False),
    (2, 130, 64, True, False, True, True), (5, 32, 1024, False, False, False, True),
])
def test_lstm_fwd_bwd_bf16_recurrence(lib, hip_device, T, B, H, use_mask, tanh_init, use_ext, use_last):
    test_lstm_fwd_bwd(lib, hip_device, T, B, H, use_mask, tanh_init, use_ext, use_last, prec="bf16")


@pytest.mark.parametrize("T,B,H,use_mask,tanh_init,use_ext,use_last", [
    (6, 32, 1024, True, True, True, False), (3, 5, 50, True, True, True, True), (4, 128, 256, False, True, True, False),
    (2, 130, 64, True, False, True, True), (5, 32, 1024, False, False, False, True), (1, 7, 33, True, False, True, True),
])
def test_lstm_bwd_bf16_img(lib, hip_device, T, B, H, use_mask, tanh_init, use_ext, use_last):
    test_lstm_fwd_bwd(lib, hip_device, T, B, H, use_mask, tanh_init, use_ext, use_last, prec="bf16_img")


def _saved16_pack(lib, gates, cs, R):
    """gates [T][B][4H] (unit-major: (i, f, g, o) per unit) and cs [T + 1][B][H] -> the workgroup-major saved-activation buffer of
    lv_lstm_persist16.hip: saved[group][member][t]{ gates [R][32][4], c [R][32] }, R rows per group (c_t = cs[t + 1])."""
    T, B, H = gates.shape[0], gates.shape[1], gates.shape[2] // 4
    g = torch.zeros(T, 8 * R, H, 4, device=gates.device); g[:, :B] = gates.view(T, B, H, 4)
    c = torch.zeros(T, 8 * R, H, device=gates.device); c[:, :B] = cs[1:]
    g = g.view(T, 8, R, 32, 32 * 4).permute(1, 3, 0, 2, 4).reshape(8, 32, T, R * 128)
    c = c.view(T, 8, R, 32, 32).permute(1, 3, 0, 2, 4).reshape(8, 32, T, R * 32)
    out = torch.cat([g, c], dim=3).contiguous().view(-1)
    assert out.numel() == lib.lv_lstm_persist16_saved_floats(T, R)
    return out


def _saved16_unpack(saved, T, B, R, H=1024):
    """The inverse: (gates [T][B][4H], c_0 .. c_{T-1} as [T][B][H])."""
    sv = saved.view(8, 32, T, R * 160)
    g = sv[..., :R * 128].reshape(8, 32, T, R, 32 * 4).permute(2, 0, 3, 1, 4).reshape(T, 8 * R, 4 * H)
    c = sv[..., R * 128:].reshape(8, 32, T, R, 32).permute(2, 0, 3, 1, 4).reshape(T, 8 * R, H)
    return g[:, :B].contiguous(), c[:, :B].contiguous()


@pytest.mark.parametrize("T,B,R", [(5, 32, 4), (3, 13, 2), (4, 100, 13), (2, 128, 16), (7, 32, 8)])
def test_persist16_import_saved(lib, hip_device, T, B, R):
    """lv_lstm_persist16_import_saved: the step kernels' saved activations (gates [T][B][H][4], cs [T+1][B][H]) land in the persistent
    BPTT's record buffer exactly where a persistent forward would have put them (rows beyond B of the last group are never read)."""
    dev, H = hip_device, 1024
    g = torch.Generator().manual_seed(T * 31 + B)
    gates = torch.randn(T, B, 4 * H, generator=g).to(dev)
    cs = torch.randn(T + 1, B, H, generator=g).to(dev)
    want = _saved16_pack(lib, gates, cs, R)
    got = torch.full_like(want, float("nan"))
    lib.lv_lstm_persist16_import_saved(P(gates), P(cs), P(got), T, B, R, H, _s(dev))
    g2, c2 = _saved16_unpack(got, T, B, R)
    g1, c1 = _saved16_unpack(want, T, B, R)
    assert torch.equal(g2.cpu(), g1.cpu()) and torch.equal(c2.cpu(), c1.cpu())
    assert torch.equal(g2.cpu(), gates.cpu()) and torch.equal(c2.cpu(), cs[1:].cpu())


def _bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


def _lstm_ref_bf16_recurrent(gx, whh, h0, c0):
    """float64 LSTM whose recurrent product sees what the bf16 kernels feed the matrix pipe: W_hh and h_{t-1} rounded to bf16
    (RNE), everything else exact.  A kernel then differs from it by f32 accumulation order, the hardware exp / reciprocal of the
    activations (~1e-6) and by what an h element that rounds the other way moves downstream -- not by the 2^-9 operand rounding
    itself, so the comparison can be held to 1e-3 instead of the bf16 noise floor."""
    T = gx.shape[0]
    w = _bf16_round(whh.float()).double()
    h, c = h0, c0
    hs, cs = [h0], [c0]
    for t in range(T):
        a = gx[t] + _bf16_round(h.float()).double() @ w.t()
        i, f, g, o = a.chunk(4, -1)
        i, f, o, g = torch.sigmoid(i), torch.sigmoid(f), torch.sigmoid(o), torch.tanh(g)
        c = f * c + i * g
        h = o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
    return torch.stack(hs), torch.stack(cs)


@pytest.mark.parametrize("T,B,R", [(6, 32, 4), (9, 32, 8), (5, 64, 8), (7, 128, 16), (40, 32, 8), (3, 13, 2), (4, 100, 13), (12, 32, 16),
                                   (1, 5, 5)])
@pytest.mark.parametrize("flags", [0, 1])
def test_lstm_fwd_persistent16(lib, hip_device, T, B, R, flags):
    """The one-launch persistent forward (lv_lstm_persist16.hip, H = 1024): R rows per XCD group -- 8 groups x 4 (the default
    shape), 4 groups x 8 and 2 groups x 16 (a B = 32 recurrence on half / a quarter of the chip), 8 x 8 and 8 x 16 (B = 64 / the
    stress configuration's B = 128), ragged slices; flags 1 = hand-off granules kept in the XCD's L2.  Held to 1e-3 twice: against
    the float64 recurrence on bf16-rounded recurrent operands, and against the launch-per-step kernel fed the same unit-major gx
    (same operands, different f32 summation order) -- the bound the T = 200 test below uses, which is what a half-written
    accumulator or a stale granule fails (the former `tol = 300` admitted a 2 % error)."""
    dev, H = hip_device, 1024
    g = torch.Generator().manual_seed(T * 100 + B)
    gx = (torch.randn(T, B, 4 * H, generator=g) * 0.5).to(dev)
    whh = (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(dev)
    c0 = (torch.randn(B, H, generator=g) * 0.5).to(dev)
    h0 = torch.tanh(c0)
    hs_r, cs_r = _lstm_ref_bf16_recurrent(gx.double(), whh.double(), h0.double(), c0.double())
    perm = torch.arange(4 * H).view(4, H).t().reshape(-1).to(dev)
    gxu = gx[:, :, perm].contiguous()
    res = []
    for persistent in (True, False):
        hs = torch.zeros(T + 1, B, H, device=dev)
        cs = torch.zeros(T + 1, B, H, device=dev)
        hs[0], cs[0] = h0, c0
        gates = torch.empty(T, B, 4 * H, device=dev)
        if persistent:
            wpk = torch.full((lib.lv_lstm_persist16_wpk_floats(),), float("nan"), device=dev)
            ws = torch.full((lib.lv_lstm_persist16_xch_floats(),), float("nan"), device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            lib.lv_lstm_persist16_pack(P(whh), P(wpk), 0, H, _s(dev))
            saved = torch.full((lib.lv_lstm_persist16_saved_floats(T, R),), float("nan"), device=dev)
            lib.lv_lstm_fwd_bf16_persist16(P(gxu), P(wpk), P(hs), P(cs), P(saved), P(ws), P(status), T, B, R, flags, H, _s(dev))
            assert int(status.item()) == 0
            # gates and cell states come back in the kernels' workgroup-major buffer; canonical cs holds the final state only
            gates, c_t = _saved16_unpack(saved, T, B, R)
            assert torch.equal(cs[T], c_t[T - 1]) and float(cs[1:T].abs().max() if T > 1 else 0.0) == 0.0
            cs[1:] = c_t
            gates = gates.view(T, B, 4 * H)
        else:
            ws = torch.empty(lib.lv_lstm_ws_floats(B, H), device=dev)
            hdrop = torch.empty(T, B, H, device=dev)
            lib.lv_lstm_fwd_bf16_ug(P(gxu), P(whh), P(hs), P(cs), P(gates), None, 1.0, P(hdrop), P(ws), T, B, H, _s(dev))
        assert float((hs.double() - hs_r).abs().max()) < 1e-3
        assert float((cs.double() - cs_r).abs().max()) < 1e-3 * max(1.0, float(cs_r.abs().max()))
        res.append((hs.clone(), cs.clone(), gates.clone()))
    for a, b, what in zip(*res, ("h", "c", "gates")):
        assert float((a - b).abs().max()) < 1e-3, what


@pytest.mark.parametrize("T,B,R,flags", [(6, 32, 4, 1), (9, 32, 8, 0), (7, 128, 16, 1), (3, 13, 2, 1), (60, 32, 4, 1)])
def test_lstm_fwd_persistent16_binary16_operands(lib, hip_device, T, B, R, flags):
    """flags bit 5 of the persistent forward: W_hh (register image packed with backward = 2) and the h granules as IEEE binary16 on
    v_mfma_f32_16x16x32_f16.  Against the float64 recurrence whose recurrent product sees binary16-rounded W_hh and h_{t-1} at
    2e-4 (the bf16 form is held to 1e-3 against ITS rounding), and CLOSER to the exact float64 recurrence than the bf16 form is
    (what the format is for: 11 instead of 8 bits of significand on the weights)."""
    dev, H = hip_device, 1024
    g = torch.Generator().manual_seed(T * 100 + B + 3)
    gx = (torch.randn(T, B, 4 * H, generator=g) * 0.5).to(dev)
    whh = (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(dev)
    c0 = (torch.randn(B, H, generator=g) * 0.5).to(dev)
    h0 = torch.tanh(c0)

    def ref(rnd):
        w = rnd(whh.float()).double()
        h, c = h0.double(), c0.double()
        hs = [h]
        for t in range(T):
            a = gx[t].double() + rnd(h.float()).double() @ w.t()
            i, f, gg, o = a.chunk(4, -1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            h = torch.sigmoid(o) * torch.tanh(c)
            hs.append(h)
        return torch.stack(hs)
    hs_h = ref(lambda v: v.to(torch.float16).float())
    hs_exact = ref(lambda v: v)
    perm = torch.arange(4 * H).view(4, H).t().reshape(-1).to(dev)
    gxu = gx[:, :, perm].contiguous()
    errs = {}
    for fmt, pk, fl in (("f16", 2, flags | 32), ("bf16", 0, flags)):
        hs = torch.zeros(T + 1, B, H, device=dev)
        cs = torch.zeros(T + 1, B, H, device=dev)
        hs[0], cs[0] = h0, c0
        wpk = torch.full((lib.lv_lstm_persist16_wpk_floats(),), float("nan"), device=dev)
        xch = torch.zeros(lib.lv_lstm_persist16_xch_floats(), device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        lib.lv_lstm_persist16_pack(P(whh), P(wpk), pk, H, _s(dev))
        saved = torch.empty(lib.lv_lstm_persist16_saved_floats(T, R), device=dev)
        lib.lv_lstm_fwd_bf16_persist16(P(gxu), P(wpk), P(hs), P(cs), P(saved), P(xch), P(status), T, B, R, fl, H, _s(dev))
        assert int(status.item()) == 0
        if fmt == "f16":
            assert float((hs.double() - hs_h).abs().max()) < 2e-4
        errs[fmt] = float((hs.double() - hs_exact).pow(2).mean().sqrt())
    assert errs["f16"] < 0.35 * errs["bf16"], errs        # ~8x finer operand rounding (rms over all h_t; measured ~0.13)


def test_binary16_subnormal_weights_survive_the_matrix_pipe(lib, hip_device, T=3, B=32, R=4, flags=33):
    """at the reference init U(-0.01, 0.01) about 0.6 % of the W_hh / W_ih entries are below binary16's smallest
    normal number (6.1e-5) and reach the forward's v_mfma_f32_16x16x32_f16 as SUBNORMAL operands.  Here EVERY recurrent weight is
    a positive binary16 subnormal in [1e-7, 6e-5] and h is positive, so the recurrent product is O(1e-2) per gate if subnormal
    operands are honoured and exactly 0 if the packing conversion or the matrix pipe flushes them.  The kernel must match the
    float64 recurrence that KEEPS them (binary16-rounded, as torch's .to(float16) does) and be far from the flushed one."""
    dev, H = hip_device, 1024
    g = torch.Generator().manual_seed(77)
    lo, hi = math.log(1e-7), math.log(6e-5)
    whh = torch.exp(lo + (hi - lo) * torch.rand(4 * H, H, generator=g)).to(dev)
    assert float(whh.max()) < 6.1e-5
    gx = torch.zeros(T, B, 4 * H, device=dev)
    c0 = (0.5 + torch.rand(B, H, generator=g)).to(dev)
    h0 = torch.tanh(c0)

    def ref(w):
        h, c = h0.double(), c0.double()
        hs = [h]
        for t in range(T):
            a = h.float().to(torch.float16).double() @ w.t()
            i, f, gg, o = a.chunk(4, -1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
            h = torch.sigmoid(o) * torch.tanh(c)
            hs.append(h)
        return torch.stack(hs)
    w16 = whh.to(torch.float16)
    assert float((w16.float() - whh).abs().max()) <= 2.0 ** -25 + 1e-12      # subnormal spacing 2^-24: the image keeps them
    hs_keep = ref(w16.double())
    hs_flush = ref(torch.zeros_like(whh).double())
    signal = float((hs_keep - hs_flush).abs().max())
    assert signal > 1e-3                                                        # the two hypotheses are far apart
    perm = torch.arange(4 * H).view(4, H).t().reshape(-1).to(dev)
    gxu = gx[:, :, perm].contiguous()
    hs = torch.zeros(T + 1, B, H, device=dev)
    cs = torch.zeros(T + 1, B, H, device=dev)
    hs[0], cs[0] = h0, c0
    wpk = torch.full((lib.lv_lstm_persist16_wpk_floats(),), float("nan"), device=dev)
    xch = torch.zeros(lib.lv_lstm_persist16_xch_floats(), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    lib.lv_lstm_persist16_pack(P(whh), P(wpk), 2, H, _s(dev))
    saved = torch.empty(lib.lv_lstm_persist16_saved_floats(T, R), device=dev)
    lib.lv_lstm_fwd_bf16_persist16(P(gxu), P(wpk), P(hs), P(cs), P(saved), P(xch), P(status), T, B, R, flags, H, _s(dev))
    assert int(status.item()) == 0
    e_keep = float((hs.double() - hs_keep).abs().max())
    e_flush = float((hs.double() - hs_flush).abs().max())
    print("binary16 subnormal W_hh: |h - keep| %.3e, |h - flushed| %.3e (hypotheses %.3e apart)" % (e_keep, e_flush, signal))
    assert e_keep < 2e-5 and e_flush > 0.5 * signal, (e_keep, e_flush, signal)


@pytest.mark.parametrize("mode,R,C", [("plain", 70, 50), ("gates", 4 * 24, 40), ("gather", 5 * 7, 33)])
def test_cvt_h16(lib, hip_device, mode, R, C):
    """lv_cvt_h16_f32: dst = IEEE binary16 (RNE) in the plain / unit-major gate rows / gathered layouts, dstT = the transposed BF16
    image (forward operand on the binary16 pipe, gradient operand on the bf16 pipe, one launch)."""
    g = torch.Generator().manual_seed(R * 7 + C)
    dev = hip_device
    lds, ldd, ldt = C + 3, C + 8, R + 5
    if mode == "gather":
        T, B, V = 5, 7, 19
        src = torch.randn(V, C, generator=g); lds = C
        ids = torch.randint(0, V, (B, T + 2), generator=g)
        rows = torch.stack([src[ids[b, t]] for t in range(T) for b in range(B)])
    else:
        src = torch.randn(R, lds, generator=g)
        src[0, 0] = 1.00048828125          # a tie between two binary16 values: RNE picks the even significand (1.0)
        src[1, 1], src[2, 3] = 1.0e6, -3.0e5   # beyond binary16's range: the image saturates at +-65504 (never inf); the bf16 image keeps them
        src[3, 2] = float("nan")               # a NaN stays a NaN in both images (the clamp used to turn it into -65504)
        rows = src[:, :C]
    want_d = rows.clamp(-65504.0, 65504.0).to(torch.float16).view(torch.int16)
    if mode == "gates":
        H = R // 4
        want_d = want_d[torch.arange(4 * H).view(4, H).t().reshape(-1)]
    d = torch.full((R, ldd), 0x1234, dtype=torch.int16, device=dev)
    dT = torch.full((C, ldt), 0x1234, dtype=torch.int16, device=dev)
    sd = src.to(dev)
    if mode == "gather":
        lib.lv_cvt_h16_f32(P(sd), lds, R, C, 0, P(ids.to(dev)), T + 2, B, V, P(d), ldd, P(dT), ldt, _s(dev))
    else:
        lib.lv_cvt_h16_f32(P(sd), lds, R, C, R // 4 if mode == "gates" else 0, None, 0, 1, 0, P(d), ldd, P(dT), ldt, _s(dev))
    assert torch.equal(d.cpu()[:, :C], want_d)
    gotT, wantT = dT.cpu()[:, :R], _bf16_bits(rows).t()
    nan = torch.isnan(rows).t()
    assert torch.equal(gotT[~nan], wantT[~nan])
    if bool(nan.any()):     # a NaN stays a NaN in the bf16 image too (any payload): exponent all ones, significand non-zero
        b = gotT[nan].to(torch.int32) & 0xFFFF
        assert bool(((b & 0x7F80) == 0x7F80).all()) and bool(((b & 0x007F) != 0).all())
    assert bool((d.cpu()[:, C:] == 0x1234).all()) and bool((dT.cpu()[:, R:] == 0x1234).all())


@pytest.mark.parametrize("M,N,K,nsplit", [(64, 96, 200, 32), (4096, 1536, 6400, 512), (4096, 1024 + 512, 3200, 512), (130, 72, 1000, 20)])
def test_gemm_b16_dual(lib, hip_device, M, N, K, nsplit):
    """lv_gemm_b16_dual: one weight-gradient-form product (A stored [K][M]) whose columns [0, nsplit) land in C1 (its own leading
    dimension, here wider than nsplit like the decoder's dW_ih inside [4H][ni + nz]) and the rest in C2 -- against the two separate
    lv_gemm_b16 products of the same operands (f32 summation order differs: the pieces are cut differently), untouched padding, and
    the forced two-piece split of a shape that would not split by itself."""
    dev = hip_device
    g = torch.Generator().manual_seed(M + N + K)
    A = (torch.randn(K, M, generator=g) * 0.2).to(dev)           # [K][M]: transA = 1
    Bm = (torch.randn(N, K, generator=g) * 0.2).to(dev)          # [N][K]
    ldk = (K + 7) // 8 * 8
    A16 = torch.zeros(K, (M + 7) // 8 * 8, dtype=torch.int16, device=dev)
    B16 = torch.zeros(N, ldk, dtype=torch.int16, device=dev)
    lib.lv_cvt_bf16_f32(P(A), M, K, M, P(A16), A16.shape[1], None, 0, _s(dev))
    lib.lv_cvt_bf16_f32(P(Bm), K, N, K, P(B16), ldk, None, 0, _s(dev))
    ws = torch.empty(1 << 25, device=dev)
    if not lib.lv_gemm_b16_dual_supported(M, N, K, ws.numel()):
        pytest.skip("shape takes the 256-tile route")
    ld1, ld2 = nsplit + 12, N - nsplit
    C1 = torch.full((M, ld1), 7.0, device=dev)
    C2 = torch.full((M, ld2), 7.0, device=dev)
    lib.lv_gemm_b16_dual(1, M, N, K, P(A16), A16.shape[1], P(B16), ldk, P(C1), ld1, nsplit, P(C2), ld2, P(ws), ws.numel(), _s(dev))
    R1 = torch.empty(M, nsplit, device=dev)
    R2 = torch.empty(M, N - nsplit, device=dev)
    lib.lv_gemm_b16(1, M, nsplit, K, 1.0, P(A16), A16.shape[1], P(B16), ldk, P(R1), nsplit, 0, None, 0, 1, None, 0, 1, P(ws), ws.numel(), _s(dev))
    lib.lv_gemm_b16(1, M, N - nsplit, K, 1.0, P(A16), A16.shape[1], P(B16, nsplit * ldk), ldk, P(R2), N - nsplit, 0, None, 0, 1, None, 0, 1,
                    P(ws), ws.numel(), _s(dev))
    sc = float(torch.cat([R1, R2], 1).abs().max())
    assert float((C1[:, :nsplit] - R1).abs().max()) < 2e-5 * sc * max(1.0, (K / 1000) ** 0.5)
    assert float((C2 - R2).abs().max()) < 2e-5 * sc * max(1.0, (K / 1000) ** 0.5)
    assert bool((C1[:, nsplit:] == 7.0).all())
    ref = (A.to(torch.bfloat16).double().t() @ Bm.to(torch.bfloat16).double().t()).cpu()
    got = torch.cat([C1[:, :nsplit], C2], 1).cpu().double()
    assert float((got - ref).abs().max()) < 3e-5 * float(ref.abs().max()) * max(1.0, (K / 1000) ** 0.5)


def _b16_image(lib, dev, X, rows, cols):
    ld = (cols + 7) // 8 * 8
    img = torch.zeros(rows, ld, dtype=torch.int16, device=dev)
    lib.lv_cvt_bf16_f32(P(X), cols, rows, cols, P(img), ld, None, 0, _s(dev))
    return img, ld


PAIR_SHAPES = [
    # (transA0, M0, N0, K0, nsplit0, M1, N1, K1)
    (1, 4096, 1536, 6400, 512, 6400, 512, 4096),        # the Yahoo bench shape: [dW_ih | dW_hh] + dX of one LSTM layer
    (1, 4096, 1536, 3200, 512, 3200, 512, 4096),        # Yelp
    (1, 300, 520, 200, 264, 260, 100, 500),             # ragged everywhere, ragged K tiles, most workgroups idle
    (0, 700, 300, 1000, 0, 0, 0, 0),                    # one product, NT, stream-K over all 256 workgroups
    (1, 513, 257, 1111, 0, 0, 0, 0),                    # one product, TN
]


@pytest.mark.parametrize("tA0,M0,N0,K0,nsplit,M1,N1,K1", PAIR_SHAPES, ids=["PAIR%d" % i for i in range(len(PAIR_SHAPES))])
def test_gemm_b16_pair(lib, hip_device, tA0, M0, N0, K0, nsplit, M1, N1, K1):
    """lv_gemm_b16_pair: two independent products in one grouped stream-K launch (tiles shared between workgroups are summed inside
    the launch by the last arriver, in K order): both against the float64 product of the bf16-rounded operands, padding of every
    destination untouched, and -- the point of the in-launch hand-off -- a second and third launch over the same workspace
    (arrival counters back at zero, stale slabs in the caller's L1 / L2) bit-identical to the first."""
    dev = hip_device
    g = torch.Generator().manual_seed(M0 + N0 + K0 + M1)
    A0 = (torch.randn(K0, M0, generator=g) * 0.2) if tA0 else (torch.randn(M0, K0, generator=g) * 0.2)
    B0 = torch.randn(N0, K0, generator=g) * 0.2
    A0i, lda0 = _b16_image(lib, dev, A0.to(dev), *A0.shape)
    B0i, ldb0 = _b16_image(lib, dev, B0.to(dev), N0, K0)
    two = M1 > 0
    if two:
        A1 = torch.randn(M1, K1, generator=g) * 0.2
        B1 = torch.randn(N1, K1, generator=g) * 0.2
        A1i, lda1 = _b16_image(lib, dev, A1.to(dev), M1, K1)
        B1i, ldb1 = _b16_image(lib, dev, B1.to(dev), N1, K1)
    ws = torch.full((2 * 256 * 65536 + 64,), float("nan"), device=dev)
    n0a = nsplit if nsplit > 0 else N0
    ld0, ld0b, ld1 = n0a + 12, max(N0 - nsplit, 1) + 4, N1 + 8

    def run():
        C0 = torch.full((M0, ld0), 7.0, device=dev)
        C0b = torch.full((M0, ld0b), 7.0, device=dev)
        C1 = torch.full((max(M1, 1), ld1), 7.0, device=dev)
        lib.lv_gemm_b16_pair(tA0, M0, N0, K0, P(A0i), lda0, P(B0i), ldb0, P(C0), ld0, nsplit, P(C0b) if nsplit > 0 else None, ld0b,
                             0, M1, N1, K1, P(A1i) if two else None, lda1 if two else 0, P(B1i) if two else None, ldb1 if two else 0,
                             P(C1) if two else None, ld1, P(ws), ws.numel(), _s(dev))
        pend = torch.full((1,), -1, dtype=torch.int32, device=dev)
        lib.lv_gemm_b16_pair_pending(P(pend), _s(dev))
        assert int(pend.cpu()[0]) == 0          # every arrival counter is back at zero when the launch is over
        return C0.cpu(), C0b.cpu(), C1.cpu()

    C0, C0b, C1 = run()
    a0 = A0.to(torch.bfloat16).double()
    ref0 = (a0.t() if tA0 else a0) @ B0.to(torch.bfloat16).double().t()
    got0 = torch.cat([C0[:, :n0a], C0b[:, :N0 - nsplit]], 1).double() if nsplit > 0 else C0[:, :N0].double()
    assert float((got0 - ref0).abs().max()) < 3e-5 * float(ref0.abs().max()) * max(1.0, (K0 / 1000) ** 0.5)
    assert bool((C0[:, n0a:] == 7.0).all())
    if nsplit > 0:
        assert bool((C0b[:, N0 - nsplit:] == 7.0).all())
    else:
        assert bool((C0b == 7.0).all())
    if two:
        ref1 = A1.to(torch.bfloat16).double() @ B1.to(torch.bfloat16).double().t()
        assert float((C1[:, :N1].double() - ref1).abs().max()) < 3e-5 * float(ref1.abs().max()) * max(1.0, (K1 / 1000) ** 0.5)
        assert bool((C1[:, N1:] == 7.0).all())
    for _ in range(2):
        D0, D0b, D1 = run()
        assert torch.equal(D0, C0) and torch.equal(D0b, C0b) and torch.equal(D1, C1)


@pytest.mark.parametrize("M,N,K,acc", [(130, 140, 96, 0), (256, 128, 512, 0), (64, 64, 72, 1), (200, 4096, 544, 0), (6400, 512, 4096, 0)])
def test_gemm_h16(lib, hip_device, M, N, K, acc):
    """lv_gemm_h16: C = A . B^T (+ row-cyclic addend, accumulate) on binary16 operand images, f32 accumulation: against the
    float64 product of the binary16-rounded operands (f32 summation order is all that differs), incl. a ragged K tile, the
    decoder-sized K = 544 and a split-K shape."""
    dev = hip_device
    g = torch.Generator().manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g) * 0.3
    Bm = torch.randn(N, K, generator=g) * 0.1
    add = torch.randn(3, N, generator=g)
    C0 = torch.randn(M, N, generator=g)
    lda, ldb = (K + 7) // 8 * 8, (K + 7) // 8 * 8
    A16 = torch.zeros(M, lda, dtype=torch.int16, device=dev)
    B16 = torch.zeros(N, ldb, dtype=torch.int16, device=dev)
    lib.lv_cvt_h16_f32(P(A.to(dev)), K, M, K, 0, None, 0, 1, 0, P(A16), lda, None, 0, _s(dev))
    lib.lv_cvt_h16_f32(P(Bm.to(dev)), K, N, K, 0, None, 0, 1, 0, P(B16), ldb, None, 0, _s(dev))
    C = C0.clone().to(dev)
    ws = torch.empty(1 << 24, device=dev)
    addd = add.to(dev)
    lib.lv_gemm_h16(M, N, K, 1.0, P(A16), lda, P(B16), ldb, P(C), N, acc, P(addd), N, 3, None, 0, 1, P(ws), ws.numel(), _s(dev))
    ref = A.to(torch.float16).double() @ Bm.to(torch.float16).double().t() + add.double()[torch.arange(M) % 3]
    if acc:
        ref = ref + C0.double()
    assert float((C.cpu().double() - ref).abs().max()) < 2e-5 * float(ref.abs().max()) * max(1.0, (K / 512) ** 0.5)


@pytest.mark.parametrize("T,B,R,tanh_init,use_ext,use_last", [
    (6, 32, 4, True, True, False), (9, 32, 8, False, True, True), (5, 64, 8, True, True, False), (7, 128, 16, True, True, False),
    (40, 32, 8, True, True, False), (3, 13, 2, True, True, True), (4, 100, 13, False, True, True), (17, 8, 1, False, False, True),
    (12, 32, 16, True, True, False),
])
@pytest.mark.parametrize("flags", [0, 1])
def test_lstm_bwd_persistent16(lib, hip_device, T, B, R, tanh_init, use_ext, use_last, flags):
    """The one-launch persistent BPTT (lv_lstm_persist16.hip: reduce-scatter hand-off, R batch rows per XCD group) on the saved
    activations of the step kernels' forward: against the two-launch-per-step kernels on the same inputs at the T = 200 test's
    bounds (rms 1e-3; a flipped bf16 rounding of one dG element is 2^-8 of that element), and against the float64 autograd of the
    exact recurrence at the bf16 noise floor (the operands of dh = dG . W_hh are rounded to bf16: ~2^-9 relative per product)."""
    dev, H = hip_device, 1024
    g = torch.Generator().manual_seed(T * 100 + B + 7)
    gx = (torch.randn(T, B, 4 * H, generator=g) * 0.5).to(dev)
    whh = (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(dev)
    c0 = (torch.randn(B, H, generator=g) * 0.5).to(dev)
    wext = torch.randn(T, B, H, generator=g).to(dev)
    wlast = torch.randn(B, H, generator=g).to(dev)
    gx64 = gx.double().requires_grad_(True)
    c064 = c0.double().requires_grad_(True)
    h064 = torch.tanh(c064) if tanh_init else torch.zeros_like(c064)
    hs_r, cs_r, out_r = _lstm_ref(gx64, whh.double(), h064, c064, None, 1.0)
    loss = 0
    if use_ext:
        loss = loss + (out_r * wext.double()).sum()
    if use_last:
        loss = loss + (hs_r[-1] * wlast.double()).sum()
    loss.backward()
    hs = torch.zeros(T + 1, B, H, device=dev)
    cs = torch.zeros(T + 1, B, H, device=dev)
    hs[0], cs[0] = h064.detach().float(), c0
    gates = torch.empty(T, B, 4 * H, device=dev)
    hdrop = torch.empty(T, B, H, device=dev)
    ws = torch.empty(lib.lv_lstm_ws_floats(B, H), device=dev)
    lib.lv_lstm_fwd_bf16(P(gx), P(whh), P(hs), P(cs), P(gates), None, 1.0, P(hdrop), P(ws), T, B, H, _s(dev))
    wpk = torch.full((lib.lv_lstm_persist16_wpk_floats(),), float("nan"), device=dev)
    lib.lv_lstm_persist16_pack(P(whh), P(wpk), 1, H, _s(dev))
    outs = []
    for persistent in (True, False):
        dG = torch.empty(T, B, 4 * H, device=dev)
        dG16 = torch.full((T, B, 4 * H), 0x7FC0, dtype=torch.int16, device=dev)
        dGsum = torch.full((B, 4 * H), 7.0, device=dev)
        dh0 = torch.empty(B, H, device=dev)
        dc0 = torch.empty(B, H, device=dev)
        if persistent:
            wsp = torch.full((lib.lv_lstm_persist16_xch_floats(),), float("nan"), device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            saved = _saved16_pack(lib, gates.view(T, B, 4 * H), cs, R)
            cs0 = torch.full_like(cs, float("nan")); cs0[0] = cs[0]          # the kernel may read the initial state only
            lib.lv_lstm_bwd_bf16_persist16(P(wext) if use_ext else None, P(wlast) if use_last else None, P(wpk), P(saved), P(hs), P(cs0),
                                           P(dG16), P(dGsum), P(wsp), P(status), P(dh0), P(dc0), int(tanh_init), T, B,
                                           R, flags, H, _s(dev))
            assert int(status.item()) == 0, "hand-off timeout, status %d" % int(status.item())
            dG = dG16.view(torch.bfloat16).float()                           # image-only kernel: compare through the bf16 image
        else:
            ws.fill_(float("nan"))
            lib.lv_lstm_bwd_bf16_img(P(wext) if use_ext else None, P(wlast) if use_last else None, None, 1.0, P(whh), P(gates), P(hs),
                                     P(cs), P(dG), P(dG16), P(dGsum), P(ws), P(dh0), P(dc0), int(tanh_init), T, B, H, _s(dev))
            assert torch.equal(dG16.cpu(), dG.cpu().to(torch.bfloat16).view(torch.int16))
        sc, noise = float(gx64.grad.abs().max()), 3e-2                       # bf16 noise floor against the exact recurrence
        assert float((dG.double() - gx64.grad).abs().max()) < noise * sc
        assert float((dGsum.double() - gx64.grad.sum(0)).abs().max()) < noise * sc * T
        assert float((dc0.double() - c064.grad).abs().max()) < noise * float(c064.grad.abs().max())
        if not tanh_init:
            ref_dh0 = gx64.grad[0] @ whh.double()
            assert float((dh0.double() - ref_dh0).abs().max()) < noise * float(ref_dh0.abs().max())
        outs.append((dG16.view(torch.bfloat16).float(), dGsum.clone(), dc0.clone()))
    for a, b, what in zip(outs[0], outs[1], ("dG", "dGsum", "dc0")):
        sc = float(b.abs().max())
        err = float((a - b).abs().max())
        rms = float((a - b).pow(2).mean().sqrt()) / float(b.pow(2).mean().sqrt())
        assert rms < 1e-3 and err < (2 ** -7 if what == "dG" else 1e-3) * sc, (what, err / sc, rms)


@pytest.mark.parametrize("T,seq", [(6, [(32, 4), (128, 16), (32, 4), (13, 2), (64, 8), (32, 4)])])
def test_persistent_exchange_halves_alternate_without_memsets(lib, hip_device, T, seq, local=1, repeat_fwd=3):
    """flags bit 1 of the persistent launches: the exchange buffer's halves alternate per kind of launch and every launch zeroes the
    other half of its kind in its prologue (engine._xch_flags keeps the state) -- no memset launch.  A run of forward + BPTT launches
    whose batch size (hence instantiation and polled extent) changes from launch to launch, all on ONE buffer, must give bit for bit
    what each launch gives on a freshly zeroed buffer in the memset form: a stale tag anywhere would be read as data."""
    from types import SimpleNamespace
    from vae_lagging_encoder_amd.engine import _xch_flags
    dev, H = hip_device, 1024
    g = torch.Generator().manual_seed(77)
    whh = (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(dev)
    wf = torch.empty(lib.lv_lstm_persist16_wpk_floats(), device=dev)
    wb = torch.empty(lib.lv_lstm_persist16_wpk_floats(), device=dev)
    lib.lv_lstm_persist16_pack2(P(whh), P(wf), P(wb), H, _s(dev))
    shared = torch.zeros(lib.lv_lstm_persist16_xch_floats(), device=dev)
    wi = SimpleNamespace(xstate={"f": 0, "g": 0, "gcls": [0, 0]})

    def run(B, R, xch, ff, fb, seed):
        gg = torch.Generator().manual_seed(seed)
        gx = (torch.randn(T, B, 4 * H, generator=gg) * 0.5).to(dev)
        dO = torch.randn(T, B, H, generator=gg).to(dev)
        hs = torch.zeros(T + 1, B, H, device=dev)
        cs = torch.zeros(T + 1, B, H, device=dev)
        cs[0] = (torch.randn(B, H, generator=gg) * 0.5).to(dev)
        saved = torch.empty(lib.lv_lstm_persist16_saved_floats(T, R), device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        lib.lv_lstm_fwd_bf16_persist16(P(gx), P(wf), P(hs), P(cs), P(saved), P(xch), P(status), T, B, R, ff, H, _s(dev))
        dG16 = torch.zeros(T, B, 4 * H, dtype=torch.int16, device=dev)
        dGsum = torch.empty(B, 4 * H, device=dev)
        dc0 = torch.empty(B, H, device=dev)
        lib.lv_lstm_bwd_bf16_persist16(P(dO), None, P(wb), P(saved), P(hs), P(cs), P(dG16), P(dGsum), P(xch), P(status), None, P(dc0), 0,
                                       T, B, R, fb, H, _s(dev))
        assert int(status.item()) == 0, int(status.item())
        return hs.cpu(), dG16.cpu(), dGsum.cpu(), dc0.cpu()
    for i, (B, R) in enumerate(seq):
        fresh = torch.zeros(lib.lv_lstm_persist16_xch_floats(), device=dev)
        want = run(B, R, fresh, local, local, 100 + i)                  # memset form, half 0 of a clean buffer
        ff = local | _xch_flags(wi, "f", R, "cpu")
        fb = local | _xch_flags(wi, "g", R, "cpu")
        assert (ff & 2) and (fb & 2)
        got = run(B, R, shared, ff, fb, 100 + i)
        for a, b, what in zip(got, want, ("hs", "dG16", "dGsum", "dc0")):
            assert torch.equal(a, b), (i, B, R, what)
    # a second forward in a row (the encoder's two-pass exact forward, evaluation passes) keeps alternating
    for i in range(repeat_fwd):
        ff = local | _xch_flags(wi, "f", 4, "cpu")
        gg = torch.Generator().manual_seed(5)
        gx = (torch.randn(T, 32, 4 * H, generator=gg) * 0.5).to(dev)
        hs = torch.zeros(T + 1, 32, H, device=dev); cs = torch.zeros(T + 1, 32, H, device=dev)
        saved = torch.empty(lib.lv_lstm_persist16_saved_floats(T, 4), device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        lib.lv_lstm_fwd_bf16_persist16(P(gx), P(wf), P(hs), P(cs), P(saved), P(shared), P(status), T, 32, 4, ff, H, _s(dev))
        assert int(status.item()) == 0
        if i == 0:
            first = hs.cpu()
        assert torch.equal(hs.cpu(), first)


@pytest.mark.parametrize("kernels", ["B32_R4", "B64_R8", "B128_R16", "B100_R13", "B13_R2"])
def test_lstm_persistent_recurrences_at_headline_length(lib, hip_device, kernels):
    """Both persistent recurrences (lv_lstm_persist16.hip, hand-off in the XCD's L2) at the length the metric is quoted on
    (T = 200, B = 32, H = 1024; the 8- and 16-row instantiations at their own batch sizes and T = 120) against the
    launch-per-step bf16 kernels on the SAME inputs: the two realisations see the same bf16-rounded operands and differ only
    in f32 summation order (and in what a flipped bf16 rounding moves downstream), so they must stay within 1e-3 of each other
    over all 200 steps -- a per-kernel check that localises a regression the end-to-end Yahoo fixture test would only see as a
    loss delta.  Weights at 3x the reference's init scale (U(-0.03, 0.03): a contractive recurrence, like the fixtures)."""
    dev, H = hip_device, 1024
    B, R16 = int(kernels.split("_")[0][1:]), int(kernels.split("_")[1][1:])
    T = 200 if kernels == "B32_R4" else 120
    g = torch.Generator().manual_seed(20001)
    gx = (torch.randn(T, B, 4 * H, generator=g) * 0.5).to(dev)
    whh = ((torch.rand(4 * H, H, generator=g) * 2 - 1) * 0.03).to(dev)
    c0 = (torch.randn(B, H, generator=g) * 0.5).to(dev)
    h0 = torch.tanh(c0)
    wext = (torch.randn(T, B, H, generator=g) * 0.1).to(dev)
    perm = torch.arange(4 * H).view(4, H).t().reshape(-1).to(dev)
    gxu = gx[:, :, perm].contiguous()
    fw = {}
    for persistent in (True, False):
        hs = torch.zeros(T + 1, B, H, device=dev)
        cs = torch.zeros(T + 1, B, H, device=dev)
        hs[0], cs[0] = h0, c0
        gates = torch.empty(T, B, 4 * H, device=dev)
        if persistent:
            wpk = torch.empty(lib.lv_lstm_persist16_wpk_floats(), device=dev)
            xch = torch.empty(lib.lv_lstm_persist16_xch_floats(), device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            saved = torch.empty(lib.lv_lstm_persist16_saved_floats(T, R16), device=dev)
            lib.lv_lstm_persist16_pack(P(whh), P(wpk), 0, H, _s(dev))
            lib.lv_lstm_fwd_bf16_persist16(P(gxu), P(wpk), P(hs), P(cs), P(saved), P(xch), P(status), T, B, R16, 1, H, _s(dev))
            assert int(status.item()) == 0
            gates, c_t = _saved16_unpack(saved, T, B, R16)
            cs[1:] = c_t
        else:
            ws = torch.empty(lib.lv_lstm_ws_floats(B, H), device=dev)
            lib.lv_lstm_fwd_bf16_ug(P(gxu), P(whh), P(hs), P(cs), P(gates), None, 1.0, None, P(ws), T, B, H, _s(dev))
        fw[persistent] = (hs, cs, gates.view(T, B, 4 * H))
    for a, b, what in zip(fw[True], fw[False], ("h", "c", "gates")):
        err = float((a - b).abs().max())
        assert err < 1e-3, (what, err)
    # BPTT on the step kernels' saved activations
    hs, cs, gates = fw[False]
    outs = {}
    for persistent in (True, False):
        dG16 = torch.zeros(T, B, 4 * H, dtype=torch.int16, device=dev)
        dGsum = torch.empty(B, 4 * H, device=dev)
        dc0 = torch.empty(B, H, device=dev)
        if persistent:
            wpk = torch.empty(lib.lv_lstm_persist16_wpk_floats(), device=dev)
            xch = torch.empty(lib.lv_lstm_persist16_xch_floats(), device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            lib.lv_lstm_persist16_pack(P(whh), P(wpk), 1, H, _s(dev))
            lib.lv_lstm_bwd_bf16_persist16(P(wext), None, P(wpk), P(_saved16_pack(lib, gates.view(T, B, 4 * H), cs, R16)), P(hs), P(cs), P(dG16),
                                           P(dGsum), P(xch), P(status), None, P(dc0), 1, T, B, R16, 1, H, _s(dev))
            assert int(status.item()) == 0
        else:
            ws = torch.empty(lib.lv_lstm_ws_floats(B, H), device=dev)
            lib.lv_lstm_bwd_bf16_img(P(wext), None, None, 1.0, P(whh), P(gates), P(hs), P(cs), None, P(dG16), P(dGsum), P(ws), None,
                                     P(dc0), 1, T, B, H, _s(dev))
        outs[persistent] = (dG16.view(torch.bfloat16).float(), dGsum, dc0)
    for a, b, what in zip(outs[True], outs[False], ("dG", "dGsum", "dc0")):
        sc = float(b.abs().max())
        err = float((a - b).abs().max())
        rms = float((a - b).pow(2).mean().sqrt()) / float(b.pow(2).mean().sqrt())
        # dG is compared through its bf16 image: one flipped rounding of an element is 2^-8 of THAT element
        assert rms < 1e-3 and err < (2 ** -7 if what == "dG" else 1e-3) * sc, (what, err / sc, rms)


def test_lstm_persistent16_unsupported_shapes(lib, hip_device):
    if hip_device.type != "cuda":
        pytest.skip("GPU only")
    z = torch.zeros(1 << 16, device=hip_device)
    st = torch.zeros(1, dtype=torch.int32, device=hip_device)
    with pytest.raises(_lib.LvaeError):      # H != 1024
        lib.lv_lstm_fwd_bf16_persist16(P(z), P(z), P(z), P(z), P(z), P(z), P(st), 1, 4, 1, 0, 64, _s(hip_device))
    with pytest.raises(_lib.LvaeError):      # more than 16 rows per group
        lib.lv_lstm_fwd_bf16_persist16(P(z), P(z), P(z), P(z), P(z), P(z), P(st), 1, 136, 17, 0, 1024, _s(hip_device))


@pytest.mark.parametrize("T,B,ni,V,masked", [(7, 4, 8, 53, True), (199, 32, 512, 20001, True), (12, 16, 50, 1004, False),
                                              (200, 128, 64, 300, True), (50, 32, 512, 40, True), (9, 8, 512, 3, False),
                                              (40, 8, 512, 3, True), (130, 16, 512, 7, False)])      # long runs: the 8-group kernel
def test_embed_gather_sort_scatter(lib, hip_device, T, B, ni, V, masked):
    dev = hip_device
    g = torch.Generator().manual_seed(T + B + ni)
    emb = torch.randn(V, ni, generator=g).to(dev)
    ids = torch.randint(0, V, (B, T + 1), generator=g).to(dev)
    ids[0, 0] = V - 1
    mask = (torch.rand(B, T, ni, generator=g) < 0.5).to(torch.uint8).to(dev)
    X = torch.empty(T * B, ni, device=dev)
    lib.lv_embed_gather_f32(P(emb), P(ids), T + 1, P(mask) if masked else None, 2.0, P(X), T, B, ni, V, _s(dev))
    ref = emb[ids[:, :T]]                                  # (B,T,ni)
    if masked:
        ref = ref * mask.float() * 2.0
    ref = ref.transpose(0, 1).reshape(T * B, ni)
    assert torch.equal(X, ref)
    rows = torch.empty(T * B, dtype=torch.int32, device=dev)
    toks = torch.empty(T * B, dtype=torch.int32, device=dev)
    tmp = torch.empty(2 * T * B, dtype=torch.int32, device=dev)
    lib.lv_token_sort(P(ids), T + 1, T, B, V, P(rows), P(toks), P(tmp), _s(dev))
    flat_tok = ids[:, :T].t().reshape(-1)                  # row r = t*B + b
    st, si = torch.sort(flat_tok, stable=True)
    assert torch.equal(toks.long(), st)
    assert torch.equal(rows.long(), si)
    dX = torch.randn(T * B, ni, generator=g).to(dev)
    dE = torch.zeros(V, ni, device=dev)
    lib.lv_embed_scatter_f32(P(dX), P(mask) if masked else None, 2.0, P(rows), P(toks), T, B, P(dE), ni, V - 1, 0, _s(dev))
    src = dX.double()
    if masked:
        src = src * (mask.double() * 2.0).transpose(0, 1).reshape(T * B, ni)
    refE = torch.zeros(V, ni, dtype=torch.float64, device=dev).index_add_(0, flat_tok, src)
    refE[V - 1] = 0
    assert float((dE.double() - refE).abs().max()) < 1e-4
    assert float(dE[V - 1].abs().max()) == 0.0
    dE2 = torch.zeros(V, ni, device=dev)
    lib.lv_embed_scatter_f32(P(dX), P(mask) if masked else None, 2.0, P(rows), P(toks), T, B, P(dE2), ni, V - 1, 0, _s(dev))
    assert torch.equal(dE, dE2)                            # deterministic (sorted segments, no atomics)
    # the complete form: the same sums, and every other row (and the padding row) zeroed by the same launch
    dE3 = torch.full((V, ni), float("nan"), device=dev)
    lib.lv_embed_scatter_full_f32(P(dX), P(mask) if masked else None, 2.0, P(rows), P(toks), T, B, P(dE3), ni, V, V - 1, _s(dev))
    assert torch.equal(dE3, dE)
    dE4 = torch.full((V, ni), float("nan"), device=dev)
    lib.lv_embed_scatter_full_f32(P(dX), P(mask) if masked else None, 2.0, P(rows), P(toks), T, B, P(dE4), ni, V, -1, _s(dev))
    assert torch.equal(dE4[:V - 1], dE[:V - 1]) and float(dE4[V - 1].abs().max()) > 0.0      # no padding row: token V - 1 counts
    # ... and with the table gradient's sum of squares emitted by the same pass (norm folding): the same table, partials that add
    # up to its squared norm, every slot written; sq_only leaves the table alone and reports the same partials
    n = lib.lv_embed_scatter_sumsq_parts(T, B)
    sq = torch.full((n,), float("nan"), device=dev)
    dE5 = torch.full((V, ni), float("nan"), device=dev)
    lib.lv_embed_scatter_full_sumsq_f32(P(dX), P(mask) if masked else None, 2.0, P(rows), P(toks), T, B, P(dE5), ni, V, V - 1, P(sq), 0, _s(dev))
    assert torch.equal(dE5, dE)
    want = float(dE.double().pow(2).sum())
    assert abs(float(sq.double().sum()) - want) <= 1e-5 * want
    sq2 = torch.full((n,), float("nan"), device=dev)
    dE6 = torch.full((V, ni), 7.0, device=dev)
    lib.lv_embed_scatter_full_sumsq_f32(P(dX), P(mask) if masked else None, 2.0, P(rows), P(toks), T, B, P(dE6), ni, V, V - 1, P(sq2), 1, _s(dev))
    assert torch.equal(sq2, sq) and float((dE6 - 7.0).abs().max()) == 0.0


@pytest.mark.parametrize("B,ns,nz", [(32, 1, 32), (16, 1, 1), (5, 3, 40), (128, 2, 7)])
def test_reparam_kl(lib, hip_device, B, ns, nz):
    dev = hip_device
    g = torch.Generator().manual_seed(B + nz)
    mulv = torch.randn(B, 2 * nz, generator=g).to(dev)
    eps = torch.randn(B, ns, nz, generator=g).to(dev)
    z = torch.empty(B, ns, nz, device=dev)
    kl = torch.empty(B, device=dev)
    lib.lv_reparam_kl_fwd_f32(P(mulv), P(eps), P(z), P(kl), B, ns, nz, _s(dev))
    m64 = mulv.double().requires_grad_(True)
    mu, lv = m64[:, :nz], m64[:, nz:]
    z_r = mu.unsqueeze(1) + eps.double() * (0.5 * lv).exp().unsqueeze(1)
    kl_r = 0.5 * (mu.pow(2) + lv.exp() - lv - 1).sum(1)
    assert float((z.double() - z_r.detach()).abs().max()) < 1e-5
    assert float((kl.double() - kl_r.detach()).abs().max()) < 1e-5 * (1 + float(kl_r.detach().abs().max()))
    dz = torch.randn(B, ns, nz, generator=g).to(dev)
    dkl = torch.randn(B, generator=g).to(dev)
    ((z_r * dz.double()).sum() + (kl_r * dkl.double()).sum()).backward()
    dm = torch.empty(B, 2 * nz, device=dev)
    lib.lv_reparam_kl_bwd_f32(P(mulv), P(eps), P(dz), P(dkl), P(dm), B, ns, nz, _s(dev))
    assert float((dm.double() - m64.grad).abs().max()) < 1e-5 * (1 + float(m64.grad.abs().max()))


@pytest.mark.parametrize("T,B,V", [(6, 4, 53), (20, 32, 20001), (3, 7, 1004)])
def test_softmax_nll(lib, hip_device, T, B, V):
    dev = hip_device
    g = torch.Generator().manual_seed(V)
    ldl = (V + 31) // 32 * 32
    logits = torch.zeros(T * B, ldl)
    logits[:, :V] = torch.randn(T * B, V, generator=g) * 3
    logits = logits.to(dev)
    ids = torch.randint(0, V, (B, T + 1), generator=g).to(dev)
    lse = torch.empty(T * B, device=dev)
    nll = torch.empty(T * B, device=dev)
    lib.lv_softmax_nll_fwd_f32(P(logits), ldl, P(ids), T + 1, 1, P(lse), P(nll), T, B, V, _s(dev))
    l64 = logits[:, :V].double()
    tgt = ids[:, 1:].t().reshape(-1)
    nll_r = torch.nn.functional.cross_entropy(l64, tgt, reduction="none")
    assert float((nll.double() - nll_r).abs().max()) < 1e-5 * float(nll_r.abs().max())
    rs = torch.rand(B, generator=g).to(dev)
    p = torch.softmax(l64, -1)
    p[torch.arange(T * B), tgt] -= 1
    ref = p * rs.double()[torch.arange(T * B, device=dev) % B].unsqueeze(1)
    # bf16 image of the same gradient: must equal the RNE rounding of the f32 kernel's output, padding zeroed
    ld16 = ldl + 8
    d16 = torch.full((T * B, ld16), 0x7FC0, dtype=torch.int16, device=dev)
    keep = logits.clone()
    lib.lv_softmax_nll_bwd_b16(P(logits), ldl, P(lse), P(ids), T + 1, 1, P(rs), P(d16), ld16, T, B, V, _s(dev))
    assert torch.equal(logits, keep)
    lib.lv_softmax_nll_bwd_f32(P(logits), ldl, P(lse), P(ids), T + 1, 1, P(rs), T, B, V, _s(dev))
    assert float((logits[:, :V].double() - ref).abs().max()) < 2e-6
    assert torch.equal(d16[:, :V].cpu(), logits[:, :V].cpu().to(torch.bfloat16).view(torch.int16))
    assert bool((d16[:, V:] == 0).all())
    kl2 = torch.full((B,), 2.0, device=dev)
    w = torch.tensor([0.25], device=dev)
    loss = torch.empty(B, device=dev)
    rec = torch.empty(B, device=dev)
    lib.lv_vae_loss_f32(P(nll), P(kl2), P(w), P(loss), P(rec), T, B, _s(dev))
    rec_r = nll_r.view(T, B).sum(0)
    assert float((rec.double() - rec_r).abs().max()) < 1e-5 * float(rec_r.abs().max())
    assert float((loss.double() - (rec_r + 0.5)).abs().max()) < 1e-5 * float(rec_r.abs().max())


@pytest.mark.parametrize("n", [1, 1000, 8193, 16_600_000])
def test_norm_clip_sgd(lib, hip_device, n):
    dev = hip_device
    g = torch.Generator().manual_seed(n)
    gr = torch.randn(n, generator=g).to(dev)
    p = torch.randn(n, generator=g).to(dev)
    ws = torch.empty(lib.lv_sumsq_workspace_floats(), device=dev)
    sc = torch.zeros(4, device=dev)   # sumsq, coef, norm, lr
    sc[3] = 0.5
    lib.lv_sumsq_f32(P(gr), n, P(ws), P(sc, 0), 0, _s(dev))
    lib.lv_sumsq_f32(P(gr), n, P(ws), P(sc, 0), 1, _s(dev))
    ref = 2 * float(gr.double().pow(2).sum())
    assert abs(float(sc[0]) - ref) / ref < 1e-6
    lib.lv_clip_coef_f32(P(sc, 0), 5.0, P(sc, 1), P(sc, 2), _s(dev))
    nrm = ref ** 0.5
    coef = min(1.0, 5.0 / (nrm + 1e-6))
    assert abs(float(sc[1]) - coef) < 1e-6 and abs(float(sc[2]) - nrm) / nrm < 1e-6
    p_ref = p - 0.5 * (gr * float(sc[1]))
    lib.lv_sgd_step_f32(P(p), P(gr), n, P(sc, 3), P(sc, 1), 1, _s(dev))
    assert float((p - p_ref).abs().max()) < 1e-6


def test_adam_matches_torch(lib, hip_device):
    dev = hip_device
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(5000, generator=g)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([ref], lr=1e-3)
    p = p0.clone().to(dev)
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    sc = torch.tensor([1e-3, 0.0], device=dev)   # lr, step
    for it in range(3):
        gr = torch.randn(5000, generator=g)
        ref.grad = gr.clone()
        opt.step()
        gd = gr.to(dev)
        lib.lv_add_scalar_f32(P(sc, 1), 1.0, _s(dev))
        lib.lv_adam_step_f32(P(p), P(gd), P(m), P(v), 5000, P(sc, 0), None, P(sc, 1), 0.9, 0.999, 1e-8, 0, _s(dev))
    assert float((p.cpu() - ref.detach()).abs().max()) < 1e-6


def test_philox_draws(lib, hip_device):
    dev = hip_device
    st = torch.tensor([783435, 0], dtype=torch.int64, device=dev)
    n = 1 << 20
    a = torch.empty(n, device=dev)
    lib.lv_rng_normal_f32(P(a), n, P(st), 0, _s(dev))
    assert abs(float(a.mean())) < 5e-3 and abs(float(a.std()) - 1) < 5e-3
    m = torch.empty(n, dtype=torch.uint8, device=dev)
    lib.lv_rng_keepmask_u8(P(m), n, 0.5, P(st), 1, _s(dev))
    assert abs(float(m.float().mean()) - 0.5) < 3e-3 and int(m.max()) == 1
    b = torch.empty(n, device=dev)
    lib.lv_rng_normal_f32(P(b), n, P(st), 0, _s(dev))
    assert torch.equal(a, b)                                 # counter-based: same state -> same draw
    lib.lv_rng_advance(P(st), 1, _s(dev))
    lib.lv_rng_normal_f32(P(b), n, P(st), 0, _s(dev))
    assert not torch.equal(a, b)
    assert abs(float((a * b).mean())) < 5e-3                 # successive draws uncorrelated


# ---- Omniglot path kernels -----------------------------------------------------------------------------------------
def _nhwc(x):   # (N,C,H,W) -> [N*H*W, C]
    N, C, H, W = x.shape
    return x.permute(0, 2, 3, 1).reshape(N * H * W, C).contiguous()


def _nchw(t, N, H, W):
    return t.reshape(N, H, W, -1).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("N,Cin,Cout,H,k,stride,pad,masked", [
    (2, 5, 8, 9, 7, 1, 3, "A"), (2, 8, 8, 9, 7, 1, 3, "B"), (2, 8, 8, 9, 5, 1, 2, "B"), (3, 4, 6, 7, 3, 2, 1, None),
    (2, 1, 8, 28, 3, 2, 1, None), (2, 8, 16, 4, 4, 1, 0, None), (3, 4, 6, 7, 1, 2, 0, None), (2, 8, 4, 6, 3, 1, 1, "B"),
])
def test_conv_im2col_gemm_fwd_bwd(lib, hip_device, N, Cin, Cout, H, k, stride, pad, masked):
    """conv = lv_im2col_f32 + lv_gemm_f32 (+ tap-prefix skipping for type-B masks); backward = GEMMs + lv_col2im_f32,
    against F.conv2d autograd in float64."""
    import torch.nn.functional as F
    dev = hip_device
    g = torch.Generator().manual_seed(N * 100 + Cin * 10 + k)
    W = H
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) * 0.3
    mask = torch.ones_like(w)
    nt = k * k
    if masked:
        mc = 1 if masked == "A" else Cin
        mask[:, :mc, k // 2, k // 2 + (masked == "B"):] = 0
        mask[:, :mc, k // 2 + 1:] = 0
        if masked == "B":
            nt = (k // 2) * k + k // 2 + 1
    wm = w * mask
    x64 = x.double().requires_grad_(True)
    w64 = wm.double().requires_grad_(True)
    y_ref = F.conv2d(x64, w64, stride=stride, padding=pad)
    dy = torch.randn(y_ref.shape, generator=g)
    (y_ref * dy.double()).sum().backward()
    Ho, Wo = y_ref.shape[2], y_ref.shape[3]
    Pout, KK = N * Ho * Wo, k * k
    xd = _nhwc(x).to(dev)
    wd = wm.contiguous().to(dev)
    col = torch.empty(Pout, KK * Cin, device=dev)
    lib.lv_im2col_f32(P(xd), P(col), KK * Cin, N, H, W, Cin, Ho, Wo, k, k, pad, stride, KK, _s(dev))
    wg = torch.empty(Cout, KK * Cin, device=dev)
    lib.lv_conv_pack_w_f32(P(wd), P(wg), Cout, Cin, KK, _s(dev))
    y = torch.empty(Pout, Cout, device=dev)
    ws = torch.empty(1 << 20, device=dev)
    K = nt * Cin
    lib.lv_gemm_f32(0, 1, Pout, Cout, K, 1.0, P(col), KK * Cin, P(wg), KK * Cin, P(y), Cout, 0, None, 0, 1, None, 0, 1,
                    P(ws), ws.numel(), _s(dev))
    assert float((_nchw(y.cpu(), N, Ho, Wo).double() - y_ref.detach()).abs().max()) < 1e-4
    dyd = _nhwc(dy).to(dev)
    dwg = torch.empty(Cout, KK * Cin, device=dev)
    lib.lv_gemm_f32(1, 0, Cout, KK * Cin, Pout, 1.0, P(dyd), Cout, P(col), KK * Cin, P(dwg), KK * Cin, 0, None, 0, 1, None, 0, 1,
                    P(ws), ws.numel(), _s(dev))
    dw = torch.empty(Cout, Cin, k, k, device=dev)
    lib.lv_conv_unpack_dw_f32(P(dwg), P(dw), Cout, Cin, KK, 0, _s(dev))
    assert float((dw.cpu().double() - w64.grad).abs().max()) < 1e-3      # ALL taps, masked ones included (G5)
    dcol = torch.empty(Pout, K, device=dev)
    lib.lv_gemm_f32(0, 0, Pout, K, Cout, 1.0, P(dyd), Cout, P(wg), KK * Cin, P(dcol), K, 0, None, 0, 1, None, 0, 1,
                    P(ws), ws.numel(), _s(dev))
    dx = torch.empty(N * H * W, Cin, device=dev)
    lib.lv_col2im_f32(P(dcol), K, P(dx), N, H, W, Cin, Ho, Wo, k, k, pad, stride, nt, 0, _s(dev))
    assert float((_nchw(dx.cpu(), N, H, W).double() - x64.grad).abs().max()) < 1e-3


@pytest.mark.parametrize("N,C,H,act,use_res", [(4, 64, 7, True, True), (3, 33, 5, True, False), (2, 16, 28, False, True), (50, 32, 28, True, True),
                                                (1, 1, 3, False, False)])
def test_batchnorm_eval(lib, hip_device, N, C, H, act, use_res):
    """nn.BatchNorm2d in eval mode (+ residual) (+ ELU): the running statistics are applied and left untouched."""
    import torch.nn.functional as F
    dev = hip_device
    g = torch.Generator().manual_seed(C * 3 + H)
    x = torch.randn(N, C, H, H, generator=g) * 2 + 0.5
    res = torch.randn(N, C, H, H, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    y_ref = F.batch_norm(x.double(), rm.double(), rv.double(), gamma.double(), beta.double(), False, 0.1, 1e-5)
    if use_res:
        y_ref = y_ref + res.double()
    if act:
        y_ref = F.elu(y_ref)
    Pn = N * H * H
    xd, resd = _nhwc(x).to(dev), _nhwc(res).to(dev)
    rmd, rvd, gd, bd = rm.clone().to(dev), rv.clone().to(dev), gamma.to(dev), beta.to(dev)     # (named: P() of a temporary dangles)
    y = torch.full((Pn, C), float("nan"), device=dev)
    mean, invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    lib.lv_bn_eval_f32(P(xd), P(gd), P(bd), P(rmd), P(rvd), 1e-5, P(resd) if use_res else None, int(act), P(y),
                       P(mean), P(invstd), Pn, C, _s(dev))
    assert float((_nchw(y.cpu(), N, H, H).double() - y_ref).abs().max()) < 2e-5
    assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv) and torch.equal(mean.cpu(), rm)
    assert float((invstd.cpu().double() - (rv.double() + 1e-5).rsqrt()).abs().max()) < 1e-6


@pytest.mark.parametrize("N,C,H,act,use_res", [(3, 8, 5, True, True), (4, 32, 7, True, False), (2, 64, 6, False, False),
                                                (5, 512, 1, True, False), (2, 300, 3, True, True), (3, 16, 9, True, True),
                                                (7, 256, 4, True, True), (50, 32, 28, True, True), (6, 128, 2, False, False)])
def test_batchnorm_train_fwd_bwd(lib, hip_device, N, C, H, act, use_res):
    import torch.nn.functional as F
    dev = hip_device
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn(N, C, H, H, generator=g) * 2 + 0.5
    res = torch.randn(N, C, H, H, generator=g)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g)
    rm0, rv0 = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    x64, g64, b64, r64 = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True), res.double().requires_grad_(True)
    rm, rv = rm0.double().clone(), rv0.double().clone()
    y_ref = F.batch_norm(x64, rm, rv, g64, b64, True, 0.1, 1e-5)
    if use_res:
        y_ref = y_ref + r64
    if act:
        y_ref = F.elu(y_ref)
    dy = torch.randn(y_ref.shape, generator=g)
    (y_ref * dy.double()).sum().backward()
    Pn = N * H * H
    xd, resd, gd, bd = _nhwc(x).to(dev), _nhwc(res).to(dev), gamma.to(dev), beta.to(dev)
    rmd, rvd = rm0.clone().to(dev), rv0.clone().to(dev)
    y = torch.empty(Pn, C, device=dev)
    mean = torch.empty(C, device=dev)
    invstd = torch.empty(C, device=dev)
    ws = torch.empty(lib.lv_bn_workspace_floats(C) + 2 * C, device=dev)
    lib.lv_bn_fwd_f32(P(xd), P(gd), P(bd), P(resd) if use_res else None, int(act), P(y), P(mean), P(invstd), P(rmd), P(rvd),
                      1e-5, 0.1, P(ws), Pn, C, _s(dev))
    assert float((_nchw(y.cpu(), N, H, H).double() - y_ref.detach()).abs().max()) < 2e-5
    assert float((rmd.cpu().double() - rm).abs().max()) < 1e-5 and float((rvd.cpu().double() - rv).abs().max()) < 1e-4
    dyd = _nhwc(dy).to(dev)
    dv = torch.empty(Pn, C, device=dev)
    dx = torch.empty(Pn, C, device=dev)
    dg = torch.empty(C, device=dev)
    db = torch.empty(C, device=dev)
    lib.lv_bn_bwd_f32(P(xd), P(dyd), P(y), P(mean), P(invstd), P(gd), int(act), P(dv), P(dx), P(dg), P(db), 0, P(ws), Pn, C, _s(dev))
    sc = float(x64.grad.abs().max())
    assert float((_nchw(dx.cpu(), N, H, H).double() - x64.grad).abs().max()) < 2e-4 * sc
    assert float((dg.cpu().double() - g64.grad).abs().max()) < 2e-4 * float(g64.grad.abs().max())
    assert float((db.cpu().double() - b64.grad).abs().max()) < 2e-4 * float(b64.grad.abs().max())
    if use_res:
        assert float((_nchw(dv.cpu(), N, H, H).double() - r64.grad).abs().max()) < 2e-4 * float(r64.grad.abs().max())
    # the incoming gradient as two / four summands (lv_bn_bwd2_f32 / lv_bn_bwd4_f32): bit for bit what their left-to-right f32 sum gives
    t1 = torch.randn(Pn, C, generator=g).to(dev)
    t2 = torch.randn(Pn, C, generator=g).to(dev)
    t3 = torch.randn(Pn, C, generator=g).to(dev)
    for terms in ((t1, dyd - t1), (t1, t2, t3), (t1, t2, t3, dyd)):
        total = terms[0]
        for t_ in terms[1:]:
            total = total + t_
        outs = []
        for args in ((total,), terms):
            dv2, dx2 = torch.empty(Pn, C, device=dev), torch.empty(Pn, C, device=dev)
            dg2, db2 = torch.empty(C, device=dev), torch.empty(C, device=dev)
            ptrs = [P(a) for a in args] + [None] * (4 - len(args))
            if len(args) <= 2:
                lib.lv_bn_bwd2_f32(P(xd), ptrs[0], ptrs[1], P(y), P(mean), P(invstd), P(gd), int(act), P(dv2), P(dx2), P(dg2), P(db2), 0, P(ws),
                                   Pn, C, _s(dev))
            else:
                lib.lv_bn_bwd4_f32(P(xd), ptrs[0], ptrs[1], ptrs[2], ptrs[3], P(y), P(mean), P(invstd), P(gd), int(act), P(dv2), P(dx2), P(dg2),
                                   P(db2), 0, P(ws), Pn, C, _s(dev))
            outs.append((dv2.cpu(), dx2.cpu(), dg2.cpu(), db2.cpu()))
        for u, v in zip(*outs):
            assert torch.equal(u, v)


def test_sigmoid_bce_and_dec_input(lib, hip_device):
    dev = hip_device
    g = torch.Generator().manual_seed(4)
    B, npix, fm = 5, 28 * 28, 4
    logit = (torch.randn(B, npix, generator=g) * 3).to(dev)
    x = (torch.rand(B, npix, generator=g) < 0.4).float().to(dev)
    rec = torch.empty(B, device=dev)
    lib.lv_sigmoid_bce_fwd_f32(P(logit), P(x), P(rec), B, npix, 1e-12, _s(dev))
    l64 = logit.double().requires_grad_(True)
    p = torch.sigmoid(l64)
    ref = -((p + 1e-12).log() * x.double() + (1 - p + 1e-12).log() * (1 - x.double())).sum(1)
    assert float((rec.double() - ref.detach()).abs().max()) < 1e-4 * float(ref.abs().max())
    drec = torch.rand(B, generator=g).to(dev)
    (ref * drec.double()).sum().backward()
    dl = torch.empty(B, npix, device=dev)
    lib.lv_sigmoid_bce_bwd_f32(P(logit), P(x), P(drec), P(dl), B, npix, 1e-12, _s(dev))
    assert float((dl.double() - l64.grad).abs().max()) < 1e-5
    zt = torch.randn(B, fm * npix, generator=g).to(dev)
    in5 = torch.empty(B * npix, 1 + fm, device=dev)
    lib.lv_dec_input_fwd_f32(P(x), P(zt), P(in5), B, npix, fm, _s(dev))
    ref5 = torch.cat([x.view(B, 1, npix), zt.view(B, fm, npix)], 1).permute(0, 2, 1).reshape(B * npix, 1 + fm)
    assert torch.equal(in5, ref5)
    dzt = torch.empty(B, fm * npix, device=dev)
    lib.lv_dec_input_bwd_f32(P(in5), P(dzt), B, npix, fm, _s(dev))
    assert torch.equal(dzt, zt)
    st = torch.tensor([5, 0], dtype=torch.int64, device=dev)
    probs = torch.rand(20000, generator=g).to(dev)
    out = torch.empty(20000, device=dev)
    lib.lv_rng_bernoulli_f32(P(probs), P(out), 20000, P(st), 7, _s(dev))
    assert set(out.unique().tolist()) <= {0.0, 1.0} and abs(float(out.mean()) - float(probs.mean())) < 0.02


# ---- fused glue kernels of one inner step (lv_head.hip, lv_loss_assemble, lv_clip_norm2, lv_rng_noise_step) --------------
@pytest.mark.parametrize("B,H,ns,nz", [(32, 1024, 1, 32), (5, 50, 3, 1), (7, 70, 1, 40), (128, 256, 1, 32)])
def test_enc_head_fwd_bwd(lib, hip_device, B, H, ns, nz):
    dev = hip_device
    g = torch.Generator().manual_seed(B + H)
    hT = torch.randn(B, H, generator=g)
    W = torch.randn(2 * nz, H, generator=g) / H ** 0.5
    eps = torch.randn(B, ns, nz, generator=g)
    hT64, W64 = hT.double().requires_grad_(True), W.double().requires_grad_(True)
    mulv_r = hT64 @ W64.t()
    mu, lv = mulv_r[:, :nz], mulv_r[:, nz:]
    z_r = mu.unsqueeze(1) + eps.double() * (0.5 * lv).exp().unsqueeze(1)
    kl_r = 0.5 * (mu.pow(2) + lv.exp() - lv - 1).sum(1)
    gz = torch.randn(B, ns, nz, generator=g)
    gk = torch.randn(B, generator=g)
    ((z_r * gz.double()).sum() + (kl_r * gk.double()).sum()).backward()
    d = [t.to(dev) for t in (hT, W, eps, gz, gk)]
    mulv = torch.empty(B, 2 * nz, device=dev); z = torch.empty(B, ns, nz, device=dev); kl = torch.empty(B, device=dev)
    lib.lv_enc_head_fwd_f32(P(d[0]), P(d[1]), P(d[2]), P(mulv), P(z), P(kl), B, H, ns, nz, _s(dev))
    assert float((mulv.cpu().double() - mulv_r.detach()).abs().max()) < 1e-5 * float(mulv_r.abs().max())
    assert float((z.cpu().double() - z_r.detach()).abs().max()) < 1e-5 * float(z_r.abs().max())
    assert float((kl.cpu().double() - kl_r.detach()).abs().max()) < 1e-5 * float(kl_r.abs().max())
    dmulv = torch.empty(B, 2 * nz, device=dev); dhT = torch.empty(B, H, device=dev); gW = torch.empty(2 * nz, H, device=dev)
    # dz handed over as 3 partial sums (as lv_dec_tail_bwd_f32 does)
    gz3 = torch.stack([d[3] * 0.5, d[3] * 0.25, d[3] * 0.25]).contiguous()
    lib.lv_enc_head_bwd_f32(P(mulv), P(d[2]), P(gz3), 3, P(d[4]), P(d[0]), P(d[1]), P(dmulv), P(dhT), P(gW), B, H, ns, nz, _s(dev))
    assert float((dhT.cpu().double() - hT64.grad).abs().max()) < 2e-5 * float(hT64.grad.abs().max())
    assert float((gW.cpu().double() - W64.grad).abs().max()) < 2e-5 * float(W64.grad.abs().max())


@pytest.mark.parametrize("B,H,nz,ni,unit_major", [(32, 1024, 32, 512, 1), (5, 50, 1, 50, 0), (7, 36, 5, 20, 1), (128, 64, 40, 8, 0)])
def test_dec_init_and_tail(lib, hip_device, B, H, nz, ni, unit_major):
    dev = hip_device
    g = torch.Generator().manual_seed(B * 3 + H)
    z = torch.randn(B, nz, generator=g)
    wtr = torch.randn(H, nz, generator=g)
    wih = torch.randn(4 * H, ni + nz, generator=g)
    bih, bhh = torch.randn(4 * H, generator=g), torch.randn(4 * H, generator=g)
    c0_r = z.double() @ wtr.double().t()
    zp_r = z.double() @ wih[:, ni:].double().t() + bih.double() + bhh.double()
    d = [t.to(dev) for t in (z, wtr, wih, bih, bhh)]
    c0 = torch.empty(B, H, device=dev); h0 = torch.empty(B, H, device=dev); zp = torch.empty(B, 4 * H, device=dev)
    lib.lv_dec_init_f32(P(d[0]), P(d[1]), P(d[2]), ni + nz, ni, P(d[3]), P(d[4]), P(c0), P(h0), P(zp), unit_major, B, H, nz, _s(dev))
    if unit_major:
        zp = zp.view(B, H, 4).permute(0, 2, 1).reshape(B, 4 * H)
    assert float((c0.cpu().double() - c0_r).abs().max()) < 1e-5 * float(c0_r.abs().max())
    assert float((h0.cpu().double() - torch.tanh(c0_r)).abs().max()) < 1e-5
    assert float((zp.cpu().double() - zp_r).abs().max()) < 1e-5 * float(zp_r.abs().max())
    # tail
    dGsum = torch.randn(B, 4 * H, generator=g)
    dc0 = torch.randn(B, H, generator=g)
    gwih = torch.full((4 * H, ni + nz), 7.0, device=dev)
    gwtr = torch.empty(H, nz, device=dev); gb1 = torch.empty(4 * H, device=dev); gb2 = torch.empty(4 * H, device=dev)
    parts = lib.lv_dec_tail_parts(H)
    dzp = torch.full((parts, B, nz), float("nan"), device=dev)
    dGsum_d, dc0_d = dGsum.to(dev), dc0.to(dev)          # named: P() of a temporary would dangle
    lib.lv_dec_tail_bwd_f32(P(dGsum_d), P(dc0_d), P(d[0]), P(d[2]), ni + nz, ni, P(d[1]), P(gwih), ni + nz, P(gwtr),
                            P(gb1), P(gb2), P(dzp), B, H, nz, _s(dev))
    dz = dzp.sum(0)
    r_gwih = dGsum.double().t() @ z.double()
    r_gwtr = dc0.double().t() @ z.double()
    r_b = dGsum.double().sum(0)
    r_dz = dGsum.double() @ wih[:, ni:].double() + dc0.double() @ wtr.double()
    e_g = (gwih[:, ni:].cpu().double() - r_gwih).abs()
    assert float(e_g.max()) < 2e-5 * float(r_gwih.abs().max()), (float(e_g.max()), int(e_g.argmax()), float(r_gwih.abs().max()))
    assert bool((gwih[:, :ni] == 7.0).all())                       # the word-embedding columns are not touched
    assert float((gwtr.cpu().double() - r_gwtr).abs().max()) < 2e-5 * float(r_gwtr.abs().max())
    assert float((gb1.cpu().double() - r_b).abs().max()) < 2e-5 * float(r_b.abs().max()) and torch.equal(gb1, gb2)
    assert float((dz.cpu().double() - r_dz).abs().max()) < 5e-5 * float(r_dz.abs().max())


@pytest.mark.parametrize("T,B", [(199, 32), (1, 3), (70, 130)])
def test_loss_assemble(lib, hip_device, T, B):
    dev = hip_device
    g = torch.Generator().manual_seed(T + B)
    nll = torch.rand(T, B, generator=g) * 10
    kl = torch.rand(B, generator=g)
    gl = torch.full((B,), 1.0 / B)
    klw = torch.tensor([0.37])
    acc = torch.tensor([1.0, 2.0, 3.0], device=dev)
    outs = [torch.empty(B, device=dev) for _ in range(4)]
    nll_d, kl_d, klw_d, gl_d = nll.to(dev), kl.to(dev), klw.to(dev), gl.to(dev)      # named: P() of a temporary would dangle
    lib.lv_loss_assemble_f32(P(nll_d), P(kl_d), P(klw_d), P(gl_d), P(outs[0]), P(outs[1]), P(outs[2]),
                             P(outs[3]), P(acc), T, B, _s(dev))
    rec_r = nll.double().sum(0)
    loss_r = rec_r + 0.37 * kl.double()
    assert float((outs[1].cpu().double() - rec_r).abs().max()) < 1e-5 * float(rec_r.abs().max())
    assert float((outs[0].cpu().double() - loss_r).abs().max()) < 1e-5 * float(loss_r.abs().max())
    assert torch.allclose(outs[2].cpu(), gl) and torch.allclose(outs[3].cpu(), 0.37 * gl)
    want = torch.tensor([1.0 + float(loss_r.sum()), 2.0 + float(rec_r.sum()), 3.0 + float(kl.double().sum())])
    assert float((acc.cpu() - want).abs().max()) < 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("n1,n2", [(1000, 77), (1 << 20, (1 << 21) + 13), (5, 1)])
def test_clip_norm2(lib, hip_device, n1, n2):
    dev = hip_device
    g = torch.Generator().manual_seed(n1 + n2)
    a, b = torch.randn(n1, generator=g), torch.randn(n2, generator=g) * 0.01
    ws = torch.empty(lib.lv_sumsq_workspace_floats(), device=dev)
    out = torch.zeros(3, device=dev)
    a_d, b_d = a.to(dev), b.to(dev)
    lib.lv_clip_norm2_f32(P(a_d), n1, P(b_d), n2, P(ws), 5.0, P(out, 0), P(out, 1), P(out, 2), _s(dev))
    nrm = float((a.double().pow(2).sum() + b.double().pow(2).sum()).sqrt())
    o = out.cpu().tolist()
    assert abs(o[2] - nrm) < 1e-5 * nrm and abs(o[0] - nrm * nrm) < 1e-5 * nrm * nrm
    assert abs(o[1] - min(1.0, 5.0 / (nrm + 1e-6))) < 1e-5


def test_noise_step_equals_separate_draws(lib, hip_device):
    dev = hip_device
    n_eps, n_in, n_out = 32 * 32, 32 * 199 * 512 + 3, 5 * 7 * 11
    st = torch.tensor([783435, 5], dtype=torch.int64, device=dev)
    eps = torch.empty(n_eps, device=dev); m1 = torch.empty(n_in, dtype=torch.uint8, device=dev)
    m2 = torch.empty(n_out, dtype=torch.uint8, device=dev)
    lib.lv_rng_noise_step(P(eps), n_eps, P(m1), n_in, 0.5, P(m2), n_out, 0.3, P(st), 1, _s(dev))
    assert st.cpu().tolist() == [783435, 6]
    st2 = torch.tensor([783435, 5], dtype=torch.int64, device=dev)
    e2 = torch.empty_like(eps); a2 = torch.empty_like(m1); b2 = torch.empty_like(m2)
    lib.lv_rng_normal_f32(P(e2), n_eps, P(st2), 0, _s(dev))
    lib.lv_rng_keepmask_u8(P(a2), n_in, 0.5, P(st2), 1, _s(dev))
    lib.lv_rng_keepmask_u8(P(b2), n_out, 0.3, P(st2), 2, _s(dev))
    assert torch.equal(eps, e2) and torch.equal(m1, a2) and torch.equal(m2, b2)
    # eval mode: no masks
    lib.lv_rng_noise_step(P(eps), n_eps, None, 0, 0.5, None, 0, 0.5, P(st), 1, _s(dev))
    assert st.cpu().tolist() == [783435, 7] and not torch.equal(eps, e2)


@pytest.mark.parametrize("T,B,V,H", [(5, 32, 20001, 64), (3, 7, 333, 40), (2, 5, 128, 72), (4, 33, 1000, 128)])
def test_gemm_b16_nll_fused(lib, hip_device, T, B, V, H, tile=0):
    """lv_gemm_b16_nll + lv_softmax_nll_merge_f32 + lv_softmax_nll_bwd_h16 against float64: binary16 logits image = RNE of the
    exact product of the bf16 operands, lse / nll taken from the ROUNDED logits, gradient rows sum to zero."""
    dev = hip_device
    g = torch.Generator().manual_seed(T * 7 + V)
    R = T * B
    ldv = (V + 31) // 32 * 32
    O = (torch.randn(R, H, generator=g)).to(torch.bfloat16)
    W = (torch.randn(V, H, generator=g) * (3.0 / H ** 0.5)).to(torch.bfloat16)
    x = torch.randint(0, V, (B, T + 1), generator=g)
    ref = (O.double() @ W.double().t())                                   # [R][V], rows r = t*B + b
    ref16 = ref.to(torch.float16)
    O16, W16 = O.view(torch.int16).to(dev), W.view(torch.int16).to(dev)
    l16 = torch.full((R, ldv), 0x7E00, dtype=torch.int16, device=dev)
    nparts = lib.lv_gemm_b16_nll_parts(V)
    part = torch.full((R, 2 * nparts), float("nan"), device=dev)
    tgt = torch.full((R,), float("nan"), device=dev)
    xd = x.to(dev)
    lib.lv_gemm_b16_nll_tile(tile, R, V, H, P(O16), H, P(W16), H, P(l16), ldv, P(xd), T + 1, 1, B, P(part), P(tgt), _s(dev))
    if tile and H % 64 == 0:                  # both tile sizes: the same logits image and statistics, bit for bit (a ragged K tile is
                                              # accumulated first by the 256 kernel, last by the 128 one)
        l16b = torch.full((R, ldv), 0x7E00, dtype=torch.int16, device=dev)
        partb = torch.full((R, 2 * nparts), float("nan"), device=dev)
        tgtb = torch.full((R,), float("nan"), device=dev)
        lib.lv_gemm_b16_nll_tile(128 if tile >= 256 else 256, R, V, H, P(O16), H, P(W16), H, P(l16b), ldv, P(xd), T + 1, 1, B, P(partb), P(tgtb), _s(dev))
        assert torch.equal(l16[:, :V].cpu(), l16b[:, :V].cpu()) and torch.equal(part.cpu(), partb.cpu()) and torch.equal(tgt.cpu(), tgtb.cpu())
    got16 = l16[:, :V].cpu().view(torch.float16)
    # binary16 RNE of an f32 accumulation of exact bf16 products: within 1 ulp of the float64 result's rounding
    assert float((got16.double() - ref16.double()).abs().max()) <= 2.0 * float(ref16.double().abs().max()) * 2 ** -11
    lse = torch.empty(R, device=dev); nll = torch.empty(R, device=dev)
    lib.lv_softmax_nll_merge_f32(P(part), nparts, P(tgt), P(lse), P(nll), R, _s(dev))
    tg = x[:, 1:].t().reshape(-1)                                          # row r = t*B + b -> x[b][t+1]
    lse_r = torch.logsumexp(got16.double(), dim=1)
    nll_r = lse_r - got16.double().gather(1, tg.unsqueeze(1)).squeeze(1)
    assert float((lse.cpu().double() - lse_r).abs().max()) < 1e-5 * float(lse_r.abs().max())
    assert float((nll.cpu().double() - nll_r).abs().max()) < 1e-5 * float(nll_r.abs().max()) + 1e-5
    rs = torch.rand(B, generator=g) + 0.5
    dl = torch.full((R, ldv), 0x7FC0, dtype=torch.int16, device=dev)
    rs_d = rs.to(dev)
    lib.lv_softmax_nll_bwd_h16(P(l16), ldv, P(lse), P(xd), T + 1, 1, P(rs_d), P(dl), ldv, T, B, V, _s(dev))
    gref = torch.softmax(got16.double(), dim=1)
    gref[torch.arange(R), tg] -= 1.0
    gref = gref * rs[torch.arange(R) % B].double().unsqueeze(1)
    got = dl[:, :V].cpu().view(torch.bfloat16).double()
    assert float((got - gref).abs().max()) < 2 ** -8 * float(gref.abs().max()) + 1e-7
    assert float(got.sum(1).abs().max()) < 2 ** -7 * float(rs.max())      # rows sum to ~0 up to the bf16 rounding of the (p_target - 1) entry
    assert bool((dl[:, V:] == 0).all())


@pytest.mark.parametrize("tA,M,N,K", [(0, 2100, 2304, 4100), (1, 4500, 1024, 3000), (0, 6368, 1024, 20001)])
@pytest.mark.parametrize("tile", [256, 257, 258])
def test_gemm_b16_tile256_repeatable(lib, hip_device, tA, M, N, K, tile):
    """Race screen of the 256 x 256 kernel's LDS-DMA hand-over and of the K-split tail: the same launch twelve times, on operands
    that are refilled in between (so the caches hold something else), must give the same bits every time -- a fragment read that
    overtook its DMA, or a reduce that read a slab early, shows up as a sporadic difference."""
    dev = hip_device
    g = torch.Generator().manual_seed(M + K)
    lda = (((M if tA else K) + 7) // 8) * 8
    ldb = ((K + 7) // 8) * 8
    A16 = _bf16_bits(torch.randn(K if tA else M, lda, generator=g)).to(dev)
    B16 = _bf16_bits(torch.randn(N, ldb, generator=g)).to(dev)
    ws = torch.empty(1 << 25, device=dev)
    scratch = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    first = None
    for it in range(12):
        C = torch.full((M, N), float("nan"), device=dev)
        ws.fill_(float(it))                      # stale slabs must never be read
        scratch.fill_(it)                        # evict the operands from L2
        lib.lv_gemm_b16_tile(tile, tA, M, N, K, 1.0, P(A16), lda, P(B16), ldb, P(C), N, 0, None, 0, 1, None, 0, 1, P(ws), ws.numel(), _s(dev))
        out = C.cpu()
        assert bool(torch.isfinite(out).all())
        if first is None:
            first = out
        else:
            assert torch.equal(out, first), "run %d differs" % it


@pytest.mark.parametrize("T,B,V,H", [(5, 32, 20001, 64), (3, 7, 333, 40), (2, 5, 128, 72), (9, 33, 1000, 128), (40, 32, 20001, 1024),
                                     (199, 32, 20001, 128)])      # the last: the Yahoo step's 1975 tiles
@pytest.mark.parametrize("tile", [256, 257, 258])
def test_gemm_b16_nll_fused_tile256(lib, hip_device, T, B, V, H, tile):
    test_gemm_b16_nll_fused(lib, hip_device, T, B, V, H, tile=tile)


@pytest.mark.parametrize("N,k,masked", [(2, 7, True), (1, 5, True), (3, 3, True), (2, 3, False), (1, 7, False), (50, 7, True), (50, 5, True),
                                         (50, 3, True), (37, 5, False)])
def test_conv32_direct_fwd_dgrad_wgrad(lib, hip_device, N, k, masked):
    """lv_conv32_* (direct 32 -> 32 convolution on 28 x 28 maps) against torch conv2d in float64: forward and data gradient over
    the mask's tap prefix, weight gradient over all taps (the reference keeps gradients on masked taps)."""
    dev = hip_device
    g = torch.Generator().manual_seed(N * 10 + k)
    C, S = 32, 28
    x = torch.randn(N, C, S, S, generator=g)
    w = torch.randn(C, C, k, k, generator=g) / (C * k * k) ** 0.5
    dy = torch.randn(N, C, S, S, generator=g)
    nt = (k // 2) * k + k // 2 + 1 if masked else k * k
    mask = torch.zeros(k * k)
    mask[:nt] = 1
    wm = (w.reshape(C, C, k * k) * mask).reshape(C, C, k, k)                 # what MaskedConv2d leaves in the weight
    x64 = x.double().requires_grad_(True)
    w64 = wm.double().requires_grad_(True)
    y_r = torch.nn.functional.conv2d(x64, w64, padding=k // 2)
    y_r.backward(dy.double())
    xn, dyn = _nhwc(x).to(dev), _nhwc(dy).to(dev)
    wd = wm.contiguous().to(dev)
    wp = torch.empty(lib.lv_conv32_wpack_floats(nt), device=dev)
    wpt = torch.empty(lib.lv_conv32_wpack_floats(nt), device=dev)
    lib.lv_conv32_pack_f32(P(wd), P(wp), k, nt, 0, _s(dev))
    lib.lv_conv32_pack_f32(P(wd), P(wpt), k, nt, 1, _s(dev))
    y = torch.full((N * S * S, C), float("nan"), device=dev)
    lib.lv_conv32_f32(P(xn), P(wp), P(y), N, k, nt, 0, 0, _s(dev))
    assert float((_nchw(y.cpu(), N, S, S).double() - y_r.detach()).abs().max()) < 1e-5 * float(y_r.abs().max())
    dx = torch.full((N * S * S, C), float("nan"), device=dev)
    lib.lv_conv32_f32(P(dyn), P(wpt), P(dx), N, k, nt, 1, 0, _s(dev))
    assert float((_nchw(dx.cpu(), N, S, S).double() - x64.grad).abs().max()) < 1e-5 * float(x64.grad.abs().max())
    # accumulate flag
    lib.lv_conv32_f32(P(dyn), P(wpt), P(dx), N, k, nt, 1, 1, _s(dev))
    assert float((_nchw(dx.cpu(), N, S, S).double() - 2 * x64.grad).abs().max()) < 2e-5 * float(x64.grad.abs().max())
    # weight gradient: ALL taps (gradient of the unmasked convolution wrt w at the masked weights)
    wfull = wm.double().requires_grad_(True)
    torch.nn.functional.conv2d(x.double(), wfull, padding=k // 2).backward(dy.double())
    ws = torch.full((lib.lv_conv32_wgrad_ws_floats(N, k),), float("nan"), device=dev)
    dw = torch.full((C, C, k, k), float("nan"), device=dev)
    lib.lv_conv32_wgrad_f32(P(xn), P(dyn), P(dw), P(ws), N, k, 0, _s(dev))
    assert float((dw.cpu().double() - wfull.grad).abs().max()) < 2e-5 * float(wfull.grad.abs().max())


@pytest.mark.parametrize("N,k,masked", [(2, 7, True), (1, 5, True), (3, 3, True), (2, 3, False), (50, 7, True), (50, 5, True), (37, 5, False)])
@pytest.mark.parametrize("terms", [3, 1])
def test_conv32_direct_split_bf16(lib, hip_device, N, k, masked, terms):
    """lv_conv32_b16: the same convolution with every operand as hi + lo of two bf16 numbers on the bf16 matrix pipe, against torch
    conv2d in float64 -- terms = 3 (hi*hi' + hi*lo' + lo*hi') to f32-like accuracy, terms = 1 (plain bf16 operands) to bf16's;
    forward with the BatchNorm partials, data gradient with the transposed image, the accumulate flag."""
    dev = hip_device
    g = torch.Generator().manual_seed(N * 10 + k)
    C, S = 32, 28
    x = torch.randn(N, C, S, S, generator=g)
    w = torch.randn(C, C, k, k, generator=g) / (C * k * k) ** 0.5
    dy = torch.randn(N, C, S, S, generator=g)
    nt = (k // 2) * k + k // 2 + 1 if masked else k * k
    mask = torch.zeros(k * k)
    mask[:nt] = 1
    wm = (w.reshape(C, C, k * k) * mask).reshape(C, C, k, k)
    x64 = x.double().requires_grad_(True)
    y_r = torch.nn.functional.conv2d(x64, wm.double(), padding=k // 2)
    y_r.backward(dy.double())
    tol = 3e-5 if terms == 3 else 2e-2
    xn, dyn = _nhwc(x).to(dev), _nhwc(dy).to(dev)
    wd = wm.contiguous().to(dev)
    wp = torch.empty(lib.lv_conv32_wpack_floats(nt), device=dev)
    wpt = torch.empty(lib.lv_conv32_wpack_floats(nt), device=dev)
    lib.lv_conv32_pack_b16(P(wd), P(wp), k, nt, 0, _s(dev))
    lib.lv_conv32_pack_b16(P(wd), P(wpt), k, nt, 1, _s(dev))
    y = torch.full((N * S * S, C), float("nan"), device=dev)
    nblk = lib.lv_conv32_blocks(N)
    part = torch.full((nblk, 2, C), float("nan"), device=dev)
    lib.lv_conv32_b16(P(xn), P(wp), P(y), P(part), N, k, nt, 0, 0, terms, _s(dev))
    assert float((_nchw(y.cpu(), N, S, S).double() - y_r.detach()).abs().max()) < tol * float(y_r.abs().max())
    # the BatchNorm stage-1 partials are those of the values that were stored
    yd = y.double()
    assert float((part[:, 0].double().sum(0) - yd.sum(0)).abs().max()) < 1e-4 * float(yd.abs().sum(0).max())
    assert float((part[:, 1].double().sum(0) - (yd * yd).sum(0)).abs().max()) < 1e-4 * float((yd * yd).sum(0).max())
    dx = torch.full((N * S * S, C), float("nan"), device=dev)
    lib.lv_conv32_b16(P(dyn), P(wpt), P(dx), None, N, k, nt, 1, 0, terms, _s(dev))
    assert float((_nchw(dx.cpu(), N, S, S).double() - x64.grad).abs().max()) < tol * float(x64.grad.abs().max())
    lib.lv_conv32_b16(P(dyn), P(wpt), P(dx), None, N, k, nt, 1, 1, terms, _s(dev))
    assert float((_nchw(dx.cpu(), N, S, S).double() - 2 * x64.grad).abs().max()) < 2 * tol * float(x64.grad.abs().max())
    # weight gradient over ALL taps, K = pixels through the transposing LDS reads
    wfull = wm.double().requires_grad_(True)
    torch.nn.functional.conv2d(x.double(), wfull, padding=k // 2).backward(dy.double())
    ws = torch.full((lib.lv_conv32_wgrad_ws_floats(N, k),), float("nan"), device=dev)
    dw = torch.full((C, C, k, k), float("nan"), device=dev)
    lib.lv_conv32_wgrad_b16(P(xn), P(dyn), P(dw), P(ws), N, k, 0, terms, _s(dev))
    assert float((dw.cpu().double() - wfull.grad).abs().max()) < tol * float(wfull.grad.abs().max())


def _bn_bwd_reference(g, yv, xin, mean, invstd, gamma, act):
    """dv, dx, dgamma, dbeta of a train-mode BatchNorm (+ ELU) backward in float64, from the gradient g wrt its output."""
    dv = g * torch.where(yv > 0, torch.ones_like(yv), yv + 1) if act else g
    xh = (xin - mean) * invstd
    n = xin.shape[0]
    s0, s1 = dv.sum(0), (dv * xh).sum(0)
    dx = gamma * invstd * (dv - s0 / n - xh * s1 / n)
    return dv, dx, s1, s0


@pytest.mark.parametrize("N,k,terms", [(2, 7, 0), (3, 5, 0), (50, 3, 0), (50, 7, 3), (5, 5, 3), (4, 3, 1)])
@pytest.mark.parametrize("act", [1, 0])
def test_conv32_data_gradient_with_fused_batchnorm_backward(lib, hip_device, N, k, terms, act):
    """lv_conv32_bnbwd + lv_bn_bwd_apply_partials_f32: the data gradient of a masked convolution leaves its kernel as the dv of the
    BatchNorm in front of the convolution, with the per-workgroup (sum dv, sum dv * xhat) -- against the data gradient (float64) pushed
    through a BatchNorm (+ ELU) backward in float64."""
    dev = hip_device
    g = torch.Generator().manual_seed(N * 7 + k + act)
    C, S = 32, 28
    Pn = N * S * S
    w = torch.randn(C, C, k, k, generator=g) / (C * k * k) ** 0.5
    nt = (k // 2) * k + k // 2 + 1
    mask = torch.zeros(k * k)
    mask[:nt] = 1
    wm = (w.reshape(C, C, k * k) * mask).reshape(C, C, k, k)
    dyc = torch.randn(N, C, S, S, generator=g)                       # gradient wrt the convolution's output
    xin = torch.randn(Pn, C, generator=g)                            # BatchNorm input (NHWC rows)
    gamma = torch.rand(C, generator=g) + 0.5
    mean, var = xin.double().mean(0), xin.double().var(0, unbiased=False)
    invstd = (var + 1e-5).rsqrt()
    ybn = (xin.double() - mean) * invstd * gamma.double()
    yv = torch.where(ybn > 0, ybn, ybn.exp() - 1) if act else ybn    # BatchNorm output (+ ELU): the convolution's input
    x_conv = _nchw(yv.float(), N, S, S).double().requires_grad_(True)
    torch.nn.functional.conv2d(x_conv, wm.double(), padding=k // 2).backward(dyc.double())
    gref = _nhwc(x_conv.grad.float()).double()                       # dL/d(BN output), [P][C]
    dv_r, dx_r, dgam_r, dbeta_r = _bn_bwd_reference(gref, yv, xin.double(), mean, invstd, gamma.double(), act)
    wd = wm.contiguous().to(dev)
    wpt = torch.empty(lib.lv_conv32_wpack_floats(nt), device=dev)
    (lib.lv_conv32_pack_b16 if terms else lib.lv_conv32_pack_f32)(P(wd), P(wpt), k, nt, 1, _s(dev))
    dyn, xd, yd = _nhwc(dyc).to(dev), xin.to(dev), yv.float().to(dev)
    md, isd, gd = mean.float().to(dev), invstd.float().to(dev), gamma.to(dev)
    nblk = lib.lv_conv32_blocks(N)
    dv = torch.full((Pn, C), float("nan"), device=dev)
    part = torch.full((nblk, 2, C), float("nan"), device=dev)
    lib.lv_conv32_bnbwd(P(dyn), P(wpt), P(dv), P(part), N, k, nt, P(yd) if act else None, P(xd), P(md), P(isd), act, terms, _s(dev))
    tol = 2e-5 if terms == 0 else (6e-5 if terms == 3 else 3e-2)
    assert float((dv.cpu().double() - dv_r).abs().max()) < tol * float(dv_r.abs().max())
    dvd = dv.double()
    xh = ((xd.double() - md.double()) * isd.double())
    assert float((part[:, 0].double().sum(0) - dvd.sum(0)).abs().max()) < 1e-4 * float(dvd.abs().sum(0).max())
    assert float((part[:, 1].double().sum(0) - (dvd * xh).sum(0)).abs().max()) < 1e-4 * float((dvd * xh).abs().sum(0).max())
    dx = torch.full((Pn, C), float("nan"), device=dev)
    dgam, dbeta = torch.full((C,), float("nan"), device=dev), torch.full((C,), float("nan"), device=dev)
    lib.lv_bn_bwd_apply_partials_f32(P(xd), P(dv), P(part), nblk, P(md), P(isd), P(gd), P(dx), P(dgam), P(dbeta), 0, Pn, C, _s(dev))
    assert float((dx.cpu().double() - dx_r).abs().max()) < 5 * tol * float(dx_r.abs().max())
    assert float((dgam.cpu().double() - dgam_r).abs().max()) < 5 * tol * float(dgam_r.abs().max() + dv_r.abs().sum(0).max() * 1e-3)
    assert float((dbeta.cpu().double() - dbeta_r).abs().max()) < 5 * tol * float(dbeta_r.abs().max() + dv_r.abs().sum(0).max() * 1e-3)


@pytest.mark.parametrize("P_,Cin,Cout", [(39200, 32, 64), (1000, 64, 32), (129, 32, 32)])
def test_conv1x1_data_gradient_with_fused_batchnorm_backward(lib, hip_device, P_, Cin, Cout):
    """lv_conv1x1_bnbwd_f32: the pointwise convolution's data gradient as the dv of the BatchNorm in front of it (Cin = channels of the
    BatchNorm = input channels of the forward convolution)."""
    dev = hip_device
    g = torch.Generator().manual_seed(P_ + Cin)
    w = torch.randn(Cout, Cin, generator=g) / Cin ** 0.5             # forward weight [Cout][Cin]
    dyc = torch.randn(P_, Cout, generator=g)
    xin = torch.randn(P_, Cin, generator=g)
    mean, var = xin.double().mean(0), xin.double().var(0, unbiased=False)
    invstd = (var + 1e-5).rsqrt()
    gamma = torch.rand(Cin, generator=g) + 0.5
    ybn = (xin.double() - mean) * invstd * gamma.double()
    yv = torch.where(ybn > 0, ybn, ybn.exp() - 1)
    gref = dyc.double() @ w.double()                                 # dL/d(conv input) = dL/d(BN output)
    dv_r, dx_r, dgam_r, dbeta_r = _bn_bwd_reference(gref, yv, xin.double(), mean, invstd, gamma.double(), 1)
    nblk = int(lib.lv_conv1x1_blocks(P_))
    dv = torch.full((P_, Cin), float("nan"), device=dev)
    part = torch.full((nblk, 2, Cin), float("nan"), device=dev)
    dyd, wd, xd, yd = dyc.to(dev), w.to(dev), xin.to(dev), yv.float().to(dev)
    md, isd, gd = mean.float().to(dev), invstd.float().to(dev), gamma.to(dev)
    lib.lv_conv1x1_bnbwd_f32(P(dyd), P(wd), P(dv), P(part), P_, Cout, Cin, P(yd), P(xd), P(md), P(isd), 1, _s(dev))
    assert float((dv.cpu().double() - dv_r).abs().max()) < 2e-5 * float(dv_r.abs().max())
    dx = torch.full((P_, Cin), float("nan"), device=dev)
    dgam, dbeta = torch.full((Cin,), float("nan"), device=dev), torch.full((Cin,), float("nan"), device=dev)
    lib.lv_bn_bwd_apply_partials_f32(P(xd), P(dv), P(part), nblk, P(md), P(isd), P(gd), P(dx), P(dgam), P(dbeta), 0, P_, Cin, _s(dev))
    assert float((dx.cpu().double() - dx_r).abs().max()) < 1e-4 * float(dx_r.abs().max())
    assert float((dgam.cpu().double() - dgam_r).abs().max()) < 1e-4 * float(dgam_r.abs().max() + dv_r.abs().sum(0).max() * 1e-3)


@pytest.mark.parametrize("P_,Cin,Cout", [(39200, 64, 32), (1000, 32, 64), (300, 64, 64), (129, 32, 32)])
def test_conv1x1_fwd_dgrad_wgrad(lib, hip_device, P_, Cin, Cout):
    dev = hip_device
    g = torch.Generator().manual_seed(P_ + Cin)
    x = torch.randn(P_, Cin, generator=g)
    w = torch.randn(Cout, Cin, generator=g) / Cin ** 0.5
    dy = torch.randn(P_, Cout, generator=g)
    xd, wd, dyd = x.to(dev), w.to(dev), dy.to(dev)
    y = torch.full((P_, Cout), float("nan"), device=dev)
    lib.lv_conv1x1_f32(P(xd), P(wd), P(y), P_, Cin, Cout, 0, 0, _s(dev))
    ref = x.double() @ w.double().t()
    assert float((y.cpu().double() - ref).abs().max()) < 1e-5 * float(ref.abs().max())
    dx = torch.full((P_, Cin), float("nan"), device=dev)
    lib.lv_conv1x1_f32(P(dyd), P(wd), P(dx), P_, Cout, Cin, 1, 0, _s(dev))        # dx = dy . W, W handed as stored
    refdx = dy.double() @ w.double()
    assert float((dx.cpu().double() - refdx).abs().max()) < 1e-5 * float(refdx.abs().max())
    lib.lv_conv1x1_f32(P(dyd), P(wd), P(dx), P_, Cout, Cin, 1, 1, _s(dev))
    assert float((dx.cpu().double() - 2 * refdx).abs().max()) < 2e-5 * float(refdx.abs().max())
    ws = torch.full((lib.lv_conv1x1_wgrad_ws_floats(Cin, Cout),), float("nan"), device=dev)
    dw = torch.full((Cout, Cin), float("nan"), device=dev)
    lib.lv_conv1x1_wgrad_f32(P(xd), P(dyd), P(dw), P(ws), P_, Cin, Cout, 0, _s(dev))
    refdw = dy.double().t() @ x.double()
    assert float((dw.cpu().double() - refdw).abs().max()) < 2e-5 * float(refdw.abs().max())


@pytest.mark.parametrize("N,k,Cin,Cout", [(3, 5, 64, 32), (50, 3, 32, 64), (2, 7, 64, 64)])
def test_conv_bnstat_feeds_batchnorm(lib, hip_device, N, k, Cin, Cout):
    """The convolutions that also emit the following BatchNorm's stage-1 partials (lv_conv32_bnstat_f32, lv_conv1x1_bnstat_f32):
    same outputs as the plain entries, and lv_bn_fwd_partials_f32 on their partials == lv_bn_fwd_f32 on the activation."""
    dev = hip_device
    g = torch.Generator().manual_seed(N + k)

    def bn_both(y, C, nblk, part):
        Pn = y.shape[0]
        gamma, beta = (torch.rand(C, generator=g) + 0.5).to(dev), torch.randn(C, generator=g).to(dev)
        res = torch.randn(Pn, C, generator=g).to(dev)
        outs = []
        for fused in (False, True):
            rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
            o, mean, invstd = torch.empty(Pn, C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
            if fused:
                lib.lv_bn_fwd_partials_f32(P(y), P(gamma), P(beta), P(res), 1, P(o), P(mean), P(invstd), P(rm), P(rv), 1e-5, 0.1,
                                           P(part), nblk, Pn, C, _s(dev))
            else:
                ws = torch.empty(lib.lv_bn_workspace_floats(C) + 2 * C, device=dev)
                lib.lv_bn_fwd_f32(P(y), P(gamma), P(beta), P(res), 1, P(o), P(mean), P(invstd), P(rm), P(rv), 1e-5, 0.1, P(ws), Pn, C,
                                  _s(dev))
            outs.append((o.cpu(), mean.cpu(), invstd.cpu(), rm.cpu(), rv.cpu()))
        for a, b in zip(*outs):
            assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max()))

    # 32 -> 32 k x k
    x = torch.randn(N * 784, 32, generator=g).to(dev)
    w = (torch.randn(32, 32, k, k, generator=g) / (32 * k) ** 0.5).to(dev)
    nt = (k // 2) * k + k // 2 + 1
    wp = torch.empty(lib.lv_conv32_wpack_floats(nt), device=dev)
    lib.lv_conv32_pack_f32(P(w), P(wp), k, nt, 0, _s(dev))
    y0, y1 = torch.empty(N * 784, 32, device=dev), torch.empty(N * 784, 32, device=dev)
    nblk = lib.lv_conv32_blocks(N)
    part = torch.full((nblk, 2, 32), float("nan"), device=dev)
    lib.lv_conv32_f32(P(x), P(wp), P(y0), N, k, nt, 0, 0, _s(dev))
    lib.lv_conv32_bnstat_f32(P(x), P(wp), P(y1), P(part), N, k, nt, _s(dev))
    assert torch.equal(y0.cpu(), y1.cpu())
    ref = torch.stack((y0.double().sum(0), (y0.double() ** 2).sum(0))).cpu()
    assert float((part.double().sum(0).cpu() - ref).abs().max()) < 1e-5 * float(ref.abs().max())
    bn_both(y1, 32, nblk, part)
    # pointwise
    Pn = N * 784
    x = torch.randn(Pn, Cin, generator=g).to(dev)
    w = (torch.randn(Cout, Cin, generator=g) / Cin ** 0.5).to(dev)
    y0, y1 = torch.empty(Pn, Cout, device=dev), torch.empty(Pn, Cout, device=dev)
    nblk = int(lib.lv_conv1x1_blocks(Pn))
    part = torch.full((nblk, 2, Cout), float("nan"), device=dev)
    lib.lv_conv1x1_f32(P(x), P(w), P(y0), Pn, Cin, Cout, 0, 0, _s(dev))
    lib.lv_conv1x1_bnstat_f32(P(x), P(w), P(y1), P(part), Pn, Cin, Cout, _s(dev))
    assert torch.equal(y0.cpu(), y1.cpu())
    ref = torch.stack((y0.double().sum(0), (y0.double() ** 2).sum(0))).cpu()
    assert float((part.double().sum(0).cpu() - ref).abs().max()) < 1e-5 * float(ref.abs().max())
    bn_both(y1, Cout, nblk, part)


@pytest.mark.parametrize("T,B,C", [(5, 3, 70), (7, 32, 128)])
def test_dropout_folded_into_image_conversion(lib, hip_device, T, B, C):
    """lv_cvt_bf16_keep_f32 / lv_keep_scale_f32: nn.Dropout on a time-major activation with the reference-layout mask
    [B][T][C], identical (bit for bit) to masking first and converting afterwards."""
    dev = hip_device
    g = torch.Generator().manual_seed(T + C)
    h = torch.randn(T * B, C, generator=g)
    keep = (torch.rand(B, T, C, generator=g) < 0.5).to(torch.uint8)
    ktm = keep.permute(1, 0, 2).reshape(T * B, C).float() * 2.0            # time-major keep * scale
    hd, kd = h.to(dev), keep.contiguous().to(dev)
    ldd, ldt = (C + 7) // 8 * 8, (T * B + 7) // 8 * 8
    out = torch.zeros(T * B, ldd, dtype=torch.int16, device=dev)
    outT = torch.zeros(C, ldt, dtype=torch.int16, device=dev)
    lib.lv_cvt_bf16_keep_f32(P(hd), C, T, B, C, P(kd), 2.0, P(out), ldd, P(outT), ldt, _s(dev))
    ref = (h * ktm).to(torch.bfloat16).view(torch.int16)
    assert torch.equal(out[:, :C].cpu(), ref)
    assert torch.equal(outT[:, :T * B].cpu(), ref.t())
    x = h.clone().to(dev)
    lib.lv_keep_scale_f32(P(x), P(kd), 2.0, T, B, C, _s(dev))
    assert torch.equal(x.cpu(), h * ktm)


@pytest.mark.parametrize("T,B,C,V,masked", [(5, 3, 70, 50, True), (4, 32, 512, 2000, False), (7, 33, 128, 300, True)])
def test_embed_gather_into_bf16_images(lib, hip_device, T, B, C, V, masked):
    """lv_embed_gather_b16: embedding lookup (+ dropout) written straight into the bf16 images [T*B][C] / [C][T*B], bit for bit what
    lv_embed_gather_f32 followed by lv_cvt_bf16_f32 produce; out-of-range ids are clamped like there."""
    dev = hip_device
    g = torch.Generator().manual_seed(T * 3 + C)
    emb = torch.randn(V, C, generator=g).to(dev)
    ids = torch.randint(-1, V + 1, (B, T + 1), generator=g).to(dev)           # one more column than used (ids_stride != T), ids outside [0, V)
    keep = (torch.rand(B, T, C, generator=g) < 0.6).to(torch.uint8).to(dev) if masked else None
    X = torch.empty(T * B, C, device=dev)
    lib.lv_embed_gather_f32(P(emb), P(ids), T + 1, P(keep), 1.25, P(X), T, B, C, V, _s(dev))
    ldd, ldt = (C + 7) // 8 * 8, (T * B + 7) // 8 * 8
    ref = torch.zeros(T * B, ldd, dtype=torch.int16, device=dev); refT = torch.zeros(C, ldt, dtype=torch.int16, device=dev)
    lib.lv_cvt_bf16_f32(P(X), C, T * B, C, P(ref), ldd, P(refT), ldt, _s(dev))
    out = torch.zeros(T * B, ldd, dtype=torch.int16, device=dev); outT = torch.zeros(C, ldt, dtype=torch.int16, device=dev)
    lib.lv_embed_gather_b16(P(emb), P(ids), T + 1, P(keep), 1.25, T, B, C, V, P(out), ldd, P(outT), ldt, _s(dev))
    assert torch.equal(out.cpu(), ref.cpu()) and torch.equal(outT.cpu(), refT.cpu())
    rows = emb.cpu()[ids.cpu()[:, :T].clamp(0, V - 1)]                         # [B][T][C]
    if masked:
        rows = torch.where(keep.cpu().bool(), rows * 1.25, torch.zeros(()))
    assert torch.equal(out[:, :C].cpu(), rows.permute(1, 0, 2).reshape(T * B, C).to(torch.bfloat16).view(torch.int16))


def test_wgrad_reduce_batched(lib, hip_device):
    """lv_wgrad_reduce_batched: the stage-2 reductions of several layers (32 -> 32 k x k and pointwise) in one launch give what
    the per-layer entries give (same partials; pointwise bit for bit, k x k up to f32 summation order)."""
    import ctypes
    dev = hip_device
    g = torch.Generator().manual_seed(11)
    N = 9
    layers, desc = [], []
    for k in (3, 5):
        x = torch.randn(N * 784, 32, generator=g).to(dev)
        dy = torch.randn(N * 784, 32, generator=g).to(dev)
        ws = torch.empty(lib.lv_conv32_wgrad_ws_floats(N, k), device=dev)
        ref = torch.empty(32, 32, k, k, device=dev)
        lib.lv_conv32_wgrad_f32(P(x), P(dy), P(ref), P(ws), N, k, 0, _s(dev))
        ws2 = torch.full_like(ws, float("nan"))
        lib.lv_conv32_wgrad_f32(P(x), P(dy), None, P(ws2), N, k, 0, _s(dev))
        out = torch.full((32, 32, k, k), float("nan"), device=dev)
        layers.append((ref, out, False, (x, dy, ws2)))
        desc += [ws2.data_ptr(), out.data_ptr(), (k * k * 1024) | (lib.lv_conv32_wgrad_parts(N, k) << 32), k * k]
    for Cin, Cout in ((64, 32), (32, 64)):
        Pn = N * 784
        x = torch.randn(Pn, Cin, generator=g).to(dev)
        dy = torch.randn(Pn, Cout, generator=g).to(dev)
        ws = torch.empty(lib.lv_conv1x1_wgrad_ws_floats(Cin, Cout), device=dev)
        ref = torch.empty(Cout, Cin, device=dev)
        lib.lv_conv1x1_wgrad_f32(P(x), P(dy), P(ref), P(ws), Pn, Cin, Cout, 0, _s(dev))
        ws2 = torch.full_like(ws, float("nan"))
        lib.lv_conv1x1_wgrad_f32(P(x), P(dy), None, P(ws2), Pn, Cin, Cout, 0, _s(dev))
        out = torch.full((Cout, Cin), float("nan"), device=dev)
        layers.append((ref, out, True, (x, dy, ws2)))
        desc += [ws2.data_ptr(), out.data_ptr(), (Cin * Cout) | (lib.lv_conv1x1_wgrad_parts(Pn) << 32), 0]
    arr = (ctypes.c_longlong * len(desc))(*desc)
    lib.lv_wgrad_reduce_batched(ctypes.cast(arr, ctypes.c_void_p), len(desc) // 4, _s(dev))
    for ref, out, exact, _ in layers:
        if exact:
            assert torch.equal(ref.cpu(), out.cpu())
        else:
            assert float((ref - out).abs().max()) < 1e-5 * float(ref.abs().max())


@pytest.mark.parametrize("n", [1, 7, 4096, 100003])
def test_bf16_payload_unpack(lib, hip_device, n):
    """lv_cvt_f32_bf16_scaled: bf16 -> f32 with a scale folded in (the way back from the data-parallel bf16 wire format)."""
    dev = hip_device
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    b = x.to(torch.bfloat16)
    src = b.view(torch.int16).to(dev)
    dst = torch.full((n,), float("nan"), device=dev)
    lib.lv_cvt_f32_bf16_scaled(P(src), n, 0.125, P(dst), _s(dev))
    assert torch.equal(dst.cpu(), b.float() * 0.125)

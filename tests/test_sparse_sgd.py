"""The row-sparse SGD step of the encoder's embedding table (lv_sgd_step_scale_rows_txn_f32, lv_optim.hip) against the dense entry
it stands in for (lv_sgd_step_scale_txn_f32): every comparison is of bit patterns.  Emulator (`not gpu`) and MI355X (`gpu`).

The flat buffer is an embedding table of V = 37 rows of ni = 8 floats (optionally behind `lead` other floats) followed by a tail of
19 floats that is no embedding; the batch names 12 distinct tokens, some of them more than once, tokens 0 and V - 1 among them, so 25
rows are absent: their gradient rows are the +0 lv_embed_scatter_full* writes."""
import pytest
import torch

from helpers import build_vae
from oracle import text_vae_oracle as O
from vae_lagging_encoder_amd import engine as _eng
from vae_lagging_encoder_amd import trainer as _trainer_mod
from vae_lagging_encoder_amd.engine import P

V, NI, TAIL, N2 = 37, 8, 19, 23
PRESENT = [0, 2, 3, 7, 11, 12, 18, 20, 25, 30, 31, 36]               # 12 distinct tokens: 25 rows absent
TOKENS = sorted(PRESENT + [0, 3, 3, 12, 30, 36, 36])                  # the batch's sorted token list, with repeats
GUARD = 7.0


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


def _data(tokens, lead, seed=0):
    """p, g over [lead | V x ni table | tail] and the other side's gradient x2; g is +0 on the rows no token names."""
    gen = torch.Generator().manual_seed(seed)
    n = lead + V * NI + TAIL
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 3.0
    table = g[lead:lead + V * NI].view(V, NI)
    absent = torch.ones(V, dtype=torch.bool)
    absent[torch.tensor(sorted(set(tokens)))] = False
    table[absent] = 0.0
    p[lead + 5 * NI] = -0.0                                             # an absent row holding a negative zero
    x2 = torch.randn(N2, generator=gen)
    return p, g, x2, absent


def _run(lib, dev, rows, p0, g0, x20, lead, tokens, lr, coef, void, wb):
    """One launch of the dense (rows = False) or the row-sparse entry on fresh copies; returns (p, g, x2) with their guards."""
    n = p0.numel()
    buf = lambda t: torch.cat([t, torch.full((4,), GUARD)]).to(dev)
    p, g, x2 = buf(p0), buf(g0), buf(x20)
    sc = torch.tensor([lr, coef, 1.0 if void else 0.0], dtype=torch.float32, device=dev)
    s = _eng.stream_ptr(dev)
    if rows:
        tok = torch.tensor(tokens, dtype=torch.int32, device=dev)
        lib.lv_sgd_step_scale_rows_txn_f32(P(p), P(g), n, P(sc, 0), P(sc, 1), wb, P(x2), N2, P(sc, 2), lead, V, NI, P(tok), len(tokens), s)
    else:
        lib.lv_sgd_step_scale_txn_f32(P(p), P(g), n, P(sc, 0), P(sc, 1), wb, P(x2), N2, P(sc, 2), s)
    return p.cpu(), g.cpu(), x2.cpu()


CASES = {
    "coef1": dict(coef=1.0),
    "clipped_write_back": dict(coef=0.37),
    "clipped_no_write_back": dict(coef=0.37, wb=0),
    "void": dict(coef=0.37, void=True),
    "coef_inf": dict(coef=float("inf")),
    "coef_nan": dict(coef=float("nan")),
    "coef_negative": dict(coef=-0.5),                                   # 0 * c is -0 and lr * -0 moves a p of -0: the dense walk
    "single_token": dict(coef=0.37, tokens=[V - 1]),                   # N = 1
    "single_token_coef1": dict(coef=1.0, tokens=[0]),
    "table_behind_a_lead": dict(coef=0.37, lead=8),
    "unaligned_table": dict(coef=0.37, lead=3),                        # rows off the 16-byte grid: the scalar row loop
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_rows_entry_equals_dense_entry(target, case):
    lib, dev = target
    c = dict(coef=1.0, void=False, wb=1, tokens=TOKENS, lead=0, lr=0.7)
    c.update(CASES[case])
    p0, g0, x20, absent = _data(c["tokens"], c["lead"])
    if case.startswith("single"):
        assert int(absent.sum()) == V - 1
    else:
        assert int(absent.sum()) == 25 and 0 in c["tokens"] and V - 1 in c["tokens"] and len(c["tokens"]) > 12
    args = (p0, g0, x20, c["lead"], c["tokens"], c["lr"], c["coef"], c["void"], c["wb"])
    dense = _run(lib, dev, False, *args)
    rows = _run(lib, dev, True, *args)
    for name, a, b in zip(("p", "g", "x2"), rows, dense):
        assert _same_bits(a, b), (case, name)
        assert bool((a[-4:] == GUARD).all()), (case, name, "guard")
    if c["void"]:
        assert _same_bits(rows[0][:-4], p0) and _same_bits(rows[1][:-4], g0) and _same_bits(rows[2][:-4], x20)
    elif case not in ("coef_inf", "coef_nan"):
        assert not _same_bits(rows[0][:-4], p0)                         # the step did move the weights


def test_rows_entry_leaves_absent_rows_alone(target):
    """The rows no token names are not visited: with a (contract-breaking) non-zero gradient there, p and g of those rows come back
    as they went in, while every named row and the tail equal the dense step."""
    lib, dev = target
    p0, g0, x20, absent = _data(TOKENS, 0)
    g0.view(-1)[:V * NI].view(V, NI)[absent] = 5.0
    args = (p0, g0, x20, 0, TOKENS, 0.7, 0.37, False, 1)
    dense = _run(lib, dev, False, *args)
    rows = _run(lib, dev, True, *args)
    tab = lambda t: t[:V * NI].view(V, NI)
    assert _same_bits(tab(rows[0])[absent], tab(p0)[absent]) and _same_bits(tab(rows[1])[absent], tab(g0)[absent])
    assert _same_bits(tab(rows[0])[~absent], tab(dense[0])[~absent]) and _same_bits(tab(rows[1])[~absent], tab(dense[1])[~absent])
    assert _same_bits(rows[0][V * NI:], dense[0][V * NI:]) and _same_bits(rows[2], dense[2])


def test_rows_entry_checks_its_arguments(target):
    lib, dev = target
    n = V * NI + TAIL
    p, g, x2 = torch.zeros(n, device=dev), torch.zeros(n, device=dev), torch.zeros(N2, device=dev)
    sc = torch.tensor([0.7, 1.0, 0.0], device=dev)
    tok = torch.tensor(TOKENS, dtype=torch.int32, device=dev)
    s = _eng.stream_ptr(dev)
    good = [P(p), P(g), n, P(sc, 0), P(sc, 1), 1, P(x2), N2, P(sc, 2), 0, V, NI, P(tok), len(TOKENS), s]
    for i, bad in ((12, None), (13, 0), (9, TAIL + 1), (9, -1), (10, 0), (4, None)):
        a = list(good)
        a[i] = bad
        with pytest.raises(_eng._lib.LvaeError):
            lib.lv_sgd_step_scale_rows_txn_f32(*a)
    assert float(p.abs().max()) == 0.0


# the trainer: encoder-only steps with the row-sparse entry on and off leave the same weights and gradients, bit for bit
V_, NI_, H_, NZ_, B_, T_ = 61, 8, 16, 4, 5, 7


def _trainer_run(dev, monkeypatch, rows_on):
    from vae_lagging_encoder_amd.trainer import AggressiveTextTrainer
    monkeypatch.setattr(_trainer_mod, "ROWS_SGD", rows_on)
    vae = build_vae(V_, NI_, H_, NZ_, dev, params=O.random_params(V_, NI_, H_, NZ_, seed=4, scale=0.3, emb_scale=0.5, head_scale=0.5))
    tr = AggressiveTextTrainer(vae, clip=5.0, lr=1.0)
    lib = tr.lib
    calls = []
    raw = lib.lv_sgd_step_scale_rows_txn_f32
    monkeypatch.setattr(lib, "lv_sgd_step_scale_rows_txn_f32", lambda *a: (calls.append(1), raw(*a))[1], raising=False)
    xs = [O.synthetic_batch(B_, T_, V_, seed=30 + i).to(dev) for i in range(3)]
    for i, up in enumerate(["encoder", "encoder", "decoder", "encoder", "both", "encoder"]):
        eps, mi, mo = O.draw_noise(B_, T_, NI_, H_, NZ_, seed=50 + i)
        tr.step(xs[i % 3], 0.7, noise=(eps.to(dev), mi.to(torch.uint8).to(dev), mo.to(torch.uint8).to(dev)), update=up)
    tr.commit()
    out = {"param." + k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}
    out.update({"grad." + k: p.grad.detach().cpu().clone() for k, p in vae.named_parameters()})
    return out, len(calls)


def test_trainer_rows_step_equals_dense_step(target, monkeypatch):
    _, dev = target
    a, na = _trainer_run(dev, monkeypatch, True)
    b, nb = _trainer_run(dev, monkeypatch, False)
    assert na == 4 and nb == 0, (na, nb)                                # the four encoder-only steps, and only those
    for k in a:
        assert _same_bits(a[k], b[k]), k

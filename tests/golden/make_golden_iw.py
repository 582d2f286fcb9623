"""Generate the fixtures of the importance-weighted training objective (objective="iw") by RUNNING THE REFERENCE (imported the way
make_golden.py imports it: make_golden.REF).

    python tests/golden/make_golden_iw.py [--small | --wide]     # writes tests/golden/text_iw_*.npz (or $GOLDEN_OUT)

Each case is one body of the aggressive loop (text.py:373-387) with the reference's own `vae.nll_iw(x, nsamples=ns, ns=ns)` in the
place of `vae.loss`: vae.train(), seed, .mean().backward(), clip_grad_norm_, encoder SGD step.  nll_iw is differentiable as it
stands -- encoder.sample is reparameterised, eval_complete_ll and eval_inference_dist are plain autograd graphs -- so value and
all 13 gradients are the reference's.  For a KL weight other than 1 the same unmodified methods are composed:
log w = eval_cond_ll - w * (eval_inference_dist - eval_prior_dist).  The draws the call consumed are recorded with
make_golden.NoiseCapture (same order and shapes as vae.loss(nsamples=ns): eps (B, ns, nz), mask_in (B, T-1, ni), mask_out
(B*ns, T-1, H)); log w, rec_s and the analytic KL are read off the reference's own intermediate results.

The CPU oracle does not carry this objective.  In its place every small case is run once more in float64 (vae.double(), the same
noise injected) and the f32 run is asserted to be within the bounds tests/test_iw_objective.py holds the HIP path to; the measured
distances are printed.  The generator also asserts that the cases exercise the weights: in every case with ns > 1 at least half
of the sentences have max_s softmax_s(log w) < 0.9.

  text_iw_small.npz            small cases ("<case>/<field>"), ns in {1, 2, 3, 4}, and a 3-step trajectory (encoder, encoder, both)
  text_iw_h1024_b8_t50.npz     V=20001 ni=512 H=1024 nz=32, B=8, ns=4, T=50: weights regenerated from the seed on the test side,
                               keep-masks stored as packed bits
"""
import math
import os
import sys

import numpy as np
import torch

SRC = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, SRC)
import make_golden as MG  # noqa: E402
import make_golden_multisample as MS  # noqa: E402

HERE = MG.HERE
CLIP = 5.0
RTOL, GRAD_RTOL = 1e-4, 2e-4          # tests/parity_common.py


class Tap(object):
    """Records what the reference's own eval_cond_ll / eval_prior_dist / eval_inference_dist return during one call."""

    def __init__(self, vae):
        self.got = {}
        for name in ("eval_cond_ll", "eval_prior_dist", "eval_inference_dist"):
            setattr(vae, name, self._wrap(name, getattr(vae, name)))

    def _wrap(self, name, fn):
        def f(*a, **k):
            r = fn(*a, **k)
            self.got[name] = r
            return r
        return f


def bound(vae, x, klw, ns):
    """-> loss (B,) with a graph, through the reference's methods."""
    if klw == 1.0:
        return vae.nll_iw(x, nsamples=ns, ns=ns)
    from modules.utils import log_sum_exp
    z, param = vae.encoder.sample(x, ns)
    log_w = vae.eval_cond_ll(x, z) - klw * (vae.eval_inference_dist(x, z, param) - vae.eval_prior_dist(z))
    return -(log_sum_exp(log_w, dim=-1) - math.log(ns))


def run_step(vae, tap, x, klw, ns, enc_opt, dec_opt, update, max_norm):
    enc_opt.zero_grad()
    dec_opt.zero_grad()
    loss = bound(vae, x, klw, ns)
    loss.mean(dim=-1).backward()
    ll, logp, logq = (tap.got[k].detach() for k in ("eval_cond_ll", "eval_prior_dist", "eval_inference_dist"))
    logw = ll - klw * (logq - logp)
    assert float((-(torch.logsumexp(logw.double(), 1) - math.log(ns)) - loss.detach().double()).abs().max()) < 1e-4 * float(loss.abs().max())
    with torch.no_grad():
        mu, logvar = vae.encoder.forward(x)
        kl = 0.5 * (mu.pow(2) + logvar.exp() - logvar - 1).sum(dim=1)
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in vae.named_parameters()}
    assert all(p.grad is not None for p in vae.parameters()), "a parameter got no gradient"
    total = float(torch.nn.utils.clip_grad_norm_(vae.parameters(), max_norm))
    if update in ("encoder", "both"):
        enc_opt.step()
    if update in ("decoder", "both"):
        dec_opt.step()
    return dict(loss=loss.detach().clone(), logw=logw.clone(), rec=-ll.mean(dim=1), kl=kl, grads=grads, total=total)


def ref_step(vae, cap, tap, x, klw, ns, noise_seed, enc_opt, dec_opt, update, max_norm=CLIP):
    torch.manual_seed(noise_seed)
    r = run_step(vae, tap, x, klw, ns, enc_opt, dec_opt, update, max_norm)
    eps_c, m_in, m_out = cap.noise()
    B, Td = x.shape[0], x.shape[1] - 1
    assert tuple(eps_c.shape[:2]) == (B, ns) and tuple(m_in.shape[:2]) == (B, Td) and tuple(m_out.shape[:2]) == (B * ns, Td)
    eps = MG.replay_eps(noise_seed, B, eps_c.shape[-1], ns)
    assert float((eps - eps_c).abs().max()) < 1e-4, "eps is not the first draw after the seed"
    assert torch.equal(cap.cap["mu"].unsqueeze(1) + eps * cap.cap["std"].unsqueeze(1), cap.cap["z"])
    r["noise"] = (eps, m_in.clone(), m_out.clone())
    return r


class FixedMask(torch.nn.Module):
    def __init__(self, keep, p):
        super().__init__()
        self.keep, self.p = keep, p

    def forward(self, t):
        assert tuple(t.shape) == tuple(self.keep.shape), (t.shape, self.keep.shape)
        return t * self.keep.to(t.dtype) / (1.0 - self.p)


def float64_step(build_fn, P0, x, klw, ns, noise, update, max_norm):
    """The same step in float64 on the same weights with the same noise injected -> run_step's dict, and the model."""
    vae = build_fn().double()
    vae.load_state_dict(P0)
    vae.train()
    eps, m_in, m_out = noise
    vae.decoder.dropout_in = FixedMask(m_in, vae.decoder.dropout_in.p)
    vae.decoder.dropout_out = FixedMask(m_out, vae.decoder.dropout_out.p)
    vae.encoder.reparameterize = lambda mu, logvar, nsamples=1: mu.unsqueeze(1) + eps.double() * (0.5 * logvar).exp().unsqueeze(1)
    tap = Tap(vae)
    enc_opt = torch.optim.SGD(vae.encoder.parameters(), lr=1.0, momentum=0)
    dec_opt = torch.optim.SGD(vae.decoder.parameters(), lr=1.0, momentum=0)
    return run_step(vae, tap, x, klw, ns, enc_opt, dec_opt, update, max_norm), vae


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-300))


def pair_delta(a, b):
    """largest error of a within-sentence difference log w_s - log w_s'"""
    d = a.double() - b.double()
    return float((d.unsqueeze(2) - d.unsqueeze(1)).abs().max())


def check_float64(tag, r32, r64, new32, new64, ns):
    rec_scale = float(r64["rec"].abs().max())
    e = dict(loss=rel(r32["loss"], r64["loss"]), rec=rel(r32["rec"], r64["rec"]), logw=float((r32["logw"].double() - r64["logw"]).abs().max()),
             delta=pair_delta(r32["logw"], r64["logw"]), norm=abs(r32["total"] - r64["total"]) / r64["total"])
    e["kl"] = float((r32["kl"].double() - r64["kl"]).abs().max())
    e["grads"] = max(rel(r32["grads"][k], r64["grads"][k]) for k in r64["grads"] if float(r64["grads"][k].abs().max()) > 0)
    e["w"] = max(rel(new32[k], new64[k]) for k in new64)
    print("  f32 vs float64 %-14s " % tag + " ".join("%s %.1e" % kv for kv in e.items()))
    assert e["loss"] < RTOL and e["rec"] < RTOL and e["norm"] < RTOL and e["w"] < RTOL, (tag, e)
    assert e["kl"] < RTOL * float(r64["kl"].abs().max()) + 1e-6 * (1 + rec_scale), (tag, e)
    assert e["logw"] < RTOL * rec_scale and e["delta"] < RTOL * rec_scale, (tag, e)
    assert e["grads"] < GRAD_RTOL + 2 * e["delta"], (tag, e)


def check_weights_spread(tag, logw, ns):
    wn = torch.softmax(logw.double(), dim=1)
    top = wn.max(dim=1).values
    print("  %s: max_s wn per sentence %s" % (tag, [round(float(t), 3) for t in top]))
    if ns > 1:
        assert int((top < 0.9).sum()) * 2 >= top.numel(), (tag, "the weights are not exercised", top)


def small_case(out, tag, V, ni, H, nz, B, T, ns, klw, model_seed, noise_seed, data_seed, model_scale=0.01, emb_scale=0.1,
               head_scale=None, force_last_token=False, want_clip=None, max_norm=CLIP):
    from oracle import text_vae_oracle as O
    print("case", tag)
    build_fn = lambda: MS.build(V, ni, H, nz, model_seed, model_scale, emb_scale, head_scale)
    vae = build_fn()
    x = O.synthetic_batch(B, T, V, seed=data_seed)
    if force_last_token:
        x[0, 1 if T > 2 else 0] = V - 1          # decoder INPUT token V-1 -> zero embedding gradient row
    P0 = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    cap, tap = MG.NoiseCapture(vae), Tap(vae)
    enc_opt = torch.optim.SGD(vae.encoder.parameters(), lr=1.0, momentum=0)
    dec_opt = torch.optim.SGD(vae.decoder.parameters(), lr=1.0, momentum=0)
    r = ref_step(vae, cap, tap, x, klw, ns, noise_seed, enc_opt, dec_opt, "encoder", max_norm)
    new_enc = {k: v.detach().clone() for k, v in vae.state_dict().items() if k.startswith("encoder.")}
    for k in O.DEC_KEYS:
        assert torch.equal(vae.state_dict()[k], P0[k])
    r64, vae64 = float64_step(build_fn, P0, x, klw, ns, r["noise"], "encoder", max_norm)
    check_float64(tag, r, r64, new_enc, {k: vae64.state_dict()[k] for k in new_enc}, ns)
    check_weights_spread(tag, r["logw"], ns)
    total = r["total"]
    coef = min(1.0, max_norm / (total + 1e-6))
    if want_clip is not None:
        assert (coef < 1.0) == want_clip, (tag, total, coef)
    eps, m_in, m_out = r["noise"]
    d = dict(V=V, ni=ni, H=H, nz=nz, B=B, T=T, ns=ns, kl_weight=np.float32(klw), max_norm=np.float64(max_norm), x=x.numpy(),
             eps=eps.numpy(), mask_in=m_in.numpy().astype(np.uint8), mask_out=m_out.numpy().astype(np.uint8), loss=r["loss"].numpy(),
             logw=r["logw"].numpy(), rec=r["rec"].numpy(), kl=r["kl"].numpy(), total_norm=np.float64(total), coef=np.float64(coef))
    for k in O.ALL_KEYS:
        d["param/" + k] = P0[k].numpy()
        d["grad/" + k] = r["grads"][k].numpy()
    for k in O.ENC_KEYS:
        d["new/" + k] = new_enc[k].numpy()
    for k, v in d.items():
        out[tag + "/" + k] = v
    print("  %s: loss %.4f kl %.3e norm %.4f coef %.4f" % (tag, float(r["loss"].mean()), float(r["kl"].mean()), total, coef))


def small_trajectory(out, tag, V, ni, H, nz, B, T, ns, klw, model_seed, data_seed, model_scale, head_scale, updates):
    """Consecutive steps, each on the weights the previous one left; the float64 twin runs its own trajectory on the same noise."""
    from oracle import text_vae_oracle as O
    print("trajectory", tag)
    build_fn = lambda: MS.build(V, ni, H, nz, model_seed, model_scale, 0.1, head_scale)
    vae = build_fn()
    xs = [O.synthetic_batch(B, T, V, seed=data_seed + i) for i in range(len(updates))]
    P0 = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    cap, tap = MG.NoiseCapture(vae), Tap(vae)
    enc_opt = torch.optim.SGD(vae.encoder.parameters(), lr=1.0, momentum=0)
    dec_opt = torch.optim.SGD(vae.decoder.parameters(), lr=1.0, momentum=0)
    P64 = {k: v.double() for k, v in P0.items()}
    rows = []
    for it, up in enumerate(updates):
        r = ref_step(vae, cap, tap, xs[it], klw, ns, 7100 + it, enc_opt, dec_opt, up)
        r64, vae64 = float64_step(build_fn, P64, xs[it], klw, ns, r["noise"], up, CLIP)
        P64 = {k: v.detach().clone() for k, v in vae64.state_dict().items()}
        assert rel(r["loss"], r64["loss"]) < RTOL and abs(r["total"] - r64["total"]) / r64["total"] < RTOL
        check_weights_spread("%s[%d]" % (tag, it), r["logw"], ns)
        rows.append(r)
    final = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    err = max(rel(final[k], P64[k]) for k in O.ALL_KEYS)
    print("  f32 vs float64 %s: final weights %.1e" % (tag, err))
    assert err < RTOL
    d = dict(V=V, ni=ni, H=H, nz=nz, B=B, T=T, ns=ns, kl_weight=np.float32(klw), max_norm=np.float64(CLIP), updates=np.array(updates),
             x=np.stack([x.numpy() for x in xs]), loss=np.stack([r["loss"].numpy() for r in rows]),
             logw=np.stack([r["logw"].numpy() for r in rows]), rec=np.stack([r["rec"].numpy() for r in rows]),
             kl=np.stack([r["kl"].numpy() for r in rows]), total_norm=np.array([r["total"] for r in rows]),
             eps=np.stack([r["noise"][0].numpy() for r in rows]), mask_in=np.stack([r["noise"][1].numpy().astype(np.uint8) for r in rows]),
             mask_out=np.stack([r["noise"][2].numpy().astype(np.uint8) for r in rows]))
    for k in O.ALL_KEYS:
        d["param/" + k] = P0[k].numpy()
        d["final/" + k] = final[k].numpy()
    for k, v in d.items():
        out[tag + "/" + k] = v
    print("  %s: losses %s" % (tag, [round(float(r["loss"].mean()), 4) for r in rows]))


CASES = ["ns2_wide_clip", "ns3_T2", "ns4_mid", "ns4_refinit", "ns1"]


def make_small():
    out = {}
    # the shapes and seeds of make_golden_multisample.py's cases.  ns = 2, B not a multiple of 4, wide weights (at that script's
    # model_scale 0.9 one sample takes the whole weight in four of five sentences: 0.5 here); the gradient norm was measured at 2.71,
    # so the clip threshold of this case is 1.5 -> the clip is ACTIVE; decoder input token V-1
    small_case(out, "ns2_wide_clip", V=53, ni=8, H=16, nz=4, B=5, T=7, ns=2, klw=1.0, model_seed=112, noise_seed=122, data_seed=132,
               model_scale=0.5, emb_scale=1.0, head_scale=0.6, force_last_token=True, want_clip=True, max_norm=1.5)
    # ns = 3, T = 2 (a single decoder timestep), B = 3, odd sizes, KL weight 0.1: the composed form
    small_case(out, "ns3_T2", V=37, ni=6, H=10, nz=3, B=3, T=2, ns=3, klw=0.1, model_seed=113, noise_seed=123, data_seed=133,
               model_scale=0.3, head_scale=0.4, force_last_token=True)
    # ns = 4, mid-size, the reference's nll_iw itself
    small_case(out, "ns4_mid", V=211, ni=16, H=32, nz=8, B=6, T=12, ns=4, klw=1.0, model_seed=114, noise_seed=124, data_seed=134,
               model_scale=0.3, emb_scale=0.5, head_scale=0.5, want_clip=False)
    # ns = 4 at the reference init (the weights differ through the dropout masks alone)
    small_case(out, "ns4_refinit", V=53, ni=8, H=16, nz=4, B=4, T=7, ns=4, klw=0.1, model_seed=115, noise_seed=125, data_seed=135)
    # ns = 1: the single-sample Monte-Carlo ELBO
    small_case(out, "ns1", V=53, ni=8, H=16, nz=4, B=5, T=7, ns=1, klw=0.37, model_seed=117, noise_seed=127, data_seed=137,
               model_scale=0.3, head_scale=0.5)
    small_trajectory(out, "traj_ns2", V=53, ni=8, H=16, nz=4, B=5, T=7, ns=2, klw=0.6, model_seed=116, data_seed=136,
                     model_scale=0.2, head_scale=0.5, updates=["encoder", "encoder", "both"])
    out["cases"] = np.array(CASES)
    np.savez_compressed(os.path.join(HERE, "text_iw_small.npz"), **out)
    print("wrote text_iw_small.npz")


def make_wide(name="text_iw_h1024_b8_t50", B=8, T=50, ns=4, V=20001, ni=512, H=1024, nz=32, klw=0.5, model_seed=783435, noise_seed=131,
              data_seed=141, model_scale=0.05, emb_scale=0.1, head_scale=0.2, pred_scale=0.3):
    """As make_golden_multisample.make_wide stores its cases, with log w added."""
    from oracle import text_vae_oracle as O
    print("case", name)
    vae = MS.build(V, ni, H, nz, model_seed, model_scale, emb_scale, head_scale, pred_scale)
    x = O.synthetic_batch(B, T, V, seed=data_seed)
    P0 = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    cap, tap = MG.NoiseCapture(vae), Tap(vae)
    enc_opt = torch.optim.SGD(vae.encoder.parameters(), lr=1.0, momentum=0)
    dec_opt = torch.optim.SGD(vae.decoder.parameters(), lr=1.0, momentum=0)
    r = ref_step(vae, cap, tap, x, klw, ns, noise_seed, enc_opt, dec_opt, "encoder")
    check_weights_spread(name, r["logw"], ns)
    new_enc = {k: v.detach().clone() for k, v in vae.state_dict().items() if k.startswith("encoder.")}
    grads, total = r["grads"], r["total"]
    eps, m_in, m_out = r["noise"]
    coef = min(1.0, CLIP / (total + 1e-6))
    total64 = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads.values()))
    out = dict(V=V, ni=ni, H=H, nz=nz, B=B, T=T, ns=ns, kl_weight=np.float32(klw), model_seed=model_seed, total_norm64=np.float64(total64),
               noise_seed=noise_seed, model_scale=model_scale, emb_scale=emb_scale, head_scale=np.float64(head_scale),
               pred_scale=np.float64(pred_scale), x=x.numpy(), eps=eps.numpy(),
               mask_in_bits=np.packbits(m_in.numpy().astype(np.uint8)), mask_in_shape=np.array(m_in.shape),
               mask_out_bits=np.packbits(m_out.numpy().astype(np.uint8)), mask_out_shape=np.array(m_out.shape),
               loss=r["loss"].numpy(), logw=r["logw"].numpy(), rec=r["rec"].numpy(), kl=r["kl"].numpy(), total_norm=np.float64(total),
               coef=np.float64(coef))
    g = torch.Generator().manual_seed(1234)
    for k in O.ALL_KEYS:
        out["gradnorm/" + k] = np.float64(grads[k].double().norm())
        idx = torch.randint(0, P0[k].numel(), (64,), generator=g)
        out["sample_idx/" + k] = idx.numpy()
        out["sample_grad/" + k] = grads[k].reshape(-1)[idx].numpy()
        out["sample_param/" + k] = P0[k].reshape(-1)[idx].numpy()
        if k in new_enc:
            out["sample_new/" + k] = new_enc[k].reshape(-1)[idx].numpy()
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **out)
    print("  wrote %s.npz  loss %.4f kl %.3e norm %.4f (f64 %.4f) coef %.4f" % (name, float(r["loss"].mean()), float(r["kl"].mean()), total, total64, coef))


def main():
    if "--wide" not in sys.argv:
        make_small()
    if "--small" not in sys.argv:
        make_wide()


if __name__ == "__main__":
    main()

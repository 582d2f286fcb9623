"""Generate the multi-sample (text.py --nsamples N) fixtures by RUNNING THE REFERENCE (imported the way
make_golden.py imports it: make_golden.REF).

    python tests/golden/make_golden_multisample.py [--small | --wide NAME]     # writes tests/golden/text_ms_*.npz (or $GOLDEN_OUT)

Each case runs one body of the aggressive loop exactly as text.py:373-387 does with `vae.loss(x, kl_weight, nsamples=ns)`,
records the random draws the call consumed (make_golden.NoiseCapture: eps (B, ns, nz), mask_in (B, T-1, ni) -- dropout_in acts
before the expansion over the samples --, mask_out (B*ns, T-1, H)) and, before anything is written, asserts the unchanged CPU
oracle (oracle/text_vae_oracle.py carries ns end to end) against the reference at make_golden.check_oracle's bounds.

  text_ms_small.npz           fully materialised small cases ("<case>/<field>"), ns in {2, 3, 4}, and a 3-step trajectory
  text_ms_h1024_b8.npz        V=20001 ni=512 H=1024 nz=32, B=8,  ns=4, T=200: weights regenerated from the seed on the test side
  text_ms_h1024_b32_t50.npz   the same model,              B=32, ns=4, T=50  (128 decoder rows)
The keep-masks of the wide cases are stored as packed bits ("mask_*_bits" + "mask_*_shape").
"""
import math
import os
import sys

import numpy as np
import torch

SRC = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, SRC)
import make_golden as MG  # noqa: E402

HERE = MG.HERE
CLIP = 5.0


def check_oracle(tag, P, x, klw, eps, m_in, m_out, loss, rec, kl, grads, total, new_enc, max_norm):
    """make_golden.check_oracle -- the same quantities at the same bounds -- for a clip threshold other than 5.0."""
    from oracle import text_vae_oracle as O
    for impl in ("explicit", "aten"):
        r = O.inner_step(P, x, klw, eps, m_in, m_out, lr=1.0, clip=max_norm, impl=impl)

        def rel(a, b):
            return float((a - b).abs().max() / (b.abs().max() + 1e-30))
        e = [rel(r["loss"], loss), rel(r["rec"], rec)]
        ekl = float((r["kl"] - kl).abs().max() / (kl.abs().max() + 1e-6 * (1 + float(rec.abs().max()))))
        eg = max(rel(r["grads"][k], grads[k]) for k in O.ALL_KEYS if float(grads[k].abs().max()) > 0)
        en = abs(r["total_norm"] - total) / total
        ew = max(rel(r["new_params"][k], new_enc[k]) for k in O.ENC_KEYS)
        print("  oracle[%s] vs reference %-14s loss %.1e rec %.1e kl %.1e grads %.1e norm %.1e w %.1e" % (impl, tag, e[0], e[1], ekl, eg, en, ew))
        assert max(e) < 2e-5 and ekl < 1e-4 and eg < 1e-3 and en < 1e-4 and ew < 1e-4, "oracle != reference"


def ref_step(vae, cap, x, klw, ns, noise_seed, enc_opt, dec_opt, update, max_norm=CLIP):
    """text.py:373-387 with nsamples = ns (update 'both': the joint step once aggressive training has ended, text.py:418-424)."""
    enc_opt.zero_grad()
    dec_opt.zero_grad()
    torch.manual_seed(noise_seed)
    loss, rec, kl = vae.loss(x, klw, nsamples=ns)
    loss.mean(dim=-1).backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in vae.named_parameters()}
    total = float(torch.nn.utils.clip_grad_norm_(vae.parameters(), max_norm))
    if update in ("encoder", "both"):
        enc_opt.step()
    if update in ("decoder", "both"):
        dec_opt.step()
    eps_c, m_in, m_out = cap.noise()
    B, Td = x.shape[0], x.shape[1] - 1
    assert tuple(eps_c.shape[:2]) == (B, ns) and tuple(m_in.shape[:2]) == (B, Td) and tuple(m_out.shape[:2]) == (B * ns, Td)
    eps = MG.replay_eps(noise_seed, B, eps_c.shape[-1], ns)
    assert float((eps - eps_c).abs().max()) < 1e-4, "eps is not the first draw after the seed"
    assert torch.equal(cap.cap["mu"].unsqueeze(1) + eps * cap.cap["std"].unsqueeze(1), cap.cap["z"])
    return loss.detach(), rec.detach(), kl.detach(), grads, total, (eps, m_in.clone(), m_out.clone())


def build(V, ni, H, nz, model_seed, model_scale, emb_scale, head_scale, pred_scale=None):
    vae = MG.build_ref_vae(V, ni, H, nz, model_seed, model_scale, emb_scale)
    with torch.no_grad():
        if head_scale is not None:
            vae.encoder.linear.weight.uniform_(-head_scale, head_scale)
        if pred_scale is not None:
            vae.decoder.pred_linear.weight.uniform_(-pred_scale, pred_scale)
    return vae


def small_case(out, tag, V, ni, H, nz, B, T, ns, klw, model_seed, noise_seed, data_seed, model_scale=0.01, emb_scale=0.1,
               head_scale=None, force_last_token=False, want_clip=None, max_norm=CLIP):
    from oracle import text_vae_oracle as O
    print("case", tag)
    vae = build(V, ni, H, nz, model_seed, model_scale, emb_scale, head_scale)
    x = O.synthetic_batch(B, T, V, seed=data_seed)
    if force_last_token:
        x[0, 1 if T > 2 else 0] = V - 1          # decoder INPUT token V-1 -> zero embedding gradient row (G3)
    P0 = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    cap = MG.NoiseCapture(vae)
    enc_opt = torch.optim.SGD(vae.encoder.parameters(), lr=1.0, momentum=0)
    dec_opt = torch.optim.SGD(vae.decoder.parameters(), lr=1.0, momentum=0)
    loss, rec, kl, grads, total, (eps, m_in, m_out) = ref_step(vae, cap, x, klw, ns, noise_seed, enc_opt, dec_opt, "encoder", max_norm)
    new_enc = {k: v.detach().clone() for k, v in vae.state_dict().items() if k.startswith("encoder.")}
    for k in O.DEC_KEYS:
        assert torch.equal(vae.state_dict()[k], P0[k])
    check_oracle(tag, P0, x, klw, eps, m_in, m_out, loss, rec, kl, grads, total, new_enc, max_norm)
    coef = min(1.0, max_norm / (total + 1e-6))
    if want_clip is not None:
        assert (coef < 1.0) == want_clip, (tag, total, coef)
    d = dict(V=V, ni=ni, H=H, nz=nz, B=B, T=T, ns=ns, kl_weight=np.float32(klw), max_norm=np.float64(max_norm), x=x.numpy(),
             eps=eps.numpy(), mask_in=m_in.numpy().astype(np.uint8), mask_out=m_out.numpy().astype(np.uint8), loss=loss.numpy(),
             rec=rec.numpy(), kl=kl.numpy(), total_norm=np.float64(total), coef=np.float64(coef))
    for k in O.ALL_KEYS:
        d["param/" + k] = P0[k].numpy()
        d["grad/" + k] = grads[k].numpy()
    for k in O.ENC_KEYS:
        d["new/" + k] = new_enc[k].numpy()
    for k, v in d.items():
        out[tag + "/" + k] = v
    print("  %s: loss %.4f kl %.3e norm %.4f coef %.4f" % (tag, float(loss.mean()), float(kl.mean()), total, coef))


def small_trajectory(out, tag, V, ni, H, nz, B, T, ns, klw, model_seed, data_seed, model_scale, head_scale, updates):
    """Consecutive steps, each on the weights the previous one left: `updates` = the side each step moves."""
    from oracle import text_vae_oracle as O
    print("trajectory", tag)
    vae = build(V, ni, H, nz, model_seed, model_scale, 0.1, head_scale)
    xs = [O.synthetic_batch(B, T, V, seed=data_seed + i) for i in range(len(updates))]
    P0 = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    cap = MG.NoiseCapture(vae)
    enc_opt = torch.optim.SGD(vae.encoder.parameters(), lr=1.0, momentum=0)
    dec_opt = torch.optim.SGD(vae.decoder.parameters(), lr=1.0, momentum=0)
    P = {k: v.clone() for k, v in P0.items()}
    rows = []
    for it, up in enumerate(updates):
        loss, rec, kl, grads, total, (e, mi, mo) = ref_step(vae, cap, xs[it], klw, ns, 7000 + it, enc_opt, dec_opt, up)
        r = O.inner_step(P, xs[it], klw, e, mi, mo, update=up)
        P.update(r["new_params"])
        assert abs(float(r["loss"].sum() - loss.sum())) / abs(float(loss.sum())) < 2e-5
        assert abs(r["total_norm"] - total) / total < 1e-4
        rows.append((loss.numpy(), rec.numpy(), kl.numpy(), total, e.numpy(), mi.numpy().astype(np.uint8), mo.numpy().astype(np.uint8)))
    final = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    for k in O.ALL_KEYS:
        err = float((P[k] - final[k]).abs().max() / final[k].abs().max())
        assert err < 1e-4, (k, err)
    d = dict(V=V, ni=ni, H=H, nz=nz, B=B, T=T, ns=ns, kl_weight=np.float32(klw), max_norm=np.float64(CLIP), updates=np.array(updates),
             x=np.stack([x.numpy() for x in xs]), loss=np.stack([r[0] for r in rows]), rec=np.stack([r[1] for r in rows]),
             kl=np.stack([r[2] for r in rows]), total_norm=np.array([r[3] for r in rows]), eps=np.stack([r[4] for r in rows]),
             mask_in=np.stack([r[5] for r in rows]), mask_out=np.stack([r[6] for r in rows]))
    for k in O.ALL_KEYS:
        d["param/" + k] = P0[k].numpy()
        d["final/" + k] = final[k].numpy()
    for k, v in d.items():
        out[tag + "/" + k] = v
    print("  %s: losses %s" % (tag, [round(float(r[0].mean()), 4) for r in rows]))


def make_small():
    out = {}
    # ns = 2, B not a multiple of 4, wide weights: KL O(1); the gradient norm was measured at 4.21, so the clip threshold of this
    # case is 3.0 -> the clip is ACTIVE (coef 0.71); decoder input token V-1
    small_case(out, "ns2_wide_clip", V=53, ni=8, H=16, nz=4, B=5, T=7, ns=2, klw=1.0, model_seed=112, noise_seed=122, data_seed=132,
               model_scale=0.9, emb_scale=1.0, head_scale=0.6, force_last_token=True, want_clip=True, max_norm=3.0)
    # ns = 3, T = 2 (a single decoder timestep), B = 3, odd sizes
    small_case(out, "ns3_T2", V=37, ni=6, H=10, nz=3, B=3, T=2, ns=3, klw=0.1, model_seed=113, noise_seed=123, data_seed=133,
               model_scale=0.3, head_scale=0.4, force_last_token=True)
    # ns = 4, mid-size
    small_case(out, "ns4_mid", V=211, ni=16, H=32, nz=8, B=6, T=12, ns=4, klw=1.0, model_seed=114, noise_seed=124, data_seed=134,
               model_scale=0.3, emb_scale=0.5, head_scale=0.5, want_clip=False)
    # ns = 4 at the reference init (KL ~ 1e-5: the conditioning case, compared with an absolute floor)
    small_case(out, "ns4_refinit", V=53, ni=8, H=16, nz=4, B=4, T=7, ns=4, klw=0.1, model_seed=115, noise_seed=125, data_seed=135)
    small_trajectory(out, "traj_ns2", V=53, ni=8, H=16, nz=4, B=5, T=7, ns=2, klw=0.6, model_seed=116, data_seed=136,
                     model_scale=0.2, head_scale=0.5, updates=["encoder", "encoder", "both"])
    out["cases"] = np.array(["ns2_wide_clip", "ns3_T2", "ns4_mid", "ns4_refinit"])
    np.savez_compressed(os.path.join(HERE, "text_ms_small.npz"), **out)
    print("wrote text_ms_small.npz")


def make_wide(name, B, T, ns=4, V=20001, ni=512, H=1024, nz=32, klw=0.5, model_seed=783435, noise_seed=127, data_seed=138,
              model_scale=0.05, emb_scale=0.1, head_scale=0.2, pred_scale=0.3):
    """As make_golden.make_case(store_params=False) stores text_yahoo_seeded.npz, with ns samples per sentence."""
    from oracle import text_vae_oracle as O
    print("case", name)
    vae = build(V, ni, H, nz, model_seed, model_scale, emb_scale, head_scale, pred_scale)
    x = O.synthetic_batch(B, T, V, seed=data_seed)
    P0 = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    cap = MG.NoiseCapture(vae)
    enc_opt = torch.optim.SGD(vae.encoder.parameters(), lr=1.0, momentum=0)
    dec_opt = torch.optim.SGD(vae.decoder.parameters(), lr=1.0, momentum=0)
    loss, rec, kl, grads, total, (eps, m_in, m_out) = ref_step(vae, cap, x, klw, ns, noise_seed, enc_opt, dec_opt, "encoder")
    new_enc = {k: v.detach().clone() for k, v in vae.state_dict().items() if k.startswith("encoder.")}
    MG.check_oracle(name, P0, x, klw, eps, m_in, m_out, loss, rec, kl, grads, total, new_enc, norm_tol=5e-3)
    coef = min(1.0, CLIP / (total + 1e-6))
    total64 = math.sqrt(sum(float(g.double().pow(2).sum()) for g in grads.values()))
    out = dict(V=V, ni=ni, H=H, nz=nz, B=B, T=T, ns=ns, kl_weight=np.float32(klw), model_seed=model_seed, total_norm64=np.float64(total64),
               noise_seed=noise_seed, model_scale=model_scale, emb_scale=emb_scale, head_scale=np.float64(head_scale),
               pred_scale=np.float64(pred_scale), x=x.numpy(), eps=eps.numpy(),
               mask_in_bits=np.packbits(m_in.numpy().astype(np.uint8)), mask_in_shape=np.array(m_in.shape),
               mask_out_bits=np.packbits(m_out.numpy().astype(np.uint8)), mask_out_shape=np.array(m_out.shape),
               loss=loss.numpy(), rec=rec.numpy(), kl=kl.numpy(), total_norm=np.float64(total), coef=np.float64(coef))
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
    print("  wrote %s.npz  loss %.4f kl %.3e norm %.4f (f64 %.4f) coef %.4f" % (name, float(loss.mean()), float(kl.mean()), total, total64, coef))


WIDE = {
    "text_ms_h1024_b8": lambda: make_wide("text_ms_h1024_b8", B=8, T=200),               # 32 decoder rows: 4 per XCD group
    "text_ms_h1024_b32_t50": lambda: make_wide("text_ms_h1024_b32_t50", B=32, T=50, noise_seed=129, data_seed=139),   # 128 rows
}


def main():
    if "--wide" in sys.argv:
        return WIDE[sys.argv[sys.argv.index("--wide") + 1]]()
    make_small()
    if "--small" not in sys.argv:
        for fn in WIDE.values():
            fn()


if __name__ == "__main__":
    main()

"""Generate tests/golden/varlen_small.npz by RUNNING THE REFERENCE's VarLSTMEncoder / VarLSTMDecoder (enc_lstm.py:77-126,
dec_lstm.py:370-476; imported unmodified the way make_golden.py imports the reference: make_golden.REF).

    python tests/golden/make_golden_varlen.py          # writes tests/golden/varlen_small.npz (or $GOLDEN_OUT)

Each case runs `vae.loss((x, sents_len), kl_weight, nsamples=ns)` and `loss.mean().backward()` in train mode on a padded batch
(x[b, len_b:] = <pad>, lengths sorted in decreasing order with max == T, as the reference demands) and records
  * the state_dict, x, the lengths, and the random draws the call consumed: eps (B, ns, nz) -- the first draw after the seed,
    replayed bit-exactly --, mask_in (B, T-1, ni), mask_out (B*ns, T-1, H).  The keep-masks are read off the
    dropout modules' outputs; dropout_out is fed pad_packed_sequence's exact zeros at the padded positions, where a keep-mask
    cannot be read off and does not matter: those entries are stored as 1;
  * loss, rec, kl, mu, logvar and the 13 gradients;
  * in eval mode, log_probability((x, lens), z) and eval_inference_dist((x, lens), z) at a recorded z (B, 3, nz).
Before anything is written every case is checked against the reference's EQUAL-LENGTH classes on each sentence cut to its own
length (dropout off): rec, mu, logvar row by row.

"init/*": the weights the two reference classes get from one seed (the decoder builds its parent, replaces `embed`, and runs
reset_parameters a second time).
"""
import argparse
import os
import sys

import numpy as np
import torch

SRC = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, SRC)
import make_golden as MG  # noqa: E402

HERE = MG.HERE
PAD, BOS, EOS = 0, 1, 2


def build_ref_var_vae(V, ni, H, nz, model_seed, model_scale=0.01, emb_scale=0.1, p_in=0.5, p_out=0.5):
    ref = MG.ref_modules()
    args = argparse.Namespace(ni=ni, enc_nh=H, dec_nh=H, nz=nz, dec_dropout_in=p_in, dec_dropout_out=p_out,
                              device=torch.device("cpu"))
    torch.manual_seed(model_seed)
    enc = ref.VarLSTMEncoder(args, V, MG.uniform_initializer(model_scale), MG.uniform_initializer(emb_scale))
    dec = ref.VarLSTMDecoder(args, MG.Vocab(V), MG.uniform_initializer(model_scale), MG.uniform_initializer(emb_scale))
    vae = ref.VAE(enc, dec, args)
    vae.train()
    return vae


def padded_batch(B, T, V, lens, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(4, V, (B, T), generator=g, dtype=torch.int64)
    x[:, 0] = BOS
    for b, n in enumerate(lens):
        x[b, n - 1] = EOS
        x[b, n:] = PAD
    return x


class Capture(object):
    """make_golden.NoiseCapture for a padded batch: dropout_out sees exact zeros at the padded positions (allowed there only)."""

    def __init__(self, vae, lens, ns):
        self.cap = {}
        orig = vae.encoder.reparameterize

        def rp(mu, logvar, nsamples=1):
            z = orig(mu, logvar, nsamples)
            self.cap["z"], self.cap["mu"], self.cap["logvar"] = z.detach().clone(), mu.detach().clone(), logvar.detach().clone()
            return z
        vae.encoder.reparameterize = rp
        steps = torch.tensor(lens) - 1

        def hook_in(m, inp, out):
            if not m.training:
                return
            assert float((inp[0] == 0).float().sum()) == 0, "exact zero fed to dropout_in: mask ambiguous"
            self.cap["mask_in"] = (out != 0).detach().clone()

        def hook_out(m, inp, out):
            if not m.training:
                return
            Td = inp[0].shape[1]
            live = (torch.arange(Td).view(1, Td) < steps.repeat_interleave(ns).view(-1, 1)).unsqueeze(-1)      # [B*ns][Td][1]
            assert float(((inp[0] == 0) & live).float().sum()) == 0, "exact zero at an active position fed to dropout_out"
            assert float(((inp[0] != 0) & ~live).float().sum()) == 0, "pad_packed_sequence left a non-zero padded row"
            self.cap["mask_out"] = ((out != 0) | ~live).detach().clone()
        vae.decoder.dropout_in.register_forward_hook(hook_in)
        vae.decoder.dropout_out.register_forward_hook(hook_out)


def check_against_equal_length(tag, sd, V, ni, H, nz, x, lens, z):
    """The reference's own equal-length classes, sentence by sentence (eval mode): rec, mu, logvar."""
    ref = MG.ref_modules()
    args = argparse.Namespace(ni=ni, enc_nh=H, dec_nh=H, nz=nz, dec_dropout_in=0.5, dec_dropout_out=0.5, device=torch.device("cpu"))
    init = MG.uniform_initializer(0.01)
    torch.manual_seed(0)
    plain = ref.VAE(ref.LSTMEncoder(args, V, init, init), ref.LSTMDecoder(args, MG.Vocab(V), init, init), args)
    plain.load_state_dict(sd, strict=False)
    plain.eval()
    var = build_ref_var_vae(V, ni, H, nz, 0)
    var.load_state_dict(sd, strict=False)
    var.eval()
    L = torch.tensor(lens, dtype=torch.int64)
    with torch.no_grad():
        mu_v, lv_v = var.encoder((x, L))
        rec_v = var.decoder.reconstruct_error((x, L), z)
        worst = 0.0
        for b, n in enumerate(lens):
            xb = x[b:b + 1, :n]
            mu, lv = plain.encoder(xb)
            rec = plain.decoder.reconstruct_error(xb, z[b:b + 1])
            for got, want in ((mu_v[b:b + 1], mu), (lv_v[b:b + 1], lv), (rec_v[b:b + 1], rec)):
                worst = max(worst, float((got - want).abs().max() / (want.abs().max() + 1e-6)))
    print("  %s: padded classes vs equal-length classes, sentence by sentence: %.1e" % (tag, worst))
    assert worst < 2e-5, worst


def case(out, tag, V, ni, H, nz, B, T, lens, ns, klw, model_seed, noise_seed, data_seed, model_scale=0.01, emb_scale=0.1,
         enc_scale=None, head_scale=None):
    print("case", tag)
    assert len(lens) == B and max(lens) == T and min(lens) >= 2 and sorted(lens, reverse=True) == list(lens)
    vae = build_ref_var_vae(V, ni, H, nz, model_seed, model_scale, emb_scale)
    with torch.no_grad():
        if enc_scale is not None:                      # the "wide" scale: KL O(1)
            for p in vae.encoder.parameters():
                p.uniform_(-enc_scale, enc_scale)
        if head_scale is not None:
            vae.encoder.linear.weight.uniform_(-head_scale, head_scale)
    sd = {k: v.detach().clone() for k, v in vae.state_dict().items()}
    x = padded_batch(B, T, V, lens, data_seed)
    L = torch.tensor(lens, dtype=torch.int64)
    cap = Capture(vae, lens, ns)
    vae.zero_grad()
    torch.manual_seed(noise_seed)
    loss, rec, kl = vae.loss((x, L), klw, nsamples=ns)
    loss.mean(dim=-1).backward()
    grads = {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in vae.named_parameters()}
    assert len(grads) == 13
    assert float(grads["decoder.embed.weight"][PAD].abs().max()) == 0.0
    eps = MG.replay_eps(noise_seed, B, nz, ns)
    mu, logvar = cap.cap["mu"], cap.cap["logvar"]
    assert torch.equal(mu.unsqueeze(1) + eps * (0.5 * logvar).exp().unsqueeze(1), cap.cap["z"]), "eps is not the first draw after the seed"
    m_in, m_out = cap.cap["mask_in"], cap.cap["mask_out"]
    assert tuple(m_in.shape) == (B, T - 1, ni) and tuple(m_out.shape) == (B * ns, T - 1, H)
    # eval-mode quantities at a recorded z
    g = torch.Generator().manual_seed(noise_seed + 1)
    z_eval = torch.randn(B, 3, nz, generator=g)
    vae.eval()
    with torch.no_grad():
        logp = vae.decoder.log_probability((x, L), z_eval)
        logq = vae.encoder.eval_inference_dist((x, L), z_eval)
    check_against_equal_length(tag, sd, V, ni, H, nz, x, lens, z_eval)
    d = dict(V=V, ni=ni, H=H, nz=nz, B=B, T=T, ns=ns, kl_weight=np.float32(klw), x=x.numpy(), lens=np.array(lens, dtype=np.int64),
             eps=eps.numpy(), mask_in=m_in.numpy().astype(np.uint8), mask_out=m_out.numpy().astype(np.uint8),
             loss=loss.detach().numpy(), rec=rec.detach().numpy(), kl=kl.detach().numpy(), mu=mu.numpy(), logvar=logvar.numpy(),
             z_eval=z_eval.numpy(), log_probability=logp.numpy(), eval_inference_dist=logq.numpy())
    for k, v in sd.items():
        if k != "decoder.loss.weight":
            d["param/" + k] = v.numpy()
    for k, v in grads.items():
        d["grad/" + k] = v.numpy()
    for k, v in d.items():
        out[tag + "/" + k] = v
    print("  %s: loss %.4f rec %.4f kl %.3e" % (tag, float(loss.mean()), float(rec.mean()), float(kl.mean())))
    return float(kl.mean())


def init_case(out, V, ni, H, nz, seed, model_scale, emb_scale):
    vae = build_ref_var_vae(V, ni, H, nz, seed, model_scale, emb_scale)
    d = dict(V=V, ni=ni, H=H, nz=nz, seed=seed, model_scale=np.float64(model_scale), emb_scale=np.float64(emb_scale))
    for k, v in vae.state_dict().items():
        if k != "decoder.loss.weight":
            d["param/" + k] = v.detach().numpy()
    assert vae.decoder.embed.padding_idx == PAD and float(vae.decoder.embed.weight[PAD].abs().max()) > 0     # re-initialised row
    for k, v in d.items():
        out["init/" + k] = v


def main():
    out = {}
    case(out, "a_ns1", V=53, ni=8, H=16, nz=4, B=5, T=7, lens=[7, 7, 5, 3, 2], ns=1, klw=1.0, model_seed=211, noise_seed=221,
         data_seed=231, model_scale=0.3, emb_scale=0.5, head_scale=0.4)
    case(out, "b_ns3", V=53, ni=8, H=16, nz=4, B=5, T=7, lens=[7, 7, 5, 3, 2], ns=3, klw=1.0, model_seed=211, noise_seed=222,
         data_seed=231, model_scale=0.3, emb_scale=0.5, head_scale=0.4)
    kl = case(out, "c_wide", V=97, ni=12, H=20, nz=4, B=9, T=11, lens=[11, 11, 9, 9, 9, 6, 4, 2, 2], ns=1, klw=0.7, model_seed=212,
              noise_seed=223, data_seed=232, model_scale=0.3, emb_scale=0.5, enc_scale=0.9, head_scale=0.6)
    assert kl > 0.1, "case c: the KL was meant to be O(1)"
    init_case(out, V=53, ni=8, H=16, nz=4, seed=241, model_scale=0.01, emb_scale=0.1)
    out["cases"] = np.array(["a_ns1", "b_ns3", "c_wide"])
    np.savez_compressed(os.path.join(HERE, "varlen_small.npz"), **out)
    print("wrote varlen_small.npz")


if __name__ == "__main__":
    main()

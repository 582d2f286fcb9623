"""VAE -- drop-in for the reference's modules/vae.py (normal prior) on MI355X.

`loss`, `encode`, `encode_stats` are the hot-path surface; they compose the HIP-backed
encoder / reparam+KL / decoder autograd Functions.  The evaluation helpers keep the reference's method names and
semantics on top of the same HIP forward (nll_iw, eval_*, calc_mi_q: SURVEY.md 8f "next" rows).
"""
import contextlib
import math

import torch
import torch.nn as nn

from .. import _lib
from .. import engine as _eng
from .utils import log_sum_exp

_GENERATORS = {"beam": "beam_search_decode", "greedy": "greedy_decode", "sample": "sample_decode"}


class _IWBoundFn(torch.autograd.Function):
    """(rec_s [B][ns], mulv) -> (loss [B], rec [B]) of the importance-weighted bound (lv_loss_assemble_iw_f32 on T = 1).  z enters as
    data: its gradient through the decoder arrives with rec_s (seeded with g * softmax_s(log w)), the weights' direct dependence on
    z = mu + eps * sigma and on logvar goes straight to mulv (lv_reparam_iw_bwd_f32).
    rs [B][ns] (estimator "dreg"): the forward fills it with r_s = 1 - kl_weight * (1 - wn_s) -- _ScaleSamplesFn, which
    sits on z in front of the decoder, reads it in its backward -- and the direct terms are the doubly-reparameterised ones
    (lv_loss_assemble_dreg_f32; lv_reparam_iwdz_bwd_f32 on dz = 0)."""

    @staticmethod
    def forward(ctx, rec_s, mulv, eps, z, kl, klw, rs=None, hold=None):
        one = torch.ones(mulv.shape[0], dtype=torch.float32, device=mulv.device)
        loss, rec, _, _, _ = _eng.iw_assemble(rec_s, mulv, eps, z, kl, klw, one, rs=rs)
        ctx.save_for_backward(rec_s, mulv, eps, z, kl, klw)
        ctx.dreg = rs is not None
        ctx.hold = hold
        ctx.mark_non_differentiable(rec)
        return loss, rec

    @staticmethod
    def backward(ctx, dloss, drec):
        rec_s, mulv, eps, z, kl, klw = ctx.saved_tensors
        if ctx.dreg:
            # r_s does not depend on the seed: this launch rewrites the forward's values into a buffer of its own
            rs = torch.empty_like(rec_s, memory_format=torch.contiguous_format)
            _, _, rowscale, wz, _ = _eng.iw_assemble(rec_s, mulv, eps, z, kl, klw, dloss, rs=rs)
            hold = ctx.hold
            if hold is not None:
                # a decoder that couples the rows (train-mode BatchNorm): what reaches z is the decoder's backward under the seeds
                # g * u_s = rowscale * r, a pass of its own through the decoder's graph, run here -- before the outer backward walks
                # that graph with the seeds g * wn_s for the decoder's parameters -- and handed to _ScaleSamplesFn
                eng = hold["engine"]
                eng.retain_tape = True
                try:
                    hold["dz"] = torch.autograd.grad(rec_s, hold["zs"], rowscale * rs, retain_graph=True)[0]
                finally:
                    eng.retain_tape = False
            return rowscale, _eng.reparam_iwdz_backward(mulv, eps, torch.zeros_like(eps), wz, rs), None, None, None, None, None, None
        # the same launch with the incoming gradient as seed: rowscale = dloss * wn, wz = kl_weight * rowscale
        _, _, rowscale, wz, _ = _eng.iw_assemble(rec_s, mulv, eps, z, kl, klw, dloss)
        return rowscale, _eng.reparam_iw_backward(mulv, eps, wz), None, None, None, None, None, None


class _ScaleSamplesFn(torch.autograd.Function):
    """Identity on z [B][ns][nz]; the backward multiplies the gradient of sample s by rs[b][s], read when the backward runs (the
    doubly-reparameterised estimator: only what flows from z into (mu, logvar) is rescaled, the decoder's parameters see the
    unscaled seeds)."""

    @staticmethod
    def forward(ctx, z, rs, hold=None):
        ctx.rs, ctx.hold = rs, hold
        return z.view_as(z)

    @staticmethod
    def backward(ctx, dz):
        if ctx.hold is not None:              # a row-coupling decoder: dz under the seeds g * u_s, made by _IWBoundFn.backward
            return ctx.hold.pop("dz"), None, None
        return dz * ctx.rs.unsqueeze(-1), None, None


class _SAVAEFn(torch.autograd.Function):
    """(lambda_0 = mulv, decoder parameters) -> (loss [B], rec [B], kl [B]) at the refined lambda_K of VAE.loss_savae.  `route` is
    the decoder engine (fused: engine.LSTMDecoderEngine.savae_forward / savae_backward) or a _SAVAEGeneric; the backward returns
    the gradient with respect to lambda_0 -- the encoder's backward continues from it -- and the decoder's parameters."""

    @staticmethod
    def forward(ctx, route, cfg, x, mulv, eps, mask_in, mask_out, *params):
        p_in, p_out, steps, lr, momentum, clip, fd_eps, kl_weight = cfg
        st = route.savae_forward(x, mulv, eps, mask_in, mask_out, p_in, p_out, steps, lr, momentum, clip, kl_weight)
        ctx.route, ctx.st, ctx.fd_eps = route, st, fd_eps
        loss = st.rec + kl_weight * st.kl
        rec, kl = st.rec.clone(), st.kl.clone()
        ctx.mark_non_differentiable(rec, kl)
        return loss, rec, kl

    @staticmethod
    def backward(ctx, dloss, drec, dkl):
        route = ctx.route
        if isinstance(route, _eng.LSTMDecoderEngine):
            route.flat.before_autograd_backward()
            dmulv = route.savae_backward(ctx.st, dloss, ctx.fd_eps)
            _eng.check_persistent_status(route)
            grads = route.flat.deliver_grads()
        else:
            dmulv, grads = route.savae_backward(ctx.st, dloss, ctx.fd_eps)
        return (None, None, None, dmulv, None, None, None) + tuple(grads)


class _SAVAEGeneric(object):
    """Route "generic" of VAE.loss_savae: csrc/lv_savae.hip's definition over decoder.reconstruct_error and torch.autograd.grad,
    with the same three small kernels for the per-sentence arithmetic (as VAE._svi_generic does for the refinement)."""

    def __init__(self, vae):
        self.vae = vae

    def _pass(self, x, z, masks, seeds, params):
        """reconstruct_error at z under the step's masks, differentiated with the row seeds -> (rec_s, dz, parameter gradients)."""
        with torch.enable_grad():
            z = z.detach().requires_grad_(True)
            rec_s = self.vae.decoder.reconstruct_error(x, z, masks=masks)
            g = torch.autograd.grad(rec_s, [z] + params, seeds.view_as(rec_s))
        return rec_s.detach(), g[0].contiguous(), list(g[1:])

    def savae_forward(self, x, mulv, eps, mask_in, mask_out, p_in, p_out, steps, lr, momentum, clip, kl_weight):
        dev = x.device
        lib, s = _eng.backend_for(dev), _eng.stream_ptr(dev)
        P = _eng.P
        B, ns, nz = eps.shape
        f32 = dict(dtype=torch.float32, device=dev)
        st = _eng._NS()
        lam = mulv.detach().float().contiguous().clone()
        st.g_rec, st.lam_rec = torch.empty(steps, B, 2 * nz, **f32), torch.empty(steps, B, 2 * nz, **f32)
        st.klw = torch.full((1,), float(kl_weight), **f32)
        st.masks = (mask_in, mask_out)
        vel = torch.zeros(B, 2 * nz, **f32)
        z_next, kl_next = torch.empty(B, ns, nz, **f32), torch.empty(B, **f32)
        row = torch.full((B, ns), 1.0 / ns, **f32)
        st.rec0 = st.kl0 = None
        with self.vae._decoder_gradients_preserved(dev):
            for k in range(steps):
                z, kl = _eng.reparam_kl_forward(lam, eps)
                rec_s, dz, _ = self._pass(x, z, st.masks, row, [])
                if k == 0:
                    st.rec0, st.kl0 = rec_s.sum(dim=1) / ns, kl
                lib.lv_svi_rec_step_f32(P(dz), 1, P(eps), P(st.klw), float(lr), float(momentum), float(clip), P(lam), P(vel),
                                        P(st.g_rec, k * B * 2 * nz), P(st.lam_rec, k * B * 2 * nz), P(z_next), P(kl_next), B, ns, nz, s)
            st.z, st.kl = _eng.reparam_kl_forward(lam, eps)
            with torch.no_grad():
                st.rec = self.vae.decoder.reconstruct_error(x, st.z, masks=st.masks).sum(dim=1) / ns
        if steps == 0:
            st.rec0, st.kl0 = st.rec, st.kl
        st.x, st.eps, st.lam, st.steps, st.ns = x, eps, lam, steps, ns
        st.hyper = (float(lr), float(momentum), float(clip))
        return st

    def savae_backward(self, st, seeds, fd_eps):
        vae = self.vae
        x, eps, ns, K = st.x, st.eps, st.ns, st.steps
        dev = x.device
        lib, s = _eng.backend_for(dev), _eng.stream_ptr(dev)
        P = _eng.P
        B, _, nz = eps.shape
        lr, mom, clip = st.hyper
        mask_in, mask_out = st.masks
        f32 = dict(dtype=torch.float32, device=dev)
        every = list(vae.decoder._params())
        params = [p for p in every if p.requires_grad]
        seeds = seeds.detach().float().contiguous()
        flat = getattr(getattr(vae.decoder, "_hip", None), "flat", None)
        if flat is not None:
            flat.before_autograd_backward()
        with vae._decoder_gradients_preserved(dev):
            _, dz, total = self._pass(x, st.z, st.masks, (seeds / ns).view(B, 1).expand(B, ns).contiguous(), params)
            total = [g.clone() for g in total]
            lbar = _eng.reparam_kl_backward(st.lam, eps, dz.view(B, ns, nz), seeds * st.klw)
            if K > 0:
                vbar = torch.zeros(B, 2 * nz, **f32)
                u, scal = torch.empty(B, 2 * nz, **f32), torch.empty(3, **f32)
                zpm, seeds2 = torch.empty(B, 2 * ns, nz, **f32), torch.empty(B * 2 * ns, **f32)
                mask2 = None
                if mask_out is not None:
                    m4 = mask_out.view(B, ns, mask_out.shape[1], -1)
                    mask2 = torch.cat((m4, m4), dim=1).reshape(B * 2 * ns, mask_out.shape[1], -1).contiguous()
            for k in range(K - 1, -1, -1):
                o = k * B * 2 * nz
                lib.lv_savae_adjoint_f32(P(lbar), P(vbar), P(st.g_rec, o), P(st.lam_rec, o), P(eps), lr, mom, clip, float(fd_eps),
                                         P(u), P(scal), P(zpm), P(seeds2), B, ns, nz, s)
                _, dz2, gs = self._pass(x, zpm, (mask_in, mask2), seeds2, params)
                for t, g in zip(total, gs):
                    g = g.contiguous()
                    lib.lv_add_f32(P(t), P(g), P(t), t.numel(), s)
                lib.lv_savae_hvp_f32(P(dz2), 1, P(eps), P(st.lam_rec, o), P(u), P(scal), P(st.klw), P(lbar), B, ns, nz, s)
        it = iter(total)
        return lbar, tuple(next(it) if p.requires_grad else None for p in every)


class VAE(nn.Module):
    """Encoder q(z|x), decoder p(x|z), prior N(0, I)."""

    def __init__(self, encoder, decoder, args):
        super().__init__()
        self.encoder, self.decoder = encoder, decoder
        self.args, self.nz = args, args.nz
        dev = args.device
        self.prior = torch.distributions.normal.Normal(torch.zeros(self.nz, device=dev), torch.ones(self.nz, device=dev))

    def set_precision(self, precision, encoder_forward=None, forward_operands=None):
        """Arithmetic of the HIP path behind this model's `loss` / `backward` (no counterpart in the reference, whose precision is
        the tensors' dtype): "f32" (default; exact-f32 MFMA, north_star's 1e-4 parity path) or "bf16" (BASELINE.json's GPU
        configuration: bf16 matrix pipe with f32 accumulation for the large products and the recurrent operands; master weights,
        state, gradients and reductions stay f32).  encoder_forward="f32" with "bf16": the encoder's forward f32-accurate (the KL
        then meets 1e-4 too; see trainer.AggressiveTextTrainer).  Image models also take "bf16x3".  Returns self."""
        for m in (self.encoder, self.decoder):
            eng = getattr(m, "_hip", None)
            if eng is None:
                raise TypeError("%s has no HIP engine" % type(m).__name__)
            eng.precision = precision
        if hasattr(self.encoder._hip, "exact_forward"):
            self.encoder._hip.exact_forward = ("gx", "rec") if (encoder_forward == "f32" and precision == "bf16") else ()
        if forward_operands is not None:
            self.set_forward_operands(forward_operands)
        return self

    def set_forward_operands(self, fmt):
        """Number format of the ENCODER FORWARD's matrix-pipe operands under precision "bf16": "f16" (default: IEEE binary16 images
        of X, W_ih, W_hh and the h hand-off -- 11-bit significands on the same instructions and rates as bf16, which puts the KL
        within north_star's 1e-4; range assumption: |weights|, |embeddings|, |h| << 65504 (values beyond saturate at +-65504, values
        below 6e-5 are kept as binary16 subnormals: tests/test_gpu_kernels.py::test_binary16_subnormal_*) or "bf16" (the arithmetic of
        rounds 1-4: KL 2e-4..5e-4).  Gradient products and the BPTT are bf16 either way.  Returns self."""
        if fmt not in ("f16", "bf16"):
            raise ValueError("forward operands: 'f16' or 'bf16'")
        eng = getattr(self.encoder, "_hip", None)
        if eng is None or not hasattr(eng, "fwd_operands"):
            raise TypeError("%s has no binary16 forward" % type(self.encoder).__name__)
        eng.fwd_operands = fmt
        return self

    def use_flat_grads(self, flag=True):
        """Drop-in autograd path: hand the parameters' gradients out as VIEWS of the engines' flat gradient buffers after a plain
        `loss.backward()` (default; zero-copy, engine.FlatBuffer.deliver_grads -- a .grad obtained this way is overwritten by the next
        backward) or always as fresh tensors (False: stock autograd aliasing semantics, 215 MB of copies per step at the Yahoo
        shape).  Returns self."""
        for m in (self.encoder, self.decoder):
            eng = getattr(m, "_hip", None)
            if eng is not None and getattr(eng, "flat", None) is not None:
                eng.flat.flat_grads = bool(flag)
            elif eng is not None:
                eng._flat_grads_pref = bool(flag)
        return self

    def arithmetic(self):
        """The run-config record of the HIP path's arithmetic (what a checkpoint's sidecar / a log line should carry)."""
        e = getattr(self.encoder, "_hip", None)
        return {"precision": getattr(e, "precision", None), "encoder_forward": "f32" if getattr(e, "exact_forward", ()) else "operands",
                "forward_operands": getattr(e, "fwd_operands", None)}

    @staticmethod
    def _batch(x):
        """A variable-length batch (x, sents_len) -- what VarLSTMEncoder / VarLSTMDecoder take -- in its validated form
        (engine.varlen_batch: lengths checked and moved to the device ONCE per call, however often the networks are run on it);
        anything else as it is."""
        return _eng.varlen_batch(x) if isinstance(x, (tuple, list)) and len(x) == 2 else x

    # ---- training path (reference vae.py:35-98) ---------------------------------------------------------
    def encode(self, x, nsamples=1, eps=None):
        """-> z (batch, nsamples, nz), KL (batch,).  `eps` injects the reparameterisation noise."""
        extra = {} if eps is None else {"eps": eps}
        return self.encoder.encode(x, nsamples, **extra)

    def encode_stats(self, x):
        """-> mu (batch, nz), logvar (batch, nz)."""
        return self.encoder(x)

    def loss(self, x, kl_weight, nsamples=1, noise=None, free_bits=None, free_bits_mode="dim"):
        """-> (rec + kl_weight*KL, rec, KL), each (batch,).

        noise = (eps, mask_in, mask_out) injects the random draws of this call (parity tests); the default draws
        them from torch's device generator at the same three places the reference does.

        free_bits = lambda >= 0 (nats per latent dimension; None: off, the code path above unchanged) minimises the free-bits
        objective instead (csrc/lv_freebits.hip): -> (rec + kl_weight*kl_obj, rec, KL) with kl_obj the KL
        thresholded per free_bits_mode -- "dim" (each KL_bj against lambda), "batch_dim" (the batch mean of each dimension against
        lambda; Kingma et al.'s form) or "batch" (the batch mean of the whole KL against nz*lambda) -- and KL the analytic,
        unthresholded one, for reports (detached).  The gate is a constant of the step.  free_bits = 0.0 takes the gated route (a
        dimension whose KL is exactly 0 closes its gate): not promised bit-equal to None.  The gate of the last call is kept as
        self.last_free_bits_gate [batch][nz]."""
        if free_bits is not None:
            _eng.check_free_bits(free_bits, free_bits_mode)               # refusals before anything is launched
        eps, masks = (None, None) if noise is None else (noise[0], (noise[1], noise[2]))
        x = self._batch(x)
        dec_extra = {} if masks is None else {"masks": masks}
        if free_bits is not None:
            from .encoders.encoder import _ReparamKLFreeBitsFn
            mulv = self.encoder._forward_mulv(x)
            eps = self.encoder._draw_eps(mulv.shape[0], nsamples, mulv.shape[1] // 2, mulv.device, eps)
            z, kl_obj, kl, gate = _ReparamKLFreeBitsFn.apply(mulv, eps, float(free_bits), free_bits_mode)
            self.last_free_bits_gate = gate
            rec = self.decoder.reconstruct_error(x, z, **dec_extra).mean(dim=1)
            return rec + kl_weight * kl_obj, rec, kl
        z, kl = self.encode(x, nsamples, eps=eps)
        rec = self.decoder.reconstruct_error(x, z, **dec_extra).mean(dim=1)
        return rec + kl_weight * kl, rec, kl

    def loss_iw(self, x, kl_weight=1.0, nsamples=1, noise=None, estimator="iwae"):
        """The importance-weighted bound as a training objective -> (loss, rec, KL), each (batch,):
        loss = -(logsumexp_s log w_s - log nsamples), log w_s = log p(x|z_s) + kl_weight * (log p(z_s) - log q(z_s|x)) -- with
        kl_weight = 1 what nll_iw(x, nsamples, nsamples) estimates (reference vae.py:100-129) -- differentiable through the
        reparameterised samples; rec is the sample mean of the reconstruction error and KL the analytic one, both for reports only
        (detached).  nsamples = 1 is a single-sample Monte-Carlo ELBO: its KL term is the sampled log q - log p, not the analytic KL.
        Works with every decoder that has reconstruct_error(x, z) -> (batch, nsamples).  noise: as `loss`.
        estimator = "dreg": the doubly-reparameterised estimator of the encoder's gradient (Tucker et al. 2019) --
        the same three values and the same decoder gradient; what flows from z_s into (mu, logvar) is scaled by
        r_s = 1 - kl_weight * (1 - wn_s) and the weights' direct terms take their doubly-reparameterised form.  A decoder whose rows
        are coupled (decoder.couples_samples(): the PixelCNN decoder's BatchNorm in train mode) gets a second backward pass, seeded
        with g * u_s, for what reaches z; its parameters still receive the gradient of the g * wn_s pass."""
        from .encoders.encoder import _ReparamKLFn
        if estimator not in ("iwae", "dreg"):
            raise ValueError("estimator: 'iwae' or 'dreg', not %r" % (estimator,))
        eps, masks = (None, None) if noise is None else (noise[0], (noise[1], noise[2]))
        x = self._batch(x)
        mulv = self.encoder._forward_mulv(x)
        eps = self.encoder._draw_eps(mulv.shape[0], nsamples, mulv.shape[1] // 2, mulv.device, eps)
        z, kl = _ReparamKLFn.apply(mulv, eps)
        dec_extra = {} if masks is None else {"masks": masks}
        klw = torch.full((1,), float(kl_weight), dtype=torch.float32, device=mulv.device)
        if estimator == "dreg":
            rs = torch.empty(z.shape[0], z.shape[1], dtype=torch.float32, device=mulv.device)
            coupled = getattr(self.decoder, "couples_samples", None)
            hold = {"engine": self.decoder._hip} if coupled is not None and coupled() else None
            zs = _ScaleSamplesFn.apply(z, rs, hold)
            if hold is not None:
                hold["zs"] = zs
            rec_s = self.decoder.reconstruct_error(x, zs, **dec_extra)
            loss, rec = _IWBoundFn.apply(rec_s, mulv, eps, z.detach(), kl.detach(), klw, rs, hold)
            return loss, rec, kl.detach()
        rec_s = self.decoder.reconstruct_error(x, z, **dec_extra)
        loss, rec = _IWBoundFn.apply(rec_s, mulv, eps, z.detach(), kl.detach(), klw, None, None)
        return loss, rec, kl.detach()

    # True: loss_savae takes the decoder engine's semi-amortized step where _fused_savae_ok allows it; False forces the generic
    # route (A/B runs, the tests' second oracle, the bench baseline)
    fused_savae = True

    def _fused_savae_ok(self, x, B, ns):
        eng = self.decoder._hip
        return bool(self.fused_savae and eng.savae_supported(B, ns))

    def _savae_arguments(self, who, x, svi_steps, svi_lr, svi_momentum, svi_clip, fd_eps, nsamples):
        """The refusals of semi-amortized training, all of them before anything is launched."""
        if isinstance(x, (tuple, list)):
            raise ValueError("%s: variable-length batches (x, lengths) are not supported; batch by length" % who)
        eng = getattr(self.decoder, "_hip", None)
        if not isinstance(eng, _eng.LSTMDecoderEngine) or type(self.decoder).__name__ != "LSTMDecoder":
            raise ValueError("%s: an LSTMDecoder is expected, got %s" % (who, type(self.decoder).__name__))
        for e in (eng, getattr(self.encoder, "_hip", None)):
            if getattr(e, "precision", "f32") != "f32":
                raise ValueError("%s: precision 'f32' only -- the Hessian-vector products are differences of gradients divided by the "
                                 "step, and bf16's gradient rounding (2^-9) divided by fd_eps would swamp them" % who)
        if not (torch.is_tensor(x) and x.dim() == 2 and x.dtype == torch.int64):
            raise ValueError("%s: x is an int64 tensor (batch, seq_len)" % who)
        if int(svi_steps) < 0 or int(nsamples) < 1:
            raise ValueError("%s: svi_steps >= 0 and nsamples >= 1 expected" % who)
        if not (float(svi_lr) > 0.0 and float(svi_clip) > 0.0 and float(fd_eps) > 0.0 and 0.0 <= float(svi_momentum) < 1.0):
            raise ValueError("%s: svi_lr > 0, svi_clip > 0, fd_eps > 0 and 0 <= svi_momentum < 1 expected" % who)

    def _savae_noise(self, who, x, nsamples, noise):
        """noise = (eps, mask_in, mask_out) checked against the step's shapes -> the three tensors (masks uint8 or None)."""
        B, T = x.shape
        dev = x.device
        dec = self.decoder
        if not (isinstance(noise, (tuple, list)) and len(noise) == 3):
            raise ValueError("%s: noise is (eps, mask_in, mask_out)" % who)
        eps, m_in, m_out = noise
        if not torch.is_tensor(eps) or tuple(eps.shape) != (B, nsamples, self.nz) or eps.dtype != torch.float32 or eps.device != dev:
            raise ValueError("%s: eps must be a float32 tensor of shape (%d, %d, %d) on %s" % (who, B, nsamples, self.nz, dev))
        for name, m, shape in (("mask_in", m_in, (B, T - 1, dec.ni)), ("mask_out", m_out, (B * nsamples, T - 1, dec.nh))):
            if m is not None and not (torch.is_tensor(m) and tuple(m.shape) == shape and m.device == dev
                                      and m.dtype in (torch.uint8, torch.bool, torch.float32)):
                raise ValueError("%s: %s must be a keep-mask of shape %s (uint8, bool or float32) on %s" % (who, name, shape, dev))
        cast = lambda m: None if m is None else m.to(torch.uint8).contiguous()
        return eps.contiguous(), cast(m_in), cast(m_out)

    def loss_savae(self, x, kl_weight=1.0, svi_steps=20, svi_lr=1.0, svi_momentum=0.5, svi_clip=5.0, fd_eps=1e-2, nsamples=1,
                   noise=None):
        """Semi-amortized training (SA-VAE, Kim et al. 2018) -> (loss, rec, KL), each (batch,), at the posterior
        lambda_K that `svi_steps` steps of refine_posterior's update reach from the encoder's output lambda_0 -- under THIS step's
        noise and dropout masks, the same in every decoder pass of the step.  rec and KL are detached.  `loss.mean().backward()` (or
        any seeds) differentiates THROUGH the refinement: the decoder's parameters get d loss / d theta at lambda_K plus the
        refinement's dependence on theta, the encoder is reached through lambda_0 only.  The Hessian-vector products of that backward
        pass are central differences of gradients at lambda_k +- e u with e = fd_eps * max(1, max|lambda_k|) (csrc/lv_savae.hip).
        A step costs K forwards and K backwards to z for the refinement, one full forward and backward at lambda_K, and K full passes
        on twice the rows.  svi_steps = 0 is the ordinary ELBO.

        noise = (eps, mask_in, mask_out): eps (batch, nsamples, nz) float32; keep-masks (batch, T-1, ni) and (batch * nsamples, T-1,
        dec_nh) or None; otherwise drawn where `loss` draws them.  Exact f32 only, LSTM decoder, equal-length batches.
        Routes (class switch fused_savae = False forces the second): "fused", engine.LSTMDecoderEngine.savae_forward /
        savae_backward; "generic", the same definition over decoder.reconstruct_error and torch.autograd.grad."""
        who = "loss_savae"
        self._savae_arguments(who, x, svi_steps, svi_lr, svi_momentum, svi_clip, fd_eps, nsamples)
        nsamples, svi_steps = int(nsamples), int(svi_steps)
        if noise is not None:
            noise = self._savae_noise(who, x, nsamples, noise)
        B, T = x.shape
        dec = self.decoder
        mulv = self.encoder._forward_mulv(x)
        if noise is None:
            eps = self.encoder._draw_eps(B, nsamples, self.nz, x.device)
            m_in, m_out = dec._draw_masks(B, T - 1, x.device)
            if nsamples > 1 and m_out is not None:
                m_out = torch.empty(B * nsamples, T - 1, dec.nh, device=x.device).bernoulli_(1 - dec.dropout_out.p).to(torch.uint8)
        else:
            eps, m_in, m_out = noise
        dec._hip.ensure(x.device)
        route = dec._hip if self._fused_savae_ok(x, B, nsamples) else _SAVAEGeneric(self)
        cfg = (dec.dropout_in.p, dec.dropout_out.p, svi_steps, float(svi_lr), float(svi_momentum), float(svi_clip), float(fd_eps),
               float(kl_weight))
        return _SAVAEFn.apply(route, cfg, x, mulv, eps, m_in, m_out, *dec._params())

    def KL(self, x):
        return self.encode(x, 1)[1]

    # ---- generation (delegated; generation itself is outside the hot path) -----------------------------
    def decode(self, z, strategy, K=5, return_info=False, temperature=1.0, top_k=0, top_p=1.0):
        """return_info: also the per-sentence dict the decoder's beam_search_decode / greedy_decode / sample_decode returns with
        return_info=True.  temperature / top_k / top_p: sample_decode's; non-neutral values with another strategy raise
        ValueError."""
        if strategy not in _GENERATORS:
            raise ValueError("the decoding strategy is not supported")
        neutral = _eng.sampling_filter(temperature, top_k, top_p)[3]
        if not neutral and strategy != "sample":
            raise ValueError("temperature / top_k / top_p apply to the decoding strategy \"sample\" only")
        fn = getattr(self.decoder, _GENERATORS[strategy])
        if strategy == "beam":
            return fn(z, K, return_info=True) if return_info else fn(z, K)
        if not neutral:
            return fn(z, return_info=return_info, temperature=temperature, top_k=top_k, top_p=top_p)
        return fn(z, return_info=True) if return_info else fn(z)

    def reconstruct(self, x, decoding_strategy="greedy", K=5, temperature=1.0, top_k=0, top_p=1.0):
        neutral = _eng.sampling_filter(temperature, top_k, top_p)[3]
        if not neutral and decoding_strategy != "sample":
            raise ValueError("temperature / top_k / top_p apply to the decoding strategy \"sample\" only")
        return self.decode(self.sample_from_inference(x).squeeze(1), decoding_strategy, K, temperature=temperature, top_k=top_k,
                           top_p=top_p)

    def sample_from_prior(self, nsamples):
        return self.prior.sample((nsamples,))

    def sample_from_inference(self, x, nsamples=1):
        return self.encoder.sample(x, nsamples)[0]

    # ---- evaluation (reference vae.py:100-227) -------------------------------------------------------------
    def nll_iw(self, x, nsamples, ns=100):
        """Importance-weighted estimate of -log p(x) from `nsamples` draws, `ns` at a time -> (batch,)   (reference
        vae.py:100-129).  The decoder pass over batch*ns sequences is the hot path's HIP forward; log p(z), log q(z|x) and
        the final log_sum_exp are lv_eval.hip kernels."""
        log_w = []
        x = self._batch(x)
        for _ in range(int(nsamples / ns)):
            z, stats = self.encoder.sample(x, ns)
            log_w.append(self.eval_complete_ll(x, z) - self.eval_inference_dist(x, z, stats))
        return -_eng.logsumexp_rows(torch.cat(log_w, dim=-1), -math.log(nsamples))

    def eval_prior_dist(self, zrange):
        """log N(z; 0, I) summed over the latent dimension (reference vae.py:135-145)."""
        if zrange.dim() == 3:
            return _eng.gauss_logpdf(zrange, None, None)
        return self.prior.log_prob(zrange).sum(dim=-1)

    def eval_cond_ll(self, x, z):
        return self.decoder.log_probability(x, z)

    def eval_complete_ll(self, x, z):
        """log p(z, x) for z (batch, nsamples, nz) -> (batch, nsamples)."""
        return self.eval_prior_dist(z) + self.eval_cond_ll(x, z)

    def eval_inference_dist(self, x, z, param=None):
        return self.encoder.eval_inference_dist(x, z, param)

    # True: eval_log_model_posterior / calc_model_posterior_mean take lv_grid_posterior.hip where _fused_grid_ok allows it;
    # False forces the generic route below (A/B runs, tests)
    fused_grid = True

    def _fused_decoder(self, switch, x, same_device=(), needs_no_dropout=False):
        """What every fused evaluation route asks first -> the decoder's engine, or None where the route is closed: its class
        switch is on, the decoder is an LSTM decoder, x is a 2-D int64 tensor, the tensors of same_device live on x's device,
        (needs_no_dropout: the kernel computes the eval-mode decoder) no dropout mask would be drawn -- the decoder is not
        training, or both its dropout p are 0 -- and x's device is one the package has kernels for.  The caller adds its own
        conditions and asks the engine for its kernel's envelope."""
        dec = self.decoder
        eng = getattr(dec, "_hip", None)
        if not (switch and isinstance(eng, _eng.LSTMDecoderEngine) and torch.is_tensor(x) and x.dim() == 2
                and x.dtype == torch.int64 and all(t.device == x.device for t in same_device)):
            return None
        if needs_no_dropout and dec.training and (dec.dropout_in.p > 0 or dec.dropout_out.p > 0):
            return None
        try:
            eng.ensure(x.device)
        except _lib.LvaeError:
            return None
        return eng

    def _fused_grid_ok(self, x, grid_z):
        """The fused grid kernels compute the eval-mode decoder without autograd: usable where _fused_decoder allows it (no
        dropout mask would be drawn; x and the grid share one device), autograd is off (every call site in toy.py runs under
        torch.no_grad(); with grad enabled the generic route keeps the result differentiable), the grid is (K, nz), and the
        decoder is inside lv_dec_cond_ll_f32's envelope.  Anything else keeps the generic route and its behaviour, errors
        included (e.g. toy.py's epoch-end dump, which runs in train mode and draws dropout masks there)."""
        if torch.is_grad_enabled() or not (torch.is_tensor(grid_z) and grid_z.dim() == 2 and grid_z.size(1) == self.nz):
            return False
        eng = self._fused_decoder(self.fused_grid, x, (grid_z,), needs_no_dropout=True)
        return eng is not None and eng.cond_ll_supported(x.size(1))

    def _fused_grid_posterior(self, x, grid_z, want_log_post):
        cond = self.decoder._hip.cond_ll(x, grid_z)
        return _eng.grid_posterior(cond, grid_z, want_log_post)

    def eval_log_model_posterior(self, x, grid_z):
        """log p(z|x) on a grid of K points (K, nz) -> (batch, K), normalised over the grid.  Eval-mode LSTM decoder inside the
        envelope, under torch.no_grad(): one lv_dec_cond_ll_f32 + one lv_grid_posterior_f32 launch (the grid is shared, never
        expanded; no logits)."""
        if self._fused_grid_ok(x, grid_z):
            return self._fused_grid_posterior(x, grid_z, True)[0]
        x = self._batch(x)
        n = x.size(0) if torch.is_tensor(x) else x[0].size(0)
        joint = self.eval_complete_ll(x, grid_z.unsqueeze(0).expand(n, *grid_z.size()).contiguous())
        return joint - log_sum_exp(joint, dim=1, keepdim=True)

    def calc_model_posterior_mean(self, x, grid_z):
        """E[z|x] over the grid (K, nz) -> (batch, nz); the fused route as eval_log_model_posterior's."""
        if self._fused_grid_ok(x, grid_z):
            return self._fused_grid_posterior(x, grid_z, False)[1]
        w = self.eval_log_model_posterior(x, grid_z).exp()
        return (w.unsqueeze(2) * grid_z.unsqueeze(0)).sum(1)

    # True: sample_from_posterior takes the fused chain kernel (lv_mh_chain_f32) where _fused_mh_ok allows it; False forces
    # the per-iteration route (A/B runs, tests)
    fused_mh = True

    def _fused_mh_ok(self, x, z0):
        """Route "chain" of sample_from_posterior: _fused_decoder's conditions (no dropout mask drawn, z0 on x's device) and
        lv_mh_chain_f32's envelope."""
        eng = self._fused_decoder(self.fused_mh, x, (z0,), needs_no_dropout=True)
        return eng is not None and eng.cond_ll_supported(x.size(1))

    def _chain_noise(self, who, x, chains, total, noise, generator, name="eps", iterations_only=False):
        """The random draws of `total` chain iterations -> (z0 or None, draw).  noise = (z0 [B][chains][nz], the step noise `name`
        [total][B][chains][nz], u [total][B][chains]) is checked -- the device first: the kernels take raw pointers, so a
        mismatch is refused before anything is launched; iterations_only: of the shapes only the two iteration counts -- and
        draw(i0, n) hands out its slices as contiguous float32.  noise None: z0 is left to _chain_start, and draw(i0, n) is one
        torch.randn and one torch.rand on x's device (`generator` optional)."""
        dev = x.device if torch.is_tensor(x) else x[0].device
        B = x.size(0) if torch.is_tensor(x) else x[0].size(0)
        nz = self.nz
        z0 = step_all = u_all = None
        if noise is not None:
            z0, step_all, u_all = noise
            for nm, t in (("z0", z0), (name, step_all), ("u", u_all)):
                if t.device != dev:
                    raise _lib.LvaeError("%s: %s is on %s, x on %s" % (who, nm, t.device, dev))
            if iterations_only:
                if step_all.shape[0] != total or u_all.shape[0] != total:
                    raise ValueError("%s: noise for %d iterations expected" % (who, total))
            elif (tuple(z0.shape) != (B, chains, nz) or tuple(step_all.shape) != (total, B, chains, nz)
                    or tuple(u_all.shape) != (total, B, chains)):
                raise ValueError("%s: noise z0 [%d][%d][%d], %s [%d][%d][%d][%d], u [%d][%d][%d] expected, got %s, %s, %s"
                                 % (who, B, chains, nz, name, total, B, chains, nz, total, B, chains, tuple(z0.shape),
                                    tuple(step_all.shape), tuple(u_all.shape)))

        def draw(i0, n):
            if noise is None:
                return (torch.randn(n, B, chains, nz, device=dev, generator=generator),
                        torch.rand(n, B, chains, device=dev, generator=generator))
            return step_all[i0:i0 + n].float().contiguous(), u_all[i0:i0 + n].float().contiguous()
        return z0, draw

    def _chain_start(self, x, chains, init, z0, generator):
        """Where the chains start -> (z0 [B][chains][nz], mu0, lv0), contiguous float32; mu0 / lv0 [B][nz] are q0's statistics
        for init "encoder", None (q0 = the prior) otherwise.  z0 None: drawn from q(z|x) by encoder.sample (init "encoder", and
        "sampler": sample_from_posterior's start) or from the prior by torch.randn on x's device (`generator` optional)."""
        mu0 = lv0 = None
        if init == "encoder":
            if z0 is None:
                z0, (mu0, lv0) = self.encoder.sample(x, chains)
            else:
                mu0, lv0 = self.encode_stats(x)
            mu0, lv0 = mu0.detach().float().contiguous(), lv0.detach().float().contiguous()
        elif z0 is None and init == "sampler":
            z0 = self.encoder.sample(x, chains)[0]
        elif z0 is None:
            xb = x if torch.is_tensor(x) else x[0]
            z0 = torch.randn(xb.size(0), chains, self.nz, device=xb.device, generator=generator)
        return z0.detach().float().contiguous(), mu0, lv0

    def sample_from_posterior(self, x, nsamples, chains=1, burn_in=None, thin=None, std=None, noise=None, generator=None,
                              iters_per_launch=None, return_info=False, transition="rw", leapfrog=10, step_size=None, adapt=None,
                              step_bounds=(1e-4, 0.5)):
        """Random-walk Metropolis-Hastings samples from the model posterior p(z|x) (reference vae.py:218-254)
        -> (batch, nsamples, chains, nz) float32 on x's device, computed under torch.no_grad().

        Every chain starts at a draw from q(z|x) and runs burn_in + nsamples * thin iterations: next = eps * std + cur,
        ratio = log p(next, x) - log p(cur, x) (eval_complete_ll), accepted where u < min(exp(ratio), 1); cur is kept every
        `thin` iterations after `burn_in`.  burn_in / thin / std default to args.mh_burn_in / mh_thin / mh_std (the
        reference reads these three fields, which none of its scripts defines).  `chains` independent chains per sentence
        (the reference runs one): the reference returns (batch, nsamples, 1, nz) -- its docstring says (batch, nsamples, nz),
        but cur is (batch, 1, nz) when it is unsqueezed and concatenated -- and that singleton is the chain axis here.
        The starting point is self.encoder.sample(x, chains)[0]; the reference looks `sample_from_inference` up on the
        encoder, which has no such method (it is VAE's), and evidently means this.

        Differences from the reference, on purpose: cur and cur_ll are SELECTED, never blended (mask * next + (1 - mask) * cur
        turns cur_ll into NaN for good once a proposal scores NaN; here such a proposal is rejected and the chain goes on).

        noise = (z0 [B][chains][nz], eps [iterations][B][chains][nz], u [iterations][B][chains]) injects every random draw
        (parity tests).  Without it eps and u are drawn with torch.randn / torch.rand on x's device (`generator` optional),
        one pair of draws per launch chunk of `iters_per_launch` iterations: a seed therefore reproduces a chain only for
        the same iters_per_launch.

        Routes (class switch fused_mh = False forces the second):
          "chain": eval-mode LSTM decoder inside the fused kernel's envelope -- the whole chain on the device in launches of
                   at most iters_per_launch iterations (default: the largest n with n * (T - 1) <= 2048), 16 chains of a
                   sentence per workgroup; decoder.log_probability is never called;
          "step":  everything else (H > 128, the PixelCNN decoder, a training-mode decoder with dropout, which draws its
                   masks as the reference would): one eval_cond_ll(x, next) plus one lv_mh_step_f32 launch per iteration.
        Neither reads anything back to the host inside the chain.

        return_info: also {"accept_rate": [B, chains], "log_joint": [B, chains] (the final cur_ll), "route", "iterations",
        "ratios": [iterations, B, chains], "accepts": [iterations, B, chains] (the per-iteration ratio and accept flag)}.

        transition="hmc": every iteration is a Hamiltonian transition on p(z, x) -- nll_ais's session (csrc/lv_hmc.hip, DESIGN.md
        3.1.3) with the prior as q0 and beta = 1 throughout: `leapfrog` steps of size step_size (default args.mh_step_size), std
        not passed, noise = (z0, mom [iterations][B][chains][nz], u).  adapt = (target, rate) adapts the step size during burn_in
        only, so the kept samples come from a fixed kernel.  Routes "hmc-fused" / "hmc-generic" as nll_ais has them; "ratios"
        holds dH; variable-length pairs are refused."""
        a = self.args
        if transition not in ("rw", "hmc"):
            raise ValueError("sample_from_posterior: transition 'rw' or 'hmc' expected, got %r" % (transition,))
        if transition == "hmc" and std is not None:
            raise ValueError("sample_from_posterior: std is the random-walk proposal scale; transition='hmc' takes step_size")
        vals = [burn_in, thin, std]
        for i, f in enumerate(("mh_burn_in", "mh_thin", "mh_std")[:2 if transition == "hmc" else 3]):
            if vals[i] is None:
                if not hasattr(a, f):
                    raise ValueError("sample_from_posterior: pass burn_in / thin / std or set args.mh_burn_in, args.mh_thin "
                                     "and args.mh_std (missing: %s)" % f)
                vals[i] = getattr(a, f)
        burn_in, thin = int(vals[0]), int(vals[1])
        nsamples, chains = int(nsamples), int(chains)
        if nsamples < 1 or chains < 1 or burn_in < 0 or thin < 1:
            raise ValueError("sample_from_posterior: nsamples >= 1, chains >= 1, burn_in >= 0, thin >= 1 expected")
        total = burn_in + nsamples * thin
        if transition == "hmc":
            L, step_size, adapt = self._hmc_arguments("sample_from_posterior", "mh_step_size", leapfrog, step_size, adapt, step_bounds)
            if adapt is not None:
                adapt = adapt + (burn_in,)
            r, route = self._hmc_run("sample_from_posterior", x, chains, [1.0] * (total + 1), "sampler", noise, generator, L,
                                     step_size, adapt, (burn_in, thin, nsamples), iters_per_launch)
            if not return_info:
                return r["samples"]
            return r["samples"], {"accept_rate": r["accepts"].float() / float(total), "log_joint": r["lq"] + r["g"], "route": route,
                                  "iterations": total, "ratios": r["ratios"], "accepts": r["flags"]}
        std = float(vals[2])
        x = self._batch(x)
        with torch.no_grad():
            z0, draw = self._chain_noise("sample_from_posterior", x, chains, total, noise, generator, iterations_only=True)
            z0 = self._chain_start(x, chains, "sampler", z0, generator)[0]
            _, C, nz = z0.shape
            if C != chains or nz != self.nz:
                raise ValueError("sample_from_posterior: z0 [B][%d][%d] expected, got %s" % (chains, self.nz, tuple(z0.shape)))
            if self._fused_mh_ok(x, z0):
                route = "chain"
                r = self.decoder._hip.mh_chain(x, z0, draw, burn_in, thin, nsamples, std, iters_per_launch)
                samples, log_joint, accepts, ratios, flags = r["samples"], r["log_joint"], r["accepts"], r["ratios"], r["flags"]
            else:
                route = "step"
                samples, log_joint, accepts, ratios, flags = self._mh_by_steps(x, z0, draw, burn_in, thin, nsamples, std,
                                                                               iters_per_launch)
        if not return_info:
            return samples
        return samples, {"accept_rate": accepts.float() / float(total), "log_joint": log_joint, "route": route,
                         "iterations": total, "ratios": ratios, "accepts": flags}

    def _mh_by_steps(self, x, z0, draw, burn_in, thin, nsamples, std, iters_per_launch):
        """Route "step" of sample_from_posterior: eval_cond_ll for the scores, lv_mh_step_f32 for everything else."""
        dev = z0.device
        B, C, nz = z0.shape
        total = burn_in + nsamples * thin
        per = _eng.iters_per_launch_for("sample_from_posterior", iters_per_launch, x)
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        cur, prop = z0.clone(), z0.clone()
        cur_ll, accepts = torch.zeros(B, C, **f32), torch.zeros(B, C, **i32)
        samples = torch.empty(B, nsamples, C, nz, **f32)
        ratios, flags = torch.empty(total, B, C, **f32), torch.empty(total, B, C, **i32)
        noise = _eng.NoiseCursor(draw, total, per)
        _eng.mh_step(self.eval_cond_ll(x, cur), prop, cur, cur_ll, accepts, None, noise.first(), std, samples, -1, init=True)
        for it in range(total):
            cond = self.eval_cond_ll(x, prop)
            u_it, eps_next = noise.step(it)
            _eng.mh_step(cond, prop, cur, cur_ll, accepts, u_it, eps_next, std, samples,
                         _eng.mh_keep_index(it, burn_in, thin, nsamples), ratio_out=ratios[it], flag_out=flags[it])
        return samples, cur_ll, accepts, ratios, flags

    # True: nll_ais takes the fused chain kernel (lv_ais_chain_f32) where _fused_ais_ok allows it; False forces the
    # per-iteration route (A/B runs, tests)
    fused_ais = True

    def _fused_ais_ok(self, x, z0):
        """Route "chain" of nll_ais: _fused_decoder's conditions, as _fused_mh_ok asks for them, and lv_ais_chain_f32's envelope."""
        eng = self._fused_decoder(self.fused_ais, x, (z0,), needs_no_dropout=True)
        return eng is not None and eng.ais_chain_supported(x.size(1))

    @staticmethod
    def ais_schedule(schedule, temps, transitions=1):
        """The per-iteration temperatures of nll_ais as a list of temps * transitions + 1 Python floats (float64): "sigmoid"
        (Wu et al. 2017: the logistic function on linspace(-4, 4), rescaled to [0, 1]), "linear", or an explicit sequence of
        temps + 1 values starting at 0, ending at 1 and non-decreasing; every temperature after the first is repeated
        `transitions` times (further transitions at the same temperature: their log-weight increment is 0)."""
        temps, transitions = int(temps), int(transitions)
        if temps < 1 or transitions < 1:
            raise ValueError("nll_ais: temps >= 1 and transitions >= 1 expected")
        if isinstance(schedule, str):
            if schedule == "sigmoid":
                s = torch.sigmoid(torch.linspace(-4.0, 4.0, temps + 1, dtype=torch.float64))
                b = ((s - s[0]) / (s[-1] - s[0])).tolist()
            elif schedule == "linear":
                b = torch.linspace(0.0, 1.0, temps + 1, dtype=torch.float64).tolist()
            else:
                raise ValueError("nll_ais: schedule 'sigmoid', 'linear' or a sequence of temps + 1 values expected, got %r"
                                 % (schedule,))
            b[0], b[-1] = 0.0, 1.0
        else:
            b = [float(v) for v in (schedule.tolist() if torch.is_tensor(schedule) else schedule)]
            if len(b) != temps + 1:
                raise ValueError("nll_ais: a schedule of temps + 1 = %d values expected, got %d" % (temps + 1, len(b)))
            if b[0] != 0.0 or b[-1] != 1.0 or any(not (b[i + 1] >= b[i]) for i in range(temps)):
                raise ValueError("nll_ais: the schedule must start at 0, end at 1 and be non-decreasing")
        return [b[0]] + [v for v in b[1:] for _ in range(transitions)]

    def nll_ais(self, x, chains=16, temps=500, transitions=1, std=None, schedule="sigmoid", init="prior", noise=None,
                generator=None, iters_per_launch=None, return_info=False, transition="rw", leapfrog=10, step_size=None, adapt=None,
                step_bounds=(1e-4, 0.5)):
        """Annealed importance sampling estimate of -log p(x) (Neal 2001; Wu et al. 2017) -> (batch,) float32 on x's device,
        computed under torch.no_grad().  Unlike nll_iw the estimate does not lean on the encoder: `chains` chains per sentence
        start at a draw from q0 -- the prior (init="prior") or q(z|x) (init="encoder") -- and move through N = temps *
        transitions random-walk Metropolis transitions (the kernel of sample_from_posterior) on the targets
        q0^(1 - beta_i) p(z, x)^beta_i, beta from 0 to 1 (ais_schedule); a chain's log-weight is the float64 sum of
        (beta_i - beta_{i-1}) g(z_{i-1}), g = log p(z, x) - log q0(z), and log p^(x) = logsumexp_c logw_c - log chains (the
        [batch][chains] epilogue is torch, in float64).  The contract, formula by formula, is at the top of csrc/lv_ais.hip.

        std: the proposal scale, a float or a sequence of N floats; default args.ais_std.  There is no built-in value: none
        would be right for both the prior's width and a trained posterior's.  Tune it by info["accept_rate_iter"].
        noise = (z0 [B][chains][nz], eps [N][B][chains][nz], u [N][B][chains]) injects every random draw; without it z0, eps
        and u are drawn on x's device (`generator` optional), eps / u one pair per launch chunk as sample_from_posterior does.

        Routes (class switch fused_ais = False forces the second):
          "chain": eval-mode LSTM decoder inside lv_ais_chain_f32's envelope -- the whole chain on the device in launches of at
                   most iters_per_launch iterations, 16 chains of a sentence per workgroup;
          "step":  everything else (H > 128, the PixelCNN decoder, a training-mode decoder with dropout, variable-length
                   pairs): one eval_cond_ll(x, next) plus one lv_ais_step_f32 launch per iteration.
        Neither reads anything back to the host inside the chain.

        return_info: also {"logw": [B, chains] float64, "accept_rate": [B, chains], "accept_rate_iter": [N], "route",
        "iterations", "se": [B] (the delta-method standard error of log p^: sqrt(var_c(w_c / mean w) / chains); nan for one
        chain), "ratios" / "accepts" / "logw_trace": [N, B, chains]}.

        transition="hmc": the N transitions are Hamiltonian (Wu et al. 2017; Cremer et al. 2018) -- `leapfrog` = L leapfrog steps
        of size step_size on U_beta = -log q0 - beta g with a fresh N(0, I) momentum, then a Metropolis decision on the
        Hamiltonian; the contract is at the top of csrc/lv_hmc.hip, DESIGN.md 3.1.3.  A transition costs L decoder forwards and
        backwards to z on all batch * chains rows (1 + N L passes in all), with the decoder in eval arithmetic whatever `training`
        says.  std must not be passed.  step_size: default args.ais_step_size; there is no built-in value, as for std.  adapt =
        (target, rate), e.g. (0.65, 0.02): after every transition a chain's step size is multiplied by exp(rate (1 - target)) if it
        accepted and by exp(-rate target) if not (both rounded to float32, so it is stationary at acceptance = target), and
        clamped to step_bounds; None keeps it fixed.  noise = (z0 [B][chains][nz], mom [N][B][chains][nz], u [N][B][chains]).
        Variable-length pairs are refused.  Nothing of the model changes (refine_posterior's guarantee), and with `noise` given no
        RNG state does.  Routes (class switch fused_hmc = False forces the second):
          "hmc-fused":   LSTM decoder, batch * chains rows inside svi_supported -- engine.LSTMDecoderEngine.hmc_ais;
          "hmc-generic": everything else -- decoder.reconstruct_error and torch.autograd.grad for d rec / d z (weight gradients
                         land in scratch that is restored afterwards), lv_hmc_leap_f32 for the rest.
        info then also has "step_size" [B, chains] (the final one), "leapfrog" and "cur" [B, chains, nz] (the chains' final
        states); "ratios" holds dH."""
        chains = int(chains)
        if chains < 1:
            raise ValueError("nll_ais: chains >= 1 expected")
        beta = self.ais_schedule(schedule, temps, transitions)
        total = len(beta) - 1
        if init not in ("prior", "encoder"):
            raise ValueError("nll_ais: init 'prior' or 'encoder' expected, got %r" % (init,))
        if transition not in ("rw", "hmc"):
            raise ValueError("nll_ais: transition 'rw' or 'hmc' expected, got %r" % (transition,))
        if transition == "hmc":
            if std is not None:
                raise ValueError("nll_ais: std is the random-walk proposal scale; transition='hmc' takes step_size")
            L, step_size, adapt = self._hmc_arguments("nll_ais", "ais_step_size", leapfrog, step_size, adapt, step_bounds)
            r, route = self._hmc_run("nll_ais", x, chains, beta, init, noise, generator, L, step_size, adapt, None, iters_per_launch)
            return self._ais_estimate(r, chains, total, route, beta, return_info, {"step_size": r["step_size"], "leapfrog": L,
                                                                                         "cur": r["cur"]})
        if std is None:
            if not hasattr(self.args, "ais_std"):
                raise ValueError("nll_ais: pass std or set args.ais_std (there is no default proposal scale)")
            std = self.args.ais_std
        if torch.is_tensor(std):
            std = std.tolist()
        stds = [float(v) for v in std] if isinstance(std, (list, tuple)) else [float(std)] * total
        if len(stds) != total or any(not (v >= 0.0) for v in stds):
            raise ValueError("nll_ais: std must be a float >= 0 or a sequence of temps * transitions = %d of them" % total)
        x = self._batch(x)
        with torch.no_grad():
            dev = x.device if torch.is_tensor(x) else x[0].device
            z0, draw = self._chain_noise("nll_ais", x, chains, total, noise, generator)
            z0, mu0, lv0 = self._chain_start(x, chains, init, z0, generator)
            if self._fused_ais_ok(x, z0):
                route = "chain"
                r = self.decoder._hip.ais_chain(x, z0, draw, torch.tensor(beta, dtype=torch.float64, device=dev),
                                                torch.tensor(stds, dtype=torch.float32, device=dev), mu0, lv0, iters_per_launch)
            else:
                route = "step"
                r = self._ais_by_steps(x, z0, draw, beta, stds, mu0, lv0, iters_per_launch)
        return self._ais_estimate(r, chains, total, route, beta, return_info, {"std": stds})

    @staticmethod
    def _ais_estimate(r, chains, total, route, beta, return_info, extra):
        """The float64 epilogue of nll_ais on a finished set of chains: log p^(x) = logsumexp_c logw_c - log chains."""
        with torch.no_grad():
            logw = r["logw"]
            log_px = torch.logsumexp(logw, dim=1) - math.log(chains)
            nll = (-log_px).float()
            if not return_info:
                return nll
            w = torch.exp(logw - logw.max(dim=1, keepdim=True)[0])
            w = w / w.mean(dim=1, keepdim=True)
            se = torch.sqrt(w.var(dim=1, unbiased=True) / chains) if chains > 1 else torch.full_like(log_px, float("nan"))
            flags = r["flags"]
        return nll, dict({"logw": logw, "accept_rate": r["accepts"].float() / float(total),
                          "accept_rate_iter": flags.float().mean(dim=(1, 2)), "route": route, "iterations": total, "se": se,
                          "ratios": r["ratios"], "accepts": flags, "logw_trace": r["logw_trace"], "beta": beta}, **extra)

    def _ais_by_steps(self, x, z0, draw, beta, stds, mu0, lv0, iters_per_launch):
        """Route "step" of nll_ais: eval_cond_ll for the scores, lv_ais_step_f32 for everything else.  The launch that decides
        iteration i also applies iteration i + 1's increment and writes its proposals: one launch per iteration."""
        dev = z0.device
        B, C, nz = z0.shape
        total = len(stds)
        per = _eng.iters_per_launch_for("nll_ais", iters_per_launch, x)
        f32, i32, f64 = (dict(dtype=t, device=dev) for t in (torch.float32, torch.int32, torch.float64))
        cur, prop = z0.clone(), z0.clone()
        g, lq, logw, accepts = torch.zeros(B, C, **f32), torch.zeros(B, C, **f32), torch.zeros(B, C, **f64), torch.zeros(B, C, **i32)
        ratios, flags, trace = torch.empty(total, B, C, **f32), torch.empty(total, B, C, **i32), torch.empty(total, B, C, **f64)
        noise = _eng.NoiseCursor(draw, total, per)
        try:
            cond0 = self.eval_cond_ll(x, cur)
        except (TypeError, AttributeError) as e:
            if torch.is_tensor(x):
                raise
            raise ValueError("nll_ais: this decoder's eval_cond_ll does not take a variable-length pair (%s)" % e)
        _eng.ais_step(cond0, prop, cur, g, lq, logw, accepts, None, 0.0, noise.first(), stds[0], beta[1] - beta[0],
                      mu0, lv0, init=True, logw_out_next=trace[0])
        for it in range(total):                                   # iteration it + 1 of the contract, at beta[it + 1]
            cond = self.eval_cond_ll(x, prop)
            u_it, eps_next = noise.step(it)
            more = it + 1 < total
            _eng.ais_step(cond, prop, cur, g, lq, logw, accepts, u_it, beta[it + 1], eps_next, stds[it + 1] if more else 0.0,
                          beta[it + 2] - beta[it + 1] if more else 0.0, mu0, lv0, ratio_out=ratios[it], flag_out=flags[it],
                          logw_out_next=trace[it + 1] if more else None)
        return {"logw": logw, "cur": cur, "g": g, "accepts": accepts, "ratios": ratios, "flags": flags, "logw_trace": trace}

    # True: transition="hmc" takes the decoder engine's session (LSTMDecoderEngine.hmc_ais) where _fused_hmc_ok allows it; False
    # forces the generic route (A/B runs, tests, the bench baseline)
    fused_hmc = True

    def _fused_hmc_ok(self, x, B, C):
        """Route "hmc-fused": _fused_decoder's conditions (the session runs in eval arithmetic: dropout does not matter), B * C
        decoder rows inside the session's envelope."""
        eng = self._fused_decoder(self.fused_hmc, x)
        return eng is not None and eng.svi_supported(B, C)

    def _hmc_arguments(self, who, field, leapfrog, step_size, adapt, step_bounds):
        """-> (L, step_size, None or (up, down, eps_min, eps_max)) or ValueError; up / down are rounded to float32 here, as the
        kernel receives them."""
        L = int(leapfrog)
        if L < 1:
            raise ValueError("%s: leapfrog >= 1 expected" % who)
        if step_size is None:
            if not hasattr(self.args, field):
                raise ValueError("%s: pass step_size or set args.%s (there is no default step size)" % (who, field))
            step_size = getattr(self.args, field)
        step_size = float(step_size)
        lo, hi = (float(v) for v in step_bounds)
        if not (0.0 < step_size < float("inf")) or not (0.0 < lo <= hi < float("inf")):
            raise ValueError("%s: step_size > 0 and step_bounds 0 < min <= max expected" % who)
        if adapt is None:
            return L, step_size, None
        target, rate = (float(v) for v in adapt)
        if not (0.0 < target < 1.0 and 0.0 < rate < float("inf")):
            raise ValueError("%s: adapt = (target in (0, 1), rate > 0) expected" % who)
        up, down = (float(torch.tensor(math.exp(v), dtype=torch.float32)) for v in (rate * (1.0 - target), -rate * target))
        return L, step_size, (up, down, lo, hi)

    def _hmc_run(self, who, x, chains, beta, init, noise, generator, L, step_size, adapt, keep, iters_per_launch):
        """The Hamiltonian chains of nll_ais (init "prior" / "encoder") and sample_from_posterior (init "sampler": z_0 from the
        encoder, q0 the prior) -> (engine.hmc_chain's result, route).  Every refusal comes before anything is launched; the
        decoder runs in eval arithmetic and the training flags are restored."""
        if isinstance(x, (tuple, list)):
            raise ValueError("%s: transition='hmc' does not take variable-length batches (x, lengths); batch by length" % who)
        per = _eng.iters_per_launch_for(who, iters_per_launch, x)
        z0, draw = self._chain_noise(who, x, chains, len(beta) - 1, noise, generator, name="mom")
        flags = [(m, m.training) for m in self.modules()]
        try:
            self.eval()
            with torch.no_grad():
                z0, mu0, lv0 = self._chain_start(x, chains, init, z0, generator)
                if self._fused_hmc_ok(x, x.size(0), chains):
                    return self.decoder._hip.hmc_ais(x, z0, draw, beta, L, step_size, adapt, mu0, lv0, keep, per), "hmc-fused"
                return self._hmc_generic(x, z0, draw, beta, L, step_size, adapt, mu0, lv0, keep, per), "hmc-generic"
        finally:
            for m, t in flags:
                m.training = t

    def _hmc_generic(self, x, z0, draw, beta, L, step_size, adapt, mu0, lv0, keep, iters_per_launch):
        """Route "hmc-generic": rec and d rec / d z from what every decoder has -- reconstruct_error and its autograd backward, as
        _svi_generic gets them -- and lv_hmc_leap_f32 (one plain gradient: parts = 1) for everything else."""
        pos = z0.clone()

        def score():
            with torch.enable_grad():
                z = pos.detach().requires_grad_(True)
                rec = self.decoder.reconstruct_error(x, z)
                dz = torch.autograd.grad(rec, z, torch.ones_like(rec))[0]
            return rec.detach().float().reshape(-1).contiguous(), dz.float().contiguous(), 1
        with self._decoder_gradients_preserved(z0.device):
            return _eng.hmc_chain(score, pos, draw, beta, L, step_size, adapt, mu0, lv0, keep, iters_per_launch)

    @contextlib.contextmanager
    def _decoder_gradients_preserved(self, dev):
        """A decoder backward under torch autograd leaves weight gradients as by-products: the engine's flat gradient buffers are
        saved before and restored after, and the parameters' .grad are put back (torch.autograd.grad asks for dz only)."""
        eng = getattr(self.decoder, "_hip", None)
        if hasattr(eng, "ensure"):
            eng.ensure(dev)
        flat = getattr(eng, "flat", None)
        grads = [(p, p.grad) for p in self.decoder.parameters()]
        saved = [s[0].clone() for s in flat._slots] if flat is not None else None
        detached = getattr(flat, "detached", None)
        try:
            yield
        finally:
            if saved is not None:
                for slot, keep_ in zip(flat._slots, saved):
                    slot[0].copy_(keep_)
                flat.detached = detached
            for p, g0 in grads:
                p.grad = g0

    # True: refine_posterior takes the engine's refinement session (lv_svi_step_f32, lv_dec_tail_dz_f32) where _fused_svi_ok
    # allows it; False forces the generic route (A/B runs, the tests' second oracle, the bench baseline)
    fused_svi = True

    def _fused_svi_ok(self, x, B, ns):
        """Route "fused" of refine_posterior: _fused_decoder's conditions (the refinement runs in eval arithmetic: dropout does not
        matter), B * ns decoder rows inside the LDS budget of the decoder's batch-sized ends."""
        eng = self._fused_decoder(self.fused_svi, x)
        return eng is not None and eng.svi_supported(B, ns)

    def refine_posterior(self, x, steps=20, lr=1.0, momentum=0.5, clip=5.0, kl_weight=1.0, nsamples=1, noise=None, generator=None,
                         keep="best", return_info=False):
        """Stochastic variational inference on the encoder's output (Cremer et al. 2018; the inference half of SA-VAE, Kim et al.
        2018) -> (mu, logvar), each (batch, nz), detached.  The decoder is frozen and runs in eval arithmetic (no dropout) whatever
        `training` says; each sentence's phi = (mu, logvar) starts at the encoder's values and takes `steps` steps on its own
            L_b(phi) = (1/ns) sum_s rec(x_b, mu + eps_s * exp(logvar / 2)) + kl_weight * KL(phi)
        with the noise eps held fixed over the iterations (L_b is then a deterministic function of phi):
            g = grad L_b;  g *= min(1, clip / (|g|_2 + 1e-6)) (norm over the sentence's 2 nz values);  v = momentum * v + g;
            phi -= lr * v.
        steps = K costs K + 1 decoder forwards and K backwards to z.  keep = "best": the iterate with the smallest L_b (the earliest
        on a tie); "last": phi_K.  L_b(encoder) - L_b(refined) is the sentence's amortization gap (evaluation.calc_amortization_gap).

        noise: eps (batch, nsamples, nz) float32 on x's device; otherwise drawn once with torch.randn on x's device (`generator`
        optional).  Nothing of the model changes: parameters, gradients (.grad and the engines' flat buffers), buffers and the
        training flags are as before, and with `noise` given so is every RNG state.

        Routes (class switch fused_svi = False forces the second):
          "fused":   LSTM decoder -- engine.LSTMDecoderEngine.svi_refine: everything that does not depend on z once per call, per
                     iteration no weight-gradient product, no dX, no embedding scatter;
          "generic": PixelCNNDecoderV2 (its eval-mode BatchNorm backward: lv_bn_eval_bwd_f32), batches beyond the fused envelope,
                     the second oracle and the bench baseline: per iteration decoder.reconstruct_error under eval, its autograd
                     backward (weight gradients land in scratch that is restored afterwards), lv_reparam_kl_bwd_f32 and the
                     update in torch.
        return_info: also {"trace": [steps+1, batch] (L_b of phi_0 .. phi_K), "loss0", "loss", "kl", "rec" (L_b, analytic KL and
        sample-mean reconstruction term of the returned iterate, as the loop computed them), "route"}."""
        steps, nsamples = int(steps), int(nsamples)
        lr, momentum, clip, kl_weight = float(lr), float(momentum), float(clip), float(kl_weight)
        if steps < 0 or nsamples < 1:
            raise ValueError("refine_posterior: steps >= 0 and nsamples >= 1 expected")
        if not (lr > 0.0 and clip > 0.0 and 0.0 <= momentum < 1.0):
            raise ValueError("refine_posterior: lr > 0, clip > 0 and 0 <= momentum < 1 expected")
        if keep not in ("best", "last"):
            raise ValueError("refine_posterior: keep is 'best' or 'last'")
        if isinstance(x, (tuple, list)):
            raise ValueError("refine_posterior: variable-length batches (x, lengths) are not supported; batch by length")
        B, dev = x.size(0), x.device
        if noise is not None:
            if not torch.is_tensor(noise) or tuple(noise.shape) != (B, nsamples, self.nz) or noise.dtype != torch.float32 \
                    or noise.device != dev:
                raise ValueError("refine_posterior: noise must be a float32 tensor of shape (%d, %d, %d) on %s" % (B, nsamples, self.nz, dev))
        flags = [(m, m.training) for m in self.modules()]
        try:
            self.eval()
            with torch.no_grad():
                mulv0 = self.encoder._forward_mulv(x).detach().float().contiguous()
                if steps == 0 and not return_info:          # nothing to evaluate: no noise is drawn
                    return mulv0[:, :self.nz].clone(), mulv0[:, self.nz:].clone()
                eps = noise.contiguous() if noise is not None else torch.randn(B, nsamples, self.nz, device=dev, generator=generator)
                if self._fused_svi_ok(x, B, nsamples):
                    route = "fused"
                    eng = self.decoder._hip
                    r = eng.svi_refine(x, mulv0, eps, steps, lr, momentum, clip, kl_weight)
                    _eng.check_persistent_status(eng)       # a timed-out persistent launch: no half-refined result
                else:
                    route = "generic"
                    r = self._svi_generic(x, mulv0, eps, steps, lr, momentum, clip, kl_weight)
        finally:
            for m, t in flags:
                m.training = t
        trace = r["trace"]
        if keep == "best":
            mulv, loss = r["best"], r["best_loss"]
        else:
            mulv, loss = r["last"], trace[steps]
        mu, logvar = mulv[:, :self.nz].clone(), mulv[:, self.nz:].clone()
        if not return_info:
            return mu, logvar
        # rec / kl of the returned iterate as the loop saw them (argmin: the first minimum, the iterate the strict '<' kept)
        k = trace.argmin(dim=0, keepdim=True) if keep == "best" else torch.full((1, B), steps, dtype=torch.int64, device=dev)
        return mu, logvar, {"trace": trace, "loss0": trace[0].clone(), "loss": loss, "kl": r["kl_trace"].gather(0, k)[0],
                            "rec": r["rec_trace"].gather(0, k)[0], "route": route}

    def _svi_generic(self, x, mulv0, eps, steps, lr, momentum, clip, kl_weight):
        """Route "generic" of refine_posterior, from what every decoder has: reconstruct_error and its autograd backward for dz,
        lv_reparam_kl_fwd/bwd_f32 for the variational side, the update in torch.  The decoder's weight gradients are by-products:
        its engine's flat gradient buffers are saved before and restored after, and the parameters' .grad are not touched
        (torch.autograd.grad asks for dz only)."""
        B, ns = eps.shape[0], eps.shape[1]
        dev = mulv0.device
        phi = mulv0.clone()
        vel = torch.zeros_like(phi)
        best = phi.clone()
        best_loss = torch.full((B,), float("inf"), dtype=torch.float32, device=dev)
        trace = torch.empty(steps + 1, B, dtype=torch.float32, device=dev)
        rec_trace, kl_trace = torch.empty_like(trace), torch.empty_like(trace)
        dkl = torch.full((B,), kl_weight, dtype=torch.float32, device=dev)
        with self._decoder_gradients_preserved(dev):
            for k in range(steps + 1):
                z, kl = _eng.reparam_kl_forward(phi, eps)
                with torch.enable_grad():
                    z = z.detach().requires_grad_(k < steps)
                    rec_s = self.decoder.reconstruct_error(x, z)
                    dz = torch.autograd.grad(rec_s, z, torch.full_like(rec_s, 1.0 / ns))[0] if k < steps else None
                rec = rec_s.detach().sum(dim=1) / ns
                loss = rec + kl_weight * kl
                trace[k], rec_trace[k], kl_trace[k] = loss, rec, kl
                better = loss < best_loss
                best = torch.where(better.unsqueeze(1), phi, best)
                best_loss = torch.where(better, loss, best_loss)
                if k == steps:
                    break
                g = _eng.reparam_kl_backward(phi, eps, dz.contiguous(), dkl)
                g = g * torch.clamp(clip / (g.norm(dim=1, keepdim=True) + 1e-6), max=1.0)
                vel = momentum * vel + g
                phi = phi - lr * vel
        return {"last": phi, "best": best, "best_loss": best_loss, "trace": trace, "rec_trace": rec_trace, "kl_trace": kl_trace}

    def calc_infer_mean(self, x):
        return self.encoder.forward(x)[0]

    def calc_mi_q(self, x):
        return self.encoder.calc_mi(x)

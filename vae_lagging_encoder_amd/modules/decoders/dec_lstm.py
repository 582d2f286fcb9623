"""LSTMDecoder -- drop-in for the reference's modules/decoders/dec_lstm.py:17-161 on MI355X (training path).

Same constructor, containers, construction order and state_dict keys (`embed.weight` with padding_idx=-1 => V-1
(SURVEY.md G3), `trans_linear.weight`, `lstm.*_l0`, `pred_linear.weight`).  `reconstruct_error` runs the HIP path:
embedding gather fused with dropout_in, z-projection folded into the input GEMM epilogue (the cat((embed, z)) is
never materialised), fused LSTM step kernels with dropout_out in the epilogue, f32 MFMA vocabulary projection,
row softmax-NLL; hand-written backward.  Generation (beam / greedy / sample decoding, reference lines 163-367;
SURVEY.md 8f row 4) steps the same kernels one token at a time through engine.LSTMDecodeStepper; every strategy decodes the
whole batch together with every decision on the device: beam search through engine.LSTMBeamSearcher (csrc/lv_beam.hip), greedy
and sample decoding through engine.LSTMRollout (csrc/lv_rollout.hip).
"""
import numpy as np
import torch
import torch.nn as nn

from ... import _lib
from ... import engine as _eng
from .decoder import DecoderBase


class _DecoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, x, z, mask_in, mask_out, p_in, p_out, *params):
        rec = eng.forward(x, z, mask_in, mask_out, p_in, p_out)
        ctx.eng = eng
        ctx.gen = eng.gen
        ctx.zshape = z.shape
        return rec.clone()

    @staticmethod
    def backward(ctx, drec):
        eng = ctx.eng
        eng.flat.before_autograd_backward()
        dz = eng.backward(drec, ctx.gen).clone().view(ctx.zshape)
        eng.join()
        return (None, None, dz, None, None, None, None) + eng.flat.deliver_grads()


class _VarDecoderFn(torch.autograd.Function):
    """_DecoderFn on a padded batch with lengths (engine.LSTMDecoderEngine.forward(lengths=))."""

    @staticmethod
    def forward(ctx, eng, x, z, mask_in, mask_out, p_in, p_out, lengths, *params):
        rec = eng.forward(x, z, mask_in, mask_out, p_in, p_out, lengths=lengths)
        ctx.eng = eng
        ctx.gen = eng.gen
        ctx.zshape = z.shape
        return rec.clone()

    @staticmethod
    def backward(ctx, drec):
        eng = ctx.eng
        eng.flat.before_autograd_backward()
        dz = eng.backward(drec, ctx.gen).clone().view(ctx.zshape)
        eng.join()
        return (None, None, dz, None, None, None, None, None) + eng.flat.deliver_grads()


class _DecoderByLengthFn(torch.autograd.Function):
    """The A/B route (VarLSTMDecoder.masked = False): every group of equal length through the equal-length engine, with the
    group's slices of z and of the two keep-masks."""

    @staticmethod
    def forward(ctx, eng, x, z, mask_in, mask_out, p_in, p_out, lengths, *params):
        B, T = x.shape
        ns, nz = int(z.shape[1]), int(z.shape[2])
        H = eng.dims()[2]
        rec = torch.empty(B, ns, dtype=torch.float32, device=x.device)
        ctx.groups = _eng.length_groups(lengths)
        ctx.book = _eng.GroupedBackward(eng)
        for n, rows in ctx.groups:
            Bg = int(rows.numel())
            m_in = None if mask_in is None else mask_in[rows, :n - 1].contiguous()
            m_out = None if mask_out is None else mask_out.view(B, ns, T - 1, H)[rows, :, :n - 1].reshape(Bg * ns, n - 1, H).contiguous()
            rec[rows] = eng.forward(x[rows, :n].contiguous(), z[rows].contiguous(), m_in, m_out, p_in, p_out).view(Bg, ns)
            ctx.book.after_forward(eng._ws(Bg * ns, n - 1, ns))
        ctx.eng, ctx.zshape = eng, (B, ns, nz)
        return rec.view(B * ns)

    @staticmethod
    def backward(ctx, drec):
        eng = ctx.eng
        B, ns, nz = ctx.zshape
        eng.flat.before_autograd_backward()
        dz = torch.empty(B, ns, nz, dtype=torch.float32, device=drec.device)
        drec = drec.reshape(B, ns)
        for i, (n, rows) in enumerate(ctx.groups):
            Bg = int(rows.numel())
            d = drec[rows].reshape(-1).contiguous()
            dz[rows] = ctx.book.backward(i, lambda: eng._ws(Bg * ns, n - 1, ns), lambda gen: eng.backward(d, gen)).view(Bg, ns, nz)
        return (None, None, dz, None, None, None, None, None) + eng.flat.deliver_grads()


class LSTMDecoder(DecoderBase):
    """LSTM decoder with constant-length batching (reference dec_lstm.py:17-161)."""

    def __init__(self, args, vocab, model_init, emb_init):
        super(LSTMDecoder, self).__init__()
        self.ni = args.ni
        self.nh = args.dec_nh
        self.nz = args.nz
        self.vocab = vocab
        self.device = args.device

        # "no padding" in the reference's comment, but padding_idx=-1 resolves to row V-1 (G3)
        self.embed = nn.Embedding(len(vocab), args.ni, padding_idx=-1)
        self.dropout_in = nn.Dropout(args.dec_dropout_in)
        self.dropout_out = nn.Dropout(args.dec_dropout_out)
        # initial cell state from z
        self.trans_linear = nn.Linear(args.nz, args.dec_nh, bias=False)
        # z is concatenated to every step input
        self.lstm = nn.LSTM(input_size=args.ni + args.nz, hidden_size=args.dec_nh, num_layers=1, batch_first=True)
        self.pred_linear = nn.Linear(args.dec_nh, len(vocab), bias=False)

        vocab_mask = torch.ones(len(vocab))
        self.loss = nn.CrossEntropyLoss(weight=vocab_mask, reduction="none")

        self.reset_parameters(model_init, emb_init)
        self._hip = _eng.LSTMDecoderEngine(self)

    def reset_parameters(self, model_init, emb_init):
        for param in self.parameters():
            model_init(param)
        emb_init(self.embed.weight)

    def _params(self):
        return (self.embed.weight, self.trans_linear.weight, self.lstm.weight_ih_l0, self.lstm.weight_hh_l0,
                self.lstm.bias_ih_l0, self.lstm.bias_hh_l0, self.pred_linear.weight)

    def _draw_masks(self, B, Td, device):
        """nn.Dropout keep-masks for dropout_in (B,Td,ni) / dropout_out (B,Td,nh); None when not training."""
        p_in, p_out = self.dropout_in.p, self.dropout_out.p
        m_in = m_out = None
        if self.training and p_in > 0:
            m_in = torch.empty(B, Td, self.ni, device=device).bernoulli_(1 - p_in).to(torch.uint8)
        if self.training and p_out > 0:
            m_out = torch.empty(B, Td, self.nh, device=device).bernoulli_(1 - p_out).to(torch.uint8)
        return m_in, m_out

    def reconstruct_error(self, x, z, masks=None):
        """Token cross entropy summed over time.  x (batch, seq_len) int64, z (batch, n_sample, nz)
        -> (batch, n_sample).  `masks=(mask_in, mask_out)` injects the dropout keep-masks (parity tests)."""
        B, T = x.shape
        ns = z.size(1)
        self._hip.ensure(x.device)
        if masks is None:
            m_in, m_out = self._draw_masks(B, T - 1, x.device)
            if ns > 1 and m_out is not None:
                m_out = torch.empty(B * ns, T - 1, self.nh, device=x.device).bernoulli_(1 - self.dropout_out.p).to(torch.uint8)
        else:
            m_in, m_out = masks
            m_in = None if m_in is None else m_in.to(device=x.device, dtype=torch.uint8).contiguous()
            m_out = None if m_out is None else m_out.to(device=x.device, dtype=torch.uint8).contiguous()
        if ns > 1:
            # dec_lstm.py:86-94: the same (dropped) word embeddings for every sample of a sentence
            x = x.repeat_interleave(ns, dim=0)
            if m_in is not None:
                m_in = m_in.repeat_interleave(ns, dim=0).contiguous()
            z = z.reshape(B * ns, 1, self.nz)
        rec = _DecoderFn.apply(self._hip, x, z, m_in, m_out, self.dropout_in.p, self.dropout_out.p, *self._params())
        return rec.view(B, ns)

    def log_probability(self, x, z):
        """log p(x|z): (batch, n_sample)."""
        return -self.reconstruct_error(x, z)

    def decode(self, input, z):
        """Logits (batch*n_sample, seq_len, vocab) of the teacher-forced decoder (reference dec_lstm.py:66-111).
        Inference-only view of the HIP path's logits buffer (not differentiable; training goes through
        reconstruct_error, which never hands logits back to Python)."""
        B, T = input.shape
        ns = z.size(1)
        with torch.no_grad():
            # run the teacher-forced path on `input` as the source sequence: append a dummy target column
            x = torch.cat((input, input[:, -1:]), dim=1)
            fused, self._hip.fused_nll = self._hip.fused_nll, False       # this view needs the f32 logits image
            try:
                self.reconstruct_error(x, z)
            finally:
                self._hip.fused_nll = fused
            w = self._hip._ws(B * ns, T)
            V = len(self.vocab)
            return w.logits[:, :V].reshape(T, B * ns, V).transpose(0, 1).contiguous()

    # ---- generation (reference dec_lstm.py:163-367) ------------------------------------------------------
    def _stepper(self, device):
        st = getattr(self, "_gen", None)
        if st is None or st.device != torch.device(device):
            st = self._gen = _eng.LSTMDecodeStepper(self._hip, device)
        return st

    def _roll_out(self, z, pick):
        """Shared loop of greedy_decode / sample_decode (dec_lstm.py:270-367): every sentence starts at <s>, a step feeds the
        picked word back, a sentence stops after emitting </s>, at most 99 words."""
        batch_size = z.size(0)
        dev = z.device
        st = self._stepper(dev)
        z2 = z.reshape(batch_size, -1).float()
        with torch.no_grad():
            h, c = st.init_state(z2)
            tok = torch.full((batch_size,), self.vocab["<s>"], dtype=torch.int64, device=dev)
            end = self.vocab["</s>"]
            alive = torch.ones(batch_size, dtype=torch.bool, device=dev)
            picked, masks = [], []
            length_c = 1
            while length_c < 100:
                logits, h, c = st.step(tok, z2, h, c)
                tok = pick(st, logits)
                picked.append(tok)
                masks.append(alive)
                alive = alive & (tok != end)
                length_c += 1
                if not bool(alive.any().item()):            # the reference's mask.sum().item() != 0 test (one host read per step)
                    break
        ids = torch.stack(picked, dim=1).cpu().tolist()
        keep = torch.stack(masks, dim=1).cpu().tolist()
        return [[self.vocab.id2word(w) for w, k in zip(row, krow) if k] for row, krow in zip(ids, keep)]

    # True: greedy_decode / sample_decode keep the whole loop on the device through engine.LSTMRollout (lv_rollout.hip); False
    # selects _roll_out above, one host decision per word (A/B runs, the tests' reference)
    batched_rollout = True
    rollout_poll = 8             # steps between the device route's reads of the "sentences still alive" counter

    def _rollout(self, device):
        st = self._stepper(device)
        ro = getattr(self, "_ro", None)
        if ro is None or ro.st is not st:
            ro = self._ro = _eng.LSTMRollout(st)
        ro.poll = self.rollout_poll
        return ro

    def _decode_loop(self, z, pick, sample, generator, return_info, filt=None):
        batch_size = z.size(0)
        if self.batched_rollout and batch_size > 0:
            with torch.no_grad():
                ids, info = self._rollout(z.device).decode(z.reshape(batch_size, -1).float(), self.vocab["<s>"], self.vocab["</s>"],
                                                            sample=sample, generator=generator, **(filt or {}))
            decoded = [[self.vocab.id2word(w) for w in row] for row in ids]
            return (decoded, info) if return_info else decoded
        if filt:
            return self._roll_out_filtered(z, generator, return_info, filt)
        if not return_info:
            return self._roll_out(z, pick)
        # the per-step route with the same per-sentence quantities, from the stepper's helpers
        rec = {"lp": [], "gap": []}

        def recording_pick(st, logits):
            tok = pick(st, logits)
            rec["lp"].append(st.log_softmax(logits).gather(1, tok.view(-1, 1)).view(-1))
            if not sample:
                top = torch.topk(logits, min(2, logits.shape[1]), dim=1)[0]
                rec["gap"].append(top[:, 0] - top[:, -1] if top.shape[1] > 1 else torch.full_like(top[:, 0], float("inf")))
            return tok
        decoded = self._roll_out(z, recording_pick)
        steps = np.asarray([len(s) for s in decoded], dtype=np.int64)
        live = torch.arange(len(rec["lp"])).view(1, -1) < torch.from_numpy(steps).view(-1, 1)      # [n][steps queued]
        lp = torch.stack(rec["lp"], dim=1).cpu()
        info = {"score": torch.where(live, lp, torch.zeros_like(lp)).sum(dim=1).numpy().astype(np.float32), "steps": steps}
        if not sample:
            gap = torch.stack(rec["gap"], dim=1).cpu()
            info["min_margin"] = torch.where(live, gap, torch.full_like(gap, float("inf"))).min(dim=1)[0].numpy().astype(np.float32)
        return decoded, info

    def _roll_out_filtered(self, z, generator, return_info, filt):
        """The per-step route of a tempered / truncated sample_decode: the loop of _roll_out with lv_sample_filtered_rows_f32 as the
        pick.  The running sums are kept the way the device route keeps them (f32, one addition per live step), so both routes
        return the same bits."""
        n, dev = z.size(0), z.device
        end = self.vocab["</s>"]
        run = {"score": torch.zeros(n, dtype=torch.float32, device=dev), "q": torch.zeros(n, dtype=torch.float32, device=dev),
               "alive": torch.ones(n, dtype=torch.bool, device=dev)}

        def pick(st, logits):
            u = torch.rand(logits.shape[0], device=logits.device, generator=generator)
            tok, lp, lq = st.sample_filtered(logits, u, **filt)
            live = run["alive"]
            run["score"] = torch.where(live, run["score"] + lp, run["score"])
            run["q"] = torch.where(live, run["q"] + lq, run["q"])
            run["alive"] = live & (tok != end)
            return tok
        decoded = self._roll_out(z, pick)
        if not return_info:
            return decoded
        return decoded, {"score": run["score"].cpu().numpy(), "steps": np.asarray([len(s) for s in decoded], dtype=np.int64),
                         "proposal_score": run["q"].cpu().numpy()}

    def greedy_decode(self, z, return_info=False):
        """Greedy decoding from z (batch_size, nz) -> list of word lists (reference dec_lstm.py:270-318): no <s>, </s> included
        when emitted, at most 99 words.  return_info=True also returns a dict of per-sentence numpy arrays: `score`
        (log p(words | z)), `steps` (words emitted), `min_margin` (smallest top-1 minus top-2 logit gap over the sentence's
        steps)."""
        return self._decode_loop(z, lambda st, logits: st.argmax(logits), False, None, return_info)

    def sample_decode(self, z, generator=None, return_info=False, temperature=1.0, top_k=0, top_p=1.0):
        """Ancestral sampling from z (reference dec_lstm.py:320-367).  The categorical draw is an inverse-CDF pick from a device
        uniform (torch.rand, one call of batch_size values per step; `generator` makes it reproducible) instead of
        torch.multinomial's sampler: same distribution, different stream.  Both routes draw the same uniforms in the same order;
        the device route consumes up to rollout_poll - 1 further draws after the last sentence has ended.  return_info=True also
        returns `score` and `steps` per sentence.

        temperature / top_k / top_p (the reference has none) draw every word from softmax(logits / temperature) restricted to the
        top_k most likely words (0: all) and then to the shortest prefix of those that holds top_p of their probability (1: all),
        renormalised: lv_pick.h's rule, lv_rollout_pick_filtered_f32 on the device route and lv_sample_filtered_rows_f32 on the
        per-step route, from the same uniforms.  `score` stays log p(words | z) under the model itself; return_info=True then
        adds `proposal_score`, the log-probability of the sentence under the distributions actually drawn from.  With the
        neutral values (1.0, 0, 1.0) the call is the plain one, launch for launch.  ValueError before any launch: temperature
        <= 0 or not finite, top_k not an integer or negative, top_p outside (0, 1]."""
        neutral = _eng.sampling_filter(temperature, top_k, top_p)[3]
        filt = None if neutral else {"temperature": temperature, "top_k": top_k, "top_p": top_p}

        def pick(st, logits):
            u = torch.rand(logits.shape[0], device=logits.device, generator=generator)
            return st.sample(logits, u)
        return self._decode_loop(z, pick, True, generator, return_info, filt)

    # True: beam_search_decode decodes the whole batch together through engine.LSTMBeamSearcher (lv_beam.hip) when the shape is
    # inside its envelope; False forces the sentence-by-sentence route below (A/B runs, tests)
    batched_beam = True
    beam_poll = 8                # steps between the batched route's reads of the "sentences still active" counter

    def _beam_searcher(self, device):
        st = self._stepper(device)
        bs = getattr(self, "_beam", None)
        if bs is None or bs.st is not st:
            bs = self._beam = _eng.LSTMBeamSearcher(st)
        bs.poll = self.beam_poll
        return bs

    def beam_search_decode(self, z, K=5, return_info=False):
        """Beam search (reference dec_lstm.py:163-268): live hypotheses are expanded together, the K - len(completed) best
        continuations over (hypothesis, word) survive, a hypothesis completes when it emits </s>, the best by total
        log-probability is returned with <s> in front.  With `batched_beam` and a shape inside the kernels' envelope (K <= 16,
        K * V < 2^31, batch * K <= 8192) all sentences are decoded together with every decision on the device; otherwise
        sentence by sentence as the reference does.  return_info=True also returns a dict of per-sentence numpy arrays: `score`
        (the winner's log-probability), `steps`, `n_completed`, `min_margin` (smallest gap, over the sentence's steps, between
        the last accepted and the first rejected candidate)."""
        batch_size = z.size(0)
        if self.batched_beam and batch_size > 0:
            bs = self._beam_searcher(z.device)
            if bs.supported(batch_size, K):
                with torch.no_grad():
                    ids, info = bs.search(z.reshape(batch_size, -1).float(), K, self.vocab["<s>"], self.vocab["</s>"])
                decoded = [[self.vocab.id2word(w) for w in row] for row in ids]
                return (decoded, info) if return_info else decoded
        return self._beam_search_per_sentence(z, K, return_info)

    def _beam_search_per_sentence(self, z, K=5, return_info=False):
        """The reference's procedure, sentence by sentence with the decisions on the host (the A/B route of beam_search_decode)."""
        batch_size = z.size(0)
        dev = z.device
        st = self._stepper(dev)
        z2 = z.reshape(batch_size, -1).float()
        V = len(self.vocab)
        end = self.vocab["</s>"]
        decoded = []
        info = {"score": [], "steps": [], "n_completed": [], "min_margin": []}
        with torch.no_grad():
            h_init, c_init = st.init_state(z2)
            for idx in range(batch_size):
                # a hypothesis: (word ids so far, log-probability); states live in (h, c) rows aligned with `live`
                live = [([self.vocab["<s>"]], 0.0)]
                h, c = h_init[idx:idx + 1].clone(), c_init[idx:idx + 1].clone()
                completed = []
                t = 0
                margin = float("inf")
                while len(completed) < K and t < 100:
                    t += 1
                    n = len(live)
                    tok = torch.tensor([hyp[0][-1] for hyp in live], dtype=torch.int64, device=dev)
                    logits, h, c = st.step(tok, z2[idx:idx + 1].expand(n, -1), h, c)
                    prev = torch.tensor([hyp[1] for hyp in live], dtype=torch.float32, device=dev)
                    scores = st.log_softmax(logits, prev).reshape(-1)
                    log_prob, indexes = torch.topk(scores, K - len(completed))
                    if return_info and scores.numel() > K - len(completed):
                        # the accepted set stays topk(K - done)'s; one more candidate only to measure the gap to the first rejected
                        wider = torch.topk(scores, K - len(completed) + 1)[0]
                        margin = min(margin, float(log_prob[-1] - wider[-1]))
                    live_ids = (indexes // V).tolist()
                    word_ids = (indexes % V).tolist()
                    new_live, keep_rows = [], []
                    for live_id, word_id, lp in zip(live_ids, word_ids, log_prob.tolist()):
                        hyp = (live[live_id][0] + [word_id], lp)
                        if word_id == end:
                            completed.append(hyp)
                        else:
                            new_live.append(hyp)
                            keep_rows.append(live_id)
                    live = new_live
                    if len(completed) == K or not live:
                        break
                    rows = torch.tensor(keep_rows, dtype=torch.int64, device=dev)
                    h, c = h.index_select(0, rows), c.index_select(0, rows)
                n_completed = len(completed)
                completed.extend(live)
                best = max(completed, key=lambda hyp: hyp[1]) if completed else ([self.vocab["<s>"]], 0.0)
                decoded.append([self.vocab.id2word(w) for w in best[0]])
                for key, val in (("score", best[1]), ("steps", t), ("n_completed", n_completed), ("min_margin", margin)):
                    info[key].append(val)
        if not return_info:
            return decoded
        return decoded, {"score": np.asarray(info["score"], dtype=np.float32), "steps": np.asarray(info["steps"], dtype=np.int64),
                         "n_completed": np.asarray(info["n_completed"], dtype=np.int64),
                         "min_margin": np.asarray(info["min_margin"], dtype=np.float32)}


class VarLSTMDecoder(LSTMDecoder):
    """LSTM decoder with variable-length batching (reference dec_lstm.py:370-476): `x` is a pair (x_, sents_len) of a padded
    (batch, seq_len) int64 tensor and the sentence lengths; row b is decoded for sents_len[b] - 1 steps and only those steps'
    token NLL is summed.  Construction follows the reference line by line -- the parent is built, `embed` is replaced by one
    with padding_idx = vocab['<pad>'], and reset_parameters runs a second time -- so a seed gives the reference's weights; the
    state_dict keys are the parent's.  The row vocab['<pad>'] of the embedding's gradient is zero (row V - 1 is not special here).

    Lengths: as VarLSTMEncoder's.  A <pad> id INSIDE a sentence (before its length) is outside the envelope: the reference gives
    such a target weight 0, here it is scored like any other word.  A plain tensor is taken as LSTMDecoder takes it.  The
    generation methods are inherited.  Exact-f32 configuration only."""

    # True: one length-aware pass over the padded batch; False: every group of equal length through LSTMDecoder's path with
    # slices of the same noise (A/B runs, tests)
    masked = True

    def __init__(self, args, vocab, model_init, emb_init):
        super(VarLSTMDecoder, self).__init__(args, vocab, model_init, emb_init)
        self.embed = nn.Embedding(len(vocab), args.ni, padding_idx=vocab["<pad>"])
        vocab_mask = torch.ones(len(vocab))
        vocab_mask[vocab["<pad>"]] = 0
        self.loss = nn.CrossEntropyLoss(weight=vocab_mask, reduction="none")
        self.reset_parameters(model_init, emb_init)
        self._hip = _eng.LSTMDecoderEngine(self)          # (the parent's engine was built around the embedding replaced above)

    def reconstruct_error(self, x, z, masks=None):
        """x = (x_ (batch, seq_len) int64, sents_len), z (batch, n_sample, nz) -> (batch, n_sample).  Random draws as the parent's
        (and the reference's): mask_in (batch, seq_len - 1, ni) per sentence, then mask_out (batch * n_sample, seq_len - 1, nh) per
        decoder row, seq_len being the longest sentence's length; `masks=(mask_in, mask_out)` injects them."""
        if torch.is_tensor(x):
            return super(VarLSTMDecoder, self).reconstruct_error(x, z, masks=masks)
        x, lengths = _eng.varlen_batch(x)
        _eng._refuse_bf16_lengths(self._hip)
        B, T = x.shape
        if z.dim() != 3 or z.shape[0] != B:
            raise _lib.LvaeError("the HIP decoder path takes z of shape [B, nsamples, nz]; got %s for a batch of %d" % (tuple(z.shape), B))
        _eng._same_device("VarLSTMDecoder.reconstruct_error", x.device, z=z)
        ns = z.size(1)
        self._hip.ensure(x.device)
        if masks is None:
            m_in, m_out = self._draw_masks(B, T - 1, x.device)
            if ns > 1 and m_out is not None:
                m_out = torch.empty(B * ns, T - 1, self.nh, device=x.device).bernoulli_(1 - self.dropout_out.p).to(torch.uint8)
        else:
            m_in, m_out = masks
            _eng._same_device("VarLSTMDecoder.reconstruct_error", x.device, mask_in=m_in, mask_out=m_out)

            def cut(m):          # masks drawn for the batch tensor as given: the columns of the cut padding go
                if m is None:
                    return None
                if m.dim() == 3 and m.shape[1] > T - 1:
                    m = m[:, :T - 1]
                return m.to(dtype=torch.uint8).contiguous()
            m_in, m_out = cut(m_in), cut(m_out)
        fn = _VarDecoderFn if self.masked else _DecoderByLengthFn
        rec = fn.apply(self._hip, x, z.float().contiguous(), m_in, m_out, self.dropout_in.p, self.dropout_out.p, lengths, *self._params())
        return rec.view(B, ns)

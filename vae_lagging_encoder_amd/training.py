"""Outer training loop of the reference's text.py, as a reusable driver around the fused inner loop.

text.py:325-510, restated: per epoch a random permutation of the equal-length batches; per batch the KL weight anneals
linearly (kl_start -> 1 over `warm_up` epochs), the AGGRESSIVE inner loop runs while the flag is set (encoder-only steps until
the windowed loss stops improving: AggressiveTextTrainer.inner_loop = text.py:366-400), then one joint step (decoder only while
aggressive, encoder + decoder afterwards, text.py:407-424).  Once per epoch worth of iterations the mutual information on the
validation set decides whether aggressive training goes on ("STOP BURNING" when it drops, text.py:447-455).  Epoch end:
validation loss / NLL / KL / PPL / MI / active units, best-checkpoint bookkeeping, learning-rate decay (x0.5 after
`decay_epoch` = 2 epochs without improvement once epoch >= 15, reload the best weights, stop after `max_decay` = 5 decays,
text.py:463-489), a test-set pass every `test_nepoch` epochs.  The arithmetic is the HIP hot path throughout; the policy is
plain host code with the reference's constants and comparison operators.
"""
import copy
import math
import time

import numpy as np
import torch

from . import engine as _eng
from . import evaluation as E
from .trainer import AggressiveImageTrainer, AggressiveTextTrainer, SemiAmortizedTextTrainer

CLIP_GRAD = 5.0          # text.py:17-20
DECAY_EPOCH = 2
LR_DECAY = 0.5
MAX_DECAY = 5


def guarded_eval(vae, fn, log=print):
    """Run an evaluation pass -- a forward-only use of the engines: there is no transaction gate in it -- and look at the engines'
    persistent-launch status words afterwards (one host read each; every evaluation ends in host reads anyway).  A hand-off
    timeout during the pass would have left garbage in its statistics, which drive best-state selection, learning-rate decay and
    the end of aggressive training: the engines are moved one rung down the fallback ladder (engine.demote_persistent), the event
    is logged, and the pass is run again.  Engines without persistent launches (the image model's) have no status word."""
    engines = [e for e in (getattr(vae.encoder, "_hip", None), getattr(vae.decoder, "_hip", None))
               if e is not None and getattr(e, "status", None) is not None]
    for _ in range(3):
        out = fn()
        bad = [e for e in engines if int(e.status.item()) != 0]
        if not bad:
            return out
        for e in engines:          # both engines take the same rung, as the trainers' _settle does
            if _eng.persist_rung(e) < 2:
                _eng.demote_persistent(e)
            else:
                _eng.reset_persistent_status(e)
        log("persistent LSTM launch timed out during an evaluation pass: engines moved to ladder rung %d (%s), pass repeated" % (
            max(_eng.persist_rung(e) for e in engines), _eng.PERSIST_RUNGS[max(_eng.persist_rung(e) for e in engines)]))
    raise _eng._lib.LvaeError("an evaluation pass kept reporting persistent-launch timeouts on every rung of the fallback ladder")


def _objective(args, trainer):
    """args.objective ("elbo" when the attribute is missing; "iw": the training steps minimise the importance-weighted bound,
    AggressiveTextTrainer(objective="iw")); a trainer that is handed in must have been built with the same one.  The evaluation
    passes are the same for both."""
    objective = getattr(args, "objective", "elbo")
    if objective not in ("elbo", "iw"):
        raise ValueError("args.objective: 'elbo' or 'iw', not %r" % (objective,))
    if trainer is not None and getattr(trainer, "objective", "elbo") != objective:
        raise ValueError("args.objective = %r, but the trainer was built with objective = %r" % (objective, getattr(trainer, "objective", "elbo")))
    return objective


def _iw_estimator(args, trainer, objective):
    """args.iw_estimator ("iwae" when the attribute is missing; "dreg": the doubly-reparameterised estimator of objective "iw",
    DESIGN.md 3.3c); a trainer that is handed in must have been built with the same one."""
    est = getattr(args, "iw_estimator", "iwae")
    if est not in ("iwae", "dreg"):
        raise ValueError("args.iw_estimator: 'iwae' or 'dreg', not %r" % (est,))
    if est != "iwae" and objective != "iw":
        raise ValueError("args.iw_estimator = %r is an estimator of args.objective = 'iw', not of %r" % (est, objective))
    if trainer is not None and getattr(trainer, "iw_estimator", "iwae") != est:
        raise ValueError("args.iw_estimator = %r, but the trainer was built with iw_estimator = %r"
                         % (est, getattr(trainer, "iw_estimator", "iwae")))
    return est


def _free_bits(args, trainer):
    """(args.free_bits, args.free_bits_mode) -- (None, "dim") when the fields are missing: the free-bits objective of the TRAINING
    steps (AggressiveTextTrainer / AggressiveImageTrainer (free_bits=..., free_bits_mode=...)); the evaluation passes
    never apply it.  A trainer that is handed in must have been built with the same pair."""
    fb, mode = getattr(args, "free_bits", None), getattr(args, "free_bits_mode", "dim")
    if fb is not None:
        fb = _eng.check_free_bits(fb, mode)[0]
    if trainer is not None:
        got = (getattr(trainer, "free_bits", None), getattr(trainer, "free_bits_mode", "dim"))
        if got[0] != fb or (fb is not None and got[1] != mode):
            raise ValueError("args.free_bits = %r (%s), but the trainer was built with free_bits = %r (%s)" % (fb, mode, got[0], got[1]))
    return fb, mode


class TextTrainingLoop(object):
    """args fields read (text.py's argparse names): kl_start, warm_up, batch_size, epochs, aggressive, nsamples, test_nepoch,
    iw_nsamples, free_bits / free_bits_mode (None / "dim" when missing: the free-bits objective of the training steps),
    momentum (text.py --momentum: optim.SGD(lr, momentum) on both sides, AggressiveTextTrainer(momentum=...)), and
    objective ("elbo" when missing, or "iw": AggressiveTextTrainer(objective=...)), iw_estimator ("iwae" when missing, or "dreg"),
    and svi_steps (missing or 0: the ordinary steps;
    K > 0: semi-amortized training, SemiAmortizedTextTrainer, with svi_lr, svi_momentum, svi_clip and fd_eps)."""

    def __init__(self, vae, train_batches, val_batches, test_batches, args, n_train_sentences=None, trainer=None,
                 log=print, np_rng=None, seed=783435, noise_fn=None, epoch_hook=None):
        """noise_fn(x) -> (eps, mask_in, mask_out): injects the random draws of every training step (parity replays of a
        recorded reference run, tests/test_policy_replay.py); None draws them on the device.  With args.nsamples = ns > 1
        (text.py --nsamples) in the multi-sample shapes: eps [B][ns][nz], mask_in [B][T-1][ni], mask_out [B*ns][T-1][H].
        A `trainer` that is handed in must have been built with the same nsamples and the same momentum as args'.
        epoch_hook(loop, epoch): called at the top of every epoch, before its batch permutation is drawn (checkpoint / resume
        policies; the replay test re-synchronises the weights there)."""
        self.vae, self.args, self.log = vae, args, log
        self.noise_fn = noise_fn
        self.epoch_hook = epoch_hook
        self.train_batches, self.val_batches, self.test_batches = train_batches, val_batches, test_batches
        self.momentum = float(getattr(args, "momentum", 0))
        if trainer is not None and float(getattr(trainer, "momentum", 0.0)) != self.momentum:
            raise ValueError("args.momentum = %r, but the trainer was built with momentum = %r" % (self.momentum, getattr(trainer, "momentum", 0.0)))
        self.nsamples = int(getattr(args, "nsamples", 1))
        if trainer is not None and getattr(trainer, "nsamples", 1) != self.nsamples:
            raise ValueError("args.nsamples = %d, but the trainer was built with nsamples = %d" % (self.nsamples, getattr(trainer, "nsamples", 1)))
        self.objective = _objective(args, trainer)
        self.iw_estimator = _iw_estimator(args, trainer, self.objective)
        self.free_bits, self.free_bits_mode = _free_bits(args, trainer)
        # args.svi_steps = K > 0: semi-amortized training (SemiAmortizedTextTrainer) with args.svi_lr, svi_momentum,
        # svi_clip and fd_eps (Kim et al.'s defaults when missing); missing or 0: the ordinary steps
        self.svi_steps = int(getattr(args, "svi_steps", 0) or 0)
        if self.svi_steps < 0:
            raise ValueError("args.svi_steps must be >= 0, not %r" % (self.svi_steps,))
        if self.svi_steps > 0 and (bool(args.aggressive) or self.objective == "iw"):
            raise ValueError("args.svi_steps = %d (semi-amortized training) runs neither with aggressive = 1 nor with objective = 'iw'"
                             % self.svi_steps)
        if self.svi_steps > 0 and self.free_bits is not None:
            raise ValueError("args.free_bits is not implemented together with args.svi_steps > 0 (semi-amortized training)")
        if self.svi_steps > 0 and trainer is None:
            trainer = SemiAmortizedTextTrainer(vae, svi_steps=self.svi_steps, svi_lr=float(getattr(args, "svi_lr", 1.0)),
                                               svi_momentum=float(getattr(args, "svi_momentum", 0.5)),
                                               svi_clip=float(getattr(args, "svi_clip", 5.0)), fd_eps=float(getattr(args, "fd_eps", 1e-2)),
                                               lr=1.0, clip=CLIP_GRAD, seed=seed, nsamples=self.nsamples, momentum=self.momentum)
        self.trainer = trainer if trainer is not None else AggressiveTextTrainer(vae, lr=1.0, clip=CLIP_GRAD, seed=seed,
                                                                                 nsamples=self.nsamples, momentum=self.momentum,
                                                                                 objective=self.objective, free_bits=self.free_bits,
                                                                                 free_bits_mode=self.free_bits_mode,
                                                                                 iw_estimator=self.iw_estimator)
        if hasattr(self.trainer, "prepare_batches"):
            self.trainer.prepare_batches(train_batches)          # per-batch index structures, built once with the batch list
        self.rng = np_rng if np_rng is not None else np.random
        n = n_train_sentences if n_train_sentences is not None else sum(int(b.shape[0]) for b in train_batches)
        self.n_train = n
        self.kl_weight = float(args.kl_start)
        self.anneal_rate = (1.0 - args.kl_start) / (args.warm_up * (n / args.batch_size))      # text.py:339
        self.opt = {"not_improved": 0, "lr": 1.0, "best_loss": 1e4}                              # text.py:251
        self.aggressive = bool(args.aggressive)
        self.iter_ = self.decay_cnt = 0
        self.pre_mi = 0.0
        self.best = {"loss": 1e4, "nll": 0.0, "kl": 0.0, "ppl": 0.0, "state": None}
        self.history = []           # one record per epoch
        self.iterations = []        # one record per outer iteration: what text.py's loop body did (batch, kl weight, inner steps)
        self.mi_checks = []         # (pre_mi, cur_mi) of every end-of-epoch aggressive check

    # -- pieces the tests drive directly --------------------------------------------------------------------------------------
    def _eval_mi_au(self):
        self.vae.eval()
        with torch.no_grad():
            mi, au = guarded_eval(self.vae, lambda: (E.calc_mi(self.vae, self.val_batches), E.calc_au(self.vae, self.val_batches)[0]), self.log)
        self.vae.train()
        return mi, au

    def check_aggressive(self):
        """text.py:447-455: called when a full epoch worth of iterations has passed while aggressive."""
        self.vae.eval()
        with torch.no_grad():
            cur_mi = guarded_eval(self.vae, lambda: E.calc_mi(self.vae, self.val_batches), self.log)
        self.vae.train()
        self.log("pre mi:%.4f. cur mi:%.4f" % (self.pre_mi, cur_mi))
        self.mi_checks.append((self.pre_mi, cur_mi))
        if cur_mi - self.pre_mi < 0:
            self.aggressive = False
            self.log("STOP BURNING")
        self.pre_mi = cur_mi

    def end_of_epoch(self, epoch, loss, nll, kl, ppl):
        """Best-checkpoint and learning-rate policy (text.py:463-489).  Returns True when training should stop."""
        if loss < self.best["loss"]:
            self.log("update best loss")
            self.best.update(loss=loss, nll=nll, kl=kl, ppl=ppl, state=copy.deepcopy(self.vae.state_dict()))
        if loss > self.opt["best_loss"]:
            self.opt["not_improved"] += 1
            if self.opt["not_improved"] >= DECAY_EPOCH and epoch >= 15:
                self.opt["best_loss"] = loss
                self.opt["not_improved"] = 0
                self.opt["lr"] *= LR_DECAY
                if self.best["state"] is not None:
                    self.vae.load_state_dict(self.best["state"])
                self.log("new lr: %f" % self.opt["lr"])
                self.decay_cnt += 1
                self.trainer.reset_optimizer(self.opt["lr"])          # text.py:492-493: new optimizers (momentum: zero velocities)
        else:
            self.opt["not_improved"] = 0
            self.opt["best_loss"] = loss
        return self.decay_cnt == MAX_DECAY

    # -- the loop ---------------------------------------------------------------------------------------------------------------
    def run(self):
        args, tr = self.args, self.trainer
        log_niter = max(1, (self.n_train // args.batch_size) // 10)                               # text.py:263
        start = time.time()
        self.vae.train()
        for epoch in range(args.epochs):
            if self.epoch_hook is not None:
                self.epoch_hook(self, epoch)
            rep_rec = rep_kl = 0.0
            rep_sents = 0
            for i in self.rng.permutation(len(self.train_batches)):
                batch = self.train_batches[i]
                bsz, slen = batch.shape
                rep_sents += bsz
                self.kl_weight = min(1.0, self.kl_weight + self.anneal_rate)
                inner = 0
                if self.aggressive:
                    inner = tr.inner_loop(self.train_batches, batch, self.kl_weight, np_rng=self.rng, noise_fn=self.noise_fn)
                tr.reset_stats()
                tr.step(batch, self.kl_weight, noise=None if self.noise_fn is None else self.noise_fn(batch),
                        update="decoder" if self.aggressive else "both")
                st = tr.read_stats()
                rep_rec += st["rec_sum"]
                rep_kl += st["kl_sum"]
                self.iterations.append(dict(epoch=epoch, iter=self.iter_, batch=int(i), kl_weight=self.kl_weight,
                                            aggressive=self.aggressive, inner_steps=inner, rec_sum=st["rec_sum"], kl_sum=st["kl_sum"]))
                if self.iter_ % log_niter == 0:
                    train_loss = (rep_rec + rep_kl) / rep_sents
                    if self.aggressive or epoch == 0:
                        mi, au = self._eval_mi_au()
                        self.log("epoch: %d, iter: %d, avg_loss: %.4f, kl: %.4f, mi: %.4f, recon: %.4f,au %d, time elapsed %.2fs" % (
                            epoch, self.iter_, train_loss, rep_kl / rep_sents, mi, rep_rec / rep_sents, au, time.time() - start))
                    else:
                        self.log("epoch: %d, iter: %d, avg_loss: %.4f, kl: %.4f, recon: %.4f,time elapsed %.2fs" % (
                            epoch, self.iter_, train_loss, rep_kl / rep_sents, rep_rec / rep_sents, time.time() - start))
                    rep_rec = rep_kl = 0.0
                    rep_sents = 0
                self.iter_ += 1
                if self.aggressive and self.iter_ % len(self.train_batches) == 0:
                    self.check_aggressive()
            self.log("kl weight %.4f" % self.kl_weight)
            self.vae.eval()
            with torch.no_grad():
                # (np_rng: E.test draws from it; a repeated pass after a timeout draws again -- the recorded replays never time out)
                loss, nll, kl, ppl, mi = guarded_eval(
                    self.vae, lambda: E.test(self.vae, self.val_batches, "VAL", args, verbose=False, np_rng=self.rng), self.log)
                au = guarded_eval(self.vae, lambda: E.calc_au(self.vae, self.val_batches)[0], self.log)
            self.log("VAL --- avg_loss: %.4f, kl: %.4f, mi: %.4f, nll: %.4f, ppl: %.4f, %d active units" % (loss, kl, mi, nll, ppl, au))
            self.history.append(dict(epoch=epoch, loss=loss, nll=nll, kl=kl, ppl=ppl, mi=mi, au=au, aggressive=self.aggressive,
                                     kl_weight=self.kl_weight, lr=self.opt["lr"]))
            improved = loss < self.best["loss"]
            stop = self.end_of_epoch(epoch, loss, nll, kl, ppl)
            self.history[-1].update(best_updated=improved, lr_after=self.opt["lr"], decay_cnt=self.decay_cnt)
            if stop:
                break
            if epoch % getattr(args, "test_nepoch", 5) == 0 and self.test_batches:
                with torch.no_grad():
                    guarded_eval(self.vae, lambda: E.test(self.vae, self.test_batches, "TEST", args, verbose=False, np_rng=self.rng), self.log)
            self.vae.train()
        if self.best["state"] is not None:
            self.vae.load_state_dict(self.best["state"])
        return dict(best_loss=self.best["loss"], best_nll=self.best["nll"], best_kl=self.best["kl"], best_ppl=self.best["ppl"],
                    epochs=len(self.history), history=self.history)


class ImageTrainingLoop(object):
    """Outer training loop of the reference's image.py (image.py:267-428) around AggressiveImageTrainer.

    Same skeleton as the text loop, different policy constants and three differences that matter (all reproduced):
      * aggressive training ends after FIVE end-of-epoch checks in which the validation MI is below the best MI seen so far
        (`mi_not_improved == 5`, image.py:386-393) -- not at the first drop;
      * the learning rate decays (x0.5) after `decay_epoch` = 20 epochs in which the validation loss did not reach a new best
        (the comparison is against the running best loss, image.py:411, and there is no `epoch >= 15` gate), the best
        weights are reloaded and BOTH Adam optimizers are re-created (moments and step counts reset, image.py:419-420);
      * the data come from shuffled DataLoaders (a fresh order for every pass, evaluation passes included), training batches
        are dynamically binarised (torch.bernoulli, image.py:287), validation / test batches are not.
    args fields read (image.py's argparse names): kl_start, warm_up, batch_size, epochs, aggressive, nsamples (image.py --nsamples:
    the trainer is built with it, AggressiveImageTrainer(nsamples=...), and the evaluation passes hand it to VAE.loss), test_nepoch, objective ("elbo" when missing, or "iw":
    AggressiveImageTrainer(objective=...)) and iw_estimator ("iwae" when missing, or "dreg") -- both concern the
    training steps only: the evaluation passes are untouched.

    order_fn / binarize_fn / eps_fn inject the data order, the binarisation draw and the reparameterisation noise (parity replays
    of a recorded reference run); the defaults draw them as the reference's CPU path does / on the device.  eps_fn(x) returns
    eps [B][nsamples][nz].  A `trainer` that is handed in must have been built with the same nsamples as args'."""

    CLIP_GRAD, DECAY_EPOCH, LR_DECAY, MAX_DECAY, LR0 = 5.0, 20, 0.5, 5, 0.001          # image.py:18-21, 267-269

    def __init__(self, vae, x_train, x_val, x_test, args, trainer=None, log=print, np_rng=None, seed=783435, order_fn=None,
                 binarize_fn=None, eps_fn=None, epoch_hook=None, decay_epoch=None):
        from .data import ShuffledLoader
        self.vae, self.args, self.log = vae, args, log
        self.x_train = x_train
        self.train_loader = ShuffledLoader(x_train, args.batch_size, order_fn)
        self.val_loader = ShuffledLoader(x_val, args.batch_size, order_fn)
        self.test_loader = ShuffledLoader(x_test, args.batch_size, order_fn) if x_test is not None else None
        self.nsamples = int(getattr(args, "nsamples", 1))
        if trainer is not None and getattr(trainer, "nsamples", 1) != self.nsamples:
            raise ValueError("args.nsamples = %d, but the trainer was built with nsamples = %d" % (self.nsamples, getattr(trainer, "nsamples", 1)))
        self.free_bits, self.free_bits_mode = _free_bits(args, trainer)
        # args.objective / args.iw_estimator ("elbo" / "iwae" when missing): the objective of the TRAINING steps; the evaluation passes
        # are the same for all of them
        self.objective = _objective(args, trainer)
        self.iw_estimator = _iw_estimator(args, trainer, self.objective)
        self.trainer = trainer if trainer is not None else AggressiveImageTrainer(vae, lr=self.LR0, clip=self.CLIP_GRAD, seed=seed,
                                                                                  nsamples=self.nsamples, free_bits=self.free_bits,
                                                                                  free_bits_mode=self.free_bits_mode,
                                                                                  objective=self.objective,
                                                                                  iw_estimator=self.iw_estimator)
        self.rng = np_rng if np_rng is not None else np.random
        self.binarize_fn, self.eps_fn, self.epoch_hook = binarize_fn, eps_fn, epoch_hook
        self.decay_epoch = self.DECAY_EPOCH if decay_epoch is None else decay_epoch
        self.kl_weight = float(args.kl_start)
        self.anneal_rate = (1.0 - args.kl_start) / (args.warm_up * len(self.train_loader))          # image.py:281
        self.opt = {"not_improved": 0, "lr": self.LR0, "best_loss": 1e4}
        self.aggressive = bool(args.aggressive)
        self.iter_ = self.decay_cnt = self.mi_not_improved = 0
        self.pre_mi = self.best_mi = 0.0
        self.best = {"loss": 1e4, "nll": 0.0, "kl": 0.0, "state": None}
        self.history, self.iterations, self.mi_checks = [], [], []

    def _binarize(self, probs):
        return self.binarize_fn(probs) if self.binarize_fn is not None else self.trainer.binarize(probs)

    def check_aggressive(self):
        """image.py:381-395, called when a full epoch worth of iterations has passed while aggressive."""
        self.vae.eval()
        with torch.no_grad():
            cur_mi = E.image_calc_mi(self.vae, self.val_loader)
        self.vae.train()
        self.mi_checks.append((self.best_mi, cur_mi))
        if cur_mi - self.best_mi < 0:
            self.mi_not_improved += 1
            if self.mi_not_improved == 5:
                self.aggressive = False
                self.log("STOP BURNING")
        else:
            self.best_mi = cur_mi
        self.pre_mi = cur_mi

    def end_of_epoch(self, epoch, loss, nll, kl):
        """Best-checkpoint and learning-rate policy (image.py:404-425).  Returns True when training should stop."""
        if loss < self.best["loss"]:
            self.log("update best loss")
            self.best.update(loss=loss, nll=nll, kl=kl, state=copy.deepcopy(self.vae.state_dict()))
        if loss > self.best["loss"]:
            self.opt["not_improved"] += 1
            if self.opt["not_improved"] >= self.decay_epoch:
                self.opt["best_loss"] = loss
                self.opt["not_improved"] = 0
                self.opt["lr"] *= self.LR_DECAY
                if self.best["state"] is not None:
                    self.vae.load_state_dict(self.best["state"])
                    self.trainer.dec.wgen += 1          # packed convolution weights are cached per weight version
                self.decay_cnt += 1
                self.log("new lr: %f" % self.opt["lr"])
                self.trainer.reset_optimizer(self.opt["lr"])
        else:
            self.opt["not_improved"] = 0
            self.opt["best_loss"] = loss
        return self.decay_cnt == self.MAX_DECAY

    def run(self):
        args, tr = self.args, self.trainer
        n_iter = len(self.train_loader)
        log_niter = max(1, n_iter // 5)                                                         # image.py:249
        start = time.time()
        self.vae.train()
        for epoch in range(args.epochs):
            if self.epoch_hook is not None:
                self.epoch_hook(self, epoch)
            rep_rec = rep_kl = 0.0
            rep_n = 0
            for probs, _ in self.train_loader:
                batch = self._binarize(probs)
                rep_n += int(batch.shape[0])
                self.kl_weight = min(1.0, self.kl_weight + self.anneal_rate)
                inner = 0
                if self.aggressive:
                    inner = tr.inner_loop(self.x_train, batch, self.kl_weight, batch_size=args.batch_size, np_rng=self.rng,
                                          eps_fn=self.eps_fn, binarize_fn=self.binarize_fn)
                tr.reset_stats()
                tr.step(batch, self.kl_weight, eps=None if self.eps_fn is None else self.eps_fn(batch),
                        update="decoder" if self.aggressive else "both")
                st = tr.read_stats()
                rep_rec += st["rec_sum"]
                rep_kl += st["kl_sum"]
                self.iterations.append(dict(epoch=epoch, iter=self.iter_, kl_weight=self.kl_weight, aggressive=self.aggressive,
                                            inner_steps=inner, rec_sum=st["rec_sum"], kl_sum=st["kl_sum"], n=int(batch.shape[0])))
                if self.iter_ % log_niter == 0:
                    train_loss = (rep_rec + rep_kl) / rep_n
                    if self.aggressive or epoch == 0:
                        self.vae.eval()
                        with torch.no_grad():
                            mi = E.image_calc_mi(self.vae, self.val_loader)
                            au, _ = E.image_calc_au(self.vae, self.val_loader)
                        self.vae.train()
                        self.log("epoch: %d, iter: %d, avg_loss: %.4f, kl: %.4f, mi: %.4f, recon: %.4f,au %d, time elapsed %.2fs" % (
                            epoch, self.iter_, train_loss, rep_kl / rep_n, mi, rep_rec / rep_n, au, time.time() - start))
                    else:
                        self.log("epoch: %d, iter: %d, avg_loss: %.4f, kl: %.4f, recon: %.4f,time elapsed %.2fs" % (
                            epoch, self.iter_, train_loss, rep_kl / rep_n, rep_rec / rep_n, time.time() - start))
                    rep_rec = rep_kl = 0.0
                    rep_n = 0
                self.iter_ += 1
                if self.aggressive and self.iter_ % n_iter == 0:
                    self.check_aggressive()
            self.log("kl weight %.4f" % self.kl_weight)
            self.vae.eval()
            with torch.no_grad():
                loss, nll, kl = E.image_test(self.vae, self.val_loader, "VAL", args, verbose=False)
                au, _ = E.image_calc_au(self.vae, self.val_loader)
            self.log("VAL --- avg_loss: %.4f, kl: %.4f, nll: %.4f, %d active units" % (loss, kl, nll, au))
            improved = loss < self.best["loss"]
            self.history.append(dict(epoch=epoch, loss=loss, nll=nll, kl=kl, au=au, aggressive=self.aggressive,
                                     kl_weight=self.kl_weight, lr=self.opt["lr"], best_updated=improved))
            stop = self.end_of_epoch(epoch, loss, nll, kl)
            self.history[-1].update(lr_after=self.opt["lr"], decay_cnt=self.decay_cnt)
            if stop:
                break
            if epoch % getattr(args, "test_nepoch", 5) == 0 and self.test_loader is not None:
                with torch.no_grad():
                    E.image_test(self.vae, self.test_loader, "TEST", args, verbose=False)
            self.vae.train()
        if self.best["state"] is not None:
            self.vae.load_state_dict(self.best["state"])
            self.trainer.dec.wgen += 1
        return dict(best_loss=self.best["loss"], best_nll=self.best["nll"], best_kl=self.best["kl"], epochs=len(self.history),
                    history=self.history)


class ToyTrainingLoop(object):
    """Outer training loop of the reference's toy.py (toy.py:235-539), the synthetic experiment behind the posterior-mean plots,
    around AggressiveTextTrainer.

    The skeleton is text.py's (TextTrainingLoop); what toy.py does differently is reproduced as it is:
      * `--optim adam`: both halves on torch.optim.Adam(lr=0.001) (the trainer's optimizer="adam"); a learning-rate decay
        re-creates the optimizers -- with betas (0.5, 0.999) for Adam (toy.py:506-511: trainer.reset_optimizer);
      * the MI stop check starts from pre_mi = -1, the log line has MI but no active units, there is no `epoch >= 15` gate on the
        decay, and the per-epoch VAL / TEST lines are toy.test's (four numbers);
      * plots: `plot_mode` "multiple" records the model posterior mean E[z|x] on the grid (VAE.calc_model_posterior_mean), the
        inference mean, KL and MI of `plot_data` every `plot_niter` iterations of epoch 0 (eval mode) and at every epoch end (in
        TRAIN mode under no_grad, before vae.eval(): toy.py:482-483); "single" trains on `plot_data` for every inner and joint
        step (no host draw picks a batch), follows both means after every step of epoch 0 and returns at the first plot after
        iteration 0, with no VAL / TEST / IW-NLL;
      * at the end the best checkpoint is reloaded and the importance-weighted NLL is computed on `iw_batches` (toy.py uses the
        test set in batches of one sentence).
    args fields read (toy.py's argparse names): kl_start, warm_up, batch_size, epochs, aggressive, nsamples, test_nepoch,
    iw_nsamples, optim, plot_mode, num_plot, plot_niter, zmin, zmax, dz, objective ("elbo" when missing, or "iw": the
    single-sample importance-weighted step, AggressiveTextTrainer(objective="iw")), iw_estimator ("iwae" when missing, or "dreg").

    plot_data: the (batch, lengths) pair MonoTextData.data_sample returns (toy.py:304), or the batch tensor alone.
    noise_fn / epoch_hook / np_rng: as TextTrainingLoop's.  plot_dir: when given, every plot is also written as toy.py writes it
    (`aggr%d_iter%d_multiple.pickle` / `aggr%d_single.pickle`, the keys the reference's plot_scripts read)."""

    LR0 = {"sgd": 1.0, "adam": 0.001}                       # toy.py:284-291
    DECAY_BETAS = (0.5, 0.999)                              # toy.py:510-511

    def __init__(self, vae, train_batches, val_batches, test_batches, plot_data, args, iw_batches=None, trainer=None, log=print,
                 np_rng=None, seed=783435, noise_fn=None, epoch_hook=None, plot_dir=None):
        if getattr(args, "nsamples", 1) != 1:
            raise ValueError("the fused training step draws one sample per sentence (nsamples = 1, toy.py's default)")
        self.optim = getattr(args, "optim", "sgd")
        if self.optim not in self.LR0:
            raise ValueError("optim: 'sgd' or 'adam' (toy.py:284-291), not %r" % (self.optim,))
        if args.plot_mode not in ("multiple", "single"):
            raise ValueError("plot_mode: 'multiple' or 'single'")
        if args.plot_mode == "single" and not (0 < args.plot_niter < len(train_batches)):
            # toy.py returns at the first plot after iteration 0; without one in epoch 0 its epoch-end plot call fails
            raise ValueError("plot_mode 'single' ends at the first plot after iteration 0: plot_niter must be in [1, %d)" % len(train_batches))
        self.vae, self.args, self.log = vae, args, log
        self.noise_fn, self.epoch_hook, self.plot_dir = noise_fn, epoch_hook, plot_dir
        self.train_batches, self.val_batches, self.test_batches = train_batches, val_batches, test_batches
        self.iw_batches = iw_batches
        self.plot_x = plot_data[0] if isinstance(plot_data, (tuple, list)) else plot_data
        self.single = args.plot_mode == "single"
        self.opt = {"not_improved": 0, "lr": self.LR0[self.optim], "best_loss": 1e4}
        self.objective = _objective(args, trainer)
        self.iw_estimator = _iw_estimator(args, trainer, self.objective)
        self.free_bits, self.free_bits_mode = _free_bits(args, trainer)
        if trainer is None:
            trainer = AggressiveTextTrainer(vae, lr=self.opt["lr"], clip=CLIP_GRAD, seed=seed, optimizer=self.optim, objective=self.objective,
                                            free_bits=self.free_bits, free_bits_mode=self.free_bits_mode, iw_estimator=self.iw_estimator)
        elif getattr(trainer, "optimizer", "sgd") != self.optim:
            raise ValueError("args.optim is %r but the trainer steps with %r" % (self.optim, getattr(trainer, "optimizer", "sgd")))
        self.trainer = trainer
        if hasattr(trainer, "prepare_batches"):
            trainer.prepare_batches(list(train_batches) + ([self.plot_x] if self.single else []))
        self.rng = np_rng if np_rng is not None else np.random
        self.n_train = sum(int(b.shape[0]) for b in train_batches)
        self.kl_weight = float(args.kl_start)
        self.anneal_rate = (1.0 - args.kl_start) / (args.warm_up * (self.n_train / args.batch_size))      # toy.py:302
        from .modules.utils import generate_grid
        self.grid_z = generate_grid(args.zmin, args.zmax, args.dz, self.plot_x.device, ndim=1)          # toy.py:307,311
        self.aggressive = bool(args.aggressive)
        self.iter_ = self.decay_cnt = 0
        self.pre_mi = -1.0                                                                               # toy.py:296
        self.best = {"loss": 1e4, "nll": 0.0, "kl": 0.0, "ppl": 0.0, "state": None}
        self.history, self.iterations, self.mi_checks, self.plots, self.optimizer_resets = [], [], [], [], []
        self.iw = None
        self._post, self._infer = [], []          # single mode: the two means after every step of epoch 0

    # -- plots (toy.py:188-231) ---------------------------------------------------------------------------------------------------
    def _save(self, name, data):
        if self.plot_dir is None:
            return
        import os
        import pickle
        os.makedirs(self.plot_dir, exist_ok=True)
        with open(os.path.join(self.plot_dir, name), "wb") as fh:
            pickle.dump(data, fh)

    def plot_multiple(self, iter_, where):
        """toy.py:188-218 (no_grad and the train / eval mode are the caller's, as in toy.py)."""
        vae, args = self.vae, self.args
        parts = []
        kl_sum = mi_sum = 0.0
        n = 0
        for data in torch.chunk(self.plot_x, round(args.num_plot / args.batch_size)):
            kl_sum += vae.KL(data).sum().item()
            n += data.size(0)
            mi_sum += vae.calc_mi_q(data) * data.size(0)
            post = vae.calc_model_posterior_mean(data, self.grid_z)
            parts.append(torch.cat([post, vae.calc_infer_mean(data)], 1))
        both = torch.cat(parts, 0)
        data = {"posterior": both[:, 0].cpu().numpy(), "inference": both[:, 1].cpu().numpy(), "kl": kl_sum / n, "mi": mi_sum / n}
        self.plots.append(dict(data, iter=iter_, where=where, train_mode=vae.training))
        self._save("aggr%d_iter%d_multiple.pickle" % (args.aggressive, iter_), data)

    def plot_single(self):
        """toy.py:220-231: the two means of plot_data after every step of epoch 0, one column per step."""
        data = {"posterior": torch.cat(self._post, 1).cpu().numpy(), "inference": torch.cat(self._infer, 1).cpu().numpy()}
        self.plots.append(dict(data, iter=self.iter_, where="single", train_mode=self.vae.training))
        self._save("aggr%d_single.pickle" % self.args.aggressive, data)

    # -- policy pieces ------------------------------------------------------------------------------------------------------------
    def _eval_mi(self, batches):
        self.vae.eval()
        with torch.no_grad():
            mi = guarded_eval(self.vae, lambda: E.calc_mi(self.vae, batches), self.log)
        self.vae.train()
        return mi

    def check_aggressive(self):
        """toy.py:466-474: called when a full epoch worth of iterations has passed while aggressive."""
        cur_mi = self._eval_mi(self.val_batches)
        self.mi_checks.append((self.pre_mi, cur_mi))
        if cur_mi - self.pre_mi < 0:
            self.aggressive = False
            self.log("STOP BURNING")
        self.pre_mi = cur_mi

    def end_of_epoch(self, epoch, loss, nll, kl, ppl):
        """toy.py:489-517 (no `epoch >= 15` gate; a decay re-creates the optimizers).  Returns True when training should stop."""
        if loss < self.best["loss"]:
            self.log("update best loss")
            self.best.update(loss=loss, nll=nll, kl=kl, ppl=ppl, state=copy.deepcopy(self.vae.state_dict()))
        if loss > self.opt["best_loss"]:
            self.opt["not_improved"] += 1
            if self.opt["not_improved"] >= DECAY_EPOCH:
                self.opt["best_loss"] = loss
                self.opt["not_improved"] = 0
                self.opt["lr"] *= LR_DECAY
                self.vae.load_state_dict(self.best["state"])
                self.log("new lr: %f" % self.opt["lr"])
                self.decay_cnt += 1
                betas = self.DECAY_BETAS if self.optim == "adam" else None
                self.trainer.reset_optimizer(self.opt["lr"], betas=betas)
                self.optimizer_resets.append(dict(epoch=epoch, lr=self.opt["lr"], betas=betas))
        else:
            self.opt["not_improved"] = 0
            self.opt["best_loss"] = loss
        return self.decay_cnt == MAX_DECAY

    def _test(self, batches, mode):
        """toy.test (toy.py:111-149): eval mode and no_grad are the caller's.  Returns (loss, nll, kl, ppl, mi)."""
        loss, nll, kl, ppl, mi = guarded_eval(
            self.vae, lambda: E.test(self.vae, batches, mode, self.args, verbose=False, np_rng=self.rng), self.log)
        self.log("%s --- avg_loss: %.4f, kl: %.4f, mi: %.4f, recon: %.4f, nll: %.4f, ppl: %.4f" % (mode, loss, kl, mi, nll - kl, nll, ppl))
        return loss, nll, kl, ppl, mi

    def _result(self, early):
        return dict(best_loss=self.best["loss"], best_nll=self.best["nll"], best_kl=self.best["kl"], best_ppl=self.best["ppl"],
                    epochs=len(self.history), history=self.history, iterations=self.iterations, plots=self.plots,
                    iw_nll=None if self.iw is None else self.iw[0], iw_ppl=None if self.iw is None else self.iw[1],
                    early_return=early, optimizer_resets=self.optimizer_resets)

    # -- the loop -----------------------------------------------------------------------------------------------------------------
    def run(self):
        args, tr, vae = self.args, self.trainer, self.vae
        log_niter = max(1, (self.n_train // args.batch_size) // 10)                                   # toy.py:268
        x_plot = self.plot_x
        start = time.time()
        vae.train()
        if self.single:
            # toy.py:316-317: before the loop, in train mode with autograd on (the generic grid route)
            self._post.append(vae.calc_model_posterior_mean(x_plot, self.grid_z).detach())
            self._infer.append(vae.calc_infer_mean(x_plot).detach())
        next_batch = (lambda: x_plot) if self.single else None
        for epoch in range(args.epochs):
            if self.epoch_hook is not None:
                self.epoch_hook(self, epoch)
            rep_rec = rep_kl = 0.0
            rep_sents = 0
            for i in self.rng.permutation(len(self.train_batches)):
                batch = x_plot if self.single else self.train_batches[i]
                rep_sents += int(batch.shape[0])
                self.kl_weight = min(1.0, self.kl_weight + self.anneal_rate)
                inner = 0
                if self.aggressive:
                    inner = tr.inner_loop(self.train_batches, batch, self.kl_weight, np_rng=self.rng, noise_fn=self.noise_fn,
                                          next_batch=next_batch)
                if self.single and epoch == 0 and self.aggressive:                                  # toy.py:391-396
                    vae.eval()
                    with torch.no_grad():
                        self._post.append(self._post[-1])
                        self._infer.append(vae.calc_infer_mean(x_plot))
                    vae.train()
                tr.reset_stats()
                tr.step(batch, self.kl_weight, noise=None if self.noise_fn is None else self.noise_fn(batch),
                        update="decoder" if self.aggressive else "both")
                if self.single and epoch == 0:                                                       # toy.py:417-426
                    vae.eval()
                    with torch.no_grad():
                        self._post.append(vae.calc_model_posterior_mean(x_plot, self.grid_z))
                        self._infer.append(self._infer[-1] if self.aggressive else vae.calc_infer_mean(x_plot))
                    vae.train()
                st = tr.read_stats()
                rep_rec += st["rec_sum"]
                rep_kl += st["kl_sum"]
                self.iterations.append(dict(epoch=epoch, iter=self.iter_, batch=int(i), kl_weight=self.kl_weight,
                                            aggressive=self.aggressive, inner_steps=inner, rec_sum=st["rec_sum"], kl_sum=st["kl_sum"]))
                if self.iter_ % log_niter == 0:
                    train_loss = (rep_rec + rep_kl) / rep_sents
                    if self.aggressive or epoch == 0:
                        mi = self._eval_mi(self.val_batches)
                        self.log("epoch: %d, iter: %d, avg_loss: %.4f, kl: %.4f, mi: %.4f, recon: %.4f,time elapsed %.2fs" % (
                            epoch, self.iter_, train_loss, rep_kl / rep_sents, mi, rep_rec / rep_sents, time.time() - start))
                    else:
                        self.log("epoch: %d, iter: %d, avg_loss: %.4f, kl: %.4f, recon: %.4f,time elapsed %.2fs" % (
                            epoch, self.iter_, train_loss, rep_kl / rep_sents, rep_rec / rep_sents, time.time() - start))
                    rep_rec = rep_kl = 0.0
                    rep_sents = 0
                if self.iter_ % args.plot_niter == 0 and epoch == 0:                                 # toy.py:453-462
                    vae.eval()
                    with torch.no_grad():
                        if self.single and self.iter_ != 0:
                            self.plot_single()
                            return self._result(early=True)          # toy.py:458: no VAL / TEST / IW-NLL
                        elif not self.single:
                            self.plot_multiple(self.iter_, "iter")
                    vae.train()
                self.iter_ += 1
                if self.aggressive and self.iter_ % len(self.train_batches) == 0:
                    self.check_aggressive()
            self.log("kl weight %.4f" % self.kl_weight)
            self.log("epoch: %d, VAL" % epoch)
            with torch.no_grad():
                self.plot_multiple(self.iter_, "epoch")          # toy.py:482-483: still in train mode
            vae.eval()
            with torch.no_grad():
                loss, nll, kl, ppl, mi = self._test(self.val_batches, "VAL")
            self.history.append(dict(epoch=epoch, loss=loss, nll=nll, kl=kl, ppl=ppl, mi=mi, aggressive=self.aggressive,
                                     kl_weight=self.kl_weight, lr=self.opt["lr"], best_updated=loss < self.best["loss"]))
            stop = self.end_of_epoch(epoch, loss, nll, kl, ppl)
            self.history[-1].update(lr_after=self.opt["lr"], decay_cnt=self.decay_cnt)
            if stop:
                break
            if epoch % args.test_nepoch == 0:
                with torch.no_grad():
                    t = self._test(self.test_batches, "TEST")
                self.history[-1].update(test=t)
            vae.train()
        self.log("best_loss: %.4f, kl: %.4f, nll: %.4f, ppl: %.4f" % (self.best["loss"], self.best["kl"], self.best["nll"], self.best["ppl"]))
        if self.best["state"] is not None:
            vae.load_state_dict(self.best["state"])                                                     # toy.py:532
        vae.eval()
        if self.iw_batches is not None:
            with torch.no_grad():
                self.iw = guarded_eval(vae, lambda: E.calc_iwnll(vae, self.iw_batches, args, np_rng=self.rng), self.log)
            self.log("iw nll: %.4f, iw ppl: %.4f" % self.iw)
        return self._result(early=False)

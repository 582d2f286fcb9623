"""LSTMEncoder -- drop-in for the reference's modules/encoders/enc_lstm.py:11-64 on MI355X.

Same constructor signature, same nn.Module containers in the same construction order (so seeded initialisation
and state_dict keys `embed.weight, lstm.{weight,bias}_{ih,hh}_l0, linear.weight` are interchangeable with the
reference's checkpoints), but `forward` runs the hand-written HIP path (embedding gather -> f32 MFMA input
projection -> per-timestep fused LSTM kernels -> head GEMM) through engine.LSTMEncoderEngine, with a
hand-written backward behind torch.autograd.Function.
"""
import torch
import torch.nn as nn

from ... import engine as _eng
from .encoder import GaussianEncoderBase


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, x, *params):
        mulv = eng.forward(x)
        ctx.eng = eng
        ctx.gen = eng.gen
        return mulv.clone()

    @staticmethod
    def backward(ctx, dmulv):
        eng = ctx.eng
        eng.flat.before_autograd_backward()
        eng.backward(dmulv, ctx.gen)
        return (None, None) + eng.flat.deliver_grads()


class _VarEncoderFn(torch.autograd.Function):
    """_EncoderFn on a padded batch with lengths: the length-aware recurrences (engine.LSTMEncoderEngine.forward(lengths=))."""

    @staticmethod
    def forward(ctx, eng, x, lengths, *params):
        mulv = eng.forward(x, lengths=lengths)
        ctx.eng = eng
        ctx.gen = eng.gen
        return mulv.clone()

    @staticmethod
    def backward(ctx, dmulv):
        eng = ctx.eng
        eng.flat.before_autograd_backward()
        eng.backward(dmulv, ctx.gen)
        return (None, None, None) + eng.flat.deliver_grads()


class _EncoderByLengthFn(torch.autograd.Function):
    """The A/B route (VarLSTMEncoder.masked = False): every group of equal length through the equal-length engine."""

    @staticmethod
    def forward(ctx, eng, x, lengths, *params):
        B = x.shape[0]
        V, ni, H, nz2 = eng.dims()
        out = torch.empty(B, nz2, dtype=torch.float32, device=x.device)
        ctx.groups = _eng.length_groups(lengths)
        ctx.book = _eng.GroupedBackward(eng)
        for n, rows in ctx.groups:
            out[rows] = eng.forward(x[rows, :n].contiguous())
            ctx.book.after_forward(eng._ws(int(rows.numel()), n))
        ctx.eng = eng
        return out

    @staticmethod
    def backward(ctx, dmulv):
        eng = ctx.eng
        eng.flat.before_autograd_backward()
        for i, (n, rows) in enumerate(ctx.groups):
            d = dmulv[rows].contiguous()
            ctx.book.backward(i, lambda: eng._ws(int(rows.numel()), n), lambda gen: eng.backward(d, gen))
        return (None, None, None) + eng.flat.deliver_grads()


class LSTMEncoder(GaussianEncoderBase):
    """Gaussian LSTM encoder with constant-length batching (reference enc_lstm.py:11-64)."""

    def __init__(self, args, vocab_size, model_init, emb_init):
        super(LSTMEncoder, self).__init__()
        self.ni = args.ni
        self.nh = args.enc_nh
        self.nz = args.nz

        self.embed = nn.Embedding(vocab_size, args.ni)
        self.lstm = nn.LSTM(input_size=args.ni, hidden_size=args.enc_nh, num_layers=1, batch_first=True, dropout=0)
        # mean and logvar head
        self.linear = nn.Linear(args.enc_nh, 2 * args.nz, bias=False)

        self.reset_parameters(model_init, emb_init)
        self._hip = _eng.LSTMEncoderEngine(self)

    def reset_parameters(self, model_init, emb_init):
        # every parameter (LSTM biases included), then the embedding again
        for param in self.parameters():
            model_init(param)
        emb_init(self.embed.weight)

    def _params(self):
        return (self.embed.weight, self.lstm.weight_ih_l0, self.lstm.weight_hh_l0, self.lstm.bias_ih_l0,
                self.lstm.bias_hh_l0, self.linear.weight)

    def _forward_mulv(self, input):
        self._hip.ensure(input.device)
        return _EncoderFn.apply(self._hip, input, *self._params())

    def forward(self, input):
        """input (batch, seq_len) int64 -> mean (batch, nz), logvar (batch, nz).
        The whole of `input` is embedded, <s> and </s> included."""
        mulv = self._forward_mulv(input)
        return mulv[:, :self.nz], mulv[:, self.nz:]


class VarLSTMEncoder(LSTMEncoder):
    """Gaussian LSTM encoder with variable-length batching (reference enc_lstm.py:77-126): `input` is a pair (x, sents_len) of a
    padded (batch, seq_len) int64 tensor and the sentence lengths, and mu / logvar come from the LSTM state after each row's own
    last token.  Same constructor, containers and state_dict keys as LSTMEncoder.  `encode`, `sample`, `eval_inference_dist`
    and `calc_mi` are the base class's on top of `forward`.

    Lengths count every token of a row, <s> and </s> included (what data.MonoTextData.data_iter / data_sample yield).  Beyond
    the reference: they need not be sorted, seq_len may exceed the longest sentence, and they may be a list of ints or an
    integer tensor on any device; a wrong count, a length below 2 or above seq_len raises ValueError before any launch.  A plain
    (batch, seq_len) tensor is taken as LSTMEncoder takes it.  Exact-f32 configuration only (engine.LvaeError under "bf16")."""

    # True: one length-aware recurrence over the padded batch (lv_lstm_fwd_len_f32 / lv_lstm_bwd_len_f32); False: every group of
    # equal length through LSTMEncoder's equal-length path, concatenated -- the only route before these kernels (A/B runs, tests)
    masked = True

    def _forward_mulv(self, input):
        if torch.is_tensor(input):
            return super(VarLSTMEncoder, self)._forward_mulv(input)
        x, lengths = _eng.varlen_batch(input)
        _eng._refuse_bf16_lengths(self._hip)
        self._hip.ensure(x.device)
        fn = _VarEncoderFn if self.masked else _EncoderByLengthFn
        return fn.apply(self._hip, x, lengths, *self._params())

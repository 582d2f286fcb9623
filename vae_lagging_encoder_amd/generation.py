"""Text generation to a file: the counterparts of the reference's text.py:107-121 (`--decode_from` with `--decode_input FILE`
or prior samples, `--decoding_strategy greedy | beam | sample`).

The reference reconstructs a corpus with batch_size=1 because its beam search decodes one sentence at a time anyway; here
LSTMDecoder.beam_search_decode decodes a whole batch together (engine.LSTMBeamSearcher), so `reconstruct` takes a batch size.
"""
import torch

from . import engine as _eng


def reconstruct(model, data, strategy, fname, device, batch_size=32, temperature=1.0, top_k=0, top_p=1.0):
    """Encode every sentence of `data` (a data.MonoTextData), draw one z from q(z|x), decode it with `strategy` and write one
    line per sentence to `fname`, in the corpus' order (reference text.py:107-114).

    Iterates data.data_iter(batch_size, device, batch_first=True, shuffle=False); that iterator orders a batch longest
    sentence first and leaves out a trailing partial batch, so the lines are put back into input order and the remaining
    len(data) % batch_size sentences are decoded as one last batch.  batch_size=1 reproduces the reference's call pattern.

    With batch_size > 1 the encoder's Gaussian draw is one [B][nz] draw instead of B draws of [1][nz]: same distribution,
    different stream (as LSTMDecoder.sample_decode documents for its own draw).  Sentences of different length in one batch are
    padded to the longest, and the encoder -- like the reference's -- reads the padding as input: a shorter sentence's posterior
    is then not the one batch_size=1 gives it.  A corpus of equal-length sentences, or batch_size=1, has no padding.

    temperature / top_k / top_p are LSTMDecoder.sample_decode's (strategy "sample" only: ValueError otherwise, before anything
    is encoded or written)."""
    if not _eng.sampling_filter(temperature, top_k, top_p)[3] and strategy != "sample":
        raise ValueError("temperature / top_k / top_p apply to the decoding strategy \"sample\" only")
    n = len(data)
    lines = [None] * n

    def decode(batch, index):
        with torch.no_grad():
            sents = model.reconstruct(batch, strategy, temperature=temperature, top_k=top_k, top_p=top_p)
        for j, sent in zip(index, sents):
            lines[j] = " ".join(sent)

    def longest_first(lo, hi):                  # data_iter's order inside a batch (a stable sort)
        return sorted(range(lo, hi), key=lambda j: -len(data.data[j]))

    lo = 0
    for batch, _ in data.data_iter(batch_size=batch_size, device=device, batch_first=True, shuffle=False):
        decode(batch, longest_first(lo, lo + batch.size(0)))
        lo += batch.size(0)
    if lo < n:
        index = longest_first(lo, n)
        batch, _ = data._frame([data.data[j] for j in index], True, device)
        decode(batch, index)
    with open(fname, "w") as fout:
        for line in lines:
            fout.write(line + "\n")


def sample_from_prior(model, z, strategy, fname, temperature=1.0, top_k=0, top_p=1.0):
    """Decode the latent codes z [n][nz] with `strategy` and write one line per code to `fname` (reference text.py:116-121).
    temperature / top_k / top_p are LSTMDecoder.sample_decode's (strategy "sample" only: ValueError otherwise)."""
    with torch.no_grad():
        decoded = model.decode(z, strategy, temperature=temperature, top_k=top_k, top_p=top_p)
    with open(fname, "w") as fout:
        for sent in decoded:
            fout.write(" ".join(sent) + "\n")

"""Golden record of the reference's `text.main(args)` with `--momentum 0.5` (text.py:30: both optimizers are
`optim.SGD(..., lr, momentum=args.momentum)`, text.py:325-326, and are built again after every learning-rate decay, text.py:492-493).

    python tests/golden/make_golden_policy_momentum.py      # writes tests/golden/policy_text_momentum.npz and .log

Everything is make_golden_policy.py's: the same tiny corpus, recorder, event stream and derived tables.  That module's main() is run
-- run_reference_text(seed=783435, epochs=19, corpus_seed=5, dropout=0.0) and derive_tables exactly as there -- with three of ITS
module attributes replaced for the duration: `text_args` (momentum = 0.5), `Recorder` (velocity snapshots, below) and `HERE` (a
temporary directory: main() writes policy_text.npz / .log there, and this script writes the fixture under its own name from them).
Nothing outside that module is patched except torch.optim.SGD.__init__, which registers the optimizers.  Two keys are added:
  * `momentum`;
  * `epoch_start_buf/<enc|dec>/<parameter name>` [epochs, *shape]: the momentum buffers of both optimizers at every epoch start
    (where the recorder snapshots the weights: the permutation that opens an epoch), zeros where an optimizer has not stepped yet
    or has just been re-created.  The optimizers are found through a wrapped torch.optim.SGD.__init__ (main() creates them in
    the order encoder, decoder, every time).
The replay (tests/test_sgd_momentum.py) re-synchronises weights AND velocities there and checks every epoch on its own.

corpus_seed: 5, the first choice.  The recorded run (19 epochs, 247 outer iterations, 600 inner steps, one "STOP BURNING", one
decay to lr 0.5) was replayed on the CPU emulator before any GPU run and every exit decision was reproduced, so there was no reason
to move on to corpus seeds 6 or 7.
"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden_policy as G  # noqa: E402

MOMENTUM = 0.5
NAME = "policy_text_momentum"


def main():
    out_dir = G.HERE
    opts = []                       # every optim.SGD main() created, in order: enc, dec, enc, dec, ...
    bufs = []                       # per epoch start: {"enc/<name>": array, "dec/<name>": array}

    def text_args(*a, **k):
        args = orig["text_args"](*a, **k)
        args.momentum = MOMENTUM
        return args

    def snapshot(vae):
        out = {}
        for tag, mod, opt in (("enc", vae.encoder, opts[-2]), ("dec", vae.decoder, opts[-1])):
            for name, p in mod.named_parameters():
                b = opt.state.get(p, {}).get("momentum_buffer")
                out["%s/%s" % (tag, name)] = (torch.zeros_like(p) if b is None else b).detach().numpy().copy()
        return out

    base = G.Recorder

    class Recorder(base):
        """The recorder snapshots the weights by appending to epoch_states (at the permutation that opens an epoch): the velocities
        are snapshotted at the same moment."""

        class _States(list):
            def __init__(self, rec):
                list.__init__(self)
                self.rec = rec

            def append(self, st):
                list.append(self, st)
                bufs.append(snapshot(self.rec.vae))

        def __init__(self):
            base.__init__(self)
            self.epoch_states = Recorder._States(self)

    sgd_init = torch.optim.SGD.__init__

    def init(self, *a, **k):
        sgd_init(self, *a, **k)
        opts.append(self)

    orig = {k: getattr(G, k) for k in ("text_args", "Recorder", "HERE")}
    tmp = tempfile.mkdtemp(prefix="policy_momentum_")
    G.text_args, G.Recorder, G.HERE = text_args, Recorder, tmp
    torch.optim.SGD.__init__ = init
    try:
        G.main(free=False)
    finally:
        for k, v in orig.items():
            setattr(G, k, v)
        torch.optim.SGD.__init__ = sgd_init
    assert len(opts) >= 2 and all(o.defaults["momentum"] == MOMENTUM for o in opts)
    with np.load(os.path.join(tmp, "policy_text.npz")) as fx:
        out = {k: fx[k] for k in fx.files}
    assert len(bufs) == int(out["n_epochs_run"]), (len(bufs), out["n_epochs_run"])
    out["momentum"] = MOMENTUM
    for k in bufs[0]:
        out["epoch_start_buf/" + k] = np.stack([b[k] for b in bufs])
    np.savez_compressed(os.path.join(out_dir, NAME + ".npz"), **out)
    shutil.copyfile(os.path.join(tmp, "policy_text.log"), os.path.join(out_dir, NAME + ".log"))
    shutil.rmtree(tmp)
    print("optimizers created: %d; velocity snapshots: %d; wrote %s.npz (%d bytes) and %s.log" % (
        len(opts), len(bufs), NAME, os.path.getsize(os.path.join(out_dir, NAME + ".npz")), NAME))


if __name__ == "__main__":
    main()

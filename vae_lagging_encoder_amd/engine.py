"""Host-side sequencing of the gfx950 kernels for the LSTM-VAE hot path.

This is the layer between the reference's Python class surface (modules/*.py mirrors) and the C ABI in
include/lvae.h.  PyTorch is used only for device memory (torch.empty), the current HIP stream and autograd
plumbing; every arithmetic op on the hot path is a call into liblvae_hip.so.

Layout contract: token ids stay batch-first int64 [B][T] exactly as the reference's
create_data_batch hands them over (data/text_data.py:219-255); every activation is time-major ([T][B][*]) so one
LSTM timestep is a contiguous slab; parameters of one module live in one flat fp32 buffer (FlatBuffer) whose
segments back the module's nn.Parameters, gradients in a parallel flat buffer.
"""
import ctypes
import math
import numbers
import os

import numpy as np
import torch

from . import _lib

# ---- backend selection -------------------------------------------------------------------------------
def backend_for(device):
    """The C-ABI library for tensors on `device`: the gfx950 build for ROCm 'cuda' devices, nothing else.  (The GPU-less CI
    substitutes this function from outside the package -- tests/emu/install.py -- to drive the same host code against an
    emulator build of the kernel sources; the package itself has no such path.)"""
    device = torch.device(device)
    if device.type == "cuda":
        return _lib.load()
    raise _lib.LvaeError(
        "vae_lagging_encoder_amd runs on MI355X (ROCm 'cuda' tensors) through its HIP extension; got a %s tensor. "
        "There is no CPU fallback." % device.type)


def stream_ptr(device):
    device = torch.device(device)
    if device.type == "cuda":
        return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    return None


def P(t, offset_elems=0):
    """Raw device pointer of tensor t (+ element offset); None -> NULL."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr() + offset_elems * t.element_size())


def _round_up(x, m):
    return (x + m - 1) // m * m


class FlatBuffer(object):
    """One flat fp32 buffer for a module's parameters and one for its gradients; each nn.Parameter's .data is
    re-pointed to a 16-byte-aligned segment so the global grad-norm / clip+SGD are single streaming passes."""

    def __init__(self, named_params, device):
        self.names = [n for n, _ in named_params]
        self.params = [p for _, p in named_params]
        self.offsets = {}
        off = 0
        for n, p in named_params:
            self.offsets[n] = off
            off += _round_up(p.numel(), 4)
        self.numel = off
        self.device = torch.device(device)
        self.data = torch.zeros(off, dtype=torch.float32, device=self.device)
        # gradients: zero tail padding to a multiple of 1024 elements, so the buffer splits evenly across any power-of-two
        # world size (reduce-scatter of dist.GradSync); kernels only ever touch [0, numel).  There is always at least one
        # padding element: the LAST one is the data-parallel transaction guard (lv_txn_guard_f32 writes 1 there when this rank's
        # persistent launches reported a timeout; after the mean all-reduce it is non-zero on every rank iff any rank did)
        self.grad_padded = torch.zeros(_round_up(off + 1, 1024), dtype=torch.float32, device=self.device)
        self.guard_index = self.grad_padded.numel() - 1
        self.grad = self.grad_padded[:off]
        self.views, self.gviews = {}, {}
        for n, p in named_params:
            o = self.offsets[n]
            v = self.data[o:o + p.numel()].view(p.shape)
            v.copy_(p.data.to(self.device, torch.float32))
            p.data = v
            self.views[n] = v
            self.gviews[n] = self.grad[o:o + p.numel()].view(p.shape)

        self._slots = [(self.grad_padded, self.grad, self.gviews)]
        self.detached = False

    def use_slot(self, i):
        """Gradient accumulation over micro-batches (trainer.micro_batches): slice i of a step writes its gradients into slot i --
        a second, third, ... flat gradient buffer of the same layout, created on first use -- so that slice i's exchange can be in
        flight while slice i + 1 is computed; slot 0 is the buffer param.grad aliases and the one the update reads."""
        while len(self._slots) <= i:
            gp = torch.zeros_like(self._slots[0][0])
            g = gp[:self.numel]
            gv = {n: g[self.offsets[n]:self.offsets[n] + p.numel()].view(p.shape) for n, p in zip(self.names, self.params)}
            self._slots.append((gp, g, gv))
        self.grad_padded, self.grad, self.gviews = self._slots[i]

    def bound(self):
        return all(p.data_ptr() == self.views[n].data_ptr() for n, p in zip(self.names, self.params))

    def attach_grads(self):
        """Make param.grad alias the flat gradient segments (fused driver path)."""
        for n, p in zip(self.names, self.params):
            p.grad = self._slots[0][2][n]
        self.detached = False

    def grads_are_views(self):
        """True when every parameter's .grad IS its segment of the flat gradient buffer (slot 0)."""
        gv = self._slots[0][2]
        return all(p.grad is not None and p.grad.data_ptr() == gv[n].data_ptr() and p.grad.shape == gv[n].shape
                   for n, p in zip(self.names, self.params))

    def before_autograd_backward(self):
        """Called by the drop-in autograd Functions BEFORE the engine writes a backward's gradients into the flat buffer: a .grad
        that still aliases the buffer holds something the caller has not cleared (no zero_grad since the last backward, or a fused
        trainer attached it), which autograd's += must see intact -- it is moved to storage of its own first."""
        gv = self._slots[0][2]
        for n, p in zip(self.names, self.params):
            if p.grad is not None and p.grad.data_ptr() == gv[n].data_ptr():
                p.grad = p.grad.clone()
                self.detached = True          # (a fused trainer re-attaches before its next step)

    # the drop-in path hands gradients out as views of the flat buffer (see deliver_grads); False = always as clones
    flat_grads = True

    @staticmethod
    def _accumulates_into(p):
        """True when the running backward will ACCUMULATE into leaf p's .grad -- i.e. this is a plain `loss.backward()` (or
        `backward(inputs=[..., p, ...])`).  False when the engine will not visit p's accumulation node (`backward(inputs=` without
        p, `autograd.grad` for other tensors); None under `torch.autograd.grad(..., p)`, which must be handed a real tensor to
        capture (torch refuses the query for a leaf in that mode and says so)."""
        try:
            node = torch.autograd.graph.get_gradient_edge(p).node
            return bool(torch._C._will_engine_execute_node(node))
        except (RuntimeError, AttributeError):        # autograd.grad mode -- or a torch without these hooks: hand out real tensors
            return None

    def deliver_grads(self):
        """What a drop-in autograd backward returns for the parameters once the engine has written this backward's gradients into
        the flat buffer, PER PARAMETER:
          * frozen (requires_grad False): None, and its .grad is not touched;
          * a plain `loss.backward()` reaching a parameter whose .grad is None (the state `zero_grad()` leaves, text.py:373): the
            .grad becomes a VIEW of the flat buffer and autograd is handed nothing to accumulate -- no 215 MB of clones per step at
            the Yahoo shape, and lvae.clip_grad_norm_ / lvae.SGD can run as single streaming launches over the flat buffers;
          * a backward that will not accumulate into it (`backward(inputs=...)` without it): None;
          * everything else -- `torch.autograd.grad(loss, params)` (the caller wants tensors back, .grad must stay untouched), a
            .grad that already holds something (accumulation across backward calls, zero_grad(set_to_none=False)), gradients being
            written to a micro-batch slot, `flat_grads = False` -- a clone, with autograd's usual semantics.
        ALIASING (documented contract of the zero-copy route): such a .grad is overwritten in place by the NEXT backward of the
        module; code that keeps a gradient tensor across steps (`g = p.grad; zero_grad(); ...; backward()`) must clone it, or
        switch the route off (`VAE.use_flat_grads(False)`)."""
        slot0 = self.gviews is self._slots[0][2]
        out = []
        for n, p in zip(self.names, self.params):
            if not p.requires_grad:
                out.append(None)
                continue
            acc = self._accumulates_into(p)
            if acc is False:
                out.append(None)
            elif acc and slot0 and self.flat_grads and p.grad is None:
                p.grad = self.gviews[n]
                out.append(None)
            else:
                out.append(self.gviews[n].clone())
        return tuple(out)


def _tensor_bytes(obj, depth=0):
    """Device bytes reachable from a workspace object (tensors in attributes / dict values / lists, nested up to 3 levels)."""
    if torch.is_tensor(obj):
        return obj.numel() * obj.element_size()
    if depth > 3:
        return 0
    if isinstance(obj, dict):
        return sum(_tensor_bytes(v, depth + 1) for v in obj.values())
    if isinstance(obj, (list, tuple)):
        return sum(_tensor_bytes(v, depth + 1) for v in obj)
    d = getattr(obj, "__dict__", None)
    return sum(_tensor_bytes(v, depth + 1) for v in d.values()) if d else 0


# fraction of the device memory one engine's shape-keyed workspaces may hold before the least recently used shapes are dropped
WORKSPACE_BUDGET_FRACTION = 0.2


class _WS(object):
    """Shape-keyed cache of device workspaces, least-recently-used shapes dropped beyond a byte budget.

    A (B, T) batch shape owns ~1.5 GB of activations per engine at the Yahoo dims and real corpora cycle through hundreds of
    sentence lengths (data/text_data.py batches by length): without a bound the cache grows to the whole device (a soak over
    1500 random shapes ran a 288 GB MI355X out of memory).  The shapes of the step in flight are always the most recent, so
    the budget only needs to cover one step.  `evictable = False` (set by the trainers in hipGraph mode, where captured graphs
    hold raw pointers into these buffers) keeps everything: graph mode is meant for a fixed set of shape buckets."""

    def __init__(self, device, budget_bytes=None):
        import collections
        self.device = torch.device(device)
        self.cache = collections.OrderedDict()
        self.nbytes = {}
        self.total = 0
        self.evictable = True
        self.hits = self.misses = self.evictions = 0      # (measurement: bench.py's mixed-shape run reports the hit rate)
        self.before_evict = None      # called once before workspaces are dropped (the engine orders its side streams first)
        if budget_bytes is None:
            if self.device.type == "cuda":
                budget_bytes = int(WORKSPACE_BUDGET_FRACTION * torch.cuda.get_device_properties(self.device).total_memory)
            else:
                budget_bytes = 8 << 30
        self.budget = budget_bytes

    def get(self, key, builder):
        ws = self.cache.get(key)
        if ws is not None:
            self.cache.move_to_end(key)
            self.hits += 1
            return ws
        self.misses += 1
        ws = builder()
        nb = _tensor_bytes(ws)
        self.cache[key] = ws
        self.nbytes[key] = nb
        self.total += nb
        self._trim(key)
        return ws

    def grew(self, key, nbytes):
        """A workspace of `key` allocated another buffer after it was built (lazily created images): count it."""
        if key in self.nbytes:
            self.nbytes[key] += nbytes
            self.total += nbytes
            self._trim(key)

    def _trim(self, key):
        if not self.evictable:
            return
        # drop old shapes (never one touched since the current key's shape was first used in this step: those sit at the end)
        told = False
        while self.total > self.budget and len(self.cache) > 8:
            k = next(iter(self.cache))
            if k == key:
                break
            if not told and self.before_evict is not None:
                # side-stream work of the previous step (weight-gradient GEMMs, token sort) may still read what is dropped here;
                # the caching allocator would hand the memory to the current stream at once
                self.before_evict()
                told = True
            del self.cache[k]
            self.total -= self.nbytes.pop(k)
            self.evictions += 1

    def f32(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device)

    def i16(self, *shape):
        return torch.empty(*shape, dtype=torch.int16, device=self.device)

    def i32(self, *shape):
        return torch.empty(*shape, dtype=torch.int32, device=self.device)


class _NS(object):
    pass


class _DecWS(_NS):
    """Decoder workspace; `logits` (f32 [T*B][ldl], 510 MB at the bench shape) is created on first use."""

    @property
    def logits(self):
        if self._logits is None:
            self._logits = self._alloc()
            self._grew(self._logits.numel() * self._logits.element_size())
        return self._logits


# bench.py's roofline leg: when set to a dict, kernel-launch groups are bracketed by HIP events recorded on the launch
# stream and (start, end, work, launches) is appended under the group name (measurement only; None normally).
# work = flops for the GEMM groups, timesteps for the LSTM groups.
PROFILE = None
# ... and only the groups whose name starts with this prefix (None: all).  A HIP event record costs ~5 us of an otherwise gap-free
# queue (kernel trace: profiles/r04d_timeline.txt -- 28 records = 150 us of a 3.5 ms step), so the bench brackets only the
# dominant group inside its timed region and takes the other group's times from a separate, untimed pass.
PROFILE_PREFIX = None


class _prof(object):
    def __init__(self, name, work, launches=1):
        self.name, self.work, self.launches = name, work, launches
        self.on = PROFILE is not None and (PROFILE_PREFIX is None or name.startswith(PROFILE_PREFIX))

    def __enter__(self):
        if self.on:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *a):
        if self.on:
            self.e1.record()
            PROFILE.setdefault(self.name, []).append((self.e0, self.e1, self.work, self.launches))


_GEMM_WS = {}
_PERSISTENT_DEFAULT = True


def _gemm_ws(lib, s):
    """Per-device split-K scratch (64M floats = 256 MB of the 288 GB) shared by every GEMM launch on that device's stream order."""
    dev = torch.device("cuda", torch.cuda.current_device()) if s is not None else torch.device("cpu")
    ws = _GEMM_WS.get(dev)
    if ws is None:
        ws = torch.empty(1 << 26 if dev.type == "cuda" else 1 << 20, dtype=torch.float32, device=dev)
        _GEMM_WS[dev] = ws
    return ws


def _gemm(lib, s, tA, tB, M, N, K, A, lda, B, ldb, C, ldc, alpha=1.0, acc=0, add1=None, ld1=0, mod1=1,
          add2=None, ld2=0, mod2=1, prec="f32", ws=None):
    """prec: 'f32' = exact-f32 MFMA (parity path); 'bf16' = bf16 matrix pipe with f32 accumulate (throughput path,
    only requested for the large contractions)."""
    if ws is None:
        ws = _gemm_ws(lib, s)
    fn = lib.lv_gemm_bf16 if prec == "bf16" else lib.lv_gemm_f32
    with _prof("gemm_" + prec, 2.0 * M * N * K):
        fn(tA, tB, M, N, K, alpha, A, lda, B, ldb, C, ldc, acc, add1, ld1, mod1, add2, ld2, mod2, P(ws), ws.numel(), s)


def _gemm16(lib, s, tA, M, N, K, A16, lda, B16, ldb, C, ldc, add1=None, ld1=0, mod1=1, add2=None, ld2=0, mod2=1, ws=None, acc=0):
    """C = op(A) . B^T (+ add1 + add2) with operands already rounded to bf16 in HBM (lv_gemm_b16): B stored [N][K];
    A stored [M][K] (tA = 0) or [K][M] (tA = 1).  Bit-identical to _gemm(prec='bf16') on the f32 data (up to where
    split-K cuts), at half the operand bytes and with no conversion work in the GEMM."""
    if ws is None:
        ws = _gemm_ws(lib, s)
    with _prof("gemm_bf16", 2.0 * M * N * K):
        lib.lv_gemm_b16(tA, M, N, K, 1.0, A16, lda, B16, ldb, C, ldc, acc, add1, ld1, mod1, add2, ld2, mod2,
                        P(ws), ws.numel(), s)


class _AuxStream(object):
    """A per-engine auxiliary HIP stream for work that depends only on the token ids and must merely be finished by the
    time the embedding gradient is scattered: the stable token sort (one workgroup, ~60 us at the bench shape) and the
    zero fill of the embedding-gradient table.  Runs them beside the latency-bound LSTM chains, which leave almost every
    CU idle; inline on the test backend."""

    def __init__(self):
        self.stream = None
        self.done = None

    def run(self, device, fn, keep=()):
        """keep: tensors fn reads on the side stream (told to the caching allocator, so that a caller that drops them
        right after a forward-only call cannot have them recycled underneath the side stream)."""
        device = torch.device(device)
        # inline on the test backend, and under hipGraph capture: a forked branch in a replayed graph was measured to
        # cost ~0.5 ms per step, far more than the 0.15 ms the side stream saves in eager mode
        if device.type != "cuda" or torch.cuda.is_current_stream_capturing():
            fn(None)
            return
        if self.stream is None:
            self.stream = torch.cuda.Stream(device)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self.stream.wait_event(ev)
        for t in keep:
            t.record_stream(self.stream)
        with torch.cuda.stream(self.stream):
            fn(self.stream.cuda_stream)
            self.done = torch.cuda.Event()
            self.done.record(self.stream)

    def join(self, device):
        if self.done is not None:
            torch.cuda.current_stream(torch.device(device)).wait_event(self.done)
            self.done = None


class _TokenSortCache(object):
    """The stable (token, row) sort of the embedding backward depends on the token ids alone, and the aggressive loop keeps
    meeting the same batch tensors (text.py:389 draws from the fixed list train_data_batch): the sorted (rows, tokens) pair is
    kept per batch TENSOR -- weakly (it dies with the tensor) and only while the tensor's version counter is unchanged -- so that
    in steady state the two single-workgroup sort launches of a step (75 us each, and nothing can run beside the persistent
    recurrences they used to hide behind) disappear.  Not used under hipGraph capture (a captured step owns fixed buffers).

    CONTRACT: a batch tensor handed to step() is immutable, as the reference's train_data_batch entries are.  In-place torch ops
    bump the version counter and are noticed; writes that bypass it are NOT -- `x.data.copy_(...)`, a numpy view of a CPU tensor,
    DLPack / custom-kernel writes into a reused device buffer: after those call `invalidate(x)` (or pass a fresh tensor), else the
    embedding gradients of both networks are scattered with the old batch's token lists.  At most LIMIT batches are kept, the least
    recently used ones go first."""
    LIMIT = 8192

    def __init__(self):
        import collections
        self.map = collections.OrderedDict()   # id(tensor) -> (weak reference to the tensor, {tag: (version, rows, tokens)})

    def _entries(self, key_tensor, create):
        i = id(key_tensor)
        ent = self.map.get(i)
        if ent is not None and ent[0]() is key_tensor:
            self.map.move_to_end(i)
            return ent[1]
        if not create:
            return None
        import weakref
        while len(self.map) >= self.LIMIT:
            self.map.popitem(last=False)       # least recently used batch (its buffers go back to the caching allocator)
        # (tensors compare element-wise, so they cannot key a WeakKeyDictionary: identity + a weak reference that retires the id)
        self.map[i] = (weakref.ref(key_tensor, lambda _r, i=i, m=self.map: m.pop(i, None)), {})
        return self.map[i][1]

    def get(self, key_tensor, tag):
        ent = self._entries(key_tensor, False)
        hit = ent.get(tag) if ent is not None else None
        return hit[1:] if hit is not None and hit[0] == key_tensor._version else None

    def put(self, key_tensor, tag, srows, stok):
        self._entries(key_tensor, True)[tag] = (key_tensor._version, srows, stok)

    def invalidate(self, key_tensor=None):
        """Forget the sorted lists of one batch tensor (None: of all) -- for callers that rewrote a batch behind the version counter."""
        if key_tensor is None:
            self.map.clear()
        else:
            self.map.pop(id(key_tensor), None)


def reset_persistent_status(eng):
    """Clear the status word (after the caller has handled a reported timeout, e.g. by moving down the fallback ladder)."""
    if eng.status is not None:
        eng.status.zero_()


# ---- the fallback ladder of the persistent recurrences -----------------------------------------------------------------------
# rung 0: persistent launches, hand-off granules kept in the XCD's L2 (persist_flags bit 0) -- the fast form, which ASSUMES that
#         the 32 workgroups of a group (blockIdx % 8) share an XCD: checked by the bounded spins, never proven;
# rung 1: persistent launches with agent-scope (write-through) granules: any placement works as long as all 256 workgroups are
#         resident together (they are not when something else holds compute units, e.g. a collective's kernels);
# rung 2: the launch-per-timestep kernels: no co-residency assumption at all.
# A timeout is reported through the engine's device status word; the fused trainers gate every update on it ON THE DEVICE
# (lv_clip_*_txn_f32), notice it at their next host read, call demote_persistent() and replay the voided steps.
PERSIST_RUNGS = ("persistent, XCD-local hand-off", "persistent, write-through hand-off", "launch-per-timestep kernels")


def persist_rung(eng):
    if not eng.persistent:
        return 2
    return 0 if (eng.persist_flags & 1) else 1


def demote_persistent(eng):
    """Move `eng` one rung down the ladder and clear its status word; returns the new rung.  Raises when there is nothing left
    (the launch-per-timestep kernels have no hand-off that could time out)."""
    r = persist_rung(eng)
    if r == 0:
        eng.persist_flags &= ~1
    elif r == 1:
        eng.persistent = False
    else:
        raise _lib.LvaeError("a persistent-launch timeout was reported although the engine runs the launch-per-timestep kernels")
    reset_persistent_status(eng)
    # whoever demotes (a trainer's _settle, training.guarded_eval): captured hipGraphs hold the launches of the rung that failed --
    # the trainers key their graphs by this counter and re-capture (guarded_eval demoted behind the trainer's back)
    eng.ladder_gen = getattr(eng, "ladder_gen", 0) + 1
    return r + 1


def status_ptr(eng):
    """Device pointer of the engine's persistent-launch status word (None before ensure())."""
    return P(eng.status) if eng.status is not None else None


_PERSIST_H = 1024        # lv_lstm_persist16.hip is built for this hidden size
# The persistent launches (lv_lstm_persist16.hip): <= 16 rows per XCD group, so B <= 128 (BASELINE.json configs[4] runs 16 rows on
# each of the 8 groups); eng.persist_rows asks for a row count per group (e.g. 8 rows on four groups = a B = 32 recurrence on
# half the chip); eng.persist_flags bit 0 keeps the hand-off granules in the XCD's L2 (no agent-scope write-through; measured
# 3.2 -> 2.2 us per forward timestep, 3.1 -> 2.7 us per BPTT timestep at B = 32) -- rung 0 of the ladder above.
_PERSIST_MAX_B = 128


def _persist_rows(eng, B):
    """Rows per XCD group for a persistent launch of batch B on this engine."""
    rows = getattr(eng, "persist_rows", None)
    if rows is not None and 8 * rows >= B and 1 <= rows <= 16:
        return int(rows)
    return (B + 7) // 8


def _saved_floats(eng, T, B, H):
    """Floats of one LSTM layer's saved-activation buffer: gates [T][B][4H] for the step kernels; the persistent kernels keep
    gates AND cell states in a workgroup-major record buffer of their own size."""
    n = T * B * 4 * H
    if H == _PERSIST_H and eng.precision == "bf16" and eng.persistent and B <= _PERSIST_MAX_B:
        n = max(n, eng.lib.lv_lstm_persist16_saved_floats(T, _persist_rows(eng, B)))
    return n


def _persistent_ok(eng, img, B, H, device, max_b):
    return (eng.precision == "bf16" and img is not None and eng.persistent and H == _PERSIST_H and B <= max_b
            and torch.device(device).type == "cuda" and torch.cuda.get_device_properties(device).multi_processor_count >= 256)


# The 4-row persistent forward computes its own input projection (lv_lstm_fwd_bf16_persist16_x: no Gx product, no Gx buffer);
# LVAE_FUSED_GX=0: the projection GEMM + Gx path, for A/B measurements.  FUSED_GX_ENC / FUSED_GX_DEC decide the two layers apart.
FUSED_GX = os.environ.get("LVAE_FUSED_GX", "1") != "0"
FUSED_GX_ENC = True
FUSED_GX_DEC = True
_FUSED_GX_NI = 512       # the input width lv_lstm_fwd_bf16_persist16_x is built for


def _fused_gx_ok(eng, img, B, H, ni, device, layer_on):
    """The forward of this layer runs as the persistent launch that forms Gx itself: the persistent path is on (any demotion
    down the ladder turns this off with it, and the caller computes Gx as before), the shape is the kernel's (ni = 512, <= 4 rows
    per group), and the engine does not belong to a hipGraph trainer (ws_evictable False: its workspaces are pinned and its eager
    warm-up steps must run what the captured ones will) nor is the launch being captured (captured steps keep the GEMM + Gx path)."""
    if not (FUSED_GX and layer_on and ni == _FUSED_GX_NI and eng.ws_evictable and _persistent_ok(eng, img, B, H, device, _PERSIST_MAX_B)):
        return False
    if _persist_rows(eng, B) > 4:
        return False
    return not (torch.cuda.is_current_stream_capturing() or (eng._wimg is not None and getattr(eng._wimg, "xstate", {}).get("captured")))


def _gx_buffer(c, w, rows, H):
    """w.Gx [rows][4H] f32, allocated when a path that materialises the input projection first runs (the fused forward never does:
    2 x 105 MB at the Yahoo shape)."""
    if w.Gx is None:
        w.Gx = c.f32(rows, 4 * H)
        c.grew(w.ws_key, rows * 4 * H * 4)
    return w.Gx


def weights_version(eng):
    """Changes whenever the module's weights may have changed: in-place torch updates bump the parameters' version
    counters (optimizer.step, load_state_dict, user edits), raw-pointer updates by the fused trainer bump eng.wgen."""
    return (sum(p._version for p in eng.flat.params), eng.wgen)


def _weight_images(eng, lib, s, device, want_persist, lstm=True, pred=False):
    """Engine-level bf16 images of the module's weights for the throughput path -- W_ih rows in unit-major gate order
    (4u + g: Gx comes out with each unit's (i,f,g,o) side by side), W_ih^T [ni][4H] (contraction index of dX), for the
    decoder also pred_linear.weight / its transpose, and the packed register images of W_hh for the persistent
    recurrences -- rebuilt when weights_version() changed, or on every call when eng.cache_weight_images is off.
    The decoder is frozen for the whole aggressive inner loop (text.py:371-400 steps the encoder only), so its images
    are built once per outer iteration."""
    wi = eng._wimg
    V, ni, H = eng.dims()[:3]
    v = eng.flat.views
    c = eng.wsc
    if wi is None:
        wi = eng._wimg = _NS()
        wi.ver = object()
        wi.W = wi.WT = wi.pred = wi.predT = wi.fwd16 = wi.bwd16 = wi.xch = None
        if lstm:
            wi.W = c.i16(4 * H, ni)
            wi.WT = c.i16(ni, 4 * H)
        wi.ldv = _round_up(V, 32)
        if pred:
            wi.pred = c.i16(V, H)
            wi.predT = c.i16(H, wi.ldv)
        wi.packed16 = False
    ver = weights_version(eng) if eng.cache_weight_images else object()
    h16 = bool(getattr(eng, "_h16_now", False))      # the forward's operand images in IEEE binary16 (LSTMEncoderEngine.fwd_operands)
    stale = wi.ver != ver or getattr(wi, "h16", False) != h16
    if stale:
        wih = v["lstm.weight_ih_l0"]
        if wi.W is not None and h16:
            # W (forward: Gx) as binary16, W^T (backward: dX) as bf16, one launch
            lib.lv_cvt_h16_f32(P(wih), wih.shape[1], 4 * H, ni, H, None, 0, 1, 0, P(wi.W), ni, P(wi.WT), 4 * H, s)
        elif wi.W is not None:
            lib.lv_cvt_bf16_gates_f32(P(wih), wih.shape[1], H, ni, P(wi.W), ni, P(wi.WT), 4 * H, s)
        wi.h16 = h16
        if wi.pred is not None:
            lib.lv_cvt_bf16_f32(P(v["pred_linear.weight"]), H, V, H, P(wi.pred), H, P(wi.predT), wi.ldv, s)
        wi.ver = ver
        wi.packed16 = False
    if want_persist and not wi.packed16:
        if wi.fwd16 is None:
            n = lib.lv_lstm_persist16_wpk_floats()
            wi.fwd16, wi.bwd16 = c.f32(n), c.f32(n)
            # hand-off exchange buffer, zeroed once: the launches alternate its halves and clear the other one themselves
            wi.xch = torch.zeros(lib.lv_lstm_persist16_xch_floats(), dtype=torch.float32, device=c.device)
            wi.xstate = {"f": 0, "g": 0, "gcls": [0, 0]}      # next half per kind of launch; instantiation that last used each BPTT half
        (lib.lv_lstm_persist16_pack2_h16 if h16 else lib.lv_lstm_persist16_pack2)(P(v["lstm.weight_hh_l0"]), P(wi.fwd16), P(wi.bwd16), H, s)
        wi.packed16 = True
    return wi


def _xch_flags(wi, kind, rows, device, T=1):
    """Flag bits 1.. of a persistent launch (lv_lstm_persist16_xch_floats): the exchange buffer's halves alternate per kind of launch
    ("f" forward, "g" BPTT) and every launch clears the other half of its kind itself -- no memset launch in front (4 per training
    step before: ~26 us).  Not under hipGraph capture: a replay repeats the captured half, so captured launches keep half 0 behind
    their memset (and leave the alternation state alone)."""
    st = wi.xstate
    if T <= 0:
        # the launch returns before it touches the exchange (and before it would clear the other half): the alternation must not
        # advance, or the next launch of this kind would poll a half that still holds the tags of the launch before last
        return 0
    if torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing():
        st["captured"] = True
    if st.get("captured"):
        # a captured launch dirties half 0 at every replay, unseen from here: once an engine's launches live in a graph, ALL its
        # launches (eager ones too) stay in the memset form
        return 0
    half = st[kind]
    st[kind] = 1 - half
    fl = 2 | (half << 2)
    if kind == "g":
        cls = 1 if rows <= 4 else (2 if rows <= 8 else 3)
        fl |= st["gcls"][1 - half] << 3          # clear the other half over what its last user dirtied (0: never used -> own extent)
        st["gcls"][half] = cls
        st["gcls"][1 - half] = 0
    return fl


class SeqLengths(object):
    """The validated sentence lengths of a variable-length batch (x [B][T], lengths) -- reference VarLSTMEncoder / VarLSTMDecoder,
    enc_lstm.py:95-99, dec_lstm.py:391-420.  A length counts every token of its row, <s> and </s> included.  `lengths`: a list of
    ints or an integer tensor on any device, one per row, 2 <= length <= T, in any order (the reference wants them sorted and
    max(length) == T; neither is needed here).  Anything else raises ValueError before a launch.
    .host: the lengths as ints; .max; .enc: int32 [B] on `device` (the encoder's step counts); .dec(ns): int32 [B*ns], length - 1
    repeated over a sentence's samples (the decoder predicts no <s>)."""

    def __init__(self, lengths, B, T, device):
        if torch.is_tensor(lengths):
            if lengths.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8) or lengths.dim() != 1:
                raise ValueError("sentence lengths: a 1-D integer tensor or a list of ints expected, got %s %s"
                                 % (lengths.dtype, tuple(lengths.shape)))
            host = [int(v) for v in lengths.detach().cpu().tolist()]
        else:
            try:
                host = list(lengths)
            except TypeError:
                raise ValueError("sentence lengths: a 1-D integer tensor or a list of ints expected, got %r" % (type(lengths),))
            if not all(isinstance(v, int) and not isinstance(v, bool) for v in host):
                raise ValueError("sentence lengths: a list of ints expected")
        if len(host) != B:
            raise ValueError("sentence lengths: %d values for a batch of %d sentences" % (len(host), B))
        if B > 0 and min(host) < 2:
            raise ValueError("sentence lengths: every sentence holds at least <s> and </s>; got a length of %d" % min(host))
        if B > 0 and max(host) > T:
            raise ValueError("sentence lengths: a length of %d in a batch tensor of %d columns" % (max(host), T))
        self.host, self.B, self.T = host, B, T
        self.device = torch.device(device)
        self.max = max(host) if host else 0
        self.enc = torch.tensor(host, dtype=torch.int32).to(self.device)
        self._dec = {}

    def dec(self, ns=1):
        d = self._dec.get(ns)
        if d is None:
            d = self._dec[ns] = (self.enc - 1).repeat_interleave(ns).contiguous()
        return d

    @staticmethod
    def of(lengths, B, T, device):
        if isinstance(lengths, SeqLengths) and (lengths.B, lengths.T, lengths.device) == (B, T, torch.device(device)):
            return lengths
        return SeqLengths(lengths.host if isinstance(lengths, SeqLengths) else lengths, B, T, device)


def varlen_batch(x):
    """(x [B][T], lengths) -> (x cut to max(lengths) columns, SeqLengths): the validated form of a variable-length batch.  The
    columns beyond the longest sentence are padding that no row ever reaches.  Idempotent."""
    xt, lengths = x
    if not (torch.is_tensor(xt) and xt.dim() == 2 and xt.dtype == torch.int64):
        raise ValueError("a variable-length batch is a pair (int64 tensor [batch][seq_len], lengths)")
    B, T = xt.shape
    L = SeqLengths.of(lengths, B, T, xt.device)
    if B > 0 and L.max < T:
        xt = xt[:, :L.max].contiguous()
        L = SeqLengths.of(L, B, L.max, xt.device)
    return xt, L


def length_groups(L):
    """[(length, int64 row indices on the device)] of the by-length route, in decreasing length."""
    by = {}
    for b, n in enumerate(L.host):
        by.setdefault(n, []).append(b)
    return [(n, torch.tensor(by[n], dtype=torch.int64).to(L.device)) for n in sorted(by, reverse=True)]


class GroupedBackward(object):
    """The by-length route's book-keeping (VarLSTMEncoder / VarLSTMDecoder with masked = False): an engine keeps one step in
    flight and its backward writes the flat gradient buffer with '=' semantics, so a batch cut into equal-length groups runs one
    forward per group -- each on the workspace of its own (rows, T) shape -- with the engine's record of the step (`last` and
    friends) set aside, and one backward per group with that record put back, the groups' gradients summed by lv_add_f32."""
    FIELDS = ("last", "last_ns", "last_steps", "_sort")

    def __init__(self, eng):
        self.eng = eng
        self.saved = []

    def after_forward(self, w):
        self.saved.append(({k: getattr(self.eng, k, None) for k in self.FIELDS}, w))

    def backward(self, i, current_ws, run):
        """Group i: restore its record, check that its workspace is still the one its forward wrote, run(gen), add up."""
        eng = self.eng
        rec, w = self.saved[i]
        for k, val in rec.items():
            setattr(eng, k, val)
        if current_ws() is not w:
            raise _lib.LvaeError("the by-length route's activations were dropped from the workspace cache between forward and backward "
                                 "(raise engine.WORKSPACE_BUDGET_FRACTION)")
        out = run(rec["last"][-1])
        if hasattr(eng, "join"):
            eng.join()
        f = eng.flat
        lib, s = eng.lib, stream_ptr(f.device)
        if i == 0:
            self.total = f.grad.clone()
        else:
            lib.lv_add_f32(P(self.total), P(f.grad), P(self.total), f.grad.numel(), s)
        if i == len(self.saved) - 1 and i > 0:
            f.grad.copy_(self.total)
        return out


def _refuse_bf16_lengths(eng):
    if eng.precision == "bf16":
        raise _lib.LvaeError("variable-length batches (x, lengths) run the exact-f32 configuration only: the bf16 and the persistent "
                             "recurrences have no length-aware form; call set_precision('f32') or batch by length")


def _same_device(what, dev, **operands):
    """The kernels take raw pointers: an operand on another device is refused before anything is launched."""
    for name, t in operands.items():
        if t is not None and t.device != dev:
            raise _lib.LvaeError("%s: %s is on %s, x on %s" % (what, name, t.device, dev))


def iters_per_launch_for(who, iters_per_launch, x):
    """The chunk length of a sampler's launches and noise draws: iters_per_launch, refused below 1; None is
    LSTMDecoderEngine.mh_default_iters_per_launch(T) for a 2-D tensor x (T = 33 for anything else)."""
    if iters_per_launch is None:
        T = x.size(1) if (torch.is_tensor(x) and x.dim() == 2) else 33
        return LSTMDecoderEngine.mh_default_iters_per_launch(T)
    per = int(iters_per_launch)
    if per < 1:
        raise ValueError("%s: iters_per_launch >= 1 expected" % who)
    return per


def _prefetch_noise(who, draw, total, per, B, C, nz, device, device_msg=None):
    """Every chunk's noise of a fused chain, fetched and checked before the first launch -> [(i0, n, eps, u)], float32 and
    contiguous.  device_msg: the caller's wording of the device refusal (filled with eps's, u's and x's device); None:
    _same_device's."""
    chunks = []
    for i0 in range(0, total, per):
        n = min(per, total - i0)
        eps, u = draw(i0, n)
        if device_msg is None:
            _same_device(who, device, eps=eps, u=u)
        elif eps.device != device or u.device != device:
            raise _lib.LvaeError(device_msg % (eps.device, u.device, device))
        if tuple(eps.shape) != (n, B, C, nz) or tuple(u.shape) != (n, B, C):
            raise ValueError("%s: eps [%d][%d][%d][%d] and u [%d][%d][%d] expected, got %s and %s"
                             % (who, n, B, C, nz, n, B, C, tuple(eps.shape), tuple(u.shape)))
        chunks.append((i0, n, eps.contiguous().float(), u.contiguous().float()))
    return chunks


def _lstm_forward(eng, lib, s, img, w, Gx, whh, mask, scale, hdrop, T, B, H, device, steps=None, xin=None):
    """The forward recurrence of one LSTM layer: exact f32, bf16 launch-per-step, or (bf16 image path on a >= 256-CU
    device, H = 1024, B <= 128) the single persistent launch of lv_lstm_persist16.hip.  steps = (int32 [B] on the device,
    their maximum): the length-aware exact-f32 recurrence (lv_lstm_fwd_len_f32), row b active while t < steps[b].
    xin = (addend, addend_row_stride) from _LstmImages.forward(product=False): no Gx exists, the persistent launch forms it from
    img.X and the unit-major image of W_ih (the caller asked _fused_gx_ok first)."""
    if xin is not None and not (steps is None and _persistent_ok(eng, img, B, H, device, _PERSIST_MAX_B)):
        raise _lib.LvaeError("the fused input projection exists in the persistent forward only")
    args = (Gx, whh, P(w.hs), P(w.cs), P(w.gates), mask, scale, hdrop)
    w.saved_layout = ("canonical", T, B, 0)
    if steps is not None:
        _refuse_bf16_lengths(eng)
        lib.lv_lstm_fwd_len_f32(*args, P(w.lstm_ws), P(steps[0]), steps[1], T, B, H, s)
    elif eng.precision != "bf16":
        lib.lv_lstm_fwd_f32(*args, P(w.lstm_ws), T, B, H, s)
    elif img is None:
        lib.lv_lstm_fwd_bf16(*args, P(w.lstm_ws), T, B, H, s)
    elif _persistent_ok(eng, img, B, H, device, _PERSIST_MAX_B):
        wi = eng._wimg          # packed by _weight_images(want_persist=True) at the top of the forward
        rows = _persist_rows(eng, B)
        if mask is not None or hdrop is not None:
            raise _lib.LvaeError("the persistent forward has no in-kernel dropout (the engine applies it on the images)")
        need = lib.lv_lstm_persist16_saved_floats(T, rows)
        if w.gates.numel() < need:              # eng.persist_rows / eng.persistent changed after the workspace was built
            w.gates = torch.empty(need, dtype=torch.float32, device=w.gates.device)
        flags = eng.persist_flags | _xch_flags(wi, "f", rows, device, T) | (32 if getattr(wi, "h16", False) else 0)
        if xin is not None:
            lib.lv_lstm_fwd_bf16_persist16_x(P(img.X), img.ni, P(wi.W), img.ni, xin[0], xin[1], P(wi.fwd16), P(w.hs), P(w.cs),
                                             P(w.gates), P(wi.xch), P(eng.status), T, B, rows, flags, H, s)
        else:
            lib.lv_lstm_fwd_bf16_persist16(Gx, P(wi.fwd16), P(w.hs), P(w.cs), P(w.gates), P(wi.xch), P(eng.status), T, B, rows, flags, H, s)
        w.saved_layout = ("persist16", T, B, rows)      # what w.gates holds now: the BPTT must be given the same T, B, R
    else:
        lib.lv_lstm_fwd_bf16_ug(*args, P(w.lstm_ws), T, B, H, s)


_PERSIST_BWD_MAX_B = 128


def check_persistent_status(eng):
    """Raise if a persistent LSTM launch of this engine ever reported a hand-off timeout (device status word; one host
    read -- call it where the host synchronises anyway)."""
    st = eng.status
    if st is not None and int(st.item()) != 0:
        raise _lib.LvaeError("persistent LSTM kernel reported hand-off timeout (status %d) on ladder rung %d (%s): not all 256 "
                             "workgroups were resident (e.g. another kernel held compute units for seconds), or -- with "
                             "eng.persist_flags bit 0 set -- a group's workgroups were not placed on one XCD.  The fused trainers "
                             "recover from this by themselves (engine.demote_persistent); on the drop-in autograd path call it and "
                             "redo the step" % (int(st.item()), persist_rung(eng), PERSIST_RUNGS[persist_rung(eng)]))


def _need_canonical_saved(w):
    lay = getattr(w, "saved_layout", None)
    if lay is not None and lay[0] != "canonical":
        raise _lib.LvaeError("the saved activations are in the 16-row persistent kernels' own order %r, but the backward was routed to a "
                             "kernel that reads gates [T][B][4H] / cs: eng.persistent / eng.persist_rows changed between forward and "
                             "backward" % (lay,))


def _lstm_backward(eng, lib, s, img, w, dh_ext, dh_last, mask, scale, whh, dh0, dc0, tanh_init, T, B, H, device, steps=None):
    """BPTT of one LSTM layer: exact f32, bf16 two launches per step, or the single persistent launch where supported.
    steps: as _lstm_forward's (lv_lstm_bwd_len_f32)."""
    if steps is not None:
        _refuse_bf16_lengths(eng)
        lib.lv_lstm_bwd_len_f32(dh_ext, dh_last, mask, scale, whh, P(w.gates), P(w.hs), P(w.cs), P(w.dG), P(w.dGsum), P(w.lstm_ws),
                                dh0, dc0, tanh_init, P(steps[0]), steps[1], T, B, H, s)
        return
    if eng.precision != "bf16":
        lib.lv_lstm_bwd_f32(dh_ext, dh_last, mask, scale, whh, P(w.gates), P(w.hs), P(w.cs), P(w.dG), P(w.dGsum), P(w.lstm_ws),
                            dh0, dc0, tanh_init, T, B, H, s)
        return
    dG = P(w.dG) if img is None else None
    dG16 = P(img.dG) if img is not None else None
    if _persistent_ok(eng, img, B, H, device, _PERSIST_BWD_MAX_B):
        wi = eng._wimg
        rows = _persist_rows(eng, B)
        if mask is not None:
            raise _lib.LvaeError("the persistent BPTT has no in-kernel dropout mask (the engine applies it on dO)")
        if getattr(w, "saved_layout", None) != ("persist16", T, B, rows):
            raise _lib.LvaeError("the saved activations were not written by a persistent forward with the same T, B and rows per "
                                 "group (%r): eng.persist_rows / eng.persistent changed between forward and backward" % (getattr(w, "saved_layout", None),))
        lib.lv_lstm_bwd_bf16_persist16(dh_ext, dh_last, P(wi.bwd16), P(w.gates), P(w.hs), P(w.cs), dG16, P(w.dGsum), P(wi.xch),
                                       P(eng.status), dh0, dc0, tanh_init, T, B, rows, eng.persist_flags | _xch_flags(wi, "g", rows, device, T), H, s)
    else:
        _need_canonical_saved(w)
        lib.lv_lstm_bwd_bf16_img(dh_ext, dh_last, mask, scale, whh, P(w.gates), P(w.hs), P(w.cs), dG, dG16, P(w.dGsum),
                                 P(w.lstm_ws), dh0, dc0, tanh_init, T, B, H, s)


# dW_ih and dW_hh of an LSTM layer as one product where the shape allows (LVAE_DUAL_WGRAD=0: two products, for A/B measurements)
DUAL_WGRAD = os.environ.get("LVAE_DUAL_WGRAD", "1") != "0"
# ... and dX with them in one grouped stream-K launch on the 256 x 256 tile where the shapes are big enough (LVAE_PAIR_WGRAD=0: the
# separate launches, for A/B measurements)
PAIR_WGRAD = os.environ.get("LVAE_PAIR_WGRAD", "1") != "0"
# The decoder's three hidden-state images (O, O^T, h_prev^T) from one pass over hs (lv_cvt_bf16_hs3_f32; LVAE_HS3_CVT=0: the two
# separate conversions, for A/B measurements)
HS3_CVT = os.environ.get("LVAE_HS3_CVT", "1") != "0"


class _LstmImages(object):
    """bf16 operand images of one LSTM layer's input-side GEMMs (Gx = X.W_ih^T forward; dX = dG.W_ih,
    dW_ih = dG^T.X, dW_hh = dG^T.h_prev backward), built with lv_cvt_bf16_f32 next to the f32 originals."""

    def __init__(self, c, TB, ni, H, key=None):
        self.TB, self.ni, self.H = TB, ni, H
        self.key = key                      # this object's key in the workspace cache (byte accounting of the lazy addend)
        self.ldr = _round_up(TB, 8)
        self.X = c.i16(TB, ni)              # layer input rows            [T*B][ni]
        # X^T [ni][T*B] and h_{t-1}^T [H][T*B] in ONE buffer: the two weight gradients that share dG as their A operand,
        # dW_ih = dG^T X and dW_hh = dG^T h_prev, are then one product over the image [X^T ; h_prev^T] (lv_gemm_b16_dual)
        self.XhT = c.i16(ni + H, self.ldr)
        self.addend = None                  # unit-major copy of the Gx epilogue addend (biases / z-projection)
        self.dG = c.i16(TB, 4 * H)          # gate pre-activation grads   [T*B][4H]
        self.hT_gen = None                  # the owner's forward generation whose h_prev image hT already holds (decoder: hs3)
        self.hT_ld = self.ldr

    @property
    def XT(self):                           # layer input rows, transposed [ni][T*B]
        return self.XhT[:self.ni]

    @property
    def hT(self):                           # h_{t-1} rows, transposed     [H][T*B]
        return self.XhT[self.ni:]

    @staticmethod
    def usable(precision, native16, ni, H):
        return precision == "bf16" and native16 and ni % 8 == 0 and H % 8 == 0

    def forward(self, lib, s, X, W16, Gx, add_a, add_b, rows, wsc, addend_um=None, gather=None, h16=False, product=True):
        """Gx[r][4u + g] = X[r] . W_ih[g*H + u] + (add_a + add_b)[r % rows][g*H + u]; W16: the unit-major bf16 image of W_ih
        (engine-level, _weight_images); add_a/add_b: gate-major [rows][4H] (add_b may be None), or addend_um: the addend
        already in unit-major order.  gather = (emb, ids, ids_stride, keep, kscale, T, B, V): the layer input is an embedding
        lookup (+ dropout) -- its bf16 images are gathered straight from the table (lv_embed_gather_b16) and X (f32) is not read.
        product = False: the images and the addend are built but no product is launched and Gx is not touched; returns
        (addend pointer, its row stride in floats -- 0: one row) for the forward that forms Gx itself (_lstm_forward's xin)."""
        TB, ni, H = self.TB, self.ni, self.H
        if addend_um is not None:
            addend = addend_um
        else:
            if self.addend is None or self.addend.shape[0] != rows:
                self.addend = wsc.f32(rows, 4 * H)
                if self.key is not None:
                    wsc.grew(self.key, rows * 4 * H * 4)
            lib.lv_gate_interleave_f32(add_a, add_b, rows, H, P(self.addend), s)
            addend = P(self.addend)
        if h16:
            # binary16 forward operands (W16 is the binary16 image of W_ih): X as binary16 for this product, X^T as bf16 for dW_ih
            emb, ids, ids_stride, keep, kscale, T, B, V = gather
            assert keep is None
            lib.lv_cvt_h16_f32(emb, ni, TB, ni, 0, ids, ids_stride, B, V, P(self.X), ni, P(self.XT), self.ldr, s)
            if not product:
                return addend, 4 * H if rows > 1 else 0
            ws = _gemm_ws(lib, s)
            with _prof("gemm_bf16", 2.0 * TB * 4 * H * ni):
                lib.lv_gemm_h16(TB, 4 * H, ni, 1.0, P(self.X), ni, W16, ni, Gx, 4 * H, 0, addend, 4 * H if rows > 1 else 0, rows, None, 0, 1,
                                P(ws), ws.numel(), s)
            return
        if gather is not None:
            emb, ids, ids_stride, keep, kscale, T, B, V = gather
            lib.lv_embed_gather_b16(emb, ids, ids_stride, keep, kscale, T, B, ni, V, P(self.X), ni, P(self.XT), self.ldr, s)
        else:
            lib.lv_cvt_bf16_f32(X, ni, TB, ni, P(self.X), ni, P(self.XT), self.ldr, s)
        if not product:
            return addend, 4 * H if rows > 1 else 0
        _gemm16(lib, s, 0, TB, 4 * H, ni, P(self.X), ni, W16, ni, Gx, 4 * H,
                add1=addend, ld1=4 * H if rows > 1 else 0, mod1=rows)

    def backward(self, lib, s, dG, h_prev, WT16, dX, gW_ih, ld_gw, gW_hh, ws=None, between=None, hT_current=False):
        """dG: the f32 gate gradients, or None when the BPTT kernel already wrote their bf16 image into self.dG; WT16: the
        bf16 image of W_ih^T [ni][4H] (engine-level).  between(): called once dX is queued and before the two weight-gradient
        products (the encoder scatters its embedding gradient there, so that a data-parallel exchange of it can start under
        the weight-gradient GEMMs).  hT_current: self.hT already is the image of h_prev (the decoder's forward wrote it)."""
        TB, ni, H = self.TB, self.ni, self.H
        if dG is not None:
            lib.lv_cvt_bf16_f32(dG, 4 * H, TB, 4 * H, P(self.dG), 4 * H, None, 0, s)
        wsd = ws if ws is not None else _gemm_ws(lib, s)
        if PAIR_WGRAD and DUAL_WGRAD and lib.lv_gemm_b16_pair_supported(1, 4 * H, ni + H, TB, 0, TB, ni, 4 * H, wsd.numel()):
            # all three products of the layer in ONE grouped launch on the 256 x 256 tile (lv_gemm_b16_pair): [dW_ih | dW_hh] on the
            # share of the CUs its flops ask for, dX on the rest, tiles shared between workgroups summed inside the launch
            if not hT_current:
                lib.lv_cvt_bf16_f32(h_prev, H, TB, H, None, 0, P(self.hT), self.ldr, s)
            with _prof("gemm_bf16", 2.0 * 4 * H * (ni + H) * TB + 2.0 * TB * ni * 4 * H):
                lib.lv_gemm_b16_pair(1, 4 * H, ni + H, TB, P(self.dG), 4 * H, P(self.XhT), self.ldr, gW_ih, ld_gw, ni, gW_hh, H,
                                     0, TB, ni, 4 * H, P(self.dG), 4 * H, WT16, 4 * H, dX, ni, P(wsd), wsd.numel(), s)
            if between is not None:
                between()
            return
        _gemm16(lib, s, 0, TB, ni, 4 * H, P(self.dG), 4 * H, WT16, 4 * H, dX, ni, ws=ws)
        if between is not None:
            between()
        if not hT_current:
            lib.lv_cvt_bf16_f32(h_prev, H, TB, H, None, 0, P(self.hT), self.ldr, s)
        if DUAL_WGRAD and ni % 4 == 0 and lib.lv_gemm_b16_dual_supported(4 * H, ni + H, TB, wsd.numel()):
            # both weight gradients as one product (N = ni + H columns, split between the two destinations in its reduction stage)
            with _prof("gemm_bf16", 2.0 * 4 * H * (ni + H) * TB):
                lib.lv_gemm_b16_dual(1, 4 * H, ni + H, TB, P(self.dG), 4 * H, P(self.XhT), self.ldr, gW_ih, ld_gw, ni, gW_hh, H,
                                     P(wsd), wsd.numel(), s)
            return
        _gemm16(lib, s, 1, 4 * H, ni, TB, P(self.dG), 4 * H, P(self.XT), self.ldr, gW_ih, ld_gw, ws=ws)
        _gemm16(lib, s, 1, 4 * H, H, TB, P(self.dG), 4 * H, P(self.hT), self.ldr, gW_hh, H, ws=ws)


class _LstmImagesMS(object):
    """The decoder's operand images for multi-sample training (ns > 1 samples per sentence, decoder row bd = b * ns + s): the
    INPUT side -- embedded rows X, X^T and the sample-summed gate gradients dGs -- lives on Td * B sentence rows, the
    RECURRENT side -- h_prev^T and the gate gradients dG the BPTT writes -- on Td * B * ns decoder rows.  The two weight
    gradients no longer share a contraction length (Td * B against Td * B * ns), so _LstmImages' dual product over
    [X^T ; h_prev^T] does not apply: dW_hh is a product of its own over Td * B * ns rows, dW_ih[:, :ni] and dX run over Td * B rows --
    as one grouped lv_gemm_b16_pair launch where lv_gemm_b16_pair_supported takes the two shapes, else as two lv_gemm_b16 products
    (DESIGN.md 3.3)."""

    def __init__(self, c, Td, B, ns, ni, H):
        self.Td, self.B, self.ns, self.ni, self.H = Td, B, ns, ni, H
        self.TB, self.TBd = Td * B, Td * B * ns
        self.ldr, self.ldrd = _round_up(self.TB, 8), _round_up(self.TBd, 8)
        self.X = c.i16(self.TB, ni)             # dropout_in(embed(x)) rows     [Td*B][ni]
        self.XT = c.i16(ni, self.ldr)           # ... transposed                 [ni][Td*B]
        self.hT = c.i16(H, self.ldrd)           # h_{t-1} rows, transposed       [H][Td*B*ns]
        self.dG = c.i16(self.TBd, 4 * H)        # gate pre-activation grads      [Td*B*ns][4H]
        self.dGs = c.i16(self.TB, 4 * H)        # ... summed over the samples    [Td*B][4H]
        self.hT_gen = None                      # as _LstmImages
        self.hT_ld = self.ldrd

    def forward(self, lib, s, W16, Gxw, gather):
        """Gxw[t*B + b][4u + g] = X[t*B + b] . W_ih[g*H + u][:ni] -- the word half of the input projection, no addend (the
        z-projection and the biases are added per decoder row by lv_gx_expand_add_f32)."""
        emb, ids, ids_stride, keep, kscale, T, B, V = gather
        lib.lv_embed_gather_b16(emb, ids, ids_stride, keep, kscale, T, B, self.ni, V, P(self.X), self.ni, P(self.XT), self.ldr, s)
        _gemm16(lib, s, 0, self.TB, 4 * self.H, self.ni, P(self.X), self.ni, W16, self.ni, Gxw, 4 * self.H)

    def backward(self, lib, s, dG, h_prev, WT16, dX, gW_ih, ld_gw, gW_hh, ws=None, hT_current=False):
        """Arguments as _LstmImages.backward; dG must be None: self.dG holds the BPTT's bf16 gate gradients.  dGs = sum over samples (f32 sum, one rounding); dX = dGs . W_ih[:, :ni]
        and dW_ih[:, :ni] = dGs^T . X on Td * B rows; dW_hh = dG^T . h_prev on Td * B * ns rows."""
        assert dG is None
        ni, H = self.ni, self.H
        lib.lv_sample_sum_b16(P(self.dG), 4 * H, P(self.dGs), 4 * H, self.Td, self.B, self.ns, 4 * H, s)
        wsd = ws if ws is not None else _gemm_ws(lib, s)
        if PAIR_WGRAD and lib.lv_gemm_b16_pair_supported(1, 4 * H, ni, self.TB, 0, self.TB, ni, 4 * H, wsd.numel()):
            # the two Td * B-row products in one grouped launch (single-destination first product: nsplit0 = 0)
            with _prof("gemm_bf16", 4.0 * 4 * H * ni * self.TB):
                lib.lv_gemm_b16_pair(1, 4 * H, ni, self.TB, P(self.dGs), 4 * H, P(self.XT), self.ldr, gW_ih, ld_gw, 0, None, 0,
                                     0, self.TB, ni, 4 * H, P(self.dGs), 4 * H, WT16, 4 * H, dX, ni, P(wsd), wsd.numel(), s)
        else:
            _gemm16(lib, s, 0, self.TB, ni, 4 * H, P(self.dGs), 4 * H, WT16, 4 * H, dX, ni, ws=ws)
            _gemm16(lib, s, 1, 4 * H, ni, self.TB, P(self.dGs), 4 * H, P(self.XT), self.ldr, gW_ih, ld_gw, ws=ws)
        if not hT_current:
            lib.lv_cvt_bf16_f32(h_prev, H, self.TBd, H, None, 0, P(self.hT), self.ldrd, s)
        _gemm16(lib, s, 1, 4 * H, H, self.TBd, P(self.dG), 4 * H, P(self.hT), self.ldrd, gW_hh, H, ws=ws)


def _wgrad(lib, s, M, N, K, A, lda, Bm, ldb, C, ldc, prec, ws=None):
    """Weight gradient C[M,N] = A^T . B with A stored [K][M] (lda) and B stored [K][N] (ldb).

    Both kernels read the operands as stored (TN form): each wave-level load is 256 contiguous bytes of one k-row.
    (Measured on MI355X: transposing the operands first to use the NT form is SLOWER for the bf16 kernel -- dW_pred
    1.63 ms + 0.27 ms of transposes vs ~0.9 ms as TN; profiles/r01f_*.)"""
    _gemm(lib, s, 1, 0, M, N, K, A, lda, Bm, ldb, C, ldc, prec=prec, ws=ws)


def _sorted_tokens(eng, lib, s, x, x_key, ids_stride, T_used, B, V, w):
    """(rows, tokens) of the embedding backward's stable token sort for batch x: from the engine's per-batch cache when this
    batch tensor has been seen (and not modified) before, else sorted now -- into cache-owned buffers in eager mode, into the
    workspace under hipGraph capture or when the batch has no stable identity."""
    key = x_key if x_key is not None else x
    capturing = x.device.type == "cuda" and torch.cuda.is_current_stream_capturing()
    use_cache = eng.ws_evictable and not capturing           # hipGraph trainers pin the workspaces (ws_evictable False): fixed buffers
    if use_cache:
        hit = eng._sorts.get(key, (T_used, B))
        if hit is not None:
            return hit
        srows, stok = eng.wsc.i32(T_used * B), eng.wsc.i32(T_used * B)
    else:
        srows, stok = w.srows, w.stok
    eng._aux.run(x.device, lambda sa: lib.lv_token_sort(P(x), ids_stride, T_used, B, V, P(srows), P(stok), P(w.stmp), sa if sa is not None else s),
                 keep=(x, srows, stok))
    if use_cache:
        eng._sorts.put(key, (T_used, B), srows, stok)
    return srows, stok


class LSTMEncoderEngine(object):
    """Forward/backward of LSTMEncoder.forward (reference modules/encoders/enc_lstm.py:47-64)."""

    def __init__(self, module):
        self.m = module
        self.flat = None
        self.wsc = None
        self.ws_evictable = True  # False under hipGraph capture (graphs hold pointers into the workspaces)
        self.gen = 0
        self.precision = "f32"    # precision of the large GEMMs: "f32" (parity) or "bf16" (throughput)
        self.native16 = True      # bf16 path: pre-rounded bf16 operand images (lv_gemm_b16) where the shapes allow
        self.persistent = _PERSISTENT_DEFAULT   # bf16 image path: forward recurrence as one persistent launch where supported
        self.persist_rows = None                # rows per XCD group of the persistent launches (None: B / 8; 8 at B = 32 = half the chip)
        self.persist_flags = 1                  # bit 0: hand-off granules stay in the XCD's L2 (ladder rung 0; see demote_persistent)
        self.status = None                      # device int32: a persistent launch's hand-off timeout is reported here
        self.fold = None                        # norm folding (trainer._plan_fold): {"embed": (partials tensor, norm-only flag)}
        # (sorted token list, N) of the lv_embed_scatter_full* launch that wrote the table's gradient in the last backward(): every
        # other row of that gradient is zero (the trainer's row-sparse SGD step); None when no such launch wrote it
        self.embed_rows = None
        self.cache_weight_images = False        # the encoder is stepped every inner iteration: its images are rebuilt per call
        self.wgen = 0                           # bumped by the fused trainer after a raw-pointer weight update
        # bf16 configuration only: which parts of the FORWARD run f32-accurately all the same -- "gx" (the input projection
        # X W_ih^T) and / or "rec" (the recurrence).  mu / logvar, hence z and the KL (encoder.py:55), are functions of the forward's
        # last state alone (enc_lstm.py:60-62); the weights' rounding to bf16 moves it by 2e-4..5e-4 relative (to binary16, the
        # default below: 1e-5..7e-5), the exact forward holds 2e-5 while every gradient product and the decoder stay on the bf16 pipe.
        self.exact_forward = ()
        # how: "auto" = on the bf16 pipe itself wherever the forward recurrence is a persistent launch -- split-bf16 operands for
        # the input projection and a two-pass recurrence whose second pass carries W_lo . h as part of gx (_exact_forward_split) --
        # else, and with "f32", the exact-f32 GEMM and launch-per-timestep recurrence
        self.exact_impl = "auto"
        # bf16 configuration: number format of the FORWARD's matrix-pipe operands (embedded rows, W_ih, W_hh, the h hand-off).
        # "f16" (default): IEEE binary16 -- the same instructions at the same rates with 11 instead of 8 bits of significand.  What
        # moves the forward's last state (hence mu / logvar, z and the KL of encoder.py:55) in the bf16 configuration is the
        # rounding of the WEIGHTS and embeddings, the same perturbation at every timestep (profiles/r05a_kl_ablation.txt: W_hh
        # 1.4e-4, embedding 0.4-1.9e-4, W_ih 0.2-1.2e-4 relative on the KL; the h hand-off <= 2.5e-5); these operands are bounded
        # (weights ~U(-0.01, 0.01)-ish, h in (-1, 1)), so they do not need bf16's exponent range.  The gradient products and the
        # BPTT keep bf16.  "bf16": the round-1..4 arithmetic.
        self.fwd_operands = "f16"
        self._h16_now = False
        self._wimg = None
        self._aux = _AuxStream()
        self._sorts = _TokenSortCache()

    def _quiesce_side_streams(self):
        dev = self.flat.device if self.flat is not None else None
        if dev is not None and dev.type == "cuda" and self._aux.stream is not None:
            torch.cuda.current_stream(dev).wait_stream(self._aux.stream)

    def _b16(self, B, T):
        V, ni, H, nz2 = self.dims()
        if not _LstmImages.usable(self.precision, self.native16, ni, H):
            return None
        return self.wsc.get(("b16", B, T), lambda: _LstmImages(self.wsc, T * B, ni, H, key=("b16", B, T)))

    def _exact(self, img):
        """The parts of the forward that run in exact f32 although the engine is in the bf16 configuration."""
        ex = tuple(self.exact_forward or ())
        assert all(e in ("gx", "rec") for e in ex), ex
        return ex if (img is not None and self.precision == "bf16") else ()

    def fold_parts(self, B, T):
        """Partial sums of squares this engine's backward can emit from the kernels that complete its big gradient tensors
        (name -> number of partials): the embedding table's gradient, from the scatter."""
        return {"embed": self.lib.lv_embed_scatter_sumsq_parts(T, B)}

    def refresh_weight_images(self, B, device):
        """Bring the bf16 weight images (and, where the persistent launches apply, the packed recurrent weights) up to
        date on the current stream; a no-op when caching is on and the weights have not changed."""
        V, ni, H, nz2 = self.dims()
        if not _LstmImages.usable(self.precision, self.native16, ni, H):
            return None
        self.ensure(device)
        persist = self.persistent and H == _PERSIST_H and B <= _PERSIST_MAX_B and torch.device(device).type == "cuda" and \
            torch.cuda.get_device_properties(device).multi_processor_count >= 256
        return _weight_images(self, self.lib, stream_ptr(device), device, persist)

    def ensure(self, device):
        device = torch.device(device)
        if self.flat is None or self.flat.device != device or not self.flat.bound():
            named = [("embed.weight", self.m.embed.weight), ("lstm.weight_ih_l0", self.m.lstm.weight_ih_l0),
                     ("lstm.weight_hh_l0", self.m.lstm.weight_hh_l0), ("lstm.bias_ih_l0", self.m.lstm.bias_ih_l0),
                     ("lstm.bias_hh_l0", self.m.lstm.bias_hh_l0), ("linear.weight", self.m.linear.weight)]
            self.flat = FlatBuffer(named, device)
            self.flat.flat_grads = getattr(self, "_flat_grads_pref", True)      # VAE.use_flat_grads before the buffers existed
            self.wsc = _WS(device)
            self.wsc.evictable = self.ws_evictable
            self.wsc.before_evict = self._quiesce_side_streams
            # the cached bf16 / packed weight images describe the OLD flat buffer (p.data = X, module._apply and device moves keep
            # the parameters' version counters, so weights_version() alone would not notice)
            self._wimg = None
            for p in self.flat.params:
                p._lvae_engine = self         # lets optim.clip_grad_norm_ / optim.SGD find the flat buffers from the parameters
        self.lib = backend_for(device)
        if self.status is None or self.status.device != device:
            self.status = torch.zeros(1, dtype=torch.int32, device=device)
        return self.flat

    def dims(self):
        V, ni = self.m.embed.weight.shape
        H = self.m.lstm.weight_hh_l0.shape[1]
        nz2 = self.m.linear.weight.shape[0]
        return V, ni, H, nz2

    def _ws(self, B, T):
        V, ni, H, nz2 = self.dims()
        c = self.wsc

        def build():
            w = _NS()
            w.X = c.f32(T * B, ni)
            w.Gx, w.ws_key = None, (B, T)   # _gx_buffer: only where the input projection is materialised
            # index 0 = the initial state: zero for the encoder (enc_lstm.py:60), and no kernel ever writes slot 0
            w.hs = torch.zeros(T + 1, B, H, dtype=torch.float32, device=c.device)
            w.cs = torch.zeros(T + 1, B, H, dtype=torch.float32, device=c.device)
            w.gates = c.f32(_saved_floats(self, T, B, H))
            w.mulv = c.f32(B, nz2)
            w.dmulv = c.f32(B, nz2)
            w.dG = c.f32(T * B, 4 * H)
            w.dGsum = c.f32(B, 4 * H)
            w.lstm_ws = c.f32(self.lib.lv_lstm_ws_floats(B, H))
            w.dhT = c.f32(B, H)
            w.dX = c.f32(T * B, ni)
            w.srows = c.i32(T * B)
            w.stok = c.i32(T * B)
            w.stmp = c.i32(2 * T * B)
            return w
        return c.get((B, T), build)

    def forward(self, x, head=None, x_key=None, lengths=None):
        """x int64 [B][T] on device -> mulv [B][2nz] (mu | logvar).  Keeps activations for backward().

        lengths (SeqLengths, a list of ints or an integer tensor): x is a padded batch and row b holds lengths[b]
        tokens -- mu / logvar come from the state after exactly those (enc_lstm.py:95-105).  Exact-f32 configuration only.  The
        input projection runs over the padded positions as it is; the recurrence (lv_lstm_fwd_len_f32) freezes a finished row.

        head = (eps [B][ns][nz], z, kl): also reparameterise and compute the KL in the head's launch (fused driver).
        x_key: the batch tensor x was copied from (fused driver: x is its per-shape static buffer), whose identity keys the
        cache of sorted token lists; default x itself."""
        assert x.dtype == torch.int64 and x.dim() == 2
        x = x.contiguous()
        B, T = x.shape
        steps = None
        if lengths is not None:
            _refuse_bf16_lengths(self)
            if head is not None:
                raise _lib.LvaeError("the fused head takes equal-length batches only")
            lengths = SeqLengths.of(lengths, B, T, x.device)
            steps = (lengths.enc, lengths.max)
        f = self.ensure(x.device)
        lib, s = self.lib, stream_ptr(x.device)
        V, ni, H, nz2 = self.dims()
        w = self._ws(B, T)
        v = f.views
        img = self._b16(B, T)
        exact = self._exact(img)
        self._h16_now = img is not None and not exact and self.fwd_operands == "f16"
        split = (self.exact_impl == "auto" and set(exact) == {"gx", "rec"} and _persistent_ok(self, img, B, H, x.device, _PERSIST_MAX_B))
        if img is None or ("gx" in exact and not split):
            lib.lv_embed_gather_f32(P(v["embed.weight"]), P(x), T, None, 1.0, P(w.X), T, B, ni, V, s)      # f32 rows: the exact-f32 / fallback GEMM's operand
        # the backward's token sort depends on x only: taken from the per-batch cache, or queued now (auxiliary stream)
        self._sort = _sorted_tokens(self, lib, s, x, x_key, T, T, B, V, w)
        biases = dict(add1=P(v["lstm.bias_ih_l0"]), ld1=0, mod1=1, add2=P(v["lstm.bias_hh_l0"]), ld2=0, mod2=1)
        gx_unit_major = True
        xin = None
        fuse_gx = (img is not None and not exact and steps is None and getattr(self, "gx_round", None) is None
                   and _fused_gx_ok(self, img, B, H, ni, x.device, FUSED_GX_ENC))
        if not fuse_gx:
            _gx_buffer(self.wsc, w, T * B, H)
        if split:
            self._exact_forward_split(lib, s, img, w, x, T, B, V, ni, H)
        elif img is not None and "gx" in exact:
            # exact-f32 input projection (gate-major columns, as the f32 recurrence reads them); the bf16 images of the embedded
            # rows are still gathered: the backward's dW_ih product reads them
            self.refresh_weight_images(B, x.device)
            lib.lv_embed_gather_b16(P(v["embed.weight"]), P(x), T, None, 1.0, T, B, ni, V, P(img.X), ni, P(img.XT), img.ldr, s)
            _gemm(lib, s, 0, 1, T * B, 4 * H, ni, P(w.X), ni, P(v["lstm.weight_ih_l0"]), ni, P(w.Gx), 4 * H, prec="f32", **biases)
            gx_unit_major = False
            if "rec" not in exact:          # (measurement only: the bf16 recurrences read a unit-major gx)
                if getattr(w, "Gx_gm", None) is None:
                    w.Gx_gm = self.wsc.f32(T * B, 4 * H)
                w.Gx, w.Gx_gm = w.Gx_gm, w.Gx
                lib.lv_gate_interleave_f32(P(w.Gx_gm), None, T * B, H, P(w.Gx), s)
                gx_unit_major = True
        elif img is not None:
            wi = self.refresh_weight_images(B, x.device)
            xin = img.forward(lib, s, None, P(wi.W), None if fuse_gx else P(w.Gx), P(v["lstm.bias_ih_l0"]), P(v["lstm.bias_hh_l0"]), 1,
                              self.wsc, gather=(P(v["embed.weight"]), P(x), T, None, 1.0, T, B, V), h16=self._h16_now, product=not fuse_gx)
        else:
            _gemm(lib, s, 0, 1, T * B, 4 * H, ni, P(w.X), ni, P(v["lstm.weight_ih_l0"]), ni, P(w.Gx), 4 * H,
                  prec=self.precision, **biases)
        gx_round = getattr(self, "gx_round", None)
        if gx_round is not None and not split:
            # MEASUREMENT ONLY (profiles/microbench/kl_ablation.py): what a 16-bit Gx image would cost the KL -- the f32 Gx rounded to
            # binary16 / bf16 in place before the recurrence reads it (never set by the product)
            w.Gx.copy_(w.Gx.to(torch.float16 if gx_round == "f16" else torch.bfloat16).to(torch.float32))
        if split:
            pass
        elif "rec" in exact:
            self._exact_recurrence(lib, s, img, w, gx_unit_major, T, B, H, x.device)
        else:
            with _prof("lstm_fwd_enc", float(T), 1 if _persistent_ok(self, img, B, H, x.device, _PERSIST_MAX_B) else T):
                _lstm_forward(self, lib, s, img, w, None if fuse_gx else P(w.Gx), P(v["lstm.weight_hh_l0"]), None, 1.0, None, T, B, H,
                              x.device, steps=steps, xin=xin)
        if head is not None and not fused_ends_ok(B, nz2 // 2, head[0].shape[1]):
            eps, z, kl = head
            _gemm(lib, s, 0, 1, B, nz2, H, P(w.hs, T * B * H), H, P(v["linear.weight"]), H, P(w.mulv), nz2)
            lib.lv_reparam_kl_fwd_f32(P(w.mulv), P(eps), P(z), P(kl), B, eps.shape[1], nz2 // 2, s)
        elif head is not None:
            eps, z, kl = head
            lib.lv_enc_head_fwd_f32(P(w.hs, T * B * H), P(v["linear.weight"]), P(eps), P(w.mulv), P(z), P(kl), B, H,
                                    eps.shape[1], nz2 // 2, s)
        else:
            _gemm(lib, s, 0, 1, B, nz2, H, P(w.hs, T * B * H), H, P(v["linear.weight"]), H, P(w.mulv), nz2)
        self.gen += 1
        self.last = (x, B, T, self.gen)
        self.last_steps = steps
        return w.mulv

    def _exact_forward_split(self, lib, s, img, w, x, T, B, V, ni, H):
        """The encoder's forward with f32-like WEIGHTS on the bf16 pipe (exact_forward = gx + rec where the recurrence is a
        persistent launch).  What moves the forward's last state -- hence mu / logvar, z and the KL of encoder.py:55 -- in the
        bf16 configuration is the rounding of the weights, a perturbation that acts the same way at every timestep (measured,
        profiles/r05a_kl_ablation.txt: W_hh alone 1.4e-4 relative on the KL, the embedding rows 0.4e-4..1.9e-4, W_ih 0.2e-4..1.2e-4),
        not the rounding of h_{t-1} in the hand-off (<= 2.5e-5: fresh noise at every step, which averages out).  So:
          * input projection: every operand split into hi + lo (both bf16; x = hi + lo up to 2^-17 |x|) and
            Gx = X_hi W_hi^T + X_lo W_hi^T + X_hi W_lo^T as ONE product over K = 3 ni ([X_hi | X_lo | X_hi] . [W_hi | W_hi | W_lo]^T);
          * recurrence: pass 1 = the persistent bf16 recurrence as it is -> h(1); then Gx += bf16(h(1)_{t-1}) . W_hh,lo^T for all t
            at once (one GEMM); pass 2 = the same persistent launch on the corrected Gx.  Pass 2 computes W_hi . bf16(h(2)) +
            W_lo . bf16(h(1)); against the exact W . h(2) that leaves W_lo . (h(1) - h(2)) ~ 2^-9 x 1e-3 and the hand-off rounding.
        Everything the BPTT reads (gate records, cell states, hs) is what pass 2 wrote, in the persistent kernels' own layout."""
        v = self.flat.views
        TB = T * B
        wi = self.refresh_weight_images(B, x.device)
        c = self.wsc
        if getattr(wi, "Ww", None) is None:
            wi.Ww = c.i16(4 * H, 3 * ni)           # [W_hi | W_hi | W_lo], rows unit-major
            wi.Whh_lo = c.i16(4 * H, H)            # low half of W_hh, rows unit-major (the column order of Gx)
        wih, whh = v["lstm.weight_ih_l0"], v["lstm.weight_hh_l0"]
        lib.lv_cvt_bf16_gates_f32(P(wih), wih.shape[1], H, ni, P(wi.Ww), 3 * ni, None, 0, s)
        lib.lv_cvt_bf16_gates_f32(P(wih), wih.shape[1], H, ni, P(wi.Ww, ni), 3 * ni, None, 0, s)
        lib.lv_cvt_bf16_lo_f32(P(wih), wih.shape[1], 4 * H, ni, H, None, 0, 1, 0, P(wi.Ww, 2 * ni), 3 * ni, None, 0, s)
        lib.lv_cvt_bf16_lo_f32(P(whh), H, 4 * H, H, H, None, 0, 1, 0, P(wi.Whh_lo), H, None, 0, s)
        if getattr(img, "Xw", None) is None:
            img.Xw = c.i16(TB, 3 * ni)             # [X_hi | X_lo | X_hi]
            img.h16 = c.i16(TB, H)                 # bf16(h(1)_{t-1}), rows t*B + b
            if img.key is not None:
                c.grew(img.key, TB * (3 * ni + H) * 2)
        emb = P(v["embed.weight"])
        lib.lv_embed_gather_b16(emb, P(x), T, None, 1.0, T, B, ni, V, P(img.Xw), 3 * ni, P(img.XT), img.ldr, s)      # (+ X^T for dW_ih)
        lib.lv_cvt_bf16_lo_f32(emb, ni, TB, ni, 0, P(x), T, B, V, P(img.Xw, ni), 3 * ni, None, 0, s)
        lib.lv_embed_gather_b16(emb, P(x), T, None, 1.0, T, B, ni, V, P(img.Xw, 2 * ni), 3 * ni, None, 0, s)
        if img.addend is None or img.addend.shape[0] != 1:
            img.addend = c.f32(1, 4 * H)
        lib.lv_gate_interleave_f32(P(v["lstm.bias_ih_l0"]), P(v["lstm.bias_hh_l0"]), 1, H, P(img.addend), s)
        _gemm16(lib, s, 0, TB, 4 * H, 3 * ni, P(img.Xw), 3 * ni, P(wi.Ww), 3 * ni, P(w.Gx), 4 * H, add1=P(img.addend), ld1=0, mod1=1)
        with _prof("lstm_fwd_enc", float(T), 1):
            _lstm_forward(self, lib, s, img, w, P(w.Gx), P(whh), None, 1.0, None, T, B, H, x.device)
        lib.lv_cvt_bf16_f32(P(w.hs), H, TB, H, P(img.h16), H, None, 0, s)
        _gemm16(lib, s, 0, TB, 4 * H, H, P(img.h16), H, P(wi.Whh_lo), H, P(w.Gx), 4 * H, acc=1)
        with _prof("lstm_fwd_enc", float(T), 1):
            _lstm_forward(self, lib, s, img, w, P(w.Gx), P(whh), None, 1.0, None, T, B, H, x.device)

    def _exact_recurrence(self, lib, s, img, w, gx_unit_major, T, B, H, device):
        """The forward recurrence on the exact-f32 launch-per-timestep kernels inside the bf16 configuration (exact_forward has
        "rec").  They save gates [T][B][H][4] / cs [T+1][B][H]; where the BPTT will be the persistent launch, those are copied
        into its workgroup-major record buffer (lv_lstm_persist16_import_saved) -- the same T, B, R contract as a persistent
        forward."""
        v = self.flat.views
        n = T * B * 4 * H
        if getattr(w, "gates_canon", None) is None or w.gates_canon.numel() < n:
            w.gates_canon = self.wsc.f32(n)
        fwd = lib.lv_lstm_fwd_f32_ug if gx_unit_major else lib.lv_lstm_fwd_f32
        persist_bwd = _persistent_ok(self, img, B, H, device, _PERSIST_BWD_MAX_B)
        gates = w.gates_canon if persist_bwd else w.gates
        with _prof("lstm_fwd_enc", float(T), T):
            fwd(P(w.Gx), P(v["lstm.weight_hh_l0"]), P(w.hs), P(w.cs), P(gates), None, 1.0, None, P(w.lstm_ws), T, B, H, s)
        w.saved_layout = ("canonical", T, B, 0)
        if persist_bwd:
            rows = _persist_rows(self, B)
            need = lib.lv_lstm_persist16_saved_floats(T, rows)
            if w.gates.numel() < need:
                w.gates = torch.empty(need, dtype=torch.float32, device=w.gates.device)
            lib.lv_lstm_persist16_import_saved(P(w.gates_canon), P(w.cs), P(w.gates), T, B, rows, H, s)
            w.saved_layout = ("persist16", T, B, rows)

    def backward(self, dmulv, gen=None, head=None, after_bptt=None, after_embed=None):
        """dmulv [B][2nz] -> fills self.flat.grad (all encoder parameter grads, '=' semantics).

        after_bptt: called once the BPTT recurrence has been queued (data parallel: the point where a collective can be issued
        so that it starts behind the persistent launch and runs under the weight-gradient GEMMs that follow).
        after_embed: called once the embedding gradient -- the first 41 MB of the flat gradient buffer at the Yahoo shape -- has
        been queued; the LSTM weight-gradient GEMMs follow it (data parallel: that bucket's all-reduce runs under them).

        head = (eps, dz [parts][B][ns][nz], parts, dkl [B]) instead of dmulv: the backward of reparameterise + KL runs in
        the head's launch (fused driver; dmulv is then produced into the workspace).  A fifth element "iw" selects the
        importance-weighted objective's head backward (lv_enc_head_iw_bwd_f32): the fourth is then wz [B][ns], the per-sample
        seeds of lv_loss_assemble_iw_f32, in place of the analytic-KL seed; a fifth element "dreg" followed by rs [B][ns] selects
        its doubly-reparameterised form (lv_enc_head_dreg_bwd_f32; wz and rs from lv_loss_assemble_dreg_f32; rs is read from global
        memory, so the LDS budget of fused_ends_ok is unchanged).  A fifth element that is a tensor is the free-bits gate
        [B][nz] of lv_kl_freebits_fwd_f32: the analytic-KL seed of dimension j is then dkl[b] * gate[b][j] (lv_enc_head_gated_bwd_f32,
        or lv_reparam_kl_gated_bwd_f32 in front of the GEMM sequence beyond fused_ends_ok)."""
        x, B, T, g = self.last
        if gen is not None and gen != g:
            raise _lib.LvaeError("encoder activations were overwritten by a later forward(); the HIP engine keeps "
                                 "one in-flight step per module")
        self.embed_rows = None
        f = self.flat
        lib, s = self.lib, stream_ptr(x.device)
        V, ni, H, nz2 = self.dims()
        w = self._ws(B, T)
        v, gv = f.views, f.gviews
        gate = head[4] if head is not None and len(head) == 5 and torch.is_tensor(head[4]) else None
        iw = head is not None and len(head) == 5 and gate is None and head[4] == "iw"
        rs = head[5] if head is not None and len(head) == 6 and head[4] == "dreg" else None
        if rs is not None:
            iw = True
            if not (rs.dtype == torch.float32 and rs.is_contiguous() and tuple(rs.shape) == tuple(head[3].shape)):
                raise _lib.LvaeError("estimator 'dreg': rs is a contiguous float32 tensor of wz's shape")
        if head is not None:
            head = head[:4]
        if gate is not None and not (gate.dtype == torch.float32 and gate.is_contiguous() and tuple(gate.shape) == (B, nz2 // 2)):
            raise _lib.LvaeError("free-bits gate: a contiguous float32 [%d][%d] tensor expected" % (B, nz2 // 2))
        if iw and not fused_ends_ok(B, nz2 // 2, head[0].shape[1]):
            raise _lib.LvaeError("objective 'iw' runs on the one-launch encoder head (lv_enc_head_iw_bwd_f32); B = %d, nsamples = %d, "
                                 "nz = %d is beyond its LDS budget" % (B, head[0].shape[1], nz2 // 2))
        if head is not None and not fused_ends_ok(B, nz2 // 2, head[0].shape[1]):
            eps, dz, parts, dkl = head
            assert parts == 1
            if gate is not None:
                lib.lv_reparam_kl_gated_bwd_f32(P(w.mulv), P(eps), P(dz), P(dkl), P(gate), P(w.dmulv), B, eps.shape[1], nz2 // 2, s)
            else:
                lib.lv_reparam_kl_bwd_f32(P(w.mulv), P(eps), P(dz), P(dkl), P(w.dmulv), B, eps.shape[1], nz2 // 2, s)
            _gemm(lib, s, 0, 0, B, H, nz2, P(w.dmulv), nz2, P(v["linear.weight"]), H, P(w.dhT), H)
            _gemm(lib, s, 1, 0, nz2, H, B, P(w.dmulv), nz2, P(w.hs, T * B * H), H, P(gv["linear.weight"]), H)
        elif head is not None:
            eps, dz, parts, dkl = head
            if gate is not None:
                lib.lv_enc_head_gated_bwd_f32(P(w.mulv), P(eps), P(dz), parts, P(dkl), P(gate), P(w.hs, T * B * H), P(v["linear.weight"]),
                                              P(w.dmulv), P(w.dhT), P(gv["linear.weight"]), B, H, eps.shape[1], nz2 // 2, s)
            elif rs is not None:
                lib.lv_enc_head_dreg_bwd_f32(P(w.mulv), P(eps), P(dz), parts, P(dkl), P(rs), P(w.hs, T * B * H), P(v["linear.weight"]),
                                             P(w.dmulv), P(w.dhT), P(gv["linear.weight"]), B, H, eps.shape[1], nz2 // 2, s)
            else:
                head_bwd = lib.lv_enc_head_iw_bwd_f32 if iw else lib.lv_enc_head_bwd_f32
                head_bwd(P(w.mulv), P(eps), P(dz), parts, P(dkl), P(w.hs, T * B * H), P(v["linear.weight"]), P(w.dmulv),
                         P(w.dhT), P(gv["linear.weight"]), B, H, eps.shape[1], nz2 // 2, s)
        else:
            dmulv = dmulv.contiguous()
            # head: dh_T = dmulv . W_lin ; dW_lin = dmulv^T . h_T
            _gemm(lib, s, 0, 0, B, H, nz2, P(dmulv), nz2, P(v["linear.weight"]), H, P(w.dhT), H)
            _gemm(lib, s, 1, 0, nz2, H, B, P(dmulv), nz2, P(w.hs, T * B * H), H, P(gv["linear.weight"]), H)
        img = self._b16(B, T)
        with _prof("lstm_bwd_enc", float(T), 1 if _persistent_ok(self, img, B, H, x.device, _PERSIST_BWD_MAX_B) else 2 * T):
            _lstm_backward(self, lib, s, img, w, None, P(w.dhT), None, 1.0, P(v["lstm.weight_hh_l0"]), None, None, 0, T, B, H, x.device,
                           steps=getattr(self, "last_steps", None))
        if after_bptt is not None:
            after_bptt()
        def embed_grad():
            # dX -> embedding rows (the embedding table leads the flat buffer: its gradient is the first, and largest, bucket)
            self._aux.join(x.device)                   # token sort queued by forward()
            # every row of the table's gradient is written by this launch (zeros where a token does not occur): no fill in front
            self.embed_rows = (self._sort[1], T * B)
            if self.fold and "embed" in self.fold:
                sq, only = self.fold["embed"]         # the table gradient's squares go to the clip kernel from here (no second read)
                if only:
                    self.embed_rows = None
                lib.lv_embed_scatter_full_sumsq_f32(P(w.dX), None, 1.0, P(self._sort[0]), P(self._sort[1]), T, B, P(gv["embed.weight"]), ni,
                                                    V, -1, P(sq), int(only), s)
            else:
                lib.lv_embed_scatter_full_f32(P(w.dX), None, 1.0, P(self._sort[0]), P(self._sort[1]), T, B, P(gv["embed.weight"]), ni, V, -1, s)
            if after_embed is not None:
                after_embed()
        # input-side grads: dX first, then the embedding scatter, then the two weight-gradient products
        if img is not None:
            img.backward(lib, s, None, P(w.hs), P(self._wimg.WT), P(w.dX), P(gv["lstm.weight_ih_l0"]), ni, P(gv["lstm.weight_hh_l0"]),
                         between=embed_grad)
        else:
            _gemm(lib, s, 0, 0, T * B, ni, 4 * H, P(w.dG), 4 * H, P(v["lstm.weight_ih_l0"]), ni, P(w.dX), ni, prec=self.precision)
            embed_grad()
            _wgrad(lib, s, 4 * H, ni, T * B, P(w.dG), 4 * H, P(w.X), ni, P(gv["lstm.weight_ih_l0"]), ni, self.precision)
            _wgrad(lib, s, 4 * H, H, T * B, P(w.dG), 4 * H, P(w.hs), H, P(gv["lstm.weight_hh_l0"]), H, self.precision)
        lib.lv_colsum_f32(P(w.dGsum), 4 * H, B, 4 * H, P(gv["lstm.bias_ih_l0"]), P(gv["lstm.bias_hh_l0"]), s)


class LSTMDecoderEngine(object):
    """Forward/backward of LSTMDecoder.reconstruct_error (reference modules/decoders/dec_lstm.py:66-148)."""

    def __init__(self, module):
        self.m = module
        self.flat = None
        self.wsc = None
        self.ws_evictable = True  # False under hipGraph capture (graphs hold pointers into the workspaces)
        self.gen = 0
        self.precision = "f32"    # precision of the large GEMMs: "f32" (parity) or "bf16" (throughput)
        # The BPTT chains are latency-bound (one small launch per timestep) and leave most CUs idle: the decoder's
        # weight-gradient GEMMs run on a side HIP stream underneath them (dW_pred under the decoder BPTT; dX / dW_ih /
        # dW_hh / embedding scatter under the encoder's backward).  join() orders them before anything reads the grads.
        self.overlap = None       # None = auto policy (_overlap_on); True / False force it
        self.native16 = True      # bf16 path: feed the vocabulary-sized GEMMs pre-rounded bf16 operand images (lv_gemm_b16)
        self.persistent = _PERSISTENT_DEFAULT   # bf16 image path: forward recurrence as one persistent launch where supported
        self.persist_rows = None                # rows per XCD group of the persistent launches (see LSTMEncoderEngine)
        self.persist_flags = 1
        self.status = None
        self.fold = None                        # norm folding: {"embed": (partials, only), "pred": (partials, only)}
        # The decoder is frozen for the whole aggressive inner loop (text.py:371-400 steps the encoder only): its bf16
        # weight images and packed recurrent weights are rebuilt only when weights_version() changes.
        self.cache_weight_images = True
        # bf16 image path: vocabulary projection fused with the NLL statistics, binary16 logits (lv_gemm_b16_nll)
        self.fused_nll = True
        self.wgen = 0
        self._wimg = None
        self._side = None
        self._side_ws = None
        self._pending = None
        self._aux = _AuxStream()
        self._sorts = _TokenSortCache()

    def _quiesce_side_streams(self):
        dev = self.flat.device if self.flat is not None else None
        if dev is not None and dev.type == "cuda":
            for st in (self._aux.stream, self._side):
                if st is not None:
                    torch.cuda.current_stream(dev).wait_stream(st)

    def _fork(self, device):
        """Returns a context manager that runs its body on the side stream, ordered after everything queued so far
        on the current stream (inline when overlap is off or on the test backend)."""
        import contextlib
        if not (torch.device(device).type == "cuda" and self._overlap_on()):
            return contextlib.nullcontext(), None
        if self._side is None:
            self._side = torch.cuda.Stream(device)
            self._side_ws = torch.empty(1 << 26, dtype=torch.float32, device=device)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        self._side.wait_event(ev)
        return torch.cuda.stream(self._side), self._side_ws

    def _overlap_on(self):
        if self.overlap is not None:
            return bool(self.overlap)
        # auto (measured on MI355X): on for the f32 path (-2.2 ms/step); on the bf16 path the side
        # stream is worth <= 0.1 ms in eager mode, costs 0.5 ms inside a captured hipGraph and blurs the per-kernel
        # timings the bench reports, so it stays off there
        return self.precision == "f32"

    def _mark_pending(self, device):
        if self._side is not None and torch.device(device).type == "cuda" and self._overlap_on():
            ev = torch.cuda.Event()
            ev.record(self._side)
            self._pending = ev

    def join(self):
        """Order the current stream after the side-stream gradient work of the last backward()."""
        if self._pending is not None:
            torch.cuda.current_stream().wait_event(self._pending)
            self._pending = None

    def ensure(self, device):
        device = torch.device(device)
        if self.flat is None or self.flat.device != device or not self.flat.bound():
            m = self.m
            named = [("embed.weight", m.embed.weight), ("trans_linear.weight", m.trans_linear.weight),
                     ("lstm.weight_ih_l0", m.lstm.weight_ih_l0), ("lstm.weight_hh_l0", m.lstm.weight_hh_l0),
                     ("lstm.bias_ih_l0", m.lstm.bias_ih_l0), ("lstm.bias_hh_l0", m.lstm.bias_hh_l0),
                     ("pred_linear.weight", m.pred_linear.weight)]
            self.flat = FlatBuffer(named, device)
            self.flat.flat_grads = getattr(self, "_flat_grads_pref", True)      # VAE.use_flat_grads before the buffers existed
            self.wsc = _WS(device)
            self.wsc.evictable = self.ws_evictable
            self.wsc.before_evict = self._quiesce_side_streams
            # the cached bf16 / packed weight images describe the OLD flat buffer (p.data = X, module._apply and device moves keep
            # the parameters' version counters, so weights_version() alone would not notice)
            self._wimg = None
            for p in self.flat.params:
                p._lvae_engine = self         # lets optim.clip_grad_norm_ / optim.SGD find the flat buffers from the parameters
        self.lib = backend_for(device)
        if self.status is None or self.status.device != device:
            self.status = torch.zeros(1, dtype=torch.int32, device=device)
        return self.flat

    def dims(self):
        V, ni = self.m.embed.weight.shape
        H = self.m.lstm.weight_hh_l0.shape[1]
        nz = self.m.trans_linear.weight.shape[1]
        return V, ni, H, nz

    def _ws(self, Bd, Td, ns=1):
        """Workspace of a step on Bd decoder rows; ns > 1: Bd = B * ns rows of which each ns share a sentence -- a key of its own
        ((B, ns, Td): never the buffers of an ns = 1 step on B * ns sentences), input-side buffers on the B sentence rows."""
        V, ni, H, nz = self.dims()
        c = self.wsc
        ldl = _round_up(V, 32)
        Bs = Bd // ns                      # sentence rows: the embedding gather / scatter and their token sort
        key = (Bd, Td) if ns == 1 else (Bs, ns, Td)

        def build():
            w = _DecWS()
            w.ldl = ldl
            w._alloc = lambda: c.f32(Td * Bd, ldl)
            w._grew = lambda nb: c.grew(key, nb)
            w.X = c.f32(Td * Bs, ni)
            if ns > 1:
                w.Gxw = c.f32(Td * Bs, 4 * H)          # X . W_ih[:, :ni]^T, one row per (t, sentence)
                w.dGs = c.f32(Td * Bs, 4 * H)          # gate gradients summed over a sentence's samples (f32 configuration)
                w.x_rep = torch.empty(Bd, Td + 1, dtype=torch.int64, device=c.device)     # token ids in decoder row order
                w.Zp_um = c.f32(Bd, 4 * H)             # Zp in unit-major order where the GEMM-based init produced it gate-major
            w.Zp = c.f32(Bd, 4 * H)
            w.Gx, w.ws_key = None, key      # _gx_buffer: only where the input projection is materialised
            w.hs = c.f32(Td + 1, Bd, H)
            w.cs = c.f32(Td + 1, Bd, H)
            w.gates = c.f32(_saved_floats(self, Td, Bd, H))
            w.O = c.f32(Td * Bd, H)
            w._logits = None                 # f32 logits image: allocated on first use (the fused bf16 route never needs it)
            w.lse = c.f32(Td * Bd)
            w.nll = c.f32(Td * Bd)
            w.rec = c.f32(Bd)
            w.dO = c.f32(Td * Bd, H)
            w.dG = c.f32(Td * Bd, 4 * H)
            w.dGsum = c.f32(Bd, 4 * H)
            w.lstm_ws = c.f32(self.lib.lv_lstm_ws_floats(Bd, H))
            w.dc0 = c.f32(Bd, H)
            w.dX = c.f32(Td * Bs, ni)
            w.dz = c.f32(Bd, nz)
            w.dz_parts = self.lib.lv_dec_tail_parts(H)
            w.dzp = c.f32(w.dz_parts, Bd, nz)
            w.srows = c.i32(Td * Bs)
            w.stok = c.i32(Td * Bs)
            w.stmp = c.i32(2 * Td * Bs)
            w.zero1 = torch.zeros(1, dtype=torch.float32, device=c.device)
            w.klz = torch.zeros(Bd, dtype=torch.float32, device=c.device)
            w.loss = c.f32(Bd)
            return w
        return c.get(key, build)

    def fold_parts(self, B, Td, ns=1):
        """As TextEncoderEngine.fold_parts: the embedding table's gradient from the scatter and, where the bf16 product takes the
        256 x 256 tile, dW_pred from its own epilogue (the ws size enters the tile plan, so it must be the launch's).  ns > 1: the
        scatter runs on the B sentences, dW_pred contracts over the B * ns decoder rows."""
        out = {"embed": self.lib.lv_embed_scatter_sumsq_parts(Td, B)}
        V, ni, H, nz = self.dims()
        if self._b16(B * ns, Td, ns) is not None:
            dev = self.flat.device
            on_side = torch.device(dev).type == "cuda" and self._overlap_on()
            ws_n = (1 << 26) if on_side else _gemm_ws(self.lib, stream_ptr(dev)).numel()
            n = self.lib.lv_gemm_b16_sumsq_parts(V, H, Td * B * ns, ws_n)
            if n > 0:
                out["pred"] = n
        return out

    def _b16(self, Bd, Td, ns=1):
        """bf16 images of the vocabulary-sized GEMMs' operands (throughput path), or None when the shapes do not meet
        lv_gemm_b16's 16-byte row alignment (then lv_gemm_bf16 rounds the f32 operands on the fly).  ns: see _ws."""
        V, ni, H, nz = self.dims()
        if self.precision != "bf16" or not self.native16 or H % 8 != 0:
            return None
        c = self.wsc

        def build():
            b = _NS()
            b.ldr = _round_up(Td * Bd, 8)
            b.ldv = _round_up(V, 32)
            b.O = c.i16(Td * Bd, H)           # dropout(h_t) rows      [T*B][H]
            b.OT = c.i16(H, b.ldr)            # ... transposed         [H][T*B]
            # (pred_linear.weight [V][H] and its transpose [H][V]: engine-level images, _weight_images)
            b.dl = c.i16(Td * Bd, b.ldv)      # dlogits                [T*B][V]
            # fused projection + NLL statistics (lv_gemm_b16_nll): binary16 logits image, per-piece (max, sum exp), target logit
            b.l16 = c.i16(Td * Bd, b.ldv)
            b.nparts = self.lib.lv_gemm_b16_nll_parts(V)
            b.part = c.f32(Td * Bd, 2 * b.nparts)
            b.tgt = c.f32(Td * Bd)
            return b
        return c.get(("b16", Bd, Td) if ns == 1 else ("b16", Bd // ns, ns, Td), build)

    def refresh_weight_images(self, B, device):
        """See LSTMEncoderEngine.refresh_weight_images; covers pred_linear.weight as well."""
        V, ni, H, nz = self.dims()
        use_pred = self.precision == "bf16" and self.native16 and H % 8 == 0
        use_lstm = _LstmImages.usable(self.precision, self.native16, ni, H)
        if not (use_pred or use_lstm):
            return None
        self.ensure(device)
        persist = use_lstm and self.persistent and H == _PERSIST_H and B <= _PERSIST_MAX_B and \
            torch.device(device).type == "cuda" and torch.cuda.get_device_properties(device).multi_processor_count >= 256
        return _weight_images(self, self.lib, stream_ptr(device), device, persist, lstm=use_lstm, pred=use_pred)

    def _lstm_images(self, Bd, Td, ns=1):
        V, ni, H, nz = self.dims()
        if not _LstmImages.usable(self.precision, self.native16, ni, H):
            return None
        if ns > 1:
            return self.wsc.get(("b16lstm", Bd // ns, ns, Td), lambda: _LstmImagesMS(self.wsc, Td, Bd // ns, ns, ni, H))
        return self.wsc.get(("b16lstm", Bd, Td), lambda: _LstmImages(self.wsc, Td * Bd, ni, H, key=("b16lstm", Bd, Td)))

    def forward(self, x, z, mask_in, mask_out, p_in, p_out, want_rec=True, x_key=None, lengths=None):
        """lengths (SeqLengths, a list of ints or an integer tensor): x is a padded batch, row b holds lengths[b]
        tokens and decoder row b * ns + s runs lengths[b] - 1 steps (dec_lstm.py:391-435); rec sums the token NLL over those steps
        only.  Exact-f32 configuration only.  The recurrence (lv_lstm_fwd_len_f32) leaves zero rows in the projection's input at
        the padded positions and the BPTT (lv_lstm_bwd_len_f32) ignores what the projection's backward hands it there, so the
        vocabulary projection, the softmax and the input-side products run over the padded positions unchanged.

        x int64 [B][T]; z [B][ns][nz]; masks uint8 keep-masks in the reference's batch-first layout or None (eval mode):
        mask_in [B][T-1][ni] -- one per SENTENCE, dropout_in acts before the expansion over the samples (dec_lstm.py:81-89) --,
        mask_out [B*ns][T-1][H], one per decoder row bd = b * ns + s.  Returns rec per decoder row [B*ns] (ns = 1: rec [B]; the mean
        over a sentence's rows is dec_lstm.py:146-148's value).  x_key: see LSTMEncoderEngine.forward.

        ns > 1: everything behind the input projection is the ns = 1 code on Bd = B * ns rows; the word half of the
        input projection is shared by a sentence's samples -- gather (+ dropout_in) and X . W_ih[:, :ni]^T on Td * B rows, expanded
        and joined with the per-row z-projection by lv_gx_expand_add_f32 -- and the targets are the token ids repeated into decoder
        row order (w.x_rep)."""
        assert x.dtype == torch.int64 and x.dim() == 2
        x = x.contiguous()
        B, T = x.shape
        Td = T - 1
        if z.dim() != 3 or z.shape[0] != B or z.shape[1] < 1:
            raise _lib.LvaeError("the HIP decoder path takes z of shape [B, nsamples, nz]; got %s for a batch of %d" % (tuple(z.shape), B))
        ns = int(z.shape[1])
        Bd = B * ns
        steps = None
        if lengths is not None:
            _refuse_bf16_lengths(self)
            _same_device("the length-aware decoder", x.device, z=z, mask_in=mask_in, mask_out=mask_out)
            lengths = SeqLengths.of(lengths, B, T, x.device)
            steps = (lengths.dec(ns), lengths.max - 1)
        z2 = z.reshape(Bd, -1).contiguous()
        f = self.ensure(x.device)
        lib, s = self.lib, stream_ptr(x.device)
        V, ni, H, nz = self.dims()
        w = self._ws(Bd, Td, ns)
        v = f.views
        sc_in = 1.0 / (1.0 - p_in) if mask_in is not None else 1.0
        sc_out = 1.0 / (1.0 - p_out) if mask_out is not None else 1.0
        if mask_in is not None:
            assert mask_in.dtype == torch.uint8 and tuple(mask_in.shape) == (B, Td, ni) and mask_in.is_contiguous()
        if mask_out is not None:
            assert mask_out.dtype == torch.uint8 and tuple(mask_out.shape) == (Bd, Td, H) and mask_out.is_contiguous()
        gather = (P(v["embed.weight"]), P(x), T, P(mask_in), sc_in, Td, B, V)
        img = self._lstm_images(Bd, Td, ns)
        if img is None:
            lib.lv_embed_gather_f32(P(v["embed.weight"]), P(x), T, P(mask_in), sc_in, P(w.X), Td, B, ni, V, s)
        self._sort = _sorted_tokens(self, lib, s, x, x_key, T, Td, B, V, w)      # the SENTENCES' tokens (prepare_batches' list)
        ids = x
        if ns > 1:
            lib.lv_repeat_rows_i64(P(x), P(w.x_rep), B, T, ns, s)
            ids = w.x_rep
        # c0 = z W_trans^T ; h0 = tanh(c0) (dec_lstm.py:99-101) ; Zp = z W_ih[:, ni:]^T + b_ih + b_hh, so that
        # Gx = X W_ih[:, :ni]^T + Zp[bd]   (cat((word_embed, z_)) never materialised) -- one launch
        wih = v["lstm.weight_ih_l0"]
        fused = fused_ends_ok(Bd, nz)
        if fused:
            lib.lv_dec_init_f32(P(z2), P(v["trans_linear.weight"]), P(wih), ni + nz, ni, P(v["lstm.bias_ih_l0"]),
                                P(v["lstm.bias_hh_l0"]), P(w.cs), P(w.hs), P(w.Zp), 1 if img is not None else 0, Bd, H, nz, s)
        else:
            _gemm(lib, s, 0, 1, Bd, H, nz, P(z2), nz, P(v["trans_linear.weight"]), nz, P(w.cs), H)
            lib.lv_tanh_f32(P(w.cs), P(w.hs), Bd * H, s)
            _gemm(lib, s, 0, 1, Bd, 4 * H, nz, P(z2), nz, P(wih, ni), ni + nz, P(w.Zp), 4 * H,
                  add1=P(v["lstm.bias_ih_l0"]), ld1=0, mod1=1, add2=P(v["lstm.bias_hh_l0"]), ld2=0, mod2=1)
        xin = None
        fuse_gx = (ns == 1 and img is not None and steps is None and _fused_gx_ok(self, img, Bd, H, ni, x.device, FUSED_GX_DEC)
                   and self._b16(Bd, Td, ns) is not None)
        if not fuse_gx:
            _gx_buffer(self.wsc, w, Td * Bd, H)
        if ns > 1:
            zp = w.Zp
            if img is not None and not fused:             # the image path's recurrences read Gx unit-major (4u + g)
                lib.lv_gate_interleave_f32(P(w.Zp), None, Bd, H, P(w.Zp_um), s)
                zp = w.Zp_um
            if img is not None:
                wi = self.refresh_weight_images(Bd, x.device)
                img.forward(lib, s, P(wi.W), P(w.Gxw), gather)
            else:
                _gemm(lib, s, 0, 1, Td * B, 4 * H, ni, P(w.X), ni, P(wih), ni + nz, P(w.Gxw), 4 * H, prec=self.precision)
            lib.lv_gx_expand_add_f32(P(w.Gxw), P(zp), P(w.Gx), Td, B, ns, 4 * H, s)
        elif img is not None:
            wi = self.refresh_weight_images(B, x.device)
            gxp = None if fuse_gx else P(w.Gx)
            if fused:
                xin = img.forward(lib, s, None, P(wi.W), gxp, None, None, B, self.wsc, addend_um=P(w.Zp), gather=gather, product=not fuse_gx)
            else:
                xin = img.forward(lib, s, None, P(wi.W), gxp, P(w.Zp), None, B, self.wsc, gather=gather, product=not fuse_gx)
        else:
            _gemm(lib, s, 0, 1, Td * B, 4 * H, ni, P(w.X), ni, P(wih), ni + nz, P(w.Gx), 4 * H,
                  add1=P(w.Zp), ld1=4 * H, mod1=B, prec=self.precision)
        b16 = self._b16(Bd, Td, ns)
        # persistent recurrence: dropout_out is applied while the output is converted to its bf16 images (mask loads along H)
        # instead of inside the recurrence (8 bytes per row and step: +0.3 us per timestep); same arithmetic, same bits
        late_mask = b16 is not None and _persistent_ok(self, img, Bd, H, x.device, _PERSIST_MAX_B)
        with _prof("lstm_fwd_dec", float(Td), 1 if _persistent_ok(self, img, Bd, H, x.device, _PERSIST_MAX_B) else Td):
            if late_mask:
                _lstm_forward(self, lib, s, img, w, None if fuse_gx else P(w.Gx), P(v["lstm.weight_hh_l0"]), None, 1.0, None, Td, Bd, H,
                              x.device, xin=xin)
            else:
                _lstm_forward(self, lib, s, img, w, P(w.Gx), P(v["lstm.weight_hh_l0"]), P(mask_out), sc_out, P(w.O), Td, Bd, H, x.device,
                              steps=steps)
        hs3 = HS3_CVT and late_mask and img is not None
        if hs3:
            # O, O^T (dropout_out applied) and the BPTT-side h_prev^T from ONE read of hs: backward() skips its own conversion
            lib.lv_cvt_bf16_hs3_f32(P(w.hs), H, Td, Bd, H, P(mask_out), sc_out, P(b16.O), H, P(b16.OT), b16.ldr, P(img.hT), img.hT_ld, s)
        if b16 is not None:
            if hs3:
                pass
            elif late_mask and mask_out is not None:
                lib.lv_cvt_bf16_keep_f32(P(w.hs, Bd * H), H, Td, Bd, H, P(mask_out), sc_out, P(b16.O), H, P(b16.OT), b16.ldr, s)
            elif late_mask:
                lib.lv_cvt_bf16_f32(P(w.hs, Bd * H), H, Td * Bd, H, P(b16.O), H, P(b16.OT), b16.ldr, s)
            else:
                lib.lv_cvt_bf16_f32(P(w.O), H, Td * Bd, H, P(b16.O), H, P(b16.OT), b16.ldr, s)
            wi = self.refresh_weight_images(Bd, x.device)
            if self.fused_nll:
                # logits leave the GEMM once, as binary16, with the online-softmax statistics taken in its epilogue
                with _prof("gemm_bf16", 2.0 * Td * Bd * V * H):
                    lib.lv_gemm_b16_nll(Td * Bd, V, H, P(b16.O), H, P(wi.pred), H, P(b16.l16), b16.ldv, P(ids), T, 1, Bd,
                                        P(b16.part), P(b16.tgt), s)
                lib.lv_softmax_nll_merge_f32(P(b16.part), b16.nparts, P(b16.tgt), P(w.lse), P(w.nll), Td * Bd, s)
            else:
                _gemm16(lib, s, 0, Td * Bd, V, H, P(b16.O), H, P(wi.pred), H, P(w.logits), w.ldl)
        else:
            _gemm(lib, s, 0, 1, Td * Bd, V, H, P(w.O), H, P(v["pred_linear.weight"]), H, P(w.logits), w.ldl, prec=self.precision)
        if not (b16 is not None and self.fused_nll):
            lib.lv_softmax_nll_fwd_f32(P(w.logits), w.ldl, P(ids), T, 1, P(w.lse), P(w.nll), Td, Bd, V, s)
        if steps is not None:
            lib.lv_nll_mask_len_f32(P(w.nll), P(steps[0]), steps[1], Td, Bd, s)      # the weight-0 <pad> targets (dec_lstm.py:376-378)
        if want_rec:
            # rec[bd] = sum_t nll[t][bd]  (loss assembly kernel with kl weight 0); the fused driver sums nll itself
            lib.lv_vae_loss_f32(P(w.nll), P(w.klz), P(w.zero1), P(w.loss), P(w.rec), Td, Bd, s)
        self.gen += 1
        if img is not None:
            img.hT_gen = self.gen if hs3 else None
        self.last = (x, z2, mask_in, mask_out, sc_in, sc_out, B, T, self.gen)
        self.last_ns = ns
        self.last_steps = steps
        return w.rec

    def cond_ll_supported(self, T):
        """True where lv_dec_cond_ll_f32 takes this decoder's shape with T-token sentences (H <= 128, nz <= 64)."""
        V, ni, H, nz = self.dims()
        return bool(self.lib.lv_dec_cond_ll_f32_supported(V, ni, H, nz, int(T)))

    def cond_ll(self, x, z):
        """log p(x|z) of the eval-mode decoder (no dropout) through lv_dec_cond_ll_f32: x int64 [B][T]; z [K][nz] (one grid
        shared by every sentence, never expanded) or [B][K][nz] -> [B][K].  The caller checks cond_ll_supported().  Not
        differentiable.  Every operand must live on x's device: the kernels take raw pointers, so a mismatch is refused here,
        before anything is launched."""
        device = x.device
        if z.device != device:
            raise _lib.LvaeError("cond_ll: z is on %s, x on %s" % (z.device, device))
        self.ensure(device)
        V, ni, H, nz = self.dims()
        B, T = x.shape
        if x.dtype != torch.int64 or z.dim() not in (2, 3) or z.shape[-1] != nz or (z.dim() == 3 and z.shape[0] != B):
            raise ValueError("cond_ll: x int64 [B][T] and z [K][%d] or [B][K][%d] expected, got %s %s and %s"
                             % (nz, nz, x.dtype, tuple(x.shape), tuple(z.shape)))
        x = x.contiguous()
        z = z.contiguous().float()
        K = z.shape[-2]
        z_stride = 0 if z.dim() == 2 else K * nz
        ws = torch.empty(self.lib.lv_dec_cond_ll_f32_ws_floats(V, H, nz, B, T), dtype=torch.float32, device=device)
        out = torch.empty(B, K, dtype=torch.float32, device=device)
        self.lib.lv_dec_cond_ll_f32(P(x), B, T, P(z), z_stride, K, *self._weight_ptrs(), V, ni, H, nz, P(ws), P(out),
                                    stream_ptr(device))
        return out

    def _weight_ptrs(self):
        """The decoder's seven weight pointers, in the order lv_dec_cond_ll_f32 and lv_mh_chain_prep_f32 take them."""
        v = self.flat.views
        return [P(v[k]) for k in ("embed.weight", "trans_linear.weight", "lstm.weight_ih_l0", "lstm.weight_hh_l0",
                                  "lstm.bias_ih_l0", "lstm.bias_hh_l0", "pred_linear.weight")]

    def _chain_prep(self, x):
        """The workspace of the fused chains (lv_mh_chain_f32, lv_ais_chain_f32) for the contiguous batch x, filled by
        lv_mh_chain_prep_f32: the weight images and the per-sentence input projection, once per call."""
        V, ni, H, nz = self.dims()
        B, T = x.shape
        ws = torch.empty(self.lib.lv_mh_chain_f32_ws_floats(V, H, nz, B, T), dtype=torch.float32, device=x.device)
        self.lib.lv_mh_chain_prep_f32(P(x), B, T, *self._weight_ptrs(), V, ni, H, nz, P(ws), stream_ptr(x.device))
        return ws

    @staticmethod
    def mh_default_iters_per_launch(T):
        """The largest n with n * (T - 1) <= 2048 decoder timesteps in one launch, at least 1 (a launch stays short on a
        shared device; see LSTMDecoderEngine.mh_chain)."""
        return max(1, 2048 // max(1, int(T) - 1))

    def mh_chain(self, x, z0, draw, burn_in, thin, nsamples, std, iters_per_launch=None):
        """Random-walk Metropolis-Hastings chains on p(z|x) (VAE.sample_from_posterior, reference vae.py:218-254) through
        lv_mh_chain_f32: x int64 [B][T], starting points z0 [B][C][nz] (C independent chains per sentence), burn_in +
        nsamples * thin iterations.  draw(i0, n) -> (eps [n][B][C][nz], u [n][B][C]) hands over the noise of iterations
        i0 .. i0 + n - 1.  The weight images and the per-sentence input projection are prepared once; the chain then runs in
        launches of at most iters_per_launch iterations (default: mh_default_iters_per_launch(T)) whose cut does not change
        the result.  The caller checks cond_ll_supported().  Every operand must live on x's device: a mismatch is refused
        before anything is launched.  Nothing is read back to the host.
        -> dict(samples [B][nsamples][C][nz], cur, log_joint [B][C], accepts [B][C] int32, ratios / flags [iterations][B][C])."""
        device = x.device
        if z0.device != device:
            raise _lib.LvaeError("mh_chain: z0 is on %s, x on %s" % (z0.device, device))
        self.ensure(device)
        V, ni, H, nz = self.dims()
        if x.dim() != 2 or x.dtype != torch.int64 or z0.dim() != 3 or z0.shape[0] != x.shape[0] or z0.shape[2] != nz:
            raise ValueError("mh_chain: x int64 [B][T] and z0 [B][C][%d] expected, got %s %s and %s"
                             % (nz, x.dtype, tuple(x.shape), tuple(z0.shape)))
        burn_in, thin, nsamples = int(burn_in), int(thin), int(nsamples)
        if burn_in < 0 or thin < 1 or nsamples < 1:
            raise ValueError("mh_chain: burn_in >= 0, thin >= 1, nsamples >= 1 expected")
        B, T = x.shape
        C = z0.shape[1]
        total = burn_in + nsamples * thin
        per = iters_per_launch_for("mh_chain", iters_per_launch, x)
        chunks = _prefetch_noise("mh_chain", draw, total, per, B, C, nz, device, "mh_chain: noise is on %s / %s, x on %s")
        x = x.contiguous()
        s = stream_ptr(device)
        f32 = dict(dtype=torch.float32, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        cur = z0.detach().float().contiguous().clone()
        cur_ll, accepts = torch.zeros(B, C, **f32), torch.zeros(B, C, **i32)
        samples = torch.empty(B, nsamples, C, nz, **f32)
        ratios, flags = torch.empty(total, B, C, **f32), torch.empty(total, B, C, **i32)
        ws = self._chain_prep(x)
        for i0, n, eps, u in chunks:
            self.lib.lv_mh_chain_f32(P(x), B, T, P(ws), V, H, nz, C, P(cur), P(cur_ll), P(accepts), P(eps), P(u), n, i0, burn_in,
                                     thin, nsamples, float(std), 1 if i0 == 0 else 0, P(samples), P(ratios, i0 * B * C),
                                     P(flags, i0 * B * C), s)
        return {"samples": samples, "cur": cur, "log_joint": cur_ll, "accepts": accepts, "ratios": ratios, "flags": flags,
                "iterations": total}

    def ais_chain(self, x, z0, draw, beta, std_it, mu0=None, lv0=None, iters_per_launch=None):
        """Annealed importance sampling chains (VAE.nll_ais; the contract is at the top of csrc/lv_ais.hip) through
        lv_ais_chain_f32: x int64 [B][T], starting points z0 [B][C][nz] drawn from q0 = N(mu0, diag exp(lv0)) (mu0 / lv0 [B][nz];
        both None: the prior), beta float64 [N + 1] (non-decreasing from 0 to 1; checked by the caller), std_it float32 [N].
        draw(i0, n) -> (eps [n][B][C][nz], u [n][B][C]) as for mh_chain.  Prep runs once; the chain then runs in launches of at
        most iters_per_launch iterations (default: mh_default_iters_per_launch(T)) whose cut does not change the result.  The
        caller checks ais_chain_supported().  Every operand must live on x's device: a mismatch is refused before anything is
        launched.  Nothing is read back to the host.
        -> dict(logw [B][C] float64, cur [B][C][nz], g [B][C], accepts [B][C] int32, ratios / flags / logw_trace [N][B][C])."""
        device = x.device
        _same_device("ais_chain", device, z0=z0, beta=beta, std_it=std_it, mu0=mu0, lv0=lv0)
        self.ensure(device)
        V, ni, H, nz = self.dims()
        if x.dim() != 2 or x.dtype != torch.int64 or z0.dim() != 3 or z0.shape[0] != x.shape[0] or z0.shape[2] != nz:
            raise ValueError("ais_chain: x int64 [B][T] and z0 [B][C][%d] expected, got %s %s and %s"
                             % (nz, x.dtype, tuple(x.shape), tuple(z0.shape)))
        B, T = x.shape
        C = z0.shape[1]
        total = int(std_it.numel())
        if total < 1 or beta.dim() != 1 or beta.numel() != total + 1 or beta.dtype != torch.float64 or std_it.dim() != 1:
            raise ValueError("ais_chain: beta float64 [N + 1] and std_it [N], N >= 1, expected")
        if (mu0 is None) != (lv0 is None) or (mu0 is not None and (tuple(mu0.shape) != (B, nz) or tuple(lv0.shape) != (B, nz))):
            raise ValueError("ais_chain: mu0 and lv0 [%d][%d] (or both None) expected" % (B, nz))
        per = iters_per_launch_for("ais_chain", iters_per_launch, x)
        chunks = _prefetch_noise("ais_chain", draw, total, per, B, C, nz, device)
        x = x.contiguous()
        beta, std_it = beta.contiguous(), std_it.contiguous().float()
        if mu0 is not None:
            mu0, lv0 = mu0.detach().contiguous().float(), lv0.detach().contiguous().float()
        s = stream_ptr(device)
        f32 = dict(dtype=torch.float32, device=device)
        cur = z0.detach().float().contiguous().clone()
        g, lq = torch.zeros(B, C, **f32), torch.zeros(B, C, **f32)
        logw = torch.zeros(B, C, dtype=torch.float64, device=device)
        accepts = torch.zeros(B, C, dtype=torch.int32, device=device)
        ratios, flags = torch.empty(total, B, C, **f32), torch.empty(total, B, C, dtype=torch.int32, device=device)
        trace = torch.empty(total, B, C, dtype=torch.float64, device=device)
        ws = self._chain_prep(x)
        for i0, n, eps, u in chunks:
            self.lib.lv_ais_chain_f32(P(x), B, T, P(ws), V, H, nz, C, P(cur), P(g), P(lq), P(logw), P(accepts), P(eps), P(u),
                                      P(beta, i0), P(std_it, i0), P(mu0), P(lv0), n, 1 if i0 == 0 else 0, P(ratios, i0 * B * C),
                                      P(flags, i0 * B * C), P(trace, i0 * B * C), s)
        return {"logw": logw, "cur": cur, "g": g, "accepts": accepts, "ratios": ratios, "flags": flags, "logw_trace": trace,
                "iterations": total}

    def ais_chain_supported(self, T):
        """True where lv_ais_chain_f32 takes this decoder's shape with T-token sentences."""
        V, ni, H, nz = self.dims()
        return bool(self.lib.lv_ais_chain_f32_supported(V, ni, H, nz, int(T)))

    def backward(self, drec, gen=None, partial_dz=False):
        """drec [B*ns] = dL/d rec of every decoder row -> fills self.flat.grad; returns dz [B*ns][nz] (partial_dz: the tail kernel's
        partial sums [parts][B*ns][nz] and their count instead).  ns > 1: the gate gradients are summed over a
        sentence's samples (lv_sample_sum_*: the backward of the expansion) and dX, dW_ih[:, :ni] and the embedding scatter run on
        Td * B rows with the sentence-level keep-mask and sorted token list; dW_hh and the batch-sized tail stay on B * ns rows."""
        x, z2, mask_in, mask_out, sc_in, sc_out, B, T, g = self.last
        if gen is not None and gen != g:
            raise _lib.LvaeError("decoder activations were overwritten by a later forward(); the HIP engine keeps "
                                 "one in-flight step per module")
        ns = self.last_ns
        Bd, Td = B * ns, T - 1
        f = self.flat
        lib, s = self.lib, stream_ptr(x.device)
        V, ni, H, nz = self.dims()
        w = self._ws(Bd, Td, ns)
        v, gv = f.views, f.gviews
        drec = drec.contiguous()
        if drec.numel() != Bd:
            raise _lib.LvaeError("backward takes drec per decoder row (%d values for %d samples per sentence), got %d" % (Bd, ns, drec.numel()))
        ids = x if ns == 1 else w.x_rep
        wih = v["lstm.weight_ih_l0"]
        gwih = gv["lstm.weight_ih_l0"]
        dev = x.device
        # the embedding's padding row gets no gradient: V - 1 for LSTMDecoder (padding_idx = -1), vocab['<pad>'] for
        # VarLSTMDecoder (dec_lstm.py:375)
        pad_idx = self.m.embed.padding_idx
        pad_idx = V - 1 if pad_idx is None else int(pad_idx)
        b16 = self._b16(Bd, Td, ns)
        self._bwd_dlogits(lib, s, w, b16, ids, drec, T, Td, Bd, V)
        ctx, sws = self._fork(dev)                    # side: dW_pred = dlogits^T . O (only needs dlogits and O)
        with ctx:
            if b16 is not None and self.fold and "pred" in self.fold:
                sq, only = self.fold["pred"]          # |dW_pred|^2 leaves the product's own epilogue
                gws = sws if sws is not None else _gemm_ws(lib, s)
                if lib.lv_gemm_b16_sumsq_parts(V, H, Td * Bd, gws.numel()) != sq.numel():
                    raise RuntimeError("norm folding: the plan's partial count does not match this launch's tile plan")
                with _prof("gemm_bf16", 2.0 * V * H * Td * Bd):
                    lib.lv_gemm_b16_sumsq(1, V, H, Td * Bd, P(b16.dl), b16.ldv, P(b16.OT), b16.ldr, P(gv["pred_linear.weight"]), H,
                                          P(gws), gws.numel(), P(sq), int(only), stream_ptr(dev))
            elif b16 is not None:
                _gemm16(lib, stream_ptr(dev), 1, V, H, Td * Bd, P(b16.dl), b16.ldv, P(b16.OT), b16.ldr,
                        P(gv["pred_linear.weight"]), H, ws=sws)
            else:
                _wgrad(lib, stream_ptr(dev), V, H, Td * Bd, P(w.logits), w.ldl, P(w.O), H, P(gv["pred_linear.weight"]), H,
                       self.precision, ws=sws)
        img = self._lstm_images(Bd, Td, ns)
        self._bwd_dO_bptt(lib, s, w, b16, img, mask_out, sc_out, Td, Bd, V, H, dev)
        ctx, sws = self._fork(dev)                    # side: everything that only needs dG (runs under the encoder's backward)
        with ctx:
            s2 = stream_ptr(dev)
            if img is not None:                        # (_LstmImagesMS for ns > 1: sample sum, then the Td * B-row products)
                img.backward(lib, s2, None, P(w.hs), P(self._wimg.WT), P(w.dX), P(gwih), ni + nz, P(gv["lstm.weight_hh_l0"]), ws=sws,
                             hT_current=img.hT_gen == g)
            else:
                dG = w.dG
                if ns > 1:
                    lib.lv_sample_sum_f32(P(w.dG), P(w.dGs), Td, B, ns, 4 * H, s2)
                    dG = w.dGs
                _gemm(lib, s2, 0, 0, Td * B, ni, 4 * H, P(dG), 4 * H, P(wih), ni + nz, P(w.dX), ni, prec=self.precision, ws=sws)
                _wgrad(lib, s2, 4 * H, ni, Td * B, P(dG), 4 * H, P(w.X), ni, P(gwih), ni + nz, self.precision, ws=sws)
                _wgrad(lib, s2, 4 * H, H, Td * Bd, P(w.dG), 4 * H, P(w.hs), H, P(gv["lstm.weight_hh_l0"]), H,
                       self.precision, ws=sws)
            self._aux.join(dev)                        # token sort queued by forward()
            if self.fold and "embed" in self.fold:
                sq, only = self.fold["embed"]
                lib.lv_embed_scatter_full_sumsq_f32(P(w.dX), P(mask_in), sc_in, P(self._sort[0]), P(self._sort[1]), Td, B,
                                                    P(gv["embed.weight"]), ni, V, pad_idx, P(sq), int(only), s2)
            else:
                lib.lv_embed_scatter_full_f32(P(w.dX), P(mask_in), sc_in, P(self._sort[0]), P(self._sort[1]), Td, B, P(gv["embed.weight"]), ni,
                                              V, pad_idx, s2)
        self._mark_pending(dev)
        if not fused_ends_ok(Bd, nz):
            _gemm(lib, s, 1, 0, 4 * H, nz, Bd, P(w.dGsum), 4 * H, P(z2), nz, P(gwih, ni), ni + nz)
            lib.lv_colsum_f32(P(w.dGsum), 4 * H, Bd, 4 * H, P(gv["lstm.bias_ih_l0"]), P(gv["lstm.bias_hh_l0"]), s)
            _gemm(lib, s, 0, 0, Bd, nz, 4 * H, P(w.dGsum), 4 * H, P(wih, ni), ni + nz, P(w.dz), nz)
            _gemm(lib, s, 0, 0, Bd, nz, H, P(w.dc0), H, P(v["trans_linear.weight"]), nz, P(w.dz), nz, acc=1)
            _gemm(lib, s, 1, 0, H, nz, Bd, P(w.dc0), H, P(z2), nz, P(gv["trans_linear.weight"]), nz)
            return (w.dz, 1) if partial_dz else w.dz
        # batch-sized tail in one launch (critical path: dz feeds the encoder's backward): the z-columns of dW_ih, both
        # bias gradients, dW_trans, and dz = dGsum . W_ih[:, ni:] + dc0 . W_trans
        lib.lv_dec_tail_bwd_f32(P(w.dGsum), P(w.dc0), P(z2), P(wih), ni + nz, ni, P(v["trans_linear.weight"]), P(gwih), ni + nz,
                                P(gv["trans_linear.weight"]), P(gv["lstm.bias_ih_l0"]), P(gv["lstm.bias_hh_l0"]), P(w.dzp),
                                Bd, H, nz, s)
        if partial_dz:
            return w.dzp, w.dz_parts         # the fused driver's encoder head sums the parts itself
        lib.lv_colsum_f32(P(w.dzp), Bd * nz, w.dz_parts, Bd * nz, P(w.dz), None, s)
        return w.dz

    # ---- the chain that reaches dz, shared by backward() and backward_dz() -----------------------------------------------------
    def _bwd_dlogits(self, lib, s, w, b16, ids, drec, T, Td, Bd, V):
        """dlogits = (softmax - onehot) * drec[row], in the form the route's dO product reads."""
        if b16 is not None and self.fused_nll:
            lib.lv_softmax_nll_bwd_h16(P(b16.l16), b16.ldv, P(w.lse), P(ids), T, 1, P(drec), P(b16.dl), b16.ldv, Td, Bd, V, s)
        elif b16 is not None:
            lib.lv_softmax_nll_bwd_b16(P(w.logits), w.ldl, P(w.lse), P(ids), T, 1, P(drec), P(b16.dl), b16.ldv, Td, Bd, V, s)
        else:
            lib.lv_softmax_nll_bwd_f32(P(w.logits), w.ldl, P(w.lse), P(ids), T, 1, P(drec), Td, Bd, V, s)

    def _bwd_dO_bptt(self, lib, s, w, b16, img, mask_out, sc_out, Td, Bd, V, H, dev):
        """dO = dlogits . W_pred (dropout_out backward included), then the BPTT: leaves dG (or its bf16 image), dGsum and dc0."""
        v = self.flat.views
        late_mask = _persistent_ok(self, img, Bd, H, dev, _PERSIST_BWD_MAX_B)
        if b16 is not None and late_mask and mask_out is not None:
            # dO = dlogits . W_pred with the dropout_out backward applied where the product's K pieces are summed (no pass of its own)
            gws = _gemm_ws(lib, s)
            with _prof("gemm_bf16", 2.0 * Td * Bd * H * V):
                lib.lv_gemm_b16_keep(Td * Bd, H, V, P(b16.dl), b16.ldv, P(self._wimg.predT), b16.ldv, P(w.dO), P(mask_out), sc_out, Bd,
                                     P(gws), gws.numel(), s)
        else:
            if b16 is not None:
                _gemm16(lib, s, 0, Td * Bd, H, V, P(b16.dl), b16.ldv, P(self._wimg.predT), b16.ldv, P(w.dO), H)
            else:
                _gemm(lib, s, 0, 0, Td * Bd, H, V, P(w.logits), w.ldl, P(v["pred_linear.weight"]), H, P(w.dO), H, prec=self.precision)
            if late_mask and mask_out is not None:
                lib.lv_keep_scale_f32(P(w.dO), P(mask_out), sc_out, Td, Bd, H, s)      # dropout_out backward, once, loads along H
        with _prof("lstm_bwd_dec", float(Td), 1 if late_mask else 2 * Td):
            _lstm_backward(self, lib, s, img, w, P(w.dO), None, None if late_mask else P(mask_out), 1.0 if late_mask else sc_out,
                           P(v["lstm.weight_hh_l0"]), None, P(w.dc0), 1, Td, Bd, H, dev, steps=getattr(self, "last_steps", None))

    def _bwd_tail_dz(self, lib, s, w, Bd, H, ni, nz, partial_dz):
        """dz = dGsum . W_ih[:, ni:] + dc0 . W_trans and nothing else (lv_dec_tail_dz_f32; the two products beyond its envelope)."""
        v = self.flat.views
        wih = v["lstm.weight_ih_l0"]
        if not fused_ends_ok(Bd, nz):
            _gemm(lib, s, 0, 0, Bd, nz, 4 * H, P(w.dGsum), 4 * H, P(wih, ni), ni + nz, P(w.dz), nz)
            _gemm(lib, s, 0, 0, Bd, nz, H, P(w.dc0), H, P(v["trans_linear.weight"]), nz, P(w.dz), nz, acc=1)
            return (w.dz, 1) if partial_dz else w.dz
        lib.lv_dec_tail_dz_f32(P(w.dGsum), P(w.dc0), P(wih), ni + nz, ni, P(v["trans_linear.weight"]), P(w.dzp), Bd, H, nz, s)
        if partial_dz:
            return w.dzp, w.dz_parts
        lib.lv_colsum_f32(P(w.dzp), Bd * nz, w.dz_parts, Bd * nz, P(w.dz), None, s)
        return w.dz

    def backward_dz(self, drec, gen=None, partial_dz=False):
        """backward() for a FROZEN decoder: drec [B*ns] -> dz [B*ns][nz] (partial_dz: as backward()), through the same
        launches on the chain that reaches dz -- softmax backward, dO = dlogits . W_pred, BPTT, the dz tail -- and nothing else: no
        weight-gradient product, no dX, no embedding scatter, no write to flat.grad.  In f32 dz is bit-equal to backward()'s."""
        x, z2, mask_in, mask_out, sc_in, sc_out, B, T, g = self.last
        if gen is not None and gen != g:
            raise _lib.LvaeError("decoder activations were overwritten by a later forward(); the HIP engine keeps "
                                 "one in-flight step per module")
        ns = self.last_ns
        Bd, Td = B * ns, T - 1
        lib, s = self.lib, stream_ptr(x.device)
        V, ni, H, nz = self.dims()
        w = self._ws(Bd, Td, ns)
        drec = drec.contiguous()
        if drec.numel() != Bd:
            raise _lib.LvaeError("backward_dz takes drec per decoder row (%d values for %d samples per sentence), got %d" % (Bd, ns, drec.numel()))
        b16 = self._b16(Bd, Td, ns)
        self._bwd_dlogits(lib, s, w, b16, x if ns == 1 else w.x_rep, drec, T, Td, Bd, V)
        self._bwd_dO_bptt(lib, s, w, b16, self._lstm_images(Bd, Td, ns), mask_out, sc_out, Td, Bd, V, H, x.device)
        return self._bwd_tail_dz(lib, s, w, Bd, H, ni, nz, partial_dz)

    # ---- posterior refinement (VAE.refine_posterior) ----------------------------------------------------------------
    def svi_supported(self, B, ns):
        """The refinement session's envelope: lv_dec_init_f32 / lv_dec_tail_dz_f32's LDS budget on the B * ns decoder rows."""
        return fused_ends_ok(B * ns, self.dims()[3])

    def _svi_ws(self, B, ns, Td):
        V, ni, H, nz = self.dims()
        c = self.wsc

        def build():
            sv = _NS()
            sv.Gxw = c.f32(Td * B, 4 * H)                  # X . W_ih[:, :ni]^T, one row per (t, sentence): computed once per call
            sv.z = c.f32(B * ns, nz)
            sv.kl = [c.f32(B), c.f32(B)]
            sv.klw = c.f32(1)
            sv.rowscale = c.f32(B * ns)
            return sv
        return c.get(("svi", B, ns, Td), build)

    # A frozen-decoder pass at the z in sv.z, shared by svi_refine and hmc_ais: _zpass_begin once per call, then per pass
    # _zpass_forward (leaves w.rec) and _zpass_dz (the gradient of sum_row sv.rowscale[row] * rec[row] with respect to z).
    def _zpass_begin(self, x, ns, w, sv, mask_in=None, sc_in=1.0):
        """Exact f32: the z-independent work -- embedding gather (mask_in: dropout_in's keep-mask [B][T-1][ni], savae_forward's
        training arithmetic), the word half of the input projection (sv.Gxw), the targets in decoder row order.  -> the token ids the
        per-row kernels read.  bf16: nothing (forward() repeats its own)."""
        if self.precision != "f32":
            return x
        B, T = x.shape
        Td = T - 1
        lib, s = self.lib, stream_ptr(x.device)
        V, ni, H, nz = self.dims()
        v = self.flat.views
        ids = x
        lib.lv_embed_gather_f32(P(v["embed.weight"]), P(x), T, P(mask_in), sc_in, P(w.X), Td, B, ni, V, s)
        _gemm(lib, s, 0, 1, Td * B, 4 * H, ni, P(w.X), ni, P(v["lstm.weight_ih_l0"]), ni + nz, P(sv.Gxw), 4 * H, prec=self.precision)
        if ns > 1:
            lib.lv_repeat_rows_i64(P(x), P(w.x_rep), B, T, ns, s)
            ids = w.x_rep
        _gx_buffer(self.wsc, w, Td * B * ns, H)
        self.last_steps = None                         # equal-length BPTT, whatever the last forward() was given
        return ids

    def _zpass_forward(self, x, ids, ns, w, sv, mask_out=None, sc_out=1.0):
        """mask_out: dropout_out's keep-mask [B*ns][T-1][H] (exact f32 only), as forward()'s."""
        B, T = x.shape
        V, ni, H, nz = self.dims()
        if self.precision != "f32":
            self.forward(x, sv.z.view(B, ns, nz), None, None, 0.0, 0.0)
            return
        Td, Bd = T - 1, B * ns
        lib, s = self.lib, stream_ptr(x.device)
        v = self.flat.views
        lib.lv_dec_init_f32(P(sv.z), P(v["trans_linear.weight"]), P(v["lstm.weight_ih_l0"]), ni + nz, ni, P(v["lstm.bias_ih_l0"]),
                            P(v["lstm.bias_hh_l0"]), P(w.cs), P(w.hs), P(w.Zp), 0, Bd, H, nz, s)
        lib.lv_gx_expand_add_f32(P(sv.Gxw), P(w.Zp), P(w.Gx), Td, B, ns, 4 * H, s)
        _lstm_forward(self, lib, s, None, w, P(w.Gx), P(v["lstm.weight_hh_l0"]), P(mask_out), sc_out, P(w.O), Td, Bd, H, x.device)
        _gemm(lib, s, 0, 1, Td * Bd, V, H, P(w.O), H, P(v["pred_linear.weight"]), H, P(w.logits), w.ldl, prec=self.precision)
        lib.lv_softmax_nll_fwd_f32(P(w.logits), w.ldl, P(ids), T, 1, P(w.lse), P(w.nll), Td, Bd, V, s)
        lib.lv_vae_loss_f32(P(w.nll), P(w.klz), P(w.zero1), P(w.loss), P(w.rec), Td, Bd, s)

    def _zpass_dz(self, x, ids, ns, w, sv, mask_out=None, sc_out=1.0):
        """-> (the dz tail's partial sums [parts][B*ns][nz], parts)"""
        if self.precision != "f32":
            return self.backward_dz(sv.rowscale, partial_dz=True)
        B, T = x.shape
        Td, Bd = T - 1, B * ns
        lib, s = self.lib, stream_ptr(x.device)
        V, ni, H, nz = self.dims()
        self._bwd_dlogits(lib, s, w, None, ids, sv.rowscale, T, Td, Bd, V)
        self._bwd_dO_bptt(lib, s, w, None, None, mask_out, sc_out, Td, Bd, V, H, x.device)
        return self._bwd_tail_dz(lib, s, w, Bd, H, ni, nz, True)

    def svi_refine(self, x, mulv, eps, steps, lr, momentum, clip, kl_weight):
        """`steps` SVI iterations on every sentence's phi = (mu | logvar) with this decoder frozen and in eval arithmetic (no dropout):
        x int64 [B][T], mulv [B][2nz] (the starting point; not modified), eps [B][ns][nz] (the same in every iteration).  steps + 1
        forwards, steps backwards to z.  -> dict(last [B][2nz], best [B][2nz], best_loss [B], trace, rec_trace, kl_trace
        [steps+1][B]: L_b(phi_k) and its two terms, the sample-mean reconstruction error and the analytic KL).  Nothing is read back to the host; the caller checks svi_supported().

        Exact-f32 configuration: the z-independent work -- embedding gather, the word half of the input projection, the targets in
        decoder row order -- runs once; an iteration is lv_dec_init_f32, lv_gx_expand_add_f32, the recurrence, the vocabulary
        projection + NLL, the softmax backward, dO, the BPTT, lv_dec_tail_dz_f32 and lv_svi_step_f32.  bf16: an iteration runs
        forward() as it is (step / persistent recurrences, images and all; its gather and input projection are repeated) and
        backward_dz()."""
        steps = int(steps)
        x = x.contiguous()
        B, T = x.shape
        Td = T - 1
        dev = x.device
        _same_device("svi_refine", dev, mulv=mulv, eps=eps)
        self.ensure(dev)
        nz = self.dims()[3]
        if tuple(mulv.shape) != (B, 2 * nz) or eps.dim() != 3 or eps.shape[0] != B or eps.shape[2] != nz or eps.shape[1] < 1:
            raise ValueError("svi_refine: mulv [%d][%d] and eps [%d][ns][%d] expected, got %s and %s"
                             % (B, 2 * nz, B, nz, tuple(mulv.shape), tuple(eps.shape)))
        ns = int(eps.shape[1])
        Bd = B * ns
        lib, s = self.lib, stream_ptr(dev)
        eps = eps.detach().float().contiguous()
        sv = self._svi_ws(B, ns, Td)
        f32 = dict(dtype=torch.float32, device=dev)
        phi = mulv.detach().float().contiguous().clone()
        vel = torch.zeros(B, 2 * nz, **f32)
        best = phi.clone()
        best_loss = torch.full((B,), float("inf"), **f32)
        trace = torch.empty(steps + 1, B, **f32)
        rec_trace, kl_trace = torch.empty_like(trace), torch.empty_like(trace)     # the two terms of L_b(phi_k), for the report
        sv.klw.fill_(float(kl_weight))
        sv.rowscale.fill_(1.0 / ns)
        w = self._ws(Bd, Td, ns)
        ids = self._zpass_begin(x, ns, w, sv)
        kl, kl_next = sv.kl
        lib.lv_reparam_kl_fwd_f32(P(phi), P(eps), P(sv.z), P(kl), B, ns, nz, s)
        for k in range(steps + 1):
            self._zpass_forward(x, ids, ns, w, sv)
            torch.sum(w.rec.view(B, ns), dim=1, out=rec_trace[k])
            rec_trace[k].div_(ns)
            kl_trace[k].copy_(kl)
            if k == steps:
                lib.lv_svi_step_f32(P(w.rec), None, 0, None, P(kl), P(sv.klw), float(lr), float(momentum), float(clip), P(phi), None,
                                    P(best), P(best_loss), P(trace, k * B), None, None, B, ns, nz, s)
                break
            dzp, parts = self._zpass_dz(x, ids, ns, w, sv)
            lib.lv_svi_step_f32(P(w.rec), P(dzp), parts, P(eps), P(kl), P(sv.klw), float(lr), float(momentum), float(clip), P(phi),
                                P(vel), P(best), P(best_loss), P(trace, k * B), P(sv.z), P(kl_next), B, ns, nz, s)
            kl, kl_next = kl_next, kl
        self.gen += 1                                  # the workspaces no longer hold what the last forward() left
        return {"last": phi, "best": best, "best_loss": best_loss, "trace": trace, "rec_trace": rec_trace, "kl_trace": kl_trace}

    # ---- semi-amortized training (VAE.loss_savae / trainer.SemiAmortizedTextTrainer) ---------------------------------
    def savae_supported(self, B, ns):
        """The semi-amortized step's envelope: exact f32, and the decoder's batch-sized ends (lv_dec_init_f32 / lv_dec_tail_*) on the
        largest row count it uses, the B * 2ns rows of the perturbed pair."""
        return self.precision == "f32" and fused_ends_ok(B * 2 * ns, self.dims()[3])

    def savae_forward(self, x, mulv, eps, mask_in, mask_out, p_in, p_out, steps, lr, momentum, clip, kl_weight):
        """The forward half of a semi-amortized step (contract: csrc/lv_savae.hip): `steps` refinement steps from lambda_0 = mulv
        [B][2nz] in svi_refine's session -- here with the step's dropout keep-masks (mask_in [B][T-1][ni], mask_out [B*ns][T-1][H],
        uint8, or None), the same in every pass -- recorded by lv_svi_rec_step_f32, then forward() at lambda_K, whose activations
        savae_backward starts from.  -> the step's record: rec [B] (sample mean) and kl [B] at lambda_K, lam (lambda_K), the
        [K][B][2nz] records g_rec / lam_rec, rec0 / kl0 (the two terms of L_b(lambda_0)).  Exact f32 only; nothing is read back."""
        steps = int(steps)
        x = x.contiguous()
        B, T = x.shape
        Td = T - 1
        dev = x.device
        _same_device("savae_forward", dev, mulv=mulv, eps=eps, mask_in=mask_in, mask_out=mask_out)
        self.ensure(dev)
        if self.precision != "f32":
            raise _lib.LvaeError("semi-amortized training runs in the exact-f32 configuration only")
        nz = self.dims()[3]
        if tuple(mulv.shape) != (B, 2 * nz) or eps.dim() != 3 or eps.shape[0] != B or eps.shape[2] != nz or eps.shape[1] < 1:
            raise ValueError("savae_forward: mulv [%d][%d] and eps [%d][ns][%d] expected, got %s and %s"
                             % (B, 2 * nz, B, nz, tuple(mulv.shape), tuple(eps.shape)))
        ns = int(eps.shape[1])
        Bd = B * ns
        lib, s = self.lib, stream_ptr(dev)
        eps = eps.detach().float().contiguous()
        sc_in = 1.0 / (1.0 - p_in) if mask_in is not None else 1.0
        sc_out = 1.0 / (1.0 - p_out) if mask_out is not None else 1.0
        sv = self._svi_ws(B, ns, Td)
        f32 = dict(dtype=torch.float32, device=dev)
        lam = mulv.detach().float().contiguous().clone()
        st = _NS()
        st.g_rec, st.lam_rec = torch.empty(steps, B, 2 * nz, **f32), torch.empty(steps, B, 2 * nz, **f32)
        st.klw = torch.full((1,), float(kl_weight), **f32)
        st.rec0 = st.kl0 = None
        if steps > 0:
            vel = torch.zeros(B, 2 * nz, **f32)
            sv.rowscale.fill_(1.0 / ns)
            w = self._ws(Bd, Td, ns)
            ids = self._zpass_begin(x, ns, w, sv, mask_in, sc_in)
            kl, kl_next = sv.kl
            lib.lv_reparam_kl_fwd_f32(P(lam), P(eps), P(sv.z), P(kl), B, ns, nz, s)
            for k in range(steps):
                self._zpass_forward(x, ids, ns, w, sv, mask_out, sc_out)
                if k == 0:
                    st.rec0, st.kl0 = w.rec.view(B, ns).sum(dim=1).div_(ns), kl.clone()
                dzp, parts = self._zpass_dz(x, ids, ns, w, sv, mask_out, sc_out)
                lib.lv_svi_rec_step_f32(P(dzp), parts, P(eps), P(st.klw), float(lr), float(momentum), float(clip), P(lam), P(vel),
                                        P(st.g_rec, k * B * 2 * nz), P(st.lam_rec, k * B * 2 * nz), P(sv.z), P(kl_next), B, ns, nz, s)
                kl, kl_next = kl_next, kl
        st.z, st.kl = reparam_kl_forward(lam, eps)
        rec_rows = self.forward(x, st.z, mask_in, mask_out, p_in, p_out)
        st.rec = rec_rows.view(B, ns).sum(dim=1).div_(ns)
        if steps == 0:
            st.rec0, st.kl0 = st.rec, st.kl
        st.gen = self.gen
        st.x, st.eps, st.lam, st.steps, st.ns = x, eps, lam, steps, ns
        st.masks = (mask_in, mask_out, p_in, p_out)
        st.hyper = (float(lr), float(momentum), float(clip))
        return st

    def savae_backward(self, st, seeds, fd_eps):
        """The backward half: seeds [B] = d(objective)/d loss_b.  The full backward at lambda_K, then for k = K-1 .. 0
        lv_savae_adjoint_f32, ONE forward() / backward() on the B * 2ns rows of the perturbed pair (both rows of (b, s) under
        mask_out's row (b, s)), lv_add_f32 of its weight gradients into the running sum and lv_savae_hvp_f32.  Leaves the decoder's
        gradient in flat.grad and returns the gradient with respect to lambda_0 [B][2nz] (the encoder backward's dmulv)."""
        x, eps, ns, K = st.x, st.eps, st.ns, st.steps
        B, T = x.shape
        dev = x.device
        nz = self.dims()[3]
        lib, s = self.lib, stream_ptr(dev)
        f = self.flat
        lr, mom, clip = st.hyper
        mask_in, mask_out, p_in, p_out = st.masks
        f32 = dict(dtype=torch.float32, device=dev)
        seeds = seeds.detach().float().contiguous()
        drec = (seeds / ns).repeat_interleave(ns).contiguous()
        dz = self.backward(drec, st.gen)
        self.join()
        lbar = reparam_kl_backward(st.lam, eps, dz.view(B, ns, nz), seeds * st.klw)
        if K > 0:
            total = f.grad.clone()
            vbar = torch.zeros(B, 2 * nz, **f32)
            u, scal = torch.empty(B, 2 * nz, **f32), torch.empty(3, **f32)
            zpm, seeds2 = torch.empty(B, 2 * ns, nz, **f32), torch.empty(B * 2 * ns, **f32)
            mask2 = None
            if mask_out is not None:
                m4 = mask_out.view(B, ns, T - 1, -1)
                mask2 = torch.cat((m4, m4), dim=1).reshape(B * 2 * ns, T - 1, -1).contiguous()
            for k in range(K - 1, -1, -1):
                o = k * B * 2 * nz
                lib.lv_savae_adjoint_f32(P(lbar), P(vbar), P(st.g_rec, o), P(st.lam_rec, o), P(eps), lr, mom, clip, float(fd_eps),
                                         P(u), P(scal), P(zpm), P(seeds2), B, ns, nz, s)
                self.forward(x, zpm, mask_in, mask2, p_in, p_out, want_rec=False)
                dzp, parts = self.backward(seeds2, partial_dz=True)
                self.join()
                lib.lv_add_f32(P(total), P(f.grad), P(total), f.grad.numel(), s)
                lib.lv_savae_hvp_f32(P(dzp), parts, P(eps), P(st.lam_rec, o), P(u), P(scal), P(st.klw), P(lbar), B, ns, nz, s)
            f.grad.copy_(total)
        return lbar

    def savae_step(self, x, mulv, eps, mask_in, mask_out, p_in, p_out, seeds, steps, lr, momentum, clip, fd_eps, kl_weight):
        """One semi-amortized step's decoder side: savae_forward, then savae_backward with `seeds` [B].  -> (the step's record, the
        gradient with respect to lambda_0); the decoder's gradient is in flat.grad.  A timed-out persistent launch raises."""
        st = self.savae_forward(x, mulv, eps, mask_in, mask_out, p_in, p_out, steps, lr, momentum, clip, kl_weight)
        dmulv = self.savae_backward(st, seeds, fd_eps)
        check_persistent_status(self)
        return st, dmulv

    # ---- Hamiltonian chains (VAE.nll_ais / sample_from_posterior with transition="hmc") --------------------------
    def hmc_ais(self, x, z0, draw, beta, L, step_size, adapt, mu0, lv0, keep=None, iters_per_launch=None):
        """C annealed HMC chains per sentence with this decoder frozen and in eval arithmetic (contract: csrc/lv_hmc.hip): x int64
        [B][T], z0 [B][C][nz], the other arguments and the result as hmc_chain's.  1 + N * L decoder passes for N = len(beta) - 1
        transitions, each followed by one lv_hmc_leap_f32 launch.  Exact-f32 configuration: the z-independent work runs once
        (svi_refine's), a pass is lv_dec_init_f32, lv_gx_expand_add_f32, the recurrence, the vocabulary projection + NLL, the
        softmax backward with drec = 1 per row, dO, the BPTT and lv_dec_tail_dz_f32.  bf16: forward() as it is, then backward_dz().
        The caller checks svi_supported(B, C).  Nothing is read back inside the chain; a timed-out persistent launch raises after
        it and returns nothing."""
        x = x.contiguous()
        B, T = x.shape
        dev = x.device
        _same_device("hmc_ais", dev, z0=z0, mu0=mu0, lv0=lv0)
        self.ensure(dev)
        nz = self.dims()[3]
        if z0.dim() != 3 or z0.shape[0] != B or z0.shape[2] != nz or z0.shape[1] < 1:
            raise ValueError("hmc_ais: z0 [%d][C][%d] expected, got %s" % (B, nz, tuple(z0.shape)))
        C = int(z0.shape[1])
        sv = self._svi_ws(B, C, T - 1)
        w = self._ws(B * C, T - 1, C)
        sv.rowscale.fill_(1.0)
        box = {}

        def score():
            if not box:                                # first pass: the noise has been checked, nothing was launched before it
                sv.z.copy_(z0.detach().float().reshape(B * C, nz))
                box["ids"] = self._zpass_begin(x, C, w, sv)
            self._zpass_forward(x, box["ids"], C, w, sv)
            dzp, parts = self._zpass_dz(x, box["ids"], C, w, sv)
            return w.rec, dzp, parts
        try:
            r = hmc_chain(score, sv.z.view(B, C, nz), draw, beta, L, step_size, adapt, mu0, lv0, keep,
                          self.mh_default_iters_per_launch(T) if iters_per_launch is None else iters_per_launch)
        finally:
            self.gen += 1                              # the workspaces no longer hold what the last forward() left
        check_persistent_status(self)
        return r


def fused_ends_ok(B, nz, ns=1):
    """LDS budgets of lv_head.hip (64 KB of dynamic LDS): encoder head (B*2nz + 16*(2nz + B) floats at the narrowest column
    block), decoder init / tail (B*nz + B*65 + 64*nz floats).  Beyond them the engines use the GEMM-based sequences."""
    return (B * 2 * nz + B * ns * nz + 16 * (2 * nz + B)) * 4 <= 64000 and (B * nz + B * 65 + 64 * (nz + 1)) * 4 <= 64000


def reparam_kl_forward(mulv, eps):
    """mulv [B][2nz], eps [B][ns][nz] -> z [B][ns][nz], kl [B]   (encoder.py:53-55, 71-79)."""
    lib, s = backend_for(mulv.device), stream_ptr(mulv.device)
    B, nz2 = mulv.shape
    nz = nz2 // 2
    ns = eps.shape[1]
    mulv = mulv.contiguous()
    eps = eps.contiguous()
    z = torch.empty(B, ns, nz, dtype=torch.float32, device=mulv.device)
    kl = torch.empty(B, dtype=torch.float32, device=mulv.device)
    lib.lv_reparam_kl_fwd_f32(P(mulv), P(eps), P(z), P(kl), B, ns, nz, s)
    return z, kl


def reparam_kl_backward(mulv, eps, dz, dkl):
    lib, s = backend_for(mulv.device), stream_ptr(mulv.device)
    B, nz2 = mulv.shape
    nz = nz2 // 2
    ns = eps.shape[1]
    dmulv = torch.empty_like(mulv)
    # (contiguous copies are held in locals until the launch is queued: a temporary's block may be handed out again at once)
    mulv_c, eps_c, dz_c, dkl_c = mulv.contiguous(), eps.contiguous(), dz.contiguous(), dkl.contiguous()
    lib.lv_reparam_kl_bwd_f32(P(mulv_c), P(eps_c), P(dz_c), P(dkl_c), P(dmulv), B, ns, nz, s)
    return dmulv


FREE_BITS_MODES = {"dim": 0, "batch_dim": 1, "batch": 2}


def check_free_bits(free_bits, mode):
    """(lambda, mode number) of a free-bits objective (csrc/lv_freebits.hip), or ValueError -- before anything is launched."""
    try:
        lam = float(free_bits)
    except (TypeError, ValueError):
        raise ValueError("free_bits: a number of nats per latent dimension >= 0 (or None), not %r" % (free_bits,))
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError("free_bits must be finite and >= 0, not %r" % (free_bits,))
    if mode not in FREE_BITS_MODES:
        raise ValueError("free_bits_mode: 'dim', 'batch_dim' or 'batch', not %r" % (mode,))
    return lam, FREE_BITS_MODES[mode]


def kl_freebits_forward(mulv, lam, mode, want_stat=False):
    """mulv [B][2nz] -> kl_obj [B] (the thresholded KL), gate [B][nz] of 0.0 / 1.0 (and, want_stat, the statistic that was
    compared: [B][nz] / [nz] / [1] for mode "dim" / "batch_dim" / "batch").  One launch (lv_kl_freebits_fwd_f32)."""
    lam, mode_no = check_free_bits(lam, mode)
    lib, s = backend_for(mulv.device), stream_ptr(mulv.device)
    B, nz2 = mulv.shape
    nz = nz2 // 2
    mulv_c = mulv.contiguous()
    f32 = dict(dtype=torch.float32, device=mulv.device)
    kl_obj, gate = torch.empty(B, **f32), torch.empty(B, nz, **f32)
    stat = torch.empty(((B, nz), (nz,), (1,))[mode_no], **f32) if want_stat else None
    lib.lv_kl_freebits_fwd_f32(P(mulv_c), lam, mode_no, P(kl_obj), P(gate), None if stat is None else P(stat), B, nz, s)
    return (kl_obj, gate, stat) if want_stat else (kl_obj, gate)


def reparam_kl_gated_backward(mulv, eps, dz, dkl, gate):
    """reparam_kl_backward with dkl[b] * gate[b][j] in place of dkl[b] (lv_reparam_kl_gated_bwd_f32)."""
    lib, s = backend_for(mulv.device), stream_ptr(mulv.device)
    B, nz2 = mulv.shape
    nz = nz2 // 2
    ns = eps.shape[1]
    if tuple(gate.shape) != (B, nz):
        raise ValueError("gate has shape %s; (%d, %d) expected" % (tuple(gate.shape), B, nz))
    dmulv = torch.empty_like(mulv)
    mulv_c, eps_c, dz_c, dkl_c, gate_c = mulv.contiguous(), eps.contiguous(), dz.contiguous(), dkl.contiguous(), gate.contiguous()
    lib.lv_reparam_kl_gated_bwd_f32(P(mulv_c), P(eps_c), P(dz_c), P(dkl_c), P(gate_c), P(dmulv), B, ns, nz, s)
    return dmulv


def iw_assemble(rec_s, mulv, eps, z, kl, klw, g_loss, want_logw=False, rs=None):
    """Loss assembly of the importance-weighted objective on per-sample reconstruction errors (lv_loss_assemble_iw_f32 with T = 1):
    rec_s [B][ns], mulv [B][2nz], eps / z [B][ns][nz], kl / g_loss [B], klw: device float[1] -> loss [B], rec [B] (mean over the
    samples), rowscale [B][ns] = g_loss * softmax_s(log w), wz [B][ns] = klw * rowscale, logw [B][ns] or None.
    rs: a contiguous float32 [B][ns] tensor selects the doubly-reparameterised estimator (lv_loss_assemble_dreg_f32):
    it is filled with r_s = 1 - klw * (1 - softmax_s(log w)) and wz is c'_s = klw * rowscale * r_s."""
    lib, s = backend_for(mulv.device), stream_ptr(mulv.device)
    B, ns, nz = eps.shape
    f32 = dict(dtype=torch.float32, device=mulv.device)
    t = [a.contiguous() for a in (rec_s, mulv, eps, z, kl, klw, g_loss)]      # held until the launch is queued
    loss, rec = torch.empty(B, **f32), torch.empty(B, **f32)
    rowscale, wz = torch.empty(B, ns, **f32), torch.empty(B, ns, **f32)
    logw = torch.empty(B, ns, **f32) if want_logw else None
    acc = torch.zeros(3, **f32)
    if rs is not None:
        if not (rs.dtype == torch.float32 and rs.is_contiguous() and tuple(rs.shape) == (B, ns) and rs.device == mulv.device):
            raise ValueError("rs: a contiguous float32 (%d, %d) tensor on %s expected" % (B, ns, mulv.device))
        lib.lv_loss_assemble_dreg_f32(*[P(a) for a in t], P(loss), P(rec), P(rowscale), P(wz), P(rs), P(logw) if want_logw else None,
                                      P(acc), 1, B, ns, nz, s)
        return loss, rec, rowscale, wz, logw
    lib.lv_loss_assemble_iw_f32(*[P(a) for a in t], P(loss), P(rec), P(rowscale), P(wz), P(logw) if want_logw else None, P(acc),
                                1, B, ns, nz, s)
    return loss, rec, rowscale, wz, logw


def reparam_iw_backward(mulv, eps, wz):
    """The weights' direct gradient to [mu | logvar] (lv_reparam_iw_bwd_f32); wz [B][ns] from iw_assemble."""
    lib, s = backend_for(mulv.device), stream_ptr(mulv.device)
    B, ns, nz = eps.shape
    dmulv = torch.empty_like(mulv)
    mulv_c, eps_c, wz_c = mulv.contiguous(), eps.contiguous(), wz.contiguous()
    lib.lv_reparam_iw_bwd_f32(P(mulv_c), P(eps_c), P(wz_c), P(dmulv), B, ns, nz, s)
    return dmulv


def reparam_iwdz_backward(mulv, eps, dz, wz, rs=None):
    """The complete gradient to [mu | logvar] of the importance-weighted objective from the decoder's dz [B][ns][nz]
    (lv_reparam_iwdz_bwd_f32); wz [B][ns] from iw_assemble; rs [B][ns]: its doubly-reparameterised form (wz is then c')."""
    lib, s = backend_for(mulv.device), stream_ptr(mulv.device)
    B, ns, nz = eps.shape
    dmulv = torch.empty_like(mulv)
    t = [a.contiguous() for a in (mulv, eps, dz, wz)]
    rs_c = None if rs is None else rs.contiguous()
    lib.lv_reparam_iwdz_bwd_f32(*[P(a) for a in t], None if rs_c is None else P(rs_c), P(dmulv), B, ns, nz, s)
    return dmulv


# ---- evaluation statistics (lv_eval.hip) ------------------------------------------------------------------
def gauss_logpdf(z, mu, logvar):
    """z [B][ns][nz]; mu, logvar [B][nz] or None (standard normal) -> log density [B][ns]."""
    lib, s = backend_for(z.device), stream_ptr(z.device)
    B, ns, nz = z.shape
    z = z.contiguous().float()
    out = torch.empty(B, ns, dtype=torch.float32, device=z.device)
    if mu is not None:
        mu, logvar = mu.contiguous().float(), logvar.contiguous().float()
    lib.lv_gauss_logpdf_f32(P(z), P(mu), P(logvar), P(out), B, ns, nz, s)
    return out


def logsumexp_rows(x, add=0.0):
    """x [R][C] -> log(sum_c exp(x[r][c])) + add, [R]."""
    lib, s = backend_for(x.device), stream_ptr(x.device)
    x = x.contiguous().float()
    R, C = x.shape
    out = torch.empty(R, dtype=torch.float32, device=x.device)
    lib.lv_logsumexp_rows_f32(P(x), C, R, C, float(add), P(out), s)
    return out


def grid_posterior(cond_ll, z, want_log_post=True):
    """Normalisation of log p(x|z) over a latent grid (VAE.eval_log_model_posterior / calc_model_posterior_mean): cond_ll [B][K],
    z [K][nz] (shared grid) or [B][K][nz] -> (log p(z|x) [B][K] or None, E[z|x] [B][nz])."""
    if z.device != cond_ll.device:
        raise _lib.LvaeError("grid_posterior: z is on %s, cond_ll on %s" % (z.device, cond_ll.device))
    lib, s = backend_for(cond_ll.device), stream_ptr(cond_ll.device)
    cond_ll, z = cond_ll.contiguous().float(), z.contiguous().float()
    B, K = cond_ll.shape
    nz = z.shape[-1]
    if z.dim() not in (2, 3) or z.shape[-2] != K or (z.dim() == 3 and z.shape[0] != B):
        raise ValueError("grid_posterior: z [%d][nz] or [%d][%d][nz] expected, got %s" % (K, B, K, tuple(z.shape)))
    log_post = torch.empty(B, K, dtype=torch.float32, device=cond_ll.device) if want_log_post else None
    mean = torch.empty(B, nz, dtype=torch.float32, device=cond_ll.device)
    lib.lv_grid_posterior_f32(P(cond_ll), P(z), 0 if z.dim() == 2 else K * nz, B, K, nz, P(log_post), P(mean), s)
    return log_post, mean


def _check_operands(who, anchor, device, ops, f64=(), i32=("accepts", "flag_out"), numel=None, cur_shape=None):
    """The operands of one sampler launch (None: absent), each in turn: on `device` -- that of the operand named `anchor` -- then
    contiguous and int32 (names in i32), float64 (in f64) or float32, then (numel given) numel(name) elements unless that is
    None.  The kernels take raw pointers: the first operand that fails is refused before the launch."""
    for name, t in ops.items():
        if t is None:
            continue
        if t.device != device:
            raise _lib.LvaeError("%s: %s is on %s, %s on %s" % (who, name, t.device, anchor, device))
        want = torch.int32 if name in i32 else torch.float64 if name in f64 else torch.float32
        if t.dtype != want or not t.is_contiguous():
            raise ValueError("%s: %s must be a contiguous %s tensor" % (who, name, want))
        n = None if numel is None else numel(name)
        if n is not None and t.numel() != n:
            raise ValueError("%s: %s has %d elements, %d expected for cur %s" % (who, name, t.numel(), n, cur_shape))


def mh_keep_index(it, burn_in, thin, nsamples):
    """Index of the kept sample that iteration `it` of a chain produces, or -1 (mh_keep_index of csrc/lv_cond_ll.h)."""
    if it < burn_in or (it - burn_in) % thin != 0:
        return -1
    k = (it - burn_in) // thin
    return k if k < nsamples else -1


class NoiseCursor(object):
    """The look-ahead over a per-iteration chain's noise, drawn in chunks of `per` iterations: the launch of iteration `it`
    takes u[it] and the step noise (eps, momentum) of iteration it + 1.  draw(0, n) is asked for here, the next chunk when
    it + 1 leaves the current one."""

    def __init__(self, draw, total, per):
        self.draw, self.total, self.per = draw, total, per
        self._fetch(0)

    def _fetch(self, c0):
        self.c0 = c0                                              # first iteration of the chunk (noise, u) covers
        self.noise, self.u = self.draw(c0, min(self.per, self.total - c0))

    def first(self):
        """The step noise of iteration 0, for the launch that scores the starting point."""
        return self.noise[0]

    def step(self, it):
        """-> (u[it], the step noise of iteration it + 1 or None after the last)."""
        u_it = self.u[it - self.c0]
        if it + 1 >= self.total:
            return u_it, None
        if it + 1 - self.c0 >= self.noise.shape[0]:
            self._fetch(it + 1)
        return u_it, self.noise[it + 1 - self.c0]


def mh_step(cond_ll, prop, cur, cur_ll, accepts, u, eps_next, std, samples, keep, init=False, ratio_out=None, flag_out=None):
    """One launch of lv_mh_step_f32, the propose / accept glue of VAE.sample_from_posterior (reference vae.py:218-254) for any
    decoder: cond_ll [B][C] = log p(x|prop) as eval_cond_ll returned it; prop, cur [B][C][nz], cur_ll [B][C] f32 and accepts
    [B][C] int32 are updated in place (prop becomes the next proposals eps_next * std + cur; eps_next None: left alone);
    samples [B][nsamples][C][nz] takes cur at index keep (-1: nothing stored); init: cond_ll was computed at cur -- score the
    starting point, zero the counts, write the first proposals.  Every operand on one device, contiguous, or it is refused
    before the launch."""
    device = cond_ll.device
    _check_operands("mh_step", "cond_ll", device, {"prop": prop, "cur": cur, "cur_ll": cur_ll, "accepts": accepts, "u": u,
                                                   "eps_next": eps_next, "samples": samples, "ratio_out": ratio_out,
                                                   "flag_out": flag_out})
    lib, s = backend_for(device), stream_ptr(device)
    B, C, nz = cur.shape
    rows = B * C
    cond = cond_ll.detach().contiguous().float()
    nsamples = samples.shape[1]
    if (cond.numel() != rows or tuple(prop.shape) != (B, C, nz) or cur_ll.numel() != rows or accepts.numel() != rows
            or tuple(samples.shape) != (B, nsamples, C, nz) or (u is not None and u.numel() != rows)
            or (eps_next is not None and eps_next.numel() != rows * nz)
            or (ratio_out is not None and ratio_out.numel() != rows) or (flag_out is not None and flag_out.numel() != rows)):
        raise ValueError("mh_step: operand shapes do not match cur %s" % (tuple(cur.shape),))
    lib.lv_mh_step_f32(P(cond), P(prop), P(cur), P(cur_ll), P(accepts), P(u), P(eps_next), float(std), P(samples), rows, C, nz,
                       nsamples, int(keep), 1 if init else 0, P(ratio_out), P(flag_out), s)


def ais_step(cond_ll, prop, cur, g_cur, lq_cur, logw, accepts, u, beta, eps_next, std_next, dbeta_next, mu0=None, lv0=None,
             init=False, ratio_out=None, flag_out=None, logw_out_next=None):
    """One launch of lv_ais_step_f32, the per-iteration glue of VAE.nll_ais for any decoder (contract: csrc/lv_ais.hip):
    cond_ll [B][C] = log p(x|prop) as eval_cond_ll returned it; prop, cur [B][C][nz], g_cur / lq_cur [B][C] f32, logw [B][C] f64
    and accepts [B][C] int32 are updated in place.  The launch decides this iteration at temperature `beta`, then (eps_next
    given) adds the next iteration's increment dbeta_next * g(cur) to logw, records it in logw_out_next and replaces prop by
    eps_next * std_next + cur.  init: cond_ll was computed at cur = z_0.  beta / dbeta_next are Python floats (float64).  Every
    operand on one device, contiguous, or it is refused before the launch."""
    device = cond_ll.device
    ops = {"prop": prop, "cur": cur, "g_cur": g_cur, "lq_cur": lq_cur, "logw": logw, "accepts": accepts, "u": u,
           "eps_next": eps_next, "mu0": mu0, "lv0": lv0, "ratio_out": ratio_out, "flag_out": flag_out,
           "logw_out_next": logw_out_next}
    _check_operands("ais_step", "cond_ll", device, ops, f64=("logw", "logw_out_next"))
    lib, s = backend_for(device), stream_ptr(device)
    B, C, nz = cur.shape
    rows = B * C
    cond = cond_ll.detach().contiguous().float()
    if (cond.numel() != rows or tuple(prop.shape) != (B, C, nz) or any(t.numel() != rows for t in (g_cur, lq_cur, logw, accepts))
            or (u is None and not init) or (u is not None and u.numel() != rows)
            or (eps_next is not None and eps_next.numel() != rows * nz) or (mu0 is None) != (lv0 is None)
            or (mu0 is not None and (tuple(mu0.shape) != (B, nz) or tuple(lv0.shape) != (B, nz)))
            or any(t is not None and t.numel() != rows for t in (ratio_out, flag_out, logw_out_next))):
        raise ValueError("ais_step: operand shapes do not match cur %s" % (tuple(cur.shape),))
    lib.lv_ais_step_f32(P(cond), P(prop), P(cur), P(g_cur), P(lq_cur), P(logw), P(accepts), P(u), float(beta), P(eps_next),
                        float(std_next), float(dbeta_next), P(mu0), P(lv0), rows, C, nz, 1 if init else 0, P(ratio_out),
                        P(flag_out), P(logw_out_next), s)


HMC_INIT, HMC_MID, HMC_LAST = 0, 1, 2


def hmc_leap(rec, dz, st, mode, L, u=None, mom_next=None, beta=0.0, beta_next=0.0, dbeta_next=0.0, mu0=None, lv0=None, up=1.0,
             down=1.0, eps_min=0.0, eps_max=float("inf"), dh_out=None, flag_out=None, logw_out_next=None, keep_out=None):
    """One launch of lv_hmc_leap_f32, the sampler's side of a decoder pass (contract: csrc/lv_hmc.hip).  rec [B*C] and dz
    [parts][B*C][nz] (or [B][C][nz]) are the pass at st["pos"]; st holds the chains' buffers, all updated in place: pos, mom, cur,
    d_cur [B][C][nz], k0, g_cur, lq_cur, rec_cur, eps [B][C] f32, logw [B][C] f64, accepts [B][C] int32.  mode HMC_INIT / HMC_MID /
    HMC_LAST; beta / beta_next / dbeta_next are Python floats (float64).  Every operand on one device, contiguous, of the
    stated type, or it is refused before the launch."""
    cur = st["cur"]
    device = cur.device
    B, C, nz = cur.shape
    rows = B * C
    ops = dict(st, rec=rec, dz=dz, u=u, mom_next=mom_next, mu0=mu0, lv0=lv0, dh_out=dh_out, flag_out=flag_out,
               logw_out_next=logw_out_next, keep_out=keep_out)
    numel = lambda name: (None if name == "dz" else rows * nz if name in ("pos", "mom", "cur", "d_cur", "mom_next", "keep_out")
                          else B * nz if name in ("mu0", "lv0") else rows)
    _check_operands("hmc_leap", "cur", device, ops, f64=("logw", "logw_out_next"), numel=numel, cur_shape=tuple(cur.shape))
    if dz.numel() == 0 or dz.numel() % (rows * nz) != 0 or (mu0 is None) != (lv0 is None) or (mode == HMC_LAST and u is None):
        raise ValueError("hmc_leap: operand shapes do not match cur %s" % (tuple(cur.shape),))
    lib, s = backend_for(device), stream_ptr(device)
    lib.lv_hmc_leap_f32(P(rec), P(dz), dz.numel() // (rows * nz), P(st["pos"]), P(st["mom"]), P(st["k0"]), P(cur), P(st["g_cur"]),
                        P(st["lq_cur"]), P(st["rec_cur"]), P(st["d_cur"]), P(st["logw"]), P(st["accepts"]), P(st["eps"]), P(u),
                        P(mom_next), float(beta), float(beta_next), float(dbeta_next), P(mu0), P(lv0), rows, C, nz, int(L), int(mode),
                        float(up), float(down), float(eps_min), float(eps_max), P(dh_out), P(flag_out), P(logw_out_next),
                        P(keep_out), s)


def hmc_chain(score, pos, draw, beta, L, step_size, adapt, mu0, lv0, keep=None, iters_per_launch=64):
    """The loop of the contract (csrc/lv_hmc.hip) around any scorer.  pos [B][C][nz] float32 is the buffer the scorer reads its z
    from: score() -> (rec [B*C], dz [parts][B*C][nz], parts) at the current pos -- the first call also puts z_0 there -- and the
    launches rewrite it in place.  draw(i0, n) -> (mom [n][B][C][nz], u [n][B][C]) hands over the noise of transitions i0 ..
    i0 + n - 1, asked for in chunks of iters_per_launch; beta: N + 1 Python floats; L leapfrog steps per transition; step_size:
    every chain's starting eps; adapt: None (eps fixed) or (up, down, eps_min, eps_max[, until]) -- adapted after each of the
    first `until` transitions (default: all); mu0 / lv0 [B][nz] or None (q0 = the prior); keep: None or (burn_in, thin,
    nsamples) -- cur after transition burn_in + k * thin is sample k.  1 + N * L calls of score(), one lv_hmc_leap_f32 launch
    after each, nothing read back.
    -> dict(logw [B][C] f64, cur [B][C][nz], g, lq, step_size [B][C], accepts [B][C] int32, ratios (dH) / flags / logw_trace
    [N][B][C], samples [B][nsamples][C][nz] or None)."""
    dev = pos.device
    B, C, nz = pos.shape
    N, L, per = len(beta) - 1, int(L), int(iters_per_launch)
    if N < 1 or L < 1 or per < 1:
        raise ValueError("hmc_chain: at least one transition, leapfrog >= 1 and iters_per_launch >= 1 expected")
    f32, i32, f64 = (dict(dtype=t, device=dev) for t in (torch.float32, torch.int32, torch.float64))
    st = {"pos": pos, "mom": torch.zeros(B, C, nz, **f32), "cur": torch.zeros(B, C, nz, **f32), "d_cur": torch.zeros(B, C, nz, **f32)}
    for k in ("k0", "g_cur", "lq_cur", "rec_cur"):
        st[k] = torch.zeros(B, C, **f32)
    st["eps"] = torch.full((B, C), float(step_size), **f32)
    st["logw"], st["accepts"] = torch.zeros(B, C, **f64), torch.zeros(B, C, **i32)
    ratios, flags, trace = torch.empty(N, B, C, **f32), torch.empty(N, B, C, **i32), torch.empty(N, B, C, **f64)
    kept = None
    if keep is not None:
        burn_in, thin, nsamples = keep
        kept = torch.empty(nsamples, B, C, nz, **f32)
    fixed = dict(up=1.0, down=1.0, eps_min=0.0, eps_max=float("inf"))
    tuned, until = fixed, 0
    if adapt is not None:
        tuned = dict(up=adapt[0], down=adapt[1], eps_min=adapt[2], eps_max=adapt[3])
        until = N if len(adapt) < 5 else int(adapt[4])

    def chunk(c0, n):
        m, u = draw(c0, n)
        _same_device("hmc_chain", dev, mom=m, u=u)
        return m.float().contiguous(), u.float().contiguous()
    noise = NoiseCursor(chunk, N, per)
    rec, dz, _ = score()
    hmc_leap(rec, dz, st, HMC_INIT, L, mom_next=noise.first(), beta_next=beta[1], dbeta_next=beta[1] - beta[0], mu0=mu0, lv0=lv0,
             logw_out_next=trace[0])
    for it in range(N):                                           # transition it + 1 of the contract, at beta[it + 1]
        for _ in range(L - 1):
            rec, dz, _ = score()
            hmc_leap(rec, dz, st, HMC_MID, L, beta=beta[it + 1], mu0=mu0, lv0=lv0)
        rec, dz, _ = score()
        u_it, mom_next = noise.step(it)
        more = it + 1 < N
        k = -1 if keep is None else mh_keep_index(it, burn_in, thin, nsamples)
        hmc_leap(rec, dz, st, HMC_LAST, L, u=u_it, mom_next=mom_next, beta=beta[it + 1],
                 beta_next=beta[it + 2] if more else 0.0, dbeta_next=beta[it + 2] - beta[it + 1] if more else 0.0, mu0=mu0, lv0=lv0,
                 dh_out=ratios[it], flag_out=flags[it], logw_out_next=trace[it + 1] if more else None,
                 keep_out=kept[k] if k >= 0 else None, **(tuned if it < until else fixed))
    return {"logw": st["logw"], "cur": st["cur"], "g": st["g_cur"], "lq": st["lq_cur"], "step_size": st["eps"],
            "accepts": st["accepts"], "ratios": ratios, "flags": flags, "logw_trace": trace,
            "samples": None if kept is None else kept.permute(1, 0, 2, 3).contiguous()}


def calc_mi(mu, logvar, z):
    """mu, logvar [Bx][nz], z [Bz][nz] -> device tensor (MI, E log q(z|x), E log q(z))."""
    lib, s = backend_for(mu.device), stream_ptr(mu.device)
    mu, logvar, z = mu.contiguous().float(), logvar.contiguous().float(), z.contiguous().float()
    Bx, nz = mu.shape
    Bz = z.shape[0]
    ws = torch.empty(Bz, dtype=torch.float32, device=mu.device)
    out = torch.empty(3, dtype=torch.float32, device=mu.device)
    lib.lv_calc_mi_f32(P(mu), P(logvar), P(z), P(ws), P(out), Bx, Bz, nz, s)
    return out


def au_accumulate(mu, mean, acc):
    """acc[k] += sum_b mu[b][k] (mean None) or sum_b (mu[b][k] - mean[k])^2."""
    lib, s = backend_for(mu.device), stream_ptr(mu.device)
    mu = mu.contiguous().float()
    lib.lv_au_accum_f32(P(mu), P(mean), P(acc), mu.shape[0], mu.shape[1], s)


# ---- generation -------------------------------------------------------------------------------------------
def sampling_filter(temperature=1.0, top_k=0, top_p=1.0):
    """The arguments of a tempered / truncated draw as the kernels take them: (inv_temp, top_k, top_p, neutral) with
    inv_temp = float32(1 / temperature).  `neutral`: the draw is the plain one (temperature 1, no top-k, no top-p).
    ValueError: temperature not finite or <= 0 (or 1 / temperature not a finite positive float32), top_k not an integer or
    negative, top_p outside (0, 1]."""
    try:
        t = float(temperature)
    except (TypeError, ValueError):
        raise ValueError("temperature must be a positive finite number, got %r" % (temperature,))
    if not (math.isfinite(t) and t > 0.0):
        raise ValueError("temperature must be a positive finite number, got %r" % (temperature,))
    with np.errstate(over="ignore", under="ignore"):
        inv_temp = float(np.float32(1.0 / t))
    if not (math.isfinite(inv_temp) and inv_temp > 0.0):
        raise ValueError("1 / temperature is not a positive finite float32 for temperature %r" % (temperature,))
    if isinstance(top_k, bool) or not isinstance(top_k, numbers.Integral) or int(top_k) < 0 or int(top_k) > 0x7fffffff:
        raise ValueError("top_k must be a non-negative integer (0: off), got %r" % (top_k,))
    try:
        p = float(top_p)
    except (TypeError, ValueError):
        raise ValueError("top_p must lie in (0, 1], got %r" % (top_p,))
    p32 = float(np.float32(p))
    if not (0.0 < p <= 1.0 and 0.0 < p32 <= 1.0):
        raise ValueError("top_p must lie in (0, 1], got %r" % (top_p,))
    return inv_temp, int(top_k), p32, (inv_temp == 1.0 and int(top_k) == 0 and p32 == 1.0)


class LSTMDecodeStepper(object):
    """One decoder timestep at a time for greedy / sample / beam decoding (reference modules/decoders/dec_lstm.py:163-367):
    embed(token) ++ z -> LSTM cell -> pred_linear, through the same C-ABI kernels as the training path in exact f32
    (lv_embed_gather_f32, lv_gemm_f32 with the z-projection folded into its epilogue, lv_lstm_fwd_f32 with T = 1)."""

    def __init__(self, eng, device):
        self.eng = eng
        self.device = torch.device(device)
        eng.ensure(self.device)
        self.lib = eng.lib
        self.ws = {}

    def _refresh(self):
        """The decoder's parameters may have been rebound since this stepper was built (p.data = X, a dtype round trip): bring
        the flat copy up to date before reading it."""
        self.eng.ensure(self.device)
        self.lib = self.eng.lib

    def _w(self, n):
        w = self.ws.get(n)
        if w is None:
            V, ni, H, nz = self.eng.dims()
            d = self.device
            w = _NS()
            w.X = torch.empty(n, ni, dtype=torch.float32, device=d)
            w.Zp = torch.empty(n, 4 * H, dtype=torch.float32, device=d)
            w.Gx = torch.empty(n, 4 * H, dtype=torch.float32, device=d)
            w.hs = torch.empty(2, n, H, dtype=torch.float32, device=d)
            w.cs = torch.empty(2, n, H, dtype=torch.float32, device=d)
            w.gates = torch.empty(n, 4 * H, dtype=torch.float32, device=d)
            w.lstm_ws = torch.empty(self.lib.lv_lstm_ws_floats(n, H), dtype=torch.float32, device=d)
            w.ldl = _round_up(V, 32)
            w.logits = torch.empty(n, w.ldl, dtype=torch.float32, device=d)
            self.ws[n] = w
        return w

    def init_state(self, z2):
        """z2 [n][nz] -> (h0, c0) [n][H]: c0 = trans_linear(z), h0 = tanh(c0)   (dec_lstm.py:181-182, 284-285)."""
        self._refresh()
        V, ni, H, nz = self.eng.dims()
        v = self.eng.flat.views
        lib, s = self.lib, stream_ptr(self.device)
        n = z2.shape[0]
        z2 = z2.contiguous().float()
        c0 = torch.empty(n, H, dtype=torch.float32, device=self.device)
        _gemm(lib, s, 0, 1, n, H, nz, P(z2), nz, P(v["trans_linear.weight"]), nz, P(c0), H)
        h0 = torch.empty_like(c0)
        lib.lv_tanh_f32(P(c0), P(h0), n * H, s)
        return h0, c0

    def step(self, tokens, z2, h, c):
        """tokens int64 [n], z2 [n][nz], (h, c) [n][H] -> logits [n][V] (a view, valid until the next call), (h', c')."""
        self._refresh()
        V, ni, H, nz = self.eng.dims()
        v = self.eng.flat.views
        lib, s = self.lib, stream_ptr(self.device)
        n = tokens.shape[0]
        w = self._w(n)
        tok = tokens.reshape(n, 1).contiguous()
        z2 = z2.contiguous().float()
        lib.lv_embed_gather_f32(P(v["embed.weight"]), P(tok), 1, None, 1.0, P(w.X), 1, n, ni, V, s)
        wih = v["lstm.weight_ih_l0"]
        _gemm(lib, s, 0, 1, n, 4 * H, nz, P(z2), nz, P(wih, ni), ni + nz, P(w.Zp), 4 * H,
              add1=P(v["lstm.bias_ih_l0"]), ld1=0, mod1=1, add2=P(v["lstm.bias_hh_l0"]), ld2=0, mod2=1)
        _gemm(lib, s, 0, 1, n, 4 * H, ni, P(w.X), ni, P(wih), ni + nz, P(w.Gx), 4 * H, add1=P(w.Zp), ld1=4 * H, mod1=n)
        w.hs[0].copy_(h)
        w.cs[0].copy_(c)
        lib.lv_lstm_fwd_f32(P(w.Gx), P(v["lstm.weight_hh_l0"]), P(w.hs), P(w.cs), P(w.gates), None, 1.0, None, P(w.lstm_ws), 1, n, H, s)
        _gemm(lib, s, 0, 1, n, V, H, P(w.hs, n * H), H, P(v["pred_linear.weight"]), H, P(w.logits), w.ldl)
        return w.logits[:, :V], w.hs[1].clone(), w.cs[1].clone()

    def argmax(self, logits):
        n, V = logits.shape
        idx = torch.empty(n, dtype=torch.int64, device=self.device)
        self.lib.lv_argmax_rows_f32(P(logits), logits.stride(0), n, V, P(idx), stream_ptr(self.device))
        return idx

    def sample(self, logits, u):
        n, V = logits.shape
        idx = torch.empty(n, dtype=torch.int64, device=self.device)
        u = u.contiguous().float()
        self.lib.lv_sample_rows_f32(P(logits), logits.stride(0), n, V, P(u), P(idx), stream_ptr(self.device))
        return idx

    def sample_filtered(self, logits, u, temperature=1.0, top_k=0, top_p=1.0):
        """The draw of `sample` at a temperature, from the top_k most likely words (0: all) cut to the nucleus top_p (1: all):
        lv_sample_filtered_rows_f32.  -> (idx int64 [n], lp f32 [n]: the model's log-probability of the pick at temperature 1,
        lq f32 [n]: its log-probability under the distribution drawn from).  Rows of `logits` must be 16-byte aligned."""
        inv_temp, top_k, top_p, _ = sampling_filter(temperature, top_k, top_p)
        n, V = logits.shape
        idx = torch.empty(n, dtype=torch.int64, device=self.device)
        lp = torch.empty(n, dtype=torch.float32, device=self.device)
        lq = torch.empty(n, dtype=torch.float32, device=self.device)
        u = u.contiguous().float()
        self.lib.lv_sample_filtered_rows_f32(P(logits), logits.stride(0), n, V, P(u), inv_temp, top_k, top_p, P(idx), P(lp), P(lq),
                                             None, None, None, stream_ptr(self.device))
        return idx, lp, lq

    def log_softmax(self, logits, addrow=None):
        n, V = logits.shape
        out = torch.empty(n, V, dtype=torch.float32, device=self.device)
        if addrow is not None:
            addrow = addrow.contiguous().float()
        self.lib.lv_log_softmax_rows_f32(P(logits), logits.stride(0), n, V, P(addrow), P(out), V, stream_ptr(self.device))
        return out


class LSTMBeamSearcher(object):
    """Beam search for all sentences of a batch together, every per-step decision on the device (lv_beam.hip; reference
    modules/decoders/dec_lstm.py:163-268, which decodes sentence by sentence and decides on the host).

    B sentences x K slots are B * K rows of LSTMDecodeStepper's exact-f32 launch sequence (embedding gather, input product
    with the z-projection as its addend, the T = 1 cell, the vocabulary product); the cell reads half 0 of the (h, c) workspace
    and writes half 1, lv_beam_advance_f32 gathers the survivors' rows back into half 0 -- no clone() / copy_() per step.  The
    z-projection (+ biases) of a row never changes, so it is computed once per call.  Dead slots compute on whatever finite
    state they last held; their score of -inf keeps them out of every selection.  No host read inside a step: the host reads
    the one-int active counter every `poll` steps and stops queueing when it is zero; steps queued past that point are
    no-ops by the kernels' `active` gate, so the result does not depend on `poll`."""

    TMAX = 100                                                       # the reference's `t < 100`

    def __init__(self, stepper, poll=8):
        self.st = stepper
        self.device = stepper.device
        self.poll = poll
        self.ws = {}

    def supported(self, B, K):
        V = self.st.eng.dims()[0]
        return B > 0 and K > 0 and bool(self.st.lib.lv_beam_supported(B, K, V))

    def _w(self, B, K):
        w = self.ws.get((B, K))
        if w is None:
            V, ni, H, nz = self.st.eng.dims()
            d, T, n = self.device, self.TMAX, B * K
            w = _NS()
            w.tok = torch.empty(n, dtype=torch.int64, device=d)
            w.score = torch.empty(n, dtype=torch.float32, device=d)
            w.meta = torch.empty(B, 4, dtype=torch.int32, device=d)
            w.done_score = torch.empty(n, dtype=torch.float32, device=d)
            w.done_ref = torch.zeros(n, 2, dtype=torch.int32, device=d)
            w.trace = torch.zeros(T, n, 3, dtype=torch.int32, device=d)
            w.margin = torch.empty(B, dtype=torch.float32, device=d)
            w.counter = torch.empty(1, dtype=torch.int32, device=d)
            w.part = torch.empty(self.st.lib.lv_beam_ws_floats(B, K, V), dtype=torch.float32, device=d)
            w.pick_score = torch.empty(B, K + 1, dtype=torch.float32, device=d)
            w.pick_flat = torch.empty(B, K + 1, dtype=torch.int32, device=d)
            w.ids = torch.empty(B, T + 1, dtype=torch.int64, device=d)
            w.len = torch.empty(B, dtype=torch.int32, device=d)
            w.win = torch.empty(B, dtype=torch.float32, device=d)
            self.ws[(B, K)] = w
        return w

    def search(self, z2, K, start_tok, end_tok):
        """z2 [B][nz] -> (ids: list of B int lists with <s> in front, info: dict of numpy arrays score / steps / n_completed /
        min_margin, one entry per sentence)."""
        st = self.st
        B = z2.shape[0]
        h0, c0 = st.init_state(z2)                                   # refreshes the stepper's view of the parameters
        V, ni, H, nz = st.eng.dims()
        v = st.eng.flat.views
        lib, s = st.lib, stream_ptr(self.device)
        n, T = B * K, self.TMAX
        w, sw = self._w(B, K), st._w(B * K)
        lib.lv_beam_init_f32(P(h0), P(c0), P(sw.hs), P(sw.cs), P(w.tok), P(w.score), P(w.meta), P(w.done_score), P(w.margin),
                             P(w.counter), B, K, H, V, start_tok, s)
        zr = z2.contiguous().float().repeat_interleave(K, dim=0)
        wih = v["lstm.weight_ih_l0"]
        _gemm(lib, s, 0, 1, n, 4 * H, nz, P(zr), nz, P(wih, ni), ni + nz, P(sw.Zp), 4 * H,
              add1=P(v["lstm.bias_ih_l0"]), ld1=0, mod1=1, add2=P(v["lstm.bias_hh_l0"]), ld2=0, mod2=1)
        poll = max(1, int(self.poll))
        for t in range(T):
            lib.lv_embed_gather_f32(P(v["embed.weight"]), P(w.tok), 1, None, 1.0, P(sw.X), 1, n, ni, V, s)
            _gemm(lib, s, 0, 1, n, 4 * H, ni, P(sw.X), ni, P(wih), ni + nz, P(sw.Gx), 4 * H, add1=P(sw.Zp), ld1=4 * H, mod1=n)
            lib.lv_lstm_fwd_f32(P(sw.Gx), P(v["lstm.weight_hh_l0"]), P(sw.hs), P(sw.cs), P(sw.gates), None, 1.0, None,
                                P(sw.lstm_ws), 1, n, H, s)
            _gemm(lib, s, 0, 1, n, V, H, P(sw.hs, n * H), H, P(v["pred_linear.weight"]), H, P(sw.logits), sw.ldl)
            lib.lv_beam_select_f32(P(sw.logits), sw.ldl, P(w.score), P(w.meta), P(w.part), P(w.pick_score), P(w.pick_flat),
                                   P(w.margin), B, K, V, s)
            lib.lv_beam_advance_f32(P(w.pick_score), P(w.pick_flat), P(sw.hs, n * H), P(sw.cs, n * H), P(sw.hs), P(sw.cs),
                                    P(w.tok), P(w.score), P(w.meta), P(w.done_score), P(w.done_ref), P(w.trace), P(w.counter),
                                    t, T, B, K, H, V, end_tok, s)
            if (t + 1) % poll == 0 and t + 1 < T and int(w.counter.item()) == 0:      # the only host read of the loop
                break
        lib.lv_beam_backtrace(P(w.score), P(w.meta), P(w.done_score), P(w.done_ref), P(w.trace), P(w.ids), P(w.len), P(w.win),
                              B, K, T, start_tok, s)
        # one device-to-host copy: ids | len | meta | the bits of (winner's score, min margin)
        out = torch.cat((w.ids, w.len.to(torch.int64).unsqueeze(1), w.meta.to(torch.int64),
                         torch.stack((w.win, w.margin), dim=1).view(torch.int32).to(torch.int64)), dim=1).cpu()
        lens = out[:, T + 1].tolist()
        ids = [row[:m] for row, m in zip(out[:, :T + 1].tolist(), lens)]
        meta = out[:, T + 2:T + 6].numpy()
        fl = out[:, T + 6:].to(torch.int32).contiguous().view(torch.float32).numpy()
        info = {"score": fl[:, 0].copy(), "steps": meta[:, 2].copy(), "n_completed": meta[:, 0].copy(),
                "min_margin": fl[:, 1].copy()}
        return ids, info


class LSTMRollout(object):
    """Greedy / sample decoding for all sentences of a batch with every per-step decision on the device (lv_rollout.hip;
    reference modules/decoders/dec_lstm.py:270-367, whose loop -- like LSTMDecoder._roll_out -- masks on the host and reads
    "anybody alive" once per word).

    n sentences are n rows of LSTMDecodeStepper's exact-f32 launch sequence.  The z-projection (+ biases) of a row never changes,
    so it is computed once per call into Zp; a step is five launches: embedding gather of `tok`, input product with Zp as its
    addend, the T = 1 cell (reads half 0 of the (h, c) workspace, writes half 1), the vocabulary product, and
    lv_rollout_pick_f32, which picks, keeps ids / len / score / margin / alive, and moves the state back into half 0 -- no
    clone() / copy_() per step.  The host reads the one-int alive counter every `poll` steps and stops queueing when it is zero;
    steps queued past that point are no-ops by the kernel's counter gate, so the result does not depend on `poll`.

    Sampling draws torch.rand(n, generator=...) per queued step: the call LSTMDecoder._roll_out makes, in the same order, so for a
    given generator state both routes pick from the same uniforms.  The one difference: up to poll - 1 further draws are consumed
    after the last sentence has ended."""

    TMAX = 99                                                        # the reference's `length_c < 100`

    def __init__(self, stepper, poll=8):
        self.st = stepper
        self.device = stepper.device
        self.poll = poll
        self.ws = {}

    def _w(self, n):
        w = self.ws.get(n)
        if w is None:
            d, T = self.device, self.TMAX
            w = _NS()
            w.tok = torch.empty(n, dtype=torch.int64, device=d)
            w.alive = torch.empty(n, dtype=torch.int32, device=d)
            w.ids = torch.zeros(n, T, dtype=torch.int64, device=d)
            w.len = torch.empty(n, dtype=torch.int32, device=d)
            w.score = torch.empty(n, dtype=torch.float32, device=d)
            w.margin = torch.empty(n, dtype=torch.float32, device=d)
            w.counter = torch.empty(1, dtype=torch.int32, device=d)
            self.ws[n] = w
        return w

    def decode(self, z2, start_tok, end_tok, sample=False, generator=None, temperature=1.0, top_k=0, top_p=1.0):
        """z2 [n][nz] -> (ids: list of n int lists without <s>, info: dict of numpy arrays score / steps and, for greedy,
        min_margin, one entry per sentence).  A non-neutral temperature / top_k / top_p (sample only) takes
        lv_rollout_pick_filtered_f32 as the pick and adds proposal_score, the log-probability of the sentence under the
        distributions drawn from; score stays the model's log-probability."""
        inv_temp, top_k, top_p, neutral = sampling_filter(temperature, top_k, top_p)
        if not neutral and not sample:
            raise ValueError("temperature / top_k / top_p apply to sampling only")
        st = self.st
        n = z2.shape[0]
        h0, c0 = st.init_state(z2)                                   # refreshes the stepper's view of the parameters
        V, ni, H, nz = st.eng.dims()
        v = st.eng.flat.views
        lib, s = st.lib, stream_ptr(self.device)
        T = self.TMAX
        w, sw = self._w(n), st._w(n)
        lib.lv_rollout_init_f32(P(h0), P(c0), P(sw.hs), P(sw.cs), P(w.tok), P(w.alive), P(w.len), P(w.score), P(w.margin),
                                P(w.counter), n, H, V, start_tok, s)
        zr = z2.contiguous().float()
        wih = v["lstm.weight_ih_l0"]
        _gemm(lib, s, 0, 1, n, 4 * H, nz, P(zr), nz, P(wih, ni), ni + nz, P(sw.Zp), 4 * H,
              add1=P(v["lstm.bias_ih_l0"]), ld1=0, mod1=1, add2=P(v["lstm.bias_hh_l0"]), ld2=0, mod2=1)
        if not neutral:
            if getattr(w, "qscore", None) is None:
                w.qscore = torch.empty(n, dtype=torch.float32, device=self.device)
            w.qscore.zero_()
        poll = max(1, int(self.poll))
        for t in range(T):
            lib.lv_embed_gather_f32(P(v["embed.weight"]), P(w.tok), 1, None, 1.0, P(sw.X), 1, n, ni, V, s)
            _gemm(lib, s, 0, 1, n, 4 * H, ni, P(sw.X), ni, P(wih), ni + nz, P(sw.Gx), 4 * H, add1=P(sw.Zp), ld1=4 * H, mod1=n)
            lib.lv_lstm_fwd_f32(P(sw.Gx), P(v["lstm.weight_hh_l0"]), P(sw.hs), P(sw.cs), P(sw.gates), None, 1.0, None,
                                P(sw.lstm_ws), 1, n, H, s)
            _gemm(lib, s, 0, 1, n, V, H, P(sw.hs, n * H), H, P(v["pred_linear.weight"]), H, P(sw.logits), sw.ldl)
            u = torch.rand(n, device=self.device, generator=generator) if sample else None
            if neutral:
                lib.lv_rollout_pick_f32(P(sw.logits), sw.ldl, P(u), P(sw.hs, n * H), P(sw.cs, n * H), P(sw.hs), P(sw.cs), P(w.tok),
                                        P(w.alive), P(w.ids), P(w.len), P(w.score), P(w.margin), P(w.counter), t, T, n, H, V,
                                        end_tok, s)
            else:
                lib.lv_rollout_pick_filtered_f32(P(sw.logits), sw.ldl, P(u), inv_temp, top_k, top_p, P(sw.hs, n * H), P(sw.cs, n * H),
                                                 P(sw.hs), P(sw.cs), P(w.tok), P(w.alive), P(w.ids), P(w.len), P(w.score),
                                                 P(w.qscore), P(w.counter), t, T, n, H, V, end_tok, s)
            if (t + 1) % poll == 0 and t + 1 < T and int(w.counter.item()) == 0:      # the only host read of the loop
                break
        # one device-to-host copy: ids | len | the bits of (score, min margin[, proposal score])
        fcols = (w.score, w.margin) if neutral else (w.score, w.margin, w.qscore)
        out = torch.cat((w.ids, w.len.to(torch.int64).unsqueeze(1),
                         torch.stack(fcols, dim=1).view(torch.int32).to(torch.int64)), dim=1).cpu()
        lens = out[:, T].tolist()
        ids = [row[:m] for row, m in zip(out[:, :T].tolist(), lens)]
        fl = out[:, T + 1:].to(torch.int32).contiguous().view(torch.float32).numpy()
        info = {"score": fl[:, 0].copy(), "steps": out[:, T].numpy().copy()}
        if not sample:
            info["min_margin"] = fl[:, 1].copy()
        if not neutral:
            info["proposal_score"] = fl[:, 2].copy()
        return ids, info

"""Chunked / batched synthesis around ``model.inference`` (reference call site
/root/reference/parallel_wavegan/bin/decode.py:214-243).

The reference synthesises one whole utterance per call.  A convolutional vocoder only looks at a
bounded window of mel frames around each output sample, so a long utterance (or many utterances)
can be cut into equal-length chunks that carry ``halo`` frames of real context on both sides, run
as ONE batched forward (one hipGraph replay per chunk shape) and stitched by dropping the halos.
With ``halo >= receptive field`` every kept sample is computed from exactly the inputs the
full-length forward would use -- the result is exact, not an overlap-add approximation (it differs
from the one-shot forward only by the fp32 summation order of whichever tile configuration the
convolution kernel picks for the two shapes, <= 1e-5).

The first / last chunk of an utterance see the model's own zero padding on their outer side, so they
run without a halo there (they are batched across utterances when their lengths agree).

``RaggedSynthesizer`` batches WHOLE utterances of different lengths of the non-causal HiFi-GAN instead: one forward
over a padded block with a device table of frames per item, every item exactly what it gives alone;
``MelGANRaggedSynthesizer`` and ``PWGRaggedSynthesizer`` do the same for the reflect-padded (multi-band) MelGAN (s9.5)
and for Parallel WaveGAN, whose block carries each item's replicated edge frames and whose forward takes noise (s9.6).

Everything on the device runs in libpwgkernels.so: feature normalisation + (T', C) -> (C, T')
transpose, the generator, and the float -> PCM16 conversion.

``CausalStream`` is the other regime: synthesis WHILE the mel frames arrive, for generators built with
``use_causal_conv=True``.  Every causal layer keeps the last ``(k-1)*d`` columns of its raw input (one column for a
transposed layer) on the device, so a push of ``n`` frames costs ``n`` frames of work with zero look-ahead
(csrc/conv1d_stream.hip).  A causal multi-band MelGAN streams through a stateful PQMF synthesis, whose
symmetric filter adds a fixed latency of ``latency_samples`` (32 for the recipe filter; csrc/pqmf.hip).

``LookaheadStream`` streams the standard NON-causal HiFi-GAN: every layer runs in its causal form on a shifted time
axis, so a push of ``n`` frames still costs ``n`` frames of work and every sample leaves a fixed ``latency_samples``
late (3258 samples, 12.73 frames, for HiFi-GAN V1).  ``PWGLookaheadStream`` does the same for the
standard NON-causal Parallel WaveGAN (3921 samples, 15.3 frames, for ``parallel_wavegan.v1``), and
``MelGANLookaheadStream`` for the standard NON-causal, reflect-padded MelGAN and multi-band MelGAN, whose reflect-padded
layers mirror their window on read (1425 samples for ``melgan.v1``, 2720 for ``multi_band_melgan.v2``).

``StreamPool`` and ``PWGStreamPool`` run many look-ahead streams of the non-causal HiFi-GAN / Parallel WaveGAN in one
batch whose utterances start, pause and end independently: every launch reads each item's position from a small device
table; ``MelGANStreamPool`` does the same for the reflect-padded (multi-band) MelGAN, whose
mirrored launches also take their edges per item from the table (s11.12).
"""
import collections
import ctypes

import torch

from .. import _lib
from ..graphs import GraphedInference
from ..ops import (_ptr, _require_device, _stream, conv1d_stream_bf16_delayed_supported, conv1d_stream_bf16_supported,
                   conv1d_stream_delayed_supported, conv1d_stream_mirrored_supported, conv1d_stream_supported)


def normalize_transpose(c, mean=None, scale=None):
    """(B, T', C) features -> (B, C, T') with optional ``(c - mean) / scale`` (one HIP launch)."""
    c = c.contiguous()
    _require_device(c, mean, scale)
    b, t, ch = c.shape
    y = torch.empty((b, ch, t), device=c.device, dtype=torch.float32)
    _lib.check(_lib.lib().pwg_normalize_transpose(_ptr(c), _ptr(mean), _ptr(scale), _ptr(y), b, t, ch, _stream()),
               "normalize_transpose")
    return y


def to_pcm16(wave):
    """float waveform -> int16 PCM (clip to [-1, 1], scale 32767, round to nearest) on the device."""
    wave = wave.contiguous()
    _require_device(wave)
    pcm = torch.empty(wave.shape, device=wave.device, dtype=torch.int16)
    if wave.numel() == 0:  # (a push that emits nothing yet: warm-up, or inside the PQMF delay)
        return pcm
    _lib.check(_lib.lib().pwg_wave_to_pcm16(_ptr(wave), ctypes.c_void_p(pcm.data_ptr()), wave.numel(), _stream()),
               "wave_to_pcm16")
    return pcm


@torch.no_grad()
def receptive_field_frames(model, in_channels=None, probe_frames=96):
    """Measured reach of the generator in mel frames: (left, right) = how many frames before / after
    frame t can influence the samples generated for frame t.  Found by perturbing one half of a random
    input and locating the first / last output sample that changes (exact for a convolutional model;
    the probe is doubled until the reach fits inside it)."""
    dev = next(model.parameters()).device
    ch = in_channels or getattr(model, "in_channels", None) or 80
    up = model.upsample_factor
    while True:
        n = probe_frames
        gen = torch.Generator(device="cpu").manual_seed(1234)
        c1 = torch.randn(1, ch, n, generator=gen).to(dev)
        half = n // 2
        c_future, c_past = c1.clone(), c1.clone()
        c_future[..., half:] = torch.randn(1, ch, n - half, generator=gen).to(dev)
        c_past[..., :half] = torch.randn(1, ch, half, generator=gen).to(dev)
        y = model(c1)
        # (several output channels, i.e. sub-bands: a change is located along time, whichever band shows it)
        d_future = (model(c_future) != y).flatten().nonzero() % y.shape[-1]
        d_past = (model(c_past) != y).flatten().nonzero() % y.shape[-1]
        # frames >= half changed: earliest affected sample tells how far the future reaches back
        first = int(d_future.min()) if d_future.numel() else half * up
        last = int(d_past.max()) if d_past.numel() else half * up - 1
        right = -(-(half * up - first) // up)          # frames of look-ahead
        left = -(-(last + 1 - half * up) // up)        # frames of look-back
        right, left = max(right, 0), max(left, 0)
        if max(left, right) < half - 1:
            return left, right
        probe_frames *= 2


class ChunkedSynthesizer:
    """Exact chunked synthesis for generators that map (B, C, T') mel -> (B, 1, T' * upsample_factor)
    from the mel alone (HiFi-GAN, MelGAN).  ``chunk_frames`` frames of output per chunk;
    ``max_batch`` chunks per forward.  A multi-band model (``model.pqmf`` attached) has its K sub-band rows stitched
    the same way, then one ``pqmf.synthesis`` per utterance: T' * upsample_factor * K samples.  Several output channels
    without a PQMF are an error."""

    def __init__(self, model, chunk_frames=256, max_batch=16, halo=None, use_graph=True):
        self.model = model.eval()
        self.chunk = int(chunk_frames)
        self.max_batch = int(max_batch)
        self.left, self.right = halo if halo is not None else receptive_field_frames(model)
        self.up = model.upsample_factor
        self.pqmf = getattr(model, "pqmf", None)
        self.rows = self.pqmf.subbands if self.pqmf is not None else 1  # output channels of the generator
        self._run = GraphedInference(self.model) if use_graph else self.model

    def _plan(self, n_frames):
        """[(start, end, ctx_start, ctx_end)] frame ranges of one utterance."""
        if n_frames <= self.chunk + self.left + self.right:
            return [(0, n_frames, 0, n_frames)]
        out = []
        for s in range(0, n_frames, self.chunk):
            e = min(n_frames, s + self.chunk)
            out.append((s, e, max(0, s - self.left), min(n_frames, e + self.right)))
        return out

    @torch.no_grad()
    def synthesize_many(self, feats, normalize_before=False):
        """feats: list of (T'_i, C) tensors/arrays -> list of (T'_i * upsample_factor [* subbands],) float waveforms."""
        dev = next(self.model.parameters()).device
        mean = getattr(self.model, "mean", None) if normalize_before else None
        scale = getattr(self.model, "scale", None) if normalize_before else None
        mels = []
        for f in feats:
            f = torch.as_tensor(f, dtype=torch.float32).to(dev)
            mels.append(normalize_transpose(f.unsqueeze(0), mean, scale)[0])  # (C, T')
        outs = [torch.empty(self.rows, m.shape[-1] * self.up, device=dev) for m in mels]
        # group chunks by (context length, whether the model's own padding is on the left / right):
        # only equal-shaped chunks share a batch, and edge chunks keep their true zero-padded side
        groups = {}
        for ui, m in enumerate(mels):
            n = m.shape[-1]
            for (s, e, cs, ce) in self._plan(n):
                groups.setdefault((ce - cs, cs == 0, ce == n), []).append((ui, s, e, cs, ce))
        for (length, _, _), items in groups.items():
            for i in range(0, len(items), self.max_batch):
                part = items[i:i + self.max_batch]
                batch = torch.stack([mels[ui][:, cs:ce] for (ui, s, e, cs, ce) in part])
                if len(part) < self.max_batch and len(items) > self.max_batch:
                    # keep one graph per chunk shape: pad the last partial batch with copies
                    pad = self.max_batch - len(part)
                    batch = torch.cat([batch, batch[:1].expand(pad, -1, -1)], 0)
                y = self._run(batch.contiguous())
                if y.shape[1] != self.rows:
                    raise ValueError(f"ChunkedSynthesizer: the generator emits {y.shape[1]} channels but "
                                     + (f"model.pqmf has {self.rows} sub-bands" if self.pqmf is not None else
                                        "no PQMF is attached (model.pqmf = PQMF(subbands=...), as utils.load_model does)"))
                for j, (ui, s, e, cs, ce) in enumerate(part):
                    outs[ui][:, s * self.up:e * self.up] = y[j, :, (s - cs) * self.up:(e - cs) * self.up]
        if self.pqmf is not None:
            return [self.pqmf.synthesis(o.unsqueeze(0))[0, 0] for o in outs]
        return [o[0] for o in outs]

    def synthesize(self, feat, normalize_before=False):
        """(T', C) -> (T' * upsample_factor [* subbands],)"""
        return self.synthesize_many([feat], normalize_before)[0]


def _capture_directions(halves, run):
    """Graphs for both directions (A -> B, B -> A) of one chunk shape: ``run(hist_in, hist_out)`` on static inputs ->
    {cur: (graph, static_out)}.  The warm-up runs write history: both halves are saved and put back, so capturing never
    advances a stream."""
    saved = [[t.clone() for t in half] for half in halves]
    out = {}
    for cur in (0, 1):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):  # fills the weight caches / sets kernel attributes outside the capture
                run(halves[cur], halves[1 - cur])
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            static_out = run(halves[cur], halves[1 - cur])
        out[cur] = (g, static_out)
    for half, keep in zip(halves, saved):
        for t, k in zip(half, keep):
            t.copy_(k)
    return out


class _Stream:
    """What the stream classes share: the constructor's checks (small class methods; the class name in a message is
    the caller's), the ping-pong state (``_halves``: two lists of history tensors, a push reads ``_halves[_cur]`` and
    writes the other), feature and noise coercion, the counters, the step (eager first push, then replay or run, then
    swap) and the captured graphs (``_graphs``: chunk shape -> entry, most recently used last; ``_state``: the model's
    parameter state they were captured under; ``_watch``: a ``GraphedInference`` asked for that state only).  A subclass
    validates its model, then calls ``__init__``; it provides ``push``, ``reset`` and ``_run(feats, [z,] hist_in,
    hist_out)``, the model on one push's inputs in steady state."""

    max_graph_shapes = 4  # chunk sizes whose graphs are kept (least recently used evicted)
    _pooled = False       # a pool of slots (the wording of some refusals), not lock-step streams

    def __init__(self, model, layers, batch, use_graph, normalize_before, extra_history=()):
        """``layers``: ``model.stream_layers()``; ``batch``: from ``_checked_batch``; ``extra_history``: shapes of
        further state tensors that ride behind the layers' in both halves."""
        name = type(self).__name__
        _require_device(next(model.parameters()))  # no CPU fallback
        if normalize_before and not (hasattr(model, "mean") and hasattr(model, "scale")):
            raise ValueError(f"{name}: normalize_before=True needs model.register_stats(...)")
        self.model = model.eval()
        self.batch = batch
        self.use_graph = bool(use_graph)
        self.normalize_before = bool(normalize_before)
        self._layers = layers
        self._device = next(model.parameters()).device
        shapes = [layer.history_shape(batch) for layer, _ in layers] + list(extra_history)
        self._halves = [[torch.zeros(shape, device=self._device) for shape in shapes] for _ in range(2)]
        self._watch = GraphedInference(model)  # (only its parameter-state key is used)
        self._state = None
        self._graphs = {}
        self.reset()

    @classmethod
    def _checked_batch(cls, batch):
        batch = int(batch)
        if batch < 1:
            raise ValueError(f"{cls.__name__}: batch must be >= 1")
        return batch

    @classmethod
    def _checked_sizes(cls, batch, columns=None):
        """``(batch, columns of a launch the kernel coverage is asked about)``; a pool's are its slots and chunk."""
        return cls._checked_batch(batch), 8

    @classmethod
    def _checked_precision(cls, precision, no_bf16=None):
        """The constructor's ``precision`` -> ``"fp32"`` (also for None) or ``"bf16"``; ``no_bf16``: why the class has no
        bf16 stream."""
        if no_bf16 is None:
            if precision not in (None, "fp32", "bf16"):
                raise ValueError(f"{cls.__name__}: precision must be None, 'fp32' or 'bf16', got {precision!r}")
        elif precision == "bf16":
            raise ValueError(f"{cls.__name__}: precision='bf16' is not available: {no_bf16}")
        elif precision not in (None, "fp32"):
            raise ValueError(f"{cls.__name__}: precision must be None or 'fp32', got {precision!r}")
        return precision or "fp32"

    @classmethod
    def _refuse_bf16_model(cls, model, precision, stream, has_bf16=True):
        """An fp32 stream does not read the mode ``set_inference_precision(model, 'bf16')`` put the modules in."""
        from ..layers.conv import each_conv

        if precision == "bf16" or all(cv.precision == "fp32" for cv in each_conv(model)):
            return
        name, undo = cls.__name__, "utils.set_inference_precision(model, 'fp32')"
        if has_bf16:
            raise ValueError(f"{name}: the model is in bf16 inference precision; the fp32 {stream} does not read that mode "
                             f"({undo}, or stream with bf16 operands: {name}(model, precision='bf16'))")
        raise ValueError(f"{name}: the model is in bf16 inference precision; the {stream} is fp32 ({undo})")

    @classmethod
    def _checked_pqmf(cls, model, out_channels):
        """``model.pqmf`` (None: full-band) of a generator that emits ``out_channels`` rows, or the refusal."""
        from ..layers.pqmf import PQMF
        from ..models import MelGANGenerator

        name, pqmf = cls.__name__, getattr(model, "pqmf", None)
        if out_channels != 1 and (pqmf is None or not isinstance(model, MelGANGenerator)):
            raise ValueError(f"{name}: the generator emits {out_channels} sub-bands; only a multi-band MelGANGenerator with "
                             "its PQMF attached (model.pqmf = PQMF(subbands=...), as utils.load_model does) can be "
                             "streamed, through the stateful PQMF synthesis")
        if pqmf is not None:
            if not isinstance(pqmf, PQMF) or pqmf.subbands != out_channels:
                raise ValueError(f"{name}: model.pqmf must be a PQMF with as many sub-bands as the generator emits "
                                 f"({out_channels}); got {getattr(pqmf, 'subbands', pqmf.__class__.__name__)}")
            if pqmf.subbands > 8:
                raise ValueError(f"{name}: a PQMF of {pqmf.subbands} sub-bands cannot be streamed (the stream kernel "
                                 "covers up to 8)")
        return pqmf

    @classmethod
    def _require_supported(cls, ok, what, how=""):
        """``ok``: the answer of a kernel's ``*_supported``, whose reason for a refusal is ``pwg_last_error``."""
        if not ok:
            raise ValueError(f"{cls.__name__}: {what} cannot be streamed{how}: "
                             + _lib.lib().pwg_last_error().decode(errors="replace"))

    @property
    def state_bytes(self):
        """Bytes of history held on the device (both ping-pong halves)."""
        return sum(t.numel() * t.element_size() for half in self._halves for t in half)

    def _restart(self):
        """Back to start of stream: half 0 is written next, from ``hist_in = None``; the counters start over."""
        self._cur = 0          # which half holds the current history
        self._started = False  # False: the next run passes hist_in = None
        self.frames_in = 0
        self.frames_out = 0
        self.samples_out = 0

    def _features(self, feats):
        """(B, n, C) features -> (B, C, n), normalised with the model's statistics if the stream says so."""
        mean = self.model.mean if self.normalize_before else None
        scale = self.model.scale if self.normalize_before else None
        return normalize_transpose(feats, mean, scale)

    def _coerce(self, feats):
        """What ``push`` takes -> contiguous (batch, n, C) fp32 on the stream's device."""
        feats = torch.as_tensor(feats, dtype=torch.float32).to(self._device)
        if feats.dim() == 2:
            feats = feats.unsqueeze(0)
        if feats.dim() != 3 or feats.shape[0] != self.batch:
            raise ValueError(f"{type(self).__name__}.push: expected (n, C) or ({self.batch}, n, C) features, got "
                             f"{tuple(feats.shape)}")
        return feats.contiguous()

    def _coerce_noise(self, noise, n):
        """The noise ``push`` takes for ``n`` frames -> contiguous (batch, 1, n * up) fp32 on the stream's device; None
        (drawn on the device in ``_push_step``) stays None."""
        if noise is None:
            return None
        noise = torch.as_tensor(noise, dtype=torch.float32).to(self._device)
        if noise.dim() == 1:
            noise = noise.unsqueeze(0).expand(self.batch, -1)
        if tuple(noise.shape) != (self.batch, n * self.up):
            raise ValueError(f"{type(self).__name__}.push: expected ({n * self.up},) or ({self.batch}, {n * self.up}) noise "
                             f"for {n} frame(s), got {tuple(noise.shape)}")
        return noise.reshape(self.batch, 1, n * self.up).contiguous()

    def _empty(self):
        """The emission of a push that emits nothing."""
        return torch.empty((self.batch, 0), device=self._device, dtype=torch.float32)

    def _graph_entry(self, key, capture):
        """The entry of chunk shape ``key``, captured by ``capture()`` on first use.  All graphs are dropped when the
        model's parameter state changed, so a replay never uses old weights."""
        state = self._watch._param_state()
        if state != self._state:
            self._graphs, self._state = {}, state
        entry = self._graphs.pop(key, None)
        if entry is None:
            while len(self._graphs) >= self.max_graph_shapes:
                del self._graphs[next(iter(self._graphs))]  # least recently used chunk shape
            entry = capture()
        self._graphs[key] = entry  # most recently used last
        return entry

    def _capture(self, *inputs):
        """Graphs for both directions of one chunk shape, ``_run`` on static copies of ``inputs`` -> ``(*statics,
        graphs)``.  The warm-up runs write history: both halves are saved and put back, so capturing never advances the
        stream."""
        statics = [t.clone() for t in inputs]
        return (*statics, _capture_directions(self._halves, lambda hi, ho: self._run(*statics, hi, ho)))

    def _step(self, n, key, eager, capture, fill_static):
        """One push of ``n`` frames through the ping-pong halves -> (batch, samples), the caller's own tensor.
        ``eager(hist_in, hist_out)`` runs the model.  Start of stream (the layers' own padding; once per utterance):
        ``eager(None, half 0)``.  Afterwards current half -> other half, then the halves swap: eagerly, or with
        ``capture`` (not None: graph mode) by replaying the graph of chunk shape ``key`` -- ``capture()`` ->
        ``(*statics, graphs)`` on first use -- after ``fill_static(*statics)`` wrote this push's inputs."""
        if not self._started:
            y = eager(None, self._halves[0])
            self._cur, self._started = 0, True
        else:
            if capture is not None:
                *statics, graphs = self._graph_entry(key, capture)
                g, static_out = graphs[self._cur]
                fill_static(*statics)
                g.replay()
                y = static_out.clone()
            else:
                y = eager(self._halves[self._cur], self._halves[1 - self._cur])
            self._cur = 1 - self._cur
        self.frames_out += n
        self.samples_out += y.shape[1]
        return y

    def _push_step(self, feats, noise, run, graph):
        """``_step`` on the inputs of one push: ``feats`` from ``_coerce``; ``noise``: ``()`` for a stream that takes
        none, else ``(z,)`` from ``_coerce_noise``, None being drawn with ``torch.randn`` on the device -- never inside a
        graph: it is written into the graph's static buffer before the replay.  ``run(feats, *noise, hist_in,
        hist_out)``: the eager run of this push; ``graph``: may it replay the graphs of its chunk shape instead."""
        n = feats.shape[1]
        shape = (self.batch, 1, n * self.up)

        def eager(hist_in, hist_out):
            return run(feats, *(torch.randn(shape, device=self._device) if z is None else z for z in noise), hist_in,
                       hist_out)

        def capture():
            return self._capture(feats, *(torch.zeros(shape, device=self._device) for _ in noise))

        def fill_static(static_in, *static_noise):
            static_in.copy_(feats, non_blocking=True)
            for static_z, z in zip(static_noise, noise):
                if z is None:
                    static_z.normal_()  # (outside the graph: a replay never draws)
                else:
                    static_z.copy_(z, non_blocking=True)

        return self._step(n, (n, feats.shape[2]), eager, capture if graph else None, fill_static)

    def push_pcm16(self, *args, **kwargs):
        """``push`` through the float -> PCM16 conversion: (batch, samples) int16."""
        return to_pcm16(self.push(*args, **kwargs))

    def close(self):
        """End of the utterance.  Nothing is held back here; a stream that can hold frames overrides it."""

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        return False


class CausalStream(_Stream):
    """Stateful streaming synthesis for ``HiFiGANGenerator`` and ``MelGANGenerator`` built with
    ``use_causal_conv=True``: ``push`` takes the next mel frames of ``batch`` lock-step streams and returns their
    samples; any partition of the same frames gives bit-identical audio, equal to the whole-utterance ``forward`` up to
    fp32 summation order.

    Multi-band MelGAN (``model.pqmf`` attached, up to 8 sub-bands): the sub-bands of a push go through
    ``PQMF.stream_synthesis`` in the same push.  The synthesis filter is symmetric, so every sample leaves
    ``latency_samples`` (K * ceil(taps / 2 / K); 32 for the recipe filter) late: the first emissions of an utterance are
    short by that much in total, afterwards a push of ``n`` frames returns ``n * up`` samples (``up`` =
    ``upsample_factor * K``), and ``flush()`` returns the tail, after which the emissions total ``frames * up`` samples and
    equal ``pqmf.synthesis`` of the whole utterance's sub-bands bit for bit.  ``close()`` does not flush: an unflushed
    tail is dropped.

    State: per causal layer two history tensors (ping-pong: a push reads one half and writes the other, in the layer's
    own launch).  ``use_graph``: steady-state pushes of one chunk size replay two captured graphs (A -> B, B -> A);
    the first push of a stream (the layers' own start-of-stream padding) runs eagerly, as do the pushes of a
    multi-band stream that has not yet received more columns than the PQMF delay.  Graphs are dropped when the
    model's parameter state (``GraphedInference._param_state``) changes, so a replay never uses old weights.
    Graph mode wants a fixed chunk size: the first push of a new size captures inside ``push`` (four warm-up runs and
    two captures), each captured size holds a private pool of all activations, and only the ``max_graph_shapes`` most
    recently used sizes are kept.  A stream whose chunk size varies freely should pass ``use_graph=False``.

    ``precision="bf16"``: every convolution of every push runs with bf16 operands (csrc/conv1d_stream_bf16.hip, DESIGN.md
    s11.2: the activated window and the weights are rounded to bf16, sums, epilogues, tensors and history stay fp32; the
    PQMF synthesis stays fp32).  The precision belongs to the stream, is fixed for its life (``.precision``) and neither
    reads nor writes the modules' own ``precision`` attributes; partition invariance holds bit for bit as in fp32, and a
    bf16 stream's state is interchangeable with an fp32 stream's.  ``None`` and ``"fp32"`` are the fp32 stream, which
    refuses a model that ``set_inference_precision`` put in bf16 mode.

    Reflect-padded models (causal MelGAN) need the first ``warmup_frames`` frames before anything can be emitted -- an
    utterance shorter than that is one the whole-utterance forward cannot pad either: the stream holds what is pushed
    until then, returning zero-length waveforms, and ``close()`` raises if frames are still held.
    """

    def __init__(self, model, batch=1, use_graph=True, normalize_before=False, precision=None):
        from ..models import HiFiGANGenerator, MelGANGenerator

        precision = self._checked_precision(precision)
        if not isinstance(model, (HiFiGANGenerator, MelGANGenerator)):
            raise ValueError(f"CausalStream: {model.__class__.__name__} is not supported (only the causal HiFiGANGenerator "
                             "and MelGANGenerator map mel frames to samples layer by layer; a causal "
                             "ParallelWaveGANGenerator, which also takes noise, streams through utils.PWGStream)")
        layers = model.stream_layers()  # ValueError for a non-causal model
        out_channels = model.output_conv[1].conv.out_channels if isinstance(model, HiFiGANGenerator) else \
            layers[-1][0].conv.out_channels
        pqmf = self._checked_pqmf(model, out_channels)
        self._refuse_bf16_model(model, precision, "streaming kernel")
        batch = self._checked_batch(batch)
        supported = conv1d_stream_bf16_supported if precision == "bf16" else conv1d_stream_supported
        for layer, _ in layers:
            self._require_supported(supported(layer.stream_desc(batch, 8)), layer)
        self.precision = precision  # of the stream, fixed for its life
        self.pqmf = pqmf
        self.subbands = out_channels
        self.up = model.upsample_factor * out_channels  # samples per frame
        self._delay = pqmf.stream_delay_columns if pqmf is not None else 0
        self.latency_samples = self._delay * out_channels
        self.warmup_frames = self.required_warmup_frames(model)
        # the PQMF history rides behind the layers' in both ping-pong halves
        super().__init__(model, layers, batch, use_graph, normalize_before,
                         [pqmf.history_shape(batch)] if pqmf is not None else [])

    @staticmethod
    def required_warmup_frames(model):
        """Frames the first emission needs, from the layer geometry alone (no device, no kernel): the maximum over
        the causal layers of ``ceil(columns the layer's start-of-stream padding reads / the layer's columns per
        frame)`` -- 1 for zero-padded models."""
        return max(-(-layer.history_columns_at_start() // rate) for layer, rate in model.stream_layers())

    def reset(self):
        """Back to start of stream: the next push starts from the layers' own padding and, for a multi-band model, from
        the PQMF's zero context.  Held frames and an unflushed tail are dropped."""
        self._restart()
        self._held = []
        self._columns = 0      # sub-band columns the PQMF stream has taken (multi-band)
        self._flushed = False

    def _emit(self, n_cols):
        """Positions a PQMF launch over the next ``n_cols`` columns completes: ``n_cols`` once the stream is past the
        delay, fewer (or none) before."""
        return max(0, self._columns + n_cols - self._delay) - max(0, self._columns - self._delay)

    def _run(self, feats, hist_in, hist_out, n_emit=None):
        """``hist_in`` (None: start of stream) / ``hist_out``: one ping-pong half each.  -> (batch, samples)."""
        k = len(self._layers)  # (a multi-band stream's halves end with the PQMF's history)
        y = self.model.stream_forward(self._features(feats), None if hist_in is None else hist_in[:k], hist_out[:k],
                                      precision=self.precision)
        if self.pqmf is None:
            return y.reshape(self.batch, -1)
        return self.pqmf.stream_synthesis(y, None if hist_in is None else hist_in[-1], hist_out[-1],
                                          y.shape[-1] if n_emit is None else n_emit)

    @torch.no_grad()
    def push(self, feats):
        """feats: (n, C) or (batch, n, C) float features -> (batch, samples) fp32: ``m * up`` samples, ``m`` the frames
        emitted by this push (``n``, except around the warm-up of a reflect-padded model), less what the PQMF delay of a
        multi-band model still holds back at the start of an utterance (``latency_samples`` in total).  The result is the
        caller's own tensor (not a graph's static buffer)."""
        if self._flushed:
            raise RuntimeError("CausalStream.push: the utterance was flushed; reset() starts the next one")
        feats = self._coerce(feats)
        self.frames_in += feats.shape[1]
        if not self._started:
            self._held.append(feats)
            if sum(f.shape[1] for f in self._held) < self.warmup_frames:
                return self._empty()
            feats = torch.cat(self._held, 1) if len(self._held) > 1 else feats
            self._held = []
        n = feats.shape[1]
        if n == 0:
            return self._empty()
        n_cols = n * self.model.upsample_factor
        n_emit = self._emit(n_cols)
        graph = self.use_graph and n_emit == n_cols  # (a multi-band stream still inside the PQMF delay: eager)
        y = self._push_step(feats, (), lambda f, hi, ho: self._run(f, hi, ho, n_emit), graph)
        self._columns += n_cols
        return y

    @torch.no_grad()
    def flush(self):
        """End of the utterance of a multi-band stream: ``stream_delay_columns`` zero columns through the PQMF launch
        (the zeros the whole-utterance synthesis pads with) -> the last ``latency_samples`` samples, (batch, samples).
        Zero-length for a full-band model, before anything was synthesised, and on a second call.  The next utterance
        starts with ``reset()``."""
        if self.pqmf is None or not self._started or self._flushed:
            return self._empty()
        zeros = torch.zeros((self.batch, self.subbands, self._delay), device=self._device)
        y = self.pqmf.stream_synthesis(zeros, self._halves[self._cur][-1], self._halves[1 - self._cur][-1],
                                       self._emit(self._delay))
        self._columns += self._delay
        self._flushed = True  # (the halves are not swapped: nothing may follow but reset())
        self.samples_out += y.shape[1]
        return y

    def close(self):
        """End of the utterance: raises if frames are still held (the utterance was shorter than ``warmup_frames``,
        which the whole-utterance forward cannot pad either).  It does not flush: the last ``latency_samples`` samples of
        a multi-band utterance come from ``flush()``, and without it they are dropped."""
        held = sum(f.shape[1] for f in self._held)
        if held:
            raise RuntimeError(f"CausalStream: {held} frame(s) were pushed but the reflect-padded start of this model "
                               f"needs {self.warmup_frames} before the first sample can be emitted")


class PWGStream(_Stream):
    """Stateful streaming synthesis for ``ParallelWaveGANGenerator`` built with ``use_causal_conv=True``: ``push`` takes
    the next mel frames (and, optionally, the noise for their samples) of ``batch`` lock-step streams and returns their
    samples, one launch per layer: the upsampler's ``conv_in`` and stages, the 1 x 1 convolutions and the 30 gated
    residual blocks each run their stream kernel on the chunk (csrc/wavenet_stream.hip, csrc/elementwise.hip,
    csrc/conv1d_stream.hip).  Any partition of the same frames and noise gives bit-identical audio,
    equal to the whole-utterance ``forward`` up to fp32 summation order.

    State: ``conv_in`` keeps the last ``aux_context_window`` frames, an upsampling stage the last 2 columns of its
    input, a residual block the last ``2 * dilation`` columns of its input (``state_bytes``: both ping-pong halves).
    ``reset()``: the next push starts an utterance as ``model.inference`` does -- ``conv_in`` sees its first frame
    replicated to the left, every other layer zeros.  ``reset(context)`` seeds ``conv_in`` with ``aux_context_window``
    real frames instead (the frames before a cut): the stream then equals ``model.forward(z, concat(context, frames,
    anything))``.

    ``use_graph``, ``max_graph_shapes`` and the parameter-state watch are those of :class:`CausalStream`: steady-state
    pushes of one chunk size replay two captured graphs; the first push of an utterance started without context runs
    eagerly.  Noise is never drawn inside a graph: it is written into the graph's static buffer before the replay.

    ``precision="bf16"``: ``conv_in``, the 1 x 1 convolutions and the 30 residual blocks of every push run with bf16
    operands (csrc/conv1d_stream_bf16.hip, csrc/wavenet_stream_bf16.hip; DESIGN.md s11.7: windows, weights and the gate
    output are rounded to bf16; sums, the gate, biases, residual, skip sum, tensors and history stay fp32; the stretch
    stages of the upsampler stay fp32).  As in :class:`CausalStream` the precision belongs to the stream, is fixed for its
    life (``.precision``) and neither reads nor writes the modules' own ``precision`` attributes; state, ``reset(context)``
    and partition invariance are those of the fp32 stream, and a bf16 stream's state is interchangeable with an fp32
    stream's.  ``None`` and ``"fp32"`` are the fp32 stream, which refuses a model that ``set_inference_precision`` put in
    bf16 mode.
    """

    warmup_frames = 1  # zero / replicate start: the first frame can be synthesised at once

    def __init__(self, model, batch=1, use_graph=True, normalize_before=False, precision=None):
        from ..layers.causal_conv import pointwise_desc
        from ..layers.upsample import ConvInStream
        from ..models import ParallelWaveGANGenerator

        precision = self._checked_precision(precision)
        if not isinstance(model, ParallelWaveGANGenerator):
            raise ValueError(f"PWGStream: {model.__class__.__name__} is not supported (only the causal "
                             "ParallelWaveGANGenerator; HiFiGANGenerator and MelGANGenerator stream through CausalStream)")
        batch = self._checked_batch(batch)
        reason = model.stream_unsupported_reason(batch, precision)
        if reason is not None:
            raise ValueError(f"PWGStream: {reason}")
        if model.in_channels != 1 or model.out_channels != 1:
            raise ValueError(f"PWGStream: in_channels / out_channels = {model.in_channels} / {model.out_channels} (the "
                             "stream takes one noise row and emits one waveform per stream)")
        self._refuse_bf16_model(model, precision, "streaming layer kernel")
        layers = model.stream_layers()
        supported = conv1d_stream_bf16_supported if precision == "bf16" else conv1d_stream_supported
        for layer, _ in layers:
            if isinstance(layer, ConvInStream):
                self._require_supported(supported(layer.stream_desc(batch, 8)), layer)
        if precision == "bf16":  # a bf16 stream never runs a convolution the bf16 kernel refuses in fp32 instead
            for cv in model.pointwise_convs():
                self._require_supported(supported(pointwise_desc(cv, batch, 8)), cv, " with bf16 operands")
        self.precision = precision  # of the stream, fixed for its life
        self.up = model.upsample_factor  # samples per frame
        self._context = model.aux_context_window if isinstance(layers[0][0], ConvInStream) else 0
        super().__init__(model, layers, batch, use_graph, normalize_before)

    @torch.no_grad()
    def reset(self, context=None):
        """Back to start of stream.  ``context`` None: the next push starts from ``conv_in``'s replicated first frame and
        zero history everywhere else (``model.inference``).  ``context`` (batch, aux_context_window, C) or
        (aux_context_window, C): those frames are ``conv_in``'s history, every other layer starts from zeros
        (``model.forward`` on ``concat(context, frames, anything)``)."""
        self._restart()
        if context is None:
            return
        if self._context == 0:
            raise ValueError("PWGStream.reset: the model has no aux_context_window, so there is no context to seed")
        context = torch.as_tensor(context, dtype=torch.float32).to(self._device)
        if context.dim() == 2:
            context = context.unsqueeze(0).expand(self.batch, -1, -1)
        if context.dim() != 3 or context.shape[0] != self.batch or context.shape[1] != self._context:
            raise ValueError(f"PWGStream.reset: expected ({self._context}, C) or ({self.batch}, {self._context}, C) context "
                             f"frames, got {tuple(context.shape)}")
        for t in self._halves[0]:
            t.zero_()
        self._halves[0][0].copy_(self._features(context.contiguous()))
        self._started = True

    def _run(self, feats, z, hist_in, hist_out):
        """``hist_in`` (None: start of stream) / ``hist_out``: one ping-pong half each.  -> (batch, samples)."""
        return self.model.stream_forward(z, self._features(feats), hist_in, hist_out,
                                         precision=self.precision).reshape(self.batch, -1)

    @torch.no_grad()
    def push(self, feats, noise=None):
        """feats: (n, C) or (batch, n, C) float features; noise: (batch, n * up) or (n * up,) (the same for every
        stream), drawn with ``torch.randn`` on the device if omitted -> (batch, n * up) fp32.  The result is the caller's
        own tensor (not a graph's static buffer)."""
        feats = self._coerce(feats)
        n = feats.shape[1]
        noise = self._coerce_noise(noise, n)
        self.frames_in += n
        if n == 0:
            return self._empty()
        return self._push_step(feats, (noise,), self._run, self.use_graph)


# What a look-ahead stream or pool is built from, for one model, batch and precision: ``batch`` / ``columns`` from
# ``_checked_sizes``; ``plan``: ``model.lookahead_plan()``; ``pqmf``: of a multi-band model, else None; ``up``: samples per
# frame; ``latency_samples``: how late every sample leaves; ``settle_frames``: frames after which no launch has an edge of
# the utterance in its window or history and nothing is trimmed; ``min_frames``: the shortest utterance; ``state_shapes``:
# of one ping-pong half, the PQMF history last.
StreamFigures = collections.namedtuple("StreamFigures", "batch columns plan pqmf up latency_samples settle_frames min_frames "
                                                        "state_shapes")


def _figures(model, plan, pqmf, batch, columns, state_shapes, settle_frames=0, min_frames=1):
    """The figures that follow from a plan, whatever the family: ``latency_samples`` = the generator's delay times the
    sub-band count, plus the PQMF's ``K * stream_delay_columns``; ``settle_frames``: what the plan's edges need
    (``settle_frames``), and the latency in frames."""
    k = pqmf.subbands if pqmf is not None else 1
    up = model.upsample_factor * k
    latency = (plan[-1].delay + (pqmf.stream_delay_columns if pqmf is not None else 0)) * k
    return StreamFigures(batch, columns, plan, pqmf, up, latency, max(settle_frames, -(-latency // up)), min_frames,
                         state_shapes + ([pqmf.history_shape(batch)] if pqmf is not None else []))


class _Family:
    """One family of look-ahead streaming (a generator class): whether a model can be streamed and with which figures,
    for the lock-step class and the pool alike -- both inherit the family beside their core.  ``_streamable(model, batch,
    columns, precision)`` runs the refusals in the family's order, under the caller's name and in its wording
    (``_pooled``), and returns the :class:`StreamFigures`; ``_figures_of(model, batch)`` is its part that needs neither a
    device nor a kernel, which the ``*_of`` class methods read."""

    @classmethod
    def _conv_plan_figures(cls, model, plan, pqmf, batch=1, columns=8):
        """:func:`_figures` of a convolution plan (HiFi-GAN, MelGAN); for a plan without a reflect-padded launch
        ``settle_frames`` is the latency in frames and ``min_frames`` 1."""
        from ..layers.causal_conv import lookahead_settle_frames, lookahead_state_shapes, mirrored_min_frames

        return _figures(model, plan, pqmf, batch, columns, lookahead_state_shapes(plan, batch),
                        lookahead_settle_frames(plan), mirrored_min_frames(plan))

    @classmethod
    def _require_plan(cls, plan, batch, columns, precision):
        """Every launch of a convolution plan must be one its kernel covers (the slotted forms cover what the delayed
        and mirrored forms cover; the answer does not depend on the column count)."""
        from ..layers.causal_conv import launch_desc, launch_is_mirrored

        delayed = conv1d_stream_bf16_delayed_supported if precision == "bf16" else conv1d_stream_delayed_supported
        for launch in plan:
            desc = launch_desc(launch, batch, columns)
            cls._require_supported(conv1d_stream_mirrored_supported(desc) if launch_is_mirrored(launch) else
                                   delayed(desc, launch.delay1, launch.delay2), launch.conv)

    @classmethod
    def latency_samples_of(cls, model):
        """Samples every output leaves late, from the module geometry alone (no device, no kernel): the generator's
        delay times the sub-band count, plus the PQMF's ``K * stream_delay_columns`` for a multi-band model."""
        return cls._figures_of(model).latency_samples

    @classmethod
    def settle_frames_of(cls, model):
        """Frames after which a push has no edge of the utterance in any window or history and emits ``n * up``
        samples, from the module geometry alone: the plan's ``lookahead_settle_frames`` and ``latency_frames``."""
        return cls._figures_of(model).settle_frames

    @classmethod
    def min_frames_of(cls, model):
        """The shortest utterance: what reflection can pad (``layers.causal_conv.mirrored_min_frames`` of the plan)."""
        return cls._figures_of(model).min_frames

    @classmethod
    def state_bytes_of(cls, model, batch):
        """``state_bytes`` for ``batch`` streams or slots, from the plan's shapes alone (no device): both ping-pong halves
        of every launch's state and, for a multi-band model, of the PQMF history; fp32 in either precision."""
        return 2 * 4 * sum(b * ch * cols for b, ch, cols in cls._figures_of(model, int(batch)).state_shapes)


class _HiFiGANFamily(_Family):
    """The standard NON-causal ``HiFiGANGenerator`` (``LookaheadStream``, ``StreamPool``)."""

    @classmethod
    def _figures_of(cls, model, batch=1):
        return cls._conv_plan_figures(model, model.lookahead_plan(), None, batch)

    @classmethod
    def _streamable(cls, model, batch, columns, precision):
        from ..models import HiFiGANGenerator

        name, pool = cls.__name__, cls._pooled
        if not isinstance(model, HiFiGANGenerator):
            raise ValueError(f"{name}: {model.__class__.__name__} is not supported (only the non-causal "
                             "HiFiGANGenerator; a non-causal MelGANGenerator streams " + ("in lock step " if pool else "")
                             + "through utils.MelGANLookaheadStream, a ParallelWaveGANGenerator through "
                             "utils.PWGLookaheadStream)")
        if model.use_causal_conv:
            raise ValueError(f"{name}: the model is causal (use_causal_conv=True) and streams "
                             + ("in lock step, without look-ahead," if pool else "without look-ahead")
                             + " through utils.CausalStream")
        out_channels = model.output_conv[1].out_channels
        if out_channels != 1:
            raise ValueError(f"{name}: the generator emits {out_channels} channels; "
                             + ("a slot returns one waveform" if pool else "the stream returns one waveform per stream")
                             + " (out_channels == 1)")
        cls._refuse_bf16_model(model, precision, "look-ahead stream")
        batch, columns = cls._checked_sizes(batch, columns)
        plan = model.lookahead_plan()  # ValueError: decreasing block delays, a layer without a causal form
        cls._require_plan(plan, batch, columns, precision)
        return cls._conv_plan_figures(model, plan, None, batch, columns)


class _MelGANFamily(_Family):
    """The standard NON-causal, reflect-padded ``MelGANGenerator``, multi-band included (``MelGANLookaheadStream``,
    ``MelGANStreamPool``).  fp32 only: ``_NO_BF16`` is what ``_checked_precision`` says."""

    _NO_BF16 = ("the mirrored form of the streaming kernel, which the reflect-padded layers run, does not exist with bf16 "
                "operands yet")

    @classmethod
    def _checked_model(cls, model):
        """The refusals that need no device, in order: the class, a causal model, the padding and the layer geometry (the
        plan), the sub-bands, a bf16 model -> ``(plan, pqmf or None)``."""
        from ..models import MelGANGenerator

        name = cls.__name__
        if not isinstance(model, MelGANGenerator):
            raise ValueError(f"{name}: {model.__class__.__name__} is not supported (only the non-causal MelGANGenerator; "
                             "HiFiGANGenerator streams through utils.LookaheadStream, ParallelWaveGANGenerator through "
                             "utils.PWGLookaheadStream)")
        try:
            plan = model.lookahead_plan()  # ValueError: causal, a pad other than reflection, an even kernel
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None
        pqmf = cls._checked_pqmf(model, plan[-1].conv.out_channels)
        cls._refuse_bf16_model(model, "fp32", "look-ahead stream of a reflect-padded model", has_bf16=False)
        return plan, pqmf

    @classmethod
    def _figures_of(cls, model, batch=1):
        return cls._conv_plan_figures(model, *cls._checked_model(model), batch)

    @classmethod
    def _streamable(cls, model, batch, columns, precision):
        plan, pqmf = cls._checked_model(model)
        batch, columns = cls._checked_sizes(batch, columns)
        cls._require_plan(plan, batch, columns, precision)
        figures = cls._conv_plan_figures(model, plan, pqmf, batch, columns)
        # a pool closes an utterance too short for reflection in end(): nothing of it may have left by then
        if cls._pooled and (figures.min_frames - 1) * figures.up > figures.latency_samples:  # (no recipe: a first layer
            # reaches less far than the whole generator)
            raise ValueError(f"{cls.__name__}: an utterance of {figures.min_frames - 1} frame(s), too short for "
                             f"reflection, would emit samples before its end is known (latency "
                             f"{figures.latency_samples} samples, {figures.up} per frame)")
        return figures


class _PWGFamily(_Family):
    """The standard NON-causal ``ParallelWaveGANGenerator`` (``PWGLookaheadStream``, ``PWGStreamPool``)."""

    @classmethod
    def _figures_of(cls, model, batch=1, columns=8, plan=None):
        from ..layers.causal_conv import pwg_lookahead_state_shapes

        plan = model.lookahead_plan() if plan is None else plan
        return _figures(model, plan, None, batch, columns, pwg_lookahead_state_shapes(plan, batch))

    @classmethod
    def _streamable(cls, model, batch, columns, precision):
        from ..layers.causal_conv import pointwise_desc
        from ..models import HiFiGANGenerator, ParallelWaveGANGenerator

        name, pool = cls.__name__, cls._pooled
        if not isinstance(model, ParallelWaveGANGenerator):
            other = "pools through utils.StreamPool" if pool else "streams through utils.LookaheadStream"
            hint = f"; the non-causal HiFiGANGenerator {other}" if isinstance(model, HiFiGANGenerator) else ""
            raise ValueError(f"{name}: {model.__class__.__name__} is not supported (only the non-causal "
                             f"ParallelWaveGANGenerator{hint})")
        batch, columns = cls._checked_sizes(batch, columns)
        reason = model.lookahead_unsupported_reason(batch, precision)
        if reason is not None:
            raise ValueError(f"{name}: {reason}")
        if model.in_channels != 1 or model.out_channels != 1:
            raise ValueError(f"{name}: in_channels / out_channels = {model.in_channels} / {model.out_channels} ("
                             + ("a slot takes one noise row and returns one waveform" if pool else
                                "the stream takes one noise row and emits one waveform per stream") + ")")
        cls._refuse_bf16_model(model, precision, "look-ahead stream")
        plan = model.lookahead_plan()
        # a bf16 stream never runs a convolution the bf16 kernel refuses in fp32 instead; a pool asks in fp32 too
        if precision == "bf16" or pool:
            delayed = conv1d_stream_bf16_delayed_supported if precision == "bf16" else conv1d_stream_delayed_supported
            for launch in plan:
                if launch.kind == "conv_in":
                    desc = model.upsample_net._lookahead_desc(batch, columns)
                elif launch.kind in ("first_conv", "last_conv"):
                    desc = pointwise_desc(launch.module, batch, columns * launch.rate)
                else:
                    continue
                cls._require_supported(delayed(desc), launch.module, " with bf16 operands" if precision == "bf16" else "")
        return cls._figures_of(model, batch, columns, plan)


class _LookaheadStream(_Stream):
    """The look-ahead streams' core: what streaming a NON-causal generator with a fixed look-ahead is, whatever the
    model.  Every layer runs in its causal form on a shifted time axis (``model.lookahead_plan()`` lists the launches and
    their delays), so a push of ``n`` frames costs ``n`` frames of work and every sample leaves ``latency_samples`` late
    (``latency_frames``: the ceiling in frames).

    Emission rule: after any push the samples emitted total ``max(0, frames_in * up - latency_samples)``, so the first
    pushes of an utterance return short or empty tensors; ``flush()`` returns the tail, after which the emissions total
    ``frames * up`` samples; ``reset()`` starts the next utterance.  ``close()`` does not flush: an unflushed tail is
    dropped.  Any partition of the same inputs gives bit-identical audio, equal to the whole-utterance forward up to fp32
    summation order.  Of ``latency_samples`` the generator's own delay (``_front``) stands in front of the audio in the
    late stream; a multi-band model's PQMF synthesis holds the rest (``_hold``) back behind the newest column.

    State (``state_bytes``: both ping-pong halves): what the plan's launches keep -- histories and delay lines.
    ``use_graph``: a captured graph has fixed window arguments, so a push replays the two graphs of its chunk size, as in
    :class:`CausalStream`, only if no launch has an edge of the utterance in its window or history and nothing is trimmed
    from its emission: ``settle_frames`` frames went before it (``latency_frames``, or more for a reflect-padded plan).
    Earlier pushes and ``flush()`` run eagerly.  ``flush()`` refuses an utterance shorter than ``min_frames`` (1, or what
    reflection needs), which the whole-utterance forward cannot pad either.

    ``precision``: of the stream, fixed for its life (``.precision``); as in :class:`CausalStream` it neither reads nor
    writes the modules' own ``precision`` attributes, every launch of every push, the eager pushes and ``flush()``
    included, runs in it, and plan, latency, state and partition invariance do not depend on it.  ``None`` and ``"fp32"``
    are the fp32 stream, which refuses a model that ``set_inference_precision`` put in bf16 mode.

    A subclass names its family (:class:`_Family`: the model's checks in its own order, the plan, the figures) and
    supplies ``_run`` and ``_run_tail``, what ``flush`` feeds; the ones here run a convolution plan (HiFi-GAN, MelGAN)."""

    warmup_frames = 1
    _takes_noise = False  # does ``push`` take noise beside the features
    _keeps_last = False   # does ``flush`` replicate the last frame pushed (``_last``)

    def __init__(self, model, use_graph, normalize_before, precision, figures):
        """``figures``: the family's ``_streamable(model, batch, None, precision)``.  The PQMF history of a multi-band
        model rides behind the plan's state in both halves."""
        pqmf = figures.pqmf
        self.precision = precision
        self.up = figures.up  # samples per frame
        self._plan = figures.plan
        self._pqmf = pqmf
        self._hold = pqmf.stream_delay_columns * pqmf.subbands if pqmf is not None else 0
        self._front = figures.latency_samples - self._hold
        self.latency_samples = figures.latency_samples
        self.latency_frames = -(-self.latency_samples // self.up)
        self.settle_frames = figures.settle_frames
        self.min_frames = figures.min_frames
        super().__init__(model, [], figures.batch, use_graph, normalize_before, figures.state_shapes)

    def reset(self):
        """Back to start of stream; an unflushed tail is dropped."""
        self._restart()
        self._flushed = False
        self._last = None  # the last frame pushed, (batch, 1, C), where the flush replicates it (``_keeps_last``)

    def _positions(self, frames_before, n):
        """``(first, count)``: the samples of the whole late stream (``_front`` zeros, then the utterance) that a push of
        ``n`` frames after ``frames_before`` completes -- all of its ``n * up`` for a full-band model, those ``_hold``
        behind the newest column for a multi-band one."""
        first = max(0, frames_before * self.up - self._hold)
        return first, max(0, (frames_before + n) * self.up - self._hold) - first

    def _walk_run(self, c, state_in, state_out, frames_before, total_frames):
        """``c``: (batch, C, n) features, normalised, through the convolution plan and the PQMF."""
        from ..layers.causal_conv import LookaheadWalk

        k = len(state_out) - (self._pqmf is not None)  # (a multi-band stream's halves end with the PQMF's history)
        walk = LookaheadWalk(self._plan, None if state_in is None else state_in[:k], state_out[:k], frames_before,
                             total_frames, self.precision)
        y = self.model.walk_forward(c, walk)
        if self._pqmf is None:
            return y.reshape(self.batch, -1)
        n_emit = y.shape[-1] if frames_before is None else \
            self._positions(frames_before, c.shape[-1])[1] // self._pqmf.subbands
        return self._pqmf.stream_synthesis(y, None if state_in is None else state_in[-1], state_out[-1], n_emit)

    def _run(self, feats, state_in, state_out, frames_before=None):
        """The inputs of one push; ``state_in`` (None: start of stream) / ``state_out``: one ping-pong half each;
        ``frames_before`` None: steady state.  -> (batch, samples): the positions of the whole late stream this push
        completes, not yet trimmed."""
        return self._walk_run(self._features(feats), state_in, state_out, frames_before, None)

    def _run_tail(self, state_in, state_out, total):
        """``_run`` on what ``flush`` feeds after an utterance of ``total`` frames, with the end-of-utterance windows:
        ``latency_frames`` zero frames (normalised: the whole-utterance padding; a reflect-padded first layer mirrors at
        the utterance's last frame, so it never reads them)."""
        zeros = torch.zeros((self.batch, self._plan[0].conv.in_channels, self.latency_frames), device=self._device)
        return self._walk_run(zeros, state_in, state_out, total, total)

    @torch.no_grad()
    def push(self, feats, noise=None):
        """feats: (n, C) or (batch, n, C) float features; noise, for a stream that takes it (Parallel WaveGAN):
        (batch, n * up) or (n * up,) (the same for every stream) for the samples of THESE frames, undelayed, drawn with
        ``torch.randn`` on the device if omitted -> (batch, samples) fp32, the samples that became complete: ``n * up``
        once ``latency_samples`` are behind, fewer (or none) before.  The result is the caller's own tensor."""
        if noise is not None and not self._takes_noise:
            raise TypeError(f"{type(self).__name__}.push takes no noise")
        if self._flushed:
            raise RuntimeError(f"{type(self).__name__}.push: the utterance was flushed; reset() starts the next one")
        feats = self._coerce(feats)
        n = feats.shape[1]
        z = (self._coerce_noise(noise, n),) if self._takes_noise else ()
        if n == 0:
            return self._empty()
        before = self.frames_in
        self.frames_in += n
        if self._keeps_last:
            self._last = feats[:, -1:, :].clone()
        steady = before >= self.settle_frames  # no edge in reach, nothing to trim
        skip = 0 if steady else max(0, self._front - self._positions(before, n)[0])  # samples in front of the first one
        return self._push_step(feats, z, lambda *a: self._run(*a, before)[:, skip:].contiguous(),
                               self.use_graph and steady)

    @torch.no_grad()
    def flush(self):
        """End of the utterance: ``latency_frames`` more frames (``_run_tail``) with the end-of-utterance windows --
        every launch stores zeros past the utterance's last column, as the whole-utterance padding is, and a multi-band
        model's PQMF tail drains with them -> the last ``min(latency_samples, frames * up)`` samples, (batch, samples).
        Zero-length before anything was pushed and on a second call.  RuntimeError for an utterance shorter than
        ``min_frames``.  The next utterance starts with ``reset()``."""
        if not self._started or self._flushed:
            return self._empty()
        total = self.frames_in
        if total < self.min_frames:
            raise RuntimeError(f"{type(self).__name__}.flush: the utterance has {total} frame(s); reflection padding needs "
                               f"at least {self.min_frames} (the whole-utterance forward cannot pad a shorter one either)")
        y = self._run_tail(self._halves[self._cur], self._halves[1 - self._cur], total)
        first = self._positions(total, self.latency_frames)[0]
        y = y[:, max(0, self._front - first):self._front + total * self.up - first].contiguous()
        self._flushed = True  # (the halves are not swapped: nothing may follow but reset())
        self.samples_out += y.shape[1]
        return y


class LookaheadStream(_HiFiGANFamily, _LookaheadStream):
    """Stateful streaming synthesis for the standard NON-causal ``HiFiGANGenerator`` (symmetric ``Conv1d``,
    ``ConvTranspose1d(padding = s//2 + s%2)``: every recipe and released checkpoint) with a fixed look-ahead.  Interface,
    emission rule, graph rule, ``flush`` / ``close`` and the precision's scope: :class:`_LookaheadStream`.
    ``latency_samples`` is 3258 (12.73 frames) for HiFi-GAN V1; ``settle_frames == latency_frames``, ``min_frames == 1``.

    How: csrc/conv1d_stream.hip, the delayed form.  A tensor of the network is a stream with a delay:
    a symmetric convolution adds its padding, a transposed one multiplies by its stride and adds its padding; the
    residual input of a unit and the MRF running sum are older than the launch that adds them and go through delay
    lines; every launch stores exact zeros outside the utterance, which is what the next layer's zero padding is.

    State: per convolution the last ``(k - 1) * d`` columns of its raw input (one for a transposed layer) and the delay
    lines of its addends.  ``precision="bf16"``: every convolution runs with bf16 operands (csrc/conv1d_stream_bf16.hip,
    the delayed form; DESIGN.md s11.5: the activated window and the weights are rounded to bf16; sums, epilogues,
    addends, tensors, history and delay lines stay fp32).
    """

    def __init__(self, model, batch=1, use_graph=True, normalize_before=False, precision=None):
        precision = self._checked_precision(precision)
        super().__init__(model, use_graph, normalize_before, precision, self._streamable(model, batch, None, precision))


class MelGANLookaheadStream(_MelGANFamily, _LookaheadStream):
    """Stateful streaming synthesis for the standard NON-causal ``MelGANGenerator`` (reflect padding: every recipe and
    released checkpoint, ``multi_band_melgan.v2`` included) with a fixed look-ahead.  Interface, emission rule, graph
    rule and ``flush`` / ``close``: :class:`_LookaheadStream`; the whole-utterance forward is ``forward`` /
    ``inference``.  ``latency_samples`` is 1425 (5.6 frames) for ``melgan.v1``, 2720 (10.6 frames) for the LJSpeech
    ``multi_band_melgan.v2`` (scales ``[8, 4, 2]``) and 4208 (14.0 frames) for its 24 kHz variants (``[5, 5, 3]``).

    How: a reflect-padded layer of padding ``p`` produces output column ``q`` once input column
    ``q + p`` has arrived, and by then the columns reflection reads at either edge have arrived too; its launch
    (csrc/conv1d_stream.hip, the mirrored form) reads its window through a mirror at the edges of the input's valid
    window, while the history keeps the raw stored zeros.  The transposed and 1 x 1 convolutions run the delayed form
    unchanged; a residual stack is three launches, the skip branch going through a delay line.

    Multi-band (``model.pqmf`` attached, ``out_channels == pqmf.subbands``): the sub-band columns of a push go through
    ``PQMF.stream_synthesis`` in the same push, as in :class:`CausalStream` -- the stored zeros around the utterance are
    the zero padding the whole-utterance synthesis applies -- and ``latency_samples`` = generator delay * K + the PQMF's
    ``K * stream_delay_columns``.  ``flush()`` drains that tail too.

    ``settle_frames``: ``frames_before * rate >= delay + pad`` for every launch, and ``latency_frames``.  The frames
    ``flush()`` feeds are dummies: the first layer mirrors at the utterance's end.  ``min_frames``: 4 for a first layer
    of kernel 7.  ``precision`` may be ``None`` or ``"fp32"``: the mirrored form has no bf16 form yet.
    """

    def __init__(self, model, batch=1, use_graph=True, normalize_before=False, precision=None):
        precision = self._checked_precision(precision, self._NO_BF16)
        figures = self._streamable(model, batch, None, precision)
        self.pqmf = figures.pqmf
        self.subbands = figures.plan[-1].conv.out_channels
        super().__init__(model, use_graph, normalize_before, precision, figures)


class PWGLookaheadStream(_PWGFamily, _LookaheadStream):
    """Stateful streaming synthesis for the standard NON-causal ``ParallelWaveGANGenerator`` (every recipe and released
    checkpoint) with a fixed look-ahead; ``push`` also takes, optionally, the noise for the samples of its frames, and
    the whole-utterance forward is ``model.inference``.  Interface, emission rule, graph rule, ``flush`` / ``close`` and
    the precision's scope: :class:`_LookaheadStream`.  ``latency_samples`` is 3921 (15.3 frames) for
    ``parallel_wavegan.v1``; ``settle_frames == latency_frames``, ``min_frames == 1``.

    How: ``conv_in`` is ``w`` frames late and starts from its first frame replicated; an upsampling
    stage of scale ``s`` takes a delay ``D`` to ``D * s + s``; the noise waits in a delay line for the conditioning; a
    gated layer of dilation ``d`` adds ``d`` columns, takes its residual from the middle tap, reads the conditioning from
    one shared line at its own delay and the running skip sum through a line of ``d`` columns
    (csrc/wavenet_stream.hip, the delayed form; one launch per layer); every launch stores exact zeros outside the
    utterance.  ``model.lookahead_plan()`` lists the launches, delays and state.

    State: the layers' histories (``2 d`` columns each), their skip lines, the conditioning line (``sum d`` columns of 80
    rows), the noise line and the upsampler's few columns -- about 3.3 MB per half and stream for V1.  Noise is never
    drawn inside a graph.  ``flush()`` feeds ``latency_frames`` copies of the last frame (what ``inference()``'s
    replicate padding gives ``conv_in`` on the right) with zero noise.

    ``precision="bf16"``: ``conv_in``, the 1 x 1 convolutions and the gated layers run with bf16 operands
    (csrc/conv1d_stream_bf16.hip and csrc/wavenet_stream_bf16.hip, the delayed forms; DESIGN.md s11.7: windows, weights
    and the gate output are rounded to bf16; sums, the gate, biases, residual, skip sum, tensors, history and lines stay
    fp32; the stretch stages and the delay lines stay fp32).
    """

    _takes_noise = _keeps_last = True

    def __init__(self, model, batch=1, use_graph=True, normalize_before=False, precision=None):
        precision = self._checked_precision(precision)
        super().__init__(model, use_graph, normalize_before, precision, self._streamable(model, batch, None, precision))

    def _run(self, feats, z, state_in, state_out, frames_before=None, total_frames=None):
        """``feats``: (batch, n, C) features; ``z``: (batch, 1, n * up) noise; the rest as in the core."""
        from ..layers.causal_conv import PWGLookaheadWalk

        walk = PWGLookaheadWalk(self._plan, state_in, state_out, frames_before, total_frames, self.precision)
        return self.model.lookahead_forward(z, self._features(feats), walk).reshape(self.batch, -1)

    def _run_tail(self, state_in, state_out, total):
        feats = self._last.expand(-1, self.latency_frames, -1).contiguous()
        zeros = torch.zeros((self.batch, 1, self.latency_frames * self.up), device=self._device)
        return self._run(feats, zeros, state_in, state_out, total, total)


# ---- a pool of look-ahead streams whose utterances start and end independently -------------------

def slot_window(delay, rate, t_out, before, left=None):
    """The window rule of the slotted stream kernel (``stream_slot_window``, csrc/stream_common.h), restated: the valid
    columns ``(lo, hi)`` of a launch ``delay`` columns late at ``rate`` columns per frame, on a push of ``t_out`` columns
    that ``before`` frames went before; ``left``: frames of the utterance from this push's first frame on (negative past
    its end), None while unknown.  ``layers.causal_conv.lookahead_window`` with ``left = total_frames - frames_before``."""
    lo = min(max(delay - before * rate, 0), t_out)
    hi = t_out if left is None else min(max(delay + left * rate, 0), t_out)
    return lo, hi


STREAM_MAX_TILE_COLUMNS = 64  # kStreamMaxNt (csrc/stream_common.h): the widest column tile of the streaming kernel


def slot_mirror_window(delay, pad, rate, n, before, left=None):
    """The input edges of one item of a slotted-mirrored launch (``StreamSlots::mirrored_at``, csrc/stream_common.h),
    restated, saturation included: a reflect-padded layer of padding ``pad`` (history ``2 * pad``) whose OUTPUT is
    ``delay`` columns late at ``rate`` columns per frame, on a chunk of ``n`` columns that ``before`` frames went before;
    ``left`` as in :func:`slot_window`.  The input is ``delay - pad`` columns late, so it is valid on ``[delay - pad -
    before * rate, delay - pad + left * rate)``, unbounded on the right while ``left`` is unknown; both edges are
    saturated to ``[-2 * pad, n + 64]`` (``mirror_bound``), which changes no column a window inside ``[-2 * pad, n)`` maps
    to.  -> ``(in_lo, in_hi)``, what ``ops.conv1d_stream_mirrored_forward`` takes as ``in_window`` for the item alone;
    its valid window is :func:`slot_window`'s, equal to ``(in_lo + pad, in_hi + pad)`` clamped to ``[0, n]``."""
    bound = lambda edge: max(-2 * pad, min(n + STREAM_MAX_TILE_COLUMNS, edge))  # noqa: E731
    in_delay = delay - pad
    return bound(in_delay - before * rate), (n + STREAM_MAX_TILE_COLUMNS if left is None else bound(in_delay + left * rate))


# What one slot does in one step of the pool.  ``action``: "empty" (no utterance: fresh and paused), "pause" (fewer
# than a chunk queued, not ended), "run" (a chunk of queued frames), "tail" (ended: what is left, zero-padded) or "drain"
# (ended: zero frames only); ``take``: queued frames it consumes; ``row``: its row of the kernels' table; ``emit``: the
# range of the step's ``chunk * up`` output samples that became complete; ``closes``: the utterance is done.
SlotStep = collections.namedtuple("SlotStep", "slot action take row emit closes")


class SlotSchedule:
    """The bookkeeping of :class:`StreamPool`, with no device in it: which slot holds an utterance, how many frames each
    has queued and taken, and what every slot does in a step -- its action, its row of the slotted kernels' table
    (``ops.conv1d_stream_slots_forward``) and the samples it emits.

    Emission follows ``_LookaheadStream``: after a step in which a slot has taken ``frames_in`` frames (padding and
    drain frames included) its emissions total ``clamp(frames_in * up - latency_samples, 0, frames * up)``, ``frames``
    being the utterance's length once it has ended.  The table's position saturates at ``settle_frames`` (past every
    delay of the plan) and the frames left at ``[-settle_frames, chunk]``, which changes no window and keeps the kernel's
    arithmetic small however long an utterance is."""

    def __init__(self, slots, chunk_frames, up, latency_samples, settle_frames):
        self.slots, self.chunk, self.up = int(slots), int(chunk_frames), int(up)
        self.latency, self.settle = int(latency_samples), max(int(settle_frames), 1)
        self._state = [None] * self.slots  # per slot None (free) or [queued, fed, ended, before]

    @property
    def open_slots(self):
        return [s for s, st in enumerate(self._state) if st is not None]

    def _of(self, slot, what):
        if not 0 <= slot < self.slots or self._state[slot] is None:
            raise RuntimeError(f"StreamPool.{what}: slot {slot} is not open")
        return self._state[slot]

    def open(self):
        for s, st in enumerate(self._state):
            if st is None:
                self._state[s] = [0, 0, False, 0]
                return s
        raise RuntimeError(f"StreamPool.open: all {self.slots} slots are taken")

    def feed(self, slot, n):
        st = self._of(slot, "feed")
        if st[2]:
            raise RuntimeError(f"StreamPool.feed: slot {slot} was ended")
        st[0] += n
        st[1] += n

    def end(self, slot):
        st = self._of(slot, "end")
        st[2] = True
        if st[1] == 0:  # an empty utterance emits nothing
            self._state[slot] = None

    def reset(self):
        self._state = [None] * self.slots

    def advance(self):
        """The next step: one :class:`SlotStep` per slot, or ``[]`` (and no change) if no slot runs."""
        from ..ops import SLOT_LEFT_KNOWN, SLOT_PAUSED

        steps, runs = [], False
        for s, st in enumerate(self._state):
            if st is None:
                steps.append(SlotStep(s, "empty", 0, (0, 0, SLOT_PAUSED, 0), (0, 0), False))
                continue
            queued, fed, ended, before = st
            position = min(before, self.settle)
            if queued < self.chunk and not ended:
                steps.append(SlotStep(s, "pause", 0, (position, 0, SLOT_PAUSED, 0), (0, 0), False))
                continue
            runs = True
            take = min(queued, self.chunk)
            cap = fed * self.up if ended else None
            lo, hi = (max(0, frames * self.up - self.latency) for frames in (before, before + self.chunk))
            if ended:
                lo, hi = min(lo, cap), min(hi, cap)
            left = max(-self.settle, min(fed - before, self.chunk)) if ended else 0
            action = "run" if take == self.chunk else ("tail" if take else "drain")
            offset = self.latency - before * self.up  # the step's sample 0 is the late stream's before * up
            steps.append(SlotStep(s, action, take, (position, left, SLOT_LEFT_KNOWN if ended else 0, take),
                                  (lo + offset, hi + offset), ended and hi == cap))
        if not runs:
            return []
        for step in steps:
            if step.closes:
                self._state[step.slot] = None
            elif step.action in ("run", "tail", "drain"):
                st = self._state[step.slot]
                st[0] -= step.take
                st[3] += self.chunk
        return steps


class _SlotPool(_Stream):
    """What the pools share (:class:`StreamPool`, :class:`PWGStreamPool`): the schedule, the per-slot host queues and
    ``_take``, what a step uploads -- the table first, then the model's inputs, each a device tensor with two pinned
    twins used in turn (a twin is written again only after its copy of two steps ago has finished) --, the graph entry
    (ONE pair of graphs, from the first step on) and the step loop.  A subclass names its family (:class:`_Family`),
    calls ``__init__`` with the family's figures and the shapes of its inputs, and supplies ``_fill(steps, table,
    *hosts)``, which writes a step's pinned twins, and ``_run(*inputs, state_in, state_out)``, the model on the device
    inputs behind the table; ``_before_run(steps)`` is what a step does on the device between the upload and the launches
    (nothing here)."""

    _pooled = True

    def __init__(self, model, use_graph, normalize_before, precision, figures, table_rows, input_shapes):
        """``figures``: the family's ``_streamable(model, slots, chunk_frames, precision)``; ``table_rows``: rows of the
        device table (``slots``, or twice that where a second table rides behind the first); ``input_shapes``: of the
        device inputs behind the table, the features first."""
        from ..ops import SLOT_INTS

        self.precision = precision
        self.slots, self.chunk_frames = figures.batch, figures.columns
        self._plan = figures.plan
        self.up = figures.up
        self.latency_samples = figures.latency_samples
        self.settle_frames, self.min_frames = figures.settle_frames, figures.min_frames
        self._schedule = SlotSchedule(self.slots, self.chunk_frames, self.up, self.latency_samples, self.settle_frames)
        super().__init__(model, [], self.slots, use_graph, normalize_before, figures.state_shapes)
        self._table = torch.zeros((table_rows, SLOT_INTS), device=self._device, dtype=torch.int32)
        self._inputs = [torch.zeros(shape, device=self._device) for shape in input_shapes]
        self._feats = self._inputs[0]
        self._staging = [(torch.zeros((table_rows, SLOT_INTS), dtype=torch.int32).pin_memory(),
                          *(torch.zeros(shape).pin_memory() for shape in input_shapes), torch.cuda.Event())
                         for _ in range(2)]

    @classmethod
    def _checked_sizes(cls, slots, chunk_frames):
        slots, chunk_frames = int(slots), int(chunk_frames)
        if slots < 1:
            raise ValueError(f"{cls.__name__}: slots must be >= 1")
        if chunk_frames < 1:
            raise ValueError(f"{cls.__name__}: chunk_frames must be >= 1")
        return slots, chunk_frames

    @property
    def open_slots(self):
        """The ids that hold an utterance, ascending."""
        return self._schedule.open_slots

    @property
    def graphs_captured(self):
        """How many graphs the pool holds: 0, or 2 (both directions of its one chunk size)."""
        return sum(len(graphs) for graphs in self._graphs.values())

    def reset(self):
        """Closes every slot, dropping what is queued; the state needs no clearing (a new utterance is fresh)."""
        self._restart()
        self._queues = [[] for _ in range(self.batch)]
        self._step = 0
        self._schedule.reset()

    def open(self):
        return self._schedule.open()

    def end(self, slot):
        self._schedule.end(slot)

    def _checked_frames(self, frames):
        """What ``feed`` takes -> (n, C) fp32 on the host."""
        frames = torch.as_tensor(frames, dtype=torch.float32).cpu()
        if frames.dim() != 2 or frames.shape[1] != self._feats.shape[2]:
            raise ValueError(f"{type(self).__name__}.feed: expected (n, {self._feats.shape[2]}) features, got "
                             f"{tuple(frames.shape)}")
        return frames

    @staticmethod
    def _take_from(queue, n, out):
        """Moves the next ``n`` queued rows of ``queue`` (a list of host tensors) into ``out[:n]`` and zeros the rest."""
        at = 0
        while at < n:
            head = queue[0]
            k = min(n - at, head.shape[0])
            out[at:at + k] = head[:k]
            at += k
            if k == head.shape[0]:
                queue.pop(0)
            else:
                queue[0] = head[k:]
        if n < out.shape[0]:
            out[n:] = 0.0

    def _take(self, slot, n, out):
        """Moves the next ``n`` queued frames of ``slot`` into ``out[:n]`` and zeros the rest of ``out``."""
        self._take_from(self._queues[slot], n, out)

    def _before_run(self, steps):
        """On the device, after the upload and outside the graph."""

    @torch.no_grad()
    def step(self):
        steps = self._schedule.advance()
        if not steps:
            return {}
        *hosts, copied = self._staging[self._step % 2]
        self._step += 1
        copied.synchronize()
        self._fill(steps, *hosts)
        for device, host in zip([self._table] + self._inputs, hosts):
            device.copy_(host, non_blocking=True)
        copied.record()
        self._before_run(steps)
        state_in, state_out = self._halves[self._cur], self._halves[1 - self._cur]
        if self.use_graph:
            graphs = self._graph_entry("pool", lambda: _capture_directions(
                self._halves, lambda hist_in, hist_out: self._run(*self._inputs, hist_in, hist_out)))
            graph, static_out = graphs[self._cur]
            graph.replay()
            y = static_out.clone()
        else:
            y = self._run(*self._inputs, state_in, state_out)
        self._cur = 1 - self._cur
        out = {}
        for st in steps:
            if st.action in ("run", "tail", "drain"):
                out[st.slot] = y[st.slot, st.emit[0]:st.emit[1]]
                self.frames_out += self.chunk_frames
                self.samples_out += st.emit[1] - st.emit[0]
        return out


class _FeaturePool(_SlotPool):
    """What the pools of the generators that take features alone share (:class:`StreamPool`, :class:`MelGANStreamPool`):
    a step uploads the table and the features, the tail's padding frames are zeros after normalisation, and the model
    runs its convolution plan through a ``SlotWalk``; the PQMF history of a multi-band model rides behind the plan's
    state."""

    def __init__(self, model, use_graph, normalize_before, precision, figures):
        self._pqmf = figures.pqmf
        super().__init__(model, use_graph, normalize_before, precision, figures, figures.batch,
                         [(figures.batch, figures.columns, figures.plan[0].conv.in_channels)])
        self._columns = torch.arange(self.chunk_frames, device=self._device).reshape(1, 1, -1)

    def feed(self, slot, frames):
        frames = self._checked_frames(frames)
        self._schedule.feed(slot, frames.shape[0])
        self.frames_in += frames.shape[0]
        if frames.shape[0]:
            self._queues[slot].append(frames)

    def _fill(self, steps, table, feats):
        table.copy_(torch.tensor([st.row for st in steps], dtype=torch.int32))
        for st in steps:
            if st.action in ("run", "tail", "drain"):
                self._take(st.slot, st.take, feats[st.slot])

    def _walk_run(self, feats, state_in, state_out):
        """The generator on one step's inputs, every launch slotted -> (slots, rows, chunk_frames * rate)."""
        from ..layers.causal_conv import SlotWalk

        c = self._features(feats)
        if self.normalize_before:  # the padding frames are zeros AFTER normalisation (row[3]: the real frames)
            c.masked_fill_(self._columns >= self._table[:, 3].reshape(-1, 1, 1), 0.0)
        walk = SlotWalk(self._plan, state_in, state_out, self._table, self.precision)
        return self.model.walk_forward(c, walk)

    def _run(self, feats, state_in, state_out):
        """The generator on one step's inputs, then the slotted PQMF synthesis of a multi-band model -> (slots,
        chunk_frames * up)."""
        if self._pqmf is None:
            return self._walk_run(feats, state_in, state_out).reshape(self.batch, -1)
        y = self._walk_run(feats, state_in[:-1], state_out[:-1])
        return self._pqmf.stream_synthesis_slots(y, state_in[-1], state_out[-1], self._table)


class StreamPool(_HiFiGANFamily, _FeaturePool):
    """``slots`` look-ahead streams of the standard NON-causal ``HiFiGANGenerator`` in one batch, whose utterances start
    and end whenever they like: what :class:`LookaheadStream` does for ``batch`` lock-step streams, for a server
    (:class:`PWGStreamPool` is the same for the non-causal ``ParallelWaveGANGenerator``).

    ``open()`` -> a free slot id (RuntimeError when every slot is taken); ``feed(slot, frames)`` queues ``(n, C)``
    features, any ``n >= 0``, on the host; ``end(slot)``: no more frames.  ``step()`` is ONE set of launches over all
    slots -> ``{slot: (samples,) fp32}`` for every slot that ran, the samples that became complete (views of one tensor
    that is the caller's own).  In a step a slot with ``chunk_frames`` queued runs on them; one with fewer, not ended, is
    paused (its state stays, it emits nothing); an ended one runs on what is left, padded with zero frames (inserted
    after normalisation, as ``flush()`` does; the kernels know the remaining length), then on zero chunks until it has
    emitted ``frames * up`` samples, and closes: its id leaves ``open_slots`` and is free again.  An utterance ended
    without frames closes at once.  If no slot runs, ``step()`` returns ``{}`` and launches nothing.  A slot's
    concatenated emissions are bit for bit what ``LookaheadStream(model, batch=1)`` emits for the same frames, pushes
    and flush together; ``latency_samples`` is that class's.

    How: every launch is the slotted form of the streaming kernel (csrc/conv1d_stream.hip), which
    reads each item's position from a small device table -- frames before, frames left, paused -- and derives the
    item's window itself; a slot taken for a new utterance is fresh and reads none of the old state.  A step uploads the
    table and the features (two copies from pinned memory), so ``use_graph`` captures ONE pair of graphs (A -> B, B -> A)
    and replays it from the first step on: start, steady state and tail are the same launches.  ``precision``,
    ``normalize_before`` and the refusals are :class:`LookaheadStream`'s; ``reset()`` closes every slot."""

    def __init__(self, model, slots=16, chunk_frames=8, use_graph=True, normalize_before=False, precision=None):
        precision = self._checked_precision(precision)
        super().__init__(model, use_graph, normalize_before, precision,
                         self._streamable(model, slots, chunk_frames, precision))


class MelGANStreamPool(_MelGANFamily, _FeaturePool):
    """``slots`` look-ahead streams of the standard NON-causal, reflect-padded ``MelGANGenerator``
    (``multi_band_melgan.v2`` included) in one batch, whose utterances start and end whenever they like: what
    :class:`MelGANLookaheadStream` does for ``batch`` lock-step streams, for a server.  The interface is
    :class:`StreamPool`'s -- ``open()``, ``feed(slot, frames)``, ``end(slot)``, ``step()`` -> ``{slot: (samples,) fp32}``,
    ``reset()``, ``open_slots``, ``graphs_captured``, ``latency_samples``, ``state_bytes`` -- and a slot's concatenated
    emissions are bit for bit what ``MelGANLookaheadStream(model, batch=1)`` emits for the same frames, pushes and flush
    together.  ``up = upsample_factor * K`` samples per frame, ``K`` the sub-bands (1: full-band).

    How: a reflect-padded launch runs the slotted-mirrored form of the streaming kernel
    (csrc/conv1d_stream.hip), which takes both edges of each item's input window from the table; the transposed and 1 x 1
    convolutions run the slotted form; a multi-band model's sub-bands go through the slotted PQMF synthesis
    (csrc/pqmf.hip) in the same step, which always emits one position per column -- the schedule's emission rule, with
    the generator's delay and the PQMF's as ``latency_samples``, picks the samples that are the utterance's.  While an
    utterance's length is unknown its columns stop short of the end by more than any padding, so no output that needs the
    right-hand mirror is computed before ``end(slot)`` has put the length into the table.  The padding frames of a tail
    are zeros after normalisation; the first layer mirrors at the utterance's end and never reads them.

    ``end(slot)`` on an utterance of fewer than ``min_frames`` frames (4 for a first layer of kernel 7; one without
    frames closes silently, as in :class:`StreamPool`) raises RuntimeError, as ``flush()`` does: the slot is closed and
    free again and has emitted nothing.  ``precision`` may be ``None`` or ``"fp32"``; ``normalize_before`` and the
    refusals are :class:`MelGANLookaheadStream`'s, for ``slots x chunk_frames``; ``reset()`` closes every slot."""

    def __init__(self, model, slots=16, chunk_frames=8, use_graph=True, normalize_before=False, precision=None):
        precision = self._checked_precision(precision, self._NO_BF16)
        figures = self._streamable(model, slots, chunk_frames, precision)
        self.pqmf = figures.pqmf
        self.subbands = figures.plan[-1].conv.out_channels
        super().__init__(model, use_graph, normalize_before, precision, figures)

    def end(self, slot):
        st = self._schedule._of(slot, "end")
        total = st[1]
        if 0 < total < self.min_frames:  # nothing of it was emitted: (min_frames - 1) * up <= latency_samples
            self._schedule._state[slot] = None
            self._queues[slot] = []
            raise RuntimeError(f"MelGANStreamPool.end: the utterance has {total} frame(s); reflection padding needs at "
                               f"least {self.min_frames} (the whole-utterance forward cannot pad a shorter one either); "
                               f"slot {slot} is closed and has emitted nothing")
        self._schedule.end(slot)


class PWGStreamPool(_PWGFamily, _SlotPool):
    """``slots`` look-ahead streams of the standard NON-causal ``ParallelWaveGANGenerator`` in one batch, whose
    utterances start and end whenever they like: what :class:`PWGLookaheadStream` does for ``batch`` lock-step streams,
    for a server.  The interface is :class:`StreamPool`'s -- ``open()``, ``feed(slot, frames, noise=None)``,
    ``end(slot)``, ``step()`` -> ``{slot: (samples,) fp32}``, ``reset()``, ``open_slots``, ``graphs_captured``,
    ``latency_samples``, ``state_bytes`` -- and a slot's concatenated emissions are bit for bit what
    ``PWGLookaheadStream(model, batch=1)`` emits for the same frames and noise, pushes and flush together.

    ``noise``: ``(n * up,)`` for the samples of the ``n`` frames of that ``feed`` (finite values); where none is given
    the pool draws it with ``torch.randn`` on the device, after the step's upload and never inside a graph.  Given and
    drawn noise may mix within a slot.  An ended slot runs on what is left, padded with copies of its last real frame
    (kept on the host; what ``flush()`` feeds) and zero noise, then on chunks of that frame until it has emitted
    ``frames * up`` samples; the padding is inserted before normalisation, as ``flush()`` does.

    How: every launch of a step is slotted -- the gated layers (csrc/wavenet_stream.hip,
    csrc/wavenet_stream_bf16.hip), the upsampling stages and the two delay lines (csrc/elementwise.hip), ``conv_in`` and
    the 1 x 1 convolutions (csrc/conv1d_stream.hip) -- and reads each item's position from the device table.  ``conv_in``
    starts an utterance from its first frame replicated: a seeding kernel writes that into the history of the fresh
    running items, and ``conv_in`` runs with ``delay + rate`` over a second table of rows ``(before + 1, left - 1,
    flags)``, which gives the same windows and in which no item is fresh; both tables go up in the one table upload.  A
    step uploads the tables, the features and the noise (three copies from pinned memory), so ``use_graph`` captures ONE
    pair of graphs and replays it from the first step on.  ``precision`` (scope: :class:`PWGLookaheadStream`; the state
    a bf16 pool writes is the fp32 pool's bit for bit), ``normalize_before`` and the refusals are
    :class:`PWGLookaheadStream`'s, for ``slots x chunk_frames``; ``reset()`` closes every slot."""

    def __init__(self, model, slots=16, chunk_frames=8, use_graph=True, normalize_before=False, precision=None):
        precision = self._checked_precision(precision)
        figures = self._streamable(model, slots, chunk_frames, precision)
        slots, chunk_frames, plan = figures.batch, figures.columns, figures.plan
        # conv_in with a context window keeps a history: the second table rides behind the first
        self._two_tables = plan[0].kind == "conv_in" and bool(plan[0].state)
        # what a step uploads: the table(s), the features and the noise
        super().__init__(model, use_graph, normalize_before, precision, figures, slots * (2 if self._two_tables else 1),
                         [(slots, chunk_frames, model.aux_channels), (slots, 1, chunk_frames * figures.up)])
        self._noise = self._inputs[1]

    def reset(self):
        super().reset()
        self._noise_queues = [[] for _ in range(self.batch)]
        self._last = [None] * self.batch  # per slot its last real frame, (C,), on the host

    def feed(self, slot, frames, noise=None):
        frames = self._checked_frames(frames)
        n = frames.shape[0]
        if noise is None:  # (NaN on the host: drawn on the device once it is uploaded)
            noise = torch.full((n * self.up,), float("nan"))
        else:
            noise = torch.as_tensor(noise, dtype=torch.float32).cpu().reshape(-1)
            if noise.shape[0] != n * self.up:
                raise ValueError(f"PWGStreamPool.feed: expected ({n * self.up},) noise for {n} frame(s), got "
                                 f"{tuple(noise.shape)}")
            if not torch.isfinite(noise).all():
                raise ValueError("PWGStreamPool.feed: the noise must be finite")
        self._schedule.feed(slot, n)
        self.frames_in += n
        if n:
            self._queues[slot].append(frames)
            self._noise_queues[slot].append(noise)

    def _fill(self, steps, table, feats, noise):
        from ..layers.causal_conv import slot_table_rows_in

        rows = [st.row for st in steps]
        table.copy_(torch.tensor(rows + (slot_table_rows_in(rows) if self._two_tables else []), dtype=torch.int32))
        for st in steps:
            if st.action in ("run", "tail", "drain"):
                self._take(st.slot, st.take, feats[st.slot])
                self._take_from(self._noise_queues[st.slot], st.take * self.up, noise[st.slot, 0])
                if st.take:
                    self._last[st.slot] = feats[st.slot, st.take - 1].clone()
                if st.take < self.chunk_frames:
                    feats[st.slot, st.take:] = self._last[st.slot]  # what flush() feeds: the last real frame

    def _before_run(self, steps):
        """Draws the noise nobody gave (NaN in the upload), on the device and outside the graph.  (One look at the whole
        staged buffer: a row a paused slot left there may ask for a draw nobody reads, never the other way round.)"""
        *_, noise, _ = self._staging[(self._step - 1) % 2]
        if bool(torch.isnan(noise).any()):
            self._noise.copy_(torch.where(torch.isnan(self._noise), torch.randn_like(self._noise), self._noise))

    def _run(self, feats, z, state_in, state_out):
        """The generator on one step's inputs, every launch slotted -> (slots, chunk_frames * up)."""
        from ..layers.causal_conv import PWGSlotWalk

        first, second = (self._table[:self.slots], self._table[self.slots:]) if self._two_tables else (self._table, None)
        walk = PWGSlotWalk(self._plan, state_in, state_out, first, second, self.precision)
        return self.model.lookahead_forward(z, self._features(feats), walk).reshape(self.batch, -1)


RaggedGroup = collections.namedtuple("RaggedGroup", "indices frames t_pad")
RaggedGroup.__doc__ = """One batched forward of :class:`RaggedSynthesizer`: ``indices`` -- which inputs ride in it, by item;
``frames`` -- frames per item, ``max_batch`` long (0: an unused item); ``t_pad`` -- the batch's length in frames."""
RaggedPlan = collections.namedtuple("RaggedPlan", "groups padded_fraction")


class _RaggedSynthesizer:
    """What :class:`RaggedSynthesizer`, :class:`MelGANRaggedSynthesizer` and :class:`PWGRaggedSynthesizer` share: the
    plan, one padded upload per group, one graph per ``(max_batch, T_pad)`` and the recapture when the parameters
    change.  A subclass checks its model, calls :meth:`_setup` and gives :meth:`_forward`."""

    max_graph_shapes = 4  # (max_batch, T_pad) shapes whose graphs are kept (least recently used evicted)
    precision = None

    def _setup(self, model, max_batch, bucket_frames, use_graph, channels, samples_per_frame, widest_row, min_frames=1,
               slack_frames=0):
        name = type(self).__name__
        self.max_batch, self.bucket_frames = int(max_batch), int(bucket_frames)
        if self.max_batch < 1 or self.bucket_frames < 1:
            raise ValueError(f"{name}: max_batch and bucket_frames must be >= 1")
        _require_device(next(model.parameters()))  # no CPU fallback
        self.model = model.eval()
        self.use_graph = bool(use_graph)
        self.up = int(samples_per_frame)
        self.channels = int(channels)
        self.min_frames, self.slack_frames = int(min_frames), int(slack_frames)
        self.max_frames = (2 ** 31 - 1) // int(widest_row) - self.slack_frames  # 32-bit element counts per item
        self._device = next(model.parameters()).device
        self._watch = GraphedInference(model)  # (only its parameter-state key is used)
        self._state = None
        self._graphs = collections.OrderedDict()
        self.captures = 0  # graphs captured since construction

    @property
    def graphs_captured(self):
        """How many graphs are held now."""
        return len(self._graphs)

    @staticmethod
    def plan_groups(lengths, max_batch=16, bucket_frames=64, max_frames=None, min_frames=1, slack_frames=0,
                    who="RaggedSynthesizer"):
        """Pure host logic: ``lengths`` (frames per utterance) -> ``RaggedPlan(groups, padded_fraction)``.  The
        utterances are sorted by length (ties in input order) and cut into groups of ``max_batch``; a group's ``t_pad`` is
        its longest length + ``slack_frames`` (the room a reflect-padded model's mirror columns need behind an item,
        DESIGN.md s9.5) rounded up to ``bucket_frames``; a last, partial group is filled with items of 0 frames.
        ``padded_fraction``: the share of all ``max_batch * t_pad`` frame slots that hold no frame.  ValueError for an
        empty item, for one shorter than ``min_frames`` and for one longer than ``max_frames``."""
        lengths = [int(n) for n in lengths]
        for i, n in enumerate(lengths):
            if n < 1:
                raise ValueError(f"{who}: item {i} is empty ({n} frames)")
            if n < min_frames:
                raise ValueError(f"{who}: item {i} has {n} frames, fewer than reflection can pad ({min_frames})")
            if max_frames is not None and n > max_frames:
                raise ValueError(f"{who}: item {i} has {n} frames, more than one forward holds ({max_frames}; "
                                 "utils.ChunkedSynthesizer cuts long utterances)")
        order = sorted(range(len(lengths)), key=lambda i: lengths[i])
        groups, slots = [], 0
        for at in range(0, len(order), max_batch):
            idx = order[at:at + max_batch]
            t_pad = -(-(lengths[idx[-1]] + slack_frames) // bucket_frames) * bucket_frames
            groups.append(RaggedGroup(tuple(idx), tuple(lengths[i] for i in idx) + (0,) * (max_batch - len(idx)), t_pad))
            slots += max_batch * t_pad
        return RaggedPlan(groups, 1.0 - sum(lengths) / slots if slots else 0.0)

    def plan(self, lengths):
        """:meth:`plan_groups` with this synthesizer's ``max_batch``, ``bucket_frames``, ``max_frames``, ``min_frames``
        and ``slack_frames``."""
        return self.plan_groups(lengths, self.max_batch, self.bucket_frames, self.max_frames, self.min_frames,
                                self.slack_frames, type(self).__name__)

    def _forward(self, c, frames, *noise):
        """The ragged forward of one group -> (max_batch, 1, T_pad * up), whatever it holds past an item's end.
        ``noise``: the one extra input of a model that takes one (Parallel WaveGAN), else nothing."""
        raise NotImplementedError

    def _capture(self, *inputs):
        statics = tuple(t.clone() for t in inputs)  # (c, frames) and, for a model that takes it, the noise
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):  # fills the weight caches / sets kernel attributes outside the capture
                self._forward(*statics)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_out = self._forward(*statics)
        self.captures += 1
        return graph, statics, static_out

    def _run(self, c, frames, noise=None, draw=False):
        """The ragged forward of one group -> (max_batch, 1, T_pad * up); in graph mode the graph's own output buffer.
        ``noise``: the extra input of a model that takes one; ``draw``: its values are not given -- standard normal noise
        is drawn on the device into it (in graph mode into the graph's static buffer, before the replay and outside
        the graph)."""
        inputs = (c, frames) if noise is None else (c, frames, noise)
        if not self.use_graph:
            if draw:
                noise.normal_()
            return self._forward(*inputs)
        from .precision import inference_precision

        with inference_precision(self.model, self.precision):
            state = self._watch._param_state()
        if state != self._state:
            self._graphs.clear()  # the parameters changed: a replay would use the old weight images
            self._state = state
        key = tuple(c.shape)
        entry = self._graphs.pop(key, None)
        if entry is None:
            while len(self._graphs) >= self.max_graph_shapes:
                self._graphs.popitem(last=False)  # least recently used shape
            entry = self._capture(*inputs)
        self._graphs[key] = entry  # most recently used last
        graph, statics, static_out = entry
        for static, value in zip(statics, inputs):
            if draw and value is noise:
                static.normal_()
            else:
                static.copy_(value, non_blocking=True)
        graph.replay()
        return static_out

    def _host_block(self, group, feats):
        """One group's padded upload: (max_batch, T_pad, C), zeros where there is no frame."""
        block = torch.zeros((self.max_batch, group.t_pad, self.channels)).pin_memory()
        for j, i in enumerate(group.indices):
            block[j, :feats[i].shape[0]] = feats[i]
        return block

    def _run_group(self, c, frames, group, noises):
        """One group's forward on the uploaded features and table (a subclass with a noise input builds it here)."""
        return self._run(c, frames)

    @torch.no_grad()
    def _synthesize(self, feats, normalize_before, convert, noises=None):
        if normalize_before and not (hasattr(self.model, "mean") and hasattr(self.model, "scale")):
            raise ValueError(f"{type(self).__name__}: normalize_before=True needs model.register_stats(...)")
        mean = self.model.mean if normalize_before else None
        scale = self.model.scale if normalize_before else None
        feats = [torch.as_tensor(f, dtype=torch.float32).cpu() for f in feats]
        for i, f in enumerate(feats):
            if f.dim() != 2 or f.shape[1] != self.channels:
                raise ValueError(f"{type(self).__name__}: item {i}: expected (T, {self.channels}) features, got "
                                 f"{tuple(f.shape)}")
        outs = [None] * len(feats)
        for group in self.plan([f.shape[0] for f in feats]).groups:
            block = self._host_block(group, feats)  # one padded upload per group
            frames = torch.tensor(group.frames, dtype=torch.int32).pin_memory()
            c = normalize_transpose(block.to(self._device, non_blocking=True), mean, scale)
            y = convert(self._run_group(c, frames.to(self._device, non_blocking=True), group, noises))
            for j, i in enumerate(group.indices):
                outs[i] = y[j, 0, :feats[i].shape[0] * self.up].clone()  # (the graph's buffer is written again)
        return outs

    def synthesize_many(self, feats, normalize_before=False):
        """feats: list of ``(T_i, C)`` tensors / arrays -> list of ``(T_i * up,)`` fp32 device tensors, in input order
        (``up``: samples per frame).  ValueError for an empty, too short or over-long item."""
        return self._synthesize(feats, normalize_before, lambda y: y)

    def synthesize_many_pcm16(self, feats, normalize_before=False):
        """:meth:`synthesize_many` through the float -> PCM16 conversion on the device: int16 tensors."""
        return self._synthesize(feats, normalize_before, to_pcm16)


class RaggedSynthesizer(_RaggedSynthesizer):
    """Whole utterances of DIFFERENT lengths, ``max_batch`` per forward, each exactly what it gives alone: the batched
    form of the reference's decode loop (/root/reference/parallel_wavegan/bin/decode.py:214-243) for the non-causal
    ``HiFiGANGenerator``.

    The utterances are sorted by length and grouped; a group is uploaded once as a ``(max_batch, T_pad, C)`` block,
    ``T_pad`` its longest length rounded up to ``bucket_frames``, with a device table of frames per item, and runs
    ``model.forward_ragged``: every layer leaves exact zeros past each item's end, so a short item
    reads the zero padding it would read alone -- zero mel frames alone would not do that (a hidden layer is not zero
    where the mel is zero).  Nothing on the host depends on the table, so ``use_graph`` replays ONE graph per
    ``(max_batch, T_pad)``; a last, partial group is filled with items of 0 frames to reuse it.  ``max_graph_shapes``
    graphs are kept, least recently used dropped, and all are dropped when the model's parameter state changes.
    ``precision``: None = the modes ``utils.set_inference_precision`` left on the model, else ``"fp32"`` / ``"bf16"`` for
    this synthesizer's forwards.

    Only the non-causal ``HiFiGANGenerator`` with one output channel: a reflect-padded MelGAN needs a mirror at each
    item's own end (:class:`MelGANRaggedSynthesizer`) and Parallel WaveGAN replicates its edge and takes noise
    (:class:`PWGRaggedSynthesizer`); ``ChunkedSynthesizer`` batches the equal-shaped chunks of any mel-only generator."""

    def __init__(self, model, max_batch=16, bucket_frames=64, use_graph=True, precision=None):
        from ..models import HiFiGANGenerator

        name = type(model).__name__
        other = "utils.ChunkedSynthesizer batches the equal-shaped chunks of any mel-only generator"
        if not isinstance(model, HiFiGANGenerator):
            raise ValueError(f"RaggedSynthesizer: {name} is not supported (only the non-causal HiFiGANGenerator; {other})")
        if model.use_causal_conv:
            raise ValueError(f"RaggedSynthesizer: this {name} is causal (use_causal_conv=True) and has no ragged forward "
                             f"({other}; utils.CausalStream streams it)")
        if model.output_conv[1].out_channels != 1:
            raise ValueError(f"RaggedSynthesizer: this {name} emits {model.output_conv[1].out_channels} channels; an item "
                             f"returns one waveform ({other})")
        if precision not in (None, "fp32", "bf16"):
            raise ValueError(f"RaggedSynthesizer: precision must be None, 'fp32' or 'bf16', got {precision!r}")
        self.precision = precision
        self._setup(model, max_batch, bucket_frames, use_graph, model.input_conv.in_channels, model.upsample_factor,
                    model.upsample_factor * model.input_conv.out_channels)

    def _forward(self, c, frames):
        from .precision import inference_precision

        with inference_precision(self.model, self.precision):
            return self.model.forward_ragged(c, frames)


class MelGANRaggedSynthesizer(_RaggedSynthesizer):
    """:class:`RaggedSynthesizer` for the non-causal, reflect-padded ``MelGANGenerator``, ``multi_band_melgan.v2``
    included: the same interface, plan, graphs and recapture, on ``model.forward_ragged``, which mirrors
    every ``ReflectionPad1d`` at each item's own end.  fp32 only (MelGAN has no bf16 mode).

    ``T_pad`` is the smallest multiple of ``bucket_frames`` that is at least the group's longest length +
    ``model.ragged_slack_frames`` (the mirror columns behind an item must fit inside the buffer), and an item shorter
    than ``model.ragged_min_frames`` (4 for kernel 7) is a ValueError naming it -- the reference raises for it too (a
    reflection longer than its input).  With that every item of a group meets what ``forward_ragged`` asks of the
    table: 0, or ``min_frames <= n <= T_pad - slack``.

    Multi-band (``model.pqmf`` attached, as ``utils.load_model`` attaches it): ``pqmf.synthesis`` runs once per group
    on the sub-bands, which are exact zeros past each item's end -- the zero padding the synthesis filter applies to the
    item alone -- and an item returns ``T_i * upsample_factor * subbands`` samples; a plain model returns ``T_i *
    upsample_factor``."""

    def __init__(self, model, max_batch=16, bucket_frames=64, use_graph=True):
        from ..layers.pqmf import PQMF
        from ..models import HiFiGANGenerator, MelGANGenerator

        name = type(model).__name__
        if isinstance(model, HiFiGANGenerator):
            raise ValueError(f"MelGANRaggedSynthesizer: {name} is not supported (only the non-causal MelGANGenerator; "
                             "utils.RaggedSynthesizer batches HiFi-GAN utterances of different lengths)")
        if not isinstance(model, MelGANGenerator):
            raise ValueError(f"MelGANRaggedSynthesizer: {name} is not supported (only the non-causal MelGANGenerator; "
                             "utils.ChunkedSynthesizer batches the equal-shaped chunks of any mel-only generator)")
        try:
            walk = model._ragged_walk()  # ValueError: causal, a pad other than reflection
            min_frames, slack = model.ragged_min_frames, model.ragged_slack_frames
        except ValueError as e:
            raise ValueError(f"MelGANRaggedSynthesizer: {e} (utils.ChunkedSynthesizer batches the equal-shaped chunks of "
                             "any mel-only generator)") from None
        out_channels = walk[-1][0].out_channels
        self.pqmf = getattr(model, "pqmf", None)
        if self.pqmf is None and out_channels != 1:
            raise ValueError(f"MelGANRaggedSynthesizer: this {name} emits {out_channels} channels without a PQMF "
                             "(model.pqmf = PQMF(subbands=...), as utils.load_model attaches it); an item returns one "
                             "waveform")
        if self.pqmf is not None and (not isinstance(self.pqmf, PQMF) or self.pqmf.subbands != out_channels):
            raise ValueError(f"MelGANRaggedSynthesizer: model.pqmf must be a PQMF with as many sub-bands as the generator "
                             f"emits ({out_channels}); got {getattr(self.pqmf, 'subbands', type(self.pqmf).__name__)}")
        self.subbands = out_channels
        widest = max(m.out_channels * rate * (m.stride if m.transposed else 1) for m, _, _, rate in walk
                     if hasattr(m, "out_channels"))
        self._setup(model, max_batch, bucket_frames, use_graph, walk[0][0].in_channels,
                    model.upsample_factor * out_channels, max(widest, model.upsample_factor * out_channels), min_frames,
                    slack)

    def _forward(self, c, frames):
        y = self.model.forward_ragged(c, frames)
        return y if self.pqmf is None else self.pqmf.synthesis(y)


class PWGRaggedSynthesizer(_RaggedSynthesizer):
    """:class:`RaggedSynthesizer` for the non-causal ``ParallelWaveGANGenerator``: the same plan, graphs (one per
    ``(max_batch, T_pad)``, ``max_graph_shapes`` kept) and recapture on a parameter change, on ``model.forward_ragged``
    (DESIGN.md s9.6), whose gated layers read nothing at or past an item's end.

    The generator's two extras are the host's and the noise.  The context window: a group's block is ``(max_batch,
    T_pad + 2 w, C)``, ``w = model.aux_context_window``, with item ``j``'s frames at the rows ``[w, w + T_j)`` and its
    first and last frame replicated ``w`` rows outward -- per item what ``inference`` pads onto the utterance alone.
    The noise: ``synthesize_many(feats, noises=...)`` takes one ``(T_i * up,)`` tensor or array per utterance and item
    ``i`` uses exactly that noise (with it the result is what ``model.inference(c, x)`` gives, to summation order);
    ``noises=None`` draws standard normal noise on the device into the graph's static noise buffer before each replay,
    outside the graph, so two calls differ.  ``precision``: None = the modes ``utils.set_inference_precision`` left on
    the model, else ``"fp32"`` / ``"bf16"`` for this synthesizer's forwards.  ``max_frames`` is the layer kernel's limit
    on a row (``pwg_wavenet_layer_ragged_supported``)."""

    def __init__(self, model, max_batch=16, bucket_frames=64, use_graph=True, precision=None):
        from ..models import ParallelWaveGANGenerator
        name = type(model).__name__
        other = "utils.ChunkedSynthesizer batches the equal-shaped chunks of any mel-only generator"
        if not isinstance(model, ParallelWaveGANGenerator):
            raise ValueError(f"PWGRaggedSynthesizer: {name} is not supported (only the non-causal "
                             f"ParallelWaveGANGenerator; utils.RaggedSynthesizer and utils.MelGANRaggedSynthesizer batch "
                             f"HiFi-GAN and MelGAN utterances of different lengths; {other})")
        if precision not in (None, "fp32", "bf16"):
            raise ValueError(f"PWGRaggedSynthesizer: precision must be None, 'fp32' or 'bf16', got {precision!r}")
        reason = model.ragged_unsupported_reason(precision or "fp32")
        if reason is not None:
            raise ValueError(f"PWGRaggedSynthesizer: this {name} has no ragged forward: {reason} (model.inference runs "
                             f"one utterance per call; utils.PWGStream / utils.PWGLookaheadStream stream it)")
        self.precision = precision
        from ..layers.upsample import ConvInUpsampleNetwork

        self.context = model.aux_context_window if isinstance(model.upsample_net, ConvInUpsampleNetwork) else 0
        up = model.upsample_factor
        block = model.conv_layers[0]
        widest = max(model.aux_channels, block.conv.in_channels, block.conv1x1_skip.out_channels)
        self._setup(model, max_batch, bucket_frames, use_graph, model.aux_channels, up, up * widest)
        self.max_frames = min(self.max_frames, self.kernel_max_columns(block, up) // up)

    @staticmethod
    def kernel_max_columns(block, rate):
        """The layer kernel's own limit on a row: the largest ``T`` its ragged form takes for ``block`` at ``rate``
        columns per frame, asked of ``pwg_wavenet_layer_ragged_supported`` (host logic, monotone in ``T``)."""
        from ..ops import wavenet_layer_ragged_supported

        lo, hi = 0, 2 ** 31 - 1
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if wavenet_layer_ragged_supported(block.fused_desc(1, mid), rate) else (lo, mid - 1)
        return lo

    def _forward(self, c, frames, z):
        from .precision import inference_precision

        with inference_precision(self.model, self.precision):
            return self.model.forward_ragged(z, c, frames)

    @staticmethod
    def block_layout(group, feats, context, max_batch, channels):
        """Pure host logic: one group's block (max_batch, T_pad + 2 w, C), ``w = context``: item j's frames at the rows
        [w, w + T_j), its edge frames replicated w rows outward (``Fn.pad1d(..., "replicate")`` of the item alone),
        zeros behind."""
        w = int(context)
        block = torch.zeros((max_batch, group.t_pad + 2 * w, channels))
        for j, i in enumerate(group.indices):
            n = feats[i].shape[0]
            block[j, w:w + n] = feats[i]
            block[j, :w] = feats[i][0]
            block[j, w + n:n + 2 * w] = feats[i][n - 1]
        return block

    def _host_block(self, group, feats):
        return self.block_layout(group, feats, self.context, self.max_batch, self.channels).pin_memory()

    def _noise_block(self, group, noises):
        """(max_batch, 1, T_pad * up) on the host: item j's noise at its samples, zeros behind."""
        z = torch.zeros((self.max_batch, 1, group.t_pad * self.up)).pin_memory()
        for j, i in enumerate(group.indices):
            z[j, 0, :noises[i].shape[0]] = noises[i]
        return z

    def _run_group(self, c, frames, group, noises):
        if noises is None:
            z = torch.empty((self.max_batch, 1, group.t_pad * self.up), device=self._device)
            return self._run(c, frames, z, draw=True)
        return self._run(c, frames, self._noise_block(group, noises).to(self._device, non_blocking=True))

    def _checked_noises(self, feats, noises):
        if noises is None:
            return None
        noises = [torch.as_tensor(z, dtype=torch.float32).cpu().reshape(-1) for z in noises]
        if len(noises) != len(feats):
            raise ValueError(f"PWGRaggedSynthesizer: {len(noises)} noises for {len(feats)} utterances")
        for i, (f, z) in enumerate(zip(feats, noises)):
            n = len(f) * self.up
            if z.shape[0] != n:
                raise ValueError(f"PWGRaggedSynthesizer: item {i}: expected ({n},) noise for {len(f)} frames, got "
                                 f"({z.shape[0]},)")
        return noises

    def synthesize_many(self, feats, normalize_before=False, noises=None):
        """feats: list of ``(T_i, C)`` tensors / arrays -> list of ``(T_i * up,)`` fp32 device tensors, in input order.
        ``noises``: None (drawn on the device) or one ``(T_i * up,)`` tensor / array per utterance."""
        return self._synthesize(feats, normalize_before, lambda y: y, self._checked_noises(feats, noises))

    def synthesize_many_pcm16(self, feats, normalize_before=False, noises=None):
        """:meth:`synthesize_many` through the float -> PCM16 conversion on the device: int16 tensors."""
        return self._synthesize(feats, normalize_before, to_pcm16, self._checked_noises(feats, noises))


class StyleMelGANRaggedSynthesizer(_RaggedSynthesizer):
    """:class:`RaggedSynthesizer` for ``StyleMelGANGenerator``: the same plan, one upload per group, graphs (one per
    shape, ``max_graph_shapes`` kept) and recapture on a parameter change, on ``model.forward_ragged``.
    Every TADE layer starts with an instance norm over the whole time axis, so a padded batch is another signal, not an
    approximation; the ragged forward takes each item's statistics over the item alone.

    The unit of length is the noise segment, ``F = model.noise_upsample_factor`` frames: ``inference`` runs an utterance
    of ``T`` frames on ``ceil(T / F)`` noise columns and ``ceil(T / F) * F`` frames, the last frame replicated, and cuts
    the audio to ``T * upsample_factor`` samples.  So the plan works in segments -- a group's ``t_pad`` is ``S_pad``, its
    longest item's segment count rounded up to ``bucket_segments``, and its ``frames`` are segment counts --, the host
    replicates each item's last frame up to its own segment boundary (:meth:`block_layout`) and cuts each result.

    The noise: ``synthesize_many(feats, noises=...)`` takes one ``(in_channels, n_i)`` tensor or array per utterance, ``n_i
    = ceil(T_i / F)``, and item ``i`` uses exactly that noise (``model.inference(c, z=...)`` to summation order);
    ``noises=None`` draws on the host, per utterance in input order, with ``torch.randn(1, in_channels, n_i)`` -- the call
    ``inference`` makes, so a seeded run reproduces a seeded loop of ``inference`` calls.  fp32 only: the modules'
    ``precision`` is not touched."""

    def __init__(self, model, max_batch=16, bucket_segments=2, use_graph=True):
        from ..models import HiFiGANGenerator, MelGANGenerator, ParallelWaveGANGenerator, StyleMelGANGenerator

        name = type(model).__name__
        other = "utils.ChunkedSynthesizer batches the equal-shaped chunks of any mel-only generator"
        if not isinstance(model, StyleMelGANGenerator):
            right = {HiFiGANGenerator: "utils.RaggedSynthesizer", MelGANGenerator: "utils.MelGANRaggedSynthesizer",
                     ParallelWaveGANGenerator: "utils.PWGRaggedSynthesizer"}
            hint = next((f"{syn} batches its utterances of different lengths; " for cls, syn in right.items()
                         if isinstance(model, cls)), "")
            raise ValueError(f"StyleMelGANRaggedSynthesizer: {name} is not supported (only StyleMelGANGenerator; "
                             f"{hint}{other})")
        conv = model.output_conv[0]
        if conv.out_channels != 1:
            raise ValueError(f"StyleMelGANRaggedSynthesizer: this {name} emits {conv.out_channels} channels; an item "
                             f"returns one waveform ({other})")
        if int(bucket_segments) < 1:
            raise ValueError("StyleMelGANRaggedSynthesizer: max_batch and bucket_segments must be >= 1")
        self.segment_frames = model.noise_upsample_factor
        self.noise_channels = model.in_channels
        # the widest row: the 2 * channels rows of a gated convolution at the output rate
        self._setup(model, max_batch, bucket_segments, use_graph, model.blocks[0].tade1.aux_conv[0].in_channels,
                    model.upsample_factor, 2 * conv.in_channels * model.upsample_factor)
        self.bucket_segments = self.bucket_frames

    def segments_of(self, n_frames):
        """Noise columns of an utterance of ``n_frames`` frames: ``ceil(n_frames / F)``, as ``inference`` draws them."""
        return -(-int(n_frames) // self.segment_frames)

    @classmethod
    def plan_segments(cls, lengths, segment_frames, max_batch=16, bucket_segments=2, max_frames=None):
        """Pure host logic: ``lengths`` (FRAMES per utterance) -> :meth:`plan_groups` over their segment counts
        ``ceil(n / segment_frames)``: a group's ``frames`` are segments per item, its ``t_pad`` is ``S_pad`` and
        ``padded_fraction`` is the share of the ``max_batch * S_pad`` segment slots that hold no segment.  ValueError
        for an empty or over-long item, counted in frames."""
        cls.plan_groups(lengths, 1, 1, max_frames, who=cls.__name__)  # (only its checks)
        return cls.plan_groups([-(-int(n) // int(segment_frames)) for n in lengths], max_batch, bucket_segments,
                               who=cls.__name__)

    def plan(self, lengths):
        """:meth:`plan_segments` with this synthesizer's ``F``, ``max_batch``, ``bucket_segments`` and ``max_frames``."""
        return self.plan_segments(lengths, self.segment_frames, self.max_batch, self.bucket_segments, self.max_frames)

    def _forward(self, c, segments, z):
        return self.model.forward_ragged(c, z, segments)

    @staticmethod
    def block_layout(group, feats, segment_frames, max_batch, channels):
        """Pure host logic: one group's block (max_batch, S_pad * F, C), ``F = segment_frames``: item j's frames first,
        its last frame replicated up to its segment boundary ``segments_j * F`` (``Fn.pad1d(..., "replicate")`` of the
        item alone in ``inference``), zeros behind."""
        F = int(segment_frames)
        block = torch.zeros((max_batch, group.t_pad * F, channels))
        for j, i in enumerate(group.indices):
            n = feats[i].shape[0]
            block[j, :n] = feats[i]
            block[j, n:group.frames[j] * F] = feats[i][n - 1]
        return block

    def _host_block(self, group, feats):
        return self.block_layout(group, feats, self.segment_frames, self.max_batch, self.channels).pin_memory()

    def _run_group(self, c, segments, group, noises):
        z = torch.zeros((self.max_batch, self.noise_channels, group.t_pad)).pin_memory()
        for j, i in enumerate(group.indices):
            z[j, :, :noises[i].shape[1]] = noises[i]
        return self._run(c, segments, z.to(self._device, non_blocking=True))

    def _checked_noises(self, feats, noises):
        lengths = [len(f) for f in feats]
        if noises is None:  # inference's own draw, per utterance in input order
            return [torch.randn(1, self.noise_channels, self.segments_of(n), dtype=torch.float)[0] for n in lengths]
        noises = [torch.as_tensor(z, dtype=torch.float32).cpu() for z in noises]
        if len(noises) != len(feats):
            raise ValueError(f"StyleMelGANRaggedSynthesizer: {len(noises)} noises for {len(feats)} utterances")
        for i, (n, z) in enumerate(zip(lengths, noises)):
            want = (self.noise_channels, self.segments_of(n))
            if tuple(z.shape) != want:
                raise ValueError(f"StyleMelGANRaggedSynthesizer: item {i}: expected {want} noise for {n} frames, got "
                                 f"{tuple(z.shape)}")
        return noises

    def synthesize_many(self, feats, normalize_before=False, noises=None):
        """feats: list of ``(T_i, C)`` tensors / arrays -> list of ``(T_i * up,)`` fp32 device tensors, in input order.
        ``noises``: None (drawn on the host as ``inference`` draws) or one ``(in_channels, ceil(T_i / F))`` tensor / array
        per utterance."""
        return self._synthesize(feats, normalize_before, lambda y: y, self._checked_noises(feats, noises))

    def synthesize_many_pcm16(self, feats, normalize_before=False, noises=None):
        """:meth:`synthesize_many` through the float -> PCM16 conversion on the device: int16 tensors."""
        return self._synthesize(feats, normalize_before, to_pcm16, self._checked_noises(feats, noises))

"""CPU: host logic of the pool of (multi-band) MelGAN look-ahead streams (utils.MelGANStreamPool, the slotted-mirrored
form of the streaming convolution and the slotted PQMF synthesis) -- the per-item input edges and their
saturation, a float64 emulation of a whole pool against the whole-utterance oracle, the pool's figures, the entry
points, and what the pool refuses and in which order.  Nothing here launches a kernel."""
import ctypes
import itertools
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import torch_cpu
from parallelwavegan_amd import _lib, layers, models, ops
from parallelwavegan_amd.layers.causal_conv import (_STREAM_KERNELS, LookaheadLaunch, launch_is_mirrored,
                                                    lookahead_settle_frames, mirrored_in_window)
from parallelwavegan_amd.utils import MelGANLookaheadStream, MelGANStreamPool, set_inference_precision
from parallelwavegan_amd.utils.streaming import SlotSchedule, slot_mirror_window, slot_window
from tests.golden import synth
from tests.util import max_abs, synth_for

# the configs of tests/test_stream_melgan_lookahead_gpu.py, restated
TINY = dict(synth.MELGAN_CAUSAL, use_causal_conv=False)  # channels 64, scales [4, 2, 2], 2 stacks: 16 samples a frame
TINY_MB = dict(in_channels=80, out_channels=4, kernel_size=7, channels=32, upsample_scales=[3, 2], stack_kernel_size=3,
               stacks=3)  # an odd stride, dilations 1, 3, 9, 4 sub-bands: 24 samples a frame
V1 = dict()
MB_V2 = dict(out_channels=4, channels=384, upsample_scales=[8, 4, 2], stacks=4)
MB_V2_24K = dict(out_channels=4, channels=384, upsample_scales=[5, 5, 3], stacks=4)
MAX_NT = 64  # kStreamMaxNt
PQMF_TAPS = 62


def _multi_band(cfg):
    g = models.MelGANGenerator(**cfg)
    if cfg.get("out_channels", 1) > 1:
        g.pqmf = layers.PQMF(subbands=cfg["out_channels"])
    return g


def _bound(edge, hist, n):
    """``mirror_bound`` (csrc/stream_common.h), restated."""
    return max(-hist, min(n + MAX_NT, edge))


def _expected_edges(launch, n, before, left):
    """The edges by the lock-step stream's rule, ``mirrored_in_window``, saturated as the mirrored entry does."""
    lo, hi = mirrored_in_window(launch, before, None if left is None else before + left)
    hist = 2 * launch.conv.padding
    return _bound(lo, hist, n), n + MAX_NT if hi is None else _bound(hi, hist, n)


# ---- the per-item input edges ----------------------------------------------------------------------------------------
def test_slot_mirror_window_equals_the_lockstep_window_on_a_small_grid():
    count = 0
    for rate, p, chunk in itertools.product((1, 3, 16), (3, 9, 27), (1, 4, 8)):
        delay = p + 5 * rate + 1  # the input is 5 frames and a column late
        launch = LookaheadLaunch(types.SimpleNamespace(padding=p), rate, delay, 0, 0)
        settle, n = -(-(delay + p) // rate), chunk * rate
        for before in range(0, settle + 3):
            for left in [None] + list(range(-settle - 2, chunk + 3)):
                if left is not None and before + left < 0:  # (an utterance has no negative length)
                    continue
                got = slot_mirror_window(delay, p, rate, n, before, left)
                assert got == _expected_edges(launch, n, before, left), (rate, p, chunk, before, left)
                # the valid window of the output is the input's, shifted by the padding and clamped
                assert slot_window(delay, rate, n, before, left) == \
                    tuple(min(max(e + p, 0), n) for e in got), (rate, p, chunk, before, left)
                count += 1
    assert count > 8000


def test_slot_mirror_window_near_2_to_the_31_frames():
    p, rate, n, delay = 27, 256, 2048, 672
    for before in (2 ** 31 - 4, 2 ** 31 - 1, 2 ** 31 + 5, 2 ** 40):
        for left in (None, -2 ** 31 + 1, -3, 0, 2, 8, 2 ** 31 - 1):
            lo, hi = slot_mirror_window(delay, p, rate, n, before, left)
            assert lo == -2 * p
            assert hi == (n + MAX_NT if left is None else _bound(delay - p + left * rate, 2 * p, n)), (before, left)
    assert slot_mirror_window(delay, p, rate, n, 0, 2 ** 31 - 1) == (delay - p, n + MAX_NT)


def _columns(in_lo, in_hi, hist, n):
    """What every window column ``t`` in ``[-hist, n)`` reads under the mirror rule: the mapped column, None if it lies
    outside ``[-hist, n)`` (it reads as zero).  ``in_hi`` None: unbounded."""
    out = []
    for t in range(-hist, n):
        m = 2 * in_lo - t if t < in_lo else (2 * (in_hi - 1) - t if in_hi is not None and t >= in_hi else t)
        out.append(m if -hist <= m < n else None)
    return out


@pytest.mark.parametrize("cfg", [TINY, TINY_MB], ids=["tiny", "tiny_mb"])
def test_saturated_rows_map_every_column_as_the_true_numbers_do(cfg):
    """What ``SlotSchedule`` puts into the table -- the position capped at ``settle``, the frames left clamped to
    ``[-settle, chunk]`` -- and the kernel's own saturation of the edges change no mapped column in ``[-H, n)`` and no
    valid window, for every reflect-padded launch of the plan."""
    g, chunk = _multi_band(cfg), 4
    settle = MelGANLookaheadStream.settle_frames_of(g)
    seen = 0
    for launch in g.lookahead_plan():
        if not launch_is_mirrored(launch):
            continue
        p, rate, n = launch.conv.padding, launch.rate, chunk * launch.rate
        for before in (0, 1, settle - 1, settle, settle + 1, 10 ** 12):
            for left in (None, -10 ** 12, -settle - 1, -settle, -1, 0, 1, chunk, chunk + 1, 10 ** 12):
                true_lo = launch.delay - p - before * rate
                true_hi = None if left is None else launch.delay - p + left * rate
                sat = None if left is None else max(-settle, min(left, chunk))
                lo, hi = slot_mirror_window(launch.delay, p, rate, n, min(before, settle), sat)
                assert _columns(lo, hi, 2 * p, n) == _columns(true_lo, true_hi, 2 * p, n), (launch[1:], before, left)
                assert slot_window(launch.delay, rate, n, min(before, settle), sat) == \
                    slot_window(launch.delay, rate, n, before, left) == tuple(min(max(e + p, 0), n) for e in (lo, hi))
                seen += 1
    assert seen >= 60 * 5


# ---- a pool, emulated in float64 -------------------------------------------------------------------------------------
class PoolEmulation:
    """The rules of DESIGN.md s11.12 in float64 torch, independent of the package's plan and walk.  Per slot and layer a
    RAW history (stored zeros outside the utterance; NaN before a slot's first utterance: a fresh slot must not read it);
    a step takes, per slot, the table row ``(before, left, flags)`` and a chunk of frames.  A paused slot keeps its
    state (zeros if it is also fresh) and gives zeros; a running one runs every layer in causal form over
    ``concat(history, chunk)``: a reflect-padded layer maps each window column through the mirror at its slot's input
    edges before it reads, every layer stores zeros outside ``[D - before * rate, D + left * rate)``, the skip branch of
    a stack goes through a delay line, and the PQMF synthesis emits one position per column (``n_emit = n``).
    ``sd``: reference-format state dict."""

    def __init__(self, sd, cfg, slots):
        self.sd = {k: v.double() for k, v in sd.items()}
        self.cfg, self.slots = cfg, slots
        self.state = [{} for _ in range(slots)]
        self.k = cfg.get("out_channels", 1)
        pad = PQMF_TAPS // 2
        self.pqmf_delay, self.pqmf_hist = -(-pad // self.k), -(-pad // self.k) + pad // self.k
        self.latency_columns = None

    # -- one slot
    def _line(self, st, name, new, length, fresh):
        ch = new.shape[0]
        old = torch.zeros(ch, length, dtype=torch.float64) if fresh else \
            st.get(name, torch.full((ch, length), float("nan"), dtype=torch.float64))
        cat = torch.cat([old, new], -1)
        st[name] = cat[..., cat.shape[-1] - length:]
        return cat

    @staticmethod
    def _mask(y, delay, rate, before, left):
        t = torch.arange(y.shape[-1])
        valid = t >= delay - before * rate
        if left is not None:
            valid &= t < delay + left * rate
        return torch.where(valid, y, torch.zeros((), dtype=torch.float64))  # stored zeros, also where y is not finite

    def _mirrored(self, st, name, x, d_in, rate, row, dilation=1, slope=None, post=None):
        before, left, fresh = row
        w, b = torch_cpu.get_weight(self.sd, name), torch_cpu.get_bias(self.sd, name)
        reach = (w.shape[-1] - 1) * dilation
        p, n = reach // 2, x.shape[-1]
        cat = self._line(st, name + ":hist", x, reach, fresh)  # window column t = -reach .. n - 1 at index t + reach
        in_lo = d_in - before * rate
        t = torch.arange(-reach, n)
        m = torch.where(t < in_lo, 2 * in_lo - t, t)
        if left is not None:
            in_hi = d_in + left * rate
            m = torch.where((t >= in_lo) & (t >= in_hi), 2 * (in_hi - 1) - t, m)
        live = (m >= -reach) & (m < n)
        win = torch.where(live, cat[..., (m + reach).clamp(0, reach + n - 1)], torch.zeros((), dtype=torch.float64))
        y = F.conv1d((win if slope is None else F.leaky_relu(win, slope))[None], w, b, dilation=dilation)[0]
        if post is not None:
            y = post(y)
        return self._mask(y, d_in + p, rate, before, left), d_in + p

    def _pointwise(self, st, name, x, d_in, rate, row, slope=None, addend=None):
        before, left, fresh = row
        w, b = torch_cpu.get_weight(self.sd, name), torch_cpu.get_bias(self.sd, name)
        y = F.conv1d((x if slope is None else F.leaky_relu(x, slope))[None], w, b)[0]
        if addend is not None:
            a, d_a = addend
            y = y + self._line(st, name + ":add", a, d_in - d_a, fresh)[..., :x.shape[-1]]
        return self._mask(y, d_in, rate, before, left), d_in

    def _up(self, st, name, x, d_in, rate_in, s, slope, row):
        before, left, fresh = row
        w, b = torch_cpu.get_weight(self.sd, name), torch_cpu.get_bias(self.sd, name)
        d_out = d_in * s + s // 2 + s % 2
        win = self._line(st, name + ":hist", x, 1, fresh)
        n = x.shape[-1]
        y = F.conv_transpose1d(F.leaky_relu(win, slope)[None], w, b, stride=s)[0][..., s:s + n * s]
        return self._mask(y, d_out, rate_in * s, before, left), d_out

    def _pqmf(self, st, y, fresh):
        """``n_emit = n``: the chunk positions ``[-D, n - D)`` of the whole-signal synthesis of ``concat(history, y)``."""
        h_cols, d, k = self.pqmf_hist, self.pqmf_delay, self.k
        window = self._line(st, "pqmf:hist", y, h_cols, fresh)
        _, hs = torch_cpu.pqmf_filters(k, PQMF_TAPS, 0.142, 9.0)
        up = F.conv_transpose1d(window[None], torch_cpu._updown(k).double() * k, stride=k)
        x = F.conv1d(F.pad(up, (PQMF_TAPS // 2, PQMF_TAPS // 2)), hs.double())[0, 0]
        return x[(h_cols - d) * k:(h_cols - d + y.shape[-1]) * k]

    def _run_slot(self, st, c, row):
        cfg, slope = self.cfg, 0.2
        x, d = self._mirrored(st, "melgan.1", c, 0, 1, row)
        rate, idx = 1, 2
        for s in cfg["upsample_scales"]:
            x, d = self._up(st, f"melgan.{idx + 1}", x, d, rate, s, slope, row)
            rate *= s
            idx += 2
            for j in range(cfg["stacks"]):
                pre = f"melgan.{idx}"
                skip = self._pointwise(st, pre + ".skip_layer", x, d, rate, row)
                t, dt = self._mirrored(st, pre + ".stack.2", x, d, rate, row, cfg["stack_kernel_size"] ** j, slope)
                x, d = self._pointwise(st, pre + ".stack.4", t, dt, rate, row, slope, addend=skip)
                idx += 1
        y, self.latency_columns = self._mirrored(st, f"melgan.{idx + 2}", x, d, rate, row, 1, slope, post=torch.tanh)
        return self._pqmf(st, y, row[2]) if self.k > 1 else y[0]

    # -- one step of all slots
    def step(self, rows, feats):
        """rows: per slot the table row; feats: (slots, chunk, C) float64 -> (slots, chunk * up)."""
        outs = []
        for s, (before, left, flags, _) in enumerate(rows):
            fresh, paused = before == 0, bool(flags & ops.SLOT_PAUSED)
            if paused:
                if fresh:  # zeros are copied through (nothing of the slot's old utterance survives)
                    self.state[s] = {k: torch.zeros_like(v) for k, v in self.state[s].items()}
                outs.append(None)
                continue
            assert not torch.isnan(feats[s]).any()
            outs.append(self._run_slot(self.state[s], feats[s].t(), (before, left if flags & ops.SLOT_LEFT_KNOWN else None,
                                                                     fresh)))
        width = next(o for o in outs if o is not None).shape[-1]
        return torch.stack([torch.zeros(width, dtype=torch.float64) if o is None else o for o in outs])

    def state_floats(self, slot):
        return sum(v.numel() for v in self.state[slot].values())


LENGTHS = (4, 5, 9, 14, 23)  # min_frames; past both settle counts; no multiples of the chunk


def _serve(cfg, sd, utterances, slots=3, chunk=4):
    """The utterances through an emulated pool driven by ``SlotSchedule``: staggered opens, irregular feeds, slots
    reused, tails zero-padded and drained -> (per utterance the emitted samples, the emulation, facts)."""
    g = _multi_band(cfg)
    k = cfg.get("out_channels", 1)
    up = g.upsample_factor * k
    latency = MelGANLookaheadStream.latency_samples_of(g)
    sch = SlotSchedule(slots, chunk, up, latency, MelGANLookaheadStream.settle_frames_of(g))
    em = PoolEmulation(sd, cfg, slots)
    pending, active = list(range(len(utterances))), {}
    queues, outs = {}, {i: [] for i in pending}
    sizes = itertools.cycle((1, 3, 0, 6, 2))
    facts = dict(pause=0, tail=0, drain=0, reused=0, empty=0)
    used = []
    for tick in range(300):
        if not pending and not active:
            break
        if pending and tick % 2 == 0 and len(sch.open_slots) < slots:
            slot = sch.open()
            facts["reused"] += slot in used
            used.append(slot)
            active[slot] = [pending.pop(0), 0]
            queues[slot] = []
        for slot, st in active.items():
            f = utterances[st[0]]
            if st[1] == f.shape[0]:
                continue
            n = min(next(sizes), f.shape[0] - st[1])
            sch.feed(slot, n)
            queues[slot] += list(f[st[1]:st[1] + n])
            st[1] += n
            if st[1] == f.shape[0]:
                sch.end(slot)
        steps = sch.advance()
        if not steps:
            continue
        feats = torch.full((slots, chunk, 80), float("nan"), dtype=torch.float64)  # (what no running slot may read)
        for stp in steps:
            facts[stp.action] = facts.get(stp.action, 0) + 1
            if stp.action in ("run", "tail", "drain"):
                rows = [queues[stp.slot].pop(0) for _ in range(stp.take)]
                # the padding frames are dummies: the first layer mirrors at the utterance's end and never reads them
                feats[stp.slot] = 7.0
                if rows:
                    feats[stp.slot, :stp.take] = torch.stack(rows).double()
        y = em.step([stp.row for stp in steps], feats)
        for stp in steps:
            if stp.action in ("run", "tail", "drain"):
                outs[active[stp.slot][0]].append(y[stp.slot, stp.emit[0]:stp.emit[1]])
            if stp.closes:
                del active[stp.slot]
    assert not pending and not active
    return [torch.cat(outs[i]) for i in range(len(utterances))], em, facts


@pytest.mark.parametrize("cfg", [TINY, TINY_MB], ids=["tiny", "tiny_mb"])
def test_emulated_pool_equals_the_whole_utterance_oracle(cfg):
    sd = synth_for(models.MelGANGenerator(**cfg), 21, synth.MELGAN_G_SCALE)
    utterances = [synth.synth_input(f"mpool{i}", (t, 80), seed=70 + i) for i, t in enumerate(LENGTHS)]
    got, em, facts = _serve(cfg, sd, utterances)
    assert facts["pause"] and facts["tail"] and facts["drain"] and facts["reused"] and facts["empty"], facts
    k = cfg.get("out_channels", 1)
    sd64 = {name: v.double() for name, v in sd.items()}
    for i, (y, f) in enumerate(zip(got, utterances)):
        ref = torch_cpu.melgan_generator(sd64, f.t()[None].double(), **cfg)
        if k > 1:
            _, hs = torch_cpu.pqmf_filters(k, PQMF_TAPS, 0.142, 9.0)
            ref = F.conv_transpose1d(ref, torch_cpu._updown(k).double() * k, stride=k)
            ref = F.conv1d(F.pad(ref, (PQMF_TAPS // 2, PQMF_TAPS // 2)), hs.double())
        ref = ref[0, 0]
        assert y.shape == ref.shape == (f.shape[0] * _multi_band(cfg).upsample_factor * k,)
        assert max_abs(y, ref) < 1e-10, (i, max_abs(y, ref))
    # the emulation's state is the pool's: what every launch keeps, and the PQMF history
    g = _multi_band(cfg)
    assert MelGANStreamPool.state_bytes_of(g, 3) == 2 * 4 * 3 * em.state_floats(0)
    assert MelGANLookaheadStream.latency_samples_of(g) == (em.latency_columns + (em.pqmf_delay if k > 1 else 0)) * k


# ---- the pool's figures ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,latency,settle,min_frames,up", [
    (TINY, 90, 6, 4, 16), (TINY_MB, 65 * 4 + 32, 13, 4, 24), (V1, 1425, 7, 4, 256), (MB_V2, 672 * 4 + 32, 12, 4, 256),
    (MB_V2_24K, 1044 * 4 + 32, 17, 6, 300)],
    ids=["tiny", "tiny_mb", "melgan.v1", "multi_band_melgan.v2", "multi_band_melgan.v2 [5, 5, 3]"])
def test_latency_settling_minimum_and_state_from_the_geometry(cfg, latency, settle, min_frames, up):
    """The pool's figures are the lock-step stream's, and an utterance too short for reflection has emitted nothing by
    the time ``end()`` refuses it: ``(min_frames - 1) * up <= latency_samples``."""
    from parallelwavegan_amd.layers.causal_conv import lookahead_state_shapes

    g = _multi_band(cfg)
    assert MelGANLookaheadStream.latency_samples_of(g) == latency
    assert MelGANLookaheadStream.settle_frames_of(g) == settle >= lookahead_settle_frames(g.lookahead_plan())
    assert MelGANLookaheadStream.min_frames_of(g) == min_frames
    assert g.upsample_factor * cfg.get("out_channels", 1) == up and (min_frames - 1) * up <= latency
    shapes = lookahead_state_shapes(g.lookahead_plan(), 16) + ([g.pqmf.history_shape(16)] if cfg.get("out_channels", 1) > 1 else [])
    assert MelGANStreamPool.state_bytes_of(g, 16) == 2 * 4 * sum(b * c * n for b, c, n in shapes)
    sch = SlotSchedule(1, 1, up, latency, settle)  # chunks of one frame: a too-short utterance runs, and emits nothing
    s = sch.open()
    sch.feed(s, min_frames - 1)
    for _ in range(min_frames - 1):
        (st,) = sch.advance()
        assert st.action == "run" and st.emit[0] == st.emit[1]
    assert sch.advance() == []


# ---- the entry points --------------------------------------------------------------------------------------------------
def test_new_entry_points_are_exported_under_the_same_abi():
    assert _lib.ABI_VERSION == _lib.lib().pwg_abi_version() == 15
    for name in ("pwg_conv1d_stream_slots_mirrored_forward", "pwg_pqmf_up_stream_slots"):
        assert name in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    # the arguments of the mirrored entry, its four windows replaced by (slots, rate, delay) in front of y
    res, args = _lib.SIGNATURES["pwg_conv1d_stream_mirrored_forward"]
    assert _lib.SIGNATURES["pwg_conv1d_stream_slots_mirrored_forward"] == \
        (res, args[:6] + [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32] + [args[6], args[-1]])
    assert _STREAM_KERNELS["slots_mirrored", "fp32"][1:] == (ops.conv1d_stream_mirrored_supported,
                                                             ops.conv1d_stream_slots_mirrored_forward)
    assert ("slots_mirrored", "bf16") not in _STREAM_KERNELS


def test_new_wrappers_refuse_cpu_tensors():
    d = ops.make_conv_desc(1, 4, 4, 8, 8, 3, pad_left=2, pad_mode="reflect")
    table = torch.zeros(1, ops.SLOT_INTS, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.conv1d_stream_slots_mirrored_forward(d, torch.zeros(1, 4, 8), torch.zeros(1, 4, 2), torch.zeros(1, 4, 2),
                                                 torch.zeros(3 * 16 * 128), slots=table, delay=1)
    pq = layers.PQMF(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pq.stream_synthesis_slots(torch.zeros(1, 4, 20), torch.zeros(pq.history_shape(1)), torch.zeros(pq.history_shape(1)),
                                  table)


# ---- what the pool refuses, and in which order -------------------------------------------------------------------------
def test_pool_refuses_what_the_lockstep_stream_refuses_in_its_order():
    # (all of these models live on the CPU: a refusal that names the model comes before "no CPU fallback")
    g = models.MelGANGenerator(**TINY)
    reason = "bf16.*does not exist"
    with pytest.raises(ValueError, match=reason) as pool_says:
        MelGANStreamPool(models.HiFiGANGenerator(**synth.HIFIGAN_TINY), precision="bf16")  # the precision comes first
    with pytest.raises(ValueError, match=reason) as stream_says:
        MelGANLookaheadStream(g, precision="bf16")
    assert str(pool_says.value).split(": ", 1)[1] == str(stream_says.value).split(": ", 1)[1]  # the stream's reason
    with pytest.raises(ValueError, match="precision must be"):
        MelGANStreamPool(g, precision="fp16")
    with pytest.raises(ValueError, match="MelGANStreamPool: HiFiGANGenerator is not supported"):
        MelGANStreamPool(models.HiFiGANGenerator(**synth.HIFIGAN_TINY))
    with pytest.raises(ValueError, match="CausalStream"):
        MelGANStreamPool(models.MelGANGenerator(**synth.MELGAN_CAUSAL))
    with pytest.raises(ValueError, match="ReflectionPad1d"):
        MelGANStreamPool(models.MelGANGenerator(**dict(TINY, pad="ReplicationPad1d")))
    with pytest.raises(ValueError, match="PQMF attached"):
        MelGANStreamPool(models.MelGANGenerator(**TINY_MB))
    mb = _multi_band(TINY_MB)
    mb.pqmf = layers.PQMF(subbands=3)
    with pytest.raises(ValueError, match="as many sub-bands"):
        MelGANStreamPool(mb)
    # order: a causal bf16-mode model is told about CausalStream, a non-causal one about its precision, and both
    # before the sizes
    causal = models.MelGANGenerator(**synth.MELGAN_CAUSAL)
    set_inference_precision(causal, "bf16")
    with pytest.raises(ValueError, match="CausalStream"):
        MelGANStreamPool(causal, slots=0)
    in_bf16 = models.MelGANGenerator(**TINY)
    set_inference_precision(in_bf16, "bf16")
    with pytest.raises(ValueError, match="bf16 inference precision"):
        MelGANStreamPool(in_bf16, slots=0)
    with pytest.raises(ValueError, match="slots"):
        MelGANStreamPool(g, slots=0)
    with pytest.raises(ValueError, match="chunk_frames"):
        MelGANStreamPool(g, chunk_frames=0)
    # a layer the kernel turns down: (k - 1) * d = 2 * 81 = 162 columns of history
    with pytest.raises(ValueError, match="LDS"):
        MelGANStreamPool(models.MelGANGenerator(**dict(TINY, stacks=5)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # (past every check of the model: the device check)
        MelGANStreamPool(g)


def test_the_other_pools_keep_their_refusals():
    from parallelwavegan_amd.utils import PWGStreamPool, StreamPool

    g = models.MelGANGenerator(**TINY)
    with pytest.raises(ValueError, match="in lock step through utils.MelGANLookaheadStream"):
        StreamPool(g)
    with pytest.raises(ValueError, match="MelGANGenerator is not supported"):
        PWGStreamPool(g)


def test_end_refuses_an_utterance_too_short_for_reflection():
    """``end()`` needs no device: a pool's host side alone (the schedule, the queues, ``min_frames``)."""
    pool = object.__new__(MelGANStreamPool)
    pool.min_frames, pool.batch = 4, 2
    pool._schedule = SlotSchedule(2, 4, 16, 90, 6)
    pool._queues = [[] for _ in range(2)]
    a, b = pool._schedule.open(), pool._schedule.open()
    for slot, n in ((a, 3), (b, 4)):
        pool._schedule.feed(slot, n)
        pool._queues[slot].append(torch.zeros(n, 80))
    with pytest.raises(RuntimeError, match=r"the utterance has 3 frame\(s\); reflection padding needs at least 4") as info:
        pool.end(a)
    # flush()'s words, and the slot is free again with nothing queued
    assert "the whole-utterance forward cannot pad a shorter one either" in str(info.value)
    assert pool._schedule.open_slots == [b] and pool._queues[a] == []
    assert pool._schedule.open() == a
    pool.end(b)  # exactly the minimum is an utterance
    step = pool._schedule.advance()[b]
    assert (step.action, step.row) == ("run", (0, 4, ops.SLOT_LEFT_KNOWN, 4))  # (a whole chunk, the length known)
    pool.end(a)  # one without frames closes silently, as in StreamPool
    assert pool._schedule.open_slots == [b]
    with pytest.raises(RuntimeError, match="not open"):
        pool.end(a)

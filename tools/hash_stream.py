"""SHA-256 of what the stream classes of utils/streaming.py emit and keep on a fixed case list, as JSON on stdout: what a
change of their host code that must not change a bit is compared by (run this file on both checkouts, one process each,
and compare the two objects).  GPU box only.  Every input is seeded on the CPU; only the public classes are used (and
``_halves`` / ``_cur``, which the tests pin), so the file runs unchanged on an older checkout.
Models, the small ones of the GPU tests: the causal HiFi-GAN, MelGAN and multi-band MelGAN (tests/test_stream_gpu.py,
tests/test_stream_mb_gpu.py), the small non-causal HiFi-GAN (tests/test_stream_lookahead_gpu.py), the small non-causal
MelGAN and multi-band MelGAN (tests/test_stream_melgan_lookahead_gpu.py) and the ``layers=10, stacks=1,
upsample_scales=[4, 4]`` Parallel WaveGAN, causal and non-causal.
Every case runs at batch 2, with ``use_graph`` False and True, in fp32 and (where the class has it) bf16, over one push
sequence: a zero-frame push; pushes shorter than the latency (an empty, then a short emission); the push that crosses
``settle_frames``; two equal steady pushes (graph mode replays both directions), an odd size and the first size again;
``flush()``; ``reset()`` and an utterance shorter than ``latency_frames``, flushed; for ``PWGStream`` ``reset(context)``
and two more pushes.  Per utterance one line: the hash of the emitted bytes (every push's, then the flush's), of the
tensors of ``_halves[_cur]`` and the three counters.  Noise is given explicitly; the omitted-noise path draws from the
device generator, so a second pass records its shapes and counters only.
The pools (``utils.StreamPool`` on the small non-causal HiFi-GAN, ``utils.PWGStreamPool`` on the non-causal Parallel
WaveGAN, ``utils.MelGANStreamPool`` on the small non-causal MelGAN and multi-band MelGAN, fp32; ``run_pool_case``) add
their lines where the checkout has the class."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

BATCH = 2


def models_under_test(dev):
    """name -> (stream class, model, takes noise)"""
    from parallelwavegan_amd import layers, models, utils
    from tests.golden import synth
    from tests.test_stream_mb_host import MB_CAUSAL
    from tests.test_stream_melgan_lookahead_gpu import TINY, TINY_MB
    from tests.util import synth_for

    def load(cls, cfg, seed, scale, subbands=0):
        m = cls(**cfg)
        m.load_state_dict(synth_for(m, seed, scale))
        if subbands:
            m.pqmf = layers.PQMF(subbands=subbands)
        return m.to(dev).eval()

    hifigan, melgan, pwg = models.HiFiGANGenerator, models.MelGANGenerator, models.ParallelWaveGANGenerator
    deep = dict(layers=10, stacks=1, aux_context_window=2, upsample_params={"upsample_scales": [4, 4]})
    return {
        "causal/hifigan": (utils.CausalStream, load(hifigan, synth.HIFIGAN_CAUSAL, 3, 1.0), False),
        "causal/melgan": (utils.CausalStream, load(melgan, synth.MELGAN_CAUSAL, 4, synth.MELGAN_G_SCALE), False),
        "causal/mb_melgan": (utils.CausalStream, load(melgan, MB_CAUSAL, 31, synth.MELGAN_G_SCALE, 4), False),
        "causal/pwg": (utils.PWGStream, load(pwg, dict(deep, use_causal_conv=True), 77, 1.0), True),
        "lookahead/hifigan": (utils.LookaheadStream,
                              load(hifigan, dict(synth.HIFIGAN_TINY, use_additional_convs=True), 21, 1.0), False),
        "lookahead/melgan": (utils.MelGANLookaheadStream, load(melgan, TINY, 21, synth.MELGAN_G_SCALE), False),
        "lookahead/mb_melgan": (utils.MelGANLookaheadStream, load(melgan, TINY_MB, 21, synth.MELGAN_G_SCALE, 4), False),
        "lookahead/pwg": (utils.PWGLookaheadStream, load(pwg, deep, 77, synth.PWG_G_SCALE), True),
    }


def sequence(s):
    """The pushes of the first utterance and of the second, short one, from the stream's own public numbers."""
    latency = getattr(s, "latency_frames", 0)
    settle = max(getattr(s, "settle_frames", latency), s.warmup_frames, 3)
    first = [0, 1, settle // 2, settle, 4, 4, 3, 4]  # 1 + settle // 2 < settle <= 1 + settle // 2 + settle
    short = max(getattr(s, "min_frames", 1), 3)   # (reflection cannot pad fewer than min_frames)
    assert not latency or short < latency, (short, latency)
    return first, [1, short - 1]


class Recorder:
    def __init__(self, s, noise, gen):
        self.s, self.noise, self.gen = s, noise, gen
        self.emitted, self.shapes = hashlib.sha256(), []

    def take(self, y):
        torch.cuda.synchronize()
        self.emitted.update(y.detach().cpu().contiguous().numpy().tobytes())
        self.shapes.append(list(y.shape))

    def push(self, n, explicit):
        feats = torch.randn(BATCH, n, 80, generator=self.gen)
        z = torch.randn(BATCH, n * self.s.up, generator=self.gen)
        self.take(self.s.push(feats, z) if self.noise and explicit else self.s.push(feats))

    def line(self, explicit):
        s = self.s
        torch.cuda.synchronize()
        state = hashlib.sha256()
        for t in s._halves[s._cur]:
            state.update(t.detach().cpu().contiguous().numpy().tobytes())
        counters = [s.frames_in, s.frames_out, s.samples_out]
        out = {"counters": counters, "shapes": self.shapes}
        if explicit:
            out.update(emitted=self.emitted.hexdigest(), state=state.hexdigest())
        self.emitted, self.shapes = hashlib.sha256(), []
        return out


def run_case(out, name, cls, model, noise, graph, precision, explicit):
    from parallelwavegan_amd import utils

    s = cls(model, batch=BATCH, use_graph=graph, precision=precision)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 131 + 7)
    rec = Recorder(s, noise, gen)
    first, second = sequence(s)
    tag = f"{name}/{'graph' if graph else 'eager'}/{precision}/{'noise' if explicit else 'drawn'}"
    for n in first:
        rec.push(n, explicit)
    if hasattr(s, "flush"):
        rec.take(s.flush())
    out[f"{tag}/utterance1"] = rec.line(explicit)
    s.reset()
    for n in second:
        rec.push(n, explicit)
    if hasattr(s, "flush"):
        rec.take(s.flush())
    out[f"{tag}/utterance2"] = rec.line(explicit)
    if cls is utils.PWGStream:
        s.reset(torch.randn(BATCH, model.aux_context_window, 80, generator=gen))
        for n in (2, 3):
            rec.push(n, explicit)
        out[f"{tag}/context"] = rec.line(explicit)


POOL_LENGTHS = (2, 9, 14, 5)  # shorter than the latency, not a multiple of the chunk, more utterances than slots
MELGAN_POOL_LENGTHS = (4, 9, 14, 5)  # (reflection cannot pad fewer than 4 frames)


def run_pool_case(out, name, cls, model, noise, graph, precision, lengths=POOL_LENGTHS):
    """A pool (``utils.StreamPool`` / ``utils.PWGStreamPool``; a checkout that lacks the class has no such lines) of 3
    slots and chunks of 4 frames over four utterances with staggered ``open()`` and irregular ``feed()`` sizes, noise
    given: per utterance the hash of its concatenated emissions, and at the end the state's and the counters."""
    pool = cls(model, slots=3, chunk_frames=4, use_graph=graph, precision=precision)
    gen = torch.Generator().manual_seed(sum(map(ord, name)) * 131 + 11)
    utts = [(torch.randn(t, 80, generator=gen), torch.randn(t * pool.up, generator=gen)) for t in lengths]
    pending, active, outs = list(range(len(utts))), {}, {i: [] for i in range(len(utts))}
    sizes = [1, 3, 0, 6, 2]
    for tick in range(400):
        if not pending and not active:
            break
        if pending and tick % 2 == 0 and len(pool.open_slots) < pool.slots:
            active[pool.open()] = [pending.pop(0), 0, False]
        for k, (slot, st) in enumerate(active.items()):
            if st[2]:
                continue
            f, z = utts[st[0]]
            n = min(sizes[(tick + k) % len(sizes)], f.shape[0] - st[1])
            args = (f[st[1]:st[1] + n], z[st[1] * pool.up:(st[1] + n) * pool.up]) if noise else (f[st[1]:st[1] + n],)
            pool.feed(slot, *args)
            st[1] += n
            if st[1] == f.shape[0]:
                pool.end(slot)
                st[2] = True
        for slot, y in pool.step().items():
            outs[active[slot][0]].append(y)
        for slot in [s for s in active if s not in pool.open_slots]:
            del active[slot]
    assert not pending and not active
    torch.cuda.synchronize()
    tag = f"{name}/{'graph' if graph else 'eager'}/{precision}"
    for i, ys in outs.items():
        y = torch.cat(ys).detach().cpu().contiguous()
        out[f"{tag}/utterance{i + 1}"] = {"shape": list(y.shape), "emitted": hashlib.sha256(y.numpy().tobytes()).hexdigest()}
    state = hashlib.sha256()
    for t in pool._halves[pool._cur]:
        state.update(t.detach().cpu().contiguous().numpy().tobytes())
    out[f"{tag}/end"] = {"counters": [pool.frames_in, pool.frames_out, pool.samples_out], "state": state.hexdigest()}


if __name__ == "__main__":
    from parallelwavegan_amd import utils

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = {}
    under_test = models_under_test(dev)
    for name, pool_name, noise in (("lookahead/hifigan", "StreamPool", False), ("lookahead/pwg", "PWGStreamPool", True)):
        if hasattr(utils, pool_name):
            for precision in ("fp32", "bf16"):
                for graph in (False, True):
                    run_pool_case(lines, "pool/" + name.split("/")[1], getattr(utils, pool_name), under_test[name][1], noise,
                                  graph, precision)
    if hasattr(utils, "MelGANStreamPool"):
        for name in ("lookahead/melgan", "lookahead/mb_melgan"):
            for graph in (False, True):
                run_pool_case(lines, "pool/" + name.split("/")[1], utils.MelGANStreamPool, under_test[name][1], False, graph,
                              "fp32", MELGAN_POOL_LENGTHS)
    for name, (cls, model, noise) in under_test.items():
        for precision in ("fp32",) if cls is utils.MelGANLookaheadStream else ("fp32", "bf16"):
            for graph in (False, True):
                run_case(lines, name, cls, model, noise, graph, precision, True)
                if noise:
                    run_case(lines, name, cls, model, noise, graph, precision, False)
    print(json.dumps({"lines": len(lines), "sha256": lines}, indent=1, sort_keys=True))

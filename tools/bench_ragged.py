"""16 utterances of different lengths through HiFi-GAN V1: ``utils.RaggedSynthesizer`` against the other ways to run
them, alternating in one process.  GPU box only.
usage: bench_ragged.py [--precision fp32|bf16] [--model hifigan|melgan|pwg|style_melgan] [--multiband] [--json FILE]
``--model melgan``: the same lengths and contenders through ``utils.MelGANRaggedSynthesizer`` on
``melgan.v1`` (the class defaults) or, with ``--multiband``, on the ``multi_band_melgan.v2`` generator with its PQMF
attached; seeded weights, fp32 only.
Contenders, each timed as one call over the whole list with a host clock that stops after a device synchronisation
(uploads and the slicing of the results included), ROUNDS rounds x REPS calls, alternating:
  ragged16 / ragged8  RaggedSynthesizer.synthesize_many, max_batch 16 (one group) / 8 (two groups), graphs captured
  chunked             ChunkedSynthesizer.synthesize_many (chunk_frames 256, max_batch 16), graphs captured
  chunked_cold        the same from a new ChunkedSynthesizer, i.e. with its captures: a fresh set of lengths keeps it cold
  inference           16 model.inference calls
and, on the padded (16, T_pad) block of ragged16, graph replays alone (device events):
  forward_graph       the plain forward (wrong past each item's end: zero mel frames are not zero padding)
  ragged_graph        forward_ragged (--multiband: + the PQMF synthesis of the group)
Their gap is what exactness costs on the device; the library's profiler (eager runs, per kernel family) splits it into
the zero_tail launches, the fp32 units that run as separate convolutions, the ragged split units against the plain ones
and the rest: the launches both forwards share, which read zeros past an item's end in the ragged one.  (MelGAN: the
mirror_tail launches, the ragged stacks against the plain ones, the rest.)
``--model pwg`` (fp32 or bf16): the same lengths through ``utils.PWGRaggedSynthesizer`` on
``parallel_wavegan.v1`` (the class defaults, seeded weights).  Contenders: ragged16 / ragged8 with the noise drawn on the
device, ``inference`` = 16 ``model.inference(c)`` calls as ``parallel-wavegan-decode`` makes them (each draws its noise
on the host), ``inference_noise_given`` = the same calls with the noise already on the device, and ragged16_noise_given
(host noises uploaded with the group).  ``ChunkedSynthesizer`` is no contender: it runs mel-only generators, and this
forward takes noise.  On the padded block: the plain forward (inexact) against ``forward_ragged``, graph replays; their
gap is what the dependent table read costs and the skipped tiles save; the profiler names the ragged layer launches and
the zero_tail launches.
``--model style_melgan`` (fp32): the same lengths through ``utils.StyleMelGANRaggedSynthesizer`` on the
default ``StyleMelGANGenerator`` (seeded weights).  Contenders: ragged16 / ragged8 and ``inference`` = 16
``model.inference(c)`` calls as ``parallel-wavegan-decode`` made them, every one drawing its noise on the host as
``inference`` does.  On the padded block: the plain forward (inexact: its instance norms see the padding) against
``forward_ragged``, graph replays, and the launches of one forward of each kind."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from parallelwavegan_amd import ops
from parallelwavegan_amd.graphs import GraphedInference
from parallelwavegan_amd.layers import PQMF
from parallelwavegan_amd.models import (HiFiGANGenerator, MelGANGenerator, ParallelWaveGANGenerator,
                                        StyleMelGANGenerator)
from parallelwavegan_amd.utils import (ChunkedSynthesizer, MelGANRaggedSynthesizer, PWGRaggedSynthesizer,
                                       RaggedSynthesizer, StyleMelGANRaggedSynthesizer, set_inference_precision)
from parallelwavegan_amd.utils.streaming import receptive_field_frames
from tests.golden import synth

LENGTHS = [200, 237, 281, 318, 352, 395, 431, 476, 512, 548, 590, 633, 671, 714, 762, 800]  # mel frames
ROUNDS, REPS, COLD_RUNS = 5, 3, 3


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def families(prof):
    return {k: dict(launches=int(v["launches"]), ms=float(v["ms"])) for k, v in sorted(prof.results.items())}


def split_gap(fam_plain, fam_ragged, melgan=False):
    """The profiler's kernel time of forward_ragged minus forward's, in its parts (ms)."""
    def ms(fam, name):
        return fam.get(name, dict(ms=0.0))["ms"]

    total = lambda fam: sum(v["ms"] for v in fam.values())  # noqa: E731
    if melgan:
        parts = dict(mirror_tail=ms(fam_ragged, "mirror_tail_kernel"),
                     # the ragged stacks against the plain ones: less the tiles past an item's end that only store zeros
                     ragged_stacks=ms(fam_ragged, "resstack_ragged_kernel") - ms(fam_plain, "resstack_kernel"))
        parts["same_launches_on_tails"] = total(fam_ragged) - total(fam_plain) - sum(parts.values())
        return parts
    parts = dict(
        zero_tail=ms(fam_ragged, "zero_tail_kernel"),
        # the fp32 units (csrc/resunit.hip) run as two convolutions on the fp32 MFMA kernel
        fp32_units_as_convolutions=ms(fam_ragged, "conv1d_mfma_dma_kernel") - ms(fam_plain, "conv1d_mfma_dma_kernel")
        - ms(fam_plain, "resunit_kernel"),
        # the ragged split units against the plain ones: the masks, less the tiles past an item's end that only store zeros
        ragged_units=ms(fam_ragged, "resunit_split_ragged_kernel") - ms(fam_plain, "resunit_split_kernel"))
    parts["same_launches_on_zero_tails"] = total(fam_ragged) - total(fam_plain) - sum(parts.values())
    return parts


def summary(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v), runs=v)


def main_pwg(args, dev):
    """``--model pwg``: see the module docstring."""
    model = ParallelWaveGANGenerator()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=5, g_scale=synth.PWG_G_SCALE))
    model.remove_weight_norm()
    model = model.to(dev).eval()
    if args.precision == "bf16":
        set_inference_precision(model, "bf16")
    up, w = model.upsample_factor, model.aux_context_window
    gen = torch.Generator().manual_seed(1)
    feats = [torch.randn(n, 80, generator=gen) for n in LENGTHS]
    noises = [torch.randn(n * up, generator=gen) for n in LENGTHS]
    feats_dev = [f.to(dev) for f in feats]
    noises_dev = [z.reshape(-1, 1).to(dev) for z in noises]
    ragged = {k: PWGRaggedSynthesizer(model, max_batch=k, bucket_frames=64) for k in (16, 8)}

    def inference():  # (decode's loop: the features go up per utterance, the noise is drawn by inference itself)
        with torch.no_grad():
            return [model.inference(f.to(dev)).reshape(-1) for f in feats]

    def inference_noise_given():
        with torch.no_grad():
            return [model.inference(f, z).reshape(-1) for f, z in zip(feats_dev, noises_dev)]

    runs = {"ragged16": lambda: ragged[16].synthesize_many(feats), "ragged8": lambda: ragged[8].synthesize_many(feats),
            "ragged16_noise_given": lambda: ragged[16].synthesize_many(feats, noises=noises),
            "inference": inference, "inference_noise_given": inference_noise_given}
    # what the contenders compute, on the same noise: every utterance against model.inference
    ref = inference_noise_given()
    diffs = {f"ragged{k}": max(float((y - r).abs().max()) for y, r in zip(ragged[k].synthesize_many(feats, noises=noises), ref))
             for k in ragged}
    peak = max(float(r.abs().max()) for r in ref)
    for fn in runs.values():  # warm: graphs captured, weight images cached
        fn()
    ms = {n: [] for n in runs}
    for _ in range(ROUNDS):
        for n, fn in runs.items():
            ms[n].append(wall_ms(fn, REPS))

    # the padded block of ragged16: the plain forward (inexact) against forward_ragged, graph replays
    plan = ragged[16].plan(LENGTHS)
    t_pad = plan.groups[0].t_pad
    c = torch.randn(16, 80, t_pad + 2 * w, device=dev)
    z = torch.randn(16, 1, t_pad * up, device=dev)
    frames = torch.tensor(plan.groups[0].frames, dtype=torch.int32, device=dev)
    plain_graph = GraphedInference(model)
    plain_graph(z, c)
    ragged[16]._run(c, frames, z)
    dev_ms = {"forward_graph": [], "ragged_graph": []}
    for _ in range(ROUNDS):
        dev_ms["forward_graph"].append(event_ms(lambda: plain_graph(z, c), REPS))
        dev_ms["ragged_graph"].append(event_ms(lambda: ragged[16]._run(c, frames, z), REPS))
    with torch.no_grad():
        model(z, c), model.forward_ragged(z, c, frames)
        with ops.profile() as prof_plain:
            model(z, c)
        with ops.profile() as prof_ragged:
            model.forward_ragged(z, c, frames)
    fam_plain, fam_ragged = families(prof_plain), families(prof_ragged)
    kernels_plain = sum(v["ms"] for v in fam_plain.values())
    kernels_ragged = sum(v["ms"] for v in fam_ragged.values())
    layer = "wavenet_bf16_layer_kernel" if args.precision == "bf16" else "wavenet_layer_kernel"
    layer_ragged = layer.replace("_kernel", "_ragged_kernel")
    gap = dict(zero_tail=fam_ragged.get("zero_tail_kernel", dict(ms=0.0))["ms"],
               ragged_layers=fam_ragged[layer_ragged]["ms"] - fam_plain[layer]["ms"])
    gap["same_launches"] = kernels_ragged - kernels_plain - sum(gap.values())
    samples = sum(LENGTHS) * up
    out = dict(model="parallel_wavegan.v1", precision=args.precision, lengths=LENGTHS, frames_total=sum(LENGTHS),
               weights="seeded synthetic weights (tests/golden/synth.py, seed 5), weight norm removed",
               audio_seconds_at_22050=samples / 22050.0, rounds=ROUNDS, reps=REPS,
               padded_fraction={k: ragged[k].plan(LENGTHS).padded_fraction for k in ragged},
               t_pad={k: [g.t_pad for g in ragged[k].plan(LENGTHS).groups] for k in ragged},
               wall_ms_per_list={n: summary(v) for n, v in ms.items()},
               msamples_per_s={n: samples / statistics.median(v) / 1e3 for n, v in ms.items()},
               max_abs_vs_inference_same_noise=diffs, peak_abs_of_inference=peak,
               padded_block=dict(shape=[16, 80, t_pad + 2 * w], device_ms={n: summary(v) for n, v in dev_ms.items()},
                                 launches=dict(forward=sum(v["launches"] for v in fam_plain.values()),
                                               forward_ragged=sum(v["launches"] for v in fam_ragged.values())),
                                 profiler_ms=dict(forward=kernels_plain, forward_ragged=kernels_ragged, gap=gap),
                                 families=dict(forward=fam_plain, forward_ragged=fam_ragged)))
    for n, v in ms.items():
        print(f"{n:22s} {statistics.median(v):8.2f} ms per list  [{min(v):8.2f} .. {max(v):8.2f}]  "
              f"{out['msamples_per_s'][n]:6.1f} M samples/s")
    print("max |ragged - inference| on the same noise: " + ", ".join(f"{k} {v:.2e}" for k, v in diffs.items())
          + f" (peak |inference| {peak:.2e})")
    for n, v in dev_ms.items():
        print(f"{n:22s} {statistics.median(v):8.2f} ms per replay [{min(v):8.2f} .. {max(v):8.2f}]  (16 x {t_pad} frames)")
    print(f"profiler (eager): forward {kernels_plain:.2f} ms in {out['padded_block']['launches']['forward']} launches; "
          f"forward_ragged {kernels_ragged:.2f} ms in {out['padded_block']['launches']['forward_ragged']} launches; the gap "
          "in parts: " + ", ".join(f"{k} {v:+.2f}" for k, v in gap.items()))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


def main_style_melgan(args, dev):
    """``--model style_melgan``: see the module docstring."""
    model = StyleMelGANGenerator()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=12, g_scale=0.8))
    model.remove_weight_norm()
    model = model.to(dev).eval()
    up, sf = model.upsample_factor, model.noise_upsample_factor
    gen = torch.Generator().manual_seed(1)
    feats = [torch.randn(n, 80, generator=gen) for n in LENGTHS]
    noises = [torch.randn(model.in_channels, -(-n // sf), generator=gen) for n in LENGTHS]
    ragged = {k: StyleMelGANRaggedSynthesizer(model, max_batch=k, bucket_segments=2) for k in (16, 8)}

    def inference():  # (decode's loop: the features go up per utterance, the noise is drawn by inference itself)
        with torch.no_grad():
            return [model.inference(f.to(dev)).reshape(-1) for f in feats]

    runs = {"ragged16": lambda: ragged[16].synthesize_many(feats), "ragged8": lambda: ragged[8].synthesize_many(feats),
            "inference": inference}
    # what the contenders compute, on the same noise: every utterance against model.inference
    with torch.no_grad():
        ref = [model.inference(f.to(dev), z=z.unsqueeze(0).to(dev)).reshape(-1) for f, z in zip(feats, noises)]
    diffs = {f"ragged{k}": max(float((y - r).abs().max()) for y, r in zip(ragged[k].synthesize_many(feats, noises=noises), ref))
             for k in ragged}
    peak = max(float(r.abs().max()) for r in ref)
    for fn in runs.values():  # warm: graphs captured, weight images cached
        fn()
    ms = {n: [] for n in runs}
    for _ in range(ROUNDS):
        for n, fn in runs.items():
            ms[n].append(wall_ms(fn, REPS))

    # the padded block of ragged16: the plain forward (inexact: its norms see the padding) against forward_ragged
    plan = ragged[16].plan(LENGTHS)
    s_pad = plan.groups[0].t_pad
    c = torch.randn(16, 80, s_pad * sf, device=dev)
    z = torch.randn(16, model.in_channels, s_pad, device=dev)
    segments = torch.tensor(plan.groups[0].frames, dtype=torch.int32, device=dev)
    plain_graph = GraphedInference(model)
    plain_graph(c, z)
    ragged[16]._run(c, segments, z)
    dev_ms = {"forward_graph": [], "ragged_graph": []}
    for _ in range(ROUNDS):
        dev_ms["forward_graph"].append(event_ms(lambda: plain_graph(c, z), REPS))
        dev_ms["ragged_graph"].append(event_ms(lambda: ragged[16]._run(c, segments, z), REPS))
    with torch.no_grad():
        model(c, z), model.forward_ragged(c, z, segments)
        with ops.profile() as prof_plain:
            model(c, z)
        with ops.profile() as prof_ragged:
            model.forward_ragged(c, z, segments)
    fam_plain, fam_ragged = families(prof_plain), families(prof_ragged)
    # the plain upsample / modulate / gate launches carry no profile scope (csrc/elementwise.hip): counted from
    # TADEResBlock.forward -- two modulations, two gates, the residual upsample + add, and tade2's upsample where f != 1
    unscoped = sum(5 + (b.upsample_factor != 1) for b in model.blocks)
    launches = dict(forward=sum(v["launches"] for v in fam_plain.values()) + unscoped,
                    forward_ragged=sum(v["launches"] for v in fam_ragged.values()),
                    plain_launches_without_a_profile_scope=unscoped)
    samples = sum(LENGTHS) * up
    out = dict(model="style_melgan.v1 generator (the class defaults)", precision="fp32", lengths=LENGTHS,
               frames_total=sum(LENGTHS), weights="seeded synthetic weights (tests/golden/synth.py, seed 12, g_scale 0.8), "
               "weight norm removed", audio_seconds_at_22050=samples / 22050.0, rounds=ROUNDS, reps=REPS,
               segment_frames=sf, segments=[-(-n // sf) for n in LENGTHS],
               padded_fraction={k: ragged[k].plan(LENGTHS).padded_fraction for k in ragged},
               s_pad={k: [g.t_pad for g in ragged[k].plan(LENGTHS).groups] for k in ragged},
               wall_ms_per_list={n: summary(v) for n, v in ms.items()},
               msamples_per_s={n: samples / statistics.median(v) / 1e3 for n, v in ms.items()},
               max_abs_vs_inference_same_noise=diffs, peak_abs_of_inference=peak,
               padded_block=dict(shape=[16, 80, s_pad * sf], device_ms={n: summary(v) for n, v in dev_ms.items()},
                                 launches=launches,
                                 profiler_ms=dict(forward_scoped_kernels_only=sum(v["ms"] for v in fam_plain.values()),
                                                  forward_ragged=sum(v["ms"] for v in fam_ragged.values())),
                                 families=dict(forward=fam_plain, forward_ragged=fam_ragged)))
    for n, v in ms.items():
        print(f"{n:13s} {statistics.median(v):8.2f} ms per list  [{min(v):8.2f} .. {max(v):8.2f}]  "
              f"{out['msamples_per_s'][n]:6.1f} M samples/s")
    print("max |ragged - inference| on the same noise: " + ", ".join(f"{k} {v:.2e}" for k, v in diffs.items())
          + f" (peak |inference| {peak:.2e})")
    for n, v in dev_ms.items():
        print(f"{n:13s} {statistics.median(v):8.2f} ms per replay [{min(v):8.2f} .. {max(v):8.2f}]  (16 x {s_pad} segments)")
    print(f"launches: one plain forward {launches['forward']} ({unscoped} of them counted from the code), one ragged forward "
          f"{launches['forward_ragged']}, {fam_ragged['zero_tail_kernel']['launches']} of them zero_tail")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16"))
    ap.add_argument("--model", default="hifigan", choices=("hifigan", "melgan", "pwg", "style_melgan"))
    ap.add_argument("--multiband", action="store_true", help="--model melgan: the multi_band_melgan.v2 generator + PQMF")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ragged.py measures on an MI355X: no device visible")
    melgan = args.model == "melgan"
    if melgan and args.precision != "fp32":
        raise SystemExit("bench_ragged.py: MelGAN has no bf16 mode")
    if args.multiband and not melgan:
        raise SystemExit("bench_ragged.py: --multiband goes with --model melgan")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    if args.model == "pwg":
        return main_pwg(args, dev)
    if args.model == "style_melgan":
        if args.precision != "fp32":
            raise SystemExit("bench_ragged.py: the ragged StyleMelGAN forward is fp32 only")
        return main_style_melgan(args, dev)
    if melgan:
        # seeded weights of audible amplitude (tests/golden/synth.py), as tools/bench_stream.py builds them
        params = dict(out_channels=4, channels=384, upsample_scales=[8, 4, 2], stacks=4) if args.multiband else {}
        model = MelGANGenerator(**params)
        model.load_state_dict(synth.synth_state_dict(model.state_dict(), seed=13, g_scale=synth.MELGAN_G_SCALE))
        model.remove_weight_norm()
        if args.multiband:
            model.pqmf = PQMF(subbands=4)
        name = "multi_band_melgan.v2 generator + PQMF" if args.multiband else "melgan.v1"
        weights = "seeded synthetic weights (tests/golden/synth.py, seed 13), weight norm removed"
    else:
        model = HiFiGANGenerator()
        model.remove_weight_norm()
        name = "HiFi-GAN V1"
        weights = ("N(0, 0.01) initialisation (HiFiGANGenerator()), weight norm removed; the differences against "
                   "model.inference are on waveforms of small amplitude and say only that the paths agree")
    model = model.to(dev).eval()
    if args.precision == "bf16":
        set_inference_precision(model, "bf16")
    gen = torch.Generator().manual_seed(1)
    feats = [torch.randn(n, 80, generator=gen) for n in LENGTHS]
    up = model.upsample_factor * (4 if args.multiband else 1)

    cls = MelGANRaggedSynthesizer if melgan else RaggedSynthesizer
    ragged = {16: cls(model, max_batch=16, bucket_frames=64), 8: cls(model, max_batch=8, bucket_frames=64)}
    halo = receptive_field_frames(model)
    chunked = ChunkedSynthesizer(model, chunk_frames=256, max_batch=16, halo=halo)

    def inference():
        with torch.no_grad():
            return [model.inference(f.to(dev)).reshape(-1) for f in feats]

    def chunked_cold():
        return ChunkedSynthesizer(model, chunk_frames=256, max_batch=16, halo=halo).synthesize_many(feats)

    runs = {"ragged16": lambda: ragged[16].synthesize_many(feats), "ragged8": lambda: ragged[8].synthesize_many(feats),
            "chunked": lambda: chunked.synthesize_many(feats), "inference": inference}
    # what the contenders compute: every utterance against model.inference
    ref = inference()
    diffs = {n: max(float((y - r).abs().max()) for y, r in zip(fn(), ref)) for n, fn in runs.items()}
    for fn in runs.values():  # warm: graphs captured, weight images cached
        fn()
    ms = {n: [] for n in runs}
    for _ in range(ROUNDS):
        for n, fn in runs.items():
            ms[n].append(wall_ms(fn, REPS))
    ms["chunked_cold"] = [wall_ms(chunked_cold, 1) for _ in range(COLD_RUNS)]

    # the device cost of exactness on the padded block of ragged16
    plan = ragged[16].plan(LENGTHS)
    t_pad = plan.groups[0].t_pad
    c = torch.randn(16, 80, t_pad, device=dev)
    frames = torch.tensor(plan.groups[0].frames, dtype=torch.int32, device=dev)
    plain_graph = GraphedInference(model)  # (``forward``: the sub-bands of a multi-band model, no PQMF)
    plain_graph(c)
    ragged[16]._run(c, frames)
    dev_ms = {"forward_graph": [], "ragged_graph": []}
    for _ in range(ROUNDS):
        dev_ms["forward_graph"].append(event_ms(lambda: plain_graph(c), REPS))
        dev_ms["ragged_graph"].append(event_ms(lambda: ragged[16]._run(c, frames), REPS))
    with torch.no_grad():
        model(c), model.forward_ragged(c, frames)
        with ops.profile() as prof_plain:
            model(c)
        with ops.profile() as prof_ragged:
            model.forward_ragged(c, frames)
    fam_plain, fam_ragged = families(prof_plain), families(prof_ragged)
    tail_kernel = "mirror_tail_kernel" if melgan else "zero_tail_kernel"
    zero_tail = fam_ragged.get(tail_kernel, dict(launches=0, ms=0.0))
    kernels_plain = sum(v["ms"] for v in fam_plain.values())
    kernels_ragged = sum(v["ms"] for v in fam_ragged.values())

    audio_s = sum(LENGTHS) * up / 22050.0
    out = dict(model=name, precision=args.precision, lengths=LENGTHS, frames_total=sum(LENGTHS), weights=weights,
               audio_seconds_at_22050=audio_s, rounds=ROUNDS, reps=REPS,
               padded_fraction={k: ragged[k].plan(LENGTHS).padded_fraction for k in ragged},
               t_pad={k: [g.t_pad for g in ragged[k].plan(LENGTHS).groups] for k in ragged},
               wall_ms_per_list={n: summary(v) for n, v in ms.items()},
               max_abs_vs_inference=diffs,
               padded_block=dict(shape=[16, 80, t_pad], device_ms={n: summary(v) for n, v in dev_ms.items()},
                                 launches=dict(forward=sum(v["launches"] for v in fam_plain.values()),
                                               forward_ragged=sum(v["launches"] for v in fam_ragged.values())),
                                 profiler_ms=dict(forward=kernels_plain, forward_ragged=kernels_ragged,
                                                  **{tail_kernel[:-len("_kernel")] + "_launches": zero_tail["launches"]},
                                                  gap=split_gap(fam_plain, fam_ragged, melgan)),
                                 families=dict(forward=fam_plain, forward_ragged=fam_ragged)))
    for n, v in ms.items():
        print(f"{n:13s} {statistics.median(v):8.2f} ms per list  [{min(v):8.2f} .. {max(v):8.2f}]  "
              f"max |y - inference| {diffs.get(n, float('nan')):.2e}")
    for n, v in dev_ms.items():
        print(f"{n:13s} {statistics.median(v):8.2f} ms per replay [{min(v):8.2f} .. {max(v):8.2f}]  (16 x {t_pad} frames)")
    print(f"profiler (eager): forward {kernels_plain:.2f} ms in {out['padded_block']['launches']['forward']} launches; "
          f"forward_ragged {kernels_ragged:.2f} ms in {out['padded_block']['launches']['forward_ragged']} launches, "
          f"{zero_tail['launches']} of them {tail_kernel[:-len('_kernel')]}; the gap in parts: "
          + ", ".join(f"{k} {v:+.2f}" for k, v in out["padded_block"]["profiler_ms"]["gap"].items()))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

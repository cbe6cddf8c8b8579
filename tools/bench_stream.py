"""Stateful streaming synthesis (utils.CausalStream) against the halo-recompute path, in ONE process: causal HiFi-GAN at
the V1 geometry, chunks of 4 / 8 / 32 frames, 1 and 16 concurrent streams.

A causal MelGAN at the recipe's geometry is measured at 8 frames as well.  For every combination a steady-state ``CausalStream.push`` of n frames (hipGraph replay, history kept per layer on the
device) alternates with what exists without it: one ``GraphedInference`` forward over ``left + n`` frames, ``left`` from
``receptive_field_frames`` -- what ``ChunkedSynthesizer`` runs for an interior chunk.  (The halo side is timed WITHOUT the
feature transposition and without copying the result out, both of which ``push`` includes: the comparison leans towards
the halo path.)  Device events around ``--reps`` calls after warm-up, three alternating repeats to show the spread;
launches per call counted through pwg_prof_* on one eager run of each.  GPU box only.

``--multiband``: the same method for a causal multi-band MelGAN (the multi_band_melgan.v2 generator geometry of
tests/fixtures/conf with use_causal_conv=True and its PQMF attached), 1 and 16 streams x 8 and 32 frames, into
profiles/stream_mb_infer.json.  ``push`` includes the stateful PQMF synthesis; the halo side is ONE graph of the forward
over ``left + n`` frames and ``pqmf.synthesis`` over that output.  The PQMF launch's own time per push comes from the
library's profiler scope (pwg_prof_*) on eager pushes.

``--precision bf16``: the bf16-operand stream (``CausalStream(model, precision="bf16")``, csrc/conv1d_stream_bf16.hip)
against the fp32 stream of the SAME model, same method: graph-replayed ``push`` of the two streams alternate, at the
table points of DESIGN.md s11 (HiFi-GAN V1 causal 1 / 16 streams x 4 / 8 / 32 frames, MelGAN recipe 1 / 16 x 8; with
``--multiband`` the multi-band geometry at 1 / 16 x 8 / 32 as well), into profiles/stream_bf16_infer.json.  The time
inside the two convolution kernels per push comes from the library's profiler scope on eager pushes.

``--model pwg``: the causal Parallel WaveGAN (PWG.v1 geometry, use_causal_conv=True) through ``utils.PWGStream`` -- one
launch per gated layer on the chunk (csrc/wavenet_stream.hip) -- against halo recompute, same method: pushes of 4 / 8 /
32 frames at 1 and 16 streams, into profiles/stream_pwg_infer.json.  The halo side is ONE graph of the package's own
whole-utterance causal ``forward`` over ``left + n`` frames (plus the context window), ``left`` from
``receptive_field_frames``, on static noise; ``push`` is given its noise too (it copies it into the graph's buffer).

``--lookahead``: the standard NON-causal HiFi-GAN V1 through ``utils.LookaheadStream`` (every layer in causal form on a
shifted time axis, csrc/conv1d_stream.hip's delayed form) against halo recompute, same method: steady-
state pushes of 4 / 8 / 32 frames at 1 and 16 streams, into profiles/stream_lookahead_infer.json.  The halo side is ONE
graph of the whole-utterance forward over ``left + n + right`` frames, both from ``receptive_field_frames``: a non-causal
chunk needs its future context too, and cannot be emitted before those ``right`` frames arrived either.

``--lookahead --precision bf16``: the bf16-operand look-ahead stream (``LookaheadStream(model, precision="bf16")``, the
delayed form of csrc/conv1d_stream_bf16.hip) at the same grid, four measurements alternating in one
process: the fp32 push, the bf16 push, one graph of the halo forward over ``left + n + right`` frames in fp32, and the
same halo forward of a second instance of the model put in bf16 inference precision -- the fair comparator of the bf16
push, since the whole-utterance forward runs those shapes on the bf16 matrix pipe.  Into
profiles/stream_lookahead_bf16_infer.json.

``--model pwg --lookahead``: the standard NON-causal Parallel WaveGAN (PWG.v1) through ``utils.PWGLookaheadStream`` (one
delayed launch per gated layer, csrc/wavenet_stream.hip) against halo recompute, same method: steady-
state pushes of 4 / 8 / 32 frames at 1 and 16 streams, into profiles/stream_pwg_lookahead_infer.json.  The halo side is
ONE graph of the whole-utterance forward over ``L + n + L`` frames (plus the context window), ``L`` = the stream's
latency in frames, rounded up -- the receptive field is symmetric -- on static noise.

``--model pwg [--lookahead] --precision bf16``: the bf16-operand Parallel WaveGAN streams (``PWGStream`` /
``PWGLookaheadStream`` with ``precision="bf16"``, csrc/wavenet_stream_bf16.hip) at the same grids, four
measurements alternating in one process as for ``--lookahead --precision bf16``: the fp32 push, the bf16 push, and the halo
forward of the two fp32 tools above in fp32 and -- on a second instance of the model put in bf16 inference precision -- in
bf16.  Into profiles/stream_pwg_bf16_infer.json and profiles/stream_pwg_lookahead_bf16_infer.json.

``--model melgan --lookahead [--multiband]``: the standard NON-causal MelGAN (melgan.v1 geometry) or, with ``--multiband``,
the non-causal multi-band MelGAN (multi_band_melgan.v2 generator, PQMF attached) through ``utils.MelGANLookaheadStream``
(the reflect-padded layers on the mirrored form of csrc/conv1d_stream.hip) against halo recompute, the
method of ``--lookahead``: steady-state pushes of 4 / 8 / 32 frames at 1 and 16 streams, the halo side ONE graph of the
whole-utterance forward (and, multi-band, ``pqmf.synthesis`` of its output) over ``left + n + right`` frames of the
generator's reach (the PQMF filter's own 31 samples are not added: the comparison leans towards the halo path).  Into
profiles/stream_melgan_lookahead_infer.json; ``--multiband`` adds the multi-band model to the same file.

``--pool --model pwg [--precision bf16]``: the same two measurements for ``utils.PWGStreamPool`` on the non-causal
``parallel_wavegan.v1`` against ``utils.PWGLookaheadStream`` (profiles/stream_pwg_pool[_bf16]_infer.json).
``--pool [--precision bf16]``: ``utils.StreamPool`` on the non-causal HiFi-GAN V1 (the slotted form of the stream kernels;
DESIGN.md s11.10).  (a) a step of 16 running slots -- every slot fed its 4 / 8 / 32 frames from the host, then ``step()``
-- against ``LookaheadStream(batch=16).push`` of the same frames, already on the device, alternating; with the two uploads,
the replay and the output copy of a step timed alone.  (b) 16 staggered utterances through the pool against the same 16
through 16 batch-1 ``LookaheadStream``s stepped in turn, in frames per second of wall-clock time.  Into
profiles/stream_pool_infer.json / profiles/stream_pool_bf16_infer.json.
``--pool --model melgan [--multiband]``: the same two measurements for ``utils.MelGANStreamPool`` on the non-causal
melgan.v1 geometry or, with ``--multiband``, multi_band_melgan.v2, against ``utils.MelGANLookaheadStream`` (fp32 only;
DESIGN.md s11.12; profiles/stream_melgan_pool_infer.json / profiles/stream_mb_melgan_pool_infer.json).

usage: python tools/bench_stream.py [--model pwg|melgan [--lookahead]] [--multiband] [--precision bf16] [--lookahead] [--pool] [--reps 200]
                                    [--repeats 3] [--out profiles/stream_infer.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from parallelwavegan_amd import ops  # noqa: E402
from parallelwavegan_amd.graphs import GraphedInference  # noqa: E402
from parallelwavegan_amd.layers import PQMF  # noqa: E402
from parallelwavegan_amd.models import HiFiGANGenerator, MelGANGenerator, ParallelWaveGANGenerator  # noqa: E402
from parallelwavegan_amd.utils import (CausalStream, LookaheadStream, MelGANLookaheadStream,  # noqa: E402
                                       MelGANStreamPool, PWGLookaheadStream, PWGStream, PWGStreamPool,
                                       StreamPool, set_inference_precision)
from parallelwavegan_amd.utils.streaming import receptive_field_frames  # noqa: E402
from tests.golden import synth  # noqa: E402

CHUNKS = (4, 8, 32)
STREAMS = (1, 16)
MELGAN_CHUNKS = (8,)  # a second family at one chunk size: its 1 x 1 layers run on the stream kernel too
MB_CHUNKS = (8, 32)
MELGAN_RECIPE_CAUSAL = dict(in_channels=80, out_channels=1, kernel_size=7, channels=512, upsample_scales=[8, 8, 2, 2],
                            stack_kernel_size=3, stacks=3, use_causal_conv=True)


def build_model(dev):
    """Causal HiFi-GAN V1 on seeded weights: the recipe of tests/util.py::synth_for, weight norm removed."""
    g = HiFiGANGenerator(**dict(synth.HIFIGAN_V1, use_causal_conv=True))
    g.load_state_dict(synth.synth_state_dict(g.state_dict(), seed=11, g_scale=1.25))
    g.remove_weight_norm()
    return g.to(dev).eval()


def build_noncausal(dev):
    """The standard (non-causal) HiFi-GAN V1 on the same seeded weights, weight norm removed."""
    g = HiFiGANGenerator(**synth.HIFIGAN_V1)
    g.load_state_dict(synth.synth_state_dict(g.state_dict(), seed=11, g_scale=1.25))
    g.remove_weight_norm()
    return g.to(dev).eval()


def build_melgan(dev):
    """Causal MelGAN at the recipe's geometry on seeded weights, weight norm removed."""
    g = MelGANGenerator(**MELGAN_RECIPE_CAUSAL)
    g.load_state_dict(synth.synth_state_dict(g.state_dict(), seed=12, g_scale=synth.MELGAN_G_SCALE))
    g.remove_weight_norm()
    return g.to(dev).eval()


def build_melgan_noncausal(dev):
    """The standard (non-causal) MelGAN at the recipe's geometry on the same seeded weights, weight norm removed."""
    g = MelGANGenerator(**dict(MELGAN_RECIPE_CAUSAL, use_causal_conv=False))
    g.load_state_dict(synth.synth_state_dict(g.state_dict(), seed=12, g_scale=synth.MELGAN_G_SCALE))
    g.remove_weight_norm()
    return g.to(dev).eval()


def build_multiband(dev, causal=True):
    """Multi-band MelGAN at the multi_band_melgan.v2 geometry (causal, or the standard non-causal one) on seeded
    weights, weight norm removed, PQMF attached (the recipe's default filter)."""
    import yaml

    with open(os.path.join(ROOT, "tests", "fixtures", "conf", "multi_band_melgan.v2.yaml")) as f:
        params = dict(yaml.safe_load(f)["generator_params"], use_causal_conv=causal)
    g = MelGANGenerator(**params)
    g.load_state_dict(synth.synth_state_dict(g.state_dict(), seed=13, g_scale=synth.MELGAN_G_SCALE))
    g.remove_weight_norm()
    g.pqmf = PQMF(subbands=params["out_channels"])
    return g.to(dev).eval()


def build_pwg(dev, causal=True):
    """Parallel WaveGAN at the PWG.v1 geometry (causal, or the standard non-causal one) on seeded weights, weight norm
    removed."""
    g = ParallelWaveGANGenerator(use_causal_conv=causal)
    g.load_state_dict(synth.synth_state_dict(g.state_dict(), seed=14, g_scale=synth.PWG_G_SCALE))
    g.remove_weight_norm()
    return g.to(dev).eval()


class _MelOnly(torch.nn.Module):
    """The causal PWG generator as a map from mel frames alone (zero noise, the context window replicated on both sides
    as ``inference`` does): what ``receptive_field_frames`` probes."""

    def __init__(self, model):
        super().__init__()
        self.model = model
        self.upsample_factor = model.upsample_factor

    def forward(self, c):
        from parallelwavegan_amd import functional as Fn

        w = self.model.aux_context_window
        z = torch.zeros(c.shape[0], 1, c.shape[-1] * self.upsample_factor, device=c.device)
        return self.model(z, Fn.pad1d(c, w, w, "replicate"))


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def launches(fn):
    """Kernel launches of one eager call, per kernel family (pwg_prof_*)."""
    with torch.no_grad():
        fn()
        with ops.profile() as prof:
            fn()
    fam = {k: v["launches"] for k, v in prof.results.items()}
    return sum(fam.values()), fam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--model", choices=("default", "pwg", "melgan"), default="default")
    ap.add_argument("--multiband", action="store_true")
    ap.add_argument("--precision", choices=("fp32", "bf16"), default="fp32")
    ap.add_argument("--lookahead", action="store_true")
    ap.add_argument("--pool", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.pool:
        pwg, melgan = args.model == "pwg", args.model == "melgan"
        if args.lookahead or (args.multiband and not melgan):
            ap.error("--pool is the stream pool of the non-causal HiFi-GAN, (--model pwg) Parallel WaveGAN (only --precision "
                     "goes with them) or (--model melgan [--multiband]) MelGAN")
        if melgan and args.precision != "fp32":
            ap.error("--pool --model melgan is fp32: the mirrored form of the streaming kernel has no bf16 form")
        stem = ("stream_mb_melgan_pool" if args.multiband else "stream_melgan_pool") if melgan else \
            "stream_pwg_pool" if pwg else "stream_pool"
        args.out = args.out or os.path.join(ROOT, "profiles", stem + ("_bf16" if args.precision == "bf16" else "") + "_infer.json")
        rec = {"tool": "tools/bench_stream.py --pool" + (" --model " + args.model if pwg or melgan else "")
               + (" --multiband" if args.multiband else ""),
               "device": torch.cuda.get_device_name(0), "reps": args.reps, "repeats": args.repeats, "models": {}, "points": []}
        dev = torch.device("cuda:0")
        if melgan:
            name, model = ("multi_band_melgan_v2", build_multiband(dev, causal=False)) if args.multiband else \
                ("melgan_v1", build_melgan_noncausal(dev))
        else:
            name, model = ("parallel_wavegan_v1", build_pwg(dev, causal=False)) if pwg else ("hifigan_v1", build_noncausal(dev))
        measure_pool(rec, name, model, CHUNKS, torch.Generator(device="cpu").manual_seed(100), args, dev, pwg, melgan)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps({"out": args.out, "points": [[p["chunk_frames"], p["pool_step_ms"], p["lockstep_push_ms"]]
                                                      if p["part"] == "a" else
                                                      [p["pool_frames_per_s"], p["singles_frames_per_s"]]
                                                      for p in rec["points"]]}))
        return
    if args.model == "melgan":
        if not args.lookahead or args.precision != "fp32":
            ap.error("--model melgan is the fp32 look-ahead stream of the non-causal MelGAN: pass --lookahead (no --precision)")
        args.out = args.out or os.path.join(ROOT, "profiles", "stream_melgan_lookahead_infer.json")
    elif args.lookahead and args.multiband:
        ap.error("--lookahead is the non-causal HiFi-GAN or (--model pwg) Parallel WaveGAN stream (no --multiband)")
    if args.model == "pwg" and args.multiband:
        ap.error("--model pwg is the full-band Parallel WaveGAN stream (no --multiband)")
    default_out = ("stream_pwg_lookahead_bf16_infer.json" if args.lookahead else "stream_pwg_bf16_infer.json") if args.model == "pwg" and args.precision == "bf16" else "stream_pwg_lookahead_infer.json" if args.lookahead and args.model == "pwg" else "stream_lookahead_bf16_infer.json" if args.lookahead and args.precision == "bf16" else "stream_lookahead_infer.json" if args.lookahead else "stream_pwg_infer.json" if args.model == "pwg" else "stream_bf16_infer.json" if args.precision == "bf16" else (
        "stream_mb_infer.json" if args.multiband else "stream_infer.json")
    args.out = args.out or os.path.join(ROOT, "profiles", default_out)
    dev = torch.device("cuda:0")
    rec = {"tool": "tools/bench_stream.py", "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "repeats": args.repeats, "models": {}, "points": []}
    gen = torch.Generator(device="cpu").manual_seed(100)
    if args.model == "pwg" and args.precision == "bf16":
        causal = not args.lookahead
        model16 = build_pwg(dev, causal=causal)  # the halo forward's own instance: the streamed one stays in fp32 mode
        set_inference_precision(model16, "bf16")
        measure_pwg_precision(rec, "parallel_wavegan_v1_causal" if causal else "parallel_wavegan_v1",
                              build_pwg(dev, causal=causal), model16, args.lookahead, CHUNKS, gen, args, dev)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps({"out": args.out, "points": [[p["model"], p["streams"], p["chunk_frames"], p["fp32_push_ms"],
                                                       p["bf16_push_ms"], p["halo_fp32_ms"], p["halo_bf16_ms"]]
                                                      for p in rec["points"]]}))
        return
    if args.lookahead and args.precision == "bf16":
        model16 = build_noncausal(dev)  # the halo forward's own instance: the streamed one stays in fp32 mode
        set_inference_precision(model16, "bf16")
        measure_lookahead_precision(rec, "hifigan_v1", build_noncausal(dev), model16, CHUNKS, gen, args, dev)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps({"out": args.out, "points": [[p["model"], p["streams"], p["chunk_frames"], p["fp32_push_ms"],
                                                       p["bf16_push_ms"], p["halo_fp32_ms"], p["halo_bf16_ms"]]
                                                      for p in rec["points"]]}))
        return
    if args.precision == "bf16":
        families = [("hifigan_v1_causal", build_model, CHUNKS), ("melgan_recipe_causal", build_melgan, MELGAN_CHUNKS)]
        if args.multiband:
            families.append(("multi_band_melgan_v2_causal", build_multiband, MB_CHUNKS))
        for name, build, chunks in families:
            measure_precision(rec, name, build(dev), chunks, gen, args, dev)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
        print(json.dumps({"out": args.out, "points": [[p["model"], p["streams"], p["chunk_frames"], p["fp32_push_ms"],
                                                       p["bf16_push_ms"]] for p in rec["points"]]}))
        return
    if args.model == "melgan":
        measure_lookahead(rec, "melgan_v1", build_melgan_noncausal(dev), CHUNKS, gen, args, dev, MelGANLookaheadStream)
        if args.multiband:
            measure_lookahead(rec, "multi_band_melgan_v2", build_multiband(dev, causal=False), CHUNKS, gen, args, dev,
                              MelGANLookaheadStream)
    elif args.lookahead and args.model == "pwg":
        measure_pwg_lookahead(rec, "parallel_wavegan_v1", build_pwg(dev, causal=False), CHUNKS, gen, args, dev)
    elif args.lookahead:
        measure_lookahead(rec, "hifigan_v1", build_noncausal(dev), CHUNKS, gen, args, dev)
    elif args.model == "pwg":
        measure_pwg(rec, "parallel_wavegan_v1_causal", build_pwg(dev), CHUNKS, gen, args, dev)
    elif args.multiband:
        measure(rec, "multi_band_melgan_v2_causal", build_multiband(dev), MB_CHUNKS, gen, args, dev)
    else:
        for name, model, chunks in (("hifigan_v1_causal", build_model(dev), CHUNKS),
                                    ("melgan_recipe_causal", build_melgan(dev), MELGAN_CHUNKS)):
            measure(rec, name, model, chunks, gen, args, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "points": [[p["model"], p["streams"], p["chunk_frames"], p["stream_push_ms"],
                                                   p["halo_forward_ms"]] for p in rec["points"]]}))


def measure(rec, name, model, chunks, gen, args, dev):
    left, right = receptive_field_frames(model)
    assert right == 0, "a causal generator has no look-ahead"
    pqmf = getattr(model, "pqmf", None)
    up = model.upsample_factor * (pqmf.subbands if pqmf is not None else 1)
    # what exists without the stream: the forward over left + n frames and, for a multi-band model, the synthesis of
    # that output, in one graph
    whole = model if pqmf is None else (lambda c: pqmf.synthesis(model(c)))
    rec["models"][name] = {"workload": "seeded weights, weight norm removed", "halo_left_frames": left,
                           "stream_state_bytes_per_stream": CausalStream(model, use_graph=False).state_bytes}
    for b in STREAMS:
        for n in chunks:
            feats = torch.randn(b, n, 80, generator=gen).to(dev)
            ctx = torch.randn(b, 80, left + n, generator=gen).to(dev)
            s = CausalStream(model, batch=b, use_graph=True)
            halo = GraphedInference(whole)
            for _ in range(6):  # start of stream, both graph directions, and the halo graph
                s.push(feats)
                halo(ctx)
            t_s, t_h = [], []
            for _ in range(args.repeats):
                t_s.append(event_ms(lambda: s.push(feats), args.reps))
                t_h.append(event_ms(lambda: halo(ctx), args.reps))
            eager = CausalStream(model, batch=b, use_graph=False)
            while eager.frames_out == 0:  # past the start of the stream (and a reflect-padded model's warm-up)
                eager.push(feats)
            n_s, fam_s = launches(lambda: eager.push(feats))
            n_h, fam_h = launches(lambda: whole(ctx))
            med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
            spread = max(max(t_s) - min(t_s), max(t_h) - min(t_h))
            p = {"model": name, "streams": b, "chunk_frames": n, "samples_per_push": b * n * up,
                 "stream_push_ms": round(med(t_s), 4), "stream_runs_ms": [round(t, 4) for t in t_s],
                 "halo_forward_ms": round(med(t_h), 4), "halo_runs_ms": [round(t, 4) for t in t_h],
                 "halo_frames_computed": left + n, "arithmetic_ratio_halo_over_stream": round((left + n) / n, 2),
                 "spread_ms": round(spread, 4), "speedup_stream_over_halo": round(med(t_h) / med(t_s), 3),
                 "stream_not_slower_beyond_spread": med(t_s) <= med(t_h) + spread,
                 "stream_faster_beyond_spread": med(t_s) + spread < med(t_h),
                 "real_time_factor_22050Hz": round(n * up / 22050.0 / (med(t_s) / 1e3), 1),
                 "launches_per_push_stream": n_s, "launches_per_forward_halo": n_h,
                 "stream_kernels": fam_s, "halo_kernels": fam_h}
            if pqmf is not None:
                with ops.profile() as prof:  # the PQMF launch of a push, by the library's own event scope
                    for _ in range(20):
                        eager.push(feats)
                r = prof.results["pqmf_up_stream_kernel"]
                p["pqmf_stream_launch_ms"] = round(r["ms"] / r["launches"], 5)
                p["real_time_factor_24000Hz"] = round(n * up / 24000.0 / (med(t_s) / 1e3), 1)
            rec["points"].append(p)
            print(json.dumps({k: p[k] for k in ("model", "streams", "chunk_frames", "stream_push_ms", "halo_forward_ms",
                                                "spread_ms", "speedup_stream_over_halo", "launches_per_push_stream",
                                                "launches_per_forward_halo")}), file=sys.stderr, flush=True)


def measure_pwg(rec, name, model, chunks, gen, args, dev):
    """``PWGStream.push`` against the whole-utterance causal forward over ``left + n`` frames, alternating."""
    with torch.no_grad():
        left, right = receptive_field_frames(_MelOnly(model), in_channels=80)
    assert right == 0, "a causal generator has no look-ahead"
    up, w = model.upsample_factor, model.aux_context_window
    rec["models"][name] = {"workload": "seeded weights, weight norm removed", "halo_left_frames": left,
                           "stream_state_bytes_per_stream": PWGStream(model, use_graph=False).state_bytes}
    for b in STREAMS:
        for n in chunks:
            feats = torch.randn(b, n, 80, generator=gen).to(dev)
            noise = torch.randn(b, n * up, generator=gen).to(dev)
            ctx = torch.randn(b, 80, left + n + 2 * w, generator=gen).to(dev)
            z_halo = torch.randn(b, 1, (left + n) * up, generator=gen).to(dev)
            whole = lambda c: model(z_halo, c)  # noqa: E731
            s = PWGStream(model, batch=b, use_graph=True)
            halo = GraphedInference(whole)
            for _ in range(6):  # start of stream, both graph directions, and the halo graph
                s.push(feats, noise)
                halo(ctx)
            t_s, t_h = [], []
            for _ in range(args.repeats):
                t_s.append(event_ms(lambda: s.push(feats, noise), args.reps))
                t_h.append(event_ms(lambda: halo(ctx), args.reps))
            eager = PWGStream(model, batch=b, use_graph=False)
            eager.push(feats, noise)
            n_s, fam_s = launches(lambda: eager.push(feats, noise))
            n_h, fam_h = launches(lambda: whole(ctx))
            with ops.profile() as prof:  # the layer launches of a push, by the library's own event scope
                for _ in range(10):
                    eager.push(feats, noise)
            r = prof.results["wavenet_stream_kernel"]
            med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
            spread = max(max(t_s) - min(t_s), max(t_h) - min(t_h))
            p = {"model": name, "streams": b, "chunk_frames": n, "samples_per_push": b * n * up,
                 "stream_push_ms": round(med(t_s), 4), "stream_runs_ms": [round(t, 4) for t in t_s],
                 "halo_forward_ms": round(med(t_h), 4), "halo_runs_ms": [round(t, 4) for t in t_h],
                 "halo_frames_computed": left + n, "arithmetic_ratio_halo_over_stream": round((left + n) / n, 2),
                 "spread_ms": round(spread, 4), "speedup_stream_over_halo": round(med(t_h) / med(t_s), 3),
                 "stream_not_slower_beyond_spread": med(t_s) <= med(t_h) + spread,
                 "stream_faster_beyond_spread": med(t_s) + spread < med(t_h),
                 "real_time_factor_22050Hz": round(n * up / 22050.0 / (med(t_s) / 1e3), 1),
                 "launches_per_push_stream": n_s, "launches_per_forward_halo": n_h,
                 "layer_launch_ms": round(r["ms"] / r["launches"], 5),
                 "stream_kernels": fam_s, "halo_kernels": fam_h}
            rec["points"].append(p)
            print(json.dumps({k: p[k] for k in ("model", "streams", "chunk_frames", "stream_push_ms", "halo_forward_ms",
                                                "spread_ms", "speedup_stream_over_halo", "launches_per_push_stream",
                                                "launches_per_forward_halo", "layer_launch_ms")}), file=sys.stderr,
                  flush=True)


def measure_lookahead(rec, name, model, chunks, gen, args, dev, stream_cls=LookaheadStream):
    """Steady-state ``stream_cls.push`` (``LookaheadStream``, ``MelGANLookaheadStream``) against the whole-utterance
    forward over ``left + n + right`` frames -- and, for a multi-band model, the PQMF synthesis of its output --
    alternating."""
    left, right = receptive_field_frames(model)
    pqmf = getattr(model, "pqmf", None)
    up = model.upsample_factor * (pqmf.subbands if pqmf is not None else 1)
    whole = model if pqmf is None else (lambda c: pqmf.synthesis(model(c)))
    probe = stream_cls(model, use_graph=False)
    settle = getattr(probe, "settle_frames", probe.latency_frames)  # frames before a push replays a graph
    rec["models"][name] = {"workload": "seeded weights, weight norm removed", "halo_left_frames": left,
                           "halo_right_frames": right, "latency_samples": probe.latency_samples,
                           "latency_frames": probe.latency_frames, "stream_state_bytes_per_stream": probe.state_bytes}
    for b in STREAMS:
        for n in chunks:
            feats = torch.randn(b, n, 80, generator=gen).to(dev)
            ctx = torch.randn(b, 80, left + n + right, generator=gen).to(dev)
            s = stream_cls(model, batch=b, use_graph=True)
            halo = GraphedInference(whole)
            while s.frames_in < settle + 4 * n:  # the eager start, then both graph directions; the halo graph
                s.push(feats)
                halo(ctx)
            t_s, t_h = [], []
            for _ in range(args.repeats):
                t_s.append(event_ms(lambda: s.push(feats), args.reps))
                t_h.append(event_ms(lambda: halo(ctx), args.reps))
            eager = stream_cls(model, batch=b, use_graph=False)
            while eager.frames_in < settle:  # past the partial windows
                eager.push(feats)
            n_s, fam_s = launches(lambda: eager.push(feats))
            n_h, fam_h = launches(lambda: whole(ctx))
            med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
            spread = max(max(t_s) - min(t_s), max(t_h) - min(t_h))
            p = {"model": name, "streams": b, "chunk_frames": n, "samples_per_push": b * n * up,
                 "stream_push_ms": round(med(t_s), 4), "stream_runs_ms": [round(t, 4) for t in t_s],
                 "halo_forward_ms": round(med(t_h), 4), "halo_runs_ms": [round(t, 4) for t in t_h],
                 "halo_frames_computed": left + n + right,
                 "arithmetic_ratio_halo_over_stream": round((left + n + right) / n, 2),
                 "spread_ms": round(spread, 4), "speedup_stream_over_halo": round(med(t_h) / med(t_s), 3),
                 "stream_not_slower_beyond_spread": med(t_s) <= med(t_h) + spread,
                 "stream_faster_beyond_spread": med(t_s) + spread < med(t_h),
                 "real_time_factor_22050Hz": round(n * up / 22050.0 / (med(t_s) / 1e3), 1),
                 "launches_per_push_stream": n_s, "launches_per_forward_halo": n_h,
                 "stream_kernels": fam_s, "halo_kernels": fam_h}
            rec["points"].append(p)
            print(json.dumps({k: p[k] for k in ("model", "streams", "chunk_frames", "stream_push_ms", "halo_forward_ms",
                                                "spread_ms", "speedup_stream_over_halo", "launches_per_push_stream",
                                                "launches_per_forward_halo")}), file=sys.stderr, flush=True)


def measure_pwg_lookahead(rec, name, model, chunks, gen, args, dev):
    """Steady-state ``PWGLookaheadStream.push`` against the whole-utterance forward over ``L + n + L`` frames, ``L`` the
    stream's latency in frames, alternating."""
    up, w = model.upsample_factor, model.aux_context_window
    probe = PWGLookaheadStream(model, use_graph=False)
    halo_frames = probe.latency_frames
    rec["models"][name] = {"workload": "seeded weights, weight norm removed", "halo_left_frames": halo_frames,
                           "halo_right_frames": halo_frames, "latency_samples": probe.latency_samples,
                           "latency_frames": probe.latency_frames, "stream_state_bytes_per_stream": probe.state_bytes}
    for b in STREAMS:
        for n in chunks:
            total = 2 * halo_frames + n
            feats = torch.randn(b, n, 80, generator=gen).to(dev)
            noise = torch.randn(b, n * up, generator=gen).to(dev)
            ctx = torch.randn(b, 80, total + 2 * w, generator=gen).to(dev)
            z_halo = torch.randn(b, 1, total * up, generator=gen).to(dev)
            whole = lambda c: model(z_halo, c)  # noqa: E731
            s = PWGLookaheadStream(model, batch=b, use_graph=True)
            halo = GraphedInference(whole)
            while s.frames_in < s.latency_frames + 4 * n:  # the eager start, then both graph directions; the halo graph
                s.push(feats, noise)
                halo(ctx)
            t_s, t_h = [], []
            for _ in range(args.repeats):
                t_s.append(event_ms(lambda: s.push(feats, noise), args.reps))
                t_h.append(event_ms(lambda: halo(ctx), args.reps))
            eager = PWGLookaheadStream(model, batch=b, use_graph=False)
            while eager.frames_in < eager.latency_frames:  # past the partial windows
                eager.push(feats, noise)
            n_s, fam_s = launches(lambda: eager.push(feats, noise))
            n_h, fam_h = launches(lambda: whole(ctx))
            with ops.profile() as prof:  # the layer launches of a push, by the library's own event scope
                for _ in range(10):
                    eager.push(feats, noise)
            r = prof.results["wavenet_stream_delayed_kernel"]
            med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
            spread = max(max(t_s) - min(t_s), max(t_h) - min(t_h))
            p = {"model": name, "streams": b, "chunk_frames": n, "samples_per_push": b * n * up,
                 "stream_push_ms": round(med(t_s), 4), "stream_runs_ms": [round(t, 4) for t in t_s],
                 "halo_forward_ms": round(med(t_h), 4), "halo_runs_ms": [round(t, 4) for t in t_h],
                 "halo_frames_computed": total, "arithmetic_ratio_halo_over_stream": round(total / n, 2),
                 "spread_ms": round(spread, 4), "speedup_stream_over_halo": round(med(t_h) / med(t_s), 3),
                 "stream_not_slower_beyond_spread": med(t_s) <= med(t_h) + spread,
                 "stream_faster_beyond_spread": med(t_s) + spread < med(t_h),
                 "real_time_factor_22050Hz": round(n * up / 22050.0 / (med(t_s) / 1e3), 1),
                 "launches_per_push_stream": n_s, "launches_per_forward_halo": n_h,
                 "layer_launch_ms": round(r["ms"] / r["launches"], 5),
                 "stream_kernels": fam_s, "halo_kernels": fam_h}
            rec["points"].append(p)
            print(json.dumps({k: p[k] for k in ("model", "streams", "chunk_frames", "stream_push_ms", "halo_forward_ms",
                                                "spread_ms", "speedup_stream_over_halo", "launches_per_push_stream",
                                                "launches_per_forward_halo", "layer_launch_ms")}), file=sys.stderr,
                  flush=True)


def measure_lookahead_precision(rec, name, model, model16, chunks, gen, args, dev):
    """Steady-state fp32 and bf16 ``LookaheadStream.push`` of ``model`` and the halo forward over ``left + n + right``
    frames of ``model`` (fp32) and of ``model16`` (the same weights in bf16 inference precision), alternating."""
    left, right = receptive_field_frames(model)
    up = model.upsample_factor
    probe = LookaheadStream(model, use_graph=False, precision="bf16")
    rec["models"][name] = {"workload": "seeded weights, weight norm removed", "halo_left_frames": left,
                           "halo_right_frames": right, "latency_samples": probe.latency_samples,
                           "latency_frames": probe.latency_frames, "stream_state_bytes_per_stream": probe.state_bytes}
    kernels = {"fp32": "conv1d_stream_delayed_kernel", "bf16": "conv1d_stream_bf16_delayed_kernel"}
    for b in STREAMS:
        for n in chunks:
            feats = torch.randn(b, n, 80, generator=gen).to(dev)
            ctx = torch.randn(b, 80, left + n + right, generator=gen).to(dev)
            streams = {prec: LookaheadStream(model, batch=b, use_graph=True, precision=prec) for prec in kernels}
            halos = {"fp32": GraphedInference(model), "bf16": GraphedInference(model16)}
            while streams["fp32"].frames_in < probe.latency_frames + 4 * n:  # the eager start, both graph directions
                for prec in kernels:
                    streams[prec].push(feats)
                    halos[prec](ctx)
            calls = {"fp32_push": lambda: streams["fp32"].push(feats), "bf16_push": lambda: streams["bf16"].push(feats),
                     "halo_fp32": lambda: halos["fp32"](ctx), "halo_bf16": lambda: halos["bf16"](ctx)}
            runs = {k: [] for k in calls}
            for _ in range(args.repeats):
                for k, fn in calls.items():
                    runs[k].append(event_ms(fn, args.reps))
            kernel_ms, n_launch = {}, {}
            for prec, kernel in kernels.items():
                eager = LookaheadStream(model, batch=b, use_graph=False, precision=prec)
                while eager.frames_in < eager.latency_frames:  # past the partial windows
                    eager.push(feats)
                eager.push(feats)
                with ops.profile() as prof:
                    for _ in range(10):
                        eager.push(feats)
                kernel_ms[prec] = round(prof.results[kernel]["ms"] / 10, 4)
                n_launch[prec] = prof.results[kernel]["launches"] // 10
            _, fam_h16 = launches(lambda: model16(ctx))
            med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
            spread = max(max(v) - min(v) for v in runs.values())
            p = {"model": name, "streams": b, "chunk_frames": n, "samples_per_push": b * n * up,
                 "halo_frames_computed": left + n + right, "spread_ms": round(spread, 4)}
            for k in calls:
                p[k + "_ms"] = round(med[k], 4)
                p[k + "_runs_ms"] = [round(t, 4) for t in runs[k]]
            p.update({"speedup_bf16_push_over_fp32_push": round(med["fp32_push"] / med["bf16_push"], 3),
                      "speedup_bf16_push_over_halo_fp32": round(med["halo_fp32"] / med["bf16_push"], 3),
                      "speedup_bf16_push_over_halo_bf16": round(med["halo_bf16"] / med["bf16_push"], 3),
                      "speedup_fp32_push_over_halo_fp32": round(med["halo_fp32"] / med["fp32_push"], 3),
                      "bf16_push_faster_than_halo_bf16_beyond_spread": med["bf16_push"] + spread < med["halo_bf16"],
                      "bf16_push_slower_than_halo_bf16_beyond_spread": med["bf16_push"] > med["halo_bf16"] + spread,
                      "real_time_factor_22050Hz": round(n * up / 22050.0 / (med["bf16_push"] / 1e3), 1),
                      "conv_kernel_ms_per_eager_push": kernel_ms, "conv_launches_per_push": n_launch,
                      "halo_bf16_kernels": fam_h16})
            rec["points"].append(p)
            print(json.dumps({k: p[k] for k in ("model", "streams", "chunk_frames", "fp32_push_ms", "bf16_push_ms",
                                                "halo_fp32_ms", "halo_bf16_ms", "spread_ms",
                                                "speedup_bf16_push_over_fp32_push", "speedup_bf16_push_over_halo_bf16",
                                                "conv_kernel_ms_per_eager_push")}), file=sys.stderr, flush=True)


def measure_pwg_precision(rec, name, model, model16, lookahead, chunks, gen, args, dev):
    """Steady-state fp32 and bf16 pushes of ``model`` through ``PWGStream`` (``lookahead``: ``PWGLookaheadStream``) and
    the halo forward of :func:`measure_pwg` (:func:`measure_pwg_lookahead`) of ``model`` (fp32) and of ``model16`` (the
    same weights in bf16 inference precision), alternating."""
    up, w = model.upsample_factor, model.aux_context_window
    cls = PWGLookaheadStream if lookahead else PWGStream
    probe = cls(model, use_graph=False, precision="bf16")
    if lookahead:
        left = right = probe.latency_frames
        warm = lambda s, n: s.frames_in < probe.latency_frames + 4 * n  # noqa: E731  (the eager start, both directions)
        kernels = {"fp32": "wavenet_stream_delayed_kernel", "bf16": "wavenet_stream_bf16_delayed_kernel"}
    else:
        with torch.no_grad():
            left, right = receptive_field_frames(_MelOnly(model), in_channels=80)
        assert right == 0, "a causal generator has no look-ahead"
        warm = lambda s, n: s.frames_in < 6 * n  # noqa: E731
        kernels = {"fp32": "wavenet_stream_kernel", "bf16": "wavenet_stream_bf16_kernel"}
    rec["models"][name] = {"workload": "seeded weights, weight norm removed", "halo_left_frames": left,
                           "halo_right_frames": right, "stream_state_bytes_per_stream": probe.state_bytes}
    if lookahead:
        rec["models"][name].update(latency_samples=probe.latency_samples, latency_frames=probe.latency_frames)
    for b in STREAMS:
        for n in chunks:
            total = left + n + right
            feats = torch.randn(b, n, 80, generator=gen).to(dev)
            noise = torch.randn(b, n * up, generator=gen).to(dev)
            ctx = torch.randn(b, 80, total + 2 * w, generator=gen).to(dev)
            z_halo = torch.randn(b, 1, total * up, generator=gen).to(dev)
            streams = {prec: cls(model, batch=b, use_graph=True, precision=prec) for prec in kernels}
            halos = {"fp32": GraphedInference(lambda c: model(z_halo, c)),
                     "bf16": GraphedInference(lambda c: model16(z_halo, c))}
            while warm(streams["fp32"], n):
                for prec in kernels:
                    streams[prec].push(feats, noise)
                    halos[prec](ctx)
            calls = {"fp32_push": lambda: streams["fp32"].push(feats, noise),
                     "bf16_push": lambda: streams["bf16"].push(feats, noise),
                     "halo_fp32": lambda: halos["fp32"](ctx), "halo_bf16": lambda: halos["bf16"](ctx)}
            runs = {k: [] for k in calls}
            for _ in range(args.repeats):
                for k, fn in calls.items():
                    runs[k].append(event_ms(fn, args.reps))
            layer_ms, fam = {}, {}
            for prec, kernel in kernels.items():
                eager = cls(model, batch=b, use_graph=False, precision=prec)
                while eager.frames_in < (probe.latency_frames if lookahead else 1):  # past the partial windows
                    eager.push(feats, noise)
                _, fam[prec] = launches(lambda: eager.push(feats, noise))
                with ops.profile() as prof:  # the layer launches of a push, by the library's own event scope
                    for _ in range(10):
                        eager.push(feats, noise)
                layer_ms[prec] = round(prof.results[kernel]["ms"] / prof.results[kernel]["launches"], 5)
            _, fam_h16 = launches(lambda: model16(z_halo, ctx))
            med = {k: sorted(v)[len(v) // 2] for k, v in runs.items()}
            spread = max(max(v) - min(v) for v in runs.values())
            p = {"model": name, "streams": b, "chunk_frames": n, "samples_per_push": b * n * up,
                 "halo_frames_computed": total, "spread_ms": round(spread, 4)}
            for k in calls:
                p[k + "_ms"] = round(med[k], 4)
                p[k + "_runs_ms"] = [round(t, 4) for t in runs[k]]
            p.update({"speedup_bf16_push_over_fp32_push": round(med["fp32_push"] / med["bf16_push"], 3),
                      "speedup_bf16_push_over_halo_fp32": round(med["halo_fp32"] / med["bf16_push"], 3),
                      "speedup_bf16_push_over_halo_bf16": round(med["halo_bf16"] / med["bf16_push"], 3),
                      "speedup_fp32_push_over_halo_fp32": round(med["halo_fp32"] / med["fp32_push"], 3),
                      "bf16_push_faster_than_fp32_push_beyond_spread": med["bf16_push"] + spread < med["fp32_push"],
                      "bf16_push_slower_than_fp32_push_beyond_spread": med["bf16_push"] > med["fp32_push"] + spread,
                      "bf16_push_faster_than_halo_bf16_beyond_spread": med["bf16_push"] + spread < med["halo_bf16"],
                      "bf16_push_slower_than_halo_bf16_beyond_spread": med["bf16_push"] > med["halo_bf16"] + spread,
                      "real_time_factor_22050Hz": round(n * up / 22050.0 / (med["bf16_push"] / 1e3), 1),
                      "layer_launch_ms": layer_ms, "stream_kernels": fam, "halo_bf16_kernels": fam_h16})
            rec["points"].append(p)
            print(json.dumps({k: p[k] for k in ("model", "streams", "chunk_frames", "fp32_push_ms", "bf16_push_ms",
                                                "halo_fp32_ms", "halo_bf16_ms", "spread_ms",
                                                "speedup_bf16_push_over_fp32_push", "speedup_bf16_push_over_halo_bf16",
                                                "layer_launch_ms")}), file=sys.stderr, flush=True)


def measure_pool(rec, name, model, chunks, gen, args, dev, pwg=False, melgan=False):
    """``StreamPool``, or with ``pwg`` ``PWGStreamPool`` against ``PWGLookaheadStream`` (s11.11; both
    sides get the same given noise, the pool's from the host), or with ``melgan`` ``MelGANStreamPool`` against
    ``MelGANLookaheadStream`` (s11.12), in ``args.precision``.  (a) the cost of the table: a step with all 16 slots
    running in steady state (every slot fed its ``n`` frames from the host, then ``step()``) against
    ``LookaheadStream(batch=16).push`` of ``n`` device-resident frames, alternating; and where a step's time goes (the two
    uploads, the replay, the output copy, each timed alone).  (b) what a server gains: 16 staggered utterances through
    the pool against the same 16 through 16 batch-1 ``LookaheadStream``s stepped in turn, both fed from the host, in
    frames per second of wall-clock time."""
    import time

    pqmf = getattr(model, "pqmf", None)
    up, slots = model.upsample_factor * (pqmf.subbands if pqmf is not None else 1), 16  # samples per frame
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    pool_cls, lock_cls = (PWGStreamPool, PWGLookaheadStream) if pwg else \
        (MelGANStreamPool, MelGANLookaheadStream) if melgan else (StreamPool, LookaheadStream)
    probe = pool_cls(model, slots=slots, chunk_frames=8, use_graph=False, precision=args.precision)
    rec["models"][name] = {"workload": "seeded weights, weight norm removed", "precision": args.precision, "slots": slots,
                           "latency_samples": probe.latency_samples, "pool_state_bytes": probe.state_bytes}
    for n in chunks:
        host = torch.randn(slots, n, 80, generator=gen)
        feats = host.to(dev)
        host_z = [torch.randn(slots, n * up, generator=gen)] if pwg else []  # (the noise of a Parallel WaveGAN push)
        z = [t.to(dev) for t in host_z]
        pool = pool_cls(model, slots=slots, chunk_frames=n, use_graph=True, precision=args.precision)
        lock = lock_cls(model, batch=slots, use_graph=True, precision=args.precision)
        ids = [pool.open() for _ in range(slots)]

        def pool_step():
            for s in ids:
                pool.feed(s, host[s], *(t[s] for t in host_z))
            pool.step()

        while lock.frames_in < lock.settle_frames + 4 * n:  # past every edge; both graph directions of both
            lock.push(feats, *z)
            pool_step()
        t_p, t_l = [], []
        for _ in range(args.repeats):
            t_p.append(event_ms(pool_step, args.reps))
            t_l.append(event_ms(lambda: lock.push(feats, *z), args.reps))
        graph, static_out = pool._graphs["pool"][0]
        *staged, _ = pool._staging[0]
        uploads = list(zip([pool._table] + pool._inputs, staged))  # the table(s), the features, the noise
        parts = {"upload_ms": event_ms(lambda: [d.copy_(h, non_blocking=True) for d, h in uploads], args.reps),
                 "replay_ms": event_ms(graph.replay, args.reps),
                 "output_copy_ms": event_ms(static_out.clone, args.reps),
                 "lockstep_input_copy_ms": event_ms(lambda: feats.clone(), args.reps)}
        spread = max(max(t_p) - min(t_p), max(t_l) - min(t_l))
        p = {"part": "a", "model": name, "precision": args.precision, "slots": slots, "chunk_frames": n,
             "samples_per_step": slots * n * up, "pool_step_ms": round(med(t_p), 4),
             "pool_runs_ms": [round(t, 4) for t in t_p], "lockstep_push_ms": round(med(t_l), 4),
             "lockstep_runs_ms": [round(t, 4) for t in t_l], "spread_ms": round(spread, 4),
             "pool_over_lockstep": round(med(t_p) / med(t_l), 3),
             "pool_not_slower_beyond_spread": med(t_p) <= med(t_l) + spread,
             "pool_step_parts_ms": {k: round(v, 4) for k, v in parts.items()}}
        rec["points"].append(p)
        print(json.dumps({k: p[k] for k in ("part", "chunk_frames", "pool_step_ms", "lockstep_push_ms", "spread_ms",
                                            "pool_not_slower_beyond_spread", "pool_step_parts_ms")}), file=sys.stderr,
              flush=True)

    # (b) 16 utterances of 200 .. 395 frames, one arriving every second step, 8 frames per utterance and step
    n = 8
    utts = [torch.randn(200 + 13 * i, 80, generator=gen) for i in range(slots)]
    noises = [torch.randn(u.shape[0] * up, generator=gen) for u in utts] if pwg else None
    frames = sum(u.shape[0] for u in utts)
    pool = pool_cls(model, slots=slots, chunk_frames=n, use_graph=True, precision=args.precision)
    singles = [lock_cls(model, batch=1, use_graph=True, precision=args.precision) for _ in range(slots)]

    def inputs(i, lo):
        """The next ``n`` frames of utterance ``i`` from frame ``lo`` (and their noise), on the host."""
        return (utts[i][lo:lo + n],) + ((noises[i][lo * up:(lo + n) * up],) if pwg else ())

    def serve(open_, feed, end, step):
        """Wall-clock seconds to serve every utterance; ``step()`` -> are utterances still in flight."""
        torch.cuda.synchronize()
        t0, at, tick = time.perf_counter(), {}, 0
        while True:
            if tick % 2 == 0 and tick // 2 < slots:
                at[tick // 2] = [open_(tick // 2), 0]
            for i, st in list(at.items()):
                feed(st[0], *inputs(i, st[1]))
                st[1] += n
                if st[1] >= utts[i].shape[0]:
                    end(st[0])
                    del at[i]
            busy = step()
            tick += 1
            if not at and not busy and tick // 2 >= slots:
                break
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    samples = {"pool": 0, "singles": 0}

    def pool_open(i):
        return pool.open()

    def pool_busy():
        samples["pool"] += sum(y.shape[0] for y in pool.step().values())
        return bool(pool.open_slots)

    def single_open(i):
        singles[i].reset()
        return i

    def single_feed(i, *f):
        samples["singles"] += singles[i].push(*f).shape[1]

    def single_end(i):
        samples["singles"] += singles[i].flush().shape[1]

    legs = {"pool": lambda: serve(pool_open, pool.feed, pool.end, pool_busy),
            "singles": lambda: serve(single_open, single_feed, single_end, lambda: False)}
    for fn in legs.values():  # graphs, weight images
        fn()
    samples.update(pool=0, singles=0)
    runs = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            runs[k].append(fn())
    assert samples["pool"] == samples["singles"] == args.repeats * frames * up, samples
    fps = {k: frames / med(v) for k, v in runs.items()}
    p = {"part": "b", "model": name, "precision": args.precision, "utterances": slots, "frames": frames, "chunk_frames": n,
         "pool_frames_per_s": round(fps["pool"], 1), "singles_frames_per_s": round(fps["singles"], 1),
         "pool_runs_s": [round(t, 4) for t in runs["pool"]], "singles_runs_s": [round(t, 4) for t in runs["singles"]],
         "pool_over_singles": round(fps["pool"] / fps["singles"], 2),
         "pool_real_time_streams_22050Hz": round(fps["pool"] * up / 22050.0, 1)}
    rec["points"].append(p)
    print(json.dumps(p), file=sys.stderr, flush=True)


def measure_precision(rec, name, model, chunks, gen, args, dev):
    """fp32 ``push`` and bf16 ``push`` of the same model, alternating."""
    pqmf = getattr(model, "pqmf", None)
    up = model.upsample_factor * (pqmf.subbands if pqmf is not None else 1)
    rec["models"][name] = {"workload": "seeded weights, weight norm removed",
                           "stream_state_bytes_per_stream": CausalStream(model, use_graph=False).state_bytes}
    for b in STREAMS:
        for n in chunks:
            feats = torch.randn(b, n, 80, generator=gen).to(dev)
            s32 = CausalStream(model, batch=b, use_graph=True)
            s16 = CausalStream(model, batch=b, use_graph=True, precision="bf16")
            for _ in range(6):  # start of stream and both graph directions of both
                s32.push(feats)
                s16.push(feats)
            t32, t16 = [], []
            for _ in range(args.repeats):
                t32.append(event_ms(lambda: s32.push(feats), args.reps))
                t16.append(event_ms(lambda: s16.push(feats), args.reps))
            kernel_ms, n_launch = {}, {}
            for prec, kernel in (("fp32", "conv1d_stream_kernel"), ("bf16", "conv1d_stream_bf16_kernel")):
                eager = CausalStream(model, batch=b, use_graph=False, precision=prec)
                while eager.frames_out == 0:
                    eager.push(feats)
                eager.push(feats)
                with ops.profile() as prof:
                    for _ in range(10):
                        eager.push(feats)
                kernel_ms[prec] = round(prof.results[kernel]["ms"] / 10, 4)
                n_launch[prec] = prof.results[kernel]["launches"] // 10
            med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
            spread = max(max(t32) - min(t32), max(t16) - min(t16))
            p = {"model": name, "streams": b, "chunk_frames": n, "samples_per_push": b * n * up,
                 "fp32_push_ms": round(med(t32), 4), "fp32_runs_ms": [round(t, 4) for t in t32],
                 "bf16_push_ms": round(med(t16), 4), "bf16_runs_ms": [round(t, 4) for t in t16],
                 "spread_ms": round(spread, 4), "speedup_bf16_over_fp32": round(med(t32) / med(t16), 3),
                 "bf16_not_slower_beyond_spread": med(t16) <= med(t32) + spread,
                 "bf16_faster_beyond_spread": med(t16) + spread < med(t32),
                 "conv_kernel_ms_per_eager_push": kernel_ms, "conv_launches_per_push": n_launch}
            rec["points"].append(p)
            print(json.dumps({k: p[k] for k in ("model", "streams", "chunk_frames", "fp32_push_ms", "bf16_push_ms", "spread_ms",
                                                "speedup_bf16_over_fp32", "conv_kernel_ms_per_eager_push")}),
                  file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()

"""fp32 against bf16-operand inference (utils.set_inference_precision) on the headline workload, in ONE process:
HiFi-GAN V1, B x F frames replayed as one hipGraph exactly as bench.py's headline does it, then the per-layer table of
tools/bench_conv.py's problem set for both kernels (both bf16 MFMA shapes), batch-1 latencies, and the accuracy figures
of tests/test_conv_bf16_gpu.py / tests/test_hifigan_bf16_gpu.py.  Random operands everywhere (never zeros).  GPU box only.

``--model pwg``: Parallel WaveGAN.v1 as bench.py::bench_pwg_inference runs it (B x 400 frames and B1 x 100 frames, graph
replay), fp32 and bf16 interleaved, the per-kernel table, the one-launch residual layer at every dilation (fp32 kernel
against both bf16 MFMA shapes), and the accuracy figures of tests/test_wavenet_bf16_gpu.py / tests/test_pwg_bf16_gpu.py
-> profiles/bf16_pwg_infer.json.

usage: python tools/bench_bf16.py [--model hifigan|pwg] [--batch 16] [--frames 800|400] [--steps 20] [--warmup 3]
                                  [--no-accuracy] [--no-layers] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402  (load_conf: the recipe bench.py's headline uses)
from parallelwavegan_amd import ops  # noqa: E402
from parallelwavegan_amd.graphs import GraphedInference  # noqa: E402
from parallelwavegan_amd.models import HiFiGANGenerator, ParallelWaveGANGenerator  # noqa: E402
from parallelwavegan_amd.utils import set_inference_precision  # noqa: E402

HBM_STREAM_GBS = 6300.0  # the streaming rate profiles/r06_hbm_helpers.txt measures against


def clocks():
    """Current clocks as the driver reports them (read only)."""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=30).stdout
        card = next(iter(json.loads(out).values()))
        return {k: v for k, v in card.items() if "sclk" in k or "mclk" in k}
    except Exception as e:  # noqa: BLE001  (a box without the tool still gets its record)
        return {"unavailable": repr(e)}


def timed_forward(run, c, warmup, steps):
    with torch.no_grad():
        for _ in range(warmup):
            y = run(c)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            y = run(c)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3, y


def event_ms(fn, reps=10):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def layer_problems(frames):
    rows = [("input 80->512 k7", "input", 1, dict(c_in=80, c_out=512, kernel=7, dil=1, T=frames))]
    ch, t = 512, frames
    for s, k in zip((8, 8, 2, 2), (16, 16, 4, 4)):
        rows.append((f"convT {ch}->{ch // 2} k{k} s{s}", "upsample", 1,
                     dict(c_in=ch, c_out=ch // 2, kernel=k, stride=s, T=t, transposed=True)))
        ch //= 2
        t *= s
        for ks in (3, 7, 11):
            for d in (1, 5):
                rows.append((f"res {ch} k{ks} d{d}", f"res{ch}", 4 if d == 1 else 2,
                             dict(c_in=ch, c_out=ch, kernel=ks, dil=d, T=t, res=True)))
    rows.append(("output 32->1 k7", "output", 1, dict(c_in=32, c_out=1, kernel=7, dil=1, T=t)))
    return rows


def layer_table(batch, frames, dev):
    """ms / TFLOP/s / achieved GB/s (algorithmic bytes: fp32 input + output (+ residual) + the weight image) of every
    distinct convolution of the forward, fp32 kernel next to the bf16 kernel in both MFMA shapes."""
    table, classes = [], {}
    for name, cls, count, p in layer_problems(frames):
        k = p["kernel"]
        if p.get("transposed"):
            s = p["stride"]
            t_out = p["T"] * s
            desc = ops.make_conv_desc(batch, p["c_in"], p["c_out"], p["T"], t_out, k, stride=s, pad_left=s // 2 + s % 2,
                                      transposed=True, pre_act="leaky_relu", pre_slope=0.1)
            w = torch.randn(p["c_in"], p["c_out"], k, device=dev) * 0.05
        else:
            d = p["dil"]
            t_out = p["T"]
            desc = ops.make_conv_desc(batch, p["c_in"], p["c_out"], p["T"], t_out, k, dilation=d,
                                      pad_left=(k - 1) // 2 * d, pre_act="leaky_relu", pre_slope=0.1)
            w = torch.randn(p["c_out"], p["c_in"], k, device=dev) * 0.05
        flops = 2.0 * p["c_in"] * p["c_out"] * k * p["T"] * batch
        x = torch.randn(batch, p["c_in"], p["T"], device=dev)
        bias = torch.randn(p["c_out"], device=dev)
        add1 = torch.randn(batch, p["c_out"], t_out, device=dev) if p.get("res") else None
        y = torch.empty(batch, p["c_out"], t_out, device=dev)
        nbytes = 4.0 * (x.numel() + y.numel() * (2 if add1 is not None else 1))
        wp32, wp16 = ops.pack_weight(desc, w), ops.pack_weight_bf16(desc, w)
        ms = {"fp32": event_ms(lambda: ops.conv1d_forward(desc, x, wp32, bias, add1, out=y)),
              "bf16_32x32x16": event_ms(lambda: ops.conv1d_forward_bf16(desc, x, wp16, bias, add1, out=y, mfma_shape=32)),
              "bf16_16x16x32": event_ms(lambda: ops.conv1d_forward_bf16(desc, x, wp16, bias, add1, out=y, mfma_shape=16)),
              "bf16": event_ms(lambda: ops.conv1d_forward_bf16(desc, x, wp16, bias, add1, out=y))}
        row = {"layer": name, "class": cls, "launches_per_forward": count, "T": p["T"], "gflop": flops / 1e9,
               "algorithmic_MB": nbytes / 1e6}
        for key, v in ms.items():
            wbytes = (wp32.numel() * 4 if key == "fp32" else wp16.numel())
            row[key] = {"ms": round(v, 4), "tflops": round(flops / v / 1e9, 1), "GBps": round((nbytes + wbytes) / v / 1e6, 0),
                        "frac_of_6300_GBps": round((nbytes + wbytes) / v / 1e6 / HBM_STREAM_GBS, 3)}
        table.append(row)
        c = classes.setdefault(cls, {"fp32_ms": 0.0, "bf16_ms": 0.0, "stream_ms": 0.0})
        c["fp32_ms"] += ms["fp32"] * count
        c["bf16_ms"] += ms["bf16"] * count
        c["stream_ms"] += nbytes / HBM_STREAM_GBS / 1e6 * count
        print(f"{name:26s} T={p['T']:7d} fp32 {ms['fp32'] * 1e3:8.1f} us | bf16 32x32 {ms['bf16_32x32x16'] * 1e3:8.1f} us "
              f"16x16 {ms['bf16_16x16x32'] * 1e3:8.1f} us | {row['bf16']['tflops']:7.1f} TF {row['bf16']['GBps']:6.0f} GB/s",
              file=sys.stderr, flush=True)
    for c in classes.values():
        c["bf16_fraction_of_streaming"] = round(c["stream_ms"] / c["bf16_ms"], 3)
        c["fp32_fraction_of_streaming"] = round(c["stream_ms"] / c["fp32_ms"], 3)
        for k in ("fp32_ms", "bf16_ms", "stream_ms"):
            c[k] = round(c[k], 3)
    return table, classes


def accuracy(dev):
    """The figures the tests assert on: per-layer worst relative-to-max error, and per generator case
    rms(gpu_bf16 - oracle) / rms(emulation - oracle)."""
    from tests import test_conv_bf16_gpu as tl
    from tests import test_hifigan_bf16_gpu as tg

    worst = 0.0
    for c in tl.ALL:
        for shape in (32, 16):
            y, err = tl.run_case(c, dev, shape, return_error=True)
            worst = max(worst, err)
    cases = []
    for frames, batch, seed in tg.GENERATOR_CASES:
        cases.append(tg.measure_case(frames, batch, seed, dev))
        print(cases[-1], file=sys.stderr, flush=True)
    return {"per_layer_cases": 2 * len(tl.ALL), "per_layer_worst_rel_to_max_error": worst, "per_layer_bar": tl.RTOL,
            "generator_cases": cases}


PWG_LAYER_BYTES_PER_SAMPLE = 4 * (64 + 80 + 64 + 64 + 64)  # x, c, skip sum in; x', skip sum out (fp32)
PWG_LAYER_FLOP_PER_SAMPLE = 2 * (128 * (3 * 64 + 80) + 128 * 64)


def pwg_layer_table(batch, t, dev):
    """The one-launch residual layer at every dilation of PWG.v1: fp32 kernel (csrc/wavenet.hip) next to the bf16 kernel
    (csrc/wavenet_bf16.hip) in both MFMA shapes; TFLOP/s and the fraction of the 6.3 TB/s streaming time of the
    layer's 1344 B per sample."""
    import math

    samples = batch * t
    flops, nbytes = PWG_LAYER_FLOP_PER_SAMPLE * samples, PWG_LAYER_BYTES_PER_SAMPLE * samples
    stream_ms = nbytes / HBM_STREAM_GBS / 1e6
    gen = torch.Generator(device="cpu").manual_seed(7)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)  # noqa: E731
    x, c, skips = rnd(batch, 64, t), rnd(batch, 80, t), rnd(batch, 64, t)
    ws = (rnd(128, 64, 3) * 0.07, None, rnd(128, 80, 1) * 0.1, None, rnd(64, 64, 1) * 0.12, None, rnd(64, 64, 1) * 0.12, None)
    bs = (rnd(128), rnd(64), rnd(64))
    s_out = torch.empty_like(skips)
    rows = []
    for dil in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512):
        desc = ops.make_wavenet_desc(batch, t, dil, out_mul=math.sqrt(0.5))
        img32, img16 = ops.wavenet_pack_weights(desc, *ws), ops.wavenet_bf16_pack_weights(desc, *ws)
        ms = {"fp32": event_ms(lambda: ops.wavenet_layer_forward(desc, x, c, skips, img32, *bs, skips_out=s_out)),
              "bf16_32x32x16": event_ms(lambda: ops.wavenet_bf16_layer_forward(desc, x, c, skips, img16, *bs,
                                                                               skips_out=s_out, mfma_shape=32)),
              "bf16_16x16x32": event_ms(lambda: ops.wavenet_bf16_layer_forward(desc, x, c, skips, img16, *bs,
                                                                               skips_out=s_out, mfma_shape=16)),
              "bf16": event_ms(lambda: ops.wavenet_bf16_layer_forward(desc, x, c, skips, img16, *bs, skips_out=s_out))}
        row = {"dilation": dil, "batch": batch, "T": t}
        for k, v in ms.items():
            row[k] = {"us": round(v * 1e3, 1), "tflops": round(flops / v / 1e9, 1),
                      "frac_of_streaming_time": round(stream_ms / v, 3)}
        rows.append(row)
        print(f"PWG layer d={dil:3d} B{batch} T{t}: fp32 {ms['fp32'] * 1e3:7.1f} us | bf16 32x32 {ms['bf16_32x32x16'] * 1e3:7.1f}"
              f" us 16x16 {ms['bf16_16x16x32'] * 1e3:7.1f} us | {row['bf16']['tflops']:6.1f} TF, "
              f"{row['bf16']['frac_of_streaming_time']:.2f} of streaming", file=sys.stderr, flush=True)
    return {"streaming_us_per_layer": round(stream_ms * 1e3, 1), "flop_per_sample_per_layer": PWG_LAYER_FLOP_PER_SAMPLE,
            "bytes_per_sample_per_layer": PWG_LAYER_BYTES_PER_SAMPLE, "rows": rows,
            "total_us_30_layers": {k: round(sum(r[k]["us"] for r in rows) * 3, 1)
                                   for k in ("fp32", "bf16_32x32x16", "bf16_16x16x32", "bf16")}}


def pwg_accuracy(dev):
    """The figures the PWG tests assert on: the three stage errors of every case of tests/test_wavenet_bf16_gpu.py (both
    MFMA shapes) and the error ratios of tests/test_pwg_bf16_gpu.py."""
    from tests import test_pwg_bf16_gpu as tg
    from tests import test_wavenet_bf16_gpu as tl

    stages = []
    for case in tl.CASES:
        for shape in (32, 16):
            inputs, out, desc = tl.run_layer(*case, dev, shape)
            e = tl.stage_errors(inputs, out, desc)
            stages.append(dict(B=case[0], T=case[1], dilation=case[2], with_skips=case[3], skip_mul=case[4], mfma_shape=shape,
                               **{k: float(v) for k, v in e.items()}))
            print(stages[-1], file=sys.stderr, flush=True)
    cases = []
    for frames, batch, seed in tg.GENERATOR_CASES:
        cases.append(tg.measure_case(frames, batch, seed, dev))
        print(cases[-1], file=sys.stderr, flush=True)
    return {"stage_bar_rel_to_max": tl.RTOL, "stage_errors": stages,
            "ratio_band": [tg.LOWER, tg.UPPER], "generator_cases": cases,
            "causal": tg.measure_causal(dev), "melgan_upsampler": tg.measure_melgan_upsampler(dev)}


def hifigan_bf16_digest(dev):
    """sha256 of the HiFi-GAN V1 bf16-mode output on seeded weights and input (compare across builds)."""
    import hashlib

    from tests.golden import synth
    from tests.util import synth_for

    g = HiFiGANGenerator(**synth.HIFIGAN_V1)
    g.load_state_dict(synth_for(g, 5, 1.25))
    g = g.to(dev).eval()
    set_inference_precision(g, "bf16")
    c = synth.synth_input("c", (2, 80, 100), seed=100).to(dev)
    with torch.no_grad():
        y = g(c).cpu().contiguous()
    return {"input": "HIFIGAN_V1, synth_for seed 5, c = synth_input('c', (2, 80, 100), seed=100)",
            "sha256": hashlib.sha256(y.numpy().tobytes()).hexdigest()}


def main_pwg(args):
    """Parallel WaveGAN.v1 as bench.py::bench_pwg_inference runs it (weight norm removed, B x F frames and B1 x 100
    frames under GraphedInference), fp32 and bf16 interleaved in one process."""
    dev = torch.device("cuda:0")
    conf = bench.load_conf("parallel_wavegan.v1")
    gp = conf["generator_params"]
    torch.manual_seed(99)
    g = ParallelWaveGANGenerator(**gp)
    g.remove_weight_norm()
    g = g.to(dev).eval()
    acw, hop = gp["aux_context_window"], conf["hop_size"]
    rec = {"tool": "tools/bench_bf16.py --model pwg", "workload": f"Parallel WaveGAN.v1, {args.batch} x {args.frames} frames "
           "and 1 x 100 frames, hipGraph replay (bench.py::bench_pwg_inference)", "steps": args.steps,
           "warmup": args.warmup, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
           "clocks_before": clocks()}
    head = {}
    for tag, (b, f, n) in {"batch": (args.batch, args.frames, args.steps), "B1_F100": (1, 100, 20)}.items():
        c = torch.randn(b, gp["aux_channels"], f + 2 * acw).to(dev)
        z = torch.randn(b, 1, f * hop).to(dev)
        run = GraphedInference(g)
        times, outs = {}, {}
        for _ in range(args.repeats):  # interleaved: fp32, bf16, fp32, bf16, ...
            for precision in ("fp32", "bf16"):
                set_inference_precision(g, precision)
                ms, y = timed_forward(lambda zc: run(*zc), (z, c), args.warmup, n)
                assert torch.isfinite(y).all()
                outs[precision] = y.clone()
                times.setdefault(precision, []).append(ms)
        samples = b * f * hop
        r = {"batch": b, "frames": f}
        for p, v in times.items():
            r[p] = {"ms_per_forward": round(sorted(v)[len(v) // 2], 4), "runs_ms": [round(t, 4) for t in v],
                    "spread_ms": round(max(v) - min(v), 4), "Msamples_per_s": round(samples / sorted(v)[len(v) // 2] / 1e3, 2)}
        r["speedup_bf16_over_fp32"] = round(r["fp32"]["ms_per_forward"] / r["bf16"]["ms_per_forward"], 3)
        r["bf16_faster_by_more_than_the_spread"] = (r["fp32"]["ms_per_forward"] - r["bf16"]["ms_per_forward"]
                                                    > max(r["fp32"]["spread_ms"], r["bf16"]["spread_ms"]))
        d = (outs["bf16"] - outs["fp32"]).double()
        r["bf16_vs_fp32_output"] = {"rms_difference": float(d.pow(2).mean().sqrt()),
                                    "rms_signal": float(outs["fp32"].double().pow(2).mean().sqrt())}
        head[tag] = r
        print(tag, json.dumps(r), file=sys.stderr, flush=True)
        if tag == "batch":
            kernels = {}
            for precision in ("fp32", "bf16"):
                set_inference_precision(g, precision)
                with torch.no_grad():
                    g(z, c)
                    with ops.profile() as prof:
                        g(z, c)
                kernels[precision] = {k: {"launches": v["launches"], "ms": round(v["ms"], 3)} for k, v in prof.results.items()}
            rec["kernels_of_one_eager_forward"] = kernels
    set_inference_precision(g, "fp32")
    rec["forward"] = head
    if not args.no_layers:
        rec["layer_kernel"] = pwg_layer_table(args.batch, args.frames * hop, dev)
    rec["hifigan_bf16_output"] = hifigan_bf16_digest(dev)
    if not args.no_accuracy:
        rec["accuracy"] = pwg_accuracy(dev)
    rec["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "forward": head}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("hifigan", "pwg"), default="hifigan")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frames", type=int, default=None, help="default: 800 (hifigan), 400 (pwg)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3, help="pwg: interleaved fp32 / bf16 passes (their spread is recorded)")
    ap.add_argument("--no-accuracy", action="store_true")
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--hifigan-digest-only", action="store_true",
                    help="print the sha256 of the HiFi-GAN bf16 output on seeded inputs and exit")
    ap.add_argument("--parent-ms", type=float, default=None,
                    help="ms_per_step of `python bench.py` on the parent commit, measured in the same session")
    ap.add_argument("--out", default=None, help="default: profiles/bf16_infer.json (hifigan), bf16_pwg_infer.json (pwg)")
    args = ap.parse_args()
    if args.hifigan_digest_only:
        print(json.dumps(hifigan_bf16_digest(torch.device("cuda:0"))))
        return
    if args.model == "pwg":
        args.frames = args.frames or 400
        args.out = args.out or os.path.join(ROOT, "profiles", "bf16_pwg_infer.json")
        return main_pwg(args)
    args.frames = args.frames or 800
    args.out = args.out or os.path.join(ROOT, "profiles", "bf16_infer.json")
    dev = torch.device("cuda:0")

    # the headline workload, set up as bench.py does
    g_params = bench.load_conf("hifigan.v1")["generator_params"]
    torch.manual_seed(1234)
    g = HiFiGANGenerator(**g_params)
    g.remove_weight_norm()
    g = g.to(dev).eval()
    c = torch.randn(args.batch, 80, args.frames, generator=torch.Generator(device="cpu").manual_seed(100)).to(dev)
    samples = args.batch * args.frames * g.upsample_factor
    rec = {"tool": "tools/bench_bf16.py", "workload": f"HiFi-GAN V1, {args.batch} x {args.frames} frames, hipGraph replay, "
           "MRF blocks as graph branches", "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "clocks_before": clocks()}

    g.branch_streams = True
    run = GraphedInference(g)
    head = {}
    outs = {}
    for precision in ("fp32", "bf16", "fp32", "bf16"):  # twice, interleaved: the second pass is the record
        n = set_inference_precision(g, precision)
        ms, y = timed_forward(run, c, args.warmup, args.steps)
        assert torch.isfinite(y).all()
        outs[precision] = y.clone()
        head.setdefault(precision, []).append(ms)
        print(f"{precision}: {n} convolutions, {ms:.3f} ms per forward, {samples / ms / 1e3:.2f} M samples/s",
              file=sys.stderr, flush=True)
    g.branch_streams = False
    rec["headline"] = {p: {"ms_per_forward": round(v[-1], 4), "ms_per_forward_first_pass": round(v[0], 4),
                           "Msamples_per_s": round(samples / v[-1] / 1e3, 2)} for p, v in head.items()}
    rec["headline"]["speedup_bf16_over_fp32"] = round(head["fp32"][-1] / head["bf16"][-1], 3)
    d = (outs["bf16"] - outs["fp32"]).double()
    rec["headline"]["bf16_vs_fp32_output"] = {"rms_difference": float(d.pow(2).mean().sqrt()),
                                              "rms_signal": float(outs["fp32"].double().pow(2).mean().sqrt()),
                                              "bit_identical": bool(torch.equal(outs["bf16"], outs["fp32"]))}
    if args.parent_ms is not None:
        rec["headline"]["parent_commit_bench_py_ms_per_step"] = args.parent_ms
        rec["headline"]["bf16_over_parent"] = round(head["bf16"][-1] / args.parent_ms, 4)
        rec["headline"]["fp32_over_parent"] = round(head["fp32"][-1] / args.parent_ms, 4)

    # per-kernel launch accounting of one eager forward in each mode (pwg_prof_*)
    kernels = {}
    for precision in ("fp32", "bf16"):
        set_inference_precision(g, precision)
        with torch.no_grad():
            g(c)
            with ops.profile() as prof:
                g(c)
        kernels[precision] = {k: {"launches": v["launches"], "ms": round(v["ms"], 3)} for k, v in prof.results.items()}
    rec["kernels_of_one_eager_forward"] = kernels

    # batch-1 latencies under GraphedInference
    lat = {}
    for frames in (100, 800):
        c1 = torch.randn(1, 80, frames, generator=torch.Generator(device="cpu").manual_seed(frames)).to(dev)
        for precision in ("fp32", "bf16"):
            set_inference_precision(g, precision)
            ms, _ = timed_forward(GraphedInference(g), c1, 3, 20)
            lat[f"B1_F{frames}_{precision}_ms"] = round(ms, 4)
    rec["latency"] = lat
    set_inference_precision(g, "fp32")

    if not args.no_layers:
        rec["layers"], rec["layer_classes"] = layer_table(args.batch, args.frames, dev)
        tot = {k: sum(r[k]["ms"] * r["launches_per_forward"] for r in rec["layers"]) for k in
               ("fp32", "bf16", "bf16_32x32x16", "bf16_16x16x32")}
        rec["layer_totals_ms"] = {k: round(v, 3) for k, v in tot.items()}
    if not args.no_accuracy:
        rec["accuracy"] = accuracy(dev)
    rec["clocks_after"] = clocks()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "headline": rec["headline"], "latency": lat}))


if __name__ == "__main__":
    main()

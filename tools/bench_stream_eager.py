"""Eager (``use_graph=False``) ms per push / pool step and launches per push of the checkout this file is run FROM (the
current directory), for what a heavier host-side walk would show up in: a graph replay hides the host, an eager push is
bound by it.  Models of tools/bench_stream.py, 8 frames at batch 1: ``CausalStream`` on the causal HiFi-GAN V1 and the
causal MelGAN recipe, ``MelGANLookaheadStream`` on ``melgan.v1``, ``LookaheadStream`` on HiFi-GAN V1, and a ``StreamPool``
step of 16 running slots fed from the host.  Wall clock over ``REPS`` calls with one synchronize, median and max - min of
``REPEATS``; launches per call through pwg_prof_* as in tools/bench_stream.py.  GPU box only.

To compare two checkouts, run this file from the root of each, alternating, one process each:
``python tools/bench_stream_eager.py LABEL OUT.json`` (the file only uses public classes, so it runs on an older
checkout given by path)."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

from parallelwavegan_amd.utils import CausalStream, LookaheadStream, MelGANLookaheadStream, StreamPool  # noqa: E402
from tools import bench_stream as B  # noqa: E402

REPS, REPEATS, N = 100, 5, 8


def wall_ms(fn):
    runs = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) * 1e3 / REPS)
    return runs


def point(runs, launches, kernels, what):
    return {f"eager_{what}_ms": sorted(runs)[len(runs) // 2], "runs_ms": runs, "spread_ms": max(runs) - min(runs),
            f"launches_per_{what}": launches, "kernels": kernels}


def main():
    label, out = sys.argv[1], sys.argv[2]
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(5)
    feats = torch.randn(1, N, 80, generator=gen).to(dev)
    rec = {"label": label, "reps": REPS, "repeats": REPEATS, "chunk_frames": N, "modes": {}}
    cases = [("default/hifigan_v1_causal", CausalStream, B.build_model),
             ("default/melgan_recipe_causal", CausalStream, B.build_melgan),
             ("melgan_lookahead/melgan_v1", MelGANLookaheadStream, B.build_melgan_noncausal),
             ("lookahead/hifigan_v1", LookaheadStream, B.build_noncausal)]
    for name, cls, build in cases:
        s = cls(build(dev), batch=1, use_graph=False)
        while s.frames_in < getattr(s, "settle_frames", 0) + 4 * N or s.frames_out == 0:  # past every edge
            s.push(feats)
        runs = wall_ms(lambda: s.push(feats))
        rec["modes"][name] = point(runs, *B.launches(lambda: s.push(feats)), "push")
    slots = 16
    host = torch.randn(slots, N, 80, generator=gen)
    pool = StreamPool(B.build_noncausal(dev), slots=slots, chunk_frames=N, use_graph=False)
    ids = [pool.open() for _ in range(slots)]

    def pool_step():
        for i in ids:
            pool.feed(i, host[i])
        pool.step()

    for _ in range(pool.latency_samples // (N * pool.up) + 6):
        pool_step()
    runs = wall_ms(pool_step)
    rec["modes"]["pool/hifigan_v1"] = point(runs, *B.launches(pool_step), "step")
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({k: {a: (round(b, 4) if isinstance(b, float) else b) for a, b in v.items()
                          if a not in ("kernels", "runs_ms")} for k, v in rec["modes"].items()}))


if __name__ == "__main__":
    main()

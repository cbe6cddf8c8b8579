"""``parallel-wavegan-decode``: dumped mel features -> ``<utt_id>_gen.wav`` with a trained generator, the command line
of the reference's ``bin/decode.py`` (its mel -> waveform case, decode.py:158-248) on the HIP kernels.

A non-causal HiFi-GAN checkpoint is decoded ``--batch-size`` utterances per forward through
``utils.RaggedSynthesizer`` -- every utterance exactly what ``model.inference`` gives for it alone --
a non-causal, reflect-padded (multi-band) MelGAN checkpoint through ``utils.MelGANRaggedSynthesizer`` (s9.5), and a
Parallel WaveGAN checkpoint whose ``ragged_unsupported_reason()`` is None (the non-causal v1 geometry) through
``utils.PWGRaggedSynthesizer`` (s9.6), its noise drawn on the device, and a StyleMelGAN checkpoint with one output
channel through ``utils.StyleMelGANRaggedSynthesizer`` (s9.7), its noise drawn on the host utterance by utterance as
``model.inference`` draws it; every other supported generator -- a causal
Parallel WaveGAN, one with a MelGAN upsampler or other channel widths -- runs the reference's loop over
``model.inference`` (decode.py:214-243).  The float ->
int16 step is ``utils.to_pcm16`` on the device and the files are written with the standard library's ``wave`` module.
The RTF is timed after a device synchronisation; the reference stops its clock without one.
"""
import argparse
import logging
import os
import time
import wave

import numpy as np
import torch


def write_wav_pcm16(path, pcm, sampling_rate):
    """``pcm``: int16 samples (one channel) -> a PCM_16 WAV file."""
    pcm = np.ascontiguousarray(np.asarray(pcm).reshape(-1))
    if pcm.dtype != np.int16:
        raise ValueError(f"write_wav_pcm16: expected int16 samples, got {pcm.dtype}")
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(int(sampling_rate))
        f.writeframes(pcm.astype("<i2", copy=False).tobytes())


def read_wav_pcm16(path):
    """A one-channel PCM_16 WAV file -> ``(int16 samples, sampling_rate)``."""
    with wave.open(path, "rb") as f:
        if f.getnchannels() != 1 or f.getsampwidth() != 2:
            raise ValueError(f"read_wav_pcm16: {path} is not one-channel PCM_16")
        return np.frombuffer(f.readframes(f.getnframes()), dtype="<i2").astype(np.int16), f.getframerate()


def _parser():
    p = argparse.ArgumentParser(description="Decode dumped features with a trained generator on MI355X "
                                            "(see parallelwavegan_amd/bin/decode.py).")
    p.add_argument("--scp", default=None, type=str, help="kaldi-style feats.scp (not supported here)")
    p.add_argument("--dumpdir", default=None, type=str, help="directory including the feature files")
    p.add_argument("--segments", default=None, type=str, help="kaldi-style segments (not supported here)")
    p.add_argument("--outdir", type=str, required=True, help="directory to save the generated speech")
    p.add_argument("--checkpoint", type=str, required=True, help="checkpoint file to be loaded")
    p.add_argument("--config", default=None, type=str,
                   help="yaml format configuration file (default: config.yml beside the checkpoint)")
    p.add_argument("--normalize-before", default=False, action="store_true",
                   help="normalise the features with the registered statistics before the model")
    p.add_argument("--batch-size", default=16, type=int,
                   help="utterances per forward of a non-causal HiFi-GAN, MelGAN or Parallel WaveGAN "
                        "(utils.RaggedSynthesizer / utils.MelGANRaggedSynthesizer / utils.PWGRaggedSynthesizer; "
                        "default 16); other generators decode one utterance per call")
    p.add_argument("--verbose", type=int, default=1, help="logging level; higher is more logging")
    return p


def _melgan_is_ragged(model):
    """Does ``utils.MelGANRaggedSynthesizer`` take this ``MelGANGenerator``: non-causal, every padding a
    ``ReflectionPad1d``, and one waveform per item (one output channel, or sub-bands with the PQMF ``load_model``
    attached)?"""
    try:
        walk = model._ragged_walk()
    except ValueError:
        return False
    return walk[-1][0].out_channels == 1 or getattr(model, "pqmf", None) is not None


def main(argv=None):
    """``parallel-wavegan-decode`` (see the module docstring)."""
    import yaml

    from ..datasets import MelDataset
    from ..models import HiFiGANGenerator, MelGANGenerator, ParallelWaveGANGenerator, StyleMelGANGenerator
    from ..utils import (MelGANRaggedSynthesizer, PWGRaggedSynthesizer, RaggedSynthesizer, StyleMelGANRaggedSynthesizer,
                         load_model)
    from ..utils.streaming import to_pcm16

    args = _parser().parse_args(argv)
    level = logging.DEBUG if args.verbose > 1 else logging.INFO if args.verbose > 0 else logging.WARN
    logging.basicConfig(level=level, format="%(asctime)s (%(module)s:%(lineno)d) %(levelname)s: %(message)s")
    if args.scp is not None and args.dumpdir is None:
        raise NotImplementedError("kaldi scp input is Kaldi glue (out of scope, SURVEY.md s2): use --dumpdir")
    if (args.scp is None) == (args.dumpdir is None):
        raise ValueError("give either --dumpdir or --scp, not both and not neither")
    if args.batch_size < 1:
        raise ValueError("--batch-size must be >= 1")
    if args.config is None:
        args.config = os.path.join(os.path.dirname(args.checkpoint), "config.yml")
    with open(args.config) as f:
        config = yaml.load(f, Loader=yaml.Loader)
    config.update(vars(args))
    gtype = config.get("generator_type", "ParallelWaveGANGenerator")
    if "VQVAE" in gtype or gtype == "UHiFiGANGenerator" or config.get("use_local_condition") \
            or config.get("use_global_condition"):
        raise NotImplementedError(f"{gtype} / conditioning inputs: only the mel -> waveform case is decoded here "
                                  "(SURVEY.md s2)")
    if not torch.cuda.is_available():
        raise RuntimeError("parallel-wavegan-decode of this package needs an MI355X: there is no CPU compute path")
    device = torch.device("cuda")
    os.makedirs(args.outdir, exist_ok=True)

    model = load_model(args.checkpoint, config)
    if args.normalize_before and not (hasattr(model, "mean") and hasattr(model, "scale")):
        raise ValueError("--normalize-before needs the feature statistics (stats.h5 / stats.npy beside the checkpoint)")
    model.remove_weight_norm()
    model = model.eval().to(device)

    fmt = config.get("format", "hdf5")
    if fmt not in ("hdf5", "npy"):
        raise ValueError(f"format: {fmt!r} in the config (only hdf5 and npy dumps are read)")
    dataset = MelDataset(args.dumpdir, format=fmt, return_utt_id=True)
    logging.info(f"{len(dataset)} utterances to decode from {args.dumpdir}.")
    rate = config["sampling_rate"]

    def save(utt_id, pcm):
        write_wav_pcm16(os.path.join(args.outdir, f"{utt_id}_gen.wav"), pcm.cpu().numpy(), rate)

    ragged = isinstance(model, HiFiGANGenerator) and not model.use_causal_conv \
        and model.output_conv[1].out_channels == 1
    ragged_melgan = isinstance(model, MelGANGenerator) and _melgan_is_ragged(model)
    ragged_pwg = isinstance(model, ParallelWaveGANGenerator) and model.ragged_unsupported_reason() is None
    ragged_style = isinstance(model, StyleMelGANGenerator) and model.output_conv[0].out_channels == 1
    total_rtf, n_done = 0.0, 0
    if ragged or ragged_melgan or ragged_pwg or ragged_style:
        cls = RaggedSynthesizer if ragged else MelGANRaggedSynthesizer if ragged_melgan else \
            PWGRaggedSynthesizer if ragged_pwg else StyleMelGANRaggedSynthesizer
        synth = cls(model, max_batch=args.batch_size)
        logging.info(f"{gtype}: {args.batch_size} utterances of their own lengths per forward "
                     f"({type(synth).__name__}).")
        # one call per batch_size utterances in dump order: the host holds that many utterances at a time
        for at in range(0, len(dataset), args.batch_size):
            items = [dataset[i] for i in range(at, min(at + args.batch_size, len(dataset)))]
            torch.cuda.synchronize()
            start = time.time()
            pcms = synth.synthesize_many_pcm16([c for _, c in items], normalize_before=args.normalize_before)
            torch.cuda.synchronize()
            rtf = (time.time() - start) / (sum(len(p) for p in pcms) / rate)
            logging.info(f"[decode] {at + len(items)}/{len(dataset)} RTF = {rtf:.4f}")
            total_rtf += rtf * len(items)
            for (utt_id, _), pcm in zip(items, pcms):
                save(utt_id, pcm)
            n_done += len(items)
    else:
        with torch.no_grad():
            for utt_id, c in dataset:
                c = torch.tensor(c, dtype=torch.float).to(device)
                torch.cuda.synchronize()
                start = time.time()
                pcm = to_pcm16(model.inference(c=c, normalize_before=args.normalize_before).reshape(-1))
                torch.cuda.synchronize()
                rtf = (time.time() - start) / (len(pcm) / rate)
                logging.info(f"[decode] {utt_id} RTF = {rtf:.4f}")
                total_rtf += rtf
                save(utt_id, pcm)
                n_done += 1
    logging.info(f"Wrote {n_done} files to {args.outdir}; mean RTF {total_rtf / max(n_done, 1):.4f} (synchronised).")


if __name__ == "__main__":
    main()

"""CPU: the host side of ragged batches -- the three exported symbols and what they refuse without a
device, ``RaggedSynthesizer``'s plan and refusals, ``MelDataset``, the WAV writer and the command line's argument
errors."""
import ctypes

import numpy as np
import pytest
import torch

from parallelwavegan_amd import _lib, ops
from parallelwavegan_amd.bin import decode
from parallelwavegan_amd.datasets import MelDataset
from parallelwavegan_amd.models import HiFiGANGenerator, MelGANGenerator, ParallelWaveGANGenerator
from parallelwavegan_amd.utils import RaggedSynthesizer
from tests.golden import synth


def _last_error():
    return _lib.lib().pwg_last_error().decode()


def _p(addr):
    return ctypes.c_void_p(addr)


def test_symbols_are_exported_and_the_abi_stays():
    lib = _lib.lib()
    for name in ("pwg_zero_tail", "pwg_resunit_split_ragged_supported", "pwg_resunit_split_forward_ragged"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 15 and lib.pwg_abi_version() == 15


def test_ragged_unit_supported_is_a_function_of_descriptor_and_rate():
    for c in (32, 64):
        for rate in (4, 128):
            for pair in (True, False):
                desc = ops.make_resunit_desc(3, c, 1000, 7, 3, pair)
                assert ops.resunit_split_ragged_supported(desc, rate), (c, rate, pair)
        for rate in (1, 2, 6, 0, -4):
            assert not ops.resunit_split_ragged_supported(ops.make_resunit_desc(3, c, 1000, 7, 3), rate), (c, rate)
            assert f"rate = {rate}" in _last_error() and "multiple of 4" in _last_error()
    # what the plain query refuses, with the plain query's reason
    for desc, reason in ((ops.make_resunit_desc(1, 128, 64, 3, 1), "channels = 128"),
                         (ops.make_resunit_desc(1, 32, 66, 3, 1), "multiple of 4"),
                         (ops.make_resunit_desc(1, 32, 64, 4, 1), "odd"),
                         (ops.make_resunit_desc(1, 64, 64, 3, 30), "LDS")):
        assert not ops.resunit_split_supported(desc)
        assert not ops.resunit_split_ragged_supported(desc, 4)
        assert reason in _last_error(), (reason, _last_error())


def test_zero_tail_refuses_bad_arguments_without_a_device():
    lib = _lib.lib()
    assert lib.pwg_zero_tail(None, _p(64), 1, 1, 8, 1, None) != 0 and "NULL" in _last_error()
    assert lib.pwg_zero_tail(_p(64), None, 1, 1, 8, 1, None) != 0 and "NULL" in _last_error()
    assert lib.pwg_zero_tail(_p(66), _p(64), 1, 1, 8, 1, None) != 0 and "aligned" in _last_error()
    assert lib.pwg_zero_tail(_p(64), _p(66), 1, 1, 8, 1, None) != 0 and "aligned" in _last_error()
    for rate in (0, -1):
        assert lib.pwg_zero_tail(_p(64), _p(64), 1, 1, 8, rate, None) != 0 and f"rate = {rate}" in _last_error()
    for batch, channels, t in ((0, 1, 8), (65536, 1, 8), (1, 0, 8), (1, 1, 0)):
        assert lib.pwg_zero_tail(_p(64), _p(64), batch, channels, t, 1, None) != 0 and "bad shape" in _last_error()


def test_ragged_unit_refuses_bad_arguments_without_a_device():
    lib = _lib.lib()
    desc = ops.make_resunit_desc(2, 32, 256, 3, 1)

    def call(frames, rate, x=64):
        return lib.pwg_resunit_split_forward_ragged(ctypes.byref(desc), _p(x), _p(64), None, _p(64), None, None, _p(128),
                                                    16, frames, rate, None)

    assert call(None, 4) != 0 and "NULL frames" in _last_error()
    assert call(_p(66), 4) != 0 and "4-B aligned" in _last_error()
    for rate in (0, -4, 6):
        assert call(_p(64), rate) != 0 and f"rate = {rate}" in _last_error()
    # ... and everything the plain launch refuses (here: x not 16-B aligned), still without a launch
    assert call(_p(64), 4, x=68) != 0 and "16-B aligned" in _last_error()


def test_plan_groups_sorts_buckets_and_fills():
    lengths = [5, 90, 33, 64, 65, 1, 12]
    plan = RaggedSynthesizer.plan_groups(lengths, max_batch=4, bucket_frames=32)
    assert [g.indices for g in plan.groups] == [(5, 0, 6, 2), (3, 4, 1)]
    assert [g.frames for g in plan.groups] == [(1, 5, 12, 33), (64, 65, 90, 0)], "the partial group is filled with 0"
    assert [g.t_pad for g in plan.groups] == [64, 96]
    assert plan.padded_fraction == pytest.approx(1 - sum(lengths) / (4 * 64 + 4 * 96))
    # every input exactly once: the order can be restored
    assert sorted(i for g in plan.groups for i in g.indices) == list(range(len(lengths)))
    # a length on the bucket boundary is not rounded further; ties keep the input order
    plan = RaggedSynthesizer.plan_groups([64, 64, 32], max_batch=2, bucket_frames=32)
    assert [(g.indices, g.frames, g.t_pad) for g in plan.groups] == [((2, 0), (32, 64), 64), ((1,), (64, 0), 64)]
    # one full group: nothing to fill, no padding at equal lengths
    plan = RaggedSynthesizer.plan_groups([8, 8], max_batch=2, bucket_frames=8)
    assert plan.groups[0].frames == (8, 8) and plan.padded_fraction == 0.0
    assert RaggedSynthesizer.plan_groups([], 4, 32) == ([], 0.0)


def test_plan_groups_refuses_empty_and_over_long_items():
    with pytest.raises(ValueError, match="item 1 is empty"):
        RaggedSynthesizer.plan_groups([5, 0], 4, 32)
    with pytest.raises(ValueError, match="item 0 has 101 frames"):
        RaggedSynthesizer.plan_groups([101, 3], 4, 32, max_frames=100)


def test_refused_models_and_cpu_tensors():
    with pytest.raises(ValueError, match="MelGANGenerator.*ChunkedSynthesizer"):
        RaggedSynthesizer(MelGANGenerator())
    with pytest.raises(ValueError, match="ParallelWaveGANGenerator.*ChunkedSynthesizer"):
        RaggedSynthesizer(ParallelWaveGANGenerator())
    causal = HiFiGANGenerator(**synth.HIFIGAN_CAUSAL)
    with pytest.raises(ValueError, match="HiFiGANGenerator is causal.*ChunkedSynthesizer"):
        RaggedSynthesizer(causal)
    with pytest.raises(ValueError, match="causal generator has no ragged forward"):
        causal.forward_ragged(torch.zeros(1, 80, 8), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="emits 4 channels"):
        RaggedSynthesizer(HiFiGANGenerator(**dict(synth.HIFIGAN_TINY, out_channels=4)))
    g = HiFiGANGenerator(**synth.HIFIGAN_TINY)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        RaggedSynthesizer(g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        g.forward_ragged(torch.zeros(2, 80, 8), torch.tensor([8, 3], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.zero_tail(torch.zeros(2, 3, 8), torch.tensor([8, 3], dtype=torch.int32), 1)


def test_mel_dataset_reads_npy_dumps(tmp_path):
    rng = np.random.default_rng(0)
    mels = {f"utt{i}": rng.standard_normal((5 + 3 * i, 80)).astype(np.float32) for i in range(3)}
    for utt, mel in mels.items():
        np.save(tmp_path / f"{utt}-feats.npy", mel)
        np.save(tmp_path / f"{utt}-wave.npy", np.zeros(4, np.float32))  # (not a feature file)
    ds = MelDataset(str(tmp_path), format="npy")
    assert len(ds) == 3 and ds.utt_ids == ["utt0", "utt1", "utt2"]
    assert ds[1].dtype == np.float32 and np.array_equal(ds[1], mels["utt1"])
    ds = MelDataset(str(tmp_path), format="npy", return_utt_id=True, allow_cache=True)
    assert [(u, m.shape) for u, m in ds] == [(u, m.shape) for u, m in mels.items()]
    assert ds[2][1] is ds[2][1], "allow_cache keeps the loaded item"
    assert len(MelDataset(str(tmp_path), format="npy", mel_length_threshold=5)) == 2
    with pytest.raises(ValueError, match="hdf5 or npy"):
        MelDataset(str(tmp_path), format="kaldi")


def test_wav_writer_round_trips_int16(tmp_path):
    pcm = np.array([0, 1, -1, 32767, -32768, 12345, -12345], dtype=np.int16)
    path = str(tmp_path / "a.wav")
    decode.write_wav_pcm16(path, pcm, 22050)
    back, rate = decode.read_wav_pcm16(path)
    assert rate == 22050 and back.dtype == np.int16 and np.array_equal(back, pcm)
    import wave

    with wave.open(path, "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getnframes()) == (1, 2, len(pcm))
    with pytest.raises(ValueError, match="int16"):
        decode.write_wav_pcm16(path, pcm.astype(np.float32), 22050)


def test_cli_argument_errors(tmp_path):
    common = ["--outdir", str(tmp_path / "out"), "--checkpoint", str(tmp_path / "none.pkl"), "--verbose", "0"]
    with pytest.raises(NotImplementedError, match="kaldi scp input is Kaldi glue"):
        decode.main(["--scp", "feats.scp"] + common)
    with pytest.raises(ValueError, match="either --dumpdir or --scp"):
        decode.main(common)
    with pytest.raises(ValueError, match="either --dumpdir or --scp"):
        decode.main(["--scp", "feats.scp", "--dumpdir", str(tmp_path)] + common)
    assert decode._parser().parse_args(["--dumpdir", "d"] + common).batch_size == 16

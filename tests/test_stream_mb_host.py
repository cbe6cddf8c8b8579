"""CPU: host side of the stateful PQMF synthesis (pwg_pqmf_up_stream, PQMF.stream_synthesis) and of a multi-band
utils.CausalStream -- the ABI, the history / delay of a filter, which models a stream accepts, and the DEFINITION the GPU
tests rely on (window, delay, history carry-over, flush), emulated on the oracle.  Nothing here launches a kernel."""
import ctypes
import os
import re

import pytest
import torch

from oracle import torch_cpu
from parallelwavegan_amd import _lib, layers, models
from parallelwavegan_amd.utils import CausalStream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB_CAUSAL = dict(in_channels=80, out_channels=4, kernel_size=7, channels=64, upsample_scales=[4, 2, 2],
                 stack_kernel_size=3, stacks=2, use_causal_conv=True)
# partitions of N = 50 and N = 1324 sub-band columns (tests/test_stream_mb_gpu.py runs the kernel over the same ones)
PARTITIONS = [(50,), (1,) * 50, (1, 7, 2, 13, 5, 1, 21), (1030, 294), (3, 1321)]


def test_abi_15_in_library_header_and_binding():
    assert _lib.ABI_VERSION == 15 == _lib.lib().pwg_abi_version()
    header = open(os.path.join(ROOT, "include", "pwg_kernels.h")).read()
    assert "ABI v15" in header
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pwg_pqmf_up_stream", "pwg_pqmf_up_stream_geometry"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    res, args = _lib.SIGNATURES["pwg_pqmf_up_stream"]
    assert res is ctypes.c_int and len(args) == 12  # y, hist_in, hist_out, g, x, batch, n, n_emit, K, len, pad, stream


def _reach(subbands, taps):
    """(dlo, dhi) by enumeration: the column offsets d = i - q for which some output x[qK + r], r < K, has a tap
    g[k][r + pad - dK] inside the filter, 0 <= index <= taps."""
    pad = taps // 2
    ds = [d for d in range(-taps - 1, taps + 2) if any(0 <= r + pad - d * subbands <= taps for r in range(subbands))]
    assert ds == list(range(ds[0], ds[-1] + 1))
    return ds[0], ds[-1]


@pytest.mark.parametrize("subbands,taps,hist,delay", [(4, 62, 15, 8), (2, 62, 31, 16), (3, 62, 21, 11), (8, 126, 15, 8),
                                                      (4, 30, 7, 4), (5, 14, 3, 2), (4, 8, 2, 1)])
def test_history_and_delay_columns(subbands, taps, hist, delay):
    pad = taps // 2
    assert (-(-pad // subbands) + pad // subbands, -(-pad // subbands)) == (hist, delay)  # the formulas
    dlo, dhi = _reach(subbands, taps)
    assert (dhi - dlo, dhi) == (hist, delay)  # what the taps reach
    h, d = ctypes.c_int32(), ctypes.c_int32()
    assert _lib.lib().pwg_pqmf_up_stream_geometry(subbands, taps + 1, pad, ctypes.byref(h), ctypes.byref(d)) == 0
    assert (h.value, d.value) == (hist, delay)
    pq = layers.PQMF(subbands, taps, 0.1, 9.0)
    assert (pq.stream_history_columns, pq.stream_delay_columns) == (hist, delay)
    assert pq.history_shape(3) == (3, subbands, hist)


def test_more_than_eight_subbands_are_refused():
    h = ctypes.c_int32()
    assert _lib.lib().pwg_pqmf_up_stream_geometry(9, 63, 31, ctypes.byref(h), None) == -2  # PWG_ERR_UNSUPPORTED
    assert b"subbands" in _lib.lib().pwg_last_error()
    with pytest.raises(ValueError, match="sub-bands"):
        layers.PQMF(16, 62, 0.03, 9.0).stream_history_columns
    m = models.MelGANGenerator(**dict(MB_CAUSAL, out_channels=16))
    m.pqmf = layers.PQMF(16, 62, 0.03, 9.0)
    with pytest.raises(ValueError, match="up to 8"):
        CausalStream(m)


def test_stream_synthesis_refuses_cpu_tensors():
    pq = layers.PQMF(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pq.stream_synthesis(torch.zeros(1, 4, 20), None, torch.zeros(pq.history_shape(1)), 12)


def test_causal_stream_on_multi_band_models():
    m = models.MelGANGenerator(**MB_CAUSAL)
    with pytest.raises(ValueError, match="PQMF"):  # as constructed: nothing to synthesise the sub-bands with
        CausalStream(m)
    m.pqmf = layers.PQMF(subbands=2, cutoff_ratio=0.267)
    with pytest.raises(ValueError, match="sub-bands"):
        CausalStream(m)
    m.pqmf = torch.nn.Identity()
    with pytest.raises(ValueError, match="PQMF"):
        CausalStream(m)
    m.pqmf = layers.PQMF(subbands=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # accepted up to the device check
        CausalStream(m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CausalStream(m, batch=2, use_graph=False)
    full = models.MelGANGenerator(**dict(MB_CAUSAL, out_channels=1))
    full.pqmf = layers.PQMF(subbands=4)
    with pytest.raises(ValueError, match="sub-bands"):
        CausalStream(full)


def test_worst_case_gain_of_the_default_filter():
    """G = max_r sum_k sum_d |g[k][r + pad - dK]|: what one unit of sub-band error can add to a sample (the bound the
    model-level GPU tests scale by)."""
    pq = layers.PQMF(4)
    g, pad = pq._synthesis_weight[:, 0].double(), pq.taps // 2
    gain = max(sum(g[:, m].abs().sum().item() for m in range(pq.taps + 1) if (m - r - pad) % 4 == 0) for r in range(4))
    assert abs(gain - 7.83) < 0.01, gain


class _EmulatedStream:
    """The definition of pwg_pqmf_up_stream on the oracle: the window is concat(history, chunk) (zeros at the start of a
    stream), a launch emits the last ``n_emit`` positions complete in it, and the last H window columns become the next
    history.  The whole-utterance oracle applied to the window gives those positions exactly where its own zero padding
    does not reach: window positions [-dlo, H + n - dhi)."""

    def __init__(self, subbands, taps, cutoff, beta):
        self.k, self.filt = subbands, (subbands, taps, cutoff, beta)
        self.dlo, self.dhi = _reach(subbands, taps)
        self.hist_cols, self.delay = self.dhi - self.dlo, self.dhi
        self.hist, self.columns = None, 0

    def push(self, y):
        b, k, n = y.shape
        n_emit = max(0, self.columns + n - self.delay) - max(0, self.columns - self.delay)
        assert 0 <= n_emit <= n
        window = torch.cat([self.hist if self.hist is not None else torch.zeros(b, k, self.hist_cols), y], -1)
        full = torch_cpu.pqmf_synthesis(window, *self.filt)[:, 0]
        last = n - self.dlo  # one past the last complete position of the window
        self.hist, self.columns = window[..., window.shape[-1] - self.hist_cols:], self.columns + n
        return full[:, (last - n_emit) * k:last * k]

    def flush(self, batch):
        return self.push(torch.zeros(batch, self.k, self.delay))


@pytest.mark.parametrize("subbands,taps,cutoff,beta", [(4, 62, 0.142, 9.0), (5, 14, 0.12, 7.0)])
def test_stream_definition_reproduces_the_whole_utterance_oracle(subbands, taps, cutoff, beta):
    for pieces in PARTITIONS:
        total = sum(pieces)
        y = torch.randn(2, subbands, total, generator=torch.Generator().manual_seed(total + subbands))
        ref = torch_cpu.pqmf_synthesis(y, subbands, taps, cutoff, beta)[:, 0]
        s = _EmulatedStream(subbands, taps, cutoff, beta)
        outs, t = [], 0
        for n in pieces:
            outs.append(s.push(y[..., t:t + n]))
            t += n
            assert sum(o.shape[-1] for o in outs) == subbands * max(0, t - s.delay)
        tail = s.flush(2)
        assert tail.shape[-1] == subbands * min(total, s.delay)
        out = torch.cat(outs + [tail], -1)
        assert out.shape == ref.shape == (2, subbands * total)
        # the oracle's own fp32 convolution on two different lengths: summation order only
        assert (out - ref).abs().max().item() <= 2e-6 * max(1.0, ref.abs().max().item()), pieces[:4]

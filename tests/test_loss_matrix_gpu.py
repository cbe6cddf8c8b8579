"""GPU: the twelve entry points of csrc/stft_fft.hip and csrc/stft_loss.hip, one launch per assertion, against the float64
references of tests/loss_refs.py.  Every launch runs on inputs of its OWN: ``sums``, ``g2``, ``gout``, ``mel_x`` and
``mel_y`` of a backward launch are test data, not a forward launch's output.

The table covers: the four FFT sizes for each FFT entry point; workgroups that transform one frame, one or two (2103
units over 2048 workgroups at n_fft 256, 512 and 1024, 1053 over 1024 at 2048) and two or three (4203 units); T = n_fft / 2 + 1 and + 2,
T a multiple of the hop and not, hop > win (samples no window touches: dx exactly 0), hop 1; win = n_fft, an odd
n_fft - win, win = 3, asymmetric random windows throughout; a silent item, x == y, a clamp that bites on real data;
g2 in {(1, 1), (-0.7, 0), (0, 2.5)} and sums[0] = 0 handed in with x != y; 1 .. 128 mels over synthetic supports (an empty
filter, a one-bin filter, a filter over all bins, bins no filter covers) and the module's Slaney tables, the three log
bases, a negative gout.  Dense kernels: bins 11 / 32 / 33 / 86 / 193 / 342, frames 1 / 31 / 32 / 33 / 65, units % 4 in
{0, 1, 2, 3}, hop 1 / 2 / 7 / 30, one tap, win off the hop grid, n_cols at and above its minimum, 1 .. 130 mels of a dense
random filterbank and the Slaney one, stored mels below eps and exact ties as backward inputs.

What every launch has in common: every output is a view in the middle of a sentinel-filled buffer (``Guarded``: bands
intact, every element written); every workspace has exactly ``*_workspace_floats`` floats and is NaN-filled; the LDS is
NaN-poisoned before the launch; one case per entry point is launched twice (bit-identical); a refused call leaves every
buffer as the sentinel.

Bars (relative to the largest reference magnitude): loss values 2e-5, FFT-path gradients 2e-4, dense-path gradients 2e-3,
stored mels MEL_STORED_RTOL (8 x the worst float32 CPU row, tests/test_loss_refs_host.py).  The discontinuous terms (sign
of the L1, the clamp) are kept off their edges by the data, which the host test checks on the float64 reference alone:
rows with more than a few thousand elements run the backward twice, the smooth term on independent noise with g2 = (g, 0)
and the full g2 on y[b] = 2^(+-1) x[b], where the log difference is +- ln 2 at every bin.

Measured on an MI355X, worst per entry point, relative to the largest reference magnitude: stft_fft forward sums 1.4e-7,
backward dframes 2.1e-5 / dx 1.6e-5 (11 % of the bar); mel_fft forward total 3.1e-7, backward dframes / dx 8.2e-6;
stft_loss forward sums 1.4e-7, backward dspec 5.7e-5 (3 % of its bar); mel_loss forward stored mels 2.7e-7 (4 % of theirs),
total 2.9e-7, backward dspec 2.8e-6.  The gather never left its derived bound.  The whole file takes 4 s.

Tried by hand against this file: the window indexed backwards, the right reflect image dropped from the gather, the
Nyquist bin left out of the bin loop, S_d stored in the S_y slot, the last bin left out of the dense backward store and
the last mel tile skipped each fail every row of at least one test here.  Dropping the barrier at the head of the frame
loop of ``stft_fft_kernel`` did NOT show in two runs: the rows above the grid cap reach the buffer that the next frame's
load overwrites at every size (forward at 512 and 2048, backward at all four), but the four waves of a workgroup leave
the short bin and store loops within a few cycles of each other, so the window for the race hardly opens.  That barrier
is guarded by reading the code, not by this file."""
import collections
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from parallelwavegan_amd import _lib, ops
from tests import loss_refs as R
from tests.test_wavenet_matrix_gpu import SENTINEL, Guarded
from tests.util import poison_lds

pytestmark = pytest.mark.gpu
D = R.D

LOSS_RTOL, FFT_GRAD_RTOL, DENSE_GRAD_RTOL = 2e-5, 2e-4, 2e-3
# Stored mels (pre-clamp): no bar existed.  8 x the worst float32 CPU evaluation of the dense mel rows below against
# float64 (8.1e-7, mel_y of row md-683-80: 342 bins under 80 dense filters; test_loss_refs_host.py::test_room_under_the_bars
# asserts that every row's float32 error is within a quarter of this).
MEL_STORED_RTOL = 6.5e-6

# entry point -> the test that drives it directly (checked by tests/test_loss_refs_host.py)
COVERED = {
    "pwg_stft_fft_supported": "test_stft_fft_forward",
    "pwg_stft_fft_workspace_floats": "test_stft_fft_forward",
    "pwg_stft_fft_loss_forward": "test_stft_fft_forward",
    "pwg_stft_fft_loss_backward": "test_stft_fft_backward",
    "pwg_mel_fft_loss_forward": "test_mel_fft_forward",
    "pwg_mel_fft_loss_backward": "test_mel_fft_backward",
    "pwg_stft_loss_workspace_floats": "test_stft_dense_forward",
    "pwg_stft_loss_forward": "test_stft_dense_forward",
    "pwg_stft_loss_backward": "test_stft_dense_backward",
    "pwg_mel_loss_workspace_floats": "test_mel_dense_forward",
    "pwg_mel_loss_forward": "test_mel_dense_forward",
    "pwg_mel_loss_backward": "test_mel_dense_backward",
}

G11, GSC, GMAG = (1.0, 1.0), (-0.7, 0.0), (0.0, 2.5)
LN2, LN10 = math.log(2.0), math.log(10.0)


def bar_of(name):
    if name.startswith(("sums", "total")):
        return LOSS_RTOL
    if name.startswith(("dframes", "dx")):
        return FFT_GRAD_RTOL
    if name.startswith("dspec"):
        return DENSE_GRAD_RTOL
    assert name.startswith("mel_"), name
    return MEL_STORED_RTOL


# ------------------------------------------------------------------------------------------------ the FFT table
# bwd: the backward launches of the row, (data, g2, sums[0] handed in as zero)
Fft = collections.namedtuple("Fft", "id n_fft hop win B T seed eps data bwd big")
SPLIT = (("noise", GSC, False), ("scaled", G11, False))  # rows too large for a tie-free log term on independent noise
# ... and rows so large (271 k bins and more) that among independent noise some |X| is 1e-3 of the typical one: the log
# term's 1 / |X| then makes that one bin the largest gradient, and float32 itself is 8e-4 away from float64 there.  Their
# full-g2 launch runs on one pulse per window length over faint noise, whose |X| is bounded away from 0 in every frame.
SPLIT_BIG = (("noise", GSC, False), ("pulses+scaled", G11, False))


def F(id, n_fft, hop, win, B, T, seed=0, eps=1e-7, data="noise", bwd=SPLIT, big=False):
    return Fft(id, n_fft, hop, win, B, T, seed, eps, data, bwd, big)


FFT_CASES = [
    F("256-cap+rem", 256, 16, 199, 3, 11200, bwd=SPLIT_BIG, big=True),       # 2103 units over 2048 workgroups
    F("2048-cap+rem", 2048, 64, 1200, 3, 22400, bwd=SPLIT_BIG, big=True),    # 1053 units over 1024 workgroups
    F("256-2cap", 256, 8, 256, 3, 11200, bwd=SPLIT_BIG, big=True),           # 4203 units: two or three frames per workgroup
    F("512-cap+rem", 512, 16, 301, 3, 11200, bwd=SPLIT_BIG, big=True),       # 2103 units; an even number of forward passes
    F("1024-cap+rem", 1024, 16, 600, 3, 11200, bwd=SPLIT_BIG, big=True),     # 2103 units
    F("512-ragged", 512, 50, 240, 2, 1303, seed=7),                   # T % hop != 0
    F("1024-oddoff", 1024, 120, 601, 2, 2400),                # n_fft - win odd, T % hop == 0
    F("2048-full", 2048, 300, 2048, 1, 3000),
    F("256-shortest", 256, 64, 256, 2, 129, seed=1, bwd=(("noise", G11, False),)),   # both reflect images on the same samples
    F("256-shortest+1", 256, 64, 255, 2, 130, seed=1, bwd=(("noise", G11, False), ("noise", GMAG, False))),
    F("256-hop>win", 256, 150, 100, 2, 920, seed=0, bwd=(("noise", G11, False), ("noise", G11, True))),
    F("256-hop1", 256, 1, 37, 1, 200),
    F("512-win3", 512, 2, 3, 2, 300),
    F("1024-silent", 1024, 256, 1024, 2, 1500, data="silent", bwd=(("silent", GSC, False), ("silent+scaled", G11, False))),
    F("512-same", 512, 120, 400, 2, 300, data="same", bwd=(("same", G11, False),)),
    F("256-bigeps", 256, 64, 200, 2, 300, seed=2, eps=0.3, data="quiet", bwd=(("quiet", G11, False),)),
]
FFT_TWICE = "256-cap+rem"

# mel rows: supports "slaney" or a list; bwd: (data, gout)
MelFft = collections.namedtuple("MelFft", "id n_fft hop win B T seed eps data n_mels supports log_div bwd big")


def _bands(n, step, width, **special):
    s = [(step * j + 2, step * j + 2 + width) for j in range(n)]
    for j, v in special.items():
        s[int(j[1:])] = v
    return s


def MF(id, n_fft, hop, win, B, T, n_mels, supports, log_div, seed=0, eps=1e-10, data="noise", bwd=(("scaled", 1.0),),
       big=False):
    supports = supports if isinstance(supports, str) else tuple(supports)
    return MelFft(id, n_fft, hop, win, B, T, seed, eps, data, n_mels, supports, log_div, bwd, big)


MEL_FFT_CASES = [
    # bins 0, 1 and 108 .. 127 uncovered; filter 4 empty, filter 7 one bin, the last one reaches the Nyquist bin
    MF("m256-33", 256, 64, 256, 2, 1000, 33, _bands(33, 3, 7, j4=(0, -1), j7=(40, 40), j32=(100, 128)), LN2,
       bwd=(("scaled", -1.5),)),
    MF("m512-1", 512, 128, 399, 2, 1301, 1, [(0, 256)], 1.0, bwd=(("scaled", 1.0),)),
    MF("m1024-80", 1024, 256, 1024, 2, 2048, 80, "slaney", LN10),
    MF("m2048-128", 2048, 300, 1200, 2, 3000, 128,
       _bands(128, 7, 15, j5=(0, -1), j6=(500, 500), j100=(0, 1024), j127=(1010, 1024)), 1.0,
       bwd=(("scaled", 0.5),)),
    MF("m256-cap+rem", 256, 16, 199, 3, 11200, 33, _bands(33, 3, 7, j4=(0, -1), j7=(40, 40), j32=(100, 128)), LN10,
       big=True),
    MF("m256-tiny", 256, 64, 200, 1, 140, 33, _bands(33, 3, 7), LN2, seed=3, bwd=(("noise", -2.0),)),
]
MEL_FFT_TWICE = "m256-33"

# ------------------------------------------------------------------------------------------------ the dense table
Dense = collections.namedtuple("Dense", "id n_fft hop win B frames extra seed eps data bwd")


def DN(id, n_fft, hop, win, B, frames, extra=0, seed=0, eps=1e-7, data="noise", bwd=SPLIT):
    return Dense(id, n_fft, hop, win, B, frames, extra, seed, eps, data, bwd)


TINY = (("noise", G11, False),)
DENSE_CASES = [
    DN("d20-f1", 20, 30, 20, 1, 1, bwd=TINY + (("noise", G11, True),)),       # bins 11, one tap, 1 unit
    DN("d62-f31", 62, 1, 7, 2, 31, bwd=TINY + (("noise", GSC, False),)),                                 # bins 32, hop 1, 2 units
    DN("d64-f32", 64, 2, 63, 3, 32, extra=3, seed=11,                         # bins 33, 6 units, odd n_fft - win
       bwd=TINY + (("noise", GMAG, False), ("noise", GSC, False))),
    DN("d171-f32", 171, 7, 60, 1, 32, bwd=TINY),                              # bins 86, 3 units
    DN("d171-f33", 171, 7, 60, 2, 33, extra=1),                               # 12 units
    DN("d384-f65", 384, 30, 150, 1, 65),                                      # bins 193, 21 units
    DN("d683-f33", 683, 60, 300, 1, 33),                                      # bins 342, 22 units
    DN("d64-silent", 64, 2, 63, 2, 33, data="silent", bwd=(("silent", GSC, False), ("silent+scaled", G11, False))),
    DN("d64-same", 64, 2, 63, 2, 31, data="same", bwd=(("same", G11, False),)),
    DN("d62-bigeps", 62, 7, 40, 2, 9, seed=5, eps=0.05, data="quiet", bwd=(("quiet", G11, False),)),
]
DENSE_TWICE = "d171-f33"

MelDense = collections.namedtuple("MelDense", "id n_fft hop win B frames extra seed eps data n_mels fb log_div gout")


def MD(id, n_fft, hop, win, B, frames, n_mels, fb, log_div, gout=1.0, extra=0, seed=0, eps=1e-10, data="noise"):
    return MelDense(id, n_fft, hop, win, B, frames, extra, seed, eps, data, n_mels, fb, log_div, gout)


MEL_DENSE_CASES = [
    MD("md-20-1", 20, 30, 20, 1, 1, 1, "dense", 1.0),
    MD("md-62-31", 62, 1, 7, 2, 31, 31, "dense", LN2, gout=-1.5),
    MD("md-64-32", 64, 2, 63, 3, 32, 32, "dense", LN10, extra=2),
    MD("md-171-33", 171, 7, 60, 1, 32, 33, "dense", 1.0),
    MD("md-384-130", 384, 30, 150, 1, 65, 130, "dense", LN10),
    MD("md-384-slaney", 384, 30, 150, 2, 33, 80, "slaney", LN10, gout=-0.5),
    MD("md-683-80", 683, 60, 300, 1, 33, 80, "dense", LN2),
]
MEL_DENSE_TWICE = "md-171-33"
EVERY_CASE = FFT_CASES + MEL_FFT_CASES + DENSE_CASES + MEL_DENSE_CASES


# ------------------------------------------------------------------------------------------------ test data
@functools.lru_cache(maxsize=None)
def window_of(c):
    """An asymmetric random window, exact in float32."""
    g = torch.Generator().manual_seed(1000 + c.seed + c.win)
    return ((0.15 + torch.rand(c.win, generator=g)) * torch.linspace(0.3, 1.0, c.win)).float()


def signals(B, T, seed, data, burst, period=None):
    """(x, y) float32.  x carries an alternating component (the last bin matters) and a loud stretch ``burst`` (the last
    frame matters): tests/test_loss_refs_host.py::test_sensitivity is what they are there for."""
    g = torch.Generator().manual_seed(seed)
    x, y = 0.5 * torch.randn(B, T, generator=g), 0.5 * torch.randn(B, T, generator=g)
    x = x + 0.25 * (1.0 - 2.0 * (torch.arange(T) % 2)).float()
    x[:, burst] *= 4.0
    kinds = data.split("+")
    if "pulses" in kinds:  # one pulse per ``period`` samples (and one on the last sample), over faint noise
        x = 0.001 * torch.randn(B, T, generator=g)
        at = torch.cat([torch.arange(0, T, period), torch.tensor([T - 1])])
        sign = 1.0 - 2.0 * (torch.rand(B, at.numel(), generator=g) < 0.5).float()
        x[:, at] = (1.0 + torch.rand(B, at.numel(), generator=g)) * sign
    if "quiet" in kinds:
        x[1] *= 2.0 ** -6
    if "silent" in kinds:
        x[0] = 0.0
    if "scaled" in kinds:
        y = x * torch.tensor([2.0, 0.5] * B)[:B, None]
    if "same" in kinds:
        y = x.clone()
    return x, y


def fft_signals(c, data):
    return signals(c.B, c.T, 17 * c.n_fft + c.T + c.seed, data, slice(c.T - max(1, min(c.win, c.T) // 4), c.T), period=c.win)


def dense_cols(c):
    return c.frames + -(-c.win // c.hop) - 1 + c.extra


def dense_signals(c, data):
    """The folded pair (B, hop, n_cols) float32: column q, row r holds sample q * hop + r of a signal."""
    n = c.hop * dense_cols(c)
    end = (c.frames - 1) * c.hop + c.win
    x, y = signals(c.B, n, 13 * c.n_fft + c.frames + c.seed, data, slice(end - max(1, c.win // 4), end))
    fold = lambda s: s.reshape(c.B, -1, c.hop).transpose(1, 2).contiguous()  # noqa: E731
    return fold(x), fold(y)


def filters_of(c):
    """fb (n_mels, bins_pad) float64 (float32-exact), mel_range, bin_range of a mel row."""
    bins = c.n_fft // 2 + 1
    if isinstance(c, MelFft) and c.supports != "slaney":
        return R.make_filters(c.supports, bins, 77 + c.seed)
    bins_pad = 32 * ((bins + 31) // 32)
    if getattr(c, "fb", None) == "dense":
        g = torch.Generator().manual_seed(99 + c.n_mels)
        fb = torch.zeros(c.n_mels, bins_pad)
        fb[:, :bins] = 0.05 + torch.rand(c.n_mels, bins, generator=g)
        return fb.double(), None, None
    ms = mel_module(c)
    from parallelwavegan_amd.losses.mel_loss import MelFftPairLossFn

    fb, mr, br = MelFftPairLossFn._tables(ms, torch.device("cpu"))
    return fb.double(), mr.numpy(), br.numpy()


@functools.lru_cache(maxsize=None)
def mel_module(c):
    from parallelwavegan_amd.losses import MelSpectrogramLoss

    return MelSpectrogramLoss(fs=22050, fft_size=c.n_fft, hop_size=c.hop, win_length=c.win, window="hann",
                              num_mels=c.n_mels, fmin=0, fmax=11025, log_base=None).mel_spectrogram


def _inv_n(c, frames):
    return 1.0 / (c.B * (c.n_fft // 2 + 1) * frames)


def _sums_in(s64, zero_sd):
    """``sums`` of a backward launch: the float64 sums of the row, each moved off what a forward launch would return."""
    s = (s64 * torch.tensor([1.7, 0.6, 1.3, 1.0, 1.0], dtype=D)).float()
    if zero_sd:
        s[0] = 0.0
    return s


# ------------------------------------------------------------------------------------------------ references
PLANTS = ("window", "off", "nyquist", "frame", "image", "filter", "swap")


class _Frames:
    """frames -> spectra -> ... of one row under an optional planted error, in ``dtype``."""

    def __init__(self, c, dtype, plant):
        self.c, self.dtype, self.plant = c, dtype, plant
        self.fft = isinstance(c, (Fft, MelFft)) and (c.big or dtype != D)
        self.off = (c.n_fft - c.win) // 2
        w = window_of(c)
        self.planted_window = plant in ("window", "off")
        if plant == "window":
            w = w.flip(0)
        self.w = w
        self.wp = R.padded_window(w, c.n_fft, c.win)
        if plant == "off":
            self.wp = torch.roll(self.wp, 1)

    def cut(self, s):
        c = self.c
        s = s.to(self.dtype)
        if isinstance(c, (Fft, MelFft)):
            if self.planted_window:
                return R.frames(s, c.n_fft, c.hop, c.n_fft, self.wp)
            return R.frames(s, c.n_fft, c.hop, c.win, self.w)
        if self.planted_window:  # the folded samples of a frame, then the (moved) padded window
            fr = R.frames_of_folded(s, c.n_fft, c.hop, c.win, torch.ones(c.win), c.frames)
            return fr * self.wp.to(self.dtype)
        return R.frames_of_folded(s, c.n_fft, c.hop, c.win, self.w, c.frames)

    def spectra(self, s):
        X = R.spectra(self.cut(s), fft=self.fft)
        if self.plant == "nyquist":
            X = tuple(t[..., :-1] for t in X)
        if self.plant == "frame":
            X = tuple(t[:, :-1] for t in X)
        return X

    def whole(self, ds):
        """d spectra back at the row's full (frames, bins): what a planted error dropped holds zeros."""
        out = []
        for t in ds:
            if self.plant == "nyquist":
                t = torch.nn.functional.pad(t, (0, 1))
            if self.plant == "frame":
                t = torch.nn.functional.pad(t, (0, 0, 0, 1))
            out.append(t)
        return tuple(out)

    def dframes(self, ds):
        c = self.c
        if self.planted_window:
            return R.dframes_of(ds, self.wp, 0, c.n_fft, c.n_fft, fft=self.fft)[..., self.off:self.off + c.win]
        return R.dframes_of(ds, self.w, self.off, c.win, c.n_fft, fft=self.fft)

    def back(self, ds, q, i):
        c = self.c
        df = self.dframes(self.whole(ds))
        q[f"dframes{i}"] = df
        q[f"dx{i}"] = R.overlap_add(df, c.T, c.n_fft, c.hop, c.win, images=(0, 1) if self.plant == "image" else (0, 1, 2))


def _n_frames(c):
    return R.n_frames(c.T, c.n_fft, c.hop) if isinstance(c, (Fft, MelFft)) else c.frames


def _signals(c, data):
    return fft_signals(c, data) if isinstance(c, (Fft, MelFft)) else dense_signals(c, data)


def _pair_quantities(c, dtype, plant):
    fr = _Frames(c, dtype, plant)
    x, y = _signals(c, c.data)
    q = collections.OrderedDict()
    s = R.pair_sums(fr.spectra(x), fr.spectra(y), c.eps)
    for j in range(5):
        q[f"sums{j}"] = s[j]
    for i, (data, g2, zero_sd) in enumerate(c.bwd):
        x, y = _signals(c, data)
        s_in = _sums_in(sums64(c, data), zero_sd)
        ds = R.pair_dspec(fr.spectra(x), fr.spectra(y), c.eps, s_in.double(), g2, _inv_n(c, _n_frames(c)),
                          swap_sd=plant == "swap")
        if isinstance(c, Fft):
            fr.back(ds, q, i)
        else:
            q[f"dspec{i}"] = torch.cat([t.transpose(1, 2) for t in fr.whole(ds)], dim=1)
    return q


@functools.lru_cache(maxsize=None)
def sums64(c, data):
    """The float64 sums of the row's data ``data`` (no planted error): what the backward rows' ``sums`` derive from."""
    fr = _Frames(c, D, None)
    x, y = _signals(c, data)
    return R.pair_sums(fr.spectra(x), fr.spectra(y), c.eps)


def stored_mels(c):
    """mel_x, mel_y (B, n_mels, frames) float32 handed to the dense mel backward: positive values a clear factor apart,
    with elements below eps (zero gradient), exact zeros and exact ties (sign 0) among them."""
    g = torch.Generator().manual_seed(5 + c.n_mels + c.frames)
    mx = torch.exp(torch.randn(c.B, c.n_mels, c.frames, generator=g))
    my = mx * torch.where(torch.rand(mx.shape, generator=g) < 0.5, 1.5, 0.5)
    flat_x, flat_y = mx.view(-1), my.view(-1)
    flat_x[1::7] = c.eps * 0.01      # below eps: zero gradient
    flat_x[3::11] = 0.0
    flat_y[5::13] = flat_x[5::13]    # exact ties: sign 0
    flat_y[2::17] = c.eps * 0.5      # y below eps, x not: the clamp of y alone
    return mx.float(), my.float()


def _mel_quantities(c, dtype, plant):
    fr = _Frames(c, dtype, plant)
    fb, _, _ = filters_of(c)
    if plant == "filter":
        fb = fb[:-1]
    q = collections.OrderedDict()
    x, y = _signals(c, c.data)
    mel_x, mel_y, total = R.mel_pair(R.magnitude(fr.spectra(x), c.eps), R.magnitude(fr.spectra(y), c.eps), fb.to(dtype),
                                     c.eps, c.log_div)
    if isinstance(c, MelDense):
        q["mel_x"], q["mel_y"] = mel_x, mel_y
    q["total"] = total
    if isinstance(c, MelFft):
        for i, (data, gout) in enumerate(c.bwd):
            x, y = _signals(c, data)
            X = fr.spectra(x)
            mel_x, mel_y, _ = R.mel_pair(R.magnitude(X, c.eps), R.magnitude(fr.spectra(y), c.eps), fb.to(dtype), c.eps,
                                         c.log_div)
            fr.back(R.mel_dspec(X, R.mel_dmag(mel_x, mel_y, fb, c.eps, c.log_div, gout), c.eps), q, i)
    else:
        mx, my = stored_mels(c)
        if plant == "filter":
            mx, my = mx[:, :-1], my[:, :-1]
        if plant == "frame":
            mx, my = mx[..., :-1], my[..., :-1]
        X = fr.spectra(x)
        ds = R.mel_dspec(X, R.mel_dmag(mx.to(dtype), my.to(dtype), fb, c.eps, c.log_div, c.gout), c.eps)
        q["dspec0"] = torch.cat([t.transpose(1, 2) for t in fr.whole(ds)], dim=1)
    return q


def quantities(c, dtype=D, plant=None):
    """name -> reference of every quantity the GPU tests compare for row ``c``."""
    return (_pair_quantities if isinstance(c, (Fft, Dense)) else _mel_quantities)(c, dtype, plant)


@functools.lru_cache(maxsize=None)
def want(c):
    return quantities(c)


# ------------------------------------------------------------------------------------------------ launches
WORST = collections.defaultdict(float)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for k, err in sorted(WORST.items()):
        print(f"worst error, {k[0]} {k[1]}: {err:.3e} ({err / bar_of(k[1]):.1%} of its bar)")


def _within(got, ref, entry, name, what):
    got = got.detach().cpu().double().reshape(ref.shape)
    assert torch.isfinite(got).all(), f"{what} {name}: not finite"
    top = ref.abs().max().item()
    if top == 0.0:
        assert got.abs().max().item() == 0.0, f"{what} {name}: the reference is exactly 0, got {got.abs().max().item():.3e}"
        return
    err = (got - ref).abs().max().item() / top
    key = (entry, "".join(ch for ch in name if not ch.isdigit()))
    WORST[key] = max(WORST[key], err)
    print(f"{what} {name}: rel-to-max error {err:.3e}")
    assert err <= bar_of(name), f"{what} {name}: rel-to-max error {err:.3e} above {bar_of(name):.1e}"


def _call(name, *args):
    lib = _lib.lib()
    conv = [ops._ptr(a) if isinstance(a, torch.Tensor) else a for a in args]
    rc = getattr(lib, name)(*conv, ops._stream())
    assert rc == 0, f"{name}: status {rc}: {lib.pwg_last_error().decode(errors='replace')}"


def _nan(n, device):
    return torch.full((int(n),), float("nan"), dtype=torch.float32, device=device)


def _ip(t):
    return ctypes.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def _stft_module(c):
    from parallelwavegan_amd.losses.stft import STFTMagnitude

    return STFTMagnitude(c.n_fft, c.hop, c.win, window_of(c), eps=c.eps)


def _fft_tables(c, device):
    window, twiddle = _stft_module(c)._fft_tables(device)
    assert torch.equal(window.cpu(), window_of(c))
    return window, twiddle


def fft_grid(c):
    return _lib.lib().pwg_stft_fft_workspace_floats(c.B, R.n_frames(c.T, c.n_fft, c.hop), c.n_fft) // 4


def _fft_forward(c, device):
    L = _lib.lib()
    assert L.pwg_stft_fft_supported(c.n_fft, c.win, c.hop)
    x, y = fft_signals(c, c.data)
    window, twiddle = _fft_tables(c, device)
    ws = _nan(L.pwg_stft_fft_workspace_floats(c.B, R.n_frames(c.T, c.n_fft, c.hop), c.n_fft), device)
    sums = Guarded((5,), device)
    with poison_lds():
        _call("pwg_stft_fft_loss_forward", x.to(device), y.to(device), window, twiddle, c.B, c.T, c.n_fft, c.hop, c.win,
              c.eps, ws, sums.out)
        return sums.check(f"{c.id}: sums").cpu()


@pytest.mark.parametrize("c", FFT_CASES, ids=[c.id for c in FFT_CASES])
def test_stft_fft_forward(c, device):
    units = c.B * R.n_frames(c.T, c.n_fft, c.hop)
    assert fft_grid(c) == min(units, 256 * (4 if c.n_fft == 2048 else 8))
    got, ref = _fft_forward(c, device), want(c)
    for j in range(5):
        _within(got[j], ref[f"sums{j}"], "stft_fft_forward", f"sums{j}", c.id)
    if c.data == "same":
        assert got[0].item() == 0.0 and got[2].item() == 0.0 and got[3].item() == 0.0 and got[4].item() == 0.0
    if c.id == FFT_TWICE:
        assert torch.equal(_fft_forward(c, device), got), f"{c.id}: the second launch differs"


def _gather_alone(c, df, dx, what):
    """dx against the overlap-add of the kernel's OWN dframes summed in float64: per sample at most
    n_terms = 3 ceil(win / hop) terms added in float32, each addition rounding once: n_terms * 2^-24 * sum |terms|."""
    df64 = df.cpu().double()
    ref = R.overlap_add(df64, c.T, c.n_fft, c.hop, c.win)
    bound = 3 * -(-c.win // c.hop) * 2.0 ** -24 * R.overlap_add(df64.abs(), c.T, c.n_fft, c.hop, c.win)
    over = (dx.cpu().double() - ref).abs() - bound
    assert bool((over <= 0).all()), \
        f"{what}: gather off the overlap-add of its own dframes by {over.max().item():.3e} past the bound"
    if c.hop > c.win:  # samples no window touches
        untouched = R.overlap_add(torch.ones_like(df64), c.T, c.n_fft, c.hop, c.win) == 0
        assert bool(untouched.any()) and bool((dx.cpu()[untouched] == 0.0).all()), f"{what}: dx not exactly 0 off every window"


def _fft_backward(c, i, device):
    data, g2, zero_sd = c.bwd[i]
    x, y = fft_signals(c, data)
    window, twiddle = _fft_tables(c, device)
    frames = R.n_frames(c.T, c.n_fft, c.hop)
    df, dx = Guarded((c.B, frames, c.win), device), Guarded((c.B, c.T), device)
    with poison_lds():
        _call("pwg_stft_fft_loss_backward", x.to(device), y.to(device), window, twiddle, c.B, c.T, c.n_fft, c.hop, c.win,
              c.eps, _sums_in(sums64(c, data), zero_sd).to(device), torch.tensor(g2, dtype=torch.float32, device=device),
              df.out, dx.out)
        return df.check(f"{c.id}/{i}: dframes").cpu(), dx.check(f"{c.id}/{i}: dx").cpu()


@pytest.mark.parametrize("c", FFT_CASES, ids=[c.id for c in FFT_CASES])
def test_stft_fft_backward(c, device):
    ref = want(c)
    for i, (data, g2, zero_sd) in enumerate(c.bwd):
        what = f"{c.id}/{data}/g2={g2}/zero_sd={zero_sd}"
        df, dx = _fft_backward(c, i, device)
        _within(df, ref[f"dframes{i}"], "stft_fft_backward", f"dframes{i}", what)
        _within(dx, ref[f"dx{i}"], "stft_fft_backward", f"dx{i}", what)
        _gather_alone(c, df, dx, what)
        if "silent" in data:
            assert float(df[0].abs().max()) == 0.0 and float(dx[0].abs().max()) == 0.0, f"{what}: the silent item has a gradient"
        if c.id == FFT_TWICE and i == 0:
            df2, dx2 = _fft_backward(c, i, device)
            assert torch.equal(df2, df) and torch.equal(dx2, dx), f"{what}: the second launch differs"


def _mel_fft_tables(c, device):
    fb, mr, br = filters_of(c)
    return (fb.float().to(device), torch.from_numpy(np.ascontiguousarray(mr)).to(device),
            torch.from_numpy(np.ascontiguousarray(br)).to(device))


def _mel_fft_forward(c, device):
    L = _lib.lib()
    x, y = fft_signals(c, c.data)
    window, twiddle = _fft_tables(c, device)
    fb, mr, br = _mel_fft_tables(c, device)
    ws = _nan(L.pwg_stft_fft_workspace_floats(c.B, R.n_frames(c.T, c.n_fft, c.hop), c.n_fft), device)
    total = Guarded((1,), device)
    with poison_lds():
        _call("pwg_mel_fft_loss_forward", x.to(device), y.to(device), window, twiddle, fb, _ip(mr), _ip(br), c.B, c.T,
              c.n_fft, c.hop, c.win, c.n_mels, fb.shape[1], c.eps, c.log_div, ws, total.out)
        return total.check(f"{c.id}: total").cpu()


@pytest.mark.parametrize("c", MEL_FFT_CASES, ids=[c.id for c in MEL_FFT_CASES])
def test_mel_fft_forward(c, device):
    got = _mel_fft_forward(c, device)
    _within(got, want(c)["total"], "mel_fft_forward", "total", c.id)
    if c.id == MEL_FFT_TWICE:
        assert torch.equal(_mel_fft_forward(c, device), got), f"{c.id}: the second launch differs"


def _mel_fft_backward(c, i, device):
    data, gout = c.bwd[i]
    x, y = fft_signals(c, data)
    window, twiddle = _fft_tables(c, device)
    fb, mr, br = _mel_fft_tables(c, device)
    df, dx = Guarded((c.B, R.n_frames(c.T, c.n_fft, c.hop), c.win), device), Guarded((c.B, c.T), device)
    with poison_lds():
        _call("pwg_mel_fft_loss_backward", x.to(device), y.to(device), window, twiddle, fb, _ip(mr), _ip(br), c.B, c.T,
              c.n_fft, c.hop, c.win, c.n_mels, fb.shape[1], c.eps, c.log_div,
              torch.tensor([gout], dtype=torch.float32, device=device), df.out, dx.out)
        return df.check(f"{c.id}/{i}: dframes").cpu(), dx.check(f"{c.id}/{i}: dx").cpu()


@pytest.mark.parametrize("c", MEL_FFT_CASES, ids=[c.id for c in MEL_FFT_CASES])
def test_mel_fft_backward(c, device):
    ref = want(c)
    for i, (data, gout) in enumerate(c.bwd):
        what = f"{c.id}/{data}/gout={gout}"
        df, dx = _mel_fft_backward(c, i, device)
        _within(df, ref[f"dframes{i}"], "mel_fft_backward", f"dframes{i}", what)
        _within(dx, ref[f"dx{i}"], "mel_fft_backward", f"dx{i}", what)
        _gather_alone(c, df, dx, what)
        if c.id == MEL_FFT_TWICE:
            df2, dx2 = _mel_fft_backward(c, i, device)
            assert torch.equal(df2, df) and torch.equal(dx2, dx), f"{what}: the second launch differs"


# ---- the dense kernels
def dense_units(c):
    return c.B * -(-(c.n_fft // 2 + 1) // 32) * -(-c.frames // 32)


def _dense_args(c, data, device):
    fx, fy = dense_signals(c, data)
    mod = _stft_module(c)
    assert mod.taps == -(-c.win // c.hop) and mod.bins == c.n_fft // 2 + 1
    return fx.to(device), fy.to(device), mod.pair_basis.to(device), mod


def _dense_forward(c, device):
    L = _lib.lib()
    fx, fy, basis, mod = _dense_args(c, c.data, device)
    n_ws = L.pwg_stft_loss_workspace_floats(c.B, mod.bins, c.frames)
    assert n_ws == 16 * -(-dense_units(c) // 4)
    ws, sums = _nan(n_ws, device), Guarded((5,), device)
    with poison_lds():
        _call("pwg_stft_loss_forward", fx, fy, basis, c.B, c.hop, dense_cols(c), mod.taps, mod.bins, c.frames, c.eps, ws,
              sums.out)
        return sums.check(f"{c.id}: sums").cpu()


@pytest.mark.parametrize("c", DENSE_CASES, ids=[c.id for c in DENSE_CASES])
def test_stft_dense_forward(c, device):
    got, ref = _dense_forward(c, device), want(c)
    for j in range(5):
        _within(got[j], ref[f"sums{j}"], "stft_loss_forward", f"sums{j}", c.id)
    if c.data == "same":
        assert got[0].item() == 0.0 and got[2].item() == 0.0
    if c.id == DENSE_TWICE:
        assert torch.equal(_dense_forward(c, device), got), f"{c.id}: the second launch differs"


def _dense_backward(c, i, device):
    data, g2, zero_sd = c.bwd[i]
    fx, fy, basis, mod = _dense_args(c, data, device)
    ds = Guarded((c.B, 2 * mod.bins, c.frames), device)
    with poison_lds():
        _call("pwg_stft_loss_backward", fx, fy, basis, c.B, c.hop, dense_cols(c), mod.taps, mod.bins, c.frames, c.eps,
              _sums_in(sums64(c, data), zero_sd).to(device), torch.tensor(g2, dtype=torch.float32, device=device), ds.out)
        return ds.check(f"{c.id}/{i}: dspec").cpu()


@pytest.mark.parametrize("c", DENSE_CASES, ids=[c.id for c in DENSE_CASES])
def test_stft_dense_backward(c, device):
    ref = want(c)
    for i, (data, g2, zero_sd) in enumerate(c.bwd):
        what = f"{c.id}/{data}/g2={g2}/zero_sd={zero_sd}"
        ds = _dense_backward(c, i, device)
        _within(ds, ref[f"dspec{i}"], "stft_loss_backward", f"dspec{i}", what)
        if "silent" in data:
            assert float(ds[0].abs().max()) == 0.0, f"{what}: the silent item has a gradient"
        if c.id == DENSE_TWICE and i == 0:
            assert torch.equal(_dense_backward(c, i, device), ds), f"{what}: the second launch differs"


def _mel_images(c, device):
    """mel_t [bins_pad][mels_pad], mel_b [mels_pad][bins_pad]: the module's own where the row names the Slaney basis."""
    if c.fb == "slaney":
        ms = mel_module(c)
        return ms.mel_t.to(device), ms.mel_b.to(device)
    fb, _, _ = filters_of(c)
    mels_pad = 32 * ((c.n_mels + 31) // 32)
    mel_b = torch.zeros(mels_pad, fb.shape[1])
    mel_b[:c.n_mels] = fb.float()
    return mel_b.T.contiguous().to(device), mel_b.to(device)


def _mel_dense_forward(c, device):
    L = _lib.lib()
    fx, fy, basis, mod = _dense_args(c, c.data, device)
    mel_t, _ = _mel_images(c, device)
    ws = _nan(L.pwg_mel_loss_workspace_floats(c.B, mod.bins, c.frames, c.n_mels), device)
    mx, my = Guarded((c.B, c.n_mels, c.frames), device), Guarded((c.B, c.n_mels, c.frames), device)
    total = Guarded((1,), device)
    with poison_lds():
        _call("pwg_mel_loss_forward", fx, fy, basis, mel_t, c.B, c.hop, dense_cols(c), mod.taps, mod.bins, c.frames,
              c.n_mels, c.eps, c.log_div, ws, mx.out, my.out, total.out)
        return mx.check(f"{c.id}: mel_x").cpu(), my.check(f"{c.id}: mel_y").cpu(), total.check(f"{c.id}: total").cpu()


@pytest.mark.parametrize("c", MEL_DENSE_CASES, ids=[c.id for c in MEL_DENSE_CASES])
def test_mel_dense_forward(c, device):
    got, ref = _mel_dense_forward(c, device), want(c)
    for t, name in zip(got, ("mel_x", "mel_y", "total")):
        _within(t, ref[name], "mel_loss_forward", name, c.id)
    if c.id == MEL_DENSE_TWICE:
        for a, b in zip(_mel_dense_forward(c, device), got):
            assert torch.equal(a, b), f"{c.id}: the second launch differs"


def _mel_dense_backward(c, device):
    fx, _, basis, mod = _dense_args(c, c.data, device)
    _, mel_b = _mel_images(c, device)
    mx, my = stored_mels(c)
    ds = Guarded((c.B, 2 * mod.bins, c.frames), device)
    with poison_lds():
        _call("pwg_mel_loss_backward", fx, basis, mel_b, mx.to(device), my.to(device), c.B, c.hop, dense_cols(c), mod.taps,
              mod.bins, c.frames, c.n_mels, c.eps, c.log_div, torch.tensor([c.gout], dtype=torch.float32, device=device),
              ds.out)
        return ds.check(f"{c.id}: dspec").cpu()


@pytest.mark.parametrize("c", MEL_DENSE_CASES, ids=[c.id for c in MEL_DENSE_CASES])
def test_mel_dense_backward(c, device):
    ds = _mel_dense_backward(c, device)
    _within(ds, want(c)["dspec0"], "mel_loss_backward", "dspec0", c.id)
    if c.id == MEL_DENSE_TWICE:
        assert torch.equal(_mel_dense_backward(c, device), ds), f"{c.id}: the second launch differs"


# ---- refusals
def _sentinel(n, device):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device=device)


def test_refused_calls_write_nothing(device):
    """T = n_fft / 2, n_cols below frames + taps - 1, 129 mels on the FFT path, a NULL table: a status, and every buffer
    the call was handed still holds the sentinel."""
    L = _lib.lib()
    c = FFT_CASES[3]
    x, y = (s.to(device) for s in fft_signals(c, "noise"))
    window, twiddle = _fft_tables(c, device)
    bufs = [_sentinel(4096, device) for _ in range(3)]
    f = [b.view(torch.float32) for b in bufs]
    P, S = ops._ptr, ops._stream
    half = c.n_fft // 2
    g2 = torch.ones(2, device=device)
    m = MEL_FFT_CASES[0]
    mx, my = (s.to(device) for s in fft_signals(m, "noise"))
    mwin, mtw = _fft_tables(m, device)
    fb, mr, br = _mel_fft_tables(m, device)
    fb129 = torch.zeros(129, fb.shape[1], device=device)
    d = DENSE_CASES[3]
    fx, fy, basis, mod = _dense_args(d, "noise", device)
    short = dense_cols(d) - 1
    refused = {
        "fft forward, T = n_fft / 2": L.pwg_stft_fft_loss_forward(P(x), P(y), P(window), P(twiddle), c.B, half, c.n_fft, c.hop,
                                                                 c.win, c.eps, P(f[0]), P(f[1]), S()),
        "fft backward, T = n_fft / 2": L.pwg_stft_fft_loss_backward(P(x), P(y), P(window), P(twiddle), c.B, half, c.n_fft,
                                                                   c.hop, c.win, c.eps, P(f[0]), P(g2), P(f[1]), P(f[2]), S()),
        "fft forward, NULL twiddle": L.pwg_stft_fft_loss_forward(P(x), P(y), P(window), None, c.B, c.T, c.n_fft, c.hop, c.win,
                                                                c.eps, P(f[0]), P(f[1]), S()),
        "mel fft forward, 129 mels": L.pwg_mel_fft_loss_forward(P(mx), P(my), P(mwin), P(mtw), P(fb129), _ip(mr), _ip(br), m.B,
                                                               m.T, m.n_fft, m.hop, m.win, 129, fb.shape[1], m.eps, m.log_div,
                                                               P(f[0]), P(f[1]), S()),
        "mel fft backward, 129 mels": L.pwg_mel_fft_loss_backward(P(mx), P(my), P(mwin), P(mtw), P(fb129), _ip(mr), _ip(br),
                                                                 m.B, m.T, m.n_fft, m.hop, m.win, 129, fb.shape[1], m.eps,
                                                                 m.log_div, P(g2), P(f[0]), P(f[1]), S()),
        "mel fft forward, NULL bin_range": L.pwg_mel_fft_loss_forward(P(mx), P(my), P(mwin), P(mtw), P(fb), _ip(mr), None, m.B,
                                                                     m.T, m.n_fft, m.hop, m.win, m.n_mels, fb.shape[1], m.eps,
                                                                     m.log_div, P(f[0]), P(f[1]), S()),
        "dense forward, n_cols short": L.pwg_stft_loss_forward(P(fx), P(fy), P(basis), d.B, d.hop, short, mod.taps, mod.bins,
                                                              d.frames, d.eps, P(f[0]), P(f[1]), S()),
        "dense backward, n_cols short": L.pwg_stft_loss_backward(P(fx), P(fy), P(basis), d.B, d.hop, short, mod.taps, mod.bins,
                                                                d.frames, d.eps, P(f[0]), P(g2), P(f[1]), S()),
        "dense forward, NULL basis": L.pwg_stft_loss_forward(P(fx), P(fy), None, d.B, d.hop, dense_cols(d), mod.taps, mod.bins,
                                                            d.frames, d.eps, P(f[0]), P(f[1]), S()),
        "dense mel forward, n_cols short": L.pwg_mel_loss_forward(P(fx), P(fy), P(basis), P(fb), d.B, d.hop, short, mod.taps,
                                                                 mod.bins, d.frames, 33, 1e-10, 1.0, P(f[0]), P(f[1]), P(f[2]),
                                                                 P(f[2]), S()),
        "dense mel backward, NULL mel_b": L.pwg_mel_loss_backward(P(fx), P(basis), None, P(f[0]), P(f[0]), d.B, d.hop,
                                                                 dense_cols(d), mod.taps, mod.bins, d.frames, 33, 1e-10, 1.0,
                                                                 P(g2), P(f[1]), S()),
    }
    torch.cuda.synchronize()
    for what, rc in refused.items():
        assert rc != 0, f"{what}: accepted"
    for b in bufs:
        assert bool((b == SENTINEL).all()), "a refused call wrote to a buffer"


# ---- routing
def test_modules_route_to_the_kernels_this_file_tests(device):
    """STFTMagnitude.pair_losses and MelSpectrogramLoss take the FFT kernels at 256 .. 2048 with T > n_fft / 2 and at most
    128 mels, the dense ones at 171, at center=False and at 130 mels."""
    from parallelwavegan_amd.losses import MelSpectrogramLoss
    from parallelwavegan_amd.losses.stft import STFTMagnitude

    def kernels(fn):
        with ops.profile() as prof:
            fn()
            torch.cuda.synchronize()
        return set(prof.results)

    g = torch.Generator().manual_seed(0)
    x, y = (0.5 * torch.randn(2, 2600, generator=g)).to(device), (0.5 * torch.randn(2, 2600, generator=g)).to(device)
    for n_fft in (256, 512, 1024, 2048):
        mod = STFTMagnitude(n_fft, n_fft // 4, n_fft // 2, "hann").to(device)
        k = kernels(lambda: mod.pair_losses(x.clone().requires_grad_(), y).sum().backward())
        assert {"stft_fft_fwd_kernel", "stft_fft_bwd_kernel", "stft_fft_gather_kernel"} <= k, (n_fft, k)
        assert "stft_loss_fwd_kernel" not in k, (n_fft, k)
        crit = MelSpectrogramLoss(fs=22050, fft_size=n_fft, hop_size=n_fft // 4, num_mels=40, fmin=0, fmax=11025).to(device)
        k = kernels(lambda: crit(x.clone().requires_grad_(), y).backward())
        assert {"mel_fft_fwd_kernel", "mel_fft_bwd_kernel"} <= k and "mel_loss_fwd_kernel" not in k, (n_fft, k)
    for mod in (STFTMagnitude(171, 10, 60, "hann"), STFTMagnitude(512, 128, 512, "hann", center=False)):
        mod = mod.to(device)
        k = kernels(lambda: mod.pair_losses(x.clone().requires_grad_(), y).sum().backward())
        assert {"stft_loss_fwd_kernel", "stft_loss_bwd_kernel"} <= k and "stft_fft_fwd_kernel" not in k, k
    for kw in (dict(fft_size=171, hop_size=10, win_length=60, num_mels=40), dict(fft_size=512, hop_size=128, num_mels=130)):
        crit = MelSpectrogramLoss(fs=22050, fmin=0, fmax=11025, **kw).to(device)
        k = kernels(lambda: crit(x.clone().requires_grad_(), y).backward())
        assert {"mel_loss_fwd_kernel", "mel_loss_bwd_kernel"} <= k and "mel_fft_fwd_kernel" not in k, (kw, k)

"""No GPU: the float64 references of tests/loss_refs.py pinned to ``torch.stft`` and autograd, and what the table of
tests/test_loss_matrix_gpu.py rests on: the float32 room under every bar, the conditions its data must meet for the
discontinuous terms, the sensitivity of every row to the errors a loss kernel is likely to have, the table's axes, the map
from entry points to the tests that drive them, the Slaney range tables and the refusals of the FFT path."""
import importlib
import math
import os
import re

import numpy as np
import pytest
import torch

from parallelwavegan_amd import _lib
from tests import loss_refs as R
from tests import test_loss_matrix_gpu as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = torch.float64
TIGHT = 1e-10


def _rel(a, b):
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-300)


# ------------------------------------------------------------------------------------------------ references vs torch
# n_fft, hop, win, B, T: an odd n_fft - win, the shortest signals, hop > win, win = n_fft, hop 1
GEOMETRIES = [(64, 16, 37, 2, 100), (32, 5, 32, 2, 17), (32, 8, 9, 1, 18), (128, 50, 20, 2, 300), (16, 1, 5, 1, 23),
              (256, 64, 199, 1, 400)]
EPS = 1e-7


def _pin_data(n_fft, hop, win, b, t):
    g = torch.Generator().manual_seed(n_fft + t)
    w = ((0.15 + torch.rand(win, generator=g)) * torch.linspace(0.3, 1.0, win)).double()  # asymmetric
    return w, torch.randn(b, t, generator=g, dtype=D), torch.randn(b, t, generator=g, dtype=D)


def _torch_mag(s, n_fft, hop, win, w, eps):
    sp = torch.stft(s, n_fft, hop, win, w, center=True, pad_mode="reflect", return_complex=True)
    return torch.sqrt(torch.clamp(sp.real ** 2 + sp.imag ** 2, min=eps)).transpose(2, 1)  # (B, frames, bins)


@pytest.mark.parametrize("fft", [False, True], ids=["dft", "fft"])
@pytest.mark.parametrize("n_fft,hop,win,b,t", GEOMETRIES)
def test_stft_references_equal_torch_stft_and_autograd(n_fft, hop, win, b, t, fft):
    """pair_sums, and pair_dspec -> dframes_of -> overlap_add, against the formulas of losses/stft_loss.py:16-40, :61, :82
    on torch.stft in float64, for g2 = (1, 1), (-0.7, 0), (0, 2.5)."""
    w, x, y = _pin_data(n_fft, hop, win, b, t)
    off = (n_fft - win) // 2
    X, Y = R.spectra(R.frames(x, n_fft, hop, win, w), fft), R.spectra(R.frames(y, n_fft, hop, win, w), fft)
    sums = R.pair_sums(X, Y, EPS)
    xd = x.clone().requires_grad_()
    xm, ym = _torch_mag(xd, n_fft, hop, win, w, EPS), _torch_mag(y, n_fft, hop, win, w, EPS)
    assert xm.shape == X[0].shape and xm.shape[1] == R.n_frames(t, n_fft, hop)
    sc = torch.norm(ym - xm, p="fro") / torch.norm(ym, p="fro")
    mag = torch.nn.functional.l1_loss(torch.log(ym), torch.log(xm))
    want = torch.stack([((ym - xm) ** 2).sum(), (ym ** 2).sum(), (torch.log(ym) - torch.log(xm)).abs().sum(), sc, mag])
    assert _rel(sums, want.detach()) <= TIGHT and abs(sums[3] / sc.item() - 1) <= TIGHT and abs(sums[4] / mag.item() - 1) <= TIGHT
    for g2 in (M.G11, M.GSC, M.GMAG):
        xd.grad = None
        (g2[0] * sc + g2[1] * mag).backward(retain_graph=True)
        ds = R.pair_dspec(X, Y, EPS, sums, g2, 1.0 / xm.numel())
        dx = R.overlap_add(R.dframes_of(ds, w, off, win, n_fft, fft), t, n_fft, hop, win)
        assert _rel(dx, xd.grad) <= TIGHT, g2


def test_pair_dspec_rules():
    """gd = 0 where sums[0] == 0 (whatever x and y are); the clamp passes the gradient where p >= eps, and only there;
    sign(0) = 0."""
    X = (torch.tensor([[[3.0, 0.1, 2.0]]], dtype=D), torch.tensor([[[4.0, 0.0, 0.0]]], dtype=D))
    Y = (torch.tensor([[[1.0, 5.0, 2.0]]], dtype=D), torch.zeros(1, 1, 3, dtype=D))
    eps = 0.01  # p = 25, 0.01 (== eps: passes), 4
    dre, dim = R.pair_dspec(X, Y, eps, torch.tensor([0.0, 2.0]), (1.0, 0.0), 1.0)
    assert float(dre.abs().max()) == 0.0 and float(dim.abs().max()) == 0.0
    dre, _ = R.pair_dspec(X, Y, eps, torch.tensor([0.0, 2.0]), (1.0, 3.0), 1.0)
    assert dre[0, 0, 2].item() == 0.0                                  # |Y| == |X|: sign(0) = 0, and gd = 0
    assert dre[0, 0, 1].item() == pytest.approx(-3.0 / 0.1 / 0.1 * 0.1)  # p == eps passes: -gl * sign(+) / mx / mx * re
    dre, _ = R.pair_dspec(X, Y, 0.0101, torch.tensor([0.0, 2.0]), (1.0, 3.0), 1.0)
    assert dre[0, 0, 1].item() == 0.0                                  # p < eps: clamped, no gradient


@pytest.mark.parametrize("log_div", [1.0, M.LN2, M.LN10])
@pytest.mark.parametrize("n_fft,hop,win,b,t", GEOMETRIES[:4])
def test_mel_references_equal_torch_stft_and_autograd(n_fft, hop, win, b, t, log_div):
    """mel_pair, mel_dmag and mel_dspec against the formulas of losses/mel_loss.py:95-110 (clamped magnitude, filterbank,
    clamp, log / log_div, L1 mean) on torch.stft in float64, over a filterbank with an empty filter, a one-bin filter, a
    filter over all bins and bins no filter covers."""
    w, x, y = _pin_data(n_fft, hop, win, b, t)
    bins, eps = n_fft // 2 + 1, 1e-10
    fb, mel_range, bin_range = R.make_filters([(1, 4), (0, -1), (3, 3), (0, bins - 3), (2, 7)], bins, 5)
    assert (bin_range[bins - 1] == (0, -1)).all() and (mel_range[1] == (0, -1)).all() and fb.shape[1] % 32 == 0
    melmat = fb[:, :bins].T
    xd = x.clone().requires_grad_()
    lm = [torch.log(torch.clamp(torch.matmul(_torch_mag(s, n_fft, hop, win, w, eps), melmat), min=eps)) / log_div
          for s in (xd, y)]
    loss = torch.nn.functional.l1_loss(lm[0], lm[1])
    loss.backward()
    X, Y = R.spectra(R.frames(x, n_fft, hop, win, w)), R.spectra(R.frames(y, n_fft, hop, win, w))
    mel_x, mel_y, total = R.mel_pair(R.magnitude(X, eps), R.magnitude(Y, eps), fb, eps, log_div)
    n = mel_x.numel()
    assert abs(total.item() / n / loss.item() - 1) <= TIGHT
    ds = R.mel_dspec(X, R.mel_dmag(mel_x, mel_y, fb, eps, log_div, 1.0 / n), eps)
    dx = R.overlap_add(R.dframes_of(ds, w, (n_fft - win) // 2, win, n_fft), t, n_fft, hop, win)
    assert _rel(dx, xd.grad) <= TIGHT


def test_folded_frames_are_the_frames():
    """fold + frames_of_folded (the dense kernels' view of a signal) == frames, with n_cols at and above its minimum."""
    for n_fft, hop, win, b, t in GEOMETRIES + [(171, 7, 60, 2, 300)]:
        w, x, _ = _pin_data(n_fft, hop, win, b, t)
        fr = R.frames(x, n_fft, hop, win, w)
        for extra in (0, 2):
            n_cols = fr.shape[1] + -(-win // hop) - 1 + extra
            assert torch.equal(R.frames_of_folded(R.fold(x, n_fft, hop, win, n_cols), n_fft, hop, win, w, fr.shape[1]), fr)


def test_module_basis_is_the_windowed_dft():
    """STFTMagnitude.pair_basis (what the GPU rows hand the dense kernels) holds cos / -sin of 2 pi k (j + off) / n_fft
    times window[j] at [tap][c][group * 64 + (0 | 32) + bin % 32], zeros elsewhere: the explicit window tensor is taken as
    given and ``off`` is the floor of (n_fft - win) / 2."""
    c = M.DENSE_CASES[2]
    assert (c.n_fft - c.win) % 2 == 1
    pair = M._stft_module(c).pair_basis.double()
    w, off, bins = M.window_of(c).double(), (c.n_fft - c.win) // 2, c.n_fft // 2 + 1
    want = torch.zeros_like(pair)
    for j in range(c.win):
        for k in range(bins):
            ang = 2.0 * math.pi * ((k * (j + off)) % c.n_fft) / c.n_fft
            want[j // c.hop, j % c.hop, (k // 32) * 64 + k % 32] = math.cos(ang) * w[j]
            want[j // c.hop, j % c.hop, (k // 32) * 64 + 32 + k % 32] = -math.sin(ang) * w[j]
    assert (pair - want).abs().max().item() <= 2.0 ** -24 * 1.2


# ------------------------------------------------------------------------------------------------ the GPU table
CASES = M.EVERY_CASE
IDS = [c.id for c in CASES]


@pytest.fixture(scope="module")
def room():
    worst = {}
    yield worst
    by_kind = {}
    for (cid, name), err in worst.items():
        kind = "".join(ch for ch in name if not ch.isdigit())
        if err / M.bar_of(name) > by_kind.get(kind, (0, 0, ""))[0]:
            by_kind[kind] = (err / M.bar_of(name), err, cid)
    for kind, (share, err, cid) in sorted(by_kind.items()):
        print(f"float32 vs float64, worst {kind}: {err:.3e} ({share:.1%} of its bar) at {cid}")


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_room_under_the_bars(c, room):
    """The float32 CPU evaluation of the same formulas on the same data is within a quarter of every bar: what a kernel is
    allowed beyond float32 is summation order, not the data's conditioning.  For the stored mels, whose bar is DEFINED as
    8 x the worst float32 row, this asserts that the constant in the GPU file is at least that."""
    want, got = M.want(c), M.quantities(c, torch.float32)
    for name, ref in want.items():
        top = ref.abs().max().item()
        if top == 0.0:
            assert got[name].abs().max().item() == 0.0, name
            continue
        err = (got[name].double() - ref).abs().max().item() / top
        room[(c.id, name)] = err
        print(f"{c.id} {name}: float32 {err:.3e}")
        assert err <= 0.25 * M.bar_of(name), (name, err)


def _log_pairs(c, dtype):
    """For every backward launch of the row whose L1 term is live: (what, log a, log b, p of x or None)."""
    fr = M._Frames(c, dtype, None)
    if isinstance(c, (M.Fft, M.Dense)):
        for data, g2, _ in c.bwd:
            x, y = M._signals(c, data)
            X, Y = fr.spectra(x), fr.spectra(y)
            p = X[0] * X[0] + X[1] * X[1]
            if g2[1] != 0.0:
                yield data, torch.log(R.magnitude(Y, c.eps)), torch.log(R.magnitude(X, c.eps)), p
            else:
                yield data, None, None, p
    elif isinstance(c, M.MelFft):
        fb, _, _ = M.filters_of(c)
        for data, _ in c.bwd:
            x, y = M._signals(c, data)
            X = fr.spectra(x)
            mel_x, mel_y, _ = R.mel_pair(R.magnitude(X, c.eps), R.magnitude(fr.spectra(y), c.eps), fb, c.eps, c.log_div)
            yield data, torch.log(torch.clamp(mel_x, min=c.eps)), torch.log(torch.clamp(mel_y, min=c.eps)), \
                X[0] * X[0] + X[1] * X[1]
            yield data + " (mel clamp)", None, None, mel_x
    else:
        mx, my = M.stored_mels(c)
        X = fr.spectra(M._signals(c, c.data)[0])
        yield "stored", torch.log(torch.clamp(mx.to(dtype), min=c.eps)), torch.log(torch.clamp(my.to(dtype), min=c.eps)), \
            X[0] * X[0] + X[1] * X[1]
        yield "stored (mel clamp)", None, None, mx.to(dtype)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_data_keeps_off_the_discontinuities(c):
    """On the float64 reference alone, for every backward launch of the row: no log difference with 0 < |d| < tau, tau =
    8 x the largest error of the float32 CPU evaluation of that difference on the same data (printed); no p (and no stored
    or recomputed mel) within 5 % of eps unless it is exactly 0."""
    for (what, a, b, p), (_, a32, b32, _) in zip(_log_pairs(c, D), _log_pairs(c, torch.float32)):
        if a is not None:
            d = a - b
            tau = 8.0 * ((a32 - b32).double() - d).abs().max().item()
            live = d.abs()[d != 0]
            low = live.min().item() if live.numel() else float("inf")
            print(f"{c.id} {what}: {d.numel()} elements, min |dlog| {low:.3e}, float32 error {tau / 8:.3e}, tau {tau:.3e}")
            assert low >= tau, (what, low, tau)
        near = ((p / c.eps - 1.0).abs() < 0.05) & (p != 0)
        assert not bool(near.any()), (what, int(near.sum()), "values within 5 % of eps")


def _applicable(c, plant):
    mel = isinstance(c, (M.MelFft, M.MelDense))
    if plant == "image":  # needs a dx that is not all zeros
        return isinstance(c, (M.Fft, M.MelFft)) and c.data != "same"
    if plant == "filter":
        return mel
    if plant == "swap":  # needs a backward launch whose S_d term is live
        return not mel and any(g2[0] != 0 and not zero and "same" not in data for data, g2, zero in c.bwd)
    if plant == "frame":  # a row of one frame has none left to compare
        return M._n_frames(c) > 1
    if plant == "nyquist" and mel:  # some filter must weigh the last bin
        return bool(M.filters_of(c)[0][:, c.n_fft // 2].any())
    return True


def _fit(t, shape):
    """``t`` zero-padded at the end of every dimension to ``shape`` (a planted error that drops a frame or a filter)."""
    out = torch.zeros(shape, dtype=t.dtype)
    out[tuple(slice(0, n) for n in t.shape)] = t
    return out


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_sensitivity(c):
    """Each planted error -- the window reversed, ``off`` one off, the last bin dropped, the last frame dropped, one reflect
    image dropped from the overlap-add, the last mel filter dropped, x and y exchanged in S_d -- moves at least one compared
    quantity of the row by 100 x its bar, relative to that quantity's largest magnitude."""
    want = M.want(c)
    for plant in M.PLANTS:
        if not _applicable(c, plant):
            continue
        got = M.quantities(c, D, plant)
        moved = {}
        for name, ref in want.items():
            top = ref.abs().max().item()
            if top > 0.0:
                moved[name] = (_fit(got[name], ref.shape) - ref).abs().max().item() / top / M.bar_of(name)
        best = max(moved, key=moved.get)
        print(f"{c.id} {plant}: {best} moves by {moved[best]:.0f} bars")
        assert moved[best] >= 100.0, (plant, moved)


def test_table_covers_its_axes():
    f, mf, dn, md = M.FFT_CASES, M.MEL_FFT_CASES, M.DENSE_CASES, M.MEL_DENSE_CASES
    units = lambda c: c.B * R.n_frames(c.T, c.n_fft, c.hop)  # noqa: E731
    cap = lambda c: 256 * (4 if c.n_fft == 2048 else 8)      # noqa: E731
    for rows in (f, mf):
        assert {c.n_fft for c in rows} == {256, 512, 1024, 2048}
        assert any(units(c) < cap(c) for c in rows)
        assert any(cap(c) < units(c) < 2 * cap(c) and units(c) % cap(c) for c in rows)
    assert {(c.n_fft, units(c)) for c in f} >= {(256, 2103), (2048, 1053), (256, 4203)}
    assert all(M.fft_grid(c) == min(units(c), cap(c)) for c in f + mf)
    assert {c.T - c.n_fft // 2 for c in f} >= {1, 2}
    assert {c.T % c.hop == 0 for c in f} == {True, False}
    assert any(c.hop > c.win for c in f) and any(c.hop == 1 for c in f) and any(c.win == 3 for c in f)
    assert any(c.win == c.n_fft for c in f) and any((c.n_fft - c.win) % 2 for c in f)
    assert {c.data for c in f} >= {"noise", "silent", "same", "quiet"} and any(c.eps > 1e-3 for c in f)
    for rows in (f, dn):
        g2s = {(g2, zero) for c in rows for _, g2, zero in c.bwd}
        assert g2s >= {(M.G11, False), (M.GSC, False), (M.GMAG, False), (M.G11, True)}
        assert any(zero and "same" not in data for c in rows for data, _, zero in c.bwd)
        assert all(c.B <= 3 for c in rows)
    for c in CASES:  # asymmetric windows throughout
        w = M.window_of(c)
        assert c.win == 1 or not torch.equal(w, w.flip(0))
    assert {c.n_mels for c in mf} >= {1, 33, 80, 128} and {c.log_div for c in mf} == {1.0, M.LN2, M.LN10}
    assert any(g < 0 for c in mf for _, g in c.bwd) and any(c.supports == "slaney" for c in mf)
    sup = [s for c in mf if c.supports != "slaney" for s in [c.supports]]
    assert any(any(hi < lo for lo, hi in s) for s in sup) and any(any(hi == lo for lo, hi in s) for s in sup)
    assert any(any((lo, hi) == (0, c.n_fft // 2) for lo, hi in c.supports) for c in mf if c.supports != "slaney")
    assert any((M.filters_of(c)[2][:, 1] < 0).any() for c in mf if c.supports != "slaney")  # bins no filter covers
    assert {c.n_fft // 2 + 1 for c in dn} >= {11, 32, 33, 86, 193, 342} and {c.n_fft for c in dn} >= {20, 62, 64, 171, 384, 683}
    assert {c.frames for c in dn} >= {1, 31, 32, 33, 65}
    assert {M.dense_units(c) % 4 for c in dn} == {0, 1, 2, 3} == {M.dense_units(c) % 4 for c in md}
    assert {c.hop for c in dn} >= {1, 2, 7, 30}
    assert any(c.win <= c.hop for c in dn) and any(c.win % c.hop for c in dn)
    assert {c.extra > 0 for c in dn} == {True, False} == {c.extra > 0 for c in md}
    assert {c.data for c in dn} >= {"noise", "silent", "same", "quiet"}
    assert {c.n_mels for c in md} >= {1, 31, 32, 33, 80, 130} and {c.fb for c in md} == {"dense", "slaney"}
    assert any(c.gout < 0 for c in md) and {c.log_div for c in md} == {1.0, M.LN2, M.LN10}
    for c in md:
        mx, my = M.stored_mels(c)
        if mx.numel() > 20:
            assert bool(((mx < c.eps) & (mx > 0)).any()) and bool((mx == 0).any()) and bool(((mx == my) & (mx >= c.eps)).any())


# ------------------------------------------------------------------------------------------------ completeness
def _entry_points():
    names, total = [], 0
    for f in ("stft_fft.hip", "stft_loss.hip"):
        src = open(os.path.join(ROOT, "parallelwavegan_amd", "csrc", f)).read()
        names += re.findall(r'^extern "C" (?:int|size_t) (pwg_\w+)\(', src, re.M)
        total += len(re.findall(r'extern "C"', src))
    return names, total


def test_every_entry_point_names_the_test_that_drives_it():
    names, total = _entry_points()
    assert len(names) == 12 == total, names
    header = open(os.path.join(ROOT, "include", "pwg_kernels.h")).read()
    assert all(re.search(rf"\b{n}\(", header) for n in names)
    gpu = importlib.import_module("tests.test_loss_matrix_gpu")
    assert sorted(gpu.COVERED) == sorted(names), (sorted(set(names) ^ set(gpu.COVERED)))
    marks = getattr(gpu, "pytestmark", [])
    marks = list(marks) if isinstance(marks, (list, tuple)) else [marks]
    src = open(gpu.__file__).read()
    for name, where in gpu.COVERED.items():
        fn = getattr(gpu, where, None)
        assert callable(fn) and where.startswith("test_"), f"{name}: no test function {where}"
        assert any(m.name == "gpu" for m in marks + list(getattr(fn, "pytestmark", []))), f"{where} is not marked gpu"
        assert re.search(rf'\b{name}\b', src.split("COVERED = {")[1].split("}", 1)[1]), f"{name} is not called in the GPU file"


@pytest.mark.parametrize("n_fft", [1024, 2048])
def test_slaney_range_tables_hold_the_filterbank(n_fft):
    """MelFftPairLossFn._tables at 80 mels: mel_range is the non-zero support of each row of mel_b, and every non-zero
    fb[j][k] lies inside bin_range[k] -- the table that lets the backward kernel skip filters."""
    from parallelwavegan_amd.losses import MelSpectrogramLoss
    from parallelwavegan_amd.losses.mel_loss import MelFftPairLossFn

    ms = MelSpectrogramLoss(fs=24000 if n_fft == 2048 else 22050, fft_size=n_fft, hop_size=256, num_mels=80, fmin=0,
                            fmax=None).mel_spectrogram
    fb, mel_range, bin_range = (t.numpy() for t in MelFftPairLossFn._tables(ms, torch.device("cpu")))
    bins = n_fft // 2 + 1
    assert fb.shape == (80, 32 * ((bins + 31) // 32)) and np.array_equal(fb, ms.mel_b[:80].numpy()) and not fb[:, bins:].any()
    for j in range(80):
        nz = np.nonzero(fb[j])[0]
        assert nz.size and tuple(mel_range[j]) == (nz[0], nz[-1]), j
    for j, k in zip(*np.nonzero(fb)):
        assert bin_range[k, 0] <= j <= bin_range[k, 1], (j, k)


def test_fft_path_refusals():
    ok = _lib.lib().pwg_stft_fft_supported
    for n_fft in (256, 512, 1024, 2048):
        assert ok(n_fft, n_fft, 1) and ok(n_fft, 1, 5000)
    for n_fft, win, hop in ((128, 128, 32), (4096, 1024, 256), (768, 512, 128), (1000, 400, 100), (512, 513, 128),
                            (512, 0, 128), (512, 400, 0), (512, -1, 128), (512, 400, -3)):
        assert not ok(n_fft, win, hop), (n_fft, win, hop)

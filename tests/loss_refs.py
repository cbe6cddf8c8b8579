"""Plain references of what ONE launch of the STFT / mel loss kernels (csrc/stft_fft.hip, csrc/stft_loss.hip) computes,
in the dtype of their inputs (float64 for the bars, float32 to measure the room under them).  CPU only; no project
kernel and no ``torch.stft`` in here -- tests/test_loss_refs_host.py pins these functions to ``torch.stft`` and autograd.

Spectra are (re, im) pairs of (B, frames, bins) tensors.  ``fft=True`` takes the transform through ``numpy.fft`` (float64)
or ``torch.fft`` (float32) instead of the dense DFT matrix: the big rows of the GPU table use it, the host test pins
the two to each other on the small ones."""
import math

import numpy as np
import torch

D = torch.float64


def n_frames(t, n_fft, hop):
    """torch.stft(center=True): 1 + (T + 2 (n_fft // 2) - n_fft) // hop  (= 1 + T // hop for an even n_fft)."""
    return 1 + (t + 2 * (n_fft // 2) - n_fft) // hop


def reflect_index(t, half):
    """Sample of x behind every position of the signal reflect-padded by ``half`` on both sides (T > half)."""
    assert t > half
    p = torch.arange(-half, t + half)
    p = p.abs()
    return torch.where(p >= t, 2 * (t - 1) - p, p)


def padded_window(window, n_fft, win, off=None):
    off = (n_fft - win) // 2 if off is None else off
    w = torch.zeros(n_fft, dtype=window.dtype)
    w[off:off + win] = window
    return w


def frames(x, n_fft, hop, win, window, off=None):
    """(B, frames, n_fft): reflect-pad by n_fft // 2, cut a frame every ``hop``, window placed at ``off``."""
    b, t = x.shape
    padded = x[:, reflect_index(t, n_fft // 2)]
    pos = torch.arange(n_frames(t, n_fft, hop))[:, None] * hop + torch.arange(n_fft)[None, :]
    return padded[:, pos] * padded_window(window.to(x.dtype), n_fft, win, off)


def fold(x, n_fft, hop, win, n_cols):
    """The folded signal the dense kernels read: (B, hop, n_cols), folded[c][q] = padded[q * hop + c + off]
    (zero past the padded signal)."""
    b, t = x.shape
    off = (n_fft - win) // 2
    padded = x[:, reflect_index(t, n_fft // 2)]
    flat = torch.zeros(b, hop * n_cols + off, dtype=x.dtype)
    n = min(flat.shape[1], padded.shape[1])
    flat[:, :n] = padded[:, :n]
    return flat[:, off:].reshape(b, n_cols, hop).transpose(1, 2).contiguous()


def frames_of_folded(fx, n_fft, hop, win, window, n_fr, off=None):
    """(B, frames, n_fft) from a folded signal: sample j = tap * hop + c of frame f is fx[c][f + tap], j < win."""
    off = (n_fft - win) // 2 if off is None else off
    j = torch.arange(win)
    cols = torch.arange(n_fr)[:, None] + (j // hop)[None, :]
    fr = torch.zeros(fx.shape[0], n_fr, n_fft, dtype=fx.dtype)
    fr[:, :, off:off + win] = fx[:, (j % hop)[None, :].expand(n_fr, win), cols] * window.to(fx.dtype)
    return fr


def dft_matrix(n_fft, dtype=D):
    """cos, sin of 2 pi k n / n_fft, (bins, n_fft), k = 0 .. n_fft // 2: angles reduced mod n_fft in integers."""
    kn = (torch.arange(n_fft // 2 + 1)[:, None] * torch.arange(n_fft)[None, :]) % n_fft
    ang = kn.to(D) * (2.0 * math.pi / n_fft)
    return torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)


def spectra(fr, fft=False):
    """X[k] = sum_n fr[n] e^{-2 pi i k n / N}, k = 0 .. N // 2 -> (re, im)."""
    if fft:
        if fr.dtype == D:
            s = np.fft.rfft(fr.numpy(), axis=-1)
            return torch.from_numpy(np.ascontiguousarray(s.real)), torch.from_numpy(np.ascontiguousarray(s.imag))
        s = torch.fft.rfft(fr, dim=-1)
        return s.real.contiguous(), s.imag.contiguous()
    c, s = dft_matrix(fr.shape[-1], fr.dtype)
    return fr @ c.T, -(fr @ s.T)


def magnitude(X, eps):
    return torch.sqrt(torch.clamp(X[0] * X[0] + X[1] * X[1], min=eps))


def pair_sums(X, Y, eps):
    """S_d = sum (|Y| - |X|)^2, S_y = sum |Y|^2, S_l = sum |log|Y| - log|X||, sc = sqrt(S_d) / sqrt(S_y), mag = S_l / n."""
    mx, my = magnitude(X, eps), magnitude(Y, eps)
    s_d, s_y = ((my - mx) ** 2).sum(), (my * my).sum()
    s_l = (torch.log(my) - torch.log(mx)).abs().sum()
    return torch.stack([s_d, s_y, s_l, torch.sqrt(s_d) / torch.sqrt(s_y), s_l / mx.numel()])


def pair_dspec(X, Y, eps, sums, g2, inv_n, swap_sd=False):
    """d (g2[0] sc + g2[1] mag) / d (re X, im X) given ``sums`` (an INPUT: S_d, S_y of whoever calls).  gd = 0 where
    sums[0] == 0 (the zero subgradient of the Frobenius norm), the clamp passes the gradient where p >= eps,
    sign(0) = 0.  ``swap_sd``: a planted error (x and y exchanged in the S_d term)."""
    dt = X[0].dtype
    s_d, s_y = float(sums[0]), float(sums[1])
    gd = float(g2[0]) / (2.0 * math.sqrt(s_d) * math.sqrt(s_y)) if s_d > 0.0 else 0.0
    gl = float(g2[1]) * inv_n
    p = X[0] * X[0] + X[1] * X[1]
    mx, my = torch.sqrt(torch.clamp(p, min=eps)), magnitude(Y, eps)
    dl = torch.log(my) - torch.log(mx)
    dm = -2.0 * gd * ((mx - my) if swap_sd else (my - mx)) - gl * torch.sign(dl) / mx
    s = torch.where(p >= eps, dm / mx, torch.zeros((), dtype=dt))
    return s * X[0], s * X[1]


def dframes_of(dspec, window, off, win, n_fft, fft=False):
    """Adjoint of the real DFT, windowed: d xw[n] = sum_k dre[k] cos(2 pi k n / N) - dim[k] sin(2 pi k n / N),
    dframes[j] = window[j] * d xw[j + off] -> (B, frames, win)."""
    dre, dim = dspec
    if fft and dre.dtype == D:
        g = np.zeros(dre.shape[:-1] + (n_fft,), dtype=np.complex128)
        g[..., :dre.shape[-1]] = dre.numpy() + 1j * dim.numpy()
        dxw = torch.from_numpy(np.ascontiguousarray(np.fft.ifft(g, axis=-1).real * n_fft))
    elif fft:
        g = torch.zeros(dre.shape[:-1] + (n_fft,), dtype=torch.complex64)
        g[..., :dre.shape[-1]] = torch.complex(dre, dim)
        dxw = torch.fft.ifft(g, dim=-1).real * n_fft
    else:
        c, s = dft_matrix(n_fft, dre.dtype)
        dxw = dre @ c - dim @ s
    return dxw[..., off:off + win] * window.to(dre.dtype)


def overlap_add(dframes, t, n_fft, hop, win, off=None, images=(0, 1, 2)):
    """Adjoint of ``frames``: every windowed frame sample goes back to the sample of x the reflect padding took it from.
    ``images``: which of (left reflection, the signal itself, right reflection) are kept -- all three unless an error
    is planted."""
    b, n_fr, _ = dframes.shape
    half = n_fft // 2
    off = (n_fft - win) // 2 if off is None else off
    pos = (torch.arange(n_fr)[:, None] * hop + off + torch.arange(win)[None, :]).reshape(-1)
    image = torch.where(pos < half, 0, torch.where(pos >= half + t, 2, 1))
    keep = torch.isin(image, torch.tensor(images))
    src = reflect_index(t, half)[pos]
    dx = torch.zeros(b, t, dtype=dframes.dtype)
    dx.index_add_(1, src[keep], dframes.reshape(b, -1)[:, keep])
    return dx


# ------------------------------------------------------------------------------------------------ mel
def mel_pair(mag_x, mag_y, fb, eps, log_div):
    """mel = |X| . fb^T, stored (B, n_mels, frames) BEFORE the clamp;
    total = sum |log clamp(mel_x) - log clamp(mel_y)| / log_div."""
    fbt = fb[:, :mag_x.shape[-1]].to(mag_x.dtype).T  # (fb may be padded to bins_pad columns)
    mel_x, mel_y = (mag_x @ fbt).transpose(1, 2), (mag_y @ fbt).transpose(1, 2)
    total = (torch.log(torch.clamp(mel_x, min=eps)) - torch.log(torch.clamp(mel_y, min=eps))).abs().sum() / log_div
    return mel_x.contiguous(), mel_y.contiguous(), total


def mel_dmag(mel_x, mel_y, fb, eps, log_div, gout):
    """d (gout * total) / d |X| (B, frames, bins) from the stored mels (INPUTS): zero where mel_x < eps, sign(0) = 0."""
    dt = mel_x.dtype
    lx, ly = torch.log(torch.clamp(mel_x, min=eps)), torch.log(torch.clamp(mel_y, min=eps))
    dmel = torch.where(mel_x >= eps, torch.sign(lx - ly) * (gout / log_div) / mel_x, torch.zeros((), dtype=dt))
    return dmel.transpose(1, 2) @ fb.to(dt)


def mel_dspec(X, dmag, eps):
    """|X| = sqrt(clamp(p, eps)): the clamp passes the gradient where p >= eps."""
    p = X[0] * X[0] + X[1] * X[1]
    dmag = dmag[..., :p.shape[-1]]
    sc = torch.where(p >= eps, dmag / torch.sqrt(torch.clamp(p, min=eps)), torch.zeros((), dtype=p.dtype))
    return sc * X[0], sc * X[1]


def make_filters(supports, bins, seed, bins_pad=None):
    """A filterbank from (first bin, last bin) supports (last < first: an empty filter) with random weights in
    [0.25, 1] that float32 holds exactly -> fb (n_mels, bins_pad) float64, mel_range (n_mels, 2), bin_range (bins, 2)
    int32 as csrc/stft_fft.hip reads them: per filter its support, per bin the first / last filter whose support holds it
    ((0, -1): none)."""
    bins_pad = bins_pad or 32 * ((bins + 31) // 32)
    g = torch.Generator().manual_seed(seed)
    fb = torch.zeros(len(supports), bins_pad, dtype=D)
    mel_range = np.zeros((len(supports), 2), dtype=np.int32)
    for j, (lo, hi) in enumerate(supports):
        assert hi < bins and lo >= 0
        if hi >= lo:
            fb[j, lo:hi + 1] = (0.25 + 0.75 * torch.rand(hi - lo + 1, generator=g)).float().double()
            mel_range[j] = (lo, hi)
        else:
            mel_range[j] = (0, -1)
    bin_range = np.zeros((bins, 2), dtype=np.int32)
    for k in range(bins):
        cover = [j for j, (lo, hi) in enumerate(supports) if lo <= k <= hi]
        bin_range[k] = (cover[0], cover[-1]) if cover else (0, -1)
    return fb, mel_range, bin_range

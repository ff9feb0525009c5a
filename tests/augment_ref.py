"""NumPy restatement of the rendering rule of the augmented trainers (test infrastructure): what csrc/fft_render.hip must
compute, in float64 on the host.  A track is ``(x, k, g, c)``: source signal, shift in samples, gain, output channel.

    r_s[n] = g_s * x_s[n - k_s] if 0 <= n - k_s < len(x_s) else 0,   0 <= n < size
    mix[n] = m * (((r_0 + r_1) + r_2) + ...)                         in list order

Every product and sum is one float64 operation, as NumPy evaluates it: the device's float64 path does the same operations
in the same order without fused multiply-adds, so its frames are compared bit for bit."""
import numpy as np

from oracle import stft_np


def shifted(x, size, k, g=1.0):
    """``g * circular_shift(x, min_size=size)`` for a shift of ``k`` samples, by the closed form."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros(int(size))
    n0, n1 = max(0, k), min(int(size), len(x) + k)
    if n1 > n0:
        out[n0:n1] = x[n0 - k:n1 - k]
    return g * out


def render(tracks, m, size):
    """``[1 + S, size]`` float64: the mixture, then the rendered tracks at their output channels."""
    out = np.zeros((1 + len(tracks), int(size)))
    mix = None
    for x, k, g, c in tracks:
        out[c] = shifted(x, size, k, g)
        mix = out[c].copy() if mix is None else mix + out[c]
    out[0] = m * mix
    return out


def chunk_audio(rendered, a, Lc):
    """The ``[Lc, 1 + S]`` array the reference hands to compute_transform for the chunk ``[a, a + Lc)``."""
    return np.ascontiguousarray(rendered[:, a:a + Lc].T)


def blocks_np(rendered, chunks, frame, hop, window):
    """``[chunk] -> [1 + S, T, F]`` float64 through oracle/stft_np.compute_file (the reference's stft_norm)."""
    return [np.stack([stft_np.compute_file(rendered[j, a:a + Lc], frameSize=frame, hopSize=hop, window=window)
                      for j in range(rendered.shape[0])]) for a, Lc in chunks]

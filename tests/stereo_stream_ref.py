"""Float64 NumPy statement of the STEREO stream of csrc/stream.hip (``dcs_stream_create_stereo``, include/dcs.h) -- test
infrastructure, in the manner of ``stream_ref``.

The stereo (ILD) graph answers per (source, channel); the stereo trainer masks each input channel with the outputs of THAT
channel (examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100.py:176-189),

    m_sc = p_sc / (sum_s' p_s'c + e),      source_sc = m_sc * x_c + e,      e = 1e-12 * 0.1

and cross-fades the sources over the tiles (``overlapadd_multi``).  The stream folds the MASKS, multiplies with the unscaled
magnitudes and adds ``c0 = e / scale``: the same thing in exact arithmetic, because the cross-fade weights of a frame sum to one.
``whole_file`` is that statement on a complete signal; ``tests/test_stereo_stream_cpu.py`` ties it to
``oracle.pipeline.separate_stereo``.
"""
import numpy as np

from oracle import stft_np, tiling_np

import chanmask_ref

EPS_R = np.float32(1e-13)                     # dsd.hip MODE 3: 1e-12 x 0.1 as a float32 constant


def c0_f32(scale):
    """the constant on the unscaled magnitudes as create forms it: float32(1e-13) / float32(scale), in float32"""
    return float(np.float32(EPS_R / np.float32(scale)))


def tile_masks_ild(p, eps=None):
    """p ``[S, C, n, tc, F]`` (rectified network output, source s / input channel c = output channel ``s C + c``) -> the float64
    masks of the same shape: per channel, over the sources of that channel"""
    p = np.asarray(p, dtype=np.float64)
    e = float(EPS_R) if eps is None else float(eps)
    return p / (p.sum(axis=0, keepdims=True) + e)


def from_lasagne(p, S, C):
    """network output ``[S * C, n, tc, F]`` (or ``[n, S * C, tc, F]`` with ``batch_first``) -> ``[S, C, n, tc, F]``"""
    p = np.asarray(p)
    return p.reshape((S, C) + p.shape[1:])


def whole_file(audio, N, h, tc, ov, tiler, S, win, scale, p, mag=None, phase=None, c0=None, eps=None):
    """``audio [L, C]``, ``p [S, C, n, tc, F]`` for the tiles of the whole signal -> dict(mag, phase [C, T, F], est [C, S, T, F]
    on the UNSCALED magnitudes, pcm [C, S, L], T, n_tiles).  ``mag`` / ``phase`` given: evaluated at those (a device's own)
    instead of the oracle's.  Rows past the last tile are zeros, without ``c0`` (util.py:313)."""
    audio = np.asarray(audio, dtype=np.float64)
    L, C = audio.shape
    X = np.stack([stft_np.stft_norm(audio[:, c], win, float(h), float(N)) for c in range(C)])
    T, F = X.shape[1:]
    mag = np.abs(X) / np.sqrt(N) if mag is None else np.asarray(mag, dtype=np.float64)
    phase = np.angle(X) if phase is None else np.asarray(phase, dtype=np.float64)
    c0 = c0_f32(scale) if c0 is None else float(c0)
    n = len(tiling_np.tile_starts(T, tc, ov, tiler))
    p = np.asarray(p, dtype=np.float64)
    assert p.shape == (S, C, n, tc, F), (p.shape, (S, C, n, tc, F))
    m = tile_masks_ild(p, eps)
    est = np.zeros((C, S, T, F))
    covered = min(T, (n - 1) * (tc - ov) + tc) if n else 0
    for c in range(C):
        acc = chanmask_ref.fold(m[:, c], ov, n_frames=T)                  # [S, T, F]
        est[c, :, :covered] = acc[:, :covered] * mag[c][None, :covered] + c0
    pcm = np.stack([np.stack([stft_np.compute_inverse(est[c, s], phase[c], N, h, win)[:L] for s in range(S)]) for c in range(C)])
    return dict(mag=mag, phase=phase, est=est, pcm=pcm, T=T, n_tiles=n, covered=covered)


def bound(S, tc, ov, mag, c0=0.0):
    """``(S + 2 m + 5) 2^-23 (mag + c0)``: ``chanmask_ref.bound``'s rule -- twice the first-order float32 rounding count of the
    kernel: S - 1 additions, the eps addition, one division, two roundings per fold step, one product -- with one more rounding
    for the added constant"""
    return (S + 2 * chanmask_ref.covering_tiles(tc, ov) + 5) * 2.0 ** -23 * (np.asarray(mag, dtype=np.float64) + c0)


def make_p(rs, S, C, n, tc, F):
    """synthetic rectified outputs in the Lasagne layout ``[S * C, n, tc, F]`` float32, built like ``chanmask_ref.make_p``:
    scales from 1e-19 to 50, a third exact zeros, column 3 all-zero, column 5 with a single live source per channel"""
    scale = np.array([1e-19, 1e-6, 1.0, 50.0])[rs.randint(0, 4, (S, C, n, tc, F))]
    p = (rs.rand(S, C, n, tc, F) * scale * (rs.rand(S, C, n, tc, F) > 1.0 / 3)).astype(np.float32)
    p[..., 3] = 0
    p[1:, ..., 5] = 0
    p[0, ..., 5] = np.maximum(p[0, ..., 5], np.float32(1e-19))
    return p.reshape(S * C, n, tc, F)


def tile_p(k, S, C, tc, F, seed=0):
    """the synthetic output of tile k, ``[S * C, tc, F]``: a seeded function of the absolute tile index"""
    rs = np.random.RandomState((7919 * (seed + 1) + 31 * k) % (2 ** 31 - 1))
    return make_p(rs, S, C, 1, tc, F)[:, 0]

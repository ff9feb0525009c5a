"""Float64 statement of ``dcs_mask_fold_apply`` (include/dcs.h) and the cases its tests run.

The masks are the reference's (separate_dsd.py:258-271, separate_bach10.py:251-264) as ``oracle/maskcheck.py`` writes them,

    A:  m_i = (p_i + e) / (sum_j p_j + S e)        B:  m_i = p_i / (sum_j p_j + e),      e = 5e-19

stitched over the tiles by ``oracle.tiling_np.overlapadd_multi`` (util.py:297-327) and multiplied by each channel's magnitudes.
"""
import numpy as np

from oracle import tiling_np
from oracle.maskcheck import EPS_R

CONVENTIONS = ("A", "B")                      # DCS_EPS_A = 0, DCS_EPS_B = 1


def tile_masks(p, conv):
    """p ``[S, n, tc, F]`` (rectified network output) -> float64 masks of the same shape"""
    p = np.asarray(p, dtype=np.float64)
    S = p.shape[0]
    if conv == "A":
        return (p + EPS_R) / (p.sum(axis=0) + S * EPS_R)
    return p / (p.sum(axis=0) + EPS_R)


def _fit(x, n_frames):
    """rows cut or zero-padded to n_frames (axis -2)"""
    if n_frames is None or n_frames == x.shape[-2]:
        return x
    if n_frames < x.shape[-2]:
        return np.ascontiguousarray(x[..., :n_frames, :])
    pad = np.zeros(x.shape[:-2] + (n_frames - x.shape[-2], x.shape[-1]))
    return np.concatenate([x, pad], axis=-2)


def fold(m, overlap, n_frames=None):
    """the sequential cross-fade of ``overlapadd_multi`` on ``m [S, n, tc, F]`` -> ``[S, n_frames, F]`` (default: all
    ``n (tc - overlap) + tc`` rows; rows past them are zero)"""
    m = np.asarray(m, dtype=np.float64)
    n = m.shape[1]
    sep = tiling_np.overlapadd_multi(m[None, :, :, None], n, overlap)       # [nb = 1, S, B = n, 1, tc, F]
    return _fit(sep, n_frames)


def fold_frame_parallel(m, overlap, n_frames=None):
    """the same through the per-frame closed form the kernel follows"""
    m = np.asarray(m, dtype=np.float64)
    return _fit(np.stack([tiling_np.overlapadd_frame_parallel(m[s], overlap) for s in range(m.shape[0])]), n_frames)


def chanmask_ref(p, mag, overlap, conv, n_frames=None):
    """p ``[S, n, tc, F]``, mag ``[C, T, F]`` (T >= n_frames, default n_frames = T) -> (est ``[C, S, n_frames, F]``, mask
    ``[S, n_frames, F]``), float64"""
    mag = np.asarray(mag, dtype=np.float64)
    rows = mag.shape[1] if n_frames is None else n_frames
    mask = fold(tile_masks(p, conv), overlap, rows)
    return mask[None] * mag[:, None, :rows], mask


def covering_tiles(tc, overlap):
    """m = ceil(ov / st) + 1: the tiles that can reach one frame"""
    st = tc - overlap
    return (overlap + st - 1) // st + 1


def bound(S, tc, overlap, mag=1.0):
    """``(S + 2 m + 4) 2^-23 mag``: twice the first-order float32 rounding count of the kernel -- S - 1 additions, the eps
    addition, one division, two roundings per fold step, one product"""
    return (S + 2 * covering_tiles(tc, overlap) + 4) * 2.0 ** -23 * np.asarray(mag, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ the cases
SHAPES = ((30, 25), (30, 20), (8, 5), (8, 1), (30, 29))
TILES = (0, 1, 2, 11)
SOURCES = (1, 2, 4, 5, 8, (4, 6))             # (4, 6): S = 4 read out of a buffer of 6 channels (p_src_stride spans 6)
CHANNELS = (1, 2, 3)
ROWS = ("below", "equal", "above")            # n_frames against n st + tc
BINS = ((33, 40), (70, 72))


def kernel_path(S, tc, overlap):
    """which instantiation the launcher picks: 'mm3' / 'mm6' (all tiles of a frame requested at once, S 2 or 4), 'loop'"""
    m = covering_tiles(tc, overlap)
    if S in (2, 4) and m <= 3:
        return "mm3"
    if S in (2, 4) and m <= 6:
        return "mm6"
    return "loop"


def make_p(rs, CH, n, tc, F):
    """rectified outputs at scales 1e-19, 1e-6, 1 and 50, a third of them exactly zero; column 3: every source zero; column 5:
    only source 0 non-zero"""
    scale = np.array([1e-19, 1e-6, 1.0, 50.0])[rs.randint(0, 4, (CH, n, tc, F))]
    p = (rs.rand(CH, n, tc, F) * scale * (rs.rand(CH, n, tc, F) > 1.0 / 3)).astype(np.float32)
    p[..., 3] = 0
    p[1:, ..., 5] = 0
    p[0, ..., 5] = np.maximum(p[0, ..., 5], np.float32(1e-19))
    return p


def make_mag(rs, C, T, F):
    mag = (rs.rand(C, T, F) * np.array([1e-3, 1.0, 300.0])[rs.randint(0, 3, (C, T, F))]).astype(np.float32)
    mag[:, :, 7] = 0
    return mag


def build_cases():
    """name -> dict(p [CH, n, tc, F] float32, S, mag [C, T, F] float32, tc, ov, conv, n_frames, F, ld).  Every (tc, ov) meets
    every tile count under both conventions; S, C, the row count and the bin count cycle through their values so that every
    S value meets every kernel path it can take (test_chanmask_ref_cpu.py checks the table)."""
    cases = {}

    def add(i, j, c, tc, ov, n, S_spec, C, rows, F, ld, seed):
        S, CH = S_spec if isinstance(S_spec, tuple) else (S_spec, S_spec)
        total = n * (tc - ov) + tc
        n_frames = {"below": max(1, total - 7), "equal": total, "above": total + 5}[rows]
        rs = np.random.RandomState(seed)
        name = "tc%d_ov%d_n%d_S%d%s_C%d_%s_%s_F%d" % (tc, ov, n, S, "of%d" % CH if CH != S else "", C, CONVENTIONS[c], rows, F)
        cases[name] = dict(p=make_p(rs, CH, n, tc, F), S=S, mag=make_mag(rs, C, n_frames, F), tc=tc, ov=ov,
                           conv=CONVENTIONS[c], n_frames=n_frames, F=F, ld=ld)

    for i, (tc, ov) in enumerate(SHAPES):
        for j, n in enumerate(TILES):
            for c in range(2):
                F, ld = BINS[(i + j) % 2]
                add(i, j, c, tc, ov, n, SOURCES[(i + 4 * j + 3 * c) % 6], CHANNELS[(i + j + c) % 3], ROWS[(i + 2 * j + c) % 3],
                    F, ld, 100 * i + 10 * j + c)
    # every S on every path the cycling above left out, at 11 tiles
    seen = set((kernel_path(v["S"], v["tc"], v["ov"]), v["S"], v["p"].shape[0]) for v in cases.values() if v["p"].shape[1] == 11)
    k = 0
    for i, (tc, ov) in enumerate(SHAPES):
        for S_spec in SOURCES:
            S, CH = S_spec if isinstance(S_spec, tuple) else (S_spec, S_spec)
            key = (kernel_path(S, tc, ov), S, CH)
            if key not in seen:
                seen.add(key)
                add(i, 3, k % 2, tc, ov, 11, S_spec, CHANNELS[k % 3], ROWS[k % 3], BINS[k % 2][0], BINS[k % 2][1], 1000 + k)
                k += 1
    # the separators' own bin count: more than one workgroup along the bins, a ragged last one
    add(0, 3, 0, 30, 25, 11, 4, 2, "equal", 513, 513, 2000)
    add(1, 3, 1, 30, 20, 11, 2, 2, "equal", 513, 513, 2001)
    return cases

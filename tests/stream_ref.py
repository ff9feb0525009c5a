"""Float64 NumPy statement of the STREAMING computation of csrc/stream.hip, and the cases its tests run (test infrastructure).

``StreamRef`` takes the signal block by block and emits frames, tiles, folded rows and samples on the schedule of
``deepconvsep_amd.streaming.StreamCounts``, keeping only bounded state (the samples, frame rows, tile outputs and windowed
time-domain frames a later push or pull can still reach; everything older is dropped and ``state_sizes`` reports what is held).
``whole_file`` is the computation it must reproduce: ``oracle.stft_np`` -> ``oracle.tiling_np`` -> ``chanmask_ref`` ->
``stft_np.compute_inverse`` on the complete signal.  Both use the same NumPy expressions in the same order, so they agree to
float64 round-off however the signal is cut.
"""
import numpy as np

from deepconvsep_amd.streaming import StreamCounts
from oracle import stft_np, tiling_np

import chanmask_ref

# (frameSize, hop, time_context, overlap, window)
SHAPES = (
    (64, 16, 8, 5, "hanning"),
    (64, 32, 8, 1, "hanning"),
    (128, 32, 30, 29, "hanning"),
    (1024, 512, 30, 25, "hanning"),
    (4096, 512, 30, 25, "hanning"),
    (4096, 512, 30, 25, "blackmanharris"),
)
TILERS = (tiling_np.SCRIPT, tiling_np.LIBRARY)
PARTITIONS = ("one", "hop", "random", "empty_last")
# the grid the look-ahead bound was found on
GRID_FRAMES = ((64, 16), (64, 32), (128, 32), (1024, 512), (1024, 256), (4096, 512))
GRID_TILES = ((8, 5), (8, 1), (30, 25), (30, 20), (30, 29))


def shape_id(shape):
    return "N%d_h%d_tc%d_ov%d_%s" % shape


def window(name, N):
    if name == "hanning":
        return np.hanning(N)
    from scipy.signal.windows import blackmanharris
    return blackmanharris(N)


def lengths(N, h, tc, ov):
    """three signal lengths with a few tiles each: not a multiple of the hop; a multiple of it; one where the script tiler drops
    a tail that the library tiler pads (as long a tail as the stride allows)"""
    st = tc - ov
    base = (tc + 3 * st + 1) * h
    out = [base + 7, base]
    for L in range(base + 3, base + 3 + (st + 1) * h, h):
        T = stft_np.frame_count(L, h)
        ks = len(tiling_np.tile_starts(T, tc, ov, tiling_np.SCRIPT))
        kl = len(tiling_np.tile_starts(T, tc, ov, tiling_np.LIBRARY))
        if ks >= 1 and kl > ks and T - ((ks - 1) * st + tc) >= min(2, st):
            out.append(L)
            return out
    raise AssertionError("no length with a dropped tail")


def partition(kind, L, h, seed=0):
    """block sizes that add up to L; the last block ends the signal"""
    if kind == "one":
        return [L]
    if kind == "hop":
        return [h] * (L // h) + ([L % h] if L % h else [])
    rs = np.random.RandomState(seed)
    sizes, left = [], L
    while left:
        n = 0 if rs.rand() < 0.2 else int(min(left, rs.randint(1, 2 * h + 2)))
        sizes.append(n)
        left -= n
    sizes.insert(len(sizes) // 2, 0)                                      # an empty push mid-stream, whatever the draw
    if kind == "empty_last":
        sizes.append(0)
    return sizes


def signal(L, seed=0):
    rs = np.random.RandomState(1000 + seed)
    t = np.arange(L)
    return 0.4 * np.sin(0.031 * t) + 0.2 * np.sin(0.37 * t + 1.0) + 0.1 * rs.randn(L)


def tile_p(k, S, tc, F, seed=0):
    """the synthetic rectified network output of tile k: a seeded POSITIVE function of the absolute tile index"""
    rs = np.random.RandomState((7919 * (seed + 1) + 31 * k) % (2 ** 31 - 1))
    return (0.05 + rs.rand(S, tc, F)).astype(np.float32)


def whole_file(audio, N, h, tc, ov, tiler, conv, S, win, scale=1.0, seed=0, p=None, mag=None, phase=None):
    """the whole-file composition -> dict(X, mag, phase, tiles, p, est [S, T, F], pcm [S, L]).  ``p`` / ``mag`` / ``phase``
    given: evaluated at those (a device's own) instead of the oracle's."""
    audio = np.asarray(audio, dtype=np.float64)
    L = audio.size
    X = stft_np.stft_norm(audio, win, float(h), float(N))
    T, F = X.shape
    if mag is None:
        mag = np.abs(X) / np.sqrt(N)
    if phase is None:
        phase = np.angle(X)
    mag, phase = np.asarray(mag, dtype=np.float64), np.asarray(phase, dtype=np.float64)
    starts = tiling_np.tile_starts(T, tc, ov, tiler)
    n = len(starts)
    fb, n2 = tiling_np.generate_overlapadd(scale * mag, F, tc, ov, max(n, 1), tiler)
    assert n2 == n
    tiles = fb.reshape(-1, tc, F)[:n]
    if p is None:
        p = np.stack([tile_p(k, S, tc, F, seed) for k in range(n)], axis=1) if n else np.zeros((S, 0, tc, F), np.float32)
    est, _ = chanmask_ref.chanmask_ref(p, mag[None], ov, conv, n_frames=T)
    est = est[0]
    pcm = np.stack([stft_np.compute_inverse(est[s], phase, N, h, win)[:L] for s in range(S)])
    return dict(X=X, mag=mag, phase=phase, tiles=tiles, p=p, est=est, pcm=pcm, T=T, n_tiles=n)


class StreamRef(object):
    """push(block, last) -> dict(X, tiles, first_tile); pull(p [S, n, tc, F]) -> dict(est [S, rows, F], pcm [S, n])"""

    def __init__(self, N, h, tc, ov, tiler, conv, S, win, scale=1.0):
        self.N, self.h, self.tc, self.ov, self.st, self.H = N, h, tc, ov, tc - ov, N // 2
        self.conv, self.S, self.win, self.scale = conv, S, np.asarray(win, dtype=np.float64), scale
        self.counts = StreamCounts(N, h, tc, ov, tiler)
        self.rise = np.linspace(0.0, 1.0, num=ov)
        self.reset()

    def reset(self):
        self.P = self.A = self.K = self.Tf = self.E = 0
        self.ended, self.pending = False, None
        self.hist = np.zeros(0)          # the last samples, hist[-1] = sample P - 1
        self.rows = {}                   # frame -> (mag row, phase row)
        self.masks = {}                  # tile -> masks [S, tc, F]
        self.tf = {}                     # frame -> windowed time-domain frames [S, N]

    def state_sizes(self):
        return dict(samples=self.hist.size, rows=len(self.rows), masks=len(self.masks), tf=len(self.tf))

    def _sample_run(self, a, b, lim):
        """samples [a, b) with zeros outside [0, lim)"""
        out = np.zeros(b - a)
        lo, hi = max(a, 0), min(b, lim)
        if hi > lo:
            first = self.P - self.hist.size
            assert lo >= first, "a frame reaches back past the sample history"
            out[lo - a:hi - a] = self.hist[lo - first:hi - first]
        return out

    def push(self, block, last=False):
        assert self.pending is None and not self.ended
        block = np.asarray(block, dtype=np.float64)
        self.hist = np.concatenate([self.hist, block])
        self.P += block.size
        c = self.counts
        A, K = c.frames(self.P, last), c.tiles(self.P, last)
        F = self.N // 2 + 1
        X = np.zeros((A - self.A, F), dtype=complex)
        for n in range(self.A, A):
            seg = self._sample_run(n * self.h - self.H, n * self.h - self.H + self.N, self.P)
            X[n - self.A] = np.fft.rfft(self.win * seg, self.N)
            self.rows[n] = (np.abs(X[n - self.A]) / np.sqrt(self.N), np.angle(X[n - self.A]))
        tiles = np.zeros((K - self.K, self.tc, F))
        for k in range(self.K, K):
            for j in range(self.tc):
                t = k * self.st + j
                if t < A:
                    tiles[k - self.K, j] = self.scale * self.rows[t][0]
        first_tile = self.K
        self.A, self.K, self.ended, self.pending = A, K, bool(last), K - first_tile
        self.hist = self.hist[max(0, self.hist.size - self.N):]           # a later frame reaches back less than N samples
        return dict(X=X, tiles=tiles, first_tile=first_tile)

    def pull(self, p):
        assert self.pending is not None and (0 if p is None else p.shape[1]) == self.pending
        c, S, st, tc, ov = self.counts, self.S, self.st, self.tc, self.ov
        F = self.N // 2 + 1
        if self.ended and self.K == 0:
            raise ValueError("no tile")
        for i in range(self.pending):
            k = self.K - self.pending + i
            self.masks[k] = chanmask_ref.tile_masks(p[:, i], self.conv)
        Tf, E = c.folded(self.P, self.ended), c.emitted(self.P, self.ended)
        est = np.zeros((S, Tf - self.Tf, F))
        for t in range(self.Tf, Tf):
            k0 = 0 if t < ov else min((t - ov) // st, self.K - 1)
            j0 = t - k0 * st
            if j0 < tc:
                acc = self.masks[k0][:, j0].copy()
                k = k0 + 1
                while k < self.K and k * st <= t:
                    j = t - k * st
                    acc = self.rise[::-1][j] * acc + self.rise[j] * self.masks[k][:, j]
                    k += 1
                est[:, t - self.Tf] = acc * self.rows[t][0][None]
            Xs = (est[:, t - self.Tf] * np.sqrt(self.N)) * np.exp(1j * self.rows[t][1])[None]
            self.tf[t] = self.win[None] * np.fft.irfft(Xs, self.N, axis=1)[:, :self.N]
        ww = self.win * self.win
        pcm = np.zeros((S, E - self.E))
        for n in sorted(self.tf):                      # increasing n: the accumulation order of istft_norm
            a = n * self.h - self.H                    # first output sample of frame n
            lo, hi = max(a, self.E), min(a + self.N, E)
            if hi > lo:
                pcm[:, lo - self.E:hi - self.E] += self.tf[n][:, lo - a:hi - a]
        norm = np.zeros(E - self.E)
        for q0 in range(0, E - self.E, 1 << 16):
            q = np.arange(self.E + q0, min(E, self.E + q0 + (1 << 16)))
            pp = q + self.H
            n_hi = np.minimum(pp // self.h, Tf - 1)
            n_lo = np.where(pp < self.N, 0, (pp - self.N) // self.h + 1)
            acc = np.zeros(q.size)
            for d in range(self.N // self.h):
                n = n_lo + d
                ok = n <= n_hi
                acc = np.where(ok, acc + ww[np.clip(pp - n * self.h, 0, self.N - 1)], acc)
            norm[q0:q0 + q.size] = acc
        norm[norm == 0] = 1.0
        pcm = pcm / norm[None]
        self.Tf, self.E, self.pending = Tf, E, None
        # what nothing later can reach: rows and masks below the next frame to fold / its first covering tile, time frames that
        # end before the next sample to emit
        for n in [n for n in self.rows if n < Tf]:
            del self.rows[n]
        k_min = 0 if Tf < ov else (Tf - ov) // st
        for k in [k for k in self.masks if k < min(k_min, self.K - 1)]:
            del self.masks[k]
        for n in [n for n in self.tf if n * self.h - self.H + self.N <= E]:
            del self.tf[n]
        return dict(est=est, pcm=pcm)

    def run(self, audio, sizes, seed=0):
        """the whole signal through the stream in blocks of ``sizes`` -> dict(X, tiles, est, pcm) concatenated, plus the largest
        state held"""
        audio = np.asarray(audio, dtype=np.float64)
        F = self.N // 2 + 1
        Xs, tiles, ests, pcms, pos, worst = [], [], [], [], 0, {}
        for i, n in enumerate(sizes):
            out = self.push(audio[pos:pos + n], last=(i == len(sizes) - 1))
            pos += n
            nt = out["tiles"].shape[0]
            p = np.stack([tile_p(out["first_tile"] + j, self.S, self.tc, F, seed) for j in range(nt)], axis=1) if nt else None
            got = self.pull(p)
            Xs.append(out["X"]); tiles.append(out["tiles"]); ests.append(got["est"]); pcms.append(got["pcm"])
            for key, v in self.state_sizes().items():
                worst[key] = max(worst.get(key, 0), v)
        assert pos == audio.size
        return dict(X=np.concatenate(Xs), tiles=np.concatenate(tiles), est=np.concatenate(ests, axis=1),
                    pcm=np.concatenate(pcms, axis=1), state=worst)

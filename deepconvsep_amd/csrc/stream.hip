// dcs_stream: separation of a signal that arrives in blocks (include/dcs.h has the contract, DESIGN.md section 4r the
// formulas and the state sizes).
//
// The whole-file paths run STFT -> tiles -> network -> fold -> iSTFT once, on a signal that is complete and resident.  Here
// the same values are produced as the samples come: every frame depends on N samples, every tile on tc frames, the fold of a
// frame on the tiles that cover it and an output sample on the N / hop frames that cover it, so a sample of the whole-file
// result is final tc hop + N samples after it went in.  A push appends samples to a ring, transforms the frames that became
// complete into a ring of magnitude / phase rows and hands out the tiles that became ready; the caller runs them through the
// network; a pull folds the masks of those tiles (and of the few before them, kept in a ring of p) over the frames no later
// tile can reach, inverts each of these frames into a ring of windowed time-domain frames and gathers the samples no later
// frame can reach.  All counts are host integers.  Every kernel is a pure function of ABSOLUTE sample, frame and tile indices
// (a ring slot is index mod ring length), nothing is accumulated across threads and no ring slot is read before the push or
// pull that needs it has written it: however the signal is cut into blocks, the same bits come out.
//
// A CHANNEL stream (dcs_stream_create_channels) carries C signal channels next to the down-mix the network sees: C + 1 rows of
// samples and magnitudes (the down-mix last), phases of the C channels.  The tiles come from the down-mix row, the fold
// computes acc_s once per (frame, bin) and multiplies it with every channel's magnitude, the inverse and the gather run per
// (channel, source).  The kernels are the same ones: a row / channel index from the grid selects the ring, and the mono
// stream is the case of one row that is its own down-mix.
//
// A SCORE stream (dcs_stream_create_score) feeds the score-informed graphs: the note table is converted and uploaded once, a push
// also writes the harmonic masks M_j of the frames it completed into a ring [ninst][rf][F] next to the magnitudes (one workgroup
// per frame, from the few note rows that can meet the push's frames), the tiles carry one channel M_j * (scale * mag) per
// instrument and the fold multiplies acc_s with the score-informed mixture formed from the two rings.  Everything else is the
// mono stream.
//
// A FOLLOWED score stream (dcs_stream_set_follow) has its score at nominal tempo: a push runs dcs_chroma's kernel on its new
// magnitude rows, sends the rows through the caller's follower (follow.hip) and paints audio frame t from score frame pos[t]
// with a second mask kernel that looks at the whole table.  A score stream that never arms it runs what it ran before.
//
// A STEREO stream (dcs_stream_create_stereo) feeds the stereo (ILD) graph, which sees the C channels themselves and answers per
// (source, channel): C rows of samples, magnitudes and phases and no down-mix, the tiles carry the channels of a frame side by
// side (the row layout dcs_model_forward_stereo reads), the ring of p holds every (source, channel) once and the fold forms the
// stereo trainer's mask per channel -- den over the sources of THAT channel plus 1e-13 -- and adds the trainer's constant to
// the estimate.  Append, frames, inverse and gather are the kernels above with C rows.
//
// The WIENER FILTER (dcs_stream_set_mwf, channel and stereo streams of two channels): a pull sends the rows it folded through the
// online filter of mwf_online.hip -- causal, its state one 2x2 matrix per (source, bin), its bits independent of how the frames
// reach it, so the rows may go in two pieces where they wrap in the rings -- into two buffers [C][S][ff][F], and the inverse
// reads magnitudes AND phases from there (its second instantiation).  A stream that never arms it runs what it ran before.
#include "dcs_internal.h"
#include "fft_frame.h"
#include "chanmask.h"

#include <math.h>

#include <algorithm>
#include <vector>

namespace {

constexpr int kMaxSources = 8;
constexpr int kMaxChannels = 8;                         // the range of dcs_mask_fold_apply

__device__ __forceinline__ int64_t ring_slot(int64_t i, int64_t len) { return i % len; }

// ------------------------------------------------------------------------------------------ push: samples into the ring
// row blockIdx.y of the caller's block into row blockIdx.y of the ring [rows][cap]
__global__ __launch_bounds__(kThreads) void stream_append_kernel(const float* __restrict__ audio, int64_t row_stride, int64_t n,
                                                                 int64_t p0, float* __restrict__ ring, int64_t cap) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) ring[blockIdx.y * cap + ring_slot(p0 + i, cap)] = audio[blockIdx.y * row_stride + i];
}

// ------------------------------------------------------------------------------------------ push: the frames that became complete
// Frame n = n0 + blockIdx.x covers samples [n hop - N/2, n hop + N/2); samples < 0 or >= lim (the samples pushed so far, the
// signal's length once it has ended) read as zero, as stft_norm pads.  The tail is stft_forward_kernel's, term for term.
// Row r = blockIdx.y of the sample ring goes to row r of the magnitude ring [rows][rf][F]; the first n_ph rows also keep their
// phase (ring [n_ph][rf][F]) and copy both to the caller (row r at + r out_ch_stride).
__global__ __launch_bounds__(kThreads) void stream_frames_kernel(
    const float* __restrict__ ring, int64_t cap, int64_t lim, int64_t n0, int64_t rf, float* __restrict__ mag_ring,
    float* __restrict__ phase_ring, int n_ph, float* __restrict__ mag_out, float* __restrict__ phase_out, int64_t out_ch_stride,
    int64_t ld, const float* __restrict__ win, const float2* __restrict__ tw, int N, int hop, int log2m, float sqrt_n, int tw_lds) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int M = N >> 1;
    const int tid = threadIdx.x;
    const int64_t n = n0 + blockIdx.x;
    const int64_t base = n * (int64_t)hop - M;
    const int r = blockIdx.y;
    const bool keep = r < n_ph;
    ring += r * cap;
    const float2* Z = render_frame<float, float2, false>(smem, win, tw, tw_lds, M, log2m, base, [&](int64_t q) -> float {
        return (q < 0 || q >= lim) ? 0.f : ring[ring_slot(q, cap)];
    });
    float* mrow = mag_ring + (r * rf + ring_slot(n, rf)) * (int64_t)(M + 1);
    float* prow = keep ? phase_ring + (r * rf + ring_slot(n, rf)) * (int64_t)(M + 1) : nullptr;
    float* mo = (mag_out && keep) ? mag_out + r * out_ch_stride + (int64_t)blockIdx.x * ld : nullptr;
    float* po = (phase_out && keep) ? phase_out + r * out_ch_stride + (int64_t)blockIdx.x * ld : nullptr;
    for (int k = tid; k <= M; k += kThreads) {
        const float2 zk = Z[k & (M - 1)];
        const float2 zm = Z[(M - k) & (M - 1)];
        // E = (zk + conj(zm))/2 ; O = -i (zk - conj(zm))/2 ; X = E + w^k O
        const float er = 0.5f * (zk.x + zm.x), ei = 0.5f * (zk.y - zm.y);
        const float orr = 0.5f * (zk.y + zm.y), oi = -0.5f * (zk.x - zm.x);
        const float2 w = tw[k];
        const float xr = er + (w.x * orr - w.y * oi);
        const float xi = ei + (w.x * oi + w.y * orr);
        const float ax = dcs_sqrt(xr * xr + xi * xi);
        const float mg = ax / sqrt_n, ph = dcs_atan2(xi, xr);
        mrow[k] = mg;
        if (prow) prow[k] = ph;
        if (mo) mo[k] = mg;
        if (po) po[k] = ph;
    }
    for (int k = M + 1 + tid; k < ld; k += kThreads) {   // row padding of the caller's copies
        if (mo) mo[k] = 0.f;
        if (po) po[k] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------ push: the tiles that became ready
// tiles[i][0][j][:] = scale * mag[(k0 + i) st + j][:], zero for rows >= T (the library tiler's last tiles, after the end)
__global__ __launch_bounds__(kThreads) void stream_tiles_kernel(const float* __restrict__ mag_ring, int64_t rf, int F, int tc,
                                                                int st, int64_t k0, int64_t T, float scale,
                                                                float* __restrict__ tiles) {
    const int64_t i = blockIdx.x / tc;
    const int j = (int)(blockIdx.x - i * tc);
    const int64_t t = (k0 + i) * st + j;
    float* dst = tiles + (i * tc + j) * (int64_t)F;
    if (t < T) {
        const float* src = mag_ring + ring_slot(t, rf) * (int64_t)F;
        for (int f = threadIdx.x; f < F; f += kThreads) dst[f] = scale * src[f];
    } else {
        for (int f = threadIdx.x; f < F; f += kThreads) dst[f] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------ push (stereo): the tiles that became ready
// tiles[i][j][c][:] = scale * mag[c][(k0 + i) st + j][:] for channel c = blockIdx.y of the magnitude ring [C][rf][F], rows of
// ldt = round_up(F, 4) floats: zero for rows >= T and for the columns F .. ldt - 1 (conv1's K axis runs over them)
__global__ __launch_bounds__(kThreads) void stream_stereo_tiles_kernel(const float* __restrict__ mag_ring, int64_t rf, int F,
                                                                       int ldt, int tc, int st, int64_t k0, int64_t T, float scale,
                                                                       float* __restrict__ tiles) {
    const int64_t i = blockIdx.x / tc;
    const int j = (int)(blockIdx.x - i * tc);
    const int c = blockIdx.y, C = gridDim.y;
    const int64_t t = (k0 + i) * st + j;
    float* dst = tiles + ((i * tc + j) * C + c) * (int64_t)ldt;
    if (t < T) {
        const float* src = mag_ring + (c * rf + ring_slot(t, rf)) * (int64_t)F;
        for (int f = threadIdx.x; f < ldt; f += kThreads) dst[f] = f < F ? scale * src[f] : 0.f;
    } else {
        for (int f = threadIdx.x; f < ldt; f += kThreads) dst[f] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------ push (score): the masks of the new frames
// The converted note table: one row of kRowHead + 2 npairs int32 per counting note row -- instrument, first frame, end frame, a
// pad, then the bin pairs (f0, f1), an empty pair where the slot does not count -- sorted by first frame.
constexpr int kRowHead = 4;
constexpr int kMaskChunk = 4096;                        // bins per pass: 16 KB of LDS whatever the frame size

struct ScoreVals {                                       // DCS_SCORE_NORM_MAX: the two values an instrument's mask takes
    float lo[kMaxChannels], hi[kMaxChannels];
};

// Frame t = n0 + blockIdx.x: M_j[t][:] for every instrument into slot t mod rf of the ring [ninst][rf][F].  One LDS word per bin,
// bit j = on_j: the lanes walk the (row, pair) items of the candidate rows [r_lo, r_hi) -- every row that covers a frame of this
// push is among them -- and paint the bands of those that cover t with atomicOr (order-independent, so the bits are
// deterministic); after the barrier each lane turns its bins into the ninst values.  normalise = DCS_SCORE_NORM_SUM:
// score_sumnorm_kernel's expressions.
__global__ __launch_bounds__(kThreads) void stream_masks_kernel(const int* __restrict__ table, int npairs, int r_lo, int r_hi,
                                                                int64_t n0, int64_t rf, int F, int ninst, int normalise,
                                                                ScoreVals vals, float* __restrict__ mask_ring) {
    __shared__ unsigned bits[kMaskChunk];
    const int tid = threadIdx.x;
    const int64_t t = n0 + blockIdx.x;
    const int64_t slot = ring_slot(t, rf);
    const int W = kRowHead + 2 * npairs;
    const int items = (r_hi - r_lo) * npairs;
    for (int c0 = 0; c0 < F; c0 += kMaskChunk) {
        const int c1 = c0 + kMaskChunk < F ? c0 + kMaskChunk : F;
        for (int i = tid; i < c1 - c0; i += kThreads) bits[i] = 0u;
        __syncthreads();
        for (int it = tid; it < items; it += kThreads) {
            const int* row = table + (int64_t)(r_lo + it / npairs) * W;
            if (row[1] <= t && t < row[2]) {
                const int k = it % npairs;
                const int f0 = row[kRowHead + 2 * k] > c0 ? row[kRowHead + 2 * k] : c0;
                const int f1 = row[kRowHead + 2 * k + 1] < c1 ? row[kRowHead + 2 * k + 1] : c1;
                const unsigned bit = 1u << row[0];
                for (int f = f0; f < f1; ++f) atomicOr(&bits[f - c0], bit);
            }
        }
        __syncthreads();
        for (int i = tid; i < c1 - c0; i += kThreads) {
            const unsigned on = bits[i];
            float* dst = mask_ring + slot * (int64_t)F + c0 + i;
            if (normalise == DCS_SCORE_NORM_SUM) {
                float total = 0.f;
                for (int j = 0; j < ninst; ++j) {
                    const float v = ((on >> j) & 1u) ? 1.0f : 1e-18f;
                    total = j == 0 ? v : __fadd_rn(total, v);
                }
                for (int j = 0; j < ninst; ++j)
                    dst[j * rf * (int64_t)F] = __fdiv_rn(((on >> j) & 1u) ? 1.0f : 1e-18f, total);
            } else {
#pragma unroll
                for (int j = 0; j < kMaxChannels; ++j)
                    if (j < ninst) dst[j * rf * (int64_t)F] = ((on >> j) & 1u) ? vals.hi[j] : vals.lo[j];
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ push (followed score): the masks of the new frames
// stream_masks_kernel for a stream whose score is at nominal tempo (dcs_stream_set_follow): audio frame t = n0 + blockIdx.x is
// painted from SCORE frame pos[blockIdx.x], the position the follower gave it, into slot t mod rf.  The host does not know
// which rows a push can meet, so the lanes walk all n_rows rows of the table (a few hundred); the rest is that kernel's.
__global__ __launch_bounds__(kThreads) void stream_follow_masks_kernel(const int* __restrict__ table, int npairs, int n_rows,
                                                                       const int32_t* __restrict__ pos, int64_t n0, int64_t rf,
                                                                       int F, int ninst, int normalise, ScoreVals vals,
                                                                       float* __restrict__ mask_ring) {
    __shared__ unsigned bits[kMaskChunk];
    const int tid = threadIdx.x;
    const int64_t slot = ring_slot(n0 + blockIdx.x, rf);
    const int t = pos[blockIdx.x];
    const int W = kRowHead + 2 * npairs;
    const int items = n_rows * npairs;
    for (int c0 = 0; c0 < F; c0 += kMaskChunk) {
        const int c1 = c0 + kMaskChunk < F ? c0 + kMaskChunk : F;
        for (int i = tid; i < c1 - c0; i += kThreads) bits[i] = 0u;
        __syncthreads();
        for (int it = tid; it < items; it += kThreads) {
            const int* row = table + (int64_t)(it / npairs) * W;
            if (row[1] <= t && t < row[2]) {
                const int k = it % npairs;
                const int f0 = row[kRowHead + 2 * k] > c0 ? row[kRowHead + 2 * k] : c0;
                const int f1 = row[kRowHead + 2 * k + 1] < c1 ? row[kRowHead + 2 * k + 1] : c1;
                const unsigned bit = 1u << row[0];
                for (int f = f0; f < f1; ++f) atomicOr(&bits[f - c0], bit);
            }
        }
        __syncthreads();
        for (int i = tid; i < c1 - c0; i += kThreads) {
            const unsigned on = bits[i];
            float* dst = mask_ring + slot * (int64_t)F + c0 + i;
            if (normalise == DCS_SCORE_NORM_SUM) {
                float total = 0.f;
                for (int j = 0; j < ninst; ++j) {
                    const float v = ((on >> j) & 1u) ? 1.0f : 1e-18f;
                    total = j == 0 ? v : __fadd_rn(total, v);
                }
                for (int j = 0; j < ninst; ++j)
                    dst[j * rf * (int64_t)F] = __fdiv_rn(((on >> j) & 1u) ? 1.0f : 1e-18f, total);
            } else {
#pragma unroll
                for (int j = 0; j < kMaxChannels; ++j)
                    if (j < ninst) dst[j * rf * (int64_t)F] = ((on >> j) & 1u) ? vals.hi[j] : vals.lo[j];
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------ push (score): the tiles that became ready
// tiles[i][j][r][:] = M_j[t][:] * (scale * mag[t][:]), t = (k0 + i) st + r, zero for rows >= T: score_floor_kernel's product on
// the tiler's rows.  Workgroup blockIdx.x = (i ninst + j) tc + r.
__global__ __launch_bounds__(kThreads) void stream_score_tiles_kernel(const float* __restrict__ mag_ring,
                                                                      const float* __restrict__ mask_ring, int64_t rf, int F, int tc,
                                                                      int st, int ninst, int64_t k0, int64_t T, float scale,
                                                                      float* __restrict__ tiles) {
    const int64_t b = blockIdx.x / tc;
    const int r = (int)(blockIdx.x - b * tc);
    const int64_t i = b / ninst;
    const int j = (int)(b - i * ninst);
    const int64_t t = (k0 + i) * st + r;
    float* dst = tiles + (int64_t)blockIdx.x * F;
    if (t < T) {
        const float* src = mag_ring + ring_slot(t, rf) * (int64_t)F;
        const float* msk = mask_ring + (j * rf + ring_slot(t, rf)) * (int64_t)F;
        for (int f = threadIdx.x; f < F; f += kThreads) dst[f] = __fmul_rn(msk[f], __fmul_rn(scale, src[f]));
    } else {
        for (int f = threadIdx.x; f < F; f += kThreads) dst[f] = 0.f;
    }
}

// ------------------------------------------------------------------------------------------ pull: p of the new tiles into its ring
__global__ __launch_bounds__(kThreads) void stream_keep_p_kernel(const float* __restrict__ p, int64_t p_src_stride, int64_t k0,
                                                                 int64_t tile_elems, float* __restrict__ p_ring, int64_t rp) {
    const int64_t i = blockIdx.x;                       // tile of this pull
    const int s = blockIdx.z;
    const float* src = p + s * p_src_stride + i * tile_elems;
    float* dst = p_ring + ((int64_t)s * rp + ring_slot(k0 + i, rp)) * tile_elems;
    for (int64_t e = (int64_t)blockIdx.y * kThreads + threadIdx.x; e < tile_elems; e += (int64_t)gridDim.y * kThreads)
        dst[e] = src[e];
}

// ------------------------------------------------------------------------------------------ pull: fold + apply
// The per-frame definition of dcs_mask_fold_apply (mask_fold_apply_kernel<0, 0>, expression for expression) with absolute
// t = t0 + blockIdx.x and k, p and the magnitudes read from their rings.  n = the tiles that exist so far: mid-stream every
// frame folded has its owner below n, so the clamp acts only after the end.  est[c][s][blockIdx.x][f] = acc_s * mag[c][t][f]
// for the C channels of the magnitude ring: acc_s is computed once.
// MIX: kMixMag the magnitude itself (the mono and channel streams); a score stream (C = 1) multiplies with the score-informed
// mixture instead, formed from the mask ring [ninst][rf][F]: kMixCh0 M_0 * mag, kMixSum ((x_0 + x_1) + ...) with x_j = M_j * mag.
enum { kMixMag = 0, kMixCh0 = 1, kMixSum = 2 };
template <int MIX>
__global__ __launch_bounds__(kThreads) void stream_fold_kernel(
    const float* __restrict__ p_ring, int64_t rp, int64_t n, int S, int tc, int ov, int F, int mode,
    const float* __restrict__ rise, const float* __restrict__ mag_ring, int64_t rf, int C, int64_t t0, float* __restrict__ est,
    int64_t est_src_stride, float* __restrict__ est_out, int64_t out_ch_stride, int64_t out_src_stride, int64_t ld,
    const float* __restrict__ mask_ring, int ninst) {
    const int f = blockIdx.y * kThreads + threadIdx.x;
    if (f >= F) return;
    const int64_t t = t0 + blockIdx.x;
    const int st = tc - ov;
    const int64_t tile_elems = (int64_t)tc * F, src_stride = rp * tile_elems;
    int64_t k0 = (t < ov) ? 0 : (t - ov) / st;
    if (k0 > n - 1) k0 = n - 1;
    const int64_t j0 = (n > 0) ? t - k0 * st : tc;

    float acc[kMaxSources];
#pragma unroll
    for (int s = 0; s < kMaxSources; ++s) acc[s] = 0.f;
    if (j0 < tc) {                                       // else: past the last tile, the zeros of util.py:313
        for (int64_t k = k0; k < n && k * st <= t; ++k) {
            const int j = (int)(t - k * st);
            const int64_t r = ring_slot(k, rp) * tile_elems + (int64_t)j * F + f;
            float p[kMaxSources];
#pragma unroll
            for (int s = 0; s < kMaxSources; ++s) p[s] = s < S ? p_ring[s * src_stride + r] : 0.f;
            soft_masks<kMaxSources>(p, S, mode);
            if (k == k0) {
#pragma unroll
                for (int s = 0; s < kMaxSources; ++s) acc[s] = p[s];
            } else {
                const float down = rise[ov - 1 - j], up = rise[j];
#pragma unroll
                for (int s = 0; s < kMaxSources; ++s) acc[s] = fmaf(down, acc[s], __fmul_rn(up, p[s]));   // one explicit form: see overlap_add_kernel
            }
        }
    }
    for (int c = 0; c < C; ++c) {
        float mg = mag_ring[(c * rf + ring_slot(t, rf)) * (int64_t)F + f];
        if (MIX != kMixMag) {
            const float m = mg;
            const float* mk_row = mask_ring + ring_slot(t, rf) * (int64_t)F + f;
            mg = __fmul_rn(mk_row[0], m);
            if (MIX == kMixSum)
                for (int j = 1; j < ninst; ++j) mg = __fadd_rn(mg, __fmul_rn(mk_row[j * rf * (int64_t)F], m));
        }
#pragma unroll
        for (int s = 0; s < kMaxSources; ++s)
            if (s < S) {
                const float e = __fmul_rn(acc[s], mg);
                est[(c * S + s) * est_src_stride + (int64_t)blockIdx.x * F + f] = e;
                if (est_out) est_out[c * out_ch_stride + s * out_src_stride + (int64_t)blockIdx.x * ld + f] = e;
            }
    }
}

// ------------------------------------------------------------------------------------------ pull (stereo): p of the new tiles into its ring
// Row blockIdx.x = i tc + j of (source blockIdx.z, channel blockIdx.y): F floats from the caller's strides into the compact
// ring [S][C][rp][tc][F].
__global__ __launch_bounds__(kThreads) void stream_keep_p_stereo_kernel(const float* __restrict__ p, int64_t p_src_stride,
                                                                        int64_t p_ch_stride, int64_t p_ld, int64_t k0, int tc, int F,
                                                                        float* __restrict__ p_ring, int64_t rp) {
    const int64_t i = blockIdx.x / tc;
    const int j = (int)(blockIdx.x - i * tc);
    const int c = blockIdx.y, C = gridDim.y, s = blockIdx.z;
    const float* src = p + s * p_src_stride + c * p_ch_stride + (int64_t)blockIdx.x * p_ld;
    float* dst = p_ring + ((((int64_t)s * C + c) * rp + ring_slot(k0 + i, rp)) * tc + j) * (int64_t)F;
    for (int f = threadIdx.x; f < F; f += kThreads) dst[f] = src[f];
}

// ------------------------------------------------------------------------------------------ pull (stereo): fold + apply
// stream_fold_kernel's walk over the covering tiles for channel c = blockIdx.z of gridDim.z, with the stereo trainer's mask
// (dsd.hip MODE 3: den = ((p_0c + p_1c) + ...) + 1e-13f, m_s = p_sc / den) from the ring [S][C][rp][tc][F], and
// est[c][s][blockIdx.x][f] = acc_sc * mag[c][t][f] + c0: product and sum each rounded once.  Rows past the last tile are zeros
// without c0.
__global__ __launch_bounds__(kThreads) void stream_fold_stereo_kernel(
    const float* __restrict__ p_ring, int64_t rp, int64_t n, int S, int tc, int ov, int F, const float* __restrict__ rise,
    const float* __restrict__ mag_ring, int64_t rf, int64_t t0, float c0, float* __restrict__ est, int64_t est_src_stride,
    float* __restrict__ est_out, int64_t out_ch_stride, int64_t out_src_stride, int64_t ld) {
    const int f = blockIdx.y * kThreads + threadIdx.x;
    if (f >= F) return;
    const int c = blockIdx.z, C = gridDim.z;
    const int64_t t = t0 + blockIdx.x;
    const int st = tc - ov;
    const int64_t tile_elems = (int64_t)tc * F, src_stride = C * rp * tile_elems;
    const float* pc = p_ring + c * rp * tile_elems;
    const float eps_r = 1e-13f;
    int64_t k0 = (t < ov) ? 0 : (t - ov) / st;
    if (k0 > n - 1) k0 = n - 1;
    const int64_t j0 = (n > 0) ? t - k0 * st : tc;
    const bool covered = j0 < tc;

    float acc[kMaxSources];
#pragma unroll
    for (int s = 0; s < kMaxSources; ++s) acc[s] = 0.f;
    if (covered) {
        for (int64_t k = k0; k < n && k * st <= t; ++k) {
            const int j = (int)(t - k * st);
            const int64_t r = ring_slot(k, rp) * tile_elems + (int64_t)j * F + f;
            float p[kMaxSources];
            float den = 0.f;
#pragma unroll
            for (int s = 0; s < kMaxSources; ++s) {
                p[s] = s < S ? pc[s * src_stride + r] : 0.f;
                if (s < S) den = s == 0 ? p[s] : __fadd_rn(den, p[s]);
            }
            den = __fadd_rn(den, eps_r);
#pragma unroll
            for (int s = 0; s < kMaxSources; ++s) p[s] = __fdiv_rn(p[s], den);
            if (k == k0) {
#pragma unroll
                for (int s = 0; s < kMaxSources; ++s) acc[s] = p[s];
            } else {
                const float down = rise[ov - 1 - j], up = rise[j];
#pragma unroll
                for (int s = 0; s < kMaxSources; ++s) acc[s] = fmaf(down, acc[s], __fmul_rn(up, p[s]));   // as stream_fold_kernel
            }
        }
    }
    const float mg = mag_ring[(c * rf + ring_slot(t, rf)) * (int64_t)F + f];
#pragma unroll
    for (int s = 0; s < kMaxSources; ++s)
        if (s < S) {
            const float e = covered ? __fadd_rn(__fmul_rn(acc[s], mg), c0) : 0.f;
            est[(c * S + s) * est_src_stride + (int64_t)blockIdx.x * F + f] = e;
            if (est_out) est_out[c * out_ch_stride + s * out_src_stride + (int64_t)blockIdx.x * ld + f] = e;
        }
}

// ------------------------------------------------------------------------------------------ pull: one frame of one source back to time
// y_n = w * irfft(est[c][s][n] sqrt(N) exp(j phase[c][n])) into slot n mod rt of the time-frame ring [rt][C][S][N]: the packed real-inverse
// pre-processing, transform and window product of istft_fused_kernel (fft.hip), term for term, for ONE frame -- the sum over
// the frames that cover a sample is stream_gather_kernel's.  Workgroup (blockIdx.x, blockIdx.y, blockIdx.z) = (frame t0 + x,
// source y, channel z of gridDim.z).  OWN_PHASE (a stream with the Wiener filter armed): `phase_ring` is the filter's phase buffer, a
// row per (channel, source, frame of the pull) laid out as est, instead of the ring's row per (channel, frame).
template <bool OWN_PHASE>
__global__ __launch_bounds__(kThreads) void stream_inverse_kernel(
    const float* __restrict__ est, int64_t est_src_stride, const float* __restrict__ phase_ring, int64_t rf, int64_t t0,
    float* __restrict__ tf_ring, int64_t rt, int S, const float* __restrict__ win, const float2* __restrict__ tw, int N, int log2m,
    float sqrt_n, int tw_lds) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int M = N >> 1;
    const int tid = threadIdx.x;
    const int s = blockIdx.y, c = blockIdx.z, C = gridDim.z;
    const int64_t n = t0 + blockIdx.x;
    float2* buf0 = reinterpret_cast<float2*>(smem);
    float2* buf1 = buf0 + M;  // M+1 entries: holds X first, then serves as the FFT ping-pong buffer
    float2* X = buf1;
    if (tw_lds) {
        float2* twl = buf1 + (M + 1);
        for (int k = tid; k <= M; k += kThreads) twl[k] = tw[k];
        tw = twl;
    }
    const float* mrow = est + (c * S + s) * est_src_stride + (int64_t)blockIdx.x * (M + 1);
    const float* prow = OWN_PHASE ? phase_ring + (c * S + s) * est_src_stride + (int64_t)blockIdx.x * (M + 1)
                                  : phase_ring + (c * rf + ring_slot(n, rf)) * (int64_t)(M + 1);
    for (int k = tid; k <= M; k += kThreads) {
        const float a = mrow[k] * sqrt_n;
        float sn, cs;
        dcs_sincos(prow[k], &sn, &cs);
        float2 x = mk<float2, float>(a * cs, a * sn);
        if (k == 0 || k == M) x.y = 0.f;
        X[k] = x;
    }
    __syncthreads();
    for (int k = tid; k < M; k += kThreads) {
        const float2 xk = X[k];
        const float2 xm = X[M - k];
        // E = (xk + conj(xm))/2 ; D = (xk - conj(xm))/2 ; O = D * conj(w^k) ; Z = E + i O
        const float er = 0.5f * (xk.x + xm.x), ei = 0.5f * (xk.y - xm.y);
        const float dr = 0.5f * (xk.x - xm.x), di = 0.5f * (xk.y + xm.y);
        const float2 w = tw[k];
        const float orr = dr * w.x + di * w.y;
        const float oi = di * w.x - dr * w.y;
        buf0[k] = mk<float2, float>(er - oi, ei + orr);
    }
    __syncthreads();
    const float2* z = fft_lds<float, float2, +1>(buf0, buf1, tw, M, log2m);
    const float inv_m = 1.f / (float)M;
    const float2* w2 = reinterpret_cast<const float2*>(win);
    float2* dst = reinterpret_cast<float2*>(tf_ring + ((ring_slot(n, rt) * C + c) * S + s) * (int64_t)N);
    for (int m = tid; m < M; m += kThreads) {
        const float2 v = z[m];
        const float2 w = w2[m];
        dst[m] = mk<float2, float>((v.x * inv_m) * w.x, (v.y * inv_m) * w.y);
    }
}

// ------------------------------------------------------------------------------------------ pull: the samples that became final
// out[c][s][q - q0] (c = blockIdx.z of gridDim.z channels) = (y_lo[..] + y_{lo+1}[..] + ... in increasing n) / norm over the frames n < T with n hop <= q + N/2 < n hop + N,
// norm = the sum of w^2 over the same frames, 0 replaced by 1 (istft_norm).  T = the frames folded so far (every frame there is,
// once the signal has ended): mid-stream a sample is emitted only when all its frames are below it.
__global__ __launch_bounds__(kThreads) void stream_gather_kernel(const float* __restrict__ tf_ring, int64_t rt, int S, int N,
                                                                 int hop, int64_t T, const float* __restrict__ wsq, int64_t q0,
                                                                 int64_t n_out, float* __restrict__ pcm, int64_t pcm_ch_stride,
                                                                 int64_t pcm_stride) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_out) return;
    const int s = blockIdx.y, c = blockIdx.z, C = gridDim.z;
    const int64_t p = q0 + i + (N >> 1);                // position in the padded signal
    int64_t n_hi = p / hop;
    if (n_hi > T - 1) n_hi = T - 1;
    const int64_t n_lo = (p < N) ? 0 : (p - N) / hop + 1;
    float acc = 0.f, norm = 0.f;
    for (int64_t n = n_lo; n <= n_hi; ++n) {
        const int64_t off = p - n * hop;
        acc += tf_ring[((ring_slot(n, rt) * C + c) * S + s) * (int64_t)N + off];
        norm += wsq[off];
    }
    if (norm == 0.f) norm = 1.f;
    pcm[c * pcm_ch_stride + s * pcm_stride + i] = acc / norm;
}

// ------------------------------------------------------------------------------------------ the filtered rows of the last pull
// row blockIdx.x of (channel c, source s) = blockIdx.z of the filter's two buffers [C][S][ff][F] to the caller
__global__ __launch_bounds__(kThreads) void stream_mwf_copy_kernel(const float* __restrict__ fmag, const float* __restrict__ fphase,
                                                                   int64_t buf_src_stride, int S, int F, float* __restrict__ mag,
                                                                   float* __restrict__ phase, int64_t ch_stride, int64_t src_stride,
                                                                   int64_t ld) {
    const int f = blockIdx.y * kThreads + threadIdx.x;
    if (f >= F) return;
    const int c = blockIdx.z / S, s = blockIdx.z % S;
    const int64_t i = (int64_t)blockIdx.z * buf_src_stride + (int64_t)blockIdx.x * F + f;
    const int64_t o = c * ch_stride + s * src_stride + (int64_t)blockIdx.x * ld + f;
    mag[o] = fmag[i];
    phase[o] = fphase[i];
}

}  // namespace

// ------------------------------------------------------------------------------------------ the handle
struct dcs_stream {
    dcs_stft* plan = nullptr;
    dcs_ctx* ctx = nullptr;
    int S = 0, tc = 0, ov = 0, st = 0, tiler = 0, eps_mode = 0, N = 0, hop = 0, F = 0;
    // C: the signal channels of a channel stream, 0 for the mono stream; rows of samples and magnitudes (the down-mix last);
    // nch: the rows that keep their phase and come back as stems (the mono stream's one row is both)
    int C = 0, rows = 1, nch = 1;
    bool stereo = false;       // a stereo stream: C rows, no down-mix, p per (source, channel)
    float scale = 1.f, c0 = 0.f;   // c0: the stereo trainer's constant on the unscaled magnitudes, 1e-13f / scale
    int64_t max_push = 0;
    // ring lengths: samples; frames a push can complete, the end included; tiles it can return; frame rows; tiles of p; frames
    // a pull can fold; time-domain frames
    int64_t cap = 0, fp = 0, max_tiles = 0, rf = 0, rp = 0, ff = 0, rt = 0;
    float *samples = nullptr, *mag = nullptr, *phase = nullptr, *p = nullptr, *est = nullptr, *tf = nullptr, *rise = nullptr;
    int64_t bytes = 0;
    // host counts (the table of include/dcs.h): samples pushed, frames transformed, tiles handed out, frames folded, samples
    // emitted; T and L are known once the signal has ended
    int64_t P = 0, A = 0, K = 0, Tf = 0, E = 0, T = 0, L = 0;
    int64_t pending = 0;       // tiles of the last push, which the next pull must bring p for
    bool want_pull = false, ended = false;
    // a score stream (ninst > 0): the converted table on the device, the ring of mask rows, and on the host the first frames of
    // the sorted rows with the running maximum of their end frames (the candidate range of a push)
    int ninst = 0, npairs = 0, normalise = 0, mixture = 0;
    int* table = nullptr;
    float* masks = nullptr;
    ScoreVals vals = {};
    std::vector<int> row_t0, row_end_max;
    // the online Wiener filter (dcs_stream_set_mwf; null: off), its outputs [C][S][ff][F] and the rows the last pull filtered
    dcs_mwf_online* mwf = nullptr;
    float *fmag = nullptr, *fphase = nullptr;
    int64_t mwf_bytes = 0, mwf_rows = 0;
    // a followed score stream (dcs_stream_set_follow; null: off): the caller's follower, the class table of the chroma kernel,
    // chroma rows and positions of one push's frames [fp], and the frames the last push followed
    dcs_follow* follow = nullptr;
    int8_t* follow_cls = nullptr;
    float* follow_chroma = nullptr;
    int32_t* follow_pos = nullptr;
    float follow_floor = 0.f;
    int64_t follow_bytes = 0, follow_rows = 0;
    // a push failed (a HIP error) after the follower had taken its frames: follower and stream disagree until dcs_stream_reset
    bool follow_stale = false;
};

namespace {

// the score of dcs_stream_create_score as the caller gave it
struct ScoreSpec {
    const double* notes;
    int ninst, n_notes, width, normalise, mixture;
};

struct ScoreRow {
    int inst, t0, t1;
    std::vector<int> pairs;                              // npairs x (f0, f1)
};

// dcs_score_masks_scaled's reading of the table with start = 0 and stop = +inf: the counting rows sorted by first frame, and
// the two values of DCS_SCORE_NORM_MAX per instrument
int score_convert(const char* who, const ScoreSpec& sc, int F, std::vector<ScoreRow>* rows, ScoreVals* vals) {
    const int npairs = (sc.width - 3) / 2;
    const double t_max = 2147483647.0;
    for (int j = 0; j < sc.ninst; ++j) {
        bool any = false;
        for (int p = 0; p < sc.n_notes; ++p) {
            const double* n = sc.notes + ((size_t)j * sc.n_notes + p) * sc.width;
            const double n0 = n[0], n1 = n[1], midi = n[2];
            const double a = n0 > 0.0 ? n0 : 0.0, b = n1;
            if (!(midi > 0) || !((b - a > 0 ? b - a : 0) > 0)) continue;
            ScoreRow r;
            r.inst = j;
            r.t0 = (int)(a < t_max ? a : t_max);
            r.t1 = (int)(b < t_max ? b : t_max);
            r.pairs.assign((size_t)2 * npairs, 0);
            bool painted = false;
            for (int k = 0; k < npairs; ++k) {
                const double fs = n[3 + 2 * k], fe = n[4 + 2 * k];
                if (!(fe > 0)) continue;
                if (!(fs > -1.0) || !(fe < (double)F + 1.0))             // the casts below truncate, as the whole-file call's
                    DCS_FAIL(DCS_ESHAPE, "%s: bin range [%g, %g) outside 0..%d", who, fs, fe, F);
                const int f0 = (int)fs, f1 = (int)fe;
                if (f0 < 0 || f1 > F) DCS_FAIL(DCS_ESHAPE, "%s: bin range [%d, %d) outside 0..%d", who, f0, f1, F);
                if (r.t1 > r.t0 && f1 > f0) {
                    r.pairs[2 * k] = f0;
                    r.pairs[2 * k + 1] = f1;
                    painted = true;
                }
            }
            if (painted) {
                rows->push_back(r);
                any = true;
            }
        }
        // filtered[j] / np.max(filtered[j]) in float32, as dcs_score_masks_scaled forms the two values
        const float floor_v = 1e-18f, maxv = any ? 1.0f : floor_v;
        vals->lo[j] = floor_v / maxv;
        vals->hi[j] = 1.0f / maxv;
    }
    std::stable_sort(rows->begin(), rows->end(), [](const ScoreRow& x, const ScoreRow& y) { return x.t0 < y.t0; });
    return DCS_OK;
}

// C = 0: the mono stream; sc != nullptr: a score stream; stereo: C rows and no down-mix
int stream_create(const char* who, dcs_stft* plan, int S, int C, int time_context, int overlap, int tiler, int eps_mode,
                  float scale, const double* rise_h, int64_t max_push, dcs_stream** out, const ScoreSpec* sc = nullptr,
                  bool stereo = false) {
    if (!plan || !rise_h || !out) DCS_FAIL(DCS_EINVAL, "%s: null argument", who);
    if (S < 1 || S > kMaxSources) DCS_FAIL(DCS_EINVAL, "%s: %d sources (1 .. %d)", who, S, kMaxSources);
    if (overlap < 1 || overlap >= time_context) DCS_FAIL(DCS_EINVAL, "%s: overlap %d not in [1, %d)", who, overlap, time_context);
    if (tiler != DCS_TILER_SCRIPT && tiler != DCS_TILER_LIBRARY) DCS_FAIL(DCS_EINVAL, "%s: bad tiler", who);
    if (eps_mode != DCS_EPS_A && eps_mode != DCS_EPS_B) DCS_FAIL(DCS_EINVAL, "%s: bad eps_mode", who);
    if (max_push < 1 || max_push > (1LL << 30)) DCS_FAIL(DCS_EINVAL, "%s: max_push %lld not in [1, 2^30]", who, (long long)max_push);
    const int N = plan->frame, hop = plan->hop, H = N / 2;
    if (hop > H) DCS_FAIL(DCS_EINVAL, "%s: hopSize %d above frameSize / 2 = %d", who, hop, H);
    if (N % hop) DCS_FAIL(DCS_EUNSUPPORTED, "%s: hopSize %d does not divide frameSize %d", who, hop, N);
    if (N < 64) DCS_FAIL(DCS_EUNSUPPORTED, "%s: frameSize %d below 64", who, N);
    std::vector<ScoreRow> score_rows;
    ScoreVals vals = {};
    int64_t table_rows = 0;
    if (sc) {
        if (!sc->notes) DCS_FAIL(DCS_EINVAL, "%s: null argument", who);
        if (sc->ninst < 1 || sc->ninst > kMaxChannels)
            DCS_FAIL(DCS_EINVAL, "%s: %d instruments (1 .. %d)", who, sc->ninst, kMaxChannels);
        if (sc->n_notes < 0 || sc->width < 5 || ((sc->width - 3) & 1))
            DCS_FAIL(DCS_EINVAL, "%s: bad table shape (notes %d, width %d)", who, sc->n_notes, sc->width);
        if (sc->normalise != DCS_SCORE_NORM_MAX && sc->normalise != DCS_SCORE_NORM_SUM)
            DCS_FAIL(DCS_EINVAL, "%s: normalise %d", who, sc->normalise);
        if (sc->mixture != DCS_MIX_CH0 && sc->mixture != DCS_MIX_SUM) DCS_FAIL(DCS_EINVAL, "%s: mixture %d", who, sc->mixture);
        table_rows = (int64_t)sc->ninst * sc->n_notes;
        if (table_rows * ((sc->width - 3) / 2) > (1LL << 30))
            DCS_FAIL(DCS_EUNSUPPORTED, "%s: a table of %lld rows x %d pairs", who, (long long)table_rows, (sc->width - 3) / 2);
        DCS_CHECK(score_convert(who, *sc, H + 1, &score_rows, &vals));
        if (table_rows < 1) table_rows = 1;              // the block exists whatever the table holds
    }
    DCS_ON_DEVICE(plan->ctx->device);

    dcs_stream* s = new dcs_stream();
    s->plan = plan;
    s->ctx = plan->ctx;
    s->S = S; s->tc = time_context; s->ov = overlap; s->st = time_context - overlap;
    s->tiler = tiler; s->eps_mode = eps_mode; s->scale = scale;
    s->C = C; s->rows = stereo ? C : (C ? C + 1 : 1); s->nch = C ? C : 1;
    s->stereo = stereo;
    if (stereo) s->c0 = 1e-13f / scale;
    s->N = N; s->hop = hop; s->F = H + 1; s->max_push = max_push;
    s->cap = N + max_push;                                            // a new frame reaches back less than N samples before the push
    s->fp = (max_push + H + hop - 1) / hop + 3;                       // T - A <= (L - P + N/2) / hop + 3 at the end; fewer mid-stream
    s->max_tiles = (s->fp + s->st - 1) / s->st + 2;
    s->rf = time_context + s->fp;                                     // A - Tf < tc after a pull, plus one push
    s->rp = (time_context + s->st - 1) / s->st + s->max_tiles;        // the tiles that reach the oldest unfolded frame, plus one push
    s->ff = time_context + s->fp;                                     // T - Tf of a pull
    s->rt = N / hop + s->ff;                                          // the frames that reach the oldest sample not yet emitted, plus one pull

    const int64_t F = s->F;
    struct { float** ptr; int64_t elems; const char* name; } blocks[] = {
        {&s->samples, s->rows * s->cap, "stream.samples"},
        {&s->mag, s->rows * s->rf * F, "stream.mag"},
        {&s->phase, s->nch * s->rf * F, "stream.phase"},
        {&s->p, (int64_t)S * (stereo ? C : 1) * s->rp * time_context * F, "stream.p"},
        {&s->est, (int64_t)s->nch * S * s->ff * F, "stream.est"},
        {&s->tf, s->rt * s->nch * S * N, "stream.tf"},
        {&s->rise, overlap, "stream.rise"},
    };
    for (auto& b : blocks) {
        const hipError_t e = dcs_dev_alloc((void**)b.ptr, (size_t)b.elems * sizeof(float), b.name);
        if (e != hipSuccess) {
            dcs_set_error("%s: %lld bytes for %s: %s", who, (long long)(b.elems * sizeof(float)), b.name, hipGetErrorString(e));
            dcs_stream_destroy(s);
            return e == hipErrorOutOfMemory ? DCS_ENOMEM : DCS_EHIP;
        }
        s->bytes += b.elems * (int64_t)sizeof(float);
    }
    if (sc) {
        s->ninst = sc->ninst; s->npairs = (sc->width - 3) / 2; s->normalise = sc->normalise; s->mixture = sc->mixture;
        s->vals = vals;
        const int W = kRowHead + 2 * s->npairs;
        // the table at its capacity (every row of the caller's table), so that the size does not depend on the notes
        struct { void** ptr; int64_t bytes; const char* name; } extra[] = {
            {(void**)&s->masks, (int64_t)s->ninst * s->rf * F * (int64_t)sizeof(float), "stream.masks"},
            {(void**)&s->table, table_rows * W * (int64_t)sizeof(int), "stream.score"},
        };
        for (auto& b : extra) {
            const hipError_t e = dcs_dev_alloc(b.ptr, (size_t)b.bytes, b.name);
            if (e != hipSuccess) {
                dcs_set_error("%s: %lld bytes for %s: %s", who, (long long)b.bytes, b.name, hipGetErrorString(e));
                dcs_stream_destroy(s);
                return e == hipErrorOutOfMemory ? DCS_ENOMEM : DCS_EHIP;
            }
            s->bytes += b.bytes;
        }
        std::vector<int> flat(score_rows.size() * (size_t)W, 0);
        int end_max = 0;
        for (size_t r = 0; r < score_rows.size(); ++r) {
            const ScoreRow& row = score_rows[r];
            int* dst = flat.data() + r * (size_t)W;
            dst[0] = row.inst; dst[1] = row.t0; dst[2] = row.t1;
            std::copy(row.pairs.begin(), row.pairs.end(), dst + kRowHead);
            end_max = row.t1 > end_max ? row.t1 : end_max;
            s->row_t0.push_back(row.t0);
            s->row_end_max.push_back(end_max);
        }
        if (!flat.empty() && hipMemcpy(s->table, flat.data(), flat.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
            dcs_stream_destroy(s);
            DCS_FAIL(DCS_EHIP, "%s: uploading the note table failed", who);
        }
    }
    std::vector<float> rise((size_t)overlap);
    for (int i = 0; i < overlap; ++i) rise[i] = (float)rise_h[i];
    if (hipMemcpy(s->rise, rise.data(), rise.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        dcs_stream_destroy(s);
        DCS_FAIL(DCS_EHIP, "%s: uploading the cross-fade ramp failed", who);
    }
    *out = s;
    return DCS_OK;
}

}  // namespace

extern "C" int dcs_stream_create(dcs_stft* plan, int S, int time_context, int overlap, int tiler, int eps_mode, float scale,
                                 const double* rise_h, int64_t max_push, dcs_stream** out) {
    return stream_create("dcs_stream_create", plan, S, 0, time_context, overlap, tiler, eps_mode, scale, rise_h, max_push, out);
}

extern "C" int dcs_stream_create_channels(dcs_stft* plan, int S, int C, int time_context, int overlap, int tiler, int eps_mode,
                                          float scale, const double* rise_h, int64_t max_push, dcs_stream** out) {
    if (C < 1 || C > kMaxChannels)
        DCS_FAIL(DCS_EINVAL, "dcs_stream_create_channels: %d channels (1 .. %d)", C, kMaxChannels);
    return stream_create("dcs_stream_create_channels", plan, S, C, time_context, overlap, tiler, eps_mode, scale, rise_h, max_push,
                         out);
}

extern "C" int dcs_stream_create_stereo(dcs_stft* plan, int S, int C, int time_context, int overlap, int tiler, float scale,
                                        const double* rise_h, int64_t max_push, dcs_stream** out) {
    if (C < 1 || C > kMaxChannels) DCS_FAIL(DCS_EINVAL, "dcs_stream_create_stereo: %d channels (1 .. %d)", C, kMaxChannels);
    if (scale == 0.f) DCS_FAIL(DCS_EINVAL, "dcs_stream_create_stereo: scale 0");
    return stream_create("dcs_stream_create_stereo", plan, S, C, time_context, overlap, tiler, DCS_EPS_B, scale, rise_h, max_push,
                         out, nullptr, true);
}

extern "C" int dcs_stream_create_score(dcs_stft* plan, int S, int time_context, int overlap, int tiler, int eps_mode, float scale,
                                       const double* rise_h, int64_t max_push, const double* notes_h, int ninst, int n_notes,
                                       int width, int normalise, int mixture, dcs_stream** out) {
    const ScoreSpec sc = {notes_h, ninst, n_notes, width, normalise, mixture};
    return stream_create("dcs_stream_create_score", plan, S, 0, time_context, overlap, tiler, eps_mode, scale, rise_h, max_push,
                         out, &sc);
}

extern "C" int dcs_stream_destroy(dcs_stream* s) {
    if (!s) return DCS_OK;
    DCS_ON_DEVICE(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    dcs_dev_free(s->samples);
    dcs_dev_free(s->mag);
    dcs_dev_free(s->phase);
    dcs_dev_free(s->p);
    dcs_dev_free(s->est);
    dcs_dev_free(s->tf);
    dcs_dev_free(s->rise);
    dcs_dev_free(s->masks);
    dcs_dev_free(s->table);
    dcs_dev_free(s->fmag);
    dcs_dev_free(s->fphase);
    dcs_dev_free(s->follow_cls);
    dcs_dev_free(s->follow_chroma);
    dcs_dev_free(s->follow_pos);
    dcs_mwf_online_destroy(s->mwf);
    delete s;
    return DCS_OK;
}

extern "C" int dcs_stream_reset(dcs_stream* s) {
    if (!s) DCS_FAIL(DCS_EINVAL, "dcs_stream_reset: null stream");
    // the rings keep their contents: no slot is read before the push or pull that needs it has written it (the score stays too)
    s->P = s->A = s->K = s->Tf = s->E = s->T = s->L = s->pending = 0;
    s->want_pull = s->ended = false;
    s->mwf_rows = 0;
    if (s->mwf) DCS_CHECK(dcs_mwf_online_reset(s->mwf));      // frame 0 reads no state: nothing is cleared on the device
    s->follow_rows = 0;
    s->follow_stale = false;
    if (s->follow) DCS_CHECK(dcs_follow_reset(s->follow));
    return DCS_OK;
}

extern "C" int dcs_stream_set_mwf(dcs_stream* s, int niter, double forget, double loading, double eps) {
    if (!s) DCS_FAIL(DCS_EINVAL, "dcs_stream_set_mwf: null stream");
    if (s->C != 2) DCS_FAIL(DCS_EINVAL, "dcs_stream_set_mwf: a channel or stereo stream of 2 channels (this one has %d)", s->C);
    if (s->P > 0 || s->want_pull || s->ended) DCS_FAIL(DCS_EINVAL, "dcs_stream_set_mwf: the stream has samples (reset it first)");
    DCS_CHECK(dcs_mwf_online_check("dcs_stream_set_mwf", s->F, s->S, niter, forget, loading, eps));
    DCS_ON_DEVICE(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    dcs_mwf_online_destroy(s->mwf);
    dcs_dev_free(s->fmag);
    dcs_dev_free(s->fphase);
    s->mwf = nullptr;
    s->fmag = s->fphase = nullptr;
    s->bytes -= s->mwf_bytes;
    s->mwf_bytes = s->mwf_rows = 0;
    if (niter == 0) return DCS_OK;
    const int64_t buf = (int64_t)s->nch * s->S * s->ff * s->F * (int64_t)sizeof(float);
    int rc = dcs_mwf_online_create(s->ctx, s->F, s->S, niter, forget, loading, eps, &s->mwf);
    if (rc == DCS_OK) {
        hipError_t e = dcs_dev_alloc((void**)&s->fmag, (size_t)buf, "stream.mwf_mag");
        if (e == hipSuccess) e = dcs_dev_alloc((void**)&s->fphase, (size_t)buf, "stream.mwf_phase");
        if (e != hipSuccess) {
            dcs_set_error("dcs_stream_set_mwf: 2 x %lld bytes: %s", (long long)buf, hipGetErrorString(e));
            rc = e == hipErrorOutOfMemory ? DCS_ENOMEM : DCS_EHIP;
        }
    }
    if (rc != DCS_OK) {                                       // the stream is left with the filter off
        dcs_mwf_online_destroy(s->mwf);
        dcs_dev_free(s->fmag);
        dcs_dev_free(s->fphase);
        s->mwf = nullptr;
        s->fmag = s->fphase = nullptr;
        return rc;
    }
    s->mwf_bytes = 2 * buf + dcs_mwf_online_bytes(s->mwf);
    s->bytes += s->mwf_bytes;
    return DCS_OK;
}

extern "C" int dcs_stream_mwf_last(dcs_stream* s, float* mag_d, float* phase_d, int64_t ch_stride, int64_t src_stride, int64_t ld) {
    if (!s) DCS_FAIL(DCS_EINVAL, "dcs_stream_mwf_last: null stream");
    if (!s->mwf) DCS_FAIL(DCS_EINVAL, "dcs_stream_mwf_last: the filter is off (dcs_stream_set_mwf)");
    const int64_t rows = s->mwf_rows;
    if (rows == 0) return DCS_OK;
    if (!mag_d || !phase_d) DCS_FAIL(DCS_EINVAL, "dcs_stream_mwf_last: null buffer");
    if (ld < s->F || src_stride < rows * ld || ch_stride < (s->S - 1) * src_stride + rows * ld)
        DCS_FAIL(DCS_EINVAL, "dcs_stream_mwf_last: ld %lld, strides %lld / %lld below %lld rows of %d bins", (long long)ld,
                 (long long)src_stride, (long long)ch_stride, (long long)rows, s->F);
    DCS_ON_DEVICE(s->ctx->device);
    hipLaunchKernelGGL(stream_mwf_copy_kernel, dim3((unsigned)rows, (unsigned)dcs_cdiv(s->F, kThreads), (unsigned)(s->nch * s->S)),
                       dim3(kThreads), 0, s->ctx->stream, (const float*)s->fmag, (const float*)s->fphase, s->ff * s->F, s->S, s->F,
                       mag_d, phase_d, ch_stride, src_stride, ld);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

extern "C" int dcs_stream_set_follow(dcs_stream* s, dcs_follow* f, const int8_t* cls_h, float floor) {
    if (!s || !f || !cls_h) DCS_FAIL(DCS_EINVAL, "dcs_stream_set_follow: null argument");
    if (!s->ninst) DCS_FAIL(DCS_EINVAL, "dcs_stream_set_follow: not a score stream (dcs_stream_create_score)");
    if (s->P > 0 || s->want_pull || s->ended) DCS_FAIL(DCS_EINVAL, "dcs_stream_set_follow: the stream has samples (reset it first)");
    if (f->frames > 0) DCS_FAIL(DCS_EINVAL, "dcs_stream_set_follow: the follower has taken %lld frames (reset it first)", (long long)f->frames);
    if (f->ctx != s->ctx) DCS_FAIL(DCS_EINVAL, "dcs_stream_set_follow: the follower belongs to another context");
    if (f->max_frames < s->fp)
        DCS_FAIL(DCS_EINVAL, "dcs_stream_set_follow: the follower takes %lld frames a push, one push of this stream can complete %lld",
                 (long long)f->max_frames, (long long)s->fp);
    if (!(floor >= 0.f)) DCS_FAIL(DCS_EINVAL, "dcs_stream_set_follow: floor %g", (double)floor);
    for (int k = 0; k < s->F; ++k)
        if (cls_h[k] < -1 || cls_h[k] >= 12) DCS_FAIL(DCS_EINVAL, "dcs_stream_set_follow: class %d of bin %d (-1 .. 11)", (int)cls_h[k], k);
    DCS_ON_DEVICE(s->ctx->device);
    if (!s->follow_cls) {                                     // the first arming: the three buffers, whose sizes are the stream's own
        struct { void** ptr; int64_t bytes; const char* name; } extra[] = {
            {(void**)&s->follow_cls, dcs_round_up(s->F, 256), "stream.follow_cls"},
            {(void**)&s->follow_chroma, s->fp * 12 * (int64_t)sizeof(float), "stream.follow_chroma"},
            {(void**)&s->follow_pos, s->fp * (int64_t)sizeof(int32_t), "stream.follow_pos"},
        };
        hipError_t e = hipSuccess;
        int64_t total = 0;
        for (auto& b : extra) {
            if (e == hipSuccess) e = dcs_dev_alloc(b.ptr, (size_t)b.bytes, b.name);
            total += b.bytes;
        }
        if (e != hipSuccess) {                                // the stream is left as it was: not armed
            for (auto& b : extra) {
                dcs_dev_free(*b.ptr);
                *b.ptr = nullptr;
            }
            dcs_set_error("dcs_stream_set_follow: %lld bytes: %s", (long long)total, hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? DCS_ENOMEM : DCS_EHIP;
        }
        s->follow_bytes = total;
    }
    (void)hipStreamSynchronize(s->ctx->stream);               // no earlier launch still reads the table this call replaces
    if (hipMemcpy(s->follow_cls, cls_h, (size_t)s->F, hipMemcpyHostToDevice) != hipSuccess) {
        if (!s->follow) {                                     // never armed: the buffers go, the stream is left as it was
            dcs_dev_free(s->follow_cls);
            dcs_dev_free(s->follow_chroma);
            dcs_dev_free(s->follow_pos);
            s->follow_cls = nullptr;
            s->follow_chroma = nullptr;
            s->follow_pos = nullptr;
            s->follow_bytes = 0;
        }
        DCS_FAIL(DCS_EHIP, "dcs_stream_set_follow: uploading the class table failed");
    }
    if (!s->follow) s->bytes += s->follow_bytes;              // counted once, when the stream is first armed
    s->follow = f;
    s->follow_floor = floor;
    s->follow_rows = 0;
    return DCS_OK;
}

extern "C" int dcs_stream_follow_last(dcs_stream* s, int32_t* pos_d, int64_t cap, int64_t* n) {
    if (!s || !n) DCS_FAIL(DCS_EINVAL, "dcs_stream_follow_last: null argument");
    if (!s->follow) DCS_FAIL(DCS_EINVAL, "dcs_stream_follow_last: the stream follows no score (dcs_stream_set_follow)");
    const int64_t rows = s->follow_rows;
    if (rows > cap || (rows > 0 && !pos_d))
        DCS_FAIL(DCS_EINVAL, "dcs_stream_follow_last: %lld positions, room for %lld", (long long)rows, (long long)(pos_d ? cap : 0));
    if (rows > 0) {
        DCS_ON_DEVICE(s->ctx->device);
        DCS_HIP(hipMemcpyAsync(pos_d, s->follow_pos, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToDevice, s->ctx->stream));
    }
    *n = rows;
    return DCS_OK;
}

extern "C" int64_t dcs_stream_max_tiles(const dcs_stream* s) { return s ? s->max_tiles : -1; }
extern "C" int64_t dcs_stream_bytes(const dcs_stream* s) { return s ? s->bytes : -1; }

namespace {

// both kinds of push: audio_d rows at row_stride, the callers' frame copies at ch_stride (neither is read for one row)
int stream_push(const char* who, dcs_stream* s, const float* audio_d, int64_t row_stride, int64_t n, int last, float* tiles_d,
                int64_t tiles_cap, int64_t* n_tiles_out, float* mag_d, float* phase_d, int64_t ch_stride, int64_t ld,
                int64_t* n_frames_out) {
    if (s->want_pull) DCS_FAIL(DCS_EINVAL, "%s: the tiles of the previous push have not been pulled", who);
    if (s->ended) DCS_FAIL(DCS_EINVAL, "%s: the signal has ended (dcs_stream_reset starts another)", who);
    if (s->follow_stale)
        DCS_FAIL(DCS_EINVAL, "%s: an earlier push failed after the follower had taken its frames (dcs_stream_reset starts again)", who);
    if (n < 0 || n > s->max_push)
        DCS_FAIL(DCS_EINVAL, "%s: %lld samples (0 .. max_push = %lld)", who, (long long)n, (long long)s->max_push);
    if (n > 0 && !audio_d) DCS_FAIL(DCS_EINVAL, "%s: null audio", who);
    if (n > 0 && s->rows > 1 && row_stride < n)
        DCS_FAIL(DCS_EINVAL, "%s: row stride %lld below %lld samples", who, (long long)row_stride, (long long)n);
    if ((mag_d || phase_d) && ld < s->F) DCS_FAIL(DCS_EINVAL, "%s: ld %lld below the %d bins", who, (long long)ld, s->F);
    const int N = s->N, hop = s->hop, H = N / 2;
    const int64_t P = s->P + n;
    int64_t A, K, T = 0;
    if (last) {
        T = dcs_frame_count(P, hop);
        A = T;
        K = dcs_tile_count(T, s->tc, s->ov, s->tiler);
    } else {
        A = P < H ? 0 : (P - H) / hop + 1;
        K = A < s->tc ? 0 : (A - s->tc) / s->st + 1;
    }
    const int64_t n_frames = A - s->A, n_tiles = K - s->K;
    if (n_frames < 0 || n_frames > s->fp || n_tiles < 0 || n_tiles > s->max_tiles)
        DCS_FAIL(DCS_EHIP, "%s: internal count out of range (%lld frames, %lld tiles)", who, (long long)n_frames,
                 (long long)n_tiles);
    if (n_tiles > tiles_cap || (n_tiles > 0 && !tiles_d))
        DCS_FAIL(DCS_EINVAL, "%s: %lld tiles become ready, room for %lld (dcs_stream_max_tiles: %lld)", who,
                 (long long)n_tiles, (long long)(tiles_d ? tiles_cap : 0), (long long)s->max_tiles);
    if ((mag_d || phase_d) && s->nch > 1 && ch_stride < n_frames * ld)
        DCS_FAIL(DCS_EINVAL, "%s: channel stride %lld below %lld rows", who, (long long)ch_stride, (long long)n_frames);
    DCS_ON_DEVICE(s->ctx->device);
    hipStream_t q = s->ctx->stream;
    if (n > 0) {
        hipLaunchKernelGGL(stream_append_kernel, dim3((unsigned)dcs_cdiv(n, kThreads), (unsigned)s->rows), dim3(kThreads), 0, q,
                           audio_d, row_stride, n, s->P, s->samples, s->cap);
        DCS_HIP(hipGetLastError());
    }
    if (n_frames > 0)   // grid (n_frames, rows)
        DCS_CHECK((launch_frames<float, float2>(s->plan, stream_frames_kernel, n_frames, s->rows - 1, s->plan->win_f,
                                                s->plan->tw_f, (const float*)s->samples, s->cap, P, s->A, s->rf, s->mag,
                                                s->phase, s->nch, mag_d, phase_d, ch_stride, ld)));
    // set once the follower has taken this push's frames; a failure behind that point leaves it ahead of the stream's counts
    struct FollowAhead {
        dcs_stream* s;
        bool on;
        ~FollowAhead() { if (on) s->follow_stale = true; }
    } ahead = {s, false};
    if (s->follow && n_frames > 0) {
        // chroma of the new rows of the magnitude ring (two pieces where it wraps), the follower, the masks from its positions
        const int64_t a0 = s->A % s->rf, n1 = n_frames < s->rf - a0 ? n_frames : s->rf - a0;
        DCS_CHECK(dcs_launch_chroma(q, s->mag + a0 * s->F, s->F, n1, s->F, s->follow_cls, s->follow_floor, s->follow_chroma));
        if (n_frames > n1)
            DCS_CHECK(dcs_launch_chroma(q, s->mag, s->F, n_frames - n1, s->F, s->follow_cls, s->follow_floor,
                                        s->follow_chroma + n1 * 12));
        DCS_CHECK(dcs_follow_push(s->follow, s->follow_chroma, n_frames, s->follow_pos));
        ahead.on = true;
        DcsTimer tm(s->ctx, DCS_TAG_SCORE);
        hipLaunchKernelGGL(stream_follow_masks_kernel, dim3((unsigned)n_frames), dim3(kThreads), 0, q, (const int*)s->table,
                           s->npairs, (int)s->row_t0.size(), (const int32_t*)s->follow_pos, s->A, s->rf, s->F, s->ninst,
                           s->normalise, s->vals, s->masks);
        tm.done();
        DCS_HIP(hipGetLastError());
    } else if (s->ninst && n_frames > 0) {
        // the candidate rows of frames [s->A, A): first frame below A (the rows are sorted by it) and, by the running maximum of
        // the end frames, no row before r_lo reaching s->A -- two binary searches, whatever the length of the score
        const int64_t a_hi = A < 2147483647LL ? A : 2147483647LL, a_lo = s->A < 2147483647LL ? s->A : 2147483647LL;
        const int r_hi = (int)(std::lower_bound(s->row_t0.begin(), s->row_t0.end(), (int)a_hi) - s->row_t0.begin());
        int r_lo = (int)(std::upper_bound(s->row_end_max.begin(), s->row_end_max.end(), (int)a_lo) - s->row_end_max.begin());
        if (r_lo > r_hi) r_lo = r_hi;
        DcsTimer tm(s->ctx, DCS_TAG_SCORE);
        hipLaunchKernelGGL(stream_masks_kernel, dim3((unsigned)n_frames), dim3(kThreads), 0, q, (const int*)s->table, s->npairs,
                           r_lo, r_hi, s->A, s->rf, s->F, s->ninst, s->normalise, s->vals, s->masks);
        tm.done();
        DCS_HIP(hipGetLastError());
    }
    if (n_tiles > 0 && s->ninst) {
        DcsTimer tm(s->ctx, DCS_TAG_TILE);
        hipLaunchKernelGGL(stream_score_tiles_kernel, dim3((unsigned)(n_tiles * s->ninst * s->tc)), dim3(kThreads), 0, q,
                           (const float*)s->mag, (const float*)s->masks, s->rf, s->F, s->tc, s->st, s->ninst, s->K, A, s->scale,
                           tiles_d);
        tm.done();
        DCS_HIP(hipGetLastError());
    } else if (n_tiles > 0 && s->stereo) {
        DcsTimer tm(s->ctx, DCS_TAG_TILE);
        hipLaunchKernelGGL(stream_stereo_tiles_kernel, dim3((unsigned)(n_tiles * s->tc), (unsigned)s->C), dim3(kThreads), 0, q,
                           (const float*)s->mag, s->rf, s->F, (int)dcs_round_up(s->F, 4), s->tc, s->st, s->K, A, s->scale, tiles_d);
        tm.done();
        DCS_HIP(hipGetLastError());
    } else if (n_tiles > 0) {
        DcsTimer tm(s->ctx, DCS_TAG_TILE);
        const float* mix = s->mag + (int64_t)(s->rows - 1) * s->rf * s->F;     // the down-mix: the last row
        hipLaunchKernelGGL(stream_tiles_kernel, dim3((unsigned)(n_tiles * s->tc)), dim3(kThreads), 0, q, mix, s->rf, s->F, s->tc,
                           s->st, s->K, A, s->scale, tiles_d);
        tm.done();
        DCS_HIP(hipGetLastError());
    }
    s->P = P; s->A = A; s->K = K;
    ahead.on = false;
    if (s->follow) s->follow_rows = n_frames;
    s->pending = n_tiles;
    s->want_pull = true;
    if (last) {
        s->ended = true;
        s->T = T;
        s->L = P;
    }
    if (n_tiles_out) *n_tiles_out = n_tiles;
    if (n_frames_out) *n_frames_out = n_frames;
    return DCS_OK;
}

// every kind of pull: channel c of the samples at + c pcm_ch_stride, of the estimates at + c est_ch_stride; p_ch_stride and
// p_ld are read for a stereo stream alone
int stream_pull(const char* who, dcs_stream* s, const float* p_d, int64_t p_src_stride, int64_t n_tiles, float* pcm_d,
                int64_t pcm_ch_stride, int64_t pcm_stride, int64_t pcm_cap, int64_t* n_out, float* est_d, int64_t est_ch_stride,
                int64_t est_src_stride, int64_t ld, int64_t p_ch_stride = 0, int64_t p_ld = 0) {
    if (!s->want_pull) DCS_FAIL(DCS_EINVAL, "%s: no push to pull for", who);
    if (n_tiles != s->pending)
        DCS_FAIL(DCS_EINVAL, "%s: p of %lld tiles, the preceding push returned %lld", who, (long long)n_tiles,
                 (long long)s->pending);
    if (n_tiles > 0 && !p_d) DCS_FAIL(DCS_EINVAL, "%s: null p", who);
    const int64_t tile_elems = (int64_t)s->tc * s->F;
    if (n_tiles > 0 && !s->stereo && s->S > 1 && p_src_stride < n_tiles * tile_elems)
        DCS_FAIL(DCS_EINVAL, "%s: source stride %lld below %lld tiles", who, (long long)p_src_stride, (long long)n_tiles);
    if (n_tiles > 0 && s->stereo) {
        // the extent of one channel's rows, and of one source: the channels are whole planes or sit side by side in a row
        if (p_ld < s->F || p_ch_stride < 0 || p_ld > (1LL << 40) || p_ch_stride > (1LL << 40))
            DCS_FAIL(DCS_EINVAL, "%s: row pitch %lld below the %d bins (channel stride %lld)", who, (long long)p_ld, s->F,
                     (long long)p_ch_stride);
        const int64_t ch_extent = (n_tiles * s->tc - 1) * p_ld + s->F;
        if (s->C > 1 && p_ch_stride < ch_extent && (p_ch_stride < s->F || p_ld < (s->C - 1) * p_ch_stride + s->F))
            DCS_FAIL(DCS_EINVAL, "%s: channel stride %lld: neither whole planes of %lld floats nor side by side in rows of %lld",
                     who, (long long)p_ch_stride, (long long)ch_extent, (long long)p_ld);
        const int64_t src_extent = p_ch_stride >= ch_extent ? (s->C - 1) * p_ch_stride + ch_extent
                                                             : (n_tiles * s->tc - 1) * p_ld + (s->C - 1) * p_ch_stride + s->F;
        if (s->S > 1 && p_src_stride < src_extent)
            DCS_FAIL(DCS_EINVAL, "%s: source stride %lld below the %lld floats of one source", who, (long long)p_src_stride,
                     (long long)src_extent);
    }
    if (est_d && ld < s->F) DCS_FAIL(DCS_EINVAL, "%s: ld %lld below the %d bins", who, (long long)ld, s->F);
    if (s->ended && s->K == 0) {
        s->want_pull = false;
        DCS_FAIL(DCS_EINVAL, "%s: %lld frames give no tile (the reference fails in overlapadd_multi)", who, (long long)s->T);
    }
    const int N = s->N, hop = s->hop, H = N / 2;
    const int64_t Tf = s->ended ? s->T : s->K * s->st;
    int64_t E = s->ended ? s->L : Tf * hop - H;
    if (E < 0) E = 0;
    const int64_t n_fold = Tf - s->Tf, n_pcm = E - s->E;
    if (n_fold < 0 || n_fold > s->ff || n_pcm < 0)
        DCS_FAIL(DCS_EHIP, "%s: internal count out of range (%lld frames, %lld samples)", who, (long long)n_fold,
                 (long long)n_pcm);
    if (n_pcm > 0 && (!pcm_d || n_pcm > pcm_cap || (s->S > 1 && pcm_stride < n_pcm) ||
                      (s->nch > 1 && pcm_ch_stride < (s->S - 1) * pcm_stride + n_pcm)))
        DCS_FAIL(DCS_EINVAL, "%s: %lld samples become final, room for %lld (source stride %lld, channel stride %lld)", who,
                 (long long)n_pcm, (long long)(pcm_d ? pcm_cap : 0), (long long)pcm_stride, (long long)pcm_ch_stride);
    if (est_d && ((s->S > 1 && est_src_stride < n_fold * ld) ||
                  (s->nch > 1 && est_ch_stride < (s->S - 1) * est_src_stride + n_fold * ld)))
        DCS_FAIL(DCS_EINVAL, "%s: estimate strides %lld / %lld below %lld rows", who, (long long)est_src_stride,
                 (long long)est_ch_stride, (long long)n_fold);
    DCS_ON_DEVICE(s->ctx->device);
    hipStream_t q = s->ctx->stream;
    const int64_t k_first = s->K - n_tiles;
    if (n_tiles > 0 && s->stereo) {
        hipLaunchKernelGGL(stream_keep_p_stereo_kernel, dim3((unsigned)(n_tiles * s->tc), (unsigned)s->C, (unsigned)s->S),
                           dim3(kThreads), 0, q, p_d, p_src_stride, p_ch_stride, p_ld, k_first, s->tc, s->F, s->p, s->rp);
        DCS_HIP(hipGetLastError());
    } else if (n_tiles > 0) {
        const unsigned gy = (unsigned)(tile_elems < 64 * kThreads ? dcs_cdiv(tile_elems, kThreads) : 64);
        hipLaunchKernelGGL(stream_keep_p_kernel, dim3((unsigned)n_tiles, gy, (unsigned)s->S), dim3(kThreads), 0, q, p_d,
                           p_src_stride, k_first, tile_elems, s->p, s->rp);
        DCS_HIP(hipGetLastError());
    }
    if (n_fold > 0) {
        if (s->stereo) {
            DcsTimer tm(s->ctx, DCS_TAG_MASK);
            hipLaunchKernelGGL(stream_fold_stereo_kernel, dim3((unsigned)n_fold, (unsigned)dcs_cdiv(s->F, kThreads), (unsigned)s->C),
                               dim3(kThreads), 0, q, (const float*)s->p, s->rp, s->K, s->S, s->tc, s->ov, s->F, (const float*)s->rise,
                               (const float*)s->mag, s->rf, s->Tf, s->c0, s->est, s->ff * s->F, est_d, est_ch_stride, est_src_stride,
                               ld);
            tm.done();
            DCS_HIP(hipGetLastError());
        } else {
            DcsTimer tm(s->ctx, DCS_TAG_MASK);
            auto fold = stream_fold_kernel<kMixMag>;
            if (s->ninst) fold = s->mixture == DCS_MIX_SUM ? stream_fold_kernel<kMixSum> : stream_fold_kernel<kMixCh0>;
            hipLaunchKernelGGL(fold, dim3((unsigned)n_fold, (unsigned)dcs_cdiv(s->F, kThreads)), dim3(kThreads), 0, q,
                               (const float*)s->p, s->rp, s->K, s->S, s->tc, s->ov, s->F, s->eps_mode, (const float*)s->rise,
                               (const float*)s->mag, s->rf, s->nch, s->Tf, s->est, s->ff * s->F, est_d, est_ch_stride,
                               est_src_stride, ld, (const float*)s->masks, s->ninst);
            tm.done();
            DCS_HIP(hipGetLastError());
        }
        if (s->mwf) {
            // the online filter over exactly the rows this pull folded: the frames are contiguous in est, in the rings up to the
            // wrap (the filter's bits do not depend on the cut)
            for (int64_t t = s->Tf; t < Tf;) {
                const int64_t slot = t % s->rf, n = std::min(Tf - t, s->rf - slot), row = t - s->Tf;
                DCS_CHECK(dcs_mwf_online_push_f32(s->mwf, s->mag + slot * s->F, s->phase + slot * s->F, s->rf * s->F,
                                                  s->est + row * s->F, (int64_t)s->S * s->ff * s->F, s->ff * s->F, s->F, n, 1.f,
                                                  s->fmag + row * s->F, s->fphase + row * s->F));
                t += n;
            }
        }
        const int M = N / 2;
        size_t lds = (3 * (size_t)M + 2) * sizeof(float2);
        const int tw_lds = lds <= 64 * 1024;
        if (!tw_lds) lds = (2 * (size_t)M + 1) * sizeof(float2);
        auto inverse = s->mwf ? stream_inverse_kernel<true> : stream_inverse_kernel<false>;
        if (lds > 48 * 1024)
            DCS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(inverse), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        DcsTimer tm(s->ctx, DCS_TAG_ISTFT);
        hipLaunchKernelGGL(inverse, dim3((unsigned)n_fold, (unsigned)s->S, (unsigned)s->nch), dim3(kThreads), lds, q,
                           (const float*)(s->mwf ? s->fmag : s->est), s->ff * s->F, (const float*)(s->mwf ? s->fphase : s->phase), s->rf,
                           s->Tf, s->tf, s->rt, s->S, (const float*)s->plan->win_f, (const float2*)s->plan->tw_f, N, s->plan->log2m,
                           (float)sqrt((double)N), tw_lds);
        tm.done();
        DCS_HIP(hipGetLastError());
    }
    if (n_pcm > 0) {
        DcsTimer tm(s->ctx, DCS_TAG_ISTFT);
        hipLaunchKernelGGL(stream_gather_kernel, dim3((unsigned)dcs_cdiv(n_pcm, kThreads), (unsigned)s->S, (unsigned)s->nch),
                           dim3(kThreads), 0, q, (const float*)s->tf, s->rt, s->S, N, hop, Tf, (const float*)s->plan->wsq_f, s->E,
                           n_pcm, pcm_d, pcm_ch_stride, pcm_stride);
        tm.done();
        DCS_HIP(hipGetLastError());
    }
    s->mwf_rows = n_fold;
    s->Tf = Tf; s->E = E;
    s->want_pull = false;
    if (n_out) *n_out = n_pcm;
    return DCS_OK;
}

}  // namespace

extern "C" int dcs_stream_push(dcs_stream* s, const float* audio_d, int64_t n, int last, float* tiles_d, int64_t tiles_cap,
                               int64_t* n_tiles_out, float* mag_d, float* phase_d, int64_t ld, int64_t* n_frames_out) {
    if (!s) DCS_FAIL(DCS_EINVAL, "dcs_stream_push: null stream");
    if (s->stereo) DCS_FAIL(DCS_EINVAL, "dcs_stream_push: a stereo stream takes dcs_stream_push_stereo");
    if (s->C) DCS_FAIL(DCS_EINVAL, "dcs_stream_push: a channel stream takes dcs_stream_push_channels");
    return stream_push("dcs_stream_push", s, audio_d, 0, n, last, tiles_d, tiles_cap, n_tiles_out, mag_d, phase_d, 0, ld,
                       n_frames_out);
}

extern "C" int dcs_stream_push_channels(dcs_stream* s, const float* audio_d, int64_t row_stride, int64_t n, int last,
                                        float* tiles_d, int64_t tiles_cap, int64_t* n_tiles_out, float* mag_d, float* phase_d,
                                        int64_t ch_stride, int64_t ld, int64_t* n_frames_out) {
    if (!s) DCS_FAIL(DCS_EINVAL, "dcs_stream_push_channels: null stream");
    if (s->stereo) DCS_FAIL(DCS_EINVAL, "dcs_stream_push_channels: a stereo stream takes dcs_stream_push_stereo");
    if (!s->C) DCS_FAIL(DCS_EINVAL, "dcs_stream_push_channels: a mono stream takes dcs_stream_push");
    return stream_push("dcs_stream_push_channels", s, audio_d, row_stride, n, last, tiles_d, tiles_cap, n_tiles_out, mag_d,
                       phase_d, ch_stride, ld, n_frames_out);
}

extern "C" int dcs_stream_pull(dcs_stream* s, const float* p_d, int64_t p_src_stride, int64_t n_tiles, float* pcm_d,
                               int64_t pcm_stride, int64_t pcm_cap, int64_t* n_out, float* est_d, int64_t est_src_stride,
                               int64_t ld) {
    if (!s) DCS_FAIL(DCS_EINVAL, "dcs_stream_pull: null stream");
    if (s->stereo) DCS_FAIL(DCS_EINVAL, "dcs_stream_pull: a stereo stream takes dcs_stream_pull_stereo");
    if (s->C) DCS_FAIL(DCS_EINVAL, "dcs_stream_pull: a channel stream takes dcs_stream_pull_channels");
    return stream_pull("dcs_stream_pull", s, p_d, p_src_stride, n_tiles, pcm_d, 0, pcm_stride, pcm_cap, n_out, est_d, 0,
                       est_src_stride, ld);
}

extern "C" int dcs_stream_pull_channels(dcs_stream* s, const float* p_d, int64_t p_src_stride, int64_t n_tiles, float* pcm_d,
                                        int64_t pcm_ch_stride, int64_t pcm_stride, int64_t pcm_cap, int64_t* n_out, float* est_d,
                                        int64_t est_ch_stride, int64_t est_src_stride, int64_t ld) {
    if (!s) DCS_FAIL(DCS_EINVAL, "dcs_stream_pull_channels: null stream");
    if (s->stereo) DCS_FAIL(DCS_EINVAL, "dcs_stream_pull_channels: a stereo stream takes dcs_stream_pull_stereo");
    if (!s->C) DCS_FAIL(DCS_EINVAL, "dcs_stream_pull_channels: a mono stream takes dcs_stream_pull");
    return stream_pull("dcs_stream_pull_channels", s, p_d, p_src_stride, n_tiles, pcm_d, pcm_ch_stride, pcm_stride, pcm_cap,
                       n_out, est_d, est_ch_stride, est_src_stride, ld);
}

extern "C" int dcs_stream_push_stereo(dcs_stream* s, const float* audio_d, int64_t row_stride, int64_t n, int last, float* tiles_d,
                                      int64_t tiles_cap, int64_t* n_tiles_out, float* mag_d, float* phase_d, int64_t ch_stride,
                                      int64_t ld, int64_t* n_frames_out) {
    if (!s) DCS_FAIL(DCS_EINVAL, "dcs_stream_push_stereo: null stream");
    if (!s->stereo) DCS_FAIL(DCS_EINVAL, "dcs_stream_push_stereo: not a stereo stream (dcs_stream_create_stereo)");
    return stream_push("dcs_stream_push_stereo", s, audio_d, row_stride, n, last, tiles_d, tiles_cap, n_tiles_out, mag_d, phase_d,
                       ch_stride, ld, n_frames_out);
}

extern "C" int dcs_stream_pull_stereo(dcs_stream* s, const float* p_d, int64_t p_src_stride, int64_t p_ch_stride, int64_t p_ld,
                                      int64_t n_tiles, float* pcm_d, int64_t pcm_ch_stride, int64_t pcm_stride, int64_t pcm_cap,
                                      int64_t* n_out, float* est_d, int64_t est_ch_stride, int64_t est_src_stride, int64_t ld) {
    if (!s) DCS_FAIL(DCS_EINVAL, "dcs_stream_pull_stereo: null stream");
    if (!s->stereo) DCS_FAIL(DCS_EINVAL, "dcs_stream_pull_stereo: not a stereo stream (dcs_stream_create_stereo)");
    return stream_pull("dcs_stream_pull_stereo", s, p_d, p_src_stride, n_tiles, pcm_d, pcm_ch_stride, pcm_stride, pcm_cap, n_out,
                       est_d, est_ch_stride, est_src_stride, ld, p_ch_stride, p_ld);
}

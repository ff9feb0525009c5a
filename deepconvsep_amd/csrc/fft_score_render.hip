// Score-rendered forward STFT for gfx950: the RWC-sample training features of the Bach10 trainers, computed from a bank of
// note samples resident on the device.
//
// Replaces the note-by-note synthesis of examples/bach10/compute_features_bach10rwc.py:112-139, the float64 feature files
// it writes through compute_transform (:141; 318 MB per 45 s chunk and combination) and LargeDataset reading them back
// (dataset.py:383-488).
//
// A track is assembled from many note samples, written in list order by assignment, so a later note overwrites an earlier
// one where they overlap:
//
//   track_s[n] = bank[off_m + (n - b_m)]  for the LARGEST m of track s with b_m <= n < b_m + len_m, else 0   (0 <= n < size)
//   mix[n]     = ((track_0[n] + track_1[n]) + track_2[n]) + ...       in list order, one addition each
//
// Note table (int64 rows (b, off, len, E), grouped per track in list order): b is non-decreasing within a track and E is
// the running maximum of b + len over the track's notes so far (dcs_score_render_pack builds and checks it on the host).
// With that order the note covering n is found from the last note with b <= n by walking back while E > n.  One workgroup
// (256 threads) forms one windowed frame of one channel: it first resolves, once, the frame's candidate notes of every
// track -- those with b < frame end and E > frame start, two binary searches by one thread per track, four integers per
// track in LDS (frame_candidates, the prepare step) -- and a sample's lookup (score_sample, the sample source) then stays
// inside that range.  The frame is formed and transformed by render_frame (fft_frame.h, shared with stft_render_kernel: the
// FFT body of stft_forward_kernel) and ends in that kernel's tail (packed_real_mag_row): the float64 block equals the
// existing kernel on host-rendered audio bit for bit.
//
// Descriptor of a virtual file (DCS_SCORE_RENDER_ROW(S) int64): size, T, then S x (first note, note count).  The file path
// builds both tables on the host (validated there); the feed reads tables the caller keeps on the device, so the kernel
// itself bounds every note index and every bank index: what lies outside reads as zero.
//
// The score-informed trainer's feed on the same data (examples/bach10_scoreinformed/compute_features_bach10rwc.py:96-163 read
// back by LargeDatasetMask2) is stft_score_informed_kernel below: the render feed with train::gather_score_kernel's harmonic
// masks applied to the mixture row in the same launch -- the same prepare step and sample source, and a tail of its own.
#include "dcs_internal.h"
#include "fft_frame.h"

namespace {

constexpr int kFileHead = 2;    // size, T
constexpr int kMaxTracks = 8;

// sample n of a track whose candidate notes are [lo, hi) of `notes`
template <typename R>
__device__ __forceinline__ R score_track(const R* __restrict__ bank, int64_t bank_len, const int64_t* __restrict__ notes, int lo,
                                         int hi, int64_t n) {
    int a = lo, z = hi;                     // a = one past the last note with b <= n
    while (a < z) {
        const int mid = (a + z) >> 1;
        if (notes[4 * (int64_t)mid] <= n) a = mid + 1; else z = mid;
    }
    for (int m = a - 1; m >= lo; --m) {
        const int64_t* r = notes + 4 * (int64_t)m;
        const int64_t i = n - r[0];
        if (i < r[2]) {                     // the latest note that covers n
            const int64_t bi = r[1] + i;
            return (i < 0 || bi < 0 || bi >= bank_len) ? R(0) : bank[bi];
        }
        if (r[3] <= n) break;               // no earlier note reaches n
    }
    return R(0);
}

// sample n (relative to the rendered signal) of channel j (0: the mixture, 1 + s: track s)
template <typename R>
__device__ __forceinline__ R score_sample(const R* __restrict__ bank, int64_t bank_len, const int64_t* __restrict__ notes,
                                          const int* __restrict__ lo, const int* __restrict__ hi, int64_t size, int S, int j,
                                          int64_t n) {
#pragma clang fp contract(off)
    if (n < 0 || n >= size) return R(0);
    if (j > 0) return score_track<R>(bank, bank_len, notes, lo[j - 1], hi[j - 1], n);
    R acc = score_track<R>(bank, bank_len, notes, lo[0], hi[0], n);
    for (int s = 1; s < S; ++s) acc = acc + score_track<R>(bank, bank_len, notes, lo[s], hi[s], n);
    return acc;
}

// the frame's candidate notes [lo, hi) of track s: b < f1 and E > f0 for the frame's samples [f0, f1) inside [0, size)
__device__ __forceinline__ void frame_candidates(const int64_t* __restrict__ notes, int n_notes, const int64_t* __restrict__ row,
                                                 int s, int64_t base, int N, int64_t size, int* lo_out, int* hi_out) {
    const int64_t f0 = base > 0 ? base : 0;
    const int64_t f1 = base + N < size ? base + N : size;
    const int64_t first = row[kFileHead + 2 * s], count = row[kFileHead + 2 * s + 1];
    int lo = 0, hi = 0;
    if (f0 < f1 && first >= 0 && count > 0 && first <= (int64_t)n_notes - count) {
        int a = (int)first, z = (int)(first + count);
        while (a < z) {                 // first note with b >= f1
            const int mid = (a + z) >> 1;
            if (notes[4 * (int64_t)mid] < f1) a = mid + 1; else z = mid;
        }
        hi = a;
        a = (int)first;
        z = hi;
        while (a < z) {                 // first note with E > f0
            const int mid = (a + z) >> 1;
            if (notes[4 * (int64_t)mid + 3] <= f0) a = mid + 1; else z = mid;
        }
        lo = a;
    }
    *lo_out = lo;
    *hi_out = hi;
}

// FEED = false: one virtual file (row 0 of `files`), blockIdx.x = frame t, output row (j T + t) of out0 [1 + S][T][ld].
// FEED = true: blockIdx.x = b * tc + t of window b = (file, first frame); out0 = inputs [B][1][tc][F], out1 = targets
//   [B][S][tc][F], values times `scale`; zero rows for file < 0, file >= n_files and frames past T.
// blockIdx.y = j: 0 the mixture, 1 + s track s.
template <typename R, typename R2, bool FEED>
__global__ __launch_bounds__(kThreads) void stft_score_render_kernel(
    const R* __restrict__ bank, int64_t bank_len, const int64_t* __restrict__ notes, int n_notes,
    const int64_t* __restrict__ files, int n_files, int S, const int* __restrict__ windows, int tc, R scale, R* __restrict__ out0,
    R* __restrict__ out1, int64_t ld, const R* __restrict__ win, const R2* __restrict__ tw, int N, int hop, int log2m, R sqrt_n,
    int tw_lds) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_lo[kMaxTracks], s_hi[kMaxTracks];
    const int M = N >> 1;
    const int tid = threadIdx.x;
    const int j = blockIdx.y;
    FeedWindow w = {0, 0, blockIdx.x, 0, true};
    R* orow;
    if (FEED) {
        w = feed_window(windows, tc, n_files);
        orow = j == 0 ? out0 + (w.b * tc + w.tt) * ld : out1 + (((w.b * S + j - 1) * tc) + w.tt) * ld;
    }
    const int64_t t = w.t;
    const int64_t* row = files + (w.live ? w.fi : 0) * (kFileHead + 2 * S);
    const int64_t size = w.live ? row[0] : 0;
    const int64_t T = w.live ? row[1] : 0;
    if (!FEED) orow = out0 + ((int64_t)j * T + t) * ld;
    if (!w.live || t >= T) return zero_row(orow, ld);
    const int64_t base = t * (int64_t)hop - M;   // index of padded sample t * hop in the rendered signal
    if (tid < S) frame_candidates(notes, n_notes, row, tid, base, N, size, &s_lo[tid], &s_hi[tid]);
    const R2* Z = render_frame<R, R2, true>(smem, win, tw, tw_lds, M, log2m, base, [&](int64_t q) {
        return score_sample<R>(bank, bank_len, notes, s_lo, s_hi, size, S, j, q);
    });
    packed_real_mag_row<R, R2, FEED>(Z, tw, M, ld, sqrt_n, scale, orow);
}

// ---- the score-informed feed: the windows of stft_score_render_kernel<float, float2, true> with train::gather_score_kernel's
// harmonic masks (train_core.hip) applied to the mixture row while it is still in registers.

// blockIdx.x = b * tc + t of window b = (file, first frame); blockIdx.y = j: 0 the mixture, 1 + s track s.
// j > 0: targets [B][S][tc][F] row (b, j - 1, t) = scale * mag(track), as the render feed writes it.
// j = 0: the workgroup marks, one bit per instrument, the bins of the mask notes that sound in frame fr = first frame + t
//   (first <= fr < end; integer OR in LDS, in the buffer of the FFT's ping-pong pair that does not hold Z) and writes inputs
//   [B][S][tc][F] rows (b, i, t) = (filtered_i / sum filtered) * x, x = scale * mag(mix).
// masks: per file (mask_files[2 i] = offset in ints, mask_files[2 i + 1] = P) an int table [S][P][2 + 2 npairs] as
//   dcs_trainer_pack_score writes it; a table that does not lie inside [0, mask_len) paints nothing.
__global__ __launch_bounds__(kThreads) void stft_score_informed_kernel(
    const float* __restrict__ bank, int64_t bank_len, const int64_t* __restrict__ notes, int n_notes,
    const int64_t* __restrict__ files, int n_files, int S, const int* __restrict__ masks, int64_t mask_len,
    const int64_t* __restrict__ mask_files, int npairs, const int* __restrict__ windows, int tc, float scale,
    float* __restrict__ inputs, float* __restrict__ targets, const float* __restrict__ win, const float2* __restrict__ tw, int N,
    int hop, int log2m, float sqrt_n, int tw_lds) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_lo[kMaxTracks], s_hi[kMaxTracks];
    const int M = N >> 1;
    const int F = M + 1;
    const int tid = threadIdx.x;
    const int j = blockIdx.y;
    // own window decode and zero rows, not feed_window / zero_row: with those the compiler moves this kernel's row addresses
    // into its tails and a batch took 0.9 % longer; the rule is feed_window's
    const int rs = kFileHead + 2 * S;
    const int64_t b = blockIdx.x / tc;
    const int tt = (int)(blockIdx.x - b * tc);
    const int64_t fi = windows[2 * b];
    const int64_t t = (int64_t)windows[2 * b + 1] + tt;
    const bool live = fi >= 0 && fi < n_files && t >= 0;
    const int64_t plane = (int64_t)tc * F;
    float* irow = inputs + b * S * plane + (int64_t)tt * F;                 // row (b, 0, tt); instrument i at + i * plane
    float* trow = targets + (b * S + (j > 0 ? j - 1 : 0)) * plane + (int64_t)tt * F;
    const int64_t* row = files + (live ? fi : 0) * rs;
    const int64_t size = live ? row[0] : 0;
    const int64_t T = live ? row[1] : 0;
    if (!live || t >= T) {
        if (j > 0) {
            for (int k = tid; k < F; k += kThreads) trow[k] = 0.f;
        } else {
            for (int i = 0; i < S; ++i)
                for (int k = tid; k < F; k += kThreads) irow[i * plane + k] = 0.f;
        }
        return;
    }
    const int64_t base = t * (int64_t)hop - M;   // index of padded sample t * hop in the rendered signal
    if (tid < S) frame_candidates(notes, n_notes, row, tid, base, N, size, &s_lo[tid], &s_hi[tid]);
    const float2* Z = render_frame<float, float2, true>(smem, win, tw, tw_lds, M, log2m, base, [&](int64_t q) {
        return score_sample<float>(bank, bank_len, notes, s_lo, s_hi, size, S, j, q);
    });
    if (j > 0) {
        packed_real_mag_row<float, float2, true>(Z, tw, M, F, sqrt_n, scale, trow);
        return;
    }
    // fft_lds ended with a barrier: the other buffer (8 M bytes) is free and takes the F bin flags
    float2* buf0 = reinterpret_cast<float2*>(smem);
    unsigned* on = reinterpret_cast<unsigned*>(Z == buf0 ? buf0 + M : buf0);
    for (int k = tid; k < F; k += kThreads) on[k] = 0u;
    const int pw = 2 + 2 * npairs;
    int64_t moff = mask_files[2 * fi], P = mask_files[2 * fi + 1];
    const int64_t per = (int64_t)S * pw;
    if (moff < 0 || P < 0 || P > mask_len / per || moff > mask_len - P * per) P = 0;
    const int* tab = masks + (P > 0 ? moff : 0);
    // mag(mix) goes through the very loop that writes it into the file path's block (packed_real_mag_row<.., false>: the
    // compiler contracts that loop's unrolled pairs and its remainder differently, so only the loop itself gives the block's
    // bits), parked in instrument 0's output row: thread tid writes bins tid, tid + 256, .. there and reads back only those
    packed_real_mag_row<float, float2, false>(Z, tw, M, F, sqrt_n, scale, irow);
    __syncthreads();
    for (int64_t i = tid; i < S * P; i += kThreads) {
        const int* n = tab + i * pw;
        if (t < n[0] || t >= n[1]) continue;
        const unsigned bit = 1u << (int)(i / P);
        for (int k = 0; k < npairs; ++k) {
            const int f0 = max(n[2 + 2 * k], 0), f1 = min(n[3 + 2 * k], F);
            for (int f = f0; f < f1; ++f) atomicOr(&on[f], bit);
        }
    }
    __syncthreads();
    for (int k = tid; k <= M; k += kThreads) {
        const float mag = irow[k];
        // gather_score_kernel, operation for operation
        const unsigned m = on[k];
        float total = 0.f;
        for (int i = 0; i < S; ++i) {
            const float v = ((m >> i) & 1u) ? 1.0f : 1e-18f;
            total = i == 0 ? v : total + v;
        }
        const float x = scale * mag;
        for (int i = 0; i < S; ++i) {
            const float v = (((m >> i) & 1u) ? 1.0f : 1e-18f) / total;
            irow[i * plane + k] = v * x;
        }
    }
}

int64_t sum_counts(const int64_t* counts_h, int n_tracks) {
    int64_t n = 0;
    for (int s = 0; s < n_tracks; ++s) {
        if (counts_h[s] < 0 || counts_h[s] > 0x7fffffffLL - n) return -1;
        n += counts_h[s];
    }
    return n;
}

template <typename R, typename R2>
int score_render_file(dcs_stft* p, const R* win, const R2* tw, const R* bank_d, int64_t bank_len, int S, const int64_t* notes_h,
                      const int64_t* counts_h, int64_t size, R* out_d, int64_t ld, int64_t out_rows, int64_t* frames_h) {
    if (!p || !counts_h || (!bank_d && bank_len > 0))
        DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_score_render: null argument");
    if (S < 1 || S > kMaxTracks) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_score_render: %d tracks (1 .. 8)", S);
    if (bank_len < 0 || size < 0)
        DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_score_render: bank of %lld samples, size %lld", (long long)bank_len,
                 (long long)size);
    if (ld < p->frame / 2 + 1)
        DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_score_render: ld %lld < bins %d", (long long)ld, p->frame / 2 + 1);
    const int64_t n = sum_counts(counts_h, S);
    if (n < 0) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_score_render: a negative note count, or more than 2^31 - 1 notes");
    if (n > 0 && !notes_h) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_score_render: null note table");
    const int rs = DCS_SCORE_RENDER_ROW(S);
    // one block: the packed notes [n][4], then the file's descriptor [rs]
    std::vector<int64_t> tab((size_t)n * 4 + rs);
    DCS_CHECK(dcs_score_render_pack(notes_h, counts_h, S, bank_len, tab.data()));
    const int64_t T = dcs_frame_count(size, p->hop);
    int64_t* row = tab.data() + (size_t)n * 4;
    row[0] = size;
    row[1] = T;
    int64_t first = 0;
    for (int s = 0; s < S; ++s) {
        row[kFileHead + 2 * s] = first;
        row[kFileHead + 2 * s + 1] = counts_h[s];
        first += counts_h[s];
    }
    if (frames_h) *frames_h = T;
    if (!out_d) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_score_render: null output");
    if (out_rows < (1 + S) * T)
        DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_score_render: out_rows %lld < %lld", (long long)out_rows, (long long)((1 + S) * T));
    if (T > 0x7fffffffLL) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_score_render: %lld frames in one launch", (long long)T);
    DCS_ON_DEVICE(p->ctx->device);
    return with_own_table(p, tab, "stft.score_render_table", "dcs_stft_forward_score_render", "note", [&](const int64_t* notes_d) {
        return launch_frames(p, stft_score_render_kernel<R, R2, false>, T, S, win, tw, bank_d, bank_len, notes_d, (int)n,
                             notes_d + (size_t)n * 4, 1, S, (const int*)nullptr, 1, R(1), out_d, (R*)nullptr, ld);
    });
}

}  // namespace

DCS_API int dcs_score_render_pack(const int64_t* notes_h, const int64_t* counts_h, int n_tracks, int64_t bank_len,
                                  int64_t* packed_h) {
    if (!counts_h || n_tracks < 0) DCS_FAIL(DCS_EINVAL, "dcs_score_render_pack: null argument");
    const int64_t n = sum_counts(counts_h, n_tracks);
    if (n < 0) DCS_FAIL(DCS_EINVAL, "dcs_score_render_pack: a negative note count, or more than 2^31 - 1 notes");
    if (n > 0 && (!notes_h || !packed_h)) DCS_FAIL(DCS_EINVAL, "dcs_score_render_pack: null note table");
    if (bank_len < 0) DCS_FAIL(DCS_EINVAL, "dcs_score_render_pack: bank of %lld samples", (long long)bank_len);
    int64_t m = 0;
    for (int s = 0; s < n_tracks; ++s) {
        int64_t prev = 0, E = 0;
        for (int64_t i = 0; i < counts_h[s]; ++i, ++m) {
            const int64_t b = notes_h[3 * m], off = notes_h[3 * m + 1], len = notes_h[3 * m + 2];
            if (b < 0 || len < 0 || b > INT64_MAX - len)
                DCS_FAIL(DCS_EINVAL, "dcs_score_render_pack: note %lld of track %d begins at %lld with %lld samples", (long long)i,
                         s, (long long)b, (long long)len);
            if (off < 0 || off > bank_len || len > bank_len - off)
                DCS_FAIL(DCS_EINVAL, "dcs_score_render_pack: note %lld of track %d = [%lld, + %lld) reaches past the bank of %lld "
                         "samples", (long long)i, s, (long long)off, (long long)len, (long long)bank_len);
            if (b < prev)
                DCS_FAIL(DCS_EINVAL, "dcs_score_render_pack: note %lld of track %d begins at %lld, before its predecessor at %lld "
                         "(the notes of a track are ordered by their beginning)", (long long)i, s, (long long)b, (long long)prev);
            prev = b;
            if (b + len > E) E = b + len;
            packed_h[4 * m] = b;
            packed_h[4 * m + 1] = off;
            packed_h[4 * m + 2] = len;
            packed_h[4 * m + 3] = E;
        }
    }
    return DCS_OK;
}

DCS_API int dcs_stft_forward_score_render_f64(dcs_stft* p, const double* bank_d, int64_t bank_len, int S, const int64_t* notes_h,
                                              const int64_t* counts_h, int64_t size, double* out_d, int64_t ld, int64_t out_rows,
                                              int64_t* frames_h) {
    return score_render_file<double, double2>(p, p ? p->win_d : nullptr, p ? p->tw_d : nullptr, bank_d, bank_len, S, notes_h,
                                              counts_h, size, out_d, ld, out_rows, frames_h);
}

DCS_API int dcs_stft_forward_score_render_f32(dcs_stft* p, const float* bank_d, int64_t bank_len, int S, const int64_t* notes_h,
                                              const int64_t* counts_h, int64_t size, float* out_d, int64_t ld, int64_t out_rows,
                                              int64_t* frames_h) {
    return score_render_file<float, float2>(p, p ? p->win_f : nullptr, p ? p->tw_f : nullptr, bank_d, bank_len, S, notes_h,
                                            counts_h, size, out_d, ld, out_rows, frames_h);
}

DCS_API int dcs_trainer_gather_score_render(dcs_ctx* ctx, dcs_stft* p, const float* bank_d, int64_t bank_len,
                                            const int64_t* notes_d, int64_t n_notes, const int64_t* files_d, int n_files,
                                            const int* windows_d, int batch, int time_context, int S, float scale,
                                            float* inputs_d, float* targets_d) {
    if (!ctx || !p || !bank_d || !files_d || !windows_d || !inputs_d || !targets_d || (!notes_d && n_notes > 0))
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_score_render: null argument");
    if (p->ctx != ctx) DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_score_render: the plan belongs to another context");
    if (batch < 1 || time_context < 1 || S < 1 || S > kMaxTracks || n_files < 1 || bank_len < 1 || n_notes < 0 ||
        n_notes > 0x7fffffffLL)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_score_render: batch %d, time_context %d, S %d (1 .. 8), %d files, %lld notes, "
                 "bank of %lld samples", batch, time_context, S, n_files, (long long)n_notes, (long long)bank_len);
    if ((int64_t)batch * time_context > 0x7fffffffLL)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_score_render: %lld frames in one launch", (long long)batch * time_context);
    DCS_ON_DEVICE(ctx->device);
    return launch_frames(p, stft_score_render_kernel<float, float2, true>, (int64_t)batch * time_context, S, p->win_f, p->tw_f,
                         bank_d, bank_len, notes_d, (int)n_notes, files_d, n_files, S, windows_d, time_context, scale, inputs_d,
                         targets_d, (int64_t)(p->frame / 2 + 1));
}

DCS_API int dcs_trainer_gather_score_informed_render(dcs_ctx* ctx, dcs_stft* p, const float* bank_d, int64_t bank_len,
                                                     const int64_t* notes_d, int64_t n_notes, const int64_t* files_d,
                                                     int n_files, const int* masks_d, int64_t mask_len,
                                                     const int64_t* mask_files_d, int width, const int* windows_d, int batch,
                                                     int time_context, int S, float scale, float* inputs_d, float* targets_d) {
    if (!ctx || !p || !bank_d || !files_d || !masks_d || !mask_files_d || !windows_d || !inputs_d || !targets_d ||
        (!notes_d && n_notes > 0))
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_score_informed_render: null argument");
    if (p->ctx != ctx) DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_score_informed_render: the plan belongs to another context");
    if (batch < 1 || time_context < 1 || S < 1 || S > kMaxTracks || n_files < 1 || bank_len < 1 || n_notes < 0 ||
        n_notes > 0x7fffffffLL || mask_len < 0)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_score_informed_render: batch %d, time_context %d, S %d (1 .. 8), %d files, "
                 "%lld notes, bank of %lld samples, %lld mask ints", batch, time_context, S, n_files, (long long)n_notes,
                 (long long)bank_len, (long long)mask_len);
    const int npairs = (width - 3) / 2;
    // a packed mask note is (first frame, end frame) and npairs bands: width - 1 ints
    if (width < 5 || 2 * npairs + 2 != width - 1)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_score_informed_render: width %d (odd, from 5)", width);
    if ((int64_t)batch * time_context > 0x7fffffffLL)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_score_informed_render: %lld frames in one launch",
                 (long long)batch * time_context);
    DCS_ON_DEVICE(ctx->device);
    return launch_frames(p, stft_score_informed_kernel, (int64_t)batch * time_context, S, p->win_f, p->tw_f, bank_d, bank_len,
                         notes_d, (int)n_notes, files_d, n_files, S, masks_d, mask_len, mask_files_d, npairs, windows_d,
                         time_context, scale, inputs_d, targets_d);
}

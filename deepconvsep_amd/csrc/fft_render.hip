// Rendered forward STFT for gfx950: the augmented features of the hiphop (HHDS) trainers, computed from source audio
// resident on the device.
//
// Replaces util.circular_shift (util.py:62-81), the time-domain mixing and chunk slicing of
// examples/hiphopss/compute_features.py:55-85 and augmentations/compute_features_{cs,instr,mix}_aug.py, the float64 feature
// files they write (14 variants of every song for cs_aug) and LargeDataset reading them back (dataset.py:383-488).
//
// An augmented feature is a pure function of S mono signals and a few integers, so the variant is rendered inside the
// STFT's LOADER: one workgroup (256 threads) forms one windowed frame of one channel straight from the bank through three
// nested bounds -- chunk [a, a + Lc), rendered length `size`, source length L_s -- and transforms it with the FFT body of
// stft_forward_kernel (fft_lds.h: fft_lds, the packed real transform, mag = |X| / sqrt(N)).  Neither the rendered audio nor
// (for the feed) the feature block ever exists in memory.  This file holds the sample source (render_sample), the mapping
// of a workgroup to its frame and output row, and the entry points' checks; the frame itself, the feed's window decode, the
// launch and the life of the file path's own table are fft_frame.h, shared with fft_score_render.hip.
//
//   r_s[n] = g_s * x_s[n - k_s] if 0 <= n - k_s < L_s else 0 ;  mix[n] = m * (((r_0 + r_1) + r_2) + ...)
//
// The mixture is added in the time domain, in list order, without contraction into fused multiply-adds, in float32 as in
// float64: the float64 block then equals the existing kernel on host-rendered audio bit for bit, and the float32 feed does
// the arithmetic of the float32 STFT kernel on the float32 mixture.  A shift k_s of any parity is taken sample by sample
// (the loader's pair (p, p + 1) maps to (p - k_s, p + 1 - k_s) in the source: no alignment is assumed).
//
// Descriptor of a virtual file (DCS_RENDER_ROW(S) int64): size, a, Lc, T, then S x (offset, L_s, k_s, c_s); its gains
// (1 + S float64): m, g_0 .. g_{S-1}.  The file path builds one descriptor per chunk on the host (validated there); the
// feed reads a table the caller keeps on the device, so the kernel itself bounds every bank index and output channel.
#include "dcs_internal.h"
#include "fft_frame.h"

namespace {

constexpr int kHead = 4;   // size, a, Lc, T

// sample n (0 <= n < size) of rendered track s; x_s = bank[offset_s ..+ L_s)
template <typename R>
__device__ __forceinline__ R render_track(const R* __restrict__ bank, int64_t bank_len, const int64_t* __restrict__ tr, R g,
                                          int64_t n) {
#pragma clang fp contract(off)
    const int64_t i = n - tr[2];
    if (i < 0 || i >= tr[1]) return R(0);
    const int64_t bi = tr[0] + i;
    if (bi < 0 || bi >= bank_len) return R(0);
    return g * bank[bi];
}

// chunk-relative sample q of channel j (0: the mixture, 1 + s: track s)
template <typename R>
__device__ __forceinline__ R render_sample(const R* __restrict__ bank, int64_t bank_len, const int64_t* __restrict__ row,
                                           const double* __restrict__ gains, int S, int j, int64_t q) {
#pragma clang fp contract(off)
    const int64_t size = row[0], a = row[1], Lc = row[2];
    if (q < 0 || q >= Lc) return R(0);
    const int64_t n = a + q;
    if (n < 0 || n >= size) return R(0);
    if (j > 0) return render_track<R>(bank, bank_len, row + kHead + 4 * (j - 1), (R)gains[j], n);
    R acc = render_track<R>(bank, bank_len, row + kHead, (R)gains[1], n);
    for (int s = 1; s < S; ++s) acc = acc + render_track<R>(bank, bank_len, row + kHead + 4 * s, (R)gains[1 + s], n);
    return (R)gains[0] * acc;
}

// FEED = false: blockIdx.x = frame index over all chunks (descriptor c = the chunk with first[c] <= x < first[c + 1]),
//   output row ((1 + S) first[c] + ch T_c + t) of out0 [.., ld], padded to ld.
// FEED = true: blockIdx.x = b * tc + t of window b = (file, first frame); out0 = inputs [B][1][tc][F], out1 = targets
//   [B][S][tc][F], values times `scale`; zero rows for file < 0, file >= n_files and frames past T.
// blockIdx.y = j: 0 the mixture (channel 0), 1 + s track s (channel c_s).
template <typename R, typename R2, bool FEED>
__global__ __launch_bounds__(kThreads) void stft_render_kernel(
    const R* __restrict__ bank, int64_t bank_len, const int64_t* __restrict__ files, const double* __restrict__ gains_all,
    int n_files, int S, const int64_t* __restrict__ first, const int* __restrict__ windows, int tc, R scale,
    R* __restrict__ out0, R* __restrict__ out1, int64_t ld, const R* __restrict__ win, const R2* __restrict__ tw, int N, int hop,
    int log2m, R sqrt_n, int tw_lds) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int M = N >> 1;
    const int j = blockIdx.y;
    const int rs = kHead + 4 * S;
    FeedWindow w = {};
    if (FEED) {
        w = feed_window(windows, tc, n_files);
    } else {
        const int64_t g = blockIdx.x;
        w.fi = 0;
        while (w.fi + 1 < n_files && first[w.fi + 1] <= g) ++w.fi;
        w.t = g - first[w.fi];
        w.live = true;
    }
    const int64_t fi = w.fi, t = w.t;
    const bool live = w.live;
    const int64_t* row = files + (live ? fi : 0) * rs;
    const double* gains = gains_all + (live ? fi : 0) * (1 + S);
    const int64_t T = live ? row[3] : 0;
    int ch = 0;
    if (j > 0) {
        // channel of track j - 1; a dead window has no descriptor: its S target planes are zeroed in track order
        ch = live ? (int)row[kHead + 4 * (j - 1) + 3] : j;
        if (ch < 1 || ch > S) return;
    }
    R* orow = !FEED    ? out0 + ((1 + S) * first[fi] + (int64_t)ch * T + t) * ld
              : ch == 0 ? out0 + (w.b * tc + w.tt) * ld
                        : out1 + (((w.b * S + ch - 1) * tc) + w.tt) * ld;
    if (!live || t >= T) return zero_row(orow, ld);
    const int64_t base = t * (int64_t)hop - M;   // chunk-relative index of padded sample t * hop
    const R2* Z = render_frame<R, R2, false>(smem, win, tw, tw_lds, M, log2m, base, [&](int64_t q) {
        return render_sample<R>(bank, bank_len, row, gains, S, j, q);
    });
    packed_real_mag_row<R, R2, FEED>(Z, tw, M, ld, sqrt_n, scale, orow);
}

template <typename R, typename R2>
int render_file(dcs_stft* p, const R* win, const R2* tw, const R* bank_d, int64_t bank_len, int S, const int64_t* tracks_h,
                const double* gains_h, int64_t size, const int64_t* chunks_h, int n_chunks, R* out_d, int64_t ld,
                int64_t out_rows, int64_t* frames_h) {
    if (!p || !tracks_h || !gains_h || (!chunks_h && n_chunks > 0) || (!bank_d && bank_len > 0))
        DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_render: null argument");
    if (S < 1 || S > 8) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_render: %d tracks (1 .. 8)", S);
    if (bank_len < 0 || size < 0 || n_chunks < 0)
        DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_render: bank of %lld samples, size %lld, %d chunks", (long long)bank_len,
                 (long long)size, n_chunks);
    if (ld < p->frame / 2 + 1) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_render: ld %lld < bins %d", (long long)ld, p->frame / 2 + 1);
    unsigned seen = 0;
    for (int s = 0; s < S; ++s) {
        const int64_t off = tracks_h[4 * s], L = tracks_h[4 * s + 1], c = tracks_h[4 * s + 3];
        if (off < 0 || L < 0 || off > bank_len || L > bank_len - off)
            DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_render: track %d = [%lld, + %lld) reaches past the bank of %lld samples", s,
                     (long long)off, (long long)L, (long long)bank_len);
        if (c < 1 || c > S || (seen >> c & 1))
            DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_render: track %d has output channel %lld (1 .. %d, each once)", s,
                     (long long)c, S);
        seen |= 1u << c;
    }
    const int rs = DCS_RENDER_ROW(S);
    // one block: descriptors [n_chunks][rs] int64, first frame of each chunk [n_chunks + 1] int64, gains [n_chunks][1 + S] f64
    std::vector<int64_t> tab((size_t)n_chunks * rs + n_chunks + 1 + (size_t)n_chunks * (1 + S));
    int64_t* first = tab.data() + (size_t)n_chunks * rs;
    double* gains = reinterpret_cast<double*>(first + n_chunks + 1);
    int64_t total = 0;
    for (int c = 0; c < n_chunks; ++c) {
        const int64_t a = chunks_h[2 * c], Lc = chunks_h[2 * c + 1];
        if (a < 0 || Lc < 0 || a > size || Lc > size - a)
            DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_render: chunk %d = [%lld, + %lld) reaches past the rendered length %lld", c,
                     (long long)a, (long long)Lc, (long long)size);
        const int64_t T = dcs_frame_count(Lc, p->hop);
        int64_t* row = tab.data() + (size_t)c * rs;
        row[0] = size; row[1] = a; row[2] = Lc; row[3] = T;
        for (int i = 0; i < 4 * S; ++i) row[kHead + i] = tracks_h[i];
        for (int i = 0; i <= S; ++i) gains[(size_t)c * (1 + S) + i] = gains_h[i];
        first[c] = total;
        total += T;
        if (frames_h) frames_h[c] = T;
    }
    first[n_chunks] = total;
    if (n_chunks == 0) return DCS_OK;
    if (!out_d) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_render: null output");
    if (out_rows < (1 + S) * total)
        DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_render: out_rows %lld < %lld", (long long)out_rows, (long long)((1 + S) * total));
    if (total > 0x7fffffffLL) DCS_FAIL(DCS_EINVAL, "dcs_stft_forward_render: %lld frames in one launch", (long long)total);
    DCS_ON_DEVICE(p->ctx->device);
    return with_own_table(p, tab, "stft.render_table", "dcs_stft_forward_render", "chunk", [&](const int64_t* files_d) {
        const int64_t* first_d = files_d + (size_t)n_chunks * rs;
        return launch_frames(p, stft_render_kernel<R, R2, false>, total, S, win, tw, bank_d, bank_len, files_d,
                             (const double*)(first_d + n_chunks + 1), n_chunks, S, first_d, (const int*)nullptr, 1, R(1), out_d,
                             (R*)nullptr, ld);
    });
}

}  // namespace

DCS_API int dcs_stft_forward_render_f64(dcs_stft* p, const double* bank_d, int64_t bank_len, int S, const int64_t* tracks_h,
                                        const double* gains_h, int64_t size, const int64_t* chunks_h, int n_chunks,
                                        double* out_d, int64_t ld, int64_t out_rows, int64_t* frames_h) {
    return render_file<double, double2>(p, p ? p->win_d : nullptr, p ? p->tw_d : nullptr, bank_d, bank_len, S, tracks_h, gains_h,
                                        size, chunks_h, n_chunks, out_d, ld, out_rows, frames_h);
}

DCS_API int dcs_stft_forward_render_f32(dcs_stft* p, const float* bank_d, int64_t bank_len, int S, const int64_t* tracks_h,
                                        const double* gains_h, int64_t size, const int64_t* chunks_h, int n_chunks, float* out_d,
                                        int64_t ld, int64_t out_rows, int64_t* frames_h) {
    return render_file<float, float2>(p, p ? p->win_f : nullptr, p ? p->tw_f : nullptr, bank_d, bank_len, S, tracks_h, gains_h,
                                      size, chunks_h, n_chunks, out_d, ld, out_rows, frames_h);
}

DCS_API int dcs_trainer_gather_render(dcs_ctx* ctx, dcs_stft* p, const float* bank_d, int64_t bank_len, const int64_t* files_d,
                                      const double* gains_d, int n_files, const int* windows_d, int batch, int time_context,
                                      int S, float scale, float* inputs_d, float* targets_d) {
    if (!ctx || !p || !bank_d || !files_d || !gains_d || !windows_d || !inputs_d || !targets_d)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_render: null argument");
    if (p->ctx != ctx) DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_render: the plan belongs to another context");
    if (batch < 1 || time_context < 1 || S < 1 || S > 8 || n_files < 1 || bank_len < 1)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_render: batch %d, time_context %d, S %d (1 .. 8), %d files, bank of %lld samples",
                 batch, time_context, S, n_files, (long long)bank_len);
    if ((int64_t)batch * time_context > 0x7fffffffLL)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_render: %lld frames in one launch", (long long)batch * time_context);
    DCS_ON_DEVICE(ctx->device);
    return launch_frames(p, stft_render_kernel<float, float2, true>, (int64_t)batch * time_context, S, p->win_f, p->tw_f, bank_d,
                         bank_len, files_d, gains_d, n_files, S, (const int64_t*)nullptr, windows_d, time_context, scale,
                         inputs_d, targets_d, (int64_t)(p->frame / 2 + 1));
}

// dcs_mask_fold_apply: the soft masks of a single-channel network, cross-faded over the tiles, applied to the magnitudes of
// every input channel (include/dcs.h has the contract; DESIGN.md section 4o2 the bytes).
//
// mask_ola_kernel (generic.hip) folds mask x mixture and never forms the masks; here the fold runs on the masks themselves
//   m_s[k][j][f] = mask_kernel's expression on p[s][k][j][f]              (separate_dsd.py:258-271, separate_bach10.py:251-264)
//   acc_s[t][f]  = overlap_add_kernel's fold of m_s over the tiles that cover frame t                      (util.py:297-327)
//   est[c][s][t][f] = acc_s[t][f] * mag[c][t][f]
// so that a stereo file keeps one estimate per channel, each with its own magnitude (and, at the iSTFT, its own phase).
// One thread per (frame, bin), coalesced along the bins; the tiles that cover a frame are the same for the whole workgroup.
// Each (tile, frame, bin) of p is read exactly once, nothing is accumulated across threads: the same bits every run.
#include "dcs_internal.h"
#include "chanmask.h"       // soft_masks: the masks of one tile position

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSources = 8;
constexpr int kMaxChannels = 8;

struct ChanMaskArgs {
    const float* p;           // [S][n][tc][F], source stride p_src_stride
    int64_t p_src_stride, n;
    int S, tc, ov, F, mode;
    const float* rise;        // [ov]
    const float* mag;         // [C][T, ld]
    int64_t mag_ch_stride;
    int C;
    int64_t ld;
    float* est;               // [C][S][T, ld] or null
    int64_t est_ch_stride, est_src_stride;
    float* mask;              // [S][T, ld] or null
    int64_t mask_src_stride;
};

// MM > 0: a frame is covered by at most MM tiles and S == SS; all MM x SS values of p and the C magnitudes are requested
// before the first is used (see mask_ola_kernel).  MM == 0: any tile count, any S <= 8, one tile after the other.
template <int MM, int SS>
__global__ __launch_bounds__(kThreads) void mask_fold_apply_kernel(ChanMaskArgs a) {
    constexpr int SA = MM > 0 ? SS : kMaxSources;
    const int S = MM > 0 ? SS : a.S;
    const int f = blockIdx.y * kThreads + threadIdx.x;
    if (f >= a.F) return;
    const int64_t t = blockIdx.x;
    const int tc = a.tc, ov = a.ov, st = tc - ov, F = a.F;
    const int64_t n = a.n;
    int64_t k0 = (t < ov) ? 0 : (t - ov) / st;
    if (k0 > n - 1) k0 = n - 1;
    const int64_t j0 = (n > 0) ? t - k0 * st : tc;
    const int64_t row = t * a.ld + f;

    float mg[kMaxChannels];
#pragma unroll
    for (int c = 0; c < kMaxChannels; ++c) mg[c] = (a.est && c < a.C) ? a.mag[c * a.mag_ch_stride + row] : 0.f;

    float acc[SA];
#pragma unroll
    for (int s = 0; s < SA; ++s) acc[s] = 0.f;
    if (j0 < tc) {                                       // else: past the last tile, the zeros of util.py:313
        if (MM > 0) {
            constexpr int MA = MM > 0 ? MM : 1;
            float v[MA][SA];
            bool valid[MA];
#pragma unroll
            for (int m = 0; m < MM; ++m) {
                const int64_t k = k0 + m;
                valid[m] = k < n && k * st <= t;                       // workgroup-uniform
                const int64_t kc = valid[m] ? k : k0;                  // clamped: every load is issued, none sits behind a branch
                const int64_t r = (kc * tc + (t - kc * st)) * F + f;
#pragma unroll
                for (int s = 0; s < SA; ++s) v[m][s] = a.p[s * a.p_src_stride + r];
            }
#pragma unroll
            for (int m = 0; m < MM; ++m) {
                if (!valid[m]) continue;
                soft_masks<SA>(v[m], S, a.mode);
                if (m == 0) {
#pragma unroll
                    for (int s = 0; s < SA; ++s) acc[s] = v[m][s];
                } else {
                    const int j = (int)(t - (k0 + m) * st);
                    const float down = a.rise[ov - 1 - j], up = a.rise[j];
#pragma unroll
                    for (int s = 0; s < SA; ++s) acc[s] = fmaf(down, acc[s], __fmul_rn(up, v[m][s]));   // one explicit form: see overlap_add_kernel
                }
            }
        } else {
            for (int64_t k = k0; k < n && k * st <= t; ++k) {
                const int j = (int)(t - k * st);
                const int64_t r = (k * tc + j) * F + f;
                float p[SA];
#pragma unroll
                for (int s = 0; s < SA; ++s) p[s] = s < S ? a.p[s * a.p_src_stride + r] : 0.f;
                soft_masks<SA>(p, S, a.mode);
                if (k == k0) {
#pragma unroll
                    for (int s = 0; s < SA; ++s) acc[s] = p[s];
                } else {
                    const float down = a.rise[ov - 1 - j], up = a.rise[j];
#pragma unroll
                    for (int s = 0; s < SA; ++s) acc[s] = fmaf(down, acc[s], __fmul_rn(up, p[s]));   // one explicit form: see overlap_add_kernel
                }
            }
        }
    }
    if (a.mask) {
#pragma unroll
        for (int s = 0; s < SA; ++s)
            if (s < S) a.mask[s * a.mask_src_stride + row] = acc[s];
    }
    if (a.est) {
#pragma unroll
        for (int c = 0; c < kMaxChannels; ++c)
            if (c < a.C) {
#pragma unroll
                for (int s = 0; s < SA; ++s)
                    if (s < S) a.est[c * a.est_ch_stride + s * a.est_src_stride + row] = __fmul_rn(acc[s], mg[c]);
            }
    }
}

}  // namespace

extern "C" int dcs_mask_fold_apply(dcs_ctx* ctx, const float* p_d, int64_t p_src_stride, int64_t n_tiles, int S, int time_context,
                                   int overlap, int F, int eps_mode, const double* rise_h, const float* mag_d,
                                   int64_t mag_ch_stride, int C, int64_t n_frames, int64_t ld, float* est_d,
                                   int64_t est_ch_stride, int64_t est_src_stride, float* mask_d, int64_t mask_src_stride) {
    if (!ctx) DCS_FAIL(DCS_EINVAL, "dcs_mask_fold_apply: null ctx");
    if (S < 1 || S > kMaxSources) DCS_FAIL(DCS_EINVAL, "dcs_mask_fold_apply: %d sources (1 .. %d)", S, kMaxSources);
    if (C < 1 || C > kMaxChannels) DCS_FAIL(DCS_EINVAL, "dcs_mask_fold_apply: %d channels (1 .. %d)", C, kMaxChannels);
    if (overlap < 1 || overlap >= time_context)
        DCS_FAIL(DCS_EINVAL, "dcs_mask_fold_apply: overlap %d not in [1, %d)", overlap, time_context);
    if (F < 1 || ld < F || n_tiles < 0 || n_frames < 0)
        DCS_FAIL(DCS_EINVAL, "dcs_mask_fold_apply: bad shape (F %d, ld %lld, n_tiles %lld, n_frames %lld)", F, (long long)ld,
                 (long long)n_tiles, (long long)n_frames);
    if (eps_mode != DCS_EPS_A && eps_mode != DCS_EPS_B) DCS_FAIL(DCS_EINVAL, "dcs_mask_fold_apply: bad eps_mode");
    if (!p_d || !mag_d || !rise_h) DCS_FAIL(DCS_EINVAL, "dcs_mask_fold_apply: null input");
    if (!est_d && !mask_d) DCS_FAIL(DCS_EINVAL, "dcs_mask_fold_apply: neither the estimates nor the masks are asked for");
    if (n_frames > 0x7fffffffLL) DCS_FAIL(DCS_EUNSUPPORTED, "dcs_mask_fold_apply: %lld frames in one call", (long long)n_frames);
    if (n_frames == 0) return DCS_OK;
    DCS_ON_DEVICE(ctx->device);
    DCS_CHECK(dcs_ctx_ola_rise(ctx, rise_h, overlap));

    ChanMaskArgs a;
    a.p = p_d; a.p_src_stride = p_src_stride; a.n = n_tiles;
    a.S = S; a.tc = time_context; a.ov = overlap; a.F = F; a.mode = eps_mode;
    a.rise = ctx->ola_rise_d;
    a.mag = mag_d; a.mag_ch_stride = mag_ch_stride; a.C = C; a.ld = ld;
    a.est = est_d; a.est_ch_stride = est_ch_stride; a.est_src_stride = est_src_stride;
    a.mask = mask_d; a.mask_src_stride = mask_src_stride;

    const int st = time_context - overlap;
    const int mmax = (overlap + st - 1) / st + 1;            // tiles that can reach one frame
    const dim3 grid((unsigned)n_frames, (unsigned)dcs_cdiv(F, kThreads));
    DcsTimer tm(ctx, DCS_TAG_MASK);
#define DCS_CHANMASK(MM_, SS_) hipLaunchKernelGGL((mask_fold_apply_kernel<MM_, SS_>), grid, dim3(kThreads), 0, ctx->stream, a)
    if (S == 4 && mmax <= 3) DCS_CHANMASK(3, 4);
    else if (S == 4 && mmax <= 6) DCS_CHANMASK(6, 4);
    else if (S == 2 && mmax <= 3) DCS_CHANMASK(3, 2);
    else if (S == 2 && mmax <= 6) DCS_CHANMASK(6, 2);
    else DCS_CHANMASK(0, 0);
#undef DCS_CHANMASK
    tm.done();
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

// BSS Eval v3 (bss_eval_sources / bss_eval_images and the framewise driver of DSD100_eval_only.m) as energies, float64.
//
// One *problem* is a window (or a whole signal) of R = nsrc_ref * nchan reference channels r_k and M = nsrc_est * nchan
// estimate channels e_m, all zero outside [0, T).  Every criterion follows from five energies per (estimate channel,
// true source) (DESIGN.md "BSS Eval"); the projections onto the spans of the delayed references come from a partial
// Cholesky factorisation of the Gram matrix, never from time signals.
//
//   (a) lag correlations c_{k,n}(d) = sum_t r_k(t + d) z_n(t), d in (-L, L), z = [r; e]: bss_corr_partial_kernel
//       (workgroup = (reference k, 1024 lags, 16 signals, T-segment, window); f64 FMA, the reference segment staged in
//       LDS with its lag halo) writes per-segment sums, bss_corr_reduce_kernel adds the segments in order.
//   (b) per window one full problem (all R channels) and one per source (its nchan channels): the matrix
//       [G | D] with G[(k1,a),(k2,b)] = c_{k1,k2}(b - a) and D[(k,a),m] = c_{k,m}(-a), rows padded to a multiple of 64
//       (padding rows are zero, so the pivot rule skips them), 64 D columns of which M are used: bss_assemble_kernel.
//   (c) right-looking blocked U^T U factorisation of G, 64 rows per step, batched over the problems of a window group:
//       bss_panel_kernel factors the 64 x 64 diagonal block (every workgroup of the step the same way, so they agree
//       bit for bit) and solves U11^T X = A12 for its column block (D included: X = the projected coordinates Y);
//       bss_update_kernel subtracts U12^T U12 from the trailing upper triangle (and U12^T Y from the D rows).
//       A pivot <= N * eps * max(diag G) drops its row: the projection is onto the span actually there.
//       ||P e_m||^2 = ||Y_m||^2 (bss_colnorm_kernel); no back substitution, no time-domain synthesis.
// Every reduction runs in a fixed order (no atomics): two runs are bit-identical.
#include "bsseval.h"

#include <float.h>
#include <math.h>

#include <algorithm>

namespace {

constexpr int kCT = 256;        // samples per LDS chunk of the correlation
constexpr int kLagBlk = 1024;   // lags per correlation workgroup: 2 waves x 64 lanes x 8 (stride 64)
constexpr int kNBlk = 16;       // signals per correlation workgroup: 2 waves x 8
constexpr int kNb = 64;         // Cholesky block
constexpr int kDCols = 64;      // D columns per problem (M <= 16 used, the rest zero)

struct CorrArgs {
    const double* ref;   // [R][nsampl]
    const double* est;   // [M][nsampl]
    int64_t nsampl, win, hop, w0;
    int R, Nz, L, nlag;
    int nseg;
    int64_t tseg;
    double* partial;     // [nw][nseg][R][Nz][nlag]
};

__device__ __forceinline__ double signal_at(const CorrArgs& a, int n, int64_t off, int64_t t) {
    return n < a.R ? a.ref[(int64_t)n * a.nsampl + off + t] : a.est[(int64_t)(n - a.R) * a.nsampl + off + t];
}

__global__ __launch_bounds__(256) void bss_corr_partial_kernel(CorrArgs a) {
    __shared__ double zs[kNBlk][kCT];
    __shared__ double rs[kCT + kLagBlk];
    const int seg = blockIdx.x;
    const int nlb = (a.nlag + kLagBlk - 1) / kLagBlk;
    const int nnb = (a.Nz + kNBlk - 1) / kNBlk;
    int y = blockIdx.y;
    const int lbi = y % nlb;
    y /= nlb;
    const int nbi = y % nnb;
    const int k = y / nnb;
    const int wl = blockIdx.z;
    const int64_t off = (a.w0 + wl) * a.hop;
    const int lb = lbi * kLagBlk;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int h = wv & 1, g = wv >> 1;
    const int n0 = nbi * kNBlk + g * 8;
    const bool active = n0 < a.Nz && lb + h * 512 < a.nlag;   // wave-uniform
    const int64_t t_begin = (int64_t)seg * a.tseg;
    const int64_t t_end = min(a.win, t_begin + a.tseg);
    double acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[i][q] = 0.0;
    for (int64_t t0 = t_begin; t0 < t_end; t0 += kCT) {
        __syncthreads();
        for (int idx = tid; idx < kNBlk * kCT; idx += 256) {
            const int q = idx / kCT, tt = idx % kCT;
            const int n = nbi * kNBlk + q;
            const int64_t t = t0 + tt;
            zs[q][tt] = (n < a.Nz && t < t_end) ? signal_at(a, n, off, t) : 0.0;
        }
        // rs[p] = r_k(t0 + lb - (L - 1) + p): the reference is zero outside [0, win) of its window
        for (int p = tid; p < kCT + kLagBlk - 1; p += 256) {
            const int64_t t = t0 + lb - (a.L - 1) + p;
            rs[p] = (t >= 0 && t < a.win) ? a.ref[(int64_t)k * a.nsampl + off + t] : 0.0;
        }
        __syncthreads();
        if (active) {
            const double* rp = rs + h * 512 + lane;
#pragma unroll 2
            for (int tt = 0; tt < kCT; ++tt) {
                double zv[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) zv[q] = zs[g * 8 + q][tt];
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const double rv = rp[tt + 64 * i];
#pragma unroll
                    for (int q = 0; q < 8; ++q) acc[i][q] = fma(rv, zv[q], acc[i][q]);
                }
            }
        }
    }
    if (n0 >= a.Nz) return;
    double* out = a.partial + (((int64_t)wl * a.nseg + seg) * a.R + k) * (int64_t)a.Nz * a.nlag;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int n = n0 + q;
        if (n >= a.Nz) break;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int l = lb + h * 512 + lane + 64 * i;
            if (l < a.nlag) out[(int64_t)n * a.nlag + l] = acc[i][q];
        }
    }
}

// C[w][k][n][l] = sum over the segments, in segment order
__global__ __launch_bounds__(256) void bss_corr_reduce_kernel(const double* __restrict__ partial, int nseg, int64_t per_seg,
                                                              int64_t total, double* __restrict__ C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int64_t w = i / per_seg, r = i % per_seg;
    const double* p = partial + w * nseg * per_seg + r;
    double s = 0.0;
    for (int g = 0; g < nseg; ++g) s += p[(int64_t)g * per_seg];
    C[i] = s;
}

// out[blockIdx.x] = sum_t x[t]^2 over one window of one channel (fixed-order tree)
__global__ __launch_bounds__(256) void bss_sqnorm_kernel(const double* __restrict__ est, int64_t nsampl, int64_t win,
                                                         int64_t hop, int64_t w0, int M, double* __restrict__ out) {
    __shared__ double red[256];
    const int m = blockIdx.x % M, wl = blockIdx.x / M;
    const double* x = est + (int64_t)m * nsampl + (w0 + wl) * hop;
    double s = 0.0;
    for (int64_t t = threadIdx.x; t < win; t += 256) s = fma(x[t], x[t], s);
    red[threadIdx.x] = s;
    for (int w = 128; w > 0; w >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    }
    if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// ------------------------------------------------------------------------------------------------ problems of a group
// Per window: problem 0 = all R channels, problem 1 + j = the nchan channels of source j.  W of a problem: npad rows,
// ld = npad + kDCols columns, row-major.
struct Geom {
    int R, M, Nz, L, nlag, nchan, nsrc;
    int npad_full, npad_src;
    int64_t w_full, w_src, w_per;   // doubles of one W, of one window's W set
    int ppw;                        // problems per window
    double* W;
    const double* C;                // [nw][R][Nz][nlag]
};

struct Prob {
    int wl, ch0, nch, npad;
    int64_t ld;
    double* W;
};

__device__ __forceinline__ Prob problem(const Geom& g, int p) {
    Prob q;
    q.wl = p / g.ppw;
    const int s = p % g.ppw;
    double* base = g.W + (int64_t)q.wl * g.w_per;
    if (s == 0) {
        q.ch0 = 0;
        q.nch = g.R;
        q.npad = g.npad_full;
        q.W = base;
    } else {
        q.ch0 = (s - 1) * g.nchan;
        q.nch = g.nchan;
        q.npad = g.npad_src;
        q.W = base + g.w_full + (int64_t)(s - 1) * g.w_src;
    }
    q.ld = q.npad + kDCols;
    return q;
}

__device__ __forceinline__ double corr(const Geom& g, int wl, int k, int n, int d) {
    return g.C[(((int64_t)wl * g.R + k) * g.Nz + n) * g.nlag + d + g.L - 1];
}

// every element of every W: grid (column chunks of 256, row, problem)
__global__ __launch_bounds__(256) void bss_assemble_kernel(Geom g) {
    const Prob q = problem(g, blockIdx.z);
    const int i = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= q.npad || j >= q.ld) return;
    const int N = q.nch * g.L;
    double v = 0.0;
    if (i < N) {
        const int k1 = i / g.L, a = i % g.L;
        if (j < N) {
            const int k2 = (int)j / g.L, b = (int)j % g.L;
            v = corr(g, q.wl, q.ch0 + k1, q.ch0 + k2, b - a);
        } else if (j >= q.npad && j - q.npad < g.M) {
            v = corr(g, q.wl, q.ch0 + k1, g.R + (int)(j - q.npad), -a);
        }
    }
    q.W[(int64_t)i * q.ld + j] = v;
}

// pivot threshold of a problem: N * eps * max(diag G), diag G = c_{k,k}(0)
__device__ double pivot_tol(const Geom& g, const Prob& q) {
    double mx = 0.0;
    for (int c = 0; c < q.nch; ++c) mx = fmax(mx, corr(g, q.wl, q.ch0 + c, q.ch0 + c, 0));
    return (double)(q.nch * g.L) * DBL_EPSILON * mx;
}

// step kb: factor the diagonal block, solve the block row for column block kb + 1 + blockIdx.x
__global__ __launch_bounds__(256) void bss_panel_kernel(Geom g, int kb) {
    __shared__ double U[kNb][kNb + 1];
    __shared__ double X[kNb][kNb + 1];
    __shared__ double s_piv, s_tol;
    const Prob q = problem(g, blockIdx.y);
    const int ncb = q.npad / kNb + 1;   // + the D block
    const int cb = kb + 1 + blockIdx.x;
    if (kb * kNb >= q.npad || cb >= ncb) return;
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)kb * kNb;
    for (int idx = tid; idx < kNb * kNb; idx += 256) {
        const int r = idx / kNb, c = idx % kNb;
        U[r][c] = q.W[(r0 + r) * q.ld + r0 + c];
        X[r][c] = q.W[(r0 + r) * q.ld + (int64_t)cb * kNb + c];
    }
    if (tid == 0) s_tol = pivot_tol(g, q);
    // unblocked U^T U of the upper triangle, rows whose pivot is <= tol zeroed
    for (int i = 0; i < kNb; ++i) {
        __syncthreads();
        if (tid == 0) {
            const double d = U[i][i];
            s_piv = d > s_tol ? sqrt(d) : 0.0;
        }
        __syncthreads();
        const double piv = s_piv;
        if (tid >= i && tid < kNb) U[i][tid] = piv > 0.0 ? (tid == i ? piv : U[i][tid] / piv) : 0.0;
        __syncthreads();
        const int n = kNb - 1 - i;
        for (int idx = tid; idx < n * n; idx += 256) {
            const int r = i + 1 + idx / n, c = i + 1 + idx % n;
            if (c >= r) U[r][c] = fma(-U[i][r], U[i][c], U[r][c]);
        }
    }
    __syncthreads();
    // U11^T X = A12, column by column (a zero pivot gives a zero row of X)
    if (tid < kNb) {
        for (int i = 0; i < kNb; ++i) {
            double acc = X[i][tid];
            for (int r = 0; r < i; ++r) acc = fma(-U[r][i], X[r][tid], acc);
            X[i][tid] = U[i][i] > 0.0 ? acc / U[i][i] : 0.0;
        }
    }
    __syncthreads();
    for (int idx = tid; idx < kNb * kNb; idx += 256) {
        const int r = idx / kNb, c = idx % kNb;
        q.W[(r0 + r) * q.ld + (int64_t)cb * kNb + c] = X[r][c];
    }
}

// step kb: W[i][j] -= sum_r W[r][i] W[r][j] over the 64 rows r of block kb, tiles (ti, tj), kb < ti <= tj
__global__ __launch_bounds__(256) void bss_update_kernel(Geom g, int kb) {
    __shared__ double Ui[32][kNb + 1];
    __shared__ double Uj[32][kNb + 1];
    const Prob q = problem(g, blockIdx.z);
    const int nrb = q.npad / kNb;        // row blocks
    const int ti = kb + 1 + blockIdx.y;
    const int tj = kb + 1 + blockIdx.x;
    if (ti >= nrb || tj > nrb || tj < ti) return;   // tj == nrb: the D block
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int64_t r0 = (int64_t)kb * kNb;
    const int64_t ci = (int64_t)ti * kNb, cj = (int64_t)tj * kNb;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = q.W[(ci + ty + 16 * a) * q.ld + cj + tx + 16 * b];
    for (int half = 0; half < 2; ++half) {
        __syncthreads();
        for (int idx = tid; idx < 32 * kNb; idx += 256) {
            const int r = idx / kNb, c = idx % kNb;
            const int64_t row = (r0 + half * 32 + r) * q.ld;
            Ui[r][c] = q.W[row + ci + c];
            Uj[r][c] = q.W[row + cj + c];
        }
        __syncthreads();
        for (int r = 0; r < 32; ++r) {
            double u[4], v[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) u[a] = Ui[r][ty + 16 * a];
#pragma unroll
            for (int b = 0; b < 4; ++b) v[b] = Uj[r][tx + 16 * b];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(-u[a], v[b], acc[a][b]);
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) q.W[(ci + ty + 16 * a) * q.ld + cj + tx + 16 * b] = acc[a][b];
}

// ynorm[p][m] = sum over the rows of Y_m^2 = ||P e_m||^2 on the span of problem p (fixed-order tree)
__global__ __launch_bounds__(256) void bss_colnorm_kernel(Geom g, double* __restrict__ ynorm) {
    __shared__ double red[256];
    const int p = blockIdx.y, m = blockIdx.x;
    const Prob q = problem(g, p);
    double s = 0.0;
    for (int r = threadIdx.x; r < q.npad; r += 256) {
        const double y = q.W[(int64_t)r * q.ld + q.npad + m];
        s = fma(y, y, s);
    }
    red[threadIdx.x] = s;
    for (int w = 128; w > 0; w >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    }
    if (threadIdx.x == 0) ynorm[(int64_t)p * g.M + m] = red[0];
}

// the five energies per (window, jest, jtrue, channel)
__global__ __launch_bounds__(256) void bss_energies_kernel(Geom g, const double* __restrict__ enorm,
                                                           const double* __restrict__ ynorm, int nsrc_est, int nw,
                                                           int all_pairs, double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int per_w = nsrc_est * (all_pairs ? g.nsrc : 1) * g.nchan;
    if (idx >= (int64_t)nw * per_w) return;
    const int wl = (int)(idx / per_w);
    int r = (int)(idx % per_w);
    const int i = r % g.nchan;
    r /= g.nchan;
    int jest, jtrue;
    if (all_pairs) {
        jtrue = r % g.nsrc;
        jest = r / g.nsrc;
    } else {
        jest = jtrue = r;
    }
    const int m = jest * g.nchan + i, k = jtrue * g.nchan + i;
    const double e2 = enorm[(int64_t)wl * g.M + m];
    const double pall = ynorm[((int64_t)wl * g.ppw) * g.M + m];
    double* o = out + idx * 5;
    o[0] = e2;
    o[1] = corr(g, wl, k, k, 0);
    o[2] = corr(g, wl, k, g.R + m, 0);
    o[3] = ynorm[((int64_t)wl * g.ppw + 1 + jtrue) * g.M + m];
    o[4] = fmax(e2 - pall, 0.0);
}

struct Layout {
    int R, M, Nz, L, nlag, nseg, nw;
    int64_t tseg;
    size_t partial, C;   // doubles
};

Layout corr_layout(int R, int M, int L, int64_t win, int nw) {
    Layout s;
    s.R = R;
    s.M = M;
    s.Nz = R + M;
    s.L = L;
    s.nlag = 2 * L - 1;
    s.nw = nw;
    // at most 512 segments of at least 64 chunks: enough workgroups for one window, bounded partial sums for long signals
    s.tseg = dcs_round_up(std::max<int64_t>(64 * kCT, (win + 511) / 512), kCT);
    s.nseg = dcs_cdiv(win, s.tseg);
    s.C = (size_t)nw * R * s.Nz * s.nlag;
    s.partial = s.C * s.nseg;
    return s;
}

// stage (a) for windows [w0, w0 + nw): C (device, [nw][R][Nz][nlag]) and, when enorm != nullptr, ||e_m||^2
int launch_corr(dcs_ctx* ctx, const Layout& s, const double* ref, const double* est, int64_t nsampl, int64_t win,
                int64_t hop, int64_t w0, double* partial, double* C, double* enorm) {
    CorrArgs a;
    a.ref = ref;
    a.est = est;
    a.nsampl = nsampl;
    a.win = win;
    a.hop = hop;
    a.w0 = w0;
    a.R = s.R;
    a.Nz = s.Nz;
    a.L = s.L;
    a.nlag = s.nlag;
    a.nseg = s.nseg;
    a.tseg = s.tseg;
    a.partial = partial;
    const int nlb = dcs_cdiv(s.nlag, kLagBlk), nnb = dcs_cdiv(s.Nz, kNBlk);
    hipLaunchKernelGGL(bss_corr_partial_kernel, dim3(s.nseg, s.R * nnb * nlb, s.nw), dim3(256), 0, ctx->stream, a);
    DCS_HIP(hipGetLastError());
    const int64_t per_seg = (int64_t)s.R * s.Nz * s.nlag;
    const int64_t total = per_seg * s.nw;
    hipLaunchKernelGGL(bss_corr_reduce_kernel, dim3(dcs_cdiv(total, 256)), dim3(256), 0, ctx->stream, partial, s.nseg,
                       per_seg, total, C);
    DCS_HIP(hipGetLastError());
    if (enorm) {
        hipLaunchKernelGGL(bss_sqnorm_kernel, dim3(s.nw * s.M), dim3(256), 0, ctx->stream, est, nsampl, win, hop, w0, s.M,
                           enorm);
        DCS_HIP(hipGetLastError());
    }
    return DCS_OK;
}

constexpr size_t kScratchBudget = size_t(3) << 30;   // bytes of scratch one call may hold (window groups beyond)

size_t align_doubles(size_t n) { return (n + 31) / 32 * 32; }

}  // namespace

extern "C" int dcs_bss_lagcorr(dcs_ctx* ctx, const double* ref_d, const double* est_d, int n_ref, int n_est,
                               int64_t n_samples, int flen, double* out_d) {
    if (!ctx) DCS_FAIL(DCS_EINVAL, "dcs_bss_lagcorr: null ctx");
    if (n_ref < 1 || n_est < 0 || n_samples < 1 || !ref_d || !out_d || (n_est > 0 && !est_d))
        DCS_FAIL(DCS_EINVAL, "dcs_bss_lagcorr: bad argument (n_ref %d, n_est %d, n_samples %lld)", n_ref, n_est,
                 (long long)n_samples);
    if (flen < 16 || flen > 512 || flen % 16)
        DCS_FAIL(DCS_EINVAL, "dcs_bss_lagcorr: flen %d is not a multiple of 16 in [16, 512]", flen);
    if (n_ref > kBssMaxRef || n_est > kBssMaxEst)
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_bss_lagcorr: %d reference / %d estimate channels (at most %d / %d)", n_ref, n_est,
                 kBssMaxRef, kBssMaxEst);
    DCS_ON_DEVICE(ctx->device);
    const Layout s = corr_layout(n_ref, n_est, flen, n_samples, 1);
    DCS_CHECK(ctx->bss_ws.ensure(s.partial * sizeof(double)));
    DcsTimer t(ctx, DCS_TAG_BSS_CORR);
    DCS_CHECK(launch_corr(ctx, s, ref_d, est_d, n_samples, n_samples, 0, 0, (double*)ctx->bss_ws.ptr, out_d, nullptr));
    t.done();
    return DCS_OK;
}

extern "C" int dcs_bss_energies(dcs_ctx* ctx, const double* ref_d, const double* est_d, int nsrc_ref, int nsrc_est,
                                int nchan, int64_t nsampl, int64_t win, int64_t hop, int64_t nwin, int flen, int all_pairs,
                                double* out_d) {
    if (!ctx) DCS_FAIL(DCS_EINVAL, "dcs_bss_energies: null ctx");
    if (nsrc_ref < 1 || nsrc_est < 1 || nchan < 1 || win < 1 || hop < 1 || nwin < 0 || nsampl < 0)
        DCS_FAIL(DCS_EINVAL, "dcs_bss_energies: bad argument (nsrc %d / %d, nchan %d, win %lld, hop %lld, nwin %lld)",
                 nsrc_ref, nsrc_est, nchan, (long long)win, (long long)hop, (long long)nwin);
    if (flen < 16 || flen > 512 || flen % 16)
        DCS_FAIL(DCS_EINVAL, "dcs_bss_energies: flen %d is not a multiple of 16 in [16, 512]", flen);
    if (!all_pairs && nsrc_est != nsrc_ref)
        DCS_FAIL(DCS_EINVAL, "dcs_bss_energies: %d estimates for %d sources without all_pairs", nsrc_est, nsrc_ref);
    const int R = nsrc_ref * nchan, M = nsrc_est * nchan;
    if (R > kBssMaxRef || M > kBssMaxEst)
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_bss_energies: %d reference / %d estimate channels (at most %d / %d)", R, M,
                 kBssMaxRef, kBssMaxEst);
    if (nwin == 0) return DCS_OK;
    if (!ref_d || !est_d || !out_d) DCS_FAIL(DCS_EINVAL, "dcs_bss_energies: null buffer");
    if ((nwin - 1) > (nsampl - win) / hop || win > nsampl)
        DCS_FAIL(DCS_EINVAL, "dcs_bss_energies: %lld windows of %lld (hop %lld) run past %lld samples", (long long)nwin,
                 (long long)win, (long long)hop, (long long)nsampl);
    DCS_ON_DEVICE(ctx->device);

    Geom g;
    g.R = R;
    g.M = M;
    g.Nz = R + M;
    g.L = flen;
    g.nlag = 2 * flen - 1;
    g.nchan = nchan;
    g.nsrc = nsrc_ref;
    g.npad_full = (int)dcs_round_up((int64_t)R * flen, kNb);
    g.npad_src = (int)dcs_round_up((int64_t)nchan * flen, kNb);
    g.w_full = (int64_t)g.npad_full * (g.npad_full + kDCols);
    g.w_src = (int64_t)g.npad_src * (g.npad_src + kDCols);
    g.w_per = g.w_full + (int64_t)nsrc_ref * g.w_src;
    g.ppw = 1 + nsrc_ref;

    // windows per group: everything a window needs, within the scratch budget
    const Layout one = corr_layout(R, M, flen, win, 1);
    const size_t per_win = one.partial + one.C + (size_t)g.w_per + (size_t)M * (1 + g.ppw) + 96;
    // (grid.z of the correlation and grid.y of the factorisation count windows / problems: at most 65535)
    const int64_t fit = std::min<int64_t>((int64_t)(kScratchBudget / 8 / per_win), 65535 / g.ppw);
    const int nw_max = (int)std::max<int64_t>(1, std::min<int64_t>(nwin, fit));
    {
        const Layout s = corr_layout(R, M, flen, win, nw_max);
        const size_t need = align_doubles(s.partial) + align_doubles(s.C) + align_doubles((size_t)g.w_per * nw_max) +
                            align_doubles((size_t)nw_max * M) + align_doubles((size_t)nw_max * g.ppw * M);
        DCS_CHECK(ctx->bss_ws.ensure(need * sizeof(double)));
    }
    const int per_w_out = nsrc_est * (all_pairs ? nsrc_ref : 1) * nchan;
    for (int64_t w0 = 0; w0 < nwin; w0 += nw_max) {
        const int nw = (int)std::min<int64_t>(nw_max, nwin - w0);
        const Layout s = corr_layout(R, M, flen, win, nw);
        double* base = (double*)ctx->bss_ws.ptr;
        double* partial = base;
        double* C = partial + align_doubles(s.partial);
        double* W = C + align_doubles(s.C);
        double* enorm = W + align_doubles((size_t)g.w_per * nw);
        double* ynorm = enorm + align_doubles((size_t)nw * M);
        g.W = W;
        g.C = C;

        DcsTimer tc(ctx, DCS_TAG_BSS_CORR);
        DCS_CHECK(launch_corr(ctx, s, ref_d, est_d, nsampl, win, hop, w0, partial, C, enorm));
        tc.done();

        DcsTimer tf(ctx, DCS_TAG_BSS_CHOL);
        const int nprob = nw * g.ppw;
        const int ld_max = g.npad_full + kDCols;
        hipLaunchKernelGGL(bss_assemble_kernel, dim3(dcs_cdiv(ld_max, 256), g.npad_full, nprob), dim3(256), 0, ctx->stream,
                           g);
        DCS_HIP(hipGetLastError());
        const int nrb = g.npad_full / kNb;
        for (int kb = 0; kb < nrb; ++kb) {
            hipLaunchKernelGGL(bss_panel_kernel, dim3(nrb - kb, nprob), dim3(256), 0, ctx->stream, g, kb);
            DCS_HIP(hipGetLastError());
            if (nrb - kb - 1 > 0) {
                hipLaunchKernelGGL(bss_update_kernel, dim3(nrb - kb, nrb - kb - 1, nprob), dim3(256), 0, ctx->stream, g,
                                   kb);
                DCS_HIP(hipGetLastError());
            }
        }
        hipLaunchKernelGGL(bss_colnorm_kernel, dim3(M, nprob), dim3(256), 0, ctx->stream, g, ynorm);
        DCS_HIP(hipGetLastError());
        const int64_t n_out = (int64_t)nw * per_w_out;
        hipLaunchKernelGGL(bss_energies_kernel, dim3(dcs_cdiv(n_out, 256)), dim3(256), 0, ctx->stream, g, enorm, ynorm,
                           nsrc_est, nw, all_pairs, out_d + w0 * per_w_out * 5);
        DCS_HIP(hipGetLastError());
        tf.done();
    }
    return DCS_OK;
}

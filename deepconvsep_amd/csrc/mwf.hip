// dcs_mwf_f32: multichannel Wiener filter for two-channel separations, the EM for full-rank spatial covariances of Duong,
// Vincent and Gribonval with a time-invariant R_j[f] (include/dcs.h has the recurrence; DESIGN.md section 4 the numbers).
//
// Frequencies are independent and time is reduced per frequency once per iteration, so a pass is ONE launch over
// (blocks of 64 adjacent bins) x (chunks of kFramesPerBlock frames; past kMaxParts chunks a workgroup takes every
// kMaxParts-th one, so that what the next pass has to add up stays kMaxParts sets of sums however long the signal is):
//   pass 0          y_j = A_j e^{i phase}: v_j -> scratch, the workgroup's sum_t C_j -> partials
//   pass 1 .. n-1   prologue: R_j[f] of the block's 64 bins from the partials of the previous pass (every workgroup of a
//                   bin block reduces them again, set by set in index order); E step per frame; v_j and partials out
//   pass n          the same prologue and E step; |y_j|, angle(y_j) out, nothing else
// A workgroup is 8 waves (4 in the middle passes of 6 .. 8 sources): lane = bin, wave w of W takes frames w, w + W, ... of a
// chunk.  The per-wave sums are added in wave order through LDS, the sets in index order: no atomics, no grid barrier, the
// same bits every run.  Partials are
// double buffered (a workgroup may still be in its prologue when another one of the same bins writes its sums); v is
// updated in place (a thread reads only what it wrote).  y and C_j live in registers only.
// The 2x2 algebra, the phasors and every sum over t are float64: a*d - |b|^2 of a rank-1 Cx (both channels equal) has
// nothing left in float32.  What is stored between passes (v) is float32.
// sum_t v_j is not stored: v_j = Re tr(C_j) / 2 term by term, so it is (sum_t C_j[0][0] + sum_t C_j[1][1]) / 2.
#include "dcs_internal.h"

#include <float.h>
#include <math.h>

#include <algorithm>

namespace {

constexpr int kBins = 64;                             // lanes of a wave: adjacent bins
constexpr int kWaves = 8;                             // waves of a workgroup: interleaved frames
constexpr int kFramesPerBlock = 256;
constexpr int kThreads = kBins * kWaves;
enum { kInit = 0, kIterate = 1, kFinal = 2 };
// the middle pass of 6 .. 8 sources needs more than the 256 registers a lane has with two waves per SIMD: its workgroups are
// 4 waves (measured at J = 8, T = 3720, F = 1025: 0.15 ms per pass instead of 0.70 ms with 392 bytes per lane spilled)
constexpr int mwf_waves(int J, int mode) { return mode == kIterate && J > 5 ? 4 : kWaves; }
constexpr int kQ = 4;                                 // per source: C[0][0], C[1][1], Re C[0][1], Im C[0][1]
constexpr int kMaxSources = 8;
constexpr int kMaxParts = 32;                         // sets of per-workgroup sums a prologue adds up, at most

struct MwfArgs {
    const float* mag;
    const float* phase;
    int64_t ch_stride;
    const float* src;
    int64_t src_ch_stride, src_stride;
    float* out_mag;
    float* out_phase;
    int64_t ld, T;
    int F, n_parts;           // n_parts = gridDim.y
    float pre_div;
    double eps;
    float* v;                 // [J][T][F]
    const double* part_in;    // [n_parts][J][kQ][F], the previous pass
    double* part_out;
};

// what one frame of one bin needs from memory (kInit: the estimates and the phases; otherwise the mixture and v)
template <int J, int MODE>
struct MwfIn {
    float p0, p1, m0, m1;
    float a[MODE == kInit ? 2 * J : J];
};

template <int J, int MODE>
__device__ __forceinline__ MwfIn<J, MODE> mwf_load(const MwfArgs& a, int64_t t, int f) {
    MwfIn<J, MODE> in;
    const int64_t row = t * a.ld + f;
    in.p0 = a.phase[row];
    in.p1 = a.phase[a.ch_stride + row];
    if (MODE == kInit) {
        in.m0 = in.m1 = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            in.a[j] = a.src[j * a.src_stride + row];
            in.a[J + j] = a.src[a.src_ch_stride + j * a.src_stride + row];
        }
    } else {
        in.m0 = a.mag[row];
        in.m1 = a.mag[a.ch_stride + row];
#pragma unroll
        for (int j = 0; j < J; ++j) in.a[j] = a.v[((int64_t)j * a.T + t) * a.F + f];
    }
    return in;
}

// the n-th frame wave w of W, of workgroup row `part`, works on: frame w + W (n % (256 / W)) of chunk part + (n / (256 / W))
// n_parts.  Increasing in n, so the first one at or past T ends the wave's loop.
template <int W>
__device__ __forceinline__ int64_t mwf_frame(int part, int n_parts, int w, int n) {
    constexpr int per_wave = kFramesPerBlock / W;
    return ((int64_t)part + (int64_t)(n / per_wave) * n_parts) * kFramesPerBlock + w + (n % per_wave) * W;
}

template <int J, int MODE>
__global__ __launch_bounds__(kBins * mwf_waves(J, MODE)) void mwf_pass_kernel(MwfArgs a) {
    constexpr int W = mwf_waves(J, MODE);
    __shared__ double lds[(W > J ? W : J) * kQ][kBins];   // at most 16 KB: the J * kQ sums of the prologue, then the W * kQ wave sums
    const int lane = threadIdx.x & (kBins - 1), w = threadIdx.x >> 6;
    const int f_own = blockIdx.x * kBins + lane;
    const bool live = f_own < a.F;
    const int f = live ? f_own : a.F - 1;             // lanes past F work on the last bin again and store nothing
    const int part = blockIdx.y;

    // M step: R_j[f] = sum_t C_j / (sum_t v_j + eps)
    double r00[J], r11[J], rre[J], rim[J];
    if (MODE != kInit) {
        for (int k = w; k < J * kQ; k += W) {
            double s = 0.0;
            for (int c = 0; c < a.n_parts; ++c) s += a.part_in[((int64_t)c * (J * kQ) + k) * a.F + f];
            lds[k][lane] = s;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const double c00 = lds[j * kQ + 0][lane], c11 = lds[j * kQ + 1][lane];
            const double den = 0.5 * (c00 + c11) + a.eps;      // divisions: 0 / den is 0 for any eps > 0, 0 * (1 / den) is not
            r00[j] = c00 / den;
            r11[j] = c11 / den;
            rre[j] = lds[j * kQ + 2][lane] / den;
            rim[j] = lds[j * kQ + 3][lane] / den;
        }
        __syncthreads();
    }

    double acc[J][kQ];
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int q = 0; q < kQ; ++q) acc[j][q] = 0.0;

    auto frame = [&](int n) { return mwf_frame<W>(part, a.n_parts, w, n); };
    if (frame(0) < a.T) {
        MwfIn<J, MODE> in = mwf_load<J, MODE>(a, frame(0), f);
        for (int n = 0;; ++n) {
            const int64_t t = frame(n);
            const int64_t tn = frame(n + 1);
            const bool more = tn < a.T;                                // wave-uniform
            MwfIn<J, MODE> next = in;
            if (more) next = mwf_load<J, MODE>(a, tn, f);              // in flight while this frame is worked on

            double s0, c0, s1, c1;
            sincos((double)in.p0, &s0, &c0);
            sincos((double)in.p1, &s1, &c1);
            if (MODE == kInit) {
                const double n0 = c0 * c0 + s0 * s0, n1 = c1 * c1 + s1 * s1;
                const double ure = c0 * c1 + s0 * s1, uim = s0 * c1 - c0 * s1;   // e^{i p0} conj(e^{i p1})
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const double a0 = (double)(in.a[j] / a.pre_div), a1 = (double)(in.a[J + j] / a.pre_div);
                    const double c00 = a0 * a0 * n0, c11 = a1 * a1 * n1, aa = a0 * a1;
                    acc[j][0] += c00;
                    acc[j][1] += c11;
                    acc[j][2] += aa * ure;
                    acc[j][3] += aa * uim;
                    if (live) a.v[((int64_t)j * a.T + t) * a.F + f] = (float)(0.5 * (c00 + c11));
                }
            } else {
                const double x0r = (double)in.m0 * c0, x0i = (double)in.m0 * s0;
                const double x1r = (double)in.m1 * c1, x1i = (double)in.m1 * s1;
                // Cx = sum_j v_j R_j + eps I = [[ca, cb], [conj cb, cd]]
                double ca = a.eps, cd = a.eps, cbr = 0.0, cbi = 0.0;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const double v = (double)in.a[j];
                    ca += v * r00[j];
                    cd += v * r11[j];
                    cbr += v * rre[j];
                    cbi += v * rim[j];
                }
                // P = Cx^{-1} = [[p00, p01], [conj p01, p11]],  z = P x.  The determinant is taken of Cx / max(a, d): a bin with
                // nothing in it has Cx = eps I, and eps * eps underflows for eps below 1e-154 (then 0 * inf = NaN on zero rows)
                const double inv_s = 1.0 / fmax(ca, cd);               // >= eps >= DBL_MIN: finite
                const double na = ca * inv_s, nd = cd * inv_s, nbr = cbr * inv_s, nbi = cbi * inv_s;
                const double idet = inv_s / (na * nd - (nbr * nbr + nbi * nbi));
                const double p00 = nd * idet, p11 = na * idet, p01r = -nbr * idet, p01i = -nbi * idet;
                const double z0r = p00 * x0r + p01r * x1r - p01i * x1i, z0i = p00 * x0i + p01r * x1i + p01i * x1r;
                const double z1r = p01r * x0r + p01i * x0i + p11 * x1r, z1i = p01r * x0i - p01i * x0r + p11 * x1i;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const double v = (double)in.a[j];
                    // S = v_j R_j,  y_j = W_j x = S z
                    const double s00 = v * r00[j], s11 = v * r11[j], sr = v * rre[j], si = v * rim[j];
                    const double y0r = s00 * z0r + sr * z1r - si * z1i, y0i = s00 * z0i + sr * z1i + si * z1r;
                    const double y1r = sr * z0r + si * z0i + s11 * z1r, y1i = sr * z0i - si * z0r + s11 * z1i;
                    if (MODE == kFinal) {
                        if (live) {
                            const int64_t o = j * a.src_stride + t * a.ld + f;
                            a.out_mag[o] = (float)sqrt(y0r * y0r + y0i * y0i);
                            a.out_phase[o] = (y0r == 0.0 && y0i == 0.0) ? 0.f : (float)atan2(y0i, y0r);
                            a.out_mag[a.src_ch_stride + o] = (float)sqrt(y1r * y1r + y1i * y1i);
                            a.out_phase[a.src_ch_stride + o] = (y1r == 0.0 && y1i == 0.0) ? 0.f : (float)atan2(y1i, y1r);
                        }
                    } else {
                        // C_j = y y^H + (I - W_j) S = y y^H + S - S Q,  Q = P S
                        const double q00r = p00 * s00 + p01r * sr + p01i * si;                          // Re Q[0][0] is all S Q needs
                        const double q01r = p00 * sr + p01r * s11, q01i = p00 * si + p01i * s11;
                        const double q10r = p01r * s00 + p11 * sr, q10i = -p01i * s00 - p11 * si;
                        const double q11r = p01r * sr + p01i * si + p11 * s11, q11i = p01r * si - p01i * sr;
                        const double m00 = s00 * q00r + sr * q10r - si * q10i;                   // Re (S Q)[0][0]
                        const double m11 = sr * q01r + si * q01i + s11 * q11r;                   // Re (S Q)[1][1]
                        const double m01r = s00 * q01r + sr * q11r - si * q11i, m01i = s00 * q01i + sr * q11i + si * q11r;
                        const double c00 = y0r * y0r + y0i * y0i + s00 - m00;
                        const double c11 = y1r * y1r + y1i * y1i + s11 - m11;
                        acc[j][0] += c00;
                        acc[j][1] += c11;
                        acc[j][2] += y0r * y1r + y0i * y1i + sr - m01r;                          // y0 conj(y1)
                        acc[j][3] += y0i * y1r - y0r * y1i + si - m01i;
                        if (live) a.v[((int64_t)j * a.T + t) * a.F + f] = (float)(0.5 * (c00 + c11));
                    }
                }
            }
            if (!more) break;
            in = next;
        }
    }

    if (MODE != kFinal) {
        // the workgroup's sums: the waves added in wave order, one quantity per wave 0 .. 3
        for (int j = 0; j < J; ++j) {
            __syncthreads();
#pragma unroll
            for (int q = 0; q < kQ; ++q) lds[w * kQ + q][lane] = acc[j][q];
            __syncthreads();
            if (w < kQ) {
                double s = 0.0;
#pragma unroll
                for (int ww = 0; ww < W; ++ww) s += lds[ww * kQ + w][lane];
                if (live) a.part_out[((int64_t)part * (J * kQ) + j * kQ + w) * a.F + f] = s;
            }
        }
    }
}

// niter = 0: the estimates over pre_div and the mixture's phases, as they are
__global__ __launch_bounds__(kThreads) void mwf_copy_kernel(MwfArgs a, int J) {
    const int lane = threadIdx.x & (kBins - 1), w = threadIdx.x >> 6;
    const int f = blockIdx.x * kBins + lane;
    if (f >= a.F) return;
    for (int n = 0;; ++n) {
        const int64_t t = mwf_frame<kWaves>(blockIdx.y, a.n_parts, w, n);
        if (t >= a.T) break;
        const int64_t row = t * a.ld + f;
        for (int c = 0; c < 2; ++c) {
            const float ph = a.phase[c * a.ch_stride + row];
            for (int j = 0; j < J; ++j) {
                const int64_t o = c * a.src_ch_stride + j * a.src_stride + row;
                a.out_mag[o] = a.src[o] / a.pre_div;
                a.out_phase[o] = ph;
            }
        }
    }
}

template <int J>
void mwf_launch(const MwfArgs& a, int mode, dim3 grid, hipStream_t stream) {
    const dim3 block(kBins * mwf_waves(J, mode));
    if (mode == kInit) hipLaunchKernelGGL((mwf_pass_kernel<J, kInit>), grid, block, 0, stream, a);
    else if (mode == kIterate) hipLaunchKernelGGL((mwf_pass_kernel<J, kIterate>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((mwf_pass_kernel<J, kFinal>), grid, block, 0, stream, a);
}

}  // namespace

extern "C" int dcs_mwf_frames_per_block(void) { return kFramesPerBlock; }

extern "C" int dcs_mwf_f32(dcs_ctx* ctx, const float* mag_d, const float* phase_d, int64_t ch_stride, const float* src_d,
                           int64_t src_ch_stride, int64_t src_stride, int64_t ld, int64_t n_frames, int F, int J, int niter,
                           float pre_div, double eps, float* out_mag_d, float* out_phase_d) {
    if (!ctx) DCS_FAIL(DCS_EINVAL, "dcs_mwf_f32: null ctx");
    if (J < 1 || J > kMaxSources) DCS_FAIL(DCS_EINVAL, "dcs_mwf_f32: %d sources (1 .. %d)", J, kMaxSources);
    if (niter < 0 || niter > 100) DCS_FAIL(DCS_EINVAL, "dcs_mwf_f32: %d iterations (0 .. 100)", niter);
    if (F < 1 || ld < F || n_frames < 0)
        DCS_FAIL(DCS_EINVAL, "dcs_mwf_f32: bad shape (F %d, ld %lld, n_frames %lld)", F, (long long)ld, (long long)n_frames);
    // eps below the smallest normal double: Cx^{-1} = I / eps of an empty bin is not finite
    if (!(pre_div > 0.f) || !(eps >= DBL_MIN))
        DCS_FAIL(DCS_EINVAL, "dcs_mwf_f32: pre_div %g must be positive and eps %g a positive normal number", pre_div, eps);
    if (!mag_d || !phase_d || !src_d || !out_mag_d || !out_phase_d) DCS_FAIL(DCS_EINVAL, "dcs_mwf_f32: null buffer");
    if (n_frames == 0) return DCS_OK;
    const int64_t n_chunks = (n_frames + kFramesPerBlock - 1) / kFramesPerBlock;
    const int n_parts = (int)std::min<int64_t>(n_chunks, kMaxParts);
    DCS_ON_DEVICE(ctx->device);

    MwfArgs a;
    a.mag = mag_d;
    a.phase = phase_d;
    a.ch_stride = ch_stride;
    a.src = src_d;
    a.src_ch_stride = src_ch_stride;
    a.src_stride = src_stride;
    a.out_mag = out_mag_d;
    a.out_phase = out_phase_d;
    a.ld = ld;
    a.T = n_frames;
    a.F = F;
    a.n_parts = n_parts;
    a.pre_div = pre_div;
    a.eps = eps;
    a.v = nullptr;
    a.part_in = nullptr;
    a.part_out = nullptr;
    const dim3 grid(dcs_cdiv(F, kBins), n_parts);

    if (niter == 0) {
        DcsTimer t(ctx, DCS_TAG_MWF);
        hipLaunchKernelGGL(mwf_copy_kernel, grid, dim3(kThreads), 0, ctx->stream, a, J);
        DCS_HIP(hipGetLastError());
        t.done();
        return DCS_OK;
    }

    const size_t v_bytes = (size_t)dcs_round_up((int64_t)J * n_frames * F * (int64_t)sizeof(float), 256);
    const size_t part_bytes = (size_t)dcs_round_up((int64_t)n_parts * J * kQ * F * (int64_t)sizeof(double), 256);
    DCS_CHECK(ctx->mwf_ws.ensure(v_bytes + 2 * part_bytes));
    char* base = (char*)ctx->mwf_ws.ptr;
    a.v = (float*)base;
    double* part[2] = {(double*)(base + v_bytes), (double*)(base + v_bytes + part_bytes)};

    for (int pass = 0; pass <= niter; ++pass) {
        const int mode = pass == 0 ? kInit : pass == niter ? kFinal : kIterate;
        a.part_in = part[(pass + 1) & 1];
        a.part_out = part[pass & 1];
        DcsTimer t(ctx, DCS_TAG_MWF);
        switch (J) {
            case 1: mwf_launch<1>(a, mode, grid, ctx->stream); break;
            case 2: mwf_launch<2>(a, mode, grid, ctx->stream); break;
            case 3: mwf_launch<3>(a, mode, grid, ctx->stream); break;
            case 4: mwf_launch<4>(a, mode, grid, ctx->stream); break;
            case 5: mwf_launch<5>(a, mode, grid, ctx->stream); break;
            case 6: mwf_launch<6>(a, mode, grid, ctx->stream); break;
            case 7: mwf_launch<7>(a, mode, grid, ctx->stream); break;
            default: mwf_launch<8>(a, mode, grid, ctx->stream); break;
        }
        DCS_HIP(hipGetLastError());
        t.done();
    }
    return DCS_OK;
}

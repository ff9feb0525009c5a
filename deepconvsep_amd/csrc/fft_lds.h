// The in-LDS complex FFT and the small helpers shared by the STFT kernels of fft.hip, fft_render.hip and
// fft_score_render.hip: one definition, so that a frame transformed by any of them comes out bit for bit the same.
// What only the render kernels share -- the frame around fft_lds, their launch -- is fft_frame.h, on top of this header.
// Internal linkage (device templates).
#pragma once
#include "dcs_internal.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;

template <typename R> struct V2;
template <> struct V2<float> { using type = float2; };
template <> struct V2<double> { using type = double2; };

template <typename R2, typename R>
__device__ __forceinline__ R2 mk(R x, R y) {
    R2 r;
    r.x = x;
    r.y = y;
    return r;
}

// w(j) = exp(DIR * 2 pi i j / N) for 0 <= j < N from the half-circle table tw[0..N/2]
// (tw holds the forward sign, exp(-2 pi i j / N)).
template <typename R, typename R2, int DIR>
__device__ __forceinline__ R2 twiddle(const R2* __restrict__ tw, int j, int M) {
    R2 w;
    if (j <= M) {
        w = tw[j];
    } else {
        w = tw[j - M];
        w.x = -w.x;
        w.y = -w.y;
    }
    if (DIR > 0) w.y = -w.y;
    return w;
}

template <typename R2>
__device__ __forceinline__ R2 cmul(R2 a, R2 b) {
    R2 r;
    r.x = a.x * b.x - a.y * b.y;
    r.y = a.x * b.y + a.y * b.x;
    return r;
}

// In-LDS complex FFT of length M = 2^log2m, DIR = -1 forward / +1 inverse (unscaled).
// Input in `a`; returns the buffer that holds the natural-order result.  Every thread of the
// workgroup must call it; it ends with a barrier.
template <typename R, typename R2, int DIR>
__device__ R2* fft_lds(R2* a, R2* b, const R2* __restrict__ tw, int M, int log2m) {
    const int tid = threadIdx.x;
    int Ns = 1;
    int lg = 0;
    // radix-4 passes
    while (lg + 2 <= log2m) {
        const int quarter = M >> 2;
        const int step = (2 * M) / (4 * Ns);  // N / (4 Ns): table stride per unit of t*k
        for (int j = tid; j < quarter; j += kThreads) {
            const int k = j & (Ns - 1);
            R2 v0 = a[j];
            R2 v1 = a[j + quarter];
            R2 v2 = a[j + 2 * quarter];
            R2 v3 = a[j + 3 * quarter];
            if (Ns > 1) {
                v1 = cmul(v1, twiddle<R, R2, DIR>(tw, k * step, M));
                v2 = cmul(v2, twiddle<R, R2, DIR>(tw, 2 * k * step, M));
                v3 = cmul(v3, twiddle<R, R2, DIR>(tw, 3 * k * step, M));
            }
            R2 a02 = mk<R2, R>(v0.x + v2.x, v0.y + v2.y);
            R2 s02 = mk<R2, R>(v0.x - v2.x, v0.y - v2.y);
            R2 a13 = mk<R2, R>(v1.x + v3.x, v1.y + v3.y);
            R2 s13 = mk<R2, R>(v1.x - v3.x, v1.y - v3.y);
            // forward: y1 = s02 - i s13, y3 = s02 + i s13; inverse: swapped
            R2 ym = mk<R2, R>(s02.x + s13.y, s02.y - s13.x);  // s02 - i*s13
            R2 yp = mk<R2, R>(s02.x - s13.y, s02.y + s13.x);  // s02 + i*s13
            const int d = ((j - k) << 2) + k;                 // (j / Ns) * 4 Ns + k
            b[d] = mk<R2, R>(a02.x + a13.x, a02.y + a13.y);
            b[d + Ns] = (DIR < 0) ? ym : yp;
            b[d + 2 * Ns] = mk<R2, R>(a02.x - a13.x, a02.y - a13.y);
            b[d + 3 * Ns] = (DIR < 0) ? yp : ym;
        }
        __syncthreads();
        R2* t = a;
        a = b;
        b = t;
        Ns <<= 2;
        lg += 2;
    }
    if (lg < log2m) {  // one radix-2 pass
        const int half = M >> 1;
        const int step = (2 * M) / (2 * Ns);
        for (int j = tid; j < half; j += kThreads) {
            const int k = j & (Ns - 1);
            R2 v0 = a[j];
            R2 v1 = a[j + half];
            if (Ns > 1) v1 = cmul(v1, twiddle<R, R2, DIR>(tw, k * step, M));
            const int d = ((j - k) << 1) + k;
            b[d] = mk<R2, R>(v0.x + v1.x, v0.y + v1.y);
            b[d + Ns] = mk<R2, R>(v0.x - v1.x, v0.y - v1.y);
        }
        __syncthreads();
        R2* t = a;
        a = b;
        b = t;
    }
    return a;
}

__device__ __forceinline__ float dcs_atan2(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ double dcs_atan2(double y, double x) { return atan2(y, x); }
__device__ __forceinline__ float dcs_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double dcs_sqrt(double x) { return sqrt(x); }
__device__ __forceinline__ void dcs_sincos(float a, float* s, float* c) { sincosf(a, s, c); }
__device__ __forceinline__ void dcs_sincos(double a, double* s, double* c) { sincos(a, s, c); }

// The tail of the render kernels (fft_render.hip, fft_score_render.hip): Z = the length-M complex transform of the frame
// packed as (even, odd) samples; writes bins 0 .. M of the real transform as mag = |X| / sqrt(N) (SCALED: times `scale`)
// and zeroes the row padding up to ld.  Every thread of the workgroup calls it.
template <typename R, typename R2, bool SCALED>
__device__ __forceinline__ void packed_real_mag_row(const R2* __restrict__ Z, const R2* __restrict__ tw, int M, int64_t ld,
                                                    R sqrt_n, R scale, R* __restrict__ orow) {
    const int tid = threadIdx.x;
    for (int k = tid; k <= M; k += kThreads) {
        const R2 zk = Z[k & (M - 1)];
        const R2 zm = Z[(M - k) & (M - 1)];
        // E = (zk + conj(zm))/2 ; O = -i (zk - conj(zm))/2 ; X = E + w^k O   (stft_forward_kernel, term for term)
        const R er = R(0.5) * (zk.x + zm.x), ei = R(0.5) * (zk.y - zm.y);
        const R orr = R(0.5) * (zk.y + zm.y), oi = R(-0.5) * (zk.x - zm.x);
        const R2 w = tw[k];
        const R xr = er + (w.x * orr - w.y * oi);
        const R xi = ei + (w.x * oi + w.y * orr);
        const R ax = dcs_sqrt(xr * xr + xi * xi);
        const R mag = ax / sqrt_n;
        orow[k] = SCALED ? scale * mag : mag;
    }
    for (int k = M + 1 + tid; k < ld; k += kThreads) orow[k] = R(0);   // row padding
}

}  // namespace

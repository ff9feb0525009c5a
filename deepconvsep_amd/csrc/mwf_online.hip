// dcs_mwf_online_*: the multichannel Wiener filter of mwf.hip in a causal form for the streams (include/dcs.h has the
// recurrence; DESIGN.md section 4o3 the numbers).  The spatial covariance R_j[f] of a frame comes from a running sum S_j[f] of
// the posterior covariances of the frames before it and from this frame's own, so the state per (source, bin) is one Hermitian
// 2x2 matrix -- four float64 -- and a push of n frames is ONE launch:
//   lane = bin (64 adjacent bins per workgroup of one wave: F = 513 spreads over nine compute units), the J sources of the bin in
//   registers, time serial.  The state is loaded once (not at all when the push starts at absolute frame 0), the frame loop runs
//   with the next frame's 4 + 2 J float32 loads in flight, the state is stored once.
// Nothing is shared between lanes: no LDS, no cross-lane sum, no atomics.  The sum over j (Cx) runs in source order in one lane,
// and every product that may be fused into an addition is fused by the front end, statement by statement (the pragma below):
// what a frame computes does not depend on where the optimiser peeled or unrolled the frame loop, so the bits are the same
// however the frames are cut into pushes.
// As in mwf.hip the phasors, the 2x2 algebra and the state are float64 and the closed forms are the same (restated here: the
// batch kernels keep their code); v_j stays in registers between the iterations of a frame.
#include "dcs_internal.h"

#include <float.h>
#include <math.h>

#pragma clang fp contract(on)

namespace {

constexpr int kBins = 64;                             // lanes of a workgroup (one wave): adjacent bins
constexpr int kQ = 4;                                 // per source: S[0][0], S[1][1], Re S[0][1], Im S[0][1]
constexpr int kMaxSources = 8;

struct OnlineArgs {
    const float* mag;
    const float* phase;
    int64_t ch_stride;
    const float* src;
    int64_t src_ch_stride, src_stride;
    float* out_mag;
    float* out_phase;
    int64_t ld, T;
    int F, niter;
    int fresh;                // the push starts at absolute frame 0: the state is not read
    float pre_div;
    double forget, loading, eps;
    double* state;            // [J][kQ][F]
};

template <int J>
struct OnlineIn {
    float p0, p1, m0, m1;
    float a[2 * J];
};

template <int J>
__device__ __forceinline__ OnlineIn<J> online_load(const OnlineArgs& a, int64_t t, int f) {
    OnlineIn<J> in;
    const int64_t row = t * a.ld + f;
    in.p0 = a.phase[row];
    in.p1 = a.phase[a.ch_stride + row];
    in.m0 = a.mag[row];
    in.m1 = a.mag[a.ch_stride + row];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        in.a[j] = a.src[j * a.src_stride + row];
        in.a[J + j] = a.src[a.src_ch_stride + j * a.src_stride + row];
    }
    return in;
}

template <int J>
__global__ __launch_bounds__(kBins) void mwf_online_kernel(OnlineArgs a) {
    const int f_own = blockIdx.x * kBins + threadIdx.x;
    const bool live = f_own < a.F;
    const int f = live ? f_own : a.F - 1;             // lanes past F work on the last bin again and store nothing

    // S_j of the frame before this push
    double st[J][kQ];
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int q = 0; q < kQ; ++q) st[j][q] = a.fresh ? 0.0 : a.state[((int64_t)j * kQ + q) * a.F + f];

    const double one_load = 1.0 + a.loading;
    OnlineIn<J> in = online_load<J>(a, 0, f);
    for (int64_t t = 0; t < a.T; ++t) {
        const bool more = t + 1 < a.T;
        OnlineIn<J> next = in;
        if (more) next = online_load<J>(a, t + 1, f);                  // in flight while this frame is worked on

        double s0, c0, s1, c1;
        sincos((double)in.p0, &s0, &c0);
        sincos((double)in.p1, &s1, &c1);
        const double x0r = (double)in.m0 * c0, x0i = (double)in.m0 * s0;
        const double x1r = (double)in.m1 * c1, x1i = (double)in.m1 * s1;

        // G_j = forget * S_j[t-1] (a product on its own: never fused into N_j = G_j + C_j), C_j = y_j y_j^H of the estimates
        double g[J][kQ], c[J][kQ], v[J];
        {
            const double n0 = c0 * c0 + s0 * s0, n1 = c1 * c1 + s1 * s1;
            const double ure = c0 * c1 + s0 * s1, uim = s0 * c1 - c0 * s1;       // e^{i p0} conj(e^{i p1})
#pragma unroll
            for (int j = 0; j < J; ++j) {
#pragma unroll
                for (int q = 0; q < kQ; ++q) g[j][q] = __dmul_rn(a.forget, st[j][q]);
                const double a0 = (double)(in.a[j] / a.pre_div), a1 = (double)(in.a[J + j] / a.pre_div);
                const double aa = a0 * a1;
                c[j][0] = a0 * a0 * n0;
                c[j][1] = a1 * a1 * n1;
                c[j][2] = aa * ure;
                c[j][3] = aa * uim;
                v[j] = 0.5 * (c[j][0] + c[j][1]);
            }
        }

        for (int it = 0; it < a.niter; ++it) {
            // S = v_j R_j,  R_j = (N_j + loading n_j I) / ((1 + loading) n_j + eps),  N_j = G_j + C_j;  Cx = sum_j S + eps I
            double s[J][kQ];
            double ca = 0.0, cd = 0.0, cbr = 0.0, cbi = 0.0;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const double n00 = g[j][0] + c[j][0], n11 = g[j][1] + c[j][1];
                const double nre = g[j][2] + c[j][2], nim = g[j][3] + c[j][3];
                const double n = 0.5 * (n00 + n11);
                const double den = one_load * n + a.eps;               // divisions: 0 / den is 0 for any eps > 0
                const double ln = a.loading * n;
                s[j][0] = v[j] * ((n00 + ln) / den);
                s[j][1] = v[j] * ((n11 + ln) / den);
                s[j][2] = v[j] * (nre / den);
                s[j][3] = v[j] * (nim / den);
                ca += s[j][0];
                cd += s[j][1];
                cbr += s[j][2];
                cbi += s[j][3];
            }
            ca += a.eps;
            cd += a.eps;
            // P = Cx^{-1} = [[p00, p01], [conj p01, p11]],  z = P x.  The determinant is taken of Cx / max(a, d) (an empty bin has
            // Cx = eps I, and eps * eps underflows for eps below 1e-154) and scaled back
            const double sc = fmax(ca, cd);                            // >= eps >= DBL_MIN
            const double na = ca / sc, nd = cd / sc, nbr = cbr / sc, nbi = cbi / sc;
            const double det = (na * nd - (nbr * nbr + nbi * nbi)) * sc;
            const double p00 = nd / det, p11 = na / det, p01r = -nbr / det, p01i = -nbi / det;
            const double z0r = p00 * x0r + p01r * x1r - p01i * x1i, z0i = p00 * x0i + p01r * x1i + p01i * x1r;
            const double z1r = p01r * x0r + p01i * x0i + p11 * x1r, z1i = p01r * x0i - p01i * x0r + p11 * x1i;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const double s00 = s[j][0], s11 = s[j][1], sr = s[j][2], si = s[j][3];
                // y_j = W_j x = S z
                const double y0r = s00 * z0r + sr * z1r - si * z1i, y0i = s00 * z0i + sr * z1i + si * z1r;
                const double y1r = sr * z0r + si * z0i + s11 * z1r, y1i = sr * z0i - si * z0r + s11 * z1i;
                // C_j = y y^H + (I - W_j) S = y y^H + S - S Q,  Q = P S
                const double q00r = p00 * s00 + p01r * sr + p01i * si;                          // Re Q[0][0] is all S Q needs
                const double q01r = p00 * sr + p01r * s11, q01i = p00 * si + p01i * s11;
                const double q10r = p01r * s00 + p11 * sr, q10i = -p01i * s00 - p11 * si;
                const double q11r = p01r * sr + p01i * si + p11 * s11, q11i = p01r * si - p01i * sr;
                const double m00 = s00 * q00r + sr * q10r - si * q10i;                   // Re (S Q)[0][0]
                const double m11 = sr * q01r + si * q01i + s11 * q11r;                   // Re (S Q)[1][1]
                const double m01r = s00 * q01r + sr * q11r - si * q11i, m01i = s00 * q01i + sr * q11i + si * q11r;
                c[j][0] = y0r * y0r + y0i * y0i + s00 - m00;
                c[j][1] = y1r * y1r + y1i * y1i + s11 - m11;
                c[j][2] = y0r * y1r + y0i * y1i + sr - m01r;                             // y0 conj(y1)
                c[j][3] = y0i * y1r - y0r * y1i + si - m01i;
                v[j] = 0.5 * (c[j][0] + c[j][1]);
                if (it == a.niter - 1 && live) {                                         // wave-uniform but for `live`
                    const int64_t o = j * a.src_stride + t * a.ld + f;
                    a.out_mag[o] = (float)sqrt(y0r * y0r + y0i * y0i);
                    a.out_phase[o] = (y0r == 0.0 && y0i == 0.0) ? 0.f : (float)atan2(y0i, y0r);
                    a.out_mag[a.src_ch_stride + o] = (float)sqrt(y1r * y1r + y1i * y1i);
                    a.out_phase[a.src_ch_stride + o] = (y1r == 0.0 && y1i == 0.0) ? 0.f : (float)atan2(y1i, y1r);
                }
            }
        }

#pragma unroll
        for (int j = 0; j < J; ++j) {
#pragma unroll
            for (int q = 0; q < kQ; ++q) st[j][q] = g[j][q] + c[j][q];     // S_j[t]
        }
        in = next;
    }

    if (live) {
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int q = 0; q < kQ; ++q) a.state[((int64_t)j * kQ + q) * a.F + f] = st[j][q];
    }
}

// niter = 0: the estimates over pre_div and the mixture's phases, as they are
__global__ __launch_bounds__(kBins) void mwf_online_copy_kernel(OnlineArgs a, int J) {
    const int f = blockIdx.x * kBins + threadIdx.x;
    if (f >= a.F) return;
    for (int64_t t = blockIdx.y; t < a.T; t += gridDim.y) {
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

int64_t online_state_bytes(int F, int J) { return dcs_round_up((int64_t)J * kQ * F * (int64_t)sizeof(double), 256); }

}  // namespace

struct dcs_mwf_online {
    dcs_ctx* ctx = nullptr;
    int F = 0, J = 0, niter = 0;
    double forget = 1.0, loading = 0.0, eps = 0.0;
    int64_t frames = 0;
    double* state = nullptr;
    int64_t bytes = 0;
};

int dcs_mwf_online_check(const char* who, int F, int J, int niter, double forget, double loading, double eps) {
    if (J < 1 || J > kMaxSources) DCS_FAIL(DCS_EINVAL, "%s: %d sources (1 .. %d)", who, J, kMaxSources);
    if (niter < 0 || niter > 100) DCS_FAIL(DCS_EINVAL, "%s: %d iterations (0 .. 100)", who, niter);
    if (F < 1) DCS_FAIL(DCS_EINVAL, "%s: %d bins", who, F);
    if (!(forget > 0.0 && forget <= 1.0)) DCS_FAIL(DCS_EINVAL, "%s: forget %g must be in (0, 1]", who, forget);
    if (!(loading >= 0.0) || !(loading <= DBL_MAX)) DCS_FAIL(DCS_EINVAL, "%s: loading %g must be finite and not negative", who, loading);
    // eps below the smallest normal double: Cx^{-1} = I / eps of an empty bin is not finite
    if (!(eps >= DBL_MIN) || !(eps <= DBL_MAX)) DCS_FAIL(DCS_EINVAL, "%s: eps %g must be a positive normal number", who, eps);
    return DCS_OK;
}

extern "C" int dcs_mwf_online_create(dcs_ctx* ctx, int F, int J, int niter, double forget, double loading, double eps,
                                     dcs_mwf_online** out) {
    if (out) *out = nullptr;
    if (!ctx || !out) DCS_FAIL(DCS_EINVAL, "dcs_mwf_online_create: null argument");
    DCS_CHECK(dcs_mwf_online_check("dcs_mwf_online_create", F, J, niter, forget, loading, eps));
    DCS_ON_DEVICE(ctx->device);
    dcs_mwf_online* h = new dcs_mwf_online();
    h->ctx = ctx;
    h->F = F;
    h->J = J;
    h->niter = niter;
    h->forget = forget;
    h->loading = loading;
    h->eps = eps;
    h->bytes = online_state_bytes(F, J);
    const hipError_t e = dcs_dev_alloc((void**)&h->state, (size_t)h->bytes, "mwf_online state");
    if (e != hipSuccess) {
        delete h;
        DCS_HIP(e);
    }
    *out = h;
    return DCS_OK;
}

extern "C" int dcs_mwf_online_destroy(dcs_mwf_online* h) {
    if (!h) return DCS_OK;
    DCS_ON_DEVICE(h->ctx->device);
    if (h->state) {
        (void)hipStreamSynchronize(h->ctx->stream);
        dcs_dev_free(h->state);
    }
    delete h;
    return DCS_OK;
}

extern "C" int dcs_mwf_online_reset(dcs_mwf_online* h) {
    if (!h) DCS_FAIL(DCS_EINVAL, "dcs_mwf_online_reset: null handle");
    h->frames = 0;                                    // frame 0 reads no state: nothing to clear on the device
    return DCS_OK;
}

extern "C" int64_t dcs_mwf_online_bytes(const dcs_mwf_online* h) { return h ? h->bytes : -1; }
extern "C" int64_t dcs_mwf_online_frames(const dcs_mwf_online* h) { return h ? h->frames : -1; }

extern "C" int dcs_mwf_online_push_f32(dcs_mwf_online* h, const float* mag_d, const float* phase_d, int64_t ch_stride,
                                       const float* src_d, int64_t src_ch_stride, int64_t src_stride, int64_t ld, int64_t n_frames,
                                       float pre_div, float* out_mag_d, float* out_phase_d) {
    if (!h) DCS_FAIL(DCS_EINVAL, "dcs_mwf_online_push_f32: null handle");
    if (ld < h->F || n_frames < 0)
        DCS_FAIL(DCS_EINVAL, "dcs_mwf_online_push_f32: bad shape (F %d, ld %lld, n_frames %lld)", h->F, (long long)ld,
                 (long long)n_frames);
    if (!(pre_div > 0.f)) DCS_FAIL(DCS_EINVAL, "dcs_mwf_online_push_f32: pre_div %g must be positive", pre_div);
    if (!mag_d || !phase_d || !src_d || !out_mag_d || !out_phase_d) DCS_FAIL(DCS_EINVAL, "dcs_mwf_online_push_f32: null buffer");
    if (n_frames > INT64_MAX / ld) DCS_FAIL(DCS_EINVAL, "dcs_mwf_online_push_f32: %lld frames of %lld", (long long)n_frames, (long long)ld);
    const int64_t plane = n_frames * ld;
    if (ch_stride < plane || src_ch_stride < plane || src_stride < plane)
        DCS_FAIL(DCS_EINVAL, "dcs_mwf_online_push_f32: strides (%lld, %lld, %lld) below %lld frames of %lld", (long long)ch_stride,
                 (long long)src_ch_stride, (long long)src_stride, (long long)n_frames, (long long)ld);
    if (n_frames == 0) return DCS_OK;
    dcs_ctx* ctx = h->ctx;
    DCS_ON_DEVICE(ctx->device);

    OnlineArgs a;
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
    a.F = h->F;
    a.niter = h->niter;
    a.fresh = h->frames == 0;
    a.pre_div = pre_div;
    a.forget = h->forget;
    a.loading = h->loading;
    a.eps = h->eps;
    a.state = h->state;
    const int n_blocks = dcs_cdiv(h->F, kBins);
    const dim3 block(kBins);

    DcsTimer t(ctx, DCS_TAG_MWF);
    if (h->niter == 0) {
        const dim3 grid(n_blocks, (unsigned)(n_frames < 64 ? n_frames : 64));
        hipLaunchKernelGGL(mwf_online_copy_kernel, grid, block, 0, ctx->stream, a, h->J);
    } else {
        const dim3 grid(n_blocks);
        switch (h->J) {
            case 1: hipLaunchKernelGGL(mwf_online_kernel<1>, grid, block, 0, ctx->stream, a); break;
            case 2: hipLaunchKernelGGL(mwf_online_kernel<2>, grid, block, 0, ctx->stream, a); break;
            case 3: hipLaunchKernelGGL(mwf_online_kernel<3>, grid, block, 0, ctx->stream, a); break;
            case 4: hipLaunchKernelGGL(mwf_online_kernel<4>, grid, block, 0, ctx->stream, a); break;
            case 5: hipLaunchKernelGGL(mwf_online_kernel<5>, grid, block, 0, ctx->stream, a); break;
            case 6: hipLaunchKernelGGL(mwf_online_kernel<6>, grid, block, 0, ctx->stream, a); break;
            case 7: hipLaunchKernelGGL(mwf_online_kernel<7>, grid, block, 0, ctx->stream, a); break;
            default: hipLaunchKernelGGL(mwf_online_kernel<8>, grid, block, 0, ctx->stream, a); break;
        }
    }
    DCS_HIP(hipGetLastError());
    t.done();
    h->frames += n_frames;
    return DCS_OK;
}

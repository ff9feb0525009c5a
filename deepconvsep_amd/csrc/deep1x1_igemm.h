// The implicit-GEMM convolution kernel of build_ca_1x1 (deep1x1.hip describes the graph and the operand layouts), shared by
// the separator (deep1x1.hip) and the trainer (train_deep1x1.hip).  MODE_FWD .. MODE_LAST are the separator's; MODE_FWDC,
// MODE_Q and MODE_B11 exist for the training step only and leave the other instantiations as they were.
#pragma once

#include "dcs_internal.h"

namespace d1 {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMT = 2;                      // 16-pixel MFMA tiles per wave
constexpr int kBM = kWaves * kMT * 16;      // 128 output pixels per workgroup
constexpr int kChunk = 32;                  // tiles per pass: bounds the scratch whatever the batch
constexpr int kLayers = 6;
constexpr int kKw = 5;
constexpr int kNf = 200;                    // filters of conv6 / of one branch of the 1x1 conv (nfilt_conv)
const int kFilters[kLayers] = {30, 50, 70, 100, 200, 200};
const int kKh[kLayers] = {1, 1, 1, 1, 10, 10};

typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { MODE_FWD = 0, MODE_1X1 = 1, MODE_TR = 2, MODE_LAST = 3, MODE_FWDC = 4, MODE_Q = 5, MODE_B11 = 6 };
// training only: FWDC a forward convolution times the saved code of its output (the decoder's backward step); Q the last
// transposed convolution plus the final bias, not rectified, as [img][N][Ho][Wo]; B11 the 1x1 layer's transposed product

struct D1Args {
    const float* in;            // channels-last [img][Hi][Wi][Ci]
    const uint8_t* code;        // MODE_TR / MODE_LAST / MODE_Q / MODE_B11: r'(pre) codes of `in`, same layout; MODE_FWDC: of `out`
    int Hi, Wi, Ci;             // Ci a multiple of 4; the contiguous run of K the kernel steps through -- ntap Ci floats (FWD: one
                                // filter row of a pixel) or Ci floats (TR: one tap) -- holds at least 16: the walk (ki, kr) /
                                // (ki, jt, c) starts at 4 (lane >> 4) without wrapping.  The graph's smallest are 20 and 32.
    int Ho, Wo, Wq, par;       // output rows / columns; this launch's columns q -> f = stride q (FWD) or 2 q + par (TR)
    int kh, ntap, stride;
    const float* B;             // [Npad][Kpad] weights, one output channel's K contiguous, zero past K and past N
    int K, Kpad, N;
    const float* b0;            // FWD / 1X1: the layer's b; LAST: this branch's slice of the final BiasLayer
    const float* b1;            // FWD / 1X1: BiasLayer.b
    float* out;                 // FWD / TR: [img][Ho][Wo][Co]; 1X1: [branch][pixel][kNf]; LAST: [ch][n_total][Ho][Wo]
    uint8_t* code_out;          // FWD: [img][Ho][Wo][Co]
    int Co;                     // FWD / TR: channel pitch of `out` (channels N .. Co-1 are written 0)
    int64_t M;                  // output pixels of this launch
    int64_t n_total, k_first;   // LAST: tiles of the whole output, first tile of this chunk
    int ch_off;                 // LAST: output channel of this branch's first source
};

template <int MODE, int NT>
__global__ __launch_bounds__(kThreads) void d1_igemm_kernel(const D1Args a) {
    constexpr bool kTr = MODE == MODE_TR || MODE == MODE_LAST || MODE == MODE_Q || MODE == MODE_B11;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.x * kBM + wave * (kMT * 16);
    const int n0 = blockIdx.y * (NT * 16);
    const int64_t img_px = (int64_t)a.Ho * a.Wq;

    int64_t base[kMT];
    int trow[kMT], fcol[kMT];
    bool ok[kMT];
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt) {
        const int64_t m = m0 + mt * 16 + r16;
        ok[mt] = m < a.M;
        const int64_t mm = ok[mt] ? m : 0;
        const int64_t img = mm / img_px;
        const int rem = (int)(mm - img * img_px);
        const int t = rem / a.Wq, q = rem - t * a.Wq;
        trow[mt] = t;
        fcol[mt] = q;
        base[mt] = kTr ? img * a.Hi * a.Wi * (int64_t)a.Ci
                       : ((img * a.Hi + t) * (int64_t)a.Wi + (int64_t)a.stride * q) * a.Ci;
    }
    const float* Bp[NT];
#pragma unroll
    for (int s = 0; s < NT; ++s) Bp[s] = a.B + (int64_t)(n0 + s * 16 + r16) * a.Kpad + 4 * kq;

    f32x4 acc[kMT][NT];
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
        for (int s = 0; s < NT; ++s) acc[mt][s] = f32x4{0.f, 0.f, 0.f, 0.f};

    // this lane's K quad k0 + 4 kq as (filter row ki, offset kr in the row) -- TR: (row ki, tap jt, channel c)
    const int seg = a.ntap * a.Ci;
    const int64_t row_pitch = (int64_t)a.Wi * a.Ci;
    int ki = 0, kr = 4 * kq, jt = 0, c = 4 * kq;
    for (int k0 = 0; k0 < a.Kpad; k0 += 16) {
        const bool kin = k0 + 4 * kq < a.K;
        f32x4 av[kMT];
#pragma unroll
        for (int mt = 0; mt < kMT; ++mt) {
            av[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (!kTr) {
                if (ok[mt] && kin) av[mt] = *(const f32x4*)(a.in + base[mt] + ki * row_pitch + kr);
            } else {
                const int t = trow[mt] - ki, f = fcol[mt] - jt;
                if (ok[mt] && kin && t >= 0 && t < a.Hi && f >= 0 && f < a.Wi) {
                    const int64_t off = base[mt] + ((int64_t)t * a.Wi + f) * a.Ci + c;
                    const f32x4 g = *(const f32x4*)(a.in + off);
                    const uint32_t cd = *(const uint32_t*)(a.code + off);
                    av[mt] = f32x4{g[0] * (0.5f * (float)(cd & 0xff)), g[1] * (0.5f * (float)((cd >> 8) & 0xff)),
                                   g[2] * (0.5f * (float)((cd >> 16) & 0xff)), g[3] * (0.5f * (float)(cd >> 24))};
                }
            }
        }
        f32x4 bv[NT];
#pragma unroll
        for (int s = 0; s < NT; ++s) bv[s] = *(const f32x4*)(Bp[s] + k0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
                for (int s = 0; s < NT; ++s)
                    acc[mt][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mt][e], bv[s][e], acc[mt][s], 0, 0, 0);
        if (!kTr) {
            kr += 16;
            while (kr >= seg) { kr -= seg; ++ki; }
        } else {
            c += 16;
            while (c >= a.Ci) {
                c -= a.Ci;
                if (++jt == a.ntap) { jt = 0; ++ki; }
            }
        }
    }

    // C/D map of the 16x16 tile: column = lane & 15, row = 4 (lane >> 4) + reg
#pragma unroll
    for (int mt = 0; mt < kMT; ++mt)
#pragma unroll
        for (int s = 0; s < NT; ++s)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t m = m0 + mt * 16 + 4 * kq + reg;
                const int col = n0 + s * 16 + r16;
                if (m >= a.M) continue;
                const float v = acc[mt][s][reg];
                if (MODE == MODE_FWD) {
                    if (col >= a.Co) continue;
                    float y = 0.f;
                    uint8_t cd = 0;
                    if (col < a.N) {
                        const float pre = v + a.b0[col];
                        cd = pre > 0.f ? 2 : (pre == 0.f ? 1 : 0);
                        y = fmaxf(pre, 0.f) + a.b1[col];
                    }
                    a.out[m * a.Co + col] = y;
                    a.code_out[m * a.Co + col] = cd;
                } else if (MODE == MODE_1X1) {
                    if (col >= a.N) continue;
                    const int br = col / kNf;
                    a.out[((int64_t)br * a.M + m) * kNf + (col - br * kNf)] = fmaxf(v + a.b0[col], 0.f) + a.b1[col];
                } else if (MODE == MODE_FWDC) {
                    if (col >= a.Co) continue;
                    a.out[m * a.Co + col] = col < a.N ? v * (0.5f * (float)a.code[m * a.Co + col]) : 0.f;
                } else if (MODE == MODE_B11) {
                    if (col >= a.Co) continue;
                    a.out[m * a.Co + col] = col < a.N ? v : 0.f;
                } else {
                    const int64_t img = m / img_px;
                    const int rem = (int)(m - img * img_px);
                    const int t = rem / a.Wq, f = 2 * (rem - t * a.Wq) + a.par;
                    if (MODE == MODE_TR) {
                        if (col >= a.Co) continue;
                        a.out[((img * a.Ho + t) * (int64_t)a.Wo + f) * a.Co + col] = col < a.N ? v : 0.f;
                    } else if (MODE == MODE_Q) {
                        if (col >= a.N) continue;
                        a.out[((img * a.N + col) * a.Ho + t) * (int64_t)a.Wo + f] = v + a.b0[col];
                    } else {
                        if (col >= a.N) continue;
                        const int64_t ch = a.ch_off + col;
                        a.out[((ch * a.n_total + a.k_first + img) * a.Ho + t) * (int64_t)a.Wo + f] = fmaxf(v + a.b0[col], 0.f);
                    }
                }
            }
}

// tiles [n][C][tc][F] -> channels-last [n][tc][F][C] (C == 4)
__global__ __launch_bounds__(kThreads) void d1_to_cl_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n_px,
                                                            int64_t plane) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_px) return;
    const int64_t k = i / plane, r = i - k * plane;
    const float* s = x + k * 4 * plane + r;
    *(f32x4*)(y + 4 * i) = f32x4{s[0], s[plane], s[2 * plane], s[3 * plane]};
}

int nt_for(int N) { return N <= 16 ? 1 : (N <= 32 ? 2 : 4); }

int npad_for(int N) { return dcs_cdiv(N, 16 * nt_for(N)) * 16 * nt_for(N); }   // rows of a B operand with N live ones

// The geometry of a forward-type launch (MODE_FWD, MODE_1X1, MODE_FWDC): `images` images of [Hi][Wi][Cip] channels-last, a
// valid kh x ntap convolution with column stride `stride` to N channels.  Operands, biases and outputs are the caller's.
D1Args forward_args(int64_t images, int Hi, int Wi, int Cip, int kh, int ntap, int stride, int N) {
    D1Args a{};
    a.Hi = Hi; a.Wi = Wi; a.Ci = Cip;
    a.Ho = Hi - kh + 1; a.Wo = (Wi - ntap) / stride + 1; a.Wq = a.Wo;
    a.kh = kh; a.ntap = ntap; a.stride = stride;
    a.K = kh * ntap * Cip; a.Kpad = (int)dcs_round_up(a.K, 16); a.N = N;
    a.M = images * a.Ho * a.Wo;
    return a;
}

// The geometry of one parity of a transposed-type launch (MODE_TR, MODE_LAST, MODE_Q, MODE_B11): the transpose of a valid
// kh x kw convolution (kw == 5: column stride 2; kw == 1: the 1x1 layer, stride 1, parity 0 alone) that took [Ho][Wo] to
// [Hi][Wi]; `in` is [images][Hi][Wi][Cip], the launch writes the output columns f = stride q + par, q < Wq.  M may be 0 (a
// parity with no column): the caller skips that launch.
D1Args transposed_args(int64_t images, int Hi, int Wi, int Cip, int Ho, int Wo, int kh, int kw, int par, int N) {
    const int stride = kw == 1 ? 1 : 2;
    D1Args a{};
    a.Hi = Hi; a.Wi = Wi; a.Ci = Cip;
    a.Ho = Ho; a.Wo = Wo; a.Wq = (Wo - par + stride - 1) / stride; a.par = par;
    a.kh = kh; a.ntap = (kw - par + stride - 1) / stride;
    a.K = kh * a.ntap * Cip; a.Kpad = (int)dcs_round_up(a.K, 16); a.N = N;
    a.M = images * Ho * a.Wq;
    return a;
}

template <int MODE>
void launch(dcs_ctx* ctx, const D1Args& a) {
    const int nt = nt_for(a.N);
    const dim3 grid((unsigned)((a.M + kBM - 1) / kBM), (unsigned)dcs_cdiv(a.N, 16 * nt));
    if (nt == 1) hipLaunchKernelGGL((d1_igemm_kernel<MODE, 1>), grid, dim3(kThreads), 0, ctx->stream, a);
    else if (nt == 2) hipLaunchKernelGGL((d1_igemm_kernel<MODE, 2>), grid, dim3(kThreads), 0, ctx->stream, a);
    else hipLaunchKernelGGL((d1_igemm_kernel<MODE, 4>), grid, dim3(kThreads), 0, ctx->stream, a);
}

}  // namespace
}  // namespace d1

// The training core (train_core.h): the f32-MFMA GEMM template and its split-K helpers, Adadelta and Adam, rectify, the
// window gather, and the dcs_trainer_* entry points.  One step on the ctx stream is forward, loss, backward (the graph's) and
// the selected update, with no host synchronisation and no float atomics: two runs give bit-identical weights.
#include "train_core.h"

#include <cmath>

using namespace train;

namespace train {

Ax ax3(int64_t d0, int64_t d1, int64_t s0, int64_t s1, int64_t s2) {
    auto fdiv = [](int64_t d) {
        uint32_t s = 0;
        while ((int64_t(1) << s) < d) ++s;
        const uint64_t one = 1;
        return FDiv{(uint32_t)(((one << 32) * ((one << s) - (uint64_t)d)) / (uint64_t)d + 1), s};
    };
    const int64_t d01 = std::min<int64_t>(d0 * d1, kBig);
    return Ax{fdiv(d0), fdiv(d01), (int)d0, (int)d1, s0, s1, s2};
}

Gemm gemm0(int M, int N, int K) {
    Gemm g;
    memset(&g, 0, sizeof(g));
    g.M = M; g.N = N; g.K = K;
    g.ones_row = kBig;
    g.nbatch = 1;
    g.splits = 1;
    g.kchunk = K;
    g.bias_cs = 1;
    return g;
}

void pick_split(int64_t tiles, int64_t K, int* splits, int* kchunk, int64_t target, int64_t cap) {
    int64_t s = target / (tiles > 0 ? tiles : 1);
    s = s < 1 ? 1 : (s > cap ? cap : s);
    int64_t kc = dcs_round_up((K + s - 1) / s, kKT);
    if (kc < 256) kc = dcs_round_up(256 < K ? 256 : K, kKT);
    *kchunk = (int)kc;
    *splits = (int)((K + kc - 1) / kc);
}

__device__ __forceinline__ int fdq(int n, const FDiv f) {
    return (int)((__umulhi((uint32_t)n, f.m) + (uint32_t)n) >> f.s);
}

__device__ __forceinline__ int64_t ax_off(const Ax& a, int i) {
    const int q0 = fdq(i, a.q0), q2 = fdq(i, a.q01);
    return (int64_t)(i - q0 * a.d0) * a.s0 + (int64_t)(q0 - q2 * a.d1) * a.s1 + (int64_t)q2 * a.s2;
}

__device__ __forceinline__ float relu_d(float pre) { return pre > 0.f ? 1.f : (pre == 0.f ? 0.5f : 0.f); }

typedef float f32x4 __attribute__((ext_vector_type(4)));

// AK: A is loaded K-fastest (lane = k), else M-fastest (lane = m); BK likewise for B (K-fastest, else N-fastest).
template <int WM, int WN, int FM, int FN, bool AK, bool BK>
__global__ __launch_bounds__(kThreads) void gemm_kernel(const Gemm g) {
    constexpr int BM = WM * FM * 16, BN = WN * FN * 16;
    constexpr int NA = BM * kKT / kThreads, NB = BN * kKT / kThreads;
    static_assert(WM * WN == 4, "four waves");
    __shared__ float As[kKT][BM + 1];
    __shared__ float Bs[kKT][BN + 1];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int wm = (wave / WN) * FM * 16, wn = (wave % WN) * FN * 16;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int batch = blockIdx.z / g.splits, split = blockIdx.z - batch * g.splits;
    const int kbeg = split * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const float* Ap = g.A.p + g.A.off + g.boff[batch][0];
    const float* Bp = g.B.p + g.B.off + g.boff[batch][1];

    // A: AK -> k = t % 32, rows t / 32 + 8 j;  else rows t % BM, k = t / BM + (256 / BM) j
    const int akl = AK ? (t & 31) : t / BM;
    const int aml = AK ? (t >> 5) : t % BM;
    int64_t arow[AK ? NA : 1];
    bool aok[AK ? NA : 1], aone[AK ? NA : 1];
#pragma unroll
    for (int j = 0; j < (AK ? NA : 1); ++j) {
        const int m = m0 + aml + (AK ? 8 * j : 0);
        aok[j] = m < g.M;
        aone[j] = m >= g.ones_row;
        arow[j] = (aok[j] && !aone[j]) ? ax_off(g.A.r, m) : 0;
    }
    // B: BK -> k = t % 32, columns t / 32 + 8 j;  else columns t % BN, k = t / BN + (256 / BN) j
    const int bkl = BK ? (t & 31) : t / BN;
    const int bnl = BK ? (t >> 5) : t % BN;
    int64_t bcol[BK ? NB : 1];
    bool bok[BK ? NB : 1];
#pragma unroll
    for (int j = 0; j < (BK ? NB : 1); ++j) {
        const int n = n0 + bnl + (BK ? 8 * j : 0);
        bok[j] = n < g.N;
        bcol[j] = bok[j] ? ax_off(g.B.c, n) : 0;
    }

    float ra[NA], rb[NB];
    auto load = [&](int k0) {
        if constexpr (AK) {
            const int ka = k0 + akl;
            const bool kin = ka < kend;
            const int64_t acol = kin ? ax_off(g.A.c, ka) : 0;
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                float v = 0.f;
                if (aok[j] && kin) v = aone[j] ? (ka < g.ones_klim ? 1.f : 0.f) : Ap[arow[j] + acol];
                ra[j] = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const int ka = k0 + akl + (kThreads / BM) * j;
                float v = 0.f;
                if (aok[0] && ka < kend) v = aone[0] ? (ka < g.ones_klim ? 1.f : 0.f) : Ap[arow[0] + ax_off(g.A.c, ka)];
                ra[j] = v;
            }
        }
        if constexpr (BK) {
            const int kb = k0 + bkl;
            const bool kin = kb < kend;
            const int64_t brow = kin ? ax_off(g.B.r, kb) : 0;
#pragma unroll
            for (int j = 0; j < NB; ++j) rb[j] = (bok[j] && kin) ? Bp[brow + bcol[j]] : 0.f;
        } else {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int kb = k0 + bkl + (kThreads / BN) * j;
                rb[j] = (bok[0] && kb < kend) ? Bp[ax_off(g.B.r, kb) + bcol[0]] : 0.f;
            }
        }
    };

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (kbeg < kend) load(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += kKT) {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            if constexpr (AK) As[akl][aml + 8 * j] = ra[j];
            else As[akl + (kThreads / BM) * j][aml] = ra[j];
        }
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            if constexpr (BK) Bs[bkl][bnl + 8 * j] = rb[j];
            else Bs[bkl + (kThreads / BN) * j][bnl] = rb[j];
        }
        __syncthreads();
        if (k0 + kKT < kend) load(k0 + kKT);
#pragma unroll
        for (int s = 0; s < kKT / 4; ++s) {
            const int kk = 4 * s + kq;
            float a[FM], b[FN];
#pragma unroll
            for (int i = 0; i < FM; ++i) a[i] = As[kk][wm + 16 * i + r16];
#pragma unroll
            for (int j = 0; j < FN; ++j) b[j] = Bs[kk][wn + 16 * j + r16];
#pragma unroll
            for (int i = 0; i < FM; ++i)
#pragma unroll
                for (int j = 0; j < FN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // C/D map of the 16x16 tile: column = lane & 15, row = 4 (lane >> 4) + reg
    const float sc = g.scale ? *g.scale : 1.f;
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int m = m0 + wm + 16 * i + 4 * kq + reg;
                const int n = n0 + wn + 16 * j + r16;
                if (m >= g.M || n >= g.N) continue;
                float v = acc[i][j][reg];
                if (g.partial) {
                    g.partial[((int64_t)blockIdx.z * g.M + m) * g.N + n] = v;
                    continue;
                }
                v *= sc;
                if (g.bias) v += g.bias[g.boff[batch][4] + (int64_t)n * g.bias_cs];
                if (g.bias2) v += g.bias2[g.boff[batch][4] + (int64_t)n * g.bias_cs];
                if (g.epi & (EPI_SAVEPRE | EPI_DRELU)) {
                    float* x = g.X.p + g.X.off + g.boff[batch][3] + ax_off(g.X.r, m) + ax_off(g.X.c, n);
                    if (g.epi & EPI_SAVEPRE) *x = v;
                    else v *= relu_d(*x);
                }
                if (g.epi & EPI_RELU) v = v > 0.f ? v : 0.f;
                g.C.p[g.C.off + g.boff[batch][2] + ax_off(g.C.r, m) + ax_off(g.C.c, n)] = v;
            }
}

__global__ __launch_bounds__(kThreads) void finish_kernel(const float* __restrict__ part, int splits, int64_t count, int N,
                                                          const float* bias, float* C, float* X, int epi) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= count) return;
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += part[z * count + i];
    if (bias) s += bias[i % N];
    if (epi & EPI_SAVEPRE) X[i] = s;
    if (epi & EPI_DRELU) s *= relu_d(X[i]);
    if (epi & EPI_RELU) s = s > 0.f ? s : 0.f;
    C[i] = s;
}

__global__ __launch_bounds__(kThreads) void reduce_kernel(const Reduce r) {
    const int j = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= r.count[j]) return;
    float s = 0.f;
    for (int z = 0; z < r.splits[j]; ++z) s += r.part[j][z * r.count[j] + i];
    s *= *r.scale;
    r.dst[j][i] = s;
    if (r.dup[j] && i >= r.count[j] - r.N[j]) r.dst[j][i + r.N[j]] = s;
}

// lasagne.updates.adadelta (lasagne/updates.py adadelta): accu' = rho accu + (1 - rho) g^2,
// u = g sqrt(delta + eps) / sqrt(accu' + eps), p -= lr u, delta' = rho delta + (1 - rho) u^2.  P4: the section length in
// float4s (sections are padded to a multiple of four floats; the pad stays zero).
__global__ __launch_bounds__(kThreads) void adadelta_kernel(float4* __restrict__ state, int64_t P4, float lr, float rho,
                                                            float eps) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= P4) return;
    const float4 g = state[P4 + i];
    float4 p = state[i], acc = state[2 * P4 + i], del = state[3 * P4 + i];
    float* pp = &p.x;
    float* pa = &acc.x;
    float* pd = &del.x;
    const float* pg = &g.x;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const float gi = pg[l];
        const float a = rho * pa[l] + (1.f - rho) * gi * gi;
        const float u = gi * sqrtf(pd[l] + eps) / sqrtf(a + eps);
        pp[l] = pp[l] - lr * u;
        pa[l] = a;
        pd[l] = rho * pd[l] + (1.f - rho) * u * u;
    }
    state[i] = p;
    state[2 * P4 + i] = acc;
    state[3 * P4 + i] = del;
}

// lasagne.updates.adam (lasagne/updates.py adam): m' = beta1 m + (1 - beta1) g, v' = beta2 v + (1 - beta2) g^2,
// p -= a_t m' / (sqrt(v') + eps) with a_t = lr sqrt(1 - beta2^t) / (1 - beta1^t) from the host (eps is outside the bias
// correction).  m sits in adadelta_kernel's accu slot and v in its delta_accu slot; omb1 = 1 - beta1 and omb2 = 1 - beta2
// come rounded from double (1.f - 0.999f is 1.3e-5 off 0.001).  g = m = v = 0 gives a step of exactly 0.
__global__ __launch_bounds__(kThreads) void adam_kernel(float4* __restrict__ state, int64_t P4, float a_t, float beta1,
                                                        float omb1, float beta2, float omb2, float eps) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= P4) return;
    const float4 g = state[P4 + i];
    float4 p = state[i], m = state[2 * P4 + i], v = state[3 * P4 + i];
    float* pp = &p.x;
    float* pm = &m.x;
    float* pv = &v.x;
    const float* pg = &g.x;
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        const float gi = pg[l];
        pm[l] = beta1 * pm[l] + omb1 * gi;
        pv[l] = beta2 * pv[l] + omb2 * gi * gi;
        pp[l] = pp[l] - a_t * pm[l] / (sqrtf(pv[l]) + eps);
    }
    state[i] = p;
    state[2 * P4 + i] = m;
    state[3 * P4 + i] = v;
}

__global__ __launch_bounds__(kThreads) void relu_kernel(const float* __restrict__ q, float* __restrict__ p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) p[i] = q[i] > 0.f ? q[i] : 0.f;
}

// (file, start) windows of the resident [1 + nsrc][T][F] feature files -> network inputs and targets (dataset.py loadFile /
// initOutput): data [sum_i (1 + nsrc) T_i F] float32, file i at files[2 i] with T_i = files[2 i + 1] frames; win [B][2];
// file < 0: an all-zero window; frames past T_i are zero (the padded window of a file shorter than tc).
__global__ __launch_bounds__(kThreads) void gather_kernel(const float* __restrict__ data, const int64_t* __restrict__ files,
                                                          const int* __restrict__ win, int B, int tc, int F, int nsrc,
                                                          float scale, float* __restrict__ inputs,
                                                          float* __restrict__ targets) {
    const int64_t plane = (int64_t)tc * F;
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (int64_t)B * plane) return;
    const int b = (int)(e / plane);
    const int64_t rem = e - b * plane;
    const int t = (int)(rem / F), f = (int)(rem - (int64_t)t * F);
    const int fi = win[2 * b], start = win[2 * b + 1];
    const int64_t fr = (int64_t)start + t;
    int64_t base = 0, T = 0;
    bool live = false;
    if (fi >= 0) {
        base = files[2 * fi];
        T = files[2 * fi + 1];
        live = fr < T;
    }
    for (int c = 0; c <= nsrc; ++c) {
        const float v = live ? scale * data[base + ((int64_t)c * T + fr) * F + f] : 0.f;
        if (c == 0) inputs[e] = v;
        else targets[((int64_t)b * nsrc + c - 1) * plane + rem] = v;
    }
}

// gather_kernel for files that hold the `in` tensor's cin channels, then the `out` tensor's cout: [cin + cout][T][F]
// (dataset.py LargeDatasetMulti: the *_in_m_.data / *_out_m_.data pair of one chunk), each with its own factor.
__global__ __launch_bounds__(kThreads) void gather_channels_kernel(const float* __restrict__ data,
                                                                   const int64_t* __restrict__ files,
                                                                   const int* __restrict__ win, int B, int tc, int F, int cin,
                                                                   int cout, float scale_in, float scale_out,
                                                                   float* __restrict__ inputs, float* __restrict__ targets) {
    const int64_t plane = (int64_t)tc * F;
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (int64_t)B * plane) return;
    const int b = (int)(e / plane);
    const int64_t rem = e - b * plane;
    const int t = (int)(rem / F), f = (int)(rem - (int64_t)t * F);
    const int fi = win[2 * b], start = win[2 * b + 1];
    const int64_t fr = (int64_t)start + t;
    int64_t base = 0, T = 0;
    bool live = false;
    if (fi >= 0) {
        base = files[2 * fi];
        T = files[2 * fi + 1];
        live = fr < T;
    }
    for (int c = 0; c < cin + cout; ++c) {
        const float raw = live ? data[base + ((int64_t)c * T + fr) * F + f] : 0.f;
        if (c < cin) inputs[((int64_t)b * cin + c) * plane + rem] = live ? scale_in * raw : 0.f;
        else targets[((int64_t)b * cout + c - cin) * plane + rem] = live ? scale_out * raw : 0.f;
    }
}

// The score-informed feed (dataset.py LargeDatasetMask2: loadFile :383-488 with filterSpec :839-879, then
// trainCNNrwc.py:309-320), one workgroup per (frame, window): targets[b][j][t][f] = scale source_j and inputs[b][j][t][f] =
// mask_j (scale mixture) with mask_j = filtered_j / sum_i filtered_i in float32 (instruments added in order), filtered = 1 on
// the rectangles of instrument j's notes and 1e-18 elsewhere; every product is rounded once to float32.  data as for
// gather_kernel with [1 + ninst][T][F] blocks.  notes: per file (note_files[2 i] = offset in ints, note_files[2 i + 1] = P
// notes per instrument) an int table [ninst][P][2 + 2 npairs] = (first frame, end frame, npairs x (first bin, end bin)),
// packed and range-checked by dcs_trainer_pack_score: a note paints frames first <= start + t < end of its window, which is
// filterSpec's int(max(n0, start)) - start .. int(min(n1, stop)) - start for integer start and stop.
// The workgroup first marks in LDS, one bit per instrument, the bins of the notes that sound in its frame (integer OR: the
// order does not matter), kScoreBins bins at a time, then sweeps the bins.
constexpr int kScoreBins = 4096;

__global__ __launch_bounds__(kThreads) void gather_score_kernel(const float* __restrict__ data, const int64_t* __restrict__ files,
                                                                const int* __restrict__ notes,
                                                                const int64_t* __restrict__ note_files,
                                                                const int* __restrict__ win, int tc, int F, int ninst,
                                                                int npairs, float scale, float* __restrict__ inputs,
                                                                float* __restrict__ targets) {
    __shared__ unsigned on[kScoreBins];
    const int t = blockIdx.x, b = blockIdx.y;
    const int fi = win[2 * b], start = win[2 * b + 1];
    const int64_t fr = (int64_t)start + t;
    const int64_t plane = (int64_t)tc * F;
    const int64_t out0 = (int64_t)b * ninst * plane + (int64_t)t * F;
    int64_t base = 0, T = 0;
    bool live = false;
    if (fi >= 0) {
        base = files[2 * fi];
        T = files[2 * fi + 1];
        live = fr < T;
    }
    if (!live) {   // uniform over the workgroup
        for (int j = 0; j < ninst; ++j)
            for (int f = threadIdx.x; f < F; f += kThreads) {
                inputs[out0 + j * plane + f] = 0.f;
                targets[out0 + j * plane + f] = 0.f;
            }
        return;
    }
    const int* tab = notes + note_files[2 * fi];
    const int P = (int)note_files[2 * fi + 1];
    const int width = 2 + 2 * npairs;
    const float* mix = data + base + fr * F;
    for (int c0 = 0; c0 < F; c0 += kScoreBins) {
        const int c1 = min(F, c0 + kScoreBins);
        for (int f = threadIdx.x; f < c1 - c0; f += kThreads) on[f] = 0u;
        __syncthreads();
        for (int i = threadIdx.x; i < ninst * P; i += kThreads) {
            const int* n = tab + (int64_t)i * width;
            if (fr < n[0] || fr >= n[1]) continue;
            const unsigned bit = 1u << (i / P);
            for (int k = 0; k < npairs; ++k) {
                const int f0 = max(n[2 + 2 * k], c0), f1 = min(n[3 + 2 * k], c1);
                for (int f = f0; f < f1; ++f) atomicOr(&on[f - c0], bit);
            }
        }
        __syncthreads();
        for (int f = c0 + threadIdx.x; f < c1; f += kThreads) {
            const unsigned m = on[f - c0];
            float total = 0.f;
            for (int j = 0; j < ninst; ++j) {
                const float v = ((m >> j) & 1u) ? 1.0f : 1e-18f;
                total = j == 0 ? v : total + v;
            }
            const float x = scale * mix[f];
            for (int j = 0; j < ninst; ++j) {
                const float v = (((m >> j) & 1u) ? 1.0f : 1e-18f) / total;
                inputs[out0 + j * plane + f] = v * x;
                targets[out0 + j * plane + f] = scale * data[base + ((int64_t)(j + 1) * T + fr) * F + f];
            }
        }
        __syncthreads();
    }
}

}  // namespace train

namespace {

template <int WM, int WN, int FM, int FN>
void launch_tile(const Gemm& g, bool ak, bool bk, dim3 grid, hipStream_t s) {
    if (ak && bk) hipLaunchKernelGGL((gemm_kernel<WM, WN, FM, FN, true, true>), grid, dim3(kThreads), 0, s, g);
    else if (ak) hipLaunchKernelGGL((gemm_kernel<WM, WN, FM, FN, true, false>), grid, dim3(kThreads), 0, s, g);
    else if (bk) hipLaunchKernelGGL((gemm_kernel<WM, WN, FM, FN, false, true>), grid, dim3(kThreads), 0, s, g);
    else hipLaunchKernelGGL((gemm_kernel<WM, WN, FM, FN, false, false>), grid, dim3(kThreads), 0, s, g);
}

int gather(dcs_ctx* ctx, const float* data_d, const int64_t* files_d, const int* windows_d, int batch, int time_context, int F,
           int nsrc, float scale, float* inputs_d, float* targets_d) {
    DCS_ON_DEVICE(ctx->device);
    const int64_t n = (int64_t)batch * time_context * F;
    hipLaunchKernelGGL(gather_kernel, dim3((unsigned)dcs_cdiv(n, kThreads)), dim3(kThreads), 0, ctx->stream, data_d, files_d,
                       windows_d, batch, time_context, F, nsrc, scale, inputs_d, targets_d);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

void trainer_free(dcs_trainer* t) {
    if (!t) return;
    dcs_dev_free(t->state);
    dcs_dev_free(t->work);
    delete t;
}

}  // namespace

int dcs_trainer::launch(Gemm g, Tile tile, bool ak, bool bk, dim3* grid_out) {
    if (g.splits < 1) g.splits = 1;
    if (g.splits == 1) g.kchunk = g.K;
    const int bm = tile == T128x32 ? 128 : (tile == T64x64 ? 64 : 32), bn = tile == T64x64 ? 64 : 32;
    dim3 grid((unsigned)dcs_cdiv(g.M, bm), (unsigned)dcs_cdiv(g.N, bn), (unsigned)(g.nbatch * g.splits));
    hipStream_t s = ctx->stream;
    if (tile == T128x32) launch_tile<4, 1, 2, 2>(g, ak, bk, grid, s);
    else if (tile == T64x64) launch_tile<2, 2, 2, 2>(g, ak, bk, grid, s);
    else launch_tile<2, 2, 1, 1>(g, ak, bk, grid, s);
    if (grid_out) *grid_out = grid;
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

int dcs_trainer::finish(const float* part, int splits, int N, const float* bias, float* C, float* X, int epi) {
    const int64_t count = (int64_t)B * N;
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)dcs_cdiv(count, kThreads)), dim3(kThreads), 0, ctx->stream, part, splits,
                       count, N, bias, C, X, epi);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

int dcs_trainer::codes(float* const*, int) {
    DCS_FAIL(DCS_EUNSUPPORTED, "dcs_trainer_rectify_codes: this graph keeps pre-activations, not codes (only arch %d has them)",
             DCS_ARCH_BACH10_SI_1X1);
}

int dcs_trainer::reduce(const Reduce& r) {
    const int64_t most = std::max(r.count[0], r.count[1]);
    hipLaunchKernelGGL(reduce_kernel, dim3((unsigned)dcs_cdiv(most, kThreads), 2), dim3(kThreads), 0, ctx->stream, r);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

// The graphs, one per file: range checks with their message, then a trainer with its geometry, nsrc, nparams, shapes and
// loss_sums set.
int dsd_trainer_new(int time_context, int F, int batch, dcs_trainer** out);
int ikala_trainer_new(int time_context, int F, int batch, dcs_trainer** out);
int bach10_trainer_new(int time_context, int F, int batch, dcs_trainer** out);
int dsdild_trainer_new(int time_context, int F, int batch, dcs_trainer** out);
int bach10si_trainer_new(int arch, int time_context, int F, int batch, dcs_trainer** out);
int deep1x1_trainer_new(int time_context, int F, int batch, const int64_t* shapes, int nparams, dcs_trainer** out);

extern "C" {

DCS_API int dcs_trainer_create(dcs_ctx* ctx, int arch, int time_context, int F, int batch, const float* const* params_d,
                               const int64_t* shapes, int nparams, const float* rand_d, const double* hyper_h,
                               dcs_trainer** out) {
    if (!ctx || !out || !rand_d || !hyper_h) DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: null argument");
    *out = nullptr;
    dcs_trainer* t = nullptr;
    if (arch == DCS_ARCH_DSD) DCS_CHECK(dsd_trainer_new(time_context, F, batch, &t));
    else if (arch == DCS_ARCH_IKALA_NOPOOL) DCS_CHECK(ikala_trainer_new(time_context, F, batch, &t));
    else if (arch == DCS_ARCH_BACH10) DCS_CHECK(bach10_trainer_new(time_context, F, batch, &t));
    else if (arch == DCS_ARCH_DSD_ILD) DCS_CHECK(dsdild_trainer_new(time_context, F, batch, &t));
    else if (arch == DCS_ARCH_BACH10_SI || arch == DCS_ARCH_BACH10_SI1)
        DCS_CHECK(bach10si_trainer_new(arch, time_context, F, batch, &t));
    else if (arch == DCS_ARCH_BACH10_SI_1X1)
        DCS_CHECK(deep1x1_trainer_new(time_context, F, batch, shapes, nparams, &t));
    else
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_trainer_create: only the DSD graph (arch %d), the no-pool iKala graph (arch %d), "
                 "the Bach10 graph (arch %d), the stereo DSD graph (arch %d) and the score-informed Bach10 graphs (arch %d, "
                 "%d, %d) train here", DCS_ARCH_DSD, DCS_ARCH_IKALA_NOPOOL, DCS_ARCH_BACH10, DCS_ARCH_DSD_ILD,
                 DCS_ARCH_BACH10_SI, DCS_ARCH_BACH10_SI1, DCS_ARCH_BACH10_SI_1X1);
    // from here on every return frees t
    struct Guard {
        dcs_trainer* t;
        ~Guard() { trainer_free(t); }
    } guard{t};
    if (!params_d || !shapes || nparams != t->nparams)
        DCS_FAIL(DCS_ESHAPE, "mismatch: got %d values to set %d parameters", nparams, t->nparams);
    for (int i = 0; i < nparams; ++i) {
        if (!params_d[i]) DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: parameter %d is null", i);
        const int64_t* want = t->shapes[i];
        for (int k = 0; k < 4; ++k)
            if (shapes[4 * i + k] != want[k])
                DCS_FAIL(DCS_ESHAPE, "mismatch: parameter %d has shape (%lld, %lld, %lld, %lld) but value to set has shape "
                         "(%lld, %lld, %lld, %lld)", i, (long long)want[0], (long long)want[1], (long long)want[2],
                         (long long)want[3], (long long)shapes[4 * i], (long long)shapes[4 * i + 1],
                         (long long)shapes[4 * i + 2], (long long)shapes[4 * i + 3]);
    }
    DCS_ON_DEVICE(ctx->device);
    t->ctx = ctx;
    t->tc = time_context; t->F = F; t->B = batch;
    t->RF = (int64_t)batch * time_context * F;
    memcpy(t->hyp, hyper_h, sizeof(t->hyp));
    for (int i = 0; i < 3; ++i) t->opt[i] = hyper_h[4 + i];   // the initial optimiser: Adadelta
    if (t->nstate == 0) {
        t->nstate = nparams;
        for (int i = 0; i < nparams; ++i)
            t->state_size[i] = t->shapes[i][0] * t->shapes[i][1] * t->shapes[i][2] * t->shapes[i][3];
    }
    for (int i = 0; i < t->nstate; ++i) t->off[i + 1] = t->off[i] + t->state_size[i];
    t->P = t->off[t->nstate];
    t->P4 = dcs_cdiv(t->P, 4);

    // one work buffer: the views, each rounded to 64 floats, then the f64 loss sums and out7
    std::vector<std::pair<float**, int64_t>> parts = {{&t->rnd, t->rand_planes * t->RF}, {&t->sign, 1}};
    t->plan(parts);
    int64_t total = 0;
    for (auto& p : parts) total += dcs_round_up(p.second, 64);
    const int64_t dbl = (int64_t)kLossBlocks * t->loss_sums + std::max(8, t->nout);
    hipError_t e = dcs_dev_alloc((void**)&t->state, 16 * t->P4 * sizeof(float), "trainer state");
    if (e == hipSuccess) e = dcs_dev_alloc((void**)&t->work, total * sizeof(float) + dbl * sizeof(double), "trainer work");
    if (e != hipSuccess)
        DCS_FAIL(e == hipErrorOutOfMemory ? DCS_ENOMEM : DCS_EHIP, "dcs_trainer_create: device allocation failed: %s",
                 hipGetErrorString(e));
    int64_t at = 0;
    for (auto& p : parts) {
        *p.first = t->work + at;
        at += dcs_round_up(p.second, 64);
    }
    t->lpart = (double*)(t->work + at);
    t->out7 = t->lpart + (int64_t)kLossBlocks * t->loss_sums;
    // zero everything (the graph's zero padding stays zero for good; grads, accu, delta_accu and the section pads start at
    // zero), then the params
    if (hipMemsetAsync(t->work, 0, total * sizeof(float) + dbl * sizeof(double), ctx->stream) != hipSuccess ||
        hipMemsetAsync(t->state, 0, 16 * t->P4 * sizeof(float), ctx->stream) != hipSuccess ||
        hipMemcpyAsync(t->rnd, rand_d, t->rand_planes * t->RF * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream) !=
            hipSuccess)
        DCS_FAIL(DCS_EHIP, "dcs_trainer_create: initialisation failed");
    DCS_CHECK(t->layout(t->state, (float* const*)params_d, 1));
    guard.t = nullptr;
    *out = t;
    return DCS_OK;
}

DCS_API int dcs_trainer_destroy(dcs_trainer* t) {
    if (!t) return DCS_OK;
    DCS_ON_DEVICE(t->ctx->device);
    DCS_HIP(hipStreamSynchronize(t->ctx->stream));
    trainer_free(t);
    return DCS_OK;
}

DCS_API int dcs_trainer_step(dcs_trainer* t, const float* inputs_d, const float* targets_d, int mode, double* out7_d) {
    if (!t || !inputs_d || !targets_d) DCS_FAIL(DCS_EINVAL, "dcs_trainer_step: null argument");
    const int stage2 = t->two_stage && mode >= 4;
    if (stage2) mode -= 4;
    if (mode < 0 || mode > 2)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_step: mode %d (0 loss, 1 gradients, 2 update%s)", mode + 4 * stage2,
                 t->two_stage ? "; + 4: the stage-2 loss" : "");
    t->stage2 = stage2;
    DCS_ON_DEVICE(t->ctx->device);
    DCS_CHECK(t->forward(inputs_d));
    DCS_CHECK(t->loss(inputs_d, targets_d, out7_d));
    if (mode == 0) return DCS_OK;
    DCS_CHECK(t->backward());
    if (mode == 1) return DCS_OK;
    const dim3 grid((unsigned)dcs_cdiv(t->P4, kThreads));
    const double* o = t->opt;
    if (t->opt_kind == DCS_OPT_ADAM) {
        // lasagne/updates.py adam: t = t_prev + 1 and a_t, in double on the host (the count never leaves it)
        const double n = (double)(t->steps + 1);
        const double a_t = o[0] * sqrt(1.0 - pow(o[2], n)) / (1.0 - pow(o[1], n));
        hipLaunchKernelGGL(adam_kernel, grid, dim3(kThreads), 0, t->ctx->stream, (float4*)t->state, t->P4, (float)a_t,
                           (float)o[1], (float)(1.0 - o[1]), (float)o[2], (float)(1.0 - o[2]), (float)o[3]);
    } else {
        hipLaunchKernelGGL(adadelta_kernel, grid, dim3(kThreads), 0, t->ctx->stream, (float4*)t->state, t->P4, (float)o[0],
                           (float)o[1], (float)o[2]);
    }
    DCS_HIP(hipGetLastError());
    ++t->steps;
    return DCS_OK;
}

DCS_API int dcs_trainer_set_optimizer(dcs_trainer* t, int kind, const double* hyper_h) {
    if (!t || !hyper_h) DCS_FAIL(DCS_EINVAL, "dcs_trainer_set_optimizer: null argument");
    if (kind != DCS_OPT_ADADELTA && kind != DCS_OPT_ADAM)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_set_optimizer: kind %d (%d adadelta, %d adam)", kind, DCS_OPT_ADADELTA, DCS_OPT_ADAM);
    const double* h = hyper_h;
    auto unit = [](double v) { return v >= 0.0 && v < 1.0; };   // false for a NaN
    if (!std::isfinite(h[0]) || h[0] < 0.0)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_set_optimizer: learning rate %g (finite, not negative)", h[0]);
    if (kind == DCS_OPT_ADADELTA) {
        if (!unit(h[1])) DCS_FAIL(DCS_EINVAL, "dcs_trainer_set_optimizer: adadelta rho %g (in [0, 1))", h[1]);
        if (!(h[2] > 0.0) || !std::isfinite(h[2]))
            DCS_FAIL(DCS_EINVAL, "dcs_trainer_set_optimizer: adadelta epsilon %g (finite, above 0)", h[2]);
    } else {
        if (!unit(h[1]) || !unit(h[2]))
            DCS_FAIL(DCS_EINVAL, "dcs_trainer_set_optimizer: adam beta1 %g, beta2 %g (each in [0, 1))", h[1], h[2]);
        if (!(h[3] > 0.0) || !std::isfinite(h[3]))
            DCS_FAIL(DCS_EINVAL, "dcs_trainer_set_optimizer: adam epsilon %g (finite, above 0)", h[3]);
    }
    DCS_ON_DEVICE(t->ctx->device);
    // the two accumulator slots are adjacent
    DCS_HIP(hipMemsetAsync(t->state + 8 * t->P4, 0, 8 * t->P4 * sizeof(float), t->ctx->stream));
    t->opt_kind = kind;
    for (int i = 0; i < 4; ++i) t->opt[i] = (kind == DCS_OPT_ADADELTA && i == 3) ? 0.0 : h[i];
    t->steps = 0;
    return DCS_OK;
}

DCS_API int dcs_trainer_get_optimizer(dcs_trainer* t, int* kind, double* hyper_h, int64_t* steps) {
    if (!t || !kind || !hyper_h || !steps) DCS_FAIL(DCS_EINVAL, "dcs_trainer_get_optimizer: null argument");
    *kind = t->opt_kind;
    memcpy(hyper_h, t->opt, sizeof(t->opt));
    *steps = t->steps;
    return DCS_OK;
}

DCS_API int dcs_trainer_set_steps(dcs_trainer* t, int64_t steps) {
    if (!t) DCS_FAIL(DCS_EINVAL, "dcs_trainer_set_steps: null argument");
    if (steps < 0) DCS_FAIL(DCS_EINVAL, "dcs_trainer_set_steps: %lld steps", (long long)steps);
    t->steps = steps;
    return DCS_OK;
}

DCS_API int dcs_trainer_set_rand(dcs_trainer* t, const float* rand_d) {
    if (!t || !rand_d) DCS_FAIL(DCS_EINVAL, "dcs_trainer_set_rand: null argument");
    DCS_ON_DEVICE(t->ctx->device);
    DCS_HIP(hipMemcpyAsync(t->rnd, rand_d, t->rand_planes * t->RF * sizeof(float), hipMemcpyDeviceToDevice, t->ctx->stream));
    return DCS_OK;
}

DCS_API int dcs_trainer_out_count(dcs_trainer* t, int* count) {
    if (!t || !count) DCS_FAIL(DCS_EINVAL, "dcs_trainer_out_count: null argument");
    *count = t->nout;
    return DCS_OK;
}

DCS_API int dcs_trainer_forward(dcs_trainer* t, const float* inputs_d, float* p_d) {
    if (!t || !inputs_d || !p_d) DCS_FAIL(DCS_EINVAL, "dcs_trainer_forward: null argument");
    DCS_ON_DEVICE(t->ctx->device);
    DCS_CHECK(t->forward(inputs_d));
    const int64_t n = t->nsrc * t->RF;
    hipLaunchKernelGGL(relu_kernel, dim3((unsigned)dcs_cdiv(n, kThreads)), dim3(kThreads), 0, t->ctx->stream,
                       (const float*)t->Q, p_d, n);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

DCS_API int dcs_trainer_get(dcs_trainer* t, int which, float* const* out_d, int nparams) {
    if (!t || !out_d) DCS_FAIL(DCS_EINVAL, "dcs_trainer_get: null argument");
    if (which < 0 || which > 3) DCS_FAIL(DCS_EINVAL, "dcs_trainer_get: which %d (0 params, 1 grads, 2 accu, 3 delta_accu)", which);
    if (nparams != t->nparams) DCS_FAIL(DCS_ESHAPE, "dcs_trainer_get: %d buffers for %d parameters", nparams, t->nparams);
    for (int i = 0; i < nparams; ++i)
        if (!out_d[i]) DCS_FAIL(DCS_EINVAL, "dcs_trainer_get: buffer %d is null", i);
    DCS_ON_DEVICE(t->ctx->device);
    return t->layout(t->state + which * 4 * t->P4, out_d, 0);
}

DCS_API int dcs_trainer_set(dcs_trainer* t, int which, const float* const* in_d, int nparams) {
    if (!t || !in_d) DCS_FAIL(DCS_EINVAL, "dcs_trainer_set: null argument");
    if (which != 0 && which != 2 && which != 3)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_set: which %d (0 params, 2 accu / m, 3 delta_accu / v; the gradients are not set)",
                 which);
    if (nparams != t->nparams)
        DCS_FAIL(DCS_ESHAPE, "mismatch: got %d values to set %d parameters", nparams, t->nparams);
    for (int i = 0; i < nparams; ++i)
        if (!in_d[i]) DCS_FAIL(DCS_EINVAL, "dcs_trainer_set: buffer %d is null", i);
    DCS_ON_DEVICE(t->ctx->device);
    return t->layout(t->state + which * 4 * t->P4, (float* const*)in_d, 1);
}

DCS_API int dcs_trainer_rectify_codes(dcs_trainer* t, float* const* out_d, int n) {
    if (!t || !out_d) DCS_FAIL(DCS_EINVAL, "dcs_trainer_rectify_codes: null argument");
    for (int i = 0; i < n; ++i)
        if (!out_d[i]) DCS_FAIL(DCS_EINVAL, "dcs_trainer_rectify_codes: buffer %d is null", i);
    DCS_ON_DEVICE(t->ctx->device);
    return t->codes(out_d, n);
}

DCS_API int dcs_trainer_gather(dcs_ctx* ctx, const float* data_d, const int64_t* files_d, const int* windows_d, int batch,
                               int time_context, int F, float scale, float* inputs_d, float* targets_d) {
    if (!ctx || !data_d || !files_d || !windows_d || !inputs_d || !targets_d)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather: null argument");
    if (batch < 1 || time_context < 1 || F < 1) DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather: batch %d, time_context %d, F %d",
                                                          batch, time_context, F);
    return gather(ctx, data_d, files_d, windows_d, batch, time_context, F, 4, scale, inputs_d, targets_d);
}

DCS_API int dcs_trainer_gather_sources(dcs_ctx* ctx, const float* data_d, const int64_t* files_d, const int* windows_d,
                                       int batch, int time_context, int F, int nsrc, float scale, float* inputs_d,
                                       float* targets_d) {
    if (!ctx || !data_d || !files_d || !windows_d || !inputs_d || !targets_d)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_sources: null argument");
    if (batch < 1 || time_context < 1 || F < 1 || nsrc < 1 || nsrc > 8)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_sources: batch %d, time_context %d, F %d, nsrc %d (1 .. 8)", batch,
                 time_context, F, nsrc);
    return gather(ctx, data_d, files_d, windows_d, batch, time_context, F, nsrc, scale, inputs_d, targets_d);
}

DCS_API int dcs_trainer_gather_channels(dcs_ctx* ctx, const float* data_d, const int64_t* files_d, const int* windows_d,
                                        int batch, int time_context, int F, int cin, int cout, float scale_in,
                                        float scale_out, float* inputs_d, float* targets_d) {
    if (!ctx || !data_d || !files_d || !windows_d || !inputs_d || !targets_d)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_channels: null argument");
    if (batch < 1 || time_context < 1 || F < 1 || cin < 1 || cin > 4 || cout < 1 || cout > 16)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_channels: batch %d, time_context %d, F %d, cin %d (1 .. 4), cout %d (1 .. 16)",
                 batch, time_context, F, cin, cout);
    DCS_ON_DEVICE(ctx->device);
    const int64_t n = (int64_t)batch * time_context * F;
    hipLaunchKernelGGL(gather_channels_kernel, dim3((unsigned)dcs_cdiv(n, kThreads)), dim3(kThreads), 0, ctx->stream, data_d,
                       files_d, windows_d, batch, time_context, F, cin, cout, scale_in, scale_out, inputs_d, targets_d);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

DCS_API int dcs_trainer_pack_score(const double* notes_h, int ninst, int n_notes, int width, int F, int* packed_h) {
    if (!notes_h || !packed_h) DCS_FAIL(DCS_EINVAL, "dcs_trainer_pack_score: null argument");
    if (ninst < 1 || ninst > 32 || n_notes < 0 || width < 5 || ((width - 3) & 1) || F < 1)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_pack_score: bad shape (ninst %d (1 .. 32), notes %d, width %d, F %d)", ninst, n_notes,
                 width, F);
    const int npairs = (width - 3) / 2, pw = 2 + 2 * npairs;
    const double big = 2147483647.0;
    for (int64_t i = 0; i < (int64_t)ninst * n_notes; ++i) {
        const double* n = notes_h + i * width;
        int* o = packed_h + i * pw;
        memset(o, 0, pw * sizeof(int));
        // filterSpec's test: midi > 0; the frame test is the kernel's (an empty frame range paints nothing)
        if (!(n[2] > 0) || !(n[1] > 0)) continue;
        o[0] = n[0] > 0 ? (int)std::min(n[0], big) : 0;
        o[1] = (int)std::min(n[1], big);
        for (int k = 0; k < npairs; ++k) {
            const double fs = n[3 + 2 * k], fe = n[4 + 2 * k];
            if (!(fe > 0)) continue;
            const int64_t f0 = (int64_t)fs, f1 = (int64_t)fe;
            // the reference's fancy bin index raises past F
            if (f0 < 0 || f1 > F)
                DCS_FAIL(DCS_ESHAPE, "dcs_trainer_pack_score: bin range [%lld, %lld) outside 0..%d", (long long)f0,
                         (long long)f1, F);
            if (f1 > f0) {
                o[2 + 2 * k] = (int)f0;
                o[3 + 2 * k] = (int)f1;
            }
        }
    }
    return DCS_OK;
}

DCS_API int dcs_trainer_gather_score(dcs_ctx* ctx, const float* data_d, const int64_t* files_d, const int* notes_d,
                                     const int64_t* note_files_d, const int* windows_d, int batch, int time_context, int F,
                                     int ninst, int width, float scale, float* inputs_d, float* targets_d) {
    if (!ctx || !data_d || !files_d || !notes_d || !note_files_d || !windows_d || !inputs_d || !targets_d)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_score: null argument");
    if (batch < 1 || batch > 65535 || time_context < 1 || F < 1 || ninst < 1 || ninst > 32 || width < 5 || ((width - 3) & 1))
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_score: batch %d (1 .. 65535), time_context %d, F %d, ninst %d (1 .. 32), "
                 "width %d (odd, from 5)", batch, time_context, F, ninst, width);
    DCS_ON_DEVICE(ctx->device);
    hipLaunchKernelGGL(gather_score_kernel, dim3((unsigned)time_context, (unsigned)batch), dim3(kThreads), 0, ctx->stream,
                       data_d, files_d, notes_d, note_files_d, windows_d, time_context, F, ninst, (width - 3) / 2, scale,
                       inputs_d, targets_d);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

}  // extern "C"

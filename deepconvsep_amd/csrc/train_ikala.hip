// Training of the iKala singing-voice graph (examples/ikala/trainCNN.py: build_ca :66-118, loss :155-189, adadelta :193)
// on gfx950.  conv1 30 x (1 x 30) stride (1, 3) + BiasLayer, conv2 30 x (10 x 20) + BiasLayer, dense 256, two rectified
// dense layers of flat = 30 h2 w2 units, per source the InverseLayers of conv2 and conv1, BiasLayer(2) and rectify.
//
// One step on the ctx stream, no host synchronisation and no float atomics (two runs give bit-identical weights):
//
//   forward   F1 a1b = conv1(x) + b1 + b1b             ik_gemm 128x32  K = 30 taps (saved: a1b)
//             F2 a2b = conv2(a1b) + b2 + b2b           ik_gemm 128x32  implicit GEMM, K = (dh, dw c) = 10 x 600
//             F3 z = rectify(a2b . Wfc + bfc)          ik_gemm 32x32 split-K over flat, ik_finish (saved: z, pre-activation)
//             F4 d_k = rectify(z . W_k + b_k), k < 2   ik_gemm, 2 batches, into the zero-padded V (saved: pre-activations)
//             F5 g_k = conv2^T(d_k)                    ik_gemm 128x32  implicit GEMM over V (9 / 19 zero rows / columns)
//             F6 q = conv1^T(g_k) + bo                 ik_deconv1_kernel: 10 taps x 30 channels per output, fixed order
//   loss      ik_loss_kernel: masks, the four components, dE/dq (rectify' with the 0.5 tie), per-workgroup f64 sums
//             ik_loss_reduce_kernel: fixed-order sum -> loss and components (f64), sign(E), the output-bias gradient
//   backward  B1 dg_k = conv1(dY_k)    B2 dpre_k = conv2(dg_k) * r'(pre_k)    B3 dprez = (sum_k dpre_k . W_k^T) * r'(prez)
//             B4 da2 = dprez . Wfc^T   B5 da1 = conv2^T(da2)
//   weights   dW1|db1 = [x; dY_k] windows^T . [da1; g_k]            split-K (K = 3 B tc w1), fixed-order reduce
//             dW2|db2 = [a1b; dg_k] windows^T . [da2; d_k]          split-K (K = 3 B h2 w2), fixed-order reduce
//             dWfc|dbfc = a2b^T . dprez,  dW_k|db_k = z^T . dpre_k
//             every bias gradient is the "ones" row of its weight GEMM; b1b / b2b get copies of b1 / b2 (identical in Theano)
//   update    ik_adadelta_kernel over the flat [params | grads | accu | delta_accu] buffer, four floats per thread
//
// ik_gemm_kernel is one template: 4 waves of FM x FN v_mfma_f32_16x16x4_f32 tiles each, K staged through LDS 32 at a time
// with the next step's operands prefetched into registers.  Tiles are 128 x 32 (every conv2-family GEMM: N = 30 channels),
// 64 x 64 and 32 x 32.  Each operand loads either K-fastest or M/N-fastest, whichever is contiguous in memory.  Operands
// are addressed through Ax: index i at (i % d0) s0 + (i / d0 % d1) s1 + (i / (d0 d1)) s2 (divisions by multiply-high),
// which covers the implicit-GEMM windows of conv1 and conv2 and the K-concatenations above without copies.
//
// Internal parameter layouts (the flat buffer; dcs_trainer_get / _create convert to and from the .pkl layout):
//   W1 [30 j][30 c]: W1i[j][c] = W1[c,0,0,29-j]           W2 [10 dh][20 dw][30 c][30 o]: W2i = W2[o,c,9-dh,19-dw] (flips)
//   Wfc [(h,w,o)][256] and W_k [256][(h,w,o)], b_k [(h,w,o)]: the 30 x h2 x w2 map channels-last, .pkl order o h2 w2 + h w2 + w
// Activations are channels-last: a1b / dg / g / da1 [B][tc][w1][30], a2b / d_k / dpre [B][h2][w2][30]; d_k and da2 live in
// V [B][h2 + 18][w2 + 38][30], zero rows and columns around them, so that conv2^T is a plain implicit GEMM.
#include <math.h>
#include <algorithm>
#include <string.h>

#include "dcs_internal.h"
#include "train_ikala.h"

namespace {

constexpr int kThreads = 256;
constexpr int kKT = 32;
constexpr int kC1 = 30, kK1 = 30, kS1 = 3;       // conv1: 30 filters of 1 x 30, stride (1, 3)
constexpr int kC2 = 30, kH2 = 10, kW2 = 20;      // conv2: 30 filters of 10 x 20
constexpr int kRow = kW2 * kC1;                  // 600: one row of a conv2 window (20 taps x 30 channels), contiguous
constexpr int kK2 = kH2 * kRow;                  // 6000
constexpr int kHidden = 256, kNparams = 13;
constexpr int kBig = 1 << 30;
constexpr int kLossBlocks = 1024;
constexpr int kLossSums = 6;                     // four components, two output-bias gradient sums

// n / d for 0 <= n < 2^31 as (umulhi(n, m) + n) >> s (round-up magic numbers)
struct FDiv {
    uint32_t m, s;
};

FDiv fdiv(int64_t d) {
    uint32_t s = 0;
    while ((int64_t(1) << s) < d) ++s;
    const uint64_t one = 1;
    return FDiv{(uint32_t)(((one << 32) * ((one << s) - (uint64_t)d)) / (uint64_t)d + 1), s};
}

__device__ __forceinline__ int fdq(int n, const FDiv f) {
    return (int)((__umulhi((uint32_t)n, f.m) + (uint32_t)n) >> f.s);
}

// one operand axis: index i -> (i % d0) s0 + (i / d0 % d1) s1 + (i / (d0 d1)) s2; every index is below kBig
struct Ax {
    FDiv q0, q01;
    int d0, d1;
    int64_t s0, s1, s2;
};

Ax ax3(int64_t d0, int64_t d1, int64_t s0, int64_t s1, int64_t s2) {
    const int64_t d01 = std::min<int64_t>(d0 * d1, kBig);
    return Ax{fdiv(d0), fdiv(d01), (int)d0, (int)d1, s0, s1, s2};
}
Ax ax2(int64_t d0, int64_t s0, int64_t s1) { return ax3(d0, kBig, s0, s1, 0); }
Ax ax1(int64_t s0) { return ax3(kBig, 1, s0, 0, 0); }

__device__ __forceinline__ int64_t ax_off(const Ax& a, int i) {
    const int q0 = fdq(i, a.q0), q2 = fdq(i, a.q01);
    return (int64_t)(i - q0 * a.d0) * a.s0 + (int64_t)(q0 - q2 * a.d1) * a.s1 + (int64_t)q2 * a.s2;
}

struct Mat {
    float* p;
    int64_t off;
    Ax r, c;
};

Mat mat(float* p, int64_t off, Ax r, Ax c) { return Mat{p, off, r, c}; }

enum { EPI_RELU = 1, EPI_SAVEPRE = 2, EPI_DRELU = 4 };

struct IGemm {
    Mat A, B, C, X;               // C = A . B; X: pre-activations (EPI_SAVEPRE writes, EPI_DRELU reads), C's shape
    int M, N, K;
    int ones_row, ones_klim;      // rows >= ones_row of A read 1 for k < ones_klim, else 0 (bias gradients)
    int nbatch;
    int64_t boff[2][5];           // per batch: offsets of A, B, C, X, bias
    const float* bias;            // nullable: bias[boff[.][4] + n]
    const float* bias2;           // nullable, added too (the BiasLayer that follows a layer)
    const float* scale;           // nullable device scalar: sign(E)
    int epi;
    float* partial;               // non-null: raw sums to partial[(batch * splits + s)][M][N], no epilogue (even at one slice)
    int splits, kchunk;
};

__device__ __forceinline__ float relu_d(float pre) { return pre > 0.f ? 1.f : (pre == 0.f ? 0.5f : 0.f); }

typedef float f32x4 __attribute__((ext_vector_type(4)));

// AK: A is loaded K-fastest (lane = k), else M-fastest (lane = m); BK likewise for B (K-fastest, else N-fastest).
template <int WM, int WN, int FM, int FN, bool AK, bool BK>
__global__ __launch_bounds__(kThreads) void ik_gemm_kernel(const IGemm g) {
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
                if (g.bias) v += g.bias[g.boff[batch][4] + n];
                if (g.bias2) v += g.bias2[g.boff[batch][4] + n];
                if (g.epi & (EPI_SAVEPRE | EPI_DRELU)) {
                    float* x = g.X.p + g.X.off + g.boff[batch][3] + ax_off(g.X.r, m) + ax_off(g.X.c, n);
                    if (g.epi & EPI_SAVEPRE) *x = v;
                    else v *= relu_d(*x);
                }
                if (g.epi & EPI_RELU) v = v > 0.f ? v : 0.f;
                g.C.p[g.C.off + g.boff[batch][2] + ax_off(g.C.r, m) + ax_off(g.C.c, n)] = v;
            }
}

// The skinny split-K GEMMs' slices summed in slice order, then the epilogue: C[m][n] (row-major, ld N) = sum + bias[n],
// EPI_SAVEPRE -> X, EPI_DRELU * r'(X), EPI_RELU.
__global__ __launch_bounds__(kThreads) void ik_finish_kernel(const float* __restrict__ part, int splits, int64_t count, int N,
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

// Split-K partials summed in slice order, times sign(E), into the gradient buffer; the last row (the bias gradient) is
// written once more right after it (BiasLayer.b gets the layer bias's gradient).
struct IReduce {
    const float* part[2];
    float* dst[2];
    int64_t count[2];
    int splits[2];
    const float* scale;
};

__global__ __launch_bounds__(kThreads) void ik_reduce_kernel(const IReduce r) {
    const int j = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= r.count[j]) return;
    float s = 0.f;
    for (int z = 0; z < r.splits[j]; ++z) s += r.part[j][z * r.count[j] + i];
    s *= *r.scale;
    r.dst[j][i] = s;
    if (i >= r.count[j] - kC1) r.dst[j][i + kC1] = s;
}

// conv1^T (the InverseLayer of conv1) plus the output BiasLayer: q[b][k][t][f] = bo[k] + sum over the taps 3 w + j = f of
// sum_c g_k[b][t][w][c] W1i[j][c], w and c ascending.  Columns f > 3 (w1 - 1) + 29 get no tap and hold bo alone.
__global__ __launch_bounds__(kThreads) void ik_deconv1_kernel(const float* __restrict__ g, int64_t gslot,
                                                              const float* __restrict__ W1i, const float* __restrict__ bo,
                                                              float* __restrict__ q, int B, int tc, int F, int w1) {
    __shared__ float w[kK1 * kC1];
    for (int i = threadIdx.x; i < kK1 * kC1; i += kThreads) w[i] = W1i[i];
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (int64_t)B * 2 * tc * F) return;
    const int f = (int)(e % F);
    int64_t r = e / F;
    const int t = (int)(r % tc);
    r /= tc;
    const int k = (int)(r % 2), b = (int)(r / 2);
    const float* gr = g + k * gslot + ((int64_t)b * tc + t) * w1 * kC1;
    const int wlo = f >= kK1 - 1 ? (f - (kK1 - 1) + kS1 - 1) / kS1 : 0;
    const int whi = min(w1 - 1, f / kS1);
    float acc = 0.f;
    for (int x = wlo; x <= whi; ++x) {
        const float* gw = gr + (int64_t)x * kC1;
        const float* ww = w + (f - kS1 * x) * kC1;
#pragma unroll
        for (int c = 0; c < kC1; ++c) acc += gw[c] * ww[c];
    }
    q[e] = acc + bo[k];
}

struct ILoss {
    const float* q;       // [B][2][tc F] pre-activations of the output layer
    const float* x;       // [B][tc F] inputs
    const float* tgt;     // [B][2][tc F] targets
    const float* rnd;     // [B][tc F] the uniform draw
    float* xy;            // [3][B tc F]: slot 0 <- x, slots 1, 2 <- dE/dq_k
    double* part;         // [gridDim.x][kLossSums]
    int64_t plane, n;     // tc F, B tc F
    double eps, alpha, beta_acc, beta_voc;
};

// trainCNN.py:170-187 per element, in f64: s_k = p_k + eps r, m_k = s_k / (s_0 + s_1), vocals = m_0 x, acc = m_1 x; the four
// squared-error sums; dE/dp_k = x / D (G_k - m_0 G_0 - m_1 G_1) with G the derivative of E = vocals_error + acc_error -
// negative_error_voc in (vocals, acc) (negative_error_acc is reported only); dE/dq = dE/dp r'(q), r'(0) = 0.5.
__global__ __launch_bounds__(kThreads) void ik_loss_kernel(const ILoss a) {
    __shared__ double red[kLossSums][kThreads];
    double acc[kLossSums];
#pragma unroll
    for (int i = 0; i < kLossSums; ++i) acc[i] = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < a.n; e += (int64_t)gridDim.x * kThreads) {
        const int64_t b = e / a.plane, rem = e - b * a.plane;
        const int64_t o = b * 2 * a.plane + rem;
        const double x = a.x[e], er = a.eps * (double)a.rnd[e];
        double q[2], s[2], t[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            q[j] = a.q[o + j * a.plane];
            t[j] = a.tgt[o + j * a.plane];
            s[j] = (q[j] > 0.0 ? q[j] : 0.0) + er;
        }
        const double D = s[0] + s[1];
        const double v = s[0] / D * x, ac = s[1] / D * x;
        const double ev0 = v - t[0], ev1 = v - t[1], ea0 = ac - t[0], ea1 = ac - t[1];
        acc[0] += ev0 * ev0;                        // vocals_error
        acc[1] += a.alpha * (ea1 * ea1);            // acc_error
        acc[2] += a.beta_voc * (ev1 * ev1);         // negative_error_voc
        acc[3] += a.beta_acc * (ea0 * ea0);         // negative_error_acc
        const double G0 = 2.0 * (ev0 - a.beta_voc * ev1), G1 = 2.0 * a.alpha * ea1;
        const double mg = (s[0] * G0 + s[1] * G1) / D;
        double dq[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const double rd = q[j] > 0.0 ? 1.0 : (q[j] == 0.0 ? 0.5 : 0.0);
            dq[j] = x / D * ((j == 0 ? G0 : G1) - mg) * rd;
            acc[4 + j] += dq[j];
        }
        a.xy[e] = (float)x;
        a.xy[a.n + e] = (float)dq[0];
        a.xy[2 * a.n + e] = (float)dq[1];
    }
#pragma unroll
    for (int i = 0; i < kLossSums; ++i) red[i][threadIdx.x] = acc[i];
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w)
#pragma unroll
            for (int i = 0; i < kLossSums; ++i) red[i][threadIdx.x] += red[i][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < kLossSums) a.part[(int64_t)blockIdx.x * kLossSums + threadIdx.x] = red[threadIdx.x][0];
}

// out7 = (|E|, vocals_error, acc_error, negative_error_voc, negative_error_acc, 0, 0) with E = vocals_error + acc_error -
// negative_error_voc (trainCNN.py:189); sign(E) (abs'(0) = 0) for the gradient epilogues; the output-bias gradient.
__global__ __launch_bounds__(kThreads) void ik_loss_reduce_kernel(const double* __restrict__ part, int nblk, double* out7,
                                                                  float* sign, float* dbo) {
    __shared__ double red[kLossSums][kThreads];
    for (int i = 0; i < kLossSums; ++i) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblk; b += kThreads) s += part[(int64_t)b * kLossSums + i];
        red[i][threadIdx.x] = s;
    }
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w)
            for (int i = 0; i < kLossSums; ++i) red[i][threadIdx.x] += red[i][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double E = red[0][0] + red[1][0] - red[2][0];
        const float sg = E > 0.0 ? 1.f : (E < 0.0 ? -1.f : 0.f);
        out7[0] = fabs(E);
        for (int i = 0; i < 4; ++i) out7[1 + i] = red[i][0];
        out7[5] = out7[6] = 0.0;
        *sign = sg;
        for (int j = 0; j < 2; ++j) dbo[j] = sg * (float)red[4 + j][0];
    }
}

// lasagne.updates.adadelta (lasagne/updates.py adadelta): accu' = rho accu + (1 - rho) g^2,
// u = g sqrt(delta + eps) / sqrt(accu' + eps), p -= lr u, delta' = rho delta + (1 - rho) u^2.  P4: the section length in
// float4s (sections are padded to a multiple of four floats; the pad stays zero).
__global__ __launch_bounds__(kThreads) void ik_adadelta_kernel(float4* __restrict__ state, int64_t P4, float lr, float rho,
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

__global__ __launch_bounds__(kThreads) void ik_relu_kernel(const float* __restrict__ q, float* __restrict__ p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) p[i] = q[i] > 0.f ? q[i] : 0.f;
}

// .pkl layout <-> internal layout, one element of the flat parameter section per thread.  to_internal: flat[i] = pkl[src];
// else pkl[src] = flat[i].
struct ILayout {
    float* pkl[kNparams];
    int64_t off[kNparams + 1];
    int h2, w2;
    int to_internal;
};

__global__ __launch_bounds__(kThreads) void ik_layout_kernel(float* __restrict__ flat, const ILayout L) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= L.off[kNparams]) return;
    int s = 0;
    while (i >= L.off[s + 1]) ++s;
    const int64_t k = i - L.off[s];
    const int64_t hw = (int64_t)L.h2 * L.w2, map = kC2 * hw;
    // map position (h, w, o) channels-last -> .pkl o h2 w2 + h w2 + w
    auto pkl_of = [&](int64_t col) {
        const int64_t o = col % kC2, hwi = col / kC2;
        return o * hw + hwi;
    };
    int64_t src = k;
    if (s == 0) {                                     // W1i[j][c] = W1[c][29-j]
        const int64_t j = k / kC1, c = k % kC1;
        src = c * kK1 + (kK1 - 1 - j);
    } else if (s == 3) {                              // W2i[dh][dw][c][o] = W2[o][c][9-dh][19-dw]
        const int64_t dh = k / (kW2 * kC1 * kC2), dw = (k / (kC1 * kC2)) % kW2, c = (k / kC2) % kC1, o = k % kC2;
        src = ((o * kC1 + c) * kH2 + (kH2 - 1 - dh)) * kW2 + (kW2 - 1 - dw);
    } else if (s == 6) {                              // Wfc rows (h, w, o)
        src = pkl_of(k / kHidden) * kHidden + k % kHidden;
    } else if (s == 8 || s == 10) {                   // W_k columns (h, w, o)
        src = (k / map) * map + pkl_of(k % map);
    } else if (s == 9 || s == 11) {
        src = pkl_of(k);
    }
    if (L.to_internal) flat[i] = L.pkl[s][src];
    else L.pkl[s][src] = flat[i];
}

// (file, start) windows of resident [1 + nsrc][T][F] feature files -> inputs and targets (dataset.py loadFile / initOutput),
// as tr_gather_kernel of train_dsd.hip with nsrc sources in place of four.
__global__ __launch_bounds__(kThreads) void ik_gather_kernel(const float* __restrict__ data, const int64_t* __restrict__ files,
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

}  // namespace

struct ik_trainer {
    dcs_ctx* ctx = nullptr;
    int tc = 0, F = 0, B = 0, w1 = 0, h2 = 0, w2 = 0, hp = 0, wp = 0;
    int64_t R1 = 0, Rh = 0, RF = 0, flat = 0, P = 0, P4 = 0;
    double hyp[7] = {0};
    int64_t off[kNparams + 1] = {0};
    float* state = nullptr;      // [4][4 P4]: params, grads, accu, delta_accu
    float* work = nullptr;
    double* lpart = nullptr;
    double* out7 = nullptr;      // when the caller passes none
    // views into work
    float *rnd, *xy, *U, *GA, *V, *Q, *a2b, *z, *prez, *dprez, *pre, *dpre, *part1, *part2, *partS, *sign;
    int splits1 = 1, splits2 = 1, splits3 = 1, splitsB3 = 1, kchunk1 = 0, kchunk2 = 0, kchunk3 = 0, kchunkB3 = 0;
};

namespace {

void ik_shapes(int tc, int F, int64_t s[kNparams][4]) {
    const int64_t w1 = (F - kK1) / kS1 + 1, h2 = tc - kH2 + 1, w2 = w1 - kW2 + 1, flat = kC2 * h2 * w2;
    const int64_t t[kNparams][4] = {{kC1, 1, 1, kK1}, {kC1, 1, 1, 1}, {kC1, 1, 1, 1}, {kC2, kC1, kH2, kW2}, {kC2, 1, 1, 1},
                                    {kC2, 1, 1, 1}, {flat, kHidden, 1, 1}, {kHidden, 1, 1, 1}, {kHidden, flat, 1, 1},
                                    {flat, 1, 1, 1}, {kHidden, flat, 1, 1}, {flat, 1, 1, 1}, {2, 1, 1, 1}};
    memcpy(s, t, sizeof(t));
}

IGemm gemm0(int M, int N, int K) {
    IGemm g;
    memset(&g, 0, sizeof(g));
    g.M = M; g.N = N; g.K = K;
    g.ones_row = kBig;
    g.nbatch = 1;
    g.splits = 1;
    g.kchunk = K;
    return g;
}

enum Tile { T128x32, T64x64, T32x32 };

template <int WM, int WN, int FM, int FN>
void launch_tile(const IGemm& g, bool ak, bool bk, dim3 grid, hipStream_t s) {
    if (ak && bk) hipLaunchKernelGGL((ik_gemm_kernel<WM, WN, FM, FN, true, true>), grid, dim3(kThreads), 0, s, g);
    else if (ak) hipLaunchKernelGGL((ik_gemm_kernel<WM, WN, FM, FN, true, false>), grid, dim3(kThreads), 0, s, g);
    else if (bk) hipLaunchKernelGGL((ik_gemm_kernel<WM, WN, FM, FN, false, true>), grid, dim3(kThreads), 0, s, g);
    else hipLaunchKernelGGL((ik_gemm_kernel<WM, WN, FM, FN, false, false>), grid, dim3(kThreads), 0, s, g);
}

int launch(ik_trainer* t, IGemm g, Tile tile, bool ak, bool bk) {
    if (g.splits < 1) g.splits = 1;
    if (g.splits == 1) g.kchunk = g.K;
    const int bm = tile == T128x32 ? 128 : (tile == T64x64 ? 64 : 32), bn = tile == T64x64 ? 64 : 32;
    dim3 grid((unsigned)dcs_cdiv(g.M, bm), (unsigned)dcs_cdiv(g.N, bn), (unsigned)(g.nbatch * g.splits));
    hipStream_t s = t->ctx->stream;
    if (tile == T128x32) launch_tile<4, 1, 2, 2>(g, ak, bk, grid, s);
    else if (tile == T64x64) launch_tile<2, 2, 2, 2>(g, ak, bk, grid, s);
    else launch_tile<2, 2, 1, 1>(g, ak, bk, grid, s);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

// K split into slices of a multiple of kKT for a grid of about `target` workgroups (default 2 per CU)
void pick_split(int64_t tiles, int64_t K, int* splits, int* kchunk, int64_t target = 512) {
    int64_t s = target / (tiles > 0 ? tiles : 1);
    s = s < 1 ? 1 : (s > 128 ? 128 : s);
    int64_t kc = dcs_round_up((K + s - 1) / s, kKT);
    if (kc < 256) kc = dcs_round_up(256 < K ? 256 : K, kKT);
    *kchunk = (int)kc;
    *splits = (int)((K + kc - 1) / kc);
}

float* P_(ik_trainer* t, int i) { return t->state + t->off[i]; }

// the dense GEMMs with M = B rows: 64 x 64 tiles from 64 rows up
Tile rows_tile(int M) { return M >= 64 ? T64x64 : T32x32; }

int finish(ik_trainer* t, const float* part, int splits, int N, const float* bias, float* C, float* X, int epi) {
    const int64_t count = (int64_t)t->B * N;
    hipLaunchKernelGGL(ik_finish_kernel, dim3((unsigned)dcs_cdiv(count, kThreads)), dim3(kThreads), 0, t->ctx->stream, part,
                       splits, count, N, bias, C, X, epi);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

int forward(ik_trainer* t, const float* x) {
    const int B = t->B, tc = t->tc, F = t->F, w1 = t->w1, h2 = t->h2, w2 = t->w2, hp = t->hp, wp = t->wp;
    const int64_t R1 = t->R1, Rh = t->Rh, flat = t->flat, RF = t->RF;
    const int64_t row1 = (int64_t)w1 * kC1, img1 = (int64_t)tc * row1, rowp = (int64_t)wp * kC2, imgp = (int64_t)hp * rowp;
    const int64_t padoff = (int64_t)(kH2 - 1) * rowp + (kW2 - 1) * kC2, Vslot = (int64_t)B * imgp, Uslot = R1 * kC1;
    const int64_t wstep = t->off[10] - t->off[8];
    (void)RF;
    // F1: a1b[(b,t,w)][c] = sum_j x[b][t][3 w + j] W1i[j][c] + b1 + b1b -> U slot 0
    {
        IGemm g = gemm0((int)R1, kC1, kK1);
        g.A = mat((float*)x, 0, ax2(w1, kS1, F), ax1(1));
        g.B = mat(P_(t, 0), 0, ax1(kC1), ax1(1));
        g.C = mat(t->U, 0, ax1(kC1), ax1(1));
        g.bias = P_(t, 1); g.bias2 = P_(t, 2);
        DCS_CHECK(launch(t, g, T128x32, true, false));
    }
    // F2: a2b[(b,h,w)][o] = sum_{dh,(dw,c)} a1b[b][h+dh][w+dw][c] W2i[dh][dw][c][o] + b2 + b2b
    {
        IGemm g = gemm0((int)Rh, kC2, kK2);
        g.A = mat(t->U, 0, ax3(w2, h2, kC1, row1, img1), ax2(kRow, 1, row1));
        g.B = mat(P_(t, 3), 0, ax1(kC2), ax1(1));
        g.C = mat(t->a2b, 0, ax1(kC2), ax1(1));
        g.bias = P_(t, 4); g.bias2 = P_(t, 5);
        DCS_CHECK(launch(t, g, T128x32, true, false));
    }
    // F3: z = rectify(a2b . Wfci + bfc), pre-activation saved: split-K over flat, then the fixed-order sum
    {
        IGemm g = gemm0(B, kHidden, (int)flat);
        g.A = mat(t->a2b, 0, ax1(flat), ax1(1));
        g.B = mat(P_(t, 6), 0, ax1(kHidden), ax1(1));
        g.partial = t->partS; g.splits = t->splits3; g.kchunk = t->kchunk3;
        DCS_CHECK(launch(t, g, T32x32, true, false));
        DCS_CHECK(finish(t, t->partS, t->splits3, kHidden, P_(t, 7), t->z, t->prez, EPI_RELU | EPI_SAVEPRE));
    }
    // F4: d_k = rectify(z . W_ki + b_ki) -> V slots 1, 2 (zero-padded map), pre-activations saved
    {
        IGemm g = gemm0(B, (int)flat, kHidden);
        g.A = mat(t->z, 0, ax1(kHidden), ax1(1));
        g.B = mat(P_(t, 8), 0, ax1(flat), ax1(1));
        g.C = mat(t->V, padoff, ax1(imgp), ax2((int64_t)w2 * kC2, 1, rowp));
        g.X = mat(t->pre, 0, ax1(flat), ax1(1));
        g.bias = P_(t, 9);
        g.epi = EPI_RELU | EPI_SAVEPRE;
        g.nbatch = 2;
        for (int k = 0; k < 2; ++k) {
            g.boff[k][1] = k * wstep;
            g.boff[k][2] = (k + 1) * Vslot;
            g.boff[k][3] = k * (int64_t)B * flat;
            g.boff[k][4] = k * wstep;
        }
        DCS_CHECK(launch(t, g, rows_tile(B), true, false));
    }
    // F5: g_k[(b,t,w)][c] = sum_{dh,(dw,o)} V[b][t+dh][w+dw][o] W2i[9-dh][19-dw][c][o] -> GA slots 1, 2
    {
        IGemm g = gemm0((int)R1, kC1, kK2);
        g.A = mat(t->V, 0, ax3(w1, tc, kC2, rowp, imgp), ax2(kRow, 1, rowp));
        g.B = mat(P_(t, 3), (int64_t)(kH2 * kW2 - 1) * kC1 * kC2, ax2(kC2, 1, -(int64_t)kC1 * kC2), ax1(kC2));
        g.C = mat(t->GA, 0, ax1(kC1), ax1(1));
        g.nbatch = 2;
        for (int k = 0; k < 2; ++k) {
            g.boff[k][0] = (k + 1) * Vslot;
            g.boff[k][2] = (k + 1) * Uslot;
        }
        DCS_CHECK(launch(t, g, T128x32, true, true));
    }
    // F6: q = conv1^T(g_k) + bo
    {
        const int64_t n = 2 * (int64_t)B * tc * F;
        hipLaunchKernelGGL(ik_deconv1_kernel, dim3((unsigned)dcs_cdiv(n, kThreads)), dim3(kThreads), 0, t->ctx->stream,
                           (const float*)(t->GA + Uslot), Uslot, (const float*)P_(t, 0), (const float*)P_(t, 12), t->Q, B, tc,
                           F, w1);
        DCS_HIP(hipGetLastError());
    }
    return DCS_OK;
}

int loss(ik_trainer* t, const float* x, const float* tgt, double* out7) {
    ILoss a;
    a.q = t->Q; a.x = x; a.tgt = tgt; a.rnd = t->rnd; a.xy = t->xy; a.part = t->lpart;
    a.plane = (int64_t)t->tc * t->F;
    a.n = t->RF;
    a.eps = t->hyp[0]; a.alpha = t->hyp[1]; a.beta_acc = t->hyp[2]; a.beta_voc = t->hyp[3];
    const int nblk = (int)std::min<int64_t>(kLossBlocks, dcs_cdiv(a.n, kThreads));
    hipLaunchKernelGGL(ik_loss_kernel, dim3(nblk), dim3(kThreads), 0, t->ctx->stream, a);
    DCS_HIP(hipGetLastError());
    hipLaunchKernelGGL(ik_loss_reduce_kernel, dim3(1), dim3(kThreads), 0, t->ctx->stream, (const double*)t->lpart, nblk,
                       out7 ? out7 : t->out7, t->sign, t->state + 4 * t->P4 + t->off[12]);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

int backward(ik_trainer* t) {
    const int B = t->B, tc = t->tc, F = t->F, w1 = t->w1, h2 = t->h2, w2 = t->w2, hp = t->hp, wp = t->wp;
    const int64_t R1 = t->R1, Rh = t->Rh, flat = t->flat, RF = t->RF, Bflat = (int64_t)B * flat;
    const int64_t row1 = (int64_t)w1 * kC1, img1 = (int64_t)tc * row1, rowp = (int64_t)wp * kC2, imgp = (int64_t)hp * rowp;
    const int64_t padoff = (int64_t)(kH2 - 1) * rowp + (kW2 - 1) * kC2, Vslot = (int64_t)B * imgp, Uslot = R1 * kC1;
    const int64_t wstep = t->off[10] - t->off[8];
    float* grad = t->state + 4 * t->P4;
    // B1: dg_k[(b,t,w)][c] = sum_j dY_k[b][t][3 w + j] W1i[j][c] -> U slots 1, 2
    {
        IGemm g = gemm0((int)R1, kC1, kK1);
        g.A = mat(t->xy, 0, ax2(w1, kS1, F), ax1(1));
        g.B = mat(P_(t, 0), 0, ax1(kC1), ax1(1));
        g.C = mat(t->U, 0, ax1(kC1), ax1(1));
        g.nbatch = 2;
        for (int k = 0; k < 2; ++k) {
            g.boff[k][0] = (k + 1) * RF;
            g.boff[k][2] = (k + 1) * Uslot;
        }
        DCS_CHECK(launch(t, g, T128x32, true, false));
    }
    // B2: dpre_k = conv2(dg_k) * r'(pre_k)  (the F2 form)
    {
        IGemm g = gemm0((int)Rh, kC2, kK2);
        g.A = mat(t->U, 0, ax3(w2, h2, kC1, row1, img1), ax2(kRow, 1, row1));
        g.B = mat(P_(t, 3), 0, ax1(kC2), ax1(1));
        g.C = mat(t->dpre, 0, ax1(kC2), ax1(1));
        g.X = mat(t->pre, 0, ax1(kC2), ax1(1));
        g.epi = EPI_DRELU;
        g.nbatch = 2;
        for (int k = 0; k < 2; ++k) {
            g.boff[k][0] = (k + 1) * Uslot;
            g.boff[k][2] = k * Bflat;
            g.boff[k][3] = k * Bflat;
        }
        DCS_CHECK(launch(t, g, T128x32, true, false));
    }
    // B3: dprez = (sum_k dpre_k . W_ki^T) * r'(prez): K = 2 flat, concatenated over k, split-K
    {
        IGemm g = gemm0(B, kHidden, (int)(2 * flat));
        g.A = mat(t->dpre, 0, ax1(flat), ax2(flat, 1, Bflat));
        g.B = mat(P_(t, 8), 0, ax2(flat, 1, wstep), ax1(flat));
        g.partial = t->partS; g.splits = t->splitsB3; g.kchunk = t->kchunkB3;
        DCS_CHECK(launch(t, g, T32x32, true, true));
        DCS_CHECK(finish(t, t->partS, t->splitsB3, kHidden, nullptr, t->dprez, t->prez, EPI_DRELU));
    }
    // B4: da2 = dprez . Wfci^T -> V slot 0 (zero-padded map)
    {
        IGemm g = gemm0(B, (int)flat, kHidden);
        g.A = mat(t->dprez, 0, ax1(kHidden), ax1(1));
        g.B = mat(P_(t, 6), 0, ax1(1), ax1(kHidden));
        g.C = mat(t->V, padoff, ax1(imgp), ax2((int64_t)w2 * kC2, 1, rowp));
        DCS_CHECK(launch(t, g, rows_tile(B), true, true));
    }
    // B5: da1 = conv2^T(da2) -> GA slot 0  (the F5 form)
    {
        IGemm g = gemm0((int)R1, kC1, kK2);
        g.A = mat(t->V, 0, ax3(w1, tc, kC2, rowp, imgp), ax2(kRow, 1, rowp));
        g.B = mat(P_(t, 3), (int64_t)(kH2 * kW2 - 1) * kC1 * kC2, ax2(kC2, 1, -(int64_t)kC1 * kC2), ax1(kC2));
        g.C = mat(t->GA, 0, ax1(kC1), ax1(1));
        DCS_CHECK(launch(t, g, T128x32, true, true));
    }
    // dW1 | db1: dW1i[j][c] = sum over the 3 R1 windows of [x; dY_k][s][b][t][3 w + j] [da1; g_k][s][b][t][w][c], ones row
    // over the da1 block
    {
        IGemm g = gemm0(kK1 + 1, kC1, (int)(3 * R1));
        g.A = mat(t->xy, 0, ax1(1), ax2(w1, kS1, F));
        g.B = mat(t->GA, 0, ax1(kC1), ax1(1));
        g.ones_row = kK1; g.ones_klim = (int)R1;
        g.partial = t->part1; g.splits = t->splits1; g.kchunk = t->kchunk1;
        DCS_CHECK(launch(t, g, T32x32, false, false));
    }
    // dW2 | db2: dW2i[(dh,dw,c)][o] = sum_{(s,b,h,w)} U[s][b][h+dh][w+dw][c] V[s][b][h+9][w+19][o], ones row over da2
    {
        IGemm g = gemm0(kK2 + 1, kC2, (int)(3 * Rh));
        g.A = mat(t->U, 0, ax2(kRow, 1, row1), ax3(w2, h2, kC1, row1, img1));
        g.B = mat(t->V, padoff, ax3(w2, h2, kC2, rowp, imgp), ax1(1));
        g.ones_row = kK2; g.ones_klim = (int)Rh;
        g.partial = t->part2; g.splits = t->splits2; g.kchunk = t->kchunk2;
        DCS_CHECK(launch(t, g, T128x32, false, false));
    }
    // dWfc | dbfc = [a2b^T; 1] . dprez -> grads (Wfc and bfc are adjacent)
    {
        IGemm g = gemm0((int)flat + 1, kHidden, B);
        g.A = mat(t->a2b, 0, ax1(1), ax1(flat));
        g.B = mat(t->dprez, 0, ax1(kHidden), ax1(1));
        g.C = mat(grad + t->off[6], 0, ax1(kHidden), ax1(1));
        g.ones_row = (int)flat; g.ones_klim = B;
        g.scale = t->sign;
        DCS_CHECK(launch(t, g, T64x64, false, false));
    }
    // dW_k | db_k = [z^T; 1] . dpre_k -> grads (W_k and b_k are adjacent)
    {
        IGemm g = gemm0(kHidden + 1, (int)flat, B);
        g.A = mat(t->z, 0, ax1(1), ax1(kHidden));
        g.B = mat(t->dpre, 0, ax1(flat), ax1(1));
        g.C = mat(grad + t->off[8], 0, ax1(flat), ax1(1));
        g.ones_row = kHidden; g.ones_klim = B;
        g.scale = t->sign;
        g.nbatch = 2;
        for (int k = 0; k < 2; ++k) {
            g.boff[k][1] = k * Bflat;
            g.boff[k][2] = k * wstep;
        }
        DCS_CHECK(launch(t, g, T64x64, false, false));
    }
    {
        IReduce r;
        memset(&r, 0, sizeof(r));
        r.scale = t->sign;
        r.part[0] = t->part1; r.dst[0] = grad + t->off[0]; r.count[0] = (int64_t)(kK1 + 1) * kC1; r.splits[0] = t->splits1;
        r.part[1] = t->part2; r.dst[1] = grad + t->off[3]; r.count[1] = (int64_t)(kK2 + 1) * kC2; r.splits[1] = t->splits2;
        const int64_t most = std::max(r.count[0], r.count[1]);
        hipLaunchKernelGGL(ik_reduce_kernel, dim3((unsigned)dcs_cdiv(most, kThreads), 2), dim3(kThreads), 0, t->ctx->stream, r);
        DCS_HIP(hipGetLastError());
    }
    return DCS_OK;
}

int layout(ik_trainer* t, float* flat, float* const* pkl, int to_internal) {
    ILayout L;
    for (int i = 0; i < kNparams; ++i) {
        L.pkl[i] = pkl[i];
        L.off[i] = t->off[i];
    }
    L.off[kNparams] = t->off[kNparams];
    L.h2 = t->h2; L.w2 = t->w2;
    L.to_internal = to_internal;
    hipLaunchKernelGGL(ik_layout_kernel, dim3((unsigned)dcs_cdiv(t->P, kThreads)), dim3(kThreads), 0, t->ctx->stream, flat, L);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

void trainer_free(ik_trainer* t) {
    if (!t) return;
    dcs_dev_free(t->state);
    dcs_dev_free(t->work);
    delete t;
}

}  // namespace

int ik_trainer_create(dcs_ctx* ctx, int time_context, int F, int batch, const float* const* params_d, const int64_t* shapes,
                      int nparams, const float* rand_d, const double* hyper_h, ik_trainer** out) {
    *out = nullptr;
    if (time_context < kH2 || time_context > 64 || F < 87 || F > 2049 || batch < 1 || batch > 1024)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: iKala graph: time_context %d (10 .. 64), F %d (87 .. 2049), batch %d (1 .. 1024)",
                 time_context, F, batch);
    if (!params_d || !shapes || nparams != kNparams)
        DCS_FAIL(DCS_ESHAPE, "mismatch: got %d values to set %d parameters", nparams, kNparams);
    int64_t want[kNparams][4];
    ik_shapes(time_context, F, want);
    for (int i = 0; i < kNparams; ++i) {
        if (!params_d[i]) DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: parameter %d is null", i);
        for (int k = 0; k < 4; ++k)
            if (shapes[4 * i + k] != want[i][k])
                DCS_FAIL(DCS_ESHAPE, "mismatch: parameter %d has shape (%lld, %lld, %lld, %lld) but value to set has shape "
                         "(%lld, %lld, %lld, %lld)", i, (long long)want[i][0], (long long)want[i][1], (long long)want[i][2],
                         (long long)want[i][3], (long long)shapes[4 * i], (long long)shapes[4 * i + 1],
                         (long long)shapes[4 * i + 2], (long long)shapes[4 * i + 3]);
    }
    DCS_ON_DEVICE(ctx->device);
    ik_trainer* t = new ik_trainer();
    t->ctx = ctx;
    t->tc = time_context; t->F = F; t->B = batch;
    t->w1 = (F - kK1) / kS1 + 1;
    t->h2 = time_context - kH2 + 1;
    t->w2 = t->w1 - kW2 + 1;
    t->hp = t->h2 + 2 * (kH2 - 1);
    t->wp = t->w2 + 2 * (kW2 - 1);
    t->R1 = (int64_t)batch * time_context * t->w1;
    t->Rh = (int64_t)batch * t->h2 * t->w2;
    t->RF = (int64_t)batch * time_context * F;
    t->flat = (int64_t)kC2 * t->h2 * t->w2;
    memcpy(t->hyp, hyper_h, sizeof(t->hyp));
    t->off[0] = 0;
    for (int i = 0; i < kNparams; ++i) t->off[i + 1] = t->off[i] + want[i][0] * want[i][1] * want[i][2] * want[i][3];
    t->P = t->off[kNparams];
    t->P4 = dcs_cdiv(t->P, 4);
    pick_split(dcs_cdiv(kK1 + 1, 32), 3 * t->R1, &t->splits1, &t->kchunk1);
    // dW2: 47 row tiles of a K of 3 B h2 w2 (288 k at B = 32): 8 workgroups per CU keep the SIMDs busy
    pick_split(dcs_cdiv(kK2 + 1, 128), 3 * t->Rh, &t->splits2, &t->kchunk2, 2048);
    pick_split((int64_t)dcs_cdiv(batch, 32) * (kHidden / 32), t->flat, &t->splits3, &t->kchunk3);
    pick_split((int64_t)dcs_cdiv(batch, 32) * (kHidden / 32), 2 * t->flat, &t->splitsB3, &t->kchunkB3);

    const int64_t R1 = t->R1, RF = t->RF, B = batch, flat = t->flat;
    std::vector<std::pair<float**, int64_t>> parts = {
        {&t->rnd, RF}, {&t->xy, 3 * RF}, {&t->U, 3 * R1 * kC1}, {&t->GA, 3 * R1 * kC1},
        {&t->V, 3 * B * t->hp * t->wp * kC2}, {&t->Q, 2 * RF}, {&t->a2b, B * flat}, {&t->z, B * kHidden},
        {&t->prez, B * kHidden}, {&t->dprez, B * kHidden}, {&t->pre, 2 * B * flat}, {&t->dpre, 2 * B * flat},
        {&t->part1, (int64_t)t->splits1 * (kK1 + 1) * kC1}, {&t->part2, (int64_t)t->splits2 * (kK2 + 1) * kC2},
        {&t->partS, (int64_t)std::max(t->splits3, t->splitsB3) * B * kHidden}, {&t->sign, 1}};
    int64_t total = 0;
    for (auto& p : parts) total += dcs_round_up(p.second, 64);
    const int64_t dbl = (int64_t)kLossBlocks * kLossSums + 8;
    hipError_t e = dcs_dev_alloc((void**)&t->state, 16 * t->P4 * sizeof(float), "ikala trainer state");
    if (e == hipSuccess) e = dcs_dev_alloc((void**)&t->work, total * sizeof(float) + dbl * sizeof(double), "ikala trainer work");
    if (e != hipSuccess) {
        trainer_free(t);
        DCS_FAIL(e == hipErrorOutOfMemory ? DCS_ENOMEM : DCS_EHIP, "dcs_trainer_create: device allocation failed: %s",
                 hipGetErrorString(e));
    }
    int64_t at = 0;
    for (auto& p : parts) {
        *p.first = t->work + at;
        at += dcs_round_up(p.second, 64);
    }
    t->lpart = (double*)(t->work + at);
    t->out7 = t->lpart + (int64_t)kLossBlocks * kLossSums;
    // zero everything (the pad rows and columns of V stay zero for good; grads, accu, delta_accu and the section pads
    // start at zero), then the params
    if (hipMemsetAsync(t->work, 0, total * sizeof(float) + dbl * sizeof(double), ctx->stream) != hipSuccess ||
        hipMemsetAsync(t->state, 0, 16 * t->P4 * sizeof(float), ctx->stream) != hipSuccess ||
        hipMemcpyAsync(t->rnd, rand_d, RF * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
        trainer_free(t);
        DCS_FAIL(DCS_EHIP, "dcs_trainer_create: initialisation failed");
    }
    const int rc = layout(t, t->state, (float* const*)params_d, 1);
    if (rc != DCS_OK) {
        trainer_free(t);
        return rc;
    }
    *out = t;
    return DCS_OK;
}

int ik_trainer_destroy(ik_trainer* t) {
    if (!t) return DCS_OK;
    DCS_ON_DEVICE(t->ctx->device);
    DCS_HIP(hipStreamSynchronize(t->ctx->stream));
    trainer_free(t);
    return DCS_OK;
}

int ik_trainer_step(ik_trainer* t, const float* inputs_d, const float* targets_d, int mode, double* out7_d) {
    DCS_ON_DEVICE(t->ctx->device);
    DCS_CHECK(forward(t, inputs_d));
    DCS_CHECK(loss(t, inputs_d, targets_d, out7_d));
    if (mode == 0) return DCS_OK;
    DCS_CHECK(backward(t));
    if (mode == 1) return DCS_OK;
    hipLaunchKernelGGL(ik_adadelta_kernel, dim3((unsigned)dcs_cdiv(t->P4, kThreads)), dim3(kThreads), 0, t->ctx->stream,
                       (float4*)t->state, t->P4, (float)t->hyp[4], (float)t->hyp[5], (float)t->hyp[6]);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

int ik_trainer_forward(ik_trainer* t, const float* inputs_d, float* p_d) {
    DCS_ON_DEVICE(t->ctx->device);
    DCS_CHECK(forward(t, inputs_d));
    hipLaunchKernelGGL(ik_relu_kernel, dim3((unsigned)dcs_cdiv(2 * t->RF, kThreads)), dim3(kThreads), 0, t->ctx->stream,
                       (const float*)t->Q, p_d, 2 * t->RF);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

int ik_trainer_get(ik_trainer* t, int which, float* const* out_d, int nparams) {
    if (nparams != kNparams) DCS_FAIL(DCS_ESHAPE, "dcs_trainer_get: %d buffers for %d parameters", nparams, kNparams);
    for (int i = 0; i < kNparams; ++i)
        if (!out_d[i]) DCS_FAIL(DCS_EINVAL, "dcs_trainer_get: buffer %d is null", i);
    DCS_ON_DEVICE(t->ctx->device);
    return layout(t, t->state + which * 4 * t->P4, out_d, 0);
}

extern "C" {

DCS_API int dcs_trainer_gather_sources(dcs_ctx* ctx, const float* data_d, const int64_t* files_d, const int* windows_d,
                                       int batch, int time_context, int F, int nsrc, float scale, float* inputs_d,
                                       float* targets_d) {
    if (!ctx || !data_d || !files_d || !windows_d || !inputs_d || !targets_d)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_sources: null argument");
    if (batch < 1 || time_context < 1 || F < 1 || nsrc < 1 || nsrc > 8)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather_sources: batch %d, time_context %d, F %d, nsrc %d (1 .. 8)", batch,
                 time_context, F, nsrc);
    DCS_ON_DEVICE(ctx->device);
    const int64_t n = (int64_t)batch * time_context * F;
    hipLaunchKernelGGL(ik_gather_kernel, dim3((unsigned)dcs_cdiv(n, kThreads)), dim3(kThreads), 0, ctx->stream, data_d, files_d,
                       windows_d, batch, time_context, F, nsrc, scale, inputs_d, targets_d);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

}  // extern "C"

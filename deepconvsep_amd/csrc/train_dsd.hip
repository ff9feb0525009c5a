// Training of the DSD100 graph (examples/dsd100/trainCNN.py: build_ca :66-130, loss :167-219, adadelta :223) on gfx950.
//
// One step on the ctx stream, no host synchronisation and no float atomics (two runs give bit-identical weights):
//
//   forward   F1 a1b = x . W1 + b1 + b1b              tr_gemm_kernel  (saved: a1b)
//             F2 a2b = conv2(a1b) + b2 + b2b          tr_gemm_kernel  implicit GEMM over the tc/2 taps (saved: a2b)
//             F3 z = rectify(a2b . Wfc + bfc)          tr_gemm_kernel  (saved: z and its pre-activation)
//             F4 d_k = rectify(z . W_k + b_k), k<3     tr_gemm_kernel  3 batches (saved: d_k and pre-activations)
//             F5 g_k = conv2^T(d_k)                    tr_gemm_kernel  3 batches, implicit GEMM (InverseLayer of conv2)
//             F6 q = conv1^T(g_k) + bo                 tr_gemm_kernel  4 batches: channel 3 repeats branch 1 (l_fc14 is dead)
//   loss      tr_loss_kernel: masks, the six components, dE/dq (relu' with the 0.5 tie) per element, per-workgroup f64 sums
//             tr_loss_reduce_kernel: fixed-order sum -> loss and components (f64), sign(E), the output-bias gradient
//   backward  B1 dg_k = dY_k . W1^T     B2 dpre_k = conv2(dg_k) * r'(pre_k)     B3 dprez = (sum_k dpre_k . W_k^T) * r'(prez)
//             B4 da2 = dprez . Wfc^T    B5 da1 = conv2^T(da2)
//   weights   dW1|db1 = [x; dY_k]^T . [da1; g_k]           split-K (K = 4 B tc), fixed-order reduce
//             dW2|db2 = windows of [a1b; dg_k]^T . [da2; d_k]  split-K (K = 4 B h2), fixed-order reduce
//             dWfc|dbfc = a2b^T . dprez,  dW_k|db_k = z^T . dpre_k
//             every bias gradient is the "ones" row of its weight GEMM; b1b / b2b get copies of b1 / b2 (identical in Theano)
//   update    tr_adadelta_kernel over the flat [params | grads | accu | delta_accu] buffer
//
// Every GEMM is one template, tr_gemm_kernel: 64 x 64 tile per workgroup, 4 waves of 2 x 2 v_mfma_f32_16x16x4_f32, K staged
// through LDS 32 at a time with the next step's operands prefetched into registers.  Operands are addressed through TMat:
// element (i, j) at off + (i / idiv) * is_hi + (i % idiv) * is_lo + (j / jdiv) * js_hi + (j % jdiv) * js_lo, which covers
// row-major, transposed, the implicit-GEMM windows of conv2 and the K-concatenations above without copies.
//
// Internal parameter layouts (the flat buffer; dcs_trainer_get / _create convert to and from the .pkl layout):
//   W1 [F][50]: W1i[f][c] = W1[c,0,0,F-1-f]  (flip_filters=True)     W2 [kh][50 c][50 o]: W2i[j][c][o] = W2[o,c,j,0]
//   Wfc [(h,o)][128] and W_k [128][(h,o)], b_k [(h,o)]: the 50 x h2 map in (row h, channel o) order, .pkl order is o*h2+h
// Activations are channels-last: a1b / dg / g / da1 [B][tc][50], a2b / d_k [B][h2][50]; d_k and da2 live in a buffer padded
// by kh-1 zero rows on either side so that conv2^T is a plain implicit GEMM.
#include <math.h>
#include <algorithm>
#include <string.h>

#include "dcs_internal.h"
#include "train_ikala.h"

namespace {

constexpr int kThreads = 256;
constexpr int kBM = 64, kBN = 64, kKT = 32;
constexpr int kNf = 50, kHidden = 128, kNparams = 15;
constexpr int kBig = 1 << 30;
constexpr int kLossBlocks = 1024;
constexpr int kLossSums = 10;    // six components, four output-bias gradient sums

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct TMat {
    float* p;
    int64_t off;
    int idiv; int64_t is_hi, is_lo;
    int jdiv; int64_t js_hi, js_lo;
};

__device__ __forceinline__ int64_t tm_row(const TMat& m, int i) {
    return (int64_t)(i / m.idiv) * m.is_hi + (int64_t)(i % m.idiv) * m.is_lo;
}
__device__ __forceinline__ int64_t tm_col(const TMat& m, int j) {
    return (int64_t)(j / m.jdiv) * m.js_hi + (int64_t)(j % m.jdiv) * m.js_lo;
}

TMat tm(float* p, int64_t off, int64_t is, int64_t js) { return TMat{p, off, kBig, 0, is, kBig, 0, js}; }
TMat tm2(float* p, int64_t off, int idiv, int64_t is_hi, int64_t is_lo, int jdiv, int64_t js_hi, int64_t js_lo) {
    return TMat{p, off, idiv, is_hi, is_lo, jdiv, js_hi, js_lo};
}

enum { EPI_RELU = 1, EPI_SAVEPRE = 2, EPI_DRELU = 4 };

struct TGemm {
    TMat A, B, C, X;              // C = A . B; X: pre-activations (EPI_SAVEPRE writes, EPI_DRELU reads), C's shape
    int M, N, K;
    int ones_row, ones_klim;      // rows >= ones_row of A read 1 for k < ones_klim, else 0 (bias gradients)
    int nbatch;
    int64_t boff[4][5];           // per batch: offsets of A, B, C, X, bias
    const float* bias;            // nullable: bias[boff[.][4] + n * bias_cs]
    int bias_cs;                  // 1: per column; 0: one value per batch (the output bias of one channel)
    const float* bias2;           // nullable, added too (the BiasLayer that follows a layer)
    const float* scale;           // nullable device scalar: sign(E)
    int epi;
    float* partial;               // non-null: raw sums to partial[(batch * splits + s)][M][N], no epilogue (even at one slice)
    int splits, kchunk;
};

__device__ __forceinline__ float relu_d(float pre) { return pre > 0.f ? 1.f : (pre == 0.f ? 0.5f : 0.f); }

__global__ __launch_bounds__(kThreads) void tr_gemm_kernel(const TGemm g) {
    __shared__ float As[kKT][kBM + 1];
    __shared__ float Bs[kKT][kBN + 1];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int r16 = lane & 15, kq = lane >> 4;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * kBN;
    const int batch = blockIdx.z / g.splits, split = blockIdx.z - batch * g.splits;
    const int kbeg = split * g.kchunk;
    const int kend = min(g.K, kbeg + g.kchunk);
    const float* Ap = g.A.p + g.A.off + g.boff[batch][0];
    const float* Bp = g.B.p + g.B.off + g.boff[batch][1];

    // A tile: k fastest (lane kl = t % 32), rows t / 32 + 8 j.  B tile: n fastest (t % 64), k rows t / 64 + 4 j.
    const int akl = t & 31, aml = t >> 5;
    int64_t arow[8];
    bool aok[8], aone[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int m = m0 + aml + 8 * j;
        aok[j] = m < g.M;
        aone[j] = m >= g.ones_row;
        arow[j] = (aok[j] && !aone[j]) ? tm_row(g.A, m) : 0;
    }
    const int bnl = t & 63, bkl = t >> 6;
    const bool bok = n0 + bnl < g.N;
    const int64_t bcol = bok ? tm_col(g.B, n0 + bnl) : 0;

    float ra[8], rb[8];
    auto load = [&](int k0) {
        const int ka = k0 + akl;
        const bool kin = ka < kend;
        const int64_t acol = kin ? tm_col(g.A, ka) : 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            float v = 0.f;
            if (aok[j] && kin) v = aone[j] ? (ka < g.ones_klim ? 1.f : 0.f) : Ap[arow[j] + acol];
            ra[j] = v;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int kb = k0 + bkl + 4 * j;
            rb[j] = (bok && kb < kend) ? Bp[tm_row(g.B, kb) + bcol] : 0.f;
        }
    };

    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (kbeg < kend) load(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += kKT) {
#pragma unroll
        for (int j = 0; j < 8; ++j) As[akl][aml + 8 * j] = ra[j];
#pragma unroll
        for (int j = 0; j < 8; ++j) Bs[bkl + 4 * j][bnl] = rb[j];
        __syncthreads();
        if (k0 + kKT < kend) load(k0 + kKT);
#pragma unroll
        for (int s = 0; s < kKT / 4; ++s) {
            const int kk = 4 * s + kq;
            float a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = As[kk][wm + 16 * i + r16];
#pragma unroll
            for (int j = 0; j < 2; ++j) b[j] = Bs[kk][wn + 16 * j + r16];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // C/D map of the 16x16 tile: column = lane & 15, row = 4 (lane >> 4) + reg
    const float sc = g.scale ? *g.scale : 1.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
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
                    float* x = g.X.p + g.X.off + g.boff[batch][3] + tm_row(g.X, m) + tm_col(g.X, n);
                    if (g.epi & EPI_SAVEPRE) *x = v;
                    else v *= relu_d(*x);
                }
                if (g.epi & EPI_RELU) v = v > 0.f ? v : 0.f;
                g.C.p[g.C.off + g.boff[batch][2] + tm_row(g.C, m) + tm_col(g.C, n)] = v;
            }
}

// Split-K partials summed in slice order, times sign(E), into the gradient buffer; dup > 0: the last row (the bias
// gradient) is written once more right after it (BiasLayer.b gets the layer bias's gradient).
struct TReduce {
    const float* part[2];
    float* dst[2];
    int64_t count[2];
    int splits[2];
    int N[2];
    int dup[2];
    const float* scale;
};

__global__ __launch_bounds__(kThreads) void tr_reduce_kernel(const TReduce r) {
    const int j = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= r.count[j]) return;
    float s = 0.f;
    for (int z = 0; z < r.splits[j]; ++z) s += r.part[j][z * r.count[j] + i];
    s *= *r.scale;
    r.dst[j][i] = s;
    if (r.dup[j] && i >= r.count[j] - r.N[j]) r.dst[j][i + r.N[j]] = s;
}

struct TLoss {
    const float* q;       // [B][4][tc F] pre-activations of the output layer
    const float* x;       // [B][tc F] inputs
    const float* tgt;     // [B][4][tc F] targets
    const float* rnd;     // [B][tc F] the uniform draw
    float* xy;            // [4][B tc F]: slot 0 <- x, slots 1..3 <- dE/dY_k (branch 1 collects channels 1 and 3)
    double* part;         // [gridDim.x][kLossSums]
    int64_t plane, n;     // tc F, B tc F
    double eps, alpha, beta, beta_voc;
};

// trainCNN.py:176-219 per element, in f64: s_i = p_i + eps r, m_i = s_i / sum_j s_j, sources m_i x for vocals, bass, drums;
// the six squared-error sums; dE/dp_j = x / D (G_j - sum_i m_i G_i) with G the derivative of E in the three sources (G_3 = 0:
// "other" enters only through D); dE/dq = dE/dp r'(q) with rectify's r'(0) = 0.5.
__global__ __launch_bounds__(kThreads) void tr_loss_kernel(const TLoss a) {
    __shared__ double red[kLossSums][kThreads];
    double acc[kLossSums];
#pragma unroll
    for (int i = 0; i < kLossSums; ++i) acc[i] = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < a.n; e += (int64_t)gridDim.x * kThreads) {
        const int64_t b = e / a.plane, rem = e - b * a.plane;
        const int64_t o = b * 4 * a.plane + rem;
        const double x = a.x[e], er = a.eps * (double)a.rnd[e];
        double q[4], s[4], t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            q[j] = a.q[o + j * a.plane];
            t[j] = a.tgt[o + j * a.plane];
            s[j] = (q[j] > 0.0 ? q[j] : 0.0) + er;
        }
        const double D = s[0] + s[1] + s[2] + s[3];
        const double v = s[0] / D * x, bs = s[1] / D * x, dr = s[2] / D * x;
        const double ev0 = v - t[0], ev1 = v - t[1], ev2 = v - t[2], ev3 = v - t[3];
        const double eb0 = bs - t[0], eb1 = bs - t[1], eb2 = bs - t[2], eb3 = bs - t[3];
        const double ed0 = dr - t[0], ed1 = dr - t[1], ed2 = dr - t[2], ed3 = dr - t[3];
        acc[0] += ev0 * ev0;                                                   // vocals
        acc[1] += eb1 * eb1;                                                   // bass
        acc[2] += ed2 * ed2;                                                   // drums
        acc[3] += a.beta * (eb3 * eb3) + a.beta * (ed3 * ed3);                 // negative
        acc[4] += a.alpha * (ev1 * ev1) + a.alpha * (ev2 * ev2) + a.alpha * (eb0 * eb0) + a.alpha * (eb2 * eb2) +
                  a.alpha * (ed0 * ed0) + a.alpha * (ed1 * ed1);               // alpha
        acc[5] += a.beta_voc * (ev3 * ev3);                                    // negative_voc
        double G[3];
        G[0] = 2.0 * (ev0 - a.alpha * ev1 - a.alpha * ev2 - a.beta_voc * ev3);
        G[1] = 2.0 * (eb1 - a.alpha * eb0 - a.alpha * eb2 - a.beta * eb3);
        G[2] = 2.0 * (ed2 - a.alpha * ed0 - a.alpha * ed1 - a.beta * ed3);
        const double mg = (s[0] * G[0] + s[1] * G[1] + s[2] * G[2]) / D;
        double dq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double gj = (j < 3 ? G[j] : 0.0) - mg;
            const double rd = q[j] > 0.0 ? 1.0 : (q[j] == 0.0 ? 0.5 : 0.0);
            dq[j] = x / D * gj * rd;
            acc[6 + j] += dq[j];
        }
        a.xy[e] = (float)x;
        a.xy[a.n + e] = (float)dq[0];
        a.xy[2 * a.n + e] = (float)(dq[1] + dq[3]);
        a.xy[3 * a.n + e] = (float)dq[2];
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

// out7 = (|E|, vocals, bass, drums, negative, alpha, negative_voc) with E = vocals + drums + bass - negative - alpha -
// negative_voc (trainCNN.py:217); sign(E) (abs'(0) = 0) for the gradient epilogues; the output-bias gradient.
__global__ __launch_bounds__(kThreads) void tr_loss_reduce_kernel(const double* __restrict__ part, int nblk, double* out7,
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
        const double E = red[0][0] + red[2][0] + red[1][0] - red[3][0] - red[4][0] - red[5][0];
        const float sg = E > 0.0 ? 1.f : (E < 0.0 ? -1.f : 0.f);
        out7[0] = fabs(E);
        for (int i = 0; i < 6; ++i) out7[1 + i] = red[i][0];
        *sign = sg;
        for (int j = 0; j < 4; ++j) dbo[j] = sg * (float)red[6 + j][0];
    }
}

// lasagne.updates.adadelta (lasagne/updates.py adadelta): accu' = rho accu + (1 - rho) g^2,
// u = g sqrt(delta + eps) / sqrt(accu' + eps), p -= lr u, delta' = rho delta + (1 - rho) u^2.
__global__ __launch_bounds__(kThreads) void tr_adadelta_kernel(float* __restrict__ state, int64_t P, float lr, float rho,
                                                               float eps) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= P) return;
    float* p = state;
    const float* g = state + P;
    float* acc = state + 2 * P;
    float* del = state + 3 * P;
    const float gi = g[i];
    const float a = rho * acc[i] + (1.f - rho) * gi * gi;
    const float u = gi * sqrtf(del[i] + eps) / sqrtf(a + eps);
    p[i] = p[i] - lr * u;
    acc[i] = a;
    del[i] = rho * del[i] + (1.f - rho) * u * u;
}

__global__ __launch_bounds__(kThreads) void tr_relu_kernel(const float* __restrict__ q, float* __restrict__ p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) p[i] = q[i] > 0.f ? q[i] : 0.f;
}

// .pkl layout <-> internal layout, one element of the flat parameter section per thread.  to_internal: flat[i] = pkl[src];
// else pkl[src] = flat[i].
struct TLayout {
    float* pkl[kNparams];
    int64_t off[kNparams + 1];
    int F, kh, h2;
    int to_internal;
};

__global__ __launch_bounds__(kThreads) void tr_layout_kernel(float* __restrict__ flat, const TLayout L) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= L.off[kNparams]) return;
    int s = 0;
    while (i >= L.off[s + 1]) ++s;
    const int64_t k = i - L.off[s];
    const int64_t map = kNf * (int64_t)L.h2;
    int64_t src = k;
    if (s == 0) {                                     // W1i[f][c] = W1[c][F-1-f]
        const int64_t f = k / kNf, c = k % kNf;
        src = c * L.F + (L.F - 1 - f);
    } else if (s == 3) {                              // W2i[j][c][o] = W2[o][c][j]
        const int64_t j = k / (kNf * kNf), c = (k / kNf) % kNf, o = k % kNf;
        src = (o * kNf + c) * L.kh + j;
    } else if (s == 6) {                              // Wfc rows (h, o) <- o h2 + h
        const int64_t row = k / kHidden, n = k % kHidden;
        src = ((row % kNf) * L.h2 + row / kNf) * kHidden + n;
    } else if (s == 8 || s == 10 || s == 12) {        // W_k columns (h, o) <- o h2 + h
        const int64_t n = k / map, col = k % map;
        src = n * map + (col % kNf) * L.h2 + col / kNf;
    } else if (s == 9 || s == 11 || s == 13) {
        src = (k % kNf) * L.h2 + k / kNf;
    }
    if (L.to_internal) flat[i] = L.pkl[s][src];
    else L.pkl[s][src] = flat[i];
}

// (file, start) windows of the resident feature files -> network inputs and targets (dataset.py loadFile / initOutput):
// data [sum_i 5 T_i F] float32, file i at files[2 i] with T_i = files[2 i + 1] frames; win [B][2]; file < 0: an all-zero
// window; frames past T_i are zero (the padded window of a file shorter than tc).
__global__ __launch_bounds__(kThreads) void tr_gather_kernel(const float* __restrict__ data, const int64_t* __restrict__ files,
                                                             const int* __restrict__ win, int B, int tc, int F, float scale,
                                                             float* __restrict__ inputs, float* __restrict__ targets) {
    const int64_t plane = (int64_t)tc * F;
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (int64_t)B * plane) return;
    const int b = (int)(e / plane);
    const int64_t rem = e - b * plane;
    const int t = (int)(rem / F), f = (int)(rem - (int64_t)t * F);
    const int fi = win[2 * b], start = win[2 * b + 1];
    float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (fi >= 0) {
        const int64_t base = files[2 * fi], T = files[2 * fi + 1];
        const int64_t fr = (int64_t)start + t;
        if (fr < T)
            for (int c = 0; c < 5; ++c) v[c] = scale * data[base + ((int64_t)c * T + fr) * F + f];
    }
    inputs[e] = v[0];
    for (int c = 0; c < 4; ++c) targets[((int64_t)b * 4 + c) * plane + rem] = v[1 + c];
}

}  // namespace

struct dcs_trainer {
    dcs_ctx* ctx = nullptr;
    ik_trainer* ik = nullptr;    // the iKala graph (train_ikala.hip); null for the DSD graph
    int tc = 0, F = 0, B = 0, kh = 0, h2 = 0, hp = 0;
    int64_t R = 0, Rh = 0, map = 0, P = 0;
    double hyp[7] = {0};
    int64_t off[kNparams + 1] = {0};
    float* state = nullptr;      // [4][P]: params, grads, accu, delta_accu
    float* work = nullptr;
    double* lpart = nullptr;
    double* out7 = nullptr;      // when the caller passes none
    // views into work
    float *rnd, *xy, *U, *GA, *V, *Q, *a2b, *z, *prez, *dprez, *pre, *dpre, *part1, *part2, *sign;
    int splits1 = 1, splits2 = 1, kchunk1 = 0, kchunk2 = 0;
};

namespace {

void shapes_of(int tc, int F, int64_t s[kNparams][4]) {
    const int kh = tc / 2, h2 = tc - kh + 1, map = kNf * h2;
    const int64_t t[kNparams][4] = {{kNf, 1, 1, F}, {kNf, 1, 1, 1}, {kNf, 1, 1, 1}, {kNf, kNf, kh, 1}, {kNf, 1, 1, 1},
                                    {kNf, 1, 1, 1}, {map, kHidden, 1, 1}, {kHidden, 1, 1, 1}, {kHidden, map, 1, 1},
                                    {map, 1, 1, 1}, {kHidden, map, 1, 1}, {map, 1, 1, 1}, {kHidden, map, 1, 1},
                                    {map, 1, 1, 1}, {4, 1, 1, 1}};
    memcpy(s, t, sizeof(t));
}

TGemm gemm0(int M, int N, int K) {
    TGemm g;
    memset(&g, 0, sizeof(g));
    g.M = M; g.N = N; g.K = K;
    g.ones_row = kBig;
    g.nbatch = 1;
    g.splits = 1;
    g.kchunk = K;
    g.bias_cs = 1;
    return g;
}

int launch(dcs_trainer* t, TGemm g) {
    if (g.splits < 1) g.splits = 1;
    if (g.splits == 1) g.kchunk = g.K;
    dim3 grid((unsigned)dcs_cdiv(g.M, kBM), (unsigned)dcs_cdiv(g.N, kBN), (unsigned)(g.nbatch * g.splits));
    hipLaunchKernelGGL(tr_gemm_kernel, grid, dim3(kThreads), 0, t->ctx->stream, g);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

// K split into slices of a multiple of kKT for a grid of about 2 workgroups per CU
void pick_split(int64_t tiles, int64_t K, int* splits, int* kchunk) {
    int64_t s = 512 / (tiles > 0 ? tiles : 1);
    s = s < 1 ? 1 : (s > 64 ? 64 : s);
    int64_t kc = dcs_round_up((K + s - 1) / s, kKT);
    if (kc < 256) kc = dcs_round_up(256 < K ? 256 : K, kKT);
    *kchunk = (int)kc;
    *splits = (int)((K + kc - 1) / kc);
}

float* P_(dcs_trainer* t, int i) { return t->state + t->off[i]; }

int forward(dcs_trainer* t, const float* x) {
    const int B = t->B, tc = t->tc, F = t->F, kh = t->kh, h2 = t->h2, hp = t->hp;
    const int64_t R = t->R, Rh = t->Rh, map = t->map, padrow = (int64_t)(kh - 1) * kNf, Vslot = (int64_t)B * hp * kNf;
    const int64_t R50 = R * kNf, plane = (int64_t)tc * F;
    // F1: a1b = x . W1i + b1 + b1b -> U slot 0
    {
        TGemm g = gemm0((int)R, kNf, F);
        g.A = tm((float*)x, 0, F, 1);
        g.B = tm(P_(t, 0), 0, kNf, 1);
        g.C = tm(t->U, 0, kNf, 1);
        g.bias = P_(t, 1); g.bias2 = P_(t, 2);
        DCS_CHECK(launch(t, g));
    }
    // F2: a2b[(b,h)][o] = sum_{k',c} a1b[b][h+k'][c] W2i[kh-1-k'][c][o] + b2 + b2b
    {
        TGemm g = gemm0((int)Rh, kNf, kh * kNf);
        g.A = tm2(t->U, 0, h2, (int64_t)tc * kNf, kNf, kBig, 0, 1);
        g.B = tm2(P_(t, 3), (int64_t)(kh - 1) * kNf * kNf, kNf, -(int64_t)kNf * kNf, kNf, kBig, 0, 1);
        g.C = tm(t->a2b, 0, kNf, 1);
        g.bias = P_(t, 4); g.bias2 = P_(t, 5);
        DCS_CHECK(launch(t, g));
    }
    // F3: z = rectify(a2b . Wfci + bfc), pre-activation saved
    {
        TGemm g = gemm0(B, kHidden, (int)map);
        g.A = tm(t->a2b, 0, map, 1);
        g.B = tm(P_(t, 6), 0, kHidden, 1);
        g.C = tm(t->z, 0, kHidden, 1);
        g.X = tm(t->prez, 0, kHidden, 1);
        g.bias = P_(t, 7);
        g.epi = EPI_RELU | EPI_SAVEPRE;
        DCS_CHECK(launch(t, g));
    }
    // F4: d_k = rectify(z . W_ki + b_ki) -> V slots 1..3 (padded rows), pre-activations saved
    {
        TGemm g = gemm0(B, (int)map, kHidden);
        g.A = tm(t->z, 0, kHidden, 1);
        g.B = tm(P_(t, 8), 0, map, 1);
        g.C = tm(t->V, padrow, (int64_t)hp * kNf, 1);
        g.X = tm(t->pre, 0, map, 1);
        g.bias = P_(t, 9);
        g.epi = EPI_RELU | EPI_SAVEPRE;
        g.nbatch = 3;
        for (int k = 0; k < 3; ++k) {
            const int64_t wstep = t->off[10] - t->off[8];
            g.boff[k][1] = k * wstep;
            g.boff[k][2] = (k + 1) * Vslot;
            g.boff[k][3] = k * (int64_t)B * map;
            g.boff[k][4] = k * wstep;
        }
        DCS_CHECK(launch(t, g));
    }
    // F5: g_k[(b,t)][c] = sum_{j,o} Vpad[b][t+j][o] W2i[j][c][o] -> GA slots 1..3
    {
        TGemm g = gemm0((int)R, kNf, kh * kNf);
        g.A = tm2(t->V, 0, tc, (int64_t)hp * kNf, kNf, kBig, 0, 1);
        g.B = tm2(P_(t, 3), 0, kNf, (int64_t)kNf * kNf, 1, kBig, 0, kNf);
        g.C = tm(t->GA, 0, kNf, 1);
        g.nbatch = 3;
        for (int k = 0; k < 3; ++k) {
            g.boff[k][0] = (k + 1) * Vslot;
            g.boff[k][2] = (k + 1) * R50;
        }
        DCS_CHECK(launch(t, g));
    }
    // F6: q[b][ch][t][f] = sum_c g_br(ch)[(b,t)][c] W1i[f][c] + bo[ch], br = 0, 1, 2, 1
    {
        TGemm g = gemm0((int)R, F, kNf);
        g.A = tm(t->GA, 0, kNf, 1);
        g.B = tm(P_(t, 0), 0, 1, kNf);
        g.C = tm2(t->Q, 0, tc, 4 * plane, F, kBig, 0, 1);
        g.bias = P_(t, 14);
        g.nbatch = 4;
        const int br[4] = {0, 1, 2, 1};
        for (int ch = 0; ch < 4; ++ch) {
            g.boff[ch][0] = (br[ch] + 1) * R50;
            g.boff[ch][2] = ch * plane;
            g.boff[ch][4] = ch;
        }
        g.bias_cs = 0;
        DCS_CHECK(launch(t, g));
    }
    return DCS_OK;
}

int loss(dcs_trainer* t, const float* x, const float* tgt, double* out7) {
    TLoss a;
    a.q = t->Q; a.x = x; a.tgt = tgt; a.rnd = t->rnd; a.xy = t->xy; a.part = t->lpart;
    a.plane = (int64_t)t->tc * t->F;
    a.n = t->R * t->F;
    a.eps = t->hyp[0]; a.alpha = t->hyp[1]; a.beta = t->hyp[2]; a.beta_voc = t->hyp[3];
    const int nblk = (int)std::min<int64_t>(kLossBlocks, dcs_cdiv(a.n, kThreads));
    hipLaunchKernelGGL(tr_loss_kernel, dim3(nblk), dim3(kThreads), 0, t->ctx->stream, a);
    DCS_HIP(hipGetLastError());
    hipLaunchKernelGGL(tr_loss_reduce_kernel, dim3(1), dim3(kThreads), 0, t->ctx->stream, (const double*)t->lpart, nblk,
                       out7 ? out7 : t->out7, t->sign, t->state + t->P + t->off[14]);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

int backward(dcs_trainer* t) {
    const int B = t->B, tc = t->tc, F = t->F, kh = t->kh, h2 = t->h2, hp = t->hp;
    const int64_t R = t->R, Rh = t->Rh, map = t->map, padrow = (int64_t)(kh - 1) * kNf, Vslot = (int64_t)B * hp * kNf;
    const int64_t R50 = R * kNf, RF = R * F, Bmap = (int64_t)B * map, wstep = t->off[10] - t->off[8];
    float* grad = t->state + t->P;
    // B1: dg_k = dY_k . W1i -> U slots 1..3
    {
        TGemm g = gemm0((int)R, kNf, F);
        g.A = tm(t->xy, 0, F, 1);
        g.B = tm(P_(t, 0), 0, kNf, 1);
        g.C = tm(t->U, 0, kNf, 1);
        g.nbatch = 3;
        for (int k = 0; k < 3; ++k) {
            g.boff[k][0] = (k + 1) * RF;
            g.boff[k][2] = (k + 1) * R50;
        }
        DCS_CHECK(launch(t, g));
    }
    // B2: dpre_k = conv2(dg_k) * r'(pre_k)  (the F2 form)
    {
        TGemm g = gemm0((int)Rh, kNf, kh * kNf);
        g.A = tm2(t->U, 0, h2, (int64_t)tc * kNf, kNf, kBig, 0, 1);
        g.B = tm2(P_(t, 3), (int64_t)(kh - 1) * kNf * kNf, kNf, -(int64_t)kNf * kNf, kNf, kBig, 0, 1);
        g.C = tm(t->dpre, 0, kNf, 1);
        g.X = tm(t->pre, 0, kNf, 1);
        g.epi = EPI_DRELU;
        g.nbatch = 3;
        for (int k = 0; k < 3; ++k) {
            g.boff[k][0] = (k + 1) * R50;
            g.boff[k][2] = k * Bmap;
            g.boff[k][3] = k * Bmap;
        }
        DCS_CHECK(launch(t, g));
    }
    // B3: dprez = (sum_k dpre_k . W_ki^T) * r'(prez): K = 3 map, concatenated over k
    {
        TGemm g = gemm0(B, kHidden, (int)(3 * map));
        g.A = tm2(t->dpre, 0, kBig, 0, map, (int)map, Bmap, 1);
        g.B = tm2(P_(t, 8), 0, (int)map, wstep, 1, kBig, 0, map);
        g.C = tm(t->dprez, 0, kHidden, 1);
        g.X = tm(t->prez, 0, kHidden, 1);
        g.epi = EPI_DRELU;
        DCS_CHECK(launch(t, g));
    }
    // B4: da2 = dprez . Wfci^T -> V slot 0 (padded rows)
    {
        TGemm g = gemm0(B, (int)map, kHidden);
        g.A = tm(t->dprez, 0, kHidden, 1);
        g.B = tm(P_(t, 6), 0, 1, kHidden);
        g.C = tm(t->V, padrow, (int64_t)hp * kNf, 1);
        DCS_CHECK(launch(t, g));
    }
    // B5: da1 = conv2^T(da2) -> GA slot 0  (the F5 form)
    {
        TGemm g = gemm0((int)R, kNf, kh * kNf);
        g.A = tm2(t->V, 0, tc, (int64_t)hp * kNf, kNf, kBig, 0, 1);
        g.B = tm2(P_(t, 3), 0, kNf, (int64_t)kNf * kNf, 1, kBig, 0, kNf);
        g.C = tm(t->GA, 0, kNf, 1);
        DCS_CHECK(launch(t, g));
    }
    // dW1 | db1: [x; dY_k]^T [F][4R] . [da1; g_k] [4R][50], ones row over the x block
    {
        TGemm g = gemm0(F + 1, kNf, (int)(4 * R));
        g.A = tm(t->xy, 0, 1, F);
        g.B = tm(t->GA, 0, kNf, 1);
        g.ones_row = F; g.ones_klim = (int)R;
        g.partial = t->part1; g.splits = t->splits1; g.kchunk = t->kchunk1;
        DCS_CHECK(launch(t, g));
    }
    // dW2 | db2: dW2i[(j,c)][o] = sum_{(s,b,h)} U[s][b][h+kh-1-j][c] Vpad[s][b][h+kh-1][o], ones row over the da2 block
    {
        TGemm g = gemm0(kh * kNf + 1, kNf, (int)(4 * Rh));
        g.A = tm2(t->U, (int64_t)(kh - 1) * kNf, kNf, -(int64_t)kNf, 1, h2, (int64_t)tc * kNf, kNf);
        g.B = tm2(t->V, padrow, h2, (int64_t)hp * kNf, kNf, kBig, 0, 1);
        g.ones_row = kh * kNf; g.ones_klim = (int)Rh;
        g.partial = t->part2; g.splits = t->splits2; g.kchunk = t->kchunk2;
        DCS_CHECK(launch(t, g));
    }
    // dWfc | dbfc = [a2b^T; 1] . dprez -> grads (Wfc and bfc are adjacent)
    {
        TGemm g = gemm0((int)map + 1, kHidden, B);
        g.A = tm(t->a2b, 0, 1, map);
        g.B = tm(t->dprez, 0, kHidden, 1);
        g.C = tm(grad + t->off[6], 0, kHidden, 1);
        g.ones_row = (int)map; g.ones_klim = B;
        g.scale = t->sign;
        DCS_CHECK(launch(t, g));
    }
    // dW_k | db_k = [z^T; 1] . dpre_k -> grads (W_k and b_k are adjacent)
    {
        TGemm g = gemm0(kHidden + 1, (int)map, B);
        g.A = tm(t->z, 0, 1, kHidden);
        g.B = tm(t->dpre, 0, map, 1);
        g.C = tm(grad + t->off[8], 0, map, 1);
        g.ones_row = kHidden; g.ones_klim = B;
        g.scale = t->sign;
        g.nbatch = 3;
        for (int k = 0; k < 3; ++k) {
            g.boff[k][1] = k * Bmap;
            g.boff[k][2] = k * wstep;
        }
        DCS_CHECK(launch(t, g));
    }
    {
        TReduce r;
        memset(&r, 0, sizeof(r));
        r.scale = t->sign;
        r.part[0] = t->part1; r.dst[0] = grad + t->off[0]; r.count[0] = (int64_t)(F + 1) * kNf; r.splits[0] = t->splits1;
        r.part[1] = t->part2; r.dst[1] = grad + t->off[3]; r.count[1] = (int64_t)(kh * kNf + 1) * kNf;
        r.splits[1] = t->splits2;
        r.N[0] = r.N[1] = kNf;
        r.dup[0] = r.dup[1] = 1;
        const int64_t most = std::max(r.count[0], r.count[1]);
        hipLaunchKernelGGL(tr_reduce_kernel, dim3((unsigned)dcs_cdiv(most, kThreads), 2), dim3(kThreads), 0, t->ctx->stream, r);
        DCS_HIP(hipGetLastError());
    }
    return DCS_OK;
}

int layout(dcs_trainer* t, float* flat, float* const* pkl, int to_internal) {
    TLayout L;
    for (int i = 0; i < kNparams; ++i) {
        L.pkl[i] = pkl[i];
        L.off[i] = t->off[i];
    }
    L.off[kNparams] = t->off[kNparams];
    L.F = t->F; L.kh = t->kh; L.h2 = t->h2;
    L.to_internal = to_internal;
    hipLaunchKernelGGL(tr_layout_kernel, dim3((unsigned)dcs_cdiv(t->P, kThreads)), dim3(kThreads), 0, t->ctx->stream, flat, L);
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

extern "C" {

DCS_API int dcs_trainer_create(dcs_ctx* ctx, int arch, int time_context, int F, int batch, const float* const* params_d,
                               const int64_t* shapes, int nparams, const float* rand_d, const double* hyper_h,
                               dcs_trainer** out) {
    if (!ctx || !out || !rand_d || !hyper_h) DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: null argument");
    *out = nullptr;
    if (arch == DCS_ARCH_IKALA_NOPOOL) {
        ik_trainer* ik = nullptr;
        DCS_CHECK(ik_trainer_create(ctx, time_context, F, batch, params_d, shapes, nparams, rand_d, hyper_h, &ik));
        dcs_trainer* t = new dcs_trainer();
        t->ctx = ctx;
        t->ik = ik;
        *out = t;
        return DCS_OK;
    }
    if (arch != DCS_ARCH_DSD)
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_trainer_create: only the DSD graph (arch %d) and the no-pool iKala graph (arch %d) "
                 "train here", DCS_ARCH_DSD, DCS_ARCH_IKALA_NOPOOL);
    if (time_context < 4 || time_context > 64 || time_context % 2 || F < 1 || F > 2049 || batch < 1 || batch > 1024)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: time_context %d (even, 4 .. 64), F %d (1 .. 2049), batch %d (1 .. 1024)",
                 time_context, F, batch);
    if (!params_d || !shapes || nparams != kNparams)
        DCS_FAIL(DCS_ESHAPE, "mismatch: got %d values to set %d parameters", nparams, kNparams);
    int64_t want[kNparams][4];
    shapes_of(time_context, F, want);
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
    dcs_trainer* t = new dcs_trainer();
    t->ctx = ctx;
    t->tc = time_context; t->F = F; t->B = batch;
    t->kh = time_context / 2;
    t->h2 = time_context - t->kh + 1;
    t->hp = time_context + t->kh - 1;
    t->R = (int64_t)batch * time_context;
    t->Rh = (int64_t)batch * t->h2;
    t->map = (int64_t)kNf * t->h2;
    memcpy(t->hyp, hyper_h, sizeof(t->hyp));
    t->off[0] = 0;
    for (int i = 0; i < kNparams; ++i) t->off[i + 1] = t->off[i] + want[i][0] * want[i][1] * want[i][2] * want[i][3];
    t->P = t->off[kNparams];
    pick_split(dcs_cdiv(F + 1, kBM), 4 * t->R, &t->splits1, &t->kchunk1);
    pick_split(dcs_cdiv(t->kh * kNf + 1, kBM), 4 * t->Rh, &t->splits2, &t->kchunk2);

    const int64_t R = t->R, RF = t->R * F, B = batch;
    std::vector<std::pair<float**, int64_t>> parts = {
        {&t->rnd, RF}, {&t->xy, 4 * RF}, {&t->U, 4 * R * kNf}, {&t->GA, 4 * R * kNf}, {&t->V, 4 * B * t->hp * kNf},
        {&t->Q, 4 * RF}, {&t->a2b, B * t->map}, {&t->z, B * kHidden}, {&t->prez, B * kHidden}, {&t->dprez, B * kHidden},
        {&t->pre, 3 * B * t->map}, {&t->dpre, 3 * B * t->map}, {&t->part1, (int64_t)t->splits1 * (F + 1) * kNf},
        {&t->part2, (int64_t)t->splits2 * (t->kh * kNf + 1) * kNf}, {&t->sign, 1}};
    int64_t total = 0;
    for (auto& p : parts) total += dcs_round_up(p.second, 64);
    const int64_t dbl = (int64_t)kLossBlocks * kLossSums + 8;
    hipError_t e = dcs_dev_alloc((void**)&t->state, 4 * t->P * sizeof(float), "trainer state");
    if (e == hipSuccess) e = dcs_dev_alloc((void**)&t->work, total * sizeof(float) + dbl * sizeof(double), "trainer work");
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
    // zero everything (the pad rows of V stay zero for good; grads, accu, delta_accu start at zero), then the params
    int rc = DCS_OK;
    if (hipMemsetAsync(t->work, 0, total * sizeof(float) + dbl * sizeof(double), ctx->stream) != hipSuccess ||
        hipMemsetAsync(t->state, 0, 4 * t->P * sizeof(float), ctx->stream) != hipSuccess ||
        hipMemcpyAsync(t->rnd, rand_d, RF * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
        trainer_free(t);
        DCS_FAIL(DCS_EHIP, "dcs_trainer_create: initialisation failed");
    }
    rc = layout(t, t->state, (float* const*)params_d, 1);
    if (rc != DCS_OK) {
        trainer_free(t);
        return rc;
    }
    *out = t;
    return DCS_OK;
}

DCS_API int dcs_trainer_destroy(dcs_trainer* t) {
    if (!t) return DCS_OK;
    if (t->ik) {
        const int rc = ik_trainer_destroy(t->ik);
        delete t;
        return rc;
    }
    DCS_ON_DEVICE(t->ctx->device);
    DCS_HIP(hipStreamSynchronize(t->ctx->stream));
    trainer_free(t);
    return DCS_OK;
}

DCS_API int dcs_trainer_step(dcs_trainer* t, const float* inputs_d, const float* targets_d, int mode, double* out7_d) {
    if (!t || !inputs_d || !targets_d) DCS_FAIL(DCS_EINVAL, "dcs_trainer_step: null argument");
    if (mode < 0 || mode > 2) DCS_FAIL(DCS_EINVAL, "dcs_trainer_step: mode %d (0 loss, 1 gradients, 2 update)", mode);
    if (t->ik) return ik_trainer_step(t->ik, inputs_d, targets_d, mode, out7_d);
    DCS_ON_DEVICE(t->ctx->device);
    DCS_CHECK(forward(t, inputs_d));
    DCS_CHECK(loss(t, inputs_d, targets_d, out7_d));
    if (mode == 0) return DCS_OK;
    DCS_CHECK(backward(t));
    if (mode == 1) return DCS_OK;
    hipLaunchKernelGGL(tr_adadelta_kernel, dim3((unsigned)dcs_cdiv(t->P, kThreads)), dim3(kThreads), 0, t->ctx->stream,
                       t->state, t->P, (float)t->hyp[4], (float)t->hyp[5], (float)t->hyp[6]);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

DCS_API int dcs_trainer_forward(dcs_trainer* t, const float* inputs_d, float* p_d) {
    if (!t || !inputs_d || !p_d) DCS_FAIL(DCS_EINVAL, "dcs_trainer_forward: null argument");
    if (t->ik) return ik_trainer_forward(t->ik, inputs_d, p_d);
    DCS_ON_DEVICE(t->ctx->device);
    DCS_CHECK(forward(t, inputs_d));
    const int64_t n = 4 * t->R * t->F;
    hipLaunchKernelGGL(tr_relu_kernel, dim3((unsigned)dcs_cdiv(n, kThreads)), dim3(kThreads), 0, t->ctx->stream,
                       (const float*)t->Q, p_d, n);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

DCS_API int dcs_trainer_get(dcs_trainer* t, int which, float* const* out_d, int nparams) {
    if (!t || !out_d) DCS_FAIL(DCS_EINVAL, "dcs_trainer_get: null argument");
    if (which < 0 || which > 3) DCS_FAIL(DCS_EINVAL, "dcs_trainer_get: which %d (0 params, 1 grads, 2 accu, 3 delta_accu)", which);
    if (t->ik) return ik_trainer_get(t->ik, which, out_d, nparams);
    if (nparams != kNparams) DCS_FAIL(DCS_ESHAPE, "dcs_trainer_get: %d buffers for %d parameters", nparams, kNparams);
    for (int i = 0; i < kNparams; ++i)
        if (!out_d[i]) DCS_FAIL(DCS_EINVAL, "dcs_trainer_get: buffer %d is null", i);
    DCS_ON_DEVICE(t->ctx->device);
    return layout(t, t->state + which * t->P, out_d, 0);
}

DCS_API int dcs_trainer_gather(dcs_ctx* ctx, const float* data_d, const int64_t* files_d, const int* windows_d, int batch,
                               int time_context, int F, float scale, float* inputs_d, float* targets_d) {
    if (!ctx || !data_d || !files_d || !windows_d || !inputs_d || !targets_d)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather: null argument");
    if (batch < 1 || time_context < 1 || F < 1) DCS_FAIL(DCS_EINVAL, "dcs_trainer_gather: batch %d, time_context %d, F %d",
                                                          batch, time_context, F);
    DCS_ON_DEVICE(ctx->device);
    const int64_t n = (int64_t)batch * time_context * F;
    hipLaunchKernelGGL(tr_gather_kernel, dim3((unsigned)dcs_cdiv(n, kThreads)), dim3(kThreads), 0, ctx->stream, data_d, files_d,
                       windows_d, batch, time_context, F, scale, inputs_d, targets_d);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

}  // extern "C"

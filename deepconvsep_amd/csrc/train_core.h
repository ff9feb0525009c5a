// The training core shared by the graph files (one train_<graph>.hip per network): everything a trainer needs that does
// not depend on the network.  train_core.hip owns the kernels and the dcs_trainer_* entry points; a graph file derives its
// trainer from dcs_trainer, describes its GEMMs with Gemm / Mat / Ax and supplies forward, loss, backward and layout.
//
// The GEMM is one template, train::gemm_kernel<WM, WN, FM, FN, AK, BK>: 4 waves of FM x FN v_mfma_f32_16x16x4_f32 tiles
// each, K staged through LDS 32 at a time with the next step's operands prefetched into registers.  Tiles are 128 x 32,
// 64 x 64 and 32 x 32.  Each operand loads either K-fastest or M/N-fastest, whichever is contiguous in memory.  Operands are
// addressed through Ax: index i at (i % d0) s0 + (i / d0 % d1) s1 + (i / (d0 d1)) s2 (divisions by multiply-high), which
// covers row-major, transposed, the implicit-GEMM windows of the convolutions and K-concatenations without copies.
#pragma once

#include <math.h>
#include <algorithm>
#include <string.h>

#include "dcs_internal.h"

namespace train {

constexpr int kThreads = 256;
constexpr int kKT = 32;
constexpr int kBig = 1 << 30;
constexpr int kLossBlocks = 1024;
constexpr int kMaxParams = 22;

// n / d for 0 <= n < 2^31 as (umulhi(n, m) + n) >> s (round-up magic numbers)
struct FDiv {
    uint32_t m, s;
};

// one operand axis: index i -> (i % d0) s0 + (i / d0 % d1) s1 + (i / (d0 d1)) s2; every index is below kBig
struct Ax {
    FDiv q0, q01;
    int d0, d1;
    int64_t s0, s1, s2;
};

Ax ax3(int64_t d0, int64_t d1, int64_t s0, int64_t s1, int64_t s2);
inline Ax ax2(int64_t d0, int64_t s0, int64_t s1) { return ax3(d0, kBig, s0, s1, 0); }
inline Ax ax1(int64_t s0) { return ax3(kBig, 1, s0, 0, 0); }

struct Mat {
    float* p;
    int64_t off;
    Ax r, c;
};

inline Mat mat(float* p, int64_t off, Ax r, Ax c) { return Mat{p, off, r, c}; }

enum { EPI_RELU = 1, EPI_SAVEPRE = 2, EPI_DRELU = 4 };

struct Gemm {
    Mat A, B, C, X;               // C = A . B; X: pre-activations (EPI_SAVEPRE writes, EPI_DRELU reads), C's shape
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

Gemm gemm0(int M, int N, int K);

enum Tile { T128x32, T64x64, T32x32 };

// the dense GEMMs with M = B rows: 64 x 64 tiles from 64 rows up
inline Tile rows_tile(int M) { return M >= 64 ? T64x64 : T32x32; }

// K split into slices of a multiple of kKT for a grid of about `target` workgroups, at most `cap` slices
void pick_split(int64_t tiles, int64_t K, int* splits, int* kchunk, int64_t target, int64_t cap);

// Split-K partials summed in slice order, times sign(E), into the gradient buffer; dup > 0: the last row (the bias
// gradient) is written once more right after it (BiasLayer.b gets the layer bias's gradient).
struct Reduce {
    const float* part[2];
    float* dst[2];
    int64_t count[2];
    int splits[2];
    int N[2];
    int dup[2];
    const float* scale;
};

// .pkl layout <-> internal layout, one element of the flat parameter section per thread.  to_internal: flat[i] = pkl[src];
// else pkl[src] = flat[i].
struct Layout {
    float* pkl[kMaxParams];
    int64_t off[kMaxParams + 1];
    int nparams;
    int to_internal;
};

// The end of a loss kernel: the per-thread sums of one workgroup through the halving tree into part[blockIdx.x][NS].
template <int NS>
__device__ __forceinline__ void block_sums(const double (&acc)[NS], double* part) {
    __shared__ double red[NS][kThreads];
#pragma unroll
    for (int i = 0; i < NS; ++i) red[i][threadIdx.x] = acc[i];
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w)
#pragma unroll
            for (int i = 0; i < NS; ++i) red[i][threadIdx.x] += red[i][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < NS) part[(int64_t)blockIdx.x * NS + threadIdx.x] = red[threadIdx.x][0];
}

// The workgroups' sums in fixed order -> out7 = (|E|, the graph's kOut components, zeros), sign(E) (abs'(0) = 0) for the
// gradient epilogues, and the output-bias gradient.  G: per workgroup kOut component sums then kDbo output-bias gradient
// sums, and E(s) = the loss before abs from the component sums s[0 .. kOut).
template <class G>
__global__ __launch_bounds__(kThreads) void loss_reduce_kernel(const double* __restrict__ part, int nblk, double* out7,
                                                               float* sign, float* dbo) {
    constexpr int NS = G::kOut + G::kDbo;
    __shared__ double red[NS][kThreads];
    for (int i = 0; i < NS; ++i) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblk; b += kThreads) s += part[(int64_t)b * NS + i];
        red[i][threadIdx.x] = s;
    }
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w)
            for (int i = 0; i < NS; ++i) red[i][threadIdx.x] += red[i][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double s[G::kOut];
        for (int i = 0; i < G::kOut; ++i) s[i] = red[i][0];
        const double E = G::E(s);
        const float sg = E > 0.0 ? 1.f : (E < 0.0 ? -1.f : 0.f);
        out7[0] = fabs(E);
        for (int i = 0; i < 6; ++i) out7[1 + i] = i < G::kOut ? s[i] : 0.0;
        *sign = sg;
        for (int j = 0; j < G::kDbo; ++j) dbo[j] = sg * (float)red[G::kOut + j][0];
    }
}

// conv1^T (the InverseLayer of a 1 x K1 conv1 of C1 filters, stride (1, S1)) plus the output BiasLayer, for NS sources:
// q[b][k][t][f] = bo[k] + sum over the taps S1 w + j = f of sum_c g_k[b][t][w][c] W1i[j][c], w and c ascending (one
// thread per output, fixed order).  Columns f > S1 (w1 - 1) + K1 - 1 get no tap and hold bo alone.  g_k = g + k gslot.
template <int K1, int C1, int S1, int NS>
__global__ __launch_bounds__(kThreads) void deconv1_kernel(const float* __restrict__ g, int64_t gslot,
                                                           const float* __restrict__ W1i, const float* __restrict__ bo,
                                                           float* __restrict__ q, int B, int tc, int F, int w1) {
    __shared__ float w[K1 * C1];
    for (int i = threadIdx.x; i < K1 * C1; i += kThreads) w[i] = W1i[i];
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (int64_t)B * NS * tc * F) return;
    const int f = (int)(e % F);
    int64_t r = e / F;
    const int t = (int)(r % tc);
    r /= tc;
    const int k = (int)(r % NS), b = (int)(r / NS);
    const float* gr = g + k * gslot + ((int64_t)b * tc + t) * w1 * C1;
    const int wlo = f >= K1 - 1 ? (f - (K1 - 1) + S1 - 1) / S1 : 0;
    const int whi = min(w1 - 1, f / S1);
    float acc = 0.f;
    for (int x = wlo; x <= whi; ++x) {
        const float* gw = gr + (int64_t)x * C1;
        const float* ww = w + (f - S1 * x) * C1;
#pragma unroll
        for (int c = 0; c < C1; ++c) acc += gw[c] * ww[c];
    }
    q[e] = acc + bo[k];
}

// conv1^T of a conv1 with NC input channels (W1 [C1][NC][1][K1]): one decoder slot g writes NC output channels, each through
// its own weight slab W1i[c] [K1][C1]: q[b][c][t][f] = bo[c] + sum over the taps S1 w + j = f of sum_o g[b][t][w][o]
// W1i[c][j][o], in deconv1_kernel's order (w and o ascending, one thread per output).
template <int K1, int C1, int S1, int NC>
__global__ __launch_bounds__(kThreads) void deconv1_channels_kernel(const float* __restrict__ g, const float* __restrict__ W1i,
                                                                    const float* __restrict__ bo, float* __restrict__ q, int B,
                                                                    int tc, int F, int w1) {
    __shared__ float w[NC * K1 * C1];
    for (int i = threadIdx.x; i < NC * K1 * C1; i += kThreads) w[i] = W1i[i];
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (int64_t)B * NC * tc * F) return;
    const int f = (int)(e % F);
    int64_t r = e / F;
    const int t = (int)(r % tc);
    r /= tc;
    const int c = (int)(r % NC), b = (int)(r / NC);
    const float* gr = g + ((int64_t)b * tc + t) * w1 * C1;
    const int wlo = f >= K1 - 1 ? (f - (K1 - 1) + S1 - 1) / S1 : 0;
    const int whi = min(w1 - 1, f / S1);
    float acc = 0.f;
    for (int x = wlo; x <= whi; ++x) {
        const float* gw = gr + (int64_t)x * C1;
        const float* ww = w + (c * K1 + f - S1 * x) * C1;
#pragma unroll
        for (int o = 0; o < C1; ++o) acc += gw[o] * ww[o];
    }
    q[e] = acc + bo[c];
}

// map(s, k): the .pkl index of element k of the internal section s
template <class Map>
__global__ __launch_bounds__(kThreads) void layout_kernel(float* __restrict__ flat, const Layout L, const Map map) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= L.off[L.nparams]) return;
    int s = 0;
    while (i >= L.off[s + 1]) ++s;
    const int64_t src = map(s, i - L.off[s]);
    if (L.to_internal) flat[i] = L.pkl[s][src];
    else L.pkl[s][src] = flat[i];
}

}  // namespace train

// One trainer: the state every graph has, and the four things only its graph knows.
struct dcs_trainer {
    dcs_ctx* ctx = nullptr;
    int tc = 0, F = 0, B = 0;
    int nsrc = 0;                // output channels: Q and the targets are [B][nsrc][tc][F]
    int nparams = 0, loss_sums = 0;
    int nstate = 0;              // sections of the stepped state; 0: nparams.  Fewer than nparams: the graph holds parameters
                                 // that no gradient reaches outside the state (its layout() serves them), sizes in state_size
    int64_t state_size[train::kMaxParams] = {0};
    int nout = 7;                // doubles dcs_trainer_step writes
    int rand_planes = 1;         // the draw is [rand_planes][B][tc][F]
    bool two_stage = false;      // the graph has a second loss (mode + 4 of dcs_trainer_step)
    int stage2 = 0;              // set by dcs_trainer_step before loss()
    int64_t RF = 0, P = 0, P4 = 0;
    int64_t shapes[train::kMaxParams][4] = {{0}};   // .pkl shapes
    double hyp[7] = {0};
    int opt_kind = 0;            // the update of mode 2: 0 Adadelta (lr, rho, epsilon), 1 Adam (lr, beta1, beta2, epsilon)
    double opt[4] = {0};         // its hyper-parameters; at create hyp[4 .. 6]
    int64_t steps = 0;           // updates since the optimiser was set (Adam's t - 1), host side
    int64_t off[train::kMaxParams + 1] = {0};
    float* state = nullptr;      // [4][4 P4]: params, grads, accu, delta_accu (Adam: m, v); sections padded to four floats,
                                 // pad zero
    float* work = nullptr;
    double* lpart = nullptr;     // [kLossBlocks][loss_sums]
    double* out7 = nullptr;      // when the caller passes none
    float *rnd = nullptr, *Q = nullptr, *sign = nullptr;   // views into work: the draw, the output layer's
                                                           // pre-activations, sign(E)

    virtual ~dcs_trainer() {}
    // the split choices, then the graph's views into work (Q among them) as (pointer, floats)
    virtual void plan(std::vector<std::pair<float**, int64_t>>& parts) = 0;
    virtual int forward(const float* x) = 0;
    virtual int loss(const float* x, const float* tgt, double* out7) = 0;
    virtual int backward() = 0;
    // flat: one of the four slots of state.  A graph that holds parameters outside the state reads and writes them for slot 0
    // alone: for the other slots they are zeros on the way out and ignored on the way in.
    virtual int layout(float* flat, float* const* pkl, int to_internal) = 0;
    // dcs_trainer_rectify_codes: the graphs that keep their rectifier codes copy them out
    virtual int codes(float* const* out_d, int n);

    float* param(int i) { return state + off[i]; }
    float* grad() { return state + 4 * P4; }
    // grid (nullable): the grid of the launch
    int launch(train::Gemm g, train::Tile tile, bool ak, bool bk, dim3* grid_out = nullptr);
    // the slices of a split-K GEMM with M = B rows summed in slice order, then the epilogue: C[m][n] (row-major, ld N) =
    // sum + bias[n], EPI_SAVEPRE -> X, EPI_DRELU * r'(X), EPI_RELU
    int finish(const float* part, int splits, int N, const float* bias, float* C, float* X, int epi);
    int reduce(const train::Reduce& r);
    template <class Map>
    int run_layout(float* flat, float* const* pkl, int to_internal, const Map& map);
    template <class G>
    int loss_reduce(int nblk, double* out7_d, float* dbo);
};

template <class Map>
int dcs_trainer::run_layout(float* flat, float* const* pkl, int to_internal, const Map& map) {
    train::Layout L;
    for (int i = 0; i < nstate; ++i) {
        L.pkl[i] = pkl[i];
        L.off[i] = off[i];
    }
    L.off[nstate] = off[nstate];
    L.nparams = nstate;
    L.to_internal = to_internal;
    hipLaunchKernelGGL(train::layout_kernel<Map>, dim3((unsigned)dcs_cdiv(P, train::kThreads)), dim3(train::kThreads), 0,
                       ctx->stream, flat, L, map);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

template <class G>
int dcs_trainer::loss_reduce(int nblk, double* out7_d, float* dbo) {
    hipLaunchKernelGGL(train::loss_reduce_kernel<G>, dim3(1), dim3(train::kThreads), 0, ctx->stream, (const double*)lpart,
                       nblk, out7_d ? out7_d : out7, sign, dbo);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

// The reference's build_ca graph with a 1 x 30 conv1, shared by the graph files that train a form of it (train_ikala.hip,
// train_bach10.hip, train_bach10si.hip): conv1 30 x (1 x 30) over NCH input channels, stride (1, S1), + BiasLayer; conv2
// 30 x (kh x kw) + BiasLayer; dense 256; NB decoder branches of one rectified dense layer of flat = 30 h2 w2 units, the
// InverseLayer of conv2 and the InverseLayer of conv1; the output BiasLayer and rectify.  A graph file is a description
// (CaDesc), its loss and its conv1^T launch; train_ca.hip owns the dimensions, the work buffer, every GEMM of the step and
// the .pkl layout.
//
// One step on the ctx stream, no host synchronisation and no float atomics (two runs give bit-identical weights):
//
//   forward   F1 a1b = conv1(x) + b1 + b1b             gemm 128x32  x [B][NCH][tc][F] read in place, K = (channel, tap) = NCH x 30
//             F2 a2b = conv2(a1b) + b2 + b2b           gemm 128x32  implicit GEMM, K = (dh, dw c) = kh x 30 kw
//             F3 z = rectify(a2b . Wfc + bfc)          gemm 32x32 split-K over flat, finish (saved: z, pre-activation)
//             F4 d_k = rectify(z . W_k + b_k), k < NB  gemm, NB batches, into the zero-padded V (saved: pre-activations)
//             F5 g_k = conv2^T(d_k)                    gemm 128x32  implicit GEMM over V (kh - 1 / kw - 1 zero rows / columns)
//             F6 q = conv1^T(g_k) + bo                 the graph's train::deconv1_*_kernel, fixed order
//   loss      the graph's kernel: dE/dq (rectify' with the 0.5 tie) into xy, per-workgroup f64 sums
//             train::loss_reduce_kernel: fixed-order sum -> loss and components (f64), sign(E), the output-bias gradient
//   backward  B1 dg_k = conv1(dY_k)    B2 dpre_k = conv2(dg_k) * r'(pre_k)    B3 dprez = (sum_k dpre_k . W_k^T) * r'(prez)
//             B4 da2 = dprez . Wfc^T   B5 da1 = conv2^T(da2)
//   weights   dW1|db1 = [x; dY_k] windows^T . [da1; g_k]            split-K (K = (NB + 1) B tc w1), fixed-order reduce
//             dW2|db2 = [a1b; dg_k] windows^T . [da2; d_k]          split-K (K = (NB + 1) B h2 w2), fixed-order reduce
//             dWfc|dbfc = a2b^T . dprez,  dW_k|db_k = z^T . dpre_k
//             every bias gradient is the "ones" row of its weight GEMM; b1b / b2b get copies of b1 / b2 (identical in Theano)
//   update    train::adadelta_kernel over the flat [params | grads | accu | delta_accu] buffer, four floats per thread
//
// The GEMMs are forms of the shared template (train_core.h): 128 x 32 tiles for every conv2-family GEMM (N = 30 channels),
// 64 x 64 and 32 x 32 for the dense ones, each operand loaded K-fastest or M/N-fastest, whichever is contiguous in memory.
// The operands' Ax addressing covers the implicit-GEMM windows of conv1 and conv2 and the K-concatenations above without
// copies.
//
// Internal parameter layouts (the flat buffer; dcs_trainer_get / _create convert to and from the .pkl layout, CaMap):
//   W1 [(ch, j)][30 c]: W1i[ch][j][c] = W1[c,ch,0,29-j]   W2 [kh dh][kw dw][30 c][30 o]: W2i = W2[o,c,kh-1-dh,kw-1-dw] (flips)
//   Wfc [(h,w,o)][256] and W_k [256][(h,w,o)], b_k [(h,w,o)]: the 30 x h2 x w2 map channels-last, .pkl order
//   o h2 w2 + h w2 + w
// Sections: 0 .. 2 W1, b1, b1b; 3 .. 5 W2, b2, b2b; 6, 7 Wfc, bfc; 8 + 2 k, 9 + 2 k W_k, b_k; 8 + 2 NB the output bias.
// Activations are channels-last: a1b / dg / g / da1 [B][tc][w1][30], a2b / d_k / dpre [B][h2][w2][30].  xy holds [x; dY_k],
// U [a1b; dg_k], GA [da1; g_k], V [da2; d_k] (1 + NB slots each); a V image is [h2 + 2 (kh - 1)][w2 + 2 (kw - 1)][30], zero
// rows and columns around the map, so that conv2^T is a plain implicit GEMM.
#pragma once

#include <memory>

#include "train_core.h"

namespace train {

constexpr int kC1 = 30, kK1 = 30;   // conv1: 30 filters of 1 x 30
constexpr int kC2 = 30;             // conv2: 30 filters of kh x kw
constexpr int kHidden = 256;        // the dense layer; a constant, so that the layout map divides by it at compile time

struct CaDesc {
    int S1, NCH;                    // conv1: stride (1, S1), input channels
    int kh, kw;                     // conv2
    int NB;                         // decoder branches; the output bias is section 8 + 2 NB (CaTrainer::bo)
    int64_t split1[2], split2[2];   // pick_split's target and cap for dW1 and dW2
};

// the .pkl index of element k of the internal section s
struct CaMap {
    int kh, kw, h2, w2, NCH, NB;
    __device__ int64_t operator()(int s, int64_t k) const {
        const int64_t hw = (int64_t)h2 * w2, map = kC2 * hw;
        // map position (h, w, o) channels-last -> .pkl o h2 w2 + h w2 + w
        auto pkl_of = [&](int64_t col) {
            const int64_t o = col % kC2, hwi = col / kC2;
            return o * hw + hwi;
        };
        if (s == 0) {                                     // W1i[ch][j][c] = W1[c][ch][29-j]
            const int64_t c = k % kC1, chj = k / kC1, ch = chj / kK1, j = chj % kK1;
            return (c * NCH + ch) * kK1 + (kK1 - 1 - j);
        } else if (s == 3) {                              // W2i[dh][dw][c][o] = W2[o][c][kh-1-dh][kw-1-dw]
            const int64_t dh = k / (kw * kC1 * kC2), dw = (k / (kC1 * kC2)) % kw, c = (k / kC2) % kC1, o = k % kC2;
            return ((o * kC1 + c) * kh + (kh - 1 - dh)) * kw + (kw - 1 - dw);
        } else if (s == 6) {                              // Wfc rows (h, w, o)
            return pkl_of(k / kHidden) * kHidden + k % kHidden;
        } else if (s >= 8 && s < 8 + 2 * NB) {            // W_k columns (h, w, o), b_k
            return s % 2 == 0 ? (k / map) * map + pkl_of(k % map) : pkl_of(k);
        }
        return k;
    }
};

// The loss of the Bach10 graphs (four sources from one mixture of NCH input channels).
struct MaskLoss {
    const float* q;       // [B][4][tc F] pre-activations of the output layer
    const float* x;       // [B][NCH][tc F] inputs
    const float* tgt;     // [B][4][tc F] targets
    const float* rnd;     // [B][tc F] the uniform draw
    float* xy;            // slot 0 <- x, [B][NCH][tc F]; then dE/dq in the graph's slots (below)
    double* part;         // [gridDim.x][2 kMaskSrc]
    int64_t plane, n;     // tc F, B tc F
    double eps;
};
constexpr int kMaskSrc = 4;

// trainCNNbach10.py:173-198 (trainCNNrwc.py:248-275 of the score-informed example) per element, in f64: x = the input
// channels summed left to right, D = p_1 + .. + p_4 + eps r, m_k = p_k / D, source_k = m_k x; the four squared-error sums;
// dE/dp_k = x / D (G_k - sum_j m_j G_j) with G_k = 2 (source_k - target_k); dE/dq = dE/dp r'(q), r'(0) = 0.5.  D = 0 (all
// four outputs zero, r = 0) gives NaN, as the reference's 0 / 0 does.  Four error sums, then four output-bias gradient sums.
// dE/dq_j goes where B1 reads dY: NCH = 1 is the graph with a decoder branch per source, xy [5][B tc F], slot 1 + j; NCH = 4
// the graph with one branch whose four channels are the sources, xy [2][B][4][tc F], channel j of slot 1.
template <int NCH>
__global__ __launch_bounds__(kThreads) void mask_loss_kernel(const MaskLoss a) {
    static_assert(NCH == 1 || NCH == kMaskSrc, "a branch per source, or a channel per source");
    double acc[2 * kMaskSrc];
#pragma unroll
    for (int i = 0; i < 2 * kMaskSrc; ++i) acc[i] = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < a.n; e += (int64_t)gridDim.x * kThreads) {
        const int64_t b = e / a.plane, rem = e - b * a.plane;
        const int64_t o = b * kMaskSrc * a.plane + rem, ox = b * NCH * a.plane + rem;
        float xc[NCH];
#pragma unroll
        for (int c = 0; c < NCH; ++c) xc[c] = a.x[ox + c * a.plane];
        double x = xc[0];
#pragma unroll
        for (int c = 1; c < NCH; ++c) x += (double)xc[c];
        double q[kMaskSrc], m[kMaskSrc], G[kMaskSrc];
        double D = 0.0;
#pragma unroll
        for (int j = 0; j < kMaskSrc; ++j) {
            q[j] = a.q[o + j * a.plane];
            m[j] = q[j] > 0.0 ? q[j] : 0.0;
            D += m[j];
        }
        D += a.eps * (double)a.rnd[e];
        double mg = 0.0;
#pragma unroll
        for (int j = 0; j < kMaskSrc; ++j) {
            m[j] /= D;
            const double err = m[j] * x - (double)a.tgt[o + j * a.plane];
            acc[j] += err * err;
            G[j] = 2.0 * err;
            mg += m[j] * G[j];
        }
#pragma unroll
        for (int j = 0; j < kMaskSrc; ++j) {
            const double rd = q[j] > 0.0 ? 1.0 : (q[j] == 0.0 ? 0.5 : 0.0);
            const double dq = x / D * (G[j] - mg) * rd;
            acc[kMaskSrc + j] += dq;
            a.xy[NCH == 1 ? (j + 1) * a.n + e : NCH * a.n + o + j * a.plane] = (float)dq;
        }
#pragma unroll
        for (int c = 0; c < NCH; ++c) a.xy[ox + c * a.plane] = xc[c];
    }
    block_sums(acc, a.part);
}

// F6 of the three graph files, each the one launch site of its conv1^T instance: the trainer's deconv1() calls it, and so
// does dcs_debug_train_aux (train_debug.hip).  g: the first source's slot, source k at + k gslot; q [B][sources][tc][F].
int ikala_deconv1(hipStream_t s, const float* g, int64_t gslot, const float* W1i, const float* bo, float* q, int B, int tc,
                  int F, int w1);
int bach10_deconv1(hipStream_t s, const float* g, int64_t gslot, const float* W1i, const float* bo, float* q, int B, int tc,
                   int F, int w1);
int bach10si_deconv1(hipStream_t s, const float* g, const float* W1i, const float* bo, float* q, int B, int tc, int F, int w1);

struct CaTrainer : dcs_trainer {
    CaDesc d;
    int w1 = 0, h2 = 0, w2 = 0, hp = 0, wp = 0, K2 = 0;
    int64_t R1 = 0, Rh = 0, flat = 0;
    int64_t Uslot = 0, Vslot = 0, padoff = 0;   // one slot of U / GA and of V; the map's first element in a V image
    // views into work
    float *xy, *U, *GA, *V, *a2b, *z, *prez, *dprez, *pre, *dpre, *part1, *part2, *partS;
    int splits1 = 1, splits2 = 1, splits3 = 1, splitsB3 = 1, kchunk1 = 0, kchunk2 = 0, kchunk3 = 0, kchunkB3 = 0;

    // the dimensions, nparams and the .pkl shapes (nbo output-bias values) for the arguments the graph file has checked
    void shape(const CaDesc& desc, int time_context, int F, int batch, int nbo);
    // every GEMM index (a row, a column or a K position, Ax) stays below kBig, for nb branches
    int check_index(const char* graph, int nb) const;
    int bo() const { return 8 + 2 * d.NB; }   // the section of the output bias
    // F6: q = conv1^T(g_k) + bo from GA slots 1 .. NB
    virtual int deconv1() = 0;

    void plan(std::vector<std::pair<float**, int64_t>>& parts) override;
    int forward(const float* x) override;
    int backward() override;
    int layout(float* flat_d, float* const* pkl, int to_internal) override;
};

}  // namespace train

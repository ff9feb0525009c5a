// The reference's build_ca graph with a full-width conv1, shared by the two graph files that train a form of it
// (train_dsd.hip, train_dsdild.hip): conv1 50 x (1 x F) over NCH input channels + BiasLayer; conv2 50 x (tc/2 x 1) +
// BiasLayer; one rectified dense layer of `hidden` units; NB decoder branches of one rectified dense layer of map = 50 h2
// units, the InverseLayer of conv2 and the InverseLayer of conv1; the output BiasLayer and rectify.  A graph file is a
// description (DsdDesc) and its loss; train_dsd_graph.hip owns the dimensions, the work buffer, every GEMM of the step and
// the .pkl layout.  (The build_ca graphs with a 1 x 30 conv1 are train_ca.h's: a strided conv1, a flipped W2 and other
// tiles.)
//
// One step on the ctx stream, no host synchronisation and no float atomics (two runs give bit-identical weights):
//
//   forward   F1 a1b = x . W1 + b1 + b1b                 K = (c, f) = NCH F over x [B][NCH][tc][F] in place (saved: a1b)
//             F2 a2b = conv2(a1b) + b2 + b2b             implicit GEMM over the tc/2 taps (saved: a2b)
//             F3 z = rectify(a2b . Wfc + bfc)            one launch with the epilogue, or split-K over the map and finish
//                                                        (DsdDesc::split_dense) (saved: z and its pre-activation)
//             F4 d_k = rectify(z . W_k + b_k), k < NB    NB batches, into the row-padded V (saved: pre-activations)
//             F5 g_k = conv2^T(d_k)                      NB batches, implicit GEMM over V (InverseLayer of conv2)
//             F6 q[NCH i + c] = conv1^T(g_branch[i])[c] + bo   one launch per input channel c, four batches i
//   loss      the graph's kernels: dE/dq (rectify' with the 0.5 tie) into xy, the loss, sign(E), the output-bias gradient
//   backward  B1 dg_k = dY_k . W1       B2 dpre_k = conv2(dg_k) * r'(pre_k)     B3 dprez = (sum_k dpre_k . W_k^T) * r'(prez)
//             B4 da2 = dprez . Wfc^T    B5 da1 = conv2^T(da2)
//   weights   dW1|db1 = [x; dY_k]^T . [da1; g_k]               split-K (K = (NB + 1) B tc), fixed-order reduce
//             dW2|db2 = windows of [a1b; dg_k]^T . [da2; d_k]   split-K (K = (NB + 1) B h2), fixed-order reduce
//             dWfc|dbfc = a2b^T . dprez,  dW_k|db_k = z^T . dpre_k
//             every bias gradient is the "ones" row of its weight GEMM; b1b / b2b get copies of b1 / b2 (identical in Theano)
//   update    train::adadelta_kernel over the flat [params | grads | accu | delta_accu] buffer
//
// Every GEMM is a form of the shared template (train_core.h); its tile and load directions are the graph's (DsdDesc::form).
// The operands' Ax addressing covers row-major, transposed, the input channels of x, the implicit-GEMM windows of conv2 and
// the K-concatenations above without copies.
//
// Internal parameter layouts (the flat buffer; dcs_trainer_get / _create convert to and from the .pkl layout, DsdMap):
//   W1 [(c,f)][50]: W1i[c F + f][o] = W1[o,c,0,F-1-f]  (flip_filters=True)    W2 [kh][50 c][50 o]: W2i[j][c][o] = W2[o,c,j,0]
//   Wfc [(h,o)][hidden] and W_k [hidden][(h,o)], b_k [(h,o)]: the 50 x h2 map in (row h, channel o) order, .pkl order is
//   o h2 + h
// Sections: 0 .. 2 W1, b1, b1b; 3 .. 5 W2, b2, b2b; 6, 7 Wfc, bfc; 8 + 2 k, 9 + 2 k W_k, b_k; 8 + 2 NB the output bias.
// Activations are channels-last: a1b / dg / g / da1 [B][tc][50], a2b / d_k [B][h2][50].  xy holds [x; dY_k], U [a1b; dg_k],
// GA [da1; g_k], V [da2; d_k] (1 + NB slots each); a V image is padded by kh - 1 zero rows on either side so that conv2^T is
// a plain implicit GEMM.
#pragma once

#include "train_core.h"

namespace train {

constexpr int kNf = 50;             // filters of conv1 and of conv2

// the GEMMs of one step, in launch order
enum DsdGemm { G_F1, G_F2, G_F3, G_F4, G_F5, G_F6, G_B1, G_B2, G_B3, G_B4, G_B5, G_DW1, G_DW2, G_DWFC, G_DWK, kDsdGemms };

struct DsdForm {
    Tile tile;
    bool ak, bk;                    // A loaded K-fastest (else M-fastest), B loaded K-fastest (else N-fastest)
};

struct DsdDesc {
    int NCH;                        // input channels
    int NB;                         // decoder branches; the output bias is section 8 + 2 NB (DsdGraphTrainer::bo)
    int hidden;                     // the dense layer
    int nsrc, nbo;                  // output channels of Q, values of the output bias
    int branch[4];                  // F6: the branch batch i reads; it writes channel NCH i + c
    bool split_dense;               // F3 / B3: 32 x 32 split-K (target 512, cap 128) and finish; else one launch with the epilogue
    DsdForm form[kDsdGemms];
};

// the .pkl index of element k of the internal section s
struct DsdMap {
    int F, kh, h2, NCH, NB, hidden;
    __device__ int64_t operator()(int s, int64_t k) const {
        const int64_t map = kNf * (int64_t)h2;
        if (s == 0) {                                     // W1i[c F + f][o] = W1[o][c][F-1-f]
            const int64_t row = k / kNf, o = k % kNf;
            const int64_t c = row / F, f = row % F;
            return (o * NCH + c) * F + (F - 1 - f);
        } else if (s == 3) {                              // W2i[j][c][o] = W2[o][c][j]
            const int64_t j = k / (kNf * kNf), c = (k / kNf) % kNf, o = k % kNf;
            return (o * kNf + c) * kh + j;
        } else if (s == 6) {                              // Wfc rows (h, o) <- o h2 + h
            const int64_t row = k / hidden, n = k % hidden;
            return ((row % kNf) * h2 + row / kNf) * hidden + n;
        } else if (s >= 8 && s < 8 + 2 * NB && s % 2 == 0) {   // W_k columns (h, o) <- o h2 + h
            const int64_t n = k / map, col = k % map;
            return n * map + (col % kNf) * h2 + col / kNf;
        } else if (s >= 9 && s < 8 + 2 * NB) {            // b_k
            return (k % kNf) * h2 + k / kNf;
        }
        return k;
    }
};

struct DsdGraphTrainer : dcs_trainer {
    DsdDesc d;
    int kh = 0, h2 = 0, hp = 0;
    int64_t R = 0, Rh = 0, map = 0;
    // views into work (partS: split_dense only)
    float *xy, *U, *GA, *V, *a2b, *z, *prez, *dprez, *pre, *dpre, *part1, *part2, *partS = nullptr;
    int splits1 = 1, splits2 = 1, splits3 = 1, splitsB3 = 1, kchunk1 = 0, kchunk2 = 0, kchunk3 = 0, kchunkB3 = 0;

    // the argument ranges both graphs share; `graph` goes into the message after "dcs_trainer_create: "
    static int check_range(const char* graph, int time_context, int F, int batch);
    // the dimensions, nsrc, nparams and the .pkl shapes for arguments that passed check_range
    void shape(const DsdDesc& desc, int time_context, int F, int batch);
    int bo() const { return 8 + 2 * d.NB; }   // the section of the output bias
    int launch(const Gemm& g, DsdGemm i) { return dcs_trainer::launch(g, d.form[i].tile, d.form[i].ak, d.form[i].bk); }

    void plan(std::vector<std::pair<float**, int64_t>>& parts) override;
    int forward(const float* x) override;
    int backward() override;
    int layout(float* flat, float* const* pkl, int to_internal) override;
};

}  // namespace train

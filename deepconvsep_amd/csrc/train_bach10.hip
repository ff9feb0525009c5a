// Training of the Bach10 graph (examples/bach10/trainCNNbach10.py: build_ca :66-123, loss :160-198, adadelta :202; the same
// graph and loss as trainCNNrwc.py and trainCNNSibelius.py, which differ only in their features) on gfx950.  conv1 30 x
// (1 x 30) stride (1, 4) + BiasLayer, conv2 30 x (kh x 1) with kh = int(2 tc / 3) + BiasLayer, dense 256, four rectified
// dense layers of flat = 30 h2 w1 units, per source the InverseLayers of conv2 and conv1, BiasLayer(4) and rectify.
//
// One step on the ctx stream, no host synchronisation and no float atomics (two runs give bit-identical weights):
//
//   forward   F1 a1b = conv1(x) + b1 + b1b             gemm 128x32  K = 30 taps (saved: a1b)
//             F2 a2b = conv2(a1b) + b2 + b2b           gemm 128x32  implicit GEMM, K = (dh, c) = kh x 30
//             F3 z = rectify(a2b . Wfc + bfc)          gemm 32x32 split-K over flat, finish (saved: z, pre-activation)
//             F4 d_k = rectify(z . W_k + b_k), k < 4   gemm, 4 batches, into the row-padded V (saved: pre-activations)
//             F5 g_k = conv2^T(d_k)                    gemm 128x32  implicit GEMM over V (kh - 1 zero rows either side)
//             F6 q = conv1^T(g_k) + bo                 train::deconv1_kernel: 8 taps x 30 channels per output, fixed order
//   loss      b10_loss_kernel: masks, the four errors, dE/dq (rectify' with the 0.5 tie), per-workgroup f64 sums
//             train::loss_reduce_kernel: fixed-order sum -> loss and errors (f64), sign(E), the output-bias gradient
//   backward  B1 dg_k = conv1(dY_k)    B2 dpre_k = conv2(dg_k) * r'(pre_k)    B3 dprez = (sum_k dpre_k . W_k^T) * r'(prez)
//             B4 da2 = dprez . Wfc^T   B5 da1 = conv2^T(da2)
//   weights   dW1|db1 = [x; dY_k] windows^T . [da1; g_k]            split-K (K = 5 B tc w1), fixed-order reduce
//             dW2|db2 = [a1b; dg_k] windows^T . [da2; d_k]          split-K (K = 5 B h2 w1), fixed-order reduce
//             dWfc|dbfc = a2b^T . dprez,  dW_k|db_k = z^T . dpre_k
//             every bias gradient is the "ones" row of its weight GEMM; b1b / b2b get copies of b1 / b2 (identical in Theano)
//   update    train::adadelta_kernel over the flat [params | grads | accu | delta_accu] buffer, four floats per thread
//
// The GEMMs are forms of the shared template (train_core.h), with the tiles the iKala graph uses: 128 x 32 for every
// conv2-family GEMM (N = 30 channels), 64 x 64 and 32 x 32 for the dense ones.
//
// The loss divides by D = p1 + p2 + p3 + p4 + eps r (eps r in the denominator only, trainCNNbach10.py:178-181).  Where the
// four outputs are all zero and r = 0 the reference divides 0 by 0; so does this kernel: the NaN is kept, there is no guard.
//
// Internal parameter layouts (the flat buffer; dcs_trainer_get / _create convert to and from the .pkl layout):
//   W1 [30 j][30 c]: W1i[j][c] = W1[c,0,0,29-j]           W2 [kh dh][30 c][30 o]: W2i = W2[o,c,kh-1-dh,0] (flips)
//   Wfc [(h,w,o)][256] and W_k [256][(h,w,o)], b_k [(h,w,o)]: the 30 x h2 x w1 map channels-last, .pkl order o h2 w1 + h w1 + w
// Activations are channels-last: a1b / dg / g / da1 [B][tc][w1][30], a2b / d_k / dpre [B][h2][w1][30]; d_k and da2 live in
// V [B][h2 + 2 (kh - 1)][w1][30], zero rows above and below them, so that conv2^T is a plain implicit GEMM.
#include "train_core.h"

using namespace train;

namespace {

constexpr int kC1 = 30, kK1 = 30, kS1 = 4;       // conv1: 30 filters of 1 x 30, stride (1, 4)
constexpr int kC2 = 30;                          // conv2: 30 filters of kh x 1
constexpr int kTap = kC1 * kC2;                  // 900: one tap of W2i
constexpr int kHidden = 256, kNparams = 17, kSrc = 4;
constexpr int kMaxTc = 47;                       // the largest time context dcs_model_create's bach10 graph runs

// four errors, then four output-bias gradient sums; E = error1 + error2 + error3 + error4 (trainCNNbach10.py:198);
// out7 = (|E|, error1, error2, error3, error4, 0, 0)
struct Bach10Sums {
    static constexpr int kOut = 4, kDbo = 4;
    static __device__ double E(const double* s) { return s[0] + s[1] + s[2] + s[3]; }
};
constexpr int kLossSums = Bach10Sums::kOut + Bach10Sums::kDbo;

struct BLoss {
    const float* q;       // [B][4][tc F] pre-activations of the output layer
    const float* x;       // [B][tc F] inputs
    const float* tgt;     // [B][4][tc F] targets
    const float* rnd;     // [B][tc F] the uniform draw
    float* xy;            // [5][B tc F]: slot 0 <- x, slots 1 .. 4 <- dE/dq_k
    double* part;         // [gridDim.x][kLossSums]
    int64_t plane, n;     // tc F, B tc F
    double eps;
};

// trainCNNbach10.py:173-198 per element, in f64: D = p_1 + .. + p_4 + eps r, m_k = p_k / D, source_k = m_k x; the four
// squared-error sums; dE/dp_k = x / D (G_k - sum_j m_j G_j) with G_k = 2 (source_k - target_k); dE/dq = dE/dp r'(q),
// r'(0) = 0.5.  D = 0 (all four outputs zero, r = 0) gives NaN, as the reference's 0 / 0 does.
__global__ __launch_bounds__(kThreads) void b10_loss_kernel(const BLoss a) {
    double acc[kLossSums];
#pragma unroll
    for (int i = 0; i < kLossSums; ++i) acc[i] = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < a.n; e += (int64_t)gridDim.x * kThreads) {
        const int64_t b = e / a.plane, rem = e - b * a.plane;
        const int64_t o = b * kSrc * a.plane + rem;
        const double x = a.x[e];
        double q[kSrc], m[kSrc], G[kSrc];
        double D = 0.0;
#pragma unroll
        for (int j = 0; j < kSrc; ++j) {
            q[j] = a.q[o + j * a.plane];
            m[j] = q[j] > 0.0 ? q[j] : 0.0;
            D += m[j];
        }
        D += a.eps * (double)a.rnd[e];
        double mg = 0.0;
#pragma unroll
        for (int j = 0; j < kSrc; ++j) {
            m[j] /= D;
            const double err = m[j] * x - (double)a.tgt[o + j * a.plane];
            acc[j] += err * err;
            G[j] = 2.0 * err;
            mg += m[j] * G[j];
        }
#pragma unroll
        for (int j = 0; j < kSrc; ++j) {
            const double rd = q[j] > 0.0 ? 1.0 : (q[j] == 0.0 ? 0.5 : 0.0);
            const double dq = x / D * (G[j] - mg) * rd;
            acc[kSrc + j] += dq;
            a.xy[(j + 1) * a.n + e] = (float)dq;
        }
        a.xy[e] = (float)x;
    }
    block_sums(acc, a.part);
}

// the .pkl index of element k of the internal section s
struct Bach10Map {
    int kh, h2, w1;
    __device__ int64_t operator()(int s, int64_t k) const {
        const int64_t hw = (int64_t)h2 * w1, map = kC2 * hw;
        // map position (h, w, o) channels-last -> .pkl o h2 w1 + h w1 + w
        auto pkl_of = [&](int64_t col) {
            const int64_t o = col % kC2, hwi = col / kC2;
            return o * hw + hwi;
        };
        if (s == 0) {                                     // W1i[j][c] = W1[c][29-j]
            const int64_t j = k / kC1, c = k % kC1;
            return c * kK1 + (kK1 - 1 - j);
        } else if (s == 3) {                              // W2i[dh][c][o] = W2[o][c][kh-1-dh]
            const int64_t dh = k / kTap, c = (k / kC2) % kC1, o = k % kC2;
            return (o * kC1 + c) * kh + (kh - 1 - dh);
        } else if (s == 6) {                              // Wfc rows (h, w, o)
            return pkl_of(k / kHidden) * kHidden + k % kHidden;
        } else if (s >= 8 && s < 16 && s % 2 == 0) {      // W_k columns (h, w, o)
            return (k / map) * map + pkl_of(k % map);
        } else if (s >= 9 && s < 16) {                    // b_k
            return pkl_of(k);
        }
        return k;
    }
};

// the dense GEMMs with M = B rows: 64 x 64 tiles from 64 rows up
Tile rows_tile(int M) { return M >= 64 ? T64x64 : T32x32; }

struct Bach10Trainer : dcs_trainer {
    int kh = 0, w1 = 0, h2 = 0, hp = 0, K2 = 0;
    int64_t R1 = 0, Rh = 0, flat = 0;
    // views into work
    float *xy, *U, *GA, *V, *a2b, *z, *prez, *dprez, *pre, *dpre, *part1, *part2, *partS;
    int splits1 = 1, splits2 = 1, splits3 = 1, splitsB3 = 1, kchunk1 = 0, kchunk2 = 0, kchunk3 = 0, kchunkB3 = 0;

    void plan(std::vector<std::pair<float**, int64_t>>& parts) override {
        // dW1 is one 32 x 32 tile and dW2 five 128 x 32 tiles (tc 30) over a K of millions (5 B tc w1 = 2.4 M and 5 B h2 w1 =
        // 0.9 M at B = 32, F = 2049): up to 512 slices, about 2 and 8 workgroups per CU.  F3 / B3: the iKala graph's choices
        pick_split(dcs_cdiv(kK1 + 1, 32), (kSrc + 1) * R1, &splits1, &kchunk1, 512, 512);
        pick_split(dcs_cdiv(K2 + 1, 128), (kSrc + 1) * Rh, &splits2, &kchunk2, 2048, 512);
        pick_split((int64_t)dcs_cdiv(B, 32) * (kHidden / 32), flat, &splits3, &kchunk3, 512, 128);
        pick_split((int64_t)dcs_cdiv(B, 32) * (kHidden / 32), kSrc * flat, &splitsB3, &kchunkB3, 512, 128);
        const int64_t b = B, n5 = kSrc + 1;
        parts.insert(parts.end(), {{&xy, n5 * RF}, {&U, n5 * R1 * kC1}, {&GA, n5 * R1 * kC1}, {&V, n5 * b * hp * w1 * kC2},
                                   {&Q, kSrc * RF}, {&a2b, b * flat}, {&z, b * kHidden}, {&prez, b * kHidden},
                                   {&dprez, b * kHidden}, {&pre, kSrc * b * flat}, {&dpre, kSrc * b * flat},
                                   {&part1, (int64_t)splits1 * (kK1 + 1) * kC1},
                                   {&part2, (int64_t)splits2 * (K2 + 1) * kC2},
                                   {&partS, (int64_t)std::max(splits3, splitsB3) * b * kHidden}});
    }

    int forward(const float* x) override {
        const int64_t row1 = (int64_t)w1 * kC1, img1 = (int64_t)tc * row1, imgp = (int64_t)hp * row1;
        const int64_t padoff = (int64_t)(kh - 1) * row1, Vslot = (int64_t)B * imgp, Uslot = R1 * kC1;
        const int64_t wstep = off[10] - off[8];
        // F1: a1b[(b,t,w)][c] = sum_j x[b][t][4 w + j] W1i[j][c] + b1 + b1b -> U slot 0
        {
            Gemm g = gemm0((int)R1, kC1, kK1);
            g.A = mat((float*)x, 0, ax2(w1, kS1, F), ax1(1));
            g.B = mat(param(0), 0, ax1(kC1), ax1(1));
            g.C = mat(U, 0, ax1(kC1), ax1(1));
            g.bias = param(1); g.bias2 = param(2);
            DCS_CHECK(launch(g, T128x32, true, false));
        }
        // F2: a2b[(b,h,w)][o] = sum_{dh,c} a1b[b][h+dh][w][c] W2i[dh][c][o] + b2 + b2b
        {
            Gemm g = gemm0((int)Rh, kC2, K2);
            g.A = mat(U, 0, ax3(w1, h2, kC1, row1, img1), ax2(kC1, 1, row1));
            g.B = mat(param(3), 0, ax1(kC2), ax1(1));
            g.C = mat(a2b, 0, ax1(kC2), ax1(1));
            g.bias = param(4); g.bias2 = param(5);
            DCS_CHECK(launch(g, T128x32, true, false));
        }
        // F3: z = rectify(a2b . Wfci + bfc), pre-activation saved: split-K over flat, then the fixed-order sum
        {
            Gemm g = gemm0(B, kHidden, (int)flat);
            g.A = mat(a2b, 0, ax1(flat), ax1(1));
            g.B = mat(param(6), 0, ax1(kHidden), ax1(1));
            g.partial = partS; g.splits = splits3; g.kchunk = kchunk3;
            DCS_CHECK(launch(g, T32x32, true, false));
            DCS_CHECK(finish(partS, splits3, kHidden, param(7), z, prez, EPI_RELU | EPI_SAVEPRE));
        }
        // F4: d_k = rectify(z . W_ki + b_ki) -> V slots 1 .. 4 (the live rows of an image are contiguous), pre-activations saved
        {
            Gemm g = gemm0(B, (int)flat, kHidden);
            g.A = mat(z, 0, ax1(kHidden), ax1(1));
            g.B = mat(param(8), 0, ax1(flat), ax1(1));
            g.C = mat(V, padoff, ax1(imgp), ax1(1));
            g.X = mat(pre, 0, ax1(flat), ax1(1));
            g.bias = param(9);
            g.epi = EPI_RELU | EPI_SAVEPRE;
            g.nbatch = kSrc;
            for (int k = 0; k < kSrc; ++k) {
                g.boff[k][1] = k * wstep;
                g.boff[k][2] = (k + 1) * Vslot;
                g.boff[k][3] = k * (int64_t)B * flat;
                g.boff[k][4] = k * wstep;
            }
            DCS_CHECK(launch(g, rows_tile(B), true, false));
        }
        // F5: g_k[(b,t,w)][c] = sum_{dh,o} V[b][t+dh][w][o] W2i[kh-1-dh][c][o] -> GA slots 1 .. 4
        {
            Gemm g = gemm0((int)R1, kC1, K2);
            g.A = mat(V, 0, ax3(w1, tc, kC2, row1, imgp), ax2(kC2, 1, row1));
            g.B = mat(param(3), (int64_t)(kh - 1) * kTap, ax2(kC2, 1, -(int64_t)kTap), ax1(kC2));
            g.C = mat(GA, 0, ax1(kC1), ax1(1));
            g.nbatch = kSrc;
            for (int k = 0; k < kSrc; ++k) {
                g.boff[k][0] = (k + 1) * Vslot;
                g.boff[k][2] = (k + 1) * Uslot;
            }
            DCS_CHECK(launch(g, T128x32, true, true));
        }
        // F6: q = conv1^T(g_k) + bo
        {
            const int64_t n = kSrc * RF;
            hipLaunchKernelGGL((deconv1_kernel<kK1, kC1, kS1, kSrc>), dim3((unsigned)dcs_cdiv(n, kThreads)), dim3(kThreads),
                               0, ctx->stream, (const float*)(GA + Uslot), Uslot, (const float*)param(0),
                               (const float*)param(16), Q, B, tc, F, w1);
            DCS_HIP(hipGetLastError());
        }
        return DCS_OK;
    }

    int loss(const float* x, const float* tgt, double* out7_d) override {
        BLoss a;
        a.q = Q; a.x = x; a.tgt = tgt; a.rnd = rnd; a.xy = xy; a.part = lpart;
        a.plane = (int64_t)tc * F;
        a.n = RF;
        a.eps = hyp[0];
        const int nblk = (int)std::min<int64_t>(kLossBlocks, dcs_cdiv(a.n, kThreads));
        hipLaunchKernelGGL(b10_loss_kernel, dim3(nblk), dim3(kThreads), 0, ctx->stream, a);
        DCS_HIP(hipGetLastError());
        return loss_reduce<Bach10Sums>(nblk, out7_d, grad() + off[16]);
    }

    int backward() override {
        const int64_t Bflat = (int64_t)B * flat;
        const int64_t row1 = (int64_t)w1 * kC1, img1 = (int64_t)tc * row1, imgp = (int64_t)hp * row1;
        const int64_t padoff = (int64_t)(kh - 1) * row1, Vslot = (int64_t)B * imgp, Uslot = R1 * kC1;
        const int64_t wstep = off[10] - off[8];
        float* grad = this->grad();
        // B1: dg_k[(b,t,w)][c] = sum_j dY_k[b][t][4 w + j] W1i[j][c] -> U slots 1 .. 4
        {
            Gemm g = gemm0((int)R1, kC1, kK1);
            g.A = mat(xy, 0, ax2(w1, kS1, F), ax1(1));
            g.B = mat(param(0), 0, ax1(kC1), ax1(1));
            g.C = mat(U, 0, ax1(kC1), ax1(1));
            g.nbatch = kSrc;
            for (int k = 0; k < kSrc; ++k) {
                g.boff[k][0] = (k + 1) * RF;
                g.boff[k][2] = (k + 1) * Uslot;
            }
            DCS_CHECK(launch(g, T128x32, true, false));
        }
        // B2: dpre_k = conv2(dg_k) * r'(pre_k)  (the F2 form)
        {
            Gemm g = gemm0((int)Rh, kC2, K2);
            g.A = mat(U, 0, ax3(w1, h2, kC1, row1, img1), ax2(kC1, 1, row1));
            g.B = mat(param(3), 0, ax1(kC2), ax1(1));
            g.C = mat(dpre, 0, ax1(kC2), ax1(1));
            g.X = mat(pre, 0, ax1(kC2), ax1(1));
            g.epi = EPI_DRELU;
            g.nbatch = kSrc;
            for (int k = 0; k < kSrc; ++k) {
                g.boff[k][0] = (k + 1) * Uslot;
                g.boff[k][2] = k * Bflat;
                g.boff[k][3] = k * Bflat;
            }
            DCS_CHECK(launch(g, T128x32, true, false));
        }
        // B3: dprez = (sum_k dpre_k . W_ki^T) * r'(prez): K = 4 flat, concatenated over k, split-K
        {
            Gemm g = gemm0(B, kHidden, (int)(kSrc * flat));
            g.A = mat(dpre, 0, ax1(flat), ax2(flat, 1, Bflat));
            g.B = mat(param(8), 0, ax2(flat, 1, wstep), ax1(flat));
            g.partial = partS; g.splits = splitsB3; g.kchunk = kchunkB3;
            DCS_CHECK(launch(g, T32x32, true, true));
            DCS_CHECK(finish(partS, splitsB3, kHidden, nullptr, dprez, prez, EPI_DRELU));
        }
        // B4: da2 = dprez . Wfci^T -> V slot 0 (the live rows)
        {
            Gemm g = gemm0(B, (int)flat, kHidden);
            g.A = mat(dprez, 0, ax1(kHidden), ax1(1));
            g.B = mat(param(6), 0, ax1(1), ax1(kHidden));
            g.C = mat(V, padoff, ax1(imgp), ax1(1));
            DCS_CHECK(launch(g, rows_tile(B), true, true));
        }
        // B5: da1 = conv2^T(da2) -> GA slot 0  (the F5 form)
        {
            Gemm g = gemm0((int)R1, kC1, K2);
            g.A = mat(V, 0, ax3(w1, tc, kC2, row1, imgp), ax2(kC2, 1, row1));
            g.B = mat(param(3), (int64_t)(kh - 1) * kTap, ax2(kC2, 1, -(int64_t)kTap), ax1(kC2));
            g.C = mat(GA, 0, ax1(kC1), ax1(1));
            DCS_CHECK(launch(g, T128x32, true, true));
        }
        // dW1 | db1: dW1i[j][c] = sum over the 5 R1 windows of [x; dY_k][s][b][t][4 w + j] [da1; g_k][s][b][t][w][c], ones row
        // over the da1 block
        {
            Gemm g = gemm0(kK1 + 1, kC1, (int)((kSrc + 1) * R1));
            g.A = mat(xy, 0, ax1(1), ax2(w1, kS1, F));
            g.B = mat(GA, 0, ax1(kC1), ax1(1));
            g.ones_row = kK1; g.ones_klim = (int)R1;
            g.partial = part1; g.splits = splits1; g.kchunk = kchunk1;
            DCS_CHECK(launch(g, T32x32, false, false));
        }
        // dW2 | db2: dW2i[(dh,c)][o] = sum_{(s,b,h,w)} U[s][b][h+dh][w][c] V[s][b][h+kh-1][w][o], ones row over da2
        {
            Gemm g = gemm0(K2 + 1, kC2, (int)((kSrc + 1) * Rh));
            g.A = mat(U, 0, ax2(kC1, 1, row1), ax3(w1, h2, kC1, row1, img1));
            g.B = mat(V, padoff, ax3(w1, h2, kC2, row1, imgp), ax1(1));
            g.ones_row = K2; g.ones_klim = (int)Rh;
            g.partial = part2; g.splits = splits2; g.kchunk = kchunk2;
            DCS_CHECK(launch(g, T128x32, false, false));
        }
        // dWfc | dbfc = [a2b^T; 1] . dprez -> grads (Wfc and bfc are adjacent)
        {
            Gemm g = gemm0((int)flat + 1, kHidden, B);
            g.A = mat(a2b, 0, ax1(1), ax1(flat));
            g.B = mat(dprez, 0, ax1(kHidden), ax1(1));
            g.C = mat(grad + off[6], 0, ax1(kHidden), ax1(1));
            g.ones_row = (int)flat; g.ones_klim = B;
            g.scale = sign;
            DCS_CHECK(launch(g, T64x64, false, false));
        }
        // dW_k | db_k = [z^T; 1] . dpre_k -> grads (W_k and b_k are adjacent)
        {
            Gemm g = gemm0(kHidden + 1, (int)flat, B);
            g.A = mat(z, 0, ax1(1), ax1(kHidden));
            g.B = mat(dpre, 0, ax1(flat), ax1(1));
            g.C = mat(grad + off[8], 0, ax1(flat), ax1(1));
            g.ones_row = kHidden; g.ones_klim = B;
            g.scale = sign;
            g.nbatch = kSrc;
            for (int k = 0; k < kSrc; ++k) {
                g.boff[k][1] = k * Bflat;
                g.boff[k][2] = k * wstep;
            }
            DCS_CHECK(launch(g, T64x64, false, false));
        }
        {
            Reduce r;
            memset(&r, 0, sizeof(r));
            r.scale = sign;
            r.part[0] = part1; r.dst[0] = grad + off[0]; r.count[0] = (int64_t)(kK1 + 1) * kC1; r.splits[0] = splits1;
            r.part[1] = part2; r.dst[1] = grad + off[3]; r.count[1] = (int64_t)(K2 + 1) * kC2; r.splits[1] = splits2;
            r.N[0] = r.N[1] = kC1;
            r.dup[0] = r.dup[1] = 1;
            DCS_CHECK(reduce(r));
        }
        return DCS_OK;
    }

    int layout(float* flat_d, float* const* pkl, int to_internal) override {
        return run_layout(flat_d, pkl, to_internal, Bach10Map{kh, h2, w1});
    }
};

}  // namespace

int bach10_trainer_new(int time_context, int F, int batch, dcs_trainer** out) {
    // time_context stops at 47, not at the 64 of the other trainers: from 48 on the inference path of this graph has no
    // column convolution (its f32 kernel would need more than 160 KiB of LDS), and a model nothing can load is no use
    if (time_context < 2 || time_context > kMaxTc || F < kK1 || F > 2049 || batch < 1 || batch > 1024)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: Bach10 graph: time_context %d (2 .. %d), F %d (30 .. 2049), batch %d (1 .. 1024)",
                 time_context, kMaxTc, F, batch);
    const int64_t kh = 2 * time_context / 3, w1 = (F - kK1) / kS1 + 1, h2 = time_context - kh + 1, flat = kC2 * h2 * w1;
    const int64_t R1 = (int64_t)batch * time_context * w1, Rh = (int64_t)batch * h2 * w1;
    // every GEMM index (a row, a column or a K position, Ax) stays below kBig: the K of dW1, of dW2 and of B3, the rows of
    // dWfc, and B flat, which bounds every per-source offset unit
    const int64_t most = std::max({(kSrc + 1) * R1, (kSrc + 1) * Rh, kSrc * flat, flat + 1, (int64_t)batch * flat});
    if (most >= kBig)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: Bach10 graph: a GEMM index of %lld at time_context %d, F %d, batch %d",
                 (long long)most, time_context, F, batch);
    Bach10Trainer* t = new Bach10Trainer();
    t->kh = (int)kh; t->w1 = (int)w1; t->h2 = (int)h2;
    t->hp = t->h2 + 2 * (t->kh - 1);
    t->K2 = t->kh * kC1;
    t->R1 = R1;
    t->Rh = Rh;
    t->flat = flat;
    t->nsrc = kSrc;
    t->nparams = kNparams;
    t->loss_sums = kLossSums;
    const int64_t s[kNparams][4] = {{kC1, 1, 1, kK1}, {kC1, 1, 1, 1}, {kC1, 1, 1, 1}, {kC2, kC1, kh, 1}, {kC2, 1, 1, 1},
                                    {kC2, 1, 1, 1}, {flat, kHidden, 1, 1}, {kHidden, 1, 1, 1}, {kHidden, flat, 1, 1},
                                    {flat, 1, 1, 1}, {kHidden, flat, 1, 1}, {flat, 1, 1, 1}, {kHidden, flat, 1, 1},
                                    {flat, 1, 1, 1}, {kHidden, flat, 1, 1}, {flat, 1, 1, 1}, {kSrc, 1, 1, 1}};
    memcpy(t->shapes, s, sizeof(s));
    *out = t;
    return DCS_OK;
}

// Training of the iKala singing-voice graph (examples/ikala/trainCNN.py: build_ca :66-118, loss :155-189, adadelta :193)
// on gfx950.  conv1 30 x (1 x 30) stride (1, 3) + BiasLayer, conv2 30 x (10 x 20) + BiasLayer, dense 256, two rectified
// dense layers of flat = 30 h2 w2 units, per source the InverseLayers of conv2 and conv1, BiasLayer(2) and rectify.
//
// One step on the ctx stream, no host synchronisation and no float atomics (two runs give bit-identical weights):
//
//   forward   F1 a1b = conv1(x) + b1 + b1b             gemm 128x32  K = 30 taps (saved: a1b)
//             F2 a2b = conv2(a1b) + b2 + b2b           gemm 128x32  implicit GEMM, K = (dh, dw c) = 10 x 600
//             F3 z = rectify(a2b . Wfc + bfc)          gemm 32x32 split-K over flat, finish (saved: z, pre-activation)
//             F4 d_k = rectify(z . W_k + b_k), k < 2   gemm, 2 batches, into the zero-padded V (saved: pre-activations)
//             F5 g_k = conv2^T(d_k)                    gemm 128x32  implicit GEMM over V (9 / 19 zero rows / columns)
//             F6 q = conv1^T(g_k) + bo                 train::deconv1_kernel: 10 taps x 30 channels per output, fixed order
//   loss      ik_loss_kernel: masks, the four components, dE/dq (rectify' with the 0.5 tie), per-workgroup f64 sums
//             train::loss_reduce_kernel: fixed-order sum -> loss and components (f64), sign(E), the output-bias gradient
//   backward  B1 dg_k = conv1(dY_k)    B2 dpre_k = conv2(dg_k) * r'(pre_k)    B3 dprez = (sum_k dpre_k . W_k^T) * r'(prez)
//             B4 da2 = dprez . Wfc^T   B5 da1 = conv2^T(da2)
//   weights   dW1|db1 = [x; dY_k] windows^T . [da1; g_k]            split-K (K = 3 B tc w1), fixed-order reduce
//             dW2|db2 = [a1b; dg_k] windows^T . [da2; d_k]          split-K (K = 3 B h2 w2), fixed-order reduce
//             dWfc|dbfc = a2b^T . dprez,  dW_k|db_k = z^T . dpre_k
//             every bias gradient is the "ones" row of its weight GEMM; b1b / b2b get copies of b1 / b2 (identical in Theano)
//   update    train::adadelta_kernel over the flat [params | grads | accu | delta_accu] buffer, four floats per thread
//
// The GEMMs are forms of the shared template (train_core.h): 128 x 32 tiles for every conv2-family GEMM (N = 30 channels),
// 64 x 64 and 32 x 32 for the dense ones, each operand loaded K-fastest or M/N-fastest, whichever is contiguous in memory.
// The operands' Ax addressing covers the implicit-GEMM windows of conv1 and conv2 and the K-concatenations above without
// copies.
//
// Internal parameter layouts (the flat buffer; dcs_trainer_get / _create convert to and from the .pkl layout):
//   W1 [30 j][30 c]: W1i[j][c] = W1[c,0,0,29-j]           W2 [10 dh][20 dw][30 c][30 o]: W2i = W2[o,c,9-dh,19-dw] (flips)
//   Wfc [(h,w,o)][256] and W_k [256][(h,w,o)], b_k [(h,w,o)]: the 30 x h2 x w2 map channels-last, .pkl order o h2 w2 + h w2 + w
// Activations are channels-last: a1b / dg / g / da1 [B][tc][w1][30], a2b / d_k / dpre [B][h2][w2][30]; d_k and da2 live in
// V [B][h2 + 18][w2 + 38][30], zero rows and columns around them, so that conv2^T is a plain implicit GEMM.
#include "train_core.h"

using namespace train;

namespace {

constexpr int kC1 = 30, kK1 = 30, kS1 = 3;       // conv1: 30 filters of 1 x 30, stride (1, 3)
constexpr int kC2 = 30, kH2 = 10, kW2 = 20;      // conv2: 30 filters of 10 x 20
constexpr int kRow = kW2 * kC1;                  // 600: one row of a conv2 window (20 taps x 30 channels), contiguous
constexpr int kK2 = kH2 * kRow;                  // 6000
constexpr int kHidden = 256, kNparams = 13;

// four components, then two output-bias gradient sums; E = vocals_error + acc_error - negative_error_voc
// (trainCNN.py:189); out7 = (|E|, vocals_error, acc_error, negative_error_voc, negative_error_acc, 0, 0)
struct IkalaSums {
    static constexpr int kOut = 4, kDbo = 2;
    static __device__ double E(const double* s) { return s[0] + s[1] - s[2]; }
};
constexpr int kLossSums = IkalaSums::kOut + IkalaSums::kDbo;

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
    block_sums(acc, a.part);
}

// the .pkl index of element k of the internal section s
struct IkalaMap {
    int h2, w2;
    __device__ int64_t operator()(int s, int64_t k) const {
        const int64_t hw = (int64_t)h2 * w2, map = kC2 * hw;
        // map position (h, w, o) channels-last -> .pkl o h2 w2 + h w2 + w
        auto pkl_of = [&](int64_t col) {
            const int64_t o = col % kC2, hwi = col / kC2;
            return o * hw + hwi;
        };
        if (s == 0) {                                     // W1i[j][c] = W1[c][29-j]
            const int64_t j = k / kC1, c = k % kC1;
            return c * kK1 + (kK1 - 1 - j);
        } else if (s == 3) {                              // W2i[dh][dw][c][o] = W2[o][c][9-dh][19-dw]
            const int64_t dh = k / (kW2 * kC1 * kC2), dw = (k / (kC1 * kC2)) % kW2, c = (k / kC2) % kC1, o = k % kC2;
            return ((o * kC1 + c) * kH2 + (kH2 - 1 - dh)) * kW2 + (kW2 - 1 - dw);
        } else if (s == 6) {                              // Wfc rows (h, w, o)
            return pkl_of(k / kHidden) * kHidden + k % kHidden;
        } else if (s == 8 || s == 10) {                   // W_k columns (h, w, o)
            return (k / map) * map + pkl_of(k % map);
        } else if (s == 9 || s == 11) {
            return pkl_of(k);
        }
        return k;
    }
};

// the dense GEMMs with M = B rows: 64 x 64 tiles from 64 rows up
Tile rows_tile(int M) { return M >= 64 ? T64x64 : T32x32; }

struct IkalaTrainer : dcs_trainer {
    int w1 = 0, h2 = 0, w2 = 0, hp = 0, wp = 0;
    int64_t R1 = 0, Rh = 0, flat = 0;
    // views into work
    float *xy, *U, *GA, *V, *a2b, *z, *prez, *dprez, *pre, *dpre, *part1, *part2, *partS;
    int splits1 = 1, splits2 = 1, splits3 = 1, splitsB3 = 1, kchunk1 = 0, kchunk2 = 0, kchunk3 = 0, kchunkB3 = 0;

    void plan(std::vector<std::pair<float**, int64_t>>& parts) override {
        // about 2 workgroups per CU, at most 128 slices
        pick_split(dcs_cdiv(kK1 + 1, 32), 3 * R1, &splits1, &kchunk1, 512, 128);
        // dW2: 47 row tiles of a K of 3 B h2 w2 (288 k at B = 32): 8 workgroups per CU keep the SIMDs busy
        pick_split(dcs_cdiv(kK2 + 1, 128), 3 * Rh, &splits2, &kchunk2, 2048, 128);
        pick_split((int64_t)dcs_cdiv(B, 32) * (kHidden / 32), flat, &splits3, &kchunk3, 512, 128);
        pick_split((int64_t)dcs_cdiv(B, 32) * (kHidden / 32), 2 * flat, &splitsB3, &kchunkB3, 512, 128);
        const int64_t b = B;
        parts.insert(parts.end(), {{&xy, 3 * RF}, {&U, 3 * R1 * kC1}, {&GA, 3 * R1 * kC1}, {&V, 3 * b * hp * wp * kC2},
                                   {&Q, 2 * RF}, {&a2b, b * flat}, {&z, b * kHidden}, {&prez, b * kHidden},
                                   {&dprez, b * kHidden}, {&pre, 2 * b * flat}, {&dpre, 2 * b * flat},
                                   {&part1, (int64_t)splits1 * (kK1 + 1) * kC1},
                                   {&part2, (int64_t)splits2 * (kK2 + 1) * kC2},
                                   {&partS, (int64_t)std::max(splits3, splitsB3) * b * kHidden}});
    }

    int forward(const float* x) override {
        const int64_t row1 = (int64_t)w1 * kC1, img1 = (int64_t)tc * row1, rowp = (int64_t)wp * kC2, imgp = (int64_t)hp * rowp;
        const int64_t padoff = (int64_t)(kH2 - 1) * rowp + (kW2 - 1) * kC2, Vslot = (int64_t)B * imgp, Uslot = R1 * kC1;
        const int64_t wstep = off[10] - off[8];
        // F1: a1b[(b,t,w)][c] = sum_j x[b][t][3 w + j] W1i[j][c] + b1 + b1b -> U slot 0
        {
            Gemm g = gemm0((int)R1, kC1, kK1);
            g.A = mat((float*)x, 0, ax2(w1, kS1, F), ax1(1));
            g.B = mat(param(0), 0, ax1(kC1), ax1(1));
            g.C = mat(U, 0, ax1(kC1), ax1(1));
            g.bias = param(1); g.bias2 = param(2);
            DCS_CHECK(launch(g, T128x32, true, false));
        }
        // F2: a2b[(b,h,w)][o] = sum_{dh,(dw,c)} a1b[b][h+dh][w+dw][c] W2i[dh][dw][c][o] + b2 + b2b
        {
            Gemm g = gemm0((int)Rh, kC2, kK2);
            g.A = mat(U, 0, ax3(w2, h2, kC1, row1, img1), ax2(kRow, 1, row1));
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
        // F4: d_k = rectify(z . W_ki + b_ki) -> V slots 1, 2 (zero-padded map), pre-activations saved
        {
            Gemm g = gemm0(B, (int)flat, kHidden);
            g.A = mat(z, 0, ax1(kHidden), ax1(1));
            g.B = mat(param(8), 0, ax1(flat), ax1(1));
            g.C = mat(V, padoff, ax1(imgp), ax2((int64_t)w2 * kC2, 1, rowp));
            g.X = mat(pre, 0, ax1(flat), ax1(1));
            g.bias = param(9);
            g.epi = EPI_RELU | EPI_SAVEPRE;
            g.nbatch = 2;
            for (int k = 0; k < 2; ++k) {
                g.boff[k][1] = k * wstep;
                g.boff[k][2] = (k + 1) * Vslot;
                g.boff[k][3] = k * (int64_t)B * flat;
                g.boff[k][4] = k * wstep;
            }
            DCS_CHECK(launch(g, rows_tile(B), true, false));
        }
        // F5: g_k[(b,t,w)][c] = sum_{dh,(dw,o)} V[b][t+dh][w+dw][o] W2i[9-dh][19-dw][c][o] -> GA slots 1, 2
        {
            Gemm g = gemm0((int)R1, kC1, kK2);
            g.A = mat(V, 0, ax3(w1, tc, kC2, rowp, imgp), ax2(kRow, 1, rowp));
            g.B = mat(param(3), (int64_t)(kH2 * kW2 - 1) * kC1 * kC2, ax2(kC2, 1, -(int64_t)kC1 * kC2), ax1(kC2));
            g.C = mat(GA, 0, ax1(kC1), ax1(1));
            g.nbatch = 2;
            for (int k = 0; k < 2; ++k) {
                g.boff[k][0] = (k + 1) * Vslot;
                g.boff[k][2] = (k + 1) * Uslot;
            }
            DCS_CHECK(launch(g, T128x32, true, true));
        }
        // F6: q = conv1^T(g_k) + bo
        {
            const int64_t n = 2 * (int64_t)B * tc * F;
            hipLaunchKernelGGL((deconv1_kernel<kK1, kC1, kS1, 2>), dim3((unsigned)dcs_cdiv(n, kThreads)), dim3(kThreads),
                               0, ctx->stream, (const float*)(GA + Uslot), Uslot, (const float*)param(0),
                               (const float*)param(12), Q, B, tc, F, w1);
            DCS_HIP(hipGetLastError());
        }
        return DCS_OK;
    }

    int loss(const float* x, const float* tgt, double* out7_d) override {
        ILoss a;
        a.q = Q; a.x = x; a.tgt = tgt; a.rnd = rnd; a.xy = xy; a.part = lpart;
        a.plane = (int64_t)tc * F;
        a.n = RF;
        a.eps = hyp[0]; a.alpha = hyp[1]; a.beta_acc = hyp[2]; a.beta_voc = hyp[3];
        const int nblk = (int)std::min<int64_t>(kLossBlocks, dcs_cdiv(a.n, kThreads));
        hipLaunchKernelGGL(ik_loss_kernel, dim3(nblk), dim3(kThreads), 0, ctx->stream, a);
        DCS_HIP(hipGetLastError());
        return loss_reduce<IkalaSums>(nblk, out7_d, grad() + off[12]);
    }

    int backward() override {
        const int64_t Bflat = (int64_t)B * flat;
        const int64_t row1 = (int64_t)w1 * kC1, img1 = (int64_t)tc * row1, rowp = (int64_t)wp * kC2, imgp = (int64_t)hp * rowp;
        const int64_t padoff = (int64_t)(kH2 - 1) * rowp + (kW2 - 1) * kC2, Vslot = (int64_t)B * imgp, Uslot = R1 * kC1;
        const int64_t wstep = off[10] - off[8];
        float* grad = this->grad();
        // B1: dg_k[(b,t,w)][c] = sum_j dY_k[b][t][3 w + j] W1i[j][c] -> U slots 1, 2
        {
            Gemm g = gemm0((int)R1, kC1, kK1);
            g.A = mat(xy, 0, ax2(w1, kS1, F), ax1(1));
            g.B = mat(param(0), 0, ax1(kC1), ax1(1));
            g.C = mat(U, 0, ax1(kC1), ax1(1));
            g.nbatch = 2;
            for (int k = 0; k < 2; ++k) {
                g.boff[k][0] = (k + 1) * RF;
                g.boff[k][2] = (k + 1) * Uslot;
            }
            DCS_CHECK(launch(g, T128x32, true, false));
        }
        // B2: dpre_k = conv2(dg_k) * r'(pre_k)  (the F2 form)
        {
            Gemm g = gemm0((int)Rh, kC2, kK2);
            g.A = mat(U, 0, ax3(w2, h2, kC1, row1, img1), ax2(kRow, 1, row1));
            g.B = mat(param(3), 0, ax1(kC2), ax1(1));
            g.C = mat(dpre, 0, ax1(kC2), ax1(1));
            g.X = mat(pre, 0, ax1(kC2), ax1(1));
            g.epi = EPI_DRELU;
            g.nbatch = 2;
            for (int k = 0; k < 2; ++k) {
                g.boff[k][0] = (k + 1) * Uslot;
                g.boff[k][2] = k * Bflat;
                g.boff[k][3] = k * Bflat;
            }
            DCS_CHECK(launch(g, T128x32, true, false));
        }
        // B3: dprez = (sum_k dpre_k . W_ki^T) * r'(prez): K = 2 flat, concatenated over k, split-K
        {
            Gemm g = gemm0(B, kHidden, (int)(2 * flat));
            g.A = mat(dpre, 0, ax1(flat), ax2(flat, 1, Bflat));
            g.B = mat(param(8), 0, ax2(flat, 1, wstep), ax1(flat));
            g.partial = partS; g.splits = splitsB3; g.kchunk = kchunkB3;
            DCS_CHECK(launch(g, T32x32, true, true));
            DCS_CHECK(finish(partS, splitsB3, kHidden, nullptr, dprez, prez, EPI_DRELU));
        }
        // B4: da2 = dprez . Wfci^T -> V slot 0 (zero-padded map)
        {
            Gemm g = gemm0(B, (int)flat, kHidden);
            g.A = mat(dprez, 0, ax1(kHidden), ax1(1));
            g.B = mat(param(6), 0, ax1(1), ax1(kHidden));
            g.C = mat(V, padoff, ax1(imgp), ax2((int64_t)w2 * kC2, 1, rowp));
            DCS_CHECK(launch(g, rows_tile(B), true, true));
        }
        // B5: da1 = conv2^T(da2) -> GA slot 0  (the F5 form)
        {
            Gemm g = gemm0((int)R1, kC1, kK2);
            g.A = mat(V, 0, ax3(w1, tc, kC2, rowp, imgp), ax2(kRow, 1, rowp));
            g.B = mat(param(3), (int64_t)(kH2 * kW2 - 1) * kC1 * kC2, ax2(kC2, 1, -(int64_t)kC1 * kC2), ax1(kC2));
            g.C = mat(GA, 0, ax1(kC1), ax1(1));
            DCS_CHECK(launch(g, T128x32, true, true));
        }
        // dW1 | db1: dW1i[j][c] = sum over the 3 R1 windows of [x; dY_k][s][b][t][3 w + j] [da1; g_k][s][b][t][w][c], ones row
        // over the da1 block
        {
            Gemm g = gemm0(kK1 + 1, kC1, (int)(3 * R1));
            g.A = mat(xy, 0, ax1(1), ax2(w1, kS1, F));
            g.B = mat(GA, 0, ax1(kC1), ax1(1));
            g.ones_row = kK1; g.ones_klim = (int)R1;
            g.partial = part1; g.splits = splits1; g.kchunk = kchunk1;
            DCS_CHECK(launch(g, T32x32, false, false));
        }
        // dW2 | db2: dW2i[(dh,dw,c)][o] = sum_{(s,b,h,w)} U[s][b][h+dh][w+dw][c] V[s][b][h+9][w+19][o], ones row over da2
        {
            Gemm g = gemm0(kK2 + 1, kC2, (int)(3 * Rh));
            g.A = mat(U, 0, ax2(kRow, 1, row1), ax3(w2, h2, kC1, row1, img1));
            g.B = mat(V, padoff, ax3(w2, h2, kC2, rowp, imgp), ax1(1));
            g.ones_row = kK2; g.ones_klim = (int)Rh;
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
            g.nbatch = 2;
            for (int k = 0; k < 2; ++k) {
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
            r.part[1] = part2; r.dst[1] = grad + off[3]; r.count[1] = (int64_t)(kK2 + 1) * kC2; r.splits[1] = splits2;
            r.N[0] = r.N[1] = kC1;
            r.dup[0] = r.dup[1] = 1;
            DCS_CHECK(reduce(r));
        }
        return DCS_OK;
    }

    int layout(float* flat_d, float* const* pkl, int to_internal) override {
        return run_layout(flat_d, pkl, to_internal, IkalaMap{h2, w2});
    }
};

}  // namespace

int ikala_trainer_new(int time_context, int F, int batch, dcs_trainer** out) {
    if (time_context < kH2 || time_context > 64 || F < 87 || F > 2049 || batch < 1 || batch > 1024)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: iKala graph: time_context %d (10 .. 64), F %d (87 .. 2049), batch %d (1 .. 1024)",
                 time_context, F, batch);
    IkalaTrainer* t = new IkalaTrainer();
    const int64_t w1 = (F - kK1) / kS1 + 1, h2 = time_context - kH2 + 1, w2 = w1 - kW2 + 1, flat = kC2 * h2 * w2;
    t->w1 = (int)w1; t->h2 = (int)h2; t->w2 = (int)w2;
    t->hp = t->h2 + 2 * (kH2 - 1);
    t->wp = t->w2 + 2 * (kW2 - 1);
    t->R1 = (int64_t)batch * time_context * w1;
    t->Rh = (int64_t)batch * h2 * w2;
    t->flat = flat;
    t->nsrc = 2;
    t->nparams = kNparams;
    t->loss_sums = kLossSums;
    const int64_t s[kNparams][4] = {{kC1, 1, 1, kK1}, {kC1, 1, 1, 1}, {kC1, 1, 1, 1}, {kC2, kC1, kH2, kW2}, {kC2, 1, 1, 1},
                                    {kC2, 1, 1, 1}, {flat, kHidden, 1, 1}, {kHidden, 1, 1, 1}, {kHidden, flat, 1, 1},
                                    {flat, 1, 1, 1}, {kHidden, flat, 1, 1}, {flat, 1, 1, 1}, {2, 1, 1, 1}};
    memcpy(t->shapes, s, sizeof(s));
    *out = t;
    return DCS_OK;
}

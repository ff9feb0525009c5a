// Training of the score-informed Bach10 graph (examples/bach10_scoreinformed/trainCNNrwc.py: build_ca :134-193, loss :235-275,
// adadelta :279; trainCNNrwc_samp.py :195-235 and :275-321 train its single-branch form with the same loss) on gfx950.  The
// graph is the Bach10 graph of train_bach10.hip with three differences: conv1 reads four input channels (W1 [30, 4, 1, 30]) and
// its InverseLayer writes four output channels per decoder branch; the loss reads prediction2[:, 0:4], the four channels of
// branch 0 alone, and its mixture is the sum of the four input channels; the input is the mixture times four harmonic masks
// (the feed, train::gather_score_kernel).
//
// DCS_ARCH_BACH10_SI (17 arrays) and DCS_ARCH_BACH10_SI1 (11 arrays) train the same live computation.  The 17-array graph's
// fc12, fc13, fc14 (arrays 10 .. 15) and bo[4:16] reach no loss term: theano.grad gives them exact zeros, and Adadelta from a
// zero state leaves them, accu and delta_accu untouched for ever.  They are held once, outside the stepped state (at 2049 bins
// they are 3 x 171 MB; in the state they would be four times that and stream through the update every step):
// dcs_trainer_get(which = 0) returns them bit-identical to what create was given, which = 1, 2, 3 return zeros.
//
// One step on the ctx stream, no host synchronisation and no float atomics (two runs give bit-identical weights):
//
//   forward   F1 a1b = conv1(x) + b1 + b1b             gemm 128x32  x [B][4][tc][F] read in place, K = (channel, tap) = 4 x 30
//             F2 a2b = conv2(a1b) + b2 + b2b           gemm 128x32  implicit GEMM, K = (dh, c) = kh x 30
//             F3 z = rectify(a2b . Wfc + bfc)          gemm 32x32 split-K over flat, finish (saved: z, pre-activation)
//             F4 d = rectify(z . W_11 + b_11)          gemm, into the row-padded V (saved: pre-activation)
//             F5 g = conv2^T(d)                        gemm 128x32  implicit GEMM over V
//             F6 q_c = conv1^T(g)[c] + bo[c], c < 4    train::deconv1_channels_kernel: one slot, four weight slabs
//   loss      si_loss_kernel: x = ((x0 + x1) + x2) + x3, masks, the four errors, dE/dq (rectify' with the 0.5 tie), f64 sums
//             train::loss_reduce_kernel: fixed-order sum -> loss and errors (f64), sign(E), the output-bias gradient
//   backward  B1 dg = conv1(dY)   B2 dpre = conv2(dg) * r'(pre)   B3 dprez = (dpre . W_11^T) * r'(prez)   B4 da2 = dprez . Wfc^T
//             B5 da1 = conv2^T(da2)
//   weights   dW1|db1 = [x; dY] windows^T . [da1; g]                M = 4 x 30 + 1 = 121, split-K (K = 2 B tc w1)
//             dW2|db2 = [a1b; dg] windows^T . [da2; d]              split-K (K = 2 B h2 w1)
//             dWfc|dbfc = a2b^T . dprez,  dW_11|db_11 = z^T . dpre
//   update    train::adadelta_kernel over the 11 stepped arrays
//
// Internal layouts are train_bach10.hip's, with W1 [(ch, j)][30 c]: W1i[ch][j][c] = W1[c, ch, 0, 29 - j].  x, dY and q are
// [B][4][tc][F]; xy holds [x; dY], U [a1b; dg], GA [da1; g], V [da2; d] (two slots each, where the Bach10 graph has five).
#include "train_core.h"

using namespace train;

namespace {

constexpr int kC1 = 30, kK1 = 30, kS1 = 4, kCh = 4;   // conv1: 30 filters of 1 x 30 over 4 channels, stride (1, 4)
constexpr int kKW = kCh * kK1;                         // 120: rows of W1i
constexpr int kC2 = 30;
constexpr int kTap = kC1 * kC2;
constexpr int kHidden = 256, kNstate = 11, kSrc = 4, kBranches = 4;
// the largest time context dcs_model_create's score-informed graph runs: the inference kernels are the Bach10 graph's, whose
// f32 column convolution needs more than 160 KiB of LDS from 48 on
constexpr int kMaxTc = 47;

// out7 = (|E|, error1, error2, error3, error4, 0, 0), E = error1 + .. + error4 (trainCNNrwc.py:270-275)
struct SiSums {
    static constexpr int kOut = 4, kDbo = 4;
    static __device__ double E(const double* s) { return s[0] + s[1] + s[2] + s[3]; }
};
constexpr int kLossSums = SiSums::kOut + SiSums::kDbo;

struct SiLoss {
    const float* q;       // [B][4][tc F] pre-activations of the live output channels
    const float* x;       // [B][4][tc F] inputs
    const float* tgt;     // [B][4][tc F] targets
    const float* rnd;     // [B][tc F] the uniform draw
    float* xy;            // [2][B][4][tc F]: slot 0 <- x, slot 1 <- dE/dq
    double* part;         // [gridDim.x][kLossSums]
    int64_t plane, n;     // tc F, B tc F
    double eps;
};

// trainCNNrwc.py:248-275 per element, in f64: x = ((x0 + x1) + x2) + x3, D = p_1 + .. + p_4 + eps r, m_k = p_k / D, source_k =
// m_k x; the four squared-error sums; dE/dp_k = x / D (G_k - sum_j m_j G_j) with G_k = 2 (source_k - target_k); dE/dq = dE/dp
// r'(q), r'(0) = 0.5.  D = 0 (all four outputs zero, r = 0) gives NaN, as the reference's 0 / 0 does.
__global__ __launch_bounds__(kThreads) void si_loss_kernel(const SiLoss a) {
    double acc[kLossSums];
#pragma unroll
    for (int i = 0; i < kLossSums; ++i) acc[i] = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < a.n; e += (int64_t)gridDim.x * kThreads) {
        const int64_t b = e / a.plane, rem = e - b * a.plane;
        const int64_t o = b * kSrc * a.plane + rem;
        float xc[kCh];
#pragma unroll
        for (int c = 0; c < kCh; ++c) xc[c] = a.x[o + c * a.plane];
        const double x = (((double)xc[0] + (double)xc[1]) + (double)xc[2]) + (double)xc[3];
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
            a.xy[kSrc * a.n + o + j * a.plane] = (float)dq;
        }
#pragma unroll
        for (int c = 0; c < kCh; ++c) a.xy[o + c * a.plane] = xc[c];
    }
    block_sums(acc, a.part);
}

// the .pkl index of element k of the internal section s (sections 0 .. 9 are arrays 0 .. 9, section 10 is bo[0:4])
struct SiMap {
    int kh, h2, w1;
    __device__ int64_t operator()(int s, int64_t k) const {
        const int64_t hw = (int64_t)h2 * w1, map = kC2 * hw;
        auto pkl_of = [&](int64_t col) {
            const int64_t o = col % kC2, hwi = col / kC2;
            return o * hw + hwi;
        };
        if (s == 0) {                                     // W1i[ch][j][c] = W1[c][ch][29-j]
            const int64_t c = k % kC1, chj = k / kC1, ch = chj / kK1, j = chj % kK1;
            return (c * kCh + ch) * kK1 + (kK1 - 1 - j);
        } else if (s == 3) {                              // W2i[dh][c][o] = W2[o][c][kh-1-dh]
            const int64_t dh = k / kTap, c = (k / kC2) % kC1, o = k % kC2;
            return (o * kC1 + c) * kh + (kh - 1 - dh);
        } else if (s == 6) {                              // Wfc rows (h, w, o)
            return pkl_of(k / kHidden) * kHidden + k % kHidden;
        } else if (s == 8) {                              // W_11 columns (h, w, o)
            return (k / map) * map + pkl_of(k % map);
        } else if (s == 9) {                              // b_11
            return pkl_of(k);
        }
        return k;
    }
};

Tile rows_tile(int M) { return M >= 64 ? T64x64 : T32x32; }

struct SiTrainer : dcs_trainer {
    int kh = 0, w1 = 0, h2 = 0, hp = 0, K2 = 0;
    int64_t R1 = 0, Rh = 0, flat = 0;
    bool full = false;            // the 17-array layout: dead parameters held in `dead`
    int64_t ndead = 0;            // 3 (256 flat + flat) + 12
    float *xy, *U, *GA, *V, *a2b, *z, *prez, *dprez, *pre, *dpre, *part1, *part2, *partS, *dead = nullptr;
    int splits1 = 1, splits2 = 1, splits3 = 1, kchunk1 = 0, kchunk2 = 0, kchunk3 = 0;

    void plan(std::vector<std::pair<float**, int64_t>>& parts) override {
        // dW1 is four 32 x 32 tiles and dW2 five 128 x 32 tiles (tc 30) over a K of 2 B tc w1 and 2 B h2 w1; F3 / B3 have the
        // same shape (K = flat) and share their split
        pick_split(dcs_cdiv(kKW + 1, 32), 2 * R1, &splits1, &kchunk1, 512, 512);
        pick_split(dcs_cdiv(K2 + 1, 128), 2 * Rh, &splits2, &kchunk2, 2048, 512);
        pick_split((int64_t)dcs_cdiv(B, 32) * (kHidden / 32), flat, &splits3, &kchunk3, 512, 128);
        const int64_t b = B;
        parts.insert(parts.end(), {{&xy, 2 * kCh * RF}, {&U, 2 * R1 * kC1}, {&GA, 2 * R1 * kC1}, {&V, 2 * b * hp * w1 * kC2},
                                   {&Q, kSrc * RF}, {&a2b, b * flat}, {&z, b * kHidden}, {&prez, b * kHidden},
                                   {&dprez, b * kHidden}, {&pre, b * flat}, {&dpre, b * flat},
                                   {&part1, (int64_t)splits1 * (kKW + 1) * kC1},
                                   {&part2, (int64_t)splits2 * (K2 + 1) * kC2},
                                   {&partS, (int64_t)splits3 * b * kHidden}});
        if (full) parts.push_back({&dead, ndead});
    }

    // conv1 over a [B][4][tc][F] tensor: rows (b, t, w), K = (channel, tap)
    Mat conv1_rows(float* p, int64_t offset) const {
        return mat(p, offset, ax3(w1, tc, kS1, F, (int64_t)kCh * tc * F), ax2(kK1, 1, (int64_t)tc * F));
    }

    int forward(const float* x) override {
        const int64_t row1 = (int64_t)w1 * kC1, img1 = (int64_t)tc * row1, imgp = (int64_t)hp * row1;
        const int64_t padoff = (int64_t)(kh - 1) * row1, Vslot = (int64_t)B * imgp, Uslot = R1 * kC1;
        // F1: a1b[(b,t,w)][c] = sum_{ch,j} x[b][ch][t][4 w + j] W1i[ch][j][c] + b1 + b1b -> U slot 0
        {
            Gemm g = gemm0((int)R1, kC1, kKW);
            g.A = conv1_rows((float*)x, 0);
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
        // F4: d = rectify(z . W_11i + b_11i) -> V slot 1 (the live rows of an image are contiguous), pre-activation saved
        {
            Gemm g = gemm0(B, (int)flat, kHidden);
            g.A = mat(z, 0, ax1(kHidden), ax1(1));
            g.B = mat(param(8), 0, ax1(flat), ax1(1));
            g.C = mat(V, Vslot + padoff, ax1(imgp), ax1(1));
            g.X = mat(pre, 0, ax1(flat), ax1(1));
            g.bias = param(9);
            g.epi = EPI_RELU | EPI_SAVEPRE;
            DCS_CHECK(launch(g, rows_tile(B), true, false));
        }
        // F5: g[(b,t,w)][c] = sum_{dh,o} V[b][t+dh][w][o] W2i[kh-1-dh][c][o] -> GA slot 1
        {
            Gemm g = gemm0((int)R1, kC1, K2);
            g.A = mat(V, Vslot, ax3(w1, tc, kC2, row1, imgp), ax2(kC2, 1, row1));
            g.B = mat(param(3), (int64_t)(kh - 1) * kTap, ax2(kC2, 1, -(int64_t)kTap), ax1(kC2));
            g.C = mat(GA, Uslot, ax1(kC1), ax1(1));
            DCS_CHECK(launch(g, T128x32, true, true));
        }
        // F6: q[b][c] = conv1^T(g)[c] + bo[c]
        {
            const int64_t n = kSrc * RF;
            hipLaunchKernelGGL((deconv1_channels_kernel<kK1, kC1, kS1, kCh>), dim3((unsigned)dcs_cdiv(n, kThreads)),
                               dim3(kThreads), 0, ctx->stream, (const float*)(GA + Uslot), (const float*)param(0),
                               (const float*)param(10), Q, B, tc, F, w1);
            DCS_HIP(hipGetLastError());
        }
        return DCS_OK;
    }

    int loss(const float* x, const float* tgt, double* out7_d) override {
        SiLoss a;
        a.q = Q; a.x = x; a.tgt = tgt; a.rnd = rnd; a.xy = xy; a.part = lpart;
        a.plane = (int64_t)tc * F;
        a.n = RF;
        a.eps = hyp[0];
        const int nblk = (int)std::min<int64_t>(kLossBlocks, dcs_cdiv(a.n, kThreads));
        hipLaunchKernelGGL(si_loss_kernel, dim3(nblk), dim3(kThreads), 0, ctx->stream, a);
        DCS_HIP(hipGetLastError());
        return loss_reduce<SiSums>(nblk, out7_d, grad() + off[10]);
    }

    int backward() override {
        const int64_t row1 = (int64_t)w1 * kC1, img1 = (int64_t)tc * row1, imgp = (int64_t)hp * row1;
        const int64_t padoff = (int64_t)(kh - 1) * row1, Vslot = (int64_t)B * imgp, Uslot = R1 * kC1;
        float* grad = this->grad();
        // B1: dg[(b,t,w)][c] = sum_{ch,j} dY[b][ch][t][4 w + j] W1i[ch][j][c] -> U slot 1
        {
            Gemm g = gemm0((int)R1, kC1, kKW);
            g.A = conv1_rows(xy, kCh * RF);
            g.B = mat(param(0), 0, ax1(kC1), ax1(1));
            g.C = mat(U, Uslot, ax1(kC1), ax1(1));
            DCS_CHECK(launch(g, T128x32, true, false));
        }
        // B2: dpre = conv2(dg) * r'(pre)  (the F2 form)
        {
            Gemm g = gemm0((int)Rh, kC2, K2);
            g.A = mat(U, Uslot, ax3(w1, h2, kC1, row1, img1), ax2(kC1, 1, row1));
            g.B = mat(param(3), 0, ax1(kC2), ax1(1));
            g.C = mat(dpre, 0, ax1(kC2), ax1(1));
            g.X = mat(pre, 0, ax1(kC2), ax1(1));
            g.epi = EPI_DRELU;
            DCS_CHECK(launch(g, T128x32, true, false));
        }
        // B3: dprez = (dpre . W_11i^T) * r'(prez): split-K over flat
        {
            Gemm g = gemm0(B, kHidden, (int)flat);
            g.A = mat(dpre, 0, ax1(flat), ax1(1));
            g.B = mat(param(8), 0, ax1(1), ax1(flat));
            g.partial = partS; g.splits = splits3; g.kchunk = kchunk3;
            DCS_CHECK(launch(g, T32x32, true, true));
            DCS_CHECK(finish(partS, splits3, kHidden, nullptr, dprez, prez, EPI_DRELU));
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
        // dW1 | db1: dW1i[(ch,j)][c] = sum over the 2 R1 windows (s, b, t, w) of [x; dY][s][b][ch][t][4 w + j] [da1; g][s][b][t][w][c],
        // ones row over the da1 block
        {
            Gemm g = gemm0(kKW + 1, kC1, (int)(2 * R1));
            g.A = mat(xy, 0, ax2(kK1, 1, (int64_t)tc * F), ax3(w1, tc, kS1, F, (int64_t)kCh * tc * F));
            g.B = mat(GA, 0, ax1(kC1), ax1(1));
            g.ones_row = kKW; g.ones_klim = (int)R1;
            g.partial = part1; g.splits = splits1; g.kchunk = kchunk1;
            DCS_CHECK(launch(g, T32x32, false, false));
        }
        // dW2 | db2: dW2i[(dh,c)][o] = sum_{(s,b,h,w)} U[s][b][h+dh][w][c] V[s][b][h+kh-1][w][o], ones row over da2
        {
            Gemm g = gemm0(K2 + 1, kC2, (int)(2 * Rh));
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
        // dW_11 | db_11 = [z^T; 1] . dpre -> grads (W_11 and b_11 are adjacent)
        {
            Gemm g = gemm0(kHidden + 1, (int)flat, B);
            g.A = mat(z, 0, ax1(1), ax1(kHidden));
            g.B = mat(dpre, 0, ax1(flat), ax1(1));
            g.C = mat(grad + off[8], 0, ax1(flat), ax1(1));
            g.ones_row = kHidden; g.ones_klim = B;
            g.scale = sign;
            DCS_CHECK(launch(g, T64x64, false, false));
        }
        {
            Reduce r;
            memset(&r, 0, sizeof(r));
            r.scale = sign;
            r.part[0] = part1; r.dst[0] = grad + off[0]; r.count[0] = (int64_t)(kKW + 1) * kC1; r.splits[0] = splits1;
            r.part[1] = part2; r.dst[1] = grad + off[3]; r.count[1] = (int64_t)(K2 + 1) * kC2; r.splits[1] = splits2;
            r.N[0] = r.N[1] = kC1;
            r.dup[0] = r.dup[1] = 1;
            DCS_CHECK(reduce(r));
        }
        return DCS_OK;
    }

    // pkl: the caller's 17 (full) or 11 arrays.  The stepped arrays go through the layout kernel; the dead ones of the 17-array
    // graph are copied into `dead` at create and served from there: the parameters as given, zeros for the three other
    // sections (their gradient is exactly zero, so Adadelta never moves them or its two accumulators).
    int layout(float* flat_d, float* const* pkl, int to_internal) override {
        float* live[kNstate];
        for (int i = 0; i < 10; ++i) live[i] = pkl[i];
        live[10] = pkl[full ? 16 : 10];
        DCS_CHECK(run_layout(flat_d, live, to_internal, SiMap{kh, h2, w1}));
        if (!full) return DCS_OK;
        const int which = (int)((flat_d - state) / (4 * P4));
        const int64_t wsz = kHidden * flat;
        int64_t at = 0;
        for (int i = 10; i <= 16; ++i) {
            float* p = i < 16 ? pkl[i] : pkl[16] + kCh;
            const int64_t n = i == 16 ? (int64_t)kCh * (kBranches - 1) : (i % 2 == 0 ? wsz : flat);
            hipError_t e;
            if (to_internal) e = hipMemcpyAsync(dead + at, p, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream);
            else if (which == 0) e = hipMemcpyAsync(p, dead + at, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream);
            else e = hipMemsetAsync(p, 0, n * sizeof(float), ctx->stream);
            DCS_HIP(e);
            at += n;
        }
        return DCS_OK;
    }
};

}  // namespace

int bach10si_trainer_new(int arch, int time_context, int F, int batch, dcs_trainer** out) {
    if (time_context < 2 || time_context > kMaxTc || F < kK1 || F > 2049 || batch < 1 || batch > 1024)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: score-informed Bach10 graph: time_context %d (2 .. %d), F %d (30 .. 2049), "
                 "batch %d (1 .. 1024)", time_context, kMaxTc, F, batch);
    const int64_t kh = 2 * time_context / 3, w1 = (F - kK1) / kS1 + 1, h2 = time_context - kh + 1, flat = kC2 * h2 * w1;
    const int64_t R1 = (int64_t)batch * time_context * w1, Rh = (int64_t)batch * h2 * w1;
    // the Bach10 graph's check: every GEMM index (a row, a column or a K position, Ax) stays below kBig
    const int64_t most = std::max({(kSrc + 1) * R1, (kSrc + 1) * Rh, kSrc * flat, flat + 1, (int64_t)batch * flat});
    if (most >= kBig)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: score-informed Bach10 graph: a GEMM index of %lld at time_context %d, F %d, "
                 "batch %d", (long long)most, time_context, F, batch);
    SiTrainer* t = new SiTrainer();
    t->full = arch == DCS_ARCH_BACH10_SI;
    t->kh = (int)kh; t->w1 = (int)w1; t->h2 = (int)h2;
    t->hp = t->h2 + 2 * (t->kh - 1);
    t->K2 = t->kh * kC1;
    t->R1 = R1;
    t->Rh = Rh;
    t->flat = flat;
    t->nsrc = kSrc;
    t->loss_sums = kLossSums;
    t->ndead = (kBranches - 1) * (kHidden * flat + flat) + kCh * (kBranches - 1);
    const int64_t head[10][4] = {{kC1, kCh, 1, kK1}, {kC1, 1, 1, 1}, {kC1, 1, 1, 1}, {kC2, kC1, kh, 1}, {kC2, 1, 1, 1},
                                 {kC2, 1, 1, 1}, {flat, kHidden, 1, 1}, {kHidden, 1, 1, 1}, {kHidden, flat, 1, 1},
                                 {flat, 1, 1, 1}};
    memcpy(t->shapes, head, sizeof(head));
    int n = 10;
    if (t->full)
        for (int k = 1; k < kBranches; ++k) {
            const int64_t w[4] = {kHidden, flat, 1, 1}, b[4] = {flat, 1, 1, 1};
            memcpy(t->shapes[n++], w, sizeof(w));
            memcpy(t->shapes[n++], b, sizeof(b));
        }
    const int64_t bo[4] = {t->full ? kCh * kBranches : kCh, 1, 1, 1};
    memcpy(t->shapes[n++], bo, sizeof(bo));
    t->nparams = n;
    t->nstate = kNstate;
    for (int i = 0; i < 10; ++i) t->state_size[i] = head[i][0] * head[i][1] * head[i][2] * head[i][3];
    t->state_size[10] = kCh;
    *out = t;
    return DCS_OK;
}

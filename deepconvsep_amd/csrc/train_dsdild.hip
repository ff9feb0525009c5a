// Training of the stereo (ILD) DSD100 graph (examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100.py: build_ca :66-113, stage-1 loss
// :183-198, ILD term :210-228, adadelta :202 and :267) on gfx950.  The DSD graph widened: two input channels, conv1 50 x
// (1 x F) over both, conv2 50 x (tc/2 x 1), each + BiasLayer, dense 256, four rectified dense layers, per source the
// InverseLayers of conv2 and conv1 (two output channels each), BiasLayer(8) and rectify.  Output channel 2 s + c is source s
// in input channel c (:106-111).
//
// One step on the ctx stream, no host synchronisation and no float atomics (two runs give bit-identical weights):
//
//   forward   F1 a1b = x . W1 + b1 + b1b                gemm 64x64  K = (c, f) = 2 F over x [B][2][tc][F] in place
//             F2 a2b = conv2(a1b) + b2 + b2b            gemm 64x64  implicit GEMM over the tc/2 taps
//             F3 z = rectify(a2b . Wfc + bfc)           gemm 32x32 split-K over the map, finish (saved: z, pre-activation)
//             F4 d_s = rectify(z . W_s + b_s), s < 4    gemm, 4 batches, into the row-padded V (saved: pre-activations)
//             F5 g_s = conv2^T(d_s)                     gemm 64x64, 4 batches, implicit GEMM over V
//             F6 q[2 s + c] = conv1^T(g_s)[c] + bo      gemm 64x64, one launch per input channel c, 4 batches each
//   loss      stage 1: ild_loss_kernel (masks, the eight errors, dE/dq per element, per-workgroup f64 sums), ild_reduce_kernel
//             stage 2: ild_bin_kernel (per-bin f64 sums of the two level differences over chunks of the B 4 tc rows),
//                      ild_mean_kernel (the chunks in fixed order -> mean_est - mean_gt per bin), then the two kernels of
//                      stage 1, the first folding the ILD term's gradient into dE/dq, the second adding the term to the loss
//   backward  B1 dg_s = dY_s . W1       B2 dpre_s = conv2(dg_s) * r'(pre_s)    B3 dprez = (sum_s dpre_s . W_s^T) * r'(prez)
//             B4 da2 = dprez . Wfc^T    B5 da1 = conv2^T(da2)
//   weights   dW1|db1 = [x; dY_s]^T . [da1; g_s]               split-K (K = 5 B tc), fixed-order reduce
//             dW2|db2 = windows of [a1b; dg_s]^T . [da2; d_s]   split-K (K = 5 B h2), fixed-order reduce
//             dWfc|dbfc = a2b^T . dprez,  dW_s|db_s = z^T . dpre_s
//             every bias gradient is the "ones" row of its weight GEMM; b1b / b2b get copies of b1 / b2 (identical in Theano)
//   update    train::adadelta_kernel
//
// The loss is |E_0| + |E_1| (+ w |I|): E_j the squared error of input channel j, I the squared difference of the per-bin
// mean level differences.  Every term is a sum of squares, so its sign is 0 or 1, and a term whose sign is 0 has a gradient
// that is 0 everywhere (every 2 (source - target), every 2 (mean_est - mean_gt) is 0).  The sign of the total, which the
// gradient epilogues multiply by like sign(E) in the other graphs, therefore equals each term's own sign wherever that term's
// gradient is not zero (Theano's abs'(0) = 0).
//
// Where all four outputs of a channel are zero and the draw is zero the reference divides 0 by 0, and where a level
// ratio is 0 it takes log 0: so do these kernels; the NaN / inf is kept.
//
// Internal parameter layouts (the flat buffer; dcs_trainer_get / _create convert to and from the .pkl layout):
//   W1 [(c,f)][50]: W1i[c F + f][o] = W1[o,c,0,F-1-f]  (flip_filters=True)    W2 [kh][50 c][50 o]: W2i[j][c][o] = W2[o,c,j,0]
//   Wfc [(h,o)][256] and W_s [256][(h,o)], b_s [(h,o)]: the 50 x h2 map in (row h, channel o) order, .pkl order is o*h2+h
// Activations are channels-last: a1b / dg / g / da1 [B][tc][50], a2b / d_s [B][h2][50]; d_s and da2 live in a buffer padded
// by kh-1 zero rows on either side so that conv2^T is a plain implicit GEMM.
#include "train_core.h"

using namespace train;

namespace {

constexpr int kNf = 50, kHidden = 256, kNparams = 17, kSrc = 4, kCh = 2, kOutCh = kSrc * kCh;
constexpr int kLossSums = 2 * kOutCh;            // the eight errors (mic 0's four sources, then mic 1's), eight dbo sums
constexpr int kBinLanes = 64, kBinRows = kThreads / kBinLanes;

struct ILoss {
    const float* q;       // [B][8][tc F] pre-activations of the output layer
    const float* x;       // [B][2][tc F] inputs
    const float* tgt;     // [B][8][tc F] targets
    const float* r1;      // [B][4][tc F] the first normal draw (:164)
    const float* r2;      // [B][4][tc F] the second (:210)
    const double* diff;   // [F] mean_est - mean_gt of stage 2; null in stage 1
    float* xy;            // [5][B][2][tc F]: slot 0 <- x, slots 1 .. 4 <- dE/dq of source s (both channels)
    double* part;         // [gridDim.x][kLossSums]
    int64_t plane, n;     // tc F, B tc F
    int F;
    double eps;
    double cild;          // ild_weight 2 / (4 B tc) 20 / ln 10
};

// :183-198 for the element (b, t, f), in f64: p = rectify(q), S_j = sum_s p[2 s + j], D_js = S_j + eps r1_s,
// source_js = p_js / D_js x_j + eps r1_s; out: p, D, src and the eps r1_s
__device__ __forceinline__ void ild_sources(const ILoss& a, int64_t b, int64_t rem, double (&q)[kCh][kSrc],
                                            double (&p)[kCh][kSrc], double (&D)[kCh][kSrc], double (&src)[kCh][kSrc],
                                            double (&x)[kCh]) {
    double er[kSrc];
#pragma unroll
    for (int s = 0; s < kSrc; ++s) er[s] = a.eps * (double)a.r1[(b * kSrc + s) * a.plane + rem];
#pragma unroll
    for (int j = 0; j < kCh; ++j) {
        x[j] = a.x[(b * kCh + j) * a.plane + rem];
        double S = 0.0;
#pragma unroll
        for (int s = 0; s < kSrc; ++s) {
            q[j][s] = a.q[(b * kOutCh + 2 * s + j) * a.plane + rem];
            p[j][s] = q[j][s] > 0.0 ? q[j][s] : 0.0;
            S += p[j][s];
        }
#pragma unroll
        for (int s = 0; s < kSrc; ++s) {
            D[j][s] = S + er[s];
            src[j][s] = p[j][s] / D[j][s] * x[j] + er[s];
        }
    }
}

// One thread per (b, t, f), all four sources and both channels.  G_js = dE/dsource_js = 2 (source_js - target_js), in stage 2
// plus the ILD term's: with d = source_1s + eps r2, u = source_0s / d + eps r2 and h = cild diff[f] sgn(u) / |u| (the
// derivative of 20 log10 |u| times the mean's and the square's), G_0s += h / d and G_1s -= h source_0s / d^2.
// dE/dp_jk = x_j (G_jk / D_jk - sum_s p_js G_js / D_js^2); dE/dq = dE/dp r'(q), r'(0) = 0.5.
__global__ __launch_bounds__(kThreads) void ild_loss_kernel(const ILoss a) {
    double acc[kLossSums];
#pragma unroll
    for (int i = 0; i < kLossSums; ++i) acc[i] = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < a.n; e += (int64_t)gridDim.x * kThreads) {
        const int64_t b = e / a.plane, rem = e - b * a.plane;
        double q[kCh][kSrc], p[kCh][kSrc], D[kCh][kSrc], src[kCh][kSrc], x[kCh], G[kCh][kSrc];
        ild_sources(a, b, rem, q, p, D, src, x);
#pragma unroll
        for (int j = 0; j < kCh; ++j)
#pragma unroll
            for (int s = 0; s < kSrc; ++s) {
                const double err = src[j][s] - (double)a.tgt[(b * kOutCh + 2 * s + j) * a.plane + rem];
                acc[kSrc * j + s] += err * err;
                G[j][s] = 2.0 * err;
            }
        if (a.diff) {
            const double c = a.cild * a.diff[rem % a.F];
#pragma unroll
            for (int s = 0; s < kSrc; ++s) {
                const double er2 = a.eps * (double)a.r2[(b * kSrc + s) * a.plane + rem];
                const double d = src[1][s] + er2;
                const double u = src[0][s] / d + er2;
                const double sg = u > 0.0 ? 1.0 : (u < 0.0 ? -1.0 : 0.0);
                const double h = c * sg / fabs(u);
                G[0][s] += h / d;
                G[1][s] -= h * src[0][s] / (d * d);
            }
        }
#pragma unroll
        for (int j = 0; j < kCh; ++j) {
            double W = 0.0;
#pragma unroll
            for (int s = 0; s < kSrc; ++s) W += p[j][s] * G[j][s] / (D[j][s] * D[j][s]);
            const int64_t o = (b * kCh + j) * a.plane + rem;
#pragma unroll
            for (int s = 0; s < kSrc; ++s) {
                const double rd = q[j][s] > 0.0 ? 1.0 : (q[j][s] == 0.0 ? 0.5 : 0.0);
                const double dq = x[j] * (G[j][s] / D[j][s] - W) * rd;
                acc[kOutCh + 2 * s + j] += dq;
                a.xy[(s + 1) * kCh * a.n + o] = (float)dq;
            }
            a.xy[o] = (float)x[j];
        }
    }
    block_sums(acc, a.part);
}

// Stage 2, first pass (:214-224): a_est = 20 log10 |source_0 / (source_1 + eps r2) + eps r2| and a_gt, the same on the
// targets, summed per bin over a chunk of the B 4 tc rows (b, s, t).  A workgroup is 64 bins x 4 row lanes; a lane takes
// the rows first + lane + 4 i in order, the four lanes are added in lane order: bin[chunk][2][F].
__global__ __launch_bounds__(kThreads) void ild_bin_kernel(const ILoss a, double* __restrict__ bin, int rows, int per_chunk,
                                                           int tc) {
    __shared__ double red[2][kBinRows][kBinLanes];
    const int fl = threadIdx.x % kBinLanes, rl = threadIdx.x / kBinLanes;
    const int f = blockIdx.x * kBinLanes + fl;
    const int first = blockIdx.y * per_chunk, last = min(rows, first + per_chunk);
    double se = 0.0, sg = 0.0;
    if (f < a.F)
        for (int r = first + rl; r < last; r += kBinRows) {
            const int t = r % tc, bs = r / tc, s = bs % kSrc;
            const int64_t b = bs / kSrc, rem = (int64_t)t * a.F + f;
            const double er1 = a.eps * (double)a.r1[(b * kSrc + s) * a.plane + rem];
            const double er2 = a.eps * (double)a.r2[(b * kSrc + s) * a.plane + rem];
            double src[kCh], tg[kCh];
#pragma unroll
            for (int j = 0; j < kCh; ++j) {
                double S = 0.0, ps = 0.0;
#pragma unroll
                for (int k = 0; k < kSrc; ++k) {
                    const double qk = a.q[(b * kOutCh + 2 * k + j) * a.plane + rem];
                    const double pk = qk > 0.0 ? qk : 0.0;
                    S += pk;
                    if (k == s) ps = pk;
                }
                src[j] = ps / (S + er1) * (double)a.x[(b * kCh + j) * a.plane + rem] + er1;
                tg[j] = a.tgt[(b * kOutCh + 2 * s + j) * a.plane + rem];
            }
            se += 20.0 * log10(fabs(src[0] / (src[1] + er2) + er2));
            sg += 20.0 * log10(fabs(tg[0] / (tg[1] + er2) + er2));
        }
    red[0][rl][fl] = se;
    red[1][rl][fl] = sg;
    __syncthreads();
    if (rl == 0 && f < a.F)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            double v = red[i][0][fl];
#pragma unroll
            for (int k = 1; k < kBinRows; ++k) v += red[i][k][fl];
            bin[((int64_t)blockIdx.y * 2 + i) * a.F + f] = v;
        }
}

// the chunks -> diff[f] = mean_est[f] - mean_gt[f].  A workgroup is 32 bins x 8 lanes; a lane adds its contiguous eighth
// of the chunks in order, the eight lanes are added in lane order.
constexpr int kMeanBins = 32, kMeanLanes = kThreads / kMeanBins;

__global__ __launch_bounds__(kThreads) void ild_mean_kernel(const double* __restrict__ bin, int chunks, int F, double rows,
                                                            double* __restrict__ diff) {
    __shared__ double red[2][kMeanLanes][kMeanBins];
    const int fl = threadIdx.x % kMeanBins, cl = threadIdx.x / kMeanBins;
    const int f = blockIdx.x * kMeanBins + fl;
    const int per = (chunks + kMeanLanes - 1) / kMeanLanes;
    const int first = cl * per, last = min(chunks, first + per);
    double se = 0.0, sg = 0.0;
    if (f < F)
        for (int c = first; c < last; ++c) {
            se += bin[((int64_t)c * 2) * F + f];
            sg += bin[((int64_t)c * 2 + 1) * F + f];
        }
    red[0][cl][fl] = se;
    red[1][cl][fl] = sg;
    __syncthreads();
    if (cl == 0 && f < F) {
        se = red[0][0][fl];
        sg = red[1][0][fl];
#pragma unroll
        for (int k = 1; k < kMeanLanes; ++k) {
            se += red[0][k][fl];
            sg += red[1][k][fl];
        }
        diff[f] = se / rows - sg / rows;
    }
}

// The workgroups' sums and the bins' squared differences in fixed order -> out16 = (loss, |errors| of mic 0's four
// sources then mic 1's, the weighted ILD term, zeros), the sign of the loss for the gradient epilogues (abs'(0) = 0), the
// output-bias gradient.
__global__ __launch_bounds__(kThreads) void ild_reduce_kernel(const double* __restrict__ part, int nblk,
                                                              const double* __restrict__ diff, int F, double weight,
                                                              double* out16, float* sign, float* dbo) {
    constexpr int NS = kLossSums + 1;
    __shared__ double red[NS][kThreads];
    for (int i = 0; i < kLossSums; ++i) {
        double s = 0.0;
        for (int b = threadIdx.x; b < nblk; b += kThreads) s += part[(int64_t)b * kLossSums + i];
        red[i][threadIdx.x] = s;
    }
    {
        double s = 0.0;
        if (diff)
            for (int f = threadIdx.x; f < F; f += kThreads) s += diff[f] * diff[f];
        red[kLossSums][threadIdx.x] = s;
    }
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w)
            for (int i = 0; i < NS; ++i) red[i][threadIdx.x] += red[i][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double E[kCh];
        for (int j = 0; j < kCh; ++j) {
            E[j] = 0.0;
            for (int s = 0; s < kSrc; ++s) E[j] += red[kSrc * j + s][0];
        }
        const double ild = diff ? weight * fabs(red[kLossSums][0]) : 0.0;
        const double loss = fabs(E[0]) + fabs(E[1]) + ild;
        const float sg = loss > 0.0 ? 1.f : (loss < 0.0 ? -1.f : 0.f);
        out16[0] = loss;
        for (int i = 0; i < kOutCh; ++i) out16[1 + i] = fabs(red[i][0]);
        out16[1 + kOutCh] = ild;
        for (int i = 2 + kOutCh; i < 16; ++i) out16[i] = 0.0;
        *sign = sg;
        for (int j = 0; j < kOutCh; ++j) dbo[j] = sg * (float)red[kOutCh + j][0];
    }
}

// the .pkl index of element k of the internal section s
struct IldMap {
    int F, kh, h2;
    __device__ int64_t operator()(int s, int64_t k) const {
        const int64_t map = kNf * (int64_t)h2;
        if (s == 0) {                                     // W1i[c F + f][o] = W1[o][c][F-1-f]
            const int64_t row = k / kNf, o = k % kNf;
            const int64_t c = row / F, f = row % F;
            return (o * kCh + c) * F + (F - 1 - f);
        } else if (s == 3) {                              // W2i[j][c][o] = W2[o][c][j]
            const int64_t j = k / (kNf * kNf), c = (k / kNf) % kNf, o = k % kNf;
            return (o * kNf + c) * kh + j;
        } else if (s == 6) {                              // Wfc rows (h, o) <- o h2 + h
            const int64_t row = k / kHidden, n = k % kHidden;
            return ((row % kNf) * h2 + row / kNf) * kHidden + n;
        } else if (s >= 8 && s < 16 && s % 2 == 0) {      // W_s columns (h, o) <- o h2 + h
            const int64_t n = k / map, col = k % map;
            return n * map + (col % kNf) * h2 + col / kNf;
        } else if (s >= 9 && s < 16) {
            return (k % kNf) * h2 + k / kNf;
        }
        return k;
    }
};

struct IldTrainer : dcs_trainer {
    int kh = 0, h2 = 0, hp = 0;
    int64_t R = 0, Rh = 0, map = 0;
    // views into work; bin and diff hold doubles (two floats each; every view starts on a multiple of 64 floats)
    float *xy, *U, *GA, *V, *a2b, *z, *prez, *dprez, *pre, *dpre, *part1, *part2, *partS, *bin, *diff;
    int splits1 = 1, splits2 = 1, splits3 = 1, splitsB3 = 1, kchunk1 = 0, kchunk2 = 0, kchunk3 = 0, kchunkB3 = 0;
    int bin_chunks = 1, bin_per_chunk = 1;

    void plan(std::vector<std::pair<float**, int64_t>>& parts) override {
        // about 2 workgroups per CU, at most 64 slices (the DSD graph's choices); F3 / B3: the Bach10 graph's
        pick_split(dcs_cdiv(kCh * F + 1, 64), (kSrc + 1) * R, &splits1, &kchunk1, 512, 64);
        pick_split(dcs_cdiv(kh * kNf + 1, 64), (kSrc + 1) * Rh, &splits2, &kchunk2, 512, 64);
        pick_split((int64_t)dcs_cdiv(B, 32) * (kHidden / 32), map, &splits3, &kchunk3, 512, 128);
        pick_split((int64_t)dcs_cdiv(B, 32) * (kHidden / 32), kSrc * map, &splitsB3, &kchunkB3, 512, 128);
        // the per-bin sums: about kLossBlocks workgroups of 64 bins, a chunk at least kBinRows rows
        const int64_t rows = kSrc * R, fblocks = dcs_cdiv(F, kBinLanes);
        int64_t chunks = std::max<int64_t>(1, kLossBlocks / fblocks);
        chunks = std::min<int64_t>(chunks, dcs_cdiv(rows, kBinRows));
        bin_per_chunk = (int)dcs_cdiv(rows, chunks);
        bin_chunks = (int)dcs_cdiv(rows, bin_per_chunk);
        const int64_t b = B, n5 = kSrc + 1;
        parts.insert(parts.end(), {{&xy, n5 * kCh * RF}, {&U, n5 * R * kNf}, {&GA, n5 * R * kNf}, {&V, n5 * b * hp * kNf},
                                   {&Q, kOutCh * RF}, {&a2b, b * map}, {&z, b * kHidden}, {&prez, b * kHidden},
                                   {&dprez, b * kHidden}, {&pre, kSrc * b * map}, {&dpre, kSrc * b * map},
                                   {&part1, (int64_t)splits1 * (kCh * F + 1) * kNf},
                                   {&part2, (int64_t)splits2 * (kh * kNf + 1) * kNf},
                                   {&partS, (int64_t)std::max(splits3, splitsB3) * b * kHidden},
                                   {&bin, 2 * (int64_t)bin_chunks * 2 * F}, {&diff, 2 * (int64_t)F}});
    }

    int forward(const float* x) override {
        const int64_t padrow = (int64_t)(kh - 1) * kNf, Vslot = (int64_t)B * hp * kNf;
        const int64_t R50 = R * kNf, plane = (int64_t)tc * F, wstep = off[10] - off[8];
        // F1: a1b[(b,t)][o] = sum_{c,f} x[b][c][t][f] W1i[c F + f][o] + b1 + b1b -> U slot 0
        {
            Gemm g = gemm0((int)R, kNf, kCh * F);
            g.A = mat((float*)x, 0, ax2(tc, F, kCh * plane), ax2(F, 1, plane));
            g.B = mat(param(0), 0, ax1(kNf), ax1(1));
            g.C = mat(U, 0, ax1(kNf), ax1(1));
            g.bias = param(1); g.bias2 = param(2);
            DCS_CHECK(launch(g, T64x64, true, false));
        }
        // F2: a2b[(b,h)][o] = sum_{k',c} a1b[b][h+k'][c] W2i[kh-1-k'][c][o] + b2 + b2b
        {
            Gemm g = gemm0((int)Rh, kNf, kh * kNf);
            g.A = mat(U, 0, ax2(h2, kNf, (int64_t)tc * kNf), ax1(1));
            g.B = mat(param(3), (int64_t)(kh - 1) * kNf * kNf, ax2(kNf, kNf, -(int64_t)kNf * kNf), ax1(1));
            g.C = mat(a2b, 0, ax1(kNf), ax1(1));
            g.bias = param(4); g.bias2 = param(5);
            DCS_CHECK(launch(g, T64x64, true, false));
        }
        // F3: z = rectify(a2b . Wfci + bfc), pre-activation saved: split-K over the map, then the fixed-order sum
        {
            Gemm g = gemm0(B, kHidden, (int)map);
            g.A = mat(a2b, 0, ax1(map), ax1(1));
            g.B = mat(param(6), 0, ax1(kHidden), ax1(1));
            g.partial = partS; g.splits = splits3; g.kchunk = kchunk3;
            DCS_CHECK(launch(g, T32x32, true, false));
            DCS_CHECK(finish(partS, splits3, kHidden, param(7), z, prez, EPI_RELU | EPI_SAVEPRE));
        }
        // F4: d_s = rectify(z . W_si + b_si) -> V slots 1 .. 4 (padded rows), pre-activations saved
        {
            Gemm g = gemm0(B, (int)map, kHidden);
            g.A = mat(z, 0, ax1(kHidden), ax1(1));
            g.B = mat(param(8), 0, ax1(map), ax1(1));
            g.C = mat(V, padrow, ax1((int64_t)hp * kNf), ax1(1));
            g.X = mat(pre, 0, ax1(map), ax1(1));
            g.bias = param(9);
            g.epi = EPI_RELU | EPI_SAVEPRE;
            g.nbatch = kSrc;
            for (int k = 0; k < kSrc; ++k) {
                g.boff[k][1] = k * wstep;
                g.boff[k][2] = (k + 1) * Vslot;
                g.boff[k][3] = k * (int64_t)B * map;
                g.boff[k][4] = k * wstep;
            }
            DCS_CHECK(launch(g, rows_tile(B), true, false));
        }
        // F5: g_s[(b,t)][c] = sum_{j,o} Vpad[b][t+j][o] W2i[j][c][o] -> GA slots 1 .. 4
        {
            Gemm g = gemm0((int)R, kNf, kh * kNf);
            g.A = mat(V, 0, ax2(tc, kNf, (int64_t)hp * kNf), ax1(1));
            g.B = mat(param(3), 0, ax2(kNf, 1, (int64_t)kNf * kNf), ax1(kNf));
            g.C = mat(GA, 0, ax1(kNf), ax1(1));
            g.nbatch = kSrc;
            for (int k = 0; k < kSrc; ++k) {
                g.boff[k][0] = (k + 1) * Vslot;
                g.boff[k][2] = (k + 1) * R50;
            }
            DCS_CHECK(launch(g, T64x64, true, true));
        }
        // F6: q[b][2 s + c][t][f] = sum_o g_s[(b,t)][o] W1i[c F + f][o] + bo[2 s + c]: per input channel c, four batches s
        for (int c = 0; c < kCh; ++c) {
            Gemm g = gemm0((int)R, F, kNf);
            g.A = mat(GA, 0, ax1(kNf), ax1(1));
            g.B = mat(param(0), (int64_t)c * F * kNf, ax1(1), ax1(kNf));
            g.C = mat(Q, 0, ax2(tc, F, kOutCh * plane), ax1(1));
            g.bias = param(16);
            g.bias_cs = 0;
            g.nbatch = kSrc;
            for (int s = 0; s < kSrc; ++s) {
                g.boff[s][0] = (s + 1) * R50;
                g.boff[s][2] = (2 * s + c) * plane;
                g.boff[s][4] = 2 * s + c;
            }
            DCS_CHECK(launch(g, T64x64, true, true));
        }
        return DCS_OK;
    }

    int loss(const float* x, const float* tgt, double* out_d) override {
        const int64_t rows = kSrc * R;
        ILoss a;
        a.q = Q; a.x = x; a.tgt = tgt; a.r1 = rnd; a.r2 = rnd + kSrc * RF; a.xy = xy; a.part = lpart;
        a.diff = stage2 ? (const double*)diff : nullptr;
        a.plane = (int64_t)tc * F;
        a.n = RF;
        a.F = F;
        a.eps = hyp[0];
        a.cild = hyp[1] * 2.0 / (double)rows * 20.0 / log(10.0);
        if (stage2) {
            hipLaunchKernelGGL(ild_bin_kernel, dim3((unsigned)dcs_cdiv(F, kBinLanes), (unsigned)bin_chunks), dim3(kThreads), 0,
                               ctx->stream, a, (double*)bin, (int)rows, bin_per_chunk, tc);
            DCS_HIP(hipGetLastError());
            hipLaunchKernelGGL(ild_mean_kernel, dim3((unsigned)dcs_cdiv(F, kMeanBins)), dim3(kThreads), 0, ctx->stream,
                               (const double*)bin, bin_chunks, F, (double)rows, (double*)diff);
            DCS_HIP(hipGetLastError());
        }
        const int nblk = (int)std::min<int64_t>(kLossBlocks, dcs_cdiv(a.n, kThreads));
        hipLaunchKernelGGL(ild_loss_kernel, dim3(nblk), dim3(kThreads), 0, ctx->stream, a);
        DCS_HIP(hipGetLastError());
        hipLaunchKernelGGL(ild_reduce_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, (const double*)lpart, nblk, a.diff, F,
                           hyp[1], out_d ? out_d : out7, sign, grad() + off[16]);
        DCS_HIP(hipGetLastError());
        return DCS_OK;
    }

    int backward() override {
        const int64_t padrow = (int64_t)(kh - 1) * kNf, Vslot = (int64_t)B * hp * kNf;
        const int64_t R50 = R * kNf, Bmap = (int64_t)B * map, wstep = off[10] - off[8];
        const int64_t plane = (int64_t)tc * F, slot = kCh * RF;
        float* grad = this->grad();
        // B1: dg_s = dY_s . W1i -> U slots 1 .. 4  (the F1 form)
        {
            Gemm g = gemm0((int)R, kNf, kCh * F);
            g.A = mat(xy, 0, ax2(tc, F, kCh * plane), ax2(F, 1, plane));
            g.B = mat(param(0), 0, ax1(kNf), ax1(1));
            g.C = mat(U, 0, ax1(kNf), ax1(1));
            g.nbatch = kSrc;
            for (int k = 0; k < kSrc; ++k) {
                g.boff[k][0] = (k + 1) * slot;
                g.boff[k][2] = (k + 1) * R50;
            }
            DCS_CHECK(launch(g, T64x64, true, false));
        }
        // B2: dpre_s = conv2(dg_s) * r'(pre_s)  (the F2 form)
        {
            Gemm g = gemm0((int)Rh, kNf, kh * kNf);
            g.A = mat(U, 0, ax2(h2, kNf, (int64_t)tc * kNf), ax1(1));
            g.B = mat(param(3), (int64_t)(kh - 1) * kNf * kNf, ax2(kNf, kNf, -(int64_t)kNf * kNf), ax1(1));
            g.C = mat(dpre, 0, ax1(kNf), ax1(1));
            g.X = mat(pre, 0, ax1(kNf), ax1(1));
            g.epi = EPI_DRELU;
            g.nbatch = kSrc;
            for (int k = 0; k < kSrc; ++k) {
                g.boff[k][0] = (k + 1) * R50;
                g.boff[k][2] = k * Bmap;
                g.boff[k][3] = k * Bmap;
            }
            DCS_CHECK(launch(g, T64x64, true, false));
        }
        // B3: dprez = (sum_s dpre_s . W_si^T) * r'(prez): K = 4 map, concatenated over s, split-K
        {
            Gemm g = gemm0(B, kHidden, (int)(kSrc * map));
            g.A = mat(dpre, 0, ax1(map), ax2(map, 1, Bmap));
            g.B = mat(param(8), 0, ax2(map, 1, wstep), ax1(map));
            g.partial = partS; g.splits = splitsB3; g.kchunk = kchunkB3;
            DCS_CHECK(launch(g, T32x32, true, true));
            DCS_CHECK(finish(partS, splitsB3, kHidden, nullptr, dprez, prez, EPI_DRELU));
        }
        // B4: da2 = dprez . Wfci^T -> V slot 0 (padded rows)
        {
            Gemm g = gemm0(B, (int)map, kHidden);
            g.A = mat(dprez, 0, ax1(kHidden), ax1(1));
            g.B = mat(param(6), 0, ax1(1), ax1(kHidden));
            g.C = mat(V, padrow, ax1((int64_t)hp * kNf), ax1(1));
            DCS_CHECK(launch(g, rows_tile(B), true, true));
        }
        // B5: da1 = conv2^T(da2) -> GA slot 0  (the F5 form)
        {
            Gemm g = gemm0((int)R, kNf, kh * kNf);
            g.A = mat(V, 0, ax2(tc, kNf, (int64_t)hp * kNf), ax1(1));
            g.B = mat(param(3), 0, ax2(kNf, 1, (int64_t)kNf * kNf), ax1(kNf));
            g.C = mat(GA, 0, ax1(kNf), ax1(1));
            DCS_CHECK(launch(g, T64x64, true, true));
        }
        // dW1 | db1: [x; dY_s]^T [(c,f)][5 R] . [da1; g_s] [5 R][50], ones row over the x block
        {
            Gemm g = gemm0(kCh * F + 1, kNf, (int)((kSrc + 1) * R));
            g.A = mat(xy, 0, ax2(F, 1, plane), ax2(tc, F, kCh * plane));
            g.B = mat(GA, 0, ax1(kNf), ax1(1));
            g.ones_row = kCh * F; g.ones_klim = (int)R;
            g.partial = part1; g.splits = splits1; g.kchunk = kchunk1;
            DCS_CHECK(launch(g, T64x64, false, false));
        }
        // dW2 | db2: dW2i[(j,c)][o] = sum_{(s,b,h)} U[s][b][h+kh-1-j][c] Vpad[s][b][h+kh-1][o], ones row over the da2 block
        {
            Gemm g = gemm0(kh * kNf + 1, kNf, (int)((kSrc + 1) * Rh));
            g.A = mat(U, (int64_t)(kh - 1) * kNf, ax2(kNf, 1, -(int64_t)kNf), ax2(h2, kNf, (int64_t)tc * kNf));
            g.B = mat(V, padrow, ax2(h2, kNf, (int64_t)hp * kNf), ax1(1));
            g.ones_row = kh * kNf; g.ones_klim = (int)Rh;
            g.partial = part2; g.splits = splits2; g.kchunk = kchunk2;
            DCS_CHECK(launch(g, T64x64, false, false));
        }
        // dWfc | dbfc = [a2b^T; 1] . dprez -> grads (Wfc and bfc are adjacent)
        {
            Gemm g = gemm0((int)map + 1, kHidden, B);
            g.A = mat(a2b, 0, ax1(1), ax1(map));
            g.B = mat(dprez, 0, ax1(kHidden), ax1(1));
            g.C = mat(grad + off[6], 0, ax1(kHidden), ax1(1));
            g.ones_row = (int)map; g.ones_klim = B;
            g.scale = sign;
            DCS_CHECK(launch(g, T64x64, false, false));
        }
        // dW_s | db_s = [z^T; 1] . dpre_s -> grads (W_s and b_s are adjacent)
        {
            Gemm g = gemm0(kHidden + 1, (int)map, B);
            g.A = mat(z, 0, ax1(1), ax1(kHidden));
            g.B = mat(dpre, 0, ax1(map), ax1(1));
            g.C = mat(grad + off[8], 0, ax1(map), ax1(1));
            g.ones_row = kHidden; g.ones_klim = B;
            g.scale = sign;
            g.nbatch = kSrc;
            for (int k = 0; k < kSrc; ++k) {
                g.boff[k][1] = k * Bmap;
                g.boff[k][2] = k * wstep;
            }
            DCS_CHECK(launch(g, T64x64, false, false));
        }
        {
            Reduce r;
            memset(&r, 0, sizeof(r));
            r.scale = sign;
            r.part[0] = part1; r.dst[0] = grad + off[0]; r.count[0] = (int64_t)(kCh * F + 1) * kNf; r.splits[0] = splits1;
            r.part[1] = part2; r.dst[1] = grad + off[3]; r.count[1] = (int64_t)(kh * kNf + 1) * kNf;
            r.splits[1] = splits2;
            r.N[0] = r.N[1] = kNf;
            r.dup[0] = r.dup[1] = 1;
            DCS_CHECK(reduce(r));
        }
        return DCS_OK;
    }

    int layout(float* flat, float* const* pkl, int to_internal) override {
        return run_layout(flat, pkl, to_internal, IldMap{F, kh, h2});
    }
};

}  // namespace

int dsdild_trainer_new(int time_context, int F, int batch, dcs_trainer** out) {
    if (time_context < 4 || time_context > 64 || time_context % 2 || F < 1 || F > 2049 || batch < 1 || batch > 1024)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: stereo DSD graph: time_context %d (even, 4 .. 64), F %d (1 .. 2049), batch %d "
                 "(1 .. 1024)", time_context, F, batch);
    IldTrainer* t = new IldTrainer();
    const int kh = time_context / 2, h2 = time_context - kh + 1, map = kNf * h2;
    t->kh = kh; t->h2 = h2;
    t->hp = time_context + kh - 1;
    t->R = (int64_t)batch * time_context;
    t->Rh = (int64_t)batch * h2;
    t->map = map;
    t->nsrc = kOutCh;
    t->nparams = kNparams;
    t->loss_sums = kLossSums;
    t->nout = 16;
    t->rand_planes = 2 * kSrc;
    t->two_stage = true;
    const int64_t s[kNparams][4] = {{kNf, kCh, 1, F}, {kNf, 1, 1, 1}, {kNf, 1, 1, 1}, {kNf, kNf, kh, 1}, {kNf, 1, 1, 1},
                                    {kNf, 1, 1, 1}, {map, kHidden, 1, 1}, {kHidden, 1, 1, 1}, {kHidden, map, 1, 1},
                                    {map, 1, 1, 1}, {kHidden, map, 1, 1}, {map, 1, 1, 1}, {kHidden, map, 1, 1},
                                    {map, 1, 1, 1}, {kHidden, map, 1, 1}, {map, 1, 1, 1}, {kOutCh, 1, 1, 1}};
    memcpy(t->shapes, s, sizeof(s));
    *out = t;
    return DCS_OK;
}

// Training of the stereo (ILD) DSD100 graph (examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100.py: build_ca :66-113, stage-1 loss
// :183-198, ILD term :210-228, adadelta :202 and :267) on gfx950: the full-width build_ca graph of train_dsd_graph.h (the
// step, the GEMMs and the layouts are there) with the description below: two input channels, dense 256, four decoder
// branches, two output channels per source, 17 arrays.  Output channel 2 s + c is source s in input channel c (:106-111).
// F3 / B3 are split-K with a fixed-order finish; operands whose K runs contiguously in memory load K-fastest, and the weight
// GEMMs load A M-fastest (dsdild_trainer_new).
//
//   loss      stage 1: ild_loss_kernel (masks, the eight errors, dE/dq per element, per-workgroup f64 sums), ild_reduce_kernel
//             stage 2: ild_bin_kernel (per-bin f64 sums of the two level differences over chunks of the B 4 tc rows),
//                      ild_mean_kernel (the chunks in fixed order -> mean_est - mean_gt per bin), then the two kernels of
//                      stage 1, the first folding the ILD term's gradient into dE/dq, the second adding the term to the loss
//
// The loss is |E_0| + |E_1| (+ w |I|): E_j the squared error of input channel j, I the squared difference of the per-bin
// mean level differences.  Every term is a sum of squares, so its sign is 0 or 1, and a term whose sign is 0 has a gradient
// that is 0 everywhere (every 2 (source - target), every 2 (mean_est - mean_gt) is 0).  The sign of the total, which the
// gradient epilogues multiply by like sign(E) in the other graphs, therefore equals each term's own sign wherever that term's
// gradient is not zero (Theano's abs'(0) = 0).
//
// Where all four outputs of a channel are zero and the draw is zero the reference divides 0 by 0, and where a level
// ratio is 0 it takes log 0: so do these kernels; the NaN / inf is kept.
#include "train_dsd_graph.h"

using namespace train;

namespace {

constexpr int kSrc = 4, kCh = 2, kOutCh = kSrc * kCh;
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

struct IldTrainer : DsdGraphTrainer {
    // views into work; bin and diff hold doubles (two floats each; every view starts on a multiple of 64 floats)
    float *bin, *diff;
    int bin_chunks = 1, bin_per_chunk = 1;

    void plan(std::vector<std::pair<float**, int64_t>>& parts) override {
        DsdGraphTrainer::plan(parts);
        // the per-bin sums: about kLossBlocks workgroups of 64 bins, a chunk at least kBinRows rows
        const int64_t rows = kSrc * R, fblocks = dcs_cdiv(F, kBinLanes);
        int64_t chunks = std::max<int64_t>(1, kLossBlocks / fblocks);
        chunks = std::min<int64_t>(chunks, dcs_cdiv(rows, kBinRows));
        bin_per_chunk = (int)dcs_cdiv(rows, chunks);
        bin_chunks = (int)dcs_cdiv(rows, bin_per_chunk);
        parts.insert(parts.end(), {{&bin, 2 * (int64_t)bin_chunks * 2 * F}, {&diff, 2 * (int64_t)F}});
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
                           hyp[1], out_d ? out_d : out7, sign, grad() + off[bo()]);
        DCS_HIP(hipGetLastError());
        return DCS_OK;
    }
};

}  // namespace

int dsdild_trainer_new(int time_context, int F, int batch, dcs_trainer** out) {
    DCS_CHECK(DsdGraphTrainer::check_range("stereo DSD graph: ", time_context, F, batch));
    const DsdForm kn = {T64x64, true, false}, kk = {T64x64, true, true}, mn = {T64x64, false, false};
    const Tile rows = rows_tile(batch);
    const DsdDesc desc = {kCh, kSrc, 256, kOutCh, kOutCh, {0, 1, 2, 3}, true,
                          // F1, F2, F3, F4, F5, F6
                          {kn, kn, {T32x32, true, false}, {rows, true, false}, kk, kk,
                           // B1 .. B5
                           kn, kn, {T32x32, true, true}, {rows, true, true}, kk,
                           // dW1, dW2, dWfc, dW_s
                           mn, mn, mn, mn}};
    IldTrainer* t = new IldTrainer();
    t->shape(desc, time_context, F, batch);
    t->loss_sums = kLossSums;
    t->nout = 16;
    t->rand_planes = 2 * kSrc;
    t->two_stage = true;
    *out = t;
    return DCS_OK;
}

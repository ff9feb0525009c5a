// Training of the iKala singing-voice graph (examples/ikala/trainCNN.py: build_ca :66-118, loss :155-189, adadelta :193)
// on gfx950.  conv1 30 x (1 x 30) stride (1, 3) + BiasLayer, conv2 30 x (10 x 20) + BiasLayer, dense 256, two rectified
// dense layers of flat = 30 h2 w2 units, per source the InverseLayers of conv2 and conv1, BiasLayer(2) and rectify: the
// build_ca graph of train_ca.h (the step, the GEMMs and the layouts are there) with the description below, 13 arrays.
//
//   F6        train::deconv1_kernel: 10 taps x 30 channels per output, fixed order
//   loss      ik_loss_kernel: masks, the four components, dE/dq (rectify' with the 0.5 tie), per-workgroup f64 sums
#include "train_ca.h"

using namespace train;

namespace {

constexpr int kS1 = 3, kH2 = 10, kW2 = 20, kSrc = 2;
// dW1: about 2 workgroups per CU; dW2: 47 row tiles of a K of 3 B h2 w2 (288 k at B = 32), 8 workgroups per CU keep the
// SIMDs busy; at most 128 slices each
constexpr CaDesc kIkala = {kS1, 1, kH2, kW2, kSrc, {512, 128}, {2048, 128}};

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

}  // namespace

// F6, the one launch site of this graph's conv1^T instance (train_ca.h)
int train::ikala_deconv1(hipStream_t s, const float* g, int64_t gslot, const float* W1i, const float* bo, float* q, int B,
                         int tc, int F, int w1) {
    const int64_t n = (int64_t)kSrc * B * tc * F;
    hipLaunchKernelGGL((deconv1_kernel<kK1, kC1, kS1, kSrc>), dim3((unsigned)dcs_cdiv(n, kThreads)), dim3(kThreads), 0, s, g,
                       gslot, W1i, bo, q, B, tc, F, w1);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

namespace {

struct IkalaTrainer : CaTrainer {
    int deconv1() override {
        return ikala_deconv1(ctx->stream, GA + Uslot, Uslot, param(0), param(bo()), Q, B, tc, F, w1);
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
        return loss_reduce<IkalaSums>(nblk, out7_d, grad() + off[bo()]);
    }
};

}  // namespace

int ikala_trainer_new(int time_context, int F, int batch, dcs_trainer** out) {
    // no CaTrainer::check_index here, as before: within these ranges every row, column and K position of a GEMM (what Ax
    // decomposes) stays below kBig -- the largest, dW1's K of 3 B tc w1, is 133 M.  B flat, which that check bounds too, is
    // only a 64-bit offset unit; it passes kBig at the far corner (1024, 64, 2049), which this graph has always accepted.
    if (time_context < kH2 || time_context > 64 || F < 87 || F > 2049 || batch < 1 || batch > 1024)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: iKala graph: time_context %d (10 .. 64), F %d (87 .. 2049), batch %d (1 .. 1024)",
                 time_context, F, batch);
    std::unique_ptr<IkalaTrainer> t(new IkalaTrainer());
    t->shape(kIkala, time_context, F, batch, kSrc);
    t->nsrc = kSrc;
    t->loss_sums = kLossSums;
    *out = t.release();
    return DCS_OK;
}

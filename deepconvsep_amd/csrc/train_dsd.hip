// Training of the DSD100 graph (examples/dsd100/trainCNN.py: build_ca :66-130, loss :167-219, adadelta :223) on gfx950: the
// full-width build_ca graph of train_dsd_graph.h (the step, the GEMMs and the layouts are there) with the description below:
// one input channel, dense 128, three live decoder branches, 15 arrays.  Output channel 3 repeats branch 1 (l_fc14 is dead),
// so branch 1 collects the gradients of channels 1 and 3.  Every GEMM is the 64 x 64 form, A loaded K-fastest and B
// N-fastest, and F3 / B3 are one launch each.
//
//   loss      dsd_loss_kernel: masks, the six components, dE/dq (relu' with the 0.5 tie) per element, per-workgroup f64 sums
//             train::loss_reduce_kernel: fixed-order sum -> loss and components (f64), sign(E), the output-bias gradient
#include "train_dsd_graph.h"

using namespace train;

namespace {

// six components, then four output-bias gradient sums; E = vocals + drums + bass - negative - alpha - negative_voc
// (trainCNN.py:217); out7 = (|E|, vocals, bass, drums, negative, alpha, negative_voc)
struct DsdSums {
    static constexpr int kOut = 6, kDbo = 4;
    static __device__ double E(const double* s) { return s[0] + s[2] + s[1] - s[3] - s[4] - s[5]; }
};
constexpr int kLossSums = DsdSums::kOut + DsdSums::kDbo;

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
__global__ __launch_bounds__(kThreads) void dsd_loss_kernel(const TLoss a) {
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
    block_sums(acc, a.part);
}

struct DsdTrainer : DsdGraphTrainer {
    int loss(const float* x, const float* tgt, double* out7_d) override {
        TLoss a;
        a.q = Q; a.x = x; a.tgt = tgt; a.rnd = rnd; a.xy = xy; a.part = lpart;
        a.plane = (int64_t)tc * F;
        a.n = RF;
        a.eps = hyp[0]; a.alpha = hyp[1]; a.beta = hyp[2]; a.beta_voc = hyp[3];
        const int nblk = (int)std::min<int64_t>(kLossBlocks, dcs_cdiv(a.n, kThreads));
        hipLaunchKernelGGL(dsd_loss_kernel, dim3(nblk), dim3(kThreads), 0, ctx->stream, a);
        DCS_HIP(hipGetLastError());
        return loss_reduce<DsdSums>(nblk, out7_d, grad() + off[bo()]);
    }
};

}  // namespace

int dsd_trainer_new(int time_context, int F, int batch, dcs_trainer** out) {
    DCS_CHECK(DsdGraphTrainer::check_range("", time_context, F, batch));
    DsdDesc desc = {1, 3, 128, 4, 4, {0, 1, 2, 1}, false, {}};
    for (DsdForm& f : desc.form) f = {T64x64, true, false};
    DsdTrainer* t = new DsdTrainer();
    t->shape(desc, time_context, F, batch);
    t->loss_sums = kLossSums;
    *out = t;
    return DCS_OK;
}

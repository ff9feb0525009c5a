// Training of the Bach10 graph (examples/bach10/trainCNNbach10.py: build_ca :66-123, loss :160-198, adadelta :202; the same
// graph and loss as trainCNNrwc.py and trainCNNSibelius.py, which differ only in their features) on gfx950.  conv1 30 x
// (1 x 30) stride (1, 4) + BiasLayer, conv2 30 x (kh x 1) with kh = int(2 tc / 3) + BiasLayer, dense 256, four rectified
// dense layers of flat = 30 h2 w1 units, per source the InverseLayers of conv2 and conv1, BiasLayer(4) and rectify: the
// build_ca graph of train_ca.h (the step, the GEMMs and the layouts are there) with the description below, 17 arrays.  With
// kw = 1 the map is as wide as conv1's output, V is padded in rows only and the live rows of a V image are contiguous.
//
//   F6        train::deconv1_kernel: 8 taps x 30 channels per output, fixed order
//   loss      train::mask_loss_kernel<1>: masks, the four errors, dE/dq (rectify' with the 0.5 tie), per-workgroup f64 sums
//
// The loss divides by D = p1 + p2 + p3 + p4 + eps r (eps r in the denominator only, trainCNNbach10.py:178-181).  Where the
// four outputs are all zero and r = 0 the reference divides 0 by 0; so does the kernel: the NaN is kept, there is no guard.
#include "train_ca.h"

using namespace train;

namespace {

constexpr int kS1 = 4, kSrc = 4;
constexpr int kMaxTc = 47;                       // the largest time context dcs_model_create's bach10 graph runs

// four errors, then four output-bias gradient sums; E = error1 + error2 + error3 + error4 (trainCNNbach10.py:198);
// out7 = (|E|, error1, error2, error3, error4, 0, 0)
struct Bach10Sums {
    static constexpr int kOut = 4, kDbo = 4;
    static __device__ double E(const double* s) { return s[0] + s[1] + s[2] + s[3]; }
};
constexpr int kLossSums = Bach10Sums::kOut + Bach10Sums::kDbo;

}  // namespace

// F6, the one launch site of this graph's conv1^T instance (train_ca.h)
int train::bach10_deconv1(hipStream_t s, const float* g, int64_t gslot, const float* W1i, const float* bo, float* q, int B,
                          int tc, int F, int w1) {
    const int64_t n = (int64_t)kSrc * B * tc * F;
    hipLaunchKernelGGL((deconv1_kernel<kK1, kC1, kS1, kSrc>), dim3((unsigned)dcs_cdiv(n, kThreads)), dim3(kThreads), 0, s, g,
                       gslot, W1i, bo, q, B, tc, F, w1);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

namespace {

struct Bach10Trainer : CaTrainer {
    int deconv1() override {
        return bach10_deconv1(ctx->stream, GA + Uslot, Uslot, param(0), param(bo()), Q, B, tc, F, w1);
    }

    int loss(const float* x, const float* tgt, double* out7_d) override {
        MaskLoss a;
        a.q = Q; a.x = x; a.tgt = tgt; a.rnd = rnd; a.xy = xy; a.part = lpart;
        a.plane = (int64_t)tc * F;
        a.n = RF;
        a.eps = hyp[0];
        const int nblk = (int)std::min<int64_t>(kLossBlocks, dcs_cdiv(a.n, kThreads));
        hipLaunchKernelGGL(mask_loss_kernel<1>, dim3(nblk), dim3(kThreads), 0, ctx->stream, a);
        DCS_HIP(hipGetLastError());
        return loss_reduce<Bach10Sums>(nblk, out7_d, grad() + off[bo()]);
    }
};

}  // namespace

int bach10_trainer_new(int time_context, int F, int batch, dcs_trainer** out) {
    // time_context stops at 47, not at the 64 of the other trainers: from 48 on the inference path of this graph has no
    // column convolution (its f32 kernel would need more than 160 KiB of LDS), and a model nothing can load is no use
    if (time_context < 2 || time_context > kMaxTc || F < kK1 || F > 2049 || batch < 1 || batch > 1024)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: Bach10 graph: time_context %d (2 .. %d), F %d (30 .. 2049), batch %d (1 .. 1024)",
                 time_context, kMaxTc, F, batch);
    // dW1 is one 32 x 32 tile and dW2 five 128 x 32 tiles (tc 30): up to 512 slices
    const CaDesc desc = {kS1, 1, 2 * time_context / 3, 1, kSrc, {512, 512}, {2048, 512}};
    std::unique_ptr<Bach10Trainer> t(new Bach10Trainer());
    t->shape(desc, time_context, F, batch, kSrc);
    DCS_CHECK(t->check_index("Bach10", kSrc));
    t->nsrc = kSrc;
    t->loss_sums = kLossSums;
    *out = t.release();
    return DCS_OK;
}

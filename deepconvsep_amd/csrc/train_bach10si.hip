// Training of the score-informed Bach10 graph (examples/bach10_scoreinformed/trainCNNrwc.py: build_ca :134-193, loss :235-275,
// adadelta :279; trainCNNrwc_samp.py :195-235 and :275-321 train its single-branch form with the same loss) on gfx950.  The
// graph is the Bach10 graph of train_bach10.hip with three differences: conv1 reads four input channels (W1 [30, 4, 1, 30]) and
// its InverseLayer writes four output channels per decoder branch; the loss reads prediction2[:, 0:4], the four channels of
// branch 0 alone, and its mixture is the sum of the four input channels; the input is the mixture times four harmonic masks
// (the feed, train::gather_score_kernel).  It is the build_ca graph of train_ca.h (the step, the GEMMs and the layouts are
// there) with the description below: four input channels and the one live branch.
//
// DCS_ARCH_BACH10_SI (17 arrays) and DCS_ARCH_BACH10_SI1 (11 arrays) train the same live computation.  The 17-array graph's
// fc12, fc13, fc14 (arrays 10 .. 15) and bo[4:16] reach no loss term: theano.grad gives them exact zeros, and Adadelta from a
// zero state leaves them, accu and delta_accu untouched for ever.  They are held once, outside the stepped state (at 2049 bins
// they are 3 x 171 MB; in the state they would be four times that and stream through the update every step):
// dcs_trainer_get(which = 0) returns them bit-identical to what create was given, which = 1, 2, 3 return zeros.
//
//   F6        q_c = conv1^T(g)[c] + bo[c], c < 4: train::deconv1_channels_kernel, one slot, four weight slabs
//   loss      train::mask_loss_kernel<4>: x = ((x0 + x1) + x2) + x3, masks, the four errors, dE/dq (rectify' with the 0.5 tie)
//   update    train::adadelta_kernel over the 11 stepped arrays
//
// x, dY and q are [B][4][tc][F]; xy, U, GA and V have two slots each, where the Bach10 graph has five.
#include "train_ca.h"

using namespace train;

namespace {

constexpr int kS1 = 4, kCh = 4;                        // conv1: 30 filters of 1 x 30 over 4 channels, stride (1, 4)
constexpr int kNstate = 11, kSrc = 4, kBranches = 4;
// the largest time context dcs_model_create's score-informed graph runs: the inference kernels are the Bach10 graph's, whose
// f32 column convolution needs more than 160 KiB of LDS from 48 on
constexpr int kMaxTc = 47;

// out7 = (|E|, error1, error2, error3, error4, 0, 0), E = error1 + .. + error4 (trainCNNrwc.py:270-275)
struct SiSums {
    static constexpr int kOut = 4, kDbo = 4;
    static __device__ double E(const double* s) { return s[0] + s[1] + s[2] + s[3]; }
};
constexpr int kLossSums = SiSums::kOut + SiSums::kDbo;

}  // namespace

// F6, the one launch site of this graph's conv1^T instance (train_ca.h)
int train::bach10si_deconv1(hipStream_t s, const float* g, const float* W1i, const float* bo, float* q, int B, int tc, int F,
                            int w1) {
    const int64_t n = (int64_t)kSrc * B * tc * F;
    hipLaunchKernelGGL((deconv1_channels_kernel<kK1, kC1, kS1, kCh>), dim3((unsigned)dcs_cdiv(n, kThreads)), dim3(kThreads), 0,
                       s, g, W1i, bo, q, B, tc, F, w1);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

namespace {

struct SiTrainer : CaTrainer {
    bool full = false;            // the 17-array layout: dead parameters held in `dead`
    int64_t ndead = 0;            // 3 (256 flat + flat) + 12
    float* dead = nullptr;

    void plan(std::vector<std::pair<float**, int64_t>>& parts) override {
        CaTrainer::plan(parts);
        if (full) parts.push_back({&dead, ndead});
    }

    int deconv1() override { return bach10si_deconv1(ctx->stream, GA + Uslot, param(0), param(bo()), Q, B, tc, F, w1); }

    int loss(const float* x, const float* tgt, double* out7_d) override {
        MaskLoss a;
        a.q = Q; a.x = x; a.tgt = tgt; a.rnd = rnd; a.xy = xy; a.part = lpart;
        a.plane = (int64_t)tc * F;
        a.n = RF;
        a.eps = hyp[0];
        const int nblk = (int)std::min<int64_t>(kLossBlocks, dcs_cdiv(a.n, kThreads));
        hipLaunchKernelGGL(mask_loss_kernel<kCh>, dim3(nblk), dim3(kThreads), 0, ctx->stream, a);
        DCS_HIP(hipGetLastError());
        return loss_reduce<SiSums>(nblk, out7_d, grad() + off[bo()]);
    }

    // pkl: the caller's 17 (full) or 11 arrays.  The stepped arrays go through the layout kernel; the dead ones of the 17-array
    // graph are copied into `dead` at create and served from there: the parameters as given, zeros for the three other
    // sections (their gradient is exactly zero, so Adadelta never moves them or its two accumulators).
    int layout(float* flat_d, float* const* pkl, int to_internal) override {
        float* live[kNstate];
        for (int i = 0; i < 10; ++i) live[i] = pkl[i];
        live[10] = pkl[full ? 16 : 10];
        DCS_CHECK(CaTrainer::layout(flat_d, live, to_internal));
        if (!full) return DCS_OK;
        const int which = (int)((flat_d - state) / (4 * P4));
        // dcs_trainer_set on an optimiser slot: `dead` holds parameters, not accumulators, and stays as it is
        if (to_internal && which != 0) return DCS_OK;
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
    // dW1 is four 32 x 32 tiles and dW2 five 128 x 32 tiles (tc 30) over a K of 2 B tc w1 and 2 B h2 w1
    const CaDesc desc = {kS1, kCh, 2 * time_context / 3, 1, 1, {512, 512}, {2048, 512}};
    std::unique_ptr<SiTrainer> t(new SiTrainer());
    t->shape(desc, time_context, F, batch, kCh);
    // the Bach10 graph's check, with its four branches
    DCS_CHECK(t->check_index("score-informed Bach10", kBranches));
    t->nsrc = kSrc;
    t->loss_sums = kLossSums;
    // the stepped state is the 11 arrays of the single-branch form; the 17-array form lists the dead ones after them
    t->nstate = kNstate;
    for (int i = 0; i < kNstate; ++i)
        t->state_size[i] = t->shapes[i][0] * t->shapes[i][1] * t->shapes[i][2] * t->shapes[i][3];
    t->full = arch == DCS_ARCH_BACH10_SI;
    if (t->full) {
        const int64_t flat = t->flat;
        t->ndead = (kBranches - 1) * (kHidden * flat + flat) + kCh * (kBranches - 1);
        for (int k = 1; k < kBranches; ++k) {
            memcpy(t->shapes[8 + 2 * k], t->shapes[8], sizeof(t->shapes[8]));
            memcpy(t->shapes[9 + 2 * k], t->shapes[9], sizeof(t->shapes[9]));
        }
        const int64_t bo[4] = {kCh * kBranches, 1, 1, 1};
        memcpy(t->shapes[16], bo, sizeof(bo));
        t->nparams = 17;
    }
    *out = t.release();
    return DCS_OK;
}

// The test aids of the training core (include/dcs.h: dcs_debug_train_gemm, dcs_debug_train_aux): one launch of the GEMM
// template or of a helper kernel on the caller's buffers, after every address the launch can form has been checked on the host.
// Host code only: the kernels, their instantiations and their launch sites are train_core.hip's and the graph files'.
#include "train_ca.h"

using namespace train;

namespace {

// the trainer the launches need: dcs_trainer::launch and ::reduce use ctx, ::finish ctx and B
struct BareTrainer : dcs_trainer {
    void plan(std::vector<std::pair<float**, int64_t>>&) override {}
    int forward(const float*) override { return DCS_EUNSUPPORTED; }
    int loss(const float*, const float*, double*) override { return DCS_EUNSUPPORTED; }
    int backward() override { return DCS_EUNSUPPORTED; }
    int layout(float*, float* const*, int) override { return DCS_EUNSUPPORTED; }
};

bool bad_buf(const void* p, int64_t have, int64_t need_floats) {
    return !p || ((uintptr_t)p & 15) || have < need_floats * (int64_t)sizeof(float);
}

constexpr int64_t kMaxStride = (int64_t)1 << 31;   // far above any buffer; keeps the extents inside int64

bool bad_axis(const int64_t* a) {
    return a[0] < 1 || a[0] > kBig || a[1] < 1 || a[1] > kBig || a[2] < 0 || a[3] < 0 || a[4] < 0 || a[2] > kMaxStride || a[3] > kMaxStride ||
           a[4] > kMaxStride;
}

// the largest offset of the two inner levels over the indices 0 .. n - 1, 1 <= n <= d0 d1, strides not negative
int64_t top2(const int64_t* a, int64_t n) {
    const int64_t d0 = a[0], s0 = a[2], s1 = a[3];
    if (n <= d0) return (n - 1) * s0;
    const int64_t q = (n - 1) / d0, r = (n - 1) % d0;
    return std::max((d0 - 1) * s0 + (q - 1) * s1, r * s0 + q * s1);
}

// the largest offset the axis gives over the indices 0 .. n - 1 (the smallest is 0, at index 0)
int64_t top(const int64_t* a, int64_t n) {
    const int64_t d01 = std::min<int64_t>(a[0] * a[1], kBig);
    const int64_t q2 = (n - 1) / d01, rem = n - q2 * d01;
    int64_t best = q2 * a[4] + top2(a, rem);
    if (q2 > 0) best = std::max(best, (q2 - 1) * a[4] + top2(a, d01));
    return best;
}

// every batch's elements off + boff + [0, top(r, nr) + top(c, nc)] lie inside the buffer
int check_mat(const char* name, const dcs_debug_train_mat& m, int64_t nr, int64_t nc, const int64_t (*boff)[5], int which,
              int nbatch) {
    if (bad_axis(m.r) || bad_axis(m.c))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: %s: d0, d1 in 1 .. 2^30 and strides in 0 .. 2^31", name);
    if (!m.p || ((uintptr_t)m.p & 15)) DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: %s is null or not aligned to 16 bytes", name);
    const int64_t span = top(m.r, nr) + top(m.c, nc);
    for (int b = 0; b < nbatch; ++b) {
        const int64_t lo = m.off + boff[b][which];
        if (lo < 0 || (lo + span + 1) * (int64_t)sizeof(float) > m.bytes)
            DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: %s, batch %d: elements %lld .. %lld of a buffer of %lld bytes", name, b,
                     (long long)lo, (long long)(lo + span), (long long)m.bytes);
    }
    return DCS_OK;
}

Ax axis(const int64_t* a) { return ax3(a[0], a[1], a[2], a[3], a[4]); }
Mat matrix(const dcs_debug_train_mat& m) { return mat(m.p, m.off, axis(m.r), axis(m.c)); }

}  // namespace

extern "C" {

DCS_API int dcs_debug_train_gemm(dcs_ctx* ctx, dcs_debug_train_gemm_args* q) {
    if (!ctx || !q) DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: null argument");
    if (q->M < 1 || q->M >= kBig || q->N < 1 || q->N >= kBig || q->K < 1 || q->K >= kBig)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: M %d, N %d, K %d (each 1 .. 2^30 - 1)", q->M, q->N, q->K);
    if (q->tile != DCS_TRAIN_T128X32 && q->tile != DCS_TRAIN_T64X64 && q->tile != DCS_TRAIN_T32X32)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: tile %d", q->tile);
    if ((int64_t)q->M * q->N >= (int64_t)1 << 40) DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: %d x %d outputs", q->M, q->N);
    if (q->nbatch < 1 || q->nbatch > 4) DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: nbatch %d (1 .. 4)", q->nbatch);
    if (q->splits < 1 || (int64_t)q->nbatch * q->splits > 65535)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: %d slices in %d batches", q->splits, q->nbatch);
    if (q->splits > 1 && !q->partial) DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: %d slices without partial", q->splits);
    if (q->splits > 1 && (q->kchunk < kKT || q->kchunk % kKT))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: kchunk %d (a multiple of %d when K is split)", q->kchunk, kKT);
    if ((q->epi & ~(EPI_RELU | EPI_SAVEPRE | EPI_DRELU)) || ((q->epi & EPI_SAVEPRE) && (q->epi & EPI_DRELU)))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: epi %d", q->epi);
    if (q->ones_row < 0 || q->bias_cs < 0) DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: ones_row %d, bias_cs %d", q->ones_row, q->bias_cs);
    const int nb = q->nbatch;
    const int64_t arows = std::min(q->M, q->ones_row);
    if (arows > 0) DCS_CHECK(check_mat("A", q->A, arows, q->K, q->boff, 0, nb));
    DCS_CHECK(check_mat("B", q->B, q->K, q->N, q->boff, 1, nb));
    const bool has_x = !q->partial && (q->epi & (EPI_SAVEPRE | EPI_DRELU));
    if (!q->partial) DCS_CHECK(check_mat("C", q->C, q->M, q->N, q->boff, 2, nb));
    if (has_x) DCS_CHECK(check_mat("X", q->X, q->M, q->N, q->boff, 3, nb));
    if (q->partial) {
        if (bad_buf(q->partial, q->partial_bytes, (int64_t)nb * q->splits * q->M * q->N))
            DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: partial (%d x %d x %d x %d floats in %lld bytes)", nb, q->splits, q->M, q->N,
                     (long long)q->partial_bytes);
    } else {
        const float* bias[2] = {q->bias, q->bias2};
        const int64_t have[2] = {q->bias_bytes, q->bias2_bytes};
        for (int i = 0; i < 2; ++i) {
            if (!bias[i]) continue;
            for (int b = 0; b < nb; ++b) {
                const int64_t lo = q->boff[b][4];
                if (lo < 0 || bad_buf(bias[i], have[i], lo + (int64_t)(q->N - 1) * q->bias_cs + 1))
                    DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: bias%s, batch %d", i ? "2" : "", b);
            }
        }
    }
    if (q->scale && bad_buf(q->scale, q->scale_bytes, 1)) DCS_FAIL(DCS_EINVAL, "dcs_debug_train_gemm: scale");

    Gemm g = gemm0(q->M, q->N, q->K);
    if (arows > 0) g.A = matrix(q->A);
    g.B = matrix(q->B);
    if (!q->partial) g.C = matrix(q->C);
    if (has_x) g.X = matrix(q->X);
    g.ones_row = q->ones_row; g.ones_klim = q->ones_klim;
    g.nbatch = nb;
    memcpy(g.boff, q->boff, sizeof(g.boff));
    g.bias = q->bias; g.bias_cs = q->bias_cs; g.bias2 = q->bias2; g.scale = q->scale;
    g.epi = q->epi;
    g.partial = q->partial; g.splits = q->splits; g.kchunk = q->kchunk;
    DCS_ON_DEVICE(ctx->device);
    BareTrainer t;
    t.ctx = ctx;
    dim3 grid;
    const Tile tile = q->tile == DCS_TRAIN_T128X32 ? T128x32 : (q->tile == DCS_TRAIN_T64X64 ? T64x64 : T32x32);
    DCS_CHECK(t.launch(g, tile, q->ak != 0, q->bk != 0, &grid));
    DCS_HIP(hipStreamSynchronize(ctx->stream));
    q->grid_x = (int)grid.x; q->grid_y = (int)grid.y; q->grid_z = (int)grid.z;
    return DCS_OK;
}

DCS_API int dcs_debug_train_aux(dcs_ctx* ctx, int which, dcs_debug_train_aux_args* q) {
    if (!ctx || !q) DCS_FAIL(DCS_EINVAL, "dcs_debug_train_aux: null argument");
    DCS_ON_DEVICE(ctx->device);
    BareTrainer t;
    t.ctx = ctx;
    const int64_t lim = (int64_t)1 << 30;
    if (which == DCS_TRAIN_AUX_FINISH) {
        if (q->B < 1 || q->N < 1 || q->splits < 1 || (int64_t)q->B * q->N * q->splits >= lim)
            DCS_FAIL(DCS_EINVAL, "dcs_debug_train_aux: finish of %d slices of %d x %d", q->splits, q->B, q->N);
        if ((q->epi & ~(EPI_RELU | EPI_SAVEPRE | EPI_DRELU)) || ((q->epi & EPI_SAVEPRE) && (q->epi & EPI_DRELU)))
            DCS_FAIL(DCS_EINVAL, "dcs_debug_train_aux: epi %d", q->epi);
        const int64_t count = (int64_t)q->B * q->N;
        if (bad_buf(q->in, q->in_bytes, q->splits * count) || (q->in2 && bad_buf(q->in2, q->in2_bytes, q->N)) ||
            bad_buf(q->out, q->out_bytes, count) ||
            ((q->epi & (EPI_SAVEPRE | EPI_DRELU)) && bad_buf(q->out2, q->out2_bytes, count)))
            DCS_FAIL(DCS_EINVAL, "dcs_debug_train_aux: finish buffers");
        t.B = q->B;
        DCS_CHECK(t.finish(q->in, q->splits, q->N, q->in2, q->out, q->out2, q->epi));
    } else if (which == DCS_TRAIN_AUX_REDUCE) {
        Reduce r;
        memset(&r, 0, sizeof(r));
        const float* part[2] = {q->in, q->in2};
        float* dst[2] = {q->out, q->out2};
        const int64_t have_in[2] = {q->in_bytes, q->in2_bytes}, have_out[2] = {q->out_bytes, q->out2_bytes};
        if (q->count[0] < 1 || q->count[1] < 0) DCS_FAIL(DCS_EINVAL, "dcs_debug_train_aux: reduce of %lld and %lld sums",
                                                         (long long)q->count[0], (long long)q->count[1]);
        for (int j = 0; j < 2; ++j) {
            if (q->count[j] == 0) continue;
            if (q->count[j] >= lim || q->rsplits[j] < 1 || q->count[j] * q->rsplits[j] >= lim || q->rN[j] < 0 ||
                (q->dup[j] && (q->rN[j] < 1 || q->rN[j] > q->count[j])))
                DCS_FAIL(DCS_EINVAL, "dcs_debug_train_aux: reduce job %d: %d slices of %lld, the last %d once more: %d", j,
                         q->rsplits[j], (long long)q->count[j], q->rN[j], q->dup[j]);
            if (bad_buf(part[j], have_in[j], q->count[j] * q->rsplits[j]) ||
                bad_buf(dst[j], have_out[j], q->count[j] + (q->dup[j] ? q->rN[j] : 0)))
                DCS_FAIL(DCS_EINVAL, "dcs_debug_train_aux: reduce buffers of job %d", j);
            r.part[j] = part[j]; r.dst[j] = dst[j]; r.count[j] = q->count[j]; r.splits[j] = q->rsplits[j];
            r.N[j] = q->rN[j]; r.dup[j] = q->dup[j];
        }
        if (bad_buf(q->in3, q->in3_bytes, 1)) DCS_FAIL(DCS_EINVAL, "dcs_debug_train_aux: reduce scale");
        r.scale = q->in3;
        DCS_CHECK(t.reduce(r));
    } else if (which == DCS_TRAIN_AUX_DECONV1_IKALA || which == DCS_TRAIN_AUX_DECONV1_BACH10 ||
               which == DCS_TRAIN_AUX_DECONV1_BACH10SI) {
        const bool ik = which == DCS_TRAIN_AUX_DECONV1_IKALA, si = which == DCS_TRAIN_AUX_DECONV1_BACH10SI;
        const int S1 = ik ? 3 : 4, ns = ik ? 2 : 4;
        if (q->B < 1 || q->tc < 1 || q->F < kK1 || q->w1 != (q->F - kK1) / S1 + 1 || q->gslot < 0 || q->gslot >= lim ||
            (int64_t)q->B * q->tc * q->F * ns >= lim)
            DCS_FAIL(DCS_EINVAL, "dcs_debug_train_aux: conv1^T of %d x %d x %d, %d windows, slot %lld", q->B, q->tc, q->F, q->w1,
                     (long long)q->gslot);
        const int64_t gone = (int64_t)q->B * q->tc * q->w1 * kC1;
        if (bad_buf(q->in, q->in_bytes, (si ? 0 : (ns - 1) * q->gslot) + gone) ||
            bad_buf(q->in2, q->in2_bytes, (int64_t)(si ? ns : 1) * kK1 * kC1) || bad_buf(q->in3, q->in3_bytes, ns) ||
            bad_buf(q->out, q->out_bytes, (int64_t)q->B * ns * q->tc * q->F))
            DCS_FAIL(DCS_EINVAL, "dcs_debug_train_aux: conv1^T buffers");
        if (ik) DCS_CHECK(ikala_deconv1(ctx->stream, q->in, q->gslot, q->in2, q->in3, q->out, q->B, q->tc, q->F, q->w1));
        else if (si) DCS_CHECK(bach10si_deconv1(ctx->stream, q->in, q->in2, q->in3, q->out, q->B, q->tc, q->F, q->w1));
        else DCS_CHECK(bach10_deconv1(ctx->stream, q->in, q->gslot, q->in2, q->in3, q->out, q->B, q->tc, q->F, q->w1));
    } else {
        DCS_FAIL(DCS_EINVAL, "dcs_debug_train_aux: which = %d", which);
    }
    DCS_HIP(hipStreamSynchronize(ctx->stream));
    return DCS_OK;
}

}  // extern "C"

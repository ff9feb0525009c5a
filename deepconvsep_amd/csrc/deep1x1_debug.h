// The checks of the test aids dcs_debug_d1_conv / dcs_debug_d1_aux (include/dcs.h), shared by the two translation units that
// launch d1_igemm_kernel: each launches its own instances, both check and fill the arguments with this one code.
#pragma once

#include "deep1x1_igemm.h"

namespace d1 {
namespace {

constexpr int kDbgMaxDim = 32768, kDbgMaxCh = 4096, kDbgMaxKh = 64;

bool dbg_bad(const void* p, int64_t have, int64_t need) { return !p || ((uintptr_t)p & 15) || have < need; }

// Checks `q` for `mode`, fills `a` through forward_args / transposed_args and the returned fields of `q`.  DCS_EINVAL (nothing
// may be launched then) or DCS_OK.
int debug_conv_args(int mode, dcs_debug_d1_args* q, D1Args* out) {
    if (mode < MODE_FWD || mode > MODE_B11) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: mode %d", mode);
    const bool tr = mode == MODE_TR || mode == MODE_LAST || mode == MODE_Q || mode == MODE_B11;
    if (q->images < 1 || q->images > (1 << 20) || q->Hi < 1 || q->Hi > kDbgMaxDim || q->Wi < 1 || q->Wi > kDbgMaxDim ||
        q->kh < 1 || q->kh > kDbgMaxKh || q->N < 1 || q->N > kDbgMaxCh)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: %d images of %d x %d, kh %d, N %d out of range", q->images, q->Hi, q->Wi, q->kh, q->N);
    if (q->Ci < 4 || q->Ci > kDbgMaxCh || q->Ci % 4) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: channel pitch %d of the input", q->Ci);
    if (q->trainer_unit && (mode == MODE_1X1 || mode == MODE_LAST))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: the trainer launches no mode %d of the separator", mode);
    D1Args a;
    if (!tr) {
        if ((q->kw != 1 && q->kw != kKw) || q->stride < 1 || q->stride > 2 || q->kh > q->Hi || q->kw > q->Wi)
            DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: a %d x %d filter, stride %d, on %d x %d", q->kh, q->kw, q->stride, q->Hi, q->Wi);
        a = forward_args(q->images, q->Hi, q->Wi, q->Ci, q->kh, q->kw, q->stride, q->N);
        q->Ho = a.Ho; q->Wo = a.Wo;
    } else {
        const int stride = q->kw == 1 ? 1 : 2;
        if ((q->kw != 1 && q->kw != kKw) || q->par < 0 || q->par >= stride || q->Ho < 1 || q->Ho > kDbgMaxDim || q->Wo < q->kw ||
            q->Wo > kDbgMaxDim || q->Hi != q->Ho - q->kh + 1 || q->Wi != (q->Wo - q->kw) / stride + 1)
            DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: the transpose of a %d x %d convolution from %d x %d to %d x %d, parity %d", q->kh,
                     q->kw, q->Ho, q->Wo, q->Hi, q->Wi, q->par);
        if ((mode == MODE_B11) != (q->kw == 1)) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: mode %d with kw %d", mode, q->kw);
        a = transposed_args(q->images, q->Hi, q->Wi, q->Ci, q->Ho, q->Wo, q->kh, q->kw, q->par, q->N);
    }
    if ((tr ? a.Ci : a.ntap * a.Ci) < 16)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: a tap%s of %d floats (D1Args: at least 16, the 16 K values of one step start inside it)",
                 tr ? "" : " row", tr ? a.Ci : a.ntap * a.Ci);
    if (a.M < 1) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: M == 0 (no output pixel in this launch)");
    if (a.M > (int64_t)1 << 30 || (int64_t)a.Ho * a.Wq >= (int64_t)1 << 30)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: %lld output pixels", (long long)a.M);
    const int nt = nt_for(a.N), npad = npad_for(a.N);
    const int64_t px_in = (int64_t)q->images * q->Hi * q->Wi;
    const bool has_co = mode == MODE_FWD || mode == MODE_TR || mode == MODE_FWDC || mode == MODE_B11;
    if (has_co && (q->Co % 4 || q->Co < a.N || q->Co > npad))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: channel pitch %d of the output for %d channels (a multiple of 4 in %d .. %d)", q->Co,
                 a.N, a.N, npad);
    a.Co = has_co ? q->Co : 0;
    if (dbg_bad(q->in, q->in_bytes, px_in * q->Ci * 4)) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: in");
    if (dbg_bad(q->B, q->B_bytes, (int64_t)npad * a.Kpad * 4)) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: B");
    if (tr && dbg_bad(q->code, q->code_bytes, px_in * q->Ci)) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: code");
    if (mode == MODE_FWDC && dbg_bad(q->code, q->code_bytes, a.M * a.Co)) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: code");
    const bool has_b0 = mode == MODE_FWD || mode == MODE_1X1 || mode == MODE_LAST || mode == MODE_Q;
    const bool has_b1 = mode == MODE_FWD || mode == MODE_1X1;
    if (has_b0 && dbg_bad(q->b0, q->b0_bytes, (int64_t)a.N * 4)) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: b0");
    if (has_b1 && dbg_bad(q->b1, q->b1_bytes, (int64_t)a.N * 4)) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: b1");
    int64_t out_need = 0;
    if (mode == MODE_FWD || mode == MODE_FWDC || mode == MODE_B11) out_need = a.M * a.Co;
    else if (mode == MODE_TR) out_need = (int64_t)q->images * a.Ho * a.Wo * a.Co;
    else if (mode == MODE_1X1) out_need = (int64_t)dcs_cdiv(a.N, kNf) * a.M * kNf;
    else if (mode == MODE_Q) out_need = (int64_t)q->images * a.N * a.Ho * a.Wo;
    else {
        if (q->n_total < 1 || q->n_total > (1 << 16) || q->k_first < 0 || q->k_first + q->images > q->n_total || q->ch_off < 0 ||
            q->ch_off > kDbgMaxCh)
            DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: tiles %lld .. of %lld, channel offset %d", (long long)q->k_first,
                     (long long)q->n_total, q->ch_off);
        a.n_total = q->n_total; a.k_first = q->k_first; a.ch_off = q->ch_off;
        out_need = (int64_t)(q->ch_off + a.N) * q->n_total * a.Ho * a.Wo;
    }
    if (dbg_bad(q->out, q->out_bytes, out_need * 4)) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: out");
    if (mode == MODE_FWD && dbg_bad(q->code_out, q->code_out_bytes, a.M * a.Co)) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: code_out");
    a.in = q->in; a.code = q->code; a.B = q->B; a.b0 = has_b0 ? q->b0 : nullptr; a.b1 = has_b1 ? q->b1 : nullptr;
    a.out = q->out; a.code_out = mode == MODE_FWD ? q->code_out : nullptr;
    q->nt = nt; q->grid_x = (int)((a.M + kBM - 1) / kBM); q->grid_y = dcs_cdiv(a.N, 16 * nt);
    q->K = a.K; q->Kpad = a.Kpad; q->Wq = a.Wq; q->M = a.M;
    *out = a;
    return DCS_OK;
}

template <int MODE>
int debug_conv_run(dcs_ctx* ctx, const D1Args& a) {
    launch<MODE>(ctx, a);
    DCS_HIP(hipGetLastError());
    DCS_HIP(hipStreamSynchronize(ctx->stream));
    return DCS_OK;
}

}  // namespace
}  // namespace d1

// the trainer's unit (train_deep1x1.hip): FWD and TR of its own copy, FWDC, Q, B11; code_apply, codes_out and pack_kernel
int deep1x1_trainer_debug_conv(dcs_ctx* ctx, int mode, dcs_debug_d1_args* q);
int deep1x1_trainer_debug_aux(dcs_ctx* ctx, int which, dcs_debug_d1_aux_args* q);

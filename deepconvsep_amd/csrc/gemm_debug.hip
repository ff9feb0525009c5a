// Test aids (include/dcs.h, "Test aids for the GEMM kernels"): the GEMM launchers and operand packers of gemm.hip,
// gemm_bf16x3.hip and gemm_f16.hip behind entries that check every address a kernel can form against the element counts the
// caller gives, and launch nothing otherwise.  No kernel here; kernel selection stays with the launchers.
#include <string.h>

#include <vector>

#include "dcs_internal.h"
#include "generic.h"

namespace {

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// largest row index of a grouped operand over r = 0 .. M - 1 (the kernels take the flat path when gdiv >= M)
int64_t max_group_row(int64_t M, int gdiv, int64_t gmul) {
    if (gdiv >= M) return M - 1;
    const int64_t last = ((M - 1) / gdiv) * gmul + (M - 1) % gdiv;
    const int64_t full = ((M - 1) / gdiv - 1) * gmul + gdiv - 1;   // the last whole group (there is one: gdiv < M)
    return last > full ? last : full;
}

constexpr int64_t kMaxDim = 1 << 24;

}  // namespace

extern "C" int dcs_debug_gemm(dcs_ctx* ctx, int which, const dcs_debug_gemm_args* a) {
    if (!ctx || !a) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: null argument");
    if (which != DCS_GEMM_VIA_ROWS && which != DCS_GEMM_VIA_SKINNY && which != DCS_GEMM_VIA_LONGK)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: which = %d", which);
    if (a->M < 1 || a->M > kMaxDim || a->K < 1 || a->K > kMaxDim || a->n_cols < 1 || a->n_cols > kMaxDim)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: M %lld, K %d, n_cols %d", (long long)a->M, a->K, a->n_cols);
    if (a->n_store < 0 || a->n_store > a->n_cols) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: n_store %d of %d columns", a->n_store, a->n_cols);
    const int n_br = which == DCS_GEMM_VIA_SKINNY ? a->n_br : 0;
    if (a->n_br < 0 || a->n_br > 4 || (a->n_br > 0 && which != DCS_GEMM_VIA_SKINNY))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: %d branches", a->n_br);
    if (!a->A || !a->B || (n_br == 0 && !a->C)) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: null operand");
    if (a->n_A < 0 || a->n_B < 0 || a->n_C < 0 || a->n_bias < 0 || a->n_rowmap < 0 || a->Bq_bytes < 0 || a->Aq_bytes < 0 || a->n_Bfrag < 0)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: negative count");
    if (!aligned16(a->B) || !aligned16(a->Bq) || !aligned16(a->Aq) || !aligned16(a->Bfrag) || (a->a_vec && !aligned16(a->A)))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: an operand is not 16-byte aligned");
    // B: [round_up(K, 128)][ldb], read in 16-byte pieces at multiples of 4 columns
    if ((a->ldb % 64) || a->ldb < a->n_cols || a->ldb > kMaxDim) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: ldb %d for %d columns", a->ldb, a->n_cols);
    if (dcs_round_up(a->K, 128) * (int64_t)a->ldb > a->n_B)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: B needs %lld floats (K padded to a multiple of 128), has %lld",
                 (long long)(dcs_round_up(a->K, 128) * (int64_t)a->ldb), (long long)a->n_B);
    if ((a->n_cols % 64) && which != DCS_GEMM_VIA_ROWS) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: n_cols %d not a multiple of 64", a->n_cols);
    // A rows
    if (a->lda < 0 || a->lda > kMaxDim || a->a_gdiv < 1 || a->a_gmul < 0 || a->a_gmul > kMaxDim)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: lda %lld, a_gdiv %d, a_gmul %lld", (long long)a->lda, a->a_gdiv, (long long)a->a_gmul);
    if (!(a->a_scale == a->a_scale)) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: a_scale");
    DCS_ON_DEVICE(ctx->device);
    int64_t a_max_row = max_group_row(a->M, a->a_gdiv, a->a_gmul);
    if (a->a_rowmap) {
        if (which != DCS_GEMM_VIA_ROWS) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: a row map with the bf16 launchers");
        if (a->n_rowmap < a->M) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: row map of %lld for %lld rows", (long long)a->n_rowmap, (long long)a->M);
        std::vector<int32_t> map((size_t)a->M);
        DCS_HIP(hipStreamSynchronize(ctx->stream));
        DCS_HIP(hipMemcpy(map.data(), a->a_rowmap, map.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        a_max_row = 0;
        for (int64_t r = 0; r < a->M; ++r) {
            if (map[(size_t)r] < 0) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: row map entry %lld is %d", (long long)r, map[(size_t)r]);
            if (map[(size_t)r] > a_max_row) a_max_row = map[(size_t)r];
        }
    }
    if (a_max_row * a->lda + a->K > a->n_A)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: A row %lld ends at %lld of %lld floats", (long long)a_max_row,
                 (long long)(a_max_row * a->lda + a->K), (long long)a->n_A);
    // C rows, bias
    if (a->ldc < a->n_store || a->ldc > kMaxDim || a->c_gdiv < 1 || a->c_gmul < 0 || a->c_gmul > kMaxDim)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: ldc %lld, c_gdiv %d, c_gmul %lld", (long long)a->ldc, a->c_gdiv, (long long)a->c_gmul);
    if (max_group_row(a->M, a->c_gdiv, a->c_gmul) * a->ldc + a->n_store > a->n_C)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: C ends at %lld of %lld floats",
                 (long long)(max_group_row(a->M, a->c_gdiv, a->c_gmul) * a->ldc + a->n_store), (long long)a->n_C);
    if ((a->bias || n_br > 0) && a->n_bias < a->n_store) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: bias of %lld for %d columns", (long long)a->n_bias, a->n_store);
    // packed operands
    const int64_t bq_need = (int64_t)(a->bq_f32 ? dcs_gemm_b32_bytes(a->K, a->n_cols) : dcs_gemm_bq_bytes(a->K, a->n_cols));
    if ((a->Bq || n_br > 0) && a->Bq_bytes < bq_need)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: Bq of %lld bytes, needs %lld", (long long)a->Bq_bytes, (long long)bq_need);
    if (a->Aq && (a->aq_rows < 1 || a->aq_rows > kMaxDim || a->Aq_bytes < (int64_t)dcs_gemm_aq_bytes(a->K, a->aq_rows)))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: Aq of %lld bytes for %d rows", (long long)a->Aq_bytes, a->aq_rows);
    if (a->Bfrag && a->n_Bfrag < (int64_t)(a->n_cols / 16) * dcs_bfrag_chunks(a->K) * 256)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: Bfrag of %lld floats, needs %lld", (long long)a->n_Bfrag,
                 (long long)((int64_t)(a->n_cols / 16) * dcs_bfrag_chunks(a->K) * 256));
    for (int b = 0; b < n_br; ++b)
        if (!a->br_Bq[b] || !a->br_C[b] || !aligned16(a->br_Bq[b]))
            DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm: branch %d: null or misaligned operand", b);

    DcsGemm g{};
    g.A = a->A; g.lda = a->lda; g.a_gdiv = a->a_gdiv; g.a_gmul = a->a_gmul; g.a_scale = a->a_scale; g.a_rowmap = a->a_rowmap;
    g.B = a->B; g.ldb = a->ldb; g.bias = a->bias;
    g.C = a->C; g.ldc = a->ldc; g.c_gdiv = a->c_gdiv; g.c_gmul = a->c_gmul;
    g.M = a->M; g.n_cols = a->n_cols; g.n_store = a->n_store; g.K = a->K; g.relu = a->relu ? 1 : 0; g.a_vec = a->a_vec ? 1 : 0;
    g.Bq = a->Bq; g.bq_f32 = a->bq_f32 ? 1 : 0; g.Aq = a->Aq; g.aq_rows = a->Aq ? a->aq_rows : 0; g.Bfrag = a->Bfrag;
    ctx->note_gemm(0);
    if (which == DCS_GEMM_VIA_ROWS) return dcs_launch_gemm_rows(ctx, g, DCS_TAG_FC);
    bool taken;
    if (which == DCS_GEMM_VIA_SKINNY) {
        DcsGemmBranches br{};
        br.n = n_br;
        for (int b = 0; b < n_br; ++b) { br.Bq[b] = a->br_Bq[b]; br.bias[b] = a->br_bias[b]; br.C[b] = a->br_C[b]; }
        taken = dcs_launch_gemm_bf16x3_skinny(ctx, g, n_br > 0 ? &br : nullptr);
    } else
        taken = dcs_launch_gemm_bf16x3_longk(ctx, g);
    if (!taken) DCS_FAIL(DCS_EUNSUPPORTED, "dcs_debug_gemm: the launcher does not take this shape");
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

extern "C" int dcs_debug_gemm_f16_skinny(dcs_ctx* ctx, const float* Z, int64_t n_Z, int64_t ldz, int M, int K, int n_cols, int n_br,
                                         const void* const* Bh, int64_t Bh_bytes, const float* const* bias, int64_t n_bias,
                                         void* const* C, int64_t n_C, int64_t ldc, void* Ah_scratch, int64_t Ah_bytes) {
    if (!ctx || !Z || !Bh || !bias || !C || !Ah_scratch) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_f16_skinny: null argument");
    if (M < 1 || M > kMaxDim || K < 1 || K > kMaxDim || n_cols < 1 || n_cols > kMaxDim || n_br < 1 || n_br > 4)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_f16_skinny: M %d, K %d, n_cols %d, %d branches", M, K, n_cols, n_br);
    if (ldz < 0 || ldz > kMaxDim || (int64_t)(M - 1) * ldz + K > n_Z) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_f16_skinny: Z rows leave its %lld floats", (long long)n_Z);
    if (ldc < n_cols || ldc > kMaxDim || (int64_t)(M - 1) * ldc + n_cols > n_C) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_f16_skinny: C rows leave its %lld halves", (long long)n_C);
    if (n_bias < n_cols) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_f16_skinny: bias of %lld for %d columns", (long long)n_bias, n_cols);
    if (Bh_bytes < (int64_t)dcs_gemm_bh_bytes(K, n_cols)) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_f16_skinny: weight plane of %lld bytes", (long long)Bh_bytes);
    if (Ah_bytes < (int64_t)dcs_gemm_ah_bytes(K, M <= 128 ? 128 : 176) || !aligned16(Ah_scratch))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_f16_skinny: row planes of %lld bytes", (long long)Ah_bytes);
    for (int b = 0; b < n_br; ++b)
        if (!Bh[b] || !bias[b] || !C[b] || !aligned16(Bh[b])) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_f16_skinny: branch %d: null or misaligned operand", b);
    DCS_ON_DEVICE(ctx->device);
    ctx->note_gemm(0);
    if (!dcs_launch_gemm_f16_skinny(ctx, Z, ldz, M, K, n_cols, n_br, Bh, bias, C, ldc, Ah_scratch))
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_debug_gemm_f16_skinny: the launcher does not take this shape");
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

extern "C" int dcs_debug_gemm_f16_longk(dcs_ctx* ctx, const void* A, int64_t n_A, int64_t lda, int M, int K, int n_cols, const void* Bh,
                                        int64_t Bh_bytes, int a_f16, const float* bias, int64_t n_bias, float* C, int64_t n_C,
                                        int64_t ldc, int n_store, int relu) {
    if (!ctx || !A || !Bh || !C) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_f16_longk: null argument");
    if (M < 1 || M > kMaxDim || K < 1 || K > kMaxDim || n_cols < 1 || n_cols > kMaxDim)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_f16_longk: M %d, K %d, n_cols %d", M, K, n_cols);
    if (n_store < 0 || n_store > n_cols) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_f16_longk: n_store %d of %d columns", n_store, n_cols);
    if (lda < 0 || lda > kMaxDim || (int64_t)(M - 1) * lda + K > n_A) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_f16_longk: A rows leave its %lld elements", (long long)n_A);
    if (ldc < n_store || ldc > kMaxDim || (int64_t)(M - 1) * ldc + n_store > n_C) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_f16_longk: C rows leave its %lld floats", (long long)n_C);
    if (bias && n_bias < n_store) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_f16_longk: bias of %lld for %d columns", (long long)n_bias, n_store);
    if (Bh_bytes < (int64_t)dcs_gemm_bh_bytes(K, n_cols) || !aligned16(Bh)) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_f16_longk: weight plane of %lld bytes", (long long)Bh_bytes);
    DCS_ON_DEVICE(ctx->device);
    ctx->note_gemm(0);
    const int ksplit = dcs_gemm_f16_longk_slices(ctx, M, K, n_cols);
    if (ksplit < 2) DCS_FAIL(DCS_EUNSUPPORTED, "dcs_debug_gemm_f16_longk: the launcher does not take this shape");
    DCS_CHECK(ctx->gemm_ws.ensure((size_t)ksplit * M * n_cols * sizeof(float)));
    if (!dcs_launch_gemm_f16_longk(ctx, A, lda, M, K, n_cols, Bh, (float*)ctx->gemm_ws.ptr, a_f16 != 0))
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_debug_gemm_f16_longk: the launcher does not take this shape");
    DcsGemm r{};
    r.partial = (float*)ctx->gemm_ws.ptr;
    r.M = M; r.n_cols = n_cols; r.n_store = n_store; r.bias = bias; r.relu = relu ? 1 : 0;
    r.C = C; r.ldc = ldc; r.c_gdiv = 1 << 30; r.c_gmul = 0;
    dcs_launch_gemm_longk_reduce(ctx, r, ksplit);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

extern "C" int64_t dcs_debug_gemm_bytes(int kind, int K, int n) {
    if (K < 1 || n < 1 || K > kMaxDim || n > kMaxDim) return -1;
    switch (kind) {
        case DCS_GEMM_PACK_BQ: return (int64_t)dcs_gemm_bq_bytes(K, n);
        case DCS_GEMM_PACK_B32: return (int64_t)dcs_gemm_b32_bytes(K, n);
        case DCS_GEMM_PACK_BH:
        case DCS_GEMM_PACK_BH_PLAIN: return (int64_t)dcs_gemm_bh_bytes(K, n);
        case DCS_GEMM_PACK_BIAS_CL: return (int64_t)n * 4;
        case DCS_GEMM_PACK_SPLIT_A: return (int64_t)dcs_gemm_aq_bytes(K, n);
        case DCS_GEMM_PACK_BFRAG: return (int64_t)(n / 16) * dcs_bfrag_chunks(K) * 256 * 4;
        case DCS_GEMM_PACK_SPLIT_A_F16: return (int64_t)dcs_gemm_ah_bytes(K, n);
    }
    return -1;
}

extern "C" int dcs_debug_gemm_pack(dcs_ctx* ctx, int kind, const float* src, int64_t n_src, int K, int64_t ld, int n, const int64_t* p,
                                   void* dst, int64_t dst_bytes) {
    if (!ctx || !src || !dst) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_pack: null argument");
    if (kind < DCS_GEMM_PACK_BQ || kind > DCS_GEMM_PACK_BFRAG) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_pack: kind %d", kind);
    if (kind == DCS_GEMM_PACK_BIAS_CL) { K = 1; ld = 0; }
    if (K < 1 || K > kMaxDim || n < 1 || n > kMaxDim || ld < 0 || ld > kMaxDim || n_src < 0)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_pack: K %d, n %d, ld %lld", K, n, (long long)ld);
    if (dst_bytes < dcs_debug_gemm_bytes(kind, K, n) || !aligned16(dst))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_pack: dst of %lld bytes, needs %lld", (long long)dst_bytes, (long long)dcs_debug_gemm_bytes(kind, K, n));
    const bool needs_p = kind == DCS_GEMM_PACK_BH || kind == DCS_GEMM_PACK_BIAS_CL || kind == DCS_GEMM_PACK_SPLIT_A;
    if (needs_p && !p) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_pack: kind %d needs its parameters", kind);
    int64_t width = n;                         // source columns a row is read over
    int64_t rows = K;
    int64_t q[4] = {0, 0, 0, 0};
    if (p) memcpy(q, p, sizeof(q));
    for (int i = 0; i < 4; ++i)
        if (q[i] < 0 || q[i] > kMaxDim) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_pack: p[%d] = %lld", i, (long long)q[i]);
    if (kind == DCS_GEMM_PACK_BQ || kind == DCS_GEMM_PACK_B32) {
        if (q[0] > 0 && (q[1] < 1 || q[0] * q[1] > n)) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_pack: permutation wider than B");
    } else if (kind == DCS_GEMM_PACK_BH || kind == DCS_GEMM_PACK_BIAS_CL) {
        if (q[0] < 1 || q[1] < 1 || q[2] < 1 || q[0] * q[1] > kMaxDim) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_pack: nch, npos, chpad");
        width = q[0] * q[1];
    } else if (kind == DCS_GEMM_PACK_SPLIT_A) {
        if (q[0] < 1) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_pack: M");
        rows = q[0] < n ? q[0] : n;           // rows >= rows_pad are not read
        width = K;
    } else if (kind == DCS_GEMM_PACK_BFRAG && (n % 16))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_pack: n_cols %d not a multiple of 16", n);
    if (kind != DCS_GEMM_PACK_BIAS_CL && ld < width) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_pack: ld %lld < %lld", (long long)ld, (long long)width);
    if ((rows - 1) * ld + width > n_src)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_pack: src ends at %lld of %lld floats", (long long)((rows - 1) * ld + width), (long long)n_src);
    if (kind == DCS_GEMM_PACK_BFRAG) {
        dcs_gemm_pack_bfrag(src, K, (int)ld, n, reinterpret_cast<float*>(dst));
        return DCS_OK;
    }
    DCS_ON_DEVICE(ctx->device);
    switch (kind) {
        case DCS_GEMM_PACK_BQ: return dcs_gemm_pack_bq(ctx, src, K, (int)ld, n, dst, (int)q[0], (int)q[1]);
        case DCS_GEMM_PACK_B32: return dcs_gemm_pack_b32(ctx, src, K, (int)ld, n, dst, (int)q[0], (int)q[1]);
        case DCS_GEMM_PACK_BH: return dcs_gemm_pack_bh(ctx, src, K, (int)ld, n, (int)q[0], (int)q[1], (int)q[2], dst);
        case DCS_GEMM_PACK_BH_PLAIN: return dcs_gemm_pack_bh_plain(ctx, src, K, (int)ld, n, dst);
        case DCS_GEMM_PACK_BIAS_CL: return dcs_gemm_pack_bias_cl(ctx, src, n, (int)q[0], (int)q[1], (int)q[2], reinterpret_cast<float*>(dst));
        default: return dcs_gemm_split_a(ctx, src, ld, q[0], K, n, dst);
    }
}

extern "C" int dcs_debug_gemm_last_kernel(const dcs_ctx* ctx, int* code, int64_t* params) {
    if (!ctx) DCS_FAIL(DCS_EINVAL, "dcs_debug_gemm_last_kernel: null context");
    if (code) *code = ctx->last_gemm;
    if (params)
        for (int i = 0; i < 4; ++i) params[i] = ctx->last_gemm_param[i];
    return DCS_OK;
}

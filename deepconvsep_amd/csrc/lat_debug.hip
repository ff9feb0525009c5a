// The test aids of the one-batch kernels (include/dcs.h: dcs_debug_lat_gemm, dcs_debug_lat_stft_forward_f32,
// dcs_debug_lat_stft_inverse_f32): one launch of lat_gemm_kernel, of lat_stft_kernel or of lat_ifft_kernel + lat_ola_kernel on the
// caller's buffers, after every address the launch can form has been checked on the host.
// Host code only: the kernels, their instantiations and their launch sites are dsd_lat.hip's (dcs_launch_lat_gemm,
// dcs_launch_lat_stft, dcs_launch_lat_istft -- the launchers net.hip calls).
#include "dsd_lat.h"

#include <math.h>

namespace {

constexpr int64_t kMaxStride = (int64_t)1 << 31;   // far above any buffer; keeps the extents inside int64
constexpr int kMaxRows = 1 << 20;                  // the row map is walked on the host

bool bad_ptr(const void* p, unsigned mask) { return !p || ((uintptr_t)p & mask); }

}  // namespace

extern "C" {

DCS_API int dcs_debug_lat_gemm(dcs_ctx* ctx, dcs_debug_lat_gemm_args* q) {
    if (!ctx || !q) DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_gemm: null argument");
    if (q->M < 1 || q->M > kMaxRows || q->n_store < 1 || q->K < 1 || q->K > (1 << 24) || q->slice_len < 1 || q->slice_len > 80 ||
        q->n_slices < 1 || q->n_slices > 65535 || q->n_cb < 1 || q->n_cb > 65535 || q->nz < 0 || q->nz > 65535)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_gemm: M %d, n_store %d, K %d, %d slices of %d, %d column blocks, nz %d", q->M, q->n_store,
                 q->K, q->n_slices, q->slice_len, q->n_cb, q->nz);
    if (q->a_row_stride < 0 || q->a_row_stride > kMaxStride || q->a_part_stride < 0 || q->a_part_stride > kMaxStride ||
        q->c_part_stride < 0 || q->c_part_stride > kMaxStride || q->ldc < 1 || q->ldc > kMaxStride || q->a_gdiv < 0 || q->a_gmul < 0 ||
        q->a_gmul > kMaxStride)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_gemm: a stride or the row map is negative or above 2^31");
    // what dcs_launch_lat_gemm refuses
    const int J = dcs_lat_j(q->slice_len);
    const int nz = q->nz > 1 ? q->nz : 1;
    const int waves = (q->n_slices + nz - 1) / nz;
    if (waves < 4 || waves > 16 || (q->slice_len & 3) || (q->K & 3) || (q->a_row_stride & 3) || (q->a_part_stride & 3) || J < 1 || J > 5 ||
        (q->a_parts != 1 && q->a_parts != 4))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_gemm: %d slices of %d over %d workgroups (4 .. 16 waves each), K %d, row stride %lld, %d parts %lld apart",
                 q->n_slices, q->slice_len, nz, q->K, (long long)q->a_row_stride, q->a_parts, (long long)q->a_part_stride);
    if (q->n_store > q->n_cb * 16 || q->n_store > q->ldc)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_gemm: n_store %d against %d columns and ldc %lld", q->n_store, q->n_cb * 16, (long long)q->ldc);
    const int64_t c_part = (int64_t)(q->M - 1) * q->ldc + q->n_store;
    if (nz > 1 && q->c_part_stride < c_part)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_gemm: c_part_stride %lld below one part of %lld floats", (long long)q->c_part_stride, (long long)c_part);
    if (bad_ptr(q->A, 15) || bad_ptr(q->Bp, 15) || bad_ptr(q->bias, 15) || bad_ptr(q->C, 15))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_gemm: a pointer is null or not aligned to 16 bytes");
    // the highest element each operand can be asked for (the lowest is element 0: no stride is negative)
    int64_t top_row = 0;
    for (int r = 0; r < q->M; ++r) {
        const int64_t arow = q->a_gdiv > 0 ? (int64_t)(r / q->a_gdiv) * q->a_gmul + r % q->a_gdiv : r;
        if (arow > top_row) top_row = arow;
    }
    const int64_t parts_off = (int64_t)(q->a_parts - 1) * q->a_part_stride;
    int64_t need_A = top_row * q->a_row_stride + q->K + parts_off;
    if (need_A < 4 + parts_off) need_A = 4 + parts_off;                       // lanes without an operand read A[0 .. 3] of every part
    const int64_t need_Bp = (int64_t)q->n_slices * q->n_cb * J * 256;
    const int64_t need_bias = (int64_t)q->n_cb * 16;                           // read past n_store
    const int64_t need_C = (int64_t)(nz - 1) * q->c_part_stride + c_part;
    if (q->n_A < need_A || q->n_Bp < need_Bp || q->n_bias < need_bias || q->n_C < need_C)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_gemm: A %lld of %lld floats, Bp %lld of %lld, bias %lld of %lld, C %lld of %lld", (long long)q->n_A,
                 (long long)need_A, (long long)q->n_Bp, (long long)need_Bp, (long long)q->n_bias, (long long)need_bias, (long long)q->n_C,
                 (long long)need_C);

    DcsLatGemm g{};
    g.A = q->A; g.a_row_stride = q->a_row_stride; g.a_scale = q->a_scale; g.Bp = q->Bp; g.bias = q->bias;
    g.C = q->C; g.ldc = q->ldc; g.M = q->M; g.n_store = q->n_store; g.K = q->K; g.slice_len = q->slice_len;
    g.n_slices = q->n_slices; g.n_cb = q->n_cb; g.relu = q->relu;
    g.nz = q->nz; g.c_part_stride = q->c_part_stride;
    g.a_parts = q->a_parts; g.a_part_stride = q->a_part_stride; g.relu_in = q->relu_in;
    g.a_gdiv = q->a_gdiv; g.a_gmul = q->a_gmul;
    DCS_ON_DEVICE(ctx->device);
    DCS_CHECK(dcs_launch_lat_gemm(ctx, g, DCS_TAG_CONV1));
    DCS_HIP(hipStreamSynchronize(ctx->stream));
    q->J = J; q->NA = q->a_parts;
    q->grid_x = dcs_cdiv(q->M, 16); q->grid_y = q->n_cb; q->grid_z = nz; q->block_x = waves * 64;
    return DCS_OK;
}

DCS_API int dcs_debug_lat_stft_forward_f32(dcs_stft* p, const float* audio_d, int64_t n_audio, int64_t n_samples, float* mag_d,
                                           float* phase_d, float* unit_d, int64_t n_rows_elems, int64_t ld, int64_t rows_out) {
    if (!p || !p->ctx) DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_forward: null plan");
    if (!dcs_lat_stft_supported(p)) DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_forward: frameSize %d / hop %d", p->frame, p->hop);
    if (bad_ptr(audio_d, 3) || bad_ptr(mag_d, 3) || (phase_d && bad_ptr(phase_d, 3)) || bad_ptr(unit_d, 7))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_forward: a pointer is null or not aligned (samples, magnitudes, phases 4 bytes, phasors 8)");
    if (n_samples < 1 || n_samples > n_audio || n_samples > ((int64_t)1 << 40))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_forward: %lld samples in a buffer of %lld", (long long)n_samples, (long long)n_audio);
    const int64_t T = dcs_frame_count(n_samples, p->hop);
    if (rows_out < T || rows_out > (1 << 24)) DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_forward: %lld rows for %lld frames", (long long)rows_out, (long long)T);
    if (ld < p->frame / 2 + 1 || ld > (1 << 20)) DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_forward: ld %lld", (long long)ld);
    if (n_rows_elems < rows_out * ld)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_forward: outputs of %lld elements, %lld rows of %lld", (long long)n_rows_elems, (long long)rows_out,
                 (long long)ld);
    DCS_ON_DEVICE(p->ctx->device);
    DCS_CHECK(dcs_launch_lat_stft(p, audio_d, n_samples, mag_d, phase_d, reinterpret_cast<float2*>(unit_d), ld, rows_out, T));
    DCS_HIP(hipStreamSynchronize(p->ctx->stream));
    return DCS_OK;
}

DCS_API int dcs_debug_lat_stft_inverse_f32(dcs_stft* p, const float* mag_d, int64_t n_mag, int64_t src_stride, const float* unit_d,
                                           int64_t n_unit, int64_t ld, int64_t n_frames, int n_src, float pre_div, float* audio_d,
                                           int64_t n_audio, int64_t n_out, float* frames_d, int64_t frames_bytes) {
    if (!p || !p->ctx) DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_inverse: null plan");
    if (!dcs_lat_stft_supported(p)) DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_inverse: frameSize %d / hop %d", p->frame, p->hop);
    if (bad_ptr(mag_d, 3) || bad_ptr(unit_d, 7) || bad_ptr(audio_d, 3) || bad_ptr(frames_d, 7))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_inverse: a pointer is null or not aligned (magnitudes, samples 4 bytes, phasors, frames 8)");
    if (n_frames < 1 || n_frames > (1 << 24) || n_src < 1 || n_src > 65535 || n_out < 1 || n_out > ((int64_t)1 << 36) || src_stride < 0 ||
        src_stride > ((int64_t)1 << 40))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_inverse: %lld frames, %d sources %lld apart, %lld samples", (long long)n_frames, n_src,
                 (long long)src_stride, (long long)n_out);
    const int64_t bins = p->frame / 2 + 1;
    if (ld < bins || ld > (1 << 20)) DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_inverse: ld %lld", (long long)ld);
    if (!(pre_div != 0.f) || !std::isfinite(pre_div)) DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_inverse: pre_div");
    if (n_src > 1 && src_stride < n_frames * ld) DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_inverse: src_stride < n_frames * ld");
    const int64_t rows = (n_frames - 1) * ld + bins;                            // the last row is read up to the Nyquist bin
    const int64_t need_mag = (int64_t)(n_src - 1) * src_stride + rows;
    if (n_mag < need_mag || n_unit < rows || n_audio < (int64_t)n_src * n_out)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_inverse: magnitudes %lld of %lld floats, phasors %lld of %lld pairs, samples %lld of %lld",
                 (long long)n_mag, (long long)need_mag, (long long)n_unit, (long long)rows, (long long)n_audio, (long long)n_src * n_out);
    if (frames_bytes < 0 || (uint64_t)frames_bytes < (uint64_t)dcs_lat_istft_scratch_bytes(p, n_frames, n_src))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_lat_stft_inverse: frames scratch of %lld bytes, %lld needed", (long long)frames_bytes,
                 (long long)dcs_lat_istft_scratch_bytes(p, n_frames, n_src));
    DCS_ON_DEVICE(p->ctx->device);
    DCS_CHECK(dcs_launch_lat_istft(p, mag_d, src_stride, reinterpret_cast<const float2*>(unit_d), ld, n_frames, n_src, pre_div, audio_d, n_out,
                                   frames_d));
    DCS_HIP(hipStreamSynchronize(p->ctx->stream));
    return DCS_OK;
}

}  // extern "C"

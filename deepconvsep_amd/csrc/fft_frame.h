// What the rendered-feature kernels (fft_render.hip: stft_render_kernel; fft_score_render.hip: stft_score_render_kernel,
// stft_score_informed_kernel) share around the FFT body of fft_lds.h.  A renderer is a SAMPLE SOURCE -- sample q of the
// workgroup's channel -- and, where it needs them, a prepare step before render_frame (values the source reads from LDS)
// and a tail of its own after it; the feed's window decode, the zero row, the frame itself, the launch and the life of a
// call's own device table are here, once.  Internal linkage.
#pragma once
#include "fft_lds.h"

#include <vector>

namespace {

// Window blockIdx.x / tc of a feed's table (file, first frame): batch row b, frame tt of the window = frame t of file fi.
// Not live (a zero row): file < 0, file >= n_files, or a negative frame.
struct FeedWindow {
    int64_t b, fi, t;
    int tt;
    bool live;
};

__device__ __forceinline__ FeedWindow feed_window(const int* __restrict__ windows, int tc, int n_files) {
    const int64_t b = blockIdx.x / tc;
    const int tt = (int)(blockIdx.x - b * tc);
    const int64_t fi = windows[2 * b], t = (int64_t)windows[2 * b + 1] + tt;
    return {b, fi, t, tt, fi >= 0 && fi < n_files && t >= 0};
}

// the row of a dead window or of a frame past T
template <typename R>
__device__ __forceinline__ void zero_row(R* __restrict__ orow, int64_t ld) {
    for (int k = threadIdx.x; k < ld; k += kThreads) orow[k] = R(0);
}

// One windowed frame, transformed.  smem = buf0 | buf1 | twiddles (the last only with tw_lds: staged with the frame, as
// stft_forward_kernel does, and `tw` then points there).  buf0[m] = (s(base + 2m) win[2m], s(base + 2m + 1) win[2m + 1]),
// then fft_lds; returns Z for packed_real_mag_row.  READS_LDS: the source reads what the workgroup wrote to LDS just before
// the call, so a barrier comes before the loads.  Every thread of the workgroup calls it; it ends with a barrier.
template <typename R, typename R2, bool READS_LDS, typename Sample>
__device__ __forceinline__ const R2* render_frame(char* smem, const R* __restrict__ win, const R2* __restrict__& tw, int tw_lds,
                                                  int M, int log2m, int64_t base, Sample sample) {
    const int tid = threadIdx.x;
    R2* buf0 = reinterpret_cast<R2*>(smem);
    R2* buf1 = buf0 + M;
    if (tw_lds) {
        R2* twl = buf1 + M;
        for (int k = tid; k <= M; k += kThreads) twl[k] = tw[k];
        tw = twl;
    }
    if (READS_LDS) __syncthreads();
    for (int m = tid; m < M; m += kThreads) {
        const int64_t q = base + 2 * m;
        const R x0 = sample(q) * win[2 * m];
        const R x1 = sample(q + 1) * win[2 * m + 1];
        buf0[m] = mk<R2, R>(x0, x1);
    }
    __syncthreads();
    return fft_lds<R, R2, -1>(buf0, buf1, tw, M, log2m);
}

// Launch of a frame kernel whose parameter list ends (.., win, tw, N, hop, log2m, sqrt_n, tw_lds): grid (blocks, 1 + S),
// LDS = buf0 | buf1 | twiddles where that fits 64 KiB (float64 at N = 4096 does not: the twiddles stay in global memory).
template <typename R, typename R2, typename Kern, typename... Args>
int launch_frames(dcs_stft* p, Kern kern, int64_t blocks, int S, const R* win, const R2* tw, Args... args) {
    const int M = p->frame / 2;
    size_t lds = (3 * (size_t)M + 1) * sizeof(R2);
    const int tw_lds = lds <= 64 * 1024;
    if (!tw_lds) lds = 2 * (size_t)M * sizeof(R2);
    if (lds > 48 * 1024)
        DCS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds));
    DcsTimer tm(p->ctx, DCS_TAG_STFT);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)(1 + S)), dim3(kThreads), lds, p->ctx->stream, args..., win, tw,
                       p->frame, p->hop, p->log2m, (R)sqrt((double)p->frame), tw_lds);
    tm.done();
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

// A host table that is one call's own: uploaded, read by what launch(table_d) enqueues on the plan's stream, waited for
// and given back.  `who` names the entry point and `what` the table in the two messages.
template <typename Launch>
int with_own_table(dcs_stft* p, const std::vector<int64_t>& tab, const char* name, const char* who, const char* what,
                   Launch launch) {
    void* tab_d = nullptr;
    DCS_HIP(dcs_dev_alloc(&tab_d, tab.size() * sizeof(int64_t), name));
    int rc = DCS_OK;
    if (hipMemcpy(tab_d, tab.data(), tab.size() * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess) {
        dcs_set_error("%s: uploading the %s table failed", who, what);
        rc = DCS_EHIP;
    }
    if (rc == DCS_OK) rc = launch((const int64_t*)tab_d);
    if (hipStreamSynchronize(p->ctx->stream) != hipSuccess && rc == DCS_OK) {
        dcs_set_error("%s: the launch failed", who);
        rc = DCS_EHIP;
    }
    dcs_dev_free(tab_d);
    return rc;
}

}  // namespace

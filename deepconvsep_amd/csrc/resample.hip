// dcs_resample_f32: sample-rate conversion by a rational factor up / down with a windowed-sinc filter the host designs
// (deepconvsep_amd/resample.py; include/dcs.h has the definition, DESIGN.md section 4 the numbers):
//   y[m] = sum_n x[n] h[m down - n up],   |m down - n up| <= H,  0 <= n < n_in
//
// Output m has phase p = (m down) mod up and n0 = (m down) / up; its taps are h[p + j up] at n = n0 - j.  The plan stores, for
// every phase, those taps in ASCENDING n (tap i of phase p belongs to n = n0 + first[p] + i, i < count[p]) as one row of
// kpad = round_up(max count, 4) floats: a lane reads its row with 16-byte loads.
//
// A workgroup owns kThreads consecutive outputs of one clip, one per lane.  It first stages the input span those outputs touch
// in LDS -- the only loads from the signal, each one checked against [0, n_in), zeros stored for what lies outside -- and every
// lane then runs ONE float32 fmaf chain over its taps in ascending n, starting from 0.  fmaf(0, h, acc) is acc, so the zeros of
// the span are the terms the definition leaves out, and the order of one output's sum is a function of (up, down, H) alone:
// not of n_in, the clip count, the strides or the lane the output lands on.
//
// The table is up x kpad floats (43 KB for 160/147, 117 KB for 441/320) and a workgroup of 256 outputs touches every phase
// of it.  Two placements, the same arithmetic: the workgroup copies the whole table into LDS once and then walks over chunks
// of 1024 outputs (one workgroup per CU, rows read with ds_read_b128), or every lane reads its row from global memory, where
// the table stays in L2 (256 outputs per workgroup).  DESIGN.md has both times; DCS_RESAMPLE_TABLE=lds|l2 in the environment
// when the plan is made overrides the choice (scripts/bench_resample.py).
#include "dcs_internal.h"

#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace {

constexpr int kThreadsL2 = 256;                       // outputs of a workgroup, table rows from global memory
constexpr int kThreadsLds = 1024;                     // ... table in LDS: four waves per SIMD next to a table that fills the CU
constexpr int64_t kMaxTableBytes = 1 << 20;           // up x kpad float32
constexpr int kMaxFactor = 1 << 20;                   // up, down: (kThreadsLds - 1) * down + up stays below 2^31
constexpr int64_t kLdsL2 = 64 * 1024;                 // the span alone
constexpr int64_t kLdsAll = 160 * 1024;               // table + span

struct ResampleArgs {
    const float* in;
    float* out;
    const float* taps;        // [up][kpad]
    const int2* phase;        // [up] {first, count}
    int64_t n_in, n_out, in_stride, out_stride;
    int64_t chunks_per_clip, n_chunks;
    int up, down, kpad;
    int min_first;            // min over the phases of first[p]
    int span;                 // floats of LDS a chunk's input takes
};

template <bool TABLE_LDS, int THREADS>
__global__ __launch_bounds__(THREADS) void resample_kernel(ResampleArgs a) {
    extern __shared__ float4 lds4[];
    const int tid = threadIdx.x;
    const int tab_floats = TABLE_LDS ? a.up * a.kpad : 0;          // a multiple of 4
    float* xs = (float*)lds4 + tab_floats;
    if (TABLE_LDS) {
        const float4* src = (const float4*)a.taps;
        for (int i = tid; i < tab_floats / 4; i += THREADS) lds4[i] = src[i];
    }
    for (int64_t b = blockIdx.x; b < a.n_chunks; b += gridDim.x) {
        const int64_t clip = b / a.chunks_per_clip;
        const int64_t m0 = (b - clip * a.chunks_per_clip) * THREADS;
        const int64_t q0 = m0 * a.down;
        const int64_t n0_base = q0 / a.up;
        const unsigned p0 = (unsigned)(q0 - n0_base * a.up);
        const int64_t n_lo = n0_base + a.min_first;                // the lowest n any lane of the chunk touches
        const float* x = a.in + clip * a.in_stride;
        for (int i = tid; i < a.span; i += THREADS) {
            const int64_t n = n_lo + i;
            xs[i] = (n >= 0 && n < a.n_in) ? x[n] : 0.f;
        }
        __syncthreads();
        const int64_t m = m0 + tid;
        if (m < a.n_out) {
            const unsigned q = p0 + (unsigned)tid * (unsigned)a.down;
            const unsigned dn = q / (unsigned)a.up;
            const int p = (int)(q - dn * (unsigned)a.up);
            const int2 ph = a.phase[p];
            const float* xp = xs + ((int)dn + ph.x - a.min_first);
            const float4* row = TABLE_LDS ? (const float4*)((const float*)lds4 + (size_t)p * a.kpad)
                                          : (const float4*)(a.taps + (size_t)p * a.kpad);
            const int whole = ph.y >> 2, rest = ph.y & 3;
            float acc = 0.f;
            for (int c = 0; c < whole; ++c) {
                const float4 h = row[c];
                acc = fmaf(xp[4 * c + 0], h.x, acc);
                acc = fmaf(xp[4 * c + 1], h.y, acc);
                acc = fmaf(xp[4 * c + 2], h.z, acc);
                acc = fmaf(xp[4 * c + 3], h.w, acc);
            }
            if (rest) {
                const float4 h = row[whole];
                acc = fmaf(xp[4 * whole + 0], h.x, acc);
                if (rest > 1) acc = fmaf(xp[4 * whole + 1], h.y, acc);
                if (rest > 2) acc = fmaf(xp[4 * whole + 2], h.z, acc);
            }
            a.out[clip * a.out_stride + m] = acc;
        }
        __syncthreads();                                           // the span is rewritten by the next chunk
    }
}

// ------------------------------------------------------------------------------------------ the stream (dcs_resample_stream)
constexpr int kMaxStreamRows = 64;

// samples [p0, p0 + n) of row blockIdx.y into slot (absolute index) mod cap of its ring
__global__ __launch_bounds__(kThreadsL2) void resample_stream_append_kernel(const float* __restrict__ in, int64_t in_stride,
                                                                           int64_t n, int64_t p0, float* __restrict__ ring,
                                                                           int64_t cap) {
    const int64_t i = (int64_t)blockIdx.x * kThreadsL2 + threadIdx.x;
    if (i < n) ring[blockIdx.y * cap + (p0 + i) % cap] = in[blockIdx.y * in_stride + i];
}

// Output m = m0 + i of row blockIdx.y: resample_kernel's chain -- one fmaf per tap of the phase row in ascending n, starting
// from 0, zero for n outside [0, lim) -- with the samples read from the ring by their ABSOLUTE index.  lim = the samples pushed
// so far: mid-stream only outputs whose every tap lies below it are asked for, so lim acts only after the end, as n_in does.
__global__ __launch_bounds__(kThreadsL2) void resample_stream_kernel(const float* __restrict__ ring, int64_t cap, int64_t lim,
                                                                    const float* __restrict__ taps,
                                                                    const int2* __restrict__ phase, int up, int down, int kpad,
                                                                    int64_t m0, int64_t n_out, float* __restrict__ out,
                                                                    int64_t out_stride) {
    const int64_t i = (int64_t)blockIdx.x * kThreadsL2 + threadIdx.x;
    if (i >= n_out) return;
    const int64_t q = (m0 + i) * down;
    const int64_t n0 = q / up;
    const int p = (int)(q - n0 * up);
    const int2 ph = phase[p];
    const float* row = taps + (size_t)p * kpad;
    const float* x = ring + blockIdx.y * cap;
    const int64_t n_first = n0 + ph.x;
    float acc = 0.f;
    for (int j = 0; j < ph.y; ++j) {
        const int64_t n = n_first + j;
        const float v = (n >= 0 && n < lim) ? x[n % cap] : 0.f;
        acc = fmaf(v, row[j], acc);
    }
    out[blockIdx.y * out_stride + i] = acc;
}

int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// floats of input the outputs of `threads` consecutive lanes reach: the largest n0 - n0_base plus the widest row
int64_t span_floats(int threads, int up, int down, int min_first, int max_end) {
    return ((int64_t)(up - 1) + (int64_t)(threads - 1) * down) / up + (max_end - min_first);
}

}  // namespace

struct dcs_resampler {
    dcs_ctx* ctx = nullptr;
    int up = 1, down = 1, kpad = 0;
    int min_first = 0, max_end = 0;       // over the phases: min first[p], max first[p] + count[p]
    int64_t half = 0;                     // the filter's half-width: what a stream sizes its history by
    bool table_lds = false;
    float* taps_d = nullptr;
    int2* phase_d = nullptr;
};

extern "C" int64_t dcs_resample_length(int64_t n_samples, int up, int down) {
    if (n_samples < 0 || up < 1 || down < 1 || n_samples > (INT64_MAX - down) / up) return -1;
    return (n_samples * up + down - 1) / down;
}

extern "C" int dcs_resample_plan(dcs_ctx* ctx, int up, int down, const double* taps_h, int64_t half, dcs_resampler** out) {
    if (up < 1 || down < 1 || half < 0)
        DCS_FAIL(DCS_EINVAL, "dcs_resample_plan: up %d, down %d must be >= 1 and half %lld >= 0", up, down, (long long)half);
    if (!ctx || !taps_h || !out) DCS_FAIL(DCS_EINVAL, "dcs_resample_plan: null argument");
    if (up > kMaxFactor || down > kMaxFactor)
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_resample_plan: up %d / down %d above %d", up, down, kMaxFactor);
    // rows of the polyphase table: phase p has the taps t = p + j up, jmin <= j <= jmax, |t| <= half
    const int64_t kmax = (2 * half) / up + 1;
    const int64_t kpad = dcs_round_up(kmax, 4);
    if ((int64_t)up * kpad * (int64_t)sizeof(float) > kMaxTableBytes)
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_resample_plan: the polyphase table (%d phases x %lld taps, float32) is above %lld bytes", up,
                 (long long)kpad, (long long)kMaxTableBytes);
    std::vector<float> tab((size_t)up * kpad, 0.f);
    std::vector<int2> phase(up);
    int min_first = INT_MAX, max_end = INT_MIN;
    for (int p = 0; p < up; ++p) {
        const int64_t jmax = floor_div(half - p, up), jmin = -floor_div(half + p, up);
        const int64_t count = jmax >= jmin ? jmax - jmin + 1 : 0;
        phase[p].x = (int)-jmax;
        phase[p].y = (int)count;
        for (int64_t i = 0; i < count; ++i) tab[(size_t)p * kpad + i] = (float)taps_h[half + p + (jmax - i) * up];
        if (count) {
            min_first = std::min(min_first, phase[p].x);
            max_end = std::max(max_end, phase[p].x + phase[p].y);
        }
    }
    if (min_first == INT_MAX) min_first = max_end = 0;          // cannot happen: phase 0 always holds t = 0
    const int64_t tab_bytes = (int64_t)tab.size() * (int64_t)sizeof(float);
    const int64_t lds_l2 = span_floats(kThreadsL2, up, down, min_first, max_end) * (int64_t)sizeof(float);
    const int64_t lds_all = tab_bytes + span_floats(kThreadsLds, up, down, min_first, max_end) * (int64_t)sizeof(float);
    if (lds_l2 > kLdsL2)
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_resample_plan: %d outputs of %d/%d reach over %lld bytes of input, above the %lld of a "
                 "workgroup", kThreadsL2, up, down, (long long)lds_l2, (long long)kLdsL2);
    bool table_lds = lds_all <= kLdsAll;
    if (const char* e = getenv("DCS_RESAMPLE_TABLE")) {
        if (!strcmp(e, "l2")) table_lds = false;
        else if (strcmp(e, "lds") || !table_lds)
            DCS_FAIL(DCS_EINVAL, "dcs_resample_plan: DCS_RESAMPLE_TABLE=%s (lds, where table and span fit %lld bytes, or l2)", e,
                     (long long)kLdsAll);
    }
    DCS_ON_DEVICE(ctx->device);
    dcs_resampler* r = new dcs_resampler();
    r->ctx = ctx;
    r->up = up;
    r->down = down;
    r->kpad = (int)kpad;
    r->min_first = min_first;
    r->max_end = max_end;
    r->half = half;
    r->table_lds = table_lds;
    auto upload = [&](void** dst, const void* src, size_t bytes, const char* name) -> int {
        DCS_HIP(dcs_dev_alloc(dst, bytes, name));
        DCS_HIP(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
        return DCS_OK;
    };
    int rc = DCS_OK;
    if ((rc = upload((void**)&r->taps_d, tab.data(), (size_t)tab_bytes, "resample.taps")) ||
        (rc = upload((void**)&r->phase_d, phase.data(), (size_t)up * sizeof(int2), "resample.phase"))) {
        dcs_resample_plan_destroy(r);
        return rc;
    }
    *out = r;
    return DCS_OK;
}

extern "C" int dcs_resample_plan_destroy(dcs_resampler* r) {
    if (!r) return DCS_OK;
    DCS_ON_DEVICE(r->ctx->device);
    dcs_dev_free(r->taps_d);
    dcs_dev_free(r->phase_d);
    delete r;
    return DCS_OK;
}

extern "C" int dcs_resample_f32(dcs_resampler* r, const float* in_d, int64_t n_in, int64_t n_clips, int64_t in_stride,
                                float* out_d, int64_t out_stride) {
    if (!r) DCS_FAIL(DCS_EINVAL, "dcs_resample_f32: null plan");
    if (n_in < 0 || n_clips < 0) DCS_FAIL(DCS_EINVAL, "dcs_resample_f32: negative size");
    if (n_in == 0 || n_clips == 0) return DCS_OK;
    const int64_t n_out = dcs_resample_length(n_in, r->up, r->down);
    if (n_out < 0) DCS_FAIL(DCS_EINVAL, "dcs_resample_f32: %lld samples x %d overflow", (long long)n_in, r->up);
    if (!in_d || !out_d) DCS_FAIL(DCS_EINVAL, "dcs_resample_f32: null buffer");
    if (n_clips > 1 && (in_stride < n_in || out_stride < n_out))
        DCS_FAIL(DCS_EINVAL, "dcs_resample_f32: strides %lld / %lld below the lengths %lld / %lld", (long long)in_stride,
                 (long long)out_stride, (long long)n_in, (long long)n_out);
    dcs_ctx* ctx = r->ctx;
    DCS_ON_DEVICE(ctx->device);

    ResampleArgs a;
    a.in = in_d;
    a.out = out_d;
    a.taps = r->taps_d;
    a.phase = r->phase_d;
    a.n_in = n_in;
    a.n_out = n_out;
    a.in_stride = in_stride;
    a.out_stride = out_stride;
    a.up = r->up;
    a.down = r->down;
    a.kpad = r->kpad;
    a.min_first = r->min_first;
    const int threads = r->table_lds ? kThreadsLds : kThreadsL2;
    a.span = (int)span_floats(threads, r->up, r->down, r->min_first, r->max_end);
    a.chunks_per_clip = (n_out + threads - 1) / threads;
    if (a.chunks_per_clip > INT_MAX / n_clips)
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_resample_f32: %lld clips of %lld outputs are more than 2^31 workgroups", (long long)n_clips,
                 (long long)n_out);
    a.n_chunks = a.chunks_per_clip * n_clips;
    if (r->table_lds) {
        auto kern = resample_kernel<true, kThreadsLds>;
        static DcsOncePerDevice once;
        DCS_CHECK(once.run(ctx->device, [&]() -> int {
            DCS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)kLdsAll));
            return DCS_OK;
        }));
        const size_t lds = ((size_t)r->up * r->kpad + a.span) * sizeof(float);
        const int grid = (int)std::min<int64_t>(a.n_chunks, ctx->n_cu);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreadsLds), lds, ctx->stream, a);
    } else {
        hipLaunchKernelGGL((resample_kernel<false, kThreadsL2>), dim3((unsigned)a.n_chunks), dim3(kThreadsL2),
                           (size_t)a.span * sizeof(float), ctx->stream, a);
    }
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

// ------------------------------------------------------------------------------------------ the stream
// `rows` signals in lock-step on one plan.  A push appends its samples to a ring per row and computes the outputs that became
// final: output m is final once every tap of it lies below the P samples pushed, m down + half < P up, and after the end the
// outputs are the ceil(L up / down) of dcs_resample_f32.  An output not yet emitted reaches back less than 2 half / up + 2
// samples behind P, so a ring of max_push + 2 half / up + 2 samples holds everything a push reads.
struct dcs_resample_stream {
    dcs_resampler* r = nullptr;
    dcs_ctx* ctx = nullptr;
    int rows = 0;
    int64_t max_push = 0, cap = 0, bytes = 0;
    float* ring = nullptr;
    int64_t P = 0, M = 0;        // samples pushed, outputs emitted
    bool ended = false;
};

extern "C" int dcs_resample_stream_create(dcs_resampler* r, int rows, int64_t max_push, dcs_resample_stream** out) {
    if (!r || !out) DCS_FAIL(DCS_EINVAL, "dcs_resample_stream_create: null argument");
    if (rows < 1 || rows > kMaxStreamRows)
        DCS_FAIL(DCS_EINVAL, "dcs_resample_stream_create: %d rows (1 .. %d)", rows, kMaxStreamRows);
    if (max_push < 1 || max_push > (1LL << 30))
        DCS_FAIL(DCS_EINVAL, "dcs_resample_stream_create: max_push %lld not in [1, 2^30]", (long long)max_push);
    DCS_ON_DEVICE(r->ctx->device);
    dcs_resample_stream* s = new dcs_resample_stream();
    s->r = r;
    s->ctx = r->ctx;
    s->rows = rows;
    s->max_push = max_push;
    s->cap = max_push + (2 * r->half) / r->up + 2;
    s->bytes = (int64_t)rows * s->cap * (int64_t)sizeof(float);
    const hipError_t e = dcs_dev_alloc((void**)&s->ring, (size_t)s->bytes, "resample.stream");
    if (e != hipSuccess) {
        dcs_set_error("dcs_resample_stream_create: %lld bytes: %s", (long long)s->bytes, hipGetErrorString(e));
        delete s;
        return e == hipErrorOutOfMemory ? DCS_ENOMEM : DCS_EHIP;
    }
    *out = s;
    return DCS_OK;
}

extern "C" int dcs_resample_stream_destroy(dcs_resample_stream* s) {
    if (!s) return DCS_OK;
    DCS_ON_DEVICE(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    dcs_dev_free(s->ring);
    delete s;
    return DCS_OK;
}

extern "C" int dcs_resample_stream_reset(dcs_resample_stream* s) {
    if (!s) DCS_FAIL(DCS_EINVAL, "dcs_resample_stream_reset: null stream");
    // the ring keeps its contents: no slot is read before the push that needs it has written it
    s->P = s->M = 0;
    s->ended = false;
    return DCS_OK;
}

extern "C" int64_t dcs_resample_stream_bytes(const dcs_resample_stream* s) { return s ? s->bytes : -1; }

extern "C" int dcs_resample_stream_push(dcs_resample_stream* s, const float* in_d, int64_t in_stride, int64_t n, int last,
                                        float* out_d, int64_t out_stride, int64_t out_cap, int64_t* n_out) {
    if (!s) DCS_FAIL(DCS_EINVAL, "dcs_resample_stream_push: null stream");
    if (s->ended) DCS_FAIL(DCS_EINVAL, "dcs_resample_stream_push: the signal has ended (dcs_resample_stream_reset starts another)");
    if (n < 0 || n > s->max_push)
        DCS_FAIL(DCS_EINVAL, "dcs_resample_stream_push: %lld samples (0 .. max_push = %lld)", (long long)n, (long long)s->max_push);
    if (n > 0 && !in_d) DCS_FAIL(DCS_EINVAL, "dcs_resample_stream_push: null input");
    const dcs_resampler* r = s->r;
    const int64_t P = s->P + n;
    if (P > (INT64_MAX - r->down - r->half) / r->up)
        DCS_FAIL(DCS_EINVAL, "dcs_resample_stream_push: %lld samples x %d overflow", (long long)P, r->up);
    int64_t M;
    if (last) M = (P * r->up + r->down - 1) / r->down;
    else M = P * r->up - 1 - r->half < 0 ? 0 : (P * r->up - 1 - r->half) / r->down + 1;
    const int64_t n_new = M - s->M;
    if (n_new < 0) DCS_FAIL(DCS_EHIP, "dcs_resample_stream_push: internal count out of range (%lld outputs)", (long long)n_new);
    if (n_new > 0 && (!out_d || n_new > out_cap))
        DCS_FAIL(DCS_EINVAL, "dcs_resample_stream_push: %lld samples become final, room for %lld", (long long)n_new,
                 (long long)(out_d ? out_cap : 0));
    if (s->rows > 1 && ((n > 0 && in_stride < n) || (n_new > 0 && out_stride < n_new)))
        DCS_FAIL(DCS_EINVAL, "dcs_resample_stream_push: strides %lld / %lld below the counts %lld / %lld", (long long)in_stride,
                 (long long)out_stride, (long long)n, (long long)n_new);
    dcs_ctx* ctx = r->ctx;
    DCS_ON_DEVICE(ctx->device);
    if (n > 0) {
        hipLaunchKernelGGL(resample_stream_append_kernel, dim3((unsigned)dcs_cdiv(n, kThreadsL2), (unsigned)s->rows),
                           dim3(kThreadsL2), 0, ctx->stream, in_d, in_stride, n, s->P, s->ring, s->cap);
        DCS_HIP(hipGetLastError());
    }
    if (n_new > 0) {
        hipLaunchKernelGGL(resample_stream_kernel, dim3((unsigned)dcs_cdiv(n_new, kThreadsL2), (unsigned)s->rows),
                           dim3(kThreadsL2), 0, ctx->stream, (const float*)s->ring, s->cap, P, (const float*)r->taps_d,
                           (const int2*)r->phase_d, r->up, r->down, r->kpad, s->M, n_new, out_d, out_stride);
        DCS_HIP(hipGetLastError());
    }
    s->P = P;
    s->M = M;
    if (last) s->ended = true;
    if (n_out) *n_out = n_new;
    return DCS_OK;
}

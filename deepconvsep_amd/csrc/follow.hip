// dcs_follow_*: a score follower with constant memory -- online dynamic time warping, one row per audio frame (include/dcs.h
// has the contract, DESIGN.md section 4t the layout and the numbers).  dcs_dtw (align.hip) needs the whole recording and walks
// back from its last cell; here every chroma row that arrives takes ONE forward step over a window of W score frames and the
// position the performance has reached comes out with it.  Nothing of size T x U exists.
//
// A push of n frames is ONE launch of ONE workgroup of W threads; the frames are a counted loop inside it.
//   thread i owns the window cell u with u = i (mod W): when the window moves forward the cells that leave it hand their
//   thread to the cells that enter, nobody else changes cell.  The cell's score row sits in 12 registers and is reloaded only
//   then.  The frame's chroma row is one uniform read.  The previous row goes round through an LDS array of W floats (two of
//   them, taken in turn): thread i reads the slots i - 1 .. i - K.  The row's minimum and the lowest cell that attains it: a
//   butterfly over the wave on (value, cell), one LDS slot per wave, a barrier, then EVERY thread folds the W / 64 slots in
//   the same order, so q, p and the new window start are uniform without a broadcast.  Two barriers per frame: the waves'
//   minima, the new row.  The state -- the row, w0, p -- is read once at the start of the launch (not at all when the push
//   starts at frame 0: reset clears nothing on the device) and written once at its end.
// A frame's arithmetic does not depend on its place in the launch, so the bits are the same however the frames are cut into
// pushes.  What bounds the kernel is the serial chain of frames, not the work of one: 13 fused multiply-adds and K additions
// per cell against two barriers and a two-level reduction per frame.
#include "dcs_internal.h"

#include <limits.h>
#include <math.h>

namespace {

constexpr int kChroma = 12;
constexpr int kMaxWaves = 16;                            // W <= 1024
constexpr int64_t kMaxScore = (int64_t)1 << 30;          // cells and positions are int32 with room for + W

struct FollowArgs {
    const float* score;        // [U][12]
    const float* chroma;       // [n][12]
    int32_t* pos;              // [n]
    float* row;                // [W] state: slot i holds the window cell u = i (mod W), +inf past U
    int64_t* w0;               // state
    int32_t* p;                // state
    int64_t t0;                // frames pushed before this launch
    int n;
    int U, W, K, back;
    float lambda;
};

__device__ __forceinline__ void load_score_row(const float* __restrict__ score, int u, int U, float (&s)[kChroma]) {
#pragma unroll
    for (int k = 0; k < kChroma; ++k) s[k] = u < U ? score[(int64_t)u * kChroma + k] : 0.f;
}

__global__ __launch_bounds__(1024) void follow_kernel(FollowArgs a) {
    __shared__ float s_row[2][1024];
    __shared__ float s_min[kMaxWaves];
    __shared__ int s_arg[kMaxWaves];
    const int i = threadIdx.x, W = a.W, U = a.U, K = a.K;
    const int n_waves = W >> 6;
    const bool fresh = a.t0 == 0;
    int w0 = fresh ? 0 : (int)*a.w0;
    int p = fresh ? 0 : *a.p;
    // the window cell of this thread: the one u in [w0, w0 + W) with u = i (mod W)
    int u = w0 + ((i - w0 % W) + W) % W;
    float d = (fresh || u >= U) ? INFINITY : a.row[i];
    float s[kChroma];
    load_score_row(a.score, u, U, s);
    int cur = 0;
    s_row[0][i] = d;
    __syncthreads();

    for (int f = 0; f < a.n; ++f) {
        const float* __restrict__ ar = a.chroma + (int64_t)f * kChroma;
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < kChroma; ++k) dot = fmaf(ar[k], s[k], dot);
        const float c = __fsub_rn(1.0f, dot);
        float dn;
        if (a.t0 + f == 0) {
            dn = u == 0 ? c : INFINITY;
        } else {
            // cells below the window start (and below 0) are +inf; slot (i - k) mod W holds cell u - k when that is inside
            float best = u - 1 >= w0 ? s_row[cur][(i - 1 + W) % W] : INFINITY;
            best = fminf(best, __fadd_rn(d, a.lambda));
#pragma unroll
            for (int k = 2; k <= 4; ++k)
                if (k <= K) {
                    const float v = u - k >= w0 ? s_row[cur][(i - k + W) % W] : INFINITY;
                    best = fminf(best, __fadd_rn(v, a.lambda));
                }
            dn = u < U ? __fadd_rn(c, best) : INFINITY;
        }
        // the row's minimum and the lowest cell that attains it
        float mv = dn;
        int mu = u;
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) {
            const float ov = __shfl_xor(mv, sh);
            const int ou = __shfl_xor(mu, sh);
            if (ov < mv || (ov == mv && ou < mu)) {
                mv = ov;
                mu = ou;
            }
        }
        if ((i & 63) == 0) {
            s_min[i >> 6] = mv;
            s_arg[i >> 6] = mu;
        }
        __syncthreads();
        float m = s_min[0];
        int q = s_arg[0];
        for (int w = 1; w < n_waves; ++w) {
            const float ov = s_min[w];
            const int ou = s_arg[w];
            if (ov < m || (ov == m && ou < q)) {
                m = ov;
                q = ou;
            }
        }
        p = q > p ? q : p;
        d = __fsub_rn(dn, m);
        if (i == 0) a.pos[f] = p;
        // the window moves forward, tied to q; a cell that leaves hands its thread to the cell W further on, which enters at +inf
        int nw = q - a.back < U - W ? q - a.back : U - W;
        nw = nw > 0 ? nw : 0;
        w0 = nw > w0 ? nw : w0;
        if (u < w0) {
            u += W;
            d = INFINITY;
            load_score_row(a.score, u, U, s);
        }
        cur ^= 1;
        s_row[cur][i] = d;
        __syncthreads();
    }
    a.row[i] = d;
    if (i == 0) {
        *a.w0 = w0;
        *a.p = p;
    }
}

// row_out[j] = the cell w0 + j, +inf past U (and everywhere before the first frame)
__global__ __launch_bounds__(1024) void follow_row_kernel(const float* __restrict__ row, const int64_t* __restrict__ w0_s,
                                                          const int32_t* __restrict__ p_s, int fresh, int U, int W,
                                                          float* __restrict__ row_out, int64_t* __restrict__ w0_out,
                                                          int32_t* __restrict__ p_out) {
    const int j = threadIdx.x;
    const int64_t w0 = fresh ? 0 : *w0_s;
    const int64_t u = w0 + j;
    row_out[j] = (fresh || u >= U) ? INFINITY : row[u % W];
    if (j == 0) {
        *w0_out = w0;
        *p_out = fresh ? 0 : *p_s;
    }
}

}  // namespace

extern "C" int dcs_follow_create(dcs_ctx* ctx, const float* s_h, int64_t U, int W, int K, int back, float lambda,
                                 int64_t max_frames, dcs_follow** out) {
    if (!ctx || !s_h || !out) DCS_FAIL(DCS_EINVAL, "dcs_follow_create: null argument");
    if (U < 1 || max_frames < 1)
        DCS_FAIL(DCS_EINVAL, "dcs_follow_create: bad shape (U %lld, max_frames %lld)", (long long)U, (long long)max_frames);
    if (W < 64 || W > 1024 || W % 64) DCS_FAIL(DCS_EINVAL, "dcs_follow_create: window %d (a multiple of 64 in 64 .. 1024)", W);
    if (K < 1 || K > 4) DCS_FAIL(DCS_EINVAL, "dcs_follow_create: step %d (1 .. 4)", K);
    if (back < 0 || back >= W) DCS_FAIL(DCS_EINVAL, "dcs_follow_create: back %d not in [0, %d)", back, W);
    if (!(lambda >= 0.f) || !(lambda <= 3.402823466e+38f))
        DCS_FAIL(DCS_EINVAL, "dcs_follow_create: penalty %g must be finite and not negative", (double)lambda);
    if (U > kMaxScore || max_frames > INT_MAX)
        DCS_FAIL(DCS_ESHAPE, "dcs_follow_create: U %lld (at most %lld), max_frames %lld (at most %d)", (long long)U,
                 (long long)kMaxScore, (long long)max_frames, INT_MAX);
    DCS_ON_DEVICE(ctx->device);
    dcs_follow* f = new dcs_follow();
    f->ctx = ctx;
    f->U = U;
    f->W = W;
    f->K = K;
    f->back = back;
    f->lambda = lambda;
    f->max_frames = max_frames;
    // the score, then the state: the row, w0 (int64), p (int32)
    const int64_t b_score = dcs_round_up(U * kChroma * (int64_t)sizeof(float), 256);
    const int64_t b_row = (int64_t)W * (int64_t)sizeof(float);
    f->bytes = b_score + b_row + 256;
    char* base = nullptr;
    const hipError_t e = dcs_dev_alloc((void**)&base, (size_t)f->bytes, "follow");
    if (e != hipSuccess) {
        delete f;
        DCS_HIP(e);
    }
    f->score = (float*)base;
    f->row = (float*)(base + b_score);
    f->w0 = (int64_t*)(base + b_score + b_row);
    f->p = (int32_t*)(base + b_score + b_row + 8);
    if (hipMemcpy(f->score, s_h, (size_t)(U * kChroma) * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        dcs_dev_free(base);
        delete f;
        DCS_FAIL(DCS_EHIP, "dcs_follow_create: uploading the score failed");
    }
    *out = f;
    return DCS_OK;
}

extern "C" int dcs_follow_destroy(dcs_follow* f) {
    if (!f) return DCS_OK;
    DCS_ON_DEVICE(f->ctx->device);
    (void)hipStreamSynchronize(f->ctx->stream);
    dcs_dev_free(f->score);
    delete f;
    return DCS_OK;
}

extern "C" int dcs_follow_reset(dcs_follow* f) {
    if (!f) DCS_FAIL(DCS_EINVAL, "dcs_follow_reset: null handle");
    f->frames = 0;                                    // frame 0 reads no state: nothing to clear on the device
    return DCS_OK;
}

extern "C" int64_t dcs_follow_bytes(const dcs_follow* f) { return f ? f->bytes : -1; }
extern "C" int64_t dcs_follow_frames(const dcs_follow* f) { return f ? f->frames : -1; }

extern "C" int dcs_follow_push(dcs_follow* f, const float* chroma_d, int64_t n, int32_t* pos_d) {
    if (!f) DCS_FAIL(DCS_EINVAL, "dcs_follow_push: null handle");
    if (n < 0 || n > f->max_frames)
        DCS_FAIL(DCS_EINVAL, "dcs_follow_push: %lld frames (0 .. max_frames = %lld)", (long long)n, (long long)f->max_frames);
    if (n > 0 && (!chroma_d || !pos_d)) DCS_FAIL(DCS_EINVAL, "dcs_follow_push: null buffer");
    if (n == 0) return DCS_OK;
    DCS_ON_DEVICE(f->ctx->device);
    FollowArgs a;
    a.score = f->score;
    a.chroma = chroma_d;
    a.pos = pos_d;
    a.row = f->row;
    a.w0 = f->w0;
    a.p = f->p;
    a.t0 = f->frames;
    a.n = (int)n;
    a.U = (int)f->U;
    a.W = f->W;
    a.K = f->K;
    a.back = f->back;
    a.lambda = f->lambda;
    hipLaunchKernelGGL(follow_kernel, dim3(1), dim3((unsigned)f->W), 0, f->ctx->stream, a);
    DCS_HIP(hipGetLastError());
    f->frames += n;
    return DCS_OK;
}

extern "C" int dcs_follow_row(dcs_follow* f, float* row_d, int64_t* w0_d, int32_t* p_d) {
    if (!f || !row_d || !w0_d || !p_d) DCS_FAIL(DCS_EINVAL, "dcs_follow_row: null argument");
    DCS_ON_DEVICE(f->ctx->device);
    hipLaunchKernelGGL(follow_row_kernel, dim3(1), dim3((unsigned)f->W), 0, f->ctx->stream, (const float*)f->row,
                       (const int64_t*)f->w0, (const int32_t*)f->p, f->frames == 0 ? 1 : 0, (int)f->U, f->W, row_d, w0_d, p_d);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

// Score-to-audio alignment on the device: chroma features of a magnitude spectrogram (dcs_chroma) and dynamic time warping
// of two chroma sequences (dcs_dtw).  The reference has no counterpart: Bach10 ships hand-aligned scores.
//
// dcs_chroma: one wave per frame.  Lane l reads bins l, l + 64, ... of the row (coalesced) and adds each magnitude to the one of
// its twelve accumulators the bin's pitch class names; one butterfly over the wave adds the lanes' sums, then the row is divided
// by its Euclidean norm.  Columns F .. ld-1 are never read.  HBM-bound: n_frames * F * 4 B read.
//
// dcs_dtw: D[t,u] = c[t,u] + min(D[t-1,u-1], D[t-1,u], D[t,u-1]) over tiles of kTile x kTile cells, one wave per tile, lane = row.
// The wave walks the tile's columns skewed -- at step s lane l is at column s - l -- so that the upper and diagonal neighbours
// are what lane l - 1 computed one and two steps earlier (one __shfl_up per step) and the left neighbour is the lane's own last
// value: 2 kTile - 1 steps, no barrier inside.  The tile's score rows sit in LDS, the lane's audio row in registers.  Tiles
// hand their last row, last column and corner on through three strips in global memory; all tiles of one anti-diagonal of
// tiles are ONE launch and the stream orders the anti-diagonals: no kernel waits for another workgroup.  Every cell leaves a
// 2-bit direction code (16 bytes per lane, 1 KiB per tile, stored only for the tiles that touch the band); a last launch with a
// single walker follows the codes back from the end cell in a counted loop and writes the path in forward order.
#include "dcs_internal.h"

#include <limits.h>
#include <math.h>
#include <string.h>

#include <vector>

namespace {

constexpr int kTile = 64;            // cells per tile side == lanes of the wave
constexpr int kChroma = 12;
constexpr int kChromaWaves = 4;      // frames per workgroup of the chroma kernel
constexpr int64_t kMaxLen = 1 << 20; // longest sequence
constexpr int64_t kMaxBytes = (int64_t)1 << 31;

// ---------------------------------------------------------------------------------------------------------------- chroma
__global__ __launch_bounds__(kChromaWaves * 64) void chroma_kernel(const float* __restrict__ mag, int64_t ld, int64_t T, int F,
                                                                   const signed char* __restrict__ cls, float floor_v,
                                                                   float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * kChromaWaves + (threadIdx.x >> 6);
    if (t >= T) return;                                   // whole waves leave: the shuffles below see full waves
    const float* row = mag + t * ld;
    float acc[kChroma];
#pragma unroll
    for (int k = 0; k < kChroma; ++k) acc[k] = 0.f;
    for (int f = lane; f < F; f += 64) {
        const int c = cls[f];
        const float m = row[f];
#pragma unroll
        for (int k = 0; k < kChroma; ++k) acc[k] += c == k ? m : 0.f;
    }
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < kChroma; ++k) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc[k] += __shfl_xor(acc[k], d);
        sq = fmaf(acc[k], acc[k], sq);
    }
    const float n = sqrtf(sq);
    if (lane < kChroma) {
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < kChroma; ++k) v = lane == k ? acc[k] : v;
        out[t * kChroma + lane] = n > floor_v ? v / n : 0.288675134594812882f;   // 1 / sqrt(12)
    }
}

// ---------------------------------------------------------------------------------------------------------------- DTW
struct DtwGeom {
    int64_t T, U;
    int64_t band;      // < 0: none (also T == 1, where every cell is in the band)
    int64_t lim;       // band * (T - 1)
    int nTI, nTJ;      // tiles down (t) and across (u)
    int WT;            // code slots per row of tiles: the most tiles a row of tiles has in the band
};

// columns of tiles [*jlo, *jhi] that can hold in-band cells of the row of tiles I: cell (t, u) is in the band iff
// |u (T-1) - t (U-1)| <= band (T-1), i.e. ceil(t (U-1) / (T-1)) - band <= u <= floor(t (U-1) / (T-1)) + band
__host__ __device__ inline void dtw_row_tiles(const DtwGeom& g, int I, int* jlo, int* jhi) {
    if (g.band < 0) {
        *jlo = 0;
        *jhi = g.nTJ - 1;
        return;
    }
    const int64_t tm1 = g.T - 1, um1 = g.U - 1;
    const int64_t t0 = (int64_t)I * kTile, t1 = t0 + kTile - 1 < tm1 ? t0 + kTile - 1 : tm1;
    int64_t ulo = (t0 * um1 + tm1 - 1) / tm1 - g.band, uhi = t1 * um1 / tm1 + g.band;
    if (ulo < 0) ulo = 0;
    if (uhi > um1) uhi = um1;
    if (uhi < ulo) uhi = ulo;
    *jlo = (int)(ulo / kTile);
    *jhi = (int)(uhi / kTile);
}

struct DtwBufs {
    float* rowstrip;   // [nTJ * kTile]  D of the last row computed so far in every column
    float* colstrip;   // [nTI * kTile]  D of the last column computed so far in every row
    float* corner;     // [nTI + nTJ]    slot I - J + nTJ - 1: D of the last tile's corner cell on that diagonal of tiles
    int32_t* rpath;    // [T + U - 1][2] the path as the walker meets it, from the back
    uint4* codes;      // [nTI][WT][kTile] 2-bit codes, lane (row) major: bits 2 c .. 2 c + 1 of the lane's 128 are column c
};

__global__ __launch_bounds__(256) void dtw_fill_kernel(float* __restrict__ p, int64_t n, float* __restrict__ cost) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = INFINITY;
    if (i == 0) *cost = INFINITY;
}

__global__ __launch_bounds__(kTile) void dtw_tile_kernel(DtwGeom g, DtwBufs b, const float* __restrict__ a_d,
                                                         const float* __restrict__ s_d, int diag, int i_first,
                                                         float* __restrict__ cost_d) {
    __shared__ float s_feat[kTile * kChroma];
    __shared__ float s_top[kTile];
    __shared__ float s_bot[kTile];
    const int lane = threadIdx.x;
    const int I = i_first + blockIdx.x, J = diag - I;
    const int64_t t0 = (int64_t)I * kTile, u0 = (int64_t)J * kTile;
    const int64_t t = t0 + lane;

    // the tile's score rows (zeros past the end), the strip above it, the lane's audio row
    for (int i = lane; i < kTile * kChroma; i += kTile) {
        const int64_t e = u0 * kChroma + i;
        s_feat[i] = e < g.U * kChroma ? s_d[e] : 0.f;
    }
    s_top[lane] = b.rowstrip[u0 + lane];
    float a[kChroma];
#pragma unroll
    for (int k = 0; k < kChroma; ++k) a[k] = t < g.T ? a_d[t * kChroma + k] : 0.f;
    const float left_in = b.colstrip[t0 + lane];
    const int cslot = I - J + g.nTJ - 1;
    const float corner_in = b.corner[cslot];
    __syncthreads();

    float left = left_in;
    const float left_up = __shfl_up(left_in, 1);
    float dg = lane == 0 ? corner_in : left_up;
    float cur = INFINITY, last_col = INFINITY;
    unsigned long long code_lo = 0, code_hi = 0;
    const int tm1 = (int)(g.T - 1);
    const int64_t band_base = u0 * (g.T - 1) - t * (g.U - 1);     // u (T-1) - t (U-1) at the tile's first column

    for (int s = 0; s < 2 * kTile - 1; ++s) {
        float up = __shfl_up(cur, 1);                 // what lane - 1 computed last step: D[t-1][same column]
        const int c = s - lane;
        if (c >= 0 && c < kTile) {
            if (lane == 0) up = s_top[c];
            const int64_t u = u0 + c;
            const float* sf = s_feat + c * kChroma;
            float dot = 0.f;
#pragma unroll
            for (int k = 0; k < kChroma; ++k) dot = fmaf(a[k], sf[k], dot);
            const float cost = 1.0f - dot;
            bool in = t < g.T && u < g.U;
            if (g.band >= 0) {
                int64_t v = band_base + (int64_t)(c * tm1);
                v = v < 0 ? -v : v;
                in = in && v <= g.lim;
            }
            float best = dg;
            unsigned code = 0;
            if (up < best) {
                best = up;
                code = 1;
            }
            if (left < best) {
                best = left;
                code = 2;
            }
            if (t == 0 && u == 0) {
                best = 0.f;
                code = 0;
            }
            const float d = in ? cost + best : INFINITY;
            if (c < 32) code_lo |= (unsigned long long)code << (2 * c);
            else code_hi |= (unsigned long long)code << (2 * (c - 32));
            dg = up;
            left = d;
            cur = d;
            if (c == kTile - 1) last_col = d;
            if (lane == kTile - 1) s_bot[c] = d;
            if (t == g.T - 1 && u == g.U - 1) *cost_d = d;
        }
    }
    __syncthreads();
    // hand on: the corner the right-hand and lower neighbours' diagonal successor needs, the last row, the last column
    b.rowstrip[u0 + lane] = s_bot[lane];
    b.colstrip[t0 + lane] = last_col;
    if (lane == kTile - 1) b.corner[cslot] = last_col;
    int jlo, jhi;
    dtw_row_tiles(g, I, &jlo, &jhi);
    if (J >= jlo && J <= jhi && J - jlo < g.WT)
        b.codes[((int64_t)I * g.WT + (J - jlo)) * kTile + lane] =
            make_uint4((unsigned)code_lo, (unsigned)(code_lo >> 32), (unsigned)code_hi, (unsigned)(code_hi >> 32));
}

// One walker (every lane of the wave walks the same way; lane 0 writes).  At most T + U - 1 steps whatever the codes hold.
__global__ __launch_bounds__(kTile) void dtw_backtrack_kernel(DtwGeom g, DtwBufs b, const float* __restrict__ cost_d,
                                                              int32_t* __restrict__ path_d, int64_t* __restrict__ n_path_d) {
    __shared__ unsigned s_code[kTile * 4];
    const int lane = threadIdx.x;
    const int64_t max_n = g.T + g.U - 1;
    int64_t t = g.T - 1, u = g.U - 1, n = 0;
    bool done = false;
    int cur_i = -1, cur_j = -1;
    if (*cost_d < INFINITY) {
        for (int64_t i = 0; i < max_n; ++i) {
            const int I = (int)(t / kTile), J = (int)(u / kTile);
            if (I != cur_i || J != cur_j) {
                int jlo, jhi;
                dtw_row_tiles(g, I, &jlo, &jhi);
                if (J < jlo || J > jhi || J - jlo >= g.WT) break;
                __syncthreads();
                const uint4 w = b.codes[((int64_t)I * g.WT + (J - jlo)) * kTile + lane];
                s_code[lane * 4 + 0] = w.x;
                s_code[lane * 4 + 1] = w.y;
                s_code[lane * 4 + 2] = w.z;
                s_code[lane * 4 + 3] = w.w;
                __syncthreads();
                cur_i = I;
                cur_j = J;
            }
            if (lane == 0) {
                b.rpath[(max_n - 1 - i) * 2] = (int32_t)t;
                b.rpath[(max_n - 1 - i) * 2 + 1] = (int32_t)u;
            }
            n = i + 1;
            if (t == 0 && u == 0) {
                done = true;
                break;
            }
            const int r = (int)(t % kTile), c = (int)(u % kTile);
            const unsigned code = (s_code[r * 4 + (c >> 4)] >> (2 * (c & 15))) & 3u;
            if (code == 0) {
                --t;
                --u;
            } else if (code == 1) {
                --t;
            } else if (code == 2) {
                --u;
            } else {
                break;
            }
            if (t < 0 || u < 0) break;
        }
    }
    if (!done) n = 0;
    __threadfence_block();
    __syncthreads();
    for (int64_t j = lane; j < n; j += kTile) {
        path_d[j * 2] = b.rpath[(max_n - n + j) * 2];
        path_d[j * 2 + 1] = b.rpath[(max_n - n + j) * 2 + 1];
    }
    if (lane == 0) *n_path_d = n;
}

struct DtwPlan {
    DtwGeom g;
    size_t off_col, off_corner, off_rpath, off_codes, bytes;
    int64_t n_strip;   // floats of the three strips together (they are filled with +inf by one launch)
};

// DCS_OK, or the status and message of the refusal
int dtw_plan(const char* who, int64_t T, int64_t U, int64_t band, DtwPlan* p) {
    if (T < 1 || U < 1 || band < -1) DCS_FAIL(DCS_EINVAL, "%s: bad shape (T %lld, U %lld, band %lld)", who, (long long)T, (long long)U, (long long)band);
    if (T > kMaxLen || U > kMaxLen)
        DCS_FAIL(DCS_ESHAPE, "%s: T %lld, U %lld: at most %lld frames either way", who, (long long)T, (long long)U, (long long)kMaxLen);
    if (band >= 0) {
        const int64_t den = T - 1 > 1 ? T - 1 : 1, slope = (U - 1 + den - 1) / den;
        if (2 * band + 1 < slope)
            DCS_FAIL(DCS_EINVAL, "%s: band %lld cannot hold a path: the score has %lld frames per audio frame", who, (long long)band,
                     (long long)slope);
    }
    DtwGeom& g = p->g;
    g.T = T;
    g.U = U;
    g.band = (band < 0 || T == 1) ? -1 : (band > kMaxLen ? kMaxLen : band);
    g.lim = g.band < 0 ? 0 : g.band * (T - 1);
    g.nTI = (int)((T + kTile - 1) / kTile);
    g.nTJ = (int)((U + kTile - 1) / kTile);
    g.WT = 1;
    for (int I = 0; I < g.nTI; ++I) {
        int jlo, jhi;
        dtw_row_tiles(g, I, &jlo, &jhi);
        if (jhi - jlo + 1 > g.WT) g.WT = jhi - jlo + 1;
    }
    const int64_t b_row = (int64_t)g.nTJ * kTile * 4, b_col = (int64_t)g.nTI * kTile * 4;
    const int64_t b_corner = dcs_round_up((int64_t)(g.nTI + g.nTJ) * 4, 256);
    const int64_t b_rpath = dcs_round_up((T + U - 1) * 8, 256);
    const int64_t b_codes = (int64_t)g.nTI * g.WT * kTile * 16;
    p->off_col = (size_t)b_row;
    p->off_corner = (size_t)(b_row + b_col);
    p->off_rpath = (size_t)(b_row + b_col + b_corner);
    p->off_codes = (size_t)(b_row + b_col + b_corner + b_rpath);
    p->n_strip = (b_row + b_col + b_corner) / 4;
    const int64_t total = b_row + b_col + b_corner + b_rpath + b_codes;
    if (total > kMaxBytes)
        DCS_FAIL(DCS_ESHAPE, "%s: %lld bytes of scratch for T %lld, U %lld, band %lld: at most %lld", who, (long long)total, (long long)T,
                 (long long)U, (long long)band, (long long)kMaxBytes);
    p->bytes = (size_t)total;
    return DCS_OK;
}

}  // namespace

extern "C" int dcs_chroma(dcs_ctx* ctx, const float* mag_d, int64_t ld, int64_t n_frames, int F, const int8_t* cls_h, float floor,
                          float* chroma_d) {
    if (!ctx || !mag_d || !cls_h || !chroma_d) DCS_FAIL(DCS_EINVAL, "dcs_chroma: null argument");
    if (F < 1 || ld < F || n_frames < 0 || n_frames > (int64_t)INT_MAX * kChromaWaves || !(floor >= 0.f))
        DCS_FAIL(DCS_EINVAL, "dcs_chroma: bad shape (F %d, ld %lld, n_frames %lld) or floor %g", F, (long long)ld, (long long)n_frames,
                 (double)floor);
    for (int f = 0; f < F; ++f)
        if (cls_h[f] < -1 || cls_h[f] >= kChroma) DCS_FAIL(DCS_EINVAL, "dcs_chroma: class %d of bin %d (-1 .. 11)", (int)cls_h[f], f);
    if (n_frames == 0) return DCS_OK;
    DCS_ON_DEVICE(ctx->device);
    // the table travels through the context's upload ring: no synchronisation here
    void *host = nullptr, *dev = nullptr;
    DCS_CHECK(ctx->score_ring.begin((size_t)F, &host, &dev));
    memcpy(host, cls_h, (size_t)F);
    DCS_CHECK(ctx->score_ring.commit((size_t)F, ctx->stream));
    return dcs_launch_chroma(ctx->stream, mag_d, ld, n_frames, F, (const int8_t*)dev, floor, chroma_d);
}

int dcs_launch_chroma(hipStream_t stream, const float* mag_d, int64_t ld, int64_t n_frames, int F, const int8_t* cls_d, float floor,
                      float* chroma_d) {
    hipLaunchKernelGGL(chroma_kernel, dim3((unsigned)((n_frames + kChromaWaves - 1) / kChromaWaves)), dim3(kChromaWaves * 64), 0,
                       stream, mag_d, ld, n_frames, F, (const signed char*)cls_d, floor, chroma_d);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

extern "C" int dcs_dtw_tile(void) { return kTile; }

extern "C" int64_t dcs_dtw_bytes(int64_t T, int64_t U, int64_t band) {
    DtwPlan p;
    return dtw_plan("dcs_dtw_bytes", T, U, band, &p) == DCS_OK ? (int64_t)p.bytes : -1;
}

extern "C" int dcs_dtw(dcs_ctx* ctx, const float* a_d, int64_t T, const float* s_d, int64_t U, int64_t band, int32_t* path_d,
                       int64_t* n_path_d, float* cost_d) {
    if (!ctx || !a_d || !s_d || !path_d || !n_path_d || !cost_d) DCS_FAIL(DCS_EINVAL, "dcs_dtw: null argument");
    DtwPlan p;
    DCS_CHECK(dtw_plan("dcs_dtw", T, U, band, &p));
    const DtwGeom& g = p.g;
    // the rows of tiles every anti-diagonal of tiles touches inside the band
    const int n_diag = g.nTI + g.nTJ - 1;
    std::vector<int> i_lo(n_diag, INT_MAX), i_hi(n_diag, -1);
    for (int I = 0; I < g.nTI; ++I) {
        int jlo, jhi;
        dtw_row_tiles(g, I, &jlo, &jhi);
        for (int J = jlo; J <= jhi; ++J) {
            if (I < i_lo[I + J]) i_lo[I + J] = I;
            if (I > i_hi[I + J]) i_hi[I + J] = I;
        }
    }
    DCS_ON_DEVICE(ctx->device);
    DCS_CHECK(ctx->align_ws.ensure(p.bytes));
    char* base = (char*)ctx->align_ws.ptr;
    DtwBufs b;
    b.rowstrip = (float*)base;
    b.colstrip = (float*)(base + p.off_col);
    b.corner = (float*)(base + p.off_corner);
    b.rpath = (int32_t*)(base + p.off_rpath);
    b.codes = (uint4*)(base + p.off_codes);
    hipLaunchKernelGGL(dtw_fill_kernel, dim3((unsigned)((p.n_strip + 255) / 256)), dim3(256), 0, ctx->stream, b.rowstrip, p.n_strip,
                       cost_d);
    for (int d = 0; d < n_diag; ++d) {
        if (i_hi[d] < i_lo[d]) continue;
        hipLaunchKernelGGL(dtw_tile_kernel, dim3((unsigned)(i_hi[d] - i_lo[d] + 1)), dim3(kTile), 0, ctx->stream, g, b, a_d, s_d, d,
                           i_lo[d], cost_d);
    }
    hipLaunchKernelGGL(dtw_backtrack_kernel, dim3(1), dim3(kTile), 0, ctx->stream, g, b, (const float*)cost_d, path_d, n_path_d);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

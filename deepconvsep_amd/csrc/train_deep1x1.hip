// Training of the deep score-informed graph build_ca_1x1 (examples/bach10_scoreinformed/trainCNNrwc.py:66-132, chosen with
// --function build_ca_1x1; loss :246-283, adadelta :279) on gfx950.  The separator of this graph is deep1x1.hip; the step
// runs the same implicit-GEMM kernel (deep1x1_igemm.h) for every product whose M is the pixels, and the split-K GEMM of the
// training core (train_core.h) for the weight gradients, whose K is the pixels.
//
//   a_l = rectify(conv_l(a_{l-1}) + b_l) + bb_l, l = 1 .. 6 (a_0 = x), s = rectify(W_7 a_6 + b_7) + bb_7, g_6 = s[:, 0:200],
//   g_{l-1} = conv_l^T(g_l c_l), q = g_0 + fb[0:4], c_l = r'(pre_l) in {0, 0.5, 1}, one byte per unit (0, 1, 2)
//
// Only branch 0 (rows 0 .. 199 of the 1x1 layer, final-bias entries 0 .. 3) reaches the loss, so the stepped state holds those
// rows alone; the other rows are held once in `dead` (SiTrainer's rule: returned as given, zeros for the other sections).
//
// One step on the ctx stream, no host synchronisation, no float atomics:
//
//   pack      the weights of the state into the operand layouts of d1_igemm_kernel (B, Bt[parity]); pads stay zero
//   forward   x -> channels-last; MODE_FWD x 7 (a_l and c_l kept, the 1x1 layer is a 1 x 1 convolution of 200 filters);
//             MODE_TR down to g_1, MODE_Q writes q [B][4][tc][F]; after g_l has been read, g_l *= c_l in place
//   loss      train::mask_loss_kernel<4>, train::loss_reduce_kernel
//   backward  dq -> channels-last; dg_l = c_l conv_l(dg_{l-1}) MODE_FWDC; da_6 = W_7^T (ds c_7) MODE_B11;
//             da_{l-1} = conv_l^T(da_l c_l) MODE_TR; code_apply_kernel: column sums of ds and da_l (dbb), then *= c in place
//   weights   dW_l | db_l = [windows of a_{l-1}; windows of dg_{l-1}]^T . [da_l c_l; g_l c_l], ones row over the first half:
//             train::gemm_kernel, split-K over K = 2 B Ho Wo, fixed-order reduce; dW_7 | db_7 = [a_6^T; 1] . (ds c_7)
//   update    train::adadelta_kernel
//
// Buffers (views into the work buffer): X_l = [a_l; dg_l] and D_l = [da_l c_l; g_l c_l], two slots each of [B][Ho][Wo][Coutp]
// channels-last (Coutp = Cout rounded up to 4, pad channels 0), so that one Ax walks both halves of a weight gradient's K.
// Internal parameter layout: W_l [kh i][5 j][Cin][Cout] = W[co][ci][kh-1-i][4-j] (b_l follows it: the ones row), W_7 [ci][co].
#include <memory>

#include "deep1x1_debug.h"
#include "train_ca.h"

using namespace train;

namespace {

constexpr int kL = d1::kLayers, kNf = d1::kNf, kKw = d1::kKw;
constexpr int kCh = 4, kBranches = 4;
constexpr int kNparams = 3 * (kL + 1) + 1;
constexpr int kSumBlocks = 512;

struct D1Sums {
    static constexpr int kOut = 4, kDbo = 4;
    static __device__ double E(const double* s) { return s[0] + s[1] + s[2] + s[3]; }
};

struct PackArgs {
    const float* W;             // internal [kh][kw][Cin][Cout]
    float *Bf, *Bt0, *Bt1;
    int kw, Cin, Cinp, Cout, Coutp, Kpad, Ktpad0, Ktpad1;
    int64_t n;
};

// Bf[co][(i kw + j) Cinp + ci] = Bt[j & 1][ci][(i ntap + j / 2) Coutp + co] = W[i][j][ci][co]; ntap = taps of that parity
__global__ __launch_bounds__(kThreads) void pack_kernel(const PackArgs a) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= a.n) return;
    const int co = (int)(e % a.Cout);
    int64_t r = e / a.Cout;
    const int ci = (int)(r % a.Cin);
    r /= a.Cin;
    const int j = (int)(r % a.kw), i = (int)(r / a.kw);
    const float w = a.W[e];
    a.Bf[(int64_t)co * a.Kpad + (i * a.kw + j) * a.Cinp + ci] = w;
    const int p = j & 1, jt = j >> 1, nt = (a.kw - p + 1) / 2;
    float* bt = p ? a.Bt1 : a.Bt0;
    bt[(int64_t)ci * (p ? a.Ktpad1 : a.Ktpad0) + (i * nt + jt) * a.Coutp + co] = w;
}

// buf [rows][Cp] *= 0.5 code, in place; part != nullptr: the column sums of buf as it was, one row of C sums per workgroup
// (rows r0 .. r0 + per of workgroup blockIdx.x; a thread adds its rows in order, the workgroup its threads in order)
__global__ __launch_bounds__(kThreads) void code_apply_kernel(float* __restrict__ buf, const uint8_t* __restrict__ code,
                                                              int64_t rows, int Cp, int C, int64_t per, float* __restrict__ part) {
    __shared__ float red[kThreads];
    const int nsub = kThreads / Cp, sub = threadIdx.x / Cp, c = threadIdx.x - sub * Cp;
    const int64_t r0 = (int64_t)blockIdx.x * per, r1 = min(rows, r0 + per);
    float s = 0.f;
    if (sub < nsub)
        for (int64_t r = r0 + sub; r < r1; r += nsub) {
            const int64_t at = r * Cp + c;
            const float v = buf[at];
            s += v;
            buf[at] = v * (0.5f * (float)code[at]);
        }
    if (!part) return;
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < C) {
        float t = 0.f;
        for (int k = 0; k < nsub; ++k) t += red[k * Cp + threadIdx.x];
        part[(int64_t)blockIdx.x * C + threadIdx.x] = t;
    }
}

// code [B][H W][Cp] bytes -> out [B][C][H W] floats 0 / 0.5 / 1
__global__ __launch_bounds__(kThreads) void codes_out_kernel(const uint8_t* __restrict__ code, float* __restrict__ out, int64_t n,
                                                             int64_t hw, int C, int Cp) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= n) return;
    const int64_t px = e % hw, bc = e / hw;
    const int64_t c = bc % C, b = bc / C;
    out[e] = 0.5f * (float)code[(b * hw + px) * Cp + c];
}

// the .pkl index of element k of the internal section s
struct D1Map {
    int Cin[kL], Cout[kL], kh[kL];
    __device__ int64_t operator()(int s, int64_t k) const {
        if (s < 3 * kL && s % 3 == 0) {
            const int l = s / 3;
            const int64_t co = k % Cout[l], r = k / Cout[l], ci = r % Cin[l], ij = r / Cin[l], j = ij % kKw, i = ij / kKw;
            return ((co * Cin[l] + ci) * kh[l] + (kh[l] - 1 - i)) * kKw + (kKw - 1 - j);
        }
        if (s == 3 * kL) return (k % kNf) * kNf + k / kNf;
        return k;
    }
};

struct Lay {
    int Cin, Cinp, Cout, Coutp, kh, Hi, Wi, Ho, Wo;
    int K, Kpad, Kt[2], Ktpad[2], Kw;      // the operands of d1_igemm_kernel; Kw = kh 5 Cin rows of the internal W
    int64_t px, slot;                      // B Ho Wo, px Coutp
    float *Bf = nullptr, *Bt[2] = {nullptr, nullptr}, *X = nullptr, *D = nullptr, *codef = nullptr, *part = nullptr,
          *bpart = nullptr;
    int splits = 1, kchunk = 0, nsum = 1;
    int64_t per = 0;
    uint8_t* code() const { return (uint8_t*)codef; }
};

int npad_of(int N) { return d1::npad_for(N); }

struct Deep1x1Trainer : dcs_trainer {
    Lay L[kL + 1];                // L[kL]: the 1x1 layer as a 1 x 1 convolution of its 200 live filters
    int nb = kBranches;           // branches the caller's arrays hold
    int64_t ndead = 0;
    float *dead = nullptr, *xy = nullptr, *X0 = nullptr;

    void shape(int time_context, int F_, int batch, int branches) {
        tc = time_context; F = F_; B = batch; nb = branches;
        int H = tc, W = F, cin = kCh;
        for (int k = 0; k <= kL; ++k) {
            Lay& l = L[k];
            const bool last = k == kL;
            const int kw = last ? 1 : kKw;
            l.Cin = cin; l.Cinp = (int)dcs_round_up(cin, 4);
            l.Cout = last ? kNf : d1::kFilters[k]; l.Coutp = (int)dcs_round_up(l.Cout, 4);
            l.kh = last ? 1 : d1::kKh[k];
            l.Hi = H; l.Wi = W; l.Ho = H - l.kh + 1; l.Wo = last ? W : (W - kKw) / 2 + 1;
            l.Kw = l.kh * kw * l.Cin;
            l.K = l.kh * kw * l.Cinp; l.Kpad = (int)dcs_round_up(l.K, 16);
            for (int p = 0; p < 2; ++p) {
                l.Kt[p] = l.kh * ((kw - p + 1) / 2) * l.Coutp;
                l.Ktpad[p] = (int)dcs_round_up(std::max(l.Kt[p], 1), 16);
            }
            l.px = (int64_t)B * l.Ho * l.Wo; l.slot = l.px * l.Coutp;
            const int64_t w[4] = {last ? (int64_t)kNf * nb : l.Cout, l.Cin, l.kh, kw}, b[4] = {w[0], 1, 1, 1};
            memcpy(shapes[3 * k], w, sizeof(w));
            memcpy(shapes[3 * k + 1], b, sizeof(b));
            memcpy(shapes[3 * k + 2], b, sizeof(b));
            state_size[3 * k] = (int64_t)l.Kw * l.Cout;
            state_size[3 * k + 1] = state_size[3 * k + 2] = l.Cout;
            H = l.Ho; W = l.Wo; cin = l.Cout;
        }
        const int64_t fb[4] = {(int64_t)kCh * nb, 1, 1, 1};
        memcpy(shapes[kNparams - 1], fb, sizeof(fb));
        state_size[kNparams - 1] = kCh;
        nparams = nstate = kNparams;
        nsrc = kCh;
        loss_sums = D1Sums::kOut + D1Sums::kDbo;
        ndead = (int64_t)(nb - 1) * (kNf * kNf + 2 * kNf + kCh);
    }

    void plan(std::vector<std::pair<float**, int64_t>>& parts) override {
        parts.insert(parts.end(), {{&xy, 2 * kCh * RF}, {&X0, 2 * kCh * RF}, {&Q, kCh * RF}});
        for (int k = 0; k <= kL; ++k) {
            Lay& l = L[k];
            // about four workgroups per CU; a slice is at least 256 pixels, so the partials stay below the tiles' 1024 x 64 x 64
            const bool wide = l.Cout > 32;
            const int64_t tiles = (int64_t)dcs_cdiv(l.Kw + 1, wide ? 64 : 128) * dcs_cdiv(l.Cout, wide ? 64 : 32);
            pick_split(tiles, (k < kL ? 2 : 1) * l.px, &l.splits, &l.kchunk, 1024, 512);
            l.nsum = (int)std::min<int64_t>(kSumBlocks, dcs_cdiv(l.px, 64));
            l.per = dcs_cdiv(l.px, l.nsum);
            parts.insert(parts.end(), {{&l.X, k < kL ? 2 * l.slot : 0}, {&l.D, k < kL ? 2 * l.slot : 0}, {&l.codef, dcs_cdiv(l.slot, 4)},
                                       {&l.Bf, (int64_t)npad_of(l.Cout) * l.Kpad},
                                       {&l.Bt[0], (int64_t)npad_of(l.Cin) * l.Ktpad[0]},
                                       {&l.Bt[1], (int64_t)npad_of(l.Cin) * l.Ktpad[1]},
                                       {&l.part, (int64_t)l.splits * (l.Kw + 1) * l.Cout}, {&l.bpart, (int64_t)l.nsum * l.Cout}});
        }
        if (ndead > 0) parts.push_back({&dead, ndead});
    }

    d1::D1Args fwd_args(int k, const float* in, float* out) {
        const Lay& l = L[k];
        d1::D1Args a = d1::forward_args(B, l.Hi, l.Wi, l.Cinp, l.kh, k == kL ? 1 : kKw, k == kL ? 1 : 2, l.Cout);
        a.in = in; a.B = l.Bf;
        a.out = out; a.Co = l.Coutp;
        return a;
    }

    // conv_k^T of `in` times c_k, one launch per output-column parity: MODE_TR into out, or (k == 0, q) MODE_Q
    void transposed(int k, const float* in, float* out, bool q) {
        const Lay& l = L[k];
        for (int par = 0; par < 2; ++par) {
            d1::D1Args a = d1::transposed_args(B, l.Ho, l.Wo, l.Coutp, l.Hi, l.Wi, l.kh, kKw, par, l.Cin);
            a.in = in; a.code = l.code(); a.B = l.Bt[par];
            if (a.M == 0) continue;
            a.out = out; a.Co = l.Cinp;
            if (q) {
                a.b0 = param(kNparams - 1);
                d1::launch<d1::MODE_Q>(ctx, a);
            } else {
                d1::launch<d1::MODE_TR>(ctx, a);
            }
        }
    }

    void apply_code(const Lay& l, float* buf, bool sums) {
        hipLaunchKernelGGL(code_apply_kernel, dim3((unsigned)l.nsum), dim3(kThreads), 0, ctx->stream, buf,
                           (const uint8_t*)l.code(), l.px, l.Coutp, l.Cout, l.per, sums ? l.bpart : nullptr);
    }

    void to_cl(const float* x, float* y) {
        const int64_t plane = (int64_t)tc * F;
        hipLaunchKernelGGL(d1::d1_to_cl_kernel, dim3((unsigned)dcs_cdiv(RF, kThreads)), dim3(kThreads), 0, ctx->stream, x, y, RF,
                           plane);
    }

    int forward(const float* x) override {
        for (int k = 0; k <= kL; ++k) {
            const Lay& l = L[k];
            PackArgs a{param(3 * k), l.Bf, l.Bt[0], l.Bt[1], k == kL ? 1 : kKw, l.Cin, l.Cinp, l.Cout, l.Coutp, l.Kpad,
                       l.Ktpad[0], l.Ktpad[1], state_size[3 * k]};
            hipLaunchKernelGGL(pack_kernel, dim3((unsigned)dcs_cdiv(a.n, kThreads)), dim3(kThreads), 0, ctx->stream, a);
        }
        to_cl(x, X0);
        const float* cur = X0;
        for (int k = 0; k <= kL; ++k) {
            Lay& l = L[k];
            // the 1x1 layer's output is g_6: the second slot of D_6
            d1::D1Args a = fwd_args(k, cur, k == kL ? L[kL - 1].D + L[kL - 1].slot : l.X);
            a.b0 = param(3 * k + 1); a.b1 = param(3 * k + 2); a.code_out = l.code();
            d1::launch<d1::MODE_FWD>(ctx, a);
            cur = l.X;
        }
        for (int k = kL - 1; k >= 0; --k) {
            float* g = L[k].D + L[k].slot;
            transposed(k, g, k > 0 ? L[k - 1].D + L[k - 1].slot : Q, k == 0);
            apply_code(L[k], g, false);
        }
        DCS_HIP(hipGetLastError());
        return DCS_OK;
    }

    int loss(const float* x, const float* tgt, double* out7_d) override {
        MaskLoss a;
        a.q = Q; a.x = x; a.tgt = tgt; a.rnd = rnd; a.xy = xy; a.part = lpart;
        a.plane = (int64_t)tc * F;
        a.n = RF;
        a.eps = hyp[0];
        const int nblk = (int)std::min<int64_t>(kLossBlocks, dcs_cdiv(a.n, kThreads));
        hipLaunchKernelGGL(mask_loss_kernel<kCh>, dim3(nblk), dim3(kThreads), 0, ctx->stream, a);
        DCS_HIP(hipGetLastError());
        return loss_reduce<D1Sums>(nblk, out7_d, grad() + off[kNparams - 1]);
    }

    int backward() override {
        // the decoder: dg_0 = dq, dg_l = c_l conv_l(dg_{l-1}) into the second slot of X_l
        to_cl(xy + kCh * RF, X0 + kCh * RF);
        const float* cur = X0 + kCh * RF;
        for (int k = 0; k < kL; ++k) {
            Lay& l = L[k];
            d1::D1Args a = fwd_args(k, cur, l.X + l.slot);
            a.code = l.code();
            d1::launch<d1::MODE_FWDC>(ctx, a);
            cur = l.X + l.slot;
        }
        // the 1x1 layer: da_6 = W_7^T (ds c_7), then dbb_7 = sum ds and ds *= c_7 in place
        Lay& l6 = L[kL - 1];
        Lay& l7 = L[kL];
        float* ds = l6.X + l6.slot;
        {
            d1::D1Args a = d1::transposed_args(B, l7.Ho, l7.Wo, l7.Coutp, l7.Hi, l7.Wi, 1, 1, 0, l7.Cin);
            a.in = ds; a.code = l7.code(); a.B = l7.Bt[0];
            a.out = l6.D; a.Co = l7.Cinp;
            d1::launch<d1::MODE_B11>(ctx, a);
        }
        apply_code(l7, ds, true);
        // the encoder: da_{l-1} = conv_l^T(da_l c_l), dbb_l = sum da_l, da_l *= c_l in place
        for (int k = kL - 1; k >= 0; --k) {
            if (k > 0) transposed(k, L[k].D, L[k - 1].D, false);
            apply_code(L[k], L[k].D, true);
        }
        DCS_HIP(hipGetLastError());
        // dW_l | db_l: rows the (i, j, ci) of a window (+ the ones row over the encoder half), K the 2 B Ho Wo pixels
        for (int k = 0; k <= kL; ++k) {
            Lay& l = L[k];
            const bool last = k == kL;
            float* win = k == 0 ? X0 : L[k - 1].X;
            Gemm g = gemm0(l.Kw + 1, l.Cout, (int)((last ? 1 : 2) * l.px));
            const int64_t rowp = (int64_t)l.Wi * l.Cinp;
            if (last) g.A = mat(win, 0, ax1(1), ax1(l.Cinp));
            else g.A = mat(win, 0, ax3(l.Cin, kKw, 1, l.Cinp, rowp), ax3(l.Wo, l.Ho, 2 * l.Cinp, rowp, l.Hi * rowp));
            g.B = mat(last ? ds : l.D, 0, ax1(l.Coutp), ax1(1));
            g.ones_row = l.Kw; g.ones_klim = (int)l.px;
            g.partial = l.part; g.splits = l.splits; g.kchunk = l.kchunk;
            DCS_CHECK(launch(g, l.Cout > 32 ? T64x64 : T128x32, false, false));
        }
        for (int k = 0; k <= kL; ++k) {
            Lay& l = L[k];
            Reduce r;
            memset(&r, 0, sizeof(r));
            r.scale = sign;
            r.part[0] = l.part; r.dst[0] = grad() + off[3 * k]; r.count[0] = (int64_t)(l.Kw + 1) * l.Cout; r.splits[0] = l.splits;
            r.part[1] = l.bpart; r.dst[1] = grad() + off[3 * k + 2]; r.count[1] = l.Cout; r.splits[1] = l.nsum;
            r.N[0] = r.N[1] = l.Cout;
            DCS_CHECK(reduce(r));
        }
        return DCS_OK;
    }

    // pkl: the caller's 22 arrays.  The live rows of the last four are a prefix of each array and go through the layout kernel
    // with the rest; the others are copied into `dead` at create and served from there.
    int layout(float* flat_d, float* const* pkl, int to_internal) override {
        D1Map map;
        for (int k = 0; k < kL; ++k) { map.Cin[k] = L[k].Cin; map.Cout[k] = L[k].Cout; map.kh[k] = L[k].kh; }
        DCS_CHECK(run_layout(flat_d, pkl, to_internal, map));
        if (ndead == 0) return DCS_OK;
        const int which = (int)((flat_d - state) / (4 * P4));
        // dcs_trainer_set on an optimiser slot: `dead` holds parameters, not accumulators, and stays as it is
        if (to_internal && which != 0) return DCS_OK;
        int64_t at = 0;
        for (int i = 3 * kL; i < kNparams; ++i) {
            float* p = pkl[i] + state_size[i];
            const int64_t n = state_size[i] * (nb - 1);
            hipError_t e;
            if (to_internal) e = hipMemcpyAsync(dead + at, p, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream);
            else if (which == 0) e = hipMemcpyAsync(p, dead + at, n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream);
            else e = hipMemsetAsync(p, 0, n * sizeof(float), ctx->stream);
            DCS_HIP(e);
            at += n;
        }
        return DCS_OK;
    }

    int codes(float* const* out_d, int n) override {
        if (n != kL + 1) DCS_FAIL(DCS_ESHAPE, "dcs_trainer_rectify_codes: %d buffers for %d rectified layers", n, kL + 1);
        for (int k = 0; k <= kL; ++k) {
            const Lay& l = L[k];
            const int64_t cnt = l.px * l.Cout;
            hipLaunchKernelGGL(codes_out_kernel, dim3((unsigned)dcs_cdiv(cnt, kThreads)), dim3(kThreads), 0, ctx->stream,
                               (const uint8_t*)l.code(), out_d[k], cnt, (int64_t)l.Ho * l.Wo, l.Cout, l.Coutp);
        }
        DCS_HIP(hipGetLastError());
        return DCS_OK;
    }
};

}  // namespace

// shapes / nparams: the caller's, read only to tell how many branches of the 1x1 layer it holds (4, or 1 .. 3: live-only)
int deep1x1_trainer_new(int time_context, int F, int batch, const int64_t* shapes, int nparams, dcs_trainer** out) {
    // every GEMM index stays below 2^30 (train::kBig): the largest is the K of dW_1, the 2 B tc w1 pixels of conv1's two halves
    const int64_t w1 = F >= kKw ? (F - kKw) / 2 + 1 : 0;
    if (time_context < 19 || time_context > 1024 || F < 253 || F > 2049 || batch < 1 || batch > 1024 ||
        2 * (int64_t)batch * time_context * w1 >= kBig)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: build_ca_1x1 graph: time_context %d (19 .. 1024), F %d (253 .. 2049), batch %d "
                 "(1 .. 1024), and 2 batch time_context ((F - 5) / 2 + 1) below 2^30", time_context, F, batch);
    int nb = kBranches;
    if (shapes && nparams == kNparams) {
        const int64_t rows = shapes[4 * 3 * kL];
        if (rows % kNf == 0 && rows >= kNf && rows <= (int64_t)kBranches * kNf) nb = (int)(rows / kNf);
    }
    std::unique_ptr<Deep1x1Trainer> t(new Deep1x1Trainer());
    t->shape(time_context, F, batch, nb);
    *out = t.release();
    return DCS_OK;
}

// ------------------------------------------------------------------------------------------------ test aids (include/dcs.h)
int deep1x1_trainer_debug_conv(dcs_ctx* ctx, int mode, dcs_debug_d1_args* q) {
    d1::D1Args a;
    DCS_CHECK(d1::debug_conv_args(mode, q, &a));
    DCS_ON_DEVICE(ctx->device);
    switch (mode) {
        case d1::MODE_FWD: return d1::debug_conv_run<d1::MODE_FWD>(ctx, a);
        case d1::MODE_TR: return d1::debug_conv_run<d1::MODE_TR>(ctx, a);
        case d1::MODE_FWDC: return d1::debug_conv_run<d1::MODE_FWDC>(ctx, a);
        case d1::MODE_Q: return d1::debug_conv_run<d1::MODE_Q>(ctx, a);
        case d1::MODE_B11: return d1::debug_conv_run<d1::MODE_B11>(ctx, a);
        default: DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: the trainer launches no mode %d", mode);
    }
}

int deep1x1_trainer_debug_aux(dcs_ctx* ctx, int which, dcs_debug_d1_aux_args* q) {
    using d1::dbg_bad;
    const int64_t big = (int64_t)1 << 30;
    if (which == DCS_D1_AUX_CODE_APPLY) {
        if (q->rows < 1 || q->rows > big || q->Cp < 1 || q->Cp > kThreads || q->C < 1 || q->C > q->Cp || q->per < 1 || q->per > big ||
            q->nsum < 1 || q->nsum > 65536 || q->rows * q->Cp > big)
            DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: %lld rows of %d (%d live) channels, %d workgroups of %lld rows", (long long)q->rows,
                     q->Cp, q->C, q->nsum, (long long)q->per);
        if (dbg_bad(q->out, q->out_bytes, q->rows * q->Cp * 4) || dbg_bad(q->in2, q->in2_bytes, q->rows * q->Cp) ||
            (q->out2 && dbg_bad(q->out2, q->out2_bytes, (int64_t)q->nsum * q->C * 4)))
            DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: code_apply buffers");
        DCS_ON_DEVICE(ctx->device);
        hipLaunchKernelGGL(code_apply_kernel, dim3((unsigned)q->nsum), dim3(kThreads), 0, ctx->stream, (float*)q->out,
                           (const uint8_t*)q->in2, q->rows, q->Cp, q->C, q->per, (float*)q->out2);
    } else if (which == DCS_D1_AUX_CODES_OUT) {
        if (q->n < 1 || q->n > big || q->hw < 1 || q->hw > big || q->Cp < 1 || q->Cp > d1::kDbgMaxCh || q->C < 1 || q->C > q->Cp ||
            q->n * q->hw > big / q->Cp)
            DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: %lld images of %lld pixels, %d of %d channels", (long long)q->n, (long long)q->hw, q->C,
                     q->Cp);
        const int64_t cnt = q->n * q->C * q->hw;
        if (dbg_bad(q->in, q->in_bytes, q->n * q->hw * q->Cp) || dbg_bad(q->out, q->out_bytes, cnt * 4))
            DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: codes_out buffers");
        DCS_ON_DEVICE(ctx->device);
        hipLaunchKernelGGL(codes_out_kernel, dim3((unsigned)dcs_cdiv(cnt, kThreads)), dim3(kThreads), 0, ctx->stream,
                           (const uint8_t*)q->in, (float*)q->out, cnt, q->hw, q->C, q->Cp);
    } else if (which == DCS_D1_AUX_PACK_DEVICE) {
        if ((q->kw != 1 && q->kw != kKw) || q->kh < 1 || q->kh > d1::kDbgMaxKh || q->Cin < 1 || q->Cin > d1::kDbgMaxCh || q->Cout < 1 ||
            q->Cout > d1::kDbgMaxCh)
            DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: weights [%d][%d][%d][%d]", q->kh, q->kw, q->Cin, q->Cout);
        PackArgs a{};
        a.kw = q->kw; a.Cin = q->Cin; a.Cinp = (int)dcs_round_up(q->Cin, 4); a.Cout = q->Cout; a.Coutp = (int)dcs_round_up(q->Cout, 4);
        a.Kpad = (int)dcs_round_up(q->kh * q->kw * a.Cinp, 16);
        const int nt0 = (q->kw + 1) / 2, nt1 = q->kw / 2;
        a.Ktpad0 = (int)dcs_round_up(q->kh * nt0 * a.Coutp, 16);
        a.Ktpad1 = (int)dcs_round_up(q->kh * nt1 * a.Coutp, 16);
        a.n = (int64_t)q->kh * q->kw * q->Cin * q->Cout;
        if (dbg_bad(q->in, q->in_bytes, a.n * 4) || dbg_bad(q->out, q->out_bytes, (int64_t)npad_of(q->Cout) * a.Kpad * 4) ||
            dbg_bad(q->out2, q->out2_bytes, (int64_t)npad_of(q->Cin) * a.Ktpad0 * 4) ||
            (nt1 > 0 && dbg_bad(q->out3, q->out3_bytes, (int64_t)npad_of(q->Cin) * a.Ktpad1 * 4)))
            DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: pack buffers");
        a.W = (const float*)q->in; a.Bf = (float*)q->out; a.Bt0 = (float*)q->out2; a.Bt1 = (float*)q->out3;
        DCS_ON_DEVICE(ctx->device);
        hipLaunchKernelGGL(pack_kernel, dim3((unsigned)dcs_cdiv(a.n, kThreads)), dim3(kThreads), 0, ctx->stream, a);
    } else {
        DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: which = %d", which);
    }
    DCS_HIP(hipGetLastError());
    DCS_HIP(hipStreamSynchronize(ctx->stream));
    return DCS_OK;
}

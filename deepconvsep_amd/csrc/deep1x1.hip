// build_ca_1x1, the deep score-informed graph of examples/bach10_scoreinformed/trainCNNrwc.py:66-132, on the f32 matrix pipe.
//
//   conv1 .. conv6   Conv2DLayer(k x 5, stride (1, 2), rectify) + BiasLayer        d1_igemm_kernel<MODE_FWD>
//   conv (1 x 1)     800 filters, rectify + BiasLayer, sliced into 4 x 200       d1_igemm_kernel<MODE_1X1>
//   per branch       InverseLayer of conv6 .. conv2                               d1_igemm_kernel<MODE_TR>
//                    InverseLayer of conv1 + final BiasLayer + rectify            d1_igemm_kernel<MODE_LAST>
//   soft masks       separate_bach10.py / trainCNNrwc.py mask expressions         d1_mask_kernel
//
// Every convolution is an implicit GEMM over channels-last activations: M = output pixels, N = output channels,
// K = (filter row, filter tap, input channel) with the channel fastest, so one tap row of a pixel is kw * Cin contiguous
// floats.  Channel counts are padded to a multiple of 4 (the pad channels hold 0) so that a lane reads 4 consecutive K
// values as one 16-byte load.  A wave owns 32 pixels x 16 NT channels: each lane loads a 4-K quad of A and of B and feeds
// element e of both to the e-th of four v_mfma_f32_16x16x4_f32 -- the K order inside the sum differs from a plain k loop,
// the arithmetic is still a chain of exact f32 fma (f32-class results).  Operands come straight from global memory (L1 /
// L2 carry the reuse), so the kernel has no LDS and no barrier.
//
// InverseLayer(conv_k) is theano.grad through conv_k's rectify: g_{k-1} = conv_k^T(g_k * r'(pre_k)) with Theano's
// relu = 0.5 (x + |x|), r'(0) = 0.5.  The forward epilogue records r'(pre_k) as one byte per element (0, 1, 2 = 0, 0.5, 1);
// the transposed kernel multiplies g by it while loading.  The transposed conv runs once per output-column parity: the
// stride-2 taps that reach an even column are j = 0, 2, 4 and an odd one j = 1, 3, so each parity is a dense conv with 3 or 2
// taps.  A column no tap reaches (conv3's last input column at 2049 bins) has no valid operand and is written 0.
//
// Only branch 0 reaches predict_function2's masks (trainCNNrwc.py:243-263), so the masked modes run that branch alone.
#include <string.h>

#include "deep1x1.h"

#include "deep1x1_debug.h"

using namespace d1;

namespace {

// The soft masks of mask_kernel (generic.hip) on p = rectify(o + bias) already formed: p [4][n][plane] of this chunk,
// x its tiles [n][C][plane]; out [4][n_total][plane] from tile k_first.  mode 0 / 1 = DCS_EPS_A / DCS_EPS_B.
__global__ __launch_bounds__(kThreads) void d1_mask_kernel(const float* __restrict__ pin, const float* __restrict__ x,
                                                           float* __restrict__ out, int64_t n, int64_t n_total, int64_t k_first,
                                                           int C, int64_t plane, int mode, int mix_n) {
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= n * plane) return;
    const int64_t k = idx / plane, r = idx - k * plane;
    const float eps_r = 5e-19f;
    float p[4];
    float den = 0.f;
    for (int s = 0; s < 4; ++s) {
        p[s] = pin[((int64_t)s * n + k) * plane + r];
        if (mode == 0) p[s] += eps_r;
        den = (s == 0) ? p[s] : den + p[s];
    }
    if (mode == 1) den += eps_r;
    float mix = x[(k * C) * plane + r];
    for (int c = 1; c < mix_n; ++c) mix += x[(k * C + c) * plane + r];
    for (int s = 0; s < 4; ++s) out[((int64_t)s * n_total + k_first + k) * plane + r] = (p[s] / den) * mix;
}

struct D1Layer {
    int Cin, Cinp, Cout, Coutp, kh;
    int Hi, Wi, Ho, Wo;
    float *B = nullptr, *b0 = nullptr, *b1 = nullptr, *Bt[2] = {nullptr, nullptr};
};


// The operands of one convolution from its Lasagne weights W [Cout][Cin][kh][kw] (flip_filters=True: a true convolution);
// kw = 5 (stride 2: the taps of an output-column parity p are j = p + 2 jt, ntap = 3 / 2 of them) or 1 (the 1x1 layer).
//   forward                B[co][(i * kw + j) * Cinp + ci] = W[co][ci][kh-1-i][kw-1-j]                    [npad(Cout)][Kpad]
//   transposed, parity p   Bt[p][ci][(i * ntap + jt) * Coutp + co] = W[co][ci][kh-1-i][kw-1-(p+2jt)]     [npad(Cin)][Ktpad[p]]
// zero past K and past the live rows (the layouts D1Args documents).  With bt == nullptr only B is made.
void pack_host(const float* Wk, int Cin, int Cout, int kh, int kw, std::vector<float>& B, std::vector<float>* bt) {
    const int Cinp = (int)dcs_round_up(Cin, 4), Coutp = (int)dcs_round_up(Cout, 4);
    auto w = [&](int co, int ci, int i, int j) { return Wk[(((size_t)co * Cin + ci) * kh + i) * kw + j]; };
    const int Kpad = (int)dcs_round_up(kh * kw * Cinp, 16);
    B.assign((size_t)npad_for(Cout) * Kpad, 0.f);
    for (int co = 0; co < Cout; ++co)
        for (int i = 0; i < kh; ++i)
            for (int j = 0; j < kw; ++j)
                for (int ci = 0; ci < Cin; ++ci)
                    B[(size_t)co * Kpad + (i * kw + j) * Cinp + ci] = w(co, ci, kh - 1 - i, kw - 1 - j);
    for (int p = 0; bt && p < 2; ++p) {
        const int nt = (kw - p + 1) / 2;
        const int Ktpad = (int)dcs_round_up(kh * nt * Coutp, 16);
        bt[p].assign((size_t)npad_for(Cin) * Ktpad, 0.f);
        for (int ci = 0; ci < Cin; ++ci)
            for (int i = 0; i < kh; ++i)
                for (int jt = 0; jt < nt; ++jt)
                    for (int co = 0; co < Cout; ++co)
                        bt[p][(size_t)ci * Ktpad + (i * nt + jt) * Coutp + co] = w(co, ci, kh - 1 - i, kw - 1 - (p + 2 * jt));
    }
}

int upload_f32(float** dst, const std::vector<float>& src, const char* name) {
    DCS_HIP(dcs_dev_alloc((void**)dst, src.size() * sizeof(float), name));
    DCS_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(float), hipMemcpyHostToDevice));
    return DCS_OK;
}

}  // namespace

struct DcsDeep1x1Net {
    dcs_ctx* ctx = nullptr;
    int C = 4, tc = 0, F = 0, nb = 1;
    D1Layer L[kLayers];
    float *B11 = nullptr, *b11_0 = nullptr, *b11_1 = nullptr, *fbias = nullptr;
    int score_norm = DCS_SCORE_NORM_MAX, mix_sum = 0;
    DcsBuffer ws;
    float* rise_d = nullptr;
    int rise_ov = -1;
};

void dcs_deep1x1_destroy(DcsDeep1x1Net* g) {
    if (!g) return;
    for (auto& l : g->L) {
        dcs_dev_free(l.B); dcs_dev_free(l.b0); dcs_dev_free(l.b1); dcs_dev_free(l.Bt[0]); dcs_dev_free(l.Bt[1]);
    }
    dcs_dev_free(g->B11); dcs_dev_free(g->b11_0); dcs_dev_free(g->b11_1); dcs_dev_free(g->fbias); dcs_dev_free(g->rise_d);
    g->ws.release();
    delete g;
}

int dcs_deep1x1_create(dcs_ctx* ctx, int C, int tc, int F, const float* const* params_d, const int64_t* shapes, int nparams,
                       DcsDeep1x1Net** out) {
    if (C != 4) DCS_FAIL(DCS_EINVAL, "the deep score-informed network takes 4 input channels");
    if (tc < 19 || F < 253)
        DCS_FAIL(DCS_EINVAL, "time_context %d / feature size %d too small for build_ca_1x1 (needs >= 19 / >= 253)", tc, F);
    if (nparams != 3 * (kLayers + 1) + 1)
        DCS_FAIL(DCS_ESHAPE, "mismatch: got %d values to set %d parameters", nparams, 3 * (kLayers + 1) + 1);
    // branches the 1x1 layer holds: 4 (the whole graph) or 1 .. 3 (live-only layouts); any other row count is checked
    // against the whole graph's 800 and fails below
    const int64_t rows11 = shapes[4 * 3 * kLayers];
    const int nb_ok = (rows11 % kNf == 0 && rows11 >= kNf && rows11 <= 4 * kNf) ? (int)(rows11 / kNf) : 4;
    std::vector<std::vector<int64_t>> expect;
    int cin = C;
    for (int k = 0; k < kLayers; ++k) {
        expect.push_back({kFilters[k], cin, kKh[k], kKw});
        expect.push_back({kFilters[k]});
        expect.push_back({kFilters[k]});
        cin = kFilters[k];
    }
    expect.push_back({(int64_t)kNf * nb_ok, kNf, 1, 1});
    expect.push_back({(int64_t)kNf * nb_ok});
    expect.push_back({(int64_t)kNf * nb_ok});
    expect.push_back({(int64_t)C * nb_ok});
    std::vector<std::vector<float>> P(nparams);
    for (int i = 0; i < nparams; ++i) {
        int64_t cnt = 1;
        for (int k = 0; k < 4; ++k) {
            const int64_t want = k < (int)expect[i].size() ? expect[i][k] : 1;
            if (shapes[i * 4 + k] != want)
                DCS_FAIL(DCS_ESHAPE, "mismatch: parameter %d has shape dim %d = %lld but value to set has %lld", i, k,
                         (long long)want, (long long)shapes[i * 4 + k]);
            cnt *= want;
        }
        if (!params_d[i]) DCS_FAIL(DCS_EINVAL, "dcs_model_create: parameter %d is null", i);
        P[i].resize((size_t)cnt);
        DCS_HIP(hipMemcpy(P[i].data(), params_d[i], (size_t)cnt * sizeof(float), hipMemcpyDeviceToHost));
    }
    DcsDeep1x1Net* g = new DcsDeep1x1Net();
    g->ctx = ctx;
    g->C = C; g->tc = tc; g->F = F; g->nb = nb_ok;
    int H = tc, W = F;
    cin = C;
    int rc = DCS_OK;
    for (int k = 0; k < kLayers && rc == DCS_OK; ++k) {
        D1Layer& l = g->L[k];
        l.Cin = cin; l.Cinp = (int)dcs_round_up(cin, 4); l.Cout = kFilters[k]; l.Coutp = (int)dcs_round_up(l.Cout, 4);
        l.kh = kKh[k];
        l.Hi = H; l.Wi = W; l.Ho = H - l.kh + 1; l.Wo = (W - kKw) / 2 + 1;
        std::vector<float> B, Bt[2];
        pack_host(P[3 * k].data(), l.Cin, l.Cout, l.kh, kKw, B, Bt);
        char name[32];
        snprintf(name, sizeof name, "deep1x1.conv%d_B", k + 1);
        rc = upload_f32(&l.B, B, name);
        snprintf(name, sizeof name, "deep1x1.conv%d_Bt0", k + 1);
        if (rc == DCS_OK) rc = upload_f32(&l.Bt[0], Bt[0], name);
        snprintf(name, sizeof name, "deep1x1.conv%d_Bt1", k + 1);
        if (rc == DCS_OK) rc = upload_f32(&l.Bt[1], Bt[1], name);
        snprintf(name, sizeof name, "deep1x1.conv%d_b", k + 1);
        if (rc == DCS_OK) rc = upload_f32(&l.b0, P[3 * k + 1], name);
        snprintf(name, sizeof name, "deep1x1.conv%d_bias", k + 1);
        if (rc == DCS_OK) rc = upload_f32(&l.b1, P[3 * k + 2], name);
        H = l.Ho; W = l.Wo; cin = l.Cout;
    }
    if (rc == DCS_OK) {
        // 1x1: B[co][ci] = W[co][ci][0][0]
        const int n11 = kNf * nb_ok;
        std::vector<float> B;
        pack_host(P[18].data(), kNf, n11, 1, 1, B, nullptr);
        rc = upload_f32(&g->B11, B, "deep1x1.conv1x1_B");
        if (rc == DCS_OK) rc = upload_f32(&g->b11_0, P[19], "deep1x1.conv1x1_b");
        if (rc == DCS_OK) rc = upload_f32(&g->b11_1, P[20], "deep1x1.conv1x1_bias");
        if (rc == DCS_OK) rc = upload_f32(&g->fbias, P[21], "deep1x1.out_bias");
    }
    if (rc != DCS_OK) {
        dcs_deep1x1_destroy(g);
        return rc;
    }
    *out = g;
    return DCS_OK;
}

int dcs_deep1x1_out_channels(const DcsDeep1x1Net* g) { return g->C * g->nb; }

int dcs_deep1x1_set_score_semantics(DcsDeep1x1Net* g, int normalise, int mixture) {
    if ((normalise != DCS_SCORE_NORM_MAX && normalise != DCS_SCORE_NORM_SUM) || (mixture != DCS_MIX_CH0 && mixture != DCS_MIX_SUM))
        DCS_FAIL(DCS_EINVAL, "dcs_model_set_score_semantics: normalise %d / mixture %d", normalise, mixture);
    g->score_norm = normalise;
    g->mix_sum = mixture == DCS_MIX_SUM;
    return DCS_OK;
}

namespace {

struct D1Scratch {
    float *xcl, *a, *b, *g, *pm;
    uint8_t* code[kLayers];
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// bytes of one chunk of nc tiles; p != nullptr: also carve s out of p
size_t scratch_bytes(const DcsDeep1x1Net* g, int64_t nc, D1Scratch* s, char* p) {
    size_t act = (size_t)g->tc * g->F * g->C;
    for (const auto& l : g->L) act = std::max(act, (size_t)l.Ho * l.Wo * l.Coutp);
    const D1Layer& l6 = g->L[kLayers - 1];
    const size_t sz[5] = {align256((size_t)nc * g->tc * g->F * g->C * 4), align256((size_t)nc * act * 4),
                          align256((size_t)nc * act * 4), align256((size_t)g->nb * nc * l6.Ho * l6.Wo * kNf * 4),
                          align256((size_t)4 * nc * g->tc * g->F * 4)};
    size_t off = 0;
    float** f[5] = {&s->xcl, &s->a, &s->b, &s->g, &s->pm};
    for (int i = 0; i < 5; ++i) {
        if (p) *f[i] = (float*)(p + off);
        off += sz[i];
    }
    for (int k = 0; k < kLayers; ++k) {
        if (p) s->code[k] = (uint8_t*)(p + off);
        off += align256((size_t)nc * g->L[k].Ho * g->L[k].Wo * g->L[k].Coutp);
    }
    return off;
}

// nc tiles at x (from tile k_first of n_total) -> mask_mode 0/1: out [4][n_total] masked; 2: p [4 nb][n_total]
int forward_chunk(DcsDeep1x1Net* g, const float* x, int64_t nc, int64_t k_first, int64_t n_total, int mask_mode, float* out,
                  const D1Scratch& s) {
    dcs_ctx* ctx = g->ctx;
    const int64_t plane = (int64_t)g->tc * g->F;
    hipLaunchKernelGGL(d1_to_cl_kernel, dim3((unsigned)dcs_cdiv(nc * plane, kThreads)), dim3(kThreads), 0, ctx->stream, x, s.xcl,
                       nc * plane, plane);
    const float* cur = s.xcl;
    float* bufs[2] = {s.a, s.b};
    for (int k = 0; k < kLayers; ++k) {
        const D1Layer& l = g->L[k];
        D1Args a = forward_args(nc, l.Hi, l.Wi, l.Cinp, l.kh, kKw, 2, l.Cout);
        a.in = cur; a.B = l.B; a.b0 = l.b0; a.b1 = l.b1;
        a.out = bufs[k & 1]; a.code_out = s.code[k]; a.Co = l.Coutp;
        launch<MODE_FWD>(ctx, a);
        cur = bufs[k & 1];
    }
    const D1Layer& l6 = g->L[kLayers - 1];
    const int64_t m11 = nc * l6.Ho * l6.Wo;
    // the masks read branch 0 alone; the raw output wants every branch the model holds
    const int nb_run = mask_mode == 2 ? g->nb : 1;
    {
        D1Args a = forward_args(nc, l6.Ho, l6.Wo, kNf, 1, 1, 1, kNf * nb_run);
        a.in = cur; a.B = g->B11; a.b0 = g->b11_0; a.b1 = g->b11_1;
        a.out = s.g;
        launch<MODE_1X1>(ctx, a);
    }
    for (int br = 0; br < nb_run; ++br) {
        cur = s.g + (int64_t)br * m11 * kNf;
        for (int k = kLayers - 1; k >= 0; --k) {
            const D1Layer& l = g->L[k];
            float* dst = bufs[k & 1];   // conv_k's input size; k = 0 writes p instead
            for (int par = 0; par < 2; ++par) {
                D1Args a = transposed_args(nc, l.Ho, l.Wo, l.Coutp, l.Hi, l.Wi, l.kh, kKw, par, l.Cin);
                a.in = cur; a.code = s.code[k]; a.B = l.Bt[par];
                if (a.M == 0) continue;
                if (k > 0) {
                    a.out = dst; a.Co = l.Cinp;
                    launch<MODE_TR>(ctx, a);
                } else {
                    a.b0 = g->fbias + g->C * br;
                    if (mask_mode == 2) {
                        a.out = out; a.n_total = n_total; a.k_first = k_first; a.ch_off = g->C * br;
                    } else {
                        a.out = s.pm; a.n_total = nc; a.k_first = 0; a.ch_off = 0;
                    }
                    launch<MODE_LAST>(ctx, a);
                }
            }
            cur = dst;
        }
    }
    if (mask_mode != 2)
        hipLaunchKernelGGL(d1_mask_kernel, dim3((unsigned)dcs_cdiv(nc * plane, kThreads)), dim3(kThreads), 0, ctx->stream, s.pm, x,
                           out, nc, n_total, k_first, g->C, plane, mask_mode, g->mix_sum ? g->C : 1);
    DCS_HIP(hipGetLastError());
    return DCS_OK;
}

}  // namespace

int dcs_deep1x1_forward(DcsDeep1x1Net* g, const float* tiles, int64_t n, int mask_mode, float* out) {
    if (mask_mode < 0 || mask_mode > 2) DCS_FAIL(DCS_EINVAL, "bad mask mode %d", mask_mode);
    if (n == 0) return DCS_OK;
    const int64_t nc_max = std::min<int64_t>(n, kChunk);
    D1Scratch s;
    DCS_CHECK(g->ws.ensure(scratch_bytes(g, nc_max, &s, nullptr)));
    scratch_bytes(g, nc_max, &s, (char*)g->ws.ptr);
    const int64_t tile = (int64_t)g->C * g->tc * g->F;
    for (int64_t k0 = 0; k0 < n; k0 += nc_max) {
        const int64_t nc = std::min(nc_max, n - k0);
        DCS_CHECK(forward_chunk(g, tiles + k0 * tile, nc, k0, n, mask_mode, out, s));
    }
    return DCS_OK;
}

int dcs_deep1x1_separate(DcsDeep1x1Net* g, dcs_stft* plan, const float* audio, int64_t L, int ov, float scale, int eps_mode,
                         const DcsScoreNotes& notes, float* pcm, int64_t* n_tiles_out, int64_t* n_frames_out) {
    // separate_bach10.py / trainCNNrwc.py:357-416 with the library tiler: the composition of dcs_generic_separate's
    // score-informed branch, the network replaced by build_ca_1x1
    dcs_ctx* ctx = g->ctx;
    if (notes.ninst != g->C) DCS_FAIL(DCS_EINVAL, "score-informed path: %d score channels (got %d)", g->C, notes.ninst);
    if (eps_mode != DCS_EPS_A && eps_mode != DCS_EPS_B) DCS_FAIL(DCS_EINVAL, "bad eps_mode");
    const int tc = g->tc, F = g->F, st = tc - ov, S = 4;
    const int64_t T = dcs_frame_count(L, plan->hop);
    const int64_t n = dcs_tile_count(T, tc, ov, DCS_TILER_LIBRARY);
    if (n < 1) DCS_FAIL(DCS_EINVAL, "dcs_separate_scoreinformed: the tiler yields no tile");
    const int64_t ld = dcs_round_up(F, 4);
    const int64_t rows = n * st + tc;
    if (g->rise_ov != ov) {
        std::vector<float> r(ov > 0 ? ov : 1, 0.f);
        if (ov > 1) {
            const double step = 1.0 / (double)(ov - 1);
            for (int i = 0; i < ov; ++i) r[i] = (float)((double)i * step);
            r[ov - 1] = 1.0f;
        }
        if (g->rise_d) {
            DCS_HIP(hipStreamSynchronize(ctx->stream));
            dcs_dev_free(g->rise_d);
            g->rise_d = nullptr;
        }
        DCS_CHECK(upload_f32(&g->rise_d, r, "deep1x1.rise"));
        g->rise_ov = ov;
    }
    // the network's scratch first (ws grows to the larger of the two uses; the pipeline's buffers follow it)
    const int64_t nc_max = std::min<int64_t>(n, kChunk);
    D1Scratch s;
    const size_t b_net = align256(scratch_bytes(g, nc_max, &s, nullptr));
    const size_t b_mag = align256((size_t)T * ld * 4), b_unit = 2 * b_mag;
    const size_t b_inp = align256((size_t)g->C * T * F * 4);
    const size_t b_tiles = align256((size_t)n * g->C * tc * F * 4), b_out = align256((size_t)S * n * tc * F * 4);
    const size_t b_sep = align256((size_t)S * rows * ld * 4);
    DCS_CHECK(g->ws.ensure(b_net + b_mag + b_unit + b_inp + b_tiles + b_out + b_sep));
    char* p = (char*)g->ws.ptr;
    scratch_bytes(g, nc_max, &s, p); p += b_net;
    float* mag = (float*)p; p += b_mag;
    float2* unit = (float2*)p; p += b_unit;
    float* inp = (float*)p; p += b_inp;
    float* tiles = (float*)p; p += b_tiles;
    float* outm = (float*)p; p += b_out;
    float* sep = (float*)p;
    DCS_CHECK(dcs_launch_stft_forward_f32_clips(plan, audio, L, 0, 1, mag, nullptr, unit, ld, T, T));
    DCS_CHECK(dcs_score_masks_scaled(ctx, mag, ld, T, F, notes.notes_h, notes.ninst, notes.n_notes, notes.width, 0, T, scale, inp,
                                     nullptr, g->score_norm));
    DCS_CHECK(dcs_launch_tile(ctx, inp, T * (int64_t)F, F, g->C, T, F, tc, ov, DCS_TILER_LIBRARY, 1.0f, tiles, n));
    for (int64_t k0 = 0; k0 < n; k0 += nc_max) {
        const int64_t nc = std::min(nc_max, n - k0);
        DCS_CHECK(forward_chunk(g, tiles + k0 * g->C * tc * (int64_t)F, nc, k0, n, eps_mode, outm, s));
    }
    DCS_CHECK(dcs_launch_overlap_add(ctx, outm, n, S, tc, ov, F, g->rise_d, sep, rows * ld, ld, n * tc * (int64_t)F));
    DCS_CHECK(dcs_launch_stft_inverse_f32_clips(plan, sep, rows * ld, unit, T * ld, ld, T, S, 1, scale, pcm, L));
    if (n_tiles_out) *n_tiles_out = n;
    if (n_frames_out) *n_frames_out = T;
    return DCS_OK;
}

// ------------------------------------------------------------------------------------------------ test aids (include/dcs.h)
extern "C" int dcs_debug_d1_conv(dcs_ctx* ctx, int mode, dcs_debug_d1_args* q) {
    if (!ctx || !q) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_conv: null argument");
    if (mode == MODE_FWDC || mode == MODE_Q || mode == MODE_B11 || q->trainer_unit) return deep1x1_trainer_debug_conv(ctx, mode, q);
    D1Args a;
    DCS_CHECK(debug_conv_args(mode, q, &a));
    DCS_ON_DEVICE(ctx->device);
    switch (mode) {
        case MODE_FWD: return debug_conv_run<MODE_FWD>(ctx, a);
        case MODE_1X1: return debug_conv_run<MODE_1X1>(ctx, a);
        case MODE_TR: return debug_conv_run<MODE_TR>(ctx, a);
        default: return debug_conv_run<MODE_LAST>(ctx, a);
    }
}

extern "C" int dcs_debug_d1_aux(dcs_ctx* ctx, int which, dcs_debug_d1_aux_args* q) {
    if (!ctx || !q) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: null argument");
    if (which == DCS_D1_AUX_CODE_APPLY || which == DCS_D1_AUX_CODES_OUT || which == DCS_D1_AUX_PACK_DEVICE)
        return deep1x1_trainer_debug_aux(ctx, which, q);
    const int64_t big = (int64_t)1 << 30;
    if (which == DCS_D1_AUX_TO_CL) {
        if (q->n < 1 || q->plane < 1 || q->n > big || q->plane > big || q->n * q->plane > big)
            DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: %lld tiles of %lld pixels", (long long)q->n, (long long)q->plane);
        const int64_t px = q->n * q->plane;
        if (dbg_bad(q->in, q->in_bytes, px * 16) || dbg_bad(q->out, q->out_bytes, px * 16)) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: to_cl buffers");
        DCS_ON_DEVICE(ctx->device);
        hipLaunchKernelGGL(d1_to_cl_kernel, dim3((unsigned)dcs_cdiv(px, kThreads)), dim3(kThreads), 0, ctx->stream, (const float*)q->in,
                           (float*)q->out, px, q->plane);
    } else if (which == DCS_D1_AUX_MASK) {
        if (q->n < 1 || q->plane < 1 || q->n > big || q->plane > big || q->n * q->plane > big || q->n_total < q->n || q->n_total > big ||
            q->k_first < 0 || q->k_first + q->n > q->n_total || q->n_total * q->plane > big)
            DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: tiles %lld + %lld of %lld, %lld pixels each", (long long)q->k_first, (long long)q->n,
                     (long long)q->n_total, (long long)q->plane);
        if (q->C < 1 || q->C > 64 || q->mix_n < 1 || q->mix_n > q->C || (q->mode != DCS_EPS_A && q->mode != DCS_EPS_B))
            DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: %d channels, mixture of %d, eps mode %d", q->C, q->mix_n, q->mode);
        const int64_t px = q->n * q->plane;
        if (dbg_bad(q->in, q->in_bytes, 4 * px * 4) || dbg_bad(q->in2, q->in2_bytes, q->C * px * 4) ||
            dbg_bad(q->out, q->out_bytes, 4 * q->n_total * q->plane * 4))
            DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: mask buffers");
        DCS_ON_DEVICE(ctx->device);
        hipLaunchKernelGGL(d1_mask_kernel, dim3((unsigned)dcs_cdiv(px, kThreads)), dim3(kThreads), 0, ctx->stream, (const float*)q->in,
                           (const float*)q->in2, (float*)q->out, q->n, q->n_total, q->k_first, q->C, q->plane, q->mode, q->mix_n);
    } else if (which == DCS_D1_AUX_PACK_HOST) {
        if ((q->kw != 1 && q->kw != kKw) || q->kh < 1 || q->kh > kDbgMaxKh || q->Cin < 1 || q->Cin > kDbgMaxCh || q->Cout < 1 ||
            q->Cout > kDbgMaxCh)
            DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: weights [%d][%d][%d][%d]", q->Cout, q->Cin, q->kh, q->kw);
        const int64_t nw = (int64_t)q->Cout * q->Cin * q->kh * q->kw;
        if (dbg_bad(q->in, q->in_bytes, nw * 4)) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: W");
        DCS_ON_DEVICE(ctx->device);
        std::vector<float> W((size_t)nw), B, Bt[2];
        DCS_HIP(hipMemcpy(W.data(), q->in, (size_t)nw * 4, hipMemcpyDeviceToHost));
        pack_host(W.data(), q->Cin, q->Cout, q->kh, q->kw, B, Bt);
        void* dst[3] = {q->out, q->out2, q->out3};
        const int64_t have[3] = {q->out_bytes, q->out2_bytes, q->out3_bytes};
        const std::vector<float>* src[3] = {&B, &Bt[0], &Bt[1]};
        for (int i = 0; i < 3; ++i)
            if (!src[i]->empty() && dbg_bad(dst[i], have[i], (int64_t)src[i]->size() * 4)) DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: operand %d", i);
        for (int i = 0; i < 3; ++i)
            if (!src[i]->empty()) DCS_HIP(hipMemcpy(dst[i], src[i]->data(), src[i]->size() * 4, hipMemcpyHostToDevice));
    } else {
        DCS_FAIL(DCS_EINVAL, "dcs_debug_d1_aux: which = %d", which);
    }
    DCS_HIP(hipGetLastError());
    DCS_HIP(hipStreamSynchronize(ctx->stream));
    return DCS_OK;
}

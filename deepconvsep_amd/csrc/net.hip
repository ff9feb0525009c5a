// Network handle (build_ca + set_all_param_values), predict_function2 and the fused file-level
// separation path.  Reference: examples/dsd100/separate_dsd.py:172-311.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <utility>
#include <vector>

#include "dcs_internal.h"
#include "deep1x1.h"
#include "dsd.h"
#include "dsd_lat.h"
#include "generic.h"

namespace {

struct Dims {
    int nf1, kw1, sw1, w1, pool_w, wp, nf2, kh2, kw2, h2, w2, flat, hidden, n_fc, n_branch, S;
    int branch_fc[4];
};

int arch_dims(int arch, int C, int tc, int F, Dims* d) {
    memset(d, 0, sizeof(*d));
    switch (arch) {
        case DCS_ARCH_DSD:  // separate_dsd.py:198-234
            d->nf1 = 50; d->kw1 = F; d->sw1 = 1; d->pool_w = 0;
            d->nf2 = 50; d->kh2 = tc / 2; d->kw2 = 1; d->hidden = 128;
            d->n_fc = 3; d->n_branch = 4; d->S = 4;
            d->branch_fc[0] = 0; d->branch_fc[1] = 1; d->branch_fc[2] = 2; d->branch_fc[3] = 1;
            if (C != 1) DCS_FAIL(DCS_EINVAL, "dsd network takes 1 input channel");
            break;
        case DCS_ARCH_DSD_ILD:  // dsd100_2ch_ILD/trainCNN_ILD_DSD100.py:86-115: stereo input, one branch per source
            d->nf1 = 50; d->kw1 = F; d->sw1 = 1; d->pool_w = 0;
            d->nf2 = 50; d->kh2 = tc / 2; d->kw2 = 1; d->hidden = 256;
            d->n_fc = 4; d->n_branch = 4; d->S = 4;
            for (int i = 0; i < 4; ++i) d->branch_fc[i] = i;
            if (C != 2) DCS_FAIL(DCS_EINVAL, "the stereo (ILD) network takes 2 input channels");
            break;
        case DCS_ARCH_IKALA:         // separate_ikala.py:173-191
        case DCS_ARCH_IKALA_NOPOOL:  // ikala/trainCNN.py:87-118: the same graph without the MaxPool2DLayer
            d->nf1 = 30; d->kw1 = 30; d->sw1 = 3; d->pool_w = arch == DCS_ARCH_IKALA ? 4 : 0;
            d->nf2 = 30; d->kh2 = 10; d->kw2 = 20; d->hidden = 256;
            d->n_fc = 2; d->n_branch = 2; d->S = 2;
            d->branch_fc[0] = 0; d->branch_fc[1] = 1;
            if (C != 1) DCS_FAIL(DCS_EINVAL, "ikala network takes 1 input channel");
            break;
        case DCS_ARCH_BACH10:     // separate_bach10.py:197-227
        case DCS_ARCH_BACH10_SI:  // bach10_scoreinformed/separate_bach10.py:414-444
        case DCS_ARCH_BACH10_SI1: // bach10_scoreinformed/trainCNNrwc_samp.py:195-235: one dense layer back, one decoder branch
            d->nf1 = 30; d->kw1 = 30; d->sw1 = 4; d->pool_w = 0;
            d->nf2 = 30; d->kh2 = (2 * tc) / 3; d->kw2 = 1; d->hidden = 256;
            d->n_fc = 4; d->n_branch = 4; d->S = 4;
            for (int i = 0; i < 4; ++i) d->branch_fc[i] = i;
            if (arch == DCS_ARCH_BACH10_SI1) {
                d->n_fc = 1; d->n_branch = 1;
                for (int i = 1; i < 4; ++i) d->branch_fc[i] = 0;
                if (C != 4) DCS_FAIL(DCS_EINVAL, "score-informed network takes 4 input channels");
            }
            if (arch == DCS_ARCH_BACH10 && C != 1) DCS_FAIL(DCS_EINVAL, "bach10 network takes 1 input channel");
            if (arch == DCS_ARCH_BACH10_SI && C != 4)
                DCS_FAIL(DCS_EINVAL, "score-informed network takes 4 input channels");
            break;
        default:
            DCS_FAIL(DCS_EINVAL, "unknown architecture %d", arch);
    }
    if (F < d->kw1) DCS_FAIL(DCS_EINVAL, "feature size %d smaller than the conv1 filter %d", F, d->kw1);
    d->w1 = (F - d->kw1) / d->sw1 + 1;
    d->wp = d->pool_w ? d->w1 / d->pool_w : d->w1;
    d->h2 = tc - d->kh2 + 1;
    d->w2 = d->wp - d->kw2 + 1;
    if (d->h2 < 1 || d->w2 < 1 || d->kh2 < 1) DCS_FAIL(DCS_EINVAL, "time_context %d / feature size %d too small", tc, F);
    d->flat = d->nf2 * d->h2 * d->w2;
    return DCS_OK;
}

template <typename T>
int upload(T** dst, const std::vector<T>& src, const char* name) {
    DCS_HIP(dcs_dev_alloc((void**)dst, src.size() * sizeof(T), name));
    DCS_HIP(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return DCS_OK;
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

struct dcs_model {
    dcs_ctx* ctx = nullptr;
    int arch = 0, C = 1, tc = 30, F = 0;
    Dims d;
    // ---- DSD packed weights
    int CI = 0, CP = 0, K1 = 0, Fpad = 0, hid64 = 0, nd = 0, nd64 = 0;
    int d2_ng = 4, d2_gs = 0, d2_gcols = 0;  // transposed conv2: channel groups, channels per group, padded columns
    float *B1 = nullptr, *bias1 = nullptr, *B2 = nullptr, *bias2 = nullptr, *Bfc = nullptr, *biasfc = nullptr;
    float *Bd = nullptr, *biasd = nullptr, *Bw2 = nullptr, *Bw2s = nullptr, *Bfin = nullptr, *bout = nullptr;
    // conv2 -> bias -> bottleneck layer folded into one affine map over a tile's tc rows of conv1 output (pack_dsd)
    float *B2fc = nullptr, *bias2fc = nullptr;
    float* B2fc_frag = nullptr;   // the same weights in gemm_rows_splitk_kernel's fragment order (DcsGemm::Bfrag)
    // ---- generic path (ikala / bach10 / score-informed)
    DcsGenericNet* gen = nullptr;
    // ---- the deep score-informed graph build_ca_1x1 (deep1x1.hip)
    DcsDeep1x1Net* deep = nullptr;
    // ---- scratch
    DcsBuffer ws;
    // bf16x3 kernels: the transposed-conv1 and conv2 weights split into three bf16 planes
    uint16_t* Bpk = nullptr;
    uint16_t* Bw2q = nullptr;
    void* Bdq = nullptr;   // per-source dense weights as bf16 planes (gemm_bf16x3.hip)
    // one-batch ("latency") kernels, dsd_lat.hip: the GEMM B operands in MFMA fragment order, the transposed-conv2
    // weights likewise; lat_stages = -1: automatic (all stages for one clip of at most lat_max_frames frames)
    float *L1p = nullptr, *L2p = nullptr, *Lfcp = nullptr, *Ldp = nullptr, *Lw2p = nullptr;
    int lat_slice1 = 0;
    bool lat_ok = false;
    int lat_stages = -1;
    DcsUploadRing clip_ring;   // {samples, frames, tiles} per clip of a batch of different lengths (dcs_separate_ragged)
    // cross-fade ramps np.linspace(0, 1, ov), one device table per overlap ever asked for; a table is never freed or
    // re-allocated while the model lives (captured graphs of other call shapes keep pointing at theirs)
    std::vector<std::pair<int, float*>> rise_tabs;
    float* rise_d = nullptr;   // the table of the current call (set by ensure_rise)
    // ---- hipGraph of the fused step (dcs_separate; opt-in, DCS_GRAPH=1): the launches of one call replayed as one launch.
    // A graph is captured the second time the same call (same buffers, sizes, options) arrives.
    struct StepKey {
        const void* plan = nullptr; const void* audio = nullptr; const void* pcm = nullptr; const void* ws = nullptr;
        int64_t L = -1, n_clips = 1, audio_stride = 0; int ov = 0, tiler = 0, eps = 0, tie = 0, lat = -1; float scale = 0.f;
        bool operator==(const StepKey& o) const {
            return lat == o.lat && plan == o.plan && audio == o.audio && pcm == o.pcm && ws == o.ws && L == o.L && ov == o.ov &&
                   tiler == o.tiler && eps == o.eps && tie == o.tie && scale == o.scale && n_clips == o.n_clips &&
                   audio_stride == o.audio_stride;
        }
    };
    // A small LRU: a server alternates between a few call shapes (full launch groups and a remainder group, two clip
    // lengths); each keeps its own captured graph.  `seen` holds the keys that arrived once and are captured on their
    // second arrival.
    struct StepGraph {
        StepKey key;
        hipGraphExec_t exec = nullptr;
        int64_t tiles = 0, frames = 0;
        uint64_t stamp = 0;
    };
    static constexpr int kStepGraphs = 4;
    StepGraph graphs[kStepGraphs];
    StepKey seen[kStepGraphs];
    uint64_t seen_stamp[kStepGraphs] = {0, 0, 0, 0};
    uint64_t step_clock = 0;
};

namespace {

int ensure_rise(dcs_model* m, int ov) {
    for (const auto& t : m->rise_tabs)
        if (t.first == ov) {
            m->rise_d = t.second;
            return DCS_OK;
        }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (m->ctx->stream && hipStreamIsCapturing(m->ctx->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        DCS_FAIL(DCS_EHIP, "ensure_rise: new overlap %d during a stream capture", ov);   // callers create it before capturing
    std::vector<float> r(ov > 0 ? ov : 1, 0.f);
    // np.linspace(0., 1.0, num=overlap)  (util.py:306): arange * (1/(ov-1)), last element = 1.0
    if (ov > 1) {
        const double step = 1.0 / (double)(ov - 1);
        for (int i = 0; i < ov; ++i) r[i] = (float)((double)i * step);
        r[ov - 1] = 1.0f;
    }
    float* d = nullptr;
    DCS_HIP(dcs_dev_alloc((void**)&d, r.size() * sizeof(float), "dsd.rise"));
    DCS_HIP(hipMemcpy(d, r.data(), r.size() * sizeof(float), hipMemcpyHostToDevice));
    m->rise_tabs.emplace_back(ov, d);
    m->rise_d = d;
    return DCS_OK;
}

// Re-layout of the DSD parameters into the GEMM operands (see DESIGN.md "weight packing").
int pack_dsd(dcs_model* m, const std::vector<std::vector<float>>& P) {
    const Dims& d = m->d;
    const int F = m->F;
    const int CI = (int)dcs_round_up(d.nf1, 4), CP = (int)dcs_round_up(d.nf2, 4);
    m->CI = CI;
    m->CP = CP;
    // C input channels sit side by side in a spectrogram row of C * ld floats (ld = F rounded up to 4): conv1's K axis
    // and the final kernel's bin axis both run over (channel, bin)
    const int C = m->C, ldF = (int)dcs_round_up(F, 4);
    m->K1 = C * ldF;
    m->Fpad = (int)dcs_round_up((int64_t)(C - 1) * ldF + F, 128);  // pitch of the final kernel's weights: whole 128-bin workgroups
    m->d2_ng = 4;
    m->d2_gs = (CI + m->d2_ng - 1) / m->d2_ng;
    m->d2_gcols = (int)dcs_round_up(m->d2_gs * d.kh2, 16);
    m->hid64 = (int)dcs_round_up(d.hidden, 64);
    m->nd = d.n_fc * d.h2 * CP;
    m->nd64 = (int)dcs_round_up(m->nd, 64);
    if (CI > 64 || CP > 64) DCS_FAIL(DCS_EUNSUPPORTED, "dsd packing: more than 64 filters");
    const float *W1 = P[0].data(), *b1 = P[1].data(), *b1b = P[2].data();
    const float *W2 = P[3].data(), *b2 = P[4].data(), *b2b = P[5].data();
    const float *Wfc = P[6].data(), *bfc = P[7].data();

    // conv1 (true convolution = correlation with the flipped filter): B1[f][c] = W1[c,0,0,F-1-f]
    std::vector<float> B1((size_t)dcs_round_up(m->K1, 128) * 64, 0.f), bias1(64, 0.f);
    for (int c = 0; c < d.nf1; ++c) {
        for (int ch = 0; ch < C; ++ch)
            for (int f = 0; f < F; ++f)
                B1[(size_t)(ch * ldF + f) * 64 + c] = W1[((size_t)c * C + ch) * F + (F - 1 - f)];
        bias1[c] = b1[c] + b1b[c];
    }
    // conv2: B2[u*CI + ci][co] = W2[co,ci,kh-1-u,0]
    const int kh = d.kh2;
    std::vector<float> B2((size_t)dcs_round_up(kh * CI, 128) * 64, 0.f), bias2(64, 0.f);
    for (int co = 0; co < d.nf2; ++co) {
        for (int ci = 0; ci < d.nf1; ++ci)
            for (int u = 0; u < kh; ++u)
                B2[(size_t)(u * CI + ci) * 64 + co] = W2[((size_t)co * d.nf1 + ci) * kh + (kh - 1 - u)];
        bias2[co] = b2[co] + b2b[co];
    }
    // bottleneck: input index of the flattened [nf2, h2, 1] map is co*h2 + t'; ours is t'*CP + co
    std::vector<float> Bfc((size_t)dcs_round_up(d.h2 * CP, 128) * m->hid64, 0.f), biasfc(m->hid64, 0.f);
    for (int co = 0; co < d.nf2; ++co)
        for (int t = 0; t < d.h2; ++t)
            for (int h = 0; h < d.hidden; ++h)
                Bfc[(size_t)(t * CP + co) * m->hid64 + h] = Wfc[(size_t)(co * d.h2 + t) * d.hidden + h];
    for (int h = 0; h < d.hidden; ++h) biasfc[h] = bfc[h];
    // conv2 and its BiasLayer are LINEAR (nonlinearity=None, separate_dsd.py:202-203) and feed the bottleneck DenseLayer only
    // (:206), so  Z = relu(flatten(conv2(H1) + b2) . Wfc + bfc)  is one affine map of the tile's tc rows of H1 followed by the
    // rectifier:  Z = relu(sum_r H1[row0 + r] . W2fc[r] + c),  W2fc[r][ci][h] = sum_{u + t = r} sum_co W2[co,ci,u] Wfc[(co,t)][h],
    // c[h] = bfc[h] + sum_{t,co} b2[co] Wfc[(co,t)][h].  Folded here in float64, rounded once to float32: K = tc * CI = 1560
    // against conv2's 750 on 5.9 x as many rows plus the bottleneck's 832 -- fewer flops, one launch instead of two, and the
    // conv2 map (positions x 50) is never written.  The fused launches with more than one batch take it (dsd_encode).
    std::vector<float> B2fc((size_t)dcs_round_up(m->tc * CI, 128) * m->hid64, 0.f), bias2fc(m->hid64, 0.f);
    {
        std::vector<double> acc((size_t)m->tc * CI * m->hid64, 0.0), cb(m->hid64, 0.0);
        for (int u = 0; u < kh; ++u)
            for (int ci = 0; ci < d.nf1; ++ci)
                for (int co = 0; co < d.nf2; ++co) {
                    const double w2 = B2[(size_t)(u * CI + ci) * 64 + co];
                    if (w2 == 0.0) continue;
                    for (int t = 0; t < d.h2; ++t) {
                        const float* fr = &Bfc[(size_t)(t * CP + co) * m->hid64];
                        double* ar = &acc[(size_t)((u + t) * CI + ci) * m->hid64];
                        for (int h = 0; h < d.hidden; ++h) ar[h] += w2 * (double)fr[h];
                    }
                }
        for (int h = 0; h < d.hidden; ++h) cb[h] = bfc[h];
        for (int t = 0; t < d.h2; ++t)
            for (int co = 0; co < d.nf2; ++co) {
                const double b = bias2[co];
                const float* fr = &Bfc[(size_t)(t * CP + co) * m->hid64];
                for (int h = 0; h < d.hidden; ++h) cb[h] += b * (double)fr[h];
            }
        for (size_t i = 0; i < acc.size(); ++i) B2fc[i] = (float)acc[i];
        for (int h = 0; h < d.hidden; ++h) bias2fc[h] = (float)cb[h];
    }
    // per-source dense layers, concatenated along N and permuted to [branch][t'][co]
    std::vector<float> Bd((size_t)dcs_round_up(m->hid64, 128) * m->nd64, 0.f), biasd(m->nd64, 0.f);
    for (int s = 0; s < d.n_fc; ++s) {
        const float* Ws = P[8 + 2 * s].data();
        const float* bs = P[9 + 2 * s].data();
        for (int co = 0; co < d.nf2; ++co)
            for (int t = 0; t < d.h2; ++t) {
                const size_t col = (size_t)(s * d.h2 + t) * CP + co;
                for (int h = 0; h < d.hidden; ++h) Bd[(size_t)h * m->nd64 + col] = Ws[(size_t)h * d.flat + co * d.h2 + t];
                biasd[col] = bs[co * d.h2 + t];
            }
    }
    // transposed conv2: Bw2[co][g*gcols + c*kh + dt] = W2[co, g*GS + c, kh-1-dt, 0]
    const int ldw2 = m->d2_ng * m->d2_gcols;
    std::vector<float> Bw2((size_t)CP * ldw2, 0.f);
    for (int co = 0; co < d.nf2; ++co)
        for (int ci = 0; ci < d.nf1; ++ci)
            for (int dt = 0; dt < kh; ++dt)
                Bw2[(size_t)co * ldw2 + (ci / m->d2_gs) * m->d2_gcols + (ci % m->d2_gs) * kh + dt] =
                    W2[((size_t)co * d.nf1 + ci) * kh + (kh - 1 - dt)];
    // the same weights for the streaming kernel: Bw2s[ci][dt][co], 16 tap slots per channel, whole groups of 8
    std::vector<float> Bw2s((size_t)dcs_round_up(CI, kDsdGch) * 16 * CP, 0.f);
    if (kh <= 16)
        for (int co = 0; co < d.nf2; ++co)
            for (int ci = 0; ci < d.nf1; ++ci)
                for (int dt = 0; dt < kh; ++dt)
                    Bw2s[((size_t)ci * 16 + dt) * CP + co] = W2[((size_t)co * d.nf1 + ci) * kh + (kh - 1 - dt)];
    // transposed conv1: Bfin[c][f] = W1[c,0,0,F-1-f]
    std::vector<float> Bfin((size_t)CI * m->Fpad, 0.f);
    for (int c = 0; c < d.nf1; ++c)
        for (int ch = 0; ch < C; ++ch)
            for (int f = 0; f < F; ++f)
                Bfin[(size_t)c * m->Fpad + ch * ldF + f] = W1[((size_t)c * C + ch) * F + (F - 1 - f)];
    std::vector<float> bout(P[8 + 2 * d.n_fc].begin(), P[8 + 2 * d.n_fc].end());

    DCS_CHECK(upload(&m->B1, B1, "dsd.B1"));
    DCS_CHECK(upload(&m->bias1, bias1, "dsd.bias1"));
    DCS_CHECK(upload(&m->B2, B2, "dsd.B2"));
    DCS_CHECK(upload(&m->bias2, bias2, "dsd.bias2"));
    DCS_CHECK(upload(&m->Bfc, Bfc, "dsd.Bfc"));
    DCS_CHECK(upload(&m->biasfc, biasfc, "dsd.biasfc"));
    if (d.h2 + kh - 1 == m->tc) {   // (always: h2 = tc - kh + 1)
        DCS_CHECK(upload(&m->B2fc, B2fc, "dsd.B2fc"));
        DCS_CHECK(upload(&m->bias2fc, bias2fc, "dsd.bias2fc"));
        {   // fragment order of the few-rows GEMM (launch groups of up to ~1000 tiles take that kernel for this layer); whole
            // 64-K steps per column block, the chunks past K zero
            const int K = m->tc * CI, kc = dcs_bfrag_chunks(K), nt = m->hid64 / 16;
            std::vector<float> fr((size_t)nt * kc * 64 * 4, 0.f);
            dcs_gemm_pack_bfrag(B2fc.data(), K, m->hid64, m->hid64, fr.data());
            DCS_CHECK(upload(&m->B2fc_frag, fr, "dsd.B2fc_frag"));
        }
    }
    DCS_CHECK(upload(&m->Bd, Bd, "dsd.Bd"));
    DCS_CHECK(upload(&m->biasd, biasd, "dsd.biasd"));
    DCS_CHECK(upload(&m->Bw2, Bw2, "dsd.Bw2"));
    DCS_CHECK(upload(&m->Bw2s, Bw2s, "dsd.Bw2s"));
    DCS_CHECK(upload(&m->Bfin, Bfin, "dsd.Bfin"));
    DCS_CHECK(upload(&m->bout, bout, "dsd.bout"));
    {
        // the per-source dense weights once more as three bf16 planes, split on the device (the wide-B GEMM of large
        // launches runs on the bf16 matrix pipe; the encoder GEMMs are latency-bound and stay f32)
        const int rows = (int)dcs_round_up(m->hid64, 128);
        DCS_HIP(dcs_dev_alloc(&m->Bdq, dcs_gemm_bq_bytes(rows, m->nd64), "dsd.Bdq"));
        DCS_CHECK(dcs_gemm_pack_bq(m->ctx, m->Bd, rows, m->nd64, m->nd64, m->Bdq));
    }
    if (C == 1) {
        // bf16x3 variant of the final kernel: Bpk[bin][plane 3][K block 2][lane group 4][8 channels], channel
        // c = 32 kb + 8 g + j; planes by truncation, w = p0 + p1 + p2 exactly
        std::vector<uint16_t> Bpk((size_t)m->Fpad * 3 * 2 * 4 * 8, 0);
        for (int f = 0; f < m->Fpad; ++f)
            for (int c = 0; c < d.nf1 && c < 64; ++c) {
                const float w = Bfin[(size_t)c * m->Fpad + f];
                float r = w;
                for (int pl = 0; pl < 3; ++pl) {
                    uint32_t bits;
                    memcpy(&bits, &r, 4);
                    bits &= 0xffff0000u;
                    float part;
                    memcpy(&part, &bits, 4);
                    r -= part;
                    const int kb = c >> 5, g = (c & 31) >> 3, j = c & 7;
                    Bpk[((((size_t)f * 3 + pl) * 2 + kb) * 4 + g) * 8 + j] = (uint16_t)(bits >> 16);
                }
            }
        DCS_CHECK(upload(&m->Bpk, Bpk, "dsd.Bpk"));
        // streaming deconv2 on the bf16 pipe: Bw2q[group][channel 8][tap 16][25 pieces][8 bf16]; piece plane * 8 + kb * 4 +
        // kq holds filters co = 32 kb + 8 kq + j of W2c[co, ci, dt]; x = plane0 + plane1 + plane2 exactly
        std::vector<uint16_t> Bw2q(dsd_d2q_bytes(CI) / 2, 0);
        if (kh <= 16)
            for (int ci = 0; ci < d.nf1; ++ci)
                for (int dt = 0; dt < kh; ++dt)
                    for (int co = 0; co < d.nf2; ++co) {
                        float r = Bw2s[((size_t)ci * 16 + dt) * CP + co];
                        const int kb = co >> 5, kq = (co & 31) >> 3, j = co & 7;
                        for (int pl = 0; pl < 3; ++pl) {
                            uint32_t bits;
                            memcpy(&bits, &r, 4);
                            bits &= 0xffff0000u;
                            float part;
                            memcpy(&part, &bits, 4);
                            r -= part;
                            Bw2q[(((size_t)ci * 16 + dt) * kDsdD2qTapU4 + pl * 8 + kb * 4 + kq) * 8 + j] = (uint16_t)(bits >> 16);
                        }
                    }
        DCS_CHECK(upload(&m->Bw2q, Bw2q, "dsd.Bw2q"));
    }
    // one-batch kernels (dsd_lat.hip): built for the reference's DSD shapes (50 + 50 filters, time_context 30, 128 hidden units)
    if (C == 1 && CI == 52 && CP == 52 && d.h2 == 16 && kh == 15 && m->tc == 30 && m->hid64 == 128 && d.n_fc == 3 && m->Bpk) {
        std::vector<float> pk;
        m->lat_slice1 = (int)dcs_round_up((m->K1 + 15) / 16, 4);
        dcs_lat_pack_b(B1.data(), 64, m->K1, 4, m->lat_slice1, 16, &pk);
        DCS_CHECK(upload(&m->L1p, pk, "dsd.L1p"));
        dcs_lat_pack_b(B2.data(), 64, kh * CI, 4, CI, kh, &pk);       // one slice per tap
        DCS_CHECK(upload(&m->L2p, pk, "dsd.L2p"));
        dcs_lat_pack_b(Bfc.data(), m->hid64, d.h2 * CP, m->hid64 / 16, CP, d.h2, &pk);
        DCS_CHECK(upload(&m->Lfcp, pk, "dsd.Lfcp"));
        dcs_lat_pack_b(Bd.data(), m->nd64, m->hid64, m->nd64 / 16, 32, 4, &pk);
        DCS_CHECK(upload(&m->Ldp, pk, "dsd.Ldp"));
        dcs_lat_pack_deconv2(Bw2s.data(), (int)dcs_round_up(CI, kDsdGch), &pk);
        DCS_CHECK(upload(&m->Lw2p, pk, "dsd.Lw2p"));
        m->lat_ok = true;
    }
    return DCS_OK;
}

struct DsdScratch {
    float *H1, *C2, *Z, *D, *G;
    void* Gs;   // bf16 planes of G for the bf16x3 final kernel (null: f32 G only)
};

// Encoder + dense layers + transposed conv2 for n tiles whose frames are rows of `rows_src`.
//   fused   : rows_src = scaled spectrogram rows (frame t), tile k starts at frame k*st
//   per tile: rows_src = tile frames (k*tc + j)
//   clips   : n_clips > 1 stacked clips of n tiles each (fused only); clip c's frames start at row c * clip_pitch
//             (a multiple of st).  conv1 / conv2 simply run over all rows -- positions that straddle two clips are
//             computed and never read -- and the bottleneck's A row of tile (c, k) is row c*clip_pitch + k*st.
//   lat     : stage bits (dsd_lat.h) whose layer runs on the one-batch kernels of dsd_lat.hip (one clip, shared frames)
//   ragged  : (rows_total, tiles_total, rowmap) -- clips of different lengths in the compact layout (kDcsClipTab): the rows of
//             all clips back to back, the tiles of all clips back to back, rowmap[tile] = first C2 row of the tile / st
int dsd_encode(dcs_model* m, const float* rows_src, int64_t lda, bool a_vec, float a_scale, int64_t n,
               int64_t tile_row_stride /* st or tc */, bool shared_frames, const DsdScratch& w, int64_t n_clips = 1,
               int64_t clip_pitch = 0, unsigned lat = 0, int64_t rows_total = 0, int64_t tiles_total = 0,
               const int* rowmap = nullptr) {
    const Dims& d = m->d;
    const int tc = m->tc, CI = m->CI, CP = m->CP;
    const int64_t BIG = (int64_t)1 << 40;
    const bool clips = n_clips > 1;
    if (clips && (!shared_frames || clip_pitch % tile_row_stride != 0 || n > 0x7fffffff))
        DCS_FAIL(DCS_EINVAL, "dsd_encode: bad clip batch");
    if (lat && (!shared_frames || !a_vec || !m->lat_ok)) DCS_FAIL(DCS_EINVAL, "dsd_encode: the one-batch kernels need shared frames");
    // two consecutive one-batch GEMMs: the first leaves its K reduction as 4 partial arrays (4 workgroups of 4 waves per
    // output block instead of one of 16), the second adds them while it loads its operand (DESIGN.md "one batch")
    const bool split1 = (lat & DCS_LAT_CONV1) && (lat & DCS_LAT_CONV2);
    const bool split2 = (lat & DCS_LAT_CONV2) && (lat & DCS_LAT_FC);
    const bool split3 = (lat & DCS_LAT_FC) && (lat & DCS_LAT_FC1X);
    // conv1 + both biases  (separate_dsd.py:198-199)
    const bool ragged = rowmap != nullptr;
    if (ragged && (!clips || lat || rows_total < tc || tiles_total < 1)) DCS_FAIL(DCS_EINVAL, "dsd_encode: bad ragged batch");
    const int64_t n_rows1 = ragged ? rows_total : (clips ? n_clips * clip_pitch : (shared_frames ? (n - 1) * tile_row_stride + tc : n * tc));
    const int64_t n_tiles_all = ragged ? tiles_total : n * n_clips;
    DcsGemm g1{};
    g1.A = rows_src; g1.lda = lda; g1.a_gdiv = 1 << 30; g1.a_gmul = 0; g1.a_scale = a_scale;
    g1.B = m->B1; g1.ldb = 64; g1.bias = m->bias1;
    g1.C = w.H1; g1.ldc = CI; g1.c_gdiv = 1 << 30; g1.c_gmul = 0;
    g1.M = n_rows1; g1.n_cols = 64; g1.n_store = CI; g1.K = a_vec ? m->K1 : m->F; g1.relu = 0; g1.a_vec = a_vec;
    (void)BIG;
    if (lat & DCS_LAT_CONV1) {
        DcsLatGemm q{};
        q.A = rows_src; q.a_row_stride = lda; q.a_scale = a_scale; q.Bp = m->L1p; q.bias = m->bias1;
        q.C = w.H1; q.ldc = CI; q.M = (int)n_rows1; q.n_store = CI; q.K = m->K1; q.slice_len = m->lat_slice1;
        q.n_slices = 16; q.n_cb = 4; q.relu = 0; q.a_parts = 1;
        q.nz = split1 ? 4 : 1; q.c_part_stride = n_rows1 * CI;
        DCS_CHECK(dcs_launch_lat_gemm(m->ctx, q, DCS_TAG_CONV1));
    } else
        DCS_CHECK(dcs_launch_gemm_rows(m->ctx, g1, DCS_TAG_CONV1));
    // conv2 + both biases (separate_dsd.py:202-203): output row = position; its A row is kh consecutive H1 rows
    DcsGemm g2{};
    g2.A = w.H1; g2.lda = CI; g2.a_scale = 1.f;
    if (clips) { g2.a_gdiv = 1 << 30; g2.a_gmul = 0; g2.M = n_rows1 - (d.kh2 - 1); }
    else if (shared_frames) { g2.a_gdiv = 1 << 30; g2.a_gmul = 0; g2.M = (n - 1) * tile_row_stride + d.h2; }
    else { g2.a_gdiv = d.h2; g2.a_gmul = tc; g2.M = n * d.h2; }
    g2.B = m->B2; g2.ldb = 64; g2.bias = m->bias2;
    g2.C = w.C2; g2.ldc = CP; g2.c_gdiv = 1 << 30; g2.c_gmul = 0;
    g2.n_cols = 64; g2.n_store = CP; g2.K = d.kh2 * CI; g2.relu = 0; g2.a_vec = 1;
    // conv2 + bottleneck as ONE affine map of the tile's tc rows of H1 (pack_dsd: B2fc): whenever neither runs on the one-batch kernels
    static const bool fold_env = !(getenv("DCS_FOLD_CONV2") && atoi(getenv("DCS_FOLD_CONV2")) == 0);
    const bool fold2 = fold_env && m->B2fc && !(lat & (DCS_LAT_CONV2 | DCS_LAT_FC));
    if (fold2) {
    } else if (lat & DCS_LAT_CONV2) {
        DcsLatGemm q{};   // the A row of position p is kh consecutive H1 rows = kh * CI contiguous floats: one slice per tap
        q.A = w.H1; q.a_row_stride = CI; q.a_scale = 1.f; q.Bp = m->L2p; q.bias = m->bias2;
        q.C = w.C2; q.ldc = CP; q.M = (int)g2.M; q.n_store = CP; q.K = d.kh2 * CI; q.slice_len = CI;
        q.n_slices = d.kh2; q.n_cb = 4; q.relu = 0;
        q.a_parts = split1 ? 4 : 1; q.a_part_stride = n_rows1 * CI;
        q.nz = split2 ? 4 : 1; q.c_part_stride = g2.M * CP;
        DCS_CHECK(dcs_launch_lat_gemm(m->ctx, q, DCS_TAG_CONV2));
    } else
        DCS_CHECK(dcs_launch_gemm_rows(m->ctx, g2, DCS_TAG_CONV2));
    // bottleneck DenseLayer, rectify (separate_dsd.py:206): A row of tile k = h2 consecutive C2 rows
    DcsGemm g3{};
    g3.A = w.C2; g3.lda = (shared_frames ? tile_row_stride : d.h2) * (int64_t)CP; g3.a_gdiv = 1 << 30; g3.a_gmul = 0;
    if (clips) { g3.a_gdiv = (int)n; g3.a_gmul = clip_pitch / tile_row_stride; }
    if (ragged) g3.a_rowmap = rowmap;
    g3.a_scale = 1.f; g3.B = m->Bfc; g3.ldb = m->hid64; g3.bias = m->biasfc;
    g3.C = w.Z; g3.ldc = m->hid64; g3.c_gdiv = 1 << 30; g3.c_gmul = 0;
    g3.M = n_tiles_all; g3.n_cols = m->hid64; g3.n_store = m->hid64; g3.K = d.h2 * CP; g3.relu = 1; g3.a_vec = 1;
    if (fold2) {   // A row of tile k = its tc rows of H1 (the same row index as its first conv2 position)
        g3.A = w.H1; g3.lda = (shared_frames ? tile_row_stride : tc) * (int64_t)CI;
        g3.B = m->B2fc; g3.bias = m->bias2fc; g3.K = tc * CI; g3.Bfrag = m->B2fc_frag;
    }
    if (lat & DCS_LAT_FC) {
        DcsLatGemm q{};   // the A row of tile k is h2 consecutive C2 rows from row k * st: one slice per row
        q.A = w.C2; q.a_row_stride = tile_row_stride * (int64_t)CP; q.a_scale = 1.f; q.Bp = m->Lfcp; q.bias = m->biasfc;
        q.C = w.Z; q.ldc = m->hid64; q.M = (int)(n * n_clips); q.n_store = m->hid64; q.K = d.h2 * CP; q.slice_len = CP;
        q.n_slices = d.h2; q.n_cb = m->hid64 / 16; q.relu = 1;
        if (clips) { q.a_gdiv = (int)n; q.a_gmul = clip_pitch / tile_row_stride; }   // tile (c, k) starts at row c * pitch + k * st
        q.a_parts = split2 ? 4 : 1; q.a_part_stride = g2.M * CP;
        q.nz = split3 ? 4 : 1; q.c_part_stride = n * n_clips * (int64_t)m->hid64;      // split: the rectifier is the consumer's
        DCS_CHECK(dcs_launch_lat_gemm(m->ctx, q, DCS_TAG_FC));
    } else
        DCS_CHECK(dcs_launch_gemm_rows(m->ctx, g3, DCS_TAG_FC));
    // per-source DenseLayers, rectify (separate_dsd.py:209,215,221)
    DcsGemm g4{};
    g4.A = w.Z; g4.lda = m->hid64; g4.a_gdiv = 1 << 30; g4.a_gmul = 0; g4.a_scale = 1.f;
    g4.B = m->Bd; g4.ldb = m->nd64; g4.bias = m->biasd; g4.Bq = m->Bdq;
    g4.C = w.D; g4.ldc = m->nd; g4.c_gdiv = 1 << 30; g4.c_gmul = 0;
    g4.M = n_tiles_all; g4.n_cols = m->nd64; g4.n_store = m->nd; g4.K = m->hid64; g4.relu = 1; g4.a_vec = 1;
    if (lat & DCS_LAT_FC1X) {
        DcsLatGemm q{};
        q.A = w.Z; q.a_row_stride = m->hid64; q.a_scale = 1.f; q.Bp = m->Ldp; q.bias = m->biasd;
        q.C = w.D; q.ldc = m->nd; q.M = (int)(n * n_clips); q.n_store = m->nd; q.K = m->hid64; q.slice_len = 32;
        q.n_slices = 4; q.n_cb = m->nd64 / 16; q.relu = 1;
        q.a_parts = split3 ? 4 : 1; q.a_part_stride = n * n_clips * (int64_t)m->hid64; q.relu_in = split3 ? 1 : 0;
        DCS_CHECK(dcs_launch_lat_gemm(m->ctx, q, DCS_TAG_FC1X));
    } else
        DCS_CHECK(dcs_launch_gemm_rows(m->ctx, g4, DCS_TAG_FC1X));
    // InverseLayer(., l_conv2) (separate_dsd.py:211,217,223)
    if (lat & DCS_LAT_DECONV2)   // f32 G only when a consumer reads it (the one-batch final kernel multiplies the planes)
        return dcs_launch_lat_deconv2(m->ctx, w.D, m->Lw2p, (w.Gs && ((lat & DCS_LAT_FINAL) || clips)) ? nullptr : w.G, w.Gs,
                                      n * n_clips * d.n_fc);
    return dcs_launch_dsd_deconv2(m->ctx, w.D, m->Bw2, m->Bw2s, w.G, n_tiles_all * d.n_fc, d.h2, CP, CI, d.kh2, tc, m->d2_ng, m->d2_gs,
                                  m->d2_gcols, w.Gs, m->Bw2q);
}

// parts: copies of H1 / C2 / Z (the one-batch GEMMs leave their K reduction as 4 partial arrays for the next layer to add)
size_t dsd_scratch_bytes(const dcs_model* m, int64_t n, int64_t rows1, int64_t rows2, bool split = false, int parts = 1) {
    return align256((size_t)parts * rows1 * m->CI * 4) + align256((size_t)parts * rows2 * m->CP * 4) +
           align256((size_t)parts * n * m->hid64 * 4) + align256((size_t)n * m->nd * 4) +
           align256((size_t)n * m->d.n_fc * dsd_g_pitch(m->CI, m->tc) * 4) +
           (split ? align256((size_t)n * m->d.n_fc * dsd_gs_pitch(m->CI, m->tc) * 16) : 0);
}

char* dsd_carve(const dcs_model* m, char* p, int64_t n, int64_t rows1, int64_t rows2, DsdScratch* w, bool split = false,
                int parts = 1) {
    w->H1 = (float*)p; p += align256((size_t)parts * rows1 * m->CI * 4);
    w->C2 = (float*)p; p += align256((size_t)parts * rows2 * m->CP * 4);
    w->Z = (float*)p; p += align256((size_t)parts * n * m->hid64 * 4);
    w->D = (float*)p; p += align256((size_t)n * m->nd * 4);
    w->G = (float*)p; p += align256((size_t)n * m->d.n_fc * dsd_g_pitch(m->CI, m->tc) * 4);
    w->Gs = nullptr;
    if (split) { w->Gs = p; p += align256((size_t)n * m->d.n_fc * dsd_gs_pitch(m->CI, m->tc) * 16); }
    return p;
}

// What every caller of the final launchers fills the same way (dsd_forward_tiles, separate_impl, dcs_separate_stereo and the test
// aid dcs_debug_dsd_stage): weights, the ramp of the last ensure_rise, tile geometry, the bin axis over (channel, bin) and the four
// branches of the stereo model.  ov < 1: unfolded, rows = n * tc rows of the tiles themselves.  Clips, planes and the clip table
// are the caller's.
DsdFinalArgs dsd_final_args(const dcs_model* m, const float* G, const float* mix, int64_t mix_ld, float scale, float* out,
                            int64_t out_src_stride, int64_t out_ld, int64_t n, int64_t rows, int ov, int mask_mode) {
    const int tc = m->tc, st = ov > 0 ? tc - ov : tc;
    const int64_t ld = dcs_round_up(m->F, 4);
    DsdFinalArgs a{};
    a.G = G; a.Bw = m->Bfin; a.ldb = m->Fpad; a.bias = m->bout;
    a.mix = mix; a.mix_ld = mix_ld; a.mix_scale = scale;
    a.out = out; a.out_src_stride = out_src_stride; a.out_ld = out_ld;
    a.rise = m->rise_d; a.n = n; a.rows = rows; a.tc = tc; a.ov = ov > 0 ? ov : 0; a.st = st;
    a.F = (int)((m->C - 1) * ld + m->F); a.CI = m->CI; a.mmax = ov > 0 ? (ov + st - 1) / st + 1 : 1; a.mask_mode = mask_mode;
    a.g_tile_stride = m->d.n_fc * (int64_t)dsd_g_pitch(m->CI, tc);       // compact ragged layout: G of clip c at its tile offset
    a.gs_tile_stride = m->d.n_fc * (int64_t)dsd_gs_pitch(m->CI, tc);
    if (m->arch == DCS_ARCH_DSD_ILD) { a.nbr = 4; a.bias_half = (int)ld; }
    return a;
}

int dsd_forward_tiles(dcs_model* m, const float* tiles, int64_t n, int mask_mode, float* out) {
    const int tc = m->tc, F = m->F;
    const int64_t rows1 = n * tc, rows2 = n * m->d.h2;
    DCS_CHECK(m->ws.ensure(dsd_scratch_bytes(m, n, rows1, rows2)));
    DsdScratch w;
    dsd_carve(m, (char*)m->ws.ptr, n, rows1, rows2, &w);
    const bool vec = (F % 4 == 0) && (((uintptr_t)tiles & 15) == 0);
    DCS_CHECK(dsd_encode(m, tiles, F, vec, 1.f, n, tc, false, w));
    DCS_CHECK(ensure_rise(m, 1));
    const DsdFinalArgs a = dsd_final_args(m, w.G, tiles, F, 1.f, out, n * tc * (int64_t)F, F, n, n * tc, 0, mask_mode);
    return dcs_launch_dsd_final(m->ctx, a, false);
}

// The two-channel sibling: tiles [n][tc][C][ld] in the row layout of dcs_separate_stereo (row = C * ld floats, the K axis pack_dsd
// packed conv1 for: K1 = C * ld, zero weight rows under the pad columns), every tile encoded from its own tc rows; the final
// kernel unfolded and raw, four branches, the bias per (source, channel): out [S][n tc][C ld].
int dsd_forward_tiles_stereo(dcs_model* m, const float* tiles, int64_t n, float* out) {
    const int tc = m->tc;
    const int64_t ld = dcs_round_up(m->F, 4), row = m->C * ld;
    const int64_t rows1 = n * tc, rows2 = n * m->d.h2;
    DCS_CHECK(m->ws.ensure(dsd_scratch_bytes(m, n, rows1, rows2)));
    DsdScratch w;
    dsd_carve(m, (char*)m->ws.ptr, n, rows1, rows2, &w);
    DCS_CHECK(dsd_encode(m, tiles, row, true, 1.f, n, tc, false, w));
    DCS_CHECK(ensure_rise(m, 1));
    const DsdFinalArgs a = dsd_final_args(m, w.G, tiles, row, 1.f, out, n * tc * row, row, n, n * tc, 0, 2);
    return dcs_launch_dsd_final(m->ctx, a, false);
}

}  // namespace

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int dcs_model_create(dcs_ctx* ctx, int arch, int C, int tc, int F, const float* const* params_d,
                                const int64_t* shapes, int nparams, dcs_model** out) {
    if (!ctx || !params_d || !shapes || !out) DCS_FAIL(DCS_EINVAL, "dcs_model_create: null argument");
    if (tc < 2 || F < 1) DCS_FAIL(DCS_EINVAL, "dcs_model_create: bad time_context / feature size");
    if (arch == DCS_ARCH_BACH10_SI_1X1) {
        DCS_ON_DEVICE(ctx->device);
        DcsDeep1x1Net* deep = nullptr;
        DCS_CHECK(dcs_deep1x1_create(ctx, C, tc, F, params_d, shapes, nparams, &deep));
        dcs_model* m = new dcs_model();
        m->ctx = ctx; m->arch = arch; m->C = C; m->tc = tc; m->F = F;
        memset(&m->d, 0, sizeof(m->d));
        m->d.S = 4;
        m->d.n_branch = dcs_deep1x1_out_channels(deep) / C;
        m->deep = deep;
        *out = m;
        return DCS_OK;
    }
    Dims d;
    DCS_CHECK(arch_dims(arch, C, tc, F, &d));
    // expected shapes in get_all_params order
    std::vector<std::vector<int64_t>> expect;
    expect.push_back({d.nf1, C, 1, d.kw1});
    expect.push_back({d.nf1});
    expect.push_back({d.nf1});
    expect.push_back({d.nf2, d.nf1, d.kh2, d.kw2});
    expect.push_back({d.nf2});
    expect.push_back({d.nf2});
    expect.push_back({d.flat, d.hidden});
    expect.push_back({d.hidden});
    for (int i = 0; i < d.n_fc; ++i) {
        expect.push_back({d.hidden, d.flat});
        expect.push_back({d.flat});
    }
    expect.push_back({(int64_t)d.n_branch * C});
    if (nparams != (int)expect.size())
        DCS_FAIL(DCS_ESHAPE, "mismatch: got %d values to set %d parameters", nparams, (int)expect.size());
    std::vector<std::vector<float>> P(nparams);
    DCS_ON_DEVICE(ctx->device);
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
    dcs_model* m = new dcs_model();
    m->ctx = ctx;
    m->arch = arch;
    m->C = C;
    m->tc = tc;
    m->F = F;
    m->d = d;
    int rc;
    if (arch == DCS_ARCH_DSD || arch == DCS_ARCH_DSD_ILD) {
        rc = pack_dsd(m, P);
    } else {
        DcsGenericDims gd{d.nf1, d.kw1, d.sw1, d.w1, d.pool_w, d.wp, d.nf2, d.kh2, d.kw2, d.h2, d.w2,
                          d.flat, d.hidden, d.n_fc, d.n_branch, d.S, {d.branch_fc[0], d.branch_fc[1],
                          d.branch_fc[2], d.branch_fc[3]}};
        rc = dcs_generic_create(ctx, gd, C, tc, F, P, &m->gen);
    }
    if (rc != DCS_OK) {
        dcs_model_destroy(m);
        return rc;
    }
    *out = m;
    return DCS_OK;
}

extern "C" int dcs_model_destroy(dcs_model* m) {
    if (!m) return DCS_OK;
    DCS_ON_DEVICE(m->ctx->device);
    float* ptrs[] = {m->B1, m->bias1, m->B2, m->bias2, m->Bfc, m->biasfc, m->Bd, m->biasd, m->Bw2, m->Bw2s, m->Bfin, m->bout,
                     m->B2fc, m->bias2fc, m->B2fc_frag};
    for (float* p : ptrs) dcs_dev_free(p);
    for (auto& t : m->rise_tabs) dcs_dev_free(t.second);
    float* lat[] = {m->L1p, m->L2p, m->Lfcp, m->Ldp, m->Lw2p};
    for (float* p : lat) dcs_dev_free(p);
    if (m->gen) dcs_generic_destroy(m->gen);
    if (m->deep) dcs_deep1x1_destroy(m->deep);
    for (auto& g : m->graphs)
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
    m->ws.release();
    m->clip_ring.release();
    dcs_dev_free(m->Bpk);
    dcs_dev_free(m->Bw2q);
    dcs_dev_free(m->Bdq);
    delete m;
    return DCS_OK;
}

extern "C" int dcs_model_set_score_semantics(dcs_model* m, int normalise, int mixture) {
    if (!m) DCS_FAIL(DCS_EINVAL, "dcs_model_set_score_semantics: null model");
    if (m->deep) return dcs_deep1x1_set_score_semantics(m->deep, normalise, mixture);
    if (!m->gen) DCS_FAIL(DCS_EUNSUPPORTED, "score semantics belong to the score-informed graphs");
    return dcs_generic_set_score_semantics(m->gen, normalise, mixture);
}

extern "C" int dcs_model_set_conv_precision(dcs_model* m, int f16) {
    if (!m) DCS_FAIL(DCS_EINVAL, "dcs_model_set_conv_precision: null model");
    if (f16 && m->deep) DCS_FAIL(DCS_EUNSUPPORTED, "the deep score-informed graph (build_ca_1x1) runs in f32 only");
    if (f16 && !m->gen)
        DCS_FAIL(DCS_EUNSUPPORTED, "the f16 MFMA conv path exists for the ikala / bach10 / score-informed graphs");
    if (m->gen) return dcs_generic_set_conv_f16(m->gen, f16);
    return DCS_OK;
}

// one clip of at most this many frames takes the one-batch kernels
static int64_t dcs_lat_max_frames() {
    constexpr int64_t v = 1024;   // ~195 tiles: measured crossover ~220 (profiles/r03_c_lat_vs_throughput_by_tiles.txt)
    return v;
}
extern "C" int dcs_model_set_latency_stages(dcs_model* m, int stages) {
    if (!m) DCS_FAIL(DCS_EINVAL, "dcs_model_set_latency_stages: null model");
    if (stages < -1 || stages > DCS_LAT_ALL) DCS_FAIL(DCS_EINVAL, "dcs_model_set_latency_stages: %d", stages);
    if (stages > 0 && !m->lat_ok)
        DCS_FAIL(DCS_EUNSUPPORTED, "the one-batch kernels exist for the DSD graph (50 + 50 filters, time_context 30)");
    m->lat_stages = stages;
    return DCS_OK;
}

extern "C" int dcs_model_num_sources(const dcs_model* m) { return m ? m->d.S : DCS_EINVAL; }
extern "C" int dcs_model_out_channels(const dcs_model* m) { return m ? m->d.n_branch * m->C : DCS_EINVAL; }

// test aids for the convolution kernels of the generic graphs (include/dcs.h)
extern "C" int dcs_debug_conv_stage(dcs_model* m, int stage, dcs_debug_conv_args* args) {
    if (!m || !args) DCS_FAIL(DCS_EINVAL, "dcs_debug_conv_stage: null argument");
    if (!m->gen) DCS_FAIL(DCS_EUNSUPPORTED, "dcs_debug_conv_stage: not a generic-graph model (ikala / bach10 / score-informed)");
    return dcs_generic_debug_conv_stage(m->gen, stage, args);
}

extern "C" int dcs_debug_conv_fold_weights(const dcs_model* m, float* out_h, int64_t n_out, int64_t* rows, int64_t* cols) {
    if (!m) DCS_FAIL(DCS_EINVAL, "dcs_debug_conv_fold_weights: null model");
    if (!m->gen) DCS_FAIL(DCS_EUNSUPPORTED, "dcs_debug_conv_fold_weights: not a generic-graph model");
    return dcs_generic_debug_fold_weights(m->gen, out_h, n_out, rows, cols);
}

extern "C" int dcs_debug_conv_last_kernel(const dcs_model* m, int* codes, int64_t* params) {
    if (!m) DCS_FAIL(DCS_EINVAL, "dcs_debug_conv_last_kernel: null model");
    for (int r = 0; r < DCS_CONV_ROLES; ++r) {
        if (codes) codes[r] = m->ctx->last_conv[r];
        for (int i = 0; i < 3 && params; ++i) params[3 * r + i] = m->ctx->last_conv_param[r][i];
    }
    return DCS_OK;
}

// test aids for the decoder kernels of the DSD graphs (include/dcs.h)
extern "C" int dcs_debug_dsd_last_kernel(const dcs_model* m, int* codes, int64_t* params) {
    if (!m) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_last_kernel: null model");
    for (int r = 0; r < DCS_DSD_ROLES && codes; ++r) codes[r] = m->ctx->last_dsd[r];
    for (int i = 0; i < DCS_DSD_PARAMS && params; ++i) params[i] = m->ctx->last_dsd_param[i];
    return DCS_OK;
}

extern "C" int dcs_debug_dsd_stage(dcs_model* m, int stage, dcs_debug_dsd_args* q) {
    if (!m || !q) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: null argument");
    if (m->arch != DCS_ARCH_DSD && m->arch != DCS_ARCH_DSD_ILD)
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_debug_dsd_stage: not a DSD or stereo (ILD) model");
    if (q->family != DCS_DSD_FAMILY_THROUGHPUT && q->family != DCS_DSD_FAMILY_ONE_BATCH)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: family %d", q->family);
    DCS_ON_DEVICE(m->ctx->device);
    dcs_ctx* ctx = m->ctx;
    for (int r = 0; r < DCS_DSD_ROLES; ++r) ctx->note_dsd(r, 0);
    const bool lat = q->family == DCS_DSD_FAMILY_ONE_BATCH;
    const int tc = m->tc, CI = m->CI, CP = m->CP, nbr = m->d.n_fc;
    const int64_t gp = dsd_g_pitch(CI, tc), gsp = dsd_gs_pitch(CI, tc), lim = (int64_t)1 << 40;
    // a buffer the stage uses: non-null, 16-byte aligned, at least `need` bytes
    auto bad = [](const void* p, int64_t bytes, int64_t need) { return !p || ((uintptr_t)p & 15) || bytes < need; };
    if (stage == DCS_DSD_STAGE_DECONV2) {
        const int64_t n = q->n_items;
        if (n < 1 || n > 0x7fffffff / 8) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: %lld items", (long long)n);
        if (lat && !m->lat_ok) DCS_FAIL(DCS_EUNSUPPORTED, "dcs_debug_dsd_stage: the model has no one-batch kernels");
        if (bad(q->D, q->D_bytes, n * m->d.h2 * CP * 4)) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: D");
        if (lat ? (!q->G && !q->Gs) : !q->G) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: no output buffer");
        if (q->G && bad(q->G, q->G_bytes, n * gp * 4)) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: G");
        if (q->Gs && bad(q->Gs, q->Gs_bytes, n * gsp * 16)) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: Gs");
        const int rc = lat ? dcs_launch_lat_deconv2(ctx, q->D, m->Lw2p, q->G, q->Gs, n)
                           : dcs_launch_dsd_deconv2(ctx, q->D, m->Bw2, m->Bw2s, q->G, n, m->d.h2, CP, CI, m->d.kh2, tc, m->d2_ng,
                                                    m->d2_gs, m->d2_gcols, q->Gs, q->no_bq ? nullptr : m->Bw2q);
        DCS_HIP(hipStreamSynchronize(ctx->stream));
        return rc;
    }
    if (stage != DCS_DSD_STAGE_FINAL) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: stage %d", stage);
    const bool ild = m->arch == DCS_ARCH_DSD_ILD, fold = q->fold != 0;
    const int64_t ld = dcs_round_up(m->F, 4);
    const int Fe = (int)((m->C - 1) * ld + m->F);     // bins of a row: the channels of the stereo model sit side by side
    const int64_t n = q->n, rows = q->rows, n_clips = q->n_clips > 0 ? q->n_clips : 1;
    if (fold && (q->ov < 1 || q->ov >= tc)) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: overlap %d not in [1, %d)", q->ov, tc);
    if (q->mask_mode < 0 || q->mask_mode > 3 || (q->mask_mode == 3 && !ild))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: mask mode %d", q->mask_mode);
    if (n < 1 || rows < 1 || n > 0x7fffffff / tc || rows > 0x7fffffff - 16 || n_clips > 65535 || (!fold && rows != n * tc))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: %lld tiles, %lld rows, %lld clips", (long long)n, (long long)rows, (long long)n_clips);
    if (q->mix_ld < Fe || q->out_ld < Fe || q->mix_ld >= (1 << 24) || q->out_ld >= (1 << 24) || q->out_src_stride < rows * q->out_ld ||
        q->out_src_stride > lim)
        DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: row pitches %lld / %lld, source stride %lld", (long long)q->mix_ld,
                 (long long)q->out_ld, (long long)q->out_src_stride);
    if (n_clips > 1 && (q->g_clip_tiles < 0 || q->g_clip_tiles > lim || q->mix_clip_stride < 0 || q->mix_clip_stride > lim ||
                        q->out_clip_stride < 4 * q->out_src_stride || q->out_clip_stride > lim))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: clip strides");
    if (lat && !fold) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: the one-batch final kernel folds");
    if (q->clip_tab_h && !fold) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: a clip table belongs to the folded form");
    // the last tile and the last mixture float any clip reaches
    int64_t tiles_end = 0, mix_end = 0;
    bool compact = false;
    for (int64_t c = 0; c < n_clips; ++c) {
        int64_t rows_c = rows, n_c = n, mix_off = n_clips > 1 ? c * q->mix_clip_stride : 0, tile_off = n_clips > 1 ? c * q->g_clip_tiles : 0;
        if (q->clip_tab_h) {
            const int64_t* t = q->clip_tab_h + kDcsClipTab * c;
            rows_c = t[1]; n_c = t[2];
            if (rows_c < 1 || rows_c > rows || n_c < 1 || n_c > n) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: clip %lld of the table", (long long)c);
            if (c == 0) compact = t[3] >= 0;
            if ((t[3] >= 0) != compact) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: row offsets of both kinds in the clip table");
            if (compact) {
                if (t[3] > lim || t[4] < 0 || t[4] > lim) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: offsets of clip %lld", (long long)c);
                mix_off = t[3] * q->mix_ld;
                tile_off = t[4];
            }
        }
        if (tile_off + n_c > tiles_end) tiles_end = tile_off + n_c;
        if (mix_off + (rows_c - 1) * q->mix_ld + Fe > mix_end) mix_end = mix_off + (rows_c - 1) * q->mix_ld + Fe;
    }
    const int cbw = dsd_final_cbw(ctx, rows, Fe, n_clips);
    const bool planes = lat || (q->Gs && m->Bpk && fold && !ild && cbw == 2 && q->mask_mode < 2);   // which operand the launcher reads
    if (!planes && bad(q->G, q->G_bytes, tiles_end * nbr * gp * 4)) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: G");
    if (q->Gs && bad(q->Gs, q->Gs_bytes, tiles_end * nbr * gsp * 16)) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: Gs");
    if (bad(q->mix, q->mix_bytes, mix_end * 4)) DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: mixture");
    if (bad(q->out, q->out_bytes, ((n_clips - 1) * q->out_clip_stride + 3 * q->out_src_stride + rows * q->out_ld) * 4))
        DCS_FAIL(DCS_EINVAL, "dcs_debug_dsd_stage: out");
    DCS_CHECK(ensure_rise(m, fold ? q->ov : 1));
    DsdFinalArgs a = dsd_final_args(m, q->G, q->mix, q->mix_ld, q->scale, q->out, q->out_src_stride, q->out_ld, n, rows,
                                    fold ? q->ov : 0, q->mask_mode);
    a.n_clips = (int)n_clips;
    a.g_clip_stride = q->g_clip_tiles * nbr * gp;
    a.mix_clip_stride = q->mix_clip_stride;
    a.out_clip_stride = q->out_clip_stride;
    if (q->Gs) {
        a.Gs = q->Gs;
        a.Bpk = m->Bpk;
        a.gs_clip_stride = q->g_clip_tiles * nbr * gsp;
    }
    int64_t* tab_d = nullptr;
    if (q->clip_tab_h) {
        const size_t bytes = (size_t)n_clips * kDcsClipTab * sizeof(int64_t);
        DCS_HIP(dcs_dev_alloc((void**)&tab_d, bytes, "debug.dsd.clip_tab"));
        if (hipMemcpy(tab_d, q->clip_tab_h, bytes, hipMemcpyHostToDevice) != hipSuccess) {
            dcs_dev_free(tab_d);
            DCS_FAIL(DCS_EHIP, "dcs_debug_dsd_stage: clip table upload");
        }
        a.clip_tab = tab_d;
    }
    const int rc = lat ? dcs_launch_lat_final(ctx, a) : dcs_launch_dsd_final(ctx, a, fold);
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    dcs_dev_free(tab_d);
    if (se != hipSuccess) DCS_FAIL(DCS_EHIP, "dcs_debug_dsd_stage: %s", hipGetErrorString(se));
    return rc;
}

// ONE place decides which one-batch stages (dsd_lat.hip) a call takes: separate_impl (what runs), separate_graphed (whether
// the call is replayed from a hipGraph) and dcs_model_final_kernel (what bench.py prices) all ask here.  plan == nullptr /
// ov < 0: the caller does not know them (dcs_model_final_kernel) -- the frame-size and covering-tile conditions are then
// taken as met, which holds for every configuration the reference ships (frame 1024 / 2048, hop 512, overlap <= 25).
constexpr int kLatDefault = DCS_LAT_ALL;
static unsigned dsd_lat_mask(const dcs_model* m, const dcs_stft* plan, int64_t T, int64_t n_clips, bool ragged, int ov,
                             int eps_mode) {
    if (!m->lat_ok || n_clips != 1 || ragged) return 0;
    if (plan && !dcs_lat_stft_supported(plan)) return 0;
    constexpr int env_mask = -1;   // (stage selection: dcs_model_set_latency_stages)
    const int want = m->lat_stages >= 0 ? m->lat_stages : (env_mask >= 0 ? env_mask : (T <= dcs_lat_max_frames() ? kLatDefault : 0));
    unsigned lat = (unsigned)want & DCS_LAT_ALL;
    const int st = ov >= 0 ? m->tc - ov : 0;
    if ((st > 0 && (ov + st - 1) / st + 1 > dcs_lat_final_max_covers()) || eps_mode > 1)
        lat &= ~(unsigned)DCS_LAT_FINAL;   // more covering tiles than the LDS holds
    if (T >= (1 << 24)) lat = 0;
    return lat;
}

extern "C" int dcs_model_final_kernel(const dcs_model* m, int64_t n_frames, int64_t n_clips, int eps_mode) {
    if (!m || n_frames < 1) return DCS_EINVAL;
    if (m->arch != DCS_ARCH_DSD) return DCS_EUNSUPPORTED;
    if (dsd_lat_mask(m, nullptr, n_frames, n_clips < 1 ? 1 : n_clips, false, -1, eps_mode) & DCS_LAT_FINAL) return 3;
    if (m->Bpk && dsd_final_bf16x3(m->ctx, n_frames, m->F, n_clips, m->CI, eps_mode)) return 2;
    return dsd_final_cbw(m->ctx, n_frames, m->F, n_clips) == 2 ? 1 : 0;
}

static int forward_any(dcs_model* m, const float* tiles_d, int64_t n, int mask_mode, int tie_mode, float* out_d) {
    if (!m || !tiles_d || !out_d) DCS_FAIL(DCS_EINVAL, "dcs_model_forward: null argument");
    if (n < 0) DCS_FAIL(DCS_EINVAL, "dcs_model_forward: negative tile count");
    if (tie_mode != DCS_TIE_ALL && tie_mode != DCS_TIE_FIRST) DCS_FAIL(DCS_EINVAL, "bad tie_mode");
    if (n == 0) return DCS_OK;
    DCS_ON_DEVICE(m->ctx->device);
    if (m->arch == DCS_ARCH_DSD) return dsd_forward_tiles(m, tiles_d, n, mask_mode, out_d);
    if (m->deep) return dcs_deep1x1_forward(m->deep, tiles_d, n, mask_mode, out_d);   // no pooling: tie_mode has no effect
    if (m->arch == DCS_ARCH_DSD_ILD)
        DCS_FAIL(DCS_EUNSUPPORTED, "the stereo (ILD) graph runs through dcs_separate_stereo (frames shared between tiles)");
    return dcs_generic_forward(m->gen, tiles_d, n, mask_mode, tie_mode, out_d);
}

extern "C" int dcs_model_forward_masked(dcs_model* m, const float* tiles_d, int64_t n, int eps_mode, int tie_mode,
                                        float* out_d) {
    if (eps_mode != DCS_EPS_A && eps_mode != DCS_EPS_B) DCS_FAIL(DCS_EINVAL, "bad eps_mode");
    return forward_any(m, tiles_d, n, eps_mode, tie_mode, out_d);
}

extern "C" int dcs_model_forward(dcs_model* m, const float* tiles_d, int64_t n, int tie_mode, float* p_d) {
    return forward_any(m, tiles_d, n, 2, tie_mode, p_d);
}

extern "C" int dcs_model_forward_stereo(dcs_model* m, const float* tiles_d, int64_t n, float* p_d) {
    if (!m || !tiles_d || !p_d) DCS_FAIL(DCS_EINVAL, "dcs_model_forward_stereo: null argument");
    if (m->arch != DCS_ARCH_DSD_ILD) DCS_FAIL(DCS_EINVAL, "dcs_model_forward_stereo: not a stereo (ILD) model");
    if (n < 0 || n > 0x7fffffff / m->tc) DCS_FAIL(DCS_EINVAL, "dcs_model_forward_stereo: %lld tiles", (long long)n);
    if (((uintptr_t)tiles_d & 15) || ((uintptr_t)p_d & 15))
        DCS_FAIL(DCS_EINVAL, "dcs_model_forward_stereo: tiles and p must be 16-byte aligned");
    if (n == 0) return DCS_OK;
    DCS_ON_DEVICE(m->ctx->device);
    return dsd_forward_tiles_stereo(m, tiles_d, n, p_d);
}

// ------------------------------------------------------------------------------------------------ fused path

static int separate_impl(dcs_model* m, dcs_stft* plan, const float* audio_d, int64_t L, int ov, int tiler, float scale,
                         int eps_mode, int tie_mode, float* pcm_d, float* sep_out, float* mag_out, float* phase_out,
                         int64_t ld_out, int64_t* n_tiles_out, int64_t* n_frames_out, int64_t n_clips = 1,
                         int64_t audio_stride = 0, const int64_t* lens_h = nullptr, int64_t pcm_stride = 0,
                         const DcsScoreNotes* notes = nullptr) {
    if (!m || !plan || !audio_d) DCS_FAIL(DCS_EINVAL, "dcs_separate: null argument");
    if (m->deep && !(notes && n_clips == 1 && !lens_h && pcm_d && !sep_out && !mag_out && !phase_out))
        DCS_FAIL(DCS_EUNSUPPORTED, "the deep score-informed graph (build_ca_1x1) separates through dcs_separate_scoreinformed only");
    if (plan->ctx != m->ctx) DCS_FAIL(DCS_EINVAL, "dcs_separate: plan and model belong to different contexts");
    if (plan->frame / 2 + 1 != m->F)
        DCS_FAIL(DCS_EINVAL, "dcs_separate: frameSize %d gives %d bins, network was built for %d", plan->frame,
                 plan->frame / 2 + 1, m->F);
    if (notes) {
        if (!(m->gen || m->deep) || m->C != notes->ninst || n_clips != 1 || lens_h)
            DCS_FAIL(DCS_EINVAL, "dcs_separate_scoreinformed: the model takes %d score channels, the note table has %d", m->C,
                     notes->ninst);
    } else if (m->C != 1)
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_separate: multi-channel (score-informed) input goes through dcs_separate_scoreinformed");
    if (ov < 1 || ov >= m->tc) DCS_FAIL(DCS_EINVAL, "dcs_separate: overlap %d not in [1, %d)", ov, m->tc);
    if (scale == 0.f) DCS_FAIL(DCS_EINVAL, "dcs_separate: scale_factor is zero");
    if (eps_mode != DCS_EPS_A && eps_mode != DCS_EPS_B) DCS_FAIL(DCS_EINVAL, "bad eps_mode");
    if (L < 1) DCS_FAIL(DCS_EINVAL, "dcs_separate: empty signal");
    if (n_clips < 1 || n_clips > 65535) DCS_FAIL(DCS_EINVAL, "dcs_separate_batch: %lld clips", (long long)n_clips);
    if (n_clips > 1 && (m->arch == DCS_ARCH_DSD_ILD || sep_out || mag_out || phase_out || audio_stride < L))
        DCS_FAIL(DCS_EUNSUPPORTED, "dcs_separate_batch: mono graphs, PCM output and clip stride >= length only");
    DCS_ON_DEVICE(m->ctx->device);
    if (m->deep) return dcs_deep1x1_separate(m->deep, plan, audio_d, L, ov, scale, eps_mode, *notes, pcm_d, n_tiles_out, n_frames_out);
    const int tc = m->tc, F = m->F, st = tc - ov, S = m->d.S;
    int64_t T = dcs_frame_count(L, plan->hop);
    int64_t n = dcs_tile_count(T, tc, ov, tiler);
    const int64_t* clip_tab_d = nullptr;
    const int* rowmap_d = nullptr;
    bool ragged_compact = false;
    int64_t rows_sum = 0, tiles_sum = 0;
    if (lens_h) {
        // clips of different lengths in one set of launches: strides and grids are sized by the longest clip (L on
        // entry), every kernel that depends on a clip's own length reads {samples, frames, tiles} from a device table
        if (m->arch == DCS_ARCH_DSD_ILD || m->C != 1 || !pcm_d || pcm_stride < L || n_clips < 2)
            DCS_FAIL(DCS_EUNSUPPORTED, "dcs_separate_ragged: single-channel graphs with PCM output and pcm_stride >= longest clip only");
        // kDcsClipTab entries per clip {samples, frames, tiles, row offset, tile offset, rows} and, behind them, the
        // bottleneck GEMM's tile -> row map (int32).  The DSD graph takes the COMPACT layout (DCS_RAGGED_COMPACT=0: the
        // uniform pitch of round 3): clip c owns rows [row offset, + rows) and tiles [tile offset, + tiles), so the encoder
        // GEMMs, the dense layers and the transposed conv2 run over the SUM of the clips, not n x the longest.
        constexpr bool compact_env = true;
        ragged_compact = compact_env && m->arch == DCS_ARCH_DSD;
        int64_t tiles_bound = 0;
        for (int64_t c = 0; c < n_clips; ++c) {
            const int64_t Lc = lens_h[c];
            if (Lc < 1 || Lc > L) DCS_FAIL(DCS_EINVAL, "dcs_separate_ragged: clip %lld has %lld samples", (long long)c, (long long)Lc);
            tiles_bound += dcs_tile_count(dcs_frame_count(Lc, plan->hop), tc, ov, tiler);
        }
        const size_t tab_n = (size_t)n_clips * kDcsClipTab;
        const size_t tab_bytes = tab_n * sizeof(int64_t) + (ragged_compact ? (size_t)tiles_bound * sizeof(int) : 0);
        void *tab_h = nullptr, *tab_d = nullptr;
        DCS_CHECK(m->clip_ring.begin(tab_bytes, &tab_h, &tab_d));
        int64_t* tab = (int64_t*)tab_h;
        int* rowmap_h = (int*)(tab + tab_n);
        T = 0;
        n = 0;
        for (int64_t c = 0; c < n_clips; ++c) {
            const int64_t Lc = lens_h[c];
            const int64_t Tc = dcs_frame_count(Lc, plan->hop), nc = dcs_tile_count(Tc, tc, ov, tiler);
            if (nc < 1) DCS_FAIL(DCS_EINVAL, "dcs_separate_ragged: clip %lld: %lld frames give no tile", (long long)c, (long long)Tc);
            const int64_t Tcov_c = (nc - 1) * st + tc;
            const int64_t rows_c = dcs_round_up(Tcov_c > Tc ? Tcov_c : Tc, st);
            tab[kDcsClipTab * c] = Lc; tab[kDcsClipTab * c + 1] = Tc; tab[kDcsClipTab * c + 2] = nc;
            tab[kDcsClipTab * c + 3] = ragged_compact ? rows_sum : -1;
            tab[kDcsClipTab * c + 4] = tiles_sum;
            tab[kDcsClipTab * c + 5] = rows_c;
            if (ragged_compact)
                for (int64_t k = 0; k < nc; ++k) rowmap_h[tiles_sum + k] = (int)(rows_sum / st + k);
            rows_sum += rows_c;
            tiles_sum += nc;
            if (n_tiles_out) n_tiles_out[c] = nc;
            if (n_frames_out) n_frames_out[c] = Tc;
            if (Tc > T) T = Tc;
            if (nc > n) n = nc;
        }
        if (rows_sum / st + n > 0x7fffffff) DCS_FAIL(DCS_EUNSUPPORTED, "dcs_separate_ragged: %lld rows", (long long)rows_sum);
        DCS_CHECK(m->clip_ring.commit(tab_bytes, m->ctx->stream));   // no synchronisation: DcsUploadRing
        rowmap_d = ragged_compact ? (const int*)((const int64_t*)tab_d + tab_n) : nullptr;
        clip_tab_d = (const int64_t*)tab_d;
    } else {
        if (n_tiles_out) *n_tiles_out = n;
        if (n_frames_out) *n_frames_out = T;
    }
    if (n < 1)
        DCS_FAIL(DCS_EINVAL, "dcs_separate: %lld frames give no tile (the reference fails in overlapadd_multi)",
                 (long long)T);
    const int64_t Tcov = (n - 1) * st + tc;       // frames covered by the tiles
    // zero rows past T feed the zero-padding tiler; stacked clips get a row pitch that is a multiple of st
    const int64_t Trows = n_clips > 1 ? dcs_round_up(Tcov > T ? Tcov : T, st) : (Tcov > T ? Tcov : T);
    const int64_t ld = dcs_round_up(F, 4);
    // the STFT also fills rows past T of the phase / unit-phasor matrices
    const size_t b_mag = align256((size_t)n_clips * Trows * ld * 4), b_unit = 2 * b_mag, b_ph = phase_out ? b_mag : 0;
    const size_t b_sep = align256((size_t)n_clips * S * T * ld * 4);

    if (m->arch == DCS_ARCH_DSD) {
        const int64_t rows1 = n_clips > 1 ? n_clips * Trows : Tcov;
        const int64_t rows2 = n_clips > 1 ? rows1 : (n - 1) * st + m->d.h2;
        const int64_t n_all = n * n_clips;
        // large launches run the final kernel on the bf16 matrix pipe with three-way split operands (dsd_bf16x3.hip):
        // deconv2 then writes the split planes of G itself
        // one batch per call (the reference's predict_function2 shape): every stage on the short-chain kernels of
        // dsd_lat.hip.  DCS_LAT=<stage bits> / dcs_model_set_latency_stages force a selection (A/B tests, profiling).
        unsigned lat = dsd_lat_mask(m, plan, T, n_clips, clip_tab_d != nullptr, ov, eps_mode);
        const bool split = (lat & DCS_LAT_FINAL) || (m->Bpk && dsd_final_bf16x3(m->ctx, T, F, n_clips, m->CI, eps_mode));
        const size_t b_fr = (lat & DCS_LAT_ISTFT) && pcm_d ? align256(dcs_lat_istft_scratch_bytes(plan, T, S)) : 0;
        const int parts = lat ? 4 : 1;
        DCS_CHECK(m->ws.ensure(b_mag + b_unit + b_ph + b_sep + b_fr + dsd_scratch_bytes(m, n_all, rows1, rows2, split, parts)));
        char* p = (char*)m->ws.ptr;
        float* frames = (float*)p; p += b_fr;
        float* mag = (float*)p; p += b_mag;
        float2* unit = (float2*)p; p += b_unit;
        float* phase = phase_out ? (float*)p : nullptr; p += b_ph;
        float* sep = (float*)p; p += b_sep;
        DsdScratch w;
        dsd_carve(m, p, n_all, rows1, rows2, &w, split, parts);
        if (lat & DCS_LAT_STFT)
            DCS_CHECK(dcs_launch_lat_stft(plan, audio_d, L, mag, phase, unit, ld, Trows, T));
        else
            DCS_CHECK(dcs_launch_stft_forward_f32_clips(plan, audio_d, L, audio_stride, n_clips, mag, phase, unit, ld, Trows, T,
                                                        false, clip_tab_d));
        DCS_CHECK(dsd_encode(m, mag, ld, true, scale, n, st, true, w, n_clips, Trows, lat, ragged_compact ? rows_sum : 0,
                             ragged_compact ? tiles_sum : 0, ragged_compact ? rowmap_d : nullptr));
        DCS_CHECK(ensure_rise(m, ov));
        DsdFinalArgs a = dsd_final_args(m, w.G, mag, ld, scale, sep, T * ld, ld, n, T, ov, eps_mode);
        a.n_clips = (int)n_clips;
        a.g_clip_stride = n * m->d.n_fc * (int64_t)dsd_g_pitch(m->CI, tc);
        a.mix_clip_stride = Trows * ld;
        a.out_clip_stride = (int64_t)S * T * ld;
        a.clip_tab = clip_tab_d;
        if (split) {
            a.Gs = w.Gs;
            a.Bpk = m->Bpk;
            a.gs_clip_stride = n * m->d.n_fc * (int64_t)dsd_gs_pitch(m->CI, tc);
        }
        if (lat & DCS_LAT_FINAL)
            DCS_CHECK(dcs_launch_lat_final(m->ctx, a));
        else
            DCS_CHECK(dcs_launch_dsd_final(m->ctx, a, true));
        if (pcm_d && (lat & DCS_LAT_ISTFT))
            DCS_CHECK(dcs_launch_lat_istft(plan, sep, T * ld, unit, ld, T, S, scale, pcm_d, L, frames));
        else if (pcm_d)
            DCS_CHECK(dcs_launch_stft_inverse_f32_clips(plan, sep, T * ld, unit, Trows * ld, ld, T, S, n_clips, scale, pcm_d, L,
                                                        clip_tab_d, lens_h ? pcm_stride : 0));
        if (sep_out || mag_out || phase_out) {
            for (int s = 0; s < S && sep_out; ++s)
                DCS_HIP(hipMemcpy2DAsync(sep_out + (int64_t)s * T * ld_out, ld_out * 4, sep + (int64_t)s * T * ld, ld * 4,
                                         (size_t)F * 4, (size_t)T, hipMemcpyDeviceToDevice, m->ctx->stream));
            if (mag_out)
                DCS_HIP(hipMemcpy2DAsync(mag_out, ld_out * 4, mag, ld * 4, (size_t)F * 4, (size_t)T,
                                         hipMemcpyDeviceToDevice, m->ctx->stream));
            if (phase_out)
                DCS_HIP(hipMemcpy2DAsync(phase_out, ld_out * 4, phase, ld * 4, (size_t)F * 4, (size_t)T,
                                         hipMemcpyDeviceToDevice, m->ctx->stream));
        }
        return DCS_OK;
    }
    return dcs_generic_separate(m->gen, plan, audio_d, L, ov, tiler, scale, eps_mode, tie_mode, pcm_d, sep_out, mag_out,
                                phase_out, ld_out, &m->ws, n_clips, audio_stride, notes, lens_h, clip_tab_d, pcm_stride);
}

static int separate_graphed(dcs_model* m, dcs_stft* plan, const float* audio_d, int64_t n_samples, int64_t n_clips,
                            int64_t audio_stride, int overlap, int tiler, float scale, int eps_mode, int tie_mode,
                            float* pcm_d, int64_t* n_tiles_out, int64_t* n_frames_out) {
    if (!pcm_d) DCS_FAIL(DCS_EINVAL, "dcs_separate: pcm_d is null");
    if (!m) DCS_FAIL(DCS_EINVAL, "dcs_separate: null model");
    DCS_ON_DEVICE(m->ctx->device);
    // hipGraph replay of the step is OPT-IN since round 6 (DCS_GRAPH=1, read per call): on MI355X / ROCm 7.2 a replayed graph
    // starts its first kernel later than the same launches issued eagerly by a host that keeps ahead of the GPU, at every shape
    // measured -- one 32-tile batch per call 55.2 vs 51.3 us (profiles/r03_*); launch groups of 2 / 4 / 8 / 20 batches 5 / 7 / 2 /
    // 1.5 % slower, 32-batch groups over three streams equal (profiles/r06_ab_graph_replay_vs_eager.txt).  It stays for hosts that
    // cannot keep ahead (many streams per thread).  Replay needs a capturable (non-null) stream, no event timing, and an
    // identical repeat call; the one-batch path is always issued eagerly.
    const char* graph_env = getenv("DCS_GRAPH");
    const bool graphs_on = graph_env && atoi(graph_env) == 1;
    const bool lat_call = plan && m->arch == DCS_ARCH_DSD &&
                          dsd_lat_mask(m, plan, dcs_frame_count(n_samples, plan->hop), n_clips, false, overlap, eps_mode) != 0;
    const bool can_graph = graphs_on && m->ctx->stream != nullptr && m->ctx->timing_mask == 0 && m->arch == DCS_ARCH_DSD &&
                           !lat_call;
    auto eager = [&]() {
        return separate_impl(m, plan, audio_d, n_samples, overlap, tiler, scale, eps_mode, tie_mode, pcm_d, nullptr, nullptr,
                             nullptr, 0, n_tiles_out, n_frames_out, n_clips, audio_stride);
    };
    if (!can_graph) return eager();
    dcs_model::StepKey key;
    key.plan = plan; key.audio = audio_d; key.pcm = pcm_d; key.ws = m->ws.ptr; key.L = n_samples; key.ov = overlap;
    key.tiler = tiler; key.eps = eps_mode; key.tie = tie_mode; key.scale = scale;
    key.n_clips = n_clips; key.audio_stride = audio_stride; key.lat = m->lat_stages;
    const uint64_t now = ++m->step_clock;
    // graphs recorded against a workspace that has since been re-allocated point at freed memory: drop them
    for (auto& g : m->graphs)
        if (g.exec && g.key.ws != m->ws.ptr) {
            (void)hipGraphExecDestroy(g.exec);
            g = dcs_model::StepGraph();
        }
    for (auto& g : m->graphs)
        if (g.exec && g.key == key) {
            g.stamp = now;
            DCS_HIP(hipGraphLaunch(g.exec, m->ctx->stream));
            if (n_tiles_out) *n_tiles_out = g.tiles;
            if (n_frames_out) *n_frames_out = g.frames;
            return DCS_OK;
        }
    int seen_at = -1, seen_lru = 0;
    for (int i = 0; i < dcs_model::kStepGraphs; ++i) {
        if (m->seen_stamp[i] && m->seen[i] == key) seen_at = i;
        if (m->seen_stamp[i] < m->seen_stamp[seen_lru]) seen_lru = i;
    }
    if (seen_at < 0) {
        // first arrival of this call shape: run it eagerly (it sizes every buffer) and remember it
        const int rc = eager();
        if (rc == DCS_OK) {
            key.ws = m->ws.ptr;  // the call may have grown the workspace
            m->seen[seen_lru] = key;
            m->seen_stamp[seen_lru] = now;
        }
        return rc;
    }
    // second identical call: every buffer is allocated and sized, nothing in the path synchronises
    m->seen_stamp[seen_at] = 0;
    hipGraph_t graph = nullptr;
    int64_t nt = 0, nf = 0;
    DCS_CHECK(ensure_rise(m, overlap));   // anything that may allocate or synchronise happens before the capture
    DCS_HIP(hipStreamBeginCapture(m->ctx->stream, hipStreamCaptureModeRelaxed));
    const int rc = separate_impl(m, plan, audio_d, n_samples, overlap, tiler, scale, eps_mode, tie_mode, pcm_d, nullptr,
                                 nullptr, nullptr, 0, &nt, &nf, n_clips, audio_stride);
    const hipError_t ce = hipStreamEndCapture(m->ctx->stream, &graph);
    if (rc != DCS_OK || ce != hipSuccess || !graph || m->ws.ptr != key.ws) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        return eager();   // capture failed (or the captured run reported an error): run this call eagerly; an error
                          // the eager run hits as well is the one the caller gets
    }
    hipGraphExec_t exec = nullptr;
    const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ie != hipSuccess || !exec) {
        (void)hipGetLastError();
        return eager();
    }
    int slot = 0;
    for (int i = 0; i < dcs_model::kStepGraphs; ++i) {
        if (!m->graphs[i].exec) { slot = i; break; }
        if (m->graphs[i].stamp < m->graphs[slot].stamp) slot = i;
    }
    if (m->graphs[slot].exec) {
        // the evicted graph may still be executing on the stream
        DCS_HIP(hipStreamSynchronize(m->ctx->stream));
        (void)hipGraphExecDestroy(m->graphs[slot].exec);
    }
    m->graphs[slot].key = key;
    m->graphs[slot].exec = exec;
    m->graphs[slot].tiles = nt;
    m->graphs[slot].frames = nf;
    m->graphs[slot].stamp = now;
    DCS_HIP(hipGraphLaunch(exec, m->ctx->stream));
    if (n_tiles_out) *n_tiles_out = nt;
    if (n_frames_out) *n_frames_out = nf;
    return DCS_OK;
}

extern "C" int dcs_separate(dcs_model* m, dcs_stft* plan, const float* audio_d, int64_t n_samples, int overlap,
                            int tiler, float scale, int eps_mode, int tie_mode, float* pcm_d, int64_t* n_tiles_out,
                            int64_t* n_frames_out) {
    return separate_graphed(m, plan, audio_d, n_samples, 1, 0, overlap, tiler, scale, eps_mode, tie_mode, pcm_d,
                            n_tiles_out, n_frames_out);
}

extern "C" int dcs_separate_scoreinformed(dcs_model* m, dcs_stft* plan, const float* audio_d, int64_t n_samples,
                                          const double* notes_h, int ninst, int n_notes, int width, int overlap, float scale,
                                          int eps_mode, int tie_mode, float* pcm_d, int64_t* n_tiles_out,
                                          int64_t* n_frames_out) {
    if (!pcm_d || !notes_h) DCS_FAIL(DCS_EINVAL, "dcs_separate_scoreinformed: null argument");
    const DcsScoreNotes notes{notes_h, ninst, n_notes, width};
    return separate_impl(m, plan, audio_d, n_samples, overlap, DCS_TILER_LIBRARY, scale, eps_mode, tie_mode, pcm_d, nullptr,
                         nullptr, nullptr, 0, n_tiles_out, n_frames_out, 1, 0, nullptr, 0, &notes);
}

extern "C" int dcs_separate_batch(dcs_model* m, dcs_stft* plan, const float* audio_d, int64_t n_samples,
                                  int64_t n_clips, int64_t clip_stride, int overlap, int tiler, float scale, int eps_mode,
                                  int tie_mode, float* pcm_d, int64_t* n_tiles_out, int64_t* n_frames_out) {
    return separate_graphed(m, plan, audio_d, n_samples, n_clips, n_clips > 1 ? clip_stride : 0, overlap, tiler, scale,
                            eps_mode, tie_mode, pcm_d, n_tiles_out, n_frames_out);
}

extern "C" int dcs_separate_ragged(dcs_model* m, dcs_stft* plan, const float* audio_d, const int64_t* n_samples_h,
                                   int64_t n_clips, int64_t clip_stride, int overlap, int tiler, float scale, int eps_mode,
                                   int tie_mode, float* pcm_d, int64_t pcm_stride, int64_t* n_tiles_out,
                                   int64_t* n_frames_out) {
    if (!m || !plan || !audio_d || !n_samples_h || !pcm_d) DCS_FAIL(DCS_EINVAL, "dcs_separate_ragged: null argument");
    if (n_clips < 1) DCS_FAIL(DCS_EINVAL, "dcs_separate_ragged: %lld clips", (long long)n_clips);
    int64_t lmax = 0;
    bool same = true;
    for (int64_t c = 0; c < n_clips; ++c) {
        if (n_samples_h[c] > lmax) lmax = n_samples_h[c];
        same = same && n_samples_h[c] == n_samples_h[0];
    }
    if (lmax > clip_stride && n_clips > 1) DCS_FAIL(DCS_EINVAL, "dcs_separate_ragged: a clip is longer than the clip stride");
    if (same && (n_clips == 1 || pcm_stride == lmax)) {   // nothing ragged about it: the equal-length path (graph-replayed)
        int64_t nt = 0, nf = 0;
        const int rc = separate_graphed(m, plan, audio_d, lmax, n_clips, n_clips > 1 ? clip_stride : 0, overlap, tiler, scale,
                                        eps_mode, tie_mode, pcm_d, &nt, &nf);
        for (int64_t c = 0; c < n_clips && rc == DCS_OK; ++c) {
            if (n_tiles_out) n_tiles_out[c] = nt;
            if (n_frames_out) n_frames_out[c] = nf;
        }
        return rc;
    }
    if (n_clips == 1) DCS_FAIL(DCS_EINVAL, "dcs_separate_ragged: one clip with pcm_stride != its length");
    return separate_impl(m, plan, audio_d, lmax, overlap, tiler, scale, eps_mode, tie_mode, pcm_d, nullptr, nullptr, nullptr, 0,
                         n_tiles_out, n_frames_out, n_clips, clip_stride, n_samples_h, pcm_stride);
}

// ------------------------------------------------------------------------------------------------ stereo (ILD) path
// The "Separating" block of examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100.py:291-325 on the DSD kernel family: the two
// channel spectrograms live side by side in rows of 2*ld floats ([frame][channel][ld]), so conv1's K axis and the
// final kernel's bin axis run over (channel, bin); every other stage is the DSD one with 4 independent branches.
extern "C" int dcs_separate_stereo(dcs_model* m, dcs_stft* plan, const float* audio_d, int64_t L, int64_t channel_stride,
                                   int ov, int tiler, float scale, float* pcm_d, float* sep_d, int64_t ld_out,
                                   int64_t* n_tiles_out, int64_t* n_frames_out) {
    if (!m || !plan || !audio_d) DCS_FAIL(DCS_EINVAL, "dcs_separate_stereo: null argument");
    if (m->arch != DCS_ARCH_DSD_ILD) DCS_FAIL(DCS_EINVAL, "dcs_separate_stereo: not a stereo (ILD) model");
    if (plan->ctx != m->ctx) DCS_FAIL(DCS_EINVAL, "dcs_separate_stereo: plan and model belong to different contexts");
    if (plan->frame / 2 + 1 != m->F) DCS_FAIL(DCS_EINVAL, "dcs_separate_stereo: frameSize does not match the network");
    if (ov < 1 || ov >= m->tc) DCS_FAIL(DCS_EINVAL, "dcs_separate_stereo: overlap %d not in [1, %d)", ov, m->tc);
    if (scale == 0.f || L < 1 || channel_stride < L) DCS_FAIL(DCS_EINVAL, "dcs_separate_stereo: bad scale / length / stride");
    if (!pcm_d && !sep_d) DCS_FAIL(DCS_EINVAL, "dcs_separate_stereo: nothing to write");
    if (sep_d && ld_out < m->F) DCS_FAIL(DCS_EINVAL, "dcs_separate_stereo: ld_out < bins");
    DCS_ON_DEVICE(m->ctx->device);
    const int tc = m->tc, F = m->F, st = tc - ov, S = m->d.S, C = m->C;
    const int64_t T = dcs_frame_count(L, plan->hop);
    const int64_t n = dcs_tile_count(T, tc, ov, tiler);
    if (n_tiles_out) *n_tiles_out = n;
    if (n_frames_out) *n_frames_out = T;
    if (n < 1) DCS_FAIL(DCS_EINVAL, "dcs_separate_stereo: %lld frames give no tile", (long long)T);
    const int64_t Tcov = (n - 1) * st + tc, Trows = Tcov > T ? Tcov : T;
    const int64_t ld = dcs_round_up(F, 4), row = C * ld;
    const size_t b_mag = align256((size_t)Trows * row * 4), b_unit = 2 * b_mag, b_sep = align256((size_t)S * T * row * 4);
    const int64_t rows2 = (n - 1) * st + m->d.h2;
    DCS_CHECK(m->ws.ensure(b_mag + b_unit + b_sep + dsd_scratch_bytes(m, n, Tcov, rows2)));
    char* p = (char*)m->ws.ptr;
    float* mag = (float*)p; p += b_mag;
    float2* unit = (float2*)p; p += b_unit;
    float* sep = (float*)p; p += b_sep;
    DsdScratch w;
    dsd_carve(m, p, n, Tcov, rows2, &w);
    // one STFT per channel (compute_transform, transform.py:80-131), rows written [frame][channel]
    DCS_CHECK(dcs_launch_stft_forward_f32_clips(plan, audio_d, L, channel_stride, C, mag, nullptr, unit, ld, Trows, T, true));
    DCS_CHECK(dsd_encode(m, mag, row, true, scale, n, st, true, w));
    DCS_CHECK(ensure_rise(m, ov));
    const DsdFinalArgs a = dsd_final_args(m, w.G, mag, row, scale, sep, T * row, row, n, T, ov, 3);
    DCS_CHECK(dcs_launch_dsd_final(m->ctx, a, true));
    for (int c = 0; c < C; ++c) {
        // per channel the S sources are inverted with that channel's phase (:313-316)
        if (pcm_d)
            DCS_CHECK(dcs_launch_stft_inverse_f32(plan, sep + c * ld, T * row, nullptr, unit + c * ld, row, T, S, scale,
                                                  pcm_d + (int64_t)c * S * L, L));
        for (int s = 0; s < S && sep_d; ++s)
            DCS_HIP(hipMemcpy2DAsync(sep_d + ((int64_t)c * S + s) * T * ld_out, ld_out * 4, sep + (int64_t)s * T * row + c * ld,
                                     row * 4, (size_t)F * 4, (size_t)T, hipMemcpyDeviceToDevice, m->ctx->stream));
    }
    return DCS_OK;
}

extern "C" int dcs_separate_spectra(dcs_model* m, dcs_stft* plan, const float* audio_d, int64_t n_samples, int overlap,
                                    int tiler, float scale, int eps_mode, int tie_mode, float* sep_d, float* mag_d,
                                    float* phase_d, int64_t ld_out) {
    if (m && ld_out < m->F) DCS_FAIL(DCS_EINVAL, "dcs_separate_spectra: ld_out < bins");
    return separate_impl(m, plan, audio_d, n_samples, overlap, tiler, scale, eps_mode, tie_mode, nullptr, sep_d, mag_d,
                         phase_d, ld_out, nullptr, nullptr);
}

// Training of the DSD100 graph (examples/dsd100/trainCNN.py: build_ca :66-130, loss :167-219, adadelta :223) on gfx950.
//
// One step on the ctx stream, no host synchronisation and no float atomics (two runs give bit-identical weights):
//
//   forward   F1 a1b = x . W1 + b1 + b1b              train::gemm_kernel  (saved: a1b)
//             F2 a2b = conv2(a1b) + b2 + b2b          train::gemm_kernel  implicit GEMM over the tc/2 taps (saved: a2b)
//             F3 z = rectify(a2b . Wfc + bfc)          train::gemm_kernel  (saved: z and its pre-activation)
//             F4 d_k = rectify(z . W_k + b_k), k<3     train::gemm_kernel  3 batches (saved: d_k and pre-activations)
//             F5 g_k = conv2^T(d_k)                    train::gemm_kernel  3 batches, implicit GEMM (InverseLayer of conv2)
//             F6 q = conv1^T(g_k) + bo                 train::gemm_kernel  4 batches: channel 3 repeats branch 1 (l_fc14 is dead)
//   loss      dsd_loss_kernel: masks, the six components, dE/dq (relu' with the 0.5 tie) per element, per-workgroup f64 sums
//             train::loss_reduce_kernel: fixed-order sum -> loss and components (f64), sign(E), the output-bias gradient
//   backward  B1 dg_k = dY_k . W1^T     B2 dpre_k = conv2(dg_k) * r'(pre_k)     B3 dprez = (sum_k dpre_k . W_k^T) * r'(prez)
//             B4 da2 = dprez . Wfc^T    B5 da1 = conv2^T(da2)
//   weights   dW1|db1 = [x; dY_k]^T . [da1; g_k]           split-K (K = 4 B tc), fixed-order reduce
//             dW2|db2 = windows of [a1b; dg_k]^T . [da2; d_k]  split-K (K = 4 B h2), fixed-order reduce
//             dWfc|dbfc = a2b^T . dprez,  dW_k|db_k = z^T . dpre_k
//             every bias gradient is the "ones" row of its weight GEMM; b1b / b2b get copies of b1 / b2 (identical in Theano)
//   update    train::adadelta_kernel over the flat [params | grads | accu | delta_accu] buffer
//
// Every GEMM is the 64 x 64 form of the shared template (train_core.h), A loaded K-fastest and B N-fastest; the operands'
// Ax addressing covers row-major, transposed, the implicit-GEMM windows of conv2 and the K-concatenations above without
// copies.
//
// Internal parameter layouts (the flat buffer; dcs_trainer_get / _create convert to and from the .pkl layout):
//   W1 [F][50]: W1i[f][c] = W1[c,0,0,F-1-f]  (flip_filters=True)     W2 [kh][50 c][50 o]: W2i[j][c][o] = W2[o,c,j,0]
//   Wfc [(h,o)][128] and W_k [128][(h,o)], b_k [(h,o)]: the 50 x h2 map in (row h, channel o) order, .pkl order is o*h2+h
// Activations are channels-last: a1b / dg / g / da1 [B][tc][50], a2b / d_k [B][h2][50]; d_k and da2 live in a buffer padded
// by kh-1 zero rows on either side so that conv2^T is a plain implicit GEMM.
#include "train_core.h"

using namespace train;

namespace {

constexpr int kNf = 50, kHidden = 128, kNparams = 15;

// six components, then four output-bias gradient sums; E = vocals + drums + bass - negative - alpha - negative_voc
// (trainCNN.py:217); out7 = (|E|, vocals, bass, drums, negative, alpha, negative_voc)
struct DsdSums {
    static constexpr int kOut = 6, kDbo = 4;
    static __device__ double E(const double* s) { return s[0] + s[2] + s[1] - s[3] - s[4] - s[5]; }
};
constexpr int kLossSums = DsdSums::kOut + DsdSums::kDbo;

struct TLoss {
    const float* q;       // [B][4][tc F] pre-activations of the output layer
    const float* x;       // [B][tc F] inputs
    const float* tgt;     // [B][4][tc F] targets
    const float* rnd;     // [B][tc F] the uniform draw
    float* xy;            // [4][B tc F]: slot 0 <- x, slots 1..3 <- dE/dY_k (branch 1 collects channels 1 and 3)
    double* part;         // [gridDim.x][kLossSums]
    int64_t plane, n;     // tc F, B tc F
    double eps, alpha, beta, beta_voc;
};

// trainCNN.py:176-219 per element, in f64: s_i = p_i + eps r, m_i = s_i / sum_j s_j, sources m_i x for vocals, bass, drums;
// the six squared-error sums; dE/dp_j = x / D (G_j - sum_i m_i G_i) with G the derivative of E in the three sources (G_3 = 0:
// "other" enters only through D); dE/dq = dE/dp r'(q) with rectify's r'(0) = 0.5.
__global__ __launch_bounds__(kThreads) void dsd_loss_kernel(const TLoss a) {
    double acc[kLossSums];
#pragma unroll
    for (int i = 0; i < kLossSums; ++i) acc[i] = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < a.n; e += (int64_t)gridDim.x * kThreads) {
        const int64_t b = e / a.plane, rem = e - b * a.plane;
        const int64_t o = b * 4 * a.plane + rem;
        const double x = a.x[e], er = a.eps * (double)a.rnd[e];
        double q[4], s[4], t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            q[j] = a.q[o + j * a.plane];
            t[j] = a.tgt[o + j * a.plane];
            s[j] = (q[j] > 0.0 ? q[j] : 0.0) + er;
        }
        const double D = s[0] + s[1] + s[2] + s[3];
        const double v = s[0] / D * x, bs = s[1] / D * x, dr = s[2] / D * x;
        const double ev0 = v - t[0], ev1 = v - t[1], ev2 = v - t[2], ev3 = v - t[3];
        const double eb0 = bs - t[0], eb1 = bs - t[1], eb2 = bs - t[2], eb3 = bs - t[3];
        const double ed0 = dr - t[0], ed1 = dr - t[1], ed2 = dr - t[2], ed3 = dr - t[3];
        acc[0] += ev0 * ev0;                                                   // vocals
        acc[1] += eb1 * eb1;                                                   // bass
        acc[2] += ed2 * ed2;                                                   // drums
        acc[3] += a.beta * (eb3 * eb3) + a.beta * (ed3 * ed3);                 // negative
        acc[4] += a.alpha * (ev1 * ev1) + a.alpha * (ev2 * ev2) + a.alpha * (eb0 * eb0) + a.alpha * (eb2 * eb2) +
                  a.alpha * (ed0 * ed0) + a.alpha * (ed1 * ed1);               // alpha
        acc[5] += a.beta_voc * (ev3 * ev3);                                    // negative_voc
        double G[3];
        G[0] = 2.0 * (ev0 - a.alpha * ev1 - a.alpha * ev2 - a.beta_voc * ev3);
        G[1] = 2.0 * (eb1 - a.alpha * eb0 - a.alpha * eb2 - a.beta * eb3);
        G[2] = 2.0 * (ed2 - a.alpha * ed0 - a.alpha * ed1 - a.beta * ed3);
        const double mg = (s[0] * G[0] + s[1] * G[1] + s[2] * G[2]) / D;
        double dq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double gj = (j < 3 ? G[j] : 0.0) - mg;
            const double rd = q[j] > 0.0 ? 1.0 : (q[j] == 0.0 ? 0.5 : 0.0);
            dq[j] = x / D * gj * rd;
            acc[6 + j] += dq[j];
        }
        a.xy[e] = (float)x;
        a.xy[a.n + e] = (float)dq[0];
        a.xy[2 * a.n + e] = (float)(dq[1] + dq[3]);
        a.xy[3 * a.n + e] = (float)dq[2];
    }
    block_sums(acc, a.part);
}

// the .pkl index of element k of the internal section s
struct DsdMap {
    int F, kh, h2;
    __device__ int64_t operator()(int s, int64_t k) const {
        const int64_t map = kNf * (int64_t)h2;
        if (s == 0) {                                     // W1i[f][c] = W1[c][F-1-f]
            const int64_t f = k / kNf, c = k % kNf;
            return c * F + (F - 1 - f);
        } else if (s == 3) {                              // W2i[j][c][o] = W2[o][c][j]
            const int64_t j = k / (kNf * kNf), c = (k / kNf) % kNf, o = k % kNf;
            return (o * kNf + c) * kh + j;
        } else if (s == 6) {                              // Wfc rows (h, o) <- o h2 + h
            const int64_t row = k / kHidden, n = k % kHidden;
            return ((row % kNf) * h2 + row / kNf) * kHidden + n;
        } else if (s == 8 || s == 10 || s == 12) {        // W_k columns (h, o) <- o h2 + h
            const int64_t n = k / map, col = k % map;
            return n * map + (col % kNf) * h2 + col / kNf;
        } else if (s == 9 || s == 11 || s == 13) {
            return (k % kNf) * h2 + k / kNf;
        }
        return k;
    }
};

struct DsdTrainer : dcs_trainer {
    int kh = 0, h2 = 0, hp = 0;
    int64_t R = 0, Rh = 0, map = 0;
    // views into work
    float *xy, *U, *GA, *V, *a2b, *z, *prez, *dprez, *pre, *dpre, *part1, *part2;
    int splits1 = 1, splits2 = 1, kchunk1 = 0, kchunk2 = 0;

    int launch64(const Gemm& g) { return launch(g, T64x64, true, false); }

    void plan(std::vector<std::pair<float**, int64_t>>& parts) override {
        // about 2 workgroups per CU, at most 64 slices
        pick_split(dcs_cdiv(F + 1, 64), 4 * R, &splits1, &kchunk1, 512, 64);
        pick_split(dcs_cdiv(kh * kNf + 1, 64), 4 * Rh, &splits2, &kchunk2, 512, 64);
        const int64_t b = B;
        parts.insert(parts.end(), {{&xy, 4 * RF}, {&U, 4 * R * kNf}, {&GA, 4 * R * kNf}, {&V, 4 * b * hp * kNf},
                                   {&Q, 4 * RF}, {&a2b, b * map}, {&z, b * kHidden}, {&prez, b * kHidden},
                                   {&dprez, b * kHidden}, {&pre, 3 * b * map}, {&dpre, 3 * b * map},
                                   {&part1, (int64_t)splits1 * (F + 1) * kNf},
                                   {&part2, (int64_t)splits2 * (kh * kNf + 1) * kNf}});
    }

    int forward(const float* x) override {
        const int64_t padrow = (int64_t)(kh - 1) * kNf, Vslot = (int64_t)B * hp * kNf;
        const int64_t R50 = R * kNf, plane = (int64_t)tc * F;
        // F1: a1b = x . W1i + b1 + b1b -> U slot 0
        {
            Gemm g = gemm0((int)R, kNf, F);
            g.A = mat((float*)x, 0, ax1(F), ax1(1));
            g.B = mat(param(0), 0, ax1(kNf), ax1(1));
            g.C = mat(U, 0, ax1(kNf), ax1(1));
            g.bias = param(1); g.bias2 = param(2);
            DCS_CHECK(launch64(g));
        }
        // F2: a2b[(b,h)][o] = sum_{k',c} a1b[b][h+k'][c] W2i[kh-1-k'][c][o] + b2 + b2b
        {
            Gemm g = gemm0((int)Rh, kNf, kh * kNf);
            g.A = mat(U, 0, ax2(h2, kNf, (int64_t)tc * kNf), ax1(1));
            g.B = mat(param(3), (int64_t)(kh - 1) * kNf * kNf, ax2(kNf, kNf, -(int64_t)kNf * kNf), ax1(1));
            g.C = mat(a2b, 0, ax1(kNf), ax1(1));
            g.bias = param(4); g.bias2 = param(5);
            DCS_CHECK(launch64(g));
        }
        // F3: z = rectify(a2b . Wfci + bfc), pre-activation saved
        {
            Gemm g = gemm0(B, kHidden, (int)map);
            g.A = mat(a2b, 0, ax1(map), ax1(1));
            g.B = mat(param(6), 0, ax1(kHidden), ax1(1));
            g.C = mat(z, 0, ax1(kHidden), ax1(1));
            g.X = mat(prez, 0, ax1(kHidden), ax1(1));
            g.bias = param(7);
            g.epi = EPI_RELU | EPI_SAVEPRE;
            DCS_CHECK(launch64(g));
        }
        // F4: d_k = rectify(z . W_ki + b_ki) -> V slots 1..3 (padded rows), pre-activations saved
        {
            Gemm g = gemm0(B, (int)map, kHidden);
            g.A = mat(z, 0, ax1(kHidden), ax1(1));
            g.B = mat(param(8), 0, ax1(map), ax1(1));
            g.C = mat(V, padrow, ax1((int64_t)hp * kNf), ax1(1));
            g.X = mat(pre, 0, ax1(map), ax1(1));
            g.bias = param(9);
            g.epi = EPI_RELU | EPI_SAVEPRE;
            g.nbatch = 3;
            for (int k = 0; k < 3; ++k) {
                const int64_t wstep = off[10] - off[8];
                g.boff[k][1] = k * wstep;
                g.boff[k][2] = (k + 1) * Vslot;
                g.boff[k][3] = k * (int64_t)B * map;
                g.boff[k][4] = k * wstep;
            }
            DCS_CHECK(launch64(g));
        }
        // F5: g_k[(b,t)][c] = sum_{j,o} Vpad[b][t+j][o] W2i[j][c][o] -> GA slots 1..3
        {
            Gemm g = gemm0((int)R, kNf, kh * kNf);
            g.A = mat(V, 0, ax2(tc, kNf, (int64_t)hp * kNf), ax1(1));
            g.B = mat(param(3), 0, ax2(kNf, 1, (int64_t)kNf * kNf), ax1(kNf));
            g.C = mat(GA, 0, ax1(kNf), ax1(1));
            g.nbatch = 3;
            for (int k = 0; k < 3; ++k) {
                g.boff[k][0] = (k + 1) * Vslot;
                g.boff[k][2] = (k + 1) * R50;
            }
            DCS_CHECK(launch64(g));
        }
        // F6: q[b][ch][t][f] = sum_c g_br(ch)[(b,t)][c] W1i[f][c] + bo[ch], br = 0, 1, 2, 1
        {
            Gemm g = gemm0((int)R, F, kNf);
            g.A = mat(GA, 0, ax1(kNf), ax1(1));
            g.B = mat(param(0), 0, ax1(1), ax1(kNf));
            g.C = mat(Q, 0, ax2(tc, F, 4 * plane), ax1(1));
            g.bias = param(14);
            g.nbatch = 4;
            const int br[4] = {0, 1, 2, 1};
            for (int ch = 0; ch < 4; ++ch) {
                g.boff[ch][0] = (br[ch] + 1) * R50;
                g.boff[ch][2] = ch * plane;
                g.boff[ch][4] = ch;
            }
            g.bias_cs = 0;
            DCS_CHECK(launch64(g));
        }
        return DCS_OK;
    }

    int loss(const float* x, const float* tgt, double* out7_d) override {
        TLoss a;
        a.q = Q; a.x = x; a.tgt = tgt; a.rnd = rnd; a.xy = xy; a.part = lpart;
        a.plane = (int64_t)tc * F;
        a.n = RF;
        a.eps = hyp[0]; a.alpha = hyp[1]; a.beta = hyp[2]; a.beta_voc = hyp[3];
        const int nblk = (int)std::min<int64_t>(kLossBlocks, dcs_cdiv(a.n, kThreads));
        hipLaunchKernelGGL(dsd_loss_kernel, dim3(nblk), dim3(kThreads), 0, ctx->stream, a);
        DCS_HIP(hipGetLastError());
        return loss_reduce<DsdSums>(nblk, out7_d, grad() + off[14]);
    }

    int backward() override {
        const int64_t padrow = (int64_t)(kh - 1) * kNf, Vslot = (int64_t)B * hp * kNf;
        const int64_t R50 = R * kNf, Bmap = (int64_t)B * map, wstep = off[10] - off[8];
        float* grad = this->grad();
        // B1: dg_k = dY_k . W1i -> U slots 1..3
        {
            Gemm g = gemm0((int)R, kNf, F);
            g.A = mat(xy, 0, ax1(F), ax1(1));
            g.B = mat(param(0), 0, ax1(kNf), ax1(1));
            g.C = mat(U, 0, ax1(kNf), ax1(1));
            g.nbatch = 3;
            for (int k = 0; k < 3; ++k) {
                g.boff[k][0] = (k + 1) * RF;
                g.boff[k][2] = (k + 1) * R50;
            }
            DCS_CHECK(launch64(g));
        }
        // B2: dpre_k = conv2(dg_k) * r'(pre_k)  (the F2 form)
        {
            Gemm g = gemm0((int)Rh, kNf, kh * kNf);
            g.A = mat(U, 0, ax2(h2, kNf, (int64_t)tc * kNf), ax1(1));
            g.B = mat(param(3), (int64_t)(kh - 1) * kNf * kNf, ax2(kNf, kNf, -(int64_t)kNf * kNf), ax1(1));
            g.C = mat(dpre, 0, ax1(kNf), ax1(1));
            g.X = mat(pre, 0, ax1(kNf), ax1(1));
            g.epi = EPI_DRELU;
            g.nbatch = 3;
            for (int k = 0; k < 3; ++k) {
                g.boff[k][0] = (k + 1) * R50;
                g.boff[k][2] = k * Bmap;
                g.boff[k][3] = k * Bmap;
            }
            DCS_CHECK(launch64(g));
        }
        // B3: dprez = (sum_k dpre_k . W_ki^T) * r'(prez): K = 3 map, concatenated over k
        {
            Gemm g = gemm0(B, kHidden, (int)(3 * map));
            g.A = mat(dpre, 0, ax1(map), ax2(map, 1, Bmap));
            g.B = mat(param(8), 0, ax2(map, 1, wstep), ax1(map));
            g.C = mat(dprez, 0, ax1(kHidden), ax1(1));
            g.X = mat(prez, 0, ax1(kHidden), ax1(1));
            g.epi = EPI_DRELU;
            DCS_CHECK(launch64(g));
        }
        // B4: da2 = dprez . Wfci^T -> V slot 0 (padded rows)
        {
            Gemm g = gemm0(B, (int)map, kHidden);
            g.A = mat(dprez, 0, ax1(kHidden), ax1(1));
            g.B = mat(param(6), 0, ax1(1), ax1(kHidden));
            g.C = mat(V, padrow, ax1((int64_t)hp * kNf), ax1(1));
            DCS_CHECK(launch64(g));
        }
        // B5: da1 = conv2^T(da2) -> GA slot 0  (the F5 form)
        {
            Gemm g = gemm0((int)R, kNf, kh * kNf);
            g.A = mat(V, 0, ax2(tc, kNf, (int64_t)hp * kNf), ax1(1));
            g.B = mat(param(3), 0, ax2(kNf, 1, (int64_t)kNf * kNf), ax1(kNf));
            g.C = mat(GA, 0, ax1(kNf), ax1(1));
            DCS_CHECK(launch64(g));
        }
        // dW1 | db1: [x; dY_k]^T [F][4R] . [da1; g_k] [4R][50], ones row over the x block
        {
            Gemm g = gemm0(F + 1, kNf, (int)(4 * R));
            g.A = mat(xy, 0, ax1(1), ax1(F));
            g.B = mat(GA, 0, ax1(kNf), ax1(1));
            g.ones_row = F; g.ones_klim = (int)R;
            g.partial = part1; g.splits = splits1; g.kchunk = kchunk1;
            DCS_CHECK(launch64(g));
        }
        // dW2 | db2: dW2i[(j,c)][o] = sum_{(s,b,h)} U[s][b][h+kh-1-j][c] Vpad[s][b][h+kh-1][o], ones row over the da2 block
        {
            Gemm g = gemm0(kh * kNf + 1, kNf, (int)(4 * Rh));
            g.A = mat(U, (int64_t)(kh - 1) * kNf, ax2(kNf, 1, -(int64_t)kNf), ax2(h2, kNf, (int64_t)tc * kNf));
            g.B = mat(V, padrow, ax2(h2, kNf, (int64_t)hp * kNf), ax1(1));
            g.ones_row = kh * kNf; g.ones_klim = (int)Rh;
            g.partial = part2; g.splits = splits2; g.kchunk = kchunk2;
            DCS_CHECK(launch64(g));
        }
        // dWfc | dbfc = [a2b^T; 1] . dprez -> grads (Wfc and bfc are adjacent)
        {
            Gemm g = gemm0((int)map + 1, kHidden, B);
            g.A = mat(a2b, 0, ax1(1), ax1(map));
            g.B = mat(dprez, 0, ax1(kHidden), ax1(1));
            g.C = mat(grad + off[6], 0, ax1(kHidden), ax1(1));
            g.ones_row = (int)map; g.ones_klim = B;
            g.scale = sign;
            DCS_CHECK(launch64(g));
        }
        // dW_k | db_k = [z^T; 1] . dpre_k -> grads (W_k and b_k are adjacent)
        {
            Gemm g = gemm0(kHidden + 1, (int)map, B);
            g.A = mat(z, 0, ax1(1), ax1(kHidden));
            g.B = mat(dpre, 0, ax1(map), ax1(1));
            g.C = mat(grad + off[8], 0, ax1(map), ax1(1));
            g.ones_row = kHidden; g.ones_klim = B;
            g.scale = sign;
            g.nbatch = 3;
            for (int k = 0; k < 3; ++k) {
                g.boff[k][1] = k * Bmap;
                g.boff[k][2] = k * wstep;
            }
            DCS_CHECK(launch64(g));
        }
        {
            Reduce r;
            memset(&r, 0, sizeof(r));
            r.scale = sign;
            r.part[0] = part1; r.dst[0] = grad + off[0]; r.count[0] = (int64_t)(F + 1) * kNf; r.splits[0] = splits1;
            r.part[1] = part2; r.dst[1] = grad + off[3]; r.count[1] = (int64_t)(kh * kNf + 1) * kNf;
            r.splits[1] = splits2;
            r.N[0] = r.N[1] = kNf;
            r.dup[0] = r.dup[1] = 1;
            DCS_CHECK(reduce(r));
        }
        return DCS_OK;
    }

    int layout(float* flat, float* const* pkl, int to_internal) override {
        return run_layout(flat, pkl, to_internal, DsdMap{F, kh, h2});
    }
};

}  // namespace

int dsd_trainer_new(int time_context, int F, int batch, dcs_trainer** out) {
    if (time_context < 4 || time_context > 64 || time_context % 2 || F < 1 || F > 2049 || batch < 1 || batch > 1024)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: time_context %d (even, 4 .. 64), F %d (1 .. 2049), batch %d (1 .. 1024)",
                 time_context, F, batch);
    DsdTrainer* t = new DsdTrainer();
    const int kh = time_context / 2, h2 = time_context - kh + 1, map = kNf * h2;
    t->kh = kh; t->h2 = h2;
    t->hp = time_context + kh - 1;
    t->R = (int64_t)batch * time_context;
    t->Rh = (int64_t)batch * h2;
    t->map = map;
    t->nsrc = 4;
    t->nparams = kNparams;
    t->loss_sums = kLossSums;
    const int64_t s[kNparams][4] = {{kNf, 1, 1, F}, {kNf, 1, 1, 1}, {kNf, 1, 1, 1}, {kNf, kNf, kh, 1}, {kNf, 1, 1, 1},
                                    {kNf, 1, 1, 1}, {map, kHidden, 1, 1}, {kHidden, 1, 1, 1}, {kHidden, map, 1, 1},
                                    {map, 1, 1, 1}, {kHidden, map, 1, 1}, {map, 1, 1, 1}, {kHidden, map, 1, 1},
                                    {map, 1, 1, 1}, {4, 1, 1, 1}};
    memcpy(t->shapes, s, sizeof(s));
    *out = t;
    return DCS_OK;
}

// The build_ca graph of train_ca.h: its dimensions, work buffer, GEMMs and .pkl layout, written once for every CaDesc.
#include "train_ca.h"

namespace train {

void CaTrainer::shape(const CaDesc& desc, int time_context, int F_, int batch, int nbo) {
    d = desc;
    tc = time_context; F = F_; B = batch;
    w1 = (F - kK1) / d.S1 + 1;
    h2 = tc - d.kh + 1;
    w2 = w1 - d.kw + 1;
    hp = h2 + 2 * (d.kh - 1);
    wp = w2 + 2 * (d.kw - 1);
    K2 = d.kh * d.kw * kC1;
    R1 = (int64_t)B * tc * w1;
    Rh = (int64_t)B * h2 * w2;
    flat = (int64_t)kC2 * h2 * w2;
    const int64_t rowp = (int64_t)wp * kC2;
    Uslot = R1 * kC1;
    Vslot = (int64_t)B * hp * rowp;
    padoff = (int64_t)(d.kh - 1) * rowp + (d.kw - 1) * kC2;
    const int64_t head[8][4] = {{kC1, d.NCH, 1, kK1}, {kC1, 1, 1, 1}, {kC1, 1, 1, 1}, {kC2, kC1, d.kh, d.kw}, {kC2, 1, 1, 1},
                                {kC2, 1, 1, 1}, {flat, kHidden, 1, 1}, {kHidden, 1, 1, 1}};
    memcpy(shapes, head, sizeof(head));
    const int64_t w[4] = {kHidden, flat, 1, 1}, b[4] = {flat, 1, 1, 1}, bo[4] = {nbo, 1, 1, 1};
    nparams = 8;
    for (int k = 0; k < d.NB; ++k) {
        memcpy(shapes[nparams++], w, sizeof(w));
        memcpy(shapes[nparams++], b, sizeof(b));
    }
    memcpy(shapes[nparams++], bo, sizeof(bo));
}

// the K of dW1, of dW2 and of B3, the rows of dWfc, and B flat, which bounds every per-branch offset unit
int CaTrainer::check_index(const char* graph, int nb) const {
    const int64_t most = std::max({(nb + 1) * R1, (nb + 1) * Rh, nb * flat, flat + 1, (int64_t)B * flat});
    if (most >= kBig)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: %s graph: a GEMM index of %lld at time_context %d, F %d, batch %d", graph,
                 (long long)most, tc, F, B);
    return DCS_OK;
}

void CaTrainer::plan(std::vector<std::pair<float**, int64_t>>& parts) {
    // dW1 is one to four 32 x 32 tiles and dW2 a few 128 x 32 tiles over a K of millions (5 B tc w1 = 2.4 M and 5 B h2 w1 =
    // 0.9 M for the Bach10 graph at B = 32, F = 2049): about 2 and 8 workgroups per CU keep the SIMDs busy, up to the
    // graph's cap of slices
    pick_split(dcs_cdiv(d.NCH * kK1 + 1, 32), (d.NB + 1) * R1, &splits1, &kchunk1, d.split1[0], d.split1[1]);
    pick_split(dcs_cdiv(K2 + 1, 128), (d.NB + 1) * Rh, &splits2, &kchunk2, d.split2[0], d.split2[1]);
    pick_split((int64_t)dcs_cdiv(B, 32) * (kHidden / 32), flat, &splits3, &kchunk3, 512, 128);
    pick_split((int64_t)dcs_cdiv(B, 32) * (kHidden / 32), d.NB * flat, &splitsB3, &kchunkB3, 512, 128);
    const int64_t b = B, n1 = d.NB + 1;
    parts.insert(parts.end(), {{&xy, n1 * d.NCH * RF}, {&U, n1 * Uslot}, {&GA, n1 * Uslot}, {&V, n1 * Vslot},
                               {&Q, nsrc * RF}, {&a2b, b * flat}, {&z, b * kHidden}, {&prez, b * kHidden},
                               {&dprez, b * kHidden}, {&pre, d.NB * b * flat}, {&dpre, d.NB * b * flat},
                               {&part1, (int64_t)splits1 * (d.NCH * kK1 + 1) * kC1},
                               {&part2, (int64_t)splits2 * (K2 + 1) * kC2},
                               {&partS, (int64_t)std::max(splits3, splitsB3) * b * kHidden}});
}

// The operands every step shares.  conv1 over a [slot][B][NCH][tc][F] tensor: rows (slot, b, t, w), K = (channel, tap).
// A conv2 window of a channels-last image with rows of `row` floats: kh rows of kw 30 contiguous floats.
namespace {

struct Ops {
    int64_t row1, img1, rowp, imgp, plane, wstep, Bflat;
    Ax c1rows, c1k, win1, winp, map1, mapp, maprow;
    explicit Ops(CaTrainer& t) {
        const CaDesc& d = t.d;
        row1 = (int64_t)t.w1 * kC1; img1 = t.tc * row1; rowp = (int64_t)t.wp * kC2; imgp = t.hp * rowp;
        plane = (int64_t)t.tc * t.F;
        wstep = t.off[10] - t.off[8];
        Bflat = t.B * t.flat;
        c1rows = ax3(t.w1, t.tc, d.S1, t.F, d.NCH * plane);
        c1k = ax2(kK1, 1, plane);
        win1 = ax2(d.kw * kC1, 1, row1);                      // a conv2 window's K in U
        winp = ax2(d.kw * kC2, 1, rowp);                      // and in V
        map1 = ax3(t.w2, t.h2, kC1, row1, img1);              // the map positions (b, h, w) in U
        mapp = ax3(t.w2, t.h2, kC2, rowp, imgp);              // and in V
        maprow = ax2((int64_t)t.w2 * kC2, 1, rowp);           // one image's (h, w, o) in V
    }
};

}  // namespace

int CaTrainer::forward(const float* x) {
    const Ops o(*this);
    const int KW = d.NCH * kK1, NB = d.NB;
    // F1: a1b[(b,t,w)][c] = sum_{ch,j} x[b][ch][t][S1 w + j] W1i[ch][j][c] + b1 + b1b -> U slot 0
    {
        Gemm g = gemm0((int)R1, kC1, KW);
        g.A = mat((float*)x, 0, o.c1rows, o.c1k);
        g.B = mat(param(0), 0, ax1(kC1), ax1(1));
        g.C = mat(U, 0, ax1(kC1), ax1(1));
        g.bias = param(1); g.bias2 = param(2);
        DCS_CHECK(launch(g, T128x32, true, false));
    }
    // F2: a2b[(b,h,w)][o] = sum_{dh,(dw,c)} a1b[b][h+dh][w+dw][c] W2i[dh][dw][c][o] + b2 + b2b
    {
        Gemm g = gemm0((int)Rh, kC2, K2);
        g.A = mat(U, 0, o.map1, o.win1);
        g.B = mat(param(3), 0, ax1(kC2), ax1(1));
        g.C = mat(a2b, 0, ax1(kC2), ax1(1));
        g.bias = param(4); g.bias2 = param(5);
        DCS_CHECK(launch(g, T128x32, true, false));
    }
    // F3: z = rectify(a2b . Wfci + bfc), pre-activation saved: split-K over flat, then the fixed-order sum
    {
        Gemm g = gemm0(B, kHidden, (int)flat);
        g.A = mat(a2b, 0, ax1(flat), ax1(1));
        g.B = mat(param(6), 0, ax1(kHidden), ax1(1));
        g.partial = partS; g.splits = splits3; g.kchunk = kchunk3;
        DCS_CHECK(launch(g, T32x32, true, false));
        DCS_CHECK(finish(partS, splits3, kHidden, param(7), z, prez, EPI_RELU | EPI_SAVEPRE));
    }
    // F4: d_k = rectify(z . W_ki + b_ki) -> V slots 1 .. NB (zero-padded map), pre-activations saved
    {
        Gemm g = gemm0(B, (int)flat, kHidden);
        g.A = mat(z, 0, ax1(kHidden), ax1(1));
        g.B = mat(param(8), 0, ax1(flat), ax1(1));
        g.C = mat(V, padoff, ax1(o.imgp), o.maprow);
        g.X = mat(pre, 0, ax1(flat), ax1(1));
        g.bias = param(9);
        g.epi = EPI_RELU | EPI_SAVEPRE;
        g.nbatch = NB;
        for (int k = 0; k < NB; ++k) {
            g.boff[k][1] = k * o.wstep;
            g.boff[k][2] = (k + 1) * Vslot;
            g.boff[k][3] = k * o.Bflat;
            g.boff[k][4] = k * o.wstep;
        }
        DCS_CHECK(launch(g, rows_tile(B), true, false));
    }
    // F5: g_k[(b,t,w)][c] = sum_{dh,(dw,o)} V[b][t+dh][w+dw][o] W2i[kh-1-dh][kw-1-dw][c][o] -> GA slots 1 .. NB
    {
        Gemm g = gemm0((int)R1, kC1, K2);
        g.A = mat(V, 0, ax3(w1, tc, kC2, o.rowp, o.imgp), o.winp);
        g.B = mat(param(3), (int64_t)(d.kh * d.kw - 1) * kC1 * kC2, ax2(kC2, 1, -(int64_t)kC1 * kC2), ax1(kC2));
        g.C = mat(GA, 0, ax1(kC1), ax1(1));
        g.nbatch = NB;
        for (int k = 0; k < NB; ++k) {
            g.boff[k][0] = (k + 1) * Vslot;
            g.boff[k][2] = (k + 1) * Uslot;
        }
        DCS_CHECK(launch(g, T128x32, true, true));
    }
    return deconv1();
}

int CaTrainer::backward() {
    const Ops o(*this);
    const int KW = d.NCH * kK1, NB = d.NB;
    float* grad = this->grad();
    // B1: dg_k[(b,t,w)][c] = sum_{ch,j} dY_k[b][ch][t][S1 w + j] W1i[ch][j][c] -> U slots 1 .. NB
    {
        Gemm g = gemm0((int)R1, kC1, KW);
        g.A = mat(xy, 0, o.c1rows, o.c1k);
        g.B = mat(param(0), 0, ax1(kC1), ax1(1));
        g.C = mat(U, 0, ax1(kC1), ax1(1));
        g.nbatch = NB;
        for (int k = 0; k < NB; ++k) {
            g.boff[k][0] = (k + 1) * d.NCH * RF;
            g.boff[k][2] = (k + 1) * Uslot;
        }
        DCS_CHECK(launch(g, T128x32, true, false));
    }
    // B2: dpre_k = conv2(dg_k) * r'(pre_k)  (the F2 form)
    {
        Gemm g = gemm0((int)Rh, kC2, K2);
        g.A = mat(U, 0, o.map1, o.win1);
        g.B = mat(param(3), 0, ax1(kC2), ax1(1));
        g.C = mat(dpre, 0, ax1(kC2), ax1(1));
        g.X = mat(pre, 0, ax1(kC2), ax1(1));
        g.epi = EPI_DRELU;
        g.nbatch = NB;
        for (int k = 0; k < NB; ++k) {
            g.boff[k][0] = (k + 1) * Uslot;
            g.boff[k][2] = k * o.Bflat;
            g.boff[k][3] = k * o.Bflat;
        }
        DCS_CHECK(launch(g, T128x32, true, false));
    }
    // B3: dprez = (sum_k dpre_k . W_ki^T) * r'(prez): K = NB flat, concatenated over k, split-K
    {
        Gemm g = gemm0(B, kHidden, (int)(NB * flat));
        g.A = mat(dpre, 0, ax1(flat), ax2(flat, 1, o.Bflat));
        g.B = mat(param(8), 0, ax2(flat, 1, o.wstep), ax1(flat));
        g.partial = partS; g.splits = splitsB3; g.kchunk = kchunkB3;
        DCS_CHECK(launch(g, T32x32, true, true));
        DCS_CHECK(finish(partS, splitsB3, kHidden, nullptr, dprez, prez, EPI_DRELU));
    }
    // B4: da2 = dprez . Wfci^T -> V slot 0 (zero-padded map)
    {
        Gemm g = gemm0(B, (int)flat, kHidden);
        g.A = mat(dprez, 0, ax1(kHidden), ax1(1));
        g.B = mat(param(6), 0, ax1(1), ax1(kHidden));
        g.C = mat(V, padoff, ax1(o.imgp), o.maprow);
        DCS_CHECK(launch(g, rows_tile(B), true, true));
    }
    // B5: da1 = conv2^T(da2) -> GA slot 0  (the F5 form)
    {
        Gemm g = gemm0((int)R1, kC1, K2);
        g.A = mat(V, 0, ax3(w1, tc, kC2, o.rowp, o.imgp), o.winp);
        g.B = mat(param(3), (int64_t)(d.kh * d.kw - 1) * kC1 * kC2, ax2(kC2, 1, -(int64_t)kC1 * kC2), ax1(kC2));
        g.C = mat(GA, 0, ax1(kC1), ax1(1));
        DCS_CHECK(launch(g, T128x32, true, true));
    }
    // dW1 | db1: dW1i[(ch,j)][c] = sum over the (NB + 1) R1 windows (s, b, t, w) of [x; dY_k][s][b][ch][t][S1 w + j]
    // [da1; g_k][s][b][t][w][c], ones row over the da1 block
    {
        Gemm g = gemm0(KW + 1, kC1, (int)((NB + 1) * R1));
        g.A = mat(xy, 0, o.c1k, o.c1rows);
        g.B = mat(GA, 0, ax1(kC1), ax1(1));
        g.ones_row = KW; g.ones_klim = (int)R1;
        g.partial = part1; g.splits = splits1; g.kchunk = kchunk1;
        DCS_CHECK(launch(g, T32x32, false, false));
    }
    // dW2 | db2: dW2i[(dh,dw,c)][o] = sum_{(s,b,h,w)} U[s][b][h+dh][w+dw][c] V[s][b][h+kh-1][w+kw-1][o], ones row over da2
    {
        Gemm g = gemm0(K2 + 1, kC2, (int)((NB + 1) * Rh));
        g.A = mat(U, 0, o.win1, o.map1);
        g.B = mat(V, padoff, o.mapp, ax1(1));
        g.ones_row = K2; g.ones_klim = (int)Rh;
        g.partial = part2; g.splits = splits2; g.kchunk = kchunk2;
        DCS_CHECK(launch(g, T128x32, false, false));
    }
    // dWfc | dbfc = [a2b^T; 1] . dprez -> grads (Wfc and bfc are adjacent)
    {
        Gemm g = gemm0((int)flat + 1, kHidden, B);
        g.A = mat(a2b, 0, ax1(1), ax1(flat));
        g.B = mat(dprez, 0, ax1(kHidden), ax1(1));
        g.C = mat(grad + off[6], 0, ax1(kHidden), ax1(1));
        g.ones_row = (int)flat; g.ones_klim = B;
        g.scale = sign;
        DCS_CHECK(launch(g, T64x64, false, false));
    }
    // dW_k | db_k = [z^T; 1] . dpre_k -> grads (W_k and b_k are adjacent)
    {
        Gemm g = gemm0(kHidden + 1, (int)flat, B);
        g.A = mat(z, 0, ax1(1), ax1(kHidden));
        g.B = mat(dpre, 0, ax1(flat), ax1(1));
        g.C = mat(grad + off[8], 0, ax1(flat), ax1(1));
        g.ones_row = kHidden; g.ones_klim = B;
        g.scale = sign;
        g.nbatch = NB;
        for (int k = 0; k < NB; ++k) {
            g.boff[k][1] = k * o.Bflat;
            g.boff[k][2] = k * o.wstep;
        }
        DCS_CHECK(launch(g, T64x64, false, false));
    }
    {
        Reduce r;
        memset(&r, 0, sizeof(r));
        r.scale = sign;
        r.part[0] = part1; r.dst[0] = grad + off[0]; r.count[0] = (int64_t)(KW + 1) * kC1; r.splits[0] = splits1;
        r.part[1] = part2; r.dst[1] = grad + off[3]; r.count[1] = (int64_t)(K2 + 1) * kC2; r.splits[1] = splits2;
        r.N[0] = r.N[1] = kC1;
        r.dup[0] = r.dup[1] = 1;
        DCS_CHECK(reduce(r));
    }
    return DCS_OK;
}

int CaTrainer::layout(float* flat_d, float* const* pkl, int to_internal) {
    return run_layout(flat_d, pkl, to_internal, CaMap{d.kh, d.kw, h2, w2, d.NCH, d.NB});
}

}  // namespace train

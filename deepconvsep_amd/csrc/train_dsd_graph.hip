// The build_ca graph of train_dsd_graph.h: its dimensions, work buffer, GEMMs and .pkl layout, written once for every DsdDesc.
#include "train_dsd_graph.h"

namespace train {

int DsdGraphTrainer::check_range(const char* graph, int time_context, int F, int batch) {
    if (time_context < 4 || time_context > 64 || time_context % 2 || F < 1 || F > 2049 || batch < 1 || batch > 1024)
        DCS_FAIL(DCS_EINVAL, "dcs_trainer_create: %stime_context %d (even, 4 .. 64), F %d (1 .. 2049), batch %d (1 .. 1024)",
                 graph, time_context, F, batch);
    return DCS_OK;
}

void DsdGraphTrainer::shape(const DsdDesc& desc, int time_context, int F_, int batch) {
    d = desc;
    tc = time_context; F = F_; B = batch;
    kh = tc / 2;
    h2 = tc - kh + 1;
    hp = tc + kh - 1;
    R = (int64_t)B * tc;
    Rh = (int64_t)B * h2;
    map = (int64_t)kNf * h2;
    nsrc = d.nsrc;
    const int64_t H = d.hidden;
    const int64_t head[8][4] = {{kNf, d.NCH, 1, F}, {kNf, 1, 1, 1}, {kNf, 1, 1, 1}, {kNf, kNf, kh, 1}, {kNf, 1, 1, 1},
                                {kNf, 1, 1, 1}, {map, H, 1, 1}, {H, 1, 1, 1}};
    memcpy(shapes, head, sizeof(head));
    const int64_t w[4] = {H, map, 1, 1}, b[4] = {map, 1, 1, 1}, bo[4] = {d.nbo, 1, 1, 1};
    nparams = 8;
    for (int k = 0; k < d.NB; ++k) {
        memcpy(shapes[nparams++], w, sizeof(w));
        memcpy(shapes[nparams++], b, sizeof(b));
    }
    memcpy(shapes[nparams++], bo, sizeof(bo));
}

void DsdGraphTrainer::plan(std::vector<std::pair<float**, int64_t>>& parts) {
    // dW1 and dW2: about 2 workgroups per CU, at most 64 slices; F3 / B3, where split: the build_ca graph's choices
    const int64_t b = B, n1 = d.NB + 1, H = d.hidden;
    pick_split(dcs_cdiv(d.NCH * F + 1, 64), n1 * R, &splits1, &kchunk1, 512, 64);
    pick_split(dcs_cdiv(kh * kNf + 1, 64), n1 * Rh, &splits2, &kchunk2, 512, 64);
    parts.insert(parts.end(), {{&xy, n1 * d.NCH * RF}, {&U, n1 * R * kNf}, {&GA, n1 * R * kNf}, {&V, n1 * b * hp * kNf},
                               {&Q, nsrc * RF}, {&a2b, b * map}, {&z, b * H}, {&prez, b * H}, {&dprez, b * H},
                               {&pre, d.NB * b * map}, {&dpre, d.NB * b * map},
                               {&part1, (int64_t)splits1 * (d.NCH * F + 1) * kNf},
                               {&part2, (int64_t)splits2 * (kh * kNf + 1) * kNf}});
    if (d.split_dense) {
        pick_split((int64_t)dcs_cdiv(B, 32) * (H / 32), map, &splits3, &kchunk3, 512, 128);
        pick_split((int64_t)dcs_cdiv(B, 32) * (H / 32), d.NB * map, &splitsB3, &kchunkB3, 512, 128);
        parts.push_back({&partS, (int64_t)std::max(splits3, splitsB3) * b * H});
    }
}

// The operands every step shares.  conv1 over a [slot][B][NCH][tc][F] tensor: rows (slot, b, t), K = (c, f); with NCH = 1
// these are ax1(F) and ax1(1).  A conv2 window of U is kh rows of 50 contiguous floats, taps descending (W2 is unflipped);
// conv2^T reads the row-padded V with the taps ascending.
namespace {

struct Ops {
    int64_t padrow, Vslot, R50, plane, wstep, Bmap;
    Ax c1rows, c1k, mapU, mapV, w2taps, w2T;
    explicit Ops(DsdGraphTrainer& t) {
        padrow = (int64_t)(t.kh - 1) * kNf;                   // the map's first row in a V image
        Vslot = (int64_t)t.B * t.hp * kNf;
        R50 = t.R * kNf;
        plane = (int64_t)t.tc * t.F;
        wstep = t.off[10] - t.off[8];
        Bmap = t.B * t.map;
        c1rows = ax2(t.tc, t.F, t.d.NCH * plane);
        c1k = ax2(t.F, 1, plane);
        mapU = ax2(t.h2, kNf, (int64_t)t.tc * kNf);           // the map rows (b, h) in U
        mapV = ax2(t.tc, kNf, (int64_t)t.hp * kNf);           // the rows (b, t) of conv2^T in V
        w2taps = ax2(kNf, kNf, -(int64_t)kNf * kNf);          // W2i rows (k', c) from tap kh - 1 down
        w2T = ax2(kNf, 1, (int64_t)kNf * kNf);                // W2i^T rows (j, o)
    }
};

}  // namespace

int DsdGraphTrainer::forward(const float* x) {
    const Ops o(*this);
    const int NB = d.NB, H = d.hidden;
    // F1: a1b[(b,t)][o] = sum_{c,f} x[b][c][t][f] W1i[c F + f][o] + b1 + b1b -> U slot 0
    {
        Gemm g = gemm0((int)R, kNf, d.NCH * F);
        g.A = mat((float*)x, 0, o.c1rows, o.c1k);
        g.B = mat(param(0), 0, ax1(kNf), ax1(1));
        g.C = mat(U, 0, ax1(kNf), ax1(1));
        g.bias = param(1); g.bias2 = param(2);
        DCS_CHECK(launch(g, G_F1));
    }
    // F2: a2b[(b,h)][o] = sum_{k',c} a1b[b][h+k'][c] W2i[kh-1-k'][c][o] + b2 + b2b
    {
        Gemm g = gemm0((int)Rh, kNf, kh * kNf);
        g.A = mat(U, 0, o.mapU, ax1(1));
        g.B = mat(param(3), (int64_t)(kh - 1) * kNf * kNf, o.w2taps, ax1(1));
        g.C = mat(a2b, 0, ax1(kNf), ax1(1));
        g.bias = param(4); g.bias2 = param(5);
        DCS_CHECK(launch(g, G_F2));
    }
    // F3: z = rectify(a2b . Wfci + bfc), pre-activation saved; split: over the map, then the fixed-order sum
    {
        Gemm g = gemm0(B, H, (int)map);
        g.A = mat(a2b, 0, ax1(map), ax1(1));
        g.B = mat(param(6), 0, ax1(H), ax1(1));
        if (d.split_dense) {
            g.partial = partS; g.splits = splits3; g.kchunk = kchunk3;
            DCS_CHECK(launch(g, G_F3));
            DCS_CHECK(finish(partS, splits3, H, param(7), z, prez, EPI_RELU | EPI_SAVEPRE));
        } else {
            g.C = mat(z, 0, ax1(H), ax1(1));
            g.X = mat(prez, 0, ax1(H), ax1(1));
            g.bias = param(7);
            g.epi = EPI_RELU | EPI_SAVEPRE;
            DCS_CHECK(launch(g, G_F3));
        }
    }
    // F4: d_k = rectify(z . W_ki + b_ki) -> V slots 1 .. NB (padded rows), pre-activations saved
    {
        Gemm g = gemm0(B, (int)map, H);
        g.A = mat(z, 0, ax1(H), ax1(1));
        g.B = mat(param(8), 0, ax1(map), ax1(1));
        g.C = mat(V, o.padrow, ax1((int64_t)hp * kNf), ax1(1));
        g.X = mat(pre, 0, ax1(map), ax1(1));
        g.bias = param(9);
        g.epi = EPI_RELU | EPI_SAVEPRE;
        g.nbatch = NB;
        for (int k = 0; k < NB; ++k) {
            g.boff[k][1] = k * o.wstep;
            g.boff[k][2] = (k + 1) * o.Vslot;
            g.boff[k][3] = k * o.Bmap;
            g.boff[k][4] = k * o.wstep;
        }
        DCS_CHECK(launch(g, G_F4));
    }
    // F5: g_k[(b,t)][c] = sum_{j,o} Vpad[b][t+j][o] W2i[j][c][o] -> GA slots 1 .. NB
    {
        Gemm g = gemm0((int)R, kNf, kh * kNf);
        g.A = mat(V, 0, o.mapV, ax1(1));
        g.B = mat(param(3), 0, o.w2T, ax1(kNf));
        g.C = mat(GA, 0, ax1(kNf), ax1(1));
        g.nbatch = NB;
        for (int k = 0; k < NB; ++k) {
            g.boff[k][0] = (k + 1) * o.Vslot;
            g.boff[k][2] = (k + 1) * o.R50;
        }
        DCS_CHECK(launch(g, G_F5));
    }
    // F6: q[b][NCH i + c][t][f] = sum_o g_branch[i][(b,t)][o] W1i[c F + f][o] + bo[NCH i + c]: per input channel c, four
    // batches i
    for (int c = 0; c < d.NCH; ++c) {
        Gemm g = gemm0((int)R, F, kNf);
        g.A = mat(GA, 0, ax1(kNf), ax1(1));
        g.B = mat(param(0), (int64_t)c * F * kNf, ax1(1), ax1(kNf));
        g.C = mat(Q, 0, ax2(tc, F, nsrc * o.plane), ax1(1));
        g.bias = param(bo());
        g.bias_cs = 0;
        g.nbatch = 4;
        for (int i = 0; i < 4; ++i) {
            g.boff[i][0] = (d.branch[i] + 1) * o.R50;
            g.boff[i][2] = (d.NCH * i + c) * o.plane;
            g.boff[i][4] = d.NCH * i + c;
        }
        DCS_CHECK(launch(g, G_F6));
    }
    return DCS_OK;
}

int DsdGraphTrainer::backward() {
    const Ops o(*this);
    const int NB = d.NB, H = d.hidden, K1 = d.NCH * F;
    float* grad = this->grad();
    // B1: dg_k = dY_k . W1i -> U slots 1 .. NB  (the F1 form)
    {
        Gemm g = gemm0((int)R, kNf, K1);
        g.A = mat(xy, 0, o.c1rows, o.c1k);
        g.B = mat(param(0), 0, ax1(kNf), ax1(1));
        g.C = mat(U, 0, ax1(kNf), ax1(1));
        g.nbatch = NB;
        for (int k = 0; k < NB; ++k) {
            g.boff[k][0] = (k + 1) * d.NCH * RF;
            g.boff[k][2] = (k + 1) * o.R50;
        }
        DCS_CHECK(launch(g, G_B1));
    }
    // B2: dpre_k = conv2(dg_k) * r'(pre_k)  (the F2 form)
    {
        Gemm g = gemm0((int)Rh, kNf, kh * kNf);
        g.A = mat(U, 0, o.mapU, ax1(1));
        g.B = mat(param(3), (int64_t)(kh - 1) * kNf * kNf, o.w2taps, ax1(1));
        g.C = mat(dpre, 0, ax1(kNf), ax1(1));
        g.X = mat(pre, 0, ax1(kNf), ax1(1));
        g.epi = EPI_DRELU;
        g.nbatch = NB;
        for (int k = 0; k < NB; ++k) {
            g.boff[k][0] = (k + 1) * o.R50;
            g.boff[k][2] = k * o.Bmap;
            g.boff[k][3] = k * o.Bmap;
        }
        DCS_CHECK(launch(g, G_B2));
    }
    // B3: dprez = (sum_k dpre_k . W_ki^T) * r'(prez): K = NB map, concatenated over k; split: then the fixed-order sum
    {
        Gemm g = gemm0(B, H, (int)(NB * map));
        g.A = mat(dpre, 0, ax1(map), ax2(map, 1, o.Bmap));
        g.B = mat(param(8), 0, ax2(map, 1, o.wstep), ax1(map));
        if (d.split_dense) {
            g.partial = partS; g.splits = splitsB3; g.kchunk = kchunkB3;
            DCS_CHECK(launch(g, G_B3));
            DCS_CHECK(finish(partS, splitsB3, H, nullptr, dprez, prez, EPI_DRELU));
        } else {
            g.C = mat(dprez, 0, ax1(H), ax1(1));
            g.X = mat(prez, 0, ax1(H), ax1(1));
            g.epi = EPI_DRELU;
            DCS_CHECK(launch(g, G_B3));
        }
    }
    // B4: da2 = dprez . Wfci^T -> V slot 0 (padded rows)
    {
        Gemm g = gemm0(B, (int)map, H);
        g.A = mat(dprez, 0, ax1(H), ax1(1));
        g.B = mat(param(6), 0, ax1(1), ax1(H));
        g.C = mat(V, o.padrow, ax1((int64_t)hp * kNf), ax1(1));
        DCS_CHECK(launch(g, G_B4));
    }
    // B5: da1 = conv2^T(da2) -> GA slot 0  (the F5 form)
    {
        Gemm g = gemm0((int)R, kNf, kh * kNf);
        g.A = mat(V, 0, o.mapV, ax1(1));
        g.B = mat(param(3), 0, o.w2T, ax1(kNf));
        g.C = mat(GA, 0, ax1(kNf), ax1(1));
        DCS_CHECK(launch(g, G_B5));
    }
    // dW1 | db1: [x; dY_k]^T [(c,f)][(NB + 1) R] . [da1; g_k] [(NB + 1) R][50], ones row over the x block
    {
        Gemm g = gemm0(K1 + 1, kNf, (int)((NB + 1) * R));
        g.A = mat(xy, 0, o.c1k, o.c1rows);
        g.B = mat(GA, 0, ax1(kNf), ax1(1));
        g.ones_row = K1; g.ones_klim = (int)R;
        g.partial = part1; g.splits = splits1; g.kchunk = kchunk1;
        DCS_CHECK(launch(g, G_DW1));
    }
    // dW2 | db2: dW2i[(j,c)][o] = sum_{(s,b,h)} U[s][b][h+kh-1-j][c] Vpad[s][b][h+kh-1][o], ones row over the da2 block
    {
        Gemm g = gemm0(kh * kNf + 1, kNf, (int)((NB + 1) * Rh));
        g.A = mat(U, (int64_t)(kh - 1) * kNf, ax2(kNf, 1, -(int64_t)kNf), o.mapU);
        g.B = mat(V, o.padrow, ax2(h2, kNf, (int64_t)hp * kNf), ax1(1));
        g.ones_row = kh * kNf; g.ones_klim = (int)Rh;
        g.partial = part2; g.splits = splits2; g.kchunk = kchunk2;
        DCS_CHECK(launch(g, G_DW2));
    }
    // dWfc | dbfc = [a2b^T; 1] . dprez -> grads (Wfc and bfc are adjacent)
    {
        Gemm g = gemm0((int)map + 1, H, B);
        g.A = mat(a2b, 0, ax1(1), ax1(map));
        g.B = mat(dprez, 0, ax1(H), ax1(1));
        g.C = mat(grad + off[6], 0, ax1(H), ax1(1));
        g.ones_row = (int)map; g.ones_klim = B;
        g.scale = sign;
        DCS_CHECK(launch(g, G_DWFC));
    }
    // dW_k | db_k = [z^T; 1] . dpre_k -> grads (W_k and b_k are adjacent)
    {
        Gemm g = gemm0(H + 1, (int)map, B);
        g.A = mat(z, 0, ax1(1), ax1(H));
        g.B = mat(dpre, 0, ax1(map), ax1(1));
        g.C = mat(grad + off[8], 0, ax1(map), ax1(1));
        g.ones_row = H; g.ones_klim = B;
        g.scale = sign;
        g.nbatch = NB;
        for (int k = 0; k < NB; ++k) {
            g.boff[k][1] = k * o.Bmap;
            g.boff[k][2] = k * o.wstep;
        }
        DCS_CHECK(launch(g, G_DWK));
    }
    {
        Reduce r;
        memset(&r, 0, sizeof(r));
        r.scale = sign;
        r.part[0] = part1; r.dst[0] = grad + off[0]; r.count[0] = (int64_t)(K1 + 1) * kNf; r.splits[0] = splits1;
        r.part[1] = part2; r.dst[1] = grad + off[3]; r.count[1] = (int64_t)(kh * kNf + 1) * kNf; r.splits[1] = splits2;
        r.N[0] = r.N[1] = kNf;
        r.dup[0] = r.dup[1] = 1;
        DCS_CHECK(reduce(r));
    }
    return DCS_OK;
}

int DsdGraphTrainer::layout(float* flat, float* const* pkl, int to_internal) {
    return run_layout(flat, pkl, to_internal, DsdMap{F, kh, h2, d.NCH, d.NB, d.hidden});
}

}  // namespace train

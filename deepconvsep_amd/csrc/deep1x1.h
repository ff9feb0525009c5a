// The deep score-informed graph build_ca_1x1 (examples/bach10_scoreinformed/trainCNNrwc.py:66-132): six strided
// convolutions, a 1x1 convolution sliced into per-source branches, and per branch the six InverseLayers back to the input.
// Implemented in deep1x1.hip.
#pragma once
#include <stdint.h>

#include <vector>

#include "dcs_internal.h"
#include "generic.h"

struct DcsDeep1x1Net;

// params: the 22 arrays in get_all_params order (7 x (W, b, BiasLayer.b), final bias); the 1x1 layer may hold 200 k rows and the
// final bias 4 k entries for k = 1 .. 4 (k = 1: the live-only layout).  DCS_ESHAPE on any other shape.
int dcs_deep1x1_create(dcs_ctx* ctx, int C, int tc, int F, const float* const* params_d, const int64_t* shapes, int nparams,
                       DcsDeep1x1Net** out);
void dcs_deep1x1_destroy(DcsDeep1x1Net* g);
int dcs_deep1x1_out_channels(const DcsDeep1x1Net* g);
int dcs_deep1x1_set_score_semantics(DcsDeep1x1Net* g, int normalise, int mixture);
// tiles [n, C, tc, F] -> mask_mode 0/1: out [4, n, tc, F] masked; mask_mode 2: p [out_channels, n, tc, F]
int dcs_deep1x1_forward(DcsDeep1x1Net* g, const float* tiles, int64_t n, int mask_mode, float* out);
// dcs_separate_scoreinformed for this graph: STFT -> score masks -> library tiles -> network -> cross-fade -> iSTFT
int dcs_deep1x1_separate(DcsDeep1x1Net* g, dcs_stft* plan, const float* audio, int64_t L, int ov, float scale, int eps_mode,
                         const DcsScoreNotes& notes, float* pcm, int64_t* n_tiles_out, int64_t* n_frames_out);

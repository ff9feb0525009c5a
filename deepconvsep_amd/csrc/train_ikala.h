// The iKala singing-voice trainer (csrc/train_ikala.hip) behind the dcs_trainer_* entry points of train_dsd.hip, which
// dispatch on the handle's graph.
#pragma once

#include "dcs_internal.h"

struct ik_trainer;

int ik_trainer_create(dcs_ctx* ctx, int time_context, int F, int batch, const float* const* params_d, const int64_t* shapes,
                      int nparams, const float* rand_d, const double* hyper_h, ik_trainer** out);
int ik_trainer_destroy(ik_trainer* t);
int ik_trainer_step(ik_trainer* t, const float* inputs_d, const float* targets_d, int mode, double* out7_d);
int ik_trainer_forward(ik_trainer* t, const float* inputs_d, float* p_d);
int ik_trainer_get(ik_trainer* t, int which, float* const* out_d, int nparams);

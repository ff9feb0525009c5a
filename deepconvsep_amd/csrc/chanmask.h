// The per-bin soft masks shared by dcs_mask_fold_apply (chanmask.hip) and the streaming fold (stream.hip): one definition, so
// that a (tile, frame, bin) masked by either comes out bit for bit the same.  Internal linkage.
#pragma once
#include "dcs_internal.h"

namespace {

// the masks of one tile position: p[s] -> m[s], the expressions and the order of mask_kernel
template <int SA>
__device__ __forceinline__ void soft_masks(float (&p)[SA], int S, int mode) {
    const float eps_r = 5e-19f;
    float den = 0.f;
#pragma unroll
    for (int s = 0; s < SA; ++s)
        if (s < S) {
            if (mode == DCS_EPS_A) p[s] += eps_r;
            den = (s == 0) ? p[s] : den + p[s];
        }
    if (mode == DCS_EPS_B) den += eps_r;
#pragma unroll
    for (int s = 0; s < SA; ++s)
        if (s < S) p[s] = p[s] / den;
}

}  // namespace

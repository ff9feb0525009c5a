// BSS Eval v3 energies on the device (evaluation/bss_eval/bss_eval_sources.m, bss_eval_images.m; the framewise driver of
// evaluation/DSD100_eval_only.m).  Implemented in bsseval.hip; the C entry points dcs_bss_energies / dcs_bss_lagcorr are
// declared in include/dcs.h.  All arithmetic is float64; DESIGN.md "BSS Eval" states the identities and the pivot rule.
#pragma once
#include <stdint.h>

#include "dcs_internal.h"

constexpr int kBssMaxRef = 16;   // reference channels (nsrc_ref * nchan) one problem may hold
constexpr int kBssMaxEst = 16;   // estimate channels (nsrc_est * nchan)

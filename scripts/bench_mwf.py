#!/usr/bin/env python3
"""The multichannel Wiener filter (``dcs_mwf_f32``) on the MI355X at the benchmark's stereo-equivalent shape: F = 1025 bins,
T = 3720 frames, J = 4 sources, niter = 2 (three passes).  Timed warm with HIP events around the launches (``DCS_TAG_MWF``,
one bracket per pass) and around the whole call; the same filter written with torch on the device (einsum +
``torch.linalg.inv`` in complex64, what a user would write today) is timed the same way.  Prints one JSON line.

    python scripts/bench_mwf.py [--frames 3720] [--bins 1025] [--sources 4] [--niter 2] [--reps 20]

Algorithmic bytes per (frame, bin), float32: pass 0 reads 2 phases and 2 J estimates and writes J values of v; a middle pass
reads the mixture (2 magnitudes, 2 phases) and J values of v and writes J values of v; the last pass reads the same and
writes 2 J magnitudes and 2 J phases.  The partial sums over t are not counted: J x 4 float64 per bin and set, at most 32
sets, each read again by every workgroup of its bin block (about 30 MB of mostly cached reads per pass at the default shape).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_TBS = 8.0              # MI355X spec HBM3E bandwidth, not measured here


def pass_bytes(J, T, F, niter):
    """algorithmic bytes of each of the niter + 1 passes"""
    per_bin = [4 * (2 + 2 * J) + 4 * J] + [4 * (4 + J) + 4 * J] * (niter - 1) + [4 * (4 + J) + 4 * 4 * J]
    return [b * T * F for b in per_bin]


def torch_mwf(torch, mag, phase, src, niter, pre_div, eps):
    """the recurrence of include/dcs.h with torch operators, complex64"""
    unit = torch.polar(torch.ones_like(phase), phase)                                    # [2, T, F]
    x = (mag * unit).permute(1, 2, 0)                                                    # [T, F, 2]
    y = ((src / pre_div) * unit[:, None]).permute(1, 2, 3, 0)                            # [J, T, F, 2]
    eye = torch.eye(2, dtype=torch.complex64, device=mag.device)
    C = y[..., :, None] * y[..., None, :].conj()
    v = torch.einsum("jtfii->jtf", C).real * 0.5
    for _ in range(niter):
        R = C.sum(dim=1) / (v.sum(dim=1) + eps)[..., None, None]
        S = v[..., None, None] * R[:, None]
        Cx = S.sum(dim=0) + eps * eye
        W = torch.einsum("jtfab,tfbc->jtfac", S, torch.linalg.inv(Cx))
        y = torch.einsum("jtfab,tfb->jtfa", W, x)
        C = y[..., :, None] * y[..., None, :].conj() + torch.einsum("jtfab,jtfbc->jtfac", eye - W, S)
        v = torch.einsum("jtfii->jtf", C).real * 0.5
    y = y.permute(3, 0, 1, 2)
    return y.abs(), y.angle()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3720)
    ap.add_argument("--bins", type=int, default=1025)
    ap.add_argument("--sources", type=int, default=4)
    ap.add_argument("--niter", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=3)
    a = ap.parse_args()
    if a.niter < 1:
        raise SystemExit("bench_mwf.py: --niter must be at least 1")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mwf.py needs the MI355X")
    import deepconvsep_amd as dcs
    from deepconvsep_amd.runtime import default_context
    from mwf_ref import make_case, mixture, polar

    J, T, F = a.sources, a.frames, a.bins
    mag_h, phase_h, A_h, _ = make_case(J, T, F, seed=0)
    ctx = default_context()
    pre_div = 0.3
    mag, phase = ctx.to_device(mag_h, np.float32), ctx.to_device(phase_h, np.float32)
    src = ctx.to_device(A_h * np.float32(pre_div), np.float32)

    def event_ms(fn, reps):
        ms = []
        with ctx.stream_scope():
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        return out, ms

    hip = lambda: dcs.mwf(ctx, mag, phase, src, a.niter, pre_div=pre_div)
    event_ms(hip, 3)                                                                     # warm: code objects, scratch
    (om, op), call_ms = event_ms(hip, a.reps)
    ctx.timing(["mwf"])
    ctx.timing_reset()
    for _ in range(a.reps):
        hip()
    pass_ms, brackets = ctx.timing_query("mwf")
    ctx.timing(None)

    tor = lambda: torch_mwf(torch, mag, phase, src, a.niter, pre_div, 1e-10)
    event_ms(tor, 1)
    (tm, tp), torch_ms = event_ms(tor, a.torch_reps)

    peak = float(np.abs(mixture(mag_h, phase_h)).max())
    y_hip, y_torch = polar(ctx.to_host(om), ctx.to_host(op)), polar(ctx.to_host(tm), ctx.to_host(tp))
    nbytes = pass_bytes(J, T, F, a.niter)
    call = float(np.median(call_ms))
    print(json.dumps({
        "shape": {"J": J, "T": T, "F": F, "niter": a.niter},
        "hip_call_ms_median": round(call, 4), "hip_call_ms_min": round(min(call_ms), 4),
        "hip_pass_ms_mean": round(pass_ms, 4), "pass_brackets": brackets,
        "algorithmic_MB_per_pass": [round(b / 1e6, 1) for b in nbytes],
        "fraction_of_%g_TBs" % HBM_PEAK_TBS: round(sum(nbytes) / (pass_ms * (a.niter + 1) * 1e-3) / (HBM_PEAK_TBS * 1e12), 4),
        "torch_call_ms_median": round(float(np.median(torch_ms)), 3),
        "torch_over_hip": round(float(np.median(torch_ms)) / call, 1),
        "max_abs_hip_minus_torch_over_peak": float(np.abs(y_hip - y_torch).max() / peak),
    }))


if __name__ == "__main__":
    main()

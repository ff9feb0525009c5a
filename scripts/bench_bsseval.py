#!/usr/bin/env python3
"""BSS Eval on the MI355X: a synthetic DSD100-style evaluation of one 4-minute, 44.1 kHz stereo track with 4 sources --
the two framewise calls of DSD100_eval_only.m (four sources, then vocals / accompaniment), 30 s windows, 15 s hop,
512-tap filters -- timed end to end (host clock around work that ends in a device synchronise) and by stage (HIP events:
lag correlations, Gram assembly + partial Cholesky + energies), plus the float64 CPU restatement (tests/bsseval_ref.py)
on one window.  Prints one JSON line.

    python scripts/bench_bsseval.py [--seconds 240] [--reps 3] [--no-cpu]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

F64_PEAK_TFLOPS = 78.6          # MI355X spec FP64 (vector and matrix), not measured here
TAG_CORR, TAG_CHOL = 15, 16     # DCS_TAG_BSS_CORR / DCS_TAG_BSS_CHOL


def flops(nsrc, nchan, nwin, win, flen):
    """(correlation, factorisation) flop of one framewise call: 2 * R * (2 flen - 1) * (R + M) * win per window; the U^T U
    of the full problem (N = R flen) and of each source's (nchan flen), N^3 / 3 each, and the N^2 * 64 of the D columns"""
    R = M = nsrc * nchan
    corr = 2.0 * R * (2 * flen - 1) * (R + M) * win * nwin
    chol = 0.0
    for n in [R * flen] + [nchan * flen] * nsrc:
        chol += n ** 3 / 3.0 + 2.0 * n * n * 64
    return corr, chol * nwin


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=240)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--flen", type=int, default=512)
    ap.add_argument("--no-cpu", action="store_true", help="skip the CPU restatement's window")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bsseval.py needs the MI355X")
    from deepconvsep_amd import _lib
    from deepconvsep_amd.evaluation import bss_eval, framewise_count
    from deepconvsep_amd.runtime import default_context
    from ctypes import byref, c_double, c_int64

    rate, nchan, nsrc = 44100, 2, 4
    n = a.seconds * rate
    win, hop = 30 * rate, 15 * rate
    rng = np.random.default_rng(0)
    i = rng.standard_normal((n, nchan, nsrc))
    ie = i + 0.3 * np.roll(i, 1, axis=2) + 0.1 * rng.standard_normal(i.shape)
    acc_i, acc_e = i[:, :, :3].sum(axis=2), ie[:, :, :3].sum(axis=2)
    two_i = np.stack([i[:, :, 3], acc_i], axis=2)
    two_e = np.stack([ie[:, :, 3], acc_e], axis=2)
    nwin = framewise_count(n, win, hop)

    ctx = default_context()
    lib = _lib.load()

    def run():
        r4 = bss_eval(ie, i, win, hop, a.flen, ctx=ctx)
        r2 = bss_eval(two_e, two_i, win, hop, a.flen, ctx=ctx)
        return r4, r2

    run()                                                         # warm-up: code objects, scratch
    walls = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r4, r2 = run()
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    # stage times: one more pass with the two tags bracketed by events (brackets per window group)
    _lib.check(lib.dcs_timing_stride(ctx._h, 1))
    _lib.check(lib.dcs_timing_reset(ctx._h))
    _lib.check(lib.dcs_timing_enable(ctx._h, (1 << TAG_CORR) | (1 << TAG_CHOL)))
    run()
    stage = {}
    for name, tag in (("corr", TAG_CORR), ("chol", TAG_CHOL)):
        ms, cnt = c_double(), c_int64()
        _lib.check(lib.dcs_timing_query(ctx._h, tag, byref(ms), byref(cnt)))
        stage[name] = ms.value * cnt.value
    _lib.check(lib.dcs_timing_enable(ctx._h, 0))

    c4, f4 = flops(nsrc, nchan, nwin, win, a.flen)
    c2, f2 = flops(2, nchan, nwin, win, a.flen)
    total_flop = c4 + f4 + c2 + f2
    wall = float(np.median(walls))
    res = {
        "bench": "bsseval_dsd100_track", "seconds": a.seconds, "windows": nwin, "flen": a.flen,
        "track_s": round(wall, 4), "track_s_all": [round(w, 4) for w in walls],
        "corr_ms": round(stage["corr"], 2), "chol_ms": round(stage["chol"], 2),
        "model_tflop": round(total_flop / 1e12, 3),
        "corr_tflops": round((c4 + c2) / (stage["corr"] * 1e-3) / 1e12, 2) if stage["corr"] else None,
        "chol_tflops": round((f4 + f2) / (stage["chol"] * 1e-3) / 1e12, 2) if stage["chol"] else None,
        "frac_f64_peak": round(total_flop / wall / 1e12 / F64_PEAK_TFLOPS, 4),
        "finite_sdr": bool(np.isfinite(r4[0]).all() and np.isfinite(r2[0]).all()),
        "median_sdr_vocals": float(np.median(r4[0][3])),
    }
    if not a.no_cpu:
        import bsseval_ref
        t0 = time.perf_counter()
        bsseval_ref.images_pairs(ie[:win].transpose(2, 0, 1), i[:win].transpose(2, 0, 1), a.flen,
                                 pairs={(j, j) for j in range(nsrc)})
        res["cpu_restatement_window_s"] = round(time.perf_counter() - t0, 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Training-step benchmark of the DSD graph (csrc/train_dsd.hip on csrc/train_dsd_graph.hip) or, with --arch ikala_nopool / bach10 / bach10_si / dsd_ild /
bach10_si_1x1, the iKala graph (csrc/train_ikala.hip) / the Bach10 graph (csrc/train_bach10.hip) / the score-informed Bach10
graph (csrc/train_bach10si.hip; --branches 1: its 11-array layout) / the stereo DSD graph (csrc/train_dsdild.hip on csrc/train_dsd_graph.hip; --ild: its
stage-2 loss) / the deep score-informed graph build_ca_1x1 (csrc/train_deep1x1.hip; its line carries the step's FLOPs from
``Deep1x1Arch.train_flops_per_tile`` and the TFLOP/s they make), all on the shared core csrc/train_core.hip (the iKala and the two Bach10 graphs through the shared build_ca graph
csrc/train_ca.hip), against the same float32 graph, loss and Adadelta written in torch
and run with autograd on the same GPU.  Prints one JSON line per batch size.

    python scripts/bench_train.py [--arch dsd|ikala_nopool|bach10|bach10_si|dsd_ild|bach10_si_1x1] [--ild] [--branches 4|1]
                                  [--batches 32 256] [--steps 50] [--warmup 10] [--feat_size 513]

The Bach10 graphs' working size is --feat_size 2049 (frame size 4096); their lines also carry the floor of a step from its
shapes (``bach10_floor`` / ``bach10si_floor``): the bytes the dense matrices and Adadelta's state must move over the measured
HBM rate, and the convolutions' multiply-adds over the f32 MFMA peak.

ms/step is wall time over --steps steps of train_fn (forward, loss, gradients, Adadelta; no host synchronisation inside
the timed loop) divided by the steps, after --warmup steps; windows/s = batch / (ms/step).  A kernel breakdown comes from
running this script under ``rocprofv3 --kernel-trace --stats -- python scripts/bench_train.py``."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# kernels per train_fn step: 6 forward GEMMs, loss + reduce, 5 backward GEMMs, 4 weight-gradient GEMMs, split-K reduce,
# Adadelta (the graph's launches in csrc/train_dsd_graph.hip, the loss in csrc/train_dsd.hip, Adadelta in csrc/train_core.hip)
LAUNCHES_PER_STEP = 19
# iKala: 7 forward launches (F3 split-K GEMM + its sum), loss + reduce, 6 backward (B3 likewise), 4 weight-gradient GEMMs,
# split-K reduce, Adadelta (the GEMMs in csrc/train_ca.hip, conv1^T and the loss in csrc/train_ikala.hip, Adadelta in
# csrc/train_core.hip)
LAUNCHES_PER_STEP_IKALA = 21
# Bach10: the iKala list with four sources per batched launch (csrc/train_ca.hip, csrc/train_bach10.hip, csrc/train_core.hip)
LAUNCHES_PER_STEP_BACH10 = 21
# score-informed Bach10: the Bach10 list with one decoder slot (csrc/train_ca.hip, csrc/train_bach10si.hip): 7 forward, loss +
# reduce, 6 backward, 4 weight-gradient GEMMs, split-K reduce, Adadelta over the 11 stepped arrays
LAUNCHES_PER_STEP_BACH10SI = 21
# stereo DSD: 8 forward launches (F3 split-K GEMM + its sum, conv1^T once per input channel), loss + reduce (stage 2: the
# per-bin sums and their means before them), 6 backward (B3 split-K + sum), 4 weight-gradient GEMMs, split-K reduce,
# Adadelta (csrc/train_dsd_graph.hip, the loss in csrc/train_dsdild.hip, csrc/train_core.hip)
LAUNCHES_PER_STEP_ILD = {False: 22, True: 24}
# build_ca_1x1 (csrc/train_deep1x1.hip): forward 7 weight packs, the input transpose, 7 convolutions, 6 x (2 transposed
# launches + the code product) = 33; loss + reduce; backward the dq transpose, 6 convolutions, the 1x1 product and its code
# product, 5 x 2 transposed launches, 6 code products = 25; 7 weight-gradient GEMMs and their 7 reduces; Adadelta
LAUNCHES_PER_STEP_DEEP1X1 = 75
# MI355X: HBM3E as a float4 copy reaches it (8 TB/s spec) and the f32 MFMA peak (v_mfma_f32_16x16x4_f32)
HBM_BYTES_PER_S = 6.29e12
F32_MFMA_FLOP_PER_S = 157.3e12


def bach10_floor(B, tc, F):
    """What one Bach10 step cannot go below, from its shapes.  Memory: the five dense matrices are read twice (forward, data
    gradient) and their gradients written once, and Adadelta reads params, grads, accu, delta_accu and writes three of them
    (activations, a few percent at B = 32, are left out).  Compute: conv2 once forward, per source its transpose forward and
    conv2 backward, the transpose once more for da1, and the weight gradient over the 5 blocks; conv1 likewise (2 FLOP per
    multiply-add)."""
    from deepconvsep_amd.arch import ARCHS
    from deepconvsep_amd.training import param_shapes
    d = ARCHS["bach10"].dims(tc, F)
    dense = 5 * d["flat"] * 256 * 4
    state = 4 * sum(int(np.prod(s)) for s in param_shapes("bach10", tc, F))
    nbytes = 3 * dense + 7 * state
    conv2 = 2 * B * d["h2"] * d["w1"] * 30 * 30 * d["kh2"]           # conv2 over its valid rows
    conv2t = 2 * B * tc * d["w1"] * 30 * 30 * d["kh2"]               # conv2^T as an implicit GEMM over the padded map
    conv1 = 2 * B * tc * d["w1"] * 30 * 30
    flop = (1 + 4 + 5) * conv2 + (4 + 1) * conv2t + (1 + 4 + 4 + 5) * conv1 + 3 * 2 * B * 5 * d["flat"] * 256
    return dict(bytes=int(nbytes), memory_ms=round(nbytes / HBM_BYTES_PER_S * 1e3, 3), flop=int(flop),
                compute_ms=round(flop / F32_MFMA_FLOP_PER_S * 1e3, 3))


def bach10si_floor(B, tc, F):
    """The same for one score-informed step (either layout: the dead arrays of the 17-array one are outside the step).
    Memory: the two dense matrices Wfc and W_11 read twice and their gradients written once, Adadelta over the 11 stepped
    arrays.  Compute: conv2 forward, backward and its weight gradient over 2 blocks; conv2^T forward and for da1; conv1 with
    K = 4 channels x 30 taps forward, backward, transposed and its weight gradient over 2 blocks."""
    from deepconvsep_amd.arch import ARCHS
    d = ARCHS["bach10_si1"].dims(tc, F)
    dense = 2 * d["flat"] * 256 * 4
    state = 4 * sum(int(np.prod(s)) for s in ARCHS["bach10_si1"].param_shapes(tc, F))
    nbytes = 3 * dense + 7 * state
    conv2 = 2 * B * d["h2"] * d["w1"] * 30 * 30 * d["kh2"]
    conv2t = 2 * B * tc * d["w1"] * 30 * 30 * d["kh2"]
    conv1 = 2 * B * tc * d["w1"] * 30 * 4 * 30
    flop = (1 + 1 + 2) * conv2 + (1 + 1) * conv2t + (1 + 1 + 1 + 2) * conv1 + 3 * 2 * B * 2 * d["flat"] * 256
    return dict(bytes=int(nbytes), memory_ms=round(nbytes / HBM_BYTES_PER_S * 1e3, 3), flop=int(flop),
                compute_ms=round(flop / F32_MFMA_FLOP_PER_S * 1e3, 3))


def _si_inputs(B, tc, F):
    rs = np.random.RandomState(0)
    x = (0.3 * rs.uniform(0, 0.25, size=(B, 4, tc, F))).astype(np.float32)
    y = (0.1 * rs.uniform(size=(B, 4, tc, F))).astype(np.float32)
    r = rs.uniform(size=(B, 1, tc, F)).astype(np.float32)
    return x, y, r


def bench_hip_si(B, tc, F, steps, warmup, branches):
    import torch
    from deepconvsep_amd.score_training import ScoreTrainer, glorot_init
    x, y, r = _si_inputs(B, tc, F)
    t = ScoreTrainer(params=glorot_init(tc, F, 0, branches), branches=branches, batch_size=B, time_context=tc, feat_size=F,
                     rand=r)
    x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for _ in range(warmup):
        t.run(x, y, 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        t.run(x, y, 2)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    t.close()
    return ms


def bench_torch_si(B, tc, F, steps, warmup, branches):
    """float32 autograd of the same layout: with 17 arrays torch computes the three dead branches forward (autograd prunes
    their backward), as the reference's compiled function would."""
    import torch
    import train_si_ref as ref
    from deepconvsep_amd.score_training import glorot_init
    x, y, r = (torch.from_numpy(a).cuda() for a in _si_inputs(B, tc, F))
    P = [torch.from_numpy(p).cuda().requires_grad_(True) for p in glorot_init(tc, F, 0, branches)]
    opt = torch.optim.Adadelta(P, lr=1.0, rho=0.95, eps=1e-6)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = ref.components(ref.forward(P, x), x, y, r)[0]
        loss.backward()
        opt.step()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def bench_hip_deep(B, tc, F, steps, warmup, branches):
    import torch
    from deepconvsep_amd.score_training import ScoreTrainer
    from deepconvsep_amd.synth import synth_params
    x, y, r = _si_inputs(B, tc, F)
    params = synth_params('bach10_si_1x1', tc, F, seed=0)
    if branches < 4:
        import train_deep1x1_ref as ref
        params = ref.live(params)
    t = ScoreTrainer(params=params, branches=branches, batch_size=B, time_context=tc, feat_size=F, rand=r, function='build_ca_1x1')
    x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for _ in range(warmup):
        t.run(x, y, 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        t.run(x, y, 2)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    t.close()
    return ms


def bench_torch_deep(B, tc, F, steps, warmup, branches):
    """float32 autograd of tests/train_deep1x1_ref.graph (the live branch; the dead rows of the 1x1 layer forward only)."""
    import torch
    import train_deep1x1_ref as ref
    import train_ref
    from deepconvsep_amd.synth import synth_params
    x, y, r = (torch.from_numpy(a).cuda() for a in _si_inputs(B, tc, F))
    params = synth_params('bach10_si_1x1', tc, F, seed=0)
    P = [torch.from_numpy(np.asarray(p, np.float32)).cuda().requires_grad_(True) for p in (params if branches == 4 else ref.live(params))]
    opt = torch.optim.Adadelta(P, lr=1.0, rho=0.95, eps=1e-6)

    def step():
        opt.zero_grad(set_to_none=True)
        q, _, _ = ref.graph(P, x)
        loss = ref.components(train_ref.rectify(q), x, y, r)[0]
        loss.backward()
        opt.step()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def _ild_inputs(B, tc, F):
    rs = np.random.RandomState(0)
    x = (0.3 * rs.uniform(size=(B, 2, tc, F))).astype(np.float32)
    y = (0.1 * rs.uniform(size=(B, 8, tc, F))).astype(np.float32)
    r = (0.1 * rs.randn(2, B, 4, tc, F)).astype(np.float32)
    return x, y, r


def bench_hip_ild(B, tc, F, steps, warmup, ild):
    import torch
    from deepconvsep_amd.stereo_training import StereoTrainer, glorot_init
    x, y, r = _ild_inputs(B, tc, F)
    t = StereoTrainer(params=glorot_init(tc, F, 0), batch_size=B, time_context=tc, feat_size=F, rand=r)
    x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for _ in range(warmup):
        t.run(x, y, 2, ild)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        t.run(x, y, 2, ild)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def bench_torch_ild(B, tc, F, steps, warmup, ild):
    import torch
    import train_ild_ref as ref
    from deepconvsep_amd.stereo_training import glorot_init
    x, y, r = (torch.from_numpy(a).cuda() for a in _ild_inputs(B, tc, F))
    P = [torch.from_numpy(p).cuda().requires_grad_(True) for p in glorot_init(tc, F, 0)]
    opt = torch.optim.Adadelta(P, lr=1.0, rho=0.95, eps=1e-6)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = ref.components(ref.forward(P, x), x, y, r, stage=2 if ild else 1)[0]
        loss.backward()
        opt.step()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def bench_hip(B, tc, F, steps, warmup, arch="dsd"):
    import torch
    from deepconvsep_amd.training import Trainer, glorot_init, n_sources
    rs = np.random.RandomState(0)
    t = Trainer(arch=arch, params=glorot_init(arch, tc, F, 0), batch_size=B, time_context=tc, feat_size=F)
    x = torch.from_numpy((0.3 * rs.uniform(size=(B, 1, tc, F))).astype(np.float32)).cuda()
    y = torch.from_numpy((0.1 * rs.uniform(size=(B, n_sources(arch), tc, F))).astype(np.float32)).cuda()
    for _ in range(warmup):
        t.run(x, y, 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        t.run(x, y, 2)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def bench_torch(B, tc, F, steps, warmup, arch="dsd"):
    import torch
    import train_bach10_ref
    import train_ikala_ref
    import train_ref
    from deepconvsep_amd.training import glorot_init, n_sources
    ref = {"ikala_nopool": train_ikala_ref, "bach10": train_bach10_ref}.get(arch, train_ref)
    rs = np.random.RandomState(0)
    P = [torch.from_numpy(p).cuda().requires_grad_(True) for p in glorot_init(arch, tc, F, 0)]
    x = torch.from_numpy((0.3 * rs.uniform(size=(B, 1, tc, F))).astype(np.float32)).cuda()
    y = torch.from_numpy((0.1 * rs.uniform(size=(B, n_sources(arch), tc, F))).astype(np.float32)).cuda()
    r = torch.from_numpy(rs.uniform(size=(B, 1, tc, F)).astype(np.float32)).cuda()
    opt = torch.optim.Adadelta(P, lr=1.0, rho=0.95, eps=1e-6)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = ref.components(ref.forward(P, x), x, y, r)[0]
        loss.backward()
        opt.step()
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", choices=("dsd", "ikala_nopool", "bach10", "bach10_si", "dsd_ild", "bach10_si_1x1"),
                    default="dsd")
    ap.add_argument("--branches", type=int, choices=(4, 1), default=4, help="bach10_si: the 17- or the 11-array layout")
    ap.add_argument("--ild", action="store_true", help="dsd_ild: the stage-2 loss (train_fn_ILD)")
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 256])
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--time_context", type=int, default=30)
    ap.add_argument("--feat_size", type=int, default=513)
    a = ap.parse_args()
    if a.ild and a.arch != "dsd_ild":
        ap.error("--ild goes with --arch dsd_ild")
    for B in a.batches:
        if a.arch == "dsd_ild":
            ms = bench_hip_ild(B, a.time_context, a.feat_size, a.steps, a.warmup, a.ild)
            tms = bench_torch_ild(B, a.time_context, a.feat_size, a.steps, a.warmup, a.ild)
        elif a.arch == "bach10_si_1x1":
            ms = bench_hip_deep(B, a.time_context, a.feat_size, a.steps, a.warmup, a.branches)
            tms = bench_torch_deep(B, a.time_context, a.feat_size, a.steps, a.warmup, a.branches)
        elif a.arch == "bach10_si":
            ms = bench_hip_si(B, a.time_context, a.feat_size, a.steps, a.warmup, a.branches)
            tms = bench_torch_si(B, a.time_context, a.feat_size, a.steps, a.warmup, a.branches)
        else:
            ms = bench_hip(B, a.time_context, a.feat_size, a.steps, a.warmup, a.arch)
            tms = bench_torch(B, a.time_context, a.feat_size, a.steps, a.warmup, a.arch)
        extra = {} if a.arch == "dsd" else dict(arch=a.arch)
        if a.arch == "dsd_ild":
            extra.update(ild=bool(a.ild))
        if a.arch in ("bach10_si", "bach10_si_1x1"):
            extra.update(branches=a.branches)
        if a.arch == "bach10_si_1x1":
            from deepconvsep_amd.arch import ARCHS
            flop = B * ARCHS["bach10_si_1x1"].train_flops_per_tile(a.time_context, a.feat_size)
            extra.update(step_flop=int(flop), hip_tflops=round(flop / ms * 1e-9, 2), torch_tflops=round(flop / tms * 1e-9, 2))
        launches = {"dsd": LAUNCHES_PER_STEP, "bach10_si_1x1": LAUNCHES_PER_STEP_DEEP1X1, "bach10": LAUNCHES_PER_STEP_BACH10, "bach10_si": LAUNCHES_PER_STEP_BACH10SI,
                    "dsd_ild": LAUNCHES_PER_STEP_ILD[bool(a.ild)]}.get(a.arch, LAUNCHES_PER_STEP_IKALA)
        if a.arch in ("bach10", "bach10_si"):
            floor = (bach10_floor if a.arch == "bach10" else bach10si_floor)(B, a.time_context, a.feat_size)
            extra.update(floor=floor, hip_over_floor=round(ms / max(floor["memory_ms"], floor["compute_ms"]), 2))
        print(json.dumps(dict(extra, batch=B, time_context=a.time_context, feat_size=a.feat_size, hip_ms_per_step=round(ms, 4),
                              hip_windows_per_s=round(B / ms * 1e3, 1), launches_per_step=launches,
                              torch_ms_per_step=round(tms, 4), torch_windows_per_s=round(B / tms * 1e3, 1),
                              speedup=round(tms / ms, 3))), flush=True)


if __name__ == "__main__":
    main()

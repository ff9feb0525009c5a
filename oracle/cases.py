"""Seeded network test cases shared by ``tests/golden/make_golden.py`` and the tests (test infrastructure).

A case = (graph, feature size, batch, seed, weight kind).  The weight kinds go beyond a fresh Glorot draw, whose
activations are dense and well conditioned:

``glorot``    ``deepconvsep_amd.synth.synth_params`` as is.
``sparse``    trained-like statistics: larger weights (gain 1.6), dense-layer biases in ``[-0.5, 0.05]``, and the output
              bias of every channel set so that about 92 % of the network outputs are cut to exactly zero by the final
              rectifier -- whole regions where every source is 0 (convention A: masks 1/S; convention B: 0).
``tiny``      like ``sparse`` at 50 %, but each output channel's bias is shifted so that one of its bins comes out as
              ``1e-10`` (and others land within 1e-9 .. 1e-6 of zero on either side): the region where
              ``max(x, 0) + eps`` and ``max(x, eps)`` differ and where float32 cannot tell a tiny positive from 0.
``dominant``  one branch dominant: output bias of channel 0 raised by the 99th percentile of the pre-bias output, the
              others cut at 90 %.

The output biases are calibrated on the float64 oracle and STORED in the fixture, so the GPU box rebuilds exactly
the same parameters from (seed, kind, stored bias) without the reference tree.
"""
import numpy as np

from deepconvsep_amd.arch import ARCHS
from deepconvsep_amd.synth import synth_params

from . import net_ref

KINDS = ("glorot", "sparse", "tiny", "dominant")


def make_input(arch, B, tc, F, seed):
    """float32-valued tiles: 0.3 * U(0, 3), digital-silence rows inside tile 0 (max-pool ties), a silent last tile when
    B > 1."""
    rs = np.random.RandomState(seed)
    C = ARCHS[arch].C
    x = (0.3 * rs.uniform(0, 3, (B, C, tc, F))).astype(np.float32)
    x[0, :, 4:9] = 0.0
    if B > 1:
        x[B - 1] = 0.0
    return x


def base_params(arch, tc, F, seed, kind):
    if kind == "glorot":
        return synth_params(arch, tc, F, seed=seed)
    params = synth_params(arch, tc, F, seed=seed, gain=1.6)
    rs = np.random.RandomState(seed + 1000)
    n_fc = ARCHS[arch].n_fc
    for i in [7] + [9 + 2 * k for k in range(n_fc)]:      # bottleneck and per-source dense biases
        params[i] = rs.uniform(-0.5, 0.05, params[i].shape).astype(np.float32)
    return params


def pre_bias_output(arch, params, x):
    """Network output before the output BiasLayer / rectifier (float64): evaluated with a bias large enough to keep
    the rectifier inactive, which is then subtracted (exact to ~1e-13 at these magnitudes)."""
    big = 64.0
    probe = [np.array(p) for p in params]
    probe[-1] = np.full(probe[-1].shape, big, dtype=np.float32)
    y = net_ref.forward(arch, probe, np.asarray(x, dtype=np.float64), inverse='explicit').numpy()
    assert y.min() > 0
    return y - big


def calibrate(arch, tc, F, seed, kind, x):
    """Parameters of the case with the output bias calibrated for ``kind`` (float32, like a ``.pkl``)."""
    params = base_params(arch, tc, F, seed, kind)
    if kind == "glorot":
        return params
    y = pre_bias_output(arch, params, x)                     # [B, ch, tc, F]
    ch = y.shape[1]
    live = y[np.abs(x).sum(axis=(1, 2, 3)) > 0]              # calibrate on the tiles that have input
    bias = np.zeros(ch)
    for c in range(ch):
        v = live[:, c].ravel()
        if kind == "sparse":
            bias[c] = -np.quantile(v, 0.92)
        elif kind == "dominant":
            bias[c] = np.quantile(np.abs(v), 0.99) if c == 0 else -np.quantile(v, 0.90)
        else:                                                # tiny: one bin of the channel comes out as 1e-10
            bias[c] = -(np.sort(v)[v.size // 2]) + 1e-10
    params[-1] = bias.astype(np.float32)
    return params


def case_params(arch, tc, F, seed, kind, out_bias=None):
    """Rebuild the parameters of a case from its seed and the stored calibrated output bias."""
    params = base_params(arch, tc, F, seed, kind)
    if out_bias is not None:
        params[-1] = np.asarray(out_bias, dtype=np.float32)
    return params


# (name, graph, F, batch, seed, kind): the committed network fixtures tests/golden/net_*.npz
NET_CASES = [
    ("net_dsd_f65_glorot", "dsd", 65, 2, 31, "glorot"),
    ("net_dsd_f33_sparse", "dsd", 33, 2, 32, "sparse"),
    ("net_dsd_f33_tiny", "dsd", 33, 2, 33, "tiny"),
    ("net_dsd_f33_dominant", "dsd", 33, 2, 34, "dominant"),
    ("net_ikala_f270_glorot", "ikala", 270, 1, 35, "glorot"),
    ("net_ikala_f270_sparse", "ikala", 270, 1, 36, "sparse"),
    ("net_bach10_f129_glorot", "bach10", 129, 1, 37, "glorot"),
    ("net_bach10_f129_sparse", "bach10", 129, 1, 38, "sparse"),
    ("net_bach10_f129_tiny", "bach10", 129, 1, 39, "tiny"),
    ("net_bach10si_f129_sparse", "bach10_si", 129, 1, 40, "sparse"),
    ("net_dsdild_f33_glorot", "dsd_ild", 33, 1, 41, "glorot"),
    ("net_ikalanp_f150_glorot", "ikala_nopool", 150, 1, 42, "glorot"),     # the iKala trainer's graph (no max-pool)
    ("net_ikalanp_f150_sparse", "ikala_nopool", 150, 1, 43, "sparse"),
    ("net_bach10si1_f129_sparse", "bach10_si1", 129, 1, 44, "sparse"),     # the single-branch score-informed graph (11 arrays)
]


# ---- randomised draws (tests/test_oracle_net.py on the CPU against the reference's executed graph, tests/test_gpu_random.py
# on the GPU against net_ref): beyond the committed fixtures.  A draw = (graph, small F, batch, weights, input), all from one
# integer seed: weight gain 0.5 .. 2.2, dense biases of either sign, output biases from strongly negative (most outputs cut
# to exact zeros) to positive, inputs from dense noise to few-level / silent rows (max-pool ties in the iKala graph).
RANDOM_GRAPHS = (("dsd", 65), ("dsd", 129), ("ikala", 270), ("ikala", 303), ("bach10", 129), ("bach10_si", 129),
                 ("ikala_nopool", 150))
# (appending a graph here would re-deal every seed: the single-branch score-informed graph has its own draws, tests/test_oracle_net.py)


def random_draw(seed):
    rs = np.random.RandomState(10_000 + int(seed))
    arch, F = RANDOM_GRAPHS[int(seed) % len(RANDOM_GRAPHS)]
    tc, B = 30, int(rs.randint(1, 4))
    gain = float(rs.uniform(0.5, 2.2))
    params = synth_params(arch, tc, F, seed=int(rs.randint(1 << 30)), gain=gain)
    n_fc = ARCHS[arch].n_fc
    lo, hi = sorted(rs.uniform(-0.6, 0.3, 2))
    for i in [7] + [9 + 2 * k for k in range(n_fc)]:
        params[i] = rs.uniform(lo, hi, params[i].shape).astype(np.float32)
    for i in (1, 2, 4, 5):                                      # the conv / BiasLayer biases
        params[i] = rs.uniform(-0.2, 0.2, params[i].shape).astype(np.float32)
    C = ARCHS[arch].C
    style = int(rs.randint(3))
    if style == 0:
        x = 0.3 * rs.uniform(0, 3, (B, C, tc, F))
    elif style == 1:                                             # few levels: equal neighbours -> ties in the max-pool
        x = 0.3 * rs.randint(0, 3, (B, C, tc, F)).astype(np.float64)
    else:                                                        # sparse input with silent rows and a silent tile
        x = 0.3 * rs.uniform(0, 3, (B, C, tc, F)) * (rs.uniform(size=(B, C, tc, F)) < 0.3)
        x[0, :, int(rs.randint(0, tc - 6)):][:, :5] = 0.0
        if B > 1:
            x[B - 1] = 0.0
    x = x.astype(np.float32)
    y = pre_bias_output(arch, params, x)
    q = float(rs.choice([0.1, 0.5, 0.9, 0.97]))                  # share of the outputs the rectifier cuts to zero
    bias = np.array([-np.quantile(y[:, c], q) for c in range(y.shape[1])])
    bias += rs.uniform(-0.02, 0.02, bias.shape)
    params[-1] = bias.astype(np.float32)
    return arch, F, params, x


def stored_elements(shape, seed, frac=0.05, edge=4):
    """The elements of a reference output [..., frames, bins] that tests/golden/fresh_random_draws.npz keeps at full
    precision: a seeded sample of `frac` of them plus every element of the first bin and of the last `edge` bins (where
    strided filters leave columns uncovered).  The same (shape, seed) always selects the same elements."""
    sel = np.random.RandomState(20_000 + int(seed)).rand(*shape) < frac
    sel[..., :1] = True
    sel[..., -edge:] = True
    return sel


def single_branch_draw(seed):
    """Seeded draws of the single-branch score-informed graph (trainCNNrwc_samp.py): (params, x [B, 4, 30, 129])."""
    rs = np.random.RandomState(500 + seed)
    tc, F, B = 30, 129, int(rs.randint(1, 3))
    params = synth_params("bach10_si1", tc, F, seed=int(rs.randint(1 << 30)), gain=float(rs.uniform(0.6, 2.0)))
    x = (0.3 * rs.uniform(0, 3, (B, 4, tc, F)) * (rs.uniform(size=(B, 4, tc, F)) < 0.6)).astype(np.float32)
    y = pre_bias_output("bach10_si1", params, x)
    params[-1] = np.array([-np.quantile(y[:, c], 0.7) for c in range(4)], dtype=np.float32)
    return params, x


# ---- seeded inputs of the score-informed front-end draws (tests/test_oracle_golden.py; the reference's answers on them are
# tests/golden/fresh_*.npz, written by make_golden.py)
def trainer_filterspec_draw(seed):
    """Seeded rectangles that overlap within and across instruments, a window that does not start at frame 0, an
    instrument without notes on odd seeds: (mag [T - start, F], notes [ninst, 6, 43], start, T)."""
    rs = np.random.RandomState(700 + seed)
    T, F, ninst = int(rs.randint(40, 90)), int(rs.randint(60, 300)), int(rs.randint(2, 6))
    mag = rs.rand(T, F).astype(np.float32)
    notes = np.zeros((ninst, 6, 43))
    for j in range(ninst):
        for p in range(0 if j == ninst - 1 and seed % 2 else int(rs.randint(1, 6))):
            b = int(rs.randint(0, T + 20))
            notes[j, p, :3] = (b, b + int(rs.randint(1, 30)), 40 + p)
            for k in range(int(rs.randint(1, 12))):
                f0 = int(rs.randint(0, F - 16))
                notes[j, p, 3 + 2 * k], notes[j, p, 4 + 2 * k] = f0, f0 + int(rs.randint(1, 16))
    start = int(rs.randint(0, 10))
    return mag[start:], notes, start, T


def timbre_draw(seed):
    """Seeded timbre templates [2 instruments, 128 pitches, 20 harmonics] (float32) and magnitudes [520, 1025]."""
    rs = np.random.RandomState(900 + seed)
    H = rs.uniform(0.0, 2.0, (2, 128, 20)).astype(np.float32)
    mag = np.abs(rs.randn(520, 1025)).astype(np.float32)
    return H, mag

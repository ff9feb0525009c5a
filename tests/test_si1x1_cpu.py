"""The deep score-informed graph build_ca_1x1 (examples/bach10_scoreinformed/trainCNNrwc.py:66-132) on the host: how a
22-array .pkl resolves, its shapes and live part, its FLOP count, the float64 restatement tests/deep1x1_ref.py against the
reference's own graph (fixtures written by tests/golden/make_golden_1x1.py), and the kernels' register budget."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import deep1x1_ref  # noqa: E402
import make_golden_1x1  # noqa: E402
from deepconvsep_amd.arch import ARCHS, check_params, live_params, resolve  # noqa: E402
from deepconvsep_amd.synth import synth_params  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "net_bach10si1x1_f257_*.npz")))


def _fixture(path):
    z = np.load(path)
    shapes = [tuple(int(v) for v in row[:nd]) for row, nd in zip(z["shapes"], z["ndims"])]
    name = os.path.basename(path)[len("net_bach10si1x1_f257_"):-4]
    _, n, tc, zero = make_golden_1x1.CASES[name]
    params = make_golden_1x1.params_for(int(z["seed"]), int(z["tc"]), zero, shapes)
    return z, shapes, params


def test_fixtures_present():
    assert [os.path.basename(p) for p in FIXTURES] == ["net_bach10si1x1_f257_rand.npz", "net_bach10si1x1_f257_zero.npz"]


@pytest.mark.parametrize("tc,F", [(30, 2049), (20, 257), (19, 253), (45, 1025)])
def test_22_arrays_resolve_to_the_deep_graph(tc, F):
    params = synth_params("bach10_si_1x1", tc, F, seed=0)
    assert len(params) == 22
    a = resolve("bach10_si", params, tc, F)
    assert a.name == "bach10_si_1x1" and a.code == 7 and a.C == 4 and a.S == 4
    check_params(a, params, tc, F)
    # the live part: the 1x1 conv's rows 0..199 and the final bias [0:4] -- also a layout of its own that resolves and checks
    _, live = live_params(a, params)
    assert [tuple(p.shape) for p in live] == a.param_shapes(tc, F, branches=1)
    assert tuple(live[18].shape) == (200, 200, 1, 1) and tuple(live[21].shape) == (4,)
    assert np.array_equal(live[18], params[18][:200]) and np.array_equal(live[21], params[21][:4])
    assert resolve("bach10_si", live, tc, F).name == "bach10_si_1x1"
    check_params(a, live, tc, F)
    # the other score-informed layouts are untouched
    assert resolve("bach10_si", synth_params("bach10_si", 30, 129, seed=0), 30, 129).name == "bach10_si"
    assert resolve("bach10_si", synth_params("bach10_si1", 30, 129, seed=0), 30, 129).name == "bach10_si1"


def test_wrong_shapes_raise_value_error():
    a = ARCHS["bach10_si_1x1"]
    params = synth_params("bach10_si_1x1", 30, 513, seed=0)
    bad = list(params)
    bad[12] = np.zeros((200, 100, 9, 5), np.float32)                 # conv5 with 9 filter rows
    with pytest.raises(ValueError, match="mismatch"):
        check_params(a, bad, 30, 513)
    bad = list(params)
    bad[18] = np.zeros((300, 200, 1, 1), np.float32)                 # not a whole number of 200-channel branches
    with pytest.raises(ValueError, match="mismatch"):
        check_params(a, bad, 30, 513)
    check_params(a, params, 30, 1025)                                # a convolutional graph: no shape depends on F
    with pytest.raises(ValueError):
        a.dims(18, 2049)                                             # conv6 has no output row left


def test_param_shapes_match_the_reference_graph():
    """The fixtures store the shapes the reference's own build_ca_1x1 produced; with the reference tree present they
    are rebuilt here from its source as well."""
    for path in FIXTURES:
        z, shapes, _ = _fixture(path)
        assert shapes == ARCHS["bach10_si_1x1"].param_shapes(int(z["tc"]), 257)
    from oracle import ref_exec
    if ref_exec.available():
        for tc, F in ((30, 2049), (19, 253)):
            assert make_golden_1x1.param_shapes(tc, F) == ARCHS["bach10_si_1x1"].param_shapes(tc, F)


def test_flops_per_tile():
    a = ARCHS["bach10_si_1x1"]
    assert abs(a.flops_per_tile(30, 2049, live_only=True) - 9.52e9) < 0.01e9
    assert abs(a.flops_per_tile(30, 2049) - 23.9e9) < 0.1e9
    d = a.dims(30, 2049)
    assert [(l["cout"], l["ho"], l["wo"]) for l in d["layers"]] == [(30, 30, 1023), (50, 30, 510), (70, 30, 253),
                                                                    (100, 30, 125), (200, 21, 61), (200, 12, 29)]


@pytest.mark.parametrize("F", [257, 513, 1025, 2049])
def test_conv3_leaves_its_last_input_column_uncovered(F):
    l3 = ARCHS["bach10_si_1x1"].dims(30, F)["layers"][2]
    assert (l3["wi"] - 5) % 2 == 1 and 2 * (l3["wo"] - 1) + 5 == l3["wi"] - 1


@pytest.mark.parametrize("path", FIXTURES, ids=os.path.basename)
def test_restatement_matches_the_reference_graph(path):
    z, shapes, params = _fixture(path)
    assert make_golden_1x1.checksum(params) == str(z["checksum"])
    p = deep1x1_ref.forward(params, z["x"])
    assert p.shape == z["p"].shape and p.shape[1] == 16
    assert np.max(np.abs(p - z["p"])) < 1e-10
    assert np.max(z["p"]) > 1e-2 and np.mean(z["p"] > 0) > 0.1        # the signal survived six rectified layers
    # the live-only layout gives the first four channels
    _, live = live_params(ARCHS["bach10_si_1x1"], params)
    assert np.max(np.abs(deep1x1_ref.forward(live, z["x"]) - z["p"][:, :4])) < 1e-10
    for mixture, key in (("ch0", "masked_ch0"), ("sum", "masked_sum")):
        assert np.max(np.abs(deep1x1_ref.masked(p, z["x"], 1, mixture) - z[key])) < 1e-10


def test_zero_bias_fixture_pins_the_half_derivative_at_zero():
    """The fixture with zero conv1 / conv2 biases and silent frames has exact-zero pre-activations: r'(0) = 0 or 1 moves
    p by more than 1e-3, r'(0) = 0.5 (Theano's relu) reproduces it.  Conv3's uncovered column is in the fixture's p."""
    z, shapes, params = _fixture(os.path.join(HERE, "golden", "net_bach10si1x1_f257_zero.npz"))
    for alt in (0.0, 1.0):
        assert np.max(np.abs(deep1x1_ref.forward(params, z["x"], rprime0=alt) - z["p"])) > 1e-3


def test_deep1x1_kernels_do_not_spill():
    """hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage: no kernel of deep1x1.hip uses scratch."""
    src = os.path.join(ROOT, "deepconvsep_amd", "csrc", "deep1x1.hip")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
                        "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0, r.stderr[-2000:]
    names = [l for l in r.stderr.splitlines() if "Function Name:" in l]
    scratch = [l for l in r.stderr.splitlines() if "ScratchSize [bytes/lane]:" in l]
    spills = [l for l in r.stderr.splitlines() if "Spill:" in l]
    assert len(names) >= 14 and len(scratch) == len(names)
    assert all(l.rstrip().endswith(": 0 [-Rpass-analysis=kernel-resource-usage]") for l in scratch + spills), scratch + spills

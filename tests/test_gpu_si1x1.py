"""The deep score-informed graph build_ca_1x1 (examples/bach10_scoreinformed/trainCNNrwc.py:66-132) on the MI355X:
the network against the reference's own graph (fixtures of tests/golden/make_golden_1x1.py), the whole separation path
against a CPU composition of the oracle's stages and the float64 restatement tests/deep1x1_ref.py, the command line, and
the guard-band harness."""
import json
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
import deepconvsep_amd as dcs  # noqa: E402
import make_golden_1x1  # noqa: E402
from deepconvsep_amd.arch import ARCHS, EPS_A, EPS_B, live_params  # noqa: E402
from deepconvsep_amd.runtime import Network, StftPlan, default_context  # noqa: E402
from deepconvsep_amd.synth import synth_audio, synth_params  # noqa: E402
from maskcheck import check_masked  # noqa: E402

pytestmark = pytest.mark.gpu

SI_INSTS = ["bassoon_b", "clarinet_b", "saxophone_b", "violin_b"]
FIXTURES = ["net_bach10si1x1_f257_zero.npz", "net_bach10si1x1_f257_rand.npz"]


def _fixture(name):
    z = np.load(os.path.join(HERE, "golden", name))
    shapes = [tuple(int(v) for v in row[:nd]) for row, nd in zip(z["shapes"], z["ndims"])]
    _, n, tc, zero = make_golden_1x1.CASES[name[len("net_bach10si1x1_f257_"):-4]]
    params = make_golden_1x1.params_for(int(z["seed"]), int(z["tc"]), zero, shapes)
    assert make_golden_1x1.checksum(params) == str(z["checksum"])
    return z, params


@pytest.mark.parametrize("name", FIXTURES)
def test_network_matches_the_reference_graph(name):
    z, params = _fixture(name)
    ctx = default_context()
    x = z["x"]
    tc, F = x.shape[2], x.shape[3]
    xd = ctx.to_device(x, np.float32)
    full = Network(ctx, "bach10_si", params, tc, F, live_only=False)
    assert full.arch.name == "bach10_si_1x1" and full.out_channels == 16 and full.S == 4
    p16 = ctx.to_host(full.forward_raw(xd))
    assert p16.shape == z["p"].shape and np.isfinite(p16).all()
    assert np.max(np.abs(p16 - z["p"])) < 1e-4
    live = Network(ctx, "bach10_si", params, tc, F)
    assert live.out_channels == 4
    p4 = ctx.to_host(live.forward_raw(xd))
    assert np.max(np.abs(p4 - z["p"][:, :4])) < 1e-4
    # the live-only .pkl layout loads as such
    _, lp = live_params(ARCHS["bach10_si_1x1"], params)
    assert np.max(np.abs(ctx.to_host(Network(ctx, "bach10_si", lp, tc, F).forward_raw(xd)) - p4)) < 2e-6
    for net in (live, full):
        for sem, key in ((("max", "ch0"), "masked_ch0"), (("sum", "sum"), "masked_sum")):
            net.set_score_semantics(*sem)
            got = ctx.to_host(net.forward_masked(xd, eps_mode=EPS_B))
            mix = x[:, 0] if sem[1] == "ch0" else x.astype(np.float64).sum(axis=1)
            check_masked(got, z[key], z["p"][:, :4], p4, mix, 4, 'B', label="si1x1 %s %s" % (name, sem[1]))
            got_a = ctx.to_host(net.forward_masked(xd, eps_mode=EPS_A))
            want_a = deep1x1_ref.masked(z["p"], x, 0, sem[1])
            check_masked(got_a, want_a, z["p"][:, :4], p4, mix, 4, 'A', label="si1x1 %s %s A" % (name, sem[1]))


def test_unsupported_calls_say_so():
    ctx = default_context()
    params = synth_params("bach10_si_1x1", 30, 257, seed=3)
    net = Network(ctx, "bach10_si", params, 30, 257)
    with pytest.raises(NotImplementedError, match="f32"):
        net.set_conv_precision('f16')
    net.set_conv_precision('f32')
    with pytest.raises(NotImplementedError):
        net.set_latency_stages(1)
    plan = StftPlan(ctx, 512, 256, np.hanning(512))
    a = ctx.to_device(synth_audio(44100, seed=1).astype(np.float32), np.float32)
    with pytest.raises(NotImplementedError, match="build_ca_1x1"):
        net.separate(plan, a, 25)
    with pytest.raises(NotImplementedError):
        net.separate_batch(plan, a.view(1, -1), 25)
    # tie_mode is accepted and has no effect (no pooling)
    x = ctx.to_device(np.random.RandomState(0).uniform(0, 1, (3, 4, 30, 257)).astype(np.float32), np.float32)
    assert np.array_equal(ctx.to_host(net.forward_raw(x, tie_mode=0)), ctx.to_host(net.forward_raw(x, tie_mode=1)))
    # a tile shape the graph cannot take (conv6 would have no output row)
    with pytest.raises(ValueError):
        Network(ctx, "bach10_si", params, 18, 257)


def test_chunks_of_a_large_batch_are_the_tiles_alone():
    """Batches run through the network 32 tiles at a time: 70 tiles give, tile for tile, the values of smaller batches."""
    ctx = default_context()
    params = synth_params("bach10_si_1x1", 20, 257, seed=4)
    net = Network(ctx, "bach10_si", params, 20, 257, live_only=False)
    x = np.random.RandomState(5).uniform(0, 1, (70, 4, 20, 257)).astype(np.float32)
    xd = ctx.to_device(x, np.float32)
    big = ctx.to_host(net.forward_raw(xd))
    parts = [ctx.to_host(net.forward_raw(ctx.to_device(x[a:b], np.float32))) for a, b in ((0, 3), (3, 40), (40, 70))]
    assert np.array_equal(big, np.concatenate(parts))
    m_big = ctx.to_host(net.forward_masked(xd))
    m_part = ctx.to_host(net.forward_masked(ctx.to_device(x[33:70], np.float32)))
    assert np.array_equal(m_big[:, 33:], m_part)
    want = deep1x1_ref.forward(params, x[62:70])
    assert np.max(np.abs(big[62:70] - want)) < 1e-4


def _score_files(tmp_path, seconds):
    from oracle import score_np
    for i, ins in enumerate(SI_INSTS):
        score_np.synth_score(str(tmp_path / (ins + ".txt")), 900 + i, n_notes=12, total=seconds + 0.5, lo=40 + 5 * i,
                             hi=64 + 6 * i)
    return [str(tmp_path / (i + ".txt")) for i in SI_INSTS]


def _cpu_pipeline(params, audio, melody, semantics):
    """separate_scoreinformed of oracle.pipeline with the network replaced by the float64 restatement (branch 0)."""
    from scipy.signal.windows import blackmanharris
    from oracle import score_np, stft_np, tiling_np
    audio = np.asarray(audio, dtype=np.float64)
    nframes = int(np.ceil(len(audio) / 512.0)) + 2
    mag, ph = stft_np.compute_file(audio, phase=True, frameSize=4096, hopSize=512, window=blackmanharris)
    mag = 0.3 * mag.astype(np.float32)
    inp = score_np.network_input(mag, np.asarray(melody), nframes, None, normalise=semantics[0])
    batches, nchunks = tiling_np.generate_overlapadd(inp, inp.shape[-1], 30, 25, 32, tiler=tiling_np.LIBRARY, fill=0.0)
    out = []
    for b in batches:
        p = deep1x1_ref.forward(params, b, branches=1)
        out.append(list(deep1x1_ref.masked(p, b, EPS_B, semantics[1])[:, :, None]))
    mm = tiling_np.overlapadd_multi(np.array(out), nchunks, overlap=25)
    pcm = []
    for i in range(mm.shape[0]):
        a = stft_np.compute_inverse(mm[i, :len(ph)] / 0.3, ph, frameSize=4096, hopSize=512, window=blackmanharris)
        pcm.append(a[:len(audio)])
    return np.stack(pcm)


def test_whole_path_matches_the_cpu_pipeline(tmp_path):
    from deepconvsep_amd import score
    from scipy.signal.windows import blackmanharris
    L = 4 * 44100
    audio = synth_audio(L, seed=95)
    files = _score_files(tmp_path, L / 44100.0)
    nframes = int(np.ceil(L / 512.0)) + 2
    melody = score.melody_table([os.path.basename(f) for f in files], str(tmp_path), nframes, 44100, 512, 4096)
    params = synth_params("bach10_si_1x1", 30, 2049, seed=7)
    sep = dcs.Separator("bach10_si", params, 0.3, 30, 25, 32, 2049, 4096, 512, blackmanharris, tiler='library',
                        score_normalise='sum', score_mixture='sum')
    assert sep.net.arch.name == "bach10_si_1x1"
    got = sep.separate_scoreinformed(audio, melody)
    want = _cpu_pipeline(params, audio, melody, ("sum", "sum"))
    assert got.shape == want.shape == (4, L)
    assert np.max(np.abs(want)) > 1e-3
    # f32 against float64: of the ~2e8 pre-activations of this clip's 65 tiles, some lie within float32 rounding of zero
    # and take the other side of the rectify, and their r' moves the decoder output near them; the iSTFT spreads such a
    # spot over a 4096-sample window (the fixtures reject such draws; real spectra cannot be chosen).  Measured on this
    # clip: 99 % of the samples within 6e-5, 0.6 % above 1e-4, max 5.8e-4.
    err = np.abs(got - want)
    stats = "max %.3g, p99.9 %.3g, p99 %.3g, mean %.3g, %d of %d samples above 1e-4" % (
        err.max(), np.quantile(err, 0.999), np.quantile(err, 0.99), err.mean(), int((err > 1e-4).sum()), err.size)
    assert np.quantile(err, 0.99) < 1e-4 and np.mean(err > 1e-4) < 0.01, stats
    assert np.max(err) < 2e-3, stats
    sep128 = dcs.Separator("bach10_si", params, 0.3, 30, 25, 128, 2049, 4096, 512, blackmanharris, tiler='library',
                           score_normalise='sum', score_mixture='sum')
    assert np.max(np.abs(sep128.separate_scoreinformed(audio, melody) - got)) < 2e-6


def test_command_line_loads_the_22_array_model(tmp_path):
    import importlib.util
    import scipy.io.wavfile
    from deepconvsep_amd import score
    from scipy.signal.windows import blackmanharris
    L = int(1.5 * 44100)
    audio = synth_audio(L, seed=96)
    wav = tmp_path / "mix.wav"
    scipy.io.wavfile.write(str(wav), 44100, (audio * 32767).astype(np.int16))
    files = _score_files(tmp_path, L / 44100.0)
    params = synth_params("bach10_si_1x1", 30, 2049, seed=8)
    model = tmp_path / "model_1_x_1.pkl"
    dcs.save_model(str(model), params)
    out = tmp_path / "out"
    out.mkdir()
    spec = importlib.util.spec_from_file_location("si_cli_1x1", os.path.join(ROOT, "examples", "bach10_scoreinformed",
                                                                             "separate_bach10.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cli.main(["-i", str(wav), "-o", str(out), "-m", str(model), "--trainer-semantics"])
    sr, a16 = scipy.io.wavfile.read(str(wav))
    a = a16.astype('float') / 32767
    nframes = int(np.ceil(len(a) / 512.0)) + 2
    melody = score.melody_table([os.path.basename(f) for f in files], str(tmp_path), nframes, 44100, 512, 4096)
    sep = dcs.Separator("bach10_si", params, 0.3, 30, 25, 32, 2049, 4096, 512, blackmanharris, tiler='library',
                        score_normalise='sum', score_mixture='sum')
    want = sep.separate_scoreinformed(a, melody)
    for i, s in enumerate(["bassoon", "clarinet", "saxphone", "violin"]):
        sr2, got = scipy.io.wavfile.read(str(out / ("mix_%s.wav" % s)))
        assert sr2 == 44100 and got.dtype == np.int16 and len(got) == L
        assert np.array_equal(got, (want[i] * 32767).astype('int16'))


_CHILD = r'''
import hashlib, json, os, sys
ROOT, OUT = sys.argv[1], sys.argv[2]
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import deepconvsep_amd as dcs
from deepconvsep_amd import score
from deepconvsep_amd.runtime import Network, default_context
from deepconvsep_amd.synth import synth_audio, synth_params
from oracle import score_np
from scipy.signal.windows import blackmanharris
ctx = default_context()
res = {}
h = hashlib.sha256()
finite = True
def take(a):
    global finite
    a = np.ascontiguousarray(a)
    h.update(a.tobytes())
    finite = finite and bool(np.isfinite(a).all())
params = synth_params("bach10_si_1x1", 30, 2049, seed=9)
before = ctx.check_guards()
net = Network(ctx, "bach10_si", params, 30, 2049, live_only=False)
res["model_blocks"] = ctx.check_guards() - before
x = ctx.to_device(np.random.RandomState(4).uniform(0, 1, (37, 4, 30, 2049)).astype(np.float32), np.float32)
take(ctx.to_host(net.forward_raw(x)))
take(ctx.to_host(net.forward_masked(x)))
L = 2 * 44100
audio = synth_audio(L, seed=97)
d = os.path.join(OUT + ".scores")
os.makedirs(d, exist_ok=True)
names = ["bassoon_b", "clarinet_b", "saxophone_b", "violin_b"]
for i, ins in enumerate(names):
    score_np.synth_score(os.path.join(d, ins + ".txt"), 910 + i, n_notes=8, total=2.5, lo=40 + 5 * i, hi=64 + 6 * i)
melody = score.melody_table([n + ".txt" for n in names], d, int(np.ceil(L / 512.0)) + 2, 44100, 512, 4096)
sep = dcs.Separator("bach10_si", params, 0.3, 30, 25, 32, 2049, 4096, 512, blackmanharris, tiler='library')
for _ in range(2):
    take(sep.separate_scoreinformed(audio, melody))
ctx.synchronize()
res["guard_blocks"] = ctx.check_guards()
res["sha256"] = h.hexdigest()
res["finite"] = finite
json.dump(res, open(OUT, "w"))
'''


def test_guard_band_harness(tmp_path):
    """Model creation, forward and the whole path (twice) under DCS_WS_GUARD with poison 0xFF and 0x4B: red zones intact
    (check_guards raises on damage), outputs finite and bit-identical, and the model's weights inside the harness (its
    creation adds at least the 34 device blocks it keeps: per convolution B, two transposed B, b, BiasLayer.b; the 1x1
    conv's B, b, BiasLayer.b; the final bias)."""
    outs = []
    for poison in (0xFF, 0x4B):
        out = str(tmp_path / ("guard_%d.json" % poison))
        env = dict(os.environ)
        env.update({"DCS_WS_GUARD": "65536", "DCS_WS_POISON": str(poison)})
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, out], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append(json.load(open(out)))
    for o in outs:
        assert o["finite"] and o["model_blocks"] >= 6 * 5 + 4 and o["guard_blocks"] > 0
    assert outs[0]["sha256"] == outs[1]["sha256"]

"""Round-2 GPU parity tests (MI355X box, through the C ABI):

* the HIP networks against tests/golden/net_*.npz -- outputs of the reference's OWN build_ca source and mask
  expressions executed on the NumPy Lasagne stand-in -- including trained-like / adversarial weight sets, with the
  count of mask bins outside 1e-4 reported for every case;
* whole-path parity at the BASELINE.json configurations that round 1 only covered at reduced size: iKala at
  frameSize 2048 (10 s stereo, overlap 20), the Bach10 f16-MFMA conv path at F = 2049, the score-informed graph with
  one batch of 128 tiles;
* the N > 1 code path of bench.py (two ranks on this GPU) and the long-file sharding with the HIP separator as the
  per-rank worker (gloo);
* contexts on a side stream used without an enclosing ``torch.cuda.stream`` block (copy / kernel ordering).
"""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import deepconvsep_amd as dcs  # noqa: E402
from deepconvsep_amd.arch import ARCHS, TIE_FIRST  # noqa: E402
from deepconvsep_amd.runtime import Context, Network, default_context  # noqa: E402
from deepconvsep_amd.synth import synth_audio, synth_params, synth_score_text  # noqa: E402
from maskcheck import check_masked  # noqa: E402
from oracle import cases, net_ref, pipeline  # noqa: E402

NET_NAMES = [c[0] for c in cases.NET_CASES if c[1] != "dsd_ild"]     # the stereo graph runs through dcs_separate_stereo


@pytest.mark.parametrize("name", NET_NAMES)
def test_hip_network_matches_the_reference_graph_fixtures(golden, name):
    """Network output before masking within 1e-4 on every bin; masked sources within the mask-conditioning bound on
    every bin and within 1e-4 wherever that bound allows (tests/maskcheck.py); counts reported."""
    g = golden(name)
    arch, F, seed, kind = str(g["arch"]), int(g["F"]), int(g["seed"]), str(g["kind"])
    params = cases.case_params(arch, 30, F, seed, kind, g["out_bias"] if kind != "glorot" else None)
    ctx = default_context()
    net = Network(ctx, arch, params, 30, F, live_only=False)     # the whole graph, as the fixture holds it (score-informed: 16 channels)
    xd = ctx.to_device(g["x"], np.float32)
    p = ctx.to_host(net.forward_raw(xd))
    assert p.shape == g["p"].shape
    assert np.max(np.abs(p - g["p"])) < 1e-4
    if "p_tie_first" in g.files:
        p1 = ctx.to_host(net.forward_raw(xd, tie_mode=TIE_FIRST))
        assert np.max(np.abs(p1 - g["p_tie_first"])) < 1e-4
    S = ARCHS[arch].S
    got = ctx.to_host(net.forward_masked(xd))
    conv = 'A' if ARCHS[arch].eps_mode == 0 else 'B'
    rec = check_masked(got, g["masked"][:, :, 0], g["p"], p, g["x"][:, 0], S, conv, label="%s (%s)" % (name, kind))
    assert rec["mask_consistent"]
    if rec["unconditioned_bins"] == 0:                  # no ill-conditioned bin: nothing may be outside 1e-4 (a tripwire, not a lottery)
        assert rec["bins_outside_1e4"] == 0
    if "masked_sum" in g.files:       # the score-informed trainers' mask expressions (x the sum of the input channels), and the pruned model
        net.set_score_semantics('max', 'sum')
        got = ctx.to_host(net.forward_masked(xd))
        check_masked(got, g["masked_sum"][:, :, 0], g["p"], p, g["x"].astype(np.float64).sum(axis=1), S, conv,
                     label="%s (%s), channel-sum mixture" % (name, kind))
        live = Network(ctx, arch, params, 30, F)
        live.set_score_semantics('max', 'sum')
        assert live.out_channels == 4
        assert np.max(np.abs(ctx.to_host(live.forward_masked(xd)) - got)) < 2e-6


def test_ikala_trainer_pkl_selects_the_no_pool_graph(tmp_path):
    """a .pkl written by examples/ikala/trainCNN.py (no MaxPool2DLayer, fc.W with 30*21*143 = 90 090 rows at 513
    bins) loads into the no-pool graph, chosen from the shapes; whole path against the oracle through Separator('ikala', ...)
    and through the separate_ikala.py command line, and a pooled .pkl still takes the pooled graph."""
    import subprocess
    import scipy.io.wavfile
    F, N, ov = 513, 1024, 20
    # gain 1.8: with a plain Glorot draw of this 90 090-wide graph both sources come out around 1e-4 in places, and a mask
    # p_i / sum(p) there turns a 1e-7 float32 difference of p into 5e-4 of the mixture (tests/maskcheck.py's bound)
    params = synth_params("ikala_nopool", 30, F, seed=6, gain=1.8)
    assert params[6].shape == (90090, 256)
    sep = dcs.Separator("ikala", params, 0.3, 30, ov, 32, F, N, 512, np.hanning)
    assert sep.net.arch.name == "ikala_nopool"
    audio = synth_audio(66150, seed=9)
    got = sep.separate(audio)
    want = pipeline.separate("ikala_nopool", params, audio, 0.3, 30, ov, 32, N, 512, np.hanning)
    assert got.shape == want.shape == (2, audio.size)
    assert np.max(np.abs(got - want)) < 1e-4
    pooled = dcs.Separator("ikala", synth_params("ikala", 30, F, seed=6), 0.3, 30, ov, 32, F, N, 512, np.hanning)
    assert pooled.net.arch.name == "ikala"
    with pytest.raises(ValueError):                         # neither graph: set_all_param_values' failure
        bad = [np.array(p) for p in params]
        bad[6] = bad[6][:-1]
        dcs.Separator("ikala", bad, 0.3, 30, ov, 32, F, N, 512, np.hanning)
    # the command line
    model = str(tmp_path / "trainer.pkl")
    dcs.save_model(model, params)
    st = synth_audio(44100, seed=3, channels=2)
    wav = str(tmp_path / "mix.wav")
    scipy.io.wavfile.write(wav, 44100, (st * 32767).astype('int16'))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ikala", "separate_ikala.py"), "-i", wav, "-o",
                        str(tmp_path), "-m", model], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-800:]
    sr, voice = scipy.io.wavfile.read(str(tmp_path / "mix-voice.wav"))
    mono = (st * 32767).astype('int16').astype('float') / 32767
    want2 = pipeline.separate("ikala_nopool", params, mono[:, 0] + mono[:, 1], 0.3, 30, ov, 32, N, 512, np.hanning)
    assert sr == 44100 and np.max(np.abs(voice.astype(int) - (want2[0] * 32767).astype('int16').astype(int))) <= 2


# ------------------------------------------------------------------------------------------------ BASELINE configs
def test_ikala_frame2048_ten_seconds_stereo_matches_oracle():
    """BASELINE configs[0] as worded: iKala 2-source, frameSize=2048 hop=512, time_context=30, overlap 20
    (separate_ikala.py:275), a 10 s stereo wav summed L+R (:229).  84 tiles, 1025 bins."""
    F, N = 1025, 2048
    params = synth_params("ikala", 30, F, seed=1)
    stereo = synth_audio(441000, seed=0, channels=2)
    audio = stereo[:, 0] + stereo[:, 1]
    sep = dcs.Separator("ikala", params, 0.3, 30, 20, 32, F, N, 512, np.hanning)
    got = sep.separate(audio)
    assert sep.net.last_tiles == 84 and sep.net.last_frames == 864
    want = pipeline.separate("ikala", params, audio, 0.3, 30, 20, 32, N, 512, np.hanning)
    assert got.shape == want.shape == (2, audio.size)
    assert np.max(np.abs(got - want)) < 1e-4
    # convention-A masks partition the mixture and the cross-fade weights of a frame sum to one: the two sources add
    # up to the input wherever whole tiles cover the signal (the script tiler drops the tail)
    covered = (83 * 10 + 30 - 4) * 512 - N
    assert np.max(np.abs(got.sum(axis=0)[N:covered] - audio[N:covered])) < 2e-5
    d = np.abs((got * 32767).astype('int16').astype(int) - (want * 32767).astype('int16').astype(int))
    assert d.max() <= 2


def test_bach10_f16_conv_path_at_full_size_stated_tolerance():
    """BASELINE configs[3]: Bach10 4-instrument graph at its real size (frameSize 4096 -> 2049 bins, 17-array model)
    with the f16-input / f32-accumulate MFMA conv path.  f16 keeps 11 significant bits, so this path is held to its
    own stated tolerance, not to 1e-4: network output max |err| < 2e-3; masked magnitudes p99.9 < 1e-3 and max < 5e-3
    on the bins whose reference denominator exceeds 1e-2; PCM of a 1.2 s clip within 2e-3.  The statistics go to
    gpurun_out/f16_stats.txt."""
    F, N, n, S = 2049, 4096, 4, 4
    params = synth_params("bach10", 30, F, seed=3)
    rs = np.random.RandomState(12)
    x = (0.3 * rs.uniform(0, 3, (n, 1, 30, F))).astype(np.float32)
    x[1, :, 4:9] = 0.0
    x[n - 1] = 0.0
    ctx = default_context()
    net = Network(ctx, "bach10", params, 30, F)
    xd = ctx.to_device(x, np.float32)
    p_ref = net_ref.forward("bach10", params, x.astype(np.float64), inverse='explicit').numpy()
    ref = np.stack([r[:, 0] for r in net_ref.predict("bach10", params, x.astype(np.float64), inverse='explicit')])
    p32 = ctx.to_host(net.forward_raw(xd))
    f32 = ctx.to_host(net.forward_masked(xd))
    assert np.max(np.abs(p32 - p_ref)) < 1e-4
    check_masked(f32, ref, p_ref, p32, x[:, 0], S, 'B', label="bach10 F=2049 f32")
    net.set_conv_precision('f16')
    p16 = ctx.to_host(net.forward_raw(xd))
    f16 = ctx.to_host(net.forward_masked(xd))
    perr, err = np.abs(p16 - p_ref), np.abs(f16 - ref)
    well = (p_ref[:, :S].sum(axis=1) > 1e-2)[None].repeat(S, axis=0)
    stats = ("bach10 F=2049 f16 conv path: raw output max|err| %.3e; masked p99.9 %.3e, mean %.3e, max over "
             "well-conditioned bins %.3e (%.1f%% of bins), max overall %.3e; f32 path raw max %.3e" % (
                 perr.max(), np.percentile(err, 99.9), err.mean(), err[well].max(), 100.0 * well.mean(), err.max(),
                 np.abs(p32 - p_ref).max()))
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/f16_stats.txt", "a") as fh:
        fh.write(stats + "\n")
    assert perr.max() < 2e-3, stats
    assert np.percentile(err, 99.9) < 1e-3 and err[well].max() < 5e-3, stats
    check_masked(f16, ref, p_ref, p16, x[:, 0], S, 'B', tol=5e-3, label="bach10 F=2049 f16 conv path")
    # whole path with the switch on
    audio = synth_audio(52000, seed=5)
    sep = dcs.Separator("bach10", params, 0.3, 30, 25, 32, F, N, 512, dcs.blackmanharris)
    sep.net.set_conv_precision('f16')
    got = sep.separate(audio)
    want = pipeline.separate("bach10", params, audio, 0.3, 30, 25, 32, N, 512, dcs.blackmanharris)
    perr = np.abs(got - want)
    with open("gpurun_out/f16_stats.txt", "a") as fh:
        fh.write("bach10 F=2049 f16 conv path, whole path 1.18 s: PCM max|err| %.3e, p99.9 %.3e\n"
                 % (perr.max(), np.percentile(perr, 99.9)))
    assert perr.max() < 2e-3


def test_bach10_fused_decoders_at_full_size_with_128_tiles_and_more():
    """From 128 tiles on the Bach10 graph takes its round-4 paths: the bf16 planes of the per-source dense layers packed with
    permuted columns (channels-last D) and BOTH InverseLayers in one kernel -- f32-class on three-way split operands
    (colconv_x3.hip) without the switch, f16 inputs in both stages with it.  132 tiles at the real size (2049 bins, 505
    columns: 31 full column blocks + one of 9) against the float64 oracle: 1e-4 per network-output bin f32-class, the f16
    path's stated 2e-3."""
    F, n = 2049, 132
    params = synth_params("bach10", 30, F, seed=3)
    rs = np.random.RandomState(31)
    x = (0.3 * rs.uniform(0, 3, (n, 1, 30, F))).astype(np.float32)
    x[1, :, 4:9] = 0.0
    x[n - 1] = 0.0
    want = net_ref.forward("bach10", params, x.astype(np.float64), inverse='explicit').numpy()
    ctx = default_context()
    net = Network(ctx, "bach10", params, 30, F)
    xd = ctx.to_device(x, np.float32)
    p32 = ctx.to_host(net.forward_raw(xd))
    assert np.isfinite(p32).all() and np.max(np.abs(p32 - want)) < 1e-4
    net.set_conv_precision('f16')
    p16 = ctx.to_host(net.forward_raw(xd))
    assert np.isfinite(p16).all() and np.max(np.abs(p16 - want)) < 2e-3
    # fewer than 128 tiles: the f32 GEMM, channel-first D and the unfused / channel-first kernels -- same bars
    net.set_conv_precision('f32')
    q32 = ctx.to_host(net.forward_raw(xd[:40]))
    assert np.max(np.abs(q32 - want[:40])) < 1e-4
    assert np.max(np.abs(q32 - p32[:40])) < 2e-6 * max(1.0, float(np.max(np.abs(want))))


def test_scoreinformed_batch_of_128_tiles_matches_oracle(tmp_path):
    """BASELINE configs[4]: score-conditioned masks, one batch of 128 four-channel tiles [128, 4, 30, 2049] through the
    whole score-informed path (7.66 s of audio, library tiler)."""
    from deepconvsep_amd import score
    F, N = 2049, 4096
    L = (25 + 1 + 127 * 5 - 2) * 512                        # shortest signal with 128 library tiles
    audio = synth_audio(L, seed=93)
    files = []
    for i in range(4):
        files.append("inst%d.txt" % i)
        (tmp_path / files[-1]).write_text(synth_score_text(60 + i, L / 44100.0 + 0.5, 40 + 5 * i, 64 + 6 * i))
    nframes = int(np.ceil(L / 512.0)) + 2
    melody = score.melody_table(files, str(tmp_path), nframes, 44100, 512, N)
    params = synth_params("bach10_si", 30, F, seed=5)
    sep = dcs.Separator("bach10_si", params, 0.3, 30, 25, 128, F, N, 512, dcs.blackmanharris, tiler='library')
    got = sep.separate_scoreinformed(audio, melody)
    want = pipeline.separate_scoreinformed(params, audio, melody, 0.3, 30, 25, 32, N, 512, dcs.blackmanharris)
    assert got.shape == want.shape == (4, L)
    assert np.max(np.abs(got - want)) < 1e-4
    assert np.max(np.abs(want)) > 1e-3
    # the reference's batch of 32 (predict_function2 is called per batch) gives the same result
    sep32 = dcs.Separator("bach10_si", params, 0.3, 30, 25, 32, F, N, 512, dcs.blackmanharris, tiler='library')
    assert np.max(np.abs(sep32.separate_scoreinformed(audio, melody) - got)) < 2e-6
    # the TRAINERS' semantics at the same size (masks / sum over instruments, soft masks x channel sum) and the
    # single-branch .pkl layout of trainCNNrwc_samp.py (the live part of the 17 arrays): 1e-4 against the oracle
    from deepconvsep_amd.arch import ARCHS, live_params
    _, params11 = live_params(ARCHS["bach10_si"], params)
    sep_t = dcs.Separator("bach10_si", params11, 0.3, 30, 25, 128, F, N, 512, dcs.blackmanharris, tiler='library',
                          score_normalise='sum', score_mixture='sum')
    assert sep_t.net.arch.name == "bach10_si1"
    got_t = sep_t.separate_scoreinformed(audio, melody)
    want_t = pipeline.separate_scoreinformed(params11, audio, melody, 0.3, 30, 25, 32, N, 512, dcs.blackmanharris,
                                             normalise='sum', mixture='sum', arch='bach10_si1')
    assert np.max(np.abs(got_t - want_t)) < 1e-4 and np.max(np.abs(want_t - want)) > 1e-3


# ------------------------------------------------------------------------------------------------ streams
def test_side_stream_context_needs_no_enclosing_stream_block():
    """A Separator bound to a side stream is called with torch's default stream current: the host->device copy, the
    kernels and the device->host copy are all ordered on the context's own stream."""
    import torch
    F, N = 513, 1024
    params = synth_params("dsd", 30, F, seed=2)
    audio = synth_audio(3 * 44100, seed=77)
    base = dcs.Separator("dsd", params, 0.3, 30, 25, 32, F, N, 512, np.hanning).separate(audio)
    side = torch.cuda.Stream()
    ctx2 = Context(stream=side)
    sep = dcs.Separator("dsd", params, 0.3, 30, 25, 32, F, N, 512, np.hanning, ctx=ctx2)
    assert torch.cuda.current_stream() != side
    for rep in range(4):                                     # eager, capture, replays
        # keep the default stream busy so that an unordered copy would race
        junk = torch.empty(1 << 24, device="cuda").normal_()
        got = sep.separate(audio)
        assert np.array_equal(got, base) or np.max(np.abs(got - base)) < 1e-6
        del junk
    tt = dcs.transformFFT(frameSize=N, hopSize=512, precision='float32')
    tt._plan = dcs.runtime.StftPlan(ctx2, N, 512, tt.window)
    mag, ph = tt.compute_file(audio, phase=True)
    assert np.max(np.abs(tt.compute_inverse(mag, ph)[:audio.size] - audio)) < 1e-5


def test_overlapadd_with_zero_overlap_lays_tiles_end_to_end():
    """overlapadd_multi accepts overlap == 0 in the reference (an empty ramp): plain concatenation."""
    from deepconvsep_amd.runtime import overlap_add
    ctx = default_context()
    rs = np.random.RandomState(4)
    out = rs.uniform(0, 1, (2, 5, 6, 9)).astype(np.float32)
    sep = ctx.to_host(overlap_add(ctx, ctx.to_device(out, np.float32), 0))
    assert sep.shape == (2, 5 * 6 + 6, 9)
    assert np.array_equal(sep[:, :30], out.reshape(2, 30, 9)) and not sep[:, 30:].any()


def test_separate_many_confines_a_clip_without_tiles(tmp_path):
    F, N = 513, 1024
    params = synth_params("dsd", 30, F, seed=2)
    sep = dcs.Separator("dsd", params, 0.3, 30, 25, 32, F, N, 512, np.hanning)
    clips = [synth_audio(30000, seed=1), synth_audio(300, seed=2), synth_audio(31000, seed=3)]
    res = sep.separate_many(clips, on_error='return')
    assert isinstance(res[1], Exception)
    assert res[0].shape == (4, 30000) and res[2].shape == (4, 31000)
    assert np.max(np.abs(res[0] - sep.separate(clips[0]))) < 5e-6
    with pytest.raises(ValueError):
        sep.separate_many([np.zeros((1000, 2))])             # a stereo array is not silently interleaved


# ------------------------------------------------------------------------------------------------ multi-GPU code paths
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_bench_two_ranks_on_this_gpu_gather_is_exact():
    """bench.py --gpus 2 as the driver launches it (torch.distributed.run, one process per rank), both ranks on this
    GPU with gloo standing in for RCCL (RCCL refuses two ranks on one device).  DCS_BENCH_CHECK_GATHER makes every rank
    verify that the gathered int16 PCM holds each rank's own PCM (exchanged out of band) bit for bit."""
    env = dict(os.environ, DCS_BENCH_SAME_DEVICE="1", DCS_BENCH_CHECK_GATHER="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6",
           "--warmup", "2", "--full", "--sat-tiles", "0", "--min-time", "0.02", "--legs", "", "--gather", "allgather"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["steps"] == 6 and line["value"] > 0
    assert line["gather_check"] == "ok"
    assert line["scaling"] == "weak" and line["cpu_baseline"] is None
    assert line["gather"]["mode"] == "allgather" and line["gather"]["ms_per_group_collective_alone"] > 0
    # a round of ONE launch group with N > 1 goes out as two half-groups, B's kernels ordered behind A's (round 6)
    assert line["gather"]["pipelined_half_groups"] is True and line["config"]["launch_groups_per_round"] == [3, 3]
    assert line["parity_check"]["ok"] is True


def _long_file_worker(rank, world, port, audio, params, ret):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from deepconvsep_amd.dist import separate_long_file
    sep = dcs.Separator("dsd", params, 0.3, 30, 25, 32, 513, 1024, 512, np.hanning)
    out = separate_long_file(sep.separate, audio, 1024, 512, 30, 25)        # the HIP path is the per-rank worker
    if rank == 0:
        ret["pcm"] = out.numpy()
    dist.destroy_process_group()


def _long_file_device_worker(rank, world, port, audio, params, ret):
    """As _long_file_worker, but the per-rank separation is Network.separate on DEVICE tensors and the collective runs on
    them -- the branch RCCL takes on a multi-GPU node (dist.py: torch tensors in, all_gather of device buffers)."""
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from deepconvsep_amd.dist import separate_long_file
    from deepconvsep_amd.runtime import default_context
    sep = dcs.Separator("dsd", params, 0.3, 30, 25, 32, 513, 1024, 512, np.hanning)
    ctx = default_context()
    dev = ctx.to_device(audio, np.float32)

    def fn(seg):                                        # seg: a device slice of the signal
        return sep.net.separate(sep.plan, seg.contiguous(), 25, sep.tiler, 0.3)
    try:
        out = separate_long_file(fn, dev, 1024, 512, 30, 25)
        ret["device"] = bool(out.is_cuda)
        if rank == 0:
            ret["pcm"] = out.cpu().numpy()
    except RuntimeError as exc:                          # a gloo build without device-tensor collectives
        ret["error"] = str(exc)
    dist.destroy_process_group()


def test_long_file_sharded_over_two_ranks_on_device_tensors():
    import torch.multiprocessing as mp
    params = synth_params("dsd", 30, 513, seed=2)
    audio = synth_audio(6 * 44100, seed=8)
    whole = dcs.Separator("dsd", params, 0.3, 30, 25, 32, 513, 1024, 512, np.hanning).separate(audio)
    ctxm = mp.get_context("spawn")
    mgr = ctxm.Manager()
    ret = mgr.dict()
    mp.spawn(_long_file_device_worker, args=(2, _free_port(), audio, params, ret), nprocs=2, join=True)
    if "error" in ret:
        pytest.skip("gloo cannot gather device tensors here: %s" % ret["error"][:200])
    assert ret["device"] is True
    got = ret["pcm"]
    assert got.shape == whole.shape
    assert np.max(np.abs(got - whole)) < 2e-6


@pytest.mark.parametrize("mode", ["root", "none"])
def test_bench_two_ranks_gather_modes(mode):
    """bench.py --gpus 2 --gather root / none: the root gather of the north-star ("final gather") and the replica mode,
    with the per-launch-group split of compute and collective in the line."""
    env = dict(os.environ, DCS_BENCH_SAME_DEVICE="1", MASTER_ADDR="127.0.0.1")
    if mode == "root":
        env["DCS_BENCH_CHECK_GATHER"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "6",
           "--warmup", "2", "--full", "--sat-tiles", "0", "--min-time", "0.02", "--legs", "", "--gather", mode]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    if r.returncode != 0 and mode == "root" and "gloo" in (r.stderr + r.stdout).lower() and "gather" in (r.stderr + r.stdout).lower():
        pytest.skip("gloo cannot gather device tensors to a root here")
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["value"] > 0
    assert line["gather"]["mode"] == mode and line["gather"]["round_ms_without_gather"] > 0
    if mode == "root":
        assert line["gather_check"] == "ok" and line["gather"]["ms_per_group_collective_alone"] > 0
    assert line["parity_check"]["ok"] is True and line["parity_check"]["ranks"] == 2


def test_long_file_sharded_over_two_ranks_with_the_hip_separator():
    """deepconvsep_amd.dist.separate_long_file over two processes (gloo), each separating its halo-extended share
    with Separator.separate on this GPU: the gathered result equals the single-process separation."""
    import torch.multiprocessing as mp
    params = synth_params("dsd", 30, 513, seed=2)
    audio = synth_audio(6 * 44100, seed=8)
    whole = dcs.Separator("dsd", params, 0.3, 30, 25, 32, 513, 1024, 512, np.hanning).separate(audio)
    ctxm = mp.get_context("spawn")
    mgr = ctxm.Manager()
    ret = mgr.dict()
    mp.spawn(_long_file_worker, args=(2, _free_port(), audio, params, ret), nprocs=2, join=True)
    got = ret["pcm"]
    assert got.shape == whole.shape
    assert np.max(np.abs(got - whole)) < 2e-6


def test_dcs_gather_through_the_c_abi_with_a_one_rank_rccl_communicator():
    """dcs_gather (include/dcs.h) on a communicator of ONE rank -- all this box can host (RCCL refuses two ranks
    on one device): librccl is dlopen'ed by libdcs, the all-gather and the root form both deliver the shard bit for bit,
    int16 PCM travels as bytes, and the argument checks hold.  N > 1 ranks stay unmeasured."""
    import torch
    from deepconvsep_amd import _lib
    from deepconvsep_amd.dist import RcclComm
    from deepconvsep_amd.runtime import default_context
    ctx = default_context()
    try:
        comm = RcclComm(1, 0, RcclComm.unique_id())
    except (NotImplementedError, RuntimeError, OSError) as e:
        pytest.skip("no usable librccl here: %s" % e)
    try:
        pcm = torch.rand((4, 70001), device="cuda") * 2 - 1
        pcm16 = torch.empty(pcm.shape, dtype=torch.int16, device="cuda")
        _lib.check(ctx._lib.dcs_pcm_to_int16(ctx._h, ctypes.c_void_p(pcm.data_ptr()), pcm.numel(), ctypes.c_void_p(pcm16.data_ptr())))
        full = comm.gather(ctx, pcm16, root=-1)
        torch.cuda.synchronize()
        assert tuple(full.shape) == (1, 4, 70001) and torch.equal(full[0], pcm16)
        full2 = torch.zeros_like(full)
        assert comm.gather(ctx, pcm16, full2, root=0) is full2
        torch.cuda.synchronize()
        assert torch.equal(full2[0], pcm16)
        want = (pcm.cpu().numpy().astype(np.float64) * 32767).astype(np.int16)   # the scripts' float64 product, truncated (separate_dsd.py:307-309)
        assert np.array_equal(full2[0].cpu().numpy(), want)
        with pytest.raises(ValueError):
            comm.gather(ctx, pcm16, full2, root=3)                      # no such rank
        with pytest.raises(ValueError):
            _lib.check(ctx._lib.dcs_gather(ctx._h, None, ctypes.c_void_p(pcm16.data_ptr()), 16, ctypes.c_void_p(full2.data_ptr()), -1))
    finally:
        comm.close()


# ------------------------------------------------------------------ multi-GPU paths that switch themselves on
# The build box and the driver's GPU tier have ONE MI355X, so everything above runs two ranks on one device over gloo.  The
# tests below need nothing but a second GPU: on a multi-GPU node they run the real thing -- backend nccl (= RCCL over xGMI),
# one device per rank, dcs_gather on a two-rank communicator -- and skip here.  No scaling curve is implied by them.
def _gpu_count():
    try:
        import torch
        return torch.cuda.device_count()
    except Exception:
        return 0


needs_two_gpus = pytest.mark.skipif(_gpu_count() < 2, reason="needs two GPUs (RCCL refuses two ranks on one device)")


def _run_bench(n, extra, env_extra, timeout=900):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", **env_extra)
    env.pop("DCS_BENCH_SAME_DEVICE", None)
    args = ["--gpus", str(n), "--steps", "6", "--warmup", "2", "--full", "--sat-tiles", "0", "--min-time", "0.02", "--legs", "",
            "--no-cpu-baseline", "--no-host-fed", "--no-cli"] + extra
    if n > 1:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
               "127.0.0.1", "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py")] + args
    else:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py")] + args
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_bench_gather_code_path_with_a_world_of_one_rank():
    """What a 1-GPU box can run of the N > 1 leg on the REAL backend: DCS_BENCH_FORCE_GATHER makes bench.py --gpus 1 convert
    every launch group's PCM to int16 and push it through the collective of a one-rank world -- with --gather-impl dcs that is
    dcs_gather (the C-ABI entry of SURVEY 8b) on an RCCL communicator per HIP stream, inside the timed region.  Four variants
    (all-gather / root through dcs_gather, all-gather through torch.distributed, and the serial one-group schedule of rounds
    2 - 5 with --no-pipeline), four bench.py processes side by side."""
    variants = [("dcs", "allgather", False), ("dcs", "root", False), ("torch", "allgather", False), ("dcs", "root", True)]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", DCS_BENCH_FORCE_GATHER="1", DCS_BENCH_CHECK_GATHER="1")
    env.pop("DCS_BENCH_SAME_DEVICE", None)
    procs = []
    for i, (impl, mode, serial) in enumerate(variants):
        # (the oracle check of the timed launches' output -- seconds of float64 CPU work -- once: the compute path is the same in all four)
        args = ["--gpus", "1", "--steps", "6", "--warmup", "2", "--full", "--sat-tiles", "0", "--min-time", "0.02", "--legs", "",
                "--no-cpu-baseline", "--no-host-fed", "--no-cli", "--gather", mode, "--gather-impl", impl] + (["--no-pipeline"] if serial else []) + \
               (["--no-parity-check"] if i else [])
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True, cwd=ROOT))
    for (impl, mode, serial), pr in zip(variants, procs):
        out, err = pr.communicate(timeout=900)
        assert pr.returncode == 0, (impl, mode, serial, out[-2000:], err[-4000:])
        line = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
        assert line["n_gpus"] == 1 and line["value"] > 0 and line["gather_check"] == "ok", (impl, mode, serial)
        assert line["gather"]["pipelined_half_groups"] is (not serial)
        assert line["config"]["launch_groups_per_round"] == ([6] if serial else [3, 3])
        assert line["gather"]["mode"] == mode and line["gather"]["impl"].startswith("dcs_gather" if impl == "dcs" else "torch.distributed")
        assert line["gather"]["ms_per_group_collective_alone"] > 0
        if (impl, mode, serial) == variants[0]:
            assert line["parity_check"]["ok"] is True


def test_bench_times_exactly_the_given_steps_and_dumps_the_last_step(tmp_path):
    """bench.py --gpus 1 --steps 5: one timed round of exactly 5 steps (one launch group of 5 batches on lane 0), and
    --dump-outputs writes the PCM of its last batch -- the audio of clip 4 of lane 0 -- equal to a separation of that audio."""
    import bench
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--sat-tiles", "0",
           "--legs", "", "--no-cpu-baseline", "--no-host-fed", "--no-cli", "--no-parity-check", "--dump-outputs", str(tmp_path)]
    env = dict(os.environ)
    for k in ("DCS_BENCH_SAME_DEVICE", "DCS_BENCH_FORCE_GATHER"):
        env.pop(k, None)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = json.loads(r.stdout.splitlines()[-1])
    assert line["steps"] == 5 and line["rounds"] == 1 and line["ms_per_step"] > 0
    assert line["config"]["launch_groups_per_round"] == [5]
    got = np.load(str(tmp_path / "pcm.npy"))
    L = bench.samples_for_tiles(32)
    assert got.dtype == np.float32 and got.shape == (4, L)
    audio = synth_audio(L, seed=100 + 4)
    want = dcs.Separator("dsd", synth_params("dsd", 30, 1025, seed=2), 0.3, 30, 25, 32, 1025, 2048, 512,
                         np.hanning).separate(audio)
    assert np.max(np.abs(got - want)) < 1e-4


@needs_two_gpus
@pytest.mark.parametrize("impl,mode", [("torch", "allgather"), ("torch", "root"), ("dcs", "allgather"), ("dcs", "root")])
def test_bench_two_gpus_over_rccl_gather_is_exact(impl, mode):
    """bench.py --gpus 2 exactly as the driver launches it, backend nccl, one GPU per rank: the gathered int16 PCM holds
    every rank's own PCM bit for bit (DCS_BENCH_CHECK_GATHER), through torch.distributed and through dcs_gather."""
    line = _run_bench(2, ["--gather", mode, "--gather-impl", impl], {"DCS_BENCH_CHECK_GATHER": "1"})
    assert line["n_gpus"] == 2 and line["value"] > 0 and line["gather_check"] == "ok"
    assert line["gather"]["mode"] == mode and line["gather"]["round_ms_without_gather"] > 0
    assert line["parity_check"]["ok"] is True and line["parity_check"]["ranks"] == 2


def _rccl_pair_worker(rank, world, port, ret):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(rank)
    dist.init_process_group("gloo", rank=rank, world_size=world)         # side channel for the unique id only
    from deepconvsep_amd.dist import RcclComm
    from deepconvsep_amd.runtime import Context, pcm_to_int16
    ctx = Context(rank)
    comm = RcclComm.from_process_group(device=ctx)
    try:
        g = torch.Generator(device="cpu").manual_seed(100 + rank)
        pcm = (torch.rand((4, 70001), generator=g) * 2 - 1).to(ctx.device)
        mine = pcm_to_int16(ctx, pcm)
        full = comm.gather(ctx, mine, root=-1)                               # every rank receives
        at_root = comm.gather(ctx, mine, root=1)                             # rank 1 is the writer
        torch.cuda.synchronize()
        ret["all_%d" % rank] = full.cpu().numpy()
        ret["mine_%d" % rank] = mine.cpu().numpy()
        ret["root_%d" % rank] = None if at_root is None else at_root.cpu().numpy()
    finally:
        comm.close()
        dist.destroy_process_group()


@needs_two_gpus
def test_dcs_gather_on_a_two_rank_rccl_communicator():
    """dcs_gather (include/dcs.h) with TWO ranks on two GPUs: the all-gather form on every rank and the root form on the
    writer deliver both ranks' int16 PCM bit for bit, in rank order; a non-root rank of the root form gets nothing."""
    import torch.multiprocessing as mp
    ctxm = mp.get_context("spawn")
    ret = ctxm.Manager().dict()
    mp.spawn(_rccl_pair_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    want = np.stack([ret["mine_0"], ret["mine_1"]])
    assert not np.array_equal(want[0], want[1]) and want.dtype == np.int16
    for r in range(2):
        assert np.array_equal(ret["all_%d" % r], want)
    assert ret["root_0"] is None and np.array_equal(ret["root_1"], want)


def _long_file_nccl_worker(rank, world, port, audio, params, ret):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(rank)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
    from deepconvsep_amd.dist import separate_long_file
    from deepconvsep_amd.runtime import default_context
    sep = dcs.Separator("dsd", params, 0.3, 30, 25, 32, 513, 1024, 512, np.hanning, device=rank)
    dev = default_context(rank).to_device(audio, np.float32)

    def fn(seg):
        out = sep.net.separate(sep.plan, seg.contiguous(), 25, sep.tiler, 0.3)
        sep.ctx.synchronize()                                  # the collective runs on torch's stream
        return out
    out = separate_long_file(fn, dev, 1024, 512, 30, 25)
    ret["device_%d" % rank] = int(out.device.index)
    if rank == 0:
        ret["pcm"] = out.cpu().numpy()
    dist.destroy_process_group()


@needs_two_gpus
def test_long_file_sharded_over_two_gpus_with_nccl_device_tensors():
    """separate_long_file over backend nccl: each rank separates its halo-extended share on ITS GPU, the owned PCM ranges are
    all-gathered as device tensors over RCCL; equals the single-GPU separation."""
    import torch.multiprocessing as mp
    params = synth_params("dsd", 30, 513, seed=2)
    audio = synth_audio(6 * 44100, seed=8)
    whole = dcs.Separator("dsd", params, 0.3, 30, 25, 32, 513, 1024, 512, np.hanning).separate(audio)
    ctxm = mp.get_context("spawn")
    ret = ctxm.Manager().dict()
    mp.spawn(_long_file_nccl_worker, args=(2, _free_port(), audio, params, ret), nprocs=2, join=True)
    assert ret["device_0"] == 0 and ret["device_1"] == 1
    assert ret["pcm"].shape == whole.shape and np.max(np.abs(ret["pcm"] - whole)) < 2e-6

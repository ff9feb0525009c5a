"""Shared by tests/test_stft_ref_cpu.py and tests/test_gpu_stft_kernels.py (test infrastructure): the transform kernels of
csrc/fft.hip and csrc/fft_wave.hip held directly to float64.

* the float64 reference (``oracle.stft_np``) and a float32 restatement of it (complex64 spectrum, ``torch.fft`` on the CPU,
  float32 window and accumulation in frame order) whose own distance from float64 is the yardstick of the device's;
* the error measure of the inverse, ``max |got - want| * norm / max(norm)`` with ``norm`` the float64 sum of w^2: the raw
  error is amplified by ``1 / norm`` at the Hann edges and past the last frame's centre, this one is not;
* the six-int64 clip table of csrc/dcs_internal.h in both layouts;
* the launchers' arithmetic under the forcing switches (``launch_inv`` / ``launch_fwd`` of fft_wave.hip, ``launch_inverse``
  of fft.hip), so that a case can say which kernel it must reach and ``regimes`` which branches of it;
* the case tables of both test files.
"""
import numpy as np

from oracle import stft_np

PRE_DIV = 0.3
CHAIN_WAVES = 8                       # kChainWaves
K_THREADS = 256                       # kThreads of the block kernels
# kernel codes of include/dcs.h (dcs_debug_stft_last_kernel)
FWD_BLOCK, FWD_WAVE1, FWD_WAVE4 = 1, 2, 3
INV_BLOCK, INV_RING, INV_SEQ, INV_SEQ_STAGED, INV_CHAIN = 1, 2, 3, 4, 5

# the project's bounds (tests/test_gpu_parity.py: inverse 1e-5, forward magnitudes 2e-5, complex spectrum 4e-5, float64 1e-11)
BOUND_INV, BOUND_MAG, BOUND_CPX, BOUND_F64 = 1e-5, 2e-5, 4e-5, 1e-11
FACTOR = 4.0                          # a reordered float32 sum against the in-order one (tests/test_gpu_mwf.py)
# |X / |X|| - 1 in float32: xr * rcp(ax) and xi * rcp(ax) with ax = sqrt(xr^2 + xi^2) -- two roundings in the sum of squares,
# one in the square root (1 ulp), one in the reciprocal (1 ulp), one per product: seven half-ulps of 2^-24 on either
# component at the most, 4.2e-7; twice that leaves room for the test's own float32 hypot
BOUND_UNIT = 16 * 2.0 ** -24

SWITCHES = {
    "none": {},
    "block": {"DCS_FFT_BLOCK": "1"},
    "wave1": {"DCS_STFT_WAVE_MIN": "1"},
    "seq1": {"DCS_ISTFT_CHAIN": "0", "DCS_ISTFT_SEQ_HOPS": "1"},
    "seq5": {"DCS_ISTFT_CHAIN": "0", "DCS_ISTFT_SEQ_HOPS": "5"},
    "chain3": {"DCS_ISTFT_CHAIN": "3"},
    "chain7": {"DCS_ISTFT_CHAIN": "7"},
    "stage": {"DCS_ISTFT_STAGE_MIN": "1"},
}


def window(N):
    return np.hanning(N)


# ------------------------------------------------------------------------------------------------ references
def forward_ref64(audio, N, hop):
    """X / sqrt(N), complex128 [T, N/2+1]"""
    return stft_np.stft_norm(np.asarray(audio, dtype=np.float64), window(N), float(hop), float(N)) / np.sqrt(N)


def forward_ref32(audio, N, hop):
    """the same in float32: float32 samples times the float32 window, torch's float32 rfft, one float32 division"""
    import torch
    x = np.asarray(audio, dtype=np.float32)
    T = stft_np.frame_count(x.size, hop)
    padded = np.zeros((T - 1) * hop + N, dtype=np.float32)
    padded[N // 2:N // 2 + x.size] = x
    idx = np.arange(T)[:, None] * hop + np.arange(N)[None, :]
    frames = padded[idx] * window(N).astype(np.float32)[None, :]
    X = torch.fft.rfft(torch.from_numpy(frames), n=N, dim=1).numpy()
    return (X / np.float32(np.sqrt(N))).astype(np.complex64)


def inverse_norm(N, hop, T, n):
    """float64 sum of w^2 over the frames that cover output sample p, p < n (before zeros become ones)"""
    w2 = window(N) ** 2
    norm = np.zeros(hop * (T - 1) + N)
    for t in range(T):
        norm[t * hop:t * hop + N] += w2
    norm = norm[N // 2:]
    out = np.zeros(n)
    m = min(n, norm.size)
    out[:m] = norm[:m]
    return out


def inverse_ref64(mag, unit, N, hop, pre_div=PRE_DIV, phase=None):
    """istft_norm of (mag / pre_div) * sqrt(N) * unit (or exp(j phase)), full length hop (T - 1) + N / 2; mag [T, bins]"""
    ph = np.asarray(unit, dtype=np.complex128) if phase is None else np.exp(1j * np.asarray(phase, dtype=np.float64))
    X = (np.asarray(mag, dtype=np.float64) / pre_div) * np.sqrt(N) * ph
    w = window(N)
    return stft_np.istft_norm(X, w, w, float(hop), float(N))


def inverse_ref32(mag, unit, N, hop, pre_div=PRE_DIV, phase=None):
    """the same in float32: complex64 spectrum (imaginary parts at DC / Nyquist dropped as irfft drops them), torch's float32
    irfft, float32 window products added frame by frame, float32 normaliser added frame by frame, one float32 division"""
    import torch
    mag = np.asarray(mag, dtype=np.float32)
    T = mag.shape[0]
    a = (mag / np.float32(pre_div)) * np.float32(np.sqrt(N))
    if phase is None:
        X = (a * np.asarray(unit, dtype=np.complex64)).astype(np.complex64)
    else:
        ph = np.asarray(phase, dtype=np.float32)
        X = (a * np.cos(ph) + 1j * (a * np.sin(ph))).astype(np.complex64)
    X[:, 0] = X[:, 0].real
    X[:, N // 2] = X[:, N // 2].real
    frames = torch.fft.irfft(torch.from_numpy(X), n=N, dim=1).numpy().astype(np.float32)
    w = window(N).astype(np.float32)
    w2 = (window(N) ** 2).astype(np.float32)
    acc = np.zeros(hop * (T - 1) + N, dtype=np.float32)
    norm = np.zeros_like(acc)
    for t in range(T):
        acc[t * hop:t * hop + N] += w * frames[t]
        norm[t * hop:t * hop + N] += w2
    acc, norm = acc[N // 2:], norm[N // 2:]
    norm[norm == 0] = 1
    return acc / norm


def weighted_error(got, want, norm):
    """max_p |got[p] - want[p]| * norm[p] / max(norm); 0.0 for empty input"""
    got, want, norm = (np.asarray(v, dtype=np.float64) for v in (got, want, norm))
    if got.size == 0:
        return 0.0
    top = float(norm.max())
    return float(np.max(np.abs(got - want) * norm) / top) if top > 0 else 0.0


# ------------------------------------------------------------------------------------------------ clip table
CLIP_TAB = 6                          # kDcsClipTab: {samples, frames, tiles, row offset, tile offset, rows}


def clip_table(lengths, hop, compact):
    """int64 [n_clips, 6]; row offset -1 (the caller's uniform pitch) or the clips' frames packed back to back"""
    tab = np.zeros((len(lengths), CLIP_TAB), dtype=np.int64)
    row = 0
    for c, n in enumerate(lengths):
        T = stft_np.frame_count(n, hop)
        tab[c] = (n, T, 0, row if compact else -1, 0, T)
        row += T
    return tab


# ------------------------------------------------------------------------------------------------ launcher arithmetic
def n_blocks(N, hop, n_out):
    return (n_out + N // 2 + hop - 1) // hop


def n_out_for_blocks(N, hop, nb):
    """the longest output with nb hop-blocks"""
    return nb * hop - N // 2


def wave_inverse(N, hop, block_forced=False):
    return (not block_forced) and N in (1024, 2048, 4096) and N % hop == 0 and hop % 2 == 0


def seq_shape(N, hop):
    """the barrier-free kernels: N <= 2048, 2 or 4 hop-blocks per frame, hop / 2 a multiple of 64"""
    return N in (1024, 2048) and N % hop == 0 and N // hop in (2, 4) and (hop // 2) % 64 == 0


def chain_geometry(N, hop, n_out, LC):
    R = N // hop
    LC = max(LC, R - 1, 1)
    Sb = CHAIN_WAVES * LC - (R - 1)
    nb = n_blocks(N, hop, n_out)
    Gc = 1 if nb <= R - 1 else (nb - (R - 1) + Sb - 1) // Sb
    first = Sb + R - 1                                        # blocks of the first workgroup of a source
    last = nb if Gc == 1 else nb - first - (Gc - 2) * Sb      # blocks of the last one
    return dict(R=R, LC=LC, Sb=Sb, n_blocks=nb, Gc=Gc, last_blocks=last)


def seq_chunks(N, hop, n_out, Cs):
    return (n_blocks(N, hop, n_out) + Cs - 1) // Cs


def ring_slots(N, hop):
    s = 8
    while s < N // hop + 3:
        s *= 2
    return s


def ring_lds(N, hop):
    M = N // 2
    return (M + 1 + 4 * (M + M // 32) + M + ring_slots(N, hop) * (hop // 2)) * 8 + hop * 4


def block_inverse_plan(N, hop, n_out, n_src, n_cu, size=4):
    """launch_inverse of fft.hip: dict(need, PF, tw_lds, C, halved, capped, lds) or None where it returns DCS_EUNSUPPORTED"""
    M = N // 2
    hops = (n_out + M + hop - 1) // hop
    R = (N + hop - 1) // hop
    C = hops * n_src // n_cu
    capped = C > 4 * R
    C = max(1, min(C, 4 * R))
    fixed_tw, fixed_notw = (3 * M + 2) * 2 * size, (2 * M + 1) * 2 * size
    tw_lds = fixed_tw + hop * size <= 64 * 1024
    fixed = fixed_tw if tw_lds else fixed_notw
    lds, halved = fixed + C * hop * size, False
    while lds > 48 * 1024 and C > 1:
        C, halved = C // 2, True
        lds = fixed + C * hop * size
    if lds > 160 * 1024:
        return None
    need = (M + 1 + K_THREADS - 1) // K_THREADS
    PF = 3 if need <= 3 else 5 if need <= 5 else 9 if need <= 9 else 17
    return dict(need=need, PF=PF, tw_lds=tw_lds, C=C, halved=halved, capped=capped, lds=lds)


def forward_block_tw_lds(N, size=4):
    return (3 * (N // 2) + 1) * 2 * size <= 64 * 1024


def expected_inverse(case, n_cu=256):
    """(kernel code, param or None) of an inverse case under its switch set.  The forced switches fix the choice; without
    them it holds for inputs this short on any chip of at least 8 CUs: every wave gets one hop-block (Cs = 1), so the
    chain's LC = max(R - 1, 1) is shorter than the seq kernel's Cs + R - 1 and all its workgroups are resident."""
    sw, N, hop = case["switch"], case["N"], case["hop"]
    unit = not case.get("phase_input", False)
    if not wave_inverse(N, hop, sw == "block"):
        return INV_BLOCK, None
    if not seq_shape(N, hop):
        return INV_RING, None
    R = N // hop
    S = case["n_src"] * case["n_clips"]
    nb = n_blocks(N, hop, case["n_out"])
    forced_cs = {"seq1": 1, "seq5": 5}.get(sw)
    Cs = forced_cs or max(1, -(-nb * S // (n_cu * 8)))
    stage_min = 1 if sw == "stage" else 16
    staged = (Cs >= stage_min and unit and case["ld"] == N // 2 + 4 and case["n_src"] % 4 == 0 and
              case["src_stride"] % 4 == 0 and case["unit_clip_stride"] % 2 == 0 and case.get("mag_off", 0) % 4 == 0)
    if staged:
        return INV_SEQ_STAGED, Cs
    if unit and sw not in ("seq1", "seq5"):
        if sw in ("chain3", "chain7"):
            return INV_CHAIN, max(int(sw[-1]), R - 1)
        LC = max(R - 1, 1)
        if LC < Cs + R - 1:
            return INV_CHAIN, LC
    return INV_SEQ, Cs


# ------------------------------------------------------------------------------------------------ inputs
def ld_of(N, mode):
    bins = N // 2 + 1
    return {"bins": bins, "bins3": bins + 3, "M4": N // 2 + 4, "M8": N // 2 + 8}[mode]


def inverse_inputs(case):
    """mag float32 [n_clips * n_src, T, bins], unit complex64 [n_clips, T, bins].  Not a consistent STFT: magnitudes
    uniform in [0, 0.3] times a random mask with exactly-zero rows and bins, phasors at random angles, bins 0 and N / 2
    with an imaginary part that the transform must ignore.  `onehot`: every frame but that one is zero."""
    N, T = case["N"], case["T"]
    bins = N // 2 + 1
    S, nc = case["n_src"] * case["n_clips"], case["n_clips"]
    rs = np.random.RandomState(case["seed"])
    mag = (0.3 * rs.uniform(0, 1, (S, T, bins)) * rs.uniform(0, 1, (S, T, bins))).astype(np.float32)
    if T >= 8:
        mag[:, rs.randint(0, T, T // 8)] = 0
    mag[:, :, rs.randint(0, bins, max(1, bins // 16))] = 0
    ang = rs.uniform(-np.pi, np.pi, (nc, T, bins))
    unit = (np.cos(ang) + 1j * np.sin(ang)).astype(np.complex64)
    if case.get("onehot") is not None:
        keep = mag[:, case["onehot"]].copy()
        keep[keep == 0] = np.float32(0.1)
        mag[:] = 0
        mag[:, case["onehot"]] = keep
    return mag, unit


SILENCE_FACTOR = 4


def forward_audio(case):
    """float64 [n_clips, n_samples]: synth_audio (sinusoids + noise quantised to int16); where the signal is long enough, N + hop
    samples of digital silence from n / 3 on"""
    from deepconvsep_amd.synth import synth_audio
    n = case["n_samples"]
    a = np.stack([np.asarray(synth_audio(n, seed=case["seed"] + c, silence=False), dtype=np.float64).reshape(-1)
                  for c in range(case["n_clips"])])
    N, hop = case["N"], case["hop"]
    if n >= SILENCE_FACTOR * (N + hop):
        a[:, n // 3:n // 3 + N + hop] = 0                      # N + hop zeros hold one whole frame wherever they start
    for c, m in enumerate(case.get("lengths") or []):
        a[c, m:] = 0
    return a


# ------------------------------------------------------------------------------------------------ the case tables
def _inv(name, switch, N, hop, n_out=None, nb=None, T=None, n_src=1, n_clips=1, ld="bins", out_pad=0, lengths=None,
         table=None, mag_off=0, ucs_odd=False, onehot=None, seed=None, cu_cap=False):
    """n_out directly, or the longest output of nb hop-blocks; T = dcs_frame_count(n_out) unless given"""
    if lengths:
        n_out = max(lengths)
    elif n_out is None:
        n_out = n_out_for_blocks(N, hop, nb)
    T = T or stft_np.frame_count(n_out, hop)
    assert 0 < n_out <= stft_np.inverse_length(T, hop, N), name
    ldv = ld_of(N, ld)
    ucs = T * ldv + (1 if ucs_odd else 0)
    c = dict(name=name, switch=switch, N=N, hop=hop, n_out=n_out, T=T, n_src=n_src, n_clips=n_clips, ld=ldv, ld_mode=ld,
             out_stride=n_out + out_pad, out_pad=out_pad, lengths=lengths, table=table, mag_off=mag_off, src_stride=T * ldv,
             unit_clip_stride=ucs, onehot=onehot, cu_cap=cu_cap,
             seed=seed if seed is not None else (abs(hash_name(name)) % 100000))
    # the public phase-input entry can express it: one clip, dense outputs, no table, aligned as torch allocates
    c["public"] = n_clips == 1 and not lengths and out_pad == 0 and mag_off == 0 and onehot is None and not cu_cap
    return c


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % 1000003
    return h


def ragged_lengths(hop):
    return [1, 20 * hop - 1, 37 * hop + 13]


def inverse_cases():
    cs = []
    add = lambda *a, **k: cs.append(_inv(*a, **k))
    # ---- chain, R = 2, LC = 3: Sb = 23; the last workgroup owns 0 (there is none), 1 or 2 blocks.  With hop = N / 2 an output
    # of one sample already has two hop-blocks, so "at most R - 1 blocks" cannot occur at R = 2 (it does at R = 4 below)
    for nb in (2, 24, 25, 26):
        add("chain3_r2_nb%d" % nb, "chain3", 1024, 512, nb=nb, n_src=2)
    add("chain3_r2_T1", "chain3", 1024, 512, n_out=300, T=1)
    # ---- chain, R = 4: default LC = 3 (Sb = 21) and LC = 7 (Sb = 53), n_blocks at R - 1 + k Sb and +- 1
    for N, hop in ((2048, 512), (1024, 256)):
        for sw, Sb in (("none", 21), ("chain7", 53)):
            for d in (-1, 0, 1):
                add("%s_r4_%d_%d_nb%+d" % (sw if sw != "none" else "chain", N, hop, d), sw, N, hop, nb=3 + Sb + d,
                    n_src=2 if d else 1)
    add("chain_r4_le_rm1_blocks", "none", 1024, 256, n_out=200)            # 3 blocks = R - 1
    add("chain_r4_T1", "none", 2048, 512, n_out=700, T=1)
    # ---- workgroup -> (unit, source): n_units = n_clips * Gc in {1, 7, 8, 9}, sources per clip in {1, 3, 4}
    for sw in ("chain3", "none"):
        for n_clips, spc in ((1, 3), (7, 1), (7, 4), (8, 3), (9, 4), (9, 1)):
            add("%s_units%d_spc%d" % (sw if sw != "none" else "chain", n_clips, spc), sw, 1024, 512, nb=6, n_src=spc,
                n_clips=n_clips)
    add("chain3_units2x4_spc3", "chain3", 1024, 512, nb=80, n_src=3, n_clips=2)    # Gc = 4: two clips of four runs each
    # ---- odd n_out: odd sources start on 4-byte boundaries only; then a gap between the sources
    for sw, N, hop in (("chain3", 1024, 512), ("none", 2048, 512), ("seq5", 1024, 256), ("none", 4096, 512), ("block", 1024, 512)):
        add("%s_odd_%d_%d" % (sw, N, hop), sw, N, hop, n_out=25 * hop + 1, n_src=3)
        add("%s_oddgap_%d_%d" % (sw, N, hop), sw, N, hop, n_out=25 * hop + 1, n_src=3, out_pad=3)
    # ---- ragged: three clips, both table layouts
    for sw, N, hop in (("chain3", 1024, 512), ("none", 2048, 512), ("seq1", 1024, 256), ("seq5", 2048, 512), ("stage", 2048, 512)):
        for table in ("uniform", "compact"):
            add("%s_ragged_%s_%d_%d" % (sw, table, N, hop), sw, N, hop, lengths=ragged_lengths(hop), n_clips=3,
                n_src=4 if sw == "stage" else 2, table=table, ld="M4" if sw == "stage" else "bins", out_pad=3)
    # ---- seq plain: n_chunks * n_src not a multiple of 4
    for sw in ("seq1", "seq5"):
        for N, hop in ((1024, 512), (2048, 512), (1024, 256)):
            add("%s_%d_%d" % (sw, N, hop), sw, N, hop, nb=27, n_src=3)
    # ---- seq staged and its preconditions, one broken at a time
    for N, hop in ((2048, 512), (1024, 512)):
        add("stage_%d_%d_src4" % (N, hop), "stage", N, hop, nb=27, n_src=4, ld="M4")
        add("stage_%d_%d_src8" % (N, hop), "stage", N, hop, nb=27, n_src=8, ld="M4")
    add("stage_2clips", "stage", 2048, 512, nb=27, n_src=4, n_clips=2, ld="M4")
    add("stage_broken_nsrc3", "stage", 2048, 512, nb=27, n_src=3, ld="M4")
    add("stage_broken_ldM8", "stage", 2048, 512, nb=27, n_src=4, ld="M8")
    add("stage_broken_magoff", "stage", 2048, 512, nb=27, n_src=4, ld="M4", mag_off=1)
    add("stage_broken_ucs_odd", "stage", 2048, 512, nb=27, n_src=4, n_clips=2, ld="M4", ucs_odd=True)
    # ---- ring
    add("ring_4096_512", "none", 4096, 512, nb=27, n_src=3)                       # R = 8
    add("ring_2048_128", "none", 2048, 128, nb=45, n_src=3)                       # R = 16, 32 ring slots
    add("ring_1024_64", "none", 1024, 64, nb=45, n_src=3)                         # hp = 32 < 64 lanes
    add("ring_1024_1024", "none", 1024, 1024, nb=27, n_src=3)                     # R = 1
    add("ring_4096_2", "none", 4096, 2, n_out=101, n_src=1)                       # R = 2048
    add("ring_no_steady", "none", 4096, 512, n_out=1500, T=5, n_src=2)            # T <= R - 1
    add("ring_T1", "none", 4096, 512, n_out=2048, T=1, n_src=2)
    add("ring_ragged", "none", 4096, 512, lengths=ragged_lengths(512), n_clips=3, n_src=2, table="uniform", out_pad=3)
    add("ring_ragged_compact", "none", 4096, 512, lengths=ragged_lengths(512), n_clips=3, n_src=2, table="compact", out_pad=3)
    # ---- block, phasor input: forced, or a size the wave kernels do not take
    add("block_16_4", "none", 16, 4, nb=43, n_src=2)
    add("block_32_32", "none", 32, 32, nb=43, n_src=2)
    add("block_64_17", "none", 64, 17, nb=43, n_src=2)
    add("block_512_200", "none", 512, 200, nb=43, n_src=2)
    add("block_1024_700", "none", 1024, 700, nb=33, n_src=2)
    add("block_1024_512", "block", 1024, 512, nb=33, n_src=2, n_clips=2)           # PF 3
    add("block_2048_2048", "block", 2048, 2048, n_out=40 * 2048, n_src=48)         # PF 5; C = 4 halved to 2
    add("block_4096_4092", "none", 4096, 4092, nb=23, n_src=2)                     # PF 9, tw_lds on
    add("block_4096_4095", "none", 4096, 4095, nb=23, n_src=2)                     # tw_lds off
    add("block_8192_2048", "none", 8192, 2048, nb=23, n_src=2)                     # PF 17
    add("block_64_16_cap", "none", 64, 16, n_out=16, n_src=8, cu_cap=True)     # n_out is set from n_cu: C reaches 4 R
    # ---- one frame alone, at a seam of each kernel: chain f1 - 1 / f1 (LC = 3), seq chunk boundary (Cs = 5), ring step boundary
    for f in (2, 3):
        add("onehot_chain_f%d" % f, "chain3", 1024, 512, nb=24, n_src=2, onehot=f)
    for f in (4, 5):
        add("onehot_seq_f%d" % f, "seq5", 1024, 512, nb=27, n_src=3, onehot=f)
    for f in (3, 4):
        add("onehot_ring_f%d" % f, "none", 4096, 512, nb=27, n_src=3, onehot=f)
    for f in (0, 7):
        add("onehot_stage_f%d" % f, "stage", 2048, 512, nb=27, n_src=4, ld="M4", onehot=f)
        add("onehot_block_f%d" % f, "block", 1024, 512, nb=33, n_src=2, onehot=f)
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


def cap_n_out(n_cu):
    """block_64_16_cap: hops * n_src >= 16 n_cu at frameSize 64, hop 16, 8 sources -> C = min(hops n_src / n_cu, 4 R) = 16"""
    hops = -(-16 * n_cu // 8)
    return hops * 16 - 32


F64_INVERSE = [(16, 4), (64, 17), (4096, 512), (8192, 2048)]
F64_FORWARD = [(16, 4), (2048, 512), (4096, 512), (8192, 2048)]


def _fwd(name, switch, N, hop, frames=40, n_samples=None, n_clips=1, stride_pad=0, rows_extra=7, ld="bins", phase=True,
         unit=True, interleave=False, table=None, lengths=None, fpw4=False, seed=None):
    if n_samples is None:
        n_samples = (frames - 2) * hop - hop // 3              # dcs_frame_count = frames
    c = dict(name=name, switch=switch, N=N, hop=hop, n_samples=n_samples, n_clips=n_clips, rows_extra=rows_extra,
             audio_stride=n_samples + stride_pad, ld=ld_of(N, ld), ld_mode=ld, phase=phase, unit=unit, interleave=interleave,
             table=table, lengths=lengths, fpw4=fpw4, seed=seed if seed is not None else hash_name(name) % 100000)
    return c


def forward_cases():
    cs = []
    add = lambda *a, **k: cs.append(_fwd(*a, **k))
    for N in (1024, 2048, 4096):
        hop = N // 2
        for sw, fam in (("wave1", "wave"), ("block", "blk")):
            p = "%s%d_" % (fam, N)
            add(p + "plain", sw, N, hop)
            add(p + "one_sample", sw, N, hop, n_samples=1)
            add(p + "ld_bins3", sw, N, hop, ld="bins3")
            add(p + "ld_M4", sw, N, hop, ld="M4")
            add(p + "ld_M4_wide", sw, N, hop, ld="M4", phase=False)         # the vector-store rows of the wave kernel
            add(p + "no_unit", sw, N, hop, unit=False)
            add(p + "clips3", sw, N, hop, n_clips=3, stride_pad=17)
            add(p + "interleave2", sw, N, hop, n_clips=2, stride_pad=17, interleave=True, ld="M4", phase=False)
        for table in ("uniform", "compact"):
            add("wave%d_table_%s" % (N, table), "wave1", N, hop, n_samples=37 * hop + 13, n_clips=3, stride_pad=17,
                lengths=ragged_lengths(hop), table=table, ld="M4", phase=False)
        add("wave%d_fpw4" % N, "none", N, 16, fpw4=True, ld="M4", phase=False, rows_extra=0)   # n_samples from n_cu
    add("wave1024_odd_hop", "wave1", 1024, 171)                              # frames that start on odd samples: scalar loads
    for N, hop in ((16, 4), (32, 17), (64, 17), (512, 171), (8192, 700), (8192, 8192), (1024, 700)):
        add("blk%d_%d" % (N, hop), "none" if N != 1024 else "block", N, hop, frames=30 if N < 8192 else 12)
    names = [c["name"] for c in cs]
    assert len(set(names)) == len(names)
    return cs


def fpw4_samples(n_cu, hop=16):
    """8 n_cu + 5 rows: four frames per workgroup, the last workgroup with three idle waves"""
    return (8 * n_cu + 5 - 2) * hop - 5


# ------------------------------------------------------------------------------------------------ which branches a case reaches
INVERSE_REGIMES = (
    "chain_r2", "chain_r4", "chain_lc_default", "chain_lc3", "chain_lc7", "chain_last_wg_none", "chain_last_wg_1",
    "chain_last_wg_2", "chain_last_wg_part", "chain_le_rm1_blocks", "chain_T1", "chain_units_lt8", "chain_units_8",
    "chain_units_gt8_rest", "chain_spc1", "chain_spc3", "chain_spc4", "chain_gc_gt1_clips",
    "dst_unaligned", "out_gap", "ragged_uniform", "ragged_compact",
    "seq_hops1", "seq_hops5", "seq_r2", "seq_r4", "seq_idle_waves",
    "staged_src4", "staged_src8", "staged_clips", "staged_broken_nsrc", "staged_broken_ld", "staged_broken_mag_align",
    "staged_broken_unit_stride",
    "ring_r8", "ring_r16_slots32", "ring_hp32", "ring_r1", "ring_r2048", "ring_blocks_not_x4", "ring_no_steady", "ring_T1",
    "ring_ragged",
    "block_pf3", "block_pf5", "block_pf9", "block_pf17", "block_halved", "block_tw_lds_on_edge", "block_tw_lds_off",
    "block_c_cap", "block_n16", "block_n32", "block_n64", "block_odd_hop", "block_hop_eq_frame", "block_hop_gt_half",
    "block_clips", "onehot_chain", "onehot_seq", "onehot_ring", "onehot_staged", "onehot_block",
)
FORWARD_REGIMES = (
    "wave_fpw1", "wave_fpw4", "wave_idle_waves", "wave_half_table", "wave_full_table", "wave_wide_rows", "wave_odd_start",
    "block_f32", "block_tw_lds_off", "block_n16", "block_n32", "block_n64", "block_hop_eq_frame", "block_odd_hop",
    "one_sample", "rows_past_T", "ld_bins", "ld_bins3", "ld_M4", "null_phase", "null_unit", "silence", "clips_stride",
    "interleave", "table_uniform", "table_compact",
)


def regimes(case, n_cu=256):
    """names of the launcher / kernel branches an inverse case reaches (restated from the launchers, not asked of them)"""
    out = set()
    N, hop, n_out, T = case["N"], case["hop"], case["n_out"], case["T"]
    S = case["n_src"] * case["n_clips"]
    kern, param = expected_inverse(case, n_cu)
    if case["n_out"] % 2 and case["out_stride"] % 2 and S > 1:
        out.add("dst_unaligned")
    if case["out_pad"]:
        out.add("out_gap")
    if case["table"]:
        out.add("ragged_" + case["table"])
    if kern == INV_CHAIN:
        g = chain_geometry(N, hop, n_out, param)
        out.add("chain_r%d" % g["R"])
        out.add({"chain3": "chain_lc3", "chain7": "chain_lc7"}.get(case["switch"], "chain_lc_default"))
        if not case["lengths"]:
            if g["n_blocks"] <= g["R"] - 1:
                out.add("chain_le_rm1_blocks")
            elif g["Gc"] == 1 and g["n_blocks"] == g["Sb"] + g["R"] - 1:
                out.add("chain_last_wg_none")
            elif g["Gc"] > 1:
                out.add("chain_last_wg_%s" % (g["last_blocks"] if g["last_blocks"] <= 2 else "full"
                                               if g["last_blocks"] == g["Sb"] else "part"))
        if T == 1:
            out.add("chain_T1")
        units = case["n_clips"] * g["Gc"]
        out.add("chain_units_lt8" if units < 8 else "chain_units_8" if units == 8 else
                "chain_units_gt8_rest" if units % 8 else "chain_units_x8")
        out.add("chain_spc%d" % case["n_src"])
        if g["Gc"] > 1 and case["n_clips"] > 1:
            out.add("chain_gc_gt1_clips")
        if case["switch"] == "stage":
            out.add("staged_broken_" + ("nsrc" if case["n_src"] % 4 else "ld" if case["ld"] != N // 2 + 4 else
                                        "mag_align" if case["mag_off"] else "unit_stride"))
    elif kern in (INV_SEQ, INV_SEQ_STAGED):
        if kern == INV_SEQ:
            out.add("seq_hops%d" % param if case["switch"] in ("seq1", "seq5") else "seq_default")
            out.add("seq_r%d" % (N // hop))
            if (seq_chunks(N, hop, n_out, param) * S) % 4:
                out.add("seq_idle_waves")
        else:
            out.add("staged_src%d" % case["n_src"])
            if case["n_clips"] > 1:
                out.add("staged_clips")
    elif kern == INV_RING:
        R, nb = N // hop, n_blocks(N, hop, n_out)
        out.add({8: "ring_r8", 1: "ring_r1", 2048: "ring_r2048"}.get(R, "ring_r%d" % R))
        if R == 16 and ring_slots(N, hop) == 32:
            out.add("ring_r16_slots32")
        if hop // 2 == 32:
            out.add("ring_hp32")
        if nb % 4:
            out.add("ring_blocks_not_x4")
        if T <= R - 1:
            out.add("ring_no_steady")
        if T == 1:
            out.add("ring_T1")
        if case["table"]:
            out.add("ring_ragged")
    else:
        plan = block_inverse_plan(N, hop, cap_n_out(n_cu) if case["cu_cap"] else n_out, case["n_src"], n_cu)
        out.add("block_pf%d" % plan["PF"])
        if plan["halved"]:
            out.add("block_halved")
        if not plan["tw_lds"]:
            out.add("block_tw_lds_off")
        elif hop + 3 <= N and not (block_inverse_plan(N, hop + 3, n_out, case["n_src"], n_cu) or plan)["tw_lds"]:
            out.add("block_tw_lds_on_edge")
        if plan["capped"] or plan["C"] == 4 * ((N + hop - 1) // hop):
            out.add("block_c_cap")
        if N in (16, 32, 64):
            out.add("block_n%d" % N)
        if hop % 2:
            out.add("block_odd_hop")
        if hop == N:
            out.add("block_hop_eq_frame")
        elif 2 * hop > N:
            out.add("block_hop_gt_half")
        if case["n_clips"] > 1:
            out.add("block_clips")
    if case["onehot"] is not None:
        out.add("onehot_" + {INV_CHAIN: "chain", INV_SEQ: "seq", INV_RING: "ring", INV_SEQ_STAGED: "staged",
                             INV_BLOCK: "block"}[kern])
    return out


def expected_forward(case):
    if case["switch"] == "block" or case["N"] not in (1024, 2048, 4096):
        return FWD_BLOCK
    if case["fpw4"]:
        return FWD_WAVE4
    assert case["switch"] == "wave1" or case["table"], case["name"]
    return FWD_WAVE1


def forward_regimes(case):
    out = set()
    N, hop = case["N"], case["hop"]
    k = expected_forward(case)
    if k == FWD_BLOCK:
        out.add("block_f32")
        if not forward_block_tw_lds(N):
            out.add("block_tw_lds_off")
        if N in (16, 32, 64):
            out.add("block_n%d" % N)
        if hop == N:
            out.add("block_hop_eq_frame")
        if hop % 2:
            out.add("block_odd_hop")
    else:
        out.add("wave_fpw4" if k == FWD_WAVE4 else "wave_fpw1")
        if k == FWD_WAVE4:
            out.add("wave_idle_waves")                      # 8 n_cu + 5 rows
        out.add("wave_half_table" if N <= 2048 else "wave_full_table")
        if case["ld_mode"] == "M4" and not case["phase"] and case["unit"]:
            out.add("wave_wide_rows")
        if hop % 2:
            out.add("wave_odd_start")
    if case["n_samples"] == 1:
        out.add("one_sample")
    if case["rows_extra"]:
        out.add("rows_past_T")
    out.add("ld_" + case["ld_mode"])
    if not case["phase"]:
        out.add("null_phase")
    if not case["unit"]:
        out.add("null_unit")
    if case["n_samples"] >= SILENCE_FACTOR * (N + hop):
        out.add("silence")                                   # forward_audio zeroes N + hop samples from n / 3 on
    if case["n_clips"] > 1 and case["audio_stride"] > case["n_samples"]:
        out.add("clips_stride")
    if case["interleave"]:
        out.add("interleave")
    if case["table"]:
        out.add("table_" + case["table"])
    return out

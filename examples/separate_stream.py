"""Separate a 16-bit PCM wav file block by block: neither the file nor its stems are ever whole in memory.

    python examples/separate_stream.py -a dsd -i mix.wav -o outdir -m model.pkl [--block 65536] [--stereo [--mwf N]] [--resample]
    python examples/separate_stream.py -a bach10_si -i mix.wav -o outdir -m model.pkl [--trainer-semantics] [--resample]
                                       [--follow [--follow-window N] [--follow-step K] [--follow-penalty X]]
    python examples/separate_stream.py -a dsd_ild -i stereo_mix.wav -o outdir -m model.pkl [--block 65536] [--mwf N] [--resample]

The file is read with the standard ``wave`` module ``--block`` frames at a time; each block is scaled and mixed down the way
the architecture's separate script does it (element-wise, so block by block equals the whole file), pushed into
``Separator.stream()`` and the samples that come back are appended to the stems, under the script's own file names, as
``(x * 32767).astype(int16)``.  The stems trail the input by ``time_context * hopSize + frameSize`` samples at the most; host and
device memory depend on ``--block``, not on the length of the file.

``--stereo``: a two-channel file gives one two-channel stem per source (``Separator.stream_channels()``: the masks of the
down-mix on each channel's own spectrum with its own phase) where it otherwise is mixed down.  ``--resample``: a file at any
sample rate is converted to 44 100 Hz block by block on the device and the stems are converted back and written at the file's
own rate (``RateStream``); without it such a file is refused, as the reference's scripts refuse it.

``-a bach10_si``: score-informed separation (``Separator.stream_scoreinformed``).  The four score files ``bassoon_b.txt,
clarinet_b.txt, saxophone_b.txt, violin_b.txt`` are read next to the wav, as the separate script reads them, and the note table
is built before the first block from the frame count the wav HEADER gives (``ceil(frames / hop) + 2`` at 44 100 Hz; with
``--resample`` from the length the file has at 44 100 Hz).  ``--trainer-semantics``: masks divided by their sum over the
instruments and soft masks on the channel sum, what the trainer's own models saw (``separate_bach10.py`` has the same
option).  ``--stereo`` does not apply.  ``--follow``: the four score files are at the score's NOMINAL tempo, not in the
recording's time, and the stream follows them as the audio arrives (``align.ScoreFollower``: online DTW on chroma features, one
row over a window of ``--follow-window`` score frames per audio frame, at most ``--follow-step`` score frames per audio frame,
``--follow-penalty`` on every step other than one): the note table is built in score time and every audio frame is painted from
the score frame the performance has reached.  It follows forward from the score's first frame and never corrects a position.

``-a dsd_ild``: the stereo (ILD) DSD100 graph (``Separator.stream_stereo``), which sees both channels: a two-channel file gives
one two-channel stem per source under the names ``examples/dsd100_2ch_ILD/separate_dsd_ild.py`` uses (``<outdir>/<source>.wav``),
with that script's hyper-parameters.  ``--stereo`` is implied (and accepted); a mono file is refused.

``--mwf N`` (with ``--stereo`` or ``-a dsd_ild`` only, as in the whole-file scripts): N iterations per frame of the ONLINE
multichannel Wiener filter between the masks and the inverse transform (``--mwf-forget X``, default 1: how much of the past
every frame keeps; ``--mwf-loading X``, default 1e-3: the isotropic share of every spatial covariance).  It is a causal filter
with constant memory -- not the whole-file filter of ``separate_dsd.py --stereo --mwf N`` and not expected to match it: the
first frames of a file are filtered on little evidence.
"""
import argparse
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARCHS = ("dsd", "hiphop", "ikala", "bach10", "bach10_si", "dsd_ild")
# separate_dsd_ild.py: (frameSize, hopSize, window, overlap, input_size)
ILD_DEFAULTS = (1024, 512, np.hanning, 25, 513)


def read_blocks(wav, block):
    """float64 blocks ``[n]`` / ``[n, channels]`` as ``read_wav`` scales them (int16 / 32767)"""
    ch = wav.getnchannels()
    while True:
        raw = wav.readframes(block)
        if not raw:
            return
        x = np.frombuffer(raw, dtype='<i2').astype('float') / np.iinfo(np.int16).max
        yield x.reshape(-1, ch) if ch > 1 else x


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-a", "--arch", required=True, choices=ARCHS)
    ap.add_argument("-i", "--input", required=True, help="16-bit PCM wav, 44 100 Hz")
    ap.add_argument("-o", "--outdir", required=True)
    ap.add_argument("-m", "--model", required=True, help="path_to_model.pkl")
    ap.add_argument("--block", type=int, default=65536, help="frames read and pushed at a time")
    ap.add_argument("--stereo", action="store_true", help="two-channel stems from a two-channel file")
    ap.add_argument("--resample", action="store_true", help="take any sample rate; the stems keep the file's rate")
    ap.add_argument("--trainer-semantics", action="store_true",
                    help="bach10_si: masks / their sum over the instruments, soft masks x the channel sum")
    ap.add_argument("--mwf", type=int, default=0, metavar="N",
                    help="iterations per frame of the online multichannel Wiener filter (with --stereo or -a dsd_ild)")
    ap.add_argument("--mwf-forget", type=float, default=1.0, metavar="X", help="online filter: weight of the past per frame, (0, 1]")
    ap.add_argument("--mwf-loading", type=float, default=1e-3, metavar="X", help="online filter: isotropic share of the covariances")
    ap.add_argument("--follow", action="store_true", help="bach10_si: the score files are at nominal tempo; follow them")
    ap.add_argument("--follow-window", type=int, default=512, metavar="N", help="score frames in the follower's window (64 .. 1024)")
    ap.add_argument("--follow-step", type=int, default=2, metavar="K", help="most score frames per audio frame (1 .. 4)")
    ap.add_argument("--follow-penalty", type=float, default=1.0 / 16, metavar="X", help="cost of a step other than one")
    args = ap.parse_args(argv)
    if args.mwf and not (args.stereo or args.arch == "dsd_ild"):    # the Wiener filter works on two-channel estimates
        ap.print_usage()
        sys.exit(2)
    score = args.arch == "bach10_si"
    if score and args.stereo:
        raise SystemExit("--stereo does not apply to bach10_si: the score-informed graphs take one channel per instrument")
    if args.trainer_semantics and not score:
        raise SystemExit("--trainer-semantics applies to bach10_si only")
    if args.follow and not score:
        raise SystemExit("--follow applies to bach10_si only")
    ild = args.arch == "dsd_ild"
    if ild:
        args.stereo = True               # the graph is stereo by construction

    import deepconvsep_amd as dcs
    from deepconvsep_amd.separation import (SI_SCORE_FILES, SI_SCORE_PARAMS, TARGET_RATE, _SCRIPT_DEFAULTS, output_paths,
                                            rate_ratio, resampled_length, to_mono)
    from deepconvsep_amd.streaming import RateStream

    frame, hop, window, overlap, bins = ILD_DEFAULTS if ild else _SCRIPT_DEFAULTS[args.arch]
    mwf = dict(mwf_iters=args.mwf, mwf_forget=args.mwf_forget, mwf_loading=args.mwf_loading)
    src = wave.open(args.input, "rb")
    if src.getsampwidth() != 2 or src.getcomptype() != "NONE":
        raise SystemExit("%s is not a 16-bit PCM wav file" % args.input)
    rate = src.getframerate()
    if rate != 44100 and not args.resample:
        raise SystemExit("Sample rate is not 44100")
    if ild and src.getnchannels() != 2:
        raise SystemExit("-a dsd_ild takes a two-channel file (the network sees both channels), %s has %d"
                         % (args.input, src.getnchannels()))
    if args.stereo and src.getnchannels() != 2:
        raise SystemExit("--stereo takes a two-channel file, %s has %d" % (args.input, src.getnchannels()))
    if score:
        from deepconvsep_amd.score import melody_table
        sem = ('sum', 'sum') if args.trainer_semantics else ('max', 'ch0')
        sep = dcs.Separator(args.arch, dcs.load_model(args.model), 0.3, 30, overlap, 32, bins, frame, hop, window,
                            tiler='library', score_normalise=sem[0], score_mixture=sem[1])
        # the frames of the signal the network sees, known from the header before any audio is read
        n44 = src.getnframes() if rate == 44100 else resampled_length(src.getnframes(), *rate_ratio(rate, TARGET_RATE))
        nframes = int(np.ceil(n44 / np.double(hop))) + 2
        follow = {}
        if args.follow:                  # the table in score time: its frames are the score's own, whatever the file's length
            from deepconvsep_amd.score import read_score
            from deepconvsep_amd.streaming import score_frames
            scores = [read_score(os.path.join(os.path.dirname(args.input), f)) for f in SI_SCORE_FILES]
            nframes = score_frames(scores, hop)
            follow = dict(follow_scores=scores, window=args.follow_window, max_step=args.follow_step, penalty=args.follow_penalty)
        melody = melody_table(SI_SCORE_FILES, os.path.dirname(args.input), nframes, TARGET_RATE, hop, frame, **SI_SCORE_PARAMS)
        stream = sep.stream_scoreinformed(melody, max_block=args.block, **follow)
    elif ild:
        sep = dcs.Separator(args.arch, dcs.load_model(args.model), 0.3, 30, overlap, 32, bins, frame, hop, window)
        stream = sep.stream_stereo(max_block=args.block, **mwf)
    else:
        sep = dcs.Separator(args.arch, dcs.load_model(args.model), 0.3, 30, overlap, 32, bins, frame, hop, window)
        stream = sep.stream_channels(max_block=args.block, **mwf) if args.stereo else sep.stream(max_block=args.block)
    if rate != 44100:
        stream = RateStream(stream, rate)
    os.makedirs(args.outdir, exist_ok=True)
    outs = []
    if ild:
        from deepconvsep_amd.stereo_training import SOURCES
        paths = [os.path.join(args.outdir, s + ".wav") for s in SOURCES]
    else:
        paths = output_paths(args.arch, args.input, args.outdir)
    for path in paths:
        w = wave.open(path, "wb")
        w.setnchannels(2 if args.stereo else 1)
        w.setsampwidth(2)
        w.setframerate(rate)
        outs.append(w)

    def write(pcm):
        if args.stereo:
            pcm = pcm.transpose(1, 0, 2)                                  # [n, S, 2] -> per source [n, 2], interleaved
        for w, x in zip(outs, pcm):
            w.writeframes(np.ascontiguousarray((x * np.iinfo(np.int16).max).astype('<i2')).tobytes())

    try:
        for blk in read_blocks(src, args.block):
            write(stream.push(blk if args.stereo else to_mono(blk, args.arch)))
        write(stream.finish())
    finally:
        src.close()
        for w in outs:
            w.close()


if __name__ == "__main__":
    main()

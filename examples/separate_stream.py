"""Separate a 16-bit PCM wav file block by block: neither the file nor its stems are ever whole in memory.

    python examples/separate_stream.py -a dsd -i mix.wav -o outdir -m model.pkl [--block 65536]

The file is read with the standard ``wave`` module ``--block`` frames at a time; each block is scaled and mixed down the way
the architecture's separate script does it (element-wise, so block by block equals the whole file), pushed into
``Separator.stream()`` and the samples that come back are appended to the stems, under the script's own file names, as
``(x * 32767).astype(int16)``.  The stems trail the input by ``time_context * hopSize + frameSize`` samples at the most; host and
device memory depend on ``--block``, not on the length of the file.
"""
import argparse
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARCHS = ("dsd", "hiphop", "ikala", "bach10")


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
    args = ap.parse_args(argv)

    import deepconvsep_amd as dcs
    from deepconvsep_amd.separation import _SCRIPT_DEFAULTS, output_paths, to_mono

    frame, hop, window, overlap, bins = _SCRIPT_DEFAULTS[args.arch]
    src = wave.open(args.input, "rb")
    if src.getsampwidth() != 2 or src.getcomptype() != "NONE":
        raise SystemExit("%s is not a 16-bit PCM wav file" % args.input)
    if src.getframerate() != 44100:
        raise SystemExit("Sample rate is not 44100")
    sep = dcs.Separator(args.arch, dcs.load_model(args.model), 0.3, 30, overlap, 32, bins, frame, hop, window)
    stream = sep.stream(max_block=args.block)
    os.makedirs(args.outdir, exist_ok=True)
    outs = []
    for path in output_paths(args.arch, args.input, args.outdir):
        w = wave.open(path, "wb")
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(44100)
        outs.append(w)

    def write(pcm):
        for w, x in zip(outs, pcm):
            w.writeframes((x * np.iinfo(np.int16).max).astype('<i2').tobytes())

    try:
        for blk in read_blocks(src, args.block):
            write(stream.push(to_mono(blk, args.arch)))
        write(stream.finish())
    finally:
        src.close()
        for w in outs:
            w.close()


if __name__ == "__main__":
    main()

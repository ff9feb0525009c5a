"""deepconvsep_amd -- the MTG/DeepConvSep separation path on MI355X (gfx950).

Host side in Python (the reference's language), arithmetic in hand-written HIP
kernels behind the C ABI of ``include/dcs.h`` (``libdcs.so``, bound with
ctypes).  Importing the package does not need a GPU; creating a context does.
"""
from . import _lib
from .arch import (ARCHS, EPS_A, EPS_B, TIE_ALL, TIE_FIRST, TILER_LIBRARY, TILER_SCRIPT)
from .transform import TransformFFT, Transforms, compute_file, compute_inverse, sinebell, transformFFT
from .evaluation import bss_eval, bss_eval_images, bss_eval_sources
from .runtime import MwfOnline, mwf
from .resample import ResampleCounts, Resampler, StreamResampler, resample
from .separation import (PredictFunction, Separator, blackmanharris, generate_overlapadd, load_model,
                         overlapadd, overlapadd_multi, save_model, train_auto)
from .streaming import (ChannelStreamSeparator, RateStream, ScoreStreamSeparator, StereoStreamSeparator, StreamCounts,
                        StreamSeparator)
from .training import FeatureWindows, Trainer, glorot_init
from .stereo_training import StereoFeatureWindows, StereoTrainer
from .score_training import ScoreFeatureWindows, ScoreTrainer
from . import augment
from .augment import RenderedWindows, render_features
from .score_render import ScoreInformedRenderedWindows, render_score_informed_features
from . import align
from .align import (ScoreFollower, align_scores, bin_classes, chroma, dtw, follow_scores, follow_time_map, score_chroma, time_map,
                    warp_times)

__all__ = ["ARCHS", "EPS_A", "EPS_B", "TIE_ALL", "TIE_FIRST", "TILER_LIBRARY", "TILER_SCRIPT", "TransformFFT",
           "Transforms", "transformFFT", "compute_file", "compute_inverse", "sinebell", "PredictFunction",
           "Separator", "blackmanharris", "generate_overlapadd", "load_model", "save_model", "overlapadd",
           "overlapadd_multi", "train_auto", "bss_eval", "bss_eval_images", "bss_eval_sources", "mwf", "MwfOnline", "Resampler", "resample", "StreamCounts", "StreamSeparator",
           "ChannelStreamSeparator", "ScoreStreamSeparator", "StereoStreamSeparator", "RateStream", "ResampleCounts", "StreamResampler", "Trainer", "FeatureWindows", "glorot_init",
           "StereoTrainer", "StereoFeatureWindows", "ScoreTrainer", "ScoreFeatureWindows", "augment", "RenderedWindows", "render_features",
           "ScoreInformedRenderedWindows", "render_score_informed_features", "align", "align_scores", "bin_classes", "chroma", "dtw",
           "score_chroma", "time_map", "warp_times", "ScoreFollower", "follow_scores", "follow_time_map"]

"""The command-line and host surface of the stereo-stems path, without a GPU: ``--stereo`` / ``--mwf N`` of the four separate
scripts, the new keywords of ``train_auto`` and the library's side of ``dcs_mask_fold_apply``."""
import inspect
import os
import subprocess
import sys

import pytest

from deepconvsep_amd import _lib, separation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = ["examples/dsd100/separate_dsd.py", "examples/hiphopss/separate_hhds.py", "examples/ikala/separate_ikala.py",
           "examples/bach10/separate_bach10.py"]
PINNED = "-i <inputfile> -o <outputdir> -m <path_to_model.pkl>"


@pytest.mark.parametrize("script", SCRIPTS)
def test_mwf_without_stereo_prints_the_usage_and_exits_with_2(script, tmp_path):
    exe = os.path.join(ROOT, script)
    r = subprocess.run([sys.executable, exe, "-i", str(tmp_path / "none.wav"), "-o", str(tmp_path), "-m", str(tmp_path / "none.pkl"),
                        "--mwf", "2"], capture_output=True, text=True)
    assert r.returncode == 2 and PINNED in r.stdout, (r.stdout, r.stderr[-500:])
    assert "--stereo" in r.stdout and "--mwf N" in r.stdout
    r = subprocess.run([sys.executable, exe, "-h"], capture_output=True, text=True)
    assert r.returncode == 0 and PINNED in r.stdout and "--stereo" in r.stdout


def test_train_auto_keywords_default_to_the_mono_path(tmp_path):
    sig = inspect.signature(separation.train_auto).parameters
    assert sig["stereo"].default is False and sig["mwf_iters"].default == 0
    assert list(sig)[-2:] == ["stereo", "mwf_iters"]                 # behind every earlier argument: positional calls keep their meaning
    with pytest.raises(ValueError, match="stereo"):                  # refused before the model or the file is touched
        separation.train_auto("dsd", str(tmp_path / "none.wav"), str(tmp_path), str(tmp_path / "none.pkl"), mwf_iters=2)
    for script in SCRIPTS:
        sys.path.insert(0, os.path.join(ROOT, os.path.dirname(script)))
        try:
            mod = __import__(os.path.splitext(os.path.basename(script))[0])
        finally:
            sys.path.pop(0)
        p = inspect.signature(mod.train_auto).parameters
        assert p["stereo"].default is False and p["mwf_iters"].default == 0 and p["resample"].default is False
        del sys.modules[mod.__name__]                                # two scripts are called separate_bach10.py


def test_library_declares_and_exports_the_entry_point():
    assert "dcs_mask_fold_apply" in _lib.header_symbols()
    lib = _lib.load()
    assert hasattr(lib, "dcs_mask_fold_apply") and len(lib.dcs_mask_fold_apply.argtypes) == 20
    # a null context is refused before anything else is looked at
    assert lib.dcs_mask_fold_apply(None, None, 0, 0, 4, 30, 25, 513, 0, None, None, 0, 2, 0, 513, None, 0, 0, None, 0) == _lib.DCS_EINVAL

"""CPU: the library's HJD_* overrides are one table, read from the environment
once and switched in-process by hjd_debug_set_tuning (hjd.debug_tuning).
Observed through behaviour, on the frame test_entropy_emulation_spec.py pins:
the speculative sync's emulation of a q90 4:4:4 FHD frame at S = 512 needs a
repair (status 1) at a lead-in of 512 bits and none (status 0) at 1536."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as O
import test_entropy_emulation as E


@pytest.fixture(scope="module")
def frame(hjd):
    data = E._pil(1920, 1080, 90, 0, seed=5)
    return data, hjd.decode_coefs(data)[0]


def _status(hjd, frame):
    data, ref = frame
    got, status = hjd.emulate_entropy(data, 512)
    np.testing.assert_array_equal(got, ref)
    return status


def test_unknown_name_is_rejected(hjd):
    with pytest.raises(hjd._lib.HjdError, match="HJD_NO_SUCH_KNOB") as e:
        with hjd.debug_tuning("HJD_NO_SUCH_KNOB", 1):
            pass
    assert e.value.code == -1   # HJD_E_INVALID


def test_set_and_restore(hjd, frame):
    with hjd.debug_tuning("HJD_SYNC_SPEC", 1):
        unset = _status(hjd, frame)
        with hjd.debug_tuning("HJD_SPEC_LEAD", 1536):
            assert _status(hjd, frame) == 0
        with hjd.debug_tuning("HJD_SPEC_LEAD", 512):
            assert _status(hjd, frame) == 1
        assert _status(hjd, frame) == unset


def test_environment_is_read_once():
    code = r"""
import os, sys
import numpy as np
sys.path.insert(0, REPO); sys.path.insert(0, REPO + "/tests")
import ocljpegdecoder_amd as hjd, test_entropy_emulation as E
data = E._pil(1920, 1080, 90, 0, seed=5)
ref, _ = hjd.decode_coefs(data)
def status():
    got, s = hjd.emulate_entropy(data, 512)
    assert np.array_equal(got, ref)
    return s
assert status() == 0, "lead-in 1536 from the environment"
os.environ["HJD_SPEC_LEAD"] = "512"
assert status() == 0, "the environment was read again"
with hjd.debug_tuning("HJD_SPEC_LEAD", 512):
    assert status() == 1, "the setter had no effect"
print("read once ok")
""".replace("REPO", repr(O.REPO))
    env = dict(os.environ, HJD_SYNC_SPEC="1", HJD_SPEC_LEAD="1536")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "read once ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_gdec_debug_entries_are_exported_and_reject_null(hjd):
    """hjd_debug_gdec_state / hjd_debug_gdec_set_chain_epoch (per-decoder state,
    so not part of the process-wide table above): exported, bound in _lib.py,
    mirrored on GpuDecoder, and a NULL handle is HJD_E_INVALID without a device."""
    import ctypes
    lib = hjd._lib.load()
    syms = subprocess.run(["nm", "-D", "--defined-only", hjd._lib.LIB_PATH], capture_output=True, text=True,
                          check=True).stdout.split()
    st = hjd._lib.HjdGdecDebugState()
    for name, args in (("hjd_debug_gdec_state", (None, ctypes.byref(st))),
                       ("hjd_debug_gdec_set_chain_epoch", (None, 5))):
        assert name in syms and name in hjd._lib.SIGNATURES
        assert getattr(lib, name).argtypes == hjd._lib.SIGNATURES[name][1]
        assert getattr(lib, name)(*args) == -1   # HJD_E_INVALID
        assert "NULL" in hjd._lib.error_string()
    assert callable(hjd.GpuDecoder.debug_state) and callable(hjd.GpuDecoder.debug_set_chain_epoch)
    # the struct is the header's: ten 32-bit integers in the declared order
    text = open(os.path.join(O.REPO, "include", "hjd_host.h")).read()
    body = text[text.index("typedef struct hjd_gdec_debug_state {"):text.index("} hjd_gdec_debug_state;")]
    fields = re.findall(r"^\s*(u?int32_t) (\w+);", body, re.M)
    assert [n for _, n in fields] == [n for n, _ in st._fields_]
    assert [t for t, _ in fields] == ["uint32_t" if c is ctypes.c_uint32 else "int32_t" for _, c in st._fields_]


def test_setter_accepts_exactly_the_documented_names(hjd):
    text = open(os.path.join(O.REPO, "INTEGRATION.md")).read()
    table = text[text.index("### Environment overrides"):]
    names = re.findall(r"^\| `(HJD_[A-Z0-9_]+)` \|", table, re.M)
    assert names and len(names) == len(set(names))
    # the other direction: the rows of the library's table, as its source lists them
    src = open(os.path.join(O.REPO, "ocljpegdecoder_amd", "csrc", "hjd_runtime.hip")).read()
    assert sorted(re.findall(r'^    \{"(HJD_[A-Z0-9_]+)", &Tuning::', src, re.M)) == sorted(names)
    for n in names:
        with hjd.debug_tuning(n, None):
            pass
        wrong = n[:-1] + ("X" if n[-1] != "X" else "Y")
        with pytest.raises(hjd._lib.HjdError):
            with hjd.debug_tuning(wrong, None):
                pass

"""Scaled decode, host side: hjd_scaled_size, the numpy model of the definition
(tests/scaled_model.py) against the oracle, and the C ABI's declarations.  No
GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle_py as O
import scaled_model as M

SIZES = [(1, 1), (17, 9), (3840, 2160), (3841, 2161)]
SCALES = [1, 2, 4, 8]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("s", SCALES)
def test_scaled_size(hjd, w, h, s):
    exp = (-(-w // s), -(-h // s))
    assert hjd.scaled_size(w, h, s) == exp
    assert M.scaled_size(w, h, s) == exp
    lib = ctypes.CDLL(os.path.join(O.REPO, "ocljpegdecoder_amd", "lib", "libhjd.so"))
    ow, oh = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.hjd_scaled_size(w, h, s, ctypes.byref(ow), ctypes.byref(oh)) == 0
    assert (ow.value, oh.value) == exp


@pytest.mark.parametrize("s", [0, 3, 16, -2])
def test_scaled_size_refuses_a_bad_scale(hjd, s):
    from ocljpegdecoder_amd._lib import HjdError, load
    with pytest.raises(HjdError) as e:
        hjd.scaled_size(17, 9, s)
    assert e.value.code == -1 and "scale" in str(e.value)
    ow, oh = ctypes.c_int(-1), ctypes.c_int(-1)
    assert load().hjd_scaled_size(17, 9, s, ctypes.byref(ow), ctypes.byref(oh)) == -1   # HJD_E_INVALID


@pytest.mark.parametrize("w,h", [(17, 9), (130, 33)])
@pytest.mark.parametrize("sampling", [0, 1, 4])
def test_model_at_scale_1_is_the_oracle(sampling, w, h):
    """The model's MCU assembly, chroma replication and colour are the oracle's."""
    coefs, qt = O.synthetic_coefs(w, h, sampling, seed=3 * w + h + sampling)
    np.testing.assert_array_equal(M.decode_scaled(coefs, qt, w, h, sampling, 1), O.decode_q16(coefs, qt, w, h, sampling))


@pytest.mark.parametrize("sampling", [0, 1, 4])
def test_flat_frame_is_unchanged_by_scaling(sampling):
    """Every block DC-only with one DC per component: all samples of a
    component are equal, so every output pixel equals the full-size pixel."""
    w, h = 50, 35
    n = O.frame_blocks(w, h, sampling)
    coefs = np.zeros((n, 64), np.int16)
    coefs[:, 0] = np.array([37, -21, 55])[O.block_components(sampling, n)]
    qt = O.std_qtables()
    full = O.decode_q16(coefs, qt, w, h, sampling)
    assert len(np.unique(full)) == 1
    for s in (2, 4, 8):
        got = M.decode_scaled(coefs, qt, w, h, sampling, s)
        assert got.shape == (-(-h // s), -(-w // s))
        assert (got == full[0, 0]).all()


def test_box_mean_rounds_half_up_and_floors():
    blk = np.zeros((1, 64), np.int32)
    blk[0, :2] = [-1, -2]                   # one 2x2 box sums to -3: (-3 + 2) >> 2 = -1
    assert M.box_means(blk, 2)[0, 0, 0] == -1
    blk[0, :2] = [1, 1]                     # (2 + 2) >> 2 = 1
    assert M.box_means(blk, 2)[0, 0, 0] == 1
    assert M.box_means(np.full((1, 64), -256, np.int32), 8).item() == -256
    assert M.box_means(np.full((1, 64), 255, np.int32), 8).item() == 255


def test_declarations_and_abi_version():
    inc = os.path.join(O.REPO, "include")
    hjd_h = open(os.path.join(inc, "hjd.h")).read()
    host_h = open(os.path.join(inc, "hjd_host.h")).read()
    assert re.search(r"#define\s+HJD_ABI_VERSION\s+1\b", hjd_h)
    for decl in (r"int\s+hjd_scaled_size\(int width, int height, int scale, int\* out_w, int\* out_h\);",
                 r"int\s+hjd_plan_create_scaled\(", r"int\s+hjd_plan_scale\(const hjd_plan\*"):
        assert re.search(decl, hjd_h), decl
    assert re.search(r"int\s+hjd_gdec_set_scale\(hjd_gdec\*\s*\w*, int scale\);", host_h)
    from ocljpegdecoder_amd._lib import load
    lib = load()
    assert lib.hjd_abi_version() == 1
    for name in ("hjd_scaled_size", "hjd_plan_create_scaled", "hjd_plan_scale", "hjd_gdec_set_scale"):
        assert getattr(lib, name)


def test_python_names(hjd):
    import inspect
    assert "scaled_size" in hjd.__all__
    assert inspect.signature(hjd.Plan.__init__).parameters["scale"].default == 1
    assert inspect.signature(hjd.decode_frame).parameters["scale"].default == 1
    assert inspect.signature(hjd.GpuDecoder.decode_rgb).parameters["scale"].default == 1
    assert callable(hjd.GpuDecoder.set_scale)

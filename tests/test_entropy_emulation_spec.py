"""CPU: the speculative sync of latency decoders ("Single-image
latency": ent_spec_kernel / ent_cand_kernel / ent_chain_kernel, run on the
host by hjd_debug_entropy_emulate with HJD_SYNC_SPEC=1) must reproduce the
host Huffman decoder's coefficients exactly, like the round-based sync.  Every
test of test_entropy_emulation.py runs again in this mode (imported below),
and the spec runs' lead-in is swept, down to 0 bits, where the chain leaves
the candidate slots often and the chain kernel's repair path is exercised."""
import contextlib
import os

import numpy as np
import pytest

import test_entropy_emulation as E
from test_entropy_emulation import *  # noqa: F401,F403  (re-run the whole module in speculative mode)


@pytest.fixture(autouse=True)
def _spec_sync(hjd):
    with hjd.debug_tuning("HJD_SYNC_SPEC", "1"):
        yield


@pytest.fixture
def tuning(hjd):
    """tuning(name, value): hjd.debug_tuning for the rest of the test."""
    with contextlib.ExitStack() as stack:
        yield lambda name, value: stack.enter_context(hjd.debug_tuning(name, value))


@pytest.mark.parametrize("lead", [0, 64, 512, 2048])
@pytest.mark.parametrize("sub_bits", [32, 256, 512])
def test_lead_in_sweep(hjd, tuning, lead, sub_bits):
    tuning("HJD_SPEC_LEAD", lead)
    for i, (name, kw) in enumerate(E.CASES[:11]):
        kw = dict(kw)
        data = E._pil(kw.pop("w"), kw.pop("h"), kw.pop("q"), kw.pop("sub"), seed=900 + i, **kw)
        ref, _ = hjd.decode_coefs(data)
        got, status = hjd.emulate_entropy(data, sub_bits)
        np.testing.assert_array_equal(got, ref, err_msg=f"{name} S={sub_bits} lead={lead}")
        assert status & ~1 == 0


def test_reference_sample_all_leads(hjd, tuning):
    for lead in (0, 1, 300, 4096):
        tuning("HJD_SPEC_LEAD", lead)
        for name in E.O.golden_cases():
            data = open(os.path.join(E.O.GOLDEN, name + ".jpg"), "rb").read()
            ref, _ = hjd.decode_coefs(data)
            got, status = hjd.emulate_entropy(data, 64)
            np.testing.assert_array_equal(got, ref, err_msg=f"{name} lead={lead}")


def test_repair_sets_status_bit_and_long_leads_avoid_it(hjd, tuning):
    """The premise of the decoder's lead-in ladder (spec_lead_bits): status bit
    0 reports that the chain needed a repair; this q90 4:4:4 FHD frame breaks
    9 times at the short lead-in (512 bits) and never at the ladder's next
    step (1536).  The GPU test of the ladder relies on exactly this."""
    data = E._pil(1920, 1080, 90, 0, seed=5)
    ref, _ = hjd.decode_coefs(data)
    for lead, bit in ((512, 1), (1536, 0)):
        tuning("HJD_SPEC_LEAD", lead)
        got, status = hjd.emulate_entropy(data, 512)
        np.testing.assert_array_equal(got, ref, err_msg=f"lead={lead}")
        assert status == bit, (lead, status)


@pytest.mark.parametrize("seed,bits", [(0, (1, 0)), (1, (0, 0))])
def test_ladder_walk_frames(hjd, tuning, seed, bits):
    """The two frames that walk the lead-in ladder on the GPU
    (test_gpu_decoder_reuse.py): at S = 512 the 320x240 q90 4:4:4 frame of
    seed 0 needs a repair at a lead-in of 512 bits and none at 1536, and the
    frame of seed 1 is clean at both."""
    data = E._pil(320, 240, 90, 0, seed=seed)
    ref, _ = hjd.decode_coefs(data)
    for lead, bit in zip((512, 1536), bits):
        tuning("HJD_SPEC_LEAD", lead)
        got, status = hjd.emulate_entropy(data, 512)
        np.testing.assert_array_equal(got, ref, err_msg=f"lead={lead}")
        assert status == bit, (lead, status)

"""The CPU stand-ins of the gfx950 primitives (igmc_amd/csrc/g2_prims.h, g2_image.h), one at a time through
``igmc_debug_g2_prims`` on the CPU emulation of the HIP sources (tests/prims_checks.py; tests/test_gpu_prims.py holds the device
forms to the same restatements on an MI355X -- what makes the emulator's results say something about the device)."""
import pytest

import parity_checks as PC
import prims_checks as PR


@pytest.fixture(scope='module')
def be():
    return PC.EmuBackend()


def test_probe_refuses_bad_arguments(be):
    PR.check_refusals(be)


def test_split_is_round_to_nearest_even_and_exact(be):
    PR.check_split(be)


def test_byte_masks(be):
    PR.check_masks(be)


def test_mfma_exact_sums(be):
    PR.check_mfma_exact(be)


def test_mfma_random_operands(be):
    PR.check_mfma_random(be)


def test_rcp(be):
    PR.check_rcp(be)


def test_exp(be):
    PR.check_exp(be)


def test_tanh(be):
    PR.check_tanh(be)

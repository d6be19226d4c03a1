"""The device forms of the gfx950 primitives (igmc_amd/csrc/g2_prims.h, g2_image.h) on an MI355X, one at a time through
``igmc_debug_g2_prims`` (tests/prims_checks.py; CPU twin: tests/test_emu_prims.py): the bf16 conversion and the three-term split
bit for bit, the byte masks bit for bit, the matrix-core step against the float64 sum of its exact products, and the fast tanh
with the two instructions it is made of against float64."""
import pytest

import parity_checks as PC
import prims_checks as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return PC.GpuBackend()


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

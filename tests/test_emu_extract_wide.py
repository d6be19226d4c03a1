"""Kernel LOGIC of the HIP extraction on wide rating graphs (more than 256 bitmap words a side, fringes of 90 000 candidates,
batches of more than 256 links) on the CPU emulator: the rows, proofs and checks of tests/extract_wide_checks.py, which
tests/test_gpu_extract_wide.py runs on the real gfx950 binary."""
import pytest

import extract_wide_checks as XW
import parity_checks as PC


@pytest.fixture(scope='module')
def be():
    """The backend; the graphs of the rows are built here, once, and given up (device graphs closed, twins and downloads
    dropped) when the module is done."""
    XW.graphs()
    try:
        yield PC.EmuBackend()
    finally:
        XW.release()


SLOW = {'e'}
ROWS = [pytest.param(n, marks=pytest.mark.slow) if n in SLOW else n for n in XW.ROWS]


@pytest.mark.parametrize('name', ROWS)
def test_row_matches_the_host_twin(be, name):
    XW.check_row(be, name)


@pytest.mark.parametrize('name', XW.REPLAYED)
def test_replayed_twin_lists_are_the_free_run(be, name):
    XW.check_replay(be, name)


@pytest.mark.parametrize('name', XW.REPLAYED)
def test_same_bits_across_launches_and_other_nodes_in_another_epoch(be, name):
    XW.check_same_bits(be, name)

"""``igmc_amd/csrc/extract.hip`` on a real MI355X on wide rating graphs, against the host twin and the extraction oracle: the
rows, proofs and checks of tests/extract_wide_checks.py, which the emulator runs too (test_emu_extract_wide.py).  What the
single-threaded emulator cannot show is what these are for: the barriers around ``kth_radix``'s histogram and mailboxes
(``sm[8..11]``) under real wave scheduling, ``hist`` re-used as the parked key / id lists, 256 threads carrying ``running``
through a second and a thirteenth round of the bitmap scans, and the emission kernels' prefix loops over more than 256 links.
No hook lowers the 256-key bound on a device: the fringes are wide enough to cross it, which each row proves on the host first.
Everything is integer: every comparison is exact."""
import pytest

import extract_wide_checks as XW
import parity_checks as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    """The backend; the graphs of the rows are built here, once, and given up (device graphs closed, twins and downloads
    dropped) when the module is done."""
    XW.graphs()
    try:
        yield PC.GpuBackend()
    finally:
        XW.release()


@pytest.mark.parametrize('name', list(XW.ROWS))
def test_row_matches_the_host_twin(be, name):
    XW.check_row(be, name)


@pytest.mark.parametrize('name', XW.REPLAYED)
def test_replayed_twin_lists_are_the_free_run(be, name):
    XW.check_replay(be, name)


@pytest.mark.parametrize('name', XW.REPLAYED)
def test_same_bits_across_launches_and_other_nodes_in_another_epoch(be, name):
    XW.check_same_bits(be, name)

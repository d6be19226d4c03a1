"""``igmc_graph_apply`` on the host emulation build (kernel logic only; the cases and checks of tests/graph_update_checks.py, which
tests/test_gpu_graph_update.py runs unchanged on the device)."""
import pytest

import graph_update_checks as GU
import parity_checks as PC


@pytest.fixture(scope='module')
def be():
    return PC.EmuBackend()


def test_single_changes_alone_and_mixed(be):
    GU.check_single_changes(be)


def test_empty_list_with_and_without_growth(be):
    GU.check_empty_list(be)


def test_row_lengths_across_the_wave_and_workgroup_widths(be):
    GU.check_corner_rows(be)


def test_row_longer_than_the_sort_tile(be):
    GU.check_corner_rows(be, extra=(GU.SORT_TILE + 1,))


def test_duplicates_the_last_wins(be):
    GU.check_duplicates(be)


@pytest.mark.parametrize('n', [GU.ROW_STAGE, GU.ROW_STAGE + 1, 300, GU.SORT_TILE, GU.SORT_TILE + 1])
def test_all_changes_in_one_row_and_in_one_column(be, n):
    GU.check_concentration(be, n)


def test_max_rel_and_degrees_follow_removals(be):
    GU.check_max_rel_and_degrees(be)


def test_growth(be):
    GU.check_growth(be)


@pytest.mark.parametrize('seed', range(20))
def test_random(be, seed):
    GU.check_random(be, seed)


def test_chained_updates_leave_every_stage_as_it_was(be):
    GU.check_chained(be)


def test_output_does_not_depend_on_the_grid(be):
    GU.check_geometry(be)


def test_errors_leave_out_untouched_and_the_library_serving(be):
    GU.check_errors(be)

"""``igmc_shortlist_fill`` / ``igmc_shortlist_places`` (``igmc_amd/csrc/shortlist.hip``) on the CPU emulation of the HIP
sources: every segment, vote count and place is the scipy definition of ``tests/shortlist_checks.py``, written from the text of
``include/igmc_hip.h``.  Cases, references and checks run unchanged on the device (``tests/test_gpu_shortlist.py``)."""
import pytest

import shortlist_checks as SL
from helpers import emu_lib
from parity_checks import EmuBackend
from selection_checks import BAD_OFFSETS


@pytest.mark.parametrize('n_items', SL.N_ITEMS_SMALL)
@pytest.mark.parametrize('n_users', [40, 300])
def test_segments_and_votes_are_the_definition(n_users, n_items):
    SL.check_segments(EmuBackend(), n_users, n_items)


@pytest.mark.slow
@pytest.mark.parametrize('n_items', SL.N_ITEMS_WIDE)
def test_segments_and_votes_are_the_definition_around_the_vote_table_and_past_it(n_items):
    SL.check_segments(EmuBackend(), 8, n_items, thresholds=((0, 0), (3, 1)), ms=(7, 3000))


def test_every_kind_of_m():
    SL.check_every_m(EmuBackend())


def test_ties_at_the_threshold_are_cut_by_item_id():
    SL.check_ties(EmuBackend())


def test_degenerate_rows():
    SL.check_degenerate_rows(EmuBackend())


def test_request_order_grids_and_tables_left_clean():
    SL.check_order_and_grids(EmuBackend())


@pytest.mark.parametrize('delta', [-1, 0, 1])
def test_w_in_lds_and_in_the_scratch_row(delta):
    SL.check_w_table_switch(EmuBackend(), delta)


def test_what_has_no_place_is_reported_and_not_written():
    SL.check_no_place(EmuBackend())


def test_a_user_id_out_of_range_is_reported():
    SL.check_bad_user(EmuBackend(), (10, -1, 2 ** 31 - 1))


@pytest.mark.parametrize('bad', BAD_OFFSETS)
def test_inconsistent_query_offsets_are_reported_and_not_followed(bad):
    SL.check_bad_query_offsets(EmuBackend(), bad, wild=True)


def test_bad_arguments_and_a_graph_past_the_vote_bound_are_refused():
    SL.check_refusals(emu_lib())


@pytest.mark.parametrize('n_items', SL.N_ITEMS_SMALL)
def test_places_are_the_index_in_the_vote_order(n_items):
    SL.check_places(EmuBackend(), 60, n_items)


@pytest.mark.slow
@pytest.mark.parametrize('n_items', [SL.TILE + 1, 2 * SL.TILE + SL.TILE // 2])
def test_places_past_the_vote_table(n_items):
    SL.check_places(EmuBackend(), 8, n_items, thresholds=((0, 0),), masks=(True,), excludes=(1,))

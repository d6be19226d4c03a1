"""``k_candidates<0/1, 1>`` (``igmc_amd/csrc/candidates.hip``) on a real MI355X through their C entry points,
against the numpy definition of ``tests/sampled_candidates_checks.py`` -- the cases, references and checks the emulator test
runs (test_emu_sampled_candidates.py).  What the single-threaded emulator cannot show is what these are for: 256 threads
marking the same LDS bitmap words, 64 lanes adding into the same histogram bins and list cursor, ballot placement, and a
workgroup taking a second request where a launch is capped at 65 536 workgroups.

Every buffer sits between guard elements that are checked after every call, and the cases with inconsistent offsets,
capacities, must items or user ids keep their bad values within the guards: a clamp the kernel lost fails the test, it cannot
leave the allocation.  Every comparison is exact."""
import pytest

import parity_checks as PC
import sampled_candidates_checks as SC
from selection_checks import BAD_OFFSETS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    return PC.GpuBackend()


@pytest.mark.parametrize('n_items', SC.N_ITEMS)
def test_segments_are_the_definition(be, n_items):
    SC.check_segments(be, n_items)


@pytest.mark.parametrize('n_items', [65, 16385, 40000])
def test_every_negative_and_no_must_item_is_the_enumeration_byte_for_byte(be, n_items):
    SC.check_all_negatives_is_the_enumeration(be, n_items)


def test_a_crowded_deciding_byte_goes_through_the_radix_passes(be):
    SC.check_fallback_selection(be, 100000, 256)


def test_a_deciding_byte_of_256_keys_is_parked_and_one_of_257_is_not(be):
    SC.check_park_bound(be)


def test_more_users_than_workgroups_and_the_same_users_in_another_order(be):
    SC.check_many_users(be)


def test_what_has_no_place_is_reported_and_not_written(be):
    SC.check_no_place(be)


def test_a_user_id_out_of_range_is_reported(be):
    SC.check_bad_user(be, (10, -1))          # n_users and -1: next to the row pointers, never far from them


def test_a_must_item_out_of_range_is_ignored_and_reported(be):
    SC.check_bad_must_item(be)


@pytest.mark.parametrize('bad', BAD_OFFSETS)
def test_inconsistent_must_offsets_are_reported_and_not_followed(be, bad):
    SC.check_bad_must_offsets(be, bad, wild=False)


def test_bad_arguments_are_refused(be):
    SC.check_refusals(be.lib)
    be.sync()          # (nothing was launched: nothing can have gone wrong behind the calls)


@pytest.mark.parametrize('n', [150, 400, 2000])
def test_draws_are_the_restatement_and_distributed_like_uniform_k_subsets(be, n):
    SC.check_distribution(be, n)

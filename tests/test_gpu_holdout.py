"""``k_holdout<0/1>`` (``igmc_amd/csrc/holdout.hip``) on a real MI355X through its C entry points, against the numpy
definition of ``tests/holdout_checks.py`` -- the cases, references and checks the emulator test runs (test_emu_holdout.py).
What the single-threaded emulator cannot show is what these are for: 64 lanes adding into the same histogram bins and list
cursor, ballot placement across four waves, and a workgroup taking a second request where the launch is capped at 65 536
workgroups.

Every buffer sits between guard elements that are checked after every call, and the cases with a short capacity, inconsistent
offsets or bad user ids keep their bad values within the guards: a clamp the kernel lost fails the test, it cannot leave the
allocation.  Every comparison is exact."""
import pytest

import holdout_checks as HC
import parity_checks as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    return PC.GpuBackend()


@pytest.mark.parametrize('hold', HC.HOLDS)
def test_segments_are_the_definition(be, hold):
    HC.check_definition(be, holds=(hold,))


def test_kept_sets_are_nested_in_keep(be):
    HC.check_nested(be)


def test_a_long_row_goes_through_the_radix_passes(be):
    HC.check_long_row(be)


def test_a_deciding_byte_of_256_keys_is_parked_and_one_of_257_is_not(be):
    HC.check_park_bound(be)


def test_more_users_than_workgroups_and_the_same_users_in_another_order(be):
    HC.check_many_users(be)


def test_what_has_no_place_is_reported_and_not_written(be):
    HC.check_no_place(be)


def test_a_user_id_out_of_range_is_reported(be):
    HC.check_bad_user(be, (10, -1))          # n_users and -1: next to the row pointers, never far from them


def test_bad_arguments_are_refused(be):
    HC.check_refusals(be.lib)
    be.sync()          # (nothing was launched: nothing can have gone wrong behind the calls)


@pytest.mark.parametrize('keep,hold', HC.REDUCED)
def test_the_reduced_graph_is_the_graph_of_the_reduced_matrix(be, keep, hold):
    HC.check_reduced_graph(be, keep, hold)


@pytest.mark.parametrize('n', [150, 400])
def test_splits_are_the_restatement_and_distributed_like_uniform_k_subsets(be, n):
    HC.check_distribution(be, n)

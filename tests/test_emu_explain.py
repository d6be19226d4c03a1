"""Leave-one-out variants and attributions on the host emulation build (kernel logic only; the cases and checks of
tests/explain_checks.py, which tests/test_gpu_explain.py runs unchanged on the device)."""
import pytest

import explain_checks as EX
import parity_checks as PC


@pytest.fixture(scope='module')
def be():
    return PC.EmuBackend()


def test_every_size_without_a_cap_and_without_dense_blocks(be):
    EX.check_sizes_covered(be)


@pytest.mark.parametrize('lean', [False, True])
@pytest.mark.parametrize('B', [1, 7, 50])
def test_arena_with_dense_blocks(be, lean, B):
    EX.check_case(be, 1, 100, lean, B, first=3 if B == 1 else 0, want_dense=True)


@pytest.mark.parametrize('B', [1, 7])
def test_arena_without_dense_blocks(be, B):
    EX.check_case(be, 1, None, False, B, first=6 if B == 1 else 0, want_dense=False)


@pytest.mark.parametrize('B', [7, 50])
def test_two_hops_under_a_cap_that_binds(be, B):
    lists, want = EX.check_case(be, 2, 10, True, B, want_dense=True)
    assert max(len(U) for U, _, _, _ in lists) == 21 and max(ul.max() for _, ul, _, _ in lists) == 4
    removed = want['var_side'] != 255
    assert (want['var_rating'][removed] == 0).any() and (want['var_rating'][removed] > 0).any()


def test_capacities_one_short_and_bad_offsets(be):
    EX.check_capacities(be)


def test_fill_does_not_depend_on_the_grid(be):
    EX.check_grid(be)


def test_deltas_against_numpy(be):
    EX.check_deltas(be)


def test_the_oracle_deltas_stand_far_outside_the_tolerance():
    """The premise of the GPU test against the CPU oracle (tests/test_gpu_explain.py): on its 30 x 40 graph with the reference
    parameters UNSCALED, the largest |delta| of every link with a neighbour is hundreds of times the tolerance
    2 * OUT_TOL * peak |score|.  (Two of the six users: the figure for all six was 0.0096 against 1.0e-5.)"""
    A, cv, rows, cols = EX.oracle_graph()
    ref = PC.make_ref_model(4, 5, seed=6)
    ref.eval()
    res = EX.oracle_deltas(ref, A, cv, EX.oracle_pairs(A, rows, cols, users=(3, 20)))
    tol = 2 * PC.OUT_TOL * max(abs(b) for b, _ in res)
    largest = [max(abs(x) for x in d.values()) for _, d in res if d]
    assert len(largest) == len(res) > 10 and min(largest) > 100 * tol, (min(largest), tol)


def test_link_files_parse_like_new_ratings_files():
    import numpy as np
    from igmc_amd.explain import parse_links
    u, v = parse_links(['# user item', '0 5', '  7\t812   # a comment', '', '2999 0'])
    assert u.dtype == np.int32 and u.tolist() == [0, 7, 2999] and v.tolist() == [5, 812, 0]
    for bad in ('1', '1 2 3', 'a 2', '-1 2', '1 %d' % (2 ** 31 - 1)):
        with pytest.raises(ValueError, match='line 2'):
            parse_links(['0 0', bad], name='f')

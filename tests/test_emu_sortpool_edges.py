"""Sort-pool readout at odd and large k, subgraph sizes around k, tied keys and the largest admitted k -- kernel logic on the
CPU emulation vs the float64 oracle (cases and runner: ``sortpool_edge_checks``).  The bounds that bind are
``parity_checks.DGCNN_OUT_TOL / DGCNN_LOSS_RTOL / DGCNN_GRAD_TOL``, asserted inside the runner."""
import pytest

import parity_checks as PC
import sortpool_edge_checks as SE


@pytest.fixture(scope='module')
def be():
    return PC.EmuBackend()


@pytest.mark.parametrize('drop', [True, False])
def test_sizes_around_an_odd_k(be, drop):
    assert (63, drop) in SE.runs('around_k_odd')
    SE.run_case(be, 'around_k_odd', SE.make('around_k_odd'), 63, drop)


def test_three_fan_in_rounds_and_a_one_graph_row_tile_twice_bit_equal(be):
    (k, drop), = SE.runs('k131_B17')
    ctx = SE.run_case(be, 'k131_B17', SE.make('k131_B17'), k, drop, repeat=True)
    assert ctx['B'] == 17 and ctx['sp'].dense // 16 == 122


def test_smallest_odd_k(be):
    (k, drop), = SE.runs('k_min_odd')
    ctx = SE.run_case(be, 'k_min_odd', SE.make('k_min_odd'), k, drop)
    assert ctx['sp'].dense == 32


def test_k201_on_slots_of_the_402_node_shape(be):
    (k, drop), = SE.runs('k201_wide')
    SE.run_case(be, 'k201_wide', SE.make('k201_wide'), k, drop)


@pytest.mark.parametrize('name', ['tied_k12', 'tied_k63'])
def test_all_keys_tied_pools_the_first_k_nodes(be, name):
    (k, drop), = SE.runs(name)
    SE.run_case(be, name, SE.make(name), k, drop)


def test_tied_twins_cut_by_k_and_inside_a_max_pool_pair(be):
    case = SE.make('twins')
    flags = [SE.run_case(be, 'twins', case, k, drop)['twin_flags'] for k, drop in SE.runs('twins')]
    assert any(c for c, _ in flags), 'no group of twins is cut by the k boundary'
    assert any(p for _, p in flags), 'no two twins share a max-pool pair'


def test_largest_k_the_lds_plan_admits(be):
    SE.run_k_limit(be)

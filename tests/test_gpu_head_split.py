"""The head of the subgraph kernel (igmc_amd/csrc/g2_subgraph.h) on the MI355X at the headline shape (ml_1m-shaped graph, cap 100,
batches of 50: clusters of four workgroups per subgraph): the head's arrays complete, launches on the same inputs
bit-identical -- launched directly and replayed from the step's hipGraph --, no bounded device-side wait timed out.
CPU twin: tests/test_emu_head_split.py."""
import numpy as np
import pytest

import head_split_checks as HS
import parity_checks as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def be():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return PC.GpuBackend()


@pytest.fixture(scope='module')
def ml1m():
    from test_gpu_headline import ml_case
    return ml_case('ml_1m', 100, 50)


@pytest.mark.parametrize('drop', [False, True])
def test_headline_launches_are_complete_and_bit_identical(be, ml1m, drop, monkeypatch, capfd):
    monkeypatch.setenv('IGMC_GRAPH_STEP', '1')
    monkeypatch.setenv('IGMC_GS_TRACE', '1')
    res = PC.run_model_parity(be, ml1m, R=5, use_dropout=drop)
    err = capfd.readouterr().err
    assert 'k_graph_step B=50 train=1' in err and 'k_graph_step B=50 train=0' in err and 'cluster=4' in err, err[-400:]
    assert res['worst_grad_err'] < PC.GRAD_TOL
    arr = HS.head_arrays(be, res['ws'], 50)
    HS.check_head_arrays(arr, res)
    r1 = HS.relaunch(be, res, drop)
    r2 = HS.relaunch(be, res, drop)
    HS.check_bit_identical(r1, r2)
    assert np.array_equal(r1['out'], res['train_out']) and np.array_equal(r1['loss'], res['loss'])
    for k in arr:
        assert np.array_equal(arr[k], r1[k]), k
    HS.check_error_word(be, res['ws'])


def test_headline_steps_replayed_from_the_graph_are_bit_identical():
    """Two epochs of the default training structure (groups of steps replayed from a hipGraph) twice from the same seed:
    parameters, Adam moments and epoch totals bit-equal; every epoch ends in ``check()``, which raises on the error word."""
    import torch
    from igmc_amd.util_functions import MyDynamicDataset
    from test_gpu_headline import _assert_same, _trajectory, ml_case
    case = ml_case('ml_1m', 100, 1)
    A, cv = case['A'], case['class_values']
    coo = A.tocoo()
    pick = np.random.default_rng(12).permutation(coo.nnz)[:800]
    u, v, y = coo.row[pick], coo.col[pick], (coo.data[pick] - 1).astype(np.int64)
    ds = MyDynamicDataset('data/t/head_split', A, (u, v), y, 1, 1.0, 100, None, None, cv, device=0, seed=1)
    perm = torch.randperm(len(ds), generator=torch.Generator().manual_seed(6))
    sg, ref = _trajectory(ds, 0.0, perm, group=8)
    assert sg.ws.dense_path(sg.arenas[0], 50)
    assert any(g is not None for g in sg.graphs) and ref[4] == 32
    _, again = _trajectory(ds, 0.0, perm, group=8)
    _assert_same(ref, again, 'replayed steps at the headline shape, twice from the same seed')
    sg.check()

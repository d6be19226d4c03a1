"""The model step gives the same result whatever its arena and workspace held before, on the CPU emulation of the HIP
sources (tests/history_checks.py; tests/test_gpu_history.py runs the whole table on an MI355X): the subgraph kernel at 4
workgroups per subgraph (the clusters an MI355X takes, ``IGMC_GS_CLUSTER=4``), the one-launch dense layers and the row
walkers.  Per case and mask form: the target batch after a batch that filled every slot (H1) equals the target batch on new
memory (H0) in outputs, loss and the whole gradient; each subgraph's outputs follow a permutation of the batch and do not
change with dirty batch-mates; H1 is within the parity tolerances of ``oracle/pyg_ref`` in float64.  Then a history of
non-finite parameters, cleared by ``igmc_model_reset_exchange``."""
import pytest

import history_checks as HC
import parity_checks as PC

HOOKS = ('IGMC_GRAPH_STEP', 'IGMC_GS_CLUSTER', 'IGMC_GS_GRID', 'IGMC_DL', 'IGMC_DL_ALWAYS', 'IGMC_DL_FUSED', 'IGMC_DL_TS',
         'IGMC_DL_GSPLIT', 'IGMC_DL_HEAD', 'IGMC_FIN_MODE')
# (1,1) (1,128) (128,1) (2,3) (17,15) (33,31) (37,5) (65,63) of the 4-workgroup row; (1,1) (1,201) (129,127) (145,17) of the
# one-launch dense row; the row walkers' row as it is
CASES = {
    'subgraph_wg4': HC.smaller(HC.BY_ID['subgraph_wg4'], 8, [0, 1, 2, 3, 5, 6, 7, 8]),
    'dense_fused': HC.smaller(HC.BY_ID['dense_fused'], 4, [0, 1, 3, 5]),
    'rows': HC.BY_ID['rows'],
}
_CRAFTED = {}


@pytest.fixture(scope='module')
def be():
    return PC.EmuBackend()


@pytest.fixture(autouse=True)
def _clusters_of_an_mi355x(monkeypatch):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('IGMC_GS_CLUSTER', '4')


def crafted(be, name):
    if name not in _CRAFTED:
        _CRAFTED[name] = HC.Crafted(be, CASES[name])
    return _CRAFTED[name]


# (both mask forms for the subgraph kernel; the dense layers and the row walkers with both masks injected at once: five
#  emulated runs of a case take the better part of a minute)
@pytest.mark.parametrize('name,drop', [('subgraph_wg4', False), ('subgraph_wg4', True), ('dense_fused', True), ('rows', True)],
                         ids=['subgraph_wg4-lin_mask', 'subgraph_wg4-edge_flags', 'dense_fused-edge_flags', 'rows-edge_flags'])
def test_result_does_not_depend_on_history_or_position(be, name, drop):
    cr = crafted(be, name)
    h0, h1 = HC.check_histories(cr, drop)
    HC.check_oracle(cr, h1, drop)
    # (the permuted order and one of the two interleaved halves: the GPU file runs both)
    HC.check_positions(cr, drop, both_halves=False)


@pytest.mark.parametrize('name', ['subgraph_wg4', 'dense_fused'])
def test_reset_exchange_clears_a_nonfinite_history(be, name):
    HC.run_nonfinite_history(crafted(be, name), drop=True)

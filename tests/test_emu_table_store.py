"""The subgraph kernel's table stores (operands of the table product swapped, one 16-byte store a tile) on the CPU emulation
of the HIP sources (tests/table_store_checks.py; tests/test_gpu_table_store.py runs the same rows on an MI355X): a cluster of 4
and the looping grid, R = 5 and R = 2, with and without injected edge flags; one loss_grad and one Adam step each, twice from
differently filled workspaces (bit-equal) and against the float64 oracle."""
import pytest

import parity_checks as PC
import table_store_checks as TS

HOOKS = ('IGMC_GRAPH_STEP', 'IGMC_GS_CLUSTER', 'IGMC_GS_GRID', 'IGMC_DL', 'IGMC_DL_ALWAYS', 'IGMC_DL_FUSED', 'IGMC_DL_TS',
         'IGMC_DL_GSPLIT', 'IGMC_DL_HEAD', 'IGMC_FIN_MODE')
_CRAFTED = {}


@pytest.fixture(scope='module')
def be():
    return PC.EmuBackend()


@pytest.mark.parametrize('drop', [False, True], ids=['lin_mask', 'edge_flags'])
@pytest.mark.parametrize('name', list(TS.ROWS))
def test_table_stores_cover_their_slot(be, monkeypatch, name, drop):
    case, env = TS.ROWS[name]
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if name not in _CRAFTED:
        _CRAFTED[name] = TS.HC.Crafted(be, case)
    TS.check_case(_CRAFTED[name], drop)

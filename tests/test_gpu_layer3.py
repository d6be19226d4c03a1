"""Conv layer 3 of the subgraph kernel -- forward on the centre bundles only, backward in closed form -- on an MI355X
(tests/layer3_checks.py): clusters of 4, 2 and 1 workgroups and the looping single-workgroup grid, R = 5 and R = 3, with and
without injected edge flags whose centre edges keep one direction only; each against the float64 oracle tensor by tensor,
after a batch that filled every slot of the same arena and workspace, and twice on the same inputs (bit-equal)."""
import pytest

import layer3_checks as L3
import parity_checks as PC

pytestmark = pytest.mark.gpu

HOOKS = ('IGMC_GRAPH_STEP', 'IGMC_GS_CLUSTER', 'IGMC_GS_GRID', 'IGMC_DL', 'IGMC_DL_ALWAYS', 'IGMC_DL_FUSED', 'IGMC_DL_TS',
         'IGMC_DL_GSPLIT', 'IGMC_DL_HEAD', 'IGMC_FIN_MODE')
_CRAFTED = {}


@pytest.fixture(scope='module')
def be():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return PC.GpuBackend()


@pytest.mark.parametrize('drop', [False, True], ids=['lin_mask', 'edge_flags'])
@pytest.mark.parametrize('name', list(L3.ROWS))
def test_layer3_on_the_centre_rows(be, monkeypatch, name, drop):
    case, env = L3.ROWS[name]
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if name not in _CRAFTED:
        _CRAFTED[name] = L3.HC.Crafted(be, case)
    L3.check_case(_CRAFTED[name], drop)

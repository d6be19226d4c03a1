"""Every conv layer of a training launch against float64 on the launch's own stored inputs, across kernel families, relation
counts, mask forms and conv parameter scales, on an MI355X (tests/layer_checks.py; CPU twin: tests/test_emu_layers.py)."""
import pytest

import layer_checks as LC
import parity_checks as PC

pytestmark = pytest.mark.gpu

HOOKS = ('IGMC_GRAPH_STEP', 'IGMC_GS_CLUSTER', 'IGMC_GS_GRID', 'IGMC_DL', 'IGMC_DL_ALWAYS', 'IGMC_DL_FUSED', 'IGMC_DL_TS',
         'IGMC_DL_GSPLIT', 'IGMC_DL_HEAD', 'IGMC_FIN_MODE', 'IGMC_L3_VEC')
_CRAFTED = {}


@pytest.fixture(scope='module')
def be():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return PC.GpuBackend()


def _crafted(be, monkeypatch, family, R):
    case, env = LC.case(family, R)
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if case.id not in _CRAFTED:
        _CRAFTED[case.id] = LC.HC.Crafted(be, case)
    return _CRAFTED[case.id]


@pytest.mark.parametrize('s', LC.SCALES, ids=['s1', 's1_64', 's8'])
@pytest.mark.parametrize('drop', [False, True], ids=['lin_mask', 'edge_flags'])
@pytest.mark.parametrize('R', [5, 3], ids=['r5', 'r3'])
@pytest.mark.parametrize('family', list(LC.FAMILIES))
def test_each_layer_against_float64_on_its_own_inputs(be, monkeypatch, family, R, drop, s):
    cr = _crafted(be, monkeypatch, family, R)
    res = LC.run(cr, family, drop, s)
    LC.check_layers(cr, res, family, drop, s)
    LC.check_whole_step(cr, res, family, drop, s)

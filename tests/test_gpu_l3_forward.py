"""Conv layer 3's forward in closed form -- centre-row sums formed in layer 2's epilogue, handed over as tagged words, five matvecs
a side in every member -- on an MI355X (tests/l3_forward_checks.py; CPU twin: tests/test_emu_l3_forward.py): the sums against the
kernel's own h_2 at the bound of float32 summation, after a launch that wrote every bundle's words, twice on the same inputs,
the evaluation kernel against the oracle, and the head's arrays with the lin1 rows requested ahead of the readout."""
import pytest

import head_split_checks as HS
import l3_forward_checks as LF
import layer3_checks as L3
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


def _crafted(be, monkeypatch, key, case, env):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if key not in _CRAFTED:
        _CRAFTED[key] = L3.HC.Crafted(be, case)
    return _CRAFTED[key]


@pytest.mark.parametrize('drop', [False, True], ids=['lin_mask', 'edge_flags'])
@pytest.mark.parametrize('name', LF.SUM_ROWS)
def test_centre_sums_against_the_kernels_own_h2(be, monkeypatch, name, drop):
    LF.check_sums(_crafted(be, monkeypatch, name, *L3.ROWS[name]), name, drop)


@pytest.mark.parametrize('drop', [False, True], ids=['lin_mask', 'edge_flags'])
def test_words_of_an_earlier_launch_are_not_read(be, monkeypatch, drop):
    LF.check_stale(_crafted(be, monkeypatch, 'stale', LF.STALE, LF.STALE_ENV), drop)


@pytest.mark.parametrize('drop', [False, True], ids=['lin_mask', 'edge_flags'])
@pytest.mark.parametrize('name', list(L3.ROWS))
def test_evaluation_and_training_outputs_against_the_oracle(be, monkeypatch, name, drop):
    LF.check_eval(_crafted(be, monkeypatch, name, *L3.ROWS[name]), name, drop)


def test_head_arrays_with_the_lin1_rows_requested_early(be, monkeypatch):
    """A cluster of four at up to 101 nodes a side: every hidden unit of every subgraph written from its own lin1 row."""
    from helpers import load_extract_golden
    case = dict(load_extract_golden()['synth_nocap'])
    case['mnph'] = 100
    case['recs'], case['links'], case['link_labels'] = case['recs'][:4], case['links'][:4], case['link_labels'][:4]
    monkeypatch.setenv('IGMC_GRAPH_STEP', '1')
    monkeypatch.setenv('IGMC_GS_CLUSTER', '4')
    res = PC.run_model_parity(be, case, R=5, use_dropout=True)
    assert res['ws'].step_geometry(res['batch'], 4)['wg_per_graph'] == 4
    arr = HS.head_arrays(be, res['ws'], res['d']['B'])
    HS.check_head_arrays(arr, res)
    HS.check_error_word(be, res['ws'])

"""The model step gives the same result whatever its arena and workspace held before, on an MI355X
(tests/history_checks.py): one row per step family -- the subgraph kernel at 4, 2 and 1 workgroups per subgraph (the last on
its looping grid), the dense layers in one launch, per layer with and without tables, ten relations in two groups at once,
the row walkers -- each on crafted subgraphs of exactly chosen extents after a batch that filled every slot.

Per row and mask form (injected ``lin_mask``; injected edge flags too): outputs, loss and the whole gradient are
value-equal on new memory (H0), after the dirty batch on the same arena and workspace (H1), on a dirty arena with a new
workspace (H2) and on a new arena with a dirty workspace (H3); ``igmc_train_step`` after a dirty train step and an in-place
restore of the caller's buffers (HT) leaves the parameters, Adam moments, loss and outputs of a train step on new memory;
each subgraph's outputs are value-equal under a permuted link order and with dirty batch-mates; H1 is within the parity
tolerances of ``oracle/pyg_ref`` in float64 (``profiles/history_parity_observed.txt``).  Then histories of non-finite
parameters: ``igmc_model_reset_exchange`` at the C level, ``IGMC.reset_parameters()`` at the Python level."""
import numpy as np
import pytest

import geometry_cases as GC
import history_checks as HC
import parity_checks as PC

pytestmark = pytest.mark.gpu

HOOKS = ('IGMC_GRAPH_STEP', 'IGMC_GS_CLUSTER', 'IGMC_GS_GRID', 'IGMC_DL', 'IGMC_DL_ALWAYS', 'IGMC_DL_FUSED', 'IGMC_DL_TS',
         'IGMC_DL_GSPLIT', 'IGMC_DL_HEAD', 'IGMC_FIN_MODE')
IDS = [c.id for c in HC.CASES]
MASKS = dict(argvalues=[False, True], ids=['lin_mask', 'edge_flags'])
_CRAFTED = {}
REACHED_KINDS = set(GC.FAMILIES) | {'wg4', 'wg2', 'wg1_loop', 'dense_fused_tables1', 'dense_layer_tables1',
                                     'dense_layer_tables0', 'groups_gsplit1'}


@pytest.fixture(scope='module')
def be():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return PC.GpuBackend()


@pytest.fixture(autouse=True)
def _no_hooks(monkeypatch):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)


def crafted(be, name):
    if name not in _CRAFTED:
        _CRAFTED[name] = HC.Crafted(be, HC.BY_ID[name])
    return _CRAFTED[name]


@pytest.mark.parametrize('drop', **MASKS)
@pytest.mark.parametrize('name', IDS)
def test_result_does_not_depend_on_history(be, name, drop):
    cr = crafted(be, name)
    h0, h1 = HC.check_histories(cr, drop, with_sides=True)
    HC.check_oracle(cr, h1, drop)


@pytest.mark.parametrize('drop', **MASKS)
@pytest.mark.parametrize('name', IDS)
def test_train_step_does_not_depend_on_history(be, name, drop):
    HC.check_train_step_history(crafted(be, name), drop)


@pytest.mark.parametrize('drop', **MASKS)
@pytest.mark.parametrize('name', IDS)
def test_outputs_do_not_depend_on_position(be, name, drop):
    HC.check_positions(crafted(be, name), drop)


def test_every_row_of_the_table_was_reached():
    """Every step family and every split within it that the table sets out to hit, among the geometries the cases reported
    (each run asserts its own before anything else)."""
    assert len(_CRAFTED) == len(HC.CASES) and all(cr.geometry for cr in _CRAFTED.values()), 'run the whole file'
    got = GC.geometry_kinds([(cr.geometry, cr.case.B) for cr in _CRAFTED.values()])
    assert REACHED_KINDS <= got, REACHED_KINDS - got


@pytest.mark.parametrize('name', IDS)
def test_reset_exchange_clears_a_nonfinite_history(be, name):
    """(Without the reset the subgraph kernel and the one-launch dense layers, R = 10 included, predict one constant for every
    subgraph smaller than its slot; the per-layer dense kernels and the row walkers keep nothing across calls.)"""
    HC.run_nonfinite_history(crafted(be, name))


def test_reset_parameters_clears_a_nonfinite_history(be):
    """``train_multiple_epochs`` calls ``reset_parameters()`` at the start of every run on a reused model: a run after a
    diverged one must predict what a new model object with the same parameters predicts -- not one constant."""
    import torch
    from igmc_amd.models import IGMC
    from igmc_amd.util_functions import MyDynamicDataset
    B = 8
    targets = [(1, 1), (1, 128), (128, 1), (2, 3), (17, 15), (33, 31), (37, 5), (65, 63)]
    A, links = HC.crafted_graph([(128, 128, 1.0)] * B + [(nu, nv, 0.6) for nu, nv in targets], 5)
    ds = MyDynamicDataset('data/t/history', A, (links[:, 0], links[:, 1]), np.arange(len(links)) % 5, 1, 1.0, 127, None, None,
                          np.arange(1.0, 6.0))

    def new_model():
        return IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=5, num_bases=4, regression=True, adj_dropout=0.0).to('cuda')
    torch.manual_seed(7)
    model = new_model()
    model.reset_parameters()
    # ---- a diverged run: one training forward / backward on parameters that hold NaN, every slot filled
    with torch.no_grad():
        model.flat_parameters()[::7] = float('nan')
    data = ds.extract(None, 0, B)
    assert model._workspace(data).step_geometry(data.arena, B)['family'] == 'subgraph'
    model.train()
    out = model(data)
    out.sum().backward()
    assert not torch.isfinite(out).any(), 'the poisoned parameters did not reach the outputs'
    # ... and its evaluation pass (the differentiable training forward runs the conv layers as launches of their own, which
    # do not touch the exchange regions; the evaluation forward -- like the fused training step -- takes the subgraph kernel)
    model.eval()
    with torch.no_grad():
        assert not torch.isfinite(model(data)).any(), 'the poisoned parameters did not reach the outputs'
    # ---- the next run on the reused model
    torch.manual_seed(8)
    model.reset_parameters()
    assert torch.isfinite(model.flat_parameters()).all()
    fresh = new_model()
    fresh.load_state_dict(model.state_dict())
    assert torch.equal(fresh.flat_parameters(), model.flat_parameters())
    data = ds.extract(None, B, B)
    preds = []
    for m in (model, fresh):
        with torch.no_grad():
            m.eval()
            ev = m(data).cpu().numpy()
            m.train()
            m._step = 5            # (the MLP dropout is keyed on the step)
            tr = m(data).cpu().numpy()
        preds.append((ev, tr))
    for got, want, what in zip(preds[0], preds[1], ('eval', 'train')):
        assert np.isfinite(got).all() and np.isfinite(want).all(), what
        assert len(np.unique(want)) == B, '%s: the subgraphs of the target batch differ, their predictions must' % what
        assert np.array_equal(got, want), '%s predictions after reset_parameters() on a model that ran on non-finite ' \
            'parameters: %s, a new model with the same parameters: %s' % (what, got, want)

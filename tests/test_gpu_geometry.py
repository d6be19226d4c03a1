"""Every launch geometry of the model step, held to the oracle (tests/geometry_cases.py lists them: one row on each side of
every threshold the batch size, the slot capacities, the relation and hop counts and the side-feature width cross).

Per row: eval outputs, train outputs, loss and every gradient vs ``oracle/pyg_ref`` at the parity tolerances; the
geometry ``igmc_model_step_geometry`` reports; the kernels that actually launched (``igmc_profile_fetch``) agree with the
family it reports; NaN sentinels behind the batch's outputs stay untouched.  Then steps of different batch sizes on ONE
arena and workspace -- full steps through ``igmc_train_step``, the ragged ones as ``StepGraph`` runs them -- vs
``pyg_ref.train_step`` + torch Adam."""
import numpy as np
import pytest

import geometry_cases as GC
import parity_checks as PC
from igmc_amd import engine

pytestmark = pytest.mark.gpu

HOOKS = ('IGMC_GRAPH_STEP', 'IGMC_GS_CLUSTER', 'IGMC_GS_GRID', 'IGMC_DL', 'IGMC_DL_ALWAYS', 'IGMC_DL_FUSED', 'IGMC_DL_TS',
         'IGMC_DL_GSPLIT', 'IGMC_DL_HEAD', 'IGMC_FIN_MODE')
# the kernel that marks each family in the step's launches
MARKER = {'subgraph': 'k_graph_step', 'dense_fused': 'k_dl_fwd', 'dense_layer': 'k_dl_layer_fwd', 'rows': 'k_rgcn_layer_fwd'}
REACHED = {}


@pytest.fixture(scope='module')
def be():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return PC.GpuBackend()


@pytest.fixture(autouse=True)
def _no_hooks(monkeypatch):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize('r', GC.ROWS, ids=[r.id for r in GC.ROWS])
def test_geometry_matches_oracle(be, monkeypatch, r):
    for k, v in r.env.items():
        monkeypatch.setenv(k, v)
    case = GC.ml_case(r.dataset, r.mnph, r.B, hops=r.hops, seed=3 + r.B)
    seen = {}

    def around_step(ws, batch, B):
        seen['geometry'] = ws.step_geometry(batch, B)
        engine.profile_fetch(be.lib, 128)          # (drops what earlier calls left)
        engine.profile_enable(be.lib, True)

        def after():
            be.sync()
            seen['kernels'] = {name for name, _, _ in engine.profile_fetch(be.lib, 128)}
            engine.profile_enable(be.lib, False)
        return after

    try:
        res = PC.run_model_parity(be, case, R=r.R, use_dropout=True, n_side=r.side, max_graphs=r.cap, out_pad=8,
                                  on_step=around_step)
    finally:
        engine.profile_enable(be.lib, False)
    geo, kernels = seen['geometry'], seen['kernels']
    assert res['d']['B'] == r.B
    REACHED[r.id] = (geo, r.B)
    rl, ro, _ = res['oracle']
    PC.record_observed('geometry_parity', row=r.id, geometry=geo, B=int(r.B), eval_out_rel=res['eval_err'],
                       train_out_rel=PC.rel_err(res['train_out'], ro),
                       loss_rel=abs(float(res['loss'][0]) - rl) / max(abs(rl), 1e-12), worst_grad_rel=res['worst_grad_err'])
    assert geo == r.geometry, (geo, r.geometry)
    # what launched agrees with the reported family
    assert MARKER[geo['family']] in kernels, (geo['family'], sorted(kernels))
    for fam, k in MARKER.items():
        if fam != geo['family']:
            assert k not in kernels, (geo['family'], k, sorted(kernels))
    assert ('k_tail_ts' in kernels) == bool(geo['tables']), sorted(kernels)
    assert ('k_dl_bwd' in kernels) == bool(geo['dl_bwd']), sorted(kernels)
    assert ('k_dl_layer_bwd' in kernels) == (geo['family'] == 'dense_layer'), sorted(kernels)


def test_the_table_covers_every_geometry():
    """Every kernel family, every number of workgroups per subgraph (the looping grid included), dense layers with and
    without tables, relation groups with and without the split -- in the table, and among what the rows reached."""
    want = GC.REQUIRED_KINDS
    assert want <= GC.geometry_kinds([(r.geometry, r.B) for r in GC.ROWS]), want - GC.geometry_kinds(
        [(r.geometry, r.B) for r in GC.ROWS])
    if len(REACHED) == len(GC.ROWS):       # (the whole table ran in this session)
        got = GC.geometry_kinds(REACHED.values())
        assert want <= got, want - got


# ---------------------------------------------------------------- steps of several batch sizes on one arena
@pytest.mark.parametrize('dataset,mnph,R,sizes,kinds', [
    # the subgraph kernel at 4 workgroups per subgraph: grids of 224 and of 32 workgroups in one workspace
    ('ml_1m', 100, 5, [50, 50, 7, 50, 1, 50], {'wg4'}),
    # one-launch and per-layer dense layers in one workspace (64 and 57: per-layer with tables; 50 and 7: one launch)
    ('ml_100k', 200, 5, [50, 64, 7, (57, 'train_step'), 50], {'dense_fused_tables1', 'dense_layer_tables1'}),
    # ten relations: the group split (50, 7) and group after group (100, 57)
    ('ml_10m_lite', 100, 10, [100, 50, (57, 'train_step'), 7, 100], {'groups_gsplit0', 'groups_gsplit1'}),
], ids=['ml1m_subgraph', 'ml100k_fused_and_layer', 'ml10m_gsplit_and_groups'])
def test_mixed_batch_sizes_track_torch_adam(be, dataset, mnph, R, sizes, kinds):
    n = sum(s if isinstance(s, int) else s[0] for s in sizes)
    case = GC.ml_case(dataset, mnph, n, seed=11)
    res = PC.run_fused_train_trajectory(be, case, R=R, use_dropout=True, sizes=sizes)
    bs = [s if isinstance(s, int) else s[0] for s in sizes]
    got = GC.geometry_kinds(zip(res['geometries'], bs))
    assert kinds <= got, (kinds, res['geometries'])
    assert res['frac_off'] < PC.TRAJ_FRAC_OFF

"""Launch geometries of the model step on the CPU emulation of the HIP sources: what ``igmc_model_step_geometry``
answers for every row of tests/geometry_cases.py (the thresholds that do not depend on the device: the emulator takes the
clusters an MI355X takes under ``IGMC_GS_CLUSTER=4``), the looping form of the subgraph kernel (fewer workgroups than
subgraphs) and steps of several batch sizes on one arena, both against the oracle."""
import pytest

import geometry_cases as GC
import parity_checks as PC
from helpers import load_extract_golden
from igmc_amd import engine

CASES = load_extract_golden()
HOOKS = ('IGMC_GRAPH_STEP', 'IGMC_GS_CLUSTER', 'IGMC_GS_GRID', 'IGMC_DL', 'IGMC_DL_ALWAYS', 'IGMC_DL_FUSED', 'IGMC_DL_TS',
         'IGMC_DL_GSPLIT', 'IGMC_DL_HEAD', 'IGMC_FIN_MODE')


@pytest.fixture(scope='module')
def be():
    return PC.EmuBackend()


@pytest.fixture(autouse=True)
def _no_hooks(monkeypatch):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)


def sub(name, n):
    name, _, cap = name.partition(':')       # 'case:cap' = the case's graph and links with another per-hop cap
    case = dict(CASES[name])
    if cap:
        case['mnph'] = int(cap)
    case['recs'], case['links'], case['link_labels'] = case['recs'][:n], case['links'][:n], case['link_labels'][:n]
    return case


def test_query_answers_every_row_of_the_table(be, monkeypatch):
    graphs = {}
    for r in GC.ROWS:
        monkeypatch.setenv('IGMC_GS_CLUSTER', r.env.get('IGMC_GS_CLUSTER', '4'))
        if r.dataset not in graphs:
            graphs[r.dataset] = engine.Graph(GC.load_split(r.dataset)[2], device=be.device, lib=be.lib)
        b = engine.Batch(graphs[r.dataset], max_graphs=r.cap, hop=r.hops, max_nodes_per_hop=r.mnph)
        ws = engine.ModelWorkspace(be.lib, be.device, r.R, 4, 2 * r.hops + 2, r.side, b.node_capacity, b.edge_capacity,
                                   r.cap)
        try:
            assert ws.step_geometry(b, r.B) == r.geometry, r.id
            assert ws.step_geometry(b, r.B)['form'] == ws.step_form(b, r.B), r.id
        finally:
            ws.close()
            b.close()
    assert GC.REQUIRED_KINDS <= GC.geometry_kinds([(r.geometry, r.B) for r in GC.ROWS])


def test_query_refuses_a_batch_beyond_the_arena(be):
    g = engine.Graph(CASES['synth_cap']['A'], device=be.device, lib=be.lib)
    b = engine.Batch(g, max_graphs=4, hop=1, max_nodes_per_hop=15)
    ws = engine.ModelWorkspace(be.lib, be.device, 5, 4, 4, 0, b.node_capacity, b.edge_capacity, 4)
    for B in (0, 5):
        with pytest.raises(RuntimeError, match='igmc_model_step_geometry'):
            ws.step_geometry(b, B)
    assert ws.step_geometry(b, 4)['family'] == 'subgraph'


@pytest.mark.parametrize('drop', [False, True])
def test_subgraph_kernel_loops_over_subgraphs(be, monkeypatch, drop):
    """One workgroup per subgraph on a grid of 2 for 5 subgraphs: workgroup w takes subgraphs w, w + 2, w + 4 in turn and
    accumulates its partial tables (the form an MI355X runs from B = 113)."""
    monkeypatch.setenv('IGMC_GS_CLUSTER', '1')
    monkeypatch.setenv('IGMC_GS_GRID', '2')
    seen = {}

    def before(ws, b, B):
        seen['g'] = ws.step_geometry(b, B)

    res = PC.run_model_parity(be, sub('synth_cap', 5), R=5, use_dropout=drop, out_pad=8, on_step=before)
    assert seen['g']['family'] == 'subgraph' and seen['g']['wg_per_graph'] == 1 and seen['g']['grid'] == 2, seen
    assert res['worst_grad_err'] < PC.GRAD_TOL


@pytest.mark.parametrize('name,env,sizes,family', [
    ('synth_nocap:100', {'IGMC_DL_ALWAYS': '1', 'IGMC_GRAPH_STEP': '0'}, [4, 2, 4, (1, 'train_step'), 4], 'dense_fused'),
    ('synth_cap', {'IGMC_GS_CLUSTER': '1', 'IGMC_GS_GRID': '2'}, [4, 1, 4, (3, 'train_step')], 'subgraph'),
], ids=['dense_layers', 'subgraph_loop'])
def test_mixed_batch_sizes_track_torch_adam(be, monkeypatch, name, env, sizes, family):
    """Full steps (igmc_train_step) and ragged ones (loss_grad + igmc_step_finish, or igmc_train_step at the smaller size)
    on one arena and workspace vs pyg_ref.train_step + torch Adam."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    res = PC.run_fused_train_trajectory(be, sub(name, 16), R=5, use_dropout=True, sizes=sizes)
    assert {g['family'] for g in res['geometries']} == {family}, res['geometries']
    if family == 'subgraph':            # grids of 2 (looping) and of 1 workgroup
        assert {g['grid'] for g in res['geometries']} == {1, 2}, res['geometries']

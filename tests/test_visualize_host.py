"""The host half of ``--visualize`` (no GPU): ``PyGGraph_to_nx`` against what the reference's returned
(``tests/golden/visualize_golden.npz``, written by ``tests/golden/make_visualize_golden.py``), the drawing third of
``train_eval.visualize`` on a hand-made selection, and the surface (``sort_by``, ``Main.py``)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'visualize_golden.npz')


def _golden_graphs():
    from igmc_amd.util_functions import Data
    z = np.load(GOLDEN)
    for k in range(int(z['nx/count'])):
        g = lambda key: z['nx/%d/%s' % (k, key)]
        lab = torch.from_numpy(g('label').astype(np.int64))
        x = torch.nn.functional.one_hot(lab, int(g('n_labels'))).float()
        data = Data(x, torch.from_numpy(g('edge_index').astype(np.int64)),
                    edge_type=torch.from_numpy(g('edge_type').astype(np.int64)), y=torch.from_numpy(g('y')))
        yield data, dict(nodes=g('nodes'), node_type=g('node_type'), edges=g('edges'), rating=float(g('rating')))


def test_pyg_graph_to_nx_equals_the_references():
    from igmc_amd.util_functions import PyGGraph_to_nx
    seen = 0
    for data, ref in _golden_graphs():
        g = PyGGraph_to_nx(data)
        nodes = list(g.nodes())
        assert nodes == ref['nodes'].tolist()                                   # same nodes, same iteration order
        assert sorted(nodes) == list(range(data.num_nodes))
        assert [g.nodes[v]['type'] for v in nodes] == ref['node_type'].tolist()
        assert [(u, v, t) for u, v, t in g.edges(data='type')] == [tuple(r) for r in ref['edges'].tolist()]
        assert g.graph['rating'] == ref['rating']
        assert not g.is_directed()
        seen += 1
    assert seen >= 4


def test_pyg_graph_to_nx_keeps_isolated_nodes():
    from igmc_amd.util_functions import Data, PyGGraph_to_nx
    x = torch.nn.functional.one_hot(torch.tensor([0, 2, 1, 3]), 4).float()
    ei = torch.tensor([[0, 2], [2, 0]])
    g = PyGGraph_to_nx(Data(x, ei, edge_type=torch.tensor([3, 3]), y=torch.tensor([4.0])))
    assert sorted(g.nodes()) == [0, 1, 2, 3] and list(g.edges(data='type')) == [(0, 2, 3)]
    assert [g.nodes[v]['type'] for v in range(4)] == [0, 2, 1, 3] and g.graph['rating'] == 4.0
    assert g.degree(1) == 0 and g.degree(3) == 0


@pytest.mark.parametrize('num,class_values', [(3, [0.5 * k for k in range(1, 11)]), (1, list(range(1, 101)))])
def test_drawing_half_writes_the_figure(tmp_path, num, class_values):
    """2 x num axes (+ the colour bar's), the reference's title format, a non-empty PDF; 100 class values: 20 ticks."""
    from igmc_amd.train_eval import draw_subgraphs
    from igmc_amd.util_functions import PyGGraph_to_nx
    graphs = [PyGGraph_to_nx(d) for d, _ in _golden_graphs()]
    assert len(graphs) >= 2 * num
    sel = graphs[:2 * num]
    scores = [3.14159 + i for i in range(2 * num)]
    ys = [float(g.graph['rating']) for g in sel]
    # (relation ids of the golden graphs index into class_values: at most 10 relations there)
    path = str(tmp_path / 'visualization_test_prediction.pdf')
    fig = draw_subgraphs(sel, scores, ys, path, class_values, num)
    assert os.path.getsize(path) > 1000
    assert open(path, 'rb').read(5) == b'%PDF-'
    axes = fig.get_axes()
    assert len(axes) == 2 * num + 1                      # the grid + the colour bar
    titles = [ax.get_title() for ax in axes[:2 * num]]
    assert titles == ['{:.4f} ({:})'.format(s, y) for s, y in zip(scores, ys)]
    for t in titles:
        assert re.match(r'^-?\d+\.\d{4} \(-?\d+(\.\d+)?\)$', t), t
    assert len(axes[-1].get_yticks()) == min(len(class_values), 20)


def test_sort_by_outside_the_three_values_raises():
    from igmc_amd.train_eval import visualize
    with pytest.raises(ValueError, match='sort_by'):
        visualize(None, [], '.', 'x', [1., 2.], num=5, sort_by='score')
    with pytest.raises(ValueError, match='num'):
        visualize(None, [], '.', 'x', [1., 2.], num=65, sort_by='true')


def test_main_runs_visualize():
    src = open(os.path.join(ROOT, 'Main.py')).read()
    assert 'NotImplementedError' not in src
    assert re.search(r'if args\.visualize:\s*\n(\s*#.*\n)*\s*model\.load_state_dict\(torch\.load\(args\.model_pos', src)
    assert 'Transfer learning rmse is: {:.6f}' in src
    te = open(os.path.join(ROOT, 'igmc_amd', 'train_eval.py')).read()
    assert 'get_cmap' not in te and 'interpolation' not in te          # what newer matplotlib releases refuse
    assert not re.search(r'^import (matplotlib|networkx)|^from (matplotlib|networkx)', te, re.M)      # imported on use only

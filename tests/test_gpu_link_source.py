"""The ``links.LinkSource`` protocol on a real MI355X: a list refilled in place says how many links it holds NOW (``len()``) and
how many it has room for (``capacity``), the ``ScoreGraph`` that ``score_links`` keeps for it is sized by the latter and serves
every length, and ``group_extractable`` says which kinds of source a group's extraction can take in one launch per stage.

Shape: a random 30 x 40 rating graph of density 0.3 and five ratings, one hop with ``max_nodes_per_hop = 10`` (users have about
twelve ratings: the cap binds, so a link's position in its pass decides its subgraph), batches of 4 links, and
``latent_dim = [32, 32, 32, 32]`` -- the only width the kernels are built for."""
import os

import numpy as np
import pytest

from helpers import random_rating_graph

pytestmark = pytest.mark.gpu

B, CAPACITY, FIRST, SECOND = 4, 64, 37, 61          # 37 links: nine batches and a ragged one; 61: fifteen and a ragged one
CV = np.arange(1, 6, dtype=np.float64)


def _links(A):
    rows, cols = A.nonzero()
    return (rows, cols), np.asarray(A[rows, cols]).ravel().astype(np.int64) - 1


@pytest.fixture(scope='module')
def graph():
    A = random_rating_graph(30, 40, 0.3, 5, 21)
    assert np.diff(A.indptr).max() > 10          # the per-hop cap binds
    return A


@pytest.fixture(scope='module')
def dataset(graph):
    from igmc_amd.util_functions import MyDynamicDataset
    links, labels = _links(graph)
    return MyDynamicDataset('data/t/ls_dyn', graph, links, labels, 1, 1.0, 10, None, None, CV, seed=1)


@pytest.fixture(scope='module')
def passes(dataset):
    """Two passes of different lengths over ONE CandidateLinks of capacity 64 (what ScoreGraph's constructor saw of it is
    recorded), and the same two lists scored eagerly from fresh CandidateLinks of exactly their lengths."""
    import torch
    from igmc_amd import stepgraph
    from igmc_amd.models import IGMC
    from igmc_amd.recommend import CandidateLinks, score_candidates
    torch.manual_seed(4)
    model = IGMC(dataset, latent_dim=[32, 32, 32, 32], num_relations=5, num_bases=4, regression=True, adj_dropout=0.2,
                 seed=3).to('cuda')
    model.reset_parameters()
    model.eval()
    rng = np.random.default_rng(5)
    pairs = [(rng.integers(0, 30, n).astype(np.int32), rng.integers(0, 40, n).astype(np.int32)) for n in (FIRST, SECOND)]
    out = dict(built=[], lens=[], scores=[], eager=[])
    init = stepgraph.ScoreGraph.__init__

    def recording(self, model, ds, *args, **kw):
        out['built'].append((len(ds), ds.capacity))
        init(self, model, ds, *args, **kw)
        out['built'].append((len(ds), ds.capacity))

    cands = CandidateLinks(dataset, CAPACITY)
    stepgraph.ScoreGraph.__init__ = recording
    try:
        for u, v in pairs:
            cands.set_pairs(u, v)
            out['lens'].append(len(cands))
            out['scores'].append(score_candidates(model, cands, B).cpu().numpy())
            out['lens'].append(len(cands))
            out.setdefault('sg', []).append((cands._scoregraph, cands._scoregraph.graph))
    finally:
        stepgraph.ScoreGraph.__init__ = init
    before = os.environ.get('IGMC_NO_EVAL_GRAPH')
    os.environ['IGMC_NO_EVAL_GRAPH'] = '1'
    try:
        for u, v in pairs:
            fresh = CandidateLinks.from_pairs(dataset, u, v)
            assert fresh.capacity == len(fresh) == len(u)
            out['eager'].append(score_candidates(model, fresh, B).cpu().numpy())
            assert getattr(fresh, '_scoregraph', None) is None
    finally:
        if before is None:
            del os.environ['IGMC_NO_EVAL_GRAPH']
        else:
            os.environ['IGMC_NO_EVAL_GRAPH'] = before
    out['cands'] = cands
    return out


def test_the_scoregraph_is_sized_by_the_capacity_while_len_is_the_links_held(passes):
    cands = passes['cands']
    assert passes['built'] == [(FIRST, CAPACITY)] * 2          # built once; on entry and on exit the list said 37 of 64
    sg = cands._scoregraph
    assert sg.scores.numel() == CAPACITY and sg.labels.numel() == CAPACITY
    assert passes['lens'] == [FIRST, FIRST, SECOND, SECOND] and cands.capacity == CAPACITY
    assert [len(s) for s in passes['scores']] == [FIRST, SECOND]


def test_one_source_two_lengths_one_captured_graph(passes):
    (sg1, g1), (sg2, g2) = passes['sg']
    assert sg1 is sg2 and g1 is not None and g1 is g2
    for got, want in zip(passes['scores'], passes['eager']):
        assert got.dtype == np.float32 and np.isfinite(got).all()
        assert got.tobytes() == want.tobytes()


def test_group_extractable_by_source_kind(graph, dataset, tmp_path):
    from igmc_amd.explain import LeaveOneOutLinks
    from igmc_amd.recommend import CandidateLinks
    from igmc_amd.util_functions import MyDataset
    links, labels = _links(graph)
    static = MyDataset(str(tmp_path), graph, links, labels, 1, 1.0, 10, None, None, CV, seed=1)
    assert static._cache is not None and static.group_extractable is False
    assert LeaveOneOutLinks(dataset, 8, 64).group_extractable is False
    assert dataset.group_extractable is True
    assert CandidateLinks(dataset, 8).group_extractable is True

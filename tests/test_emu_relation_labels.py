"""The (relation count, label count) plane of the model step on the CPU emulation of the HIP sources: every row of
tests/relation_label_checks.py -- the geometry ``igmc_model_step_geometry`` answers (the emulator takes the clusters an
MI355X takes under ``IGMC_GS_CLUSTER=4``), the crafted extents, labels and relations through the real extraction, and eval
outputs, train outputs, loss and every gradient against ``oracle/pyg_ref`` with and without edge dropout; steps with Adam, one
per distinct tail; the one-launch tail against the two-launch tail bit for bit."""
import pytest

import relation_label_checks as RL
import parity_checks as PC


@pytest.fixture(scope='module')
def be():
    return PC.EmuBackend()


@pytest.fixture(autouse=True)
def _hooks(monkeypatch):
    for k in RL.HOOKS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('IGMC_GS_CLUSTER', '4')


def test_ring_graph_gives_rings_at_their_distance():
    """``ring_graph`` against a breadth-first search on the host: ring h of a block is at distance h of the link's ends, no
    rating joins rings further than one apart, every value 1 .. R occurs."""
    import numpy as np
    blocks = RL.blocks_of([(1, 1), (2, 3), (1, 11), (17, 16), (41, 41)], 4, 10)
    A, links = RL.ring_graph(blocks, 7)
    assert set(np.unique(A.data).astype(int)) == set(range(1, 8))
    At = A.T.tocsr()
    for (u, v), (U, V, _) in zip(links, blocks):
        assert A[u, v] != 0
        seen_u, seen_v, fu, fv = {int(u)}, {int(v)}, {int(u)}, {int(v)}
        for h in range(4):
            nv = {int(j) for i in fu for j in A.indices[A.indptr[i]:A.indptr[i + 1]]} - seen_v
            nu = {int(i) for j in fv for i in At.indices[At.indptr[j]:At.indptr[j + 1]]} - seen_u
            assert (len(nu), len(nv)) == (U[h], V[h]), (h, U, V)
            seen_u |= nu
            seen_v |= nv
            fu, fv = nu, nv
        assert len(seen_u) == 1 + sum(U) and len(seen_v) == 1 + sum(V)


def test_the_table_names_every_required_kind():
    assert RL.REQUIRED_KINDS <= RL.expected_kinds(), RL.REQUIRED_KINDS - RL.expected_kinds()


@pytest.mark.parametrize('drop', [False, True], ids=['nodrop', 'drop'])
@pytest.mark.parametrize('r', RL.ROWS, ids=[r.id for r in RL.ROWS])
def test_row_matches_oracle(be, r, drop):
    RL.check_row(be, r, drop)


@pytest.mark.parametrize('rid,what,fold', RL.TRAJECTORIES, ids=[t[0] for t in RL.TRAJECTORIES])
def test_steps_track_torch_adam(be, monkeypatch, rid, what, fold):
    r = RL.BY_ID[rid]
    if fold:      # ... and the same steps under the two-launch tail leave the same bits
        RL.check_tail_fold(be, r, monkeypatch)
    else:
        RL.check_trajectory(be, r)

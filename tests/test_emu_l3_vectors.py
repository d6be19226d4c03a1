"""Conv layer 3's weight gradient as centre vectors (``StepPlan::l3_vec``; igmc_amd/csrc/g2_subgraph.h, ``l3_vec_sum`` in
model.hip) against the per-workgroup tables it replaces (``IGMC_L3_VEC=0``), on the CPU emulation of the same sources.

``dPre_3`` lives on the two centre rows, so a cluster's layer-3 tables are one outer product a side.  In vector mode the member
that owns a centre stores the factors and both tails (``k_tail_ts``, ``k_tail_fin``) form the products where they add them, in
the order the table sums take.  Two training steps with Adam from one state must leave the SAME BITS either way: parameters,
both Adam moments, the flat gradient, predictions, the loss words, the epoch total and the weight images.

The cases are the smallest shapes at which the slot -> (member, subgraph) mapping can go wrong:

* clusters of 4 and of 2 (``IGMC_GS_CLUSTER``): the item centre's owner is member 2 and member 1;
* B = 1, 9, 17: slot strides 8, 16, 24 (slot ids with holes), cs x B slots below and above the 16 partial groups, subgraph
  counts that are no multiple of 16;
* both tails (``IGMC_TAIL_FOLD`` 1 / 0), with and without edge dropout;
* R = 5, and R = 3 (the last set of 16 columns is partly filled; vector rows 3 and 4 are never read);
* the first link of every run has a target item with a single rater (the user side is the centre row alone and the item
  centre's T_r are zeros), the second a target user with no other item (the item side likewise): B = 1 takes them as its
  two steps, every other B in its first batch.

The looping grid (fewer workgroups than subgraphs) and one workgroup per subgraph must still plan tables, and still step."""
import numpy as np
import pytest

import test_emu_tail_fold as F
from helpers import random_rating_graph
from igmc_amd import engine
from test_emu_tail_fold import be      # noqa: F401  (module-scoped fixture: the emulator backend)

STEPS = 2
_DATA = {}


def _data(R):
    """test_emu_tail_fold's graph on R rating levels, with an item only user 3 rated and a user who rated item 5 only; the links
    of those two first."""
    if R not in _DATA:
        A = random_rating_graph(44, 40, 0.3, R, seed=20).tolil()
        A[:, 39] = 0
        A[3, 39] = 2
        A[43, :] = 0
        A[43, 5] = R
        A = A.tocsr()
        A.eliminate_zeros()
        rows, cols = A.nonzero()
        lu, lv = rows.astype(np.int32).copy(), cols.astype(np.int32).copy()
        ly = np.asarray(A[rows, cols]).ravel().astype(np.float32)
        lone_item = int(np.flatnonzero((lu == 3) & (lv == 39))[0])
        lone_user = int(np.flatnonzero((lu == 43) & (lv == 5))[0])
        assert (lv == 39).sum() == 1 and (lu == 43).sum() == 1 and (lu == 3).sum() > 1 and (lv == 5).sum() > 1
        rest = np.random.default_rng(3).permutation(len(lu))
        rest = rest[(rest != lone_item) & (rest != lone_user)]
        perm = np.concatenate([[lone_item, lone_user], rest]).astype(np.int32)
        assert len(perm) >= 17 * STEPS
        _DATA[R] = (A, lu, lv, ly, perm)
    return _DATA[R]


def _plan(be, d, ws, B, cap):
    """``igmc_debug_l3_vectors`` for the workspace of a run on a new arena of the run's shape (hooks as the run left them)"""
    return ws.l3_vectors(engine.Batch(engine.Graph(d[0], lib=be.lib), B, 1, cap), B)


def _both(be, monkeypatch, R, B, cap, cs, grid, fold, drop):
    """STEPS steps in the default mode and under IGMC_L3_VEC=0 from the same state; the two plans' l3_vec"""
    monkeypatch.setattr(F, 'R', R)      # run_steps builds workspace and parameters from the module's constant
    d = _data(R)
    monkeypatch.delenv('IGMC_L3_VEC', raising=False)
    new, lab_new, ws = F.run_steps(be, d, monkeypatch, fold, B, cap, cs, grid, drop, 0.001, False, steps=STEPS)
    be.lib.call('igmc_model_check', ws.handle, None)      # no bounded wait ran out
    plan_new = _plan(be, d, ws, B, cap)
    monkeypatch.setenv('IGMC_L3_VEC', '0')
    old, lab_old, ws_old = F.run_steps(be, d, monkeypatch, fold, B, cap, cs, grid, drop, 0.001, False, steps=STEPS)
    plan_old = _plan(be, d, ws_old, B, cap)
    tail = 'k_tail_fin' if fold else 'k_tail_ts'
    assert lab_new.get(tail) == STEPS and lab_old.get(tail) == STEPS, (lab_new, lab_old)
    assert lab_new.get('k_graph_step') == STEPS and lab_old.get('k_graph_step') == STEPS
    for i, (a, b) in enumerate(zip(new, old)):
        for k in a:
            assert np.array_equal(a[k], b[k]), ('step', i, k, int((a[k] != b[k]).sum()), a[k].size)
        assert np.isfinite(a['P']).all() and np.isfinite(a['loss']).all()
    assert not np.array_equal(new[0]['P'], new[-1]['P']) and new[-1]['M2'].any()
    return plan_new, plan_old


#           R  B  cap          (cap: nodes a hop; 12 fits clusters of 2 and of 4)
SHAPES = [(5, 1, 12), (5, 9, 12), (5, 17, 12), (3, 9, 12), (3, 1, 12)]


@pytest.mark.parametrize('drop', [False, True], ids=['no_dropout', 'edge_dropout'])
@pytest.mark.parametrize('fold', [True, False], ids=['k_tail_fin', 'k_tail_ts'])
@pytest.mark.parametrize('cs', [4, 2])
@pytest.mark.parametrize('R,B,cap', SHAPES)
def test_centre_vectors_leave_the_bits_of_the_tables(be, monkeypatch, R, B, cap, cs, fold, drop):
    plan_new, plan_old = _both(be, monkeypatch, R, B, cap, cs, 0, fold, drop)
    assert plan_new == cs // 2, 'vector mode was not planned (item-centre member %d expected): %d' % (cs // 2, plan_new)
    assert plan_old == 0, 'IGMC_L3_VEC=0 did not plan tables'


@pytest.mark.parametrize('B,cap,cs,grid', [(17, 12, 1, 5), (7, 8, 1, 0)], ids=['looping_grid', 'one_workgroup'])
def test_slots_that_are_no_single_product_keep_their_tables(be, monkeypatch, B, cap, cs, grid):
    """A slot of the looping grid accumulates several subgraphs, one of a one-workgroup launch both sides' products."""
    plan_new, plan_old = _both(be, monkeypatch, 5, B, cap, cs, grid, True, True)
    assert plan_new == 0 and plan_old == 0

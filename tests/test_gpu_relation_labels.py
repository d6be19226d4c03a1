"""The (relation count, label count) plane of the model step on an MI355X: every row of tests/relation_label_checks.py with
no cluster hook (eight subgraphs take four workgroups each by themselves).

Per row and mask form: the crafted extents, labels and relations through the extraction kernels; the geometry
``igmc_model_step_geometry`` reports against the table; the kernels that actually launched (``igmc_profile_fetch``) against
the family it reports; eval outputs, train outputs, loss and every gradient tensor vs ``oracle/pyg_ref`` at the parity
tolerances; NaN sentinels behind the outputs untouched.  Then steps with Adam, one per distinct tail, vs
``pyg_ref.train_step`` + torch Adam -- for ``k_tail_fin`` (no row producers at R = 1; 6 and 8 layer-0 mains) also the bits of
the two-launch tail.  The device's figures: profiles/relation_label_observed.txt."""
import pytest

import relation_label_checks as RL
import parity_checks as PC

pytestmark = pytest.mark.gpu

REACHED = {}


@pytest.fixture(scope='module')
def be():
    import torch
    assert torch.cuda.is_available(), 'GPU tests need an MI355X'
    return PC.GpuBackend()


@pytest.fixture(autouse=True)
def _no_hooks(monkeypatch):
    for k in RL.HOOKS:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize('drop', [False, True], ids=['nodrop', 'drop'])
@pytest.mark.parametrize('r', RL.ROWS, ids=[r.id for r in RL.ROWS])
def test_row_matches_oracle(be, r, drop):
    geo, _ = RL.check_row(be, r, drop, kernels=True)
    REACHED[(r.id, drop)] = (geo, len(r.extents), 2 * r.hops + 2)


@pytest.mark.parametrize('rid,what,fold', RL.TRAJECTORIES, ids=[t[0] for t in RL.TRAJECTORIES])
def test_steps_track_torch_adam(be, monkeypatch, rid, what, fold):
    r = RL.BY_ID[rid]
    if fold:      # ... and the same steps under the two-launch tail leave the same bits
        RL.check_tail_fold(be, r, monkeypatch)
    else:
        RL.check_trajectory(be, r)


def test_the_table_covers_every_kind():
    """The subgraph kernel at L = 4, 6 and 8, the two-group dense kernels with and without the group split, the narrow dense
    layers with and without tables, the row walkers -- in the table, and among what the rows reached on the device."""
    want = RL.REQUIRED_KINDS
    assert want <= RL.expected_kinds(), want - RL.expected_kinds()
    if len(REACHED) == 2 * len(RL.ROWS):       # (the whole table ran in this session)
        got = RL.geometry_kinds(REACHED.values())
        assert want <= got, want - got

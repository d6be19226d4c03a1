"""Every Adam tail against float64 Adam, element by element, on the CPU emulation of the HIP sources (tests/adam_checks.py):
non-zero moments, Adam steps 1 / 7 / 100 000, weight decay and non-default betas / eps, the scalars as arguments and from the
control block (with the device's own advance and a learning rate changed between steps), and the weight images a
weight-decayed step leaves.  GPU twin: tests/test_gpu_adam_tails.py.

Shapes: the small graph of test_emu_tail_fold.py, batches of 7 (per-hop cap 12) and -- the subgraph rows -- of 17 with clusters
of 4 (cap 16): 68 table slots, a partly filled set."""
import pytest

import adam_checks as AC
import parity_checks as PC
from adam_checks import H0, H1


@pytest.fixture(scope='module')
def be():
    return PC.EmuBackend()


CASES, IDS = AC.CASES, AC.IDS


@pytest.mark.parametrize('row,B,drop,hyp,ts,t_ctrl', CASES, ids=IDS)
def test_scalars_as_arguments(be, monkeypatch, row, B, drop, hyp, ts, t_ctrl):
    for t in ts:
        AC.check_step(be, monkeypatch, row, B, drop, hyp, t, 'args')


@pytest.mark.parametrize('row,B,drop,hyp,ts,t_ctrl', CASES, ids=IDS)
def test_scalars_from_the_control_block_three_steps_and_a_new_learning_rate(be, monkeypatch, row, B, drop, hyp, ts, t_ctrl):
    """The block carries ``hyp``, the arguments the other set: a kernel that reads an argument it should not fails the
    identity.  After every step the device's own advance is read back; the third step runs on ``lr x 0.1`` written into the
    block the way ``StepGraph.begin_epoch`` does."""
    AC.check_step(be, monkeypatch, row, B, drop, hyp, t_ctrl, 'ctrl')


@pytest.mark.parametrize('n', [1, 2047, 2049, 49233])
@pytest.mark.parametrize('hyp', [H0, H1], ids=['H0', 'H1'])
def test_flat_adam(be, n, hyp):
    for t in AC.T_STEPS:
        AC.check_flat_adam(be, n, hyp, t)
    AC.check_flat_adam(be, n, hyp, 7, route='ctrl')


@pytest.mark.parametrize('row,B,drop', [('fold_cs1', 7, True), ('fold_cs4', 17, False), ('ts_cs2', 7, True), ('dense_r5', 7, True)])
def test_weight_images_left_by_a_weight_decayed_step_equal_the_composed_ones(be, monkeypatch, row, B, drop):
    AC.check_images(be, monkeypatch, row, B, drop)

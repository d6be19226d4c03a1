"""The head of the subgraph kernel (igmc_amd/csrc/g2_subgraph.h) under clusters of 1, 2 and 4 workgroups per subgraph, on the
CPU emulation of the same sources, which runs the members of a cluster together: what the head leaves behind -- a1, lmask, dz,
feat, gfeat, out -- is complete and right whichever member writes it, launches repeat bit for bit, no bounded wait times out.
Every member computes the whole head and member 0 stores it: a split of the head over the members, which this file is named
for, was measured and not adopted (profiles/r07_experiments/README.md).  What the file guards: the head's results under every cluster size, and -- through
the bias gradients of ``run_model_parity``, on ``hand`` with idle bundles in every workgroup -- d bias_l as the backward
epilogues form it.  Cases: ``hand`` (3 x 4 nodes: with 2 or 4 members, members
WITHOUT an active bundle still run the head), ``synth_cap`` (a few bundles: every cluster size takes it) and
``synth_nocap:100`` (up to 101 nodes a side, the headline shape: clusters of four)."""
import numpy as np
import pytest

import head_split_checks as HS
import parity_checks as PC
from helpers import load_extract_golden

CASES = load_extract_golden()


@pytest.fixture(scope='module')
def be():
    return PC.EmuBackend()


@pytest.fixture(autouse=True)
def _graph_step_path(monkeypatch):
    monkeypatch.setenv('IGMC_GRAPH_STEP', '1')


def sub(name, n):
    name, _, cap = name.partition(':')
    case = dict(CASES[name])
    if cap:
        case['mnph'] = int(cap)
    case['recs'], case['links'], case['link_labels'] = case['recs'][:n], case['links'][:n], case['link_labels'][:n]
    return case


def test_the_cases_are_what_they_are_meant_to_be():
    hand = sub('hand', 5)
    assert max(hand['A'].shape) <= 16                 # one bundle a side: members 1.. of a cluster have no active bundle
    big = sub('synth_nocap:100', 4)
    assert big['mnph'] == 100


@pytest.mark.parametrize('cs', ['1', '2', '4'])
@pytest.mark.parametrize('name,n,drop', [('hand', 5, True), ('synth_cap', 6, True), ('synth_nocap:100', 4, True), ('synth_nocap:100', 4, False)])
def test_head_under_clusters(be, monkeypatch, capfd, cs, name, n, drop):
    """Evaluation and training forward, loss and EVERY gradient against the oracle with the tolerances
    ``run_model_parity`` asserts (d lin1 / d lin2 come from a1 / lmask / dz / feat as the members left them); the head's
    arrays read back and checked unit by unit; two more launches bit-identical to each other and to the first; no
    bounded wait timed out."""
    monkeypatch.setenv('IGMC_GS_CLUSTER', cs)
    monkeypatch.setenv('IGMC_GS_TRACE', '1')
    res = PC.run_model_parity(be, sub(name, n), R=5, use_dropout=drop)
    err = capfd.readouterr().err
    # (a cluster of cs workgroups holds 32 cs rows a side: the 101-node shape needs four members -- the smaller clusters
    #  hand it to the dense-layer kernels and their head kernel; the parity and the array checks hold there as well)
    on_subgraph_kernel = res['ws'].dense_path(res['batch'], n) and 'k_graph_step B=%d train=1' % n in err
    assert on_subgraph_kernel == (name != 'synth_nocap:100' or cs == '4'), err[-400:]
    if on_subgraph_kernel:
        assert 'k_graph_step B=%d train=0' % n in err and 'cluster=%s ' % cs in err, err[-400:]
    assert res['worst_grad_err'] < PC.GRAD_TOL
    if name.startswith('synth_nocap'):
        d = res['d']
        sizes, nu = np.diff(np.asarray(d['node_off'])), np.asarray(d['n_users'])
        assert max(nu.max(), (sizes - nu).max()) == 101
    arr = HS.head_arrays(be, res['ws'], res['d']['B'])
    HS.check_head_arrays(arr, res)
    r1 = HS.relaunch(be, res, drop)
    r2 = HS.relaunch(be, res, drop)
    HS.check_bit_identical(r1, r2)
    assert np.array_equal(r1['out'], res['train_out']) and np.array_equal(r1['loss'], res['loss'])
    for k in arr:
        assert np.array_equal(arr[k], r1[k]), k
    HS.check_error_word(be, res['ws'])


def test_cluster_sizes_agree(be, monkeypatch):
    """The same batch under cs = 1, 2, 4: each within the oracle's tolerances (asserted by ``run_model_parity``), hence
    within twice that of each other; the sums over the units are taken in another order, so not bit for bit."""
    runs = {}
    for cs in ('1', '2', '4'):
        monkeypatch.setenv('IGMC_GS_CLUSTER', cs)
        runs[cs] = PC.run_model_parity(be, sub('synth_nocap:100', 4), R=5, use_dropout=True)
    for cs in ('2', '4'):
        assert PC.rel_err(runs[cs]['train_out'], runs['1']['train_out']) < 2 * PC.OUT_TOL
        assert PC.rel_err(runs[cs]['eval_out'], runs['1']['eval_out']) < 2 * PC.OUT_TOL
        for k, g in runs['1']['grads'].items():
            assert PC.rel_err(runs[cs]['grads'][k], g) < 2 * PC.GRAD_TOL, k

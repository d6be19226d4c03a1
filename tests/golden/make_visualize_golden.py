"""Golden vectors of ``--visualize`` produced by the reference's OWN code (``train_eval.visualize`` ``:248-322`` and
``util_functions.PyGGraph_to_nx`` ``:314-324``, UNMODIFIED).

Run where the reference is checked out (the place ``make_model_golden.py`` imports it from; needs no GPU):

    python tests/golden/make_visualize_golden.py

The reference is imported as in ``make_model_golden.py`` (the ``torch_geometric`` stand-in of ``oracle/ref_stub``).  File
``tests/golden/visualize_golden.npz``, keys ``<case>/...``; cases:

* ``igmc_r5``    the synthetic MovieLens-shaped 300 x 200 graph and the model of ``model_golden``'s ``igmc_r5`` (R = 5), 450
                 links, hop 1, UNCAPPED;
* ``igmc_r10``   flixster (bundled, R = 10) and the model of ``model_golden``'s ``igmc_r10``, its first 450 training links,
                 hop 1, uncapped.

Uncapped, because the engine's sampler is not the reference's ``random.sample``: where the cap does not bind both extract the
same subgraphs, and a dataset of these links reproduces what the reference scored.  450 links are nine batches of 50, so the
engine's scoring pass goes through its graph-replayed pipeline.

Per case: the links, labels, class values and the model's ``state_dict``; ``scores`` / ``ys`` -- what the reference's
``visualize`` scored (its ``R`` and ``Y``: a forward hook on the model, and the labels of the graphs in loader order) --;
``highest`` / ``lowest`` -- the dataset positions of the graphs it handed to ``PyGGraph_to_nx``, in that order (a recording
proxy around ``train_eval.PyGGraph_to_nx``: the selection, ``:262-272``, is complete before any plotting call; whatever the
plotting half then does on the installed matplotlib is caught) -- and ``num``.

``num`` is the largest value <= 5 for which the reference's selection is DECIDED at the precision the engine is held to: every
gap between consecutive scores among the ``num + 1`` lowest, and among the ``num + 1`` highest, exceeds 100 x the output
tolerance of the suite (``tests/parity_checks.py``: 2e-5 of the peak).  That covers the gap at the selection boundary (which
graphs are selected) and the gaps inside (in which order they are listed); below it, an engine within tolerance of the
reference may legitimately swap two links, and the reference's own pick among equal scores is an implementation detail of
``np.argsort``.  A case without such a ``num`` is dropped; fewer than two cases left is an error.

``nx/<k>/...``: for a few graphs of both cases, the input (``label``, ``edge_index``, ``edge_type``, ``y``) and what the
reference's ``PyGGraph_to_nx`` makes of it (``nodes`` in iteration order, ``node_type`` per node, ``edges`` as rows
(u, v, type) in iteration order, ``rating``).
"""
import os
import sys
import tempfile
import warnings

import numpy as np
import torch

warnings.simplefilter('ignore')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
os.environ.setdefault('MPLBACKEND', 'Agg')
import make_model_golden as MG  # noqa: E402  (sets up the paths of the reference and of the stand-in)
from make_model_golden import REF_M, REF_T, REF_U, ROOT  # noqa: E402
from igmc_amd import preprocessing  # noqa: E402

OUT_TOL = 2e-5          # tests/parity_checks.py: outputs within 2e-5 of the peak
GAP_FACTOR = 100.0
N_LINKS = 450


def decided_num(scores, max_num=5):
    """Largest num <= max_num whose selection (members and order, both ends) no error below GAP_FACTOR * OUT_TOL * peak can
    change; 0 if none."""
    s = np.sort(np.asarray(scores, np.float64))
    need = GAP_FACTOR * OUT_TOL * np.abs(s).max()          # (parity_checks.rel_err: relative to the peak)
    for num in range(min(max_num, len(s) - 1), 0, -1):
        low, high = np.diff(s[:num + 1]), np.diff(s[-(num + 1):])
        if low.min() > need and high.min() > need:
            return num, need, float(min(low.min(), high.min()))
    return 0, need, 0.0


def run_reference_visualize(model, graphs, class_values, num, data_name):
    """The reference's ``visualize`` with a recording proxy around ``PyGGraph_to_nx`` and a forward hook on the model."""
    index_of = {id(g): i for i, g in enumerate(graphs)}
    picked, outs = [], []
    real = REF_T.PyGGraph_to_nx

    def proxy(data):
        picked.append(index_of[id(data)])
        return real(data)

    hook = model.register_forward_hook(lambda m, i, o: outs.append(o.detach().view(-1).numpy().astype(np.float32).copy()))
    REF_T.PyGGraph_to_nx = proxy
    plotted = True
    try:
        with tempfile.TemporaryDirectory() as td:
            try:
                REF_T.visualize(model, graphs, td, data_name, class_values, num=num, sort_by='prediction')
            except Exception as e:      # noqa: BLE001  (the plotting half on a matplotlib newer than the reference's)
                if len(picked) != 2 * min(num, len(graphs)):
                    raise
                plotted = False
                print('  (plotting half of the reference raised %s: %s -- the selection was complete)' % (type(e).__name__, e))
    finally:
        REF_T.PyGGraph_to_nx = real
        hook.remove()
    n = min(num, len(graphs))
    return np.concatenate(outs), picked[:n], picked[n:2 * n], plotted


def build_case(out, case, A, links, labels, cv, model):
    graphs, _ = MG.extract(A, links, labels, cv, 1, None, seed=1)
    ys = np.array([float(g.y.item()) for g in graphs], np.float32)
    # pass 1 with num = 5: the scores do not depend on num; then the num that is decided, and the selection for it
    scores, _, _, _ = run_reference_visualize(model, graphs, cv, 5, case)
    assert len(scores) == len(graphs)
    num, need, gap = decided_num(scores)
    print('%s: %d links, peak %.4f, required gap %.3e, num = %d (smallest gap at that num %.3e)' % (
        case, len(graphs), np.abs(scores).max(), need, num, gap))
    if num < 1:
        print('  dropped: no num >= 1 with a decided selection')
        return False, graphs
    scores2, highest, lowest, plotted = run_reference_visualize(model, graphs, cv, num, case)
    assert np.array_equal(scores, scores2)
    order = np.argsort(scores, kind='stable')
    assert lowest == order[:num].tolist() and highest == order[-num:][::-1].tolist()      # (decided: any argsort agrees)
    out[case + '/links'] = np.asarray(links, np.int32).reshape(-1, 2)
    out[case + '/link_labels'] = np.asarray(labels, np.int32)
    out[case + '/class_values'] = np.asarray(cv, np.float64)
    out[case + '/graph_fingerprint'] = np.array(MG.graph_fingerprint(A), np.uint64)
    MG.put_state(out, case + '/state', MG.state_np(model))
    out[case + '/scores'] = scores.astype(np.float32)
    out[case + '/ys'] = ys
    out[case + '/num'] = np.array(num)
    out[case + '/highest'] = np.asarray(highest, np.int32)
    out[case + '/lowest'] = np.asarray(lowest, np.int32)
    out[case + '/required_gap'] = np.array(need)
    out[case + '/reference_plotted'] = np.array(int(plotted))
    return True, graphs


def put_nx(out, k, data):
    g = REF_U.PyGGraph_to_nx(data)
    p = 'nx/%d/' % k
    out[p + 'label'] = data.x.argmax(1).numpy().astype(np.uint8)
    out[p + 'n_labels'] = np.array(data.x.shape[1])
    out[p + 'edge_index'] = data.edge_index.numpy().astype(np.int32)
    out[p + 'edge_type'] = data.edge_type.numpy().astype(np.uint8)
    out[p + 'y'] = data.y.numpy().astype(np.float32)
    nodes = list(g.nodes())
    out[p + 'nodes'] = np.asarray(nodes, np.int32)
    out[p + 'node_type'] = np.asarray([g.nodes[v]['type'] for v in nodes], np.int32)
    out[p + 'edges'] = np.asarray([(u, v, t) for u, v, t in g.edges(data='type')], np.int32).reshape(-1, 3)
    out[p + 'rating'] = np.array(g.graph['rating'], np.float64)


def case_r5(out):
    A, _, _ = MG.synth_graph()
    u, v, r = preprocessing.synth_ml(300, 200, 9000, preprocessing.ML_HIST['ml_100k'][3], seed=3)
    pick = np.random.default_rng(17).choice(len(u), N_LINKS, replace=False)
    links, labels = list(zip(u[pick].tolist(), v[pick].tolist())), (r[pick].astype(int) - 1).tolist()
    cv = np.array([1., 2., 3., 4., 5.])
    probe, _ = MG.extract(A, links[:2], labels[:2], cv, 1, None, seed=1)
    model = REF_M.IGMC(probe, latent_dim=[32, 32, 32, 32], num_relations=5, num_bases=4, regression=True,
                       adj_dropout=0.2, force_undirected=False, side_features=False, n_side_features=0, multiply_by=1)
    MG.perturb(model, 1)
    return build_case(out, 'igmc_r5', A, links, labels, cv, model)


def case_r10(out):
    os.chdir(ROOT)
    (_, _, adj, tr_l, tr_u, tr_v, _, _, _, _, _, _, cv) = preprocessing.load_data_monti('flixster', testing=True)
    links, labels = list(zip(tr_u[:N_LINKS].tolist(), tr_v[:N_LINKS].tolist())), tr_l[:N_LINKS].tolist()
    assert len(cv) == 10
    probe, _ = MG.extract(adj, links[:2], labels[:2], cv, 1, None, seed=1)
    model = REF_M.IGMC(probe, latent_dim=[32, 32, 32, 32], num_relations=10, num_bases=4, regression=True,
                       adj_dropout=0.2, force_undirected=False, side_features=False, n_side_features=0, multiply_by=1)
    MG.perturb(model, 3)
    return build_case(out, 'igmc_r10', adj, links, labels, cv, model)


def main():
    out, kept, k = {}, [], 0
    for fn in (case_r5, case_r10):
        ok, graphs = fn(out)
        if ok:
            kept.append(fn.__name__)
        sizes = np.array([g.num_nodes for g in graphs])
        # a few graphs of each case: the smallest, the largest, and two in between
        for i in sorted(set([int(sizes.argmin()), int(sizes.argmax()), 0, len(graphs) // 2])):
            put_nx(out, k, graphs[i])
            k += 1
    out['nx/count'] = np.array(k)
    if len(kept) < 2:
        raise SystemExit('fewer than two cases with a decided selection: pick other seeds or cases')
    path = os.path.join(HERE, 'visualize_golden.npz')
    np.savez_compressed(path, **out)
    print('wrote %s (%d keys, %.1f KB)' % (path, len(out), os.path.getsize(path) / 1024.0))


if __name__ == '__main__':
    main()

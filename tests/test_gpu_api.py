"""The reference-shaped Python surface on a real MI355X: datasets, IGMC module, train/eval loops, checkpoints,
the differentiable forward, and RMSE parity of a fixed checkpoint against the oracle (tolerance 1e-4, the
north_star's bar, on identical inputs)."""
import math
import os

import numpy as np
import pytest

from helpers import ROOT, batch_to_pyg, load_extract_golden

pytestmark = pytest.mark.gpu
CASES = load_extract_golden()


@pytest.fixture(scope='module')
def flix():
    import torch
    assert torch.cuda.is_available()
    from igmc_amd import preprocessing
    return preprocessing.load_data_monti('flixster', testing=True)


def make_sets(split, ntr=600, nte=300, dynamic=True, mnph=10000):
    from igmc_amd.util_functions import MyDataset, MyDynamicDataset
    (uf, vf, adj, trl, tru, trv, _, _, _, tel, teu, tev, cv) = split
    cls = MyDynamicDataset if dynamic else MyDataset
    tr = cls('data/t/train', adj, (tru[:ntr], trv[:ntr]), trl[:ntr], 1, 1.0, mnph, None, None, cv)
    te = MyDataset('data/t/test', adj, (teu[:nte], tev[:nte]), tel[:nte], 1, 1.0, mnph, None, None, cv)
    return tr, te, cv


def test_extraction_api_known_answer():
    from igmc_amd.util_functions import SparseColIndexer, SparseRowIndexer, construct_pyg_graph, \
        subgraph_extraction_labeling
    c = CASES['hand']
    Arow, Acol = SparseRowIndexer(c['A']), SparseColIndexer(c['A'].tocsc())
    out = subgraph_extraction_labeling((0, 1), Arow, Acol, 1, 1.0, None, None, None, c['class_values'], 1)
    u, v, r, labels, ml, y, nf = out
    # same graph as the reference's known answer up to the order of non-target nodes
    assert labels == [0, 2, 1, 3, 3] and ml == 3 and y == 2.0 and nf is None
    d = construct_pyg_graph(*out)
    assert sorted(zip(d.edge_index[0].tolist(), d.edge_index[1].tolist(), d.edge_type.tolist())) == \
        sorted(zip([0, 0, 1, 3, 4, 2], [3, 4, 2, 0, 0, 1], [0, 4, 2, 0, 4, 2]))


def test_dataset_surface(flix):
    import torch
    tr, te, cv = make_sets(flix)
    assert len(tr) == 600 and tr.num_features == 4 and tr.__class__.__name__ == 'MyDynamicDataset'
    d = tr[3]
    assert d.x.shape[1] == 4 and d.edge_index.shape[0] == 2 and d.edge_type.shape[0] == d.edge_index.shape[1]
    assert float(d.y) == float(cv[flix[3][3]])
    assert d.x[0].tolist() == [1, 0, 0, 0]
    # the static dataset (reference MyDataset, util_functions.py:69-110): indexable, same Data layout, and -- the
    # flixster default cap never binds -- the SAME subgraph as the dynamic dataset / as links2subgraphs yield
    from igmc_amd.util_functions import MyDataset, SparseColIndexer, SparseRowIndexer, links2subgraphs
    assert te.__class__.__name__ == 'MyDataset' and len(te) == 300 and te.num_features == 4
    s0 = te[7]
    assert s0.x.shape[1] == 4 and s0.edge_index.shape == (2, s0.edge_type.shape[0]) and float(s0.y) == float(cv[flix[9][7]])
    assert s0.x[0].tolist() == [1, 0, 0, 0] and int(s0.x[:, 1].sum()) == 1
    (uf, vf, adj, trl, tru, trv, _, _, _, tel, teu, tev, _) = flix
    st = MyDataset('data/t/train_static', adj, (tru[:600], trv[:600]), trl[:600], 1, 1.0, 10000, None, None, cv)
    a, b = st[3], tr[3]
    assert torch.equal(a.x, b.x) and torch.equal(a.edge_index, b.edge_index) and torch.equal(a.edge_type, b.edge_type)
    graphs = links2subgraphs(SparseRowIndexer(adj), SparseColIndexer(adj.tocsc()), (tru[:40], trv[:40]), trl[:40], 1, 1.0,
                             10000, None, None, cv, batch_size=16)
    assert len(graphs) == 40
    g3 = graphs[3]
    assert torch.equal(g3.x, a.x) and float(g3.y) == float(a.y) and g3.edge_type.shape == a.edge_type.shape
    # same edge multiset (links2subgraphs emits the reference's [u;v],[v;u] order, the dataset the dst-sorted CSR)
    key = lambda e, t: sorted(zip(e[0].tolist(), e[1].tolist(), t.tolist()))
    assert key(g3.edge_index, g3.edge_type) == key(a.edge_index, a.edge_type)


def test_train_eval_checkpoint_roundtrip(flix, tmp_path):
    import torch
    from igmc_amd.models import IGMC
    from igmc_amd.train_eval import DataLoader, eval_rmse, test_once, train_multiple_epochs
    tr, te, cv = make_sets(flix)
    torch.manual_seed(1)
    model = IGMC(tr, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True,
                 adj_dropout=0.2, multiply_by=1)
    logs = []

    def logger(info, m, opt):
        logs.append(dict(info))
        if m is not None:
            torch.save(m.state_dict(), str(tmp_path / ('model_checkpoint%d.pth' % info['epoch'])))
            torch.save(opt.state_dict(), str(tmp_path / ('optimizer_checkpoint%d.pth' % info['epoch'])))
    rmse = train_multiple_epochs(tr, te, model, 3, 50, 1e-3, 0.1, 2, 0, ARR=0.001, test_freq=1, logger=logger,
                                 res_dir=str(tmp_path))
    assert len(logs) == 3 and math.isfinite(rmse) and rmse == logs[-1]['test_rmse']
    assert logs[0]['train_loss'] > logs[-1]['train_loss'] > 0          # it learns
    sd = torch.load(str(tmp_path / 'model_checkpoint3.pth'))
    want = {}
    for l in range(4):
        fin = 4 if l == 0 else 32
        want.update({'convs.%d.basis' % l: (4, fin, 32), 'convs.%d.att' % l: (len(cv), 4),
                     'convs.%d.root' % l: (fin, 32), 'convs.%d.bias' % l: (32,)})
    want.update({'lin1.weight': (128, 256), 'lin1.bias': (128,), 'lin2.weight': (1, 128), 'lin2.bias': (1,)})
    assert {k: tuple(v.shape) for k, v in sd.items()} == want           # reference state_dict contract
    assert list(sd.keys())[:4] == ['convs.0.basis', 'convs.0.att', 'convs.0.root', 'convs.0.bias']
    osd = torch.load(str(tmp_path / 'optimizer_checkpoint3.pth'), weights_only=False)
    assert osd['param_groups'][0]['lr'] == pytest.approx(1e-4) and len(osd['state']) == 20
    # reload into a fresh model: identical eval RMSE
    m2 = IGMC(tr, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True).to('cuda')
    m2.load_state_dict(sd)
    r2 = test_once(te, m2, 50)
    assert r2 == pytest.approx(rmse, abs=1e-6)
    # resume (reference --continue-from): runs and keeps improving or at least stays finite
    r3 = train_multiple_epochs(tr, te, m2, 4, 50, 1e-3, 0.1, 50, 0, ARR=0.001, logger=None, continue_from=3,
                               res_dir=str(tmp_path))
    assert math.isfinite(r3)


def test_eval_rmse_matches_oracle_within_1e4(flix):
    """Fixed checkpoint, fixed (static) test set: RMSE equals the PyG-restatement's within 1e-4."""
    import torch
    from igmc_amd.models import IGMC
    from igmc_amd.train_eval import DataLoader, eval_rmse
    from oracle import pyg_ref
    tr, te, cv = make_sets(flix, nte=200)
    torch.manual_seed(3)
    model = IGMC(tr, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True).to('cuda')
    model.reset_parameters()
    loader = DataLoader(te, 50, shuffle=False)
    rmse = eval_rmse(model, loader, 'cuda')
    ref = pyg_ref.IGMCRef(4, (32, 32, 32, 32), len(cv), 4, adj_dropout=0.2, fast=True)
    ref.load_state_dict({k: v.detach().cpu() for k, v in model.state_dict().items()})
    sse, n = 0.0, 0
    for data in DataLoader(te, 50, shuffle=False):
        raw = data._materialise()['raw']
        s, _ = pyg_ref.eval_sse(ref, batch_to_pyg(raw, 4))
        sse += s
        n += raw['B']
    assert n == 200
    assert rmse == pytest.approx(math.sqrt(sse / n), abs=1e-4)


def test_differentiable_forward_matches_fused_path(flix):
    """Foreign training loops: model(data) -> loss.backward() gives the same gradients as the fused kernel path."""
    import torch
    import torch.nn.functional as F
    from igmc_amd.models import IGMC
    from igmc_amd.train_eval import DataLoader
    tr, te, cv = make_sets(flix, dynamic=False)
    torch.manual_seed(5)
    model = IGMC(tr, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True,
                 adj_dropout=0.0).to('cuda')
    model.reset_parameters()
    data = next(iter(DataLoader(tr, 50, shuffle=False)))
    model.train()
    model._step = 10
    out = model(data)
    loss = F.mse_loss(out, data.y.view(-1))
    loss.backward()
    g_auto = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    step_used = model._step
    # fused path with the same MLP-dropout key (seed, step)
    ws = model._workspace(data)
    flat = model.flat_parameters()
    grad = torch.zeros_like(flat)
    outb, lossb = torch.empty(50, device='cuda'), torch.zeros(2, device='cuda')
    ws.loss_grad(flat.data_ptr(), data.arena, outb.data_ptr(), grad.data_ptr(), lossb.data_ptr(), seed=model.seed,
                 step=step_used, ARR=0.0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert lossb[0].item() == pytest.approx(loss.item(), rel=1e-5)
    where = {k: (o, n, s) for (k, o, n, s) in model._views}
    for k, g in g_auto.items():
        o, n, s = where[k]
        assert torch.allclose(g.reshape(-1), grad[o:o + n], rtol=1e-4, atol=1e-6), k
    # a torch optimiser can drive it
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    before = model.flat_parameters().clone()
    opt.step()
    assert not torch.equal(before, model.flat_parameters())


def test_ensemble_eval(flix, tmp_path):
    import torch
    from igmc_amd.models import IGMC
    from igmc_amd.train_eval import test_once
    tr, te, cv = make_sets(flix, nte=100)
    paths = []
    for i in range(3):
        torch.manual_seed(10 + i)
        m = IGMC(tr, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True).to('cuda')
        m.reset_parameters()
        p = str(tmp_path / ('model_checkpoint%d.pth' % i))
        torch.save(m.state_dict(), p)
        paths.append(p)
    m = IGMC(tr, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True).to('cuda')
    singles = []
    for p in paths:
        m.load_state_dict(torch.load(p))
        singles.append(test_once(te, m, 50))
    ens = test_once(te, m, 50, ensemble=True, checkpoints=paths)
    assert math.isfinite(ens) and ens <= max(singles) + 1e-6
    # oracle: mean of the checkpoints' predictions, then RMSE (reference train_eval.py:208-245), on the subgraphs
    # the engine extracted (static test set -> the same subgraphs every pass)
    from igmc_amd.train_eval import DataLoader
    from oracle import pyg_ref
    batches = [batch_to_pyg(data._materialise()['raw'], 4) for data in DataLoader(te, 50, shuffle=False)]
    ys = torch.cat([b.y for b in batches])
    preds, ref_singles = [], []
    for p in paths:
        ref = pyg_ref.IGMCRef(4, (32, 32, 32, 32), len(cv), 4, adj_dropout=0.2, fast=True)
        ref.load_state_dict({k: v.cpu() for k, v in torch.load(p).items()})
        out = torch.cat([pyg_ref.eval_sse(ref, b)[1] for b in batches])
        preds.append(out)
        ref_singles.append(math.sqrt(float(((out - ys) ** 2).mean())))
    ref_ens = math.sqrt(float(((torch.stack(preds, 1).mean(1) - ys) ** 2).mean()))
    assert len(ys) == 100
    assert singles == pytest.approx(ref_singles, abs=1e-4)
    assert ens == pytest.approx(ref_ens, abs=1e-4)


def test_main_script_end_to_end(tmp_path):
    """Main.py flags / result files (reference Main.py:31-45,188-210) on yahoo_music, --debug sized."""
    import subprocess
    import sys
    from helpers import ROOT
    cmd = [sys.executable, os.path.join(ROOT, 'Main.py'), '--data-name', 'yahoo_music', '--epochs', '2', '--testing',
           '--save-interval', '1', '--debug', '--dynamic-train', '--ensemble', '--save-appendix', '_t',
           '--max-nodes-per-hop', '200']
    # ensemble of range(epochs-30..): with 2 epochs the reference schedule needs checkpoints we do not have;
    # run without --ensemble for the end-to-end check of files and log format
    cmd.remove('--ensemble')
    env = dict(os.environ, PYTHONPATH=ROOT)
    # raw_data is looked up relative to cwd first, then next to the package
    r = subprocess.run(cmd, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-3000:]
    res = tmp_path / 'results' / 'yahoo_music_t_testmode'
    lines = (res / 'log.txt').read_text().strip().split('\n')
    assert len(lines) == 3 and lines[0].startswith('Epoch 1, train loss ')
    float(lines[-1].split(' ')[-1])                      # summarize_fdy.py:25-26 parses the last token
    assert (res / 'model_checkpoint2.pth').exists() and (res / 'optimizer_checkpoint2.pth').exists()
    assert (res / 'cmd_input.txt').exists()


def test_step_gate_waits_for_the_step_counter():
    """igmc_ctrl_gate: a one-wave kernel on the extraction chain's stream that ends when the running group has done its
    gk_min steps (the tick of a step on ANOTHER stream releases it), when that group is over, or after its timeout -- a
    pacing hint without a graph edge out of the step chain."""
    import ctypes as C
    import time
    import torch
    from igmc_amd import _lib
    lib = _lib.load()
    vp = lambda t: C.c_void_p(t.data_ptr())
    ctrl = torch.zeros(_lib.CTRL['WORDS'], dtype=torch.int64, device='cuda')
    main = torch.cuda.current_stream()
    lib.call('igmc_ctrl_regroup', vp(ctrl), 4, 0, 200, C.c_void_p(main.cuda_stream))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()

    def gate(q, gk, timeout_us, delay_us=0.0, always=0):
        lib.call('igmc_ctrl_gate', vp(ctrl), q, gk, float(delay_us), always, float(timeout_us), C.c_void_p(side.cuda_stream))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        side.synchronize()
        return time.perf_counter() - t0
    # nothing to wait for: no step needed / the other parity's group is not the running one
    assert timed(lambda: gate(0, 0, 50000)) < 0.02
    assert timed(lambda: gate(1, 3, 50000)) < 0.02
    # a step that never comes: the gate gives up after its timeout (and not before)
    dt = timed(lambda: gate(0, 1, 20000))
    assert 0.018 < dt < 0.2, dt

    # released by the tick of a step on the other stream
    def released():
        gate(0, 1, 500000)
        time.sleep(0.01)
        assert not side.query()              # still polling
        lib.call('igmc_ctrl_tick', vp(ctrl), C.c_void_p(main.cuda_stream))
    dt = timed(released)
    assert 0.009 < dt < 0.2, dt
    assert int(ctrl[_lib.CTRL['GK']].item()) == 1
    # ... and once the group of parity 0 is over (4 ticks: gq flips), its gates pass whatever they asked for
    for _ in range(3):
        lib.call('igmc_ctrl_tick', vp(ctrl), C.c_void_p(main.cuda_stream))
    torch.cuda.synchronize()
    assert int(ctrl[_lib.CTRL['GQ']].item()) == 1
    assert timed(lambda: gate(0, 3, 500000)) < 0.02
    # the delay behind the step: only for a gate that had to wait, or on request
    lib.call('igmc_ctrl_regroup', vp(ctrl), 4, 0, 200, C.c_void_p(main.cuda_stream))
    torch.cuda.synchronize()
    t_no, t_always = min(timed(lambda: gate(0, 0, 50000, delay_us=1000.0)) for _ in range(5)), \
        min(timed(lambda: gate(0, 0, 50000, delay_us=1000.0, always=1)) for _ in range(5))
    assert t_no < 0.0009 and 0.001 <= t_always < 0.02, (t_no, t_always)
    with pytest.raises(Exception):
        lib.call('igmc_ctrl_gate', None, 0, 0, 0.0, 0, 1.0, None)
    with pytest.raises(Exception):
        lib.call('igmc_ctrl_gate', vp(ctrl), 0, 0, 5000.0, 0, 1.0, None)


def test_step_graph_paths_agree(flix, monkeypatch):
    """The captured single-GPU step (igmc_train_step inside a hipGraph, the next group's extraction on a second stream;
    groups of 4 steps per graph launch here, one step per launch with IGMC_GROUP_STEPS=1), the eager step, and the
    multi-GPU step (igmc_train_step_dp: the single-GPU step's kernels with the exchange of the reduced gradient sources on a
    one-rank RCCL communicator between the reduction and the gradient / Adam kernel, captured into the same groups; dp_flat:
    gradient kernels -> igmc_allreduce_grads -> igmc_step_finish) must walk the same trajectory.  flixster has R = 10: the
    per-layer kernels take these steps."""
    import torch
    from igmc_amd.models import IGMC
    from igmc_amd.stepgraph import StepGraph
    from igmc_amd.train_eval import FlatAdam
    tr, te, cv = make_sets(flix, ntr=600)
    results = {}
    for name, env, kw in (('graph', {}, dict(group=4)), ('eager', {}, dict(use_graph=False, overlap=False, group=4)),
                          ('graph1', {'IGMC_GROUP_STEPS': '1'}, {}), ('dp_path', {'IGMC_FORCE_DP_PATH': '1'}, dict(group=4)),
                          # ... with the all-reduce of a REAL (one-rank) RCCL communicator enqueued inside the captured group
                          ('dp_comm', {'IGMC_FORCE_DP_PATH': '1', 'IGMC_DP_ALLREDUCE_ALWAYS': '1'}, dict(group=4)),
                          ('dp_flat', {'IGMC_FORCE_DP_PATH': '1', 'IGMC_DP_ALLREDUCE_ALWAYS': '1', 'IGMC_DP_FLAT': '1'},
                           dict(group=4))):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        torch.manual_seed(7)
        model = IGMC(tr, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True,
                     adj_dropout=0.2, seed=3).to('cuda')
        model.reset_parameters()
        opt = FlatAdam(model, lr=1e-3)
        sg = StepGraph(model, opt, tr, 50, 0.001, **kw)
        perm = torch.randperm(len(tr), generator=torch.Generator().manual_seed(5))
        total, n = sg.run_epoch(perm, 1)
        total2, _ = sg.run_epoch(perm, 2)
        torch.cuda.synchronize()
        results[name] = (model.flat_parameters().detach().cpu().clone(), float(total2.item()), opt.t, model._step)
        assert any(g is not None for g in sg.graphs) == (name != 'eager'), name
        assert (sg.comm is not None) == (name in ('dp_comm', 'dp_flat'))
        if sg.comm is not None:
            assert sg.comm.info() == (0, 1)
        for k in env:
            monkeypatch.delenv(k)
    assert results['graph'][2] == 24 and results['graph'][3] == 24
    for other in ('eager', 'graph1', 'dp_path', 'dp_comm', 'dp_flat'):
        assert torch.allclose(results['graph'][0], results[other][0], rtol=2e-4, atol=2e-6), other
        assert results['graph'][1] == pytest.approx(results[other][1], rel=1e-4)
    # the SAME kernels on the same inputs, only launched differently (4 steps per hipGraph launch / one per launch /
    # eagerly without overlap): no atomics on floats anywhere => the trajectories are bit-identical.  (Two training logs
    # of round 1 that diverged after a few epochs therefore came from different flags, not from the launch structure.)
    for other in ('eager', 'graph1'):
        assert torch.equal(results['graph'][0], results[other][0]), other
        assert results['graph'][1] == results[other][1], other
    # a sum over ONE rank is the identity, and the data-parallel step IS the single-GPU step plus that sum: bit-identical
    for other in ('dp_path', 'dp_comm'):
        assert torch.equal(results['graph'][0], results[other][0]), other
        assert results['graph'][1] == results[other][1], other


def test_full_size_headline_config_properties(monkeypatch):
    """BASELINE.json's headline shape (ml_1m-shaped graph: 6040 x 3706, ~900k train links, hop 1, cap 100, batch 50)
    is far beyond what the oracle finishes in seconds, so it is checked through size-independent properties:
    structural invariants of every extracted batch, reproducibility, and AGREEMENT of the two independent HIP
    implementations of the step (per-layer kernels vs. one workgroup per subgraph) on the same batches."""
    import torch
    import parity_checks as PC
    from igmc_amd import preprocessing
    from igmc_amd.models import IGMC
    from igmc_amd.stepgraph import StepGraph
    from igmc_amd.train_eval import FlatAdam
    from igmc_amd.util_functions import MyDynamicDataset
    split = preprocessing.create_trainvaltest_split('ml_1m', 1234, True, verbose=False)
    (_, _, A, tr_l, tr_u, tr_v, _, _, _, _, _, _, cv) = split
    assert A.shape == (6040, 3706)
    ds = MyDynamicDataset('data/t/full', A, (tr_u, tr_v), tr_l, 1, 1.0, 100, None, None, cv, device=0, seed=1)
    perm = torch.randperm(len(ds), generator=torch.Generator().manual_seed(3))[:50 * 12]
    runs = {}
    for name, env in (('per_layer', '0'), ('per_graph', '1'), ('per_layer_again', '0')):
        monkeypatch.setenv('IGMC_GRAPH_STEP', env)
        model = IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True,
                     adj_dropout=0.0, seed=1).to('cuda')
        torch.manual_seed(1)
        model.reset_parameters()
        opt = FlatAdam(model, lr=1e-3)
        sg = StepGraph(model, opt, ds, 50, 0.001, use_graph=False, overlap=False)
        sg.begin_epoch(perm, 1)
        losses, structs = [], []
        for k in range(12):
            sg.step()
            losses.append(float(sg.loss[0].item()))
            if name == 'per_layer' and k < 3:
                d = sg.arena.download()
                PC.check_batch_structure(d, 4)
                # hop-1 enclosing subgraphs with the cap: at most 1 + 100 nodes per side, target edge removed,
                # every kept edge has its reverse with the same relation
                assert d['B'] == 50 and d['N'] <= 50 * 202
                rev = PC.reverse_positions(d)
                assert np.array_equal(d['erel'][rev], d['erel'])
                structs.append((d['N'], d['E']))
        torch.cuda.synchronize()
        runs[name] = (losses, model.flat_parameters().detach().cpu().clone())
    # bit-reproducible
    assert runs['per_layer'][0] == runs['per_layer_again'][0]
    assert torch.equal(runs['per_layer'][1], runs['per_layer_again'][1])
    # two independent implementations walk the same trajectory (fp32 reassociation only)
    np.testing.assert_allclose(runs['per_layer'][0], runs['per_graph'][0], rtol=2e-5)
    # (Adam normalises every gradient: parameters whose gradient is ~0 may step in different directions)
    diff = (runs['per_layer'][1] - runs['per_graph'][1]).abs()
    assert float(diff.max()) < 2e-3 and float(diff.mean()) < 2e-5, (float(diff.max()), float(diff.mean()))


@pytest.mark.parametrize('batch,mnph', [(100, 63), (130, 31)], ids=['100', '130'])
def test_graph_step_other_cluster_sizes(monkeypatch, batch, mnph):
    """Batch 100 -> 2 workgroups per subgraph (slots of <= 64 nodes a side), batch 130 -> one workgroup per subgraph
    (<= 32 a side) with workgroups looping over subgraphs (accumulating partial tables): both must walk the trajectory of
    the kernels IGMC_GRAPH_STEP=0 takes instead."""
    import torch
    from igmc_amd import preprocessing
    from igmc_amd.models import IGMC
    from igmc_amd.stepgraph import StepGraph
    from igmc_amd.train_eval import FlatAdam
    from igmc_amd.util_functions import MyDynamicDataset
    split = preprocessing.create_trainvaltest_split('ml_1m', 1234, True, verbose=False)
    (_, _, A, tr_l, tr_u, tr_v, _, _, _, _, _, _, cv) = split
    ds = MyDynamicDataset('data/t/full2', A, (tr_u, tr_v), tr_l, 1, 1.0, mnph, None, None, cv, device=0, seed=1)
    perm = torch.randperm(len(ds), generator=torch.Generator().manual_seed(4))[:batch * 4]
    losses = {}
    for name, env in (('per_layer', '0'), ('per_graph', '1')):
        monkeypatch.setenv('IGMC_GRAPH_STEP', env)
        model = IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True,
                     adj_dropout=0.2, seed=1).to('cuda')
        torch.manual_seed(1)
        model.reset_parameters()
        opt = FlatAdam(model, lr=1e-3)
        sg = StepGraph(model, opt, ds, batch, 0.001, use_graph=False, overlap=False)
        sg.begin_epoch(perm, 1)
        out = []
        for _ in range(4):
            sg.step()
            out.append(float(sg.loss[0].item()))
        sg.check()
        losses[name] = out
        geo = sg.ws.step_geometry(sg._arena(0, 0), batch)
        if name == 'per_graph':
            assert geo['family'] == 'subgraph', geo
            assert geo['wg_per_graph'] == (2 if batch <= 112 else 1), geo
            if batch > 112:
                assert geo['grid'] < batch, geo          # workgroups loop over subgraphs
        else:
            assert geo['family'] != 'subgraph', geo
    np.testing.assert_allclose(losses['per_layer'], losses['per_graph'], rtol=5e-5)


def test_resume_continues_the_run_instead_of_replaying_it(flix, tmp_path):
    """``continue_from`` (reference train_eval.py:56-63): weights + Adam state AND the epoch / step counters that key the
    shuffles, the dynamic sampling and the dropout hashes are restored -- 1 epoch + resume for 1 epoch == 2 epochs."""
    import torch
    from igmc_amd.models import IGMC
    from igmc_amd.train_eval import train_multiple_epochs
    tr, te, cv = make_sets(flix, ntr=400, nte=100)

    def logger(info, m, opt):
        if m is not None:
            torch.save(m.state_dict(), str(tmp_path / ('model_checkpoint%d.pth' % info['epoch'])))
            torch.save(opt.state_dict(), str(tmp_path / ('optimizer_checkpoint%d.pth' % info['epoch'])))

    def fresh():
        torch.manual_seed(11)
        return IGMC(tr, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True,
                    adj_dropout=0.2, seed=4)
    m1 = fresh()
    r1 = train_multiple_epochs(tr, te, m1, 2, 50, 1e-3, 0.1, 50, 0, ARR=0.001, logger=logger, res_dir=str(tmp_path))
    m2 = fresh()
    r2 = train_multiple_epochs(tr, te, m2, 2, 50, 1e-3, 0.1, 50, 0, ARR=0.001, logger=None, continue_from=1,
                               res_dir=str(tmp_path))
    assert torch.allclose(m1.flat_parameters(), m2.flat_parameters(), rtol=1e-5, atol=1e-7)
    assert r1 == pytest.approx(r2, abs=1e-6)


def test_training_with_side_features(flix):
    """--use-features (reference models.py:186-188,208-209; Main.py:267-274): the fused / hipGraph-replayed training
    step gathers the target nodes' feature rows on the device; it must learn, and walk the eager loop's trajectory."""
    import torch
    from igmc_amd.models import IGMC
    from igmc_amd.train_eval import train_multiple_epochs
    from igmc_amd.util_functions import MyDataset, MyDynamicDataset
    (_, _, adj, trl, tru, trv, _, _, _, tel, teu, tev, cv) = flix
    rng = np.random.default_rng(0)
    uf = rng.standard_normal((adj.shape[0], 12)).astype(np.float32)
    vf = rng.standard_normal((adj.shape[1], 20)).astype(np.float32)
    tr = MyDynamicDataset('data/t/sf_train', adj, (tru[:400], trv[:400]), trl[:400], 1, 1.0, 10000, uf, vf, cv)
    te = MyDataset('data/t/sf_test', adj, (teu[:100], tev[:100]), tel[:100], 1, 1.0, 10000, uf, vf, cv)
    d = tr[5]
    assert d.u_feature.shape == (1, 12) and d.v_feature.shape == (1, 20)
    assert np.allclose(d.u_feature.numpy()[0], uf[tru[5]]) and np.allclose(d.v_feature.numpy()[0], vf[trv[5]])
    finals = {}
    for name, env in (('graph', {}), ('eager', {'IGMC_NO_GRAPH': '1', 'IGMC_NO_OVERLAP': '1'})):
        os.environ.update(env)
        try:
            torch.manual_seed(3)
            model = IGMC(tr, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True,
                         adj_dropout=0.0, side_features=True, n_side_features=32, seed=2)
            logs = []
            rmse = train_multiple_epochs(tr, te, model, 3, 50, 1e-3, 0.1, 50, 0, ARR=0.001,
                                         logger=lambda info, m, o: logs.append(dict(info)))
        finally:
            for k in env:
                os.environ.pop(k, None)
        assert math.isfinite(rmse) and logs[0]['train_loss'] > logs[-1]['train_loss']
        assert tuple(model.lin1.weight.shape) == (128, 256 + 32)
        finals[name] = (model.flat_parameters().detach().cpu().clone(), rmse)
    assert torch.allclose(finals['graph'][0], finals['eager'][0], rtol=2e-4, atol=2e-6)
    assert finals['graph'][1] == pytest.approx(finals['eager'][1], rel=1e-4)


@pytest.mark.parametrize('data_name,multiply_by', [('flixster', 1), ('douban', 1), ('yahoo_music', 20)])
def test_transfer_eval_end_to_end(tmp_path, monkeypatch, data_name, multiply_by):
    """BASELINE.json configs[4] / reference run_transfer_exps.sh + Main.py:442-470: a 5-relation checkpoint set (as an
    ml_100k run leaves it: model_checkpoint{10,20,30,40}.pth) evaluated on another dataset through ``--transfer``: the
    target's ratings are regrouped into 5 relations (post_rating_map, Main.py:162-177), predictions are multiplied
    (--multiply-by, models.py:215) and the four checkpoints ensembled.  The RMSE ``Main.main`` reports must equal the
    oracle's (same checkpoints, same subgraphs, mean of predictions) within 1e-4."""
    import importlib
    import torch
    from helpers import ROOT
    from igmc_amd import preprocessing
    from igmc_amd.models import IGMC
    from igmc_amd.train_eval import DataLoader
    from igmc_amd.util_functions import MyDataset
    from oracle import pyg_ref
    monkeypatch.chdir(tmp_path)
    src = tmp_path / 'ml_100k_ckpt'
    src.mkdir()

    class _DS(object):
        num_features = 4
    paths = []
    for i, ep in enumerate((10, 20, 30, 40)):
        torch.manual_seed(100 + i)
        m = IGMC(_DS(), latent_dim=[32, 32, 32, 32], num_relations=5, num_bases=4, regression=True)
        m.reset_parameters()
        p = str(src / ('model_checkpoint%d.pth' % ep))
        torch.save(m.state_dict(), p)
        paths.append(p)
    sys_path_main = importlib.import_module('Main') if ROOT in __import__('sys').path else None
    assert sys_path_main is not None
    argv = ['--data-name', data_name, '--epochs', '40', '--testing', '--no-train', '--ensemble', '--transfer', str(src),
            '--num-relations', '5', '--multiply-by', str(multiply_by), '--max-test-num', '200']
    rmse = sys_path_main.main(argv)
    log = (tmp_path / 'results' / ('%s_testmode' % data_name) / 'log.txt').read_text()
    assert 'transfer' in log and 'ensemble' in log
    # ---- oracle on the identical inputs
    class _A(object):
        pass
    a = _A()
    a.standard_rating, a.transfer, a.data_name, a.num_relations = False, str(src), data_name, 5
    rating_map, post_rating_map = sys_path_main.rating_maps(a)
    split = preprocessing.load_data_monti(data_name, True, rating_map, post_rating_map)
    (_, _, adj, _, _, _, _, _, _, tel, teu, tev, cv) = split
    assert int(adj.data.max()) <= 5                                   # relations regrouped onto the source model's 5
    te = MyDataset('data/x/test', adj, (teu, tev), tel, 1, 1.0, 10000, None, None, cv, max_num=200, seed=1)
    batches = []
    for data in DataLoader(te, 50, shuffle=False):
        raw = data._materialise()['raw']
        batches.append(batch_to_pyg(raw, 4))
    ys = torch.cat([b.y for b in batches])
    preds = []
    for p in paths:
        ref = pyg_ref.IGMCRef(4, (32, 32, 32, 32), 5, 4, adj_dropout=0.2, multiply_by=multiply_by, fast=True)
        ref.load_state_dict({k: v.cpu() for k, v in torch.load(p).items()})
        preds.append(torch.cat([pyg_ref.eval_sse(ref, b)[1] for b in batches]))
    ref_rmse = math.sqrt(float(((torch.stack(preds, 1).mean(1) - ys) ** 2).mean()))
    assert len(ys) == 200
    assert rmse == pytest.approx(ref_rmse, abs=1e-4 * max(1.0, multiply_by))


def test_static_dataset_cache(flix, tmp_path):
    """reference MyDataset (util_functions.py:69-110): subgraphs extracted once, cached under <root>/processed/, reused by
    later constructions; batches rebuilt from the cache equal the re-derived ones; a static dataset trains through the
    fused step (node sets served from HBM), with the trajectory of the re-deriving dataset."""
    import torch
    from igmc_amd.models import IGMC
    from igmc_amd.train_eval import DataLoader, train_multiple_epochs
    from igmc_amd.util_functions import MyDataset
    (_, _, adj, trl, tru, trv, _, _, _, tel, teu, tev, cv) = flix
    root = str(tmp_path / 'static_train')
    mk = lambda **kw: MyDataset(root, adj, (tru[:300], trv[:300]), trl[:300], 1, 1.0, 12, None, None, cv, seed=3, **kw)
    ds = mk()
    path = ds.processed_paths[0]
    assert os.path.exists(path) and path.endswith(os.path.join('processed', 'data.igmc.npz')) and ds._cache is not None
    z = np.load(path)
    assert len(z['uoff']) == 301 and z['unodes'].dtype == np.int32 and z['udist'].dtype == np.uint8
    mtime = os.path.getmtime(path)
    ds2 = mk()                                         # second construction: loaded, not rebuilt
    assert os.path.getmtime(path) == mtime and ds2._cache is not None
    ds3 = mk(cache=False)                              # re-deriving variant
    assert ds3._cache is None
    for a, b in zip(DataLoader(ds2, 50, shuffle=False), DataLoader(ds3, 50, shuffle=False)):
        ra, rb = a._materialise()['raw'], b._materialise()['raw']
        for key in ('node_off', 'node_gid', 'node_label', 'row_ptr', 'col', 'erel', 'y'):
            assert np.array_equal(ra[key], rb[key]), key
    # a different geometry invalidates the cache (fingerprint), it is rebuilt instead of being misused
    ds4 = MyDataset(root, adj, (tru[:300], trv[:300]), trl[:300], 1, 1.0, 20, None, None, cv, seed=3)
    assert os.path.getmtime(path) >= mtime and ds4._cache is not None and len(ds4) == 300
    # training on the static dataset == training on the re-deriving one
    te = MyDataset(str(tmp_path / 'static_test'), adj, (teu[:100], tev[:100]), tel[:100], 1, 1.0, 12, None, None, cv, seed=3)
    finals = []
    for d in (mk(), mk(cache=False)):
        torch.manual_seed(5)
        model = IGMC(d, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True, adj_dropout=0.0, seed=2)
        r = train_multiple_epochs(d, te, model, 2, 50, 1e-3, 0.1, 50, 0, ARR=0.001)
        finals.append((model.flat_parameters().detach().cpu().clone(), r))
    assert torch.equal(finals[0][0], finals[1][0]) and finals[0][1] == finals[1][1]


_DP2_SCRIPT = r'''
import os, sys
sys.path.insert(0, %r)
import numpy as np, torch, torch.distributed as dist
from igmc_amd import parallel, preprocessing
from igmc_amd.models import IGMC
from igmc_amd.stepgraph import StepGraph
from igmc_amd.train_eval import FlatAdam
from igmc_amd.util_functions import MyDynamicDataset
rank, world = int(os.environ['RANK']), 2
torch.cuda.set_device(int(os.environ.get('DP2_DEVICE', '0')))
dist.init_process_group(backend=os.environ.get('DP2_BACKEND', 'gloo'), init_method='tcp://127.0.0.1:%%s' %% os.environ.get('DP2_PORT', '29643'), rank=rank, world_size=world)
(_, _, adj, trl, tru, trv, _, _, _, _, _, _, cv) = preprocessing.load_data_monti('douban', testing=True)
n = 2 * (50 * 3 + 7)
tr = MyDynamicDataset('data/t/dp2_%%d' %% rank, adj, (tru[:n], trv[:n]), trl[:n], 1, 1.0, 10000, None, None, cv)
def fresh():
    torch.manual_seed(7)
    model = IGMC(tr, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True, adj_dropout=0.2,
                 seed=3).to('cuda')
    model.reset_parameters()
    return model, FlatAdam(model, lr=1e-3)
def state(model, opt):
    torch.cuda.synchronize()
    return [t.detach().cpu().clone() for t in (model.flat_parameters(), opt.exp_avg, opt.exp_avg_sq)]
perm = torch.randperm(n, generator=torch.Generator().manual_seed(5))
half = perm[:150]                    # three full batches (the ragged batch of a single-GPU epoch runs other kernels: _model / _finish)
# ---- (a) the same links on both ranks == the single-GPU step
model, opt = fresh()
sg = StepGraph(model, opt, tr, 50, 0.001, use_graph=False, overlap=False, group=2)
assert sg.dp_path and sg.world == 2 and sg.comm is not None and sg.comm.info() == (rank, 2)
assert sg.comm.transport.startswith(os.environ['DP2_EXPECT']), sg.comm.transport
tot_dp, _ = sg.run_epoch(half, 1)
dp = state(model, opt) + [float(tot_dp.item())]
model1, opt1 = fresh()
sg1 = StepGraph(model1, opt1, tr, 50, 0.001, use_graph=False, overlap=False, group=2)
sg1.dp_path, sg1.comm, sg1.world = False, None, 1          # the single-GPU step in this very process
tot_1, _ = sg1.run_epoch(half, 1)
one = state(model1, opt1) + [float(tot_1.item())]
for i, (x, y) in enumerate(zip(dp, one)):
    same = torch.equal(x, y) if torch.is_tensor(x) else x == y
    assert same, ('two identical half-batches vs the single-GPU step', i,
                  float((x - y).abs().max()) if torch.is_tensor(x) else (x, y))
# ---- (b) sharded links, ragged last batch
model, opt = fresh()
sg = StepGraph(model, opt, tr, 50, 0.001, use_graph=False, overlap=False, group=2)
mine = parallel.shard_positions(perm, rank, world, pad=True)
assert len(mine) == 157
total, cnt = sg.run_epoch(mine, 1)
P = state(model, opt)[0]
both = [torch.zeros_like(P) for _ in range(world)]
if dist.get_backend() == 'nccl':
    both = [b.cuda() for b in both]
    dist.all_gather(both, P.cuda())
    both = [b.cpu() for b in both]
else:
    dist.all_gather(both, P)
assert torch.equal(both[0], both[1]), 'replicas differ'
assert np.isfinite(float(total.item())) and float(total.item()) > 0 and opt.t == 4
assert not torch.equal(P, dp[0])
if sg.comm.transport in ('p2p', 'rccl'):
    # ---- (c) the same sharded epoch with the steps CAPTURED (pairs of one-step groups replayed from the hipGraph, the peer
    #      exchange inside them: its launch sequence number lives on the device) == the eager launches, bit for bit
    model, opt = fresh()
    sgc = StepGraph(model, opt, tr, 50, 0.001, group=1)
    assert sgc.use_graph and sgc.comm is sg.comm
    sgc.run_epoch(mine, 1)
    assert sgc.graph is not None, 'the steps were not captured'
    Pc = state(model, opt)[0]
    assert torch.equal(Pc, P), ('captured vs eager', float((Pc - P).abs().max()))
    # ... and the exchange alone, timed on the step's stream (two ranks on one device: an upper bound)
    t = torch.zeros(61000, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(5):
        sg.comm.all_reduce_(t, st)
    torch.cuda.synchronize()
    dist.barrier()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        sg.comm.all_reduce_(t, st)
    e1.record()
    if hasattr(sg.comm, 'check'):
        sg.comm.check(st)
    print('rank', rank, sg.comm.transport, 'all-reduce of 61000 floats: %%.1f us' %% (e0.elapsed_time(e1) / 50 * 1e3), 'fine-grained buffers:', getattr(sg.comm, 'fine_grained', None),
          'device', torch.cuda.current_device())
print('rank', rank, 'dp2 ok')
dist.destroy_process_group()
'''


@pytest.mark.parametrize('transport', ['p2p', 'host_comm', 'fallback'])
def test_two_ranks_on_one_gpu(tmp_path, transport):
    """The data-parallel step (igmc_train_step_dp: the subgraph kernel's tables + lin gradients summed over the ranks between
    k_tail_ts and k_finalize_ts) with TWO ranks on real kernels.  RCCL refuses two ranks on one device, so the exchange
    goes through torch.distributed's gloo group (IGMC_DP_HOST_COMM=1: a host-callback communicator staged through the
    host, steps launched eagerly) -- everything else is the product path (StepGraph's group pipeline, the ragged last
    batch).
    (a) Both ranks walk the SAME links: the mean over two identical half-batches is the single-GPU gradient, and because
        1 / (2 B) is exactly half of 1 / B every intermediate is an exact half -- the trajectory must equal the single-GPU
        step's bit for bit.
    (b) Links sharded perm[k::2] (three full batches and a ragged one per rank): replicas bit-identical, losses finite,
        two spans exchanged per step.
    `p2p`: the exchange is the library's one-shot all-reduce over peer-mapped buffers (igmc_comm_peer_*: HIP IPC handles work
    between two processes on ONE device), steps captured into the group graphs -- the product's multi-GPU transport on real
    kernels; the same two checks, plus the transport's name.
    `fallback`: p2p ruled out, the library tries its own RCCL communicator, RCCL refuses ("Duplicate GPU"), the ranks agree
    on that over the process group and all of them fall back to it (parallel.grad_comm)."""
    import os
    import subprocess
    import sys
    script = tmp_path / 'dp2.py'
    script.write_text(_DP2_SCRIPT % ROOT)
    _run_dp2(script, transport, two_devices=False)


def _run_dp2(script, transport, two_devices):
    import os
    import subprocess
    import sys
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', HSA_ENABLE_IPC_MODE_LEGACY='0',
                   DP2_PORT={'host_comm': '29643', 'fallback': '29644', 'p2p': '29645', 'rccl': '29646'}[transport],
                   DP2_EXPECT={'host_comm': 'host-callback:gloo', 'fallback': 'host-callback:gloo', 'p2p': 'p2p', 'rccl': 'rccl'}[transport])
        env.pop('IGMC_DP_HOST_COMM', None)
        env['IGMC_DP_TRANSPORT'] = {'host_comm': 'host', 'p2p': 'p2p', 'rccl': 'rccl'}.get(transport, 'auto')
        if transport == 'fallback':
            env['IGMC_DP_NO_P2P'] = '1'          # (auto would take p2p: rule it out to walk rccl -> host)
        if two_devices:
            env.update(DP2_DEVICE=str(r), DP2_BACKEND='nccl', DP2_PORT=str(int(env['DP2_PORT']) + 10))
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=600)[0].decode() for p in procs]
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o[-3000:]
        assert 'rank %d dp2 ok' % r in o
        print(o[-300:])
        assert ('rccl could not be set up on every rank' in o) == (transport == 'fallback'), o[-2000:]


@pytest.mark.parametrize('transport', ['p2p', 'rccl'])
def test_two_ranks_on_two_gpus(tmp_path, transport):
    """``test_two_ranks_on_one_gpu``'s checks with the two ranks on two DIFFERENT devices (skipped on a one-GPU box), over the
    peer-mapped exchange AND over the library's RCCL communicator, rendezvous over torch.distributed's ``nccl`` backend --
    the product's multi-GPU configuration: (a) two identical half-batches == the single-GPU step bit for bit, (b) sharded
    links with a ragged last batch: replicas bit-identical, (c) the steps captured into the group graphs (the exchange
    inside them) == the eager launches.  The steps run the subgraph kernel (uncapped douban).  This is where the exchange
    words cross xGMI: fine-grained IPC memory of another device, no shared L2 -- what one device cannot show."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs')
    script = tmp_path / 'dp2.py'
    script.write_text(_DP2_SCRIPT % ROOT)
    _run_dp2(script, transport, two_devices=True)


def test_captured_all_reduce_next_to_a_torch_distributed_process_group(tmp_path):
    """The multi-GPU configuration of bench.py / Main.py on one GPU: a REAL torch.distributed 'nccl' (= RCCL) process
    group of one rank is up (its watchdog thread polls events while the step graph is captured: thread-local capture
    mode), the library's own communicator is created from an id that travels over it, igmc_allreduce_grads is enqueued
    inside the captured groups, and the trajectory equals the eagerly launched one.  (A one-GPU box cannot say anything
    about more ranks; this pins the capture / replay mechanics the multi-GPU run relies on.)"""
    import os
    import subprocess
    import sys
    script = tmp_path / 'dp1.py'
    script.write_text(r'''
import os, sys
sys.path.insert(0, %r)
import torch, torch.distributed as dist
from igmc_amd import preprocessing
from igmc_amd.models import IGMC
from igmc_amd.stepgraph import StepGraph
from igmc_amd.train_eval import FlatAdam
from igmc_amd.util_functions import MyDynamicDataset
torch.cuda.set_device(0)
dist.init_process_group(backend='nccl', init_method='tcp://127.0.0.1:29641', rank=0, world_size=1)
(_, _, adj, trl, tru, trv, _, _, _, _, _, _, cv) = preprocessing.load_data_monti('douban', testing=True)
tr = MyDynamicDataset('data/t/dp1', adj, (tru[:1200], trv[:1200]), trl[:1200], 1, 1.0, 10000, None, None, cv)
res = {}
for name, kw in (('eager', dict(use_graph=False, overlap=False)), ('captured', {})):
    torch.manual_seed(7)
    model = IGMC(tr, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True,
                 adj_dropout=0.2, seed=3).to('cuda')
    model.reset_parameters()
    opt = FlatAdam(model, lr=1e-3)
    sg = StepGraph(model, opt, tr, 50, 0.001, group=8, **kw)
    assert sg.dp_path and sg.comm is not None and sg.comm.info() == (0, 1)
    perm = torch.randperm(len(tr), generator=torch.Generator().manual_seed(5))
    sg.run_epoch(perm, 1)
    total, n = sg.run_epoch(perm, 2)
    torch.cuda.synchronize()
    res[name] = (model.flat_parameters().detach().cpu().clone(), float(total.item()), any(g is not None for g in sg.graphs))
assert res['captured'][2], 'the groups (with the all-reduce inside) were not captured'
assert not res['eager'][2]
assert torch.equal(res['eager'][0], res['captured'][0]) and res['eager'][1] == res['captured'][1]
dist.destroy_process_group()
print('captured all-reduce ok')
''' % ROOT)
    env = dict(os.environ, IGMC_FORCE_DP_PATH='1', IGMC_DP_ALLREDUCE_ALWAYS='1', HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = subprocess.run([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode()
    assert r.returncode == 0 and 'captured all-reduce ok' in out, out[-3000:]


def test_eval_through_the_grouped_pipeline_equals_the_eager_loop(flix, monkeypatch):
    """eval_loss (reference train_eval.py:182-199) through EvalGraph -- forward + squared-error accumulation per step, the
    next group's batches extracted beside it, pairs of groups replayed from a hipGraph -- gives the same sum as the eager
    batch-by-batch loop, bit for bit; twice in a row (second call replays the captured graph from its first step), on a
    static (cached) test set and on a dynamic one, with a ragged last batch."""
    import torch
    from igmc_amd.models import IGMC
    from igmc_amd.train_eval import DataLoader, eval_loss
    from igmc_amd import preprocessing
    from igmc_amd.util_functions import MyDataset, MyDynamicDataset
    (_, _, adj, trl, tru, trv, _, _, _, tel, teu, tev, cv) = preprocessing.load_data_monti('douban', testing=True)
    sets = [MyDataset(None, adj, (teu[:1230], tev[:1230]), tel[:1230], 1, 1.0, 10000, None, None, cv, seed=2),
            MyDynamicDataset('data/t/evg', adj, (teu[:1230], tev[:1230]), tel[:1230], 1, 1.0, 40, None, None, cv, seed=2)]
    torch.manual_seed(4)
    model = IGMC(sets[0], latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True,
                 adj_dropout=0.2, seed=3).to('cuda')
    model.reset_parameters()
    for ds in sets:
        vals = {}
        for mode in ('graph', 'eager'):
            if mode == 'eager':
                monkeypatch.setenv('IGMC_NO_EVAL_GRAPH', '1')
            loader = DataLoader(ds, 50, shuffle=False)
            vals[mode] = [eval_loss(model, loader, 'cuda', regression=True) for _ in range(2)]
            if mode == 'graph':
                eg = loader._evalgraph
                assert eg.graph is not None and eg.M == 12 and eg.steps_done == 2 * 25
            monkeypatch.delenv('IGMC_NO_EVAL_GRAPH', raising=False)
        assert vals['graph'][0] == vals['eager'][0], (vals, type(ds).__name__)
        if not ds.dynamic:            # (a dynamic test set is re-sampled per evaluation: the loader's epoch counter keys it)
            assert vals['graph'][0] == vals['graph'][1]
        assert vals['graph'][1] == vals['eager'][1]

"""What ``--visualize`` costs on the GPU, at the shape ``tools/eval_bench.py`` uses (ml_1m-shaped, cap 100, batch 50):

    python tools/visualize_bench.py score  [--links 20000] [--reps 5]     score_links (the scoring pass that keeps the per-link
                                                                          predictions on the device), warm, one line per timed pass
    python tools/visualize_bench.py eval   [--links 20000] [--reps 5]     eval_loss through EvalGraph, the same way (the yardstick; to
                                                                          time another build of the project run ITS tools/eval_bench.py)
    python tools/visualize_bench.py select [--reps 20]                    igmc_select_extremes at n = 20 k and 1 M, num = 5 and 64, HIP
                                                                          events, torch.sort on the same tensor beside it

Every timed window ends in a device synchronise.  Output: one JSON line per measurement.
"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from igmc_amd.hostcpu import limit_host_threads  # noqa: E402
limit_host_threads()
import torch  # noqa: E402
from igmc_amd import _lib, engine, preprocessing  # noqa: E402
from igmc_amd.models import IGMC  # noqa: E402
from igmc_amd.train_eval import DataLoader, eval_loss, score_links  # noqa: E402
from igmc_amd.util_functions import MyDataset  # noqa: E402


def pass_bench(a):
    with contextlib.redirect_stdout(sys.stderr):
        split = preprocessing.create_trainvaltest_split('ml_1m', 1234, True, verbose=False)
    (_, _, A, _, _, _, _, _, _, te_l, te_u, te_v, cv) = split
    m = min(a.links, len(te_u))
    te = MyDataset('data/evalbench', A, (te_u[:m], te_v[:m]), te_l[:m], 1, 1.0, a.mnph, None, None, cv, seed=1)
    torch.manual_seed(1)
    model = IGMC(te, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True, adj_dropout=0.0,
                 seed=1).to('cuda')
    model.reset_parameters()
    model.eval()
    loader = DataLoader(te, 50, shuffle=False)
    run = (lambda: score_links(model, te, 50)) if a.what == 'score' else (lambda: eval_loss(model, loader, 'cuda', regression=True))
    for _ in range(a.warmup):          # the first pass starts eagerly and captures the graph
        run()
    ms = []
    for r in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({'what': a.what, 'links': m, 'rep': r, 'ms': round(ms[-1], 4), 'subgraphs_per_s': round(m / ms[-1] * 1e3)}),
              flush=True)
    print(json.dumps({'what': a.what, 'links': m, 'median_ms': round(statistics.median(ms), 4), 'min_ms': round(min(ms), 4),
                      'max_ms': round(max(ms), 4)}), flush=True)


def select_bench(a):
    lib = _lib.load()
    P = engine._p
    gen = torch.Generator(device='cuda').manual_seed(1)
    for n in (20000, 1000000):
        keys = torch.randn(n, device='cuda', generator=gen)
        for num in (5, 64):
            nbytes = lib.igmc_select_scratch_bytes(n, num, 0)
            scratch = torch.empty(nbytes // 8, dtype=torch.int64, device='cuda')
            idx = torch.empty(2, num, dtype=torch.int32, device='cuda')
            key = torch.empty(2, num, dtype=torch.float32, device='cuda')
            cnt = torch.zeros(1, dtype=torch.int32, device='cuda')
            st = torch.cuda.current_stream().cuda_stream

            def sel():
                lib.call('igmc_select_extremes', P(keys.data_ptr()), n, num, P(idx[0].data_ptr()), P(idx[1].data_ptr()),
                         P(key[0].data_ptr()), P(key[1].data_ptr()), P(cnt.data_ptr()), P(scratch.data_ptr()), nbytes, 0, P(st))

            for name, fn in (('igmc_select_extremes', sel), ('torch.sort', lambda: torch.sort(keys, stable=True))):
                for _ in range(3):
                    fn()
                us = []
                for _ in range(a.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    us.append(e0.elapsed_time(e1) * 1e3)
                print(json.dumps({'what': name, 'n': n, 'num': num, 'median_us': round(statistics.median(us), 2),
                                  'min_us': round(min(us), 2), 'max_us': round(max(us), 2)}), flush=True)
            order = torch.sort(keys, stable=True)[1]
            assert idx[0].tolist() == order[:num].tolist() and idx[1].tolist() == order[-num:].flip(0).tolist()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['score', 'eval', 'select'])
    ap.add_argument('--links', type=int, default=20000)
    ap.add_argument('--mnph', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    a = ap.parse_args()
    select_bench(a) if a.what == 'select' else pass_bench(a)

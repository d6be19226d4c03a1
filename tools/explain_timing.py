"""What explaining predictions costs beside a scoring pass of the same size (writes ``profiles/explain_timing.txt``):

    python tools/explain_timing.py [--pairs 100] [--m 5] [--reps 5] [--warmup 2] [--out profiles/explain_timing.txt]

douban, hop 1, cap 100, batch 50, ``--pairs`` test links.  Every window is warm and ends in a device synchronise; the two
ALTERNATE in one process:

* ``score_candidates`` over a ``CandidateLinks`` of as many arbitrary links as the pairs have leave-one-out variants
  (dynamic extraction: every link is sampled and extracted);
* ``explain`` end to end: extraction of the pairs, ``igmc_loo_count``, the prefix sums and their one host read,
  ``igmc_loo_fill``, the scoring pass over the variants (cached extraction), ``igmc_loo_deltas``, ``igmc_select_segments``, the
  gathers;
* the three new launches by themselves, HIP events around each kernel (``igmc_profile_fetch``).

The expectation it confirms or refutes: the variant pass runs near the evaluation rate, and the three new launches are small
beside it.
"""
import argparse
import contextlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from igmc_amd.hostcpu import limit_host_threads  # noqa: E402
limit_host_threads()
import numpy as np  # noqa: E402
import torch  # noqa: E402
from igmc_amd import _lib, engine, preprocessing  # noqa: E402
from igmc_amd.explain import explain  # noqa: E402
from igmc_amd.models import IGMC  # noqa: E402
from igmc_amd.recommend import CandidateLinks, score_candidates  # noqa: E402
from igmc_amd.util_functions import MyDynamicDataset  # noqa: E402

NEW = ('k_loo_count', 'k_loo_fill', 'k_loo_deltas')


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(ms):
    return ', '.join('%.3f' % x for x in ms)


def kernel_times(lib, fn, reps):
    """us per call of ``fn`` spent in each new kernel (all its launches), HIP events around each: {name: [one per repeat]}."""
    fn()
    torch.cuda.synchronize()
    lib.igmc_profile_enable(1)
    prof, calls_of = {}, {}
    for _ in range(reps):
        fn()
        torch.cuda.synchronize()
        for name, ms, calls in engine.profile_fetch(lib, 128):          # (the fetch empties the record: one entry per repeat)
            prof.setdefault(name, []).append(ms * 1e3)
            calls_of[name] = calls
    lib.igmc_profile_enable(0)
    return {k: v for k, v in prof.items() if k in NEW}, calls_of


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=100)
    ap.add_argument('--m', type=int, default=5)
    ap.add_argument('--mnph', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'explain_timing.txt'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('explain_timing.py measures on the GPU: no device found')
    with contextlib.redirect_stdout(sys.stderr):
        split = preprocessing.load_data_monti('douban', testing=True)
    (_, _, adj, trl, tru, trv, _, _, _, _, teu, tev, cv) = split
    train = MyDynamicDataset('data/explaintiming/train', adj, (tru, trv), trl, 1, 1.0, a.mnph, None, None, cv, seed=1)
    u, v = np.asarray(teu[:a.pairs], np.int32), np.asarray(tev[:a.pairs], np.int32)
    torch.manual_seed(1)
    model = IGMC(train, latent_dim=[32, 32, 32, 32], num_relations=len(cv), num_bases=4, regression=True, adj_dropout=0.0,
                 seed=1).to('cuda')
    model.reset_parameters()
    model.eval()
    stats = {}
    run_b = lambda: explain(model, train, u, v, m=a.m, stats=stats)
    run_b()
    nvar = stats['variants']
    rng = np.random.default_rng(1)
    cands = CandidateLinks.from_pairs(train, rng.integers(0, adj.shape[0], nvar).astype(np.int32),
                                      rng.integers(0, adj.shape[1], nvar).astype(np.int32))
    run_a = lambda: score_candidates(model, cands, 50)
    for _ in range(a.warmup):
        run_a()
        run_b()
    ms_a, ms_b = [], []
    for _ in range(a.reps):            # alternating: whatever else the host does hits both
        ms_a.append(timed(run_a)[0])
        ms_b.append(timed(run_b)[0])
    loo = train._explain_links
    run_c = lambda: score_candidates(model, loo, 50)          # the variant pass alone: the cache the last explain() left
    ms_c = [timed(run_c)[0] for _ in range(a.reps)]
    prof, calls = kernel_times(_lib.load(), run_b, a.reps)
    med_a, med_b, med_c = statistics.median(ms_a), statistics.median(ms_b), statistics.median(ms_c)
    new_ms = sum(statistics.median(x) for x in prof.values()) / 1e3
    L = []
    L.append('Cost of explaining predictions beside a scoring pass of the same size: one MI355X, one process, tools/explain_timing.py.')
    L.append('Shape: douban (3000 x 3000), hop 1, cap %d, batch 50, the first %d test links, m = %d: %d leave-one-out variants '
             '(%d batches), %d attributions, %d pass(es).' % (a.mnph, a.pairs, a.m, nvar, (nvar + 49) // 50, stats['attributions'],
                                                               stats['passes']))
    L.append('Every timed window is warm (%d runs of each before it), ends in a device synchronise inside the clock, and a / b '
             'alternate (a, b, a, b, ...).' % (a.warmup + 1))
    L.append('')
    L.append('a  score_candidates over %d arbitrary links (dynamic extraction), ms per pass:     %s' % (nvar, fmt(ms_a)))
    L.append('b  explain() end to end, ms per call:                                                %s' % fmt(ms_b))
    L.append('c  score_candidates over the %d variants alone (cached extraction), ms per pass:   %s' % (nvar, fmt(ms_c)))
    L.append('')
    L.append('median a  %.3f ms  (%.3f M links/s)      spread max - min %.3f ms' % (med_a, nvar / med_a / 1e3, max(ms_a) - min(ms_a)))
    L.append('median b  %.3f ms  (%.3f M variants/s)   spread max - min %.3f ms' % (med_b, nvar / med_b / 1e3, max(ms_b) - min(ms_b)))
    L.append('median c  %.3f ms  (%.3f M variants/s)   spread max - min %.3f ms' % (med_c, nvar / med_c / 1e3, max(ms_c) - min(ms_c)))
    L.append('b against a: %+.3f ms = %+.2f %%;  c against a: %+.2f %%' % (med_b - med_a, (med_b / med_a - 1) * 100,
                                                                        (med_c / med_a - 1) * 100))
    L.append('')
    L.append('the new kernels by themselves (HIP events around each launch, igmc_profile_fetch), us per explain() call, median of '
             '%d (min .. max), launches per call:' % a.reps)
    for name in NEW:
        if name in prof:
            us = prof[name]
            L.append('  %-14s %9.2f   (%.2f .. %.2f)   %d launch(es)' % (name, statistics.median(us), min(us), max(us), calls.get(name, 0)))
    L.append('the three together: %.3f ms = %.2f %% of explain() end to end, %.2f %% of the variant pass alone'
             % (new_ms, new_ms / med_b * 100, new_ms / med_c * 100))
    text = '\n'.join(L) + '\n'
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)
    print(text)


if __name__ == '__main__':
    main()

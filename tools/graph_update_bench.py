"""Times the two routes from "new ratings arrive" to "a resident rating graph that holds them" on the ml_1m-shaped synthetic
graph (``preprocessing.synth_ml`` at the headline's sizes), in one process, alternating:

  (a) ``engine.Graph(A')`` from a host CSR that ALREADY holds the changes -- the only route before ``igmc_graph_apply``, and
      generous to it: applying the changes to the host matrix is not timed;
  (b) ``Graph.updated`` from device arrays (``igmc_graph_apply``: graph_update.hip).

Change lists of n = 1, 1 000 and 100 000 (a third hit existing entries, a tenth repeat an earlier pair, a quarter remove).  Both
calls end synchronised, so the host clock around them is the measurement; warmed up, ``--reps`` repetitions each, median and
spread (min, max).  ``copy_floor_ms`` is a plain device copy of the six arrays of the graph -- an update must write every byte of
the new graph once -- and ``b_over_copy`` is (b)'s median as a multiple of it.  Prints one JSON line; ``--out`` also writes it."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import scipy.sparse as ssp  # noqa: E402


def spread(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median_ms=round(float(np.median(ts)), 4), min_ms=round(float(ts.min()), 4), max_ms=round(float(ts.max()), 4))


def change_list(M, n, rng):
    nu, ni = M.shape
    ex = np.argwhere(M != 0)
    u, i = rng.integers(0, nu, n), rng.integers(0, ni, n)
    hit = rng.random(n) < 1.0 / 3
    pick = ex[rng.integers(0, len(ex), n)]
    u, i = np.where(hit, pick[:, 0], u), np.where(hit, pick[:, 1], i)
    rep = np.nonzero(rng.random(n) < 0.1)[0]
    rep = rep[rep > 0]
    src = (rng.random(len(rep)) * rep).astype(np.int64)
    u[rep], i[rep] = u[src], i[src]
    r = np.where(rng.random(n) < 0.25, 0, rng.integers(1, 6, n))
    return u.astype(np.int32), i.astype(np.int32), r.astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--sizes', default='1,1000,100000')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from igmc_amd import engine, preprocessing
    nu, ni, nnz, hist = preprocessing.ML_HIST['ml_1m']
    u, v, r = preprocessing.synth_ml(nu, ni, nnz, hist, seed=0)
    levels = np.sort(np.unique(r))
    M = np.zeros((nu, ni), np.uint8)
    M[u, v] = np.searchsorted(levels, r) + 1
    g = engine.Graph(ssp.csr_matrix(M.astype(np.float32)))
    info = g.info()
    rng = np.random.default_rng(1)
    out = dict(tool='graph_update_bench', graph=info, reps=args.reps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
               lists={})
    # the floor: one device copy of the six arrays
    src = [torch.zeros(k, dtype=d, device='cuda') for k, d in ((nu + 1, torch.int32), (info['nnz'], torch.int32), (info['nnz'], torch.uint8),
                                                                (ni + 1, torch.int32), (info['nnz'], torch.int32), (info['nnz'], torch.uint8))]
    dst = [torch.empty_like(t) for t in src]
    floor = []
    for k in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for a, b in zip(dst, src):
            a.copy_(b)
        torch.cuda.synchronize()
        if k >= args.warmup:
            floor.append(time.perf_counter() - t0)
    out['copy_floor'] = spread(floor)
    out['copy_floor']['bytes'] = int(sum(t.numel() * t.element_size() for t in src))
    for n in [int(x) for x in args.sizes.split(',')]:
        cu, ci, cr = change_list(M, n, rng)
        M2 = M.copy()
        for a, b, c in zip(cu.tolist(), ci.tolist(), cr.tolist()):
            M2[a, b] = c
        A2 = ssp.csr_matrix(M2.astype(np.float32))
        du, di, dr = torch.from_numpy(cu).cuda(), torch.from_numpy(ci).cuda(), torch.from_numpy(cr).cuda()
        ta, tb = [], []
        for k in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ga = engine.Graph(A2)                       # (six synchronous uploads: ends synchronised)
            t1 = time.perf_counter()
            gb = g.updated(du, di, dr)                  # (synchronous)
            t2 = time.perf_counter()
            if k == 0:
                da, db = ga.download(), gb.download()
                assert ga.info() == gb.info() and all(da[x].tobytes() == db[x].tobytes() for x in da), 'the two routes disagree'
            ga.close()
            gb.close()
            if k >= args.warmup:
                ta.append(t1 - t0)
                tb.append(t2 - t1)
        a, b = spread(ta), spread(tb)
        out['lists'][str(n)] = dict(a_rebuild_through_host=a, b_update_on_device=b, nnz_after=int((M2 != 0).sum()),
                                    a_over_b=round(a['median_ms'] / b['median_ms'], 2),
                                    b_over_copy=round(b['median_ms'] / out['copy_floor']['median_ms'], 2))
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()

"""Experiment (GPU, variant library with phase stamps in the one-launch tail k_tail_fin): shader-clock cycles between the stamps
of the first main workgroup (layer 1, input row 0), the first lin workgroup, the loss / tick workgroup, the first row producer
(layer 1, input row 0, set 1) and layer 1's bias producer of the LAST k_tail_fin launch of a short replayed run.

    python tools/exp_fin_clocks.py [LIBRARY]      (default: igmc_amd/lib/libigmc_hip_finclk.so; e.g. a variant of another commit,
                                                   whose main workgroup summed every set itself and has no producers)

The variant is the product's sources compiled with -DIGMC_FIN_CLOCKS into a library of its own:
    HIPCC_COMPILE_FLAGS_APPEND=-DIGMC_FIN_CLOCKS IGMC_HIP_LIB_OUT=$PWD/igmc_amd/lib/libigmc_hip_finclk.so \\
        python -m igmc_amd.build --force
(The stamps of k_finalize_ts that this tool read in round 6 lived in a patch: profiles/r06_experiments.)"""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from igmc_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, 'igmc_amd', 'lib', 'libigmc_hip_finclk.so')
import torch
from igmc_amd import preprocessing
from igmc_amd.models import IGMC
from igmc_amd.stepgraph import StepGraph
from igmc_amd.train_eval import FlatAdam
from igmc_amd.util_functions import MyDynamicDataset
split = preprocessing.create_trainvaltest_split('ml_1m', 1234, True, verbose=False)
(_, _, A, tr_l, tr_u, tr_v, _, _, _, _, _, _, cv) = split
ds = MyDynamicDataset('data/x', A, (tr_u, tr_v), tr_l, 1, 1.0, 100, None, None, cv, device=0, seed=1)
model = IGMC(ds, latent_dim=[32, 32, 32, 32], num_relations=5, num_bases=4, regression=True, adj_dropout=0.0, seed=1).to('cuda')
model.reset_parameters()
opt = FlatAdam(model, lr=1e-3)
sg = StepGraph(model, opt, ds, 50, 0.001)
perm = torch.randperm(len(ds), generator=torch.Generator().manual_seed(1))
sg.begin_epoch(perm, 1)
sg.steps(1)
sg.prepare(steps_hint=64)
for rep in range(3):
    sg.steps(64)
    torch.cuda.synchronize()
    out = (C.c_ulonglong * 64)()
    lib = _lib.load()
    lib.cdll.igmc_debug_fin_clocks.argtypes = [C.c_void_p]
    assert lib.cdll.igmc_debug_fin_clocks(out) == 0
    v = list(out)
    def row(base, ks, names):
        return '  '.join('%s +%d' % (n, v[base + k] - v[base]) for k, n in zip(ks, names))
    ks = [(1, 'loads issued'), (2, 'rows reduced'), (3, 'words published'), (4, 'bias row'), (5, 'words polled'),
          (6, 'main pass stored'), (7, 'images stored')]
    ks = [(k, n) for k, n in ks if v[k]]      # (no 'bias row' stamp where a producer sums that row)
    print('main wg (layer 1, row 0): ' + row(0, [k for k, _ in ks], [n for _, n in ks]))
    # (each workgroup against its OWN first stamp: the shader clocks of different XCDs do not share an origin)
    print('lin wg: ' + row(16, [1, 2], ['gradient tile', 'adam done']))
    print('tick wg: ' + row(32, [1, 2], ['loss done', 'tick done']))
    if v[40]:
        print('row producer (layer 1, row 0, set 1): ' + row(40, [1, 2, 3], ['loads issued', 'set reduced', 'published']))
        print('bias producer (layer 1): ' + row(48, [1, 2, 3], ['loads issued', 'set reduced', 'published']))
sg.check()

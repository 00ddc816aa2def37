"""A/B of whole LIBRARY builds inside the bench step: several libcommu_hip.so files loaded side by side in one process, one
trainer, the library behind commu_amd._lib swapped between timing blocks, 3 x 20 steps each, interleaved (method of
docs/EXPERIMENTS.md 8f item 1).  Two copies of the same build give the A/A spread of the box.
python ab_lib.py parentA=/path/a.so parentB=/path/b.so new=commu-code_amd/lib/libcommu_hip.so
ms per optimiser step at the bench shape (L6 D512 T1024 B64, dropout 0.1)."""
import ctypes as C
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "commu-code_amd"))
import torch
from commu_amd import _lib
from commu_amd.model.config_helper import get_cfg
from commu_amd.model.dataset import BaseVocab, synthetic_batch
from commu_amd.train import Trainer, build_model


def open_lib(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, argtypes in _lib.PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = _lib._RESTYPE.get(name, C.c_int)
    return lib


specs = [a.split("=", 1) for a in sys.argv[1:]]
_lib.load()
libs = {n: open_lib(p) for n, p in specs}
dev = torch.device("cuda", 0)
cfg = get_cfg()
_lib._lib = libs[specs[0][0]]
model = build_model(cfg, BaseVocab(), dev, seed=1)
model.train()
tr = Trainer(model, cfg, num_gpus=1, settle_heap=False)
batches = [synthetic_batch(1024, 64, dev, seed=1111 + i) for i in range(4)]
for n, _ in specs:
    _lib._lib = libs[n]
    for i in range(4):
        tr.step(*batches[i % 4])
torch.cuda.synchronize()
res = {n: [] for n, _ in specs}
for rnd in range(3):
    for n, _ in specs:
        _lib._lib = libs[n]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(20):
            tr.step(*batches[i % 4])
        torch.cuda.synchronize()
        res[n].append(1e3 * (time.perf_counter() - t0) / 20)
        print(f"{n:12s} {res[n][-1]:.3f} ms/step", flush=True)
for n, _ in specs:
    print(f"mean {n:12s} {sum(res[n]) / len(res[n]):.3f} ms/step   ({' '.join('%.3f' % x for x in res[n])})")

"""Cost of the grouped optimiser step against the single-group one at the headline model's flat size (6 layers, d_model 512,
d_inner 1024: about 14.55 M elements).  Three arms timed alternately in one process, device events around REPS launches,
ROUNDS rounds: commu_adam_step; commu_adam_step_groups with four groups, decay on, the embedding frozen; the same with
nothing frozen.  Prints each arm's range over the rounds; the first arm's range is the yardstick for "not told apart".
Usage: python tests/probes/adam_groups_cost.py [ROUNDS [REPS]]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "commu-code_amd"))
import torch  # noqa: E402
from commu_amd import ops  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 200
D, DI, V, L = 512, 1024, 729, 6
tensors = [(D, 2), (D, 2), (V * D, 1)]                                          # r_w_bias, r_r_bias (no decay), embedding (frozen)
for layer in range(L):
    body = 0 if layer < 3 else 3                                                # the upper half at lr_mult 0.5
    tensors += [(3 * D * D, body), (D * D, body), (D, 2), (D, 2), (D * D, body), (DI * D, body), (DI, 2), (D * DI, body), (D, 2),
                (D, 2), (D, 2)]
tensors.append((V, 2))
bmap = []
for numel, grp in tensors:
    bmap += [grp] * ((numel + 63) // 64)
n = 64 * len(bmap)
dev = "cuda"
bm = torch.tensor(bmap, dtype=torch.uint8, device=dev)
p = torch.randn(n, device=dev)
g = 0.1 * torch.randn(n, device=dev)
m = 0.05 * torch.randn(n, device=dev)
v = 0.01 * torch.rand(n, device=dev) + 1e-4
pb = torch.zeros(n, device=dev, dtype=torch.bfloat16)
gn = torch.full((1,), 2.0, device=dev)
lrs, wds = [1e-3, 1e-3, 1e-3, 5e-4], [0.1, 0.1, 0.0, 0.1]
frozen_elems = 64 * sum(1 for k in bmap if k == 1)
arms = {
    "commu_adam_step": lambda: ops.adam_step(p, g, m, v, pb, 1e-3, 3, gnorm=gn, clip=0.25),
    "groups, embedding frozen": lambda: ops.adam_step_groups(p, g, m, v, pb, bm, lrs, wds, [False, True, False, False], 3,
                                                             gnorm=gn, clip=0.25),
    "groups, nothing frozen": lambda: ops.adam_step_groups(p, g, m, v, pb, bm, lrs, wds, [False] * 4, 3, gnorm=gn, clip=0.25),
}


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPS * 1e3          # us per launch


for f in arms.values():                            # warm up every arm
    for _ in range(20):
        f()
torch.cuda.synchronize()
res = {k: [] for k in arms}
for _ in range(ROUNDS):
    for k, f in arms.items():
        res[k].append(timed(f))
print(f"n = {n} elements ({len(bmap)} blocks), frozen {frozen_elems} ({100.0 * frozen_elems / n:.1f} %), {ROUNDS} rounds x {REPS} launches")
bytes_plain = n * (4 * 4 + 3 * 4 + 2)              # read p g m v, write p m v and the bf16 shadow
for k, xs in res.items():
    moved = bytes_plain + n // 64 if k != "commu_adam_step" else bytes_plain
    if "embedding frozen" in k:
        moved -= frozen_elems * (4 * 4 + 3 * 4 + 2)
    med = sorted(xs)[len(xs) // 2]
    print(f"{k:28s} {min(xs):7.2f} .. {max(xs):7.2f} us  (median {med:7.2f}; {moved / 1e6:6.1f} MB, {moved / med / 1e6:5.2f} TB/s at the median)")

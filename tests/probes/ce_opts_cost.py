"""Cost of the loss-option kernels against the plain loss kernels at the bench shape (65 536 rows x 729 logits, row pitch 768,
fp32 logits, bf16 dlogits).  Two arms timed alternately in one process, device events around REPS forward + backward pairs,
ROUNDS rounds: commu_ce_fwd + commu_ce_bwd; commu_ce_fwd_opts + commu_ce_bwd_opts (eps 0.1, zeta 1e-4).  Prints each arm's
range over the rounds; the plain arm's range is the yardstick for "not told apart".  The method of adam_groups_cost.py.
Usage: python tests/probes/ce_opts_cost.py [ROUNDS [REPS]]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "commu-code_amd"))
import torch  # noqa: E402
from commu_amd import ops  # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 50
ROWS, V, LD = 65536, 729, 768
dev = "cuda"
logits = torch.randn(ROWS, LD, device=dev)
target = torch.randint(0, V, (ROWS,), device=dev)
g = torch.full((ROWS,), 1.0 / ROWS, device=dev)
dl = torch.empty(ROWS, LD, device=dev, dtype=torch.bfloat16)


def plain():
    nll, lse = ops.ce_fwd(logits, target, V)
    ops.ce_bwd(logits, target, lse, g, V, dlogits=dl)


def opts():
    loss, nll, lse = ops.ce_fwd_opts(logits, target, V, 0.1, 1e-4)
    ops.ce_bwd_opts(logits, target, lse, g, V, 0.1, 1e-4, dlogits=dl)


arms = {"ce_fwd + ce_bwd": plain, "ce_fwd_opts + ce_bwd_opts": opts}


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPS * 1e3          # us per forward + backward pair


for f in arms.values():                            # warm up every arm
    for _ in range(10):
        f()
torch.cuda.synchronize()
res = {k: [] for k in arms}
for _ in range(ROUNDS):
    for k, f in arms.items():
        res[k].append(timed(f))
moved = ROWS * (2 * LD * 4 + LD * 2)               # the logits read twice, dlogits written once
print(f"{ROWS} rows x {V} logits (pitch {LD}), {ROUNDS} rounds x {REPS} pairs, {moved / 1e6:.0f} MB per pair")
med = {}
for k, xs in res.items():
    med[k] = sorted(xs)[len(xs) // 2]
    print(f"{k:28s} {min(xs):7.2f} .. {max(xs):7.2f} us  (median {med[k]:7.2f}; {moved / med[k] / 1e6:5.2f} TB/s at the median)")
a, b = med["ce_fwd + ce_bwd"], med["ce_fwd_opts + ce_bwd_opts"]
print(f"options / plain at the medians: {b / a:.4f}")

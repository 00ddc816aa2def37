"""fp32 TRAINING MODE (model.fp32_training / train.py --parity; csrc/train_f32.hip).

The reference trains in fp32 (train.py:48 `amp = None`).  This mode runs the gradient-enabled forward, the backward pass and
the optimiser step on fp32 operands end to end, so the reference's own gradients and optimiser steps (tests/golden/g1_train_*,
g8_optim) are held to fp32 bounds here -- the bf16 path's are cosine 0.995 / 6e-2 element-wise and 0.8 for the r_net.weight
Adam update (tests/test_model_gpu.py).
Kernels: against float64 on the CPU.  Model: against the reference's fixtures and the fp32 oracle with the same masks."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import xl_ref as X  # noqa: E402
from test_model_gpu import _dump, _load_script, _write_output_npy, build_from_fixture  # noqa: E402
from test_dropout_gpu import attn_keep  # noqa: E402

DEV = "cuda"


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name))


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def cos(a, b):
    a = torch.as_tensor(a).detach().double().cpu().flatten()
    b = torch.as_tensor(b).detach().double().cpu().flatten()
    return float(torch.dot(a, b) / (a.norm() * b.norm() + 1e-300))


def keep_p(p):
    """exact keep probability of the element-wise dropout masks (threshold round(p * 65536))"""
    return 1.0 - min(65535, max(1, int(p * 65536.0 + 0.5))) / 65536.0 if p > 0 else 1.0


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("mode", ["nt", "nn", "tn"])
@pytest.mark.parametrize("M,N,K", [(65, 129, 68), (1, 37, 1000), (130, 63, 17), (257, 200, 1024)])
def test_gemm_f32_vs_float64(mode, M, N, K):
    from commu_amd import ops
    g = torch.Generator().manual_seed(M * 31 + N * 7 + K)
    ta, tb = mode == "tn", mode == "nt"
    a_shape = (K, M) if ta else (M, K)
    b_shape = (N, K) if tb else (K, N)
    # strided leading dimensions: views into wider buffers
    A_big = torch.randn(a_shape[0], a_shape[1] + 3, generator=g)
    B_big = torch.randn(b_shape[0], b_shape[1] + 5, generator=g)
    A, B = A_big[:, 1:1 + a_shape[1]], B_big[:, 2:2 + b_shape[1]]
    opA = A.double().t() if ta else A.double()
    opB = B.double().t() if tb else B.double()
    ref = opA @ opB
    C0 = torch.randn(M, N + 7, generator=g)
    out = C0.to(DEV)
    ops.gemm_f32(A_big.to(DEV)[:, 1:1 + a_shape[1]], B_big.to(DEV)[:, 2:2 + b_shape[1]], out=out[:, :N], ta=ta, tb=tb)
    torch.cuda.synchronize()
    assert rel(out[:, :N], ref) <= 2e-6
    assert torch.equal(out[:, N:].cpu(), C0[:, N:])                  # nothing written outside the view
    ops.gemm_f32(A_big.to(DEV)[:, 1:1 + a_shape[1]], B_big.to(DEV)[:, 2:2 + b_shape[1]], out=out[:, :N], ta=ta, tb=tb,
                 accumulate=True)
    assert rel(out[:, :N], 2 * ref) <= 2e-6


def test_gemm_f32_epilogue_and_split_tn():
    from commu_amd import ops
    g = torch.Generator().manual_seed(5)
    M, N, K = 300, 70, 130
    A, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    bias, resid = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    p, seed = 0.2, 12345
    keep = ops.dropout_keep_mask(seed, M * N, p).view(M, N).double()
    ref = torch.relu(A.double() @ W.double().t() + bias.double()) * keep / keep_p(p) + resid.double()
    out = ops.gemm_f32(A.to(DEV), W.to(DEV), bias=bias.to(DEV), relu=True, drop_p=p, drop_seed=seed, resid=resid.to(DEV))
    assert rel(out, ref) <= 2e-6
    # weight gradient over 65536 rows: the row split (slabs reduced in order), accumulate; deterministic
    R, N2, K2 = 65536, 96, 80
    dY, Xa = torch.randn(R, N2, generator=g), torch.randn(R, K2, generator=g)
    ref = dY.double().t() @ Xa.double()
    assert ops.f32_slabs(N2, K2, R) > 1
    dYd, Xd = dY.to(DEV), Xa.to(DEV)
    acc = torch.ones(N2, K2, device=DEV)
    ops.gemm_f32(dYd, Xd, out=acc, ta=True, tb=False, accumulate=True)
    assert rel(acc - 1, ref) <= 1e-5
    o1 = ops.gemm_f32(dYd, Xd, ta=True, tb=False)
    o2 = ops.gemm_f32(dYd, Xd, ta=True, tb=False)
    assert torch.equal(o1, o2)
    assert rel(o1, ref) <= 1e-5


def _attn_case(T, M, B, H, DH, same_length, reset_col, clamp, patt, seed=0):
    g = torch.Generator().manual_seed(seed + 17 * T + M)
    K, HD = T + M, H * DH
    qkv = torch.randn(K * B, 3 * HD, generator=g) * 0.5
    rd = torch.randn(K, HD, generator=g) * 0.5
    if clamp > 0:                     # a clamped table: distances >= clamp share the row of `clamp`
        rd[clamp:] = rd[clamp]
    u, vb = torch.randn(HD, generator=g) * 0.3, torch.randn(HD, generator=g) * 0.3
    dO = torch.randn(T * B, HD, generator=g)
    reset = torch.zeros(B, dtype=torch.bool)
    if reset_col is not None:
        reset[reset_col] = True
    return qkv, rd, u, vb, dO, reset


# (T, M, B, H, DH, same_length, reset column, clamp_len, attention dropout)
ATTN_CASES = {
    "nomem": (40, 0, 2, 2, 64, False, None, 0, 0.0),
    "mem16": (24, 16, 3, 2, 32, False, None, 0, 0.0),
    "mem40_reset": (33, 40, 2, 2, 64, False, 1, 0, 0.0),
    "same_length": (30, 20, 2, 2, 64, True, None, 0, 0.0),
    "clamp9": (26, 14, 2, 1, 32, False, None, 9, 0.0),
    "dh50": (37, 16, 2, 2, 50, False, 0, 0, 0.0),
    "dropatt": (70, 40, 2, 2, 64, True, 1, 0, 0.15),
}


@pytest.mark.parametrize("case", list(ATTN_CASES))
def test_attention_f32_fwd_bwd_vs_float64(case):
    """out, lse, dq, dk, dv (memory rows included), dRd and both bias gradients against float64 autograd of the oracle's
    attention math (rel_attention_scores, the masked softmax, P . V) with the kernels' own dropout mask injected."""
    from commu_amd import ops
    T, M, B, H, DH, sl, rcol, clamp, patt = ATTN_CASES[case]
    K, HD = T + M, H * DH
    mem_len = M if M > 0 else T
    seed = 4242
    qkv, rd, u, vb, dO, reset = _attn_case(T, M, B, H, DH, sl, rcol, clamp, patt)
    scale = 1.0 / math.sqrt(DH)
    # float64 reference
    q64 = qkv[M * B:, :HD].double().reshape(T, B, H, DH).requires_grad_(True)
    k64 = qkv[:, HD:2 * HD].double().reshape(K, B, H, DH).requires_grad_(True)
    v64 = qkv[:, 2 * HD:].double().reshape(K, B, H, DH).requires_grad_(True)
    rd64 = rd.double().requires_grad_(True)
    u64, vb64 = u.double().view(H, DH).requires_grad_(True), vb.double().view(H, DH).requires_grad_(True)
    r_pos = rd64.flip(0).reshape(K, H, DH)                       # the oracle's table is in position order
    S = X.rel_attention_scores(q64, k64, r_pos, u64, vb64) * scale
    mask = X.attn_mask(T, M, B, reset if M > 0 else None, sl, mem_len)
    S = S.masked_fill(mask[:, None], float("-inf"))
    lse_ref = torch.logsumexp(S, 3)
    P = torch.softmax(S, 3)
    if patt > 0:
        keep, pk = attn_keep(ops.site_seed(seed, 16), B, H, T, K, patt)
        P = P * keep.double() / pk
    out_ref = torch.einsum("bnij,jbnd->ibnd", P, v64).reshape(T * B, HD)
    (out_ref * dO.double()).sum().backward()
    # kernels
    qkv_d, rd_d, u_d, vb_d = qkv.to(DEV), rd.to(DEV), u.to(DEV), vb.to(DEV)
    rst = reset.to(DEV, torch.uint8) if M > 0 else None
    args = (T, M, B, H, DH, sl, mem_len, scale)
    out, lse = ops.relattn_fwd_f32(qkv_d[M * B:, :HD], qkv_d[:, HD:2 * HD], qkv_d[:, 2 * HD:], rd_d, u_d, vb_d, rst, *args,
                                   drop_p=patt, drop_seed=ops.site_seed(seed, 16))
    dqkv = torch.full((K * B, 3 * HD), float("nan"), device=DEV)
    drd = torch.empty(K, HD, device=DEV)
    dq_ac, dq_bd = ops.relattn_bwd_f32(qkv_d[M * B:, :HD], qkv_d[:, HD:2 * HD], qkv_d[:, 2 * HD:], rd_d, u_d, vb_d, rst,
                                       out, dO.to(DEV), lse, *args, dqkv[M * B:, :HD], dqkv[:, HD:2 * HD], dqkv[:, 2 * HD:], drd,
                                       drop_p=patt, drop_seed=ops.site_seed(seed, 16))
    ones = torch.ones(T * B, device=DEV)
    gu, gvb = torch.zeros(HD, device=DEV), torch.zeros(HD, device=DEV)
    ops.colsum_f32(dq_ac, gu, ones)
    ops.colsum_f32(dq_bd, gvb, ones)
    torch.cuda.synchronize()
    tol = 1e-5
    assert rel(out, out_ref) <= tol
    assert rel(lse, lse_ref) <= tol
    assert rel(dqkv[M * B:, :HD], q64.grad.reshape(T * B, HD)) <= tol
    assert rel(dqkv[:, HD:2 * HD], k64.grad.reshape(K * B, HD)) <= tol
    assert rel(dqkv[:, 2 * HD:], v64.grad.reshape(K * B, HD)) <= tol
    assert rel(drd, rd64.grad) <= tol
    assert rel(gu, u64.grad.reshape(-1)) <= tol
    assert rel(gvb, vb64.grad.reshape(-1)) <= tol
    assert rel(dq_ac + dq_bd, dqkv[M * B:, :HD]) == 0.0


@pytest.mark.parametrize("DH", [36, 50])          # 36: the 16-byte vector path, 50: the scalar path
def test_attention_f32_forward_two_entries_agree_bitwise(DH):
    """commu_relattn_fwd_f32 without dropout and commu_relattn_f32 run ONE row function (csrc/attn_row_f32.h): the same bits
    from the same projections; the training entry's lse against float64 at the bound of the test above."""
    from commu_amd import ops
    T, M, B, H, sl, mem_len = 5, 3, 2, 2, True, 3
    K, HD = T + M, H * DH
    qkv, rd, u, vb, _, reset = _attn_case(T, M, B, H, DH, sl, 1, 0, 0.0)
    scale = 1.0 / math.sqrt(DH)
    q64 = qkv[M * B:, :HD].double().reshape(T, B, H, DH)
    k64 = qkv[:, HD:2 * HD].double().reshape(K, B, H, DH)
    S = X.rel_attention_scores(q64, k64, rd.double().flip(0).reshape(K, H, DH), u.double().view(H, DH),
                               vb.double().view(H, DH)) * scale
    S = S.masked_fill(X.attn_mask(T, M, B, reset, sl, mem_len)[:, None], float("-inf"))
    lse_ref = torch.logsumexp(S, 3)
    qkv_d, rd_d, u_d, vb_d, rst = qkv.to(DEV), rd.to(DEV), u.to(DEV), vb.to(DEV), reset.to(DEV, torch.uint8)
    q, k, v = qkv_d[M * B:, :HD], qkv_d[:, HD:2 * HD], qkv_d[:, 2 * HD:]
    out_t, lse = ops.relattn_fwd_f32(q, k, v, rd_d, u_d, vb_d, rst, T, M, B, H, DH, sl, mem_len, scale, drop_p=0.0)
    out_p = ops.relattn_f32(q, k, v, B * 3 * HD, 3 * HD, rd_d, u_d, vb_d, T, M, B, H, DH, sl, mem_len, scale, reset=rst)
    torch.cuda.synchronize()
    assert torch.isfinite(out_p).all()
    assert torch.equal(out_t, out_p)
    assert rel(lse, lse_ref) <= 1e-5


@pytest.mark.parametrize("with_add", [False, True])
def test_layernorm_f32_bwd_vs_float64(with_add):
    from commu_amd import ops
    g = torch.Generator().manual_seed(3)
    rows, D = 777, 500
    x = torch.randn(rows, D, generator=g) * 2 + 0.5
    gam, bet = torch.randn(D, generator=g), torch.randn(D, generator=g)
    dy, add = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
    x64 = x.double().requires_grad_(True)
    g64, b64 = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    y64 = X.layer_norm(x64, g64, b64)
    (y64 * (dy.double() + (add.double() if with_add else 0))).sum().backward()
    y, mu, rs = ops.layernorm_fwd_f32(x.to(DEV), gam.to(DEV), bet.to(DEV))
    assert rel(y, y64) <= 1e-6
    dgam, dbet = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    dx = ops.layernorm_bwd_f32(dy.to(DEV), x.to(DEV), mu, rs, gam.to(DEV), dgamma=dgam, dbeta=dbet,
                               add=add.to(DEV) if with_add else None)
    torch.cuda.synchronize()
    assert rel(dx, x64.grad) <= 1e-6
    assert rel(dgam, g64.grad) <= 1e-6
    assert rel(dbet, b64.grad) <= 1e-6


# ------------------------------------------------------------------------------------------------ model
def _fp32(model):
    model.fp32_training = True
    return model


@pytest.mark.parametrize("tag", ["mem", "nomem", "dh50", "clamp"])
def test_g1_forward_backward_fp32_vs_reference(golden_dir, tag):
    z = load(golden_dir, f"g1_train_{tag}.npz")
    model, cfg = build_from_fixture(z)
    _fp32(model).eval()
    mems = None
    for seg in range(3):
        data = torch.from_numpy(z[f"data{seg}"]).to(DEV)
        target = torch.from_numpy(z[f"target{seg}"]).to(DEV)
        reset = torch.from_numpy(z[f"reset{seg}"]).to(DEV)
        model.zero_grad()
        loss, mems = model(data, target, reset, mems)
        assert rel(loss, z[f"loss{seg}"]) <= 1e-5
        if tag != "nomem":
            assert mems.dtype == torch.float32 and mems.shape == z[f"mems{seg}"].shape
            assert rel(mems, z[f"mems{seg}"]) <= 1e-5
        else:
            assert mems is None
        scalar = loss[target != 0].float().mean()
        assert abs(float(scalar) - float(z[f"scalar{seg}"])) <= 1e-5 * abs(float(z[f"scalar{seg}"]))
        scalar.backward()
    worst, cosines, sign_cos, sign_mass = {}, {}, {}, {}
    for name, p in model.named_parameters():
        ref = torch.from_numpy(z["g::" + name]).flatten()
        got = p.grad.detach().float().cpu().flatten()
        worst[name] = rel(got, ref)
        cosines[name] = cos(got, ref)
        sign_cos[name] = float((torch.sign(got) * torch.sign(ref)).mean())
        sign_mass[name] = float((ref.abs() * (torch.sign(got) == torch.sign(ref))).sum() / (ref.abs().sum() + 1e-30))
    _dump(f"g1_fp32_{tag}", {"relerr": worst, "cos": cosines, "sign_cos": sign_cos, "sign_mass": sign_mass})
    assert min(cosines.values()) >= 0.99999, cosines
    for k, v in worst.items():          # every tensor, the first FFN Linear included
        assert v <= 1e-4, (k, v)


def test_g8_optimizer_steps_fp32_vs_reference(golden_dir):
    """clip + Adam + LambdaLR over the reference's 4 optimiser steps (batch_chunk 2) in fp32 training mode."""
    from commu_amd.functional import masked_mean
    from commu_amd.optim import FusedAdam, clip_grad_norm_, lr_lambda_factory
    z = load(golden_dir, "g8_optim.npz")
    model, _ = build_from_fixture(z)
    _fp32(model)
    chunk = int(z["meta"][8])
    lr = 0.004
    opt = FusedAdam(model, lr=lr)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lr_lambda_factory(int(z["warmup"]), lr, 0.0001))
    mems = [None] * chunk
    losses, gnorms = [], []
    for step in range(int(z["nsteps"])):
        data = torch.from_numpy(z[f"data{step}"]).to(DEV)
        target = torch.from_numpy(z[f"target{step}"]).to(DEV)
        reset = torch.from_numpy(z[f"reset{step}"]).to(DEV)
        model.zero_grad()
        tot = 0.0
        for i in range(chunk):
            d, t, r = [torch.chunk(x, chunk, dim)[i].contiguous() for x, dim in ((data, 1), (target, 1), (reset, 0))]
            loss, mems[i] = model(d, t, r, mems[i])
            loss = masked_mean(loss, t, 0, 1.0 / chunk)
            loss.backward()
            tot += float(loss)
        gn = float(clip_grad_norm_(model, float(z["clip"]), opt))
        opt.step()
        opt.zero_grad()
        sched.step()
        losses.append((tot, float(z[f"loss{step}"])))
        gnorms.append((gn, float(z[f"gnorm{step}"])))
    cosd = {}
    for name, p in model.named_parameters():
        before, after = z["p::" + name], z["after::" + name]
        cosd[name] = cos(p.detach().cpu() - torch.from_numpy(before), torch.from_numpy(after - before))
    _dump("g8_fp32", {"cos": cosd, "loss": losses, "gnorm": gnorms})
    for got, ref in losses:
        assert abs(got - ref) <= 1e-5 * abs(ref), losses
    for got, ref in gnorms:
        assert abs(got - ref) <= 1e-5 * abs(ref), gnorms
    for k, v in cosd.items():           # every tensor, r_net.weight included
        assert v >= 0.999, (k, v)


def _train_mode_model(golden_dir, p_drop, p_att):
    z = np.load(os.path.join(golden_dir, "g1_train_mem.npz"))
    model, cfg = build_from_fixture(z)
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = p_drop
    for layer in model.layers:
        layer.dec_attn.dropatt.p = p_att
    _fp32(model).train()
    return model, z


def test_train_mode_fp32_matches_oracle_with_same_masks(golden_dir):
    """dropout 0.1 / attention dropout 0.15, two segments with memory and a reset, against the oracle with the kernels'
    masks injected at the reference's nn.Dropout sites (exact keep probabilities)."""
    from commu_amd import ops
    p_drop, p_att = 0.1, 0.15
    model, z = _train_mode_model(golden_dir, p_drop, p_att)
    L, H, D, DI, T, B, mem_len, sl = [int(x) for x in z["meta"][:8]]
    s = X.XLShape(L, H, D, DI)
    params = {k[3:]: torch.from_numpy(z[k]).clone().requires_grad_(True) for k in z.files
              if k.startswith("p::") and not k.endswith("inv_freq")}
    data, target = torch.from_numpy(z["data0"]), torch.from_numpy(z["target0"])
    data1, target1 = torch.from_numpy(z["data2"]), torch.from_numpy(z["target2"])
    reset = torch.from_numpy(z["reset2"])
    assert bool(reset.any())

    def make_drop(seed):
        site_id = {"emb": lambda li: 0, "pos": lambda li: 1, "final": lambda li: 2, "att": lambda li: 16 + 4 * li,
                   "o": lambda li: 17 + 4 * li, "hid": lambda li: 18 + 4 * li, "out": lambda li: 19 + 4 * li}

        def drop(site, x):
            kind, li = site
            ss = ops.site_seed(seed, site_id[kind](li))
            if kind == "att":
                keep, pk = attn_keep(ss, x.shape[0], x.shape[1], x.shape[2], x.shape[3], p_att)
                return x * keep / pk
            keep = ops.dropout_keep_mask(ss, x.numel(), p_drop).view(x.shape)
            if kind == "pos":                       # the kernel's table is indexed by distance = reversed rows
                keep = ops.dropout_keep_mask(ss, x.numel(), p_drop).view(x.shape).flip(0)
            return x * keep / keep_p(p_drop)
        return drop

    torch.manual_seed(1234)
    seeds = [int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) for _ in range(2)]
    torch.manual_seed(1234)                         # the model draws the same base seeds
    model.zero_grad()
    loss0, mems = model(data.to(DEV), target.to(DEV), torch.zeros(B, dtype=torch.bool, device=DEV), None)
    loss1, mems1 = model(data1.to(DEV), target1.to(DEV), reset.to(DEV), mems)
    loss1[target1.to(DEV) != 0].float().mean().backward()
    o0, omems = X.forward_loss(params, s, data, target, torch.zeros(B, dtype=torch.bool), None, mem_len, bool(sl), make_drop(seeds[0]))
    o1, omems1 = X.forward_loss(params, s, data1, target1, reset, omems.detach(), mem_len, bool(sl), make_drop(seeds[1]))
    assert rel(loss0, o0) <= 1e-5 and rel(loss1, o1) <= 1e-5
    assert rel(mems, omems) <= 1e-5 and rel(mems1, omems1) <= 1e-5
    grads = torch.autograd.grad(o1[target1 != 0].mean(), list(params.values()))
    named = dict(model.named_parameters())
    res = {k: (rel(named[k].grad, g), cos(named[k].grad, g)) for (k, _), g in zip(params.items(), grads)}
    _dump("train_mode_fp32", res)
    for k, (r, c) in res.items():
        assert r <= 1e-4 and c >= 0.99999, (k, r, c)


def test_fp32_backward_is_deterministic(golden_dir):
    model, z = _train_mode_model(golden_dir, 0.1, 0.15)
    model.fixed_drop_seed = 777
    data, target = torch.from_numpy(z["data1"]).to(DEV), torch.from_numpy(z["target1"]).to(DEV)
    B = data.shape[1]
    reset = torch.zeros(B, dtype=torch.bool, device=DEV)
    outs = []
    for _ in range(2):
        model.zero_grad()
        _, mems = model(data, target, reset, None)
        loss, _ = model(data, target, reset, mems)
        loss[target != 0].mean().backward()
        outs.append({n: p.grad.detach().clone() for n, p in model.named_parameters()})
    for n in outs[0]:
        assert torch.equal(outs[0][n], outs[1][n]), n


def test_grad_autograd_mode_and_accumulation(golden_dir):
    """grad_mode "autograd" returns the gradients; two backward calls accumulate like the bf16 path."""
    z = load(golden_dir, "g1_train_mem.npz")
    model, _ = build_from_fixture(z)
    _fp32(model).eval()
    data, target = torch.from_numpy(z["data0"]).to(DEV), torch.from_numpy(z["target0"]).to(DEV)
    reset = torch.zeros(data.shape[1], dtype=torch.bool, device=DEV)
    model.zero_grad()
    loss, _ = model(data, target, reset, None)
    loss.mean().backward()
    g1 = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    loss, _ = model(data, target, reset, None)
    loss.mean().backward()
    for n, p in model.named_parameters():
        assert rel(p.grad, 2 * g1[n]) <= 1e-6, n
    model.zero_grad()
    model.grad_mode = "autograd"
    loss, _ = model(data, target, reset, None)
    loss.mean().backward()
    for n, p in model.named_parameters():
        assert torch.equal(p.grad, g1[n]), n


def test_grad_ready_hook_fp32_reports_layer_slices_top_down(golden_dir):
    z = load(golden_dir, "g1_train_mem.npz")
    model, _ = build_from_fixture(z)
    _fp32(model).eval()
    data, target = torch.from_numpy(z["data0"]).to(DEV), torch.from_numpy(z["target0"]).to(DEV)
    seen = []
    model.grad_ready_hook = lambda G, lo, hi: seen.append((lo, hi, G[lo:hi].clone()))
    model.zero_grad()
    loss, _ = model(data, target, torch.zeros(data.shape[1], dtype=torch.bool, device=DEV), None)
    loss.mean().backward()
    model.grad_ready_hook = None
    fl = model._flat
    L = model.n_layer
    want = [(model._name_off[f"layers.{i}.dec_attn.qkv_net.weight"],
             model._name_off[f"layers.{i + 1}.dec_attn.qkv_net.weight"] if i + 1 < L else model._name_off["crit.out_layers.0.bias"])
            for i in range(L - 1, -1, -1)]
    assert [(lo, hi) for lo, hi, _ in seen] == want
    for lo, hi, snap in seen:                # each slice was final when reported
        assert torch.equal(snap, fl["g"][lo:hi])


def test_parity_fp32_alone_still_raises_on_a_gradient_pass(golden_dir):
    from commu_amd._lib import CommuHipError
    z = load(golden_dir, "g1_train_mem.npz")
    model, _ = build_from_fixture(z)
    model.parity_fp32 = True
    model.eval()
    data, target = torch.from_numpy(z["data0"]).to(DEV), torch.from_numpy(z["target0"]).to(DEV)
    with pytest.raises(CommuHipError, match="fp32_training"):
        model(data, target, None, None)


def test_fp32_training_forward_equals_parity_forward_bitwise():
    """ONE fp32 forward schedule and one set of kernels behind both modes: the gradient-enabled fp32_training pass in eval()
    mode and the no-grad parity_fp32 pass give the same bits -- loss and new_mems of two consecutive segments, the second
    with memory and one reset sequence.  Every Linear has more than 64 rows (T * B = M * B = 130, T = 65 distances), so
    neither mode takes the decode step's skinny kernel."""
    from commu_amd.model.config_helper import get_cfg
    from commu_amd.model.dataset import BaseVocab
    from commu_amd.train import build_model
    T, B = 65, 2
    cfg = get_cfg(num_layers=2, num_heads=2, units=72, inner_size=100, tgt_length=T, mem_length=65, batch_size=B,
                  batch_chunk=1, dropout=0.1, attention_dropout=0.1)
    model = build_model(cfg, BaseVocab(), torch.device(DEV), seed=11)
    model.eval()
    assert (model.n_layer, model.n_head, model.d_model, model.d_head, model.d_inner, model.mem_len) == (2, 2, 72, 36, 100, 65)
    g = torch.Generator().manual_seed(3)
    segs = [(torch.randint(0, model.n_token, (T, B), generator=g).to(DEV),
             torch.randint(0, model.n_token, (T, B), generator=g).to(DEV),
             torch.tensor(r, dtype=torch.bool, device=DEV)) for r in ([False, False], [False, True])]

    def run():
        mems, outs = None, []
        for data, target, reset in segs:
            loss, mems = model(data, target, reset, mems)
            outs.append((loss.detach(), mems))
        return outs
    model.fp32_training = True
    train = run()
    assert train[0][0].dtype == torch.float32 and train[1][1].shape == (3, 65, B, 72)
    model.fp32_training, model.parity_fp32 = False, True
    with torch.no_grad():
        parity = run()
    for (loss_t, mems_t), (loss_p, mems_p) in zip(train, parity):
        assert torch.isfinite(loss_p).all()
        assert torch.equal(loss_t, loss_p)
        assert torch.equal(mems_t, mems_p)


# ------------------------------------------------------------------------------------------------ Trainer / CLI
@pytest.mark.parametrize("merge", [True, False])
def test_trainer_fp32_steps_vs_oracle_train_step(merge):
    from commu_amd.model.config_helper import get_cfg
    from commu_amd.model.dataset import BaseVocab, synthetic_batch
    from commu_amd.train import Trainer, build_model
    cfg = get_cfg(num_layers=2, num_heads=2, units=128, inner_size=256, tgt_length=48, mem_length=32,
                  batch_size=4, batch_chunk=2, dropout=0.0, attention_dropout=0.0)
    model = build_model(cfg, BaseVocab(), torch.device(DEV), seed=7)
    _fp32(model)
    trainer = Trainer(model, cfg, merge_chunks=merge, graph=True)
    p = {k: v.detach().float().cpu().clone() for k, v in model.state_dict().items()
         if k not in ("crit.out_layers.0.weight", "pos_emb.inv_freq")}
    p0 = {k: v.clone() for k, v in p.items()}
    s = X.XLShape(2, 2, 128, 256)
    st = X.adam_init(p)
    omems = [None, None]
    for step in range(3):
        d, t, r, n = synthetic_batch(48, 4, DEV, seed=100 + step, reset_prob=0.3)
        lr_now = trainer.optimizer.param_groups[0]["lr"]
        loss = float(trainer.step(d, t, r, n))
        oloss, _, omems, _ = X.train_step(p, st, s, d.cpu(), t.cpu(), r.cpu(), omems, batch_chunk=2, mem_len=32,
                                          same_length=False, lr_now=lr_now, clip=cfg.TRAIN.clip)
        assert abs(loss - oloss) <= 1e-5 * abs(oloss), (step, loss, oloss)
    assert trainer._graphs is None and trainer.graph_failed is not None and "fp32_training" in trainer.graph_failed
    named = dict(model.named_parameters())
    for k in p:
        c = cos(named[k].detach().cpu() - p0[k], p[k] - p0[k])
        assert c >= 0.999, (k, c)


def test_train_cli_parity_flag(tmp_path, monkeypatch):
    import commu_amd.train as tr
    from commu_amd.train import read_checkpoint
    built = []
    orig = tr.build_model

    def spy(*a, **kw):
        m = orig(*a, **kw)
        built.append(m)
        return m
    monkeypatch.setattr(tr, "build_model", spy)
    rng = np.random.RandomState(0)
    corpus = {s_: [np.concatenate([rng.randint(560, 729, 11), rng.randint(2, 560, rng.randint(20, 90)), [1]])
                   for _ in range(n)] for s_, n in (("train", 40), ("valid", 12))}
    data_dir, work = tmp_path / "output_npy", tmp_path / "work"
    data_dir.mkdir()
    _write_output_npy(str(data_dir), corpus)
    cli = _load_script("train")
    assert cli.parse_args(["--data_dir", "x", "--work_dir", "y", "--parity"]).parity is True
    run_dir = cli.main(["--data_dir", str(data_dir), "--work_dir", str(work), "--num_layers", "2", "--num_heads", "2",
                        "--units", "64", "--inner_size", "128", "--tgt_length", "16", "--mem_length", "16",
                        "--batch_size", "4", "--batch_chunk", "2", "--max_step", "4", "--log_interval", "2",
                        "--eval_interval", "2", "--parity"])
    assert len(built) == 1 and built[0].fp32_training is True and built[0].parity_fp32 is True
    log = open(os.path.join(run_dir, "train_rank0.log")).read()
    assert log.count("Train Step") == 2 and "End of training" in log
    assert log.count("| End of training | test nll") == 1
    for name in ("checkpoint_last.pt", "checkpoint_best.pt"):
        ck = read_checkpoint(os.path.join(run_dir, name))
        assert ck["train_step"] in (2, 4) and ck["amp"] is None and "optimizer" in ck
        assert all(v.dtype == torch.float32 for v in ck["model"].values())
    nll = float(log.split("nll=")[1].split(",")[0])
    assert 5.0 < nll < 7.5

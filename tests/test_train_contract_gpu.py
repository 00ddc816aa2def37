"""The training step's support kernels (csrc/elementwise.hip) against the float64 contracts of tests/train_contract.py, at
the shapes where they can go wrong: half chunks, zero-padded rows, row counts on the block / wave / pair edges, both
cross-entropy kernels of each direction, the grouped column sum with two launches, column-grouped loss means, the
optimiser's grid-stride bodies.  Guards on every launch: NaN in input pad columns, a sentinel in output columns beyond the
zeroing contract, non-zero accumulated outputs, NaN workspaces.  Every test prints its worst ratios to the bounds
(NAME~: the error beyond the output format's own rounding, see the contract's docstring); tests/test_train_contract_host.py
shows on the CPU that these inputs catch the planted defects."""
import numpy as np
import pytest
import torch

import train_contract as TC

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
DROP_P, DROP_SEED = 0.25, 424243


def ops():
    from commu_amd import ops as o
    return o


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def host(t):
    return t.detach().float().cpu().numpy()


def full(shape, value, dtype=torch.float32):
    return torch.full(shape, value, device=DEV, dtype=dtype)


def settle(name, res):
    """print the figures, then hold every one of them to its bound"""
    if not isinstance(res, dict):
        res = {"": res}
    print("RATIO " + name + " " + " ".join(f"{k}={v:.4f}" for k, v in sorted(res.items())))
    bad = {k: v for k, v in res.items() if not v <= 1.0}
    assert not bad, (name, bad)
    return max(res.values())


@pytest.mark.parametrize("case", TC.ln_cases(), ids=lambda c: "D%d_ld%d_r%d" % c)
def test_layernorm_fwd_bwd_contract(case):
    o = ops()
    inp = TC.LnInputs(*case)
    D, ld, rows = case
    z, dy, dy2 = dev(inp.z, BF), dev(inp.dy, BF), dev(inp.dy2, BF)
    gamma, beta = dev(inp.gamma), dev(inp.beta)
    y, mean, rstd = full((rows, ld), TC.SENT, BF), full((rows,), float("nan")), full((rows,), float("nan"))
    o.layernorm_fwd(z, gamma, beta, y=y, mean=mean, rstd=rstd, eps=TC.LN_EPS)
    settle("layernorm_fwd", TC.ln_check_fwd(inp, host(y), host(mean), host(rstd)))
    mu32, rs32 = TC.ln_stats32(inp)
    mu, rs = dev(mu32), dev(rs32)
    keep = o.dropout_keep_mask(DROP_SEED, rows * D, DROP_P).view(rows, D).numpy()
    scale = TC.drop_scale(DROP_P)
    nblk = (rows + 31) // 32
    for add, masked in ((False, False), (True, False), (True, True), (False, True)):
        dz, part = full((rows, ld), TC.SENT, BF), full((nblk, 3, D), float("nan"))
        dzm = full((rows, ld), TC.SENT, BF) if masked else None
        o.layernorm_bwd(dy, z, mu, rs, gamma, dz=dz, part=part, dz_masked=dzm, drop_p=DROP_P if masked else 0.0,
                        drop_seed=DROP_SEED, add=dy2 if add else None)
        res = TC.ln_check_bwd(inp, mu32, rs32, host(dz), host(part), add, keep if masked else None, scale,
                              host(dzm) if masked else None)
        settle("layernorm_bwd" + ("_add" if add else "") + ("_masked" if masked else ""), res)


def test_layernorm_bwd_reduce_contract():
    o = ops()
    for nblk in TC.REDUCE_NBLK:
        for D in TC.REDUCE_D:
            g = torch.Generator().manual_seed(nblk * 1000 + D)
            part = torch.randn(nblk, 3, D, generator=g) * (1 + torch.arange(3.0))[None, :, None]
            before = torch.randn(3, D, generator=g) * 5
            for with_bias in (True, False):
                outs = [before.clone().to(DEV) for _ in range(2)]
                for out in outs:          # twice: the sum is deterministic
                    o.layernorm_bwd_reduce(part.to(DEV), out[0], out[1], out[2] if with_bias else None)
                assert torch.equal(outs[0], outs[1])
                res = {}
                for zpl in range(2 + with_bias):
                    r = TC.colsum_check(host(outs[0][zpl]), before[zpl].numpy(), [(part[:, zpl].numpy(), 1.0)])
                    res = {k: max(v, res.get(k, 0.0)) for k, v in r.items()}
                if not with_bias:
                    assert torch.equal(outs[0][2].cpu(), before[2])
                settle(f"layernorm_bwd_reduce nblk={nblk} D={D} bias={with_bias}", res)


def _group_run(o, grp, grouped):
    """the tasks of one train_contract.group_cases() group on the device: through one ColsumGroup, or launch by launch"""
    outs = [dev(t[0]) for t in grp]
    group = o.ColsumGroup() if grouped else None
    keep = []
    for out, (_, srcs) in zip(outs, grp):
        for kind, X, alpha in srcs:
            rows, cols = X.shape
            if kind == "part":
                part = full((rows, 3, cols), float("nan"))
                part[:, 2] = dev(X)
                o.layernorm_bwd_reduce(part, None, None, out, group=group)
                keep.append(part)
                continue
            ldx = (cols + 7) // 8 * 8 if (kind == "bf16" or cols % 4 == 0) else cols
            buf = full((rows, ldx), float("nan"), BF if kind == "bf16" else torch.float32)
            buf[:, :cols] = dev(X, buf.dtype)
            keep.append(buf)
            if kind == "bf16" and not grouped:          # (ops.colsum allocates the slab workspace itself: here it starts as NaN)
                ny = o.call("commu_colsum_slabs", rows, cols, 2)
                assert ny == TC.colsum_slabs(rows, cols, 2) and ny > 1
                ws = full((ny, ldx), float("nan"))
                o.call("commu_colsum_bf16", o._p(buf), ldx, rows, cols, o._p(out), o._p(ws), ny, float(alpha), o._s())
                assert bool(torch.isfinite(ws[:, :cols]).all())
                continue
            o.colsum(buf[:, :cols], out, alpha, group=group)
    if grouped:
        group.flush()
    torch.cuda.synchronize()
    return outs


def test_colsum_group_contract():
    o = ops()
    for name, grp in zip(("three_outputs", "fifty_outputs"), TC.group_cases()):
        a, b, single = _group_run(o, grp, True), _group_run(o, grp, True), _group_run(o, grp, False)
        res = {}
        for t, oa, ob, os_ in zip(grp, a, b, single):
            assert torch.equal(oa, ob)
            src = [(X, al) for _, X, al in t[1]]
            for tag, got in (("group", oa), ("launches", os_)):
                for k, v in TC.colsum_check(host(got), t[0], src).items():
                    res[tag + "." + k] = max(v, res.get(tag + "." + k, 0.0))
        settle("colsum_group " + name, res)


@pytest.mark.parametrize("case", TC.ce_bwd_cases(), ids=lambda c: "V%d_ldl%d_ldd%d_r%d" % c)
def test_cross_entropy_contract(case):
    o = ops()
    V, ldl, ldd, rows = case
    inp = TC.CeInputs(V, ldl, rows)
    x, target = dev(inp.x), dev(inp.target, torch.int64)
    assert x.stride(0) == ldl
    nll, lse = full((rows,), float("nan")), full((rows,), float("nan"))
    o.call("commu_ce_fwd", o._p(x), ldl, o._p(target), o._p(nll), o._p(lse), rows, V, o._s())
    settle("ce_fwd" + ("_vec" if TC.ce_vec_fwd(V, ldl) else "_scalar"), TC.ce_check_fwd(inp, host(nll), host(lse)))
    lse32 = TC.ce_lse32(inp)
    d = full((rows, ldd), TC.SENT, BF)
    o.ce_bwd(x, target, dev(lse32), dev(inp.g), V, dlogits=d)
    settle("ce_bwd" + ("_vec" if TC.ce_vec_bwd(V, ldl, ldd) else "_scalar"), TC.ce_check_bwd(inp, lse32, host(d), ldd))


@pytest.mark.parametrize("case", TC.MM_CASES, ids=lambda c: "T%d_B%d_Bc%d" % c)
def test_masked_mean_groups_contract(case):
    o = ops()
    T, B, Bc = case
    G = B // Bc
    for all_pad in ((None, 1) if G > 1 else (None,)):
        inp = TC.MmInputs(T, B, Bc, all_pad)
        nll, target = dev(inp.nll), dev(inp.target, torch.int64)
        for with_all in (True, False):
            ws_sum, ws_cnt = full((G,), float("nan")), full((G,), -7, torch.int32)
            out, sum_all, g = full((1,), float("nan")), full((1,), float("nan")), full((inp.n,), float("nan"))
            o.masked_mean_groups(nll, target, TC.MM_PAD, float(inp.scale), B, Bc, ws_sum, ws_cnt, out,
                                 sum_all=sum_all if with_all else None)
            o.loss_grad_groups(target, TC.MM_PAD, ws_cnt, float(inp.scale), B, Bc, g)
            res = TC.mm_check(inp, host(out)[0], host(sum_all)[0] if with_all else None, ws_cnt.cpu().numpy(), host(g))
            if not with_all:
                assert bool(torch.isnan(sum_all).all())
            if all_pad is not None:
                assert bool(torch.isnan(out).all()) and bool(torch.isfinite(g).all())
            settle(f"masked_mean_groups all_pad={all_pad} sum_all={with_all}", res)
        if G == 1:          # one group on one workgroup: the plain masked mean, bit for bit (sums exact in any order)
            s1, c1, o1, g1 = full((1,), float("nan")), full((1,), -7, torch.int32), full((1,), float("nan")), \
                full((inp.n,), float("nan"))
            o.masked_mean(nll, target, TC.MM_PAD, float(inp.scale), s1, c1, o1)
            o.loss_grad(target, TC.MM_PAD, c1, float(inp.scale), g1)
            assert inp.n <= 1024 and torch.equal(o1, out) and torch.equal(g1, g) and torch.equal(c1, ws_cnt)


def _adam_buffers(arrs, n, off):
    """device copies with `off` elements in front (off = 1: no 16-byte alignment) and 8 guard elements behind"""
    out = []
    for a in arrs:
        t = full((off + n + 8,), TC.SENT)
        t[off:off + n] = dev(a)
        out.append(t)
    return out


@pytest.mark.parametrize("n,off", [(n, 0) for n in TC.ADAM_N] + [(TC.ADAM_N[-1], 1)])
def test_adam_and_scale_clip_contract(n, off):
    o = ops()
    p, g, m, v = TC.adam_inputs(n)
    gnorm = 2.0
    bc1, bc2 = o.adam_bias_corrections(TC.ADAM_B1, TC.ADAM_B2, TC.ADAM_STEP)
    assert abs(bc1 - float(TC.bias_corrections32(TC.ADAM_B1, TC.ADAM_B2, TC.ADAM_STEP)[0])) < 1e-6
    coef = TC.clip_coef32(gnorm, TC.ADAM_CLIP)
    want = TC.adam_ref(p, g, m, v, coef, TC.F32(bc1), TC.F32(bc2))
    gn = dev(np.array([gnorm], dtype=TC.F32))
    sl = slice(off, off + n)
    runs = []
    for form in ("host", "dev"):
        pd, gd, md, vd = _adam_buffers((p, g, m, v), n, off)
        pb = full((2 * off + n + 8,), TC.SENT, BF)
        args = (pd[sl], gd[sl], md[sl], vd[sl], pb[2 * off:2 * off + n])
        if form == "host":
            o.adam_step(*args, TC.ADAM_LR, TC.ADAM_STEP, gnorm=gn, clip=TC.ADAM_CLIP, beta1=TC.ADAM_B1, beta2=TC.ADAM_B2,
                        eps=TC.ADAM_EPS)
        else:
            scal = dev(np.array([TC.ADAM_LR, bc1, bc2], dtype=TC.F32))
            o.adam_step_dev(*args, scal, gnorm=gn, clip=TC.ADAM_CLIP, beta1=TC.ADAM_B1, beta2=TC.ADAM_B2, eps=TC.ADAM_EPS)
        runs.append((pd, md, vd, pb, gd))
    for a, b in zip(*runs):
        assert torch.equal(a, b)                                # adam_step_dev is adam_step, bit for bit
    pd, md, vd, pb, gd = runs[0]
    for t in (pd, md, vd, gd):                                  # nothing outside the slice moved
        assert bool((t[:off] == TC.SENT).all()) and bool((t[off + n:] == TC.SENT).all())
    assert bool((pb[:2 * off] == TC.SENT).all()) and bool((pb[2 * off + n:] == TC.SENT).all())
    assert torch.equal(gd[sl].cpu(), torch.from_numpy(g))
    settle(f"adam n={n} off={off}", TC.adam_check(want, host(pd[sl]), host(md[sl]), host(vd[sl]), host(pb[2 * off:2 * off + n])))
    if off == 0:
        gc = _adam_buffers((g,), n, 0)[0]
        o.scale_clip(gc[:n], gn, TC.ADAM_CLIP)
        settle(f"scale_clip n={n}", TC.exact(host(gc[:n]), TC.scale_clip_ref(g, gnorm, TC.ADAM_CLIP)))
        assert bool((gc[n:] == TC.SENT).all())


@pytest.mark.parametrize("n,npart", TC.GRAD_NORM_CASES)
def test_grad_norm_contract(n, npart):
    o = ops()
    x = TC.grad_norm_inputs(n)
    outs = []
    for _ in range(2):
        part, out = full((npart,), float("nan")), full((1,), float("nan"))
        o.grad_norm(dev(x), part, out)
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    settle(f"grad_norm n={n} npart={npart}", TC.grad_norm_check(x, npart, host(outs[0])[0]))


@pytest.mark.parametrize("n", TC.CAST_N)
def test_casts_contract(n):
    o = ops()
    x = torch.from_numpy(TC.cast_inputs(n))
    ob = full((n + 8,), TC.SENT, BF)
    o.cast_bf16(x.to(DEV), out=ob[:n])
    assert torch.equal(ob[:n].cpu(), x.to(BF)) and bool((ob[n:] == TC.SENT).all())
    of = full((n + 8,), TC.SENT)
    o.cast_f32(x.to(BF).to(DEV), out=of[:n])
    assert torch.equal(of[:n].cpu(), x.to(BF).float()) and bool((of[n:] == TC.SENT).all())
    print(f"RATIO casts n={n} exact")


def test_transpose_group_contract():
    o = ops()
    pairs, want = [], []
    for k, (rows, cols) in enumerate(TC.TRANSPOSE_SHAPES):
        src = dev(TC.transpose_inputs(k, rows, cols), BF)
        out = full((cols, rows + 2 * (k % 3)), TC.SENT, BF)
        pairs.append((src[:, :cols], out))
        want.append(src[:, :cols].t().contiguous())
    assert len(pairs) == 33                                     # two launches
    o.transpose_group_bf16(pairs)
    for (src, out), w in zip(pairs, want):
        rows = src.shape[0]
        assert torch.equal(out[:, :rows], w) and bool((out[:, rows:] == TC.SENT).all()), tuple(src.shape)
    print("RATIO transpose_group exact")

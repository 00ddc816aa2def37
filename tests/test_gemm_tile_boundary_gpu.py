"""The eight-phase NT GEMM (gemm8.hip) around an output-tile boundary: a finished tile is written out while the next tile's first
K-tiles are staged and accumulated, with counted waits only -- nothing in the epilogues may wait for the whole staging queue, and
nothing covers for a miscounted wait any more.  Small problems on tiny persistent grids (COMMU_GEMM8_GRID), so that every
workgroup crosses several tile boundaries: two K-tiles per tile (the write-out overlaps a tile that ends one K-tile later), an odd
K-tile count (the LDS buffer parity flips at every boundary), uneven tile counts per workgroup with the XCD map on (grid 8) and
off (grid 3), edge tiles between interior tiles.

Reference: the float64 product of the bf16 operands.  Bounds: those of tests/test_kernels_gpu.py for test_gemm_nt_eight_phase*
(relerr = max|a - b| / max|b|; bf16 outputs 1.2e-2: one or two bf16 roundings of O(1)-relative values).  The dropout mask is
compared bit for bit with ops.dropout_keep_mask (the hash must not move)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16_TOL = 1.2e-2      # (tests/test_kernels_gpu.py)
P, SEED = 0.1, 4711

#        M     N    K   grid
CASES = [(1024, 512, 128, 2),          # four tiles per workgroup, nk = 2
         (1024, 512, 192, 2),          # odd nk
         (1280, 768, 256, 8),          # XCD map on, 15 tiles on 8 workgroups
         (1280, 768, 256, 3),          # XCD map off, five tiles per workgroup
         (1064, 536, 128, 2)]          # edge tiles (M and N tails) between interior tiles
IDS = ["%dx%dx%d-g%d" % c for c in CASES]


def ops():
    from commu_amd import ops as o
    return o


def relerr(a, b):
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-12))


def operands(M, N, K, gen):
    bf = torch.bfloat16
    A = torch.randn(M, K, device=DEV, generator=gen).to(bf)
    B = torch.randn(N, K, device=DEV, generator=gen).to(bf)
    bias = torch.randn(N, device=DEV, generator=gen)
    resid = torch.randn(M, N, device=DEV, generator=gen).to(bf)
    return A, B, bias, resid, A.double() @ B.double().t()


def out_buf(M, N):          # NaN-filled, leading dimension a multiple of 8
    ld = (N + 7) // 8 * 8
    return torch.full((M, ld), float("nan"), device=DEV, dtype=torch.bfloat16)[:, :N]


def padded(x):
    M, N = x.shape
    t = torch.zeros(M, (N + 7) // 8 * 8, dtype=x.dtype, device=DEV)
    t[:, :N] = x
    return t[:, :N]


_KEEP = {}


def keep_mask(M, N):
    if (M, N) not in _KEEP:
        _KEEP[(M, N)] = ops().dropout_keep_mask(SEED, M * N, P, device=DEV).view(M, N)
    return _KEEP[(M, N)]


def check_forms(o, M, N, K, gen, forms):
    A, B, bias, resid, ref = operands(M, N, K, gen)
    keep = keep_mask(M, N)
    scale = 1.0 / (1.0 - int(P * 65536.0 + 0.5) / 65536.0)
    if "plain" in forms:
        out = o.gemm_nt(A, B, out=out_buf(M, N))
        assert relerr(out, ref) < BF16_TOL
    if "brd" in forms:          # bias + ReLU + dropout (pipelined write-out)
        act = torch.relu(ref + bias.double())
        out = o.gemm_nt(A, B, out=out_buf(M, N), bias=bias, relu=True, drop_p=P, drop_seed=SEED)
        assert relerr(out, act * keep * scale) < BF16_TOL
        assert bool((out[~keep] == 0).all())
        sure = keep & (act > 1e-2)
        assert bool((out[sure] != 0).all())
    if "resid" in forms:          # residual + dropout (burst write-out)
        rp = padded(resid)
        out = o.gemm_nt(A, B, out=out_buf(M, N), resid=rp, drop_p=P, drop_seed=SEED)
        assert relerr(out, ref * keep * scale + resid.double()) < BF16_TOL
        assert bool((out[~keep] == resid[~keep]).all())
        sure = keep & (ref.abs() > 0.5)
        assert bool((out[sure] != resid[sure]).all())
    return A, B, bias, ref, keep, scale


@pytest.mark.parametrize("M,N,K,grid", CASES, ids=IDS)
def test_tile_boundary_epilogues(M, N, K, grid, monkeypatch):
    o = ops()
    monkeypatch.setenv("COMMU_GEMM8_ALWAYS", "1")
    monkeypatch.setenv("COMMU_GEMM8_GRID", str(grid))
    gen = torch.Generator(device=DEV).manual_seed(1000 + K + grid)
    A, B, bias, ref, keep, scale = check_forms(o, M, N, K, gen, ("plain", "brd", "resid"))
    if M % 256 or N % 256:
        assert o.signbits_words(M, N, K) == 0          # (whole tiles only: the bf16 mask is the path for this shape)
        return
    # sign bits out (forward, bias + ReLU + dropout) and ReLU bits in (backward GEMM with the same M x N output)
    bits = torch.full((M * N // 32,), -1, device=DEV, dtype=torch.int32)
    hid = o.gemm_nt(A, B, out=out_buf(M, N), bias=bias, relu=True, drop_p=P, drop_seed=SEED, sign_bits_out=bits)
    act = torch.relu(ref + bias.double())
    assert relerr(hid, act * keep * scale) < BF16_TOL
    assert bool((hid[~keep] == 0).all()) and bool((hid[keep & (act > 1e-2)] != 0).all())
    K2 = K + 64
    G = torch.randn(M, K2, device=DEV, generator=gen).to(torch.bfloat16)
    W2t = torch.randn(N, K2, device=DEV, generator=gen).to(torch.bfloat16)
    got = o.gemm_nt(G, W2t, out=out_buf(M, N), relu_bits=bits, mask_scale=scale)
    full = (G.double() @ W2t.double().t()) * (hid > 0) * scale
    assert relerr(got, full) < BF16_TOL
    assert bool((got[~(hid > 0)] == 0).all())


@pytest.mark.parametrize("form", ["plain", "brd", "resid"])
@pytest.mark.parametrize("M,N,K,grid", CASES, ids=IDS)
def test_tile_boundary_race_screen(M, N, K, grid, form, monkeypatch):
    """50 launches with fresh random operands, every output compared: a wait that is one too wide shows as a rare wrong tile."""
    o = ops()
    monkeypatch.setenv("COMMU_GEMM8_ALWAYS", "1")
    monkeypatch.setenv("COMMU_GEMM8_GRID", str(grid))
    gen = torch.Generator(device=DEV).manual_seed(77 + K + grid)
    for _ in range(50):
        check_forms(o, M, N, K, gen, (form,))

"""The weight-only decode of block-scaled FP8 weights on the GPU: every finite code at every k of a block, lossless
operands bit for bit against the float64 chain at every edge of both kernel forms, one lit block, random data inside §39's bound,
non-finite values, guard bands, and the routes."""
import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _fp8dec_native as fn, synthetic
from tests import elementwise
from tests.guard import guarded_alloc                                   # noqa: F401  (fixture)
from tests.test_fp8_w8a8_host import code_of
from tests.test_gpu_fp8_w8a8 import DEV, DTYPES, bits, dev, same_bits

pytestmark = pytest.mark.gpu
B = fn.BLOCK
NAME = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
_BIAS = (None,) + DTYPES
f = bnb.linear_fp8_block_weight_only


def launch_of(M, N, K, dtype):
    if dtype != torch.float32 and M >= 2:
        return f"fp8_block_decode_mfma {NAME[dtype]} MT16 {M}x{N}x{K}"
    return f"fp8_block_decode {NAME[dtype]} MT{1 if M == 1 or dtype != torch.float32 else 2 if M == 2 else 4} {M}x{N}x{K}"


def chain(x, w, sW, bias=None):
    """(r, S) in float64: x [M, K] a tensor, w the codes and sW the block scales (numpy); r.to(dtype) is the chain rounded once"""
    N, K = w.shape
    scale = np.repeat(np.repeat(sW.astype(np.float64), B, axis=0)[:N], B, axis=1)[:, :K]
    with np.errstate(all="ignore"):
        Wd = torch.from_numpy(w).view(torch.float8_e4m3fn).to(torch.float64) * torch.from_numpy(scale)
        X, b = x.double().cpu(), torch.zeros(N, dtype=torch.float64) if bias is None else bias.double().cpu()
        return X @ Wd.T + b[None, :], X.abs() @ Wd.abs().T + b.abs()[None, :]


def exact_case(M, N, K, seed=0):
    """x in [-4, 4] and decoded w in [-8, 8], integers; sW[nb, t] a power of two 2^-2 .. 2^1 that differs between neighbours; an
    integer bias.  Every term is a multiple of 2^-2 and the sum of their magnitudes below 2^24 of that unit (asserted), so every
    partial, fold and sum is exact in f32 in ANY order, and float64 rounded once is the only right answer"""
    rng = np.random.default_rng(1000 * seed + M + 7 * N + 13 * K)
    x, w = rng.integers(-4, 5, (M, K)).astype(np.float32), rng.integers(-8, 9, (N, K))
    nb, t = np.meshgrid(np.arange(-(-N // B)), np.arange(-(-K // B)), indexing="ij")
    sW = (2.0 ** ((nb + 2 * t + seed) % 4 - 2)).astype(np.float32)
    bias = rng.integers(-4, 5, N).astype(np.float32)
    S = chain(torch.from_numpy(x), code_of(w), sW, torch.from_numpy(bias))[1].numpy()
    assert S.max() * 4 < 2.0 ** 24
    return torch.from_numpy(x), code_of(w), sW, torch.from_numpy(bias)


@pytest.mark.parametrize("dtype,by_row", [(torch.bfloat16, False), (torch.float16, False), (torch.bfloat16, True), (torch.float16, True), (torch.float32, False)],
                         ids=str)
def test_every_finite_code_at_every_k_decodes_exactly(dtype, by_row):
    """row r of w holds code (r + k) % 254 of the 254 finite codes at k; x is the identity: out[k, r] is that code's value, bit
    for bit, through the MFMA form (128 rows), the one-row form (row by row) and the f32-row form"""
    codes = np.array([c for c in range(256) if c & 0x7F != 0x7F], dtype=np.uint8)
    w = codes[(np.arange(254)[:, None] + np.arange(B)[None, :]) % 254]
    x, sW = torch.eye(B, dtype=dtype), np.ones((2, 1), dtype=np.float32)
    want = chain(x, w, sW)[0].to(dtype)
    assert want.abs().max() == 448 and want.abs()[want != 0].min() == 2.0 ** -9
    xd, wd, sd = x.to(DEV), dev(w), dev(sW)
    y = torch.stack([f(xd[k], wd, sd) for k in range(B)]) if by_row else f(xd, wd, sd)
    assert fn.last_launch() == launch_of(1 if by_row else B, 254, B, dtype)
    same_bits(y, want, f"decode {dtype} by_row={by_row}")


_MS, _NS, _KS = (1, 2, 15, 16, 17, 33), (1, 15, 16, 17, 127, 128, 129), (16, 112, 128, 144, 400, 1008, 1024, 1040, 2064)
EXACT_SHAPES = sorted({(M, N, K) for M in _MS for N, K in ((17, 400), (129, 1040))} | {(M, N, K) for N in _NS for M, K in ((1, 1040), (16, 144))}
                      | {(M, N, K) for K in _KS for M, N in ((1, 129), (17, 17))} | {(2, 16, 1040), (4, 129, 400)})


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("i", range(len(EXACT_SHAPES)), ids=lambda i: "%dx%dx%d" % EXACT_SHAPES[i])
def test_lossless_operands_bit_for_bit_across_every_edge(i, dtype):
    # every shape of the table in every row dtype; the output and bias dtypes (and no bias) rotate through the table
    shape = EXACT_SHAPES[i]
    x, w, sW, bias = exact_case(*shape)
    out_dtype, bias_dtype = DTYPES[(i + i // 7) % 3], _BIAS[(i + i // 5 + i // 20) % 4]
    b = None if bias_dtype is None else bias.to(bias_dtype)
    y = f(x.to(dtype).to(DEV), dev(w), dev(sW), None if b is None else b.to(DEV), out_dtype)
    assert fn.last_launch() == launch_of(*shape, dtype)
    same_bits(y, chain(x, w, sW, b)[0].to(out_dtype), f"{shape} {dtype} -> {out_dtype}, bias {bias_dtype}")


@pytest.mark.parametrize("t", (0, 1, 3))
def test_one_lit_block(t):
    """x is zero outside block t and sW differs in every block: a wrong scale index or a dropped partial block is a wrong power of two"""
    for M, dtype in ((1, torch.bfloat16), (3, torch.float16), (3, torch.float32)):
        x, w, sW, _ = exact_case(M, 130, 400, seed=7)
        sW = (2.0 ** (np.arange(4)[None, :] - 2 + np.arange(2)[:, None])).astype(np.float32)
        x = torch.where((torch.arange(400) // B == t)[None, :], x, torch.zeros(()))
        want = chain(x, w, sW)[0].float()
        assert want.abs().max() > 0
        same_bits(f(x.to(dtype).to(DEV), dev(w), dev(sW), None, torch.float32), want, f"lit block {t}, {M} rows of {dtype}")


@pytest.mark.parametrize("out_dtype", (torch.bfloat16, torch.float32), ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("M,N,K", [(5, 261, 1040), (16, 133, 2064)])
def test_random_data_inside_the_bound(M, N, K, dtype, out_dtype):
    """§39: g S + u_out (|r| + g S), g = (K + KB + 4) 2^-23: twice the any-order bound of K exact terms, KB folds, a scale product
    and the bias addition at 2^-24 each (the factor two: the MFMA's internal order); f32 rows add K 2^-24, their products round"""
    x = synthetic.normal((M, K), dtype, seed=71)
    wq, sW = (t.cpu().numpy() for t in bnb.quantize_fp8_blocks(synthetic.normal((N, K), torch.bfloat16, seed=72, std=0.02).to(DEV)))
    bias = synthetic.normal((N,), torch.bfloat16, seed=73, std=0.1)
    r, S = chain(x, wq, sW, bias)
    g = (K + -(-K // B) + 4) * 2.0 ** -23 + (K * 2.0 ** -24 if dtype == torch.float32 else 0.0)
    u_out = 0.0 if out_dtype == torch.float32 else elementwise.UNIT[out_dtype]
    y = f(x.to(DEV), dev(wq), dev(sW), bias.to(DEV), out_dtype).cpu()
    ratio = elementwise._compare(y, r, g * S + u_out * (r.abs() + g * S), *[torch.zeros(r.shape, dtype=torch.bool)] * 3, fn.last_launch(), "y = x . W^T + b")
    print(f"fp8 decode random {M}x{N}x{K} {dtype} -> {out_dtype}: worst err / bound = {ratio:.4f}")


@pytest.mark.parametrize("M,dtype", [(1, torch.bfloat16), (3, torch.float16), (3, torch.float32)], ids=str)
def test_non_finite_values_touch_their_row_or_their_block_columns_only(M, dtype):
    N, K, row = 136, 400, M // 2
    x, w, sW, _ = exact_case(M, N, K, seed=3)
    run = lambda x_, s_: f(x_.to(dtype).to(DEV), dev(w), dev(s_), None, torch.float32).cpu()      # noqa: E731
    clean = run(x, sW)
    assert torch.isfinite(clean).all()
    for k in (0, 127, 128, K - 1):
        for v in (float("inf"), float("-inf"), float("nan")):
            bad = x.clone()
            bad[row, k] = v
            y, want = run(bad, sW), chain(bad, w, sW)[0].float()          # numpy's IEEE chain: Inf x 0 is a NaN, Inf + finite an Inf
            assert torch.isnan(want[row]).any() and torch.equal(torch.isnan(y), torch.isnan(want)), (k, v)
            same_bits(torch.nan_to_num(y, nan=0.5), torch.nan_to_num(want, nan=0.5), f"{v} at k = {k}")
            assert torch.equal(bits(y[torch.arange(M) != row]), bits(clean[torch.arange(M) != row]))
    poisoned = sW.copy()
    poisoned[0, 1] = np.nan
    y = run(x, poisoned)
    assert torch.isnan(y[:, :B]).all() and torch.equal(bits(y[:, B:]), bits(clean[:, B:]))


@pytest.mark.parametrize("dtype", (torch.bfloat16, torch.float32), ids=str)
def test_outputs_stay_inside_their_buffer(guarded_alloc, dtype):      # noqa: F811
    # under both fills: the bands intact, and every output equal to the reference, so every byte of it was written
    shape = (17, 129, 400)
    x, w, sW, bias = exact_case(*shape, seed=5)
    for fill in (0xFF, 0x00):
        guarded_alloc.begin(fill, [("out", 0)], f"linear_fp8_block_weight_only {shape} {dtype}")
        y = f(x.to(dtype).to(DEV), dev(w), dev(sW), bias.to(DEV), torch.bfloat16)
        torch.cuda.synchronize()
        guarded_alloc.check()
        assert len(guarded_alloc.allocs) == 1 and fn.last_launch() == launch_of(*shape, dtype)
        same_bits(y, chain(x, w, sW, bias)[0].to(torch.bfloat16), f"{shape} fill {fill:#x}")


def test_the_routes_carry_the_same_bits():
    M, N, K = 12, 200, 400
    x = synthetic.normal((2, M // 2, 2 * K), torch.bfloat16, seed=81).to(DEV)[..., ::2]      # a view: not contiguous
    layer = bnb.LinearFP8Block.from_linear(torch.nn.Linear(K, N, dtype=torch.bfloat16), device=DEV)
    w, sW, bias = layer.weight, layer.weight_scale_inv, layer.bias
    one = f(x.contiguous().reshape(-1, K), w, sW, bias)
    assert fn.last_launch() == launch_of(M, N, K, torch.bfloat16)
    same_bits(f(x, w, sW, bias), one.reshape(2, M // 2, N), "a strided 3-D input")
    same_bits(f(x[0, 0], w, sW, bias), f(x[0, :1], w, sW, bias)[0], "a 1-D input")
    same_bits(f(x, w.view(torch.float8_e4m3fn), sW, bias), one.reshape(2, M // 2, N), "a float8_e4m3fn weight")
    layer.act_format = "none"
    same_bits(layer(x), one.reshape(2, M // 2, N), "LinearFP8Block act_format='none'")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = f(x, w, sW, bias)
    side.synchronize()
    same_bits(on_side, one.reshape(2, M // 2, N), "a side stream")
    xs, graph = x.contiguous(), torch.cuda.CUDAGraph()             # a captured graph, replayed after the input changed in place
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        captured = f(xs, w, sW, bias)
    for seed in (82, 83, 84):
        xs.copy_(synthetic.normal(tuple(xs.shape), torch.bfloat16, seed=seed))
        graph.replay()
        torch.cuda.synchronize()
        same_bits(captured, f(xs, w, sW, bias), f"graph replay {seed}")
    for call in (lambda: f(x, w[:, :-16], sW), lambda: f(x, w, sW[:, :-1]), lambda: f(x, w, sW, bias[:-1])):
        with pytest.raises(ValueError):
            call()

"""The W8A8 FP8 linear on the GPU: quantiser and GEMM bit for bit against tests/test_fp8_w8a8_host.py's restatement
and the float64 chain, the lane map, random data inside §37's bound, non-finite values, guard bands, and the routes."""
import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _fp8_native as fn, synthetic
from tests import elementwise, guard
from tests.guard import guarded_alloc                                   # noqa: F401  (fixture)
from tests.test_fp8_w8a8_host import EXACT_SHAPES, WIDE_CASES, code_of, decode, exact_case, quantize_rows

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
_BIAS = (None,) + DTYPES


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8)


def same_bits(y, want, what):
    assert y.dtype == want.dtype and y.shape == want.shape and torch.equal(bits(y), bits(want)), what


def chain(a, sA, w, sW, bias, dtype):             # the float64 chain over decoded codes, rounded once
    r = (torch.from_numpy(decode(a)) @ torch.from_numpy(decode(w)).T) * torch.from_numpy(sA.astype(np.float64))[:, None] * torch.from_numpy(sW.astype(np.float64))[None, :]
    return (r if bias is None else r + bias.double().cpu()[None, :]).to(dtype)


def _quantiser_rows(M, K, dtype):
    """Even rows: a maximum of 448 * 2^e, so r is a power of two and the scaled values sit ON every E4M3 mantissa midpoint and one
    ulp of `dtype` to either side.  Odd rows: the same times 1.37, so the roundings of 448 / amax, amax / 448 and x * r all count."""
    rng = np.random.default_rng(M * 100003 + K)
    mids = torch.tensor([(1 + (2 * m + 1) / 16) * 2.0 ** e for e in (-6, -1, 0, 7) for m in range(8)] + [2.0 ** -10 * (2 * m + 1) for m in range(8)],
                        dtype=torch.float64).to(dtype).double()
    ulp = mids * (2.0 ** -23 if dtype == torch.float32 else 2 * elementwise.UNIT[dtype])
    near = torch.cat([mids, mids + ulp, mids - ulp]).numpy()[:K - 1]
    x = rng.uniform(-0.5, 0.5, (M, K)) * 2.0 ** rng.integers(-12, 1, (M, K))
    x[:, 1:1 + len(near)] = near / 448.0 * np.where(np.arange(len(near)) % 2, -1, 1)
    x[:, 0] = 1.0
    return torch.from_numpy(x * (448.0 * 2.0 ** rng.integers(-6, 7, M) * np.where(np.arange(M) % 2, 1.37, 1.0))[:, None]).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("M,K", [(1, 16), (5, 48), (5, 4096), (5, 8192)])
def test_quantiser_is_the_restatement_bit_for_bit(M, K, dtype):
    x = _quantiser_rows(M, K, dtype)
    if M == 5:                                   # rows 3 (a generic maximum) and 4 stay as they are
        x[1], x[0, K // 2], x[2, K - 1] = 0, float("inf"), float("nan")
    want_q, want_s = quantize_rows(x.float().numpy())
    q, s = bnb.quantize_fp8_rows(x.to(DEV))
    assert not ((q.cpu() & 0x7F) == 0x7F).any() and fn.last_launch().startswith("fp8_quant_rows")
    assert torch.equal(q.cpu(), torch.from_numpy(want_q)), f"codes differ at {(q.cpu() != torch.from_numpy(want_q)).nonzero()[:4].tolist()}"
    same_bits(torch.nan_to_num(s, nan=-1.0), torch.nan_to_num(torch.from_numpy(want_s), nan=-1.0), "row scales")


def _run_exact(shape, out_dtype, bias_dtype):
    a, sA, w, sW, bias = exact_case(*shape)
    b = None if bias_dtype is None else torch.from_numpy(bias).to(bias_dtype).to(DEV)
    y = bnb.matmul_fp8_w8a8(dev(a), dev(sA), dev(w), dev(sW), b, out_dtype)
    same_bits(y, chain(a, sA, w, sW, b, out_dtype), f"{shape} -> {out_dtype}, bias {bias_dtype}: {fn.last_launch()}")
    return fn.last_launch()


@pytest.mark.parametrize("out_dtype", DTYPES, ids=str)
def test_exact_gemm_bit_for_bit_across_every_edge(out_dtype):
    # every (M, N, K) of the table; the bias dtypes (and none) rotate through it so that each meets every M, N and K
    for i, shape in enumerate(EXACT_SHAPES):
        for bias_dtype in (_BIAS[(i + i // 5 + i // 20) % 4], _BIAS[(i + i // 5 + i // 20 + 2) % 4]):
            assert _run_exact(shape, out_dtype, bias_dtype) == "gemm_fp8 256x128 %dx%dx%d" % shape


@pytest.mark.parametrize("M,N,K,out_dtype,bias_dtype", WIDE_CASES, ids=str)
def test_exact_gemm_on_the_wide_tile(M, N, K, out_dtype, bias_dtype):
    assert _run_exact((M, N, K), out_dtype, bias_dtype) == f"gemm_fp8 256x256 {M}x{N}x{K}"


def test_one_hot_activation_returns_the_decoded_weight():
    """activation row m is code 1.0 at k = m: out = dec(w)^T * sW; a misplaced half or 16-k chunk of the K-step moves a column"""
    K, N = 256, 40
    w = code_of(np.fromfunction(lambda n, k: ((3 * n + 5 * k) % 17 - 8) * 2.0 ** ((n + k // 16) % 3), (N, K)))
    sW = (2.0 ** (np.arange(N) % 4 - 1)).astype(np.float32)
    a = (np.eye(K) * 0x38).astype(np.uint8)
    y = bnb.matmul_fp8_w8a8(dev(a), dev(np.ones(K, dtype=np.float32)), dev(w), dev(sW), None, torch.float32)
    same_bits(y, torch.from_numpy((decode(w).T * sW[None, :]).astype(np.float32)), "lane map")


@pytest.mark.parametrize("M,N,K", [(33, 261, 1024), (300, 136, 272)])
@pytest.mark.parametrize("out_dtype", (torch.bfloat16, torch.float32), ids=str)
def test_random_data_inside_the_bound(M, N, K, out_dtype):
    """§37: g S + u_out (|r| + g S) with g = (K + 4) 2^-23: §25's (K + 2) 2^-23 of the sum, whose products are exact in f32, and
    2 * 2^-23 >= the three roundings of the epilogue (3 * 2^-24, and their cross terms)"""
    x, w = synthetic.normal((M, K), torch.bfloat16, seed=71), synthetic.normal((N, K), torch.bfloat16, seed=72, std=0.02)
    bias = synthetic.normal((N,), torch.bfloat16, seed=73, std=0.1)
    (xq, sA), (wq, sW) = quantize_rows(x.float().numpy()), quantize_rows(w.float().numpy())
    scale = torch.from_numpy(sA.astype(np.float64))[:, None] * torch.from_numpy(sW.astype(np.float64))[None, :]
    X, W = torch.from_numpy(decode(xq)), torch.from_numpy(decode(wq))
    r, S = (X @ W.T) * scale + bias.double(), (X.abs() @ W.abs().T) * scale + bias.double().abs()
    g, u_out = (K + 4) * 2.0 ** -23, 0.0 if out_dtype == torch.float32 else elementwise.UNIT[out_dtype]
    y = bnb.linear_fp8_w8a8(x.to(DEV), dev(wq), dev(sW), bias.to(DEV), out_dtype).cpu()
    ratio = elementwise._compare(y, r, g * S + u_out * (r.abs() + g * S), *[torch.zeros(r.shape, dtype=torch.bool)] * 3, fn.last_launch(), "y = Q(x) . W^T + b")
    print(f"fp8 w8a8 random {M}x{N}x{K} -> {out_dtype}: worst err / bound = {ratio:.4f}")


def test_non_finite_values_poison_exactly_their_row_or_column():
    M, N, K = 19, 36, 272
    a, sA, w, sW, bias = exact_case(M, N, K, seed=3)
    x = torch.from_numpy(np.where(np.arange(K) == 0, 8.0, decode(a))).to(torch.bfloat16)
    clean = bnb.linear_fp8_w8a8(x.to(DEV), dev(w), dev(sW), None, torch.float32).cpu()
    for k in (0, K // 2 + 3, K - 1):
        bad = x.clone()
        bad[4, k], bad[11, k] = float("inf"), float("nan")
        y = bnb.linear_fp8_w8a8(bad.to(DEV), dev(w), dev(sW), None, torch.float32).cpu()
        rows = (torch.arange(M) == 4) | (torch.arange(M) == 11)
        assert torch.isnan(y[rows]).all() and torch.equal(bits(y[~rows]), bits(clean[~rows])), k
    cols = torch.arange(N) == 7
    y = bnb.linear_fp8_w8a8(x.to(DEV), dev(w), dev(np.where(cols.numpy(), np.float32(np.nan), sW)), None, torch.float32).cpu()
    assert torch.isnan(y[:, cols]).all() and torch.equal(bits(y[:, ~cols]), bits(clean[:, ~cols]))


@pytest.mark.parametrize("shape", [(5, 7, 48), (257, 129, 144)], ids=str)
def test_outputs_and_workspace_stay_inside_their_buffers(guarded_alloc, shape):      # noqa: F811
    # under both fills: the bands intact, and q, sA and out equal to the reference, so every byte of them was written
    a, sA, w, sW, bias = exact_case(*shape, seed=5)
    x = torch.from_numpy(decode(a) * 7.0).to(torch.float16)              # integers; a row maximum of 56 makes both divisions exact
    x[:, 0] = 56.0
    want_q, want_s = quantize_rows(x.float().numpy())
    for fill in guard.FILLS:
        guarded_alloc.begin(fill, [("q", 0), ("sA", 0)], f"quantize_fp8_rows {shape}")
        q, s = bnb.quantize_fp8_rows(x.to(DEV))
        torch.cuda.synchronize()
        guarded_alloc.check()
        assert torch.equal(q.cpu(), torch.from_numpy(want_q)) and torch.equal(bits(s), bits(torch.from_numpy(want_s)))
        guarded_alloc.begin(fill, [("out", 0), ("workspace", 0)], f"linear_fp8_w8a8 {shape}")
        y = bnb.linear_fp8_w8a8(x.to(DEV), dev(w), dev(sW), dev(bias), torch.bfloat16)
        torch.cuda.synchronize()
        guarded_alloc.check()
        same_bits(y, chain(want_q, want_s, w, sW, torch.from_numpy(bias), torch.bfloat16), f"{shape} fill {fill:#x}")
        ws = guarded_alloc.allocs[1].view
        assert ws.numel() == fn.workspace_bytes(shape[0], shape[2]) and torch.equal(ws[:want_q.size].cpu(), torch.from_numpy(want_q).flatten())


def test_the_routes_carry_the_same_bits():
    M, N, K = 70, 200, 400
    x = synthetic.normal((2, M // 2, 2 * K), torch.bfloat16, seed=81).to(DEV)[..., ::2]      # a view: not contiguous
    layer = bnb.LinearFP8.from_linear(torch.nn.Linear(K, N, dtype=torch.bfloat16), device=DEV)
    w, sW, bias = layer.weight_fp8, layer.weight_scales, layer.bias.detach()
    with torch.no_grad():
        same_bits(layer(x), bnb.matmul_fp8_e4m3(x, w, sW, bias, torch.bfloat16), "LinearFP8 act_format='none': the present forward")
        q, sA = bnb.quantize_fp8_rows(x.reshape(-1, K))
        one = bnb.linear_fp8_w8a8(x, w, sW, bias)
        same_bits(one, bnb.matmul_fp8_w8a8(q, sA, w, sW, bias, torch.bfloat16).reshape(2, M // 2, N), "one call vs two")
        same_bits(bnb.linear_fp8_w8a8(x[0, 0], w, sW, bias), one[0, 0], "a 1-D input")
        layer.act_format = "fp8"
        same_bits(layer(x), one, "LinearFP8 act_format='fp8'")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = bnb.linear_fp8_w8a8(x, w, sW, bias)
        side.synchronize()
        same_bits(on_side, one, "a side stream")
        xs, graph = x.contiguous(), torch.cuda.CUDAGraph()             # a captured graph, replayed after the input changed in place
        torch.cuda.synchronize()
        with torch.cuda.graph(graph):
            captured = bnb.linear_fp8_w8a8(xs, w, sW, bias)
        for seed in (82, 83, 84):
            xs.copy_(synthetic.normal(tuple(xs.shape), torch.bfloat16, seed=seed))
            graph.replay()
            torch.cuda.synchronize()
            same_bits(captured, bnb.linear_fp8_w8a8(xs, w, sW, bias), f"graph replay {seed}")
    for call in (lambda: bnb.quantize_fp8_rows(x[0, :, :24]), lambda: bnb.linear_fp8_w8a8(x, w[:, :-16], sW),
                 lambda: bnb.matmul_fp8_w8a8(q, sA[:-1], w, sW), lambda: bnb.linear_fp8_w8a8(x, w, sW, bias[:-1])):
        with pytest.raises(ValueError):
            call()

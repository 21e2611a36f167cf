"""The block-scaled FP8 linear on the GPU: both quantisers bit for bit against tests/test_fp8_w8a8_host.py's
restatement applied per group and per block, the GEMM bit for bit against the float64 chain at every edge, one lit block, random data
inside §38's bound, non-finite values, guard bands, and the routes."""
import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _fp8blk_native as fn, synthetic
from tests import elementwise, guard
from tests.guard import guarded_alloc                                   # noqa: F401  (fixture)
from tests.test_fp8_w8a8_host import code_of, decode, quantize_rows
from tests.test_gpu_fp8_w8a8 import DEV, DTYPES, bits, dev, same_bits

pytestmark = pytest.mark.gpu
B = fn.BLOCK
_BIAS = (None,) + DTYPES


def exact_case(M, N, K, seed=0):
    """codes that decode to integers in [-8, 8], power-of-two scales 2^-2 .. 2^1 drawn per (m, t) and per (nb, t), a small integer
    bias: (a, sA [M, KB], w, sW [NB, KB], bias), numpy.  sum |a w| over a block is an integer below 2^24 and the scaled sum plus the
    bias a multiple of 2^-4 below 2^20: every partial, product and fold is exact in f32 in any order"""
    rng = np.random.default_rng(1000 * seed + M + 7 * N + 13 * K)
    a, w = rng.integers(-8, 9, (M, K)), rng.integers(-8, 9, (N, K))
    sA, sW = 2.0 ** rng.integers(-2, 2, (M, fn.blocks(K))), 2.0 ** rng.integers(-2, 2, (fn.blocks(N), fn.blocks(K)))
    bias = rng.integers(-4, 5, N).astype(np.float32)
    S = np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64).T
    assert S.max() < 2.0 ** 24 and S.max() * 4.0 + 4 < 2.0 ** 20 and min(sA.min(), sW.min()) >= 0.25 and max(sA.max(), sW.max()) <= 2
    return code_of(a), sA.astype(np.float32), code_of(w), sW.astype(np.float32), bias


def chain(a, sA, w, sW, bias, dtype):
    """(r, S) in float64 over the decoded codes, every term with its own scale product; r.to(dtype) is the chain rounded once"""
    K = a.shape[1]
    A = torch.from_numpy(decode(a) * np.repeat(sA.astype(np.float64), B, axis=1)[:, :K])
    W = torch.from_numpy(decode(w) * np.repeat(np.repeat(sW.astype(np.float64), B, axis=0)[:w.shape[0]], B, axis=1)[:, :K])
    b = torch.zeros(w.shape[0], dtype=torch.float64) if bias is None else bias.double().cpu()
    return (A @ W.T + b[None, :] if bias is not None else A @ W.T), A.abs() @ W.abs().T + b.abs()[None, :]


def groups_ref(x):                 # quantize_rows on every 128-wide slice of the rows: (codes [M, K], scales [M, KB])
    parts = [quantize_rows(x[:, k:k + B]) for k in range(0, x.shape[1], B)]
    return np.concatenate([p[0] for p in parts], axis=1), np.stack([p[1] for p in parts], axis=1)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("M,K", [(1, 16), (5, 144), (5, 400), (130, 272)])
def test_quantisers_are_the_restatement_bit_for_bit(M, K, dtype):
    rng = np.random.default_rng(M * 1009 + K)
    x = torch.from_numpy(rng.standard_normal((M, K)) * 2.0 ** rng.integers(-12, 5, (M, K)) * 2.0 ** rng.integers(-6, 5, (M, 1))).to(dtype)
    if M > 1:                      # a zero group in every row (a zero block), an Inf in the first group / block, a NaN in the ragged last
        x[:, B:2 * B], x[0, 0] = 0, float("inf")
        x[M - 1, K - 1] = float("nan")
    xn = x.float().numpy()
    blocks_q, blocks_s = np.zeros((M, K), dtype=np.uint8), np.zeros((fn.blocks(M), fn.blocks(K)), dtype=np.float32)
    for i in range(0, M, B):
        for k in range(0, K, B):
            q, s = quantize_rows(xn[i:i + B, k:k + B].reshape(1, -1))
            blocks_q[i:i + B, k:k + B], blocks_s[i // B, k // B] = q.reshape(xn[i:i + B, k:k + B].shape), s[0]
    for f, (want_q, want_s), launch in ((bnb.quantize_fp8_groups, groups_ref(xn), "fp8_quant_groups"), (bnb.quantize_fp8_blocks, (blocks_q, blocks_s), "fp8_quant_blocks")):
        q, s = f(x.to(DEV))
        assert not ((q.cpu() & 0x7F) == 0x7F).any() and fn.last_launch().startswith(launch)
        assert torch.equal(q.cpu(), torch.from_numpy(want_q)), f"{launch}: codes differ at {(q.cpu() != torch.from_numpy(want_q)).nonzero()[:4].tolist()}"
        same_bits(torch.nan_to_num(s, nan=-1.0), torch.nan_to_num(torch.from_numpy(want_s), nan=-1.0), launch + " scales")


EXACT_SHAPES = [(M, N, K) for M in (1, 255, 256, 257) for N in (1, 127, 128, 129, 257) for K in (16, 112, 128, 144, 400, 912)]


@pytest.mark.parametrize("out_dtype", DTYPES, ids=str)
def test_exact_gemm_bit_for_bit_across_every_edge(out_dtype):
    # every (M, N, K) of the table; the bias dtypes (and none) rotate through it so that each meets every M, N and K
    for i, shape in enumerate(EXACT_SHAPES):
        a, sA, w, sW, bias = exact_case(*shape)
        bias_dtype = _BIAS[(i + i // 6 + i // 30) % 4]
        b = None if bias_dtype is None else torch.from_numpy(bias).to(bias_dtype).to(DEV)
        y = bnb.matmul_fp8_block(dev(a), dev(sA), dev(w), dev(sW), b, out_dtype)
        assert fn.last_launch() == "gemm_fp8_block %dx%d %dx%dx%d" % (fn.TM, fn.TN, *shape)
        same_bits(y, chain(a, sA, w, sW, b, out_dtype)[0].to(out_dtype), f"{shape} -> {out_dtype}, bias {bias_dtype}")


@pytest.mark.parametrize("t", (0, 1, 3))
def test_one_lit_block(t):
    """every activation scale 0 but K-step t's: the output is exactly that block's contribution, so a fold one step early or late
    (which distinct random scales could mask by cancellation) shows"""
    a, sA, w, sW, bias = exact_case(33, 130, 400, seed=7)
    sA = np.where(np.arange(sA.shape[1])[None, :] == t, sA, np.float32(0.0))
    y = bnb.matmul_fp8_block(dev(a), dev(sA), dev(w), dev(sW), None, torch.float32)
    want = chain(a, sA, w, sW, None, torch.float32)[0]
    assert want.abs().max() > 0
    same_bits(y, want.float(), f"lit K-step {t}")


@pytest.mark.parametrize("M,N,K", [(33, 261, 1024), (300, 136, 272)])
@pytest.mark.parametrize("out_dtype", (torch.bfloat16, torch.float32), ids=str)
def test_random_data_inside_the_bound(M, N, K, out_dtype):
    """§38: g S + u_out (|r| + g S) with g = (min(K, 128) + 2 + (KB + 3) / 2) 2^-23: §25's (k + 2) 2^-23 of a 128-k MFMA sum, and
    KB + 2 roundings of 2^-24 (one per scale product, one per fold, the bias addition) with their cross terms; never above §37's"""
    x, w = synthetic.normal((M, K), torch.bfloat16, seed=71), synthetic.normal((N, K), torch.bfloat16, seed=72, std=0.02)
    bias = synthetic.normal((N,), torch.bfloat16, seed=73, std=0.1)
    xq, sA = groups_ref(x.float().numpy())
    wq, sW = (t.cpu().numpy() for t in bnb.quantize_fp8_blocks(w.to(DEV)))
    r, S = chain(xq, sA, wq, sW, bias, out_dtype)
    g, u_out = (min(K, B) + 2 + (fn.blocks(K) + 3) / 2) * 2.0 ** -23, 0.0 if out_dtype == torch.float32 else elementwise.UNIT[out_dtype]
    assert g <= (K + 4) * 2.0 ** -23
    y = bnb.linear_fp8_block(x.to(DEV), dev(wq), dev(sW), bias.to(DEV), out_dtype).cpu()
    ratio = elementwise._compare(y, r, g * S + u_out * (r.abs() + g * S), *[torch.zeros(r.shape, dtype=torch.bool)] * 3, fn.last_launch(), "y = Q(x) . W^T + b")
    print(f"fp8 block random {M}x{N}x{K} -> {out_dtype}: worst err / bound = {ratio:.4f}")


def test_non_finite_values_poison_exactly_their_row_or_block_columns():
    M, N, K = 19, 136, 272
    a, sA, w, sW, bias = exact_case(M, N, K, seed=3)
    x = torch.from_numpy(np.where(np.arange(K) % B == 0, 8.0, decode(a))).to(torch.bfloat16)
    clean = bnb.linear_fp8_block(x.to(DEV), dev(w), dev(sW), None, torch.float32).cpu()
    assert torch.isfinite(clean).all()
    for k in (0, K // 2 + 3, K - 1):
        bad = x.clone()
        bad[4, k], bad[11, k] = float("inf"), float("nan")
        y = bnb.linear_fp8_block(bad.to(DEV), dev(w), dev(sW), None, torch.float32).cpu()
        rows = (torch.arange(M) == 4) | (torch.arange(M) == 11)
        assert torch.isnan(y[rows]).all() and torch.equal(bits(y[~rows]), bits(clean[~rows])), k
    poisoned = sW.copy()
    poisoned[0, 1] = np.nan
    y = bnb.linear_fp8_block(x.to(DEV), dev(w), dev(poisoned), None, torch.float32).cpu()
    assert torch.isnan(y[:, :B]).all() and torch.equal(bits(y[:, B:]), bits(clean[:, B:]))


@pytest.mark.parametrize("shape", [(5, 7, 48), (257, 129, 144)], ids=str)
def test_outputs_scales_and_workspace_stay_inside_their_buffers(guarded_alloc, shape):      # noqa: F811
    # under both fills: the bands intact, and every output equal to the reference, so every byte of them was written
    a, sA, w, sW, bias = exact_case(*shape, seed=5)
    x = torch.from_numpy(decode(a) * 7.0).to(torch.float16)
    want_q, want_s = groups_ref(x.float().numpy())
    wsrc = torch.from_numpy(decode(w) * 3.0).to(torch.float16).to(DEV)
    for fill in guard.FILLS:
        guarded_alloc.begin(fill, [("q", 0), ("sA", 0)], f"quantize_fp8_groups {shape}")
        q, s = bnb.quantize_fp8_groups(x.to(DEV))
        torch.cuda.synchronize()
        guarded_alloc.check()
        assert torch.equal(q.cpu(), torch.from_numpy(want_q)) and torch.equal(bits(s), bits(torch.from_numpy(want_s)))
        guarded_alloc.begin(fill, [("q", 0), ("sW", 0)], f"quantize_fp8_blocks {shape}")
        bq, bs = bnb.quantize_fp8_blocks(wsrc)
        torch.cuda.synchronize()
        guarded_alloc.check()
        ref = [quantize_rows(wsrc.cpu().float().numpy()[i:i + B, k:k + B].reshape(1, -1)) for i in range(0, shape[1], B) for k in range(0, shape[2], B)]
        assert torch.equal(bits(bs).flatten(), bits(torch.from_numpy(np.concatenate([s_ for _, s_ in ref]))).flatten())
        assert torch.equal(bq.cpu()[:B, :B].flatten(), torch.from_numpy(ref[0][0]).flatten())
        guarded_alloc.begin(fill, [("out", 0), ("workspace", 0)], f"linear_fp8_block {shape}")
        y = bnb.linear_fp8_block(x.to(DEV), dev(w), dev(sW), dev(bias), torch.bfloat16)
        torch.cuda.synchronize()
        guarded_alloc.check()
        same_bits(y, chain(want_q, want_s, w, sW, torch.from_numpy(bias), torch.bfloat16)[0].to(torch.bfloat16), f"{shape} fill {fill:#x}")
        ws = guarded_alloc.allocs[1].view
        assert ws.numel() == fn.workspace_bytes(shape[0], shape[2]) and torch.equal(ws[:want_q.size].cpu(), torch.from_numpy(want_q).flatten())


def test_the_routes_carry_the_same_bits():
    M, N, K = 70, 200, 400
    x = synthetic.normal((2, M // 2, 2 * K), torch.bfloat16, seed=81).to(DEV)[..., ::2]      # a view: not contiguous
    layer = bnb.LinearFP8Block.from_linear(torch.nn.Linear(K, N, dtype=torch.bfloat16), device=DEV)
    w, sW, bias = layer.weight, layer.weight_scale_inv, layer.bias
    q, sA = bnb.quantize_fp8_groups(x.reshape(-1, K))
    one = bnb.linear_fp8_block(x, w, sW, bias)
    same_bits(one, bnb.matmul_fp8_block(q, sA, w, sW, bias, torch.bfloat16).reshape(2, M // 2, N), "one call vs two")
    same_bits(bnb.linear_fp8_block(x[0, 0], w, sW, bias), one[0, 0], "a 1-D input")
    same_bits(layer(x), one, "LinearFP8Block.from_linear")
    again = bnb.LinearFP8Block(K, N, bias=True, device=DEV)
    again.load_state_dict({k: v.view(torch.float8_e4m3fn) if k == "weight" else v for k, v in layer.state_dict().items()}, strict=True)
    same_bits(again(x), one, "the state dict through a float8_e4m3fn view")
    same_bits(bnb.linear_fp8_block(x, w.view(torch.float8_e4m3fn), sW, bias), one, "a float8_e4m3fn weight")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = bnb.linear_fp8_block(x, w, sW, bias)
    side.synchronize()
    same_bits(on_side, one, "a side stream")
    xs, graph = x.contiguous(), torch.cuda.CUDAGraph()             # a captured graph, replayed after the input changed in place
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        captured = bnb.linear_fp8_block(xs, w, sW, bias)
    for seed in (82, 83, 84):
        xs.copy_(synthetic.normal(tuple(xs.shape), torch.bfloat16, seed=seed))
        graph.replay()
        torch.cuda.synchronize()
        same_bits(captured, bnb.linear_fp8_block(xs, w, sW, bias), f"graph replay {seed}")
    for call in (lambda: bnb.quantize_fp8_groups(x[0, :, :24]), lambda: bnb.linear_fp8_block(x, w[:, :-16], sW),
                 lambda: bnb.matmul_fp8_block(q, sA[:-1], w, sW), lambda: bnb.linear_fp8_block(x, w, sW[:, :-1]), lambda: bnb.linear_fp8_block(x, w, sW, bias[:-1])):
        with pytest.raises(ValueError):
            call()

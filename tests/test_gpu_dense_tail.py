"""
k_gemm_dense's last k-steps: no LDS-DMA piece past the end of K, and the 16-bit epilogue under the last k-step (csrc/gemm_dense.h).

Every case goes through the public mbnb_gemm_dense (the C ABI behind functional.linear_dense; the tile selector in bits 8-15 of
`slices` picks the tile shape) on seeded `synthetic` operands.  Outputs and split-K workspaces are carved out of guard-banded
buffers whose every byte starts as 0xFF (tests/guard.py with the poison fill of tests/poison.py): an element no store reached is
a NaN, a store outside the buffer changes a band.  Each case checks
  * every element against the float64 product of the same 16-bit operands, within tests/elementwise.py's bound;
  * the guard bands;
  * torch.equal between the tile shapes of the same product (256 x 256, 256 x 128, and the 224 / 192 / 160-wide columns of the
    column-balanced grids -- the first two take the epilogue under the last k-step, the narrow ones the one behind the loop), and
    between a row computed alone and inside the larger M.
Shapes: 300 x 520 (ragged both ways, 2 x 3 tiles), 300 x 516 (N % 8 != 0: the scalar store path), 16 x 256; K = 128 .. 320, that
is 2 .. 5 k-steps -- both stage parities, and a slice at and above the two k-steps the tail needs; one k-step per slice is reached
with two slices at K = 128 (the ABI takes K >= 128 only: K = 64 is asserted to be refused).
"""
import pytest
import torch

from mps_bitsandbytes_amd import _native, synthetic
from tests.elementwise import assert_linear_elementwise
from tests.guard import GuardedTorch, guarded_alloc  # noqa: F401  (the fixture, by name)

pytestmark = pytest.mark.gpu

DEV = "cuda"
POISON = 0xFF
SHAPES = [(300, 520), (300, 516), (16, 256)]
KS = [128, 192, 256, 320]
DTS = {"bf16": torch.bfloat16, "f16": torch.float16}
# selector: tile code | wider columns first << 8 (codes 5 - 7: columns of 32 code, the first `wider` of 32 (code + 1))
TILES = {"256x256": 2, "256x128": 1, "224": 7 | (1 << 8), "192": 6 | (1 << 8), "160": 5}
_OPERANDS = {}


def _operands(M, N, K, dt):
    key = (M, N, K, dt)
    if key not in _OPERANDS:
        seed = 7000 + 13 * M + 7 * N + K
        _OPERANDS[key] = (synthetic.normal_device((M, K), dt, seed=seed), synthetic.normal_device((N, K), dt, seed=seed + 1, std=0.05),
                          synthetic.normal_device((N,), dt, seed=seed + 2))
    return _OPERANDS[key]


def _gemm(g, X, W, bias, odt, tile, slices=1, expect=0, out_offset=0):
    """One mbnb_gemm_dense call into a fresh poisoned, guard-banded output (and workspace); returns the output."""
    lib = _native.lib()
    (M, K), N = X.shape, W.shape[0]
    out = g.place_empty("out", (M, N), odt, DEV, offset=out_offset)
    ws = g.place_empty("workspace", (slices * M * N * 4,), torch.uint8, DEV) if slices > 1 else None
    code = _native.DTYPE_CODE[X.dtype]
    rc = lib.mbnb_gemm_dense(X.data_ptr(), W.data_ptr(), code, None if bias is None else bias.data_ptr(), _native.DTYPE_CODE[odt],
                             out.data_ptr(), M, N, K, K, None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel(),
                             slices | (tile << 8), _native.stream_ptr(DEV))
    assert rc == expect, (rc, lib.mbnb_last_error())
    return out


def _begin(where):
    g = GuardedTorch()
    g.begin(POISON, where=where)
    return g


@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("M,N", SHAPES)
def test_dense_tail_16bit(M, N, dt):
    dt_ = DTS[dt]
    for K in KS:
        X, W, b = _operands(M, N, K, dt_)
        for bias in (None, b):
            where = f"gemm_dense {M}x{N}x{K} {dt} bias={bias is not None}"
            g = _begin(where)
            outs = {name: _gemm(g, X, W, bias, dt_, sel) for name, sel in TILES.items()}
            name = _native.last_kernel()
            assert name.startswith("dense_nb "), name
            ratio = assert_linear_elementwise(outs["256x256"], X, W, bias, dt_, dt_, where)
            print(f"{where}: err / bound {ratio:.3f}")
            for tile, o in outs.items():
                assert torch.equal(o, outs["256x256"]), f"{where}: tile {tile} differs from 256x256"
            for r in (0, M - 1):    # a row alone (one k-step pipeline, rows 1 .. 255 of its tile past M) against the row inside M
                alone = _gemm(g, X[r:r + 1], W, bias, dt_, TILES["256x256"])
                assert torch.equal(alone[0], outs["256x256"][r]), f"{where}: row {r} alone differs from the row inside M = {M}"
            g.check()


@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("M,N", SHAPES)
def test_dense_tail_f32_output(M, N, dt):
    """f32 outputs keep the epilogue behind the loop: the 16-bit result, widened."""
    dt_, K = DTS[dt], 256
    X, W, b = _operands(M, N, K, dt_)
    for bias in (None, b):
        where = f"gemm_dense {M}x{N}x{K} {dt} -> f32 bias={bias is not None}"
        g = _begin(where)
        outs = {name: _gemm(g, X, W, bias, torch.float32, sel) for name, sel in TILES.items()}
        assert_linear_elementwise(outs["256x256"], X, W, bias, dt_, torch.float32, where)
        y16 = _gemm(g, X, W, bias, dt_, TILES["256x256"])
        assert torch.equal(outs["256x256"], y16.float()), f"{where}: the f32 output is not the 16-bit output widened"
        for tile, o in outs.items():
            assert torch.equal(o, outs["256x256"]), f"{where}: tile {tile} differs from 256x256"
        g.check()


@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("K", [128, 256])
@pytest.mark.parametrize("M,N", SHAPES)
def test_dense_tail_two_slices(M, N, K, dt):
    """Split-K partials: one (K = 128) and two (K = 256) k-steps per slice, f32 partials in a poisoned, guarded workspace."""
    dt_ = DTS[dt]
    X, W, b = _operands(M, N, K, dt_)
    for bias in (None, b):
        where = f"gemm_dense {M}x{N}x{K} {dt} two slices bias={bias is not None}"
        g = _begin(where)
        big = _gemm(g, X, W, bias, dt_, TILES["256x256"], slices=2)
        assert _native.last_kernel().startswith("dense"), _native.last_kernel()
        half = _gemm(g, X, W, bias, dt_, TILES["256x128"], slices=2)
        assert_linear_elementwise(big, X, W, bias, dt_, dt_, where)
        assert torch.equal(big, half), f"{where}: 256x128 tiles differ from 256x256"
        alone = _gemm(g, X[M - 1:M], W, bias, dt_, TILES["256x256"], slices=2)
        assert torch.equal(alone[0], big[M - 1]), f"{where}: the last row alone differs from the row inside M = {M}"
        g.check()


@pytest.mark.parametrize("dt", list(DTS))
@pytest.mark.parametrize("tile", ["256x256", "256x128"])
def test_dense_tail_unaligned_output_and_bias(tile, dt):
    """The tail's run-time fallbacks that the ABI does not refuse: an output 4 bytes off 16-byte alignment (the epilogue behind the
    loop, scalar stores) and a bias 4 bytes off 8-byte alignment (the tail with its bias fetched element by element): the bits of the
    aligned call, nothing outside the buffers."""
    dt_, (M, N, K) = DTS[dt], (300, 520, 192)
    X, W, b = _operands(M, N, K, dt_)
    where = f"gemm_dense {M}x{N}x{K} {dt} {tile} unaligned"
    g = _begin(where)
    want = _gemm(g, X, W, b, dt_, TILES[tile])
    assert_linear_elementwise(want, X, W, b, dt_, dt_, where)
    off_out = _gemm(g, X, W, b, dt_, TILES[tile], out_offset=4)
    assert off_out.data_ptr() % 16 == 4
    assert torch.equal(off_out, want), f"{where}: the output 4 bytes off alignment differs"
    b_off = g.place("bias", b, offset=4)
    assert b_off.data_ptr() % 8 == 4
    assert torch.equal(_gemm(g, X, W, b_off, dt_, TILES[tile]), want), f"{where}: the bias 4 bytes off alignment differs"
    assert torch.equal(_gemm(g, X, W, b_off, dt_, TILES[tile], out_offset=4), want), f"{where}: both off alignment differ"
    g.check()


def test_dense_k64_is_refused():
    """One k-step in an unsplit call would be K = 64; the ABI asks for K >= 128 (a slice of one k-step: test_dense_tail_two_slices)."""
    X, W, _ = _operands(16, 256, 128, torch.bfloat16)
    g = _begin("gemm_dense K=64")
    lib = _native.lib()
    out = g.place_empty("out", (16, 256), torch.bfloat16, DEV)
    code = _native.DTYPE_CODE[torch.bfloat16]
    rc = lib.mbnb_gemm_dense(X.data_ptr(), W.data_ptr(), code, None, code, out.data_ptr(), 16, 256, 64, 64, None, 0, 1 | (2 << 8),
                             _native.stream_ptr(DEV))
    assert rc == -2, rc
    torch.cuda.synchronize()
    assert bool((out.view(torch.uint8) == POISON).all())
    g.check()


def test_dense_tail_linear_dense(guarded_alloc):  # noqa: F811
    """functional.linear_dense (the library's own plan) on its guard-banded, poisoned output: the tiles the plan picks, same bits."""
    from mps_bitsandbytes_amd import functional as F
    M, N, K = 300, 520, 256
    for dt_ in DTS.values():
        X, W, b = _operands(M, N, K, dt_)
        guarded_alloc.begin(POISON, where=f"linear_dense {M}x{N}x{K} {dt_}")
        y = F.linear_dense(X, W, b)
        assert_linear_elementwise(y, X, W, b, dt_, dt_, _native.last_kernel())
        if int(_native.lib().mbnb_gemm_dense_workspace_bytes(M, N, K)) == 0:      # unsplit: the bits of every tile shape
            assert torch.equal(y, _gemm(guarded_alloc, X, W, b, dt_, TILES["256x256"]))
        guarded_alloc.check()


def test_dense_tail_int8_form(guarded_alloc):  # noqa: F811
    """k_gemm_dense<I8> (today's epilogue, no dead pieces; K = 256 int8 = two k-steps) through matmul_int8."""
    from tests.test_gpu_elementwise import _run_matmul_int8
    guarded_alloc.begin(POISON, where="matmul_int8 i8_dense")
    _run_matmul_int8(dict(op="matmul_int8", kernel="i8_transpose+dense", variant="i8_dense", M=24321, N=64, K=256, out="f16"))
    guarded_alloc.check()


def test_dense_tail_outlier_form(guarded_alloc):  # noqa: F811
    """k_gemm_dense<I8, OUTL> (the outlier epilogue behind the loop; two k-steps) through outlier_linear."""
    from tests.test_gpu_elementwise import _run_outlier
    guarded_alloc.begin(POISON, where="outlier_linear i8_dense+outliers")
    _run_outlier(dict(op="outlier_linear", kernel="i8_dense+outliers", variant="i8_dense OUTL1 NCH1", M=1536, N=4096, K=256, dt="f16",
                      n_out=32, bias=True))
    guarded_alloc.check()

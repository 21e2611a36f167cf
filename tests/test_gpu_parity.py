"""
GPU parity tests: the HIP path (through the C ABI, via the Python mirror of the reference API)
against (a) the golden vectors captured from the reference and (b) the CPU oracle on seeded
inputs.  Bit-exact for quantize / pack / dequantize / int8 quantization; Frobenius rel-err
tolerances (stated below) for the matmuls.  Run on the GPU box with `-m gpu`.
"""
import hashlib

import numpy as np
import pytest
import torch

import oracle
import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _native, synthetic
from mps_bitsandbytes_amd.functional import QuantState
from tests.goldenio import DT, bits_equal, from_bits, n_mismatch, rel_fro
from tests.poison import poisoned_alloc  # noqa: F401  (the fixture, by name: every torch.empty of functional.py comes back 0xFF)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_alloc")]

DEV = "cuda"

# Fused kernel vs oracle: identical B-operand bits, f32 accumulation, one rounding -> the two
# differ by summation order only.  Gates: BASELINE's hard tolerance is 1e-2;
# these are the tighter internal regression gates per compute dtype.
TOL = {torch.float16: 2e-4, torch.bfloat16: 2e-3, torch.float32: 2e-6}
HARD_TOL = 1e-2


def _state(absmax, shape, bs, qt, dtype, absmax2=None):
    st2 = None
    if absmax2 is not None:
        st2 = QuantState(absmax=absmax2.to(DEV), shape=torch.Size([absmax.numel()]), blocksize=256,
                         quant_type="int8", dtype=torch.float32)
    return QuantState(absmax=absmax.to(DEV), shape=torch.Size(shape), blocksize=bs, quant_type=qt, dtype=dtype,
                      state2=st2)


# --------------------------------------------------------------------------- golden G1 / G2
def _check_quant4_case(npz, key, case):
    dt = DT[case["dtype"]]
    x = from_bits(npz[key + "x"], dt).reshape(case["shape"])
    packed, st = bnb.quantize_4bit(x.to(DEV), blocksize=case["blocksize"], quant_type=case["quant_type"],
                                   compress_statistics=case["compress_statistics"])
    g_packed = from_bits(npz[key + "packed"])
    assert packed.dtype == torch.uint8 and packed.dim() == 1
    assert n_mismatch(packed.cpu(), g_packed) == 0, f"{key}: packed bytes differ"
    assert bits_equal(st.absmax.cpu(), from_bits(npz[key + "absmax"])), f"{key}: absmax differs"
    if case["compress_statistics"]:
        assert st.state2 is not None and st.absmax.dtype == torch.int8
        assert bits_equal(st.state2.absmax.cpu(), from_bits(npz[key + "absmax2"])), f"{key}: absmax2 differs"
    assert tuple(st.shape) == tuple(case["shape"]) and st.dtype == dt
    deq = bnb.dequantize_4bit(packed, st)
    g_deq = from_bits(npz[key + "deq"], dt).reshape(case["shape"])
    assert n_mismatch(deq.cpu(), g_deq) == 0, f"{key}: dequantized bits differ"


def test_g1_quantize_dequantize_bit_exact(golden):
    npz = golden.npz("g1_quant4.npz")
    for case in golden.manifest["g1"]:
        _check_quant4_case(npz, f"c{case['id']}_", case)


def test_g2_adversarial_bit_exact(golden):
    npz = golden.npz("g2_adversarial.npz")
    for case in golden.manifest["g2"]:
        _check_quant4_case(npz, case["id"] + "_", case)


# --------------------------------------------------------------------------- golden G3 (full BASELINE sizes)
def _sha(t):
    t = t.cpu().contiguous()
    if t.dtype in (torch.float16, torch.bfloat16):
        b = t.view(torch.int16).numpy().tobytes()
    elif t.dtype == torch.float32:
        b = t.view(torch.int32).numpy().tobytes()
    else:
        b = t.numpy().tobytes()
    return hashlib.sha256(b).hexdigest()


@pytest.mark.parametrize("name", ["A", "A_fp4", "B"])
def test_g3_full_size_digests(golden, name):
    """4096x4096 fp16 (configs[0] shape) and 11008x4096 bf16 + double quant: SHA-256 of the GPU
    outputs equals the digest of the reference's outputs."""
    g = golden.g3[name]
    x = synthetic.normal(g["shape"], DT[g["dtype"]], seed=g["seed"], std=g["std"])
    assert _sha(x) == g["input"]
    packed, st = bnb.quantize_4bit(x.to(DEV), blocksize=g["blocksize"], quant_type=g["quant_type"],
                                   compress_statistics=g["compress_statistics"])
    assert packed.numel() == g["packed_numel"] and st.absmax.numel() == g["absmax_numel"]
    assert _sha(packed) == g["packed"]
    assert _sha(st.absmax) == g["absmax"]
    if g["compress_statistics"]:
        assert _sha(st.state2.absmax) == g["absmax2"]
    assert _sha(bnb.dequantize_4bit(packed, st)) == g["deq"]


def test_g3_rowwise_digest(golden):
    g = golden.g3["A_rowwise"]
    x = synthetic.normal(g["shape"], DT[g["dtype"]], seed=g["seed"], std=g["std"])
    q, s = bnb.quantize_rowwise(x.to(DEV))
    assert _sha(q) == g["q"] and _sha(s) == g["scales"]
    assert _sha(bnb.dequantize_rowwise(q, s, torch.float16)) == g["deq"]


# --------------------------------------------------------------------------- golden G4 (matmul)
def test_g4_matmul_4bit_vs_reference_outputs(golden):
    npz = golden.npz("g4_matmul.npz")
    for c in golden.manifest["g4"]:
        key = f"c{c['id']}_"
        A = from_bits(npz[key + "A"], DT[c["a_dtype"]]).reshape(c["M"] + [c["K"]])
        packed = from_bits(npz[key + "packed"])
        absmax2 = from_bits(npz[key + "absmax2"]) if c["compress_statistics"] else None
        st = _state(from_bits(npz[key + "absmax"]), (c["N"], c["K"]), c["blocksize"], c["quant_type"],
                    DT[c["w_dtype"]], absmax2)
        bias = None if c["bias_dtype"] is None else from_bits(npz[key + "bias"], DT[c["bias_dtype"]]).to(DEV)
        cd = None if c["compute_dtype"] is None else DT[c["compute_dtype"]]
        out = bnb.matmul_4bit(A.to(DEV), packed.to(DEV), st, bias, cd)
        ref = from_bits(npz[key + "out"], DT[c["out_dtype"]]).reshape(c["M"] + [c["N"]])
        assert out.dtype == ref.dtype and tuple(out.shape) == tuple(ref.shape), key
        tol = max(TOL[DT[c["w_dtype"]]], TOL[ref.dtype])
        err = rel_fro(out, ref)
        assert err <= tol, f"{key}: rel-err {err:.3e} > {tol} ({_native.last_kernel()})"


# --------------------------------------------------------------------------- oracle parity, seeded
def _oracle_vs_gpu_matmul(M, N, K, dt, qt="nf4", bs=64, cs=False, bias=True, cd=None, seed=0, lead=None):
    W = synthetic.normal((N, K), dt, seed=seed)
    lead = lead or (M,)
    X = synthetic.normal(tuple(lead) + (K,), dt, seed=seed + 1)
    b = synthetic.normal((N,), dt, seed=seed + 2) if bias else None
    o_packed, o_absmax, o_st2 = oracle.quantize_4bit(W, bs, qt, cs)
    packed, st = bnb.quantize_4bit(W.to(DEV), blocksize=bs, quant_type=qt, compress_statistics=cs)
    assert torch.equal(packed.cpu(), o_packed)
    y = bnb.matmul_4bit(X.to(DEV), packed, st, None if b is None else b.to(DEV), cd)
    kern = _native.last_kernel()
    y_ref = oracle.matmul_4bit(X, o_packed, o_absmax, (N, K), bs, qt, dt, b, cd, o_st2)
    assert y.dtype == y_ref.dtype and tuple(y.shape) == tuple(y_ref.shape)
    err = rel_fro(y, y_ref)
    tol = max(TOL[dt], TOL[y.dtype])
    assert err <= tol, f"M={M} N={N} K={K} {dt} {qt} bs={bs} cs={cs}: rel-err {err:.3e} > {tol} ({kern})"
    return kern


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M", [1, 2, 3, 5, 8, 13, 16])
def test_matmul_gemv_path(M, dt):
    """Weight-streaming shapes: M = 1 -> wave-per-row GEMV; 2 <= M <= 32 -> skinny MFMA (16x16x32) kernel."""
    assert _oracle_vs_gpu_matmul(M, 512, 1024, dt, seed=10 + M) == ("gemv" if M == 1 else "skinny_mfma16")


@pytest.mark.parametrize("case", [
    dict(M=2, N=4096, K=4096, dt=torch.bfloat16), dict(M=7, N=1000, K=384, dt=torch.float16, qt="fp4", cs=True),
    dict(M=16, N=11008, K=4096, dt=torch.bfloat16, cs=True), dict(M=17, N=48, K=128, dt=torch.float16, bs=32),
    dict(M=28, N=4096, K=1024, dt=torch.float16, cd=torch.float32), dict(M=33, N=512, K=256, dt=torch.bfloat16),
    dict(M=28, N=4096, K=4096, dt=torch.bfloat16, bs=128), dict(M=32, N=4096, K=384, dt=torch.bfloat16),       # (29 rows and up with K % 256 == 0: k_gemm_small, round 3)
])
def test_matmul_skinny_path(case):
    """k_skinny4: 1, 2 and 4 activation tiles of 16 rows, ragged N, nested absmax, both code tables, 1-2 blocks per wave."""
    c = dict(case)
    assert _oracle_vs_gpu_matmul(c.pop("M"), c.pop("N"), c.pop("K"), c.pop("dt"), seed=27, **c) == "skinny_mfma16"


@pytest.mark.parametrize("case", [
    dict(M=256, N=4096, K=8192, dt=torch.bfloat16), dict(M=200, N=1000, K=4096, dt=torch.float16, cs=True, qt="fp4", bs=128),   # (round 3: 64-row tiles take
    dict(M=640, N=4096, K=2048, dt=torch.bfloat16, cd=torch.float32), dict(M=1024, N=2048, K=4096, dt=torch.float16),               # 256 x 4096^2 in ONE slice)
    dict(M=40, N=11008, K=4096, dt=torch.bfloat16, cs=True, bs=32),
])
def test_matmul_splitk_path(case, monkeypatch):
    """128 x 128 tiles with K split over a caller workspace (mbnb_matmul_4bit) and a deterministic slice reduction:
    M > 192 (384 for N >= 8192), or blocksize != 64 (the mid-sized-batch kernel takes the rest)."""
    monkeypatch.setattr(bnb.functional, "DECODE_ONCE", False)   # the fused split-K kernels (callers without the N x K scratch)
    c = dict(case)
    M, N, K = c["M"], c["N"], c["K"]
    want = "mfma_small_splitk" if (M <= 512 and K % 256 == 0 and K >= 512) else "mfma128_splitk"   # <= 512 rows: gemm_small.h
    assert _oracle_vs_gpu_matmul(c.pop("M"), c.pop("N"), c.pop("K"), c.pop("dt"), seed=28, **c) == want
    # run-to-run determinism (fixed slice order, no atomics)
    W = synthetic.normal((N, K), torch.bfloat16, seed=1, std=0.05).to(DEV)
    x = synthetic.normal((M, K), torch.bfloat16, seed=2).to(DEV)
    packed, st = bnb.quantize_nf4(W, blocksize=c.get("bs", 64))
    assert torch.equal(bnb.matmul_4bit(x, packed, st), bnb.matmul_4bit(x, packed, st))


@pytest.mark.parametrize("case", [
    dict(M=96, N=4096, K=4096, dt=torch.bfloat16, want="mfma_small_splitk"),                     # 64 n-tiles x 4 slices of 4 steps
    dict(M=128, N=4096, K=4096, dt=torch.float16, cs=True, want="mfma_small_splitk"),            # double-quantised absmax
    dict(M=190, N=1000, K=2048, dt=torch.float16, cs=True, qt="fp4", want="mfma_small_splitk"),  # three 64-row m-tiles x 4 slices, ragged M and N, FP4
    dict(M=133, N=777, K=2304, dt=torch.bfloat16, want="mfma_small_splitk"),                     # slices of 2 and 1 steps, odd M and N
    dict(M=100, N=4096, K=1280, dt=torch.bfloat16, want="mfma_small"),                           # 64-row tiles (round 3), 5 steps in one slice
    dict(M=190, N=1000, K=1024, dt=torch.float16, cs=True, qt="fp4", want="mfma_small"),         # 64-row tiles, one slice, ragged M and N, FP4
    dict(M=256, N=4096, K=4096, dt=torch.bfloat16, want="mfma_small"),                           # 256 workgroups x 16 steps, one slice
    dict(M=40, N=11008, K=4096, dt=torch.bfloat16, cs=True, want="mfma_small_splitk"),           # 64-row form (MF = 4), wide layer
    dict(M=64, N=4096, K=4096, dt=torch.bfloat16, want="mfma_small_splitk"),                     # 64-row form, full tile
    dict(M=256, N=1024, K=2048, dt=torch.float16, bias=False, want="mfma_small"),                # four full 64-row m-tiles, one 8-step slice
    dict(M=256, N=1024, K=8192, dt=torch.float16, bias=False, want="mfma_small_splitk"),         # two full 128-row m-tiles, 4-step slices
    dict(M=64, N=4096, K=4096, dt=torch.bfloat16, bs=128, cs=True, want="mfma_small_splitk"),    # blocksize 128, double-quantised absmax
    dict(M=150, N=520, K=2048, dt=torch.float16, bs=32, qt="fp4", want="mfma_small_splitk"),     # blocksize 32: one block per lane chunk
    dict(M=100, N=512, K=4096, dt=torch.bfloat16, bs=2048, want="mfma_small_splitk"),            # blocksize 2048: a block spans 8 steps
    dict(M=384, N=11008, K=4096, dt=torch.bfloat16, cd=torch.float32, want="mfma_small"),        # three m-tiles, f32 output (round 3: the 128-row form, one slice)
    dict(M=300, N=8192, K=256, dt=torch.float16, want="mfma_mid"),                               # 4 k-steps, no split (384 tiles), wide layer
    dict(M=65, N=64, K=256, dt=torch.bfloat16, bias=False, want="mfma_mid"),                     # one tile, K too short to split
])
def test_matmul_mid_batch_path(case, monkeypatch):
    """k_gemm_small (gemm_small.h): 32 < M <= 256 at blocksize 64 and K % 256 == 0 -- weights decoded from registers to
    registers, K split through the caller's workspace (row-major f32 partials, slices added in index order); k_gemm_mid
    (gemm_mid.h) for 256 < M <= 384 on wide layers and for K < 512."""
    monkeypatch.setattr(bnb.functional, "DECODE_ONCE", False)   # the fused mid-batch kernel (callers without the N x K scratch)
    c = dict(case)
    want = c.pop("want")
    M, N, K, dt = c.pop("M"), c.pop("N"), c.pop("K"), c.pop("dt")
    assert _oracle_vs_gpu_matmul(M, N, K, dt, seed=29, **c) == want
    W = synthetic.normal((N, K), dt, seed=3, std=0.05).to(DEV)
    x = synthetic.normal((M, K), dt, seed=4).to(DEV)
    packed, st = bnb.quantize_nf4(W)
    y = bnb.matmul_4bit(x, packed, st)
    assert torch.equal(y, bnb.matmul_4bit(x, packed, st)), "mid-batch kernel is not run-to-run deterministic"
    # without a workspace (plain C entry point semantics: no split) the same rows come out within the tolerance
    if M <= 128:
        yg = torch.cat([bnb.matmul_4bit(x[i:i + 1], packed, st) for i in range(0, M, max(1, M // 4))])
        assert rel_fro(y[::max(1, M // 4)], yg) <= TOL[dt]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", [(17, 128, 64), (64, 256, 512), (128, 128, 128), (200, 384, 1024),
                                   (256, 1024, 2048), (300, 200, 320), (129, 130, 136)])
def test_matmul_mfma_path(shape, dt):
    M, N, K = shape
    assert "mfma" in _oracle_vs_gpu_matmul(M, N, K, dt, seed=20 + M)


@pytest.mark.parametrize("case", [
    dict(M=2560, N=2560, K=256, dt=torch.bfloat16),
    dict(M=2500, N=2600, K=192, dt=torch.float16),                       # ragged M and N edges
    dict(M=2500, N=2600, K=128, dt=torch.bfloat16, qt="fp4", cs=True, bs=32),
    dict(M=3000, N=2304, K=384, dt=torch.float16, cs=True, bs=128, cd=torch.float32),
    dict(M=2304, N=3000, K=64, dt=torch.float16, cd=torch.bfloat16),      # single k-step
])
def test_matmul_mfma256_path(case, monkeypatch):
    """The fused 256x256 one-workgroup-per-CU kernel (dispatched for >= 96 tiles when the caller gives no N x K scratch)."""
    monkeypatch.setattr(bnb.functional, "DECODE_ONCE", False)
    c = dict(case)
    four = c.get("bs", 64) == 64 and c["K"] % 256 == 0     # blocksize 64, whole absmax-by-4 groups: k_gemm_fused4 (round 4), else k_gemm256p
    kern = _oracle_vs_gpu_matmul(c.pop("M"), c.pop("N"), c.pop("K"), c.pop("dt"), seed=25, **c)
    assert kern == ("mfma256f" if four else "mfma256")


@pytest.mark.parametrize("case", [
    dict(M=2560, N=2560, K=256, dt=torch.bfloat16),
    dict(M=2500, N=2600, K=192, dt=torch.float16),                       # ragged M and N edges: rows past M / N read as zeros
    dict(M=2500, N=2600, K=128, dt=torch.bfloat16, qt="fp4", cs=True, bs=32),
    dict(M=3000, N=2304, K=384, dt=torch.float16, cs=True, bs=128, cd=torch.float32),
    dict(M=2304, N=3000, K=192, dt=torch.float16, bs=128, cd=torch.bfloat16),   # K_weight = 256 > K: weight pitch != K
    dict(M=515, N=5000, K=640, dt=torch.bfloat16, bs=4096),              # one absmax block spans several rows' worth of k
    dict(M=1024, N=4096, K=1024, dt=torch.bfloat16, cs=True),            # split-K over f32 partials
    dict(M=768, N=4000, K=2048, dt=torch.float16, qt="fp4"),             # split-K, ragged N
    dict(M=700, N=3800, K=1088, dt=torch.bfloat16, cd=torch.float32),    # split-K with a short last slice, f32 output
    dict(M=640, N=4096, K=4096, dt=torch.bfloat16),                      # 128 x 128 tiles, 160 of them (512 rows and fewer: k_gemm_small, round 3)
    dict(M=257, N=11008, K=512, dt=torch.float16, cs=True),              # 256 x 128 tiles, ragged M (one row in the third tile)
    dict(M=640, N=2048, K=8192, dt=torch.bfloat16),                      # few tiles, long K (512 rows and fewer: k_gemm_small, round 3)
])
def test_matmul_decode_once_path(case, monkeypatch):
    """Large M through the Python API: dequantize_4bit into the scratch + k_gemm_dense (gemm_dense.h), any blocksize / code
    table / nested absmax.  Parity vs the oracle, and -- same B-operand bits, same f32 chain per output -- the unsplit path
    equals the fused 256 x 256 kernel bit for bit."""
    c = dict(case)
    M, N, K, dt = c.pop("M"), c.pop("N"), c.pop("K"), c.pop("dt")
    kern = _oracle_vs_gpu_matmul(M, N, K, dt, seed=25, **c)
    assert kern in ("dequant+dense", "dequant+dense_splitk"), kern
    W = synthetic.normal((N, K), dt, seed=25)
    X = synthetic.normal((M, K), dt, seed=26).to(DEV)
    b = synthetic.normal((N,), dt, seed=27).to(DEV)
    packed, st = bnb.quantize_4bit(W.to(DEV), blocksize=c.get("bs", 64), quant_type=c.get("qt", "nf4"), compress_statistics=c.get("cs", False))
    y = bnb.matmul_4bit(X, packed, st, b, c.get("cd"))
    assert _native.last_kernel() == kern
    assert torch.equal(y, bnb.matmul_4bit(X, packed, st, b, c.get("cd"))), "decode-once path is not run-to-run deterministic"
    monkeypatch.setattr(bnb.functional, "DECODE_ONCE", False)
    y_fused = bnb.matmul_4bit(X, packed, st, b, c.get("cd"))
    assert "dense" not in _native.last_kernel()
    if kern == "dequant+dense" and _native.last_kernel().startswith("mfma256"):
        assert torch.equal(y, y_fused), "dense and fused 256 x 256 kernels disagree"
    else:
        assert rel_fro(y, y_fused.cpu()) <= TOL[dt]


@pytest.mark.parametrize("case", [
    dict(M=600, N=512, K=224, want="dequant+dense_f32"),       # 64 x 64 tiles, ragged M, K too short to split
    dict(M=17, N=4096, K=4096, want="dequant+dense_f32_splitk"),   # the first row count of the path at this size: 64 tiles x 16 slices
    dict(M=300, N=1000, K=1028, cs=True, want="dequant+dense_f32_splitk"),   # ragged everything, K_weight = 1088 > K, nested absmax, short last slice
    dict(M=1203, N=96, K=336, qt="fp4", bs=16, cd=torch.float16),  # small blocksize, k tail (336 = 10 x 32 + 16), f16 output
    dict(M=2048, N=3072, K=512, bs=128, cd=torch.bfloat16, want="dequant+dense_f32"),   # 128 x 128 tiles (384 of them), bf16 output
    dict(M=2500, N=2100, K=260, bias=False, want="dequant+dense_f32"),   # 128 x 128 tiles, ragged, short last k step, no bias
    dict(M=1000, N=1000, K=1024, want="dequant+dense_f32_splitk"),        # 64 x 64 tiles, 4 slices
])
def test_matmul_f32_weight_decode_once_path(case, monkeypatch):
    """QuantState.dtype float32 (the weight of a default nn.Linear; functional.py:756-773 multiplies in f32): from 5 rows up
    dequantize_4bit (f32) into the scratch + k_gemm_f32 on v_mfma_f32_32x32x2_f32 (gemm_f32.hip) wherever that beats the generic
    kernel (from 17 rows at 4096^2, ~100 rows at 1024^2).  Parity vs the oracle at
    the f32 tolerance, run-to-run determinism, and agreement with the generic kernel it replaces."""
    c = dict(case)
    M, N, K, want = c.pop("M"), c.pop("N"), c.pop("K"), c.pop("want", None)
    kern = _oracle_vs_gpu_matmul(M, N, K, torch.float32, seed=61, **c)
    assert kern in ("dequant+dense_f32", "dequant+dense_f32_splitk") and (want is None or kern == want), kern
    W = synthetic.normal((N, K), torch.float32, seed=61)
    X = synthetic.normal((M, K), torch.float32, seed=62).to(DEV)
    packed, st = bnb.quantize_4bit(W.to(DEV), blocksize=c.get("bs", 64), quant_type=c.get("qt", "nf4"), compress_statistics=c.get("cs", False))
    y = bnb.matmul_4bit(X, packed, st, None, c.get("cd"))
    assert _native.last_kernel() == kern
    assert torch.equal(y, bnb.matmul_4bit(X, packed, st, None, c.get("cd")))
    monkeypatch.setattr(bnb.functional, "DECODE_ONCE", False)
    y_gen = bnb.matmul_4bit(X, packed, st, None, c.get("cd"))
    assert _native.last_kernel() == "generic"
    assert rel_fro(y, y_gen.cpu()) <= max(TOL[torch.float32], TOL[y.dtype])


def test_matmul_f32_weight_small_or_unaligned_stays_generic():
    assert _oracle_vs_gpu_matmul(4, 512, 1024, torch.float32, seed=63) == "generic"      # M <= 4: the packed weight streamed once
    assert _oracle_vs_gpu_matmul(16, 4096, 4096, torch.float32, seed=65) == "generic"    # two 8-row chunks: still cheaper than three launches
    assert _oracle_vs_gpu_matmul(40, 512, 256, torch.float32, seed=66) == "generic"      # small layer
    assert _oracle_vs_gpu_matmul(64, 256, 130, torch.float32, seed=64) == "generic"      # K % 4 != 0


@pytest.mark.parametrize("qt", ["nf4", "fp4"])
@pytest.mark.parametrize("cs", [False, True])
@pytest.mark.parametrize("bs", [32, 64, 128, 256])
def test_matmul_variants(qt, cs, bs):
    _oracle_vs_gpu_matmul(1, 256, 512, torch.float16, qt, bs, cs, seed=31)
    _oracle_vs_gpu_matmul(96, 256, 512, torch.bfloat16, qt, bs, cs, seed=32)


def test_matmul_generic_path_odd_shapes():
    """(M, N, K) of the reference's tests/test_edge_cases.py:254-277 and K not a multiple of 8."""
    for (M, N, K) in [(32, 63, 127), (32, 64, 65), (1, 17, 70), (3, 5, 7), (1, 1, 1)]:
        assert _oracle_vs_gpu_matmul(M, N, K, torch.float16, seed=40 + K) == "generic"
    # small blocksizes and fp32 weights also take the generic kernel
    assert _oracle_vs_gpu_matmul(4, 64, 128, torch.float16, bs=16, seed=47) == "generic"
    assert _oracle_vs_gpu_matmul(4, 64, 128, torch.float32, seed=48) == "generic"
    assert _oracle_vs_gpu_matmul(40, 64, 128, torch.float32, seed=49) == "generic"


def test_matmul_k_padded_fast_path():
    """K a multiple of 8 but not of the blocksize: K_weight > K (functional.py:219-221)."""
    assert _oracle_vs_gpu_matmul(1, 64, 96, torch.float16, seed=50) == "gemv"      # K_weight = 128
    assert _oracle_vs_gpu_matmul(2, 64, 4160, torch.float16, seed=52) == "gemv"    # ragged last k-step
    assert _oracle_vs_gpu_matmul(5, 64, 2080, torch.bfloat16, seed=53) == "gemv"
    assert _oracle_vs_gpu_matmul(1, 64, 72, torch.float16, seed=54) == "mfma128"   # K % 32 != 0: not the gemv
    assert "mfma" in _oracle_vs_gpu_matmul(64, 128, 200, torch.bfloat16, seed=51)


def test_matmul_mixed_dtypes_follow_weight_dtype():
    """bf16 activations on an fp16-origin weight compute in fp16 and are cast to bf16."""
    N, K, M = 128, 256, 48
    W = synthetic.normal((N, K), torch.float16, seed=60)
    X = synthetic.normal((M, K), torch.bfloat16, seed=61)
    packed, st = bnb.quantize_nf4(W.to(DEV))
    y = bnb.matmul_4bit(X.to(DEV), packed, st)
    assert y.dtype == torch.bfloat16
    op, oa, _ = oracle.quantize_4bit(W, 64, "nf4")
    y_ref = oracle.matmul_4bit(X, op, oa, (N, K), 64, "nf4", torch.float16, None, torch.bfloat16)
    assert rel_fro(y, y_ref) <= TOL[torch.bfloat16]
    y32 = bnb.matmul_4bit(X.to(DEV), packed, st, compute_dtype=torch.float32)
    assert y32.dtype == torch.float32


def test_matmul_batched_and_bias_dtypes():
    """[B,S,K] inputs (nn/linear4bit.py:106-117); fp32 / bf16 bias accepted and not ignored
    (tests/test_edge_cases.py:39-100)."""
    _oracle_vs_gpu_matmul(0, 128, 256, torch.float16, seed=70, lead=(2, 5))
    N, K = 64, 128
    W = synthetic.normal((N, K), torch.float16, seed=71)
    X = synthetic.normal((4, K), torch.float16, seed=72).to(DEV)
    packed, st = bnb.quantize_nf4(W.to(DEV))
    y0 = bnb.matmul_nf4(X, packed, st)
    for bdt in (torch.float32, torch.bfloat16, torch.float16):
        b = torch.full((N,), 100.0, dtype=bdt, device=DEV)
        y = bnb.matmul_nf4(X, packed, st, b)
        assert y.dtype == torch.float16
        assert torch.allclose((y.float() - y0.float()), torch.full_like(y0, 100.0).float(), atol=0.6)


def test_matmul_row_independence_and_linearity_full_size():
    """BASELINE metric shape (M=4096, 4096x4096 NF4, bf16 activations on fp16 weights is covered
    above; here fp16): size-independent properties.  (1) rows are independent: a 48-row sample of
    the full-size output equals the oracle run on just those rows; (2) exact linearity under a
    power-of-two scale; (3) the GEMV and MFMA kernels agree on the same rows."""
    N = K = 4096
    M = 4096
    W = synthetic.normal((N, K), torch.float16, seed=1234)
    packed, st = bnb.quantize_nf4(W.to(DEV))
    o_packed, o_absmax, _ = oracle.quantize_4bit(W, 64, "nf4")
    assert torch.equal(packed.cpu(), o_packed)
    X = synthetic.normal((M, K), torch.float16, seed=4321).to(DEV)
    Y = bnb.matmul_4bit(X, packed, st)
    assert _native.last_kernel() == "dequant+dense"
    assert torch.isfinite(Y).all()
    rows = torch.tensor(sorted(set(list(range(16)) + [int(v) for v in synthetic.uniform_u64(32, 9) % np.uint64(M)])))
    y_ref = oracle.matmul_4bit(X[rows.to(DEV)].cpu(), o_packed, o_absmax, (N, K), 64, "nf4", torch.float16)
    err = rel_fro(Y[rows.to(DEV)], y_ref)
    assert err <= TOL[torch.float16], f"full-size row sample rel-err {err:.3e}"
    assert err <= HARD_TOL
    # linearity: f(0.5 * X) == 0.5 * f(X) bit-for-bit away from fp16 subnormals
    Yh = bnb.matmul_4bit(X * 0.5, packed, st)
    big = Y.abs() > 1e-2
    assert torch.equal((Yh * 2)[big], Y[big])
    # the same rows through the other kernels: GEMV (1 row), skinny MFMA (4, 24 rows), k_gemm_small (96 rows: K split; 150, 240, 500 rows:
    # 16 steps of weights in registers, one K slice, round 3), decode once on 128 x 128 tiles (700)
    for rows_n, kern in ((1, "gemv"), (4, "skinny_mfma16"), (24, "skinny_mfma16"), (96, "mfma_small_splitk"), (150, "mfma_small"), (240, "mfma_small"), (500, "mfma_small"),
                         (700, "dequant+dense")):
        yg = bnb.matmul_4bit(X[:rows_n], packed, st)
        assert _native.last_kernel() == kern
        assert rel_fro(yg, Y[:rows_n]) <= TOL[torch.float16]
        if rows_n == 700:   # 128 x 128 tiles, unsplit (round 3): a row's summation order is that of the 256 x 256 tiles -> the same bits
            assert torch.equal(yg, Y[:rows_n])


def test_matmul_config_b_double_quant_full_size():
    """BASELINE configs[2]: 11008x4096 NF4 + double-quant absmax, bf16, M=4096 — row-sample parity."""
    N, K, M = 11008, 4096, 4096
    W = synthetic.normal((N, K), torch.bfloat16, seed=1235, std=0.02)
    packed, st = bnb.quantize_nf4(W.to(DEV), compress_statistics=True)
    op, oa, ost2 = oracle.quantize_4bit(W, 64, "nf4", True)
    assert torch.equal(packed.cpu(), op) and torch.equal(st.absmax.cpu(), oa)
    X = synthetic.normal((M, K), torch.bfloat16, seed=4322).to(DEV)
    Y = bnb.matmul_4bit(X, packed, st)
    assert Y.shape == (M, N) and Y.dtype == torch.bfloat16 and torch.isfinite(Y).all()
    rows = torch.arange(0, M, 128)
    y_ref = oracle.matmul_4bit(X[rows.to(DEV)].cpu(), op, oa, (N, K), 64, "nf4", torch.bfloat16, None, None, ost2)
    err = rel_fro(Y[rows.to(DEV)], y_ref)
    assert err <= TOL[torch.bfloat16], f"rel-err {err:.3e}"


# --------------------------------------------------------------------------- int8 paths
def test_g5_rowwise_and_blockwise_bit_exact(golden):
    npz = golden.npz("g5_int8.npz")
    for c in [c for c in golden.manifest["g5"] if c["kind"] == "rowwise"]:
        k = f"rw{c['id']}_"
        x = from_bits(npz[k + "x"], DT[c["dtype"]]).reshape(c["shape"])
        q, s = bnb.quantize_rowwise(x.to(DEV))
        assert n_mismatch(q.cpu(), from_bits(npz[k + "q"])) == 0 and bits_equal(s.cpu(), from_bits(npz[k + "s"]))
        for odt in ("f16", "bf16", "f32"):
            d = bnb.dequantize_rowwise(q, s, DT[odt])
            assert n_mismatch(d.cpu(), from_bits(npz[k + "deq_" + odt], DT[odt]).reshape(c["shape"])) == 0
    for k, dt in (("rwfill_", torch.float16), ("rwtie_", torch.float32), ("rwzero_", torch.float16)):
        x = from_bits(npz[k + "x"], dt)
        q, s = bnb.quantize_rowwise(x.to(DEV))
        assert n_mismatch(q.cpu(), from_bits(npz[k + "q"])) == 0, k
        assert bits_equal(s.cpu(), from_bits(npz[k + "s"])), k
    for c in [c for c in golden.manifest["g5"] if c["kind"] == "blockwise"]:
        k = f"bw{c['id']}_"
        x = from_bits(npz[k + "x"], DT[c["dtype"]])
        q, st = bnb.quantize_blockwise(x.to(DEV), blocksize=c["blocksize"], nested=c["nested"])
        assert n_mismatch(q.cpu(), from_bits(npz[k + "q"])) == 0, k
        assert bits_equal(st.absmax.cpu(), from_bits(npz[k + "absmax"])), k
        if c["nested"]:
            assert bits_equal(st.state2.absmax.cpu(), from_bits(npz[k + "absmax2"])), k
        d = bnb.dequantize_blockwise(q, st)
        assert n_mismatch(d.cpu(), from_bits(npz[k + "deq"], DT[c["dtype"]])) == 0, k


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("numel,bs", [(1 << 20, 4096), (1 << 20, 2048), (3 * 8192 + 5, 8192), (1 << 18, 64), (100 * 1000, 100),
                                      (1 << 16, 16384), (4096 * 24, 4096)])
def test_blockwise_sizes_and_kernel_forms_bit_exact(dt, numel, bs):
    """quantize_blockwise / dequantize_blockwise (functional.py:469-600) over whole blocks run on the row-wise kernels (same
    arithmetic: single-pass for 16-bit blocks of <= 8192 values, 16 values per thread on the way back), ragged tails and
    blocksizes that are no power of two on the scalar kernels: all equal the oracle bit for bit."""
    x = synthetic.normal((numel,), dt, seed=19 + bs % 97)
    oq, oa = oracle.quantize_blockwise(x, bs)
    q, st = bnb.quantize_blockwise(x.to(DEV), blocksize=bs)
    assert n_mismatch(q.cpu(), oq) == 0 and bits_equal(st.absmax.cpu(), oa)
    d = bnb.dequantize_blockwise(q, st)
    assert d.dtype == dt and n_mismatch(d.cpu(), oracle.dequantize_blockwise(oq, oa, bs, dt)) == 0


def test_g5_double_quant_bit_exact(golden):
    npz = golden.npz("g5_int8.npz")
    for c in [c for c in golden.manifest["g5"] if c["kind"] == "double_quant"]:
        k = f"dq{c['id']}_"
        x = from_bits(npz[k + "x"], DT[c["dtype"]]).reshape(c["shape"])
        oc, orow, cs, rs, outl = bnb.double_quant(x.to(DEV))
        assert outl is None
        assert n_mismatch(oc.cpu(), from_bits(npz[k + "out_col"])) == 0
        assert n_mismatch(orow.cpu(), from_bits(npz[k + "out_row"])) == 0
        assert bits_equal(cs.cpu(), from_bits(npz[k + "col_stats"])) and bits_equal(rs.cpu(), from_bits(npz[k + "row_stats"]))


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", [(1000, 2048), (37, 4104), (2051, 520), (64, 1001), (1, 8), (4096, 4096)])
def test_double_quant_vector_and_scalar_forms_bit_exact(dt, shape):
    """double_quant (functional.py:814-863): the vector form (cols % 8 == 0: one statistics pass with atomic maxima, one
    quantise pass) and the scalar form, with computed and with caller-supplied statistics: both int8 copies and both
    statistics equal the oracle's."""
    x = synthetic.normal(shape, dt, seed=53 + shape[1] % 89)
    x[0, 0] = 0.0
    want = oracle.double_quant(x)
    got = bnb.double_quant(x.to(DEV))
    assert n_mismatch(got[0].cpu(), want[0]) == 0 and n_mismatch(got[1].cpu(), want[1]) == 0
    assert bits_equal(got[2].cpu(), want[2]) and bits_equal(got[3].cpu(), want[3]) and got[4] is None
    cs = (synthetic.normal((shape[1],), torch.float32, seed=7).abs() + 0.25)
    rs = (synthetic.normal((shape[0],), torch.float32, seed=8).abs() + 0.25)
    for kw in (dict(col_stats=cs), dict(row_stats=rs), dict(col_stats=cs, row_stats=rs)):
        want = oracle.double_quant(x, **kw)
        got = bnb.double_quant(x.to(DEV), **{k: v.to(DEV) for k, v in kw.items()})
        assert n_mismatch(got[0].cpu(), want[0]) == 0 and n_mismatch(got[1].cpu(), want[1]) == 0, kw.keys()
        assert bits_equal(got[2].cpu(), want[2]) and bits_equal(got[3].cpu(), want[3]), kw.keys()


def test_g5_matmul_int8_and_linear8bit(golden):
    npz = golden.npz("g5_int8.npz")
    for c in [c for c in golden.manifest["g5"] if c["kind"] == "matmul_int8"]:
        k = f"mm{c['id']}_"
        out = bnb.matmul_int8(from_bits(npz[k + "A"]).to(DEV), from_bits(npz[k + "B"]).to(DEV),
                              from_bits(npz[k + "As"]).to(DEV), from_bits(npz[k + "Bs"]).to(DEV), DT[c["dtype"]])
        ref = from_bits(npz[k + "out"], DT[c["dtype"]]).reshape(c["M"], c["N"])
        # int32-exact contraction vs the reference's GEMM of dtype-rounded operands.  Measured on these goldens (exact
        # formula in f64 vs the reference's stored outputs): 3.7e-4 / 3.8e-4 (fp16), 3.17e-3 (bf16), 2.7e-7 (f32); the
        # regression gates are measured x 1.5, the hard budget (BASELINE) is 1e-2.
        tol = {"f16": 6e-4, "bf16": 4.8e-3, "f32": 4e-7}[c["dtype"]]
        err = rel_fro(out, ref)
        print(f"matmul_int8 golden {k} ({c['dtype']}): rel-err vs reference {err:.3e} (gate {tol:.1e}, budget {HARD_TOL:.0e})")
        assert err <= tol and err <= HARD_TOL, (k, err, _native.last_kernel())
    for c in [c for c in golden.manifest["g5"] if c["kind"] == "linear8bit"]:
        k = f"l8{c['id']}_"
        dt = DT[c["dtype"]]
        lin = torch.nn.Linear(c["K"], c["N"], bias=c["bias"]).to(dt)
        with torch.no_grad():
            lin.weight.copy_(from_bits(npz[k + "W"], dt).reshape(c["N"], c["K"]))
            if c["bias"]:
                lin.bias.copy_(from_bits(npz[k + "bias"], dt))
        l8 = bnb.Linear8bit.from_linear(lin.to(DEV))
        assert n_mismatch(l8.weight_int8.cpu(), from_bits(npz[k + "q"])) == 0
        assert bits_equal(l8.weight_scales.cpu(), from_bits(npz[k + "s"]))
        x = from_bits(npz[k + "x"], dt).reshape(c["M"] + [c["K"]])
        y = l8(x.to(DEV))
        ref = from_bits(npz[k + "y"], dt).reshape(c["M"] + [c["N"]])
        assert y.dtype == ref.dtype and tuple(y.shape) == tuple(ref.shape)
        assert rel_fro(y, ref) <= TOL[dt], (k, rel_fro(y, ref))


@pytest.mark.parametrize("shape", [(256, 256, 256), (200, 136, 320), (2500, 2600, 384), (2500, 2608, 384), (2560, 2560, 128),
                                   (2500, 2624, 384), (2560, 2560, 384), (4096, 4096, 4096)])
def test_matmul_int8_mfma_exact_vs_integer_reference(shape):
    """BASELINE configs[3] (4096^3) and smaller: the int8 MFMA contraction is exact in int32, so the
    f32 result must match torch's integer matmul formula to f32 rounding.  N % 16 == 0 and K % 128 == 0 with >= 96 tiles need
    no workspace: B is read where it lies ([K, N]) through ds_read_b64_tr_b8 -- from K = 256 up by the four-wave kernel
    (round 3, gemm_i8_inplace.h; equal bit for bit to the transposed k_gemm_dense<I8> path it replaced:
    profiles/r03_int8_inplace_ab.txt), at K = 128 by the 8-wave one; (2500, 2600, 384) takes the transposed path."""
    M, N, K = shape
    direct = K % 128 == 0 and N % 16 == 0 and ((M + 255) // 256) * ((N + 255) // 256) >= 96
    four = direct and K >= 256
    assert int(_native.lib().mbnb_matmul_int8_workspace_bytes(M, N, K)) == (0 if direct else N * K)
    A = synthetic.int8_tensor((M, K), seed=80).to(DEV)
    B = synthetic.int8_tensor((K, N), seed=81).to(DEV)
    sa = (synthetic.normal((M,), torch.float32, seed=82).abs() + 0.5).to(DEV)
    sb = (synthetic.normal((N,), torch.float32, seed=83).abs() + 0.5).to(DEV)
    out = bnb.matmul_int8(A, B, sa, sb, torch.float32)
    assert _native.last_kernel() == ("i8_inplace4" if four else "i8_mfma256" if (direct or M >= 2500) else "i8_mfma128")
    if four:    # run-to-run determinism, and the 16-bit epilogue against the f32 one (one more rounding)
        assert torch.equal(out, bnb.matmul_int8(A, B, sa, sb, torch.float32))
        assert torch.equal(bnb.matmul_int8(A, B, sa, sb, torch.bfloat16), out.to(torch.bfloat16))
    rows = torch.arange(0, M, max(1, M // 64), device=DEV)
    exact = (A[rows].double() @ B.double())  # exact: |sum| < 2^53
    ref = exact * (sa[rows].double() / 127.0).unsqueeze(1) * (sb.double() / 127.0).unsqueeze(0)
    assert rel_fro(out[rows], ref) <= 1e-6
    o16 = bnb.matmul_int8(A, B, sa, sb, torch.float16)
    y_ref = oracle.matmul_int8(A[rows].cpu(), B.cpu(), sa[rows].cpu(), sb.cpu(), torch.float16)
    finite = torch.isfinite(y_ref)
    assert rel_fro(torch.where(finite, o16[rows].cpu(), 0), torch.where(finite, y_ref, 0)) <= 1e-3


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", [(1, 128, 256), (4, 64, 70), (64, 256, 512), (300, 200, 320), (2500, 2600, 192)])
def test_linear_int8_vs_oracle(shape, dt):
    M, N, K = shape
    W = synthetic.normal((N, K), dt, seed=90, std=0.05)
    q, s = oracle.quantize_rowwise(W)
    x = synthetic.normal((M, K), dt, seed=91)
    b = synthetic.normal((N,), dt, seed=92)
    y = bnb.linear_int8(x.to(DEV), q.to(DEV), s.to(DEV), b.to(DEV))
    assert rel_fro(y, oracle.linear_int8(x, q, s, b)) <= TOL[dt], _native.last_kernel()


@pytest.mark.parametrize("M,N,K,dt,kern", [(2500, 2600, 192, torch.float16, "w8a16_dequant+dense"),
                                            (4096, 4096, 1024, torch.bfloat16, "w8a16_dequant+dense"),
                                            (1024, 4096, 2048, torch.bfloat16, "w8a16_dequant+dense"),       # 128 x 128 tiles (round 3)
                                            (512, 2048, 8192, torch.bfloat16, "w8a16_dequant+dense_splitk")])   # few tiles, long K: still split
def test_linear_int8_decode_once_path(M, N, K, dt, kern, monkeypatch):
    """Linear8bit.forward at large M: dequantize_rowwise into the workspace + k_gemm_dense; parity vs the oracle and equality
    with the fused W8A16 256 x 256 kernel (same B-operand bits) where that one serves the shape."""
    W = synthetic.normal((N, K), dt, seed=90, std=0.05)
    q, s = oracle.quantize_rowwise(W)
    x = synthetic.normal((M, K), dt, seed=91)
    b = synthetic.normal((N,), dt, seed=92)
    args = (x.to(DEV), q.to(DEV), s.to(DEV), b.to(DEV))
    y = bnb.linear_int8(*args)
    assert _native.last_kernel() == kern
    rows = torch.arange(0, M, max(1, M // 64))[:64]
    assert rel_fro(y.cpu()[rows], oracle.linear_int8(x[rows], q, s, b)) <= TOL[dt]
    # the weight the GEMM saw is dequantize_rowwise's, bit for bit
    wd = bnb.dequantize_rowwise(q.to(DEV), s.to(DEV), dt)
    assert torch.equal(wd.cpu(), oracle.dequantize_rowwise(q, s, dt))
    monkeypatch.setattr(bnb.functional, "DECODE_ONCE", False)
    yf = bnb.linear_int8(*args)
    if _native.last_kernel() == "w8a16_mfma256" and "splitk" not in kern:
        assert torch.equal(y, yf)
    else:
        assert rel_fro(y, yf.cpu()) <= TOL[dt]


@pytest.mark.parametrize("M,N,K,dt", [(2500, 2600, 192, torch.float16), (1024, 4096, 2048, torch.bfloat16), (64, 512, 256, torch.float16)])
def test_linear8bit_use_cache_keeps_the_dequantised_weight(M, N, K, dt):
    """VERDICT r2 (weak 9): with use_cache (the reference's default, nn/linear8bit.py:70-102) a large-batch forward keeps the
    dequantised weight and later calls run the dense GEMM alone -- same bits as the uncached forward (same slice plan); small
    batches stay on the fused W8A16 kernels and never fill the cache; clear_cache() drops it."""
    lin = torch.nn.Linear(K, N, bias=True)
    lin.weight.data.copy_(synthetic.normal((N, K), torch.float32, seed=95, std=0.05))
    lin.bias.data.copy_(synthetic.normal((N,), torch.float32, seed=96))
    cached = bnb.Linear8bit.from_linear(lin.to(dt).to(DEV), use_cache=True)
    plain = bnb.Linear8bit.from_linear(lin.to(dt).to(DEV), use_cache=False)
    x = synthetic.normal((M, K), dt, seed=97).to(DEV)
    y0 = plain(x)
    k_plain = _native.last_kernel()
    assert plain._weight_cache is None
    y1 = cached(x)
    large = bnb.functional.dense_path_applies(M, N, K)
    if large:
        assert k_plain.startswith("w8a16_dequant+dense")
        assert cached._weight_cache is not None and cached._weight_cache.dtype == dt
        wd = cached._weight_cache
        assert torch.equal(wd.cpu(), oracle.dequantize_rowwise(cached.weight_int8.cpu(), cached.weight_scales.cpu(), dt))
        y2 = cached(x)
        assert cached._weight_cache is wd, "the second call re-dequantised"
        assert torch.equal(y1, y0) and torch.equal(y2, y0)
        rows = torch.arange(0, M, max(1, M // 32))[:32]
        ref = oracle.linear_int8(x.cpu()[rows], cached.weight_int8.cpu(), cached.weight_scales.cpu(), cached.bias.detach().cpu())
        assert rel_fro(y1.cpu()[rows], ref) <= TOL[dt]
        cached.clear_cache()
        assert cached._weight_cache is None
    else:
        assert cached._weight_cache is None and torch.equal(y1, y0)


def test_linear8bit_cache_follows_the_weights():
    """a cached dequantised weight must not outlive the buffers it was made from -- after load_state_dict, an in-place
    copy_ into weight_int8 / weight_scales, or .to(), large-batch forwards (cache) and small-batch forwards (fused kernels) have
    to see the SAME weights."""
    M, N, K, dt = 512, 3072, 256, torch.float16
    assert bnb.functional.dense_path_applies(M, N, K)

    def make(seed):
        lin = torch.nn.Linear(K, N, bias=True)
        lin.weight.data.copy_(synthetic.normal((N, K), torch.float32, seed=seed, std=0.05))
        lin.bias.data.copy_(synthetic.normal((N,), torch.float32, seed=seed + 1))
        return bnb.Linear8bit.from_linear(lin.to(dt).to(DEV), use_cache=True)

    a, b = make(301), make(401)
    x = synthetic.normal((M, K), dt, seed=97).to(DEV)
    ya, yb = a(x), b(x)
    assert a._weight_cache is not None and not torch.equal(ya, yb)
    a.load_state_dict(b.state_dict())                       # same storage, new contents
    assert torch.equal(a(x), yb), "large-batch forward served the weights of before load_state_dict"
    assert torch.equal(a(x[:8]), b(x[:8]))
    a.weight_int8.copy_(make(301).weight_int8)              # in-place write: version counter
    a.weight_scales.copy_(make(301).weight_scales)
    a.bias.data.copy_(make(301).bias.data)
    assert torch.equal(a(x), ya), "large-batch forward served the weights of before copy_"
    wd = a._weight_cache
    assert torch.equal(a(x), ya) and a._weight_cache is wd, "an untouched layer keeps its cache"
    a = a.to(torch.device("cuda", 0))                       # _apply drops the cache even when nothing moves
    assert a._weight_cache is None and torch.equal(a(x), ya)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,N,K,ldw,slices,tile,odt", [(300, 520, 256, 256, 1, 0, None), (515, 1000, 640, 704, 2, 128, torch.float32),
                                                       (1024, 768, 2048, 2048, 4, 256, None), (129, 257, 128, 136, 1, 128, torch.float16)])
def test_gemm_dense_c_entry_point(M, N, K, ldw, slices, tile, odt, dt):
    """mbnb_gemm_dense through the C ABI: both tile shapes, split-K over a caller workspace, a weight pitch > K, ragged M / N,
    bias, output casts -- against a float64 product of the same 16-bit operands; and the tile shape does not change the bits."""
    import ctypes
    lib = _native.lib()
    odt = odt or dt
    X = synthetic.normal((M, K), dt, seed=301).to(DEV)
    Wfull = synthetic.normal((N, ldw), dt, seed=302, std=0.05).to(DEV)
    b = synthetic.normal((N,), dt, seed=303).to(DEV)
    ws = torch.empty(max(1, slices * M * N * 4), dtype=torch.uint8, device=DEV)
    code, ocode, sp = _native.DTYPE_CODE[dt], _native.DTYPE_CODE[odt], _native.stream_ptr(DEV)

    def run(tile_rows):
        out = torch.full((M, N), float("nan"), dtype=odt, device=DEV)
        rc = lib.mbnb_gemm_dense(X.data_ptr(), Wfull.data_ptr(), code, b.data_ptr(), ocode, out.data_ptr(), M, N, K, ldw, ws.data_ptr(),
                                 ws.numel(), slices | ((tile_rows // 128) << 8), sp)
        assert rc == 0, (rc, lib.mbnb_last_error())
        return out

    y = run(tile)
    ref = (X.double() @ Wfull[:, :K].double().t() + b.double())
    ref = ref.to(dt).to(odt) if odt != torch.float32 else ref.to(dt).float()       # one rounding to the weight dtype, then the cast
    assert torch.isfinite(y).all()
    assert rel_fro(y, ref.cpu()) <= TOL[dt]
    assert torch.equal(y, run(128)) and torch.equal(y, run(256)), "tile shape changed the result"


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("M,N,K,ldw,odt", [(1024, 4096, 1024, 1024, None), (515, 1000, 640, 704, torch.float32), (129, 257, 192, 200, torch.float16),
                                           (1000, 2600, 1024, 1024, None)])
def test_gemm_dense_128_tile_equals_the_256_tile(M, N, K, ldw, odt, dt):
    """k_gemm_dense128 (round 3: 128 x 128 tiles on three LDS stages, what the plan picks where the 256-wide tiles would leave CUs
    idle or split K) through mbnb_gemm_dense's tile code 3: bit-equal to the unsplit 256 x 256 tiles (same summation order per row),
    ragged M / N, a weight pitch > K, bias, output casts; and against a float64 product."""
    lib = _native.lib()
    odt = odt or dt
    X = synthetic.normal((M, K), dt, seed=311).to(DEV)
    Wfull = synthetic.normal((N, ldw), dt, seed=312, std=0.05).to(DEV)
    b = synthetic.normal((N,), dt, seed=313).to(DEV)
    code, ocode, sp = _native.DTYPE_CODE[dt], _native.DTYPE_CODE[odt], _native.stream_ptr(DEV)

    def run(tile_code, bias):
        out = torch.full((M, N), float("nan"), dtype=odt, device=DEV)
        rc = lib.mbnb_gemm_dense(X.data_ptr(), Wfull.data_ptr(), code, None if bias is None else bias.data_ptr(), ocode, out.data_ptr(), M, N, K, ldw,
                                 None, 0, 1 | (tile_code << 8), sp)
        assert rc == 0, (rc, lib.mbnb_last_error())
        return out

    for bias in (None, b):
        y128, y256 = run(3, bias), run(2, bias)
        assert torch.isfinite(y128).all()
        assert torch.equal(y128, y256)
    ref = (X.double() @ Wfull[:, :K].double().t() + b.double())
    ref = ref.to(dt).to(odt) if odt != torch.float32 else ref.to(dt).float()
    assert rel_fro(run(3, b), ref.cpu()) <= TOL[dt]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("rows,cols", [(37, 4096), (5, 48), (3, 50), (1000, 1008)])
def test_dequantize_rowwise_and_fp8_vector_and_scalar_forms_bit_exact(rows, cols, dt):
    """dequantize_rowwise / dequantize_fp8_e4m3: the 16-elements-per-thread form (cols % 16 == 0) and the scalar form give the
    oracle's bits."""
    W = synthetic.normal((rows, cols), torch.float32, seed=5 + rows, std=0.3)
    q, s = oracle.quantize_rowwise(W)
    assert torch.equal(bnb.dequantize_rowwise(q.to(DEV), s.to(DEV), dt).cpu(), oracle.dequantize_rowwise(q, s, dt))
    q8, s8 = oracle.quantize_fp8_e4m3(W)
    assert torch.equal(bnb.dequantize_fp8_e4m3(q8.to(DEV), s8.to(DEV), dt).cpu(), oracle.dequantize_fp8_e4m3(q8, s8, dt))


# --------------------------------------------------------------------------- modules
def test_linear4bit_module_matches_oracle_and_state_dict_roundtrip():
    torch.manual_seed(0)
    lin = torch.nn.Linear(256, 128, bias=True).half()
    with torch.no_grad():
        lin.weight.copy_(synthetic.normal((128, 256), torch.float16, seed=100, std=0.05))
        lin.bias.copy_(synthetic.normal((128,), torch.float16, seed=101))
    for cs in (False, True):
        l4 = bnb.Linear4bit.from_linear(lin.to(DEV), compress_statistics=cs)
        assert l4.weight.dtype == torch.uint8 and l4.weight.device.type == "cuda"
        x = synthetic.normal((2, 7, 256), torch.float16, seed=102).to(DEV)
        y = l4(x)
        assert y.shape == (2, 7, 128) and y.dtype == torch.float16
        op, oa, ost2 = oracle.quantize_4bit(lin.weight.data.cpu(), 64, "nf4", cs)
        y_ref = oracle.matmul_4bit(x.cpu(), op, oa, (128, 256), 64, "nf4", torch.float16, lin.bias.data.cpu(), None, ost2)
        assert rel_fro(y, y_ref) <= TOL[torch.float16]
        sd = l4.state_dict()
        assert sorted(sd.keys()) == ["bias", "weight", "weight_quant_state"]
        l4b = bnb.Linear4bit(256, 128, device=DEV, compress_statistics=cs)
        l4b.load_state_dict(sd)
        assert torch.equal(l4b(x), y)
        assert torch.equal(l4.dequantize(), bnb.dequantize_4bit(l4.weight, l4.weight_quant_state))
        # quantize-on-load from a full-precision state dict (nn/linear4bit.py:295-304)
        l4c = bnb.Linear4bit(256, 128, device=DEV, compress_statistics=cs)
        l4c.load_state_dict({k: v.to(DEV) for k, v in lin.state_dict().items()})
        assert torch.equal(l4c.weight, l4.weight)
        assert torch.equal(l4c(x), y)


def test_reference_envelope_tests():
    """The statistical envelopes the reference's own tests assert."""
    w = synthetic.normal((64, 128), torch.float16, seed=110).to(DEV)
    packed, st = bnb.quantize_nf4(w, blocksize=64)
    rec = bnb.dequantize_nf4(packed, st)
    assert ((w.float() - rec.float()).abs().mean() / w.float().std()).item() < 0.25      # tests/test_nf4.py:52-60
    z = torch.zeros(32, 64, dtype=torch.float16, device=DEV)
    pz, sz = bnb.quantize_nf4(z)
    assert bnb.dequantize_nf4(pz, sz).abs().max().item() == 0.0                          # tests/test_nf4.py:77-85
    c = torch.full((16, 64), 100.0, dtype=torch.float16, device=DEV)
    pc, sc = bnb.quantize_nf4(c)
    assert (bnb.dequantize_nf4(pc, sc).float() - 100.0).abs().max().item() < 10.0        # tests/test_nf4.py:87-99
    # fused vs unfused, M=128 K=N=4096 (tests/test_fused_nf4.py:10-31 compares the two implementations)
    W = synthetic.normal((4096, 4096), torch.float16, seed=111, std=0.02).to(DEV)
    X = synthetic.normal((128, 4096), torch.float16, seed=112).to(DEV)
    p, s = bnb.quantize_nf4(W)
    fused = bnb.matmul_4bit(X, p, s)
    unfused = torch.nn.functional.linear(X, bnb.dequantize_nf4(p, s))
    assert (fused.float() - unfused.float()).abs().max().item() < 0.1
    q, sc8 = bnb.quantize_rowwise(torch.full((8, 32), 0.5, dtype=torch.float16, device=DEV))
    assert (q == 127).all()                                                               # tests/test_advanced_linear.py:139-153


def test_quantize_model_replaces_linears_and_matches_layerwise_oracle():
    """integration.quantize_model: module-tree replacement with skip list, double quant wired."""
    torch.manual_seed(0)

    class MLP(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.up = torch.nn.Linear(128, 256)
            self.act = torch.nn.GELU()
            self.down = torch.nn.Linear(256, 64)
            self.lm_head = torch.nn.Linear(64, 32)

        def forward(self, x):
            return self.lm_head(self.down(self.act(self.up(x))))

    ref = MLP().half()
    cfg = bnb.BitsAndBytesConfig(load_in_4bit=True, bnb_4bit_use_double_quant=True)
    import copy
    qm = bnb.quantize_model(copy.deepcopy(ref), quantization_config=cfg, modules_to_not_convert=["lm_head"])
    assert isinstance(qm.up, bnb.Linear4bit) and isinstance(qm.down, bnb.Linear4bit) and isinstance(qm.lm_head, torch.nn.Linear)
    assert qm.up.weight_quant_state.state2 is not None and qm.up.weight.device.type == "cuda"
    x = synthetic.normal((5, 128), torch.float16, seed=200).to(DEV)
    y = qm(x)
    # layer-wise reference: oracle matmul for the quantized layers, torch for the rest
    h = x.cpu()
    for name in ("up", "down"):
        lin = getattr(ref, name)
        p, a, st2 = oracle.quantize_4bit(lin.weight.data, 64, "nf4", True)
        h = oracle.matmul_4bit(h, p, a, tuple(lin.weight.shape), 64, "nf4", torch.float16, lin.bias.data, None, st2)
        if name == "up":
            h = torch.nn.functional.gelu(h.float()).half()
    y_ref = torch.nn.functional.linear(h.float(), ref.lm_head.weight.float(), ref.lm_head.bias.float())
    assert rel_fro(y, y_ref) < 5e-3
    q8 = bnb.quantize_model(copy.deepcopy(ref), load_in_8bit=True)
    assert isinstance(q8.up, bnb.Linear8bit) and q8(x).shape == (5, 32)
    assert bnb.get_memory_footprint(qm)["quantized_params"] > 0


@pytest.mark.parametrize("M,N,K,dt,bias", [(1, 4096, 4096, torch.bfloat16, False), (7, 1000, 384, torch.float16, True),
                                            (16, 11008, 4096, torch.bfloat16, True), (33, 300, 256, torch.float16, False),
                                            (32, 4096, 1024, torch.bfloat16, True)])
def test_linear_int8_skinny_path(M, N, K, dt, bias):
    """Linear8bit.forward for 1 <= M <= 32 (<= 64 when K % 256 != 0): the int8 weight-streaming MFMA kernel (k_skinny8) vs the oracle."""
    W = synthetic.normal((N, K), dt, seed=61, std=0.05)
    q, s = oracle.quantize_rowwise(W)
    x = synthetic.normal((M, K), dt, seed=62)
    b = synthetic.normal((N,), dt, seed=63) if bias else None
    y = bnb.linear_int8(x.to(DEV), q.to(DEV), s.to(DEV), None if b is None else b.to(DEV))
    assert _native.last_kernel() == "w8a16_skinny"
    ref = oracle.linear_int8(x, q, s, b)
    assert rel_fro(y, ref) <= TOL[dt]


@pytest.mark.parametrize("M,N,K,dt,bias,kern", [(128, 4096, 4096, torch.bfloat16, True, "w8a16_small_splitk"),
                                                 (300, 1000, 1024, torch.float16, False, "w8a16_mfma128_splitk"),
                                                 (240, 2048, 2048, torch.bfloat16, True, "w8a16_small_splitk"),
                                                 (64, 4096, 1024, torch.float16, True, "w8a16_small"),
                                                 (40, 1000, 512, torch.bfloat16, False, "w8a16_small"),
                                                 (200, 520, 448, torch.float16, True, "w8a16_mfma128")])
def test_linear_int8_splitk_path(M, N, K, dt, bias, kern):
    """Linear8bit.forward for mid-sized M: 32 < M <= 256 with K % 256 == 0 -> k_gemm_small8 (weight operand decoded registers to
    registers, gemm_small8.h); otherwise 128 x 128 tiles; K split over a workspace (mbnb_linear_int8)."""
    W = synthetic.normal((N, K), dt, seed=71, std=0.05)
    q, s = oracle.quantize_rowwise(W)
    x = synthetic.normal((M, K), dt, seed=72)
    b = synthetic.normal((N,), dt, seed=73) if bias else None
    y = bnb.linear_int8(x.to(DEV), q.to(DEV), s.to(DEV), None if b is None else b.to(DEV))
    assert _native.last_kernel() == kern
    rows = torch.arange(0, M, max(1, M // 64))[:64]
    ref = oracle.linear_int8(x[rows], q, s, b)
    assert rel_fro(y.cpu()[rows], ref) <= TOL[dt]


def test_matmul_4bit_randomized_dispatch_sweep():
    """120 pseudo-random (M, N, K, blocksize, dtype, table, nested absmax, bias, compute dtype) cases against the oracle:
    every dispatch branch (gemv, skinny, 128^2, split-K, generic; 256^2 needs >= 96 tiles and the mid-batch kernel a
    K % 256 == 0 / blocksize 64 shape: both have their own tests) is hit with shapes nobody picked by hand."""
    rng = np.random.default_rng(20261004)
    seen = {}
    for case in range(120):
        M = int(rng.choice([1, 2, 3, 5, 8, 16, 17, 31, 33, 64, 65, 100, 129, 200, 257, 300, 513]))
        N = int(rng.choice([1, 7, 16, 31, 48, 64, 100, 128, 200, 256, 384, 513, 777, 1024]))
        K = int(rng.choice([8, 24, 32, 64, 72, 96, 128, 192, 256, 320, 384, 512, 640, 1024, 2048]))
        bs = int(rng.choice([16, 32, 64, 128, 256]))
        dt = [torch.float16, torch.bfloat16, torch.float32][int(rng.integers(0, 3))] if rng.random() < 0.2 else [torch.float16, torch.bfloat16][int(rng.integers(0, 2))]
        qt = "nf4" if rng.random() < 0.7 else "fp4"
        cs = bool(rng.random() < 0.35)
        bias = bool(rng.random() < 0.5)
        cd = None if rng.random() < 0.7 else [torch.float16, torch.bfloat16, torch.float32][int(rng.integers(0, 3))]
        kern = _oracle_vs_gpu_matmul(M, N, K, dt, qt=qt, bs=bs, cs=cs, bias=bias, cd=cd, seed=1000 + case)
        seen[kern] = seen.get(kern, 0) + 1
    assert {"gemv", "skinny_mfma16", "mfma128", "mfma128_splitk", "generic"} <= set(seen), seen


def test_matmul_4bit_randomized_sweep_round2_kernels():
    """48 pseudo-random shapes in the range of the round-2 kernels -- k_gemm_small (33 .. 384 rows), decode once + k_gemm_dense
    (both tile shapes, with and without split-K) -- with ragged M and N, every blocksize >= 32, both code tables, nested absmax,
    bias and output casts, against the oracle."""
    rng = np.random.default_rng(20261006)
    seen = {}
    for case in range(48):
        M = int(rng.choice([33, 40, 64, 65, 100, 128, 129, 200, 256, 257, 300, 384, 385, 500, 777, 1024, 1500, 2049]))
        N = int(rng.choice([64, 65, 100, 257, 520, 1000, 1024, 2600, 4096, 5001]))
        K = int(rng.choice([512, 768, 1024, 1280, 2048, 4096]))
        bs = int(rng.choice([32, 64, 64, 64, 128, 1024]))
        dt = [torch.float16, torch.bfloat16][int(rng.integers(0, 2))]
        qt = "nf4" if rng.random() < 0.7 else "fp4"
        cs = bool(rng.random() < 0.35)
        bias = bool(rng.random() < 0.5)
        cd = None if rng.random() < 0.7 else [torch.float16, torch.bfloat16, torch.float32][int(rng.integers(0, 3))]
        kern = _oracle_vs_gpu_matmul(M, N, K, dt, qt=qt, bs=bs, cs=cs, bias=bias, cd=cd, seed=5000 + case)
        seen[kern] = seen.get(kern, 0) + 1
    assert {"mfma_small_splitk", "mfma_small", "dequant+dense"} <= set(seen), seen     # (split-K of the dense path: test_matmul_decode_once_path, test_gemm_dense_c_entry_point)


def test_linear_int8_randomized_dispatch_sweep():
    """60 pseudo-random Linear8bit.forward shapes against the oracle (skinny, 128^2, split-K and generic paths)."""
    rng = np.random.default_rng(20261005)
    seen = {}
    for case in range(60):
        M = int(rng.choice([1, 2, 5, 16, 17, 33, 64, 65, 100, 129, 257, 300]))
        N = int(rng.choice([1, 7, 16, 48, 100, 128, 200, 384, 513, 1024]))
        K = int(rng.choice([8, 16, 24, 64, 72, 128, 192, 256, 384, 512, 1024, 2048]))
        dt = [torch.float16, torch.bfloat16][int(rng.integers(0, 2))]
        W = synthetic.normal((N, K), dt, seed=2000 + case, std=0.05)
        q, s = oracle.quantize_rowwise(W)
        x = synthetic.normal((M, K), dt, seed=3000 + case)
        b = synthetic.normal((N,), dt, seed=4000 + case) if rng.random() < 0.5 else None
        y = bnb.linear_int8(x.to(DEV), q.to(DEV), s.to(DEV), None if b is None else b.to(DEV))
        kern = _native.last_kernel()
        seen[kern] = seen.get(kern, 0) + 1
        err = rel_fro(y, oracle.linear_int8(x, q, s, b))
        assert err <= TOL[dt], f"case {case}: M={M} N={N} K={K} {dt} ({kern}): {err:.3e}"
    assert {"w8a16_skinny", "w8a16_mfma128", "w8a16_generic"} <= set(seen), seen



# --------------------------------------------------------------------------- round-2 additions: benched instantiation, config[4]
def test_matmul_benched_instantiation_bf16_plain_full_size():
    """The exact instantiation bench.py times (BASELINE metric): dequantize_4bit into the scratch + k_gemm_dense<bf16> at
    M = N = K = 4096, plain f32 absmax -- 64 k-steps, 32 rotations of the stage parity (the K = 256 cases above see two).  Row-sample parity vs the oracle: one row in every 256-row tile at a
    different in-tile position, the first rows, the last rows, and random ones; every column of those rows."""
    N = K = M = 4096
    W = synthetic.normal((N, K), torch.bfloat16, seed=1234)
    packed, st = bnb.quantize_nf4(W.to(DEV))
    op, oa, _ = oracle.quantize_4bit(W, 64, "nf4")
    assert torch.equal(packed.cpu(), op) and torch.equal(st.absmax.cpu(), oa)
    X = synthetic.normal((M, K), torch.bfloat16, seed=4321).to(DEV)
    Y = bnb.matmul_4bit(X, packed, st)
    assert _native.last_kernel() == "dequant+dense"
    assert Y.dtype == torch.bfloat16 and torch.isfinite(Y).all()
    # the fused kernel (what a caller without the N x K scratch gets) computes the same bits
    bnb.functional.DECODE_ONCE = False
    try:
        Yf = bnb.matmul_4bit(X, packed, st)
        assert _native.last_kernel() == "mfma256f"
    finally:
        bnb.functional.DECODE_ONCE = True
    assert torch.equal(Y, Yf), "k_gemm_dense and k_gemm_fused4 disagree at 4096^3"
    rows = sorted(set([t * 256 + (37 * t + 5) % 256 for t in range(16)] + list(range(8)) + [M - 1, M - 2, M - 33] +
                      [int(v) for v in synthetic.uniform_u64(24, 19) % np.uint64(M)]))
    rows_t = torch.tensor(rows)
    y_ref = oracle.matmul_4bit(X[rows_t.to(DEV)].cpu(), op, oa, (N, K), 64, "nf4", torch.bfloat16)
    err = rel_fro(Y[rows_t.to(DEV)], y_ref)
    assert err <= TOL[torch.bfloat16], f"benched instantiation: row-sample rel-err {err:.3e}"
    # element-wise as well: no single output may be off by more than a few bf16 ulps of the row scale
    diff = (Y[rows_t.to(DEV)].float().cpu() - y_ref.float()).abs().max().item()
    assert diff <= 4e-2 * y_ref.float().abs().max().item()
    assert torch.equal(Y, bnb.matmul_4bit(X, packed, st)), "the benched path is not run-to-run deterministic"
    # bias through the LDS-staged epilogue of the same instantiation
    bias = synthetic.normal((N,), torch.bfloat16, seed=77)
    Yb = bnb.matmul_4bit(X, packed, st, bias.to(DEV))
    yb_ref = oracle.matmul_4bit(X[rows_t.to(DEV)].cpu(), op, oa, (N, K), 64, "nf4", torch.bfloat16, bias)
    assert rel_fro(Yb[rows_t.to(DEV)], yb_ref) <= TOL[torch.bfloat16]


def test_matmul_config4_global_shape_on_one_gpu():
    """BASELINE configs[4]: global batch M = 32768 on the 4096 x 4096 NF4 weight (bf16).  On one GPU the whole batch is
    one launch of 128 x 16 tiles (64-bit row offsets, 2048 workgroups = 8 per CU); row-sample parity vs the oracle, and
    each of the 8 row shards computed on its own equals its slice of the unsharded result bit for bit (what the 8-way
    sharded run gathers)."""
    from mps_bitsandbytes_amd.sharding import row_shard
    M, N, K = 32768, 4096, 4096
    W = synthetic.normal((N, K), torch.bfloat16, seed=1234)
    packed, st = bnb.quantize_nf4(W.to(DEV))
    op, oa, _ = oracle.quantize_4bit(W, 64, "nf4")
    g = torch.Generator(device=DEV)
    g.manual_seed(99)
    X = torch.randn(M, K, generator=g, device=DEV, dtype=torch.float32).to(torch.bfloat16)
    Y = bnb.matmul_4bit(X, packed, st)
    assert _native.last_kernel() == "dequant+dense" and Y.shape == (M, N)
    assert torch.isfinite(Y).all()
    rows = sorted(set([t * 2048 + (611 * t + 3) % 2048 for t in range(16)] + [0, 1, 255, 256, M - 257, M - 256, M - 1] +
                      [int(v) for v in synthetic.uniform_u64(16, 23) % np.uint64(M)]))
    rows_t = torch.tensor(rows)
    y_ref = oracle.matmul_4bit(X[rows_t.to(DEV)].cpu(), op, oa, (N, K), 64, "nf4", torch.bfloat16)
    err = rel_fro(Y[rows_t.to(DEV)], y_ref)
    assert err <= TOL[torch.bfloat16], f"M=32768 row-sample rel-err {err:.3e}"
    for r in range(8):
        s, e = row_shard(M, r, 8)
        assert torch.equal(bnb.matmul_4bit(X[s:e], packed, st), Y[s:e]), f"shard {r} differs from the unsharded result"


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs")
def test_second_device_from_the_same_process():
    """One process, two devices: every kernel family that raises its dynamic-LDS limit (a per-device function attribute)
    is first used on cuda:0 and then on cuda:1 -- results must match bit for bit (SURVEY 8b threading / streams)."""
    d0, d1 = torch.device("cuda:0"), torch.device("cuda:1")
    W = synthetic.normal((2560, 512), torch.bfloat16, seed=5)
    for M in (1, 24, 200, 2560):        # gemv, skinny, 128^2 (+ split-K), 256^2
        X = synthetic.normal((M, 512), torch.bfloat16, seed=6 + M)
        outs, kerns = [], []
        for d in (d0, d1):
            packed, st = bnb.quantize_nf4(W.to(d))
            outs.append(bnb.matmul_4bit(X.to(d), packed, st).cpu())
            kerns.append(_native.last_kernel())
        assert kerns[0] == kerns[1]
        assert torch.equal(outs[0], outs[1]), f"M={M} ({kerns[0]}): cuda:1 differs from cuda:0"
    A = torch.randint(-127, 128, (2560, 512), dtype=torch.int8)
    B = torch.randint(-127, 128, (512, 2560), dtype=torch.int8)
    sa, sb = torch.rand(2560) + 0.5, torch.rand(2560) + 0.5
    o = [bnb.matmul_int8(A.to(d), B.to(d), sa.to(d), sb.to(d), torch.float16).cpu() for d in (d0, d1)]
    assert torch.equal(o[0], o[1])


def test_bench_gpus_flag_spawns_ranks_and_gathers_the_unsharded_result():
    """`python bench.py --gpus 2` without a launcher starts 2 child ranks (here: BENCH_REHEARSE=1 -> both on cuda:0 over
    gloo), reports n_gpus = 2, and the gathered output of the HIP path equals the unsharded result (--verify)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env["BENCH_REHEARSE"] = "1"
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--full",
                        "--reps", "2", "--prewarm-ms", "0", "--no-cpu-baseline", "--no-gemv", "--no-empirical", "--verify"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["n_gpus"] == 2 and rec["verified"] is True
    assert rec["config"]["global_rows"] == 8192 and rec["config"]["kernel"] == "dequant+dense"
    for curve in ("gemm_only", "sync", "overlapped", "chunked"):
        assert rec[curve]["value"] > 0


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs: the real RCCL path (one-GPU boxes rehearse it over gloo above)")
def test_bench_two_ranks_on_the_real_nccl_backend():
    """`bench.py --gpus 2 --verify` on the real `nccl` (= RCCL) backend, one rank per GPU: init_process_group
    with device_id, the async all-gather of step i on RCCL's stream under the GEMM of step i+1, ChunkedGather, and the gathered
    output == the unsharded result.  Skipped on one-GPU boxes."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("BENCH_REHEARSE", None)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2", "--full",
                        "--reps", "2", "--prewarm-ms", "0", "--no-cpu-baseline", "--no-gemv", "--no-empirical", "--verify"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rec = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert rec["n_gpus"] == 2 and rec["verified"] is True
    assert "RCCL" in rec["config"]["parallelism"]
    for curve in ("gemm_only", "sync", "overlapped", "chunked"):
        assert rec[curve]["value"] > 0


def test_dequant_absmax_legacy_form_bit_exact():
    """functional.py:866-889, the non-QuantState form, against the reference's outputs (g8_misc.npz) and the oracle."""
    import json
    import os
    from tests.goldenio import HERE
    from tests.test_oracle_misc_golden import load_case
    man = json.load(open(os.path.join(HERE, "manifest_misc.json")))
    npz = np.load(os.path.join(HERE, "g8_misc.npz"))
    for c in man["dequant_absmax"]:
        q, scales, want = load_case(npz, c)
        got = bnb.dequant_absmax(q.to(DEV), scales.to(DEV), blocksize=c["blocksize"])
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert bits_equal(got.cpu(), want), c
    # the QuantState form still routes to dequantize_blockwise
    x = synthetic.normal((1000,), torch.float32, seed=3).to(DEV)
    qb, stb = bnb.quantize_blockwise(x, blocksize=256)
    assert torch.equal(bnb.dequant_absmax(qb, stb), bnb.dequantize_blockwise(qb, stb))
    # a larger random case vs the oracle
    g = torch.Generator().manual_seed(5)
    q = torch.randint(0, 256, (37, 1111), generator=g, dtype=torch.uint8)
    sc = torch.rand(37, 5, generator=g) + 0.1
    assert bits_equal(bnb.dequant_absmax(q.to(DEV), sc.to(DEV), 256).cpu(), oracle.dequant_absmax(q, sc, 256))


def test_quant_state_from_dict_with_cpu_state2_and_mismatched_absmax():
    """QuantState.from_dict() defaults to 'cpu'; the nested absmax2 must follow the packed weight's device
    (never a host pointer into a kernel), and an absmax that does not match shape / blocksize must raise on the host."""
    N, K = 256, 512
    W = synthetic.normal((N, K), torch.float16, seed=91)
    packed, st = bnb.quantize_nf4(W.to(DEV), compress_statistics=True)
    X = synthetic.normal((8, K), torch.float16, seed=92).to(DEV)
    want = bnb.matmul_4bit(X, packed, st)
    st_cpu = QuantState.from_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in st.as_dict().items()
                                   if k != "state2"} | {"state2": {k: (v.cpu() if torch.is_tensor(v) else v)
                                                                    for k, v in st.state2.as_dict().items()}})
    assert st_cpu.absmax.device.type == "cpu" and st_cpu.state2.absmax.device.type == "cpu"
    assert torch.equal(bnb.matmul_4bit(X, packed, st_cpu), want)
    assert torch.equal(bnb.dequantize_4bit(packed, st_cpu), bnb.dequantize_4bit(packed, st))
    # first level on the GPU, second level left on the host: moved, not dereferenced
    st_mixed = QuantState(absmax=st.absmax, shape=st.shape, blocksize=64, quant_type="nf4", dtype=torch.float16,
                          state2=QuantState(absmax=st.state2.absmax.cpu(), shape=st.state2.shape, blocksize=256,
                                            quant_type="int8", dtype=torch.float32))
    assert torch.equal(bnb.matmul_4bit(X, packed, st_mixed), want)
    # a checkpoint whose blocksize disagrees with its absmax
    bad = QuantState(absmax=st.absmax, shape=st.shape, blocksize=32, quant_type="nf4", dtype=torch.float16, state2=st.state2)
    with pytest.raises(ValueError, match="absmax has"):
        bnb.matmul_4bit(X, packed, bad)
    with pytest.raises(ValueError, match="absmax has"):
        bnb.dequantize_4bit(packed, bad)
    short2 = QuantState(absmax=st.absmax, shape=st.shape, blocksize=64, quant_type="nf4", dtype=torch.float16,
                        state2=QuantState(absmax=st.state2.absmax[:1], shape=st.state2.shape, blocksize=256,
                                          quant_type="int8", dtype=torch.float32))
    with pytest.raises(ValueError, match="state2.absmax has"):
        bnb.matmul_4bit(X, packed, short2)


def test_quantize_4bit_nan_blocks_match_the_reference():
    """a NaN inside a block -> NaN absmax and index 0 for the whole block (reference: abs().max() propagates
    NaN, argmin over all-NaN distances is 0); goldens produced by the reference (g8_misc.npz)."""
    from tests.test_oracle_misc_golden import check_quant4_nan

    def q(x, bs, qt):
        packed, st = bnb.quantize_4bit(x.to(DEV), blocksize=bs, quant_type=qt)
        return packed, st.absmax
    check_quant4_nan(q)


def test_quantize_4bit_supplied_absmax_ties_match_the_reference():
    """A caller-supplied absmax far below |x|: from |x / absmax| ~ 2^23 the reference's argmin over f32 distances returns the
    first index of a tie, not the nearest code (goldens produced by the reference, g8_misc.npz)."""
    from tests.test_oracle_misc_golden import check_quant4_absmax_in
    check_quant4_absmax_in(lambda x, am, bs, qt: bnb.quantize_4bit(x.to(DEV), absmax=am.to(DEV), blocksize=bs, quant_type=qt)[0])


@pytest.mark.parametrize("dt,emin,emax", [(torch.float32, -90, 90), (torch.bfloat16, -90, 90), (torch.float16, -12, 14)])
def test_quantize_4bit_dynamic_range_bit_exact(dt, emin, emax):
    """x / absmax is an f32 true division in the reference (functional.py:236); the kernels compute the reciprocal part once
    per lane and the per-element correction chain of the IEEE expansion while absmax is in [2^-60, 2^60], the plain division
    outside.  Rows scaled by 2^e across (and beyond) that range, 65 536 distinct absmax mantissas, both code tables, a block
    larger than a wave step, the one-launch double-quant kernel and a caller-supplied absmax: packed bytes and absmax equal
    the oracle's."""
    rows, cols = 1024, 2048
    x = synthetic.normal((rows, cols), torch.float32, seed=91)
    e = torch.arange(rows) % (emax - emin + 1) + emin
    x = (x * torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double()).float().unsqueeze(1)).to(dt)
    assert torch.isfinite(x.float()).all()
    for qt, bs, cs in (("nf4", 64, False), ("fp4", 64, False), ("nf4", 2048, False), ("nf4", 32, True), ("fp4", 512, True)):
        o_packed, o_absmax, o_st2 = oracle.quantize_4bit(x, bs, qt, cs)
        packed, st = bnb.quantize_4bit(x.to(DEV), blocksize=bs, quant_type=qt, compress_statistics=cs)
        assert n_mismatch(packed.cpu(), o_packed) == 0, (qt, bs, cs)
        if cs:
            assert torch.equal(st.absmax.cpu(), o_absmax) and bits_equal(st.state2.absmax.cpu(), o_st2[0])
        else:
            assert bits_equal(st.absmax.cpu(), o_absmax)
    # a caller-supplied absmax far below |x| (quotients up to 2^60 and beyond): plain division, same bytes as the oracle
    small = torch.full((rows * cols // 64,), 2.0 ** -20 if dt != torch.float16 else 2.0 ** -10, dtype=torch.float32)
    packed, _ = bnb.quantize_4bit(x.to(DEV), absmax=small.to(DEV), blocksize=64, quant_type="nf4")
    o_packed, _, _ = oracle.quantize_4bit(x, 64, "nf4", False, absmax=small)
    assert n_mismatch(packed.cpu(), o_packed) == 0


@pytest.mark.parametrize("bs", [8, 16, 64, 128, 512, 1024])
def test_quantize_4bit_fused_double_quant_equals_two_launches(bs):
    """compress_statistics=True in one launch (mbnb_quantize_4bit_dq, 8 <= blocksize <= 512) must give exactly what
    quantize_4bit followed by quantize_blockwise(absmax, 256) gives (functional.py:288-292) -- packed bytes, int8 absmax
    codes, absmax2 -- on ragged shapes, flat tensors and groups of 256 blocks that straddle rows."""
    for shape, dt in (((300, 1000), torch.float16), ((7, 4160), torch.bfloat16), ((5000,), torch.float32), ((1, 64), torch.float16),
                      ((513, 512), torch.bfloat16)):
        x = synthetic.normal(shape, dt, seed=77 + bs).to(DEV)
        p1, s1 = bnb.quantize_4bit(x, blocksize=bs, compress_statistics=True)
        p0, s0 = bnb.quantize_4bit(x, blocksize=bs, compress_statistics=False)
        q0, st0 = bnb.quantize_blockwise(s0.absmax, blocksize=256)
        assert torch.equal(p1, p0), (shape, bs)
        assert s1.absmax.dtype == torch.int8 and torch.equal(s1.absmax, q0), (shape, bs)
        assert bits_equal(s1.state2.absmax, st0.absmax) and s1.state2.blocksize == 256 and s1.state2.dtype == torch.float32
        assert tuple(s1.state2.shape) == tuple(st0.shape) and s1.state2.quant_type == "int8"
        assert torch.equal(bnb.dequantize_4bit(p1, s1), bnb.dequantize_4bit(p0, QuantState(
            absmax=q0, shape=s0.shape, blocksize=bs, quant_type="nf4", dtype=dt, state2=st0)))


def test_reentrancy_two_threads_two_streams():
    """SURVEY 8b threading / streams: the C ABI keeps no per-call state (workspaces travel as arguments, the error text and
    the kernel name are thread-local), so two host threads driving different streams concurrently must get the results of
    a serial run -- across every kernel family that needs a dynamic-LDS attribute or a split-K workspace."""
    import threading
    N, K = 2560, 512
    W = synthetic.normal((N, K), torch.bfloat16, seed=301).to(DEV)
    packed, st = bnb.quantize_nf4(W)
    Ms = [1, 24, 100, 300, 2560]
    xs = [synthetic.normal((m, K), torch.bfloat16, seed=302 + m).to(DEV) for m in Ms]
    want = [bnb.matmul_4bit(x, packed, st) for x in xs]
    torch.cuda.synchronize()
    got = {0: None, 1: None}
    errs = []

    def worker(tid):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                outs = None
                for _ in range(20):
                    outs = [bnb.matmul_4bit(x, packed, st) for x in (xs if tid == 0 else xs[::-1])]
                s.synchronize()
            got[tid] = outs if tid == 0 else outs[::-1]
        except Exception as e:   # noqa: BLE001
            errs.append(repr(e))
    ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for tid in (0, 1):
        for w, g_ in zip(want, got[tid]):
            assert torch.equal(w, g_)


def test_matmul_4bit_inside_a_hip_graph():
    """The hot path is capturable: no allocation, synchronisation or host round trip inside the library (the workspace of
    the split-K shapes comes from torch's graph-private pool); replays reproduce the eager result."""
    N, K = 4096, 1024
    W = synthetic.normal((N, K), torch.float16, seed=311).to(DEV)
    packed, st = bnb.quantize_nf4(W, compress_statistics=True)
    for M in (1, 16, 128, 4096):
        x = synthetic.normal((M, K), torch.float16, seed=312 + M).to(DEV)
        eager = bnb.matmul_4bit(x, packed, st)
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            bnb.matmul_4bit(x, packed, st)
            with torch.cuda.graph(g, stream=side):
                y = bnb.matmul_4bit(x, packed, st)
        torch.cuda.current_stream().wait_stream(side)
        for _ in range(3):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager), M


def test_synthetic_inputs_generated_on_the_gpu_equal_the_host_form():
    """bench.py's inputs (synthetic.normal_device on the GPU) are the bits of synthetic.normal on the host, f64 -> 16-bit rounding
    included."""
    for dt in (torch.float16, torch.bfloat16, torch.float32):
        for seed, std, shape in ((1234, 1.0, (513, 1031)), (4321, 0.02, (64, 4096))):
            assert torch.equal(synthetic.normal(shape, dt, seed=seed, std=std), synthetic.normal_device(shape, dt, seed=seed, std=std, device=DEV).cpu())


@pytest.mark.parametrize("M,N,K,dt,qt,dq,with_bias", [(2048, 3072, 256, torch.bfloat16, "nf4", False, False),
                                                       (2500, 2600, 512, torch.float16, "fp4", False, True),
                                                       (2304, 3000, 768, torch.bfloat16, "nf4", True, True),
                                                       (4096, 4096, 1024, torch.float16, "nf4", True, False)])
def test_matmul_fused4_equals_the_decode_once_path(M, N, K, dt, qt, dq, with_bias):
    """k_gemm_fused4 (csrc/gemm_fused4.h: the 4-bit decode inside the four-wave MFMA pipeline, one launch, no scratch) -- since round 4
    what mbnb_matmul_4bit runs at blocksize 64 for a caller without the N x K scratch (workspace NULL, or MBNB_MATMUL_FUSED_ONLY with
    one): same B-operand bits and MFMA order as dequantize_4bit +
    k_gemm_dense, hence the same output bits; plain and double-quantised absmax, both tables, ragged M / N, bias; and the oracle."""
    import ctypes
    lib = _native.lib()
    W = synthetic.normal((N, K), dt, seed=401, std=0.05 if dq else 1.0)
    x = synthetic.normal((M, K), dt, seed=402).to(DEV)
    bias = synthetic.normal((N,), dt, seed=403).to(DEV) if with_bias else None
    packed, st = bnb.quantize_4bit(W.to(DEV), blocksize=64, quant_type=qt, compress_statistics=dq)
    y_ref = bnb.matmul_4bit(x, packed, st, bias)
    assert _native.last_kernel().startswith("dequant+dense")
    keep = []
    desc = bnb.functional._absmax_desc(st.absmax, st.state2, keep)
    out = torch.full((M, N), float("nan"), dtype=dt, device=DEV)
    code = _native.DTYPE_CODE[dt]
    ws = torch.empty(int(lib.mbnb_matmul_4bit_workspace_bytes(M, N, K, K, code, 0)), dtype=torch.uint8, device=DEV)
    assert ws.numel() >= N * K * 2
    for wsp, wsb, flags in ((None, 0, 0), (ws.data_ptr(), ws.numel(), 1)):    # no workspace; a workspace the caller does not want the weight in
        out.fill_(float("nan"))
        rc = lib.mbnb_matmul_4bit(x.data_ptr(), M, K, packed.data_ptr(), ctypes.byref(desc), N, K, 64, _native.QUANT_CODE[qt], code,
                                  None if bias is None else bias.data_ptr(), code, out.data_ptr(), wsp, wsb, flags, _native.stream_ptr(DEV))
        assert rc == 0, lib.mbnb_last_error()
        assert _native.last_kernel() == "mfma256f"
        assert torch.equal(out, y_ref)
    rows = torch.arange(0, M, max(1, M // 32))[:32]
    op, oa, os2 = oracle.quantize_4bit(W, 64, qt, dq)
    ref = oracle.matmul_4bit(x.cpu()[rows], op, oa, (N, K), 64, qt, dt, None if bias is None else bias.cpu(), None, os2)
    assert rel_fro(out.cpu()[rows], ref) <= TOL[dt]


@pytest.mark.parametrize("N,K,dt,qt,dq,with_bias", [(4096, 4096, torch.bfloat16, "nf4", False, False), (4096, 4096, torch.float16, "nf4", True, True),
                                                     (1000, 2048, torch.bfloat16, "fp4", False, True), (515, 8192, torch.float16, "nf4", False, False),
                                                     (4096, 8192, torch.bfloat16, "nf4", True, False),
                                                     (1030, 5120, torch.bfloat16, "nf4", False, True),       # 2.5 chunks: the last one half empty
                                                     (777, 11008, torch.float16, "nf4", True, False),        # 5.4 chunks on the 6-chunk form, nested absmax
                                                     (11008, 4096, torch.bfloat16, "fp4", False, False),     # N >= 8192
                                                     (300, 14336, torch.bfloat16, "nf4", False, True),       # 7 chunks on the 8-chunk form
                                                     (256, 1088, torch.float16, "nf4", False, False)])       # one partial chunk
def test_matmul_m1_lean_gemv_vs_oracle(N, K, dt, qt, dq, with_bias):
    """M = 1 at K = 2048 / 4096 / 8192, blocksize 64 -> k_gemv4_lean (round 3).  VERDICT r2's thin spot: the bf16 instantiation the
    bench's `gemv` object times at 4096^2 against the oracle at that size; plus FP4, double-quantised absmax, bias, a ragged N
    (the last workgroup's idle waves) and the 2- and 8-chunk rows.  And the row is independent of its neighbours: the same row
    through the M = 2 kernel agrees."""
    W = synthetic.normal((N, K), dt, seed=421, std=0.05 if dq else 1.0)
    x = synthetic.normal((1, K), dt, seed=422)
    bias = synthetic.normal((N,), dt, seed=423) if with_bias else None
    packed, st = bnb.quantize_4bit(W.to(DEV), blocksize=64, quant_type=qt, compress_statistics=dq)
    y = bnb.matmul_4bit(x.to(DEV), packed, st, None if bias is None else bias.to(DEV))
    assert _native.last_kernel() == "gemv"
    op, oa, os2 = oracle.quantize_4bit(W, 64, qt, dq)
    assert torch.equal(packed.cpu(), op)
    ref = oracle.matmul_4bit(x, op, oa, (N, K), 64, qt, dt, bias, None, os2)
    assert rel_fro(y.cpu(), ref) <= TOL[dt]
    x2 = torch.cat([x, synthetic.normal((1, K), dt, seed=424)]).to(DEV)
    y2 = bnb.matmul_4bit(x2, packed, st, None if bias is None else bias.to(DEV))
    assert rel_fro(y2[:1].cpu(), y.cpu()) <= TOL[dt]


@pytest.mark.parametrize("M,N,K,dt,qt,dq,with_bias,kern", [(512, 4096, 4096, torch.bfloat16, "nf4", False, False, "mfma_small"),
                                                           (450, 4096, 4096, torch.float16, "fp4", True, True, "mfma_small"),
                                                           (300, 1000, 3072, torch.bfloat16, "nf4", False, True, "mfma_small_splitk"),
                                                           (512, 2048, 4096, torch.bfloat16, "nf4", True, False, "mfma_small_splitk"),
                                                           (400, 5120, 4096, torch.bfloat16, "nf4", False, False, "dequant+dense"),
                                                           (512, 4096, 8192, torch.bfloat16, "nf4", False, False, "mfma_small_splitk"),     # 32 steps in two slices of 16
                                                           (512, 8192, 2048, torch.bfloat16, "nf4", False, True, "mfma_small"),               # the 128-row form: 256 workgroups
                                                           (512, 11008, 4096, torch.bfloat16, "nf4", True, False, "dequant+dense")])         # two rounds even of the 128-row form
def test_matmul_257_to_512_rows_stay_fused_where_one_round_serves_them(M, N, K, dt, qt, dq, with_bias, kern):
    """Round 3: 256 < M <= 512 rows go to k_gemm_small (16 steps of weights in registers: K = 4096 in one slice) where its workgroups
    fit the chip in one round -- 512 x 4096^2 35.6 us against 40.6 for dequantise + dense (profiles/r03_small16_ab.txt) -- and to the
    decode-once path where they do not (more than 256 workgroups, or K beyond 16 steps per slice).  Every row against the oracle."""
    W = synthetic.normal((N, K), dt, seed=441, std=0.05 if dq else 1.0)
    x = synthetic.normal((M, K), dt, seed=442)
    bias = synthetic.normal((N,), dt, seed=443) if with_bias else None
    packed, st = bnb.quantize_4bit(W.to(DEV), blocksize=64, quant_type=qt, compress_statistics=dq)
    y = bnb.matmul_4bit(x.to(DEV), packed, st, None if bias is None else bias.to(DEV))
    assert _native.last_kernel() == kern
    op, oa, os2 = oracle.quantize_4bit(W, 64, qt, dq)
    assert torch.equal(packed.cpu(), op)
    rows = torch.tensor(sorted(set([0, 1, 127, 128, 255, 256, 257, M - 1] + [int(v) for v in synthetic.uniform_u64(24, 77) % np.uint64(M)])))
    ref = oracle.matmul_4bit(x[rows], op, oa, (N, K), 64, qt, dt, bias, None, os2)
    assert rel_fro(y.cpu()[rows], ref) <= TOL[dt]


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,dt,qt,dq", [(600, 4096, 4096, torch.bfloat16, "nf4", False),      # four dwords per thread + write-through (<= 32 Mi elements)
                                           (2048, 2048, 2048, torch.float16, "fp4", True),        # the same, double-quantised absmax
                                           (2100, 11008, 4096, torch.bfloat16, "nf4", True),      # > 32 Mi elements, >= 2048 rows: one dword + write-through
                                           (700, 11008, 4096, torch.float16, "nf4", False)])      # > 32 Mi elements, < 2048 rows: the public kernel's stores
def test_matmul_decode_once_pass_forms_keep_the_public_kernels_bits(M, N, K, dt, qt, dq):
    """Round 3: inside matmul_4bit's decode-once path the dequantise pass runs in another shape than the public dequantize_4bit (write-through
    stores, four dwords per thread on weights of up to 32 Mi elements: quant_kernels.hip store_policy; linear8_dense_path has the same for the
    8-bit weights).  The scratch must hold the public kernel's bits: matmul_4bit == linear_dense(dequantize_4bit(...)) bit for bit, and
    linear_int8 == linear_dense(dequantize_rowwise(...))."""
    W = synthetic.normal((N, K), dt, seed=61, std=0.05).to(DEV)
    x = synthetic.normal((M, K), dt, seed=62).to(DEV)
    b = synthetic.normal((N,), dt, seed=63).to(DEV)
    packed, st = bnb.quantize_4bit(W, blocksize=64, quant_type=qt, compress_statistics=dq)
    y = bnb.matmul_4bit(x, packed, st, b)
    assert _native.last_kernel().startswith("dequant+dense")
    Wd = bnb.dequantize_4bit(packed, st)
    assert torch.equal(y, bnb.functional.linear_dense(x, Wd, b))
    del Wd
    q, sc = bnb.quantize_rowwise(W)
    y8 = bnb.linear_int8(x, q, sc, b)
    assert _native.last_kernel().startswith("w8a16_dequant+dense")
    assert torch.equal(y8, bnb.functional.linear_dense(x, bnb.dequantize_rowwise(q, sc, dt), b))


# --------------------------------------------------------------------------- round-4 additions: column-balanced grids of k_gemm_dense_nb
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,code,cols_a,dt,odt,with_bias", [
    (2304, 3584, 256, 7, 0, torch.bfloat16, None, False),          # 16 columns of 224, whole tiles
    (2304, 3000, 192, 7, 5, torch.float16, None, True),            # 5 x 256 + 8 x 224: the last column 128 wide, ragged M
    (2500, 2600, 128, 6, 3, torch.bfloat16, torch.float32, True),  # 3 x 224 + 10 x 192 (the last 8 columns wide), f32 output
    (1300, 4100, 320, 5, 0, torch.float16, None, False),           # 26 columns of 160 (the last 100 wide), five k-steps
    (4096, 1000, 384, 5, 4, torch.bfloat16, torch.float16, True),  # 4 x 192 + 2 x 160, N % 8 == 0 only
    (3000, 2041, 256, 6, 2, torch.bfloat16, None, True),           # odd N: the scalar store path of the epilogue
    (5000, 5120, 512, 7, 10, torch.bfloat16, None, False),         # 20 tile rows (tiles_m % 4 == 0, five patch rows), 500 tiles
    (3840, 3712, 256, 7, 9, torch.float16, None, False),           # 15 tile rows: a ragged patch row under every patch column
])
def test_gemm_dense_column_balanced_grids_keep_the_bits(M, N, K, code, cols_a, dt, odt, with_bias):
    """k_gemm_dense_nb (round 4, csrc/gemm_dense.h): tile columns 224 / 192 / 160 wide, alone or behind wider ones, walked in ragged XCD patches --
    forced through the diagnostic tile codes of mbnb_gemm_dense.  Every output element is written exactly as the uniform 256 x 256 tiles
    write it (same B bits, same summation order per row): torch.equal on NaN-prefilled outputs, f16 / bf16, bias, f32 and 16-bit outputs,
    ragged M and N; and a float64 product of the same operands."""
    lib = _native.lib()
    x = synthetic.normal((M, K), dt, seed=811).to(DEV)
    w = synthetic.normal((N, K), dt, seed=812, std=0.05).to(DEV)
    bias = synthetic.normal((N,), dt, seed=813).to(DEV) if with_bias else None
    odt = odt or dt
    code_dt, code_o = _native.DTYPE_CODE[dt], _native.DTYPE_CODE[odt]

    def run(sel):
        out = torch.full((M, N), float("nan"), dtype=odt, device=DEV)
        rc = lib.mbnb_gemm_dense(x.data_ptr(), w.data_ptr(), code_dt, None if bias is None else bias.data_ptr(), code_o, out.data_ptr(), M, N, K, K,
                                 None, 0, 1 | sel, _native.stream_ptr(DEV))
        assert rc == 0, lib.mbnb_last_error()
        return out, _native.last_kernel()

    y_u, name_u = run(2 << 8)
    y_b, name_b = run((code << 8) | (cols_a << 16))
    assert name_u == "dense 256x256" and name_b.startswith("dense_nb "), (name_u, name_b)
    assert f"{cols_a}x{32 * (code + 1)}+" in name_b and name_b.endswith(f"x{32 * code}")
    assert bool(torch.isfinite(y_b.float()).all()), "an output element was never written"
    assert torch.equal(y_u, y_b), f"{name_b} differs from the uniform tiles"
    rows = torch.arange(0, M, max(1, M // 24))[:24]
    ref = x[rows.to(DEV)].double() @ w.double().t() + (0 if bias is None else bias.double())
    assert rel_fro(y_b[rows.to(DEV)].cpu(), ref.cpu()) <= 1.5 * TOL[dt]     # against the EXACT product: the output's own rounding is inside


@pytest.mark.gpu
def test_matmul_4bit_takes_the_balanced_grid_where_its_plan_says_so():
    """4096 x 6144 x 4096 (24 columns of 256 = 384 tiles = 1.5 rounds of 256 CUs): the plan cuts N into 32 columns of 192 (two whole rounds of
    smaller tiles, tools/exp/ab_dense_nb.py) -- through matmul_4bit the result equals the fused kernel's bits (k_gemm_fused4: same B bits,
    same summation order) and the oracle on a row sample; BASELINE configs[2] (11008 wide) keeps its uniform columns."""
    lib = _native.lib()
    M, N, K, dt = 4096, 6144, 4096, torch.bfloat16
    W = synthetic.normal((N, K), dt, seed=821, std=0.02)
    X = synthetic.normal((M, K), dt, seed=822).to(DEV)
    packed, st = bnb.quantize_nf4(W.to(DEV), compress_statistics=True)
    wd = bnb.dequantize_4bit(packed, st)
    out = torch.empty(M, N, dtype=dt, device=DEV)
    code = _native.DTYPE_CODE[dt]
    assert lib.mbnb_gemm_dense(X.data_ptr(), wd.data_ptr(), code, None, code, out.data_ptr(), M, N, K, K, None, 0, 0, _native.stream_ptr(DEV)) == 0
    assert _native.last_kernel().startswith("dense_nb "), _native.last_kernel()
    y = bnb.matmul_4bit(X, packed, st)
    assert _native.last_kernel() == "dequant+dense"
    assert torch.equal(y, out)
    bnb.functional.DECODE_ONCE = False
    try:
        yf = bnb.matmul_4bit(X, packed, st)
        assert _native.last_kernel() == "mfma256f"
    finally:
        bnb.functional.DECODE_ONCE = True
    assert torch.equal(y, yf)
    rows = torch.arange(5, M, 173)
    op, oa, os2 = oracle.quantize_4bit(W, 64, "nf4", True)
    ref = oracle.matmul_4bit(X[rows.to(DEV)].cpu(), op, oa, (N, K), 64, "nf4", dt, None, None, os2)
    assert rel_fro(y[rows.to(DEV)].cpu(), ref) <= TOL[dt]
    out2 = torch.empty(M, 11008, dtype=dt, device=DEV)
    w2 = synthetic.normal((11008, 256), dt, seed=823).to(DEV)
    x2 = synthetic.normal((M, 256), dt, seed=824).to(DEV)
    assert lib.mbnb_gemm_dense(x2.data_ptr(), w2.data_ptr(), code, None, code, out2.data_ptr(), M, 11008, 256, 256, None, 0, 0, _native.stream_ptr(DEV)) == 0
    assert _native.last_kernel() == "dense 256x256"


@pytest.mark.gpu
def test_gemm_dense_balanced_grids_randomised():
    """36 random forced grids (tile code 5 / 6 / 7, a random number of wider columns first; M 2304 .. 6000, N 2000 .. 9000 incl. odd values, K 128 .. 320)
    against the uniform 256 x 256 tiles on NaN-prefilled outputs: every element written, every bit equal -- the tile walk (XCD-major pseudo-patches over
    ragged patches) is a bijection at every grid size drawn, and the narrow bodies' edge handling (columns past N, rows past M) matches the wide one's."""
    import random
    lib = _native.lib()
    rng = random.Random(20261005)
    sp = _native.stream_ptr(DEV)
    for case in range(36):
        M = rng.randint(2304, 6000)
        N = rng.choice([rng.randint(2000, 9000), 8 * rng.randint(250, 1100), 256 * rng.randint(9, 34)])
        K = 64 * rng.randint(2, 5)
        code = rng.choice([5, 6, 7])
        cols_a = rng.randint(0, (N // 32) // (code + 1))
        dt = rng.choice([torch.float16, torch.bfloat16])
        x = synthetic.normal((M, K), dt, seed=9000 + case).to(DEV)
        w = synthetic.normal((N, K), dt, seed=9100 + case, std=0.05).to(DEV)
        bias = synthetic.normal((N,), dt, seed=9200 + case).to(DEV) if case % 3 == 0 else None
        c = _native.DTYPE_CODE[dt]
        outs = []
        for sel in (2 << 8, (code << 8) | (cols_a << 16)):
            out = torch.full((M, N), float("nan"), dtype=dt, device=DEV)
            rc = lib.mbnb_gemm_dense(x.data_ptr(), w.data_ptr(), c, None if bias is None else bias.data_ptr(), c, out.data_ptr(), M, N, K, K, None, 0, 1 | sel, sp)
            assert rc == 0, lib.mbnb_last_error()
            outs.append(out)
        name = _native.last_kernel()
        assert name.startswith("dense_nb "), name
        assert bool(torch.isfinite(outs[1].float()).all()), f"case {case}: M={M} N={N} K={K} {name}: an element was never written"
        assert torch.equal(outs[0], outs[1]), f"case {case}: M={M} N={N} K={K} {dt} {name} differs from the uniform tiles"

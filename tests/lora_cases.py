"""
The fused cases of functional.matmul_4bit_lora_grouped, one table for the GPU test (tests/test_gpu_lora.py) and for the CPU check that
the table can tell an adapter from none (tests/test_lora_host.py).  Shapes follow tests/test_gpu_group.py's.  Operands are made on the
CPU once per argument tuple and never modified: X, A, B and the weights are synthetic.normal, scaling is 4 / R, which puts the adapter
term at the base term's magnitude -- far above the bound, so a kernel that dropped or mis-indexed the adapter fails.
"""
import functools

import torch

import oracle
from mps_bitsandbytes_amd import synthetic

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}


def _ku_form(K):
    ku = (K + 2047) // 2048
    return ku, ku if ku <= 4 else 6 if ku <= 6 else 8


def _third(count):
    return tuple(None if i % 3 == 0 else 1 + i % 5 for i in range(count))


# (id, member Ns, K, quant types, nested, members with a bias, R per member)
FUSED = [
    ("single", (4,), 1024, ("nf4", "fp4"), False, (), (3,)),                            # a group of one; KU1, half a chunk
    ("ragged", (5, 1, 130), 2112, ("nf4", "fp4"), False, (1,), (16, None, 65)),         # the biased member has no adapter; two slices of B
    ("nested", (7, 64), 2304, ("fp4", "nf4"), True, (0,), (1, 64)),                     # R = 1, and exactly one slice
] + [(f"K{K}", (3, 6), K, ("nf4",), False, (), (63, 256)) for K in (4096, 6144, 8192, 8256, 12288, 12352, 16384)] + [   # ku 2 ... 8
    ("K16384-nested", (3, 6), 16384, ("nf4",), True, (), (63, 256)),
    ("sixteen", tuple(1 + i % 5 for i in range(16)), 1024, ("nf4",), False, (3,), _third(16)),       # one call
    ("seventeen", tuple(1 + i % 5 for i in range(17)), 1024, ("nf4",), False, (16,), _third(17)),    # two calls: 16 + 1
]
FUSED_PARAMS = [(f"{name}-{qt}-{dt}", Ns, K, qt, nested, bias, Rs, dt)
                for name, Ns, K, qts, nested, bias, Rs in FUSED for qt in qts for dt in ("f16", "bf16")]


def chunks(Rs):
    """[(members, sum of R)] of the calls a table of these ranks is cut into."""
    return [(len(Rs[c:c + 16]), sum(r or 0 for r in Rs[c:c + 16])) for c in range(0, len(Rs), 16)]


def report(Rs, K):
    """The launch report after the last call of the case."""
    n, total = chunks(Rs)[-1]
    ku, KU = _ku_form(K)
    return f"lora_down G{n} R{total} ku{ku}/KU{KU} + gemv_lora G{n} ku{ku}/KU{KU}"


@functools.lru_cache(maxsize=None)
def member(N, K, dt, qt="nf4", nested=False, bs=64, seed=0):
    """(packed, absmax, state2 or None, decoded weight [N, K]) of the CPU oracle."""
    T = DT[dt]
    W = synthetic.normal((N, K), T, seed=100 + seed)
    op, oa, ost2 = oracle.quantize_4bit(W, bs, qt, nested)
    return op, oa, ost2, oracle.dequantize_4bit(op, oa, (N, K), bs, qt, T, ost2)


@functools.lru_cache(maxsize=None)
def x(K, dt, seed=7, rows=1):
    return synthetic.normal((rows, K), DT[dt], seed=seed)


@functools.lru_cache(maxsize=None)
def bias(N, dt, seed):
    return synthetic.normal((N,), DT[dt], seed=200 + seed)


@functools.lru_cache(maxsize=None)
def adapter(N, K, R, dt, seed):
    """(A [R, K], B [N, R], scaling = 4 / R), or None for R None."""
    if R is None:
        return None
    return synthetic.normal((R, K), DT[dt], seed=600 + seed), synthetic.normal((N, R), DT[dt], seed=700 + seed), 4.0 / R

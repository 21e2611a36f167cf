"""
The fused cases of functional.matmul_4bit_grouped and functional.matmul_4bit_lora_grouped for 2 to 16 activation rows (libmbnb_batch.so),
one table for the GPU test (tests/test_gpu_batch.py) and for the CPU check that each adapter case can tell an adapter from none
(tests/test_batch_host.py).  Operands come from tests/lora_cases.py (made on the CPU once per argument tuple, never modified): X, A, B and
the weights are synthetic.normal, scaling is 4 / R, which puts the adapter term at the base term's magnitude.

The shapes are the smallest at which each mechanism of k_skinny4_group can go wrong: a workgroup is 16 waves over the 128-k blocks of 16
weight rows of one member.
"""
from tests import lora_cases as lc

DT = lc.DT

# (id, member Ns, K, quant types, nested, blocksize, members with a bias, row counts, R per member for the adapter cases)
CASES = [
    # 17 blocks of 128: wave 0 makes two trips; dead rows (5 and 1 of 16), a partial last tile (130 = 8 * 16 + 2), a bias in the middle;
    # the biased member has no adapter, R = 65 takes two slices of B
    ("ragged", (5, 1, 130), 2176, ("nf4", "fp4"), False, 64, (1,), (2, 3, 15, 16), (16, None, 65)),
    ("single", (4,), 128, ("nf4",), False, 64, (), (2, 16), (3,)),                        # a group of one, one block: 15 idle waves
    ("nested", (7, 64), 2304, ("fp4",), True, 64, (0,), (2, 16), (1, 64)),                # blocksize2 blocks that span rows
    ("bs32", (5, 18), 1024, ("nf4",), False, 32, (), (2, 16), (3, 16)),                   # four absmax per 128-k block
    ("bs128", (5, 18), 1024, ("fp4",), False, 128, (1,), (2, 16), (3, 16)),               # one absmax per 128-k block
    ("K2176-wide", (3, 6), 2176, ("nf4",), False, 64, (), (2, 16), (63, 256)),            # the largest rank: four slices, pitch 257
    ("K16384", (40, 6), 16384, ("nf4",), False, 64, (), (2, 16), (63, 256)),              # the largest K: 8 trips per wave, KU8 down-projection
    ("sixteen", (3,) * 16, 256, ("nf4",), False, 64, (3,), (2, 16), tuple(None if i % 3 == 0 else 1 + i % 5 for i in range(16))),
    ("seventeen", (3,) * 17, 256, ("nf4",), False, 64, (16,), (2, 16), tuple(None if i % 3 == 0 else 1 + i % 5 for i in range(17))),
]
# the ragged case runs in both dtypes with both code tables; the others alternate
PARAMS = [(f"{name}-{qt}-{dt}-M{M}", Ns, K, qt, nested, bs, bias, Rs, dt, M)
          for i, (name, Ns, K, qts, nested, bs, bias, Ms, Rs) in enumerate(CASES)
          for qt in qts for dt in (("f16", "bf16") if name == "ragged" else (("bf16", "f16")[i % 2],)) for M in Ms]
IDS = [p[0] for p in PARAMS]
ARGS = [p[1:] for p in PARAMS]


def chunks(count):
    return [min(16, count - c) for c in range(0, count, 16)]


def grouped_report(count, M):
    """mbnb_batch_last_launch() after the last call of a grouped case."""
    return f"skinny_group G{chunks(count)[-1]} M{M}"


def lora_report(Rs, K, M):
    """mbnb_batch_last_launch() after the last call of an adapter case."""
    n, total = lc.chunks(Rs)[-1]
    ku = (K + 2047) // 2048
    KU = ku if ku <= 4 else 6 if ku <= 6 else 8
    return f"lora_down_rows G{n} R{total} M{M} ku{ku}/KU{KU} + skinny_group_lora G{n} M{M}"


def x(K, dt, M, seed=7):
    return lc.x(K, dt, seed, M)


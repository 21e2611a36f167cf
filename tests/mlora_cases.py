"""
The fused cases of functional.matmul_4bit_multilora_grouped (libmbnb_mlora.so: 2 to 16 activation rows, a different adapter per row),
one table for the GPU test (tests/test_gpu_mlora.py) and for the CPU check that each case can tell a row's adapter from the next
slot's and from none (tests/test_mlora_host.py).  Weights, activations and biases come from tests/lora_cases.py (made on the CPU once per
argument tuple, never modified).  A bank is synthetic.normal per slot with the slot scalings 4 / R * (1 + s / 4): distinct, and at the
base term's magnitude, far above the bound.

The shapes are the smallest at which each mechanism can go wrong: a workgroup of k_skinny4_mlora is 16 waves over the 128-k blocks of 16
weight rows of one member, wave w stages row w's slot; a workgroup of k_lora_down_sel is one (member, adapter row, activation row).
"""
import functools

import torch

from mps_bitsandbytes_amd import synthetic
from tests import lora_cases as lc
from tests.lora_bound import lora_bound

DT = lc.DT
PATTERNS = ("equal", "cyclic", "mixed", "none")


def ids_for(pattern, M, S):
    """The rows' slots: all rows on the last slot; one slot after the other; every second row outside [0, S) (-1, S, -7, 2^31 - 1 in
    turn); no row with an adapter."""
    if pattern == "equal":
        return [S - 1] * M
    if pattern == "cyclic":
        return [m % S for m in range(M)]
    if pattern == "mixed":
        outside = (-1, S, -7, 2 ** 31 - 1)
        return [outside[(m // 2) % 4] if m % 2 else (m // 2) % S for m in range(M)]
    assert pattern == "none", pattern
    return [-1] * M


# (id, member Ns, K, quant type, nested, blocksize, members with a bias, S, R per member (None: no bank), dtype, M, ids pattern)
_RAGGED = ((5, 1, 130), 2176)      # 17 blocks of 128: wave 0 makes two trips; dead rows, a partial last tile, a bias in the middle
CASES = []
_i = 0
for _M in (2, 3, 15, 16):
    for _dt in ("f16", "bf16"):
        for _qt in ("nf4", "fp4"):
            CASES.append((f"ragged-{_qt}-{_dt}-M{_M}", *_RAGGED, _qt, False, 64, (1,), 3, (3, 3, 3), _dt, _M, PATTERNS[(_i + _i // 4) % 4]))
            _i += 1
for _p in PATTERNS:      # every pattern at the largest batch and at an odd one
    CASES.append((f"ragged-nf4-bf16-M16-{_p}", *_RAGGED, "nf4", False, 64, (1,), 3, (3, 3, 3), "bf16", 16, _p))
    CASES.append((f"ragged-fp4-f16-M3-{_p}", *_RAGGED, "fp4", False, 64, (1,), 3, (3, 3, 3), "f16", 3, _p))
for _k, _R in enumerate((1, 16, 63, 64)):      # one rank, an even one, the largest odd one, a full slice (LDS pitches 1 | 17 | 63 | 65)
    CASES.append((f"R{_R}", *_RAGGED, "nf4", False, 64, (1,), 3, (_R,) * 3, ("bf16", "f16")[_k % 2], 15, ("mixed", "cyclic")[_k % 2]))
CASES += [
    ("no-bank-in-the-middle", *_RAGGED, "nf4", False, 64, (1,), 3, (3, None, 3), "bf16", 3, "cyclic"),
    ("nested-M2", (7, 64), 2304, "fp4", True, 64, (0,), 3, (3, 16), "f16", 2, "cyclic"),       # blocksize2 blocks that span rows
    ("nested-M16", (7, 64), 2304, "fp4", True, 64, (0,), 3, (3, 16), "f16", 16, "mixed"),
    ("bs32", (5, 18), 1024, "nf4", False, 32, (), 3, (3, 16), "bf16", 16, "mixed"),             # four absmax per 128-k block
    ("bs128", (5, 18), 1024, "fp4", False, 128, (1,), 3, (3, 16), "f16", 2, "cyclic"),          # one absmax per 128-k block
    ("single", (4,), 128, "nf4", False, 64, (), 3, (3,), "bf16", 16, "mixed"),                  # a group of one, one block: 15 idle waves
    ("K16384", (40, 6), 16384, "nf4", False, 64, (), 3, (16, 3), "bf16", 16, "mixed"),          # 8 trips per wave, KU8 down-projection
    ("sixteen", (3,) * 16, 256, "nf4", False, 64, (3,), 3, tuple(None if i % 3 == 0 else 1 + i % 5 for i in range(16)), "f16", 2, "cyclic"),
    ("seventeen", (3,) * 17, 256, "nf4", False, 64, (16,), 3, tuple(None if i % 3 == 0 else 1 + i % 5 for i in range(17)), "bf16", 16,
     "mixed"),
    ("S1", *_RAGGED, "nf4", False, 64, (1,), 1, (3, 3, 3), "bf16", 3, "mixed"),                # one slot: ids 0, -1, 0
    ("S9", *_RAGGED, "fp4", False, 64, (1,), 9, (3, 3, 3), "f16", 16, "cyclic"),               # nine distinct adapters in one batch
]
_seen = set()
CASES = [c for c in CASES if not (c[0] in _seen or _seen.add(c[0]))]
# "ragged-nf4-bf16-M16-<p>" may repeat a case of the cross under another name: keep one of each argument tuple
_args = set()
CASES = [c for c in CASES if not (c[1:] in _args or _args.add(c[1:]))]
IDS = [c[0] for c in CASES]
ARGS = [c[1:] for c in CASES]


def chunks(Rs):
    """[(members, sum of R)] of the calls a table of these ranks is cut into."""
    return lc.chunks(Rs)


def report(Rs, K, M):
    """mbnb_mlora_last_launch() after the last call of a case."""
    n, total = chunks(Rs)[-1]
    ku = (K + 2047) // 2048
    KU = ku if ku <= 4 else 6 if ku <= 6 else 8
    return f"lora_down_sel G{n} R{total} M{M} ku{ku}/KU{KU} + skinny_mlora G{n} M{M}"


def x(K, dt, M, seed=7):
    return lc.x(K, dt, seed, M)


@functools.lru_cache(maxsize=None)
def bank(N, K, R, S, dt, seed):
    """(lora_A [S, R, K], lora_B [S, N, R], scaling f32 [S]), or None for R None."""
    if R is None:
        return None
    T = DT[dt]
    scaling = torch.tensor([4.0 / R * (1 + s / 4) for s in range(S)], dtype=torch.float32)
    return synthetic.normal((S, R, K), T, seed=800 + seed), synthetic.normal((S, N, R), T, seed=900 + seed), scaling


def reference(X, Wd, bias, bank_, ids):
    """(r, S, R [M, 1]) in float64 on X's device, as tests/lora_bound.lora_reference, with row m's adapter the slot ids[m] of the bank (none
    where ids[m] is outside the bank, or the bank None).  ids: a list of ints."""
    Xd, Wdd = X.double(), Wd.double()
    r = Xd @ Wdd.t()
    S = Xd.abs() @ Wdd.abs().t()
    if bias is not None:
        r = r + bias.double()
        S = S + bias.double().abs()
    R = torch.zeros(X.shape[0], 1, dtype=torch.float64, device=X.device)      # per row: the bound of a row without an adapter has R = 0
    if bank_ is None:
        return r, S, R
    A, B, scaling = bank_
    for s in sorted(set(i for i in ids if 0 <= i < A.shape[0])):
        rows = torch.tensor([i == s for i in ids], device=X.device)
        f = float(scaling[s])          # the f32 value, exactly
        r[rows] += f * ((Xd[rows] @ A[s].double().t()) @ B[s].double().t())
        S[rows] += abs(f) * ((Xd[rows].abs() @ A[s].double().abs().t()) @ B[s].double().abs().t())
        R[rows] = float(A.shape[1])
    return r, S, R


def bound(r, S, R, K, T, path):
    return lora_bound(r, S, R, K, T, path)

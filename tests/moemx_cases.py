"""The case tables of libmbnb_moemx.so, shared by tests/test_moemx_host.py and tests/test_gpu_moemx.py."""
import numpy as np
import torch

R, CT, KS = 64, 256, 128                                     # MBNB_MOEMX_ROW_TILE, _COL_TILE, _K_STEP

# (activation format, a row per pair, output dtype): every format, layout and dtype, not their cross
FORMS = (("fp8", False, torch.bfloat16), ("fp4", True, torch.float16), ("fp8", True, torch.float32), ("fp4", False, torch.float32))
EXACT_N = (17, CT + 1)                                       # one ragged column tile; a second one with one live column
EXACT_K = (32, 64, 96, 128, 192, 416, 2880)                  # the one-step problem, every ragged last K-step, the model's K
RANDOM_NK = ((33, 1056), (CT + 1, 2880))


def exact_ids():
    """E = 3, T = 35, A = 2: 1 pair of expert 0, 65 of expert 1 (a full tile and a one-row tile), none of expert 2, four ids outside"""
    ids = np.array([0] + [1] * 65 + [-1, 3, 2 ** 30, -2 ** 31], dtype=np.int64)
    return ids[np.random.default_rng(5).permutation(70)].astype(np.int32).reshape(35, 2)


def random_ids(T, A, E, skewed, seed):
    rng = np.random.default_rng(seed)
    p = np.array([0.6] + [0.4 / (E - 1)] * (E - 1)) if skewed else None
    return rng.choice(E, size=(T, A), p=p).astype(np.int32)

"""
Operands and expectations of tests/nn_cases.py, built on the CPU from the case's data alone (seeded; the oracle for the values): shared by
tests/test_gpu_nn_forms.py, which runs the cases, and tests/test_nn_forms_host.py, which holds this arithmetic against plain torch restatements.
"""
import numpy as np
import torch

import oracle
from mps_bitsandbytes_amd import synthetic
from tests import nn_cases

DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
OUTLIER_SCALE = 64.0            # a power of two: exact in f16 and bf16


def _u64(n, seed):
    return synthetic.uniform_u64(n, seed)


def _unit(n, seed):
    """n floats in [0, 1) with 24 random bits each."""
    return torch.from_numpy(((_u64(n, seed) >> np.uint64(40)).astype(np.float64) / float(1 << 24)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ embeddings
def indices(c):
    """(index tensor, padding_idx)."""
    num = nn_cases.NUM
    kind = c["idx"]
    if kind == "one":
        return torch.tensor([3], dtype=torch.int64), None
    base = torch.from_numpy((_u64(40, 7) % np.uint64(num)).astype(np.int64))
    base[0], base[1], base[2], base[3] = 0, num - 1, 0, 5               # row 0 (twice) and the last row
    if kind == "oob":
        base[4], base[9], base[17], base[39] = -1, num, 2 ** 40, num + 3
    idx = base.reshape(5, 8)
    if kind == "i32":
        return idx.to(torch.int32), None
    if kind == "pad":
        idx[1, 2] = 2
        idx[4, 7] = 2
        return idx, 2
    return idx, None


def embedding_operands(c):
    """4-bit: (packed u8 [num, dim / 2] random bytes, absmax f32 [num, blocks] in [0.5, 1.5)); 8-bit: (q int8 [num, dim] over all of
    -128 ... 127, scales f32 [num] in [0.5, 1.5))."""
    num, dim = nn_cases.NUM, c["dim"]
    if c["op"] == "embedding_4bit":
        packed = torch.from_numpy((_u64(num * (dim // 2), 11) & np.uint64(0xFF)).astype(np.uint8)).reshape(num, dim // 2)
        nblk = (dim + c["bs"] - 1) // c["bs"]
        return packed, (_unit(num * nblk, 12) + 0.5).reshape(num, nblk)
    q = torch.from_numpy((_u64(num * dim, 13) & np.uint64(0xFF)).astype(np.uint8)).view(torch.int8).reshape(num, dim).clone()
    q.reshape(-1)[0], q.reshape(-1)[-1] = -128, 127
    return q, _unit(num, 14) + 0.5


def embedding_expected(c, a, b):
    """The oracle's rows where the index is in range, rows of zeros elsewhere (the oracle refuses an index out of range)."""
    idx, pad = indices(c)
    flat = idx.reshape(-1).to(torch.int64)
    ok = (flat >= 0) & (flat < nn_cases.NUM)
    dt = DT[c["dt"]]
    want = torch.zeros(flat.numel(), c["dim"], dtype=dt)
    if c["op"] == "embedding_4bit":
        want[ok] = oracle.embedding_4bit(flat[ok], a, b, c["dim"], c["bs"], c["qt"], pad, dt)
    else:
        want[ok] = oracle.embedding_8bit(flat[ok], a, b, pad, dt)
    return want.reshape(*idx.shape, c["dim"])


# ------------------------------------------------------------------------------------------------ the outlier-aware linear
def linear_operands(c):
    """x [M, K] normal with the outlier columns times 64 and, from the last row back, a row of zeros, a row that is zero outside the
    outlier columns and a row whose largest kept value sits next to an outlier column; int8 weights random in every column, the outlier
    columns included; positive scales; outlier weights; bias."""
    M, N, K, dt = c["M"], c["N"], c["K"], DT[c["dt"]]
    pos = nn_cases.positions(c)
    x = synthetic.normal((M, K), torch.float32, seed=21)
    keep = torch.ones(K, dtype=torch.bool)
    keep[pos] = False
    x[:, ~keep] *= OUTLIER_SCALE
    if M >= 2:
        x[M - 1] = 0
    if M >= 3 and pos:
        x[M - 2, keep] = 0
    if M >= 4 and pos:
        near = [k for k in range(K) if keep[k] and ((k > 0 and not keep[k - 1]) or (k + 1 < K and not keep[k + 1]))]
        x[M - 3, near[0]] = 7.5
    x = x.to(dt)
    q = torch.from_numpy((_u64(N * K, 22) % np.uint64(255)).astype(np.int64) - 127).to(torch.int8).reshape(N, K)
    s = (_unit(N, 23) + 0.5) * 0.02
    ow = synthetic.normal((N, len(pos)), dt, seed=24, std=0.05)
    b = synthetic.normal((N,), dt, seed=25) if c.get("bias") else None
    return dict(x=x, q=q, s=s, pos=pos, ow=ow, b=b)


def given_indices(c, ops):
    """(outlier_indices, outlier_weights) as the library is given them: for an `oob` case the entries -1 and K among the positions, with
    columns of outlier weights of their own."""
    lst = nn_cases.index_list(c)
    ow = ops["ow"]
    if c.get("oob"):
        extra = synthetic.normal((c["N"], 2), ow.dtype, seed=26, std=0.05)
        ow = torch.cat([ow[:, :1], extra[:, :1], ow[:, 1:], extra[:, 1:]], dim=1).contiguous()
    return torch.tensor(lst, dtype=torch.int64), ow


def masked(x, pos):
    xm = x.clone()
    xm[:, pos] = 0
    return xm


def workspace_expected(c, ops):
    """(xq int8 [M, K], scales f32 [M], xo [M, ldx] or None): the oracle's row quantisation of x with the in-range outlier columns zeroed;
    x[:, entry] per entry of the index list, zeros for an entry out of range and for the padding up to ldx."""
    xq, scales = oracle.quantize_rowwise(masked(ops["x"], ops["pos"]))
    m = nn_cases.model(c)
    xo = None
    if m[0] != "error" and m[1]:
        lst = nn_cases.index_list(c)
        xo = torch.zeros(c["M"], nn_cases.ldx(len(lst)), dtype=ops["x"].dtype)
        for j, k in enumerate(lst):
            if 0 <= k < c["K"]:
                xo[:, j] = ops["x"][:, k]
    return xq, scales, xo


def split_workspace(ws, M, K, n, fill):
    """The workspace's bytes (uint8, CPU) by the layout above outlier_linear_workspace_bytes: xq, scales, the xo region up to the M x ldx(n)
    values, and whether every other byte -- the pads after each region, the rest of the buffer -- holds the fill."""
    off_s, off_x, end_x = nn_cases.regions(M, K, n)
    end_x = min(end_x, ws.numel())
    xq = ws[:M * K].view(torch.int8).reshape(M, K)
    scales = ws[off_s:off_s + 4 * M].view(torch.float32)
    xo = ws[min(off_x, ws.numel()):end_x]
    pads = torch.cat([ws[M * K:off_s], ws[off_s + 4 * M:off_x], ws[end_x:]])
    return xq, scales, xo, bool((pads == fill).all())


def reference_output(c, ops, rows=None):
    """oracle.outlier_linear on the in-range positions (an entry out of range contributes nothing), on a row sample if asked."""
    x = ops["x"] if rows is None else ops["x"][rows]
    return oracle.outlier_linear(x, ops["q"], ops["s"], torch.tensor(ops["pos"], dtype=torch.int64), ops["ow"], ops["b"])


def row_sample(M):
    """The rows tests/test_gpu_nn_parity.py's test_outlier_linear_vs_oracle checks; every row of a small case."""
    if M <= 64:
        return torch.arange(M)
    return torch.cat([torch.arange(0, M, max(1, M // 60))[:60], torch.arange(M - 4, M)])

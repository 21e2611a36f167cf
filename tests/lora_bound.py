"""
Elementwise bounds of functional.matmul_4bit_lora_grouped against a float64 evaluation of what it defines:

    r = X . Wd^T + b + s (X . A^T) . B^T            s = float32(scaling), Wd the CPU oracle's decoded weight
    S = |X| . |Wd|^T + |b| + |s| (|X| . |A|^T) . |B|^T

with u_T and a as in tests/elementwise.py (the unit roundoff of the weight dtype; 2^-24 where f16 is involved).

Fused path (libmbnb_lora.so):        |y - r| <= g S + u_T (|r| + g S) + a,            g = (K + R + 6) 2^-23.
    The base's K products are exact in f32 and their adds, in any order, are the K + 2 of tests/elementwise.py.  Each t_j is a sum of K
    exact products with at most K + 2 f32 roundings (K - 1 adds, the 3 cross-wave adds).  The up-projection rounds each product
    f32(B[n, j]) t_j once and adds the R of them in a wave sum: a term passes through at most R adds that are not adds of an exact
    zero, so R + 1.  The scaling, the add to the accumulator and the bias add round once each.  A term of S therefore carries at most
    (K + 2) + (R + 1) + 3 = K + R + 6 roundings of 2^-24 each (to first order); g allows the module's usual 2x margin.  The one rounding
    to T gives u_T (|r| + g S).

Composed path (matmul_4bit + the adapter in torch ops): five roundings to T -- the base, t, u, s u and the sum:
                                      |y - r| <= g S + u_T (1 + 4 u_T) (|r| + 3 S) + a.

A member without an adapter has R = 0 and no adapter term in r and S.
"""
import numpy as np
import torch

from tests.elementwise import UNIT, assert_bound_elementwise


def lora_reference(X, Wd, bias, adapter):
    """(r, S, R) in float64 on X's device; X [M, K], Wd [N, K], bias [N] or None, adapter None or (A [R, K], B [N, R], scaling)."""
    Xd, Wdd = X.double(), Wd.double()
    r = Xd @ Wdd.t()
    S = Xd.abs() @ Wdd.abs().t()
    if bias is not None:
        r = r + bias.double()
        S = S + bias.double().abs()
    R = 0
    if adapter is not None:
        A, B, scaling = adapter
        s = float(np.float32(scaling))
        R = int(A.shape[0])
        r = r + s * ((Xd @ A.double().t()) @ B.double().t())
        S = S + abs(s) * ((Xd.abs() @ A.double().abs().t()) @ B.double().abs().t())
    return r, S, R


def lora_bound(r, S, R, K, w_dtype, path):
    g = (K + R + 6) * 2.0 ** -23
    u = UNIT[w_dtype]
    a = 2.0 ** -24 if w_dtype == torch.float16 else 0.0
    if path == "fused":
        return g * S + u * (r.abs() + g * S) + a
    assert path == "composed", path
    return g * S + u * (1 + 4 * u) * (r.abs() + 3 * S) + a


def assert_lora_elementwise(y, X, Wd, bias, adapter, w_dtype, path, kernel=""):
    """Check one member's output y [..., N] (in w_dtype) element by element; returns the largest err / bound ratio.  The operands
    may live on any device; the comparison runs on y's."""
    y2 = y.reshape(-1, y.shape[-1])
    dev = y2.device
    X2 = X.reshape(-1, X.shape[-1]).to(dev)
    assert y2.dtype == w_dtype, (y2.dtype, w_dtype)
    if adapter is not None:
        adapter = (adapter[0].to(dev), adapter[1].to(dev), adapter[2])
    r, S, R = lora_reference(X2, Wd.to(dev), None if bias is None else bias.to(dev), adapter)
    assert y2.shape == r.shape, (tuple(y.shape), tuple(r.shape))
    return assert_bound_elementwise(y2, r, lora_bound(r, S, R, X2.shape[1], w_dtype, path), kernel, "y = X . Wd^T + b + s (X . A^T) . B^T")

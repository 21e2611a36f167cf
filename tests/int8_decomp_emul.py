"""
numpy / CPU-torch emulation of the numerics contract of libmbnb_sparse.so (include/mbnb_sparse.h), for the GPU tests and for the golden
script (tests/golden/make_golden_int8_decomp.py), which asserts on its own cases that the reference is explained by it.

Col + row INT8, all in f32 with correctly rounded operations (numpy's f32 `*`, `/` are; sqrt is taken in float64 and rounded to f32,
which is the correctly rounded f32 sqrt because 53 >= 2 * 24 + 2):

    rm[i] = max(max_j |x[i, j]|, 1e-8)      cm[j] = max(max_i |x[i, j]|, 1e-8)       (NaN propagates, as torch.max)
    s     = sqrt(rm[i] * cm[j])
    q     = int8(clamp(rint(x * ((1 / s) * 127)), -127, 127)), 0 where the product is NaN
    Wd    = round_T(float(q) * (s / 127))

``lower=True`` evaluates the chain with the next f32 below s: torch's vectorised CPU sqrt is 1 ulp low on about 0.6 % of inputs, and
this is the only deviation of the reference from the chain.
"""
import numpy as np
import torch

F32 = np.float32


def colrow_stats(x: torch.Tensor):
    """(rm [R], cm [C]) as np.float32 from a 2-D CPU tensor of any float dtype."""
    a = np.abs(x.float().numpy())
    with np.errstate(invalid="ignore"):
        return np.maximum(a.max(axis=1), F32(1e-8)), np.maximum(a.max(axis=0), F32(1e-8))


def colrow_scale(rm: np.ndarray, cm: np.ndarray, lower: bool = False) -> np.ndarray:
    with np.errstate(all="ignore"):
        p = rm.astype(F32)[:, None] * cm.astype(F32)[None, :]
        s = np.sqrt(p.astype(np.float64)).astype(F32)
        if lower:
            s = np.nextafter(s, F32(-np.inf), dtype=F32)
    return s


def colrow_codes(x: torch.Tensor, s: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        inv = (F32(1.0) / s) * F32(127.0)
        p = x.float().numpy() * inv
        r = np.clip(np.rint(p), -127.0, 127.0)
        return np.where(np.isnan(p), F32(0.0), r).astype(np.int8)


def colrow_wd(q: np.ndarray, s: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    with np.errstate(all="ignore"):
        f = q.astype(F32) * (s / F32(127.0))
    return torch.from_numpy(f).to(dtype)


def bits(t: torch.Tensor) -> torch.Tensor:
    """The bit patterns of a tensor, every NaN as the dtype's default NaN: the contract says where a NaN is, not which one (0 * Inf is the
    negative default NaN on x86 and the positive one on the GPU, and the conversions to 16 bits keep different payloads)."""
    t = t.detach().contiguous().cpu()
    if t.is_floating_point():
        t = torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t)
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32) if t.dtype == torch.float32 else t


def explained(got: torch.Tensor, exact: torch.Tensor, low: torch.Tensor) -> torch.Tensor:
    """Elementwise: `got` has the bits of the chain with s (`exact`) or with the next f32 below s (`low`).  No other difference passes."""
    g = bits(got)
    return (g == bits(exact)) | (g == bits(low))


# ----------------------------------------------------------------------------- COO
def coo_from_dense(x: torch.Tensor, threshold: float = 0.0):
    """(row int64, col int64, values) of a 2-D CPU tensor by the rule of mbnb_sparse.h; the threshold is compared in x's dtype."""
    xf = x.float()
    if threshold > 0:
        thr = float(torch.tensor(float(threshold), dtype=x.dtype))
        keep = (xf.abs() >= thr) | torch.isnan(xf)
    else:
        keep = xf != 0
    idx = keep.nonzero()
    return idx[:, 0].contiguous(), idx[:, 1].contiguous(), x[keep]


def coo_quantize(values: torch.Tensor):
    """(int8 codes, scale f32 [1]) of quantize_sparse_coo."""
    v = values.float().numpy()
    with np.errstate(all="ignore"):
        scale = np.maximum(np.abs(v).max(), F32(1e-8)) / F32(127.0)
        p = v / scale
        q = np.where(np.isnan(p), F32(0.0), np.clip(np.rint(p), -127.0, 127.0)).astype(np.int8)
    return torch.from_numpy(q), torch.from_numpy(np.asarray([scale], dtype=F32))


def coo_int8_values(q: torch.Tensor, scale: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The values spmm_coo_int8 multiplies: round_T(float(q) * scale) for one scale, round_T(float(q) * float(round_T(scale[e]))) per entry."""
    s = scale.float().reshape(-1)
    if s.numel() != 1:
        s = s.to(dtype).float()
    return (q.float() * s).to(dtype)

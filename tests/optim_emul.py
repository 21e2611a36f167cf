"""
The 8-bit optimizer step as executable numpy: DESIGN.md §10 and include/mbnb_optim.h restated per element in f32, with the
arithmetic pinned down further than the prose does.  Importable without a GPU and without the reference.

- every fma is exact: the f32 product is exact in float64, the sum is rounded to odd in float64 and then once to f32;
- division and sqrt are correctly rounded (numpy's f32 `/` and `np.sqrt`), `np.rint` rounds half to even;
- the 16-bit roundings go through a torch CPU cast (f32 -> f16 / bf16 -> f32, round to nearest even);
- p and g are rounded to the parameter / gradient dtype exactly where §10 says so; Lion's and SGD's alphas are rounded to the
  tensor's dtype first;
- padding elements of a partial block count as 0 in the maxima, the maxima are clamped below at 1e-8 / 1e-12 and taken with fmax
  semantics (a NaN is dropped), a NaN code argument is stored as code 0;
- the host scalars are computed here, in double, from the group's hyperparameters and the tensor's own step count, and rounded
  once to f32 (`host_scalars`); nothing is taken from mps_bitsandbytes_amd/optim/*.py.

tests/test_optim_emul_host.py pins this module to the reference's CPU optimizers through the committed goldens;
tests/test_gpu_optim_elementwise.py holds the HIP kernels to it bit for bit.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

F32 = np.float32
RULES = ("adam", "adamw", "lion", "sgd", "sgd_nesterov")
TWO_MOMENTS = ("adam", "adamw")
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
_ERR = dict(invalid="ignore", divide="ignore", over="ignore", under="ignore")


# ----------------------------------------------------------------------------- number formats
def rnd(x: np.ndarray, dt: str) -> np.ndarray:
    """f32 values rounded (RNE) to dtype `dt` and back."""
    if dt == "f32":
        return x
    return torch.from_numpy(np.ascontiguousarray(x)).to(DT[dt]).float().numpy()


def scalar_in(x: float, dt: str) -> F32:
    """A Python scalar as an op on a tensor of `dt` sees it: double -> f32 -> dt."""
    return F32(rnd(np.array([x], dtype=np.float64).astype(F32), dt)[0])


def fma(a, b, c) -> np.ndarray:
    """a * b + c for f32 operands with ONE rounding.  a * b is exact in float64 (48 significant bits).  The float64 sum is
    rounded to odd: TwoSum gives the rounding error, and an inexact even result is moved to its odd neighbour on the side of
    the error, so the final rounding to f32 cannot be a double rounding."""
    with np.errstate(**_ERR):
        x = np.asarray(a, dtype=F32).astype(np.float64) * np.asarray(b, dtype=F32).astype(np.float64)
        y = np.broadcast_to(np.asarray(c, dtype=F32).astype(np.float64), x.shape)
        s = x + y
        bb = s - x
        err = (x - (s - bb)) + (y - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F32)


def bits(x) -> np.ndarray:
    """The bit patterns of a torch tensor or numpy array as unsigned integers (codes: the uint8 pattern)."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().contiguous()
        if x.dtype in (torch.float16, torch.bfloat16):
            return x.view(torch.int16).numpy().view(np.uint16).reshape(-1)
        x = x.numpy()
    x = np.ascontiguousarray(x).reshape(-1)
    return x.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[x.dtype.itemsize])


def from_bits(b: np.ndarray, dt: str) -> torch.Tensor:
    b = np.ascontiguousarray(b)
    if dt == "f32":
        return torch.from_numpy(b.view(np.int32)).view(torch.float32)
    return torch.from_numpy(b.view(np.int16)).view(DT[dt])


# ----------------------------------------------------------------------------- host scalars
def host_scalars(rule: str, hp: dict, step: int, pdt: str, gdt: str) -> SimpleNamespace:
    """The f32 scalars of one tensor's step, from the group's hyperparameters in double, each rounded once."""
    f = lambda v: F32(np.float64(v))
    lr, wd = float(hp["lr"]), float(hp.get("weight_decay", 0.0))
    s = SimpleNamespace(wd_on=wd != 0)
    if rule in TWO_MOMENTS or rule == "lion":
        b1, b2 = (float(b) for b in hp["betas"])
        s.b1, s.omb1, s.b2, s.omb2 = f(b1), f(1.0 - b1), f(b2), f(1.0 - b2)
        s.decay = f(1.0 - lr * wd)
    if rule in TWO_MOMENTS:
        s.eps, s.wd = f(hp["eps"]), f(wd)
        s.bc2_sqrt = f(math.sqrt(1.0 - math.pow(b2, step)))
        s.neg_step_size = f(-(lr / (1.0 - math.pow(b1, step))))
    elif rule == "lion":
        s.neg_lr = scalar_in(-lr, pdt)
    else:
        s.b1, s.omb1 = f(hp["momentum"]), f(1.0 - float(hp.get("dampening", 0.0)))
        s.wd, s.neg_lr = scalar_in(wd, gdt), scalar_in(-lr, pdt)
    return s


# ----------------------------------------------------------------------------- one step of some blocks
def step_blocks(rule: str, s: SimpleNamespace, pdt: str, gdt: str, p, g, q1, a1, q2=None, a2=None, cnt=None, trace=None):
    """One step of k blocks.  p, g: (k, bs) f32 arrays holding the parameter / gradient values (exact in f32); q1: (k, bs) int8,
    a1: (k,) f32; q2: (k, bs) uint8 and a2: (k,) f32 for the two-moment rules; cnt: (k,) valid elements per block (the rest is
    padding).  Returns (p, q1, a1, q2, a2) after the step, in the same shapes; padding positions hold no meaning.  A dict passed as `trace` receives
    the arguments of the two rint() calls ("r1", "r2"): a value exactly on k + 1/2 there is a rounding tie."""
    assert rule in RULES
    two = rule in TWO_MOMENTS
    p, g = np.asarray(p, dtype=F32), np.asarray(g, dtype=F32)
    k, bs = p.shape
    valid = np.arange(bs)[None, :] < (np.full(k, bs) if cnt is None else np.asarray(cnt))[:, None]
    a1 = np.asarray(a1, dtype=F32)
    with np.errstate(**_ERR):
        m = (q1.astype(F32) / F32(127)) * a1[:, None]
        if two:
            sq = q2.astype(F32) / F32(255)
            v = (sq * sq) * np.asarray(a2, dtype=F32)[:, None]
        if two:
            if rule == "adam" and s.wd_on:
                g = fma(p, s.wd, g)
            if rule == "adamw" and s.wd_on:
                p = rnd(p * s.decay, pdt)
            m = fma(g, s.omb1, m * s.b1)
            v = fma(s.omb2 * g, g, v * s.b2)
            den = np.sqrt(v) / s.bc2_sqrt + s.eps
            u = (m / den) * s.neg_step_size
            p = rnd(p + rnd(u, pdt), pdt)
        elif rule == "lion":
            if s.wd_on:
                p = rnd(p * s.decay, pdt)
            u = fma(g, s.omb1, m * s.b1)
            sg = (u > 0).astype(F32) - (u < 0).astype(F32)
            m = fma(g, s.omb2, m * s.b2)
            p = rnd(fma(sg, s.neg_lr, p), pdt)
        else:
            if s.wd_on:
                g = rnd(fma(p, s.wd, g), gdt)
            m = fma(g, s.omb1, m * s.b1)
            d = fma(m, s.b1, g) if rule == "sgd_nesterov" else m
            p = rnd(fma(rnd(d, pdt), s.neg_lr, p), pdt)
        zero = np.zeros((k, 1), dtype=F32)
        n1 = np.fmax(np.fmax.reduce(np.where(valid, np.abs(m), F32(0)), axis=1, initial=F32(0)), F32(1e-8)).astype(F32)
        x1 = (m / n1[:, None]) * F32(127)
        r = np.rint(x1)
        nq1 = np.where(np.isnan(r), F32(0), np.clip(r, -127, 127)).astype(np.int8)
        nq2 = n2 = None
        if two:
            vp = np.fmax(v, zero)
            n2 = np.fmax(np.fmax.reduce(np.where(valid, vp, F32(0)), axis=1, initial=F32(0)), F32(1e-12)).astype(F32)
            x2 = np.sqrt(vp / n2[:, None]) * F32(255)
            r = np.rint(x2)
            nq2 = np.where(np.isnan(r), F32(0), np.clip(r, 0, 255)).astype(np.uint8)
    if trace is not None:
        trace.update(r1=x1, r2=x2 if two else None, valid=valid)
    return p, nq1, n1, nq2, n2


def n_blocks(numel: int, bs: int) -> int:
    return (numel + bs - 1) // bs


class EmuTensor:
    """One parameter and its 8-bit state on the host, stepped by the emulation."""

    def __init__(self, rule: str, hp: dict, p: torch.Tensor, block_size: int):
        self.rule, self.hp, self.bs = rule, dict(hp), int(block_size)
        self.pdt = {v: k for k, v in DT.items()}[p.dtype]
        self.shape = tuple(p.shape)
        self.p = p.detach().cpu().reshape(-1).clone()
        n, nb = self.p.numel(), n_blocks(p.numel(), self.bs)
        self.q1, self.a1 = np.zeros(n, np.int8), np.full(nb, 1e-8, F32)
        self.q2, self.a2 = (np.zeros(n, np.uint8), np.full(nb, 1e-12, F32)) if rule in TWO_MOMENTS else (None, None)
        self.step_count = 0
        self.before = None

    def _gather(self, x, blocks, dtype):
        """(len(blocks), bs) array of the chosen blocks of flat `x`, zero padded."""
        n, bs = len(x), self.bs
        if len(blocks) and blocks[-1] - blocks[0] == len(blocks) - 1:       # a contiguous run
            lo, hi = int(blocks[0]) * bs, min(n, (int(blocks[-1]) + 1) * bs)
            out = np.zeros(len(blocks) * bs, dtype=dtype)
            out[:hi - lo] = x[lo:hi]
            return out.reshape(len(blocks), bs)
        out = np.zeros((len(blocks), bs), dtype=dtype)
        for i, b in enumerate(blocks):
            seg = x[int(b) * bs:(int(b) + 1) * bs]
            out[i, :len(seg)] = seg
        return out

    def _scatter(self, x, blocks, new, cnt):
        bs = self.bs
        if len(blocks) and blocks[-1] - blocks[0] == len(blocks) - 1:
            lo = int(blocks[0]) * bs
            k = int(cnt.sum())
            x[lo:lo + k] = new.reshape(-1)[:k]      # only the last block of a run can be partial
            return
        for i, b in enumerate(blocks):
            c, lo = int(cnt[i]), int(b) * bs
            x[lo:lo + c] = new[i, :c]

    def step(self, g: torch.Tensor, blocks=None, chunk_elems: int = 1 << 20, trace=None):
        """One step with gradient g (a torch tensor of the parameter's dtype or f32), over all blocks or the chosen ones."""
        n, nb = self.p.numel(), len(self.a1)
        gdt = {v: k for k, v in DT.items()}[g.dtype]
        g = g.detach().cpu().reshape(-1)
        assert g.numel() == n
        self.step_count += 1
        s = host_scalars(self.rule, self.hp, self.step_count, self.pdt, gdt)
        if n == 0:
            return
        self.before = dict(p=bits(self.p).copy(), g=bits(g).copy(), q1=self.q1.copy(), a1=self.a1.copy(),
                           q2=None if self.q2 is None else self.q2.copy(), a2=None if self.a2 is None else self.a2.copy())
        pf, gf = self.p.float().numpy(), g.float().numpy()
        newp = pf.copy()
        todo = np.arange(nb) if blocks is None else np.asarray(blocks, dtype=np.int64)
        per = max(1, chunk_elems // self.bs)
        for c0 in range(0, len(todo), per):
            bl = todo[c0:c0 + per]
            cnt = np.minimum(self.bs, n - bl * self.bs)
            Q2 = self._gather(self.q2, bl, np.uint8) if self.q2 is not None else None
            A2 = self.a2[bl] if self.a2 is not None else None
            np_, nq1, na1, nq2, na2 = step_blocks(self.rule, s, self.pdt, gdt, self._gather(pf, bl, F32), self._gather(gf, bl, F32),
                                                  self._gather(self.q1, bl, np.int8), self.a1[bl], Q2, A2, cnt, trace)
            self._scatter(newp, bl, np_, cnt)
            self._scatter(self.q1, bl, nq1, cnt)
            self.a1[bl] = na1
            if nq2 is not None:
                self._scatter(self.q2, bl, nq2, cnt)
                self.a2[bl] = na2
        self.p = torch.from_numpy(newp).to(self.p.dtype)

    def result(self) -> dict:
        out = dict(p=self.p, q1=self.q1, a1=self.a1)
        if self.q2 is not None:
            out.update(q2=self.q2, a2=self.a2)
        return out


def gather_blocks(blocks, block_size: int, numel: int, p, g, q1, a1, q2=None, a2=None) -> dict:
    """The chosen blocks of one large tensor, brought to the host: p, g, q1 (q2) as (k, bs) CPU tensors (positions past the
    tensor's end repeat its last element and are masked by "cnt"), a1 (a2) as (k,).  The arguments are flat tensors on any device."""
    bs = int(block_size)
    dev = p.device
    b = torch.as_tensor(np.asarray(blocks, dtype=np.int64), device=dev)
    idx = (b[:, None] * bs + torch.arange(bs, device=dev)[None, :]).clamp_(max=numel - 1)
    out = dict(cnt=np.minimum(bs, numel - np.asarray(blocks, dtype=np.int64) * bs))
    for name, t in (("p", p), ("g", g), ("q1", q1), ("q2", q2)):
        out[name] = None if t is None else t.reshape(-1)[idx].cpu()
    for name, t in (("a1", a1), ("a2", a2)):
        out[name] = None if t is None else t[b].cpu()
    return out


def step_gathered(rule: str, hp: dict, step: int, pdt: str, gdt: str, before: dict) -> dict:
    """One step of the blocks of gather_blocks(): blocks are independent, so this is the whole-tensor step restricted to them."""
    s = host_scalars(rule, hp, step, pdt, gdt)
    two = before["q2"] is not None
    p, q1, a1, q2, a2 = step_blocks(rule, s, pdt, gdt, before["p"].float().numpy(), before["g"].float().numpy(), before["q1"].numpy(),
                                    before["a1"].numpy(), before["q2"].numpy() if two else None, before["a2"].numpy() if two else None,
                                    before["cnt"])
    return dict(p=torch.from_numpy(np.ascontiguousarray(p)).to(DT[pdt]), q1=q1, a1=a1, q2=q2, a2=a2)


def compare_gathered(tag: str, blocks, got: dict, want: dict, before: dict, pdt: str) -> None:
    """compare() over gathered blocks: positions past a partial block's end are not part of the tensor and are ignored."""
    cnt = before["cnt"]
    bs = before["q1"].shape[1]
    valid = np.arange(bs)[None, :] < cnt[:, None]
    g2 = {}
    for k in ("p", "q1", "q2", "a1", "a2"):
        if want.get(k) is None:
            continue
        gv = got[k]
        if k in ("a1", "a2"):
            g2[k] = gv
            continue
        wb = bits(want[k]).reshape(valid.shape)
        gb = np.where(valid, bits(gv).reshape(valid.shape), wb)
        g2[k] = gb.astype(wb.dtype)
    w2 = {k: (bits(v) if k in ("p", "q1", "q2") else v) for k, v in want.items() if v is not None}
    ops = {k: before[k] for k in ("p", "g", "q1", "a1", "q2", "a2") if before.get(k) is not None}
    compare(tag, g2, w2, bs, pdt, ops, block_ids=np.asarray(blocks))


# ----------------------------------------------------------------------------- the comparator
class Guarded:
    """A result that lives inside a filled buffer: `buf` (uint8 numpy array of the whole buffer), the byte offset and byte
    length of the view, the view's numpy dtype.  The comparator also requires every byte outside the view to keep `fill`."""

    def __init__(self, buf, start, nbytes, dtype, fill=0xFF):
        self.buf, self.start, self.nbytes, self.dtype, self.fill = np.asarray(buf, dtype=np.uint8), start, nbytes, dtype, fill

    def view(self):
        return self.buf[self.start:self.start + self.nbytes].view(self.dtype)


def _is_nan_bits(b: np.ndarray, dt: str) -> np.ndarray:
    if dt == "f32":
        return (b & 0x7FFFFFFF) > 0x7F800000
    if dt == "f16":
        return (b & 0x7FFF) > 0x7C00
    return (b & 0x7FFF) > 0x7F80


def compare(tag: str, got: dict, want: dict, block_size: int, pdt: str, operands: dict = None, block_ids=None) -> None:
    """got / want: {"p", "q1", "a1"[, "q2", "a2"]}: tensors, arrays or (got only) Guarded views.  Every element must have the
    emulation's bits, except that where the emulation holds a NaN any NaN will do.  A Guarded result must also leave its guard
    bytes untouched.  The first mismatch raises with the tensor, the block, the element, both bit patterns and the operands of
    that element before the step (`operands`: the same keys plus "g", bit patterns / codes, as EmuTensor.before).
    `block_ids`: the tensor's block behind each block of the arrays, when they hold selected blocks only."""
    fdt = dict(p=pdt, a1="f32", a2="f32")
    for key in ("p", "q1", "a1", "q2", "a2"):
        if want.get(key) is None:
            continue
        gv = got[key]
        if isinstance(gv, Guarded):
            out = np.ones(len(gv.buf), dtype=bool)
            out[gv.start:gv.start + gv.nbytes] = False
            bad = np.flatnonzero(out & (gv.buf != gv.fill))
            if bad.size:
                off = int(bad[0]) - gv.start
                where = f"{-off} bytes before the view" if off < 0 else f"{off - gv.nbytes} bytes past its end"
                raise AssertionError(f"{tag}: {key}: guard byte written {where}: 0x{int(gv.buf[bad[0]]):02x} "
                                     f"(element {off // np.dtype(gv.dtype).itemsize} of a view of {gv.nbytes // np.dtype(gv.dtype).itemsize})")
            gv = gv.view()
        gb, wb = bits(gv), bits(want[key])
        assert gb.shape == wb.shape and gb.dtype == wb.dtype, f"{tag}: {key}: got {gb.shape} {gb.dtype}, want {wb.shape} {wb.dtype}"
        diff = gb != wb
        if key in fdt:
            wn = _is_nan_bits(wb, fdt[key])
            diff = np.where(wn, ~_is_nan_bits(gb, fdt[key]), diff)
        bad = np.flatnonzero(diff)
        if not bad.size:
            continue
        i = int(bad[0])
        per_block = key in ("a1", "a2")
        blk = i if per_block else i // block_size
        w = gb.dtype.itemsize * 2
        msg = (f"{tag}: {key}: {bad.size} of {gb.size} differ; first at "
               f"{'block' if per_block else 'element'} {i} (block {blk}, offset {0 if per_block else i % block_size}): "
               f"got 0x{int(gb[i]):0{w}x}, want 0x{int(wb[i]):0{w}x}")
        if block_ids is not None:
            msg += f" (block {blk} here is block {int(block_ids[blk])} of the tensor)"
        if operands:
            ops = []
            for k2, arr in operands.items():
                if arr is None:
                    continue
                arr = bits(arr)
                j = blk if k2 in ("a1", "a2") else i
                if per_block:      # a maximum: show the block's maxima before the step, not one element
                    if k2 in ("a1", "a2"):
                        ops.append(f"{k2}=0x{int(arr[j]):08x}")
                    continue
                if j < arr.size:
                    ops.append(f"{k2}=0x{int(arr[j]):0{arr.dtype.itemsize * 2}x}")
            msg += "; operands before the step: " + " ".join(ops)
        raise AssertionError(msg)

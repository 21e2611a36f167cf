"""
Paged optimizers (reference: mps_bitsandbytes/optim/paged.py): PagedAdamW, PagedAdam, PagedLion.

Full-precision moments in the parameter's dtype (the reference's state: `step`, `exp_avg`, `exp_avg_sq`), stepped by one fused HIP
kernel (csrc/paged_kernels.hip, libmbnb_paged.so) that restates the reference's chain of tensor ops bit for bit.

page_to_cpu=False   the moments live on the parameter's device; one launch per 48 tensors of a group and dtype.
page_to_cpu=True    the moments live in pinned host memory and never as a whole on the device.  A step cuts the group's elements
                    into pages of at most `_page_elems` elements (plan_pages) and sends them through a ring of `_slots` device
                    staging slots: page-in on a copy-in stream, the kernel on the caller's current stream, page-out on a copy-out
                    stream, ordered by events alone, so the copies of neighbouring pages overlap a page's kernel.  A step never
                    waits on the host; synchronize() does, and state_dict() calls it.

Parameters must be on a ROCm ('cuda') device; there is no CPU path.  A gradient has its parameter's dtype.
"""
from collections import defaultdict
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from .. import _native, _paged_native
from ._base import FusedOptimizer, check_hyper, f32, in_dtype

PAGE_ALIGN = 8             # elements: every segment starts on a multiple of 8 elements of its tensor (16 bytes of a 16-bit dtype)
_MOMENTS = ("exp_avg", "exp_avg_sq")


def plan_pages(numels: Sequence[int], page_elems: int) -> List[List[Tuple[int, int, int]]]:
    """Cut tensors of `numels` elements, in order, into pages.  Returns, per page, its segments (tensor index, start, count): every
    element of every tensor exactly once, in order; every start a multiple of PAGE_ALIGN; a tensor larger than what is left of a
    page continues on the next one, small tensors share a page.  A segment takes its count rounded up to PAGE_ALIGN of a page's
    `page_elems` (so that each starts 16-byte aligned in a staging slot too); empty tensors take nothing."""
    page_elems = int(page_elems)
    if page_elems < PAGE_ALIGN or page_elems % PAGE_ALIGN:
        raise ValueError(f"page_elems must be a positive multiple of {PAGE_ALIGN}, got {page_elems}")
    pages, page, room = [], [], page_elems
    for i, n in enumerate(numels):
        start, n = 0, int(n)
        while start < n:
            if room == 0:
                pages.append(page)
                page, room = [], page_elems
            count = min(room, n - start)
            page.append((i, start, count))
            start += count
            room -= -(-count // PAGE_ALIGN) * PAGE_ALIGN
    if page:
        pages.append(page)
    return pages


# two extra streams per device for the whole process, shared by every paged optimizer: with the caller's stream they stay under the
# four hardware queues a process opens by default
_STREAMS: Dict[int, Tuple["torch.cuda.Stream", "torch.cuda.Stream"]] = {}


def _copy_streams(device: torch.device):
    idx = torch.cuda.current_device() if device.index is None else device.index
    if idx not in _STREAMS:
        _STREAMS[idx] = (torch.cuda.Stream(device=idx), torch.cuda.Stream(device=idx))
    return _STREAMS[idx]


def _pinned_like(p: torch.Tensor, src: Optional[torch.Tensor] = None) -> torch.Tensor:
    t = torch.empty(p.shape, dtype=p.dtype, device="cpu", pin_memory=torch.cuda.is_available())
    return t.zero_() if src is None else t.copy_(src.detach().reshape(p.shape))


class _Ring:
    """The staging slots of one device: per slot one buffer per moment and the three events of the page it holds."""

    def __init__(self, device, slots: int, slot_bytes: int, moments: int):
        self.slot_bytes, self.moments = slot_bytes, moments
        self.bufs = [[torch.empty(slot_bytes, dtype=torch.uint8, device=device) for _ in range(moments)] for _ in range(slots)]
        cur = torch.cuda.current_stream(device)
        for s in _copy_streams(device):
            s.wait_stream(cur)                     # the allocator may hand out memory that work on the current stream still uses
            for slot in self.bufs:
                for b in slot:
                    b.record_stream(s)
        self.in_done = [torch.cuda.Event() for _ in range(slots)]
        self.k_done = [torch.cuda.Event() for _ in range(slots)]
        self.out_done = [torch.cuda.Event() for _ in range(slots)]
        self.used = [False] * slots
        self.next = 0


class _PagedBase(FusedOptimizer):
    _name = "PagedOptimizer"
    _f32_grads = False     # a gradient has its parameter's dtype
    _kind = _paged_native.ADAMW
    _moments = 2
    _page_elems = 1 << 26  # elements per page (chosen from tools/paged_bench.py's sweep)
    _slots = 3             # staging slots: one page in, one under the kernel, one out
    _step_flags = 0        # mbnb_paged_step flags (tests set FORCE_SCALAR to compare the two kernel paths)

    def _init_paging(self):
        self._rings: Dict[torch.device, _Ring] = {}
        self._last_out: Dict[torch.device, "torch.cuda.Event"] = {}

    # ------------------------------------------------------------------ state
    def synchronize(self):
        """Wait until every page-out of earlier steps has reached the host.  Call before reading the state."""
        for ev in self.__dict__.get("_last_out", {}).values():
            ev.synchronize()

    def state_dict(self):
        self.synchronize()
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        # torch.optim.Optimizer.load_state_dict moves every state tensor to the parameter's device; bring the moments of a paged
        # group back into pinned host memory, and never share a tensor with the optimizer the dict came from.  Where the moments
        # live belongs to this optimizer, not to the checkpoint: each group keeps its own page_to_cpu.
        self.synchronize()
        saved = {id(v) for st in state_dict["state"].values() for v in st.values() if isinstance(v, torch.Tensor)}
        mine = [g["page_to_cpu"] for g in self.param_groups]
        super().load_state_dict(state_dict)
        for group, page_to_cpu in zip(self.param_groups, mine):
            group["page_to_cpu"] = page_to_cpu
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if not st:
                    continue
                for k in _MOMENTS[:self._moments]:
                    if isinstance(st.get(k), torch.Tensor):
                        t = self._home(st[k], p, group["page_to_cpu"])
                        st[k] = t.clone() if id(t) in saved else t
                if isinstance(st.get("step"), torch.Tensor):
                    st["step"] = int(st["step"].item())

    def _home(self, t: torch.Tensor, p: torch.Tensor, paged: bool) -> torch.Tensor:
        """`t` as a moment of `p` where the group keeps it: pinned host memory or p's device, contiguous, in p's dtype."""
        if t.numel() != p.numel() or t.dtype != p.dtype:
            raise ValueError(f"{self._name}: optimizer state of {t.numel()} {t.dtype} elements does not fit a parameter of shape "
                             f"{tuple(p.shape)} and dtype {p.dtype} (state from another model?)")
        if paged:
            # (an empty tensor has no memory to pin and never reports itself pinned)
            if t.device.type == "cpu" and t.is_contiguous() and (t.is_pinned() or t.numel() == 0 or not torch.cuda.is_available()):
                return t
            return _pinned_like(p, t)
        if t.device == p.device and t.is_contiguous():
            return t
        return t.detach().reshape(p.shape).to(device=p.device).contiguous()

    def _moment_tensors(self, p, state, paged: bool):
        if len(state) == 0:
            if self._moments == 2:
                state["step"] = 0
            for k in _MOMENTS[:self._moments]:
                # contiguous whatever p's strides are: the kernel walks the moments in the order of p's contiguous elements
                state[k] = _pinned_like(p) if paged else torch.zeros(p.shape, dtype=p.dtype, device=p.device)
        out = []
        for k in _MOMENTS[:self._moments]:
            t = state.get(k)
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{self._name}: optimizer state {k!r} missing for a parameter of shape {tuple(p.shape)}")
            h = self._home(t, p, paged)
            if h is not t:
                self.synchronize()
                state[k] = h
            out.append(h)
        return out

    # ------------------------------------------------------------------ the step
    def _run(self, group, items: List[tuple], scalars_for) -> None:
        """items: (param, [moments], bc2_sqrt, neg_step_size) per parameter with a gradient."""
        paged = bool(group["page_to_cpu"])
        buckets: Dict[tuple, list] = defaultdict(list)
        for it in items:
            buckets[(it[0].device, it[0].dtype)].append(it)
        for (dev, dt), its in buckets.items():
            staged, writeback = self._stage([it[0] for it in its])
            work = [(w, g, moments, bc2, nss) for (w, g), (_, moments, bc2, nss) in zip(staged, its)]
            with _native.on_device(dev):
                if paged:
                    self._step_paged(dev, dt, work, scalars_for(dt))
                else:
                    segs = [(w.data_ptr(), g.data_ptr(), ms[0].data_ptr(), ms[1].data_ptr() if len(ms) > 1 else 0, w.numel(), bc2, nss)
                            for w, g, ms, bc2, nss in work]
                    _paged_native.step(self._kind, dt, scalars_for(dt), segs, _native.stream_ptr(dev), self._step_flags)
            self._unstage(writeback)

    def _ring(self, dev) -> _Ring:
        page = int(self._page_elems)
        if page < PAGE_ALIGN or page % PAGE_ALIGN:
            raise ValueError(f"{self._name}: _page_elems must be a positive multiple of {PAGE_ALIGN}, got {page}")
        mine = [p for g in self.param_groups for p in g["params"] if p.device == dev]
        esize = max(p.element_size() for p in mine)
        page = min(page, sum(-(-p.numel() // PAGE_ALIGN) * PAGE_ALIGN for p in mine))     # a small model never fills a page
        ring = self._rings.get(dev)
        if ring is None or ring.slot_bytes != page * esize or len(ring.bufs) != self._slots:
            ring = self._rings[dev] = _Ring(dev, self._slots, page * esize, self._moments)
        return ring

    def _step_paged(self, dev, dt, work, scalars) -> None:
        ring = self._ring(dev)
        s_in, s_out = _copy_streams(dev)
        cur = torch.cuda.current_stream(dev)
        esize = work[0][0].element_size()
        host = [[m.view(-1) for m in ms] for _, _, ms, _, _ in work]
        if dev in self._last_out:
            s_in.wait_event(self._last_out[dev])            # this step's page-ins read what the last step's page-outs wrote
        for page in plan_pages([w.numel() for w, *_ in work], self._page_elems):
            k = ring.next
            ring.next = (k + 1) % len(ring.bufs)
            slot = [b.view(dt) for b in ring.bufs[k]]
            if ring.used[k]:
                s_in.wait_event(ring.out_done[k])           # the slot is free once its last page has left it
            segs, off = [], 0
            with torch.cuda.stream(s_in):
                for ti, start, count in page:
                    for j, m in enumerate(host[ti]):
                        slot[j][off:off + count].copy_(m[start:start + count], non_blocking=True)
                    w, g, _, bc2, nss = work[ti]
                    segs.append((w.data_ptr() + start * esize, g.data_ptr() + start * esize, slot[0].data_ptr() + off * esize,
                                 slot[1].data_ptr() + off * esize if len(slot) > 1 else 0, count, bc2, nss, ti, start, off))
                    off += -(-count // PAGE_ALIGN) * PAGE_ALIGN
                ring.in_done[k].record(s_in)
            cur.wait_event(ring.in_done[k])
            _paged_native.step(self._kind, dt, scalars, [s[:7] for s in segs], _native.stream_ptr(dev), self._step_flags)
            ring.k_done[k].record(cur)
            s_out.wait_event(ring.k_done[k])
            with torch.cuda.stream(s_out):
                for *_, count, _, _, ti, start, off in segs:
                    for j, m in enumerate(host[ti]):
                        m[start:start + count].copy_(slot[j][off:off + count], non_blocking=True)
                ring.out_done[k].record(s_out)
            ring.used[k] = True
            self._last_out[dev] = ring.out_done[k]


class PagedAdamW(_PagedBase):
    """
    Paged AdamW optimizer that offloads states to CPU.

    Optimizer states (m, v) are stored in pinned host memory and pass through a fixed ring of device staging slots during the
    step, so the device holds the slots, not the moments, whatever the model's size.

    Args:
        params: Iterable of parameters to optimize
        lr: Learning rate (default: 1e-3)
        betas: Coefficients for computing running averages (default: (0.9, 0.999))
        eps: Term added to denominator for numerical stability (default: 1e-8)
        weight_decay: Weight decay coefficient (default: 1e-2)
        page_to_cpu: Whether to offload states to CPU (default: True)
    """
    _name = "PagedAdamW"
    _kind = _paged_native.ADAMW
    _moments = 2

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, page_to_cpu: bool = True):
        check_hyper(lr=lr, eps=eps, betas=betas, weight_decay=weight_decay)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, page_to_cpu=page_to_cpu)
        super().__init__(params, defaults)
        self._init_paging()

    @torch.no_grad()
    def step(self, closure: Optional[Callable] = None):
        """Performs a single optimization step."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            beta1, beta2 = group['betas']
            lr, wd, eps = group['lr'], group['weight_decay'], group['eps']
            items = []
            for p in self._grads(group):
                state = self.state[p]
                moments = self._moment_tensors(p, state, bool(group['page_to_cpu']))
                state['step'] += 1
                step = state['step']
                # the reference's host scalars, in double, each rounded once to f32 where the tensor op meets it
                bias_correction1 = 1 - beta1 ** step
                bias_correction2 = 1 - beta2 ** step
                step_size = lr / bias_correction1
                items.append((p, moments, f32(bias_correction2 ** 0.5), f32(-step_size)))
            if not items:
                continue
            flags = _paged_native.WEIGHT_DECAY if wd != 0 else 0
            self._run(group, items, lambda dt: _paged_native.Scalars(
                f32(beta1), in_dtype(1 - beta1, dt), f32(beta2), f32(1 - beta2), f32(eps), in_dtype(wd, dt), f32(1 - lr * wd), 0.0,
                flags, 0))
        return loss


class PagedAdam(PagedAdamW):
    """
    Paged Adam optimizer (L2 weight decay, not decoupled).

    Same as PagedAdamW but with L2 regularization applied to gradients
    instead of decoupled weight decay.
    """
    _name = "PagedAdam"
    _kind = _paged_native.ADAM

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0, page_to_cpu: bool = True):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, page_to_cpu=page_to_cpu)


class PagedLion(_PagedBase):
    """
    Paged Lion optimizer that offloads momentum to CPU.

    Lion only has one momentum state, making paging even more efficient.

    Args:
        params: Iterable of parameters to optimize
        lr: Learning rate (default: 1e-4)
        betas: Coefficients for computing running averages (default: (0.9, 0.99))
        weight_decay: Weight decay coefficient (default: 0)
        page_to_cpu: Whether to offload states to CPU (default: True)
    """
    _name = "PagedLion"
    _kind = _paged_native.LION
    _moments = 1

    def __init__(self, params, lr: float = 1e-4, betas: Tuple[float, float] = (0.9, 0.99), weight_decay: float = 0,
                 page_to_cpu: bool = True):
        check_hyper(lr=lr, betas=betas)
        defaults = dict(lr=lr, betas=betas, weight_decay=weight_decay, page_to_cpu=page_to_cpu)
        super().__init__(params, defaults)
        self._init_paging()

    @torch.no_grad()
    def step(self, closure: Optional[Callable] = None):
        """Performs a single optimization step."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            beta1, beta2 = group['betas']
            lr, wd = group['lr'], group['weight_decay']
            items = [(p, self._moment_tensors(p, self.state[p], bool(group['page_to_cpu'])), 0.0, 0.0) for p in self._grads(group)]
            if not items:
                continue
            flags = _paged_native.WEIGHT_DECAY if wd != 0 else 0
            self._run(group, items, lambda dt: _paged_native.Scalars(
                f32(beta1), in_dtype(1 - beta1, dt), f32(beta2), in_dtype(1 - beta2, dt), 0.0, 0.0, f32(1 - lr * wd),
                in_dtype(-lr, dt), flags, 0))
        return loss

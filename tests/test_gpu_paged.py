"""
The paged optimizers (libmbnb_paged.so, optim/paged.py) on the GPU.

- the kernel against the numpy emulation (tests/paged_emul.py, pinned to the reference by tests/test_paged_host.py): every rule x dtype at
  zero tolerance on every element, chained over four steps from its own state, on both kernel paths (16-byte vectors; element by element);
- parameters, gradients and moments inside 0xFF guard bands, aligned, all 2 bytes (one f32 element) off alignment (vector body with a
  scalar head and tail) and parameter and gradient alone off alignment (the element path);
- paging against the resident step and the emulation, bit for bit: page boundaries, more pages than slots, more than 48 segments on a
  page, two dtypes in a group, two groups, missing gradients, five steps without a host synchronisation in between;
- the state through state_dict / load_state_dict in both directions, and the device memory the paging holds.
"""
import copy

import numpy as np
import pytest
import torch

import mps_bitsandbytes_amd as bnb
from mps_bitsandbytes_amd import _native, _paged_native as pn, synthetic
from tests import paged_emul as emul
from tests.guard import GuardedTorch

pytestmark = pytest.mark.gpu

DT = emul.DT
CLS = {"adam": "PagedAdam", "adamw": "PagedAdamW", "lion": "PagedLion"}
HP = {"adam": dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01),
      "adamw": dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2),
      "lion": dict(lr=1e-2, betas=(0.9, 0.99), weight_decay=0.1)}
SIZES = [1, 7, 31, 33, 257, 1000, 4096 + 3, 40000]      # 40000: past the reference's 32768 small / large split


def _param(n, dt, seed):
    return torch.nn.Parameter(synthetic.normal((n,), DT[dt], seed=seed).cuda())


def _grad(n, dt, seed):
    return synthetic.normal((n,), DT[dt], seed=seed)


def _same(tag, got: torch.Tensor, want: torch.Tensor):
    g, w = emul.bits(got), emul.bits(want)
    bad = np.flatnonzero(g != w)
    assert not bad.size, f"{tag}: {bad.size} of {g.size} differ; first at {bad[0]}: got 0x{int(g[bad[0]]):x}, want 0x{int(w[bad[0]]):x}"


def _moments(opt, p):
    st = opt.state[p]
    return st["exp_avg"], st.get("exp_avg_sq")


# ----------------------------------------------------------------------------- the kernel against the emulation
@pytest.mark.parametrize("flags", [0, pn.FORCE_SCALAR], ids=["vector", "scalar"])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("rule", emul.RULES)
def test_kernel_matches_the_emulation_on_every_element(rule, dt, flags):
    hp = HP[rule]
    params = [_param(n, dt, 100 + i) for i, n in enumerate(SIZES)]
    emus = [emul.EmuTensor(rule, hp, p) for p in params]
    opt = getattr(bnb, CLS[rule])(params, page_to_cpu=False, **hp)
    opt._step_flags = flags
    for s in range(1, 5):
        for i, (p, e) in enumerate(zip(params, emus)):
            g = _grad(p.numel(), dt, 1000 * s + i)
            p.grad = g.cuda()
            e.step(g)
        opt.step()
        for i, (p, e) in enumerate(zip(params, emus)):
            m, v = _moments(opt, p)
            assert m.device == p.device and m.dtype == p.dtype and m.shape == p.shape
            _same(f"{rule} {dt} numel {SIZES[i]} step {s} p", p, e.p)
            _same(f"{rule} {dt} numel {SIZES[i]} step {s} exp_avg", m, e.m)
            if e.v is not None:
                _same(f"{rule} {dt} numel {SIZES[i]} step {s} exp_avg_sq", v, e.v)
    assert "step" not in opt.state[params[0]] if rule == "lion" else opt.state[params[0]]["step"] == 4


def test_one_launch_per_48_tensors_and_dtype():
    params = [_param(8, "bf16", i) for i in range(50)] + [_param(8, "f32", 99)]
    for p in params:
        p.grad = torch.ones_like(p)
    params[3].grad = None
    opt = bnb.PagedAdamW(params, page_to_cpu=False)
    pn.reset_launch_log()
    opt.step()
    assert pn.launch_log == [(pn.ADAMW, torch.bfloat16, 48), (pn.ADAMW, torch.bfloat16, 1), (pn.ADAMW, torch.float32, 1)]
    assert len(opt.state[params[3]]) == 0 and opt.state[params[4]]["step"] == 1


# ----------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("layout", ["aligned", "all_off", "param_grad_off"])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("rule", emul.RULES)
def test_guarded_buffers_and_misalignment(rule, dt, layout):
    """A direct library call on buffers inside 0xFF guard bands.  `all_off`: every pointer 2 bytes (f32: one element) past a 16-byte
    boundary, so the body still moves in vectors behind a scalar head; `param_grad_off`: parameter and gradient alone, so the whole
    segment goes element by element."""
    hp, two = HP[rule], rule in emul.TWO_MOMENTS
    off = 0 if layout == "aligned" else (4 if dt == "f32" else 2)
    moff = off if layout == "all_off" else 0
    gt = GuardedTorch()
    gt.begin(0xFF, where=f"paged step {rule} {dt} {layout}")
    segs, emus, views = [], [], []
    for i, n in enumerate((1000, 4096 + 3, 5)):
        p0, g0 = synthetic.normal((n,), DT[dt], seed=7 + i), _grad(n, dt, 70 + i)
        m0 = synthetic.normal((n,), DT[dt], seed=170 + i, std=0.1)
        v0 = (synthetic.normal((n,), torch.float64, seed=270 + i, std=0.1) ** 2).to(DT[dt])
        p, g = gt.place(f"param{i}", p0.cuda(), off), gt.place(f"grad{i}", g0.cuda(), off)
        m = gt.place(f"exp_avg{i}", m0.cuda(), moff)
        v = gt.place(f"exp_avg_sq{i}", v0.cuda(), moff) if two else None
        segs.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr() if two else 0, n, 0.0, 0.0))
        emus.append((p0, g0, m0, v0 if two else None))
        views.append((p, g, m, v))
    step_no = 3
    sc = emul.host_scalars(rule, hp, step_no, dt)
    if two:
        segs = [s[:5] + (float(sc.bc2_sqrt), float(sc.neg_step_size)) for s in segs]
        scal = pn.Scalars(*map(float, (sc.b1, sc.omb1, sc.b2, sc.omb2, sc.eps, sc.wd, sc.decay, 0.0)), pn.WEIGHT_DECAY, 0)
    else:
        scal = pn.Scalars(*map(float, (sc.b1, sc.omb1, sc.b2, sc.omb2, 0.0, 0.0, sc.decay, sc.neg_lr)), pn.WEIGHT_DECAY, 0)
    pn.step({"adam": pn.ADAM, "adamw": pn.ADAMW, "lion": pn.LION}[rule], DT[dt], scal, segs, _native.stream_ptr(torch.device("cuda")))
    torch.cuda.synchronize()
    gt.check()
    for i, ((p0, g0, m0, v0), (p, g, m, v)) in enumerate(zip(emus, views)):
        wp, wm, wv = emul.step_tensors(rule, hp, step_no, p0, g0, m0, v0)
        _same(f"{rule} {dt} {layout} segment {i} p", p, wp)
        _same(f"{rule} {dt} {layout} segment {i} exp_avg", m, wm)
        _same(f"{rule} {dt} {layout} segment {i} grad (read only)", g, g0)
        if two:
            _same(f"{rule} {dt} {layout} segment {i} exp_avg_sq", v, wv)


def test_non_contiguous_and_misaligned_parameters_go_through_a_copy():
    base = synthetic.normal((64, 48), torch.bfloat16, seed=3)
    flat = synthetic.normal((1001,), torch.bfloat16, seed=4)
    pt = torch.nn.Parameter(base.cuda().t())                       # non-contiguous
    pm = torch.nn.Parameter(flat.cuda()[1:])                       # 2 bytes off alignment
    gt_, gm = _grad(64 * 48, "bf16", 5).reshape(48, 64), _grad(1000, "bf16", 6)
    pt.grad, pm.grad = gt_.cuda(), gm.cuda()
    opt = bnb.PagedAdamW([pt, pm], lr=1e-2)
    opt._page_elems = 2048
    opt.step()
    opt.synchronize()
    for p, p0, g in ((pt, base.t().contiguous(), gt_), (pm, flat[1:], gm)):
        e = emul.EmuTensor("adamw", HP["adamw"], p0)
        e.step(g)
        _same("parameter", p.detach().contiguous(), e.p)
        _same("exp_avg", opt.state[p]["exp_avg"], e.m)
        assert opt.state[p]["exp_avg"].shape == p.shape and opt.state[p]["exp_avg"].is_pinned()


def test_a_gradient_of_another_dtype_is_refused():
    p = _param(64, "bf16", 1)
    p.grad_dtype = None
    p.grad = torch.zeros(64, device="cuda")
    opt = bnb.PagedAdamW([p])
    with pytest.raises(TypeError, match="gradient must have the parameter's dtype"):
        opt.step()
    assert len(opt.state[p]) == 0


# ----------------------------------------------------------------------------- paging against the resident step
PAGE = 2048
# (dtype, numel, steps without a gradient) per tensor, in two groups
GROUPS = [
    [("f32", PAGE, ()), ("f32", PAGE + 1, ()), ("bf16", 5 * PAGE - 5, ()), ("f32", 300, (2, 3))],     # ends on a page boundary; one past it; five pages
    [("bf16", 8, ())] * 60 + [("f16", 1000, (1,)), ("bf16", 0, ())],                                  # more than 48 segments on one page
]


def _run_paged_model(rule, page_to_cpu, page_elems, steps=5, snapshot_at=None):
    hp = HP[rule]
    groups, flat = [], []
    for gi, spec in enumerate(GROUPS):
        ps = [_param(n, dt, 10_000 * gi + i) for i, (dt, n, _) in enumerate(spec)]
        groups.append(dict(params=ps, lr=hp["lr"] * (gi + 1)))
        flat += [(p, dt, none, 10_000 * gi + i) for i, (p, (dt, n, none)) in enumerate(zip(ps, spec))]
    opt = getattr(bnb, CLS[rule])(groups, page_to_cpu=page_to_cpu, **{k: v for k, v in hp.items() if k != "lr"})
    opt._page_elems = page_elems
    snap = None
    for s in range(1, steps + 1):
        for p, dt, none, seed in flat:
            p.grad = None if s in none else _grad(p.numel(), dt, seed + 100_000 * s).cuda()
        opt.step()                                                  # no synchronize() between steps
        if s == snapshot_at:
            snap = opt.state_dict()                                 # synchronises; holds the live tensors, which later steps update in place
            snap = copy.deepcopy(snap) if s < steps else snap
    opt.synchronize()
    return opt, flat, snap


@pytest.fixture(scope="module")
def emulated():
    """p, m, v of every tensor of GROUPS after five steps of the emulation, per rule; computed once."""
    out = {}
    for rule in emul.RULES:
        res = []
        for gi, spec in enumerate(GROUPS):
            hp = dict(HP[rule], lr=HP[rule]["lr"] * (gi + 1))
            for i, (dt, n, none) in enumerate(spec):
                seed = 10_000 * gi + i
                e = emul.EmuTensor(rule, hp, synthetic.normal((n,), DT[dt], seed=seed))
                for s in range(1, 6):
                    if s not in none:
                        e.step(_grad(n, dt, seed + 100_000 * s))
                res.append(e)
        out[rule] = res
    return out


@pytest.mark.parametrize("rule", emul.RULES)
def test_paging_is_bit_equal_to_the_resident_step_and_the_emulation(rule, emulated):
    paged_opt, paged_flat, _ = _run_paged_model(rule, True, PAGE)
    runs = {"resident": _run_paged_model(rule, False, PAGE), "one page": _run_paged_model(rule, True, 1 << 20)}
    for k, (p, dt, none, _) in enumerate(paged_flat):
        m, v = _moments(paged_opt, p)
        e = emulated[rule][k]
        assert m.device.type == "cpu" and (m.is_pinned() or m.numel() == 0) and m.dtype == p.dtype and m.shape == p.shape
        if rule != "lion":
            assert paged_opt.state[p]["step"] == 5 - len(none) == e.step_count
        for name, (opt, flat, _) in runs.items():
            q = flat[k][0]
            qm, qv = _moments(opt, q)
            assert qm.device.type == ("cuda" if name == "resident" else "cpu")
            _same(f"{rule} tensor {k} ({dt}, {p.numel()}) p vs {name}", p, q)
            _same(f"{rule} tensor {k} exp_avg vs {name}", m, qm)
            if v is not None:
                _same(f"{rule} tensor {k} exp_avg_sq vs {name}", v, qv)
        _same(f"{rule} tensor {k} ({dt}, {p.numel()}) p vs emulation", p, e.p)
        _same(f"{rule} tensor {k} exp_avg vs emulation", m, e.m)
        if v is not None:
            _same(f"{rule} tensor {k} exp_avg_sq vs emulation", v, e.v)


def test_pages_and_launches_of_a_step():
    from mps_bitsandbytes_amd.optim.paged import plan_pages
    params = [_param(8, "bf16", i) for i in range(60)] + [_param(5 * PAGE - 5, "bf16", 77)]
    for p in params:
        p.grad = torch.ones_like(p)
    opt = bnb.PagedLion(params)
    opt._page_elems = PAGE
    pn.reset_launch_log()
    opt.step()
    opt.synchronize()
    pages = plan_pages([p.numel() for p in params], PAGE)
    assert len(pages) == 6 and len(pages[0]) == 61           # 60 x 8 elements and the head of the large tensor share the first page
    assert [n for _, _, n in pn.launch_log] == [48, 13, 1, 1, 1, 1, 1]
    ring = next(iter(opt._rings.values()))
    assert len(ring.bufs) == 3 and all(len(slot) == 1 and slot[0].numel() == PAGE * 2 for slot in ring.bufs)


# ----------------------------------------------------------------------------- the state through state_dict
@pytest.mark.parametrize("rule", emul.RULES)
def test_state_round_trip(rule):
    full, full_flat, snap = _run_paged_model(rule, True, PAGE, steps=4, snapshot_at=3)
    for src_paged, dst_paged in ((True, True), (False, True), (True, False)):
        src, src_flat, sd = _run_paged_model(rule, src_paged, PAGE, steps=3, snapshot_at=3)
        dst, dst_flat, _ = _run_paged_model(rule, dst_paged, PAGE, steps=0)
        for (p, *_), (q, *_) in zip(dst_flat, src_flat):
            p.data.copy_(q.data)                                   # the parameters after three steps
        dst.load_state_dict(sd)
        assert all(g["page_to_cpu"] is dst_paged for g in dst.param_groups)   # where the moments live is the optimizer's, not the checkpoint's
        for p, dt, none, seed in dst_flat:
            st = dst.state.get(p, {})
            for k in ("exp_avg", "exp_avg_sq"):
                if k in st:
                    t = st[k]
                    assert t.dtype == p.dtype and t.shape == p.shape and t.is_contiguous()
                    assert (t.device.type == "cpu" and (t.is_pinned() or t.numel() == 0)) if dst_paged else t.device == p.device
                    assert t.numel() == 0 or all(t.data_ptr() != u.data_ptr() for s2 in src.state.values() for u in s2.values() if isinstance(u, torch.Tensor))
            if "step" in st:
                assert isinstance(st["step"], int)
            p.grad = None if 4 in none else _grad(p.numel(), dt, seed + 100_000 * 4).cuda()
        dst.step()
        dst.synchronize()
        for (p, *_), (q, *_) in zip(dst_flat, full_flat):
            _same(f"{rule} {src_paged}->{dst_paged} p", p, q)
            if full.state[q]:
                _same(f"{rule} {src_paged}->{dst_paged} exp_avg", dst.state[p]["exp_avg"], full.state[q]["exp_avg"])
                if rule != "lion":
                    _same(f"{rule} {src_paged}->{dst_paged} exp_avg_sq", dst.state[p]["exp_avg_sq"], full.state[q]["exp_avg_sq"])
                    assert dst.state[p]["step"] == full.state[q]["step"]
    # the snapshot taken in the middle of the uninterrupted run holds the state after step 3 (state_dict synchronises)
    mid, mid_flat, _ = _run_paged_model(rule, True, PAGE, steps=3)
    ids = [pid for g in snap["param_groups"] for pid in g["params"]]
    for pid, (q, *_) in zip(ids, mid_flat):
        if pid in snap["state"]:
            _same(f"{rule} snapshot exp_avg", snap["state"][pid]["exp_avg"], mid.state[q]["exp_avg"])


# ----------------------------------------------------------------------------- device memory
def test_device_memory_held_for_moments_is_the_slots():
    page, n, count = 1 << 18, 1 << 20, 16
    params = [torch.nn.Parameter(torch.full((n,), 1.0 + i, device="cuda")) for i in range(count)]
    for p in params:
        p.grad = torch.full_like(p, 0.5)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    opt = bnb.PagedAdamW(params, lr=1e-2)
    opt._page_elems = page
    for _ in range(2):
        opt.step()
    opt.synchronize()
    held = torch.cuda.memory_allocated() - before
    assert held <= opt._slots * 2 * page * 4 + (1 << 20), f"{held} bytes held on the device"
    assert held < count * n * 4 * 2 // 8                           # an eighth of what resident moments would take
    for p in params:
        m = opt.state[p]["exp_avg"]
        assert m.is_pinned() and torch.all(m == m.view(-1)[0]) and float(m.view(-1)[0]) != 0.0
        assert torch.all(p == p.view(-1)[0])

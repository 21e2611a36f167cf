"""The 8-bit optimizer kernels against the numpy emulation of their contract (tests/optim_emul.py), at zero tolerance.

Every case of tests/optim_cases.py runs through the public optimizer classes, chained, and after every step parameters, codes and
maxima must be the emulation's bits (a NaN where the emulation has a NaN).  The emulation is pinned to the reference's CPU
optimizers by tests/test_optim_emul_host.py; the kernel's contract is the emulation's, so neither of the two torch exceptions of
DESIGN.md §10 applies here.  Then the edges a table does not fit: guard bands around every buffer, descriptor tables with empty
tensors and two launches, a tensor past 2^31 elements, parameters and gradients off 16-byte alignment, non-finite gradients."""
import time

import numpy as np
import pytest
import torch

from tests import optim_cases, optim_data
from tests import optim_emul as emul

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 4096
KEYS = {"adam": ("exp_avg_int8", "exp_avg_absmax", "exp_avg_sq_uint8", "exp_avg_sq_max"),
        "adamw": ("exp_avg_int8", "exp_avg_absmax", "exp_avg_sq_uint8", "exp_avg_sq_max"),
        "lion": ("exp_avg_int8", "exp_avg_absmax"), "sgd": ("momentum_int8", "momentum_absmax"),
        "sgd_nesterov": ("momentum_int8", "momentum_absmax")}


def _native():
    from mps_bitsandbytes_amd import _optim_native
    return _optim_native


def _kind(rule):
    n = _native()
    return {"adam": n.ADAM, "adamw": n.ADAMW, "lion": n.LION, "sgd": n.SGD_MOMENTUM, "sgd_nesterov": n.SGD_NESTEROV}[rule]


def _make_opt(c, params):
    from mps_bitsandbytes_amd import optim
    n = len(params)
    group_of = c.get("group_of") or [0] * n
    groups = [dict(params=[p for p, g in zip(params, group_of) if g == gi], **optim_cases.group_kwargs(c, gi))
              for gi in range(max(group_of) + 1)]
    opt = getattr(optim, optim_cases.CLASS[c["rule"]])(groups, **c["kwargs"])
    if c.get("force"):
        opt._step_flags = _native().FORCE_GENERIC
    return opt, group_of


def _got(c, opt, p):
    st = opt.state[p]
    return dict(zip(("q1", "a1", "q2", "a2"), (st[k] for k in KEYS[c["rule"]])), p=p.detach())


def _expected_log(c, group_of, grads):
    """One entry per mbnb_optim_step call: per group, its tensors that have a gradient, 48 to a call."""
    log = []
    for gi in range(max(group_of) + 1):
        n = sum(1 for j, g in enumerate(grads) if g is not None and group_of[j] == gi)
        log += [(_kind(c["rule"]), emul.DT[c["pdt"]], emul.DT[c["gdt"]], min(48, n - k)) for k in range(0, n, 48)]
    return log


def _run_case(c, params=None, grads_for=None):
    """Step the case on the GPU and in the emulation side by side; compare after every step."""
    tag = optim_cases.case_id(c)
    if params is None:
        params = [torch.nn.Parameter(optim_data.param(c, j).to(DEV)) for j in range(len(c["shapes"]))]
    for p in params:
        p.grad_dtype = None            # allow an f32 gradient on a 16-bit parameter
    opt, group_of = _make_opt(c, params)
    es = optim_data.emulation(c)
    for s in range(1, c["steps"] + 1):
        if s in c.get("set_step", {}):
            for p, e in zip(params, es):
                opt.state[p]["step"] = e.step_count = c["set_step"][s]
        grads = grads_for(s) if grads_for else optim_data.step_grads(c, s)
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.to(DEV)
        _native().reset_launch_log()
        opt.step()
        torch.cuda.synchronize()
        assert list(_native().launch_log) == _expected_log(c, group_of, grads), f"{tag} step {s}: {_native().launch_log}"
        for j, (p, e, g) in enumerate(zip(params, es, grads)):
            if g is None:
                continue
            e.step(g)
            if p.numel():
                emul.compare(f"{tag} param {j} step {s}", _got(c, opt, p), e.result(), e.bs, e.pdt, e.before)
    return params, opt, es


def _table_params():
    return [pytest.param(c, id=optim_cases.case_id(c), marks=[pytest.mark.xfail(strict=True, reason=c["xfail"])] if c.get("xfail") else [])
            for c in optim_cases.CASES if c is not optim_cases.LARGE]


@pytest.mark.parametrize("c", _table_params())
def test_kernel_equals_emulation(c):
    """Each case of the table: all 50 instantiations, sizes 1 to 65541, blocks of 1 to 4096 elements, gradients over the dtype's
    binades with a zero block and a constant-tiny block, rounding ties, subnormal second moments, f16 near the top of its range,
    Adam at steps 1000 and 10^6, two groups, grad = None steps.  Bit-equal after every chained step; the launch log shows the
    expected (kind, dtypes, tensors)."""
    _run_case(c)


def test_kernel_equals_emulation_at_4096_x_11008(capsys):
    """The flagship shape: one 4096 x 11008 bf16 parameter, AdamW, 3 chained steps, every element."""
    t0 = time.time()
    _run_case(optim_cases.LARGE)
    with capsys.disabled():
        print(f"\n  4096 x 11008 x 3 steps against the emulation: {time.time() - t0:.0f} s", end="")


# ----------------------------------------------------------------------------- guard bands
def _guarded(nbytes, dtype, shape=None):
    """A view of `nbytes` bytes as `dtype` inside a 0xFF-filled buffer, 4 KiB of guard on each side (the view keeps the buffer's
    alignment: 4096 is a multiple of 16)."""
    buf = torch.full((GUARD + nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    v = buf[GUARD:GUARD + nbytes].view(dtype)
    assert v.data_ptr() % 16 == 0
    return buf, (v if shape is None else v.view(shape))


def _np_of(dt):
    return {torch.float16: np.uint16, torch.bfloat16: np.uint16, torch.float32: np.float32, torch.int8: np.int8, torch.uint8: np.uint8}[dt]


@pytest.mark.parametrize("rem", [1, 2, 3])
@pytest.mark.parametrize("kernel", ["wave", "generic"])
@pytest.mark.parametrize("rule,pdt,gdt", [("adam", "bf16", "bf16"), ("lion", "f16", "f32")])
def test_guard_bands_keep_their_fill(rule, pdt, gdt, kernel, rem):
    """Parameter, gradient, codes and maxima are views into 0xFF-filled buffers with 4 KiB guards on each side (parameter and
    gradient 16-byte aligned, codes 4-byte aligned), the state injected through opt.state[p] before the first step; numel % 4 is
    1, 2, 3.  After 2 steps every guard keeps its fill, the gradient's bits are unchanged and the results are the emulation's: a
    partial-block path that stores a code past numel, or a kernel that writes the gradient, fails here."""
    n = 512 + rem
    bs = 256 if kernel == "wave" else 300
    c = optim_cases._c(rule, pdt, gdt, [(n,)], 2, 70000 + 10 * rem, hp=dict(block_size=bs))
    nb = emul.n_blocks(n, bs)
    two = rule in emul.TWO_MOMENTS
    P, G = emul.DT[pdt], emul.DT[gdt]
    bufs = {}
    bufs["p"], pv = _guarded(n * P.itemsize, P)
    bufs["g"], gv = _guarded(n * G.itemsize, G)
    bufs["q1"], q1 = _guarded(n, torch.int8)
    bufs["a1"], a1 = _guarded(4 * nb, torch.float32)
    pv.copy_(optim_data.param(c, 0))
    q1.zero_()
    a1.fill_(1e-8)
    p = torch.nn.Parameter(pv)
    assert p.data_ptr() == pv.data_ptr()
    state = {"exp_avg_int8": q1, "exp_avg_absmax": a1}
    if two:
        bufs["q2"], q2 = _guarded(n, torch.uint8)
        bufs["a2"], a2 = _guarded(4 * nb, torch.float32)
        q2.zero_()
        a2.fill_(1e-12)
        state.update(step=0, exp_avg_sq_uint8=q2, exp_avg_sq_max=a2)
    p.grad_dtype = None
    opt, _ = _make_opt(c, [p])
    opt.state[p].update(state)
    e = optim_data.emulation(c)[0]
    for s in (1, 2):
        g = optim_data.step_grads(c, s)[0]
        gv.copy_(g)
        p.grad = gv
        assert p.grad.data_ptr() == gv.data_ptr()
        opt.step()
        torch.cuda.synchronize()
        e.step(g)
        assert p.data_ptr() == pv.data_ptr() and opt.state[p]["exp_avg_int8"].data_ptr() == q1.data_ptr()
        sizes = dict(p=(n * P.itemsize, _np_of(P)), q1=(n, np.int8), a1=(4 * nb, np.float32), q2=(n, np.uint8), a2=(4 * nb, np.float32))
        got = {k: emul.Guarded(bufs[k].cpu().numpy(), GUARD, sizes[k][0], sizes[k][1]) for k in bufs if k != "g"}
        emul.compare(f"{optim_cases.case_id(c)} step {s}", got, e.result(), bs, pdt, e.before)
        gb = bufs["g"].cpu().numpy()
        assert (gb[:GUARD] == 0xFF).all() and (gb[GUARD + n * G.itemsize:] == 0xFF).all(), "the gradient's guards were written"
        assert np.array_equal(gb[GUARD:GUARD + n * G.itemsize], emul.bits(g).view(np.uint8)), "the gradient was written"


# ----------------------------------------------------------------------------- descriptor tables
def _small(i):
    return 1 + (i * 37) % 300


TABLES = {
    "48 with empty tensors first, in the middle and last": [0 if i in (0, 20, 47) else _small(i) for i in range(48)],
    "a group whose only tensor is empty": [0],
    "49 tensors, two launches": [_small(i) for i in range(49)],
    "one 2^20-element tensor among 46 small ones": [_small(i) for i in range(23)] + [1 << 20] + [_small(i) for i in range(23, 46)],
}


@pytest.mark.parametrize("kernel", ["wave", "generic"])
@pytest.mark.parametrize("name", list(TABLES))
def test_descriptor_tables(name, kernel):
    """The table of one call: empty tensors (numel 0) make owner() meet equal first_block entries; 49 tensors are two launches; one
    large tensor among small ones makes the block search uneven.  Every tensor equals the emulation after each of 2 steps."""
    sizes = TABLES[name]
    rule, pdt, gdt = ("adamw", "bf16", "bf16") if kernel == "wave" else ("lion", "f16", "f32")
    c = optim_cases._c(rule, pdt, gdt, [(n,) for n in sizes], 2, 71000 + len(sizes), hp=dict(block_size=256 if kernel == "wave" else 64))
    params, opt, _ = _run_case(c)
    assert [p.numel() for p in params] == sizes


# ----------------------------------------------------------------------------- past 2^31 elements
def test_tensor_past_2_31_elements(capsys):
    """One bf16 AdamW parameter of 2^31 + 259 elements (about 12 GiB with gradient and states), stepped twice.  The gradient is made
    on the device from the seeded generator and is nowhere zero, so every block's first-moment maximum must leave its initial 1e-8:
    every block was visited.  Bit-equal to the emulation: the first two blocks, the last two (the last one partial, 3 elements), the
    blocks on either side of element 2^30 (byte offset 2^31 of a bf16 tensor) and of element 2^31, and 4096 seeded random blocks."""
    from mps_bitsandbytes_amd import optim, synthetic
    t0 = time.time()
    n, bs = (1 << 31) + 259, 256
    nb = emul.n_blocks(n, bs)
    assert nb == (1 << 23) + 2
    hp = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    p = torch.nn.Parameter(synthetic.normal_device((n,), torch.bfloat16, seed=91000, device=DEV))
    g = synthetic.normal_device((n,), torch.bfloat16, seed=91001, device=DEV)
    g.masked_fill_(g == 0, 2.0 ** -20)
    assert int((g == 0).sum()) == 0 and bool(torch.isfinite(g).all())
    p.grad = g
    opt = optim.AdamW8bit([p], block_size=bs, **hp)
    rng = np.random.default_rng(91002)
    fixed = [0, 1, nb - 2, nb - 1, (1 << 30) // bs - 1, (1 << 30) // bs, (1 << 31) // bs - 1, (1 << 31) // bs]
    blocks = np.array(sorted(set(fixed) | set(int(b) for b in rng.integers(0, nb, 4096))), dtype=np.int64)
    assert len(blocks) >= 4096
    q1 = torch.zeros(n, dtype=torch.int8, device=DEV)
    a1 = torch.full((nb,), 1e-8, dtype=torch.float32, device=DEV)
    q2 = torch.zeros(n, dtype=torch.uint8, device=DEV)
    a2 = torch.full((nb,), 1e-12, dtype=torch.float32, device=DEV)
    opt.state[p].update(step=0, exp_avg_int8=q1, exp_avg_absmax=a1, exp_avg_sq_uint8=q2, exp_avg_sq_max=a2)
    for s in (1, 2):
        before = emul.gather_blocks(blocks, bs, n, p=p.detach(), g=g, q1=q1, a1=a1, q2=q2, a2=a2)
        want = emul.step_gathered("adamw", hp, s, "bf16", "bf16", before)
        _native().reset_launch_log()
        opt.step()
        torch.cuda.synchronize()
        assert list(_native().launch_log) == [(_native().ADAMW, torch.bfloat16, torch.bfloat16, 1)]
        st = opt.state[p]
        assert st["exp_avg_int8"].data_ptr() == q1.data_ptr() and st["step"] == s
        got = emul.gather_blocks(blocks, bs, n, p=p.detach(), g=g, q1=q1, a1=a1, q2=q2, a2=a2)
        emul.compare_gathered(f"2^31 + 259 step {s}", blocks, got, want, before, "bf16")
        assert torch.equal(got["g"].view(torch.int16), before["g"].view(torch.int16)), "the gradient was written"
        if s == 1:
            assert int((a1 == np.float32(1e-8)).sum()) == 0, "a block kept its initial first-moment maximum: it was never visited"
    with capsys.disabled():
        print(f"\n  2^31 + 259 elements, 2 steps, {len(blocks)} blocks against the emulation: {time.time() - t0:.0f} s", end="")


# ----------------------------------------------------------------------------- off 16-byte alignment
@pytest.mark.parametrize("rule,pdt,gdt", [("adamw", "bf16", "bf16"), ("sgd_nesterov", "f16", "f16")])
def test_contiguous_but_misaligned_parameter_and_gradient(rule, pdt, gdt):
    """A contiguous parameter and a contiguous gradient that are slices of flat buffers, each 2 bytes off 16-byte alignment: the
    clone-and-write-back route of optim/_base.py.  3 steps equal the emulation; the bytes around the slices keep their fill."""
    n = 1000
    c = optim_cases._c(rule, pdt, gdt, [(n,)], 3, 72000)
    P = emul.DT[pdt]
    pbuf = torch.full(((n + 16) * 2,), 0xFF, dtype=torch.uint8, device=DEV).view(P)
    gbuf = torch.full(((n + 16) * 2,), 0xFF, dtype=torch.uint8, device=DEV).view(P)
    pv, gv = pbuf[1:1 + n], gbuf[1:1 + n]
    assert pv.is_contiguous() and pv.data_ptr() % 16 == 2 and gv.data_ptr() % 16 == 2
    pv.copy_(optim_data.param(c, 0))
    p = torch.nn.Parameter(pv)
    assert p.data_ptr() == pv.data_ptr()

    def grads_for(s):
        gv.copy_(optim_data.step_grads(c, s)[0])
        return [gv]

    _run_case(c, params=[p], grads_for=grads_for)      # .to(DEV) of a tensor already there is the tensor itself
    assert p.grad.data_ptr() == gv.data_ptr() and p.data_ptr() == pv.data_ptr()
    for buf, inner in ((pbuf, None), (gbuf, optim_data.step_grads(c, 3)[0])):
        b = buf.view(torch.uint8).cpu().numpy()
        assert (b[:2] == 0xFF).all() and (b[2 + 2 * n:] == 0xFF).all(), "bytes around the slice were written"
        if inner is not None:
            assert np.array_equal(b[2:2 + 2 * n].view(np.uint16), emul.bits(inner)), "the gradient was written"


# ----------------------------------------------------------------------------- non-finite gradients
@pytest.mark.parametrize("kernel", ["wave", "generic"])
@pytest.mark.parametrize("rule", ["adamw", "sgd"])
def test_non_finite_gradients_follow_the_documented_behaviour(rule, kernel):
    """DESIGN.md §10's paragraph on non-finite gradients, pinned (this is the kernel's documented behaviour, not parity with the
    reference).  A 5-block tensor; on step 1 the gradient holds one NaN in block 1 and one +Inf in block 3; steps 2 and 3 are finite.

    What the emulation and the kernel both do:
    - the NaN element: its moments and its parameter become NaN, its codes are stored as 0, and the NaN is dropped from the block's
      maxima, so the other elements of block 1 are quantised as if it were not there.  The parameter element stays NaN for good.
      Under AdamW its moments restart from code 0 on step 2; under SGD the NaN parameter comes back through the weight decay
      (g + wd * p), so its momentum is NaN, stored as code 0, on every later step.
    - the +Inf element: its first moment is +Inf, so block 3's first-moment maximum is +Inf (under AdamW the second-moment maximum
      too) and every code of the block is 0 (x / Inf = 0, and Inf / Inf = NaN is stored as 0).  Under AdamW the element's own update
      is Inf / Inf = NaN on step 1; under SGD its parameter becomes -Inf.  On step 2 the block dequantises as 0 * Inf = NaN, so
      EVERY parameter of block 3 becomes NaN and stays NaN.  The NaN moments are dropped from the maxima, which fall back to their
      clamps (1e-8, 1e-12), with codes 0.  On step 3 AdamW's moments of the block are finite again (they restart from zero); SGD's
      stay NaN, code 0 under the clamp 1e-8, because the NaN parameters feed the weight decay.
    - blocks 0, 2 and 4 never see a non-finite value: they are bit-equal to the same run with finite gradients.
    The GPU equals the emulation throughout: bits where numbers, NaN where NaN."""
    bs = 256 if kernel == "wave" else 100
    n = 4 * bs + bs // 2 + 1                               # 5 blocks, the last one partial
    c = optim_cases._c(rule, "bf16", "f32", [(n,)], 3, 73000, hp=dict(block_size=bs))
    i_nan, i_inf = bs + 7, 3 * bs + 11

    def poisoned(s):
        g = optim_data.step_grads(c, s)[0].clone()
        if s == 1:
            g[i_nan], g[i_inf] = float("nan"), float("inf")
        return [g]

    params, opt, es = _run_case(c, grads_for=poisoned)
    clean, clean_opt, _ = _run_case(c)
    e = es[0]
    pf = params[0].detach().float().cpu()
    blk = lambda t, b: t.flatten()[b * bs:(b + 1) * bs]
    assert bool(torch.isnan(blk(pf, 3)).all()), "every parameter of the +Inf block is NaN after step 2"
    assert bool(torch.isnan(pf[i_nan])) and int(torch.isnan(blk(pf, 1)).sum()) == 1, "only the NaN element of block 1 is NaN"
    assert np.isfinite(e.a1).all() and (e.a2 is None or np.isfinite(e.a2).all()), "the maxima are finite again by step 3"
    q1_3 = e.q1[3 * bs:4 * bs]
    assert (int((q1_3 != 0).sum()) > 0) == (rule == "adamw"), "AdamW's moments of the +Inf block recover on step 3, SGD's do not"
    for b in (0, 2, 4):
        for k, v in _got(c, opt, params[0]).items():
            w = _got(c, clean_opt, clean[0])[k]
            if k in ("a1", "a2"):
                assert emul.bits(v)[b] == emul.bits(w)[b], (k, b)
            else:
                assert np.array_equal(emul.bits(blk(v, b)), emul.bits(blk(w, b))), (k, b)

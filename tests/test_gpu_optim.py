"""8-bit optimizers on the GPU: the fused HIP step against the reference's CPU optimizers (tests/golden/g10_optim.npz),
the multi-tensor launch, the generic block-size path, state_dict round trips, non-contiguous parameters and a QLoRA loop."""
import copy
import io
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import optim_emul as emul
from tests.goldenio import DT, NAME, from_bits

pytestmark = pytest.mark.gpu

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda:0")


def _optim():
    from mps_bitsandbytes_amd import optim
    return optim


@pytest.fixture(scope="module")
def g10():
    with open(os.path.join(HERE, "manifest_optim.json")) as f:
        man = json.load(f)
    return man, np.load(os.path.join(HERE, "g10_optim.npz"))


def _int_view(t):
    t = t.detach().cpu().contiguous()
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16).long()
    if t.dtype == torch.float32:
        return t.view(torch.int32).long()
    return t.long()


def _cases():
    with open(os.path.join(HERE, "manifest_optim.json")) as f:
        return [c["id"] for c in json.load(f)["g10"]]


@pytest.mark.parametrize("cid", _cases())
def test_golden_step_by_step(g10, cid):
    """Every step of every case, started from the reference's parameter and state after the previous step: parameters,
    codes and maxima are the reference's bits.  Two documented exceptions: f32 parameters under Adam may
    be 1 ulp away (torch's vectorised CPU sqrt is not correctly rounded; the kernel's is), and SGD's 16-bit parameters
    may be 1 ulp away in the last numel % 64 elements (torch's scalar tail loop rounds alpha * x to 16 bits first).
    The max_grad_norm case clips on the GPU, whose norm differs from the CPU's in the last bits: compared within a tolerance
    against the golden, and bit for bit against the emulation (tests/optim_emul.py) fed the clipped gradient that p.grad holds
    after the step."""
    from mps_bitsandbytes_amd import synthetic
    man, z = g10
    case = man["g10"][cid]
    keys = man["state_keys"][case["opt"]]
    cls = {"adam": "Adam8bit", "adamw": "AdamW8bit", "lion": "Lion8bit", "sgd": "SGD8bit"}[case["opt"]]
    pdt, gdt = DT[case["param_dtype"]], DT[case["grad_dtype"]]
    seed, shapes = case["seed"], [tuple(s) for s in case["shapes"]]
    params = [torch.nn.Parameter(synthetic.normal(shp, pdt, seed=seed + 100 * j).to(DEV)) for j, shp in enumerate(shapes)]
    for p in params:
        p.grad_dtype = None
    opt = getattr(_optim(), cls)(params, **case["kwargs"])
    clip = case["kwargs"].get("max_grad_norm") is not None
    nsteps = [0] * len(params)
    for s in range(1, case["steps"] + 1):
        for j, p in enumerate(params):
            with torch.no_grad():
                if s > 1:
                    p.copy_(from_bits(z[f"c{cid}_p{j}_s{s - 1}"], pdt).view(shapes[j]).to(DEV))
            st = opt.state[p]
            st.clear()
            if s > 1 and f"c{cid}_p{j}_s{s - 1}_{keys[0]}" in z.files:
                for k in keys:
                    st[k] = from_bits(z[f"c{cid}_p{j}_s{s - 1}_{k}"], torch.float32).to(DEV)
                    if k.endswith(("_int8", "_uint8")):
                        st[k] = st[k].view(shapes[j])
                if case["opt"] in ("adam", "adamw"):
                    st["step"] = nsteps[j]
            if s in case["none_steps"][j]:
                p.grad = None
            else:
                p.grad = synthetic.normal(shapes[j], gdt, seed=seed + 100 * j + s).to(DEV)
                nsteps[j] += 1
        emus = []
        if clip:                     # the emulation starts each step where the GPU does: the golden's parameter and state
            for j, p in enumerate(params):
                e = emul.EmuTensor(case["opt"], {"betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 1e-2, **case["kwargs"]}, p.detach(),
                                   case["kwargs"].get("block_size", 256))
                st = opt.state[p]
                if st:
                    e.q1, e.a1, e.q2, e.a2 = (st[k].detach().cpu().flatten().numpy().copy() for k in keys)
                    e.step_count = st["step"]
                emus.append(e)
        opt.step()
        for e, p in zip(emus, params):
            if p.grad is not None:
                e.step(p.grad)       # clip_grad_norm_ scaled p.grad in place: this is the gradient the kernel read
                st = opt.state[p]
                emul.compare(f"case {cid} step {s} against the emulation", dict(zip(("q1", "a1", "q2", "a2"), (st[k] for k in keys)), p=p.detach()),
                             e.result(), e.bs, NAME[pdt], e.before)
        for j, p in enumerate(params):
            want = from_bits(z[f"c{cid}_p{j}_s{s}"], pdt).view(shapes[j])
            got = p.detach().cpu()
            where = f"case {cid} ({case['opt']} {case['param_dtype']}/{case['grad_dtype']} {shapes[j]}) param {j} step {s}"
            if clip:
                assert torch.allclose(got.float(), want.float(), rtol=1e-2, atol=1e-3), where
            else:
                d = (_int_view(got) - _int_view(want)).abs().flatten()
                bad = d.nonzero().flatten()[:4].tolist()
                where += f" (elements {bad}: got {got.flatten()[bad].tolist()}, want {want.flatten()[bad].tolist()})"
                if case["opt"] in ("adam", "adamw") and pdt == torch.float32:
                    assert int(d.max()) <= 1, f"{where}: {int(d.max())} ulp"
                elif case["opt"] == "sgd" and pdt != torch.float32:
                    n = d.numel()
                    tail = n % 64
                    assert int(d[:n - tail].max()) == 0 if n > tail else True, f"{where}: vectorised part differs"
                    assert int(d.max()) <= 1, f"{where}: tail {int(d.max())} ulp"
                else:
                    assert int(d.max()) == 0, f"{where}: {int((d != 0).sum())} of {d.numel()} elements differ"
            if f"c{cid}_p{j}_s{s}_{keys[0]}" not in z.files:
                continue
            st = opt.state[p]
            for k in keys:
                want_k = from_bits(z[f"c{cid}_p{j}_s{s}_{k}"], torch.float32).flatten()
                got_k = st[k].detach().cpu().flatten()
                assert got_k.dtype == want_k.dtype, f"{where} {k}: {got_k.dtype}"
                if clip:
                    if k.endswith("int8"):
                        assert int((got_k.long() - want_k.long()).abs().max()) <= 1, f"{where} {k}"
                    else:
                        assert torch.allclose(got_k, want_k, rtol=1e-3), f"{where} {k}"
                else:
                    assert torch.equal(_int_view(got_k), _int_view(want_k)), \
                        f"{where} {k}: {int((_int_view(got_k) != _int_view(want_k)).sum())} differ"


def _lora_like(n, seed):
    """n tensors of mixed sizes (partial last blocks, one element, empty-free) and two dtypes, with gradients."""
    from mps_bitsandbytes_amd import synthetic
    shapes = [(16, 96), (96, 16), (1,), (257,), (3, 100), (1000,), (64, 64)]
    ps = []
    for i in range(n):
        dt = torch.bfloat16 if i % 3 else torch.float16
        p = torch.nn.Parameter(synthetic.normal(shapes[i % len(shapes)], dt, seed=seed + i).to(DEV))
        p.grad = synthetic.normal(p.shape, dt, seed=seed + 5000 + i).to(DEV)
        ps.append(p)
    return ps


def test_multi_tensor_launch_matches_single_tensor_steps():
    """130 tensors of two dtypes in one AdamW8bit group: one call (= one launch) per dtype pair and 48 tensors, and the
    same bits as stepping every tensor with an optimizer of its own."""
    optim = _optim()
    from mps_bitsandbytes_amd import _optim_native
    group = _lora_like(130, 77)
    alone = [torch.nn.Parameter(p.detach().clone()) for p in group]
    for a, p in zip(alone, group):
        a.grad = p.grad.clone()
    opt = optim.AdamW8bit(group, lr=1e-2)
    singles = [optim.AdamW8bit([a], lr=1e-2) for a in alone]
    for step in range(3):
        _optim_native.reset_launch_log()
        opt.step()
        log = list(_optim_native.launch_log)
        n16 = sum(1 for p in group if p.dtype == torch.float16)
        per_pair = {}
        for kind, pdt, gdt, n in log:
            per_pair.setdefault((pdt, gdt), []).append(n)
        assert set(per_pair) == {(torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16)}
        assert per_pair[(torch.float16, torch.float16)] == [48] * (n16 // 48) + ([n16 % 48] if n16 % 48 else [])
        assert sum(per_pair[(torch.bfloat16, torch.bfloat16)]) == 130 - n16
        assert len(log) == math.ceil(n16 / 48) + math.ceil((130 - n16) / 48)
        for o in singles:
            o.step()
    torch.cuda.synchronize()
    for p, a, o in zip(group, alone, singles):
        assert torch.equal(_int_view(p), _int_view(a))
        for k in ("exp_avg_int8", "exp_avg_absmax", "exp_avg_sq_uint8", "exp_avg_sq_max"):
            assert torch.equal(_int_view(opt.state[p][k]), _int_view(o.state[a][k])), k


@pytest.mark.parametrize("cls", ["AdamW8bit", "Lion8bit", "SGD8bit"])
def test_generic_block_path_equals_wave_path(cls):
    """The workgroup-per-block path (any block_size), forced at 256, gives the wave-per-block path's bits."""
    optim = _optim()
    kw = dict(lr=1e-2, momentum=0.9, nesterov=True) if cls == "SGD8bit" else dict(lr=1e-2)
    a, b = _lora_like(20, 5), _lora_like(20, 5)
    oa, ob = getattr(optim, cls)(a, **kw), getattr(optim, cls)(b, **kw)
    ob._step_flags = 1       # MBNB_OPTIM_FORCE_GENERIC
    for _ in range(3):
        oa.step()
        ob.step()
    for p, q in zip(a, b):
        assert torch.equal(_int_view(p), _int_view(q))
        for k, v in oa.state[p].items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(_int_view(v), _int_view(ob.state[q][k])), k


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16, torch.float32])
def test_state_dict_round_trip_continues_bit_exactly(dt):
    from mps_bitsandbytes_amd import synthetic
    optim = _optim()

    def make():
        ps = [torch.nn.Parameter(synthetic.normal(s, dt, seed=31 + i).to(DEV)) for i, s in enumerate([(300,), (8, 40)])]
        return ps, optim.AdamW8bit(ps, lr=1e-2)

    def grads(ps, s):
        for i, p in enumerate(ps):
            p.grad = synthetic.normal(p.shape, dt, seed=900 + 10 * s + i).to(DEV)

    ref_ps, ref_opt = make()
    for s in range(4):
        grads(ref_ps, s)
        ref_opt.step()
    ps, opt = make()
    for s in range(2):
        grads(ps, s)
        opt.step()
    buf = io.BytesIO()
    torch.save(opt.state_dict(), buf)
    saved = [p.detach().clone() for p in ps]
    ps2, opt2 = make()
    with torch.no_grad():
        for p, v in zip(ps2, saved):
            p.copy_(v)
    buf.seek(0)
    opt2.load_state_dict(torch.load(buf, weights_only=False))
    for p in ps2:
        st = opt2.state[p]
        assert st["exp_avg_int8"].dtype == torch.int8 and st["exp_avg_sq_uint8"].dtype == torch.uint8
        assert st["exp_avg_absmax"].dtype == torch.float32 and st["exp_avg_sq_max"].dtype == torch.float32
        assert isinstance(st["step"], int) and st["step"] == 2
    for s in range(2, 4):
        grads(ps2, s)
        opt2.step()
    for p, q in zip(ps2, ref_ps):
        assert torch.equal(_int_view(p), _int_view(q))
        for k in ("exp_avg_int8", "exp_avg_absmax", "exp_avg_sq_uint8", "exp_avg_sq_max"):
            assert torch.equal(_int_view(opt2.state[p][k]), _int_view(ref_opt.state[q][k])), k

    # a state_dict whose tensors torch already cast to the parameter dtype (what a plain torch.optim load leaves) loads and steps
    sd = copy.deepcopy(opt.state_dict())         # state_dict() hands out opt's live per-parameter dicts
    for st in sd["state"].values():
        for k, v in list(st.items()):
            if isinstance(v, torch.Tensor):
                st[k] = v.to(dt)
    ps3, opt3 = make()
    opt3.load_state_dict(sd)
    grads(ps3, 2)
    opt3.step()
    for p in ps3:
        assert opt3.state[p]["exp_avg_int8"].dtype == torch.int8 and opt3.state[p]["exp_avg_absmax"].dtype == torch.float32
        assert torch.isfinite(p.detach().float()).all()


def test_checkpoint_of_other_shapes_is_refused_on_the_device():
    """A rank-8 adapter's optimizer state loaded into a rank-16 model raises before any launch, and leaves the parameter as it was."""
    from mps_bitsandbytes_amd import synthetic
    optim = _optim()
    small = torch.nn.Parameter(synthetic.normal((8, 4096), torch.bfloat16, seed=1).to(DEV))
    small.grad = torch.ones_like(small)
    src = optim.AdamW8bit([small])
    src.step()
    big = torch.nn.Parameter(synthetic.normal((16, 4096), torch.bfloat16, seed=2).to(DEV))
    big.grad = torch.ones_like(big)
    before = big.detach().clone()
    dst = optim.AdamW8bit([big])
    dst.load_state_dict(src.state_dict())
    with pytest.raises(ValueError, match="do not fit the parameter"):
        dst.step()
    torch.cuda.synchronize()
    assert torch.equal(big.detach(), before)
    assert dst.state[big]["step"] == 1


def test_non_contiguous_parameter_gives_the_contiguous_bits():
    from mps_bitsandbytes_amd import synthetic
    optim = _optim()
    base = synthetic.normal((40, 24), torch.bfloat16, seed=3).to(DEV)
    p_nc = torch.nn.Parameter(base.clone().t())          # (24, 40), transposed strides
    p_c = torch.nn.Parameter(base.clone().t().contiguous())
    assert not p_nc.is_contiguous()
    o1, o2 = optim.Adam8bit([p_nc], lr=1e-2, block_size=64), optim.Adam8bit([p_c], lr=1e-2, block_size=64)
    for s in range(3):
        g = synthetic.normal((24, 40), torch.bfloat16, seed=50 + s).to(DEV)
        p_nc.grad = g.t().contiguous().t()               # a non-contiguous gradient too
        p_c.grad = g.clone()
        o1.step()
        o2.step()
    assert p_nc.stride() == (1, 24)
    assert torch.equal(_int_view(p_nc), _int_view(p_c))
    assert torch.equal(o1.state[p_nc]["exp_avg_int8"].cpu(), o2.state[p_c]["exp_avg_int8"].cpu())


def _restated_adamw_step(p, g, st, lr, b1, b2, eps, wd, bs):
    """Independent f32 restatement of AdamW8bit's rule in plain torch ops: dequantise, update, requantise."""
    n = p.numel()
    nb = -(-n // bs)

    def blocks(x):
        return torch.nn.functional.pad(x.flatten().float(), (0, nb * bs - n)).view(nb, bs)

    m = (blocks(st["m"]) / 127.0 * st["ma"][:, None]).flatten()[:n]
    s = blocks(st["v"]) / 255.0
    v = (s * s * st["vm"][:, None]).flatten()[:n]
    g = g.flatten().float()
    st["t"] += 1
    pf = p.detach().flatten().float() * (1 - lr * wd)
    m = m * b1 + (1 - b1) * g
    v = v * b2 + (1 - b2) * g * g
    upd = m / (v.sqrt() / math.sqrt(1 - b2 ** st["t"]) + eps) * (-lr / (1 - b1 ** st["t"]))
    with torch.no_grad():
        p.copy_((pf + upd).view(p.shape).to(p.dtype))
    mb = blocks(m)
    st["ma"] = mb.abs().amax(1).clamp(min=1e-8)
    st["m"] = (mb / st["ma"][:, None] * 127).round().clamp(-127, 127).to(torch.int8).flatten()[:n]
    vb = blocks(v).clamp(min=0)
    st["vm"] = vb.amax(1).clamp(min=1e-12)
    st["v"] = ((vb / st["vm"][:, None]).sqrt() * 255).round().clamp(0, 255).to(torch.uint8).flatten()[:n]


def test_qlora_adamw8bit_end_to_end():
    """A frozen NF4 base plus rank-16 adapters trained for 20 steps with AdamW8bit: the loss falls, the base's buffers
    do not change, and the adapters stay within 5e-2 (relative Frobenius) of the same loop under the f32 restatement.  The
    emulation (tests/optim_emul.py), fed each step's GPU gradients and chained from its own state, must hold the adapters, the
    codes and the maxima bit for bit after the 20 steps."""
    import mps_bitsandbytes_amd as bnb
    from mps_bitsandbytes_amd import synthetic
    optim = _optim()
    K, N, r, M = 512, 384, 16, 256
    lin = torch.nn.Linear(K, N, bias=False)
    with torch.no_grad():
        lin.weight.copy_(synthetic.normal((N, K), torch.float32, seed=1, std=0.05))
    base = bnb.Linear4bit.from_linear(lin.to(device=DEV, dtype=torch.bfloat16), quant_type="nf4", compress_statistics=True)
    before = {k: v.detach().clone() for k, v in base.state_dict().items() if isinstance(v, torch.Tensor)}
    x = synthetic.normal((M, K), torch.bfloat16, seed=2).to(DEV)
    At = synthetic.normal((r, K), torch.bfloat16, seed=6, std=0.05).to(DEV)
    Bt = synthetic.normal((N, r), torch.bfloat16, seed=7, std=0.05).to(DEV)
    with torch.no_grad():
        target = base(x) + (x @ At.t()) @ Bt.t()          # reachable by the adapters

    def adapters():
        A = torch.nn.Parameter(synthetic.normal((r, K), torch.bfloat16, seed=4, std=0.02).to(DEV))
        B = torch.nn.Parameter(synthetic.normal((N, r), torch.bfloat16, seed=5, std=0.02).to(DEV))
        return A, B

    def loss_of(A, B):
        y = base(x) + (x @ A.t()) @ B.t()
        return (y.float() - target.float()).pow(2).mean()

    A, B = adapters()
    opt = optim.AdamW8bit([A, B], lr=5e-3)
    hp = dict(lr=5e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    emus = [emul.EmuTensor("adamw", hp, t.detach(), 256) for t in (A, B)]
    A2, B2 = adapters()
    states = [dict(m=torch.zeros(t.numel(), dtype=torch.int8, device=DEV), ma=torch.full((-(-t.numel() // 256),), 1e-8, device=DEV),
                   v=torch.zeros(t.numel(), dtype=torch.uint8, device=DEV), vm=torch.full((-(-t.numel() // 256),), 1e-12, device=DEV), t=0)
              for t in (A2, B2)]
    losses = []
    for _ in range(20):
        opt.zero_grad()
        loss = loss_of(A, B)
        loss.backward()
        opt.step()
        for e, t in zip(emus, (A, B)):
            e.step(t.grad)
        losses.append(loss.item())
        A2.grad = B2.grad = None
        loss_of(A2, B2).backward()
        for t, st in zip((A2, B2), states):
            _restated_adamw_step(t, t.grad, st, 5e-3, 0.9, 0.999, 1e-8, 1e-2, 256)
    assert losses[-1] < 0.9 * losses[0], losses
    for k, v in base.state_dict().items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(v, before[k]), f"base buffer {k} changed"
    for t, t2 in zip((A, B), (A2, B2)):
        err = ((t.float() - t2.float()).norm() / t2.float().norm()).item()
        assert err < 5e-2, err
    for name, e, t in zip("AB", emus, (A, B)):
        st = opt.state[t]
        got = dict(p=t.detach(), q1=st["exp_avg_int8"], a1=st["exp_avg_absmax"], q2=st["exp_avg_sq_uint8"], a2=st["exp_avg_sq_max"])
        emul.compare(f"adapter {name} after 20 steps", got, e.result(), 256, "bf16", e.before)

"""
One table of the 8-bit optimizer kernels (csrc/optim_kernels.hip: 5 rules x 5 (parameter, gradient) dtype pairs x 2 kernels).  Data
only, importable without a GPU.  tests/test_gpu_optim_elementwise.py runs every case through the public optimizer classes, chained,
and holds parameters, codes and maxima to the emulation (tests/optim_emul.py) bit for bit after every step;
tests/test_optim_emul_host.py proves that the table reaches all 50 instantiations and runs the EDGES cases against the reference's
results (tests/golden/g13_optim_edges.npz, captured by tests/golden/make_golden_optim_edges.py).

Keys
  rule      adam | adamw | lion | sgd | sgd_nesterov
  pdt gdt   parameter / gradient dtype: "f16" | "bf16" | "f32"
  kernel    "wave" (block_size 256) or "generic" (any other block_size, or 256 with force=True: MBNB_OPTIM_FORCE_GENERIC)
  kwargs    the optimizer's hyperparameters, block_size among them (absent: 256)
  shapes    the parameters, in order;  group_of: the parameter group of each (absent: one group);  group_kwargs: per group,
            overrides of kwargs
  data      the input kind of tests/optim_data.py (absent: normal);  grange: the gradient's binary exponents for "binades"
  steps     chained steps;  none_steps[j]: the steps (1-based) on which parameter j has grad = None
  set_step  {s: n}: before step s, every state's step count is set to n (Adam at a large step count)
  pmin      parameters kept away from zero, |p| >= pmin (tests/optim_data.py says why the f32 Adam cases of EDGES need it)
  seed      parameter j is data(seed + 100 j), its gradient at step s is data(seed + 100 j + s)
  xfail     a known departure of a KERNEL from the emulation, run as a strict xfail on the GPU; none today
  ref_xfail a further self-inconsistency of torch's CPU path: the REFERENCE's result departs from the emulation in
            this case, which runs as a strict xfail in tests/test_optim_emul_host.py; the GPU test holds the kernel to the emulation
"""

RULES = ("adam", "adamw", "lion", "sgd", "sgd_nesterov")
PAIRS = (("f16", "f16"), ("f16", "f32"), ("bf16", "bf16"), ("bf16", "f32"), ("f32", "f32"))
KERNELS = ("wave", "generic")
CLASS = {"adam": "Adam8bit", "adamw": "AdamW8bit", "lion": "Lion8bit", "sgd": "SGD8bit", "sgd_nesterov": "SGD8bit"}
SIZES = (1, 3, 255, 256, 257, 1023, 1025, 65541)

BF16_RANGE = (-70, 30)       # gradient binades per dtype
F32_RANGE = (-75, 40)
F32_NARROW = (-20, 0)
F16_RANGE = (-24, 12)


def _hp(rule, **over):
    """Non-default hyperparameters that keep every term of the rule alive (weight decay on, dampening on for plain SGD)."""
    if rule in ("adam", "adamw"):
        kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    elif rule == "lion":
        kw = dict(lr=1e-2, betas=(0.9, 0.99), weight_decay=0.1)
    elif rule == "sgd":
        kw = dict(lr=1e-2, momentum=0.9, dampening=0.1, weight_decay=0.01)
    else:
        kw = dict(lr=1e-2, momentum=0.9, nesterov=True, weight_decay=0.01)
    kw.update(over)
    return kw


def _c(rule, pdt, gdt, shapes, steps, seed, **kw):
    hp = _hp(rule, **kw.pop("hp", {}))
    bs = hp.get("block_size", 256)
    force = kw.pop("force", False)
    c = dict(rule=rule, pdt=pdt, gdt=gdt, shapes=[tuple(s) for s in shapes], steps=steps, seed=seed, kwargs=hp,
             kernel="generic" if (bs != 256 or force) else "wave", force=force)
    c.update(kw)
    return c


# ---------------------------------------------------------------- the cases the reference was run on (g13_optim_edges.npz)
EDGES = [
    # all five rules on the (bf16, f32) pair, gradients over 100 binades with a zero block and a constant-tiny block
    _c("adam", "bf16", "f32", [(1300,)], 6, 13000, data="binades", grange=BF16_RANGE),
    _c("adamw", "bf16", "f32", [(1300,)], 6, 13100, data="binades", grange=BF16_RANGE, hp=dict(block_size=300)),
    _c("lion", "bf16", "f32", [(4099,)], 6, 13200, data="binades", grange=BF16_RANGE, hp=dict(block_size=2048)),
    _c("sgd", "bf16", "f32", [(1300,)], 6, 13300, data="binades", grange=BF16_RANGE),
    _c("sgd_nesterov", "bf16", "f32", [(67,)], 6, 13400, hp=dict(block_size=1)),
    _c("adamw", "bf16", "bf16", [(4099,)], 6, 13500, data="binades", grange=BF16_RANGE),
    _c("adamw", "f32", "f32", [(4099,)], 4, 13600, data="binades", grange=F32_RANGE, pmin=1.0, hp=dict(block_size=2048)),
    _c("adam", "f32", "f32", [(1300,)], 6, 13700, data="binades", grange=F32_NARROW, pmin=1.0, hp=dict(block_size=300)),
    _c("adam", "f16", "f16", [(1300,)], 6, 13800, data="binades", grange=F16_RANGE),            # L2 decay into an f16 gradient
    # f16 parameters near the top of the range, lr = 1, one block larger than the tensor
    _c("adamw", "f16", "f16", [(1000,)], 4, 13900, data="top", hp=dict(lr=1.0, block_size=5000)),
    # second moments that are f32 subnormals: |g| near 2^-69, v = 0.1 g^2 near 2^-141; eps = 0 so the parameter depends on them
    _c("adamw", "f32", "f32", [(600,)], 4, 14000, data="binades", grange=(-72, -66), holes=False, pmin=1.0,
       hp=dict(betas=(0.9, 0.9), eps=0.0)),
    # Adam at steps 1000 and 10^6
    _c("adam", "bf16", "bf16", [(700,)], 3, 14100, set_step={2: 999, 3: 10 ** 6 - 1}),
    # two parameter groups (lr, block_size and weight_decay differ), grad = None on some steps
    _c("adamw", "f16", "f16", [(300,), (257,), (5, 40)], 6, 14200, group_of=[0, 0, 1],
       group_kwargs=[dict(), dict(lr=1e-3, block_size=64, weight_decay=0.0)], none_steps=[[], [2, 3], [1]]),
    # requantisation arguments exactly on k + 1/2 (tests/test_optim_emul_host.py counts them)
    _c("lion", "f32", "f32", [(600,)], 2, 14300, data="ties_s", hp=dict(betas=(0.5, 0.5))),
    _c("adam", "bf16", "f32", [(600,)], 2, 14400, data="ties_u", hp=dict(betas=(0.5, 0.75), weight_decay=0.0),
       ref_xfail="torch's vectorised CPU sqrt is 1 ulp low on some inputs: sqrt(v / max) * 255 falls just under k + 1/2 where the "
                 "correctly rounded sqrt lands on it, and the reference's code is k where round-half-even gives k + 1"),
    _c("sgd", "bf16", "bf16", [(300,)], 2, 14500, data="ties_s", hp=dict(dampening=0.0, weight_decay=0.0)),
]
for _i, _e in enumerate(EDGES):
    _e["edge"] = _i


# ---------------------------------------------------------------- every instantiation: rule x dtype pair x kernel
def _grid():
    """One case per instantiation.  Each steps three tensors whose sizes walk through SIZES; the generic cases walk through block
    sizes 64, 300, 2048, 1 and a forced 256, so that every rule meets a block larger than the 256 threads of a workgroup (the
    second trip of the kernel's loops).  Every other case spreads its gradients over the dtype's binades."""
    out, n = [], 0
    generic_bs = (300, 64, 2048, 256, 1)
    for ri, rule in enumerate(RULES):
        for pi, (pdt, gdt) in enumerate(PAIRS):
            for kernel in KERNELS:
                sizes = [SIZES[(n + k * 3) % len(SIZES)] for k in range(3)]
                hp, extra = {}, {}
                if kernel == "generic":
                    bs = generic_bs[(ri + pi) % len(generic_bs)]
                    hp["block_size"] = bs
                    extra["force"] = bs == 256
                    if bs == 1:
                        sizes = [min(s, 1025) for s in sizes]
                if n % 2:
                    extra.update(data="binades", grange={"f16": F16_RANGE, "bf16": BF16_RANGE, "f32": F32_RANGE}[gdt])
                out.append(_c(rule, pdt, gdt, [(s,) for s in sizes], 3, 20000 + 1000 * n, hp=hp, **extra))
                n += 1
    return out


GRID = _grid()

EXTRA = [
    # more blocks of more than 256 elements, with partial last blocks
    _c("adam", "f16", "f32", [(1025,), (3,)], 3, 80000, hp=dict(block_size=1000)),
    _c("sgd", "f32", "f32", [(65541,)], 3, 81000, hp=dict(block_size=4096)),
    _c("sgd_nesterov", "bf16", "bf16", [(1023,), (257,)], 3, 82000, data="binades", grange=BF16_RANGE, hp=dict(block_size=513)),
    _c("lion", "f16", "f16", [(1025,)], 3, 83000, hp=dict(block_size=2048)),
    _c("adamw", "bf16", "bf16", [(65541,)], 3, 84000, data="binades", grange=BF16_RANGE, hp=dict(block_size=2048)),
    # ties on the wave kernel's other dtypes and on the generic kernel
    _c("adamw", "f16", "f16", [(1023,)], 2, 85000, data="ties_u", hp=dict(betas=(0.5, 0.75), weight_decay=0.0)),
    _c("adam", "f32", "f32", [(1023,)], 2, 86000, data="ties_u", hp=dict(betas=(0.5, 0.75), weight_decay=0.0, block_size=600)),
    _c("lion", "bf16", "bf16", [(600,)], 2, 87000, data="ties_s", hp=dict(betas=(0.5, 0.5)), force=True),
]

# the flagship shape: one 4096 x 11008 bf16 parameter under AdamW, 3 steps
LARGE = _c("adamw", "bf16", "bf16", [(4096, 11008)], 3, 90000)

CASES = EDGES + GRID + EXTRA + [LARGE]


def group_kwargs(c, gi):
    kw = dict(c["kwargs"])
    if c.get("group_kwargs"):
        kw.update(c["group_kwargs"][gi])
    return kw


def block_size_of(c, j):
    gi = c["group_of"][j] if c.get("group_of") else 0
    return group_kwargs(c, gi).get("block_size", 256)


def kernel_of(c, j):
    return "generic" if (block_size_of(c, j) != 256 or c.get("force")) else "wave"


def case_id(c):
    shapes = "+".join("x".join(str(d) for d in s) for s in c["shapes"])
    bs = "/".join(str(b) for b in sorted({block_size_of(c, j) for j in range(len(c["shapes"]))}))
    tag = f"{c['rule']}-{c['pdt']}-{c['gdt']}-{c['kernel']}{'-forced' if c.get('force') else ''}-bs{bs}-{shapes}-{c.get('data', 'normal')}"
    return tag + (f"-edge{c['edge']}" if "edge" in c else "")
